// Host check of sdr-j-fm_amd/csrc/fmx_plan.h (run by tests/test_call_plan_cpu.py): one query per line on stdin, one JSON object per query on stdout.
//   call n decim any_rds prepass pllc am call_pieces channels ola_mode conv2 prepass_arrays half  -> {"kind": "whole" | "rds" | "overlapped", "lens": [...]}
//   front g0 n want twins channels n_cus                                                        -> {"parts": p, "part_tiles": t}
//   stageb channels n_cus rows_on form                                                          -> {"two": 0 | 1}
//   second channels n_cus                                                                       -> {"second": c}
//   const                                                                                       -> the constants the test needs
#include "../sdr-j-fm_amd/csrc/fmx_plan.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
using namespace fmx;
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string q;
        in >> q;
        if (q == "call") {
            CallShape c{};
            int any_rds, prepass, pllc, am, ola, conv2, arrays;
            in >> c.n >> c.decim >> any_rds >> prepass >> pllc >> am >> c.call_pieces >> c.channels >> ola >> conv2 >> arrays >> c.half;
            c.any_rds = any_rds; c.prepass = prepass; c.pllc = pllc; c.am = am; c.ola_mode = ola; c.conv2 = conv2; c.prepass_arrays = arrays;
            const CallPlan p = plan_call(c);
            printf("{\"kind\": \"%s\", \"lens\": [", p.kind == CallKind::WHOLE ? "whole" : (p.kind == CallKind::RDS_PIECES ? "rds" : "overlapped"));
            for (size_t i = 0; i < p.lens.size(); i++) printf("%s%lld", i ? ", " : "", (long long)p.lens[i]);
            printf("]}\n");
        } else if (q == "front") {
            long long g0, n; int want, twins, channels, n_cus;
            in >> g0 >> n >> want >> twins >> channels >> n_cus;
            const FrontParts f = plan_front_parts(g0, n, want, twins, channels, n_cus);
            printf("{\"parts\": %d, \"part_tiles\": %d}\n", f.parts, f.part_tiles);
        } else if (q == "stageb") {
            int channels, n_cus, rows_on, form;
            in >> channels >> n_cus >> rows_on >> form;
            printf("{\"two\": %d}\n", stageb_two_kernels(channels, n_cus, rows_on != 0, form, STAGEB_WG_PER_CU) ? 1 : 0);
        } else if (q == "second") {
            int channels, n_cus;
            in >> channels >> n_cus;
            printf("{\"second\": %d}\n", second_group_channels(channels, n_cus));
        } else if (q == "const") {
            printf("{\"RDS_BLK\": %d, \"DECIM\": %d, \"FRONT_TILE\": %d}\n", RDS_BLK, DECIM, FRONT_TILE);
        } else {
            printf("{\"error\": \"unknown query\"}\n");
        }
    }
    return 0;
}

// Host check of sdr-j-fm_amd/csrc/fmx_needs.h (run by tests/test_needs_cpu.py): one query per line on stdin, one JSON object per query on stdout.
//   front ok any_lo fk parts channels n_cus                                  -> {"front4": f, "parts": p}
//   needs channels twins ola scope_taps {decoder squelch rds lo att_l att_r nd dc_k}*channels -> the CallNeeds fields
//   plain piped ola arrays conv2 rows rds gain form has_fm has_frames        -> {"plain": 0 | 1}
//   param id value inputRate                                                 -> {"code": c, "msg": "..."}
//   iq fmt denominator                                                       -> {"code": c, "msg": "..."}
//   lo_period lo inputRate | pll_seq value channels | filter value channels | defer ola pinned g_total twins max_block
//   squelch level                                                            -> the two thresholds as float bit patterns
//   hlo cols off lo inputRate {index value}*                                 -> the sum's parts as float bit patterns
//   ring produced read ring capacity                                         -> {"from": f, "count": c, "next": n, "slot": s}
//   scan fill blocks nj J0 block ring                                        -> the job, the records and the counters behind the call
//   const                                                                    -> the constants the test needs
#include "../sdr-j-fm_amd/csrc/fmx_needs.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
using namespace fmx;
static unsigned bits_of(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static double num(std::istringstream &in) { std::string t; in >> t; return std::strtod(t.c_str(), nullptr); }      // ("nan", "inf" too)
static void answer(const ParamCheck &pc) { printf("{\"code\": %d, \"msg\": \"%s\"}\n", pc.code, pc.msg ? pc.msg : ""); }
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string q;
        in >> q;
        if (q == "front") {
            int ok, lo, fk, parts, channels, n_cus;
            in >> ok >> lo >> fk >> parts >> channels >> n_cus;
            const FrontChoice f = choose_front(ok != 0, lo != 0, fk, parts, channels, n_cus);
            printf("{\"front4\": %d, \"parts\": %d}\n", f.front4, f.parts);
        } else if (q == "needs") {
            int channels, twins, ola, taps;
            in >> channels >> twins >> ola >> taps;
            CallNeeds n = needs_begin(channels, twins, ola != 0, taps);
            for (int c = 0; c < channels; c++) {
                ChanNeeds k{};
                in >> k.decoder >> k.squelch_mode >> k.rds_mode >> k.lo_freq;
                k.att_l = (float)num(in); k.att_r = (float)num(in);
                in >> k.nd >> k.dc_k;
                needs_add(n, k);
            }
            printf("{\"any_lo\": %d, \"front4_ok\": %d, \"any_rds\": %d, \"prepass\": %d, \"pllc\": %d, \"am\": %d, \"prepass_var\": %d, \"any_nsq\": %d, "
                   "\"keep_taps\": %d, \"rows_on\": %d, \"peaks_on\": %d}\n", n.any_lo, n.front4_ok, n.any_rds, n.prepass, n.pllc, n.am, n.prepass_var, n.any_nsq,
                   n.keep_taps, n.rows_on, n.peaks_on);
        } else if (q == "plain") {
            int v[10];
            for (int &x : v) in >> x;
            printf("{\"plain\": %d}\n", plain_batch(PieceFlags{v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, v[7], v[8] != 0, v[9] != 0}) ? 1 : 0);
        } else if (q == "param") {
            int id, rate;
            in >> id;
            const double v = num(in);
            in >> rate;
            answer(check_param(id, v, rate));
        } else if (q == "iq") {
            int fmt;
            in >> fmt;
            answer(check_iq_format(fmt, (float)num(in)));
        } else if (q == "lo_period") {
            int lo, rate;
            in >> lo >> rate;
            printf("{\"period\": %d}\n", lo_period(lo, rate));
        } else if (q == "pll_seq") {
            int v, channels;
            in >> v >> channels;
            printf("{\"pll_seq\": %d}\n", pll_seq(v, channels));
        } else if (q == "filter") {
            int v, channels;
            in >> v >> channels;
            const FilterForm f = filter_form(v, channels);
            printf("{\"ola_mode\": %d, \"folded_pinned\": %d}\n", f.ola_mode, f.folded_pinned);
        } else if (q == "defer") {
            int ola, pinned, twins; long long g, mb;
            in >> ola >> pinned >> g >> twins >> mb;
            printf("{\"defer\": %d}\n", defer_filter_change(ola != 0, pinned != 0, g, twins, mb) ? 1 : 0);
        } else if (q == "squelch") {
            int level;
            in >> level;
            const SquelchThr t = squelch_thresholds(level);
            printf("{\"level\": %u, \"noise\": %u}\n", bits_of(t.level), bits_of(t.noise));
        } else if (q == "hlo") {
            int cols, off, lo, rate, idx;
            in >> cols >> off >> lo >> rate;
            std::vector<float> tz((size_t)(cols + 2) * DECIM, 0.f);
            while (in >> idx) tz[(size_t)idx] = (float)num(in);
            const TapSum h = tap_sum_lo(tz.data(), cols, off, lo, rate);
            printf("{\"re\": %u, \"im\": %u}\n", bits_of(h.re), bits_of(h.im));
        } else if (q == "ring") {
            long long produced, read, ring, cap;
            in >> produced >> read >> ring >> cap;
            const RingTake t = ring_take(produced, read, ring, cap);
            printf("{\"from\": %lld, \"count\": %lld, \"next\": %lld, \"slot\": %lld}\n", (long long)t.from, (long long)t.count, (long long)t.next(), (long long)ring_slot(t.from, ring));
        } else if (q == "scan") {
            long long fill, blocks, nj, J0; int block, ring;
            in >> fill >> blocks >> nj >> J0 >> block >> ring;
            const ScanProduce p = scan_produce(fill, blocks, nj, J0, block, ring);
            printf("{\"job_fill\": %d, \"job_slot0\": %d, \"nblk\": %lld, \"new_fill\": %d, \"new_blocks\": %lld, \"records\": [", p.job_fill, p.job_slot0, (long long)p.nblk,
                   p.new_fill, (long long)p.new_blocks);
            for (long long b = p.b0; b < p.nblk; b++) printf("%s[%lld, %lld]", b > p.b0 ? ", " : "", (long long)p.slot(b), (long long)p.end_sample(b));
            printf("]}\n");
        } else if (q == "const") {
            printf("{\"LO_LDS_MAX\": %d, \"OLA_MAX_CH\": %d, \"PLL_SEQ_AUTO_MAX\": %d, \"FMX_E_INVALID\": %d}\n", LO_LDS_MAX, OLA_MAX_CH, PLL_SEQ_AUTO_MAX, (int)FMX_E_INVALID);
        } else {
            printf("{\"error\": \"unknown query\"}\n");
        }
    }
    return 0;
}

// rdsm_check -- the RDS meter's integers (sdr-j-fm_amd/csrc/fmx_rdsm.h) on the CPU.  One query per line on stdin, one JSON line per query:
//   const                 -> the header's constants, and lane / step / mean of a few samples
//   reset                 -> one channel from fmx_create on: no sample, no record, the meter off
//   piece meter dec n     -> the next piece of that channel: its meter on (1) or off (0), its decoder on or off, n RDS samples if the decoder is on.
//                            rdsm::piece against a walk sample by sample: a window is valid from its first sample if the meter is on there, and stops being
//                            valid with any of its samples that a piece with the meter off produces; a valid window's last sample leaves a record in the
//                            next slot.  {"m0", "m1", "job", "first", "w0", "nwin", "slot0", "produced"} and the walk's "b_first", "b_w" (the completed
//                            windows), "b_slots", "b_produced"
#include "../sdr-j-fm_amd/csrc/fmx_rdsm.h"

#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

using namespace fmx;

int main() {
    char line[256];
    int64_t m = 0, on_from = -1, produced = 0;          // the pure function's channel
    int64_t b_produced = 0; bool b_valid = false;       // the walk's channel
    while (fgets(line, sizeof(line), stdin)) {
        char cmd[32] = {0};
        if (sscanf(line, "%31s", cmd) != 1) continue;
        const std::string c(cmd);
        if (c == "const") {
            printf("{\"window\": %d, \"lanes\": %d, \"steps\": %d, \"ring\": %d, \"ring24\": %d, \"quant\": %d, \"order\": [%d, %d, %d, %d, %d, %d], "
                   "\"lane_2559\": %d, \"step_2559\": %d, \"lane_64\": %d, \"step_64\": %d, \"window_of_2560\": %" PRId64 ", \"window_of_2559\": %" PRId64
                   ", \"mean_2560\": %.9g, \"holds_8192\": %d, \"holds_8193\": %d}\n",
                   rdsm::WINDOW, rdsm::LANES, rdsm::STEPS, rdsm::RING, rdsm::RING24, rdsm::QUANT, (int)rdsm::Q_MX, (int)rdsm::Q_II, (int)rdsm::Q_QQ,
                   (int)rdsm::Q_IQ, (int)rdsm::Q_I, (int)rdsm::Q_Q, rdsm::lane_of(2559), rdsm::step_of(2559), rdsm::lane_of(64), rdsm::step_of(64),
                   rdsm::window_of(2560), rdsm::window_of(2559), (double)rdsm::finish_mean(2560.0f), rdsm::ring_holds(5, 8197) ? 1 : 0,
                   rdsm::ring_holds(5, 8198) ? 1 : 0);
        } else if (c == "reset") {
            m = 0; on_from = -1; produced = 0; b_produced = 0; b_valid = false;
            printf("{\"ok\": 1}\n");
        } else if (c == "piece") {
            int meter = 0, dec = 0; long long n = 0;
            if (sscanf(line, "%*s %d %d %lld", &meter, &dec, &n) != 3 || n < 0) { printf("{\"error\": \"piece\"}\n"); continue; }
            const int64_t m0 = m, m1 = dec ? m + n : m;
            const rdsm::Piece p = rdsm::piece(meter != 0, dec != 0, on_from, m0, m1, produced);
            // the walk
            int64_t b_first = -1; std::vector<int64_t> bw, bs;
            for (int64_t x = m0; x < m1; x++) {
                if (x % rdsm::WINDOW == 0) b_valid = meter != 0;
                else if (!meter) b_valid = false;
                if (b_valid && b_first < 0) b_first = x;
                if (b_valid && x % rdsm::WINDOW == rdsm::WINDOW - 1) { bw.push_back(x / rdsm::WINDOW); bs.push_back(b_produced % rdsm::RING); b_produced++; }
            }
            printf("{\"m0\": %" PRId64 ", \"m1\": %" PRId64 ", \"job\": %d, \"first\": %" PRId64 ", \"w0\": %" PRId64 ", \"nwin\": %" PRId64
                   ", \"slot0\": %" PRId64 ", \"produced\": %" PRId64 ", \"end0\": %" PRId64 ", \"b_first\": %" PRId64 ", \"b_produced\": %" PRId64 ", \"b_w\": [",
                   m0, m1, p.job ? 1 : 0, p.job ? p.first : (int64_t)-1, p.w0, p.nwin, p.slot(0), p.new_produced, p.end_sample(0), b_first, b_produced);
            for (size_t i = 0; i < bw.size(); i++) printf("%s%" PRId64, i ? ", " : "", bw[i]);
            printf("], \"b_slots\": [");
            for (size_t i = 0; i < bs.size(); i++) printf("%s%" PRId64, i ? ", " : "", bs[i]);
            printf("]}\n");
            on_from = p.on_from; produced = p.new_produced; m = m1;
        } else printf("{\"error\": \"unknown query\"}\n");
    }
    return 0;
}

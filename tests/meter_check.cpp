// meter_check -- the modulation meter's integers (sdr-j-fm_amd/csrc/fmx_meter.h) on the CPU.  One query per line on stdin, one JSON line per query:
//   walk seed base pieces  -> a stream from fm sample `base` on, cut into `pieces` random pieces with the meter switched at random between them:
//                             meter_produce of every piece against a counter stepped sample by sample; {"ok": 1, "records": n, "pieces": n} or the mismatch
//   map i                  -> lane and step of sample i of a window
//   finish bits            -> the two finishing divisions of the f32 with these bits, as bits
//   const                  -> the header's constants
#include "../sdr-j-fm_amd/csrc/fmx_meter.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace fmx::meter;

static uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static int walk(uint64_t seed, int64_t base, int pieces) {
    std::mt19937_64 rng(seed);
    // the counter: what the contract says, one sample at a time
    bool active = false;               // the window in progress has been metered from its first sample
    int64_t produced = 0, slots[RING];
    for (auto &s : slots) s = -1;
    // the header's side
    int64_t on_from = -1, h_produced = 0, h_slots[RING];
    for (auto &s : h_slots) s = -1;
    int64_t J0 = base, records = 0;
    bool on = false;
    for (int p = 0; p < pieces; p++) {
        if (rng() % 3 == 0) on = !on;
        static const int64_t lens[] = {1, 2, 63, 64, 65, 799, 1365, 4799, 9599, 9600, 9601, 19237, 32000, 87381, 700000};
        const int64_t nj = (rng() % 4 == 0) ? 1 + (int64_t)(rng() % 30000) : lens[rng() % (sizeof(lens) / sizeof(lens[0]))];
        // ---- sample by sample
        int64_t first = -1;
        std::vector<int64_t> done;
        if (!on) active = false;
        for (int64_t j = J0; j < J0 + nj; j++) {
            if (!on) break;
            if (j % WINDOW == 0) active = true;
            if (active && first < 0) first = j;
            if (active && j % WINDOW == WINDOW - 1) { done.push_back(j / WINDOW); slots[produced & (RING - 1)] = j / WINDOW; produced++; active = false; }
        }
        // ---- the header
        if (!on) on_from = -1;
        else {
            if (on_from < 0) on_from = J0;
            const Produce mp = meter_produce(on_from, J0, nj, h_produced);
            const bool job = mp.first < J0 + nj;
            if (job != (first >= 0) || (job && mp.first != first) || mp.first < J0 || mp.nwin != (int64_t)done.size() || (mp.nwin > 0 && mp.w0 != done[0]) ||
                mp.new_produced != h_produced + mp.nwin) {
                printf("{\"ok\": 0, \"piece\": %d, \"J0\": %" PRId64 ", \"nj\": %" PRId64 ", \"on_from\": %" PRId64 ", \"first\": [%" PRId64 ", %" PRId64 "], \"nwin\": [%" PRId64
                       ", %zu], \"w0\": %" PRId64 "}\n", p, J0, nj, on_from, mp.first, first, mp.nwin, done.size(), mp.w0);
                return 1;
            }
            for (int64_t k = 0; k < mp.nwin; k++) {
                if (mp.slot(k) < 0 || mp.slot(k) >= RING || mp.end_sample(k) != (mp.w0 + k + 1) * WINDOW) { printf("{\"ok\": 0, \"slot\": %" PRId64 "}\n", mp.slot(k)); return 1; }
                h_slots[mp.slot(k)] = mp.w0 + k;
            }
            h_produced = mp.new_produced; records += mp.nwin;
        }
        if (h_produced != produced || std::memcmp(slots, h_slots, sizeof(slots)) != 0) { printf("{\"ok\": 0, \"piece\": %d, \"ring\": 1}\n", p); return 1; }
        J0 += nj;
    }
    printf("{\"ok\": 1, \"records\": %" PRId64 ", \"pieces\": %d, \"end\": %" PRId64 "}\n", records, pieces, J0);
    return 0;
}

int main() {
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        char cmd[32] = {0};
        if (sscanf(line, "%31s", cmd) != 1) continue;
        const std::string c(cmd);
        if (c == "walk") {
            unsigned long long seed = 0; long long base = 0; int pieces = 0;
            if (sscanf(line, "%*s %llu %lld %d", &seed, &base, &pieces) != 3) { printf("{\"error\": \"walk\"}\n"); continue; }
            walk(seed, base, pieces);
        } else if (c == "map") {
            int i = 0;
            sscanf(line, "%*s %d", &i);
            printf("{\"lane\": %d, \"step\": %d}\n", lane_of(i), step_of(i));
        } else if (c == "finish") {
            unsigned u = 0;
            sscanf(line, "%*s %u", &u);
            float f; std::memcpy(&f, &u, 4);
            printf("{\"mean\": %u, \"pilot\": %u}\n", f2u(finish_mean(f)), f2u(finish_pilot(f)));
        } else if (c == "const") {
            printf("{\"window\": %d, \"lanes\": %d, \"steps\": %d, \"ring\": %d, \"quant\": %d}\n", WINDOW, LANES, STEPS, RING, QUANT);
        } else printf("{\"error\": \"unknown query\"}\n");
    }
    return 0;
}

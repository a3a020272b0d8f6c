// loud_check -- the programme audio meter's integers and constants (sdr-j-fm_amd/csrc/fmx_loud.h) on the CPU.  One query per line on stdin, one JSON line
// per query:
//   walk seed base pieces  -> a stream from PCM frame `base` on, cut into `pieces` random pieces (of 0, 1, 4799, 4800, 4801 frames, of three windows, of
//                             random lengths) with the meter switched at random between them: audio_produce of every piece against a counter stepped
//                             frame by frame; {"ok": 1, "records": n, ...} or the mismatch
//   finish bits            -> the finishing division of the f32 with these bits, as bits
//   const                  -> the header's constants and the ten coefficients as bits
#include "../sdr-j-fm_amd/csrc/fmx_loud.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace fmx::loud;

static uint32_t f2u(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static int walk(uint64_t seed, int64_t base, int pieces) {
    std::mt19937_64 rng(seed);
    // the counter: what the contract says, one frame at a time
    bool running = false;              // the meter was on in the last piece that had frames
    bool active = false;               // the window in progress has been metered from its first frame
    int64_t produced = 0, slots[RING];
    for (auto &s : slots) s = -1;
    // the header's side
    int64_t on_from = -1, h_produced = 0, h_slots[RING];
    for (auto &s : h_slots) s = -1;
    int64_t M0 = base, records = 0, resets = 0, empty = 0;
    bool on = false;
    for (int p = 0; p < pieces; p++) {
        if (rng() % 3 == 0) on = !on;
        static const int64_t lens[] = {0, 1, 2, 63, 64, 65, 799, 1365, 4799, 4800, 4801, 9600, 14400, 14437, 19237};
        const int64_t frames = (rng() % 4 == 0) ? (int64_t)(rng() % 12000) : lens[rng() % (sizeof(lens) / sizeof(lens[0]))];
        if (frames == 0) { empty++; continue; }      // (a piece without frames covers none: the call path does not ask)
        // ---- frame by frame
        int64_t first = -1;
        std::vector<int64_t> done;
        bool reset = false;
        if (!on) running = active = false;
        else {
            reset = !running; running = true;
            for (int64_t m = M0; m < M0 + frames; m++) {
                if (m % WINDOW == 0) active = true;
                if (active && first < 0) first = m;
                if (active && m % WINDOW == WINDOW - 1) { done.push_back(m / WINDOW); slots[produced & (RING - 1)] = m / WINDOW; produced++; active = false; }
            }
        }
        // ---- the header
        if (!on) on_from = -1;
        else {
            if (on_from < 0) on_from = M0;
            const Produce ap = audio_produce(on_from, M0, frames, h_produced);
            const bool accumulates = ap.first < M0 + frames;
            if (ap.reset != reset || accumulates != (first >= 0) || (accumulates && ap.first != first) || ap.first < M0 || ap.nwin != (int64_t)done.size() ||
                (ap.nwin > 0 && ap.w0 != done[0]) || ap.any() != !done.empty() || ap.new_produced != h_produced + ap.nwin) {
                printf("{\"ok\": 0, \"piece\": %d, \"M0\": %" PRId64 ", \"frames\": %" PRId64 ", \"on_from\": %" PRId64 ", \"first\": [%" PRId64 ", %" PRId64
                       "], \"nwin\": [%" PRId64 ", %zu], \"w0\": %" PRId64 ", \"reset\": [%d, %d]}\n", p, M0, frames, on_from, ap.first, first, ap.nwin, done.size(),
                       ap.w0, (int)ap.reset, (int)reset);
                return 1;
            }
            for (int64_t k = 0; k < ap.nwin; k++) {
                if (ap.slot(k) < 0 || ap.slot(k) >= RING || ap.end_frame(k) != (done[(size_t)k] + 1) * WINDOW) { printf("{\"ok\": 0, \"slot\": %" PRId64 "}\n", ap.slot(k)); return 1; }
                h_slots[ap.slot(k)] = ap.w0 + k;
            }
            h_produced = ap.new_produced; records += ap.nwin; resets += ap.reset ? 1 : 0;
        }
        if (h_produced != produced || std::memcmp(slots, h_slots, sizeof(slots)) != 0) { printf("{\"ok\": 0, \"piece\": %d, \"ring\": 1}\n", p); return 1; }
        M0 += frames;
    }
    printf("{\"ok\": 1, \"records\": %" PRId64 ", \"resets\": %" PRId64 ", \"empty\": %" PRId64 ", \"pieces\": %d, \"end\": %" PRId64 "}\n", records, resets, empty, pieces, M0);
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
        } else if (c == "finish") {
            unsigned u = 0;
            sscanf(line, "%*s %u", &u);
            float f; std::memcpy(&f, &u, 4);
            printf("{\"mean\": %u}\n", f2u(finish_mean(f)));
        } else if (c == "const") {
            printf("{\"window\": %d, \"ring\": %d, \"tile\": %d, \"state\": %d, \"coef\": [", WINDOW, RING, TILE, STATE);
            for (int s = 0; s < 2; s++)
                for (int k = 0; k < 5; k++) printf("%u%s", f2u(K_COEF[s][k]), s == 1 && k == 4 ? "" : ", ");
            printf("], \"window_of\": [%" PRId64 ", %" PRId64 ", %" PRId64 "]}\n", window_of(4799), window_of(4800), window_of((int64_t(1) << 40) + 4800 * 7 - 1));
        } else printf("{\"error\": \"unknown query\"}\n");
    }
    return 0;
}

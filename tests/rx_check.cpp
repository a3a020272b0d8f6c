// rx_check -- the reception meter's own integers (sdr-j-fm_amd/csrc/fmx_rx.h) on the CPU: the look-back of one sample into stage A's ring.  One query per
// line on stdin, one JSON line per query:
//   holds ring delay nj twins J0 -> ring_holds against the ring stepped position by position: stage A writes the positions J0 .. newest_bound - 1, each at
//                                   its place modulo `ring`; the reader then wants position J0 - 1 - delay as it was.  {"holds": 0|1, "stepped": 0|1}
//   const                        -> the header's constants
#include "../sdr-j-fm_amd/csrc/fmx_rx.h"

#include <cinttypes>
#include <cstdio>
#include <string>
#include <vector>

using namespace fmx;

int main() {
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        char cmd[32] = {0};
        if (sscanf(line, "%31s", cmd) != 1) continue;
        const std::string c(cmd);
        if (c == "holds") {
            long long ring = 0, delay = 0, nj = 0, twins = 0, J0 = 0;
            if (sscanf(line, "%*s %lld %lld %lld %lld %lld", &ring, &delay, &nj, &twins, &J0) != 5 || ring < 1 || (ring & (ring - 1))) { printf("{\"error\": \"holds\"}\n"); continue; }
            // the ring as a list of who wrote each place last: -1 the sample the reader wants, else a later writer
            std::vector<int64_t> owner((size_t)ring, -2);
            const int64_t want = rx::oldest_position(J0, delay);
            owner[(size_t)(want & (ring - 1))] = -1;
            for (int64_t p = want + 1; p < rx::newest_bound(J0, nj, twins); p++) owner[(size_t)(p & (ring - 1))] = p;
            const bool stepped = owner[(size_t)(want & (ring - 1))] == -1;
            printf("{\"holds\": %d, \"stepped\": %d}\n", rx::ring_holds(ring, delay, nj, twins) ? 1 : 0, stepped ? 1 : 0);
        } else if (c == "const") {
            printf("{\"ring\": %d, \"quant\": %d, \"window\": %d, \"lanes\": %d, \"order\": [%d, %d, %d, %d, %d, %d]}\n", rx::RING, rx::QUANT, meter::WINDOW, meter::LANES,
                   (int)rx::Q_MX, (int)rx::Q_MN, (int)rx::Q_S1, (int)rx::Q_S2, (int)rx::Q_CR, (int)rx::Q_CI);
        } else printf("{\"error\": \"unknown query\"}\n");
    }
    return 0;
}

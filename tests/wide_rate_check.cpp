// wide_rate_check.cpp -- the integer bookkeeping of stage W's rational-ratio form (sdr-j-fm_amd/csrc/fmx_wide_rate.h) compiled for the host, with
// no device and no HIP: tests/test_wideband_rate_cpu.py sets its answers against a brute-force count.
//
//   wide_rate_check ratio Rw [...]                 per rate: "ok L M NH NP min_call max_samples" or "refused <the rule>"
//   wide_rate_check count L M g0 n [...]           per (g0, n): before (g0), count (g0, n), and n_j, p_j of the call's first output
//   wide_rate_check crossing L M NP j0 n_out change [...]    per triple: wrate::crossing
//   wide_rate_check all                            every ratio M / L in lowest terms with 1 < L <= 576, L < M < 16 L: the largest NP, the largest
//                                                  number of call boundaries inside a window, the largest LDS image, and whether each fits
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../sdr-j-fm_amd/csrc/fmx_wide_rate.h"

using namespace fmx;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "ratio")) {
        for (int a = 2; a < argc; a++) {
            wrate::Ratio r; const char *why = "";
            if (wrate::ratio_of(std::atoll(argv[a]), &r, &why)) { std::printf("refused %s\n", why); continue; }
            std::printf("ok %lld %lld %d %d %d %d\n", (long long)r.L, (long long)r.M, r.NH, r.NP, r.min_call, (int)wrate::max_samples(r));
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "count") && argc >= 4) {
        const int64_t L = std::atoll(argv[2]), M = std::atoll(argv[3]);
        for (int a = 4; a + 1 < argc; a += 2) {
            const int64_t g0 = std::atoll(argv[a]), n = std::atoll(argv[a + 1]), j0 = wrate::before(g0, L, M);
            int64_t nj; int32_t pj;
            wrate::sample_of(j0, L, M, &nj, &pj);
            std::printf("%lld %lld %lld %d\n", (long long)j0, (long long)wrate::count(g0, n, L, M), (long long)nj, (int)pj);
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "crossing") && argc >= 5) {
        const int64_t L = std::atoll(argv[2]), M = std::atoll(argv[3]);
        const int NP = std::atoi(argv[4]);
        for (int a = 5; a + 2 < argc; a += 3)
            std::printf("%lld\n", (long long)wrate::crossing(std::atoll(argv[a]), std::atoll(argv[a + 1]), std::atoll(argv[a + 2]), NP, L, M));
        return 0;
    }
    if (!std::strcmp(argv[1], "all")) {
        int max_np = 0, max_bound = 0, max_image = 0, max_cross = 0; long long ratios = 0, misfits = 0;
        for (int64_t L = 2; L <= wrate::MAX_L; L++)
            for (int64_t M = L + 1; M < wrate::MAX_RATIO * L; M++) {
                if (wrate::gcd64(L, M) != 1) continue;
                wrate::Ratio r{M, L, M, (int32_t)(16 * M + 1), (int32_t)((16 * M + 1 + L - 1) / L), (int32_t)((M + L - 1) / L)};   // (Rw: unused here)
                ratios++;
                if (!wrate::fits(r)) misfits++;
                if (r.NP > max_np) max_np = r.NP;
                const int b = wrate::max_boundaries(r.NP, r.min_call);
                if (b > max_bound) max_bound = b;
                if (wrate::max_samples(r) > max_image) max_image = wrate::max_samples(r);
                const int c = (int)wrate::before(r.NP - 1, L, M) + 1;          // outputs whose newest sample lies within NP - 1 samples, at most
                if (c > max_cross) max_cross = c;
            }
        std::printf("%lld %d %d %d %d %lld\n", ratios, max_np, max_bound, max_image, max_cross, misfits);
        return 0;
    }
    return 2;
}

// fmx_wide_rate.h -- the integer bookkeeping and the filter design of stage W's rational-ratio form (include/fmx.h
// fmx_wideband_create_rate; kernel in fmx_wide_rate.hip, host half in fmx_wide_api.hip).  A stream at Rw S/s feeds outputs at Ro = 2 304 000 S/s,
// g = gcd (Rw, Ro), L = Ro / g, M = Rw / g: a polyphase filter of N_H = 16 M + 1 taps at the rate M Ro, of which output j uses the taps
// p_j + L i.  Everything here is integers (or host-only design arithmetic), so a host program checks it without a device:
// tests/wide_rate_check.cpp against a brute-force count.
//
//   output j (from the stream's first sample):  q_j = (j + 1) M - 1,  n_j = q_j div L (its newest sample),  p_j = q_j mod L (its phase)
//   n_j < X  <=>  (j + 1) M <= X L, so floor (X L / M) outputs have their newest sample in front of sample X: `before`.
#pragma once
#include <cstdint>
#include <vector>

#include "fmx_design.h"

#ifdef __HIPCC__
#define FMX_WR_HD __host__ __device__ __forceinline__
#else
#define FMX_WR_HD inline
#endif

namespace fmx {
namespace wrate {

constexpr int64_t RO = 2304000;
constexpr int MAX_L = 576;                   // phases
constexpr int MAX_RATIO = 16;                // Rw <= 16 Ro
constexpr int TILE = 256;                    // outputs per workgroup
constexpr int HIST = 256;                    // history entries kept per stream: NP - 1 <= 255 are used (16 M + 1 <= 256 L)
constexpr int LDS_SAMPLES = 4352;            // float2 of a workgroup's image, 34 816 bytes: max_samples () <= 4336 for every accepted rate

struct Ratio {
    int64_t Rw, L, M;
    int32_t NH;          // 16 M + 1 taps of the prototype
    int32_t NP;          // ceil (NH / L): taps of the longest phase = samples of a window
    int32_t min_call;    // ceil (M / L): the shortest call
};

FMX_WR_HD int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// The accepted rates: Ro < Rw <= 16 Ro, Rw no multiple of Ro, L <= 576.  0: accepted; otherwise *why names the rule.
inline int ratio_of(int64_t Rw, Ratio *r, const char **why) {
    if (Rw <= RO) { *why = "wide_rate_hz must be above 2304000"; return 1; }
    if (Rw > MAX_RATIO * RO) { *why = "wide_rate_hz must be at most 16 * 2304000"; return 1; }
    if (Rw % RO == 0) { *why = "wide_rate_hz is a multiple of 2304000: use fmx_wideband_create with a factor"; return 1; }
    const int64_t g = gcd64(Rw, RO);
    if (RO / g > MAX_L) { *why = "wide_rate_hz: L = 2304000 / gcd (wide_rate_hz, 2304000) must be at most 576"; return 1; }
    r->Rw = Rw; r->L = RO / g; r->M = Rw / g;
    r->NH = (int32_t)(16 * r->M + 1);
    r->NP = (int32_t)((r->NH + r->L - 1) / r->L);
    r->min_call = (int32_t)((r->M + r->L - 1) / r->L);
    *why = "";
    return 0;
}

// outputs whose newest sample lies in front of sample X (X >= 0, X L < 2^63)
FMX_WR_HD int64_t before(int64_t X, int64_t L, int64_t M) { return X * L / M; }
// outputs of a call of n samples behind g0
FMX_WR_HD int64_t count(int64_t g0, int64_t n, int64_t L, int64_t M) { return before(g0 + n, L, M) - before(g0, L, M); }
// newest sample and phase of output j
FMX_WR_HD void sample_of(int64_t j, int64_t L, int64_t M, int64_t *n, int32_t *p) {
    const int64_t q = (j + 1) * M - 1;
    *n = q / L; *p = (int32_t)(q - *n * L);
}
// How many of a call's outputs (the n_out from output j0 = before (g0) on) have a window of NP samples that reaches in front of sample
// `change`: n_j - (NP - 1) < change.  They are the call's first ones; with change <= g0 there are fewer than 256 (NP - 1 <= 255 samples
// hold at most 255 L / M + 1 outputs), so they lie in the call's first tile.
FMX_WR_HD int64_t crossing(int64_t j0, int64_t n_out, int64_t change, int32_t NP, int64_t L, int64_t M) {
    const int64_t lim = change + NP - 1;
    if (lim <= 0) return 0;
    const int64_t c = before(lim, L, M) - j0;
    return c < 0 ? 0 : c > n_out ? n_out : c;
}
// Call boundaries a window can hold: its NP samples have NP - 1 gaps, boundaries lie at least min_call gaps apart: ceil ((NP - 1) / min_call).
// L does not divide M, so min_call >= (M + 1) / L and 16 min_call >= (16 M + 16) / L >= NH / L: NP <= 16 min_call and the count is at most
// 16 -- 17 runs of one offset, W_MAX_SEG, for every accepted rate (tests/wide_rate_check.cpp walks all of them).
FMX_WR_HD int32_t max_boundaries(int32_t NP, int32_t min_call) { return (NP - 1 + min_call - 1) / min_call; }

// The LDS image of a tile holds its samples in order, from the oldest sample of the tile's first window on: at most this many, since
// n_{j + 255} - n_j <= floor (255 M / L) + 1, and NP - 1 lie in front.
inline int32_t max_samples(const Ratio &r) { return (int32_t)((TILE - 1) * r.M / r.L) + 1 + r.NP; }
inline bool fits(const Ratio &r) { return max_samples(r) <= LDS_SAMPLES && r.NP - 1 <= HIST - 1; }

// The prototype: tmp = the reference's Blackman low-pass (fir-filters.cpp:41-62, design::sinc_blackman) of NH taps with 400 kHz at M Ro,
// H [k] = f32 (tmp [k] L / sum tmp), the sum in f64 in tap order.
inline std::vector<float> prototype(const Ratio &r) {
    std::vector<float> tmp;
    const float f = (float)400000 / (float)(r.M * RO);
    (void)design::sinc_blackman(r.NH, f, tmp);
    double s = 0.0;
    for (float v : tmp) s += (double)v;
    std::vector<float> H((size_t)r.NH);
    for (int k = 0; k < r.NH; k++) H[(size_t)k] = (float)((double)tmp[(size_t)k] * (double)r.L / s);
    return H;
}
// ... and its phases, row p = H [p + L i], i < NP, zeros behind the prototype's end
inline std::vector<float> phase_table(const Ratio &r, const std::vector<float> &H) {
    std::vector<float> t((size_t)r.L * r.NP, 0.f);
    for (int64_t p = 0; p < r.L; p++)
        for (int i = 0; i < r.NP; i++)
            if (p + r.L * i < r.NH) t[(size_t)(p * r.NP + i)] = H[(size_t)(p + r.L * i)];
    return t;
}

}  // namespace wrate
}  // namespace fmx

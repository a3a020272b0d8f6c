// fmx_mpx.h -- the multiplex spectrum meter (include/fmx.h fmx_mpx_*; the reference draws this picture on its LF scope with
// setlfPlotType (DEMODULATOR), fm-processor.cpp:597-660): a windowed 4096-point power spectrum of a channel's demodulator output d [j] at fmRate -- the
// row w_dem stage B leaves behind, FMX_TAP_DEMOD's value --, mean and max-hold per record, and the host's figures over a record.  The window, the twiddles
// and the transform are the band survey's (fmx_survey.h, included unchanged); the grid, a piece's plan, the chunking and the switch's rules are the
// spectrum meter's (fmx_spec.h: spec::piece, spec::first_block, spec::delivered, spec::record_end, spec::launches, unchanged, with g := the fm sample j).
// What is this meter's own is here, as pure functions -- fmx_api.hip decides with them, fmx_mpx.hip runs them, tests/mpx_check.cpp drives them on the CPU:
//   load (): thread t's sixteen windowed samples of a block, imaginary part zero, each from the carry or from the piece's row;
//   fold (): spec::fold's twin for a ring slot of 2 x 2048 bins -- the same adds and maxima in the same order;
//   figures (): deviation in L+R, L-R, the RDS band and the auxiliary band, the pilot's and the 38 kHz carrier's lines, the floor in the guards beside
//     the pilot and a caller's own bands, all sums in f64, membership of a bin in a band decided as spec::figures decides it.
// d is real: bins 0 .. 2047 are kept (bin k at k fmRate / 4096 Hz), the Nyquist bin is dropped.  One block per transform: two real blocks are NOT
// packed into one complex transform, which would couple their roundings and make a record depend on how blocks pair up.
#pragma once
#include "fmx_spec.h"

namespace fmx {
namespace mpx {

constexpr int N = spec::N, NT = spec::NT, PER = spec::PER;
constexpr int BINS = N / 2;                               // bins kept: 0 .. 2047
constexpr int KEEP = BINS / NT;                           // of pass 3's sixteen bins t + 256 c per thread: c < 8
constexpr int RING = 4;                                   // records kept per metered channel
constexpr int MAX_B = spec::MAX_B, MAX_S = spec::MAX_S;
constexpr int DEFAULT_B = 48;                             // 1.024 s at 192 kS/s
constexpr int MAX_BANDS = 16;
constexpr int64_t SCRATCH_BLOCKS = spec::SCRATCH_BYTES / ((int64_t)BINS * (int64_t)sizeof(float));      // 32 768 blocks of 2048 f32
// the scratch a handle allocates (spec::scratch_blocks_for with this meter's block size)
inline int64_t scratch_blocks_for(int64_t channels, int64_t blocks) {
    const int64_t want = channels * (blocks > 0 ? blocks : 1);
    return want < SCRATCH_BLOCKS ? (want > 0 ? want : 1) : SCRATCH_BLOCKS;
}

// Thread t's samples of block b of a piece that begins at fm sample g0: x [n2] = (f32 (d [t + 256 n2] w [t + 256 n2]), 0); a sample in front of the piece
// is the carry's (block b0 alone), every other one the piece's row (q < n always: the block completes in the piece)
__host__ __device__ __forceinline__ void load(int t, int64_t b, int64_t g0, int64_t n, int32_t S, const float *carry, const float *row, const float *window, float2 *x) {
#pragma unroll
    for (int n2 = 0; n2 < PER; n2++) {
        const int i = t + 256 * n2;
        const int64_t q = spec::source_index(b, i, g0, S);
        float v = 0.f;
        if (q < 0) v = carry[i];
        else if (q < n) v = row[q];
        x[n2] = make_float2(v * window[i], 0.f);
    }
}

// spec::fold for a ring slot of 2 BINS floats: one bin of one channel over nb blocks from block b on, in block order; p [j * pstride] is block b + j's power
__host__ __device__ __forceinline__ void fold(float &sum, float &mx, const float *p, int64_t pstride, int64_t b, int64_t nb, int64_t first, int phase, int B,
                                              float c, float c1, float *mean, float *peak) {
    int64_t r = b / B;
    for (int64_t j = 0; j < nb; j++) {
        if (phase == 0) { sum = 0.f; mx = 0.f; }
        if (b + j >= first) { const float v = p[j * pstride]; sum += v; mx = fmaxf(mx, v); }
        if (++phase == B) {
            if (spec::delivered(r, B, first)) { const size_t at = (size_t)(r & (RING - 1)) * 2 * BINS; mean[at] = sum * c; peak[at] = mx * c1; }
            phase = 0; r++;
        }
    }
}

// ---- the figures (include/fmx.h fmx_mpx_figures) --------------------------------------------------------------------------------------------
inline int figures(const fmx_mpx_find *cfg, const float *mean, const float *peak, fmx_mpx_figs *out, const char **why) {
    *why = "";
    if (!cfg || !mean || !out) { *why = "null argument"; return FMX_E_INVALID; }
    if (cfg->struct_size != (int32_t)sizeof(fmx_mpx_find)) { *why = "fmx_mpx_find.struct_size mismatch"; return FMX_E_INVALID; }
    if (cfg->rate_hz < 8000 || cfg->rate_hz > 1000000) { *why = "rate_hz must be in [8000, 1000000]"; return FMX_E_INVALID; }
    if (!(cfg->hz_per_unit > 0.0) || !std::isfinite(cfg->hz_per_unit)) { *why = "hz_per_unit must be positive and finite"; return FMX_E_INVALID; }
    if (cfg->dc_guard_hz < 0 || cfg->dc_guard_hz > 1000) { *why = "dc_guard_hz must be in [0, 1000]"; return FMX_E_INVALID; }
    if (cfg->line_half_hz < 50 || cfg->line_half_hz > 1000) { *why = "line_half_hz must be in [50, 1000]"; return FMX_E_INVALID; }
    if (cfg->n_bands < 0 || cfg->n_bands > MAX_BANDS || (cfg->n_bands > 0 && !cfg->bands)) { *why = "bands / n_bands: none, or up to 16 bands"; return FMX_E_INVALID; }
    const double R = (double)cfg->rate_hz;
    for (int i = 0; i < cfg->n_bands; i++) {
        const fmx_mpx_band &b = cfg->bands[i];
        if (!std::isfinite(b.lo_hz) || !std::isfinite(b.hi_hz) || !(b.lo_hz >= 0.0) || !(b.lo_hz < b.hi_hz) || !(2.0 * b.hi_hz <= R)) {
            *why = "bands: 0 <= lo_hz < hi_hz <= rate_hz / 2, both finite"; return FMX_E_INVALID;
        }
    }
    for (int k = 0; k < BINS; k++) {
        if (!(mean[k] >= 0.f) || !std::isfinite(mean[k])) { *why = "mean holds a negative or non-finite entry"; return FMX_E_INVALID; }
        if (peak && (!(peak[k] >= 0.f) || !std::isfinite(peak[k]))) { *why = "peak holds a negative or non-finite entry"; return FMX_E_INVALID; }
    }
    // bin k lies at k R / N Hz; every comparison with a frequency is made on k R against the frequency times N (both exact in double for integral Hz:
    // spec::figures' integer comparison; a bound that is not integral is compared after the multiplication)
    auto usable = [&](int k) { return k > 0 && (double)k * R >= (double)cfg->dc_guard_hz * N; };
    auto in = [&](int k, double lo, double hi) { const double f = (double)k * R; return lo * N <= f && f <= hi * N; };
    const double df = R / N, half = (double)cfg->line_half_hz, u = cfg->hz_per_unit;
    struct Sum { double s; int n; };
    // the sum of P over the usable bins of [lo, hi] that lie outside [xlo, xhi]
    auto band = [&](const float *P, double lo, double hi, double xlo, double xhi) {
        Sum a{0.0, 0};
        for (int k = 0; k < BINS; k++) if (usable(k) && in(k, lo, hi) && !(xhi > xlo && in(k, xlo, xhi))) { a.s += (double)P[k]; a.n++; }
        return a;
    };
    auto power = [&](const Sum &a) { return 2.0 / N * a.s; };                          // P (band)
    auto dev = [&](const Sum &a, double hi) { return (a.n > 0 && 2.0 * hi <= R) ? u * std::sqrt(power(a)) : -HUGE_VAL; };
    fmx_mpx_figs F;
    F.total_hz = dev(band(mean, 0.0, R / 2, 0.0, 0.0), 0.0);
    F.mono_hz = dev(band(mean, (double)cfg->dc_guard_hz, 15000.0, 0.0, 0.0), 15000.0);
    F.stereo_hz = dev(band(mean, 23000.0, 53000.0, 38000.0 - half, 38000.0 + half), 53000.0);
    F.rds_hz = dev(band(mean, 54600.0, 59400.0, 0.0, 0.0), 59400.0);
    const double aux_hi = std::min(94000.0, R / 2);
    F.aux_hz = aux_hi > 61000.0 ? dev(band(mean, 61000.0, aux_hi, 0.0, 0.0), aux_hi) : -HUGE_VAL;
    auto line = [&](double f0) { const Sum a = band(mean, f0 - half, f0 + half, 0.0, 0.0); return (a.n > 0 && 2.0 * (f0 + half) <= R) ? u * std::sqrt(2.0 * power(a)) : -HUGE_VAL; };
    F.pilot_hz = line(19000.0);
    F.carrier38_hz = line(38000.0);
    F.pilot_freq_hz = F.floor_hz_rt_hz = F.pilot_cn0_db = -HUGE_VAL;
    if (F.pilot_hz > -HUGE_VAL) {
        double s = 0.0, m = 0.0;
        for (int k = 0; k < BINS; k++) if (usable(k) && in(k, 19000.0 - half, 19000.0 + half)) { s += (double)mean[k]; m += (double)mean[k] * ((double)k * df); }
        if (s > 0.0) F.pilot_freq_hz = m / s;
    }
    if (2.0 * 22500.0 <= R) {
        const Sum g1 = band(mean, 15500.0, 18500.0, 0.0, 0.0), g2 = band(mean, 19500.0, 22500.0, 0.0, 0.0);
        const Sum g{g1.s + g2.s, g1.n + g2.n};
        if (g.n > 0) {
            const double density = power(g) / ((double)g.n * df);                      // power per hertz
            F.floor_hz_rt_hz = u * std::sqrt(density);
            const Sum p = band(mean, 19000.0 - half, 19000.0 + half, 0.0, 0.0);
            if (density > 0.0 && p.n > 0 && p.s > 0.0) F.pilot_cn0_db = 10.0 * std::log10(power(p) / density);
        }
    }
    for (int i = 0; i < MAX_BANDS; i++) F.band_hz[i] = F.band_line_hz[i] = F.band_hold_line_hz[i] = F.band_hold_over_mean_db[i] = -HUGE_VAL;
    for (int i = 0; i < cfg->n_bands; i++) {
        const fmx_mpx_band &b = cfg->bands[i];
        const Sum a = band(mean, b.lo_hz, b.hi_hz, 0.0, 0.0);
        if (a.n == 0) continue;
        F.band_hz[i] = u * std::sqrt(power(a));
        int km = -1, kp = -1;
        for (int k = 0; k < BINS; k++) if (usable(k) && in(k, b.lo_hz, b.hi_hz)) {
            if (km < 0 || mean[k] > mean[km]) km = k;
            if (peak && (kp < 0 || peak[k] > peak[kp])) kp = k;
        }
        F.band_line_hz[i] = (double)km * df;
        if (kp >= 0) {
            F.band_hold_line_hz[i] = (double)kp * df;
            if (mean[kp] > 0.f && peak[kp] > 0.f) F.band_hold_over_mean_db[i] = 10.0 * std::log10((double)peak[kp] / (double)mean[kp]);
        }
    }
    *out = F;
    return FMX_OK;
}

}  // namespace mpx
}  // namespace fmx

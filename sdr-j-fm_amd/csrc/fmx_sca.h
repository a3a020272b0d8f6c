// fmx_sca.h -- the sub-carrier decoder (include/fmx.h fmx_sca_*; no counterpart in the reference, which stops at 59.4 kHz): the audio of
// an FM sub-carrier (SCA) at 67, 76 or 82 kHz of a channel's demodulator output d [j] at fmRate R -- the row w_dem stage B leaves behind, FMX_TAP_DEMOD's
// value.  Everything that decides is here, as pure functions -- fmx_api.hip decides with them, fmx_sca.hip runs them, tests/sca_check.cpp drives them on
// the CPU:
//   design_band (), design_audio (): the two filters, in double, rounded to f32: g [192] and a [128], the same for every channel;
//   mixed_taps (), rotation (): THE FORM OF THE F32 ARITHMETIC.  The mix is folded into per-channel complex taps
//       c [k] = f32 (g [k] cos (2 pi ((centre k) mod R) / R)), f32 (g [k] sin (2 pi ((centre k) mod R) / R))          (double, then rounded)
//     so that  y' [m] = sum_k c [k] d [4 m - k] = y [m] exp (+2 pi i ((4 m centre) mod R) / R):  |y'| = |y|, and
//       y [m] conj (y [m - 1]) = y' [m] conj (y' [m - 1]) rot,   rot = exp (-2 pi i ((4 centre) mod R) / R), one constant per channel.
//     No phase is formed per sample, so nothing grows with j: the arithmetic at fm sample 2^40 is the arithmetic at fm sample 0.
//   the grid: block b is the audio samples [240 b, 240 b + 240) = the fm samples [1920 b, 1920 b + 1920); it reads d [1920 b - 703, 1920 b + 1920);
//   first_block (), piece (): the switch's rule and what a piece [J0, J0 + nj) of a call means for a channel switched on by the piece that began at
//     on_from: the blocks it completes, the carry it reads and the carry it leaves;
//   y_of (), u_of (), s_of (), level_of (): the per-sample functions, every product an fmaf in ascending tap order -- the host's and the kernel's y', s
//     and level are the same bits; u goes through atan2f, whose last bit is the library's.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/fmx.h"

namespace fmx {
namespace sca {

constexpr int NG = 192, NA = 128;                          // taps of the band filter at R, of the audio filter at R / 4
constexpr int NLP = 81, NDE = 48;                          // the audio filter's low-pass and de-emphasis factors: 81 + 48 - 1 = 128
constexpr int D1 = 4, D2 = 2;                              // R -> R / 4 (y, u) -> R / 8 (s)
constexpr int BLOCK_FM = 1920, BLOCK_Y = BLOCK_FM / D1, BLOCK_AUDIO = BLOCK_Y / D2;      // 1920, 480, 240
constexpr int LOOKBACK = (NG - 1) + D1 * NA;               // 703: a block reads d [1920 b - 703, 1920 b + 1920)
constexpr int SPAN = LOOKBACK + BLOCK_FM;                  // 2623 samples of d per block
constexpr int NY = NA + BLOCK_Y;                           // 608: y' [480 b - 128 .. 480 b + 479], local index i <-> m = 480 b - 128 + i
constexpr int NU = NY - 2;                                 // 606: u [480 b - 127 .. 480 b + 478], local index i <-> y' local i + 1 and i
constexpr int CARRY_MAX = LOOKBACK + BLOCK_FM - 1;         // 2622 samples carried at the most
constexpr int CARRY_STRIDE = 2624;                         // floats per slot of the carry
constexpr int RING = 128;                                  // blocks kept per decoding channel
constexpr int NT = 256;                                    // threads of a workgroup
constexpr double BETA = 7.0;
constexpr int MPX_TOP_HZ = 59400, GUARD_HZ = 2000;         // what the chain demodulates ends at 57 000 + 2400 Hz; the band filter's transition
// bytes of device memory per decoding channel: the ring's audio and levels, the carry, the mixed taps and the rotation
constexpr int64_t BYTES_PER_CHANNEL = (int64_t)sizeof(float) * (RING * (BLOCK_AUDIO + 1) + CARRY_STRIDE + 2 * NG + 2);      // 135 432

// ---- the designs (double on the host, rounded to f32) ---------------------------------------------------------------------------------------
inline double bessel_i0(double x) {
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 64; k++) { t *= (x / (2.0 * k)) * (x / (2.0 * k)); s += t; if (t < 1e-18 * s) break; }
    return s;
}
// an n-tap Kaiser-windowed sinc with its 6 dB point at f6 Hz at `rate`, not normalised
inline std::vector<double> kaiser_lowpass(int n, double f6, double rate) {
    std::vector<double> h((size_t)n);
    const double mid = (n - 1) / 2.0, fc = 2.0 * f6 / rate, pi = 3.14159265358979323846;
    for (int i = 0; i < n; i++) {
        const double x = i - mid, r = x / mid;
        const double w = bessel_i0(BETA * std::sqrt(std::max(0.0, 1.0 - r * r))) / bessel_i0(BETA);
        h[(size_t)i] = (x == 0.0 ? fc : std::sin(pi * fc * x) / (pi * x)) * w;
    }
    return h;
}
inline void normalise(std::vector<double> &h) { double s = 0.0; for (double v : h) s += v; for (double &v : h) v /= s; }

inline const char *config_error(const fmx_sca_config *cfg, int32_t R) {
    if (!cfg) return "cfg is null";
    if (cfg->struct_size != (int32_t)sizeof(fmx_sca_config)) return "fmx_sca_config.struct_size mismatch";
    if (R < 8000 || R > 1000000 || R % 8 != 0) return "fmRate must be a multiple of 8 in [8000, 1000000]";
    if (cfg->half_band_hz < 1000 || cfg->half_band_hz > 20000) return "half_band_hz must be in [1000, 20000]";
    if (cfg->audio_cut_hz < 1000 || cfg->audio_cut_hz > 10000) return "audio_cut_hz must be in [1000, 10000]";
    if (cfg->deviation_hz < 100 || cfg->deviation_hz > 20000) return "deviation_hz must be in [100, 20000]";
    if (cfg->deemphasis_us < 0 || cfg->deemphasis_us > 1000) return "deemphasis_us must be in [0, 1000]";
    if (2 * (cfg->half_band_hz + GUARD_HZ) >= R) return "half_band_hz + 2000 must lie below fmRate / 2";
    if (8 * (cfg->audio_cut_hz + 1300) >= R) return "audio_cut_hz + 1300 must lie below fmRate / 8";
    return nullptr;
}
inline fmx_sca_config default_config() { return fmx_sca_config{(int32_t)sizeof(fmx_sca_config), 9000, 5000, 6000, 150}; }

// g [0 .. 191]: 6 dB point at half_band_hz + 2000 at rate R, sum 1
inline std::vector<float> design_band(const fmx_sca_config &cfg, int32_t R) {
    std::vector<double> h = kaiser_lowpass(NG, (double)(cfg.half_band_hz + GUARD_HZ), (double)R);
    normalise(h);
    return std::vector<float>(h.begin(), h.end());
}
// a [0 .. 127]: the 81-tap low-pass at R / 4 (6 dB point at audio_cut_hz + 1300) convolved with the first 48 values of (1 - alpha) alpha^i,
// alpha = exp (-4 / (R tau)) -- the unit impulse for tau = 0 --, the convolution normalised to sum 1
inline std::vector<float> design_audio(const fmx_sca_config &cfg, int32_t R) {
    const std::vector<double> lp = kaiser_lowpass(NLP, (double)(cfg.audio_cut_hz + 1300), (double)R / D1);
    std::vector<double> de((size_t)NDE, 0.0);
    if (cfg.deemphasis_us == 0) de[0] = 1.0;
    else {
        const double alpha = std::exp(-(double)D1 / ((double)R * (double)cfg.deemphasis_us * 1e-6));
        double p = 1.0 - alpha;
        for (int i = 0; i < NDE; i++) { de[(size_t)i] = p; p *= alpha; }
    }
    std::vector<double> h((size_t)NA, 0.0);
    for (int i = 0; i < NLP; i++) for (int k = 0; k < NDE; k++) h[(size_t)(i + k)] += lp[(size_t)i] * de[(size_t)k];
    normalise(h);
    return std::vector<float>(h.begin(), h.end());
}
// c [k] of the head: the mix folded into the band filter, the phase reduced in integers
inline std::vector<float2> mixed_taps(const std::vector<float> &g, int32_t centre_hz, int32_t R) {
    std::vector<float2> c((size_t)NG);
    const double w = 2.0 * 3.14159265358979323846 / (double)R;
    for (int k = 0; k < NG; k++) {
        const double ph = w * (double)(((int64_t)centre_hz * k) % R);
        c[(size_t)k] = make_float2((float)((double)g[(size_t)k] * std::cos(ph)), (float)((double)g[(size_t)k] * std::sin(ph)));
    }
    return c;
}
// rot of the head
inline float2 rotation(int32_t centre_hz, int32_t R) {
    const double ph = 2.0 * 3.14159265358979323846 * (double)(((int64_t)centre_hz * D1) % R) / (double)R;
    return make_float2((float)std::cos(ph), (float)(-std::sin(ph)));
}
// u's scale: R / (8 pi deviation_hz)
inline float u_scale(const fmx_sca_config &cfg, int32_t R) { return (float)((double)R / (8.0 * 3.14159265358979323846 * (double)cfg.deviation_hz)); }
// fmx_sca_enable's rule; nullptr: accepted.  Below, the pass band's edge may come within the filter's 2000 Hz transition of the top of the RDS band
// (59 400 Hz) -- 67 000 Hz with the default 9000 Hz passes at 58 000 --; above, the whole filter, transition included, stays below fmRate / 2.
inline const char *centre_error(int32_t centre_hz, int32_t half_band_hz, int32_t R) {
    if (centre_hz == 0) return nullptr;
    if ((int64_t)centre_hz - half_band_hz + GUARD_HZ < MPX_TOP_HZ) return "centre_hz - half_band_hz + 2000 lies below 59 400 Hz: the pass band reaches into what the chain demodulates";
    if (2 * ((int64_t)centre_hz + half_band_hz + GUARD_HZ) > R) return "centre_hz + half_band_hz + 2000 lies above fmRate / 2";
    return nullptr;
}

// ---- the grid, the switch, a piece ----------------------------------------------------------------------------------------------------------
// the first fm sample block b reads
__host__ __device__ __forceinline__ int64_t block_from(int64_t b) { return (int64_t)BLOCK_FM * b - LOOKBACK; }
// the first delivered block of a channel switched on by the piece that began at fm sample on_from: the first with 1920 b - 703 >= on_from
__host__ __device__ __forceinline__ int64_t first_block(int64_t on_from) { return (on_from + LOOKBACK + BLOCK_FM - 1) / BLOCK_FM; }
// where the carry of a channel begins when the stream stands at fm sample J: what the next block to complete reads first -- the block in progress at J,
// or the channel's first block where that comes later.  The carry holds d [carry_from, J) (nothing where carry_from >= J): a pure function of J and first.
__host__ __device__ __forceinline__ int64_t carry_from(int64_t J, int64_t first) {
    const int64_t b = J / BLOCK_FM;
    return block_from(b > first ? b : first);
}
struct Piece {
    int64_t b0, blocks;          // the blocks the piece completes and delivers: b0 .. b0 + blocks - 1 (blocks 0: none)
    int64_t carry_from0;         // the old carry holds d [carry_from0, J0) ...
    int32_t carry_len0;          // ... carry_len0 samples (0 .. 2622)
    int64_t carry_from1;         // the new carry holds d [carry_from1, J0 + nj) ...
    int32_t carry_len1;          // ... carry_len1 samples (0 .. 2622),
    int32_t from_carry;          // the first from_carry of them out of the old carry, from its index carry_from1 - carry_from0 on,
    int64_t row_src;             // the rest out of the piece's row, from its index row_src on
};
// (first: the channel's first delivered block)
__host__ __device__ inline Piece piece_first(int64_t J0, int64_t nj, int64_t first) {
    Piece p;
    const int64_t J1 = J0 + nj;
    const int64_t bn = J0 / BLOCK_FM, be = J1 / BLOCK_FM;            // blocks [bn, be) have their last fm sample in the piece
    p.b0 = bn > first ? bn : first;
    p.blocks = be > p.b0 ? be - p.b0 : 0;
    p.carry_from0 = carry_from(J0, first);
    p.carry_len0 = p.carry_from0 < J0 ? (int32_t)(J0 - p.carry_from0) : 0;
    p.carry_from1 = carry_from(J1, first);
    p.carry_len1 = p.carry_from1 < J1 ? (int32_t)(J1 - p.carry_from1) : 0;
    p.from_carry = (p.carry_len1 > 0 && p.carry_from1 < J0) ? (int32_t)(J0 - p.carry_from1) : 0;
    p.row_src = p.carry_from1 > J0 ? p.carry_from1 - J0 : 0;
    return p;
}
__host__ __device__ inline Piece piece(int64_t J0, int64_t nj, int64_t on_from) { return piece_first(J0, nj, first_block(on_from)); }
// sample i (0 .. 2622) of block b's span, d [1920 b - 703 + i], of a piece that begins at J0: out of the carry (which begins at carry_from0) or the row
__host__ __device__ __forceinline__ float span_sample(int64_t b, int i, int64_t J0, int64_t carry_from0, const float *carry, const float *row) {
    const int64_t j = block_from(b) + i;
    return j < J0 ? carry[j - carry_from0] : row[j - J0];
}
// sample i of the new carry
__host__ __device__ __forceinline__ float carry_sample(const Piece &p, int i, const float *carry, const float *row) {
    return i < p.from_carry ? carry[(p.carry_from1 - p.carry_from0) + i] : row[p.row_src + (i - p.from_carry)];
}

// ---- the per-sample functions (span: the block's 2623 samples of d; yl: 608 y'; ul: 606 u) ----------------------------------------------------
// y' local i: sum_k c [k] d [4 m - k], k ascending; d [4 m - k] is span [4 i + 191 - k]
__host__ __device__ __forceinline__ float2 y_of(int i, const float *span, const float2 *c) {
    float re = 0.f, im = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
    // (the same sums in the same order, four taps per step: span [4 i ..] and c are 16-byte aligned in LDS)
    const float4 *x4 = reinterpret_cast<const float4 *>(span + D1 * i);
    const float4 *c4 = reinterpret_cast<const float4 *>(c);
#pragma unroll 4
    for (int q = 0; q < NG / 4; q++) {
        const float4 v = x4[NG / 4 - 1 - q], t0 = c4[2 * q], t1 = c4[2 * q + 1];      // v.w .. v.x: d [4 m - 4 q] .. d [4 m - 4 q - 3]
        re = fmaf(t0.x, v.w, re); im = fmaf(t0.y, v.w, im);
        re = fmaf(t0.z, v.z, re); im = fmaf(t0.w, v.z, im);
        re = fmaf(t1.x, v.y, re); im = fmaf(t1.y, v.y, im);
        re = fmaf(t1.z, v.x, re); im = fmaf(t1.w, v.x, im);
    }
#else
    const float *x = span + D1 * i + (NG - 1);
    for (int k = 0; k < NG; k++) { const float v = x[-k]; re = fmaf(c[k].x, v, re); im = fmaf(c[k].y, v, im); }
#endif
    return make_float2(re, im);
}
// u local i from y' local i + 1 (y1) and i (y0): z = y1 conj (y0), rotated by rot; arg (0) = 0
__host__ __device__ __forceinline__ float u_of(float2 y1, float2 y0, float2 rot, float scale) {
    const float zr = fmaf(y1.x, y0.x, y1.y * y0.y), zi = fmaf(y1.y, y0.x, -(y1.x * y0.y));
    const float wr = fmaf(zr, rot.x, -(zi * rot.y)), wi = fmaf(zr, rot.y, zi * rot.x);
    if (wr == 0.f && wi == 0.f) return 0.f;
    return atan2f(wi, wr) * scale;
}
// s local n (0 .. 239): sum_k a [k] u [2 n - k], k ascending; u [2 n - k] is ul [2 n + 127 - k]
__host__ __device__ __forceinline__ float s_of(int n, const float *ul, const float *a) {
    const float *x = ul + D2 * n + (NA - 1);
    float s = 0.f;
    for (int k = 0; k < NA; k++) s = fmaf(a[k], x[-k], s);
    return s;
}
// |y'|^2
__host__ __device__ __forceinline__ float power_of(float2 y) { return fmaf(y.x, y.x, y.y * y.y); }
// The level's sum over the block's 480 powers p [i] = |y' local 128 + i|^2, in the kernel's order: thread t holds q [t] = p [t] + p [t + 256] (t < 224)
// or p [t] (t < 256), then q [t] += q [t + h] for h = 128, 64, .. 1 and t < h; the level is q [0] / 480
inline float level_of(const float *p) {
    float q[NT];
    for (int t = 0; t < NT; t++) q[t] = t + NT < BLOCK_Y ? p[t] + p[t + NT] : p[t];
    for (int h = NT / 2; h > 0; h >>= 1) for (int t = 0; t < h; t++) q[t] += q[t + h];
    return q[0] * (1.0f / BLOCK_Y);
}
// one block on the host, as fmx_sca.hip forms it: audio [240], level
inline void block_host(const float *span, const float2 *c, const float *a, float2 rot, float scale, float *audio, float *level) {
    std::vector<float2> yl((size_t)NY);
    std::vector<float> ul((size_t)NU), p((size_t)BLOCK_Y);
    for (int i = 0; i < NY; i++) yl[(size_t)i] = y_of(i, span, c);
    for (int i = 0; i < NU; i++) ul[(size_t)i] = u_of(yl[(size_t)i + 1], yl[(size_t)i], rot, scale);
    for (int n = 0; n < BLOCK_AUDIO; n++) audio[n] = s_of(n, ul.data(), a);
    for (int i = 0; i < BLOCK_Y; i++) p[(size_t)i] = power_of(yl[(size_t)(NA + i)]);
    *level = level_of(p.data());
}

}  // namespace sca
}  // namespace fmx

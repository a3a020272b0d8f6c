// fmx_survey.h -- the band survey of stage W (include/fmx.h fmx_wideband_survey_*; no counterpart in the reference): a windowed
// 4096-point power spectrum of every block of 4096 wide samples, summed block by block into records, and the host's station finder over a
// record.  Written so that the very same arithmetic runs on the host: tests/survey_check.cpp drives the stage functions below thread by thread
// against a float64 model, and the per-call bookkeeping (plan) and the finder (find) need no device at all.
//
// One workgroup of 256 threads per block.  4096 = 16 * 16 * 16, n = n0 + 16 n1 + 256 n2, k = a + 16 b + 256 c, W = exp (-2 pi i / 4096):
//   X [a + 16 b + 256 c] = sum_n0 W16^(n0 c) W^(n0 (a + 16 b)) [ sum_n1 W16^(n1 b) W^(16 n1 a) [ sum_n2 W16^(n2 a) x [n0 + 16 n1 + 256 n2] ] ]
// Pass 1 (thread t = n0 + 16 n1): the 16-point DFT over n2 of the windowed samples t + 256 n2 (coalesced loads), times W^(16 n1 a).
// Pass 2 (thread t = n0 + 16 a):  the 16-point DFT over n1, times W^(n0 (a + 16 b)).
// Pass 3 (thread t = a + 16 b):   the 16-point DFT over n0; the thread owns bins t + 256 c (coalesced stores of Re^2 + Im^2).
// Two exchanges through one LDS image of float2, 8-byte stores (ds_write_b64: four groups of 16 consecutive lanes, bank = dword mod 32, so a
// group is conflict-free when its 16 element indices differ mod 16) and 8-byte reads (ds_read_b64: two groups of 32 lanes, bank = dword mod
// 64: conflict-free when the 32 element indices differ mod 32):
//   exchange 1, element (n0, n1, a) at n0 + 16 a + 256 n1: a store group is n0 = 0..15 at one (n1, a) -- 16 consecutive elements; a read group
//     is n0 = 0..15 with a = 2 m, 2 m + 1 at one n1 -- 32 consecutive elements.  No padding needed.
//   exchange 2, element (n0, a, b) at a + 16 b + PAD n0, PAD = 257: a read group is a = 0..15 with b = 2 m, 2 m + 1 at one n0 -- 32 consecutive
//     elements; a store group is n0 = 0..15 at one (a, b) -- elements 257 n0 = n0 (mod 16), all different.  With PAD = 256 the 16 stores of a
//     group would meet on one pair of banks.
// The image is 16 * 257 float2 = 32 896 bytes (32 KB + 128 B of padding).  Both exchanges are conflict-free.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/fmx.h"
#include "fmx_scan.h"

namespace fmx {
namespace survey {

constexpr int N = 4096, NT = 256, PER = 16;
constexpr int PAD = 257;                     // exchange 2's pitch of n0 (odd: see above)
constexpr int LDS_N = PER * PAD;             // float2 per workgroup
constexpr int RING = 4;                      // records kept per stream
constexpr int MAX_B = 4096;                  // blocks per record
constexpr int RATE0 = 2304000;               // the narrow rate: Rw = factor * RATE0

// the periodic Hann window, f64 rounded to f32, and 1 / (B sum w^2) (sum of the ROUNDED window's squares, in f64) rounded to f32
inline void make_window(float *w) {
    for (int i = 0; i < N; i++) w[i] = (float)(0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * (double)i / (double)N));
}
inline float record_scale(const float *w, int B) {
    double s = 0.0;
    for (int i = 0; i < N; i++) s += (double)w[i] * (double)w[i];
    return (float)(1.0 / ((double)B * s));
}
// the twiddle table: W [m] = exp (-2 pi i m / 4096), rounded from double once (as scan::make_twiddles)
inline void make_twiddles(float2 *W) {
    for (int m = 0; m < N; m++) {
        const double a = -2.0 * 3.14159265358979323846 * (double)m / (double)N;
        W[m] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
}

// Where sample i of the call's block j lies: the survey's samples of a call are the carry's `fill`, then the call's own.  >= 0: index into the
// call's input; < 0: carry [fill + index].
__host__ __device__ __forceinline__ int64_t source_index(int64_t j, int i, int fill) { return j * N + i - fill; }

// forward 16-point DFT, scan::stage1's (p = a + 4 b, q = c + 4 e: 4-point DFTs over b, the twiddles W16^(a c) = W [256 a c], 4-point DFTs over a)
__host__ __device__ __forceinline__ void dft16(const float2 *x, const float2 *W, float2 *z) {
    float2 u[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        u[a][0] = x[a]; u[a][1] = x[a + 4]; u[a][2] = x[a + 8]; u[a][3] = x[a + 12];
        scan::dft4(u[a][0], u[a][1], u[a][2], u[a][3]);
#pragma unroll
        for (int c = 1; c < 4; c++) if (a > 0) u[a][c] = scan::cmul(u[a][c], W[256 * a * c]);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float2 v0 = u[0][c], v1 = u[1][c], v2 = u[2][c], v3 = u[3][c];
        scan::dft4(v0, v1, v2, v3);
        z[c] = v0; z[c + 4] = v1; z[c + 8] = v2; z[c + 12] = v3;
    }
}

// Pass 1 of thread t = n0 + 16 n1: x [n2] = the windowed sample t + 256 n2 in, element (n0, n1, a) of exchange 1 out.
__host__ __device__ __forceinline__ void pass1(int t, const float2 *x, const float2 *W, float2 *lds) {
    const int n0 = t & 15, n1 = t >> 4;
    float2 z[PER];
    dft16(x, W, z);
#pragma unroll
    for (int a = 0; a < PER; a++) lds[n0 + 16 * a + 256 * n1] = a == 0 ? z[0] : scan::cmul(z[a], W[16 * n1 * a]);
}
// Pass 2 of thread t = n0 + 16 a, in two halves with the workgroup's barrier between them: the loads of exchange 1 ...
__host__ __device__ __forceinline__ void pass2_load(int t, const float2 *lds, float2 *y) {
#pragma unroll
    for (int n1 = 0; n1 < PER; n1++) y[n1] = lds[t + 256 * n1];
}
// ... and the DFT over n1, the twiddles and the stores of exchange 2
__host__ __device__ __forceinline__ void pass2_store(int t, const float2 *y, const float2 *W, float2 *lds) {
    const int n0 = t & 15, a = t >> 4;
    float2 z[PER];
    dft16(y, W, z);
#pragma unroll
    for (int b = 0; b < PER; b++) lds[a + 16 * b + PAD * n0] = scan::cmul(z[b], W[n0 * (a + 16 * b)]);
}
// Pass 3 of thread t = a + 16 b: the DFT over n0 and p [c] = |X [t + 256 c]|^2.
__host__ __device__ __forceinline__ void pass3(int t, const float2 *lds, const float2 *W, float *p) {
    float2 y[PER], z[PER];
#pragma unroll
    for (int n0 = 0; n0 < PER; n0++) y[n0] = lds[t + PAD * n0];
    dft16(y, W, z);
#pragma unroll
    for (int c = 0; c < PER; c++) p[c] = fmaf(z[c].x, z[c].x, z[c].y * z[c].y);
}

// One bin of one stream over a call's blocks, in block order: p [j * N] is block j's power.  `phase` blocks of the current record are in `acc`
// already; at every record boundary the sum is scaled (one multiply), written to ring [slot * N] and cleared, slot counting on mod RING.
// Returns the accumulator behind the call.
__host__ __device__ __forceinline__ float accumulate(float acc, const float *p, int64_t nb, int phase, int B, float scale, float *ring, int slot) {
    for (int64_t j = 0; j < nb; j++) {
        acc += p[j * N];
        if (++phase == B) {
            ring[(size_t)slot * N] = acc * scale;
            acc = 0.f; phase = 0; slot = (slot + 1) & (RING - 1);
        }
    }
    return acc;
}

// ---- a call's bookkeeping: integers only -----------------------------------------------------------------------------------------------
struct Plan {
    int64_t blocks;          // blocks the call completes
    int32_t fill;            // samples carried behind it (0 .. N - 1)
    int32_t phase;           // blocks of the current record summed before the call (0 .. B - 1)
    int64_t record0;         // index of the record the call's first block belongs to
    int64_t records;         // records the call completes: record0 .. record0 + records - 1
};
inline Plan plan(int32_t fill, int64_t n_wide, int64_t blocks_so_far, int32_t B) {
    Plan p;
    const int64_t total = (int64_t)fill + n_wide;
    p.blocks = total / N;
    p.fill = (int32_t)(total % N);
    p.phase = (int32_t)(blocks_so_far % B);
    p.record0 = blocks_so_far / B;
    p.records = (blocks_so_far + p.blocks) / B - p.record0;
    return p;
}

// ---- the station finder (include/fmx.h fmx_wideband_survey_stations): f64 sums, membership of a bin in a window decided in integers -------
// Rw: the stream's rate, which the caller has checked (cfg->factor must then be 0), or 0: cfg->factor * 2 304 000.
// Returns FMX_OK, FMX_E_INVALID (*why says which argument) or FMX_E_TOO_LARGE.
inline int find(const fmx_survey_find *cfg, int64_t Rw, const float *power, fmx_survey_station *out, int32_t capacity, int32_t *n_stations,
                float *floor_db, const char **why) {
    *why = "";
    if (!cfg || !power || !n_stations || (!out && capacity > 0) || capacity < 0) { *why = "null argument"; return FMX_E_INVALID; }
    if (cfg->struct_size != (int32_t)sizeof(fmx_survey_find)) { *why = "fmx_survey_find.struct_size mismatch"; return FMX_E_INVALID; }
    if (Rw > 0 && cfg->factor != 0) { *why = "factor must be 0 where a wide rate is given"; return FMX_E_INVALID; }
    if (Rw <= 0 && (cfg->factor < 2 || cfg->factor > 16)) { *why = "factor must be in [2, 16]"; return FMX_E_INVALID; }
    if (Rw <= 0) Rw = (int64_t)cfg->factor * RATE0;
    if (cfg->raster_hz < 50000 || cfg->raster_hz > 1000000) { *why = "raster_hz must be in [50000, 1000000]"; return FMX_E_INVALID; }
    if (cfg->origin_hz <= -cfg->raster_hz || cfg->origin_hz >= cfg->raster_hz) { *why = "|origin_hz| must be < raster_hz"; return FMX_E_INVALID; }
    if (cfg->dc_guard_hz < 0 || cfg->dc_guard_hz > 99999) { *why = "dc_guard_hz must be in [0, 99999]"; return FMX_E_INVALID; }
    for (int k = 0; k < N; k++)
        if (!(power[k] >= 0.f) || !std::isfinite(power[k])) { *why = "power holds a negative or non-finite entry"; return FMX_E_INVALID; }
    *n_stations = 0;
    const int64_t raster = cfg->raster_hz;
    // bin k lies at kp Rw / N Hz; every comparison with a frequency is made on kp Rw against the frequency times N
    auto kp = [](int k) { return (int64_t)(k < N / 2 ? k : k - N); };
    auto usable = [&](int k) { const int64_t f = kp(k) * Rw; return (f < 0 ? -f : f) >= (int64_t)cfg->dc_guard_hz * N; };
    // the floor: the lower decile of the usable bins inside |f| <= Rw / 2 - 50 000
    std::vector<float> sorted;
    for (int k = 0; k < N; k++) {
        const int64_t f = kp(k) * Rw;
        if (usable(k) && (f < 0 ? -f : f) <= (Rw / 2 - 50000) * N) sorted.push_back(power[k]);
    }
    std::sort(sorted.begin(), sorted.end());
    const double F = sorted.empty() ? 0.0 : (double)sorted[sorted.size() / 10];
    if (floor_db) *floor_db = (float)(10.0 * std::log10(F));
    if (!(F > 0.0)) return FMX_OK;
    // the candidates f_j = origin + j raster inside the limit of fmx_wideband_set_offset, ascending, and their levels
    const int64_t lim = Rw / 2 - 150000;
    auto floor_div = [](int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && (a < 0) != (b < 0)) ? q - 1 : q; };
    const int64_t j_lo = -floor_div(lim + cfg->origin_hz, raster), j_hi = floor_div(lim - cfg->origin_hz, raster);
    std::vector<double> level;
    for (int64_t j = j_lo; j <= j_hi; j++) {
        const int64_t fj = cfg->origin_hz + j * raster;
        double sum = 0.0; int64_t n = 0;
        for (int k = 0; k < N; k++) {
            const int64_t d = kp(k) * Rw - fj * N;
            if (usable(k) && (d < 0 ? -d : d) <= (int64_t)100000 * N) { sum += (double)power[k]; n++; }
        }
        level.push_back(n ? sum / (double)n : 0.0);
    }
    const int64_t reach = (200000 - 1) / raster;          // neighbours: |j' - j| raster < 200 000
    int32_t found = 0;
    for (int64_t i = 0; i < (int64_t)level.size(); i++) {
        const double c = level[(size_t)i];
        if (!(c > 0.0)) continue;
        const double snr = 10.0 * std::log10(c / F);
        if (!(snr > (double)cfg->threshold_db)) continue;
        bool wins = true;
        for (int64_t q = std::max<int64_t>(0, i - reach); q <= std::min<int64_t>((int64_t)level.size() - 1, i + reach) && wins; q++)
            if ((q < i && !(c >= level[(size_t)q])) || (q > i && !(c > level[(size_t)q]))) wins = false;
        if (!wins) continue;
        if (found < capacity) {
            fmx_survey_station &s = out[found];
            s.offset_hz = (int32_t)(cfg->origin_hz + (j_lo + i) * raster);
            s.level_db = (float)(10.0 * std::log10(c)); s.snr_db = (float)snr; s.reserved = 0;
        }
        found++;
    }
    *n_stations = found;
    if (found > capacity) { *why = "capacity is smaller than the number of stations"; return FMX_E_TOO_LARGE; }
    return FMX_OK;
}

}  // namespace survey
}  // namespace fmx

// fmx_scan.h -- the reference's scan mode (fm-processor.cpp:478-495, getSignal / getNoise :886-904, get_db fm-constants.h:144):
// a 1024-point forward transform of every block of 1024 fm-rate samples, the means of |X [k]| over the 40 "signal" bins (k = 5..24,
// 999..1018) and the 40 "noise" bins (k = 487..506, 518..537), and their dB values.  Written so that the very same arithmetic runs on
// the host: tests/scan_check.cpp drives the stage functions below lane by lane against a float64 DFT and the reference's own
// Fft_transform.
//
// One wave per block.  1024 = 16 * 64, n = t + 64 p, k = q + 16 r:
//   X [q + 16 r] = sum_t W64^(t r) [ W1024^(t q) sum_p x [t + 64 p] W16^(p q) ]
// Stage 1 (registers): lane t takes x [t + 64 p], p = 0..15, makes the 16-point DFT over p and the twiddles W1024^(t q): z [t][q].
// Stage 2 (LDS): only 80 bins are read, and their r = k / 16 are 0, 1, 30, 31, 32, 33, 62, 63 -- d and d + 32 for d in {0, 1, 62, 63}.
// With W64^(t (d + 32)) = (-1)^t W64^(t d), lane (q, d) sums the even t and the odd t of z [t][q] W64^(t d) apart (A, B) and has
// X [q + 16 d] = A + B and X [q + 16 (d + 32)] = A - B: a pruned transform of 64 complex products per lane.
// LDS image of z: element (t, q) at t * SCAN_ROW + q, SCAN_ROW = 17.  Stage 1's stores (ds_write_b64: lanes in groups of 16) put the
// 16 lanes of a group on dwords 34 t + 2 q = 2 t + 2 q (mod 32): all distinct.  Stage 2's reads (ds_read_b64: groups of 32 lanes,
// 16 distinct addresses, each read by two lanes) cover 16 consecutive elements of one row: all distinct banks.  Conflict-free.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace fmx {
namespace scan {

constexpr int N = 1024, LANES = 64, PER = 16;
constexpr int ROW = PER + 1;                 // LDS row of one lane's 16 outputs, padded
constexpr int LDS_N = LANES * ROW;           // float2 per wave
constexpr int RING = 1024;                   // records kept per channel
constexpr int SIG_LO = 5, SIG_HI = 25;       // getSignal: i = 5 .. 24 -> k = i and size - 1 - i
constexpr float DB_REF = 256.0f;             // get_db (x, 256)

// lane (q, di) of stage 2: q = lane & 15, d = {0, 1, 62, 63} [lane >> 4]
__host__ __device__ __forceinline__ int stage2_d(int lane) { const int di = lane >> 4; return di < 2 ? di : 60 + di; }

// 1: a getSignal bin, 2: a getNoise bin, 0: neither
__host__ __device__ __forceinline__ int bin_class(int k) {
    if ((k >= SIG_LO && k < SIG_HI) || (k >= N - SIG_HI && k < N - SIG_LO)) return 1;
    if ((k >= N / 2 - SIG_HI && k < N / 2 - SIG_LO) || (k > N / 2 + SIG_LO && k <= N / 2 + SIG_HI)) return 2;
    return 0;
}

// get_db (mean, 256) = 20 log10 ((x + 1) / (float) 256) of a 40-bin mean, as the reference takes it in float
__host__ __device__ __forceinline__ float get_db(float sum40) {
    const float mean = sum40 / 40.0f;
    return 20.0f * log10f((mean + 1.0f) / DB_REF);
}

__host__ __device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}
__host__ __device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__host__ __device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__host__ __device__ __forceinline__ float2 mul_mj(float2 a) { return make_float2(a.y, -a.x); }      // -j a
__host__ __device__ __forceinline__ float cabs(float2 a) { return sqrtf(fmaf(a.x, a.x, a.y * a.y)); }

// the twiddle table: W [m] = exp (-2 pi i m / 1024), m = 0..1023, rounded from double (the host builds it; the device reads it)
inline void make_twiddles(float2 *W) {
    for (int m = 0; m < N; m++) {
        const double a = -2.0 * 3.14159265358979323846 * (double)m / (double)N;
        W[m] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
}

// forward 4-point DFT in place
__host__ __device__ __forceinline__ void dft4(float2 &a0, float2 &a1, float2 &a2, float2 &a3) {
    const float2 s02 = cadd(a0, a2), d02 = csub(a0, a2), s13 = cadd(a1, a3), d13 = mul_mj(csub(a1, a3));
    a0 = cadd(s02, s13); a2 = csub(s02, s13); a1 = cadd(d02, d13); a3 = csub(d02, d13);
}

// Stage 1 of lane t: x [p] = sample t + 64 p in, z [q] = W1024^(t q) sum_p x [p] W16^(p q) out.  tw [q] = W [t q] (q = 1..15; tw [0] unused).
// p = a + 4 b, q = c + 4 e: 4-point DFTs over b, the twiddles W16^(a c), 4-point DFTs over a.
__host__ __device__ __forceinline__ void stage1(const float2 *x, const float2 *W, const float2 *tw, float2 *z) {
    float2 u[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        u[a][0] = x[a]; u[a][1] = x[a + 4]; u[a][2] = x[a + 8]; u[a][3] = x[a + 12];
        dft4(u[a][0], u[a][1], u[a][2], u[a][3]);          // u [a][c] = sum_b x [a + 4 b] W4^(b c)
#pragma unroll
        for (int c = 1; c < 4; c++) if (a > 0) u[a][c] = cmul(u[a][c], W[64 * a * c]);   // W16^(a c) = W1024^(64 a c)
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float2 v0 = u[0][c], v1 = u[1][c], v2 = u[2][c], v3 = u[3][c];
        dft4(v0, v1, v2, v3);                               // Y [c + 4 e] = sum_a u [a][c] W16^(a c) W4^(a e)
        z[c] = v0; z[c + 4] = v1; z[c + 8] = v2; z[c + 12] = v3;
    }
#pragma unroll
    for (int q = 1; q < PER; q++) z[q] = cmul(z[q], tw[q]);
}

// Stage 2 of lane `lane` over the LDS image zs [t * ROW + q]: the two bins it owns and their |X|.  W64^m = W [16 m].
__host__ __device__ __forceinline__ void stage2(const float2 *zs, const float2 *W, int lane, int *k_a, float2 *X_a, int *k_b, float2 *X_b) {
    const int q = lane & 15, d = stage2_d(lane);
    float2 A = make_float2(0.f, 0.f), B = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int t = 0; t < LANES; t += 2) {
        const float2 ze = zs[t * ROW + q], zo = zs[(t + 1) * ROW + q];
        const float2 we = W[16 * ((t * d) & 63)], wo = W[16 * (((t + 1) * d) & 63)];
        A = cadd(A, cmul(ze, we));
        B = cadd(B, cmul(zo, wo));
    }
    *k_a = q + 16 * d; *X_a = cadd(A, B);
    *k_b = q + 16 * ((d + 32) & 63); *X_b = csub(A, B);
}

// what one lane adds to the block's two sums
__host__ __device__ __forceinline__ void lane_sums(int k_a, float2 X_a, int k_b, float2 X_b, float *sig, float *noi) {
    const int ca = bin_class(k_a), cb = bin_class(k_b);
    const float ma = cabs(X_a), mb = cabs(X_b);
    *sig = (ca == 1 ? ma : 0.f) + (cb == 1 ? mb : 0.f);
    *noi = (ca == 2 ? ma : 0.f) + (cb == 2 ? mb : 0.f);
}

}  // namespace scan
}  // namespace fmx

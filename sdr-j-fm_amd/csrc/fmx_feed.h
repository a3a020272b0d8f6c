// fmx_feed.h -- the monitoring feed (include/fmx.h fmx_feed_*; no counterpart in the reference): 16 kS/s mono audio per channel from the
// PCM a call delivers -- the frames d_pcm holds behind both channel groups' audio kernels, the gain correction and the scan mute, where the programme audio
// meter reads them.  Everything that decides is here, as pure functions -- fmx_api.hip decides with them, fmx_feed.hip runs them, tests/feed_check.cpp
// drives them on the CPU:
//   design (): the one filter h [144], in double with fmx_design.h's bessel_i0, rounded to f32: a Kaiser (beta = 8) windowed sinc with its 6 dB point at
//     8000 Hz at 48 000 frames/s, normalised to sum 1; the same for every channel and every handle;
//   the grid: feed sample n belongs to frame 3 n; block b is the feed samples [160 b, 160 b + 160) = the frames [480 b, 480 b + 480); it reads
//     v [480 b - 143, 480 b + 480);
//   first_block (), piece (): the switch's rule and what a piece [M0, M0 + frames) of a call means for a channel switched on by the piece that began at
//     on_from: the blocks it completes, the carry it reads and the carry it leaves (fmx_sca.h's Piece, restated for frames);
//   v_of (), y_of (), power_of (), to_s16 (): the per-sample functions.  y is ONE fmaf chain in ascending tap order from an accumulator of 0.0f; no phase
//     is formed per sample and nothing is recursive, so the arithmetic at frame 2^40 is the arithmetic at frame 0.
//   THE POWER'S TREE.  p [i] = y [i] * y [i] (one rounding each), i = 0 .. 159.  q [t] = p [t] + p [t + 128] for t < 32, q [t] = p [t] for 32 <= t < 128;
//     then q [t] += q [t + s] for s = 64, 32, 16, 8, 4, 2, 1 and t < s; power = q [0] * (1.0f / 160).  power_of () is that tree on the host; the kernel
//     runs the same additions in the same order.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fmx_design.h"

namespace fmx {
namespace feed {

constexpr int NTAPS = 144;                                 // taps at 48 000 frames/s
constexpr int DECIM = 3;                                   // 48 000 -> 16 000
constexpr int RATE = 16000;
constexpr int BLOCK = 160, BLOCK_FRAMES = BLOCK * DECIM;   // 160 feed samples = 480 frames = 10 ms
constexpr int LOOKBACK = NTAPS - 1;                        // 143: a block reads v [480 b - 143, 480 b + 480)
constexpr int SPAN = LOOKBACK + BLOCK_FRAMES;              // 623 values of v per block
constexpr int CARRY_MAX = LOOKBACK + BLOCK_FRAMES - 1;     // 622 values carried at the most
constexpr int CARRY_STRIDE = 624;                          // floats per slot of the carry
constexpr int RING = 128;                                  // blocks kept per feeding channel
constexpr int NT = 192;                                    // threads of a workgroup (three waves; 160 of them hold a feed sample)
constexpr int TREE = 128;                                  // the power's tree begins with this many partial sums
constexpr double BETA = 8.0, F6_HZ = 8000.0, FRAME_RATE = 48000.0;
constexpr double DELAY_FRAMES = (NTAPS - 1) / 2.0;         // 71.5: the linear-phase delay
constexpr int MODE_OFF = 0, MODE_MIX = 1, MODE_LEFT = 2, MODE_RIGHT = 3;
// bytes of device memory per feeding channel: the ring's audio and powers, the carry
constexpr int64_t BYTES_PER_CHANNEL = (int64_t)sizeof(float) * (RING * (BLOCK + 1) + CARRY_STRIDE);      // 84 928

// ---- the design (double on the host, rounded to f32) ------------------------------------------------------------------------------------------
inline std::vector<float> design() {
    std::vector<double> h((size_t)NTAPS);
    const double mid = (NTAPS - 1) / 2.0, fc = 2.0 * F6_HZ / FRAME_RATE, i0b = design::bessel_i0(BETA);
    double sum = 0.0;
    for (int i = 0; i < NTAPS; i++) {
        const double x = i - mid, r = x / mid;
        const double w = design::bessel_i0(BETA * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        h[(size_t)i] = (x == 0.0 ? fc : std::sin(design::kPi * fc * x) / (design::kPi * x)) * w;
        sum += h[(size_t)i];
    }
    std::vector<float> out((size_t)NTAPS);
    for (int i = 0; i < NTAPS; i++) out[(size_t)i] = (float)(h[(size_t)i] / sum);
    return out;
}

// ---- the grid, the switch, a piece --------------------------------------------------------------------------------------------------------------
// the first frame block b reads
__host__ __device__ __forceinline__ int64_t block_from(int64_t b) { return (int64_t)BLOCK_FRAMES * b - LOOKBACK; }
// the first delivered block of a channel switched on by the piece that began at frame on_from: the first with 480 b - 143 >= on_from
__host__ __device__ __forceinline__ int64_t first_block(int64_t on_from) { return (on_from + LOOKBACK + BLOCK_FRAMES - 1) / BLOCK_FRAMES; }
// where the carry of a channel begins when the stream stands at frame M: what the next block to complete reads first -- the block in progress at M, or the
// channel's first block where that comes later.  The carry holds v [carry_from, M) (nothing where carry_from >= M): a pure function of M and first.
__host__ __device__ __forceinline__ int64_t carry_from(int64_t M, int64_t first) {
    const int64_t b = M / BLOCK_FRAMES;
    return block_from(b > first ? b : first);
}
struct Piece {
    int64_t b0, blocks;          // the blocks the piece completes and delivers: b0 .. b0 + blocks - 1 (blocks 0: none)
    int64_t carry_from0;         // the old carry holds v [carry_from0, M0) ...
    int32_t carry_len0;          // ... carry_len0 values (0 .. 622)
    int64_t carry_from1;         // the new carry holds v [carry_from1, M0 + frames) ...
    int32_t carry_len1;          // ... carry_len1 values (0 .. 622),
    int32_t from_carry;          // the first from_carry of them out of the old carry, from its index carry_from1 - carry_from0 on,
    int64_t row_src;             // the rest out of the piece's frames, from frame index row_src on
};
// (first: the channel's first delivered block)
__host__ __device__ inline Piece piece_first(int64_t M0, int64_t frames, int64_t first) {
    Piece p;
    const int64_t M1 = M0 + frames;
    const int64_t bn = M0 / BLOCK_FRAMES, be = M1 / BLOCK_FRAMES;    // blocks [bn, be) have their last frame in the piece
    p.b0 = bn > first ? bn : first;
    p.blocks = be > p.b0 ? be - p.b0 : 0;
    p.carry_from0 = carry_from(M0, first);
    p.carry_len0 = p.carry_from0 < M0 ? (int32_t)(M0 - p.carry_from0) : 0;
    p.carry_from1 = carry_from(M1, first);
    p.carry_len1 = p.carry_from1 < M1 ? (int32_t)(M1 - p.carry_from1) : 0;
    p.from_carry = (p.carry_len1 > 0 && p.carry_from1 < M0) ? (int32_t)(M0 - p.carry_from1) : 0;
    p.row_src = p.carry_from1 > M0 ? p.carry_from1 - M0 : 0;
    return p;
}
__host__ __device__ inline Piece piece(int64_t M0, int64_t frames, int64_t on_from) { return piece_first(M0, frames, first_block(on_from)); }
// the ring slot of block b
__host__ __device__ __forceinline__ int ring_slot(int64_t b) { return (int)(b % RING); }
// Of a piece that completes more than 128 blocks only the last 128 are formed -- the others' slots would be written over within the piece --: the first
// block formed of the blocks [M0 / 480, (M0 + frames) / 480) that have their last frame in the piece (a channel skips those in front of its own first)
__host__ __device__ __forceinline__ int64_t formed_from(int64_t M0, int64_t frames) {
    const int64_t bn = M0 / BLOCK_FRAMES, be = (M0 + frames) / BLOCK_FRAMES;
    return bn > be - RING ? bn : be - RING;
}

// ---- the per-sample functions -------------------------------------------------------------------------------------------------------------------
// v of one frame: mode 1 the mix (one rounding: the sum; the halving is exact, subnormals apart, where it rounds to even as any f32 product does),
// mode 2 the left ear, mode 3 the right
__host__ __device__ __forceinline__ float v_of(float2 x, int mode) { return mode == MODE_MIX ? 0.5f * (x.x + x.y) : (mode == MODE_LEFT ? x.x : x.y); }
// value i (0 .. 622) of block b's span, v [480 b - 143 + i], of a piece that begins at M0: out of the carry (which begins at carry_from0) or the frames
__host__ __device__ __forceinline__ float span_value(int64_t b, int i, int64_t M0, int64_t carry_from0, const float *carry, const float2 *row, int mode) {
    const int64_t m = block_from(b) + i;
    return m < M0 ? carry[m - carry_from0] : v_of(row[m - M0], mode);
}
// value i of the new carry
__host__ __device__ __forceinline__ float carry_value(const Piece &p, int i, const float *carry, const float2 *row, int mode) {
    return i < p.from_carry ? carry[(p.carry_from1 - p.carry_from0) + i] : v_of(row[p.row_src + (i - p.from_carry)], mode);
}
// feed sample n (0 .. 159) of the block: sum_k h [k] v [3 n - k], k ascending; v [3 n - k] is span [3 n + 143 - k]
__host__ __device__ __forceinline__ float y_of(int n, const float *span, const float *h) {
    // (one body for the kernel and the host form.  The taps are read four per 16-byte load: h MUST be 16-byte aligned -- in the kernel it lies in LDS and
    // every lane reads the same address, a broadcast)
    const float *x = span + DECIM * n + LOOKBACK;
    const float4 *h4 = reinterpret_cast<const float4 *>(h);
    float s = 0.0f;
#pragma unroll 4
    for (int q = 0; q < NTAPS / 4; q++) {
        const float4 t = h4[q];
        s = fmaf(t.x, x[-4 * q], s); s = fmaf(t.y, x[-4 * q - 1], s); s = fmaf(t.z, x[-4 * q - 2], s); s = fmaf(t.w, x[-4 * q - 3], s);
    }
    return s;
}
// the block's power from its 160 feed samples: the tree of this file's head
inline float power_of(const float *y) {
#pragma clang fp contract(off)
    float q[TREE];
    for (int t = 0; t < TREE; t++) {
        const float p = y[t] * y[t];
        if (t + TREE < BLOCK) { const float p2 = y[t + TREE] * y[t + TREE]; q[t] = p + p2; }
        else q[t] = p;
    }
    for (int s = TREE / 2; s > 0; s >>= 1) for (int t = 0; t < s; t++) q[t] += q[t + s];
    return q[0] * (1.0f / BLOCK);
}
// FMX_FEED_S16: (int16) min (32767, max (-32768, rintf (y * 32768.0f))), round half to even (a NaN gives 0)
__host__ __device__ __forceinline__ int16_t to_s16(float y) {
    const float r = rintf(y * 32768.0f);
    return (int16_t)(r >= 32767.0f ? 32767 : (r <= -32768.0f ? -32768 : (r == r ? (int)r : 0)));
}
// one block on the host, as fmx_feed.hip forms it: audio [160], power (h 16-byte aligned: y_of)
inline void block_host(const float *span, const float *h, float *audio, float *power) {
    for (int n = 0; n < BLOCK; n++) audio[n] = y_of(n, span, h);
    *power = power_of(audio);
}

}  // namespace feed
}  // namespace fmx

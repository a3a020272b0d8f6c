// fmx_feed.hip -- the monitoring feed (grid, piece and per-sample functions: fmx_feed.h): behind stage C, the gain correction and the scan
// mute, on the stream on which the programme audio meter reads the same frames, the feeding channels' PCM of a piece -- the carry, then the piece's frames
// -- becomes blocks of 160 mono samples at 16 kS/s and a power each.  Compiled with -ffp-contract=off: the only fused operations are the fmaf written in
// fmx_feed.h.
//
// feed_block_kernel, one workgroup of 192 threads per (job, block completed in the piece): the block's 623 values of v into LDS -- the carry's come
// first, the piece's frames follow as coalesced 8-byte loads, the mix formed on the way in --, the 144 taps into LDS; lane n < 160 runs the one fmaf
// chain over v [3 n - k] (neighbouring lanes read 3 dwords apart, which is coprime with the bank count: no conflict; the taps are a broadcast, four per
// read); the power as fmx_feed.h's fixed tree; audio and power to ring slot b mod 128.  LDS: 2496 + 576 + 128 + 512 = 3712 bytes; registers are few (one
// accumulator and a float4 of taps).  A block depends on its 623 values alone, not on where they came from.
// feed_carry_kernel, behind it: one workgroup per job moves the values the next block needs -- out of the old carry and the piece's frames -- into the
// carry, through registers, with a barrier between the reads and the writes (the two ranges overlap when a piece is short).
// feed_gather_kernel, for fmx_feed_read and fmx_feed_read_device: the listed blocks to their places in the output, as f32 or converted to 16 bit here, so
// that two bytes per sample leave the device.  No atomics, no inline assembly.
#include "fmx_internal.h"
#include "fmx_feed.h"

namespace fmx {

namespace {

__global__ __launch_bounds__(feed::NT) void feed_block_kernel(FeedArgs A) {
    __shared__ float sV[feed::CARRY_STRIDE];
    __shared__ __attribute__((aligned(16))) float sH[feed::NTAPS];
    __shared__ float sP[feed::BLOCK - feed::TREE];
    __shared__ float sQ[feed::TREE];
    const int t = threadIdx.x;
    const FeedJob job = A.jobs[blockIdx.x];                              // (jobs along x: a handle may have more than 65 535 channels)
    const int64_t b = A.b_lo + (int64_t)blockIdx.y;
    if (b < job.first) return;                                           // (the whole workgroup: in front of the channel's first delivered block)
    const int64_t cf0 = feed::carry_from(A.M0, job.first);
    const float *carry = A.carry + (size_t)job.slot * feed::CARRY_STRIDE;
    const float2 *row = A.pcm + (int64_t)job.channel * A.pcm_stride;
    for (int i = t; i < feed::SPAN; i += feed::NT) sV[i] = feed::span_value(b, i, A.M0, cf0, carry, row, job.mode);
    if (t < feed::NTAPS) sH[t] = A.h[t];
    __syncthreads();
    const size_t at = (size_t)job.slot * feed::RING + (size_t)feed::ring_slot(b);
    float p = 0.0f;
    if (t < feed::BLOCK) {
        const float y = feed::y_of(t, sV, sH);
        A.audio[at * feed::BLOCK + t] = y;
        p = y * y;
        if (t >= feed::TREE) sP[t - feed::TREE] = p;
    }
    __syncthreads();
    // (the power's tree: feed::power_of's order)
    if (t < feed::TREE) sQ[t] = t + feed::TREE < feed::BLOCK ? p + sP[t] : p;
    __syncthreads();
    for (int s = feed::TREE / 2; s > 0; s >>= 1) {
        if (t < s) sQ[t] += sQ[t + s];
        __syncthreads();
    }
    if (t == 0) A.power[at] = sQ[0] * (1.0f / feed::BLOCK);
}

__global__ __launch_bounds__(feed::NT) void feed_carry_kernel(FeedArgs A) {
    constexpr int PER = (feed::CARRY_MAX + feed::NT - 1) / feed::NT;     // 4
    const int t = threadIdx.x;
    const FeedJob job = A.jobs[blockIdx.x];
    const feed::Piece p = feed::piece_first(A.M0, A.frames, job.first);
    float *carry = A.carry + (size_t)job.slot * feed::CARRY_STRIDE;
    const float2 *row = A.pcm + (int64_t)job.channel * A.pcm_stride;
    float v[PER];
#pragma unroll
    for (int r = 0; r < PER; r++) { const int i = t + feed::NT * r; v[r] = i < p.carry_len1 ? feed::carry_value(p, i, carry, row, job.mode) : 0.f; }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PER; r++) { const int i = t + feed::NT * r; if (i < p.carry_len1) carry[i] = v[r]; }
}

// the read-out's gather: workgroup q takes ring block src [q] (slot * RING + b mod RING) to block dst [q] of the output: 160 samples in the asked format at
// out_audio, the power at out_power [dst [q]] (out_power may be null)
__global__ __launch_bounds__(feed::NT) void feed_gather_kernel(const float *__restrict__ audio, const float *__restrict__ power, const int32_t *__restrict__ src,
                                                               const int32_t *__restrict__ dst, void *__restrict__ out_audio, int format,
                                                               float *__restrict__ out_power) {
    const size_t from = (size_t)src[blockIdx.x], to = (size_t)dst[blockIdx.x];
    const int t = threadIdx.x;
    if (t < feed::BLOCK) {
        const float y = audio[from * feed::BLOCK + t];
        if (format == FMX_FEED_S16) static_cast<int16_t *>(out_audio)[to * feed::BLOCK + t] = feed::to_s16(y);
        else static_cast<float *>(out_audio)[to * feed::BLOCK + t] = y;
    } else if (t == feed::BLOCK && out_power) out_power[to] = power[from];
}

}  // namespace

void launch_feed(const FeedArgs &A, hipStream_t s) {
    if (A.n_jobs <= 0 || A.frames <= 0) return;
    if (A.nb > 0) hipLaunchKernelGGL(feed_block_kernel, dim3((unsigned)A.n_jobs, (unsigned)A.nb), dim3(feed::NT), 0, s, A);
    hipLaunchKernelGGL(feed_carry_kernel, dim3((unsigned)A.n_jobs), dim3(feed::NT), 0, s, A);
    FMX_LAUNCHED();
}

void launch_feed_gather(const float *audio, const float *power, const int32_t *src, const int32_t *dst, void *out_audio, int format, float *out_power, int n,
                        hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(feed_gather_kernel, dim3((unsigned)n), dim3(feed::NT), 0, s, audio, power, src, dst, out_audio, format, out_power);
    FMX_LAUNCHED();
}

}  // namespace fmx

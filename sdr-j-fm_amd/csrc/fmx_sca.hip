// fmx_sca.hip -- the sub-carrier decoder (grid, piece and per-sample functions: fmx_sca.h): behind stage B, on the stream on which
// stage_rds, the modulation meter and the multiplex spectrum meter read the rows, the decoding channels' demodulator output of a piece -- the carry, then
// the piece's row of w_dem -- becomes blocks of 240 audio samples at fmRate / 8 and a level each.
//
// sca_block_kernel, one workgroup of 256 threads per (job, block completed in the piece): the block's 2623 samples of d from carry and row into LDS; the
// 608 y' = sum c [k] d [4 m - k] with the channel's 192 mixed taps out of LDS, four taps per 16-byte read (the reads of neighbouring lanes are 16 bytes
// apart: no bank conflict; the taps are a broadcast); the 606 u through atan2f; the 240 s with the 128-tap audio filter; the level as a fixed tree over the
// block's 480 |y'|^2; audio and level to ring slot b mod 128.  LDS: 10 496 + 4864 + 2432 + 1536 + 512 + 1024 = 20 864 bytes, so LDS allows seven
// workgroups a CU; registers are few (two accumulators and a float4 of samples).  A block depends on its 2623 samples alone, not on where they came from.
// sca_carry_kernel, behind it: one workgroup per job moves the samples the next block needs -- out of the old carry and the row -- into the carry, through
// registers, with a barrier between the reads and the writes (the two ranges overlap when a piece is short).
// sca_gather_kernel, for fmx_sca_read: the blocks of a range of channels into one staging array.  No atomics, no inline assembly.
#include "fmx_internal.h"
#include "fmx_sca.h"

namespace fmx {

namespace {

__global__ __launch_bounds__(sca::NT) void sca_block_kernel(ScaArgs A) {
    __shared__ __attribute__((aligned(16))) float sD[sca::CARRY_STRIDE];
    __shared__ __attribute__((aligned(16))) float2 sC[sca::NG];
    __shared__ float2 sY[sca::NY];
    __shared__ float sU[sca::NY];
    __shared__ float sA[sca::NA];
    __shared__ float sQ[sca::NT];
    const int t = threadIdx.x;
    const ScaJob job = A.jobs[blockIdx.y];
    const int64_t b = A.b_lo + (int64_t)blockIdx.x;
    if (b < job.first) return;                                           // (the whole workgroup: in front of the channel's first delivered block)
    const int64_t cf0 = sca::carry_from(A.J0, job.first);
    const float *carry = A.carry + (size_t)job.slot * sca::CARRY_STRIDE;
    const float *row = A.w_dem + (size_t)job.channel * (size_t)A.lin_rows;
    const float2 *taps = A.taps + (size_t)job.slot * (sca::NG + 1);
    for (int i = t; i < sca::SPAN; i += sca::NT) sD[i] = sca::span_sample(b, i, A.J0, cf0, carry, row);
    if (t < sca::NG) sC[t] = taps[t];
    if (t < sca::NA) sA[t] = A.a[t];
    const float2 rot = taps[sca::NG];
    __syncthreads();
    for (int i = t; i < sca::NY; i += sca::NT) sY[i] = sca::y_of(i, sD, sC);
    __syncthreads();
    for (int i = t; i < sca::NU; i += sca::NT) sU[i] = sca::u_of(sY[i + 1], sY[i], rot, A.scale);
    // (the level's tree: sca::level_of's order)
    float q = sca::power_of(sY[sca::NA + t]);
    if (t + sca::NT < sca::BLOCK_Y) q += sca::power_of(sY[sca::NA + t + sca::NT]);
    sQ[t] = q;
    __syncthreads();
    const size_t at = (size_t)job.slot * sca::RING + (size_t)(b % sca::RING);
    if (t < sca::BLOCK_AUDIO) A.audio[at * sca::BLOCK_AUDIO + t] = sca::s_of(t, sU, sA);
    for (int h = sca::NT / 2; h > 0; h >>= 1) {
        if (t < h) sQ[t] += sQ[t + h];
        __syncthreads();
    }
    if (t == 0) A.level[at] = sQ[0] * (1.0f / sca::BLOCK_Y);
}

__global__ __launch_bounds__(sca::NT) void sca_carry_kernel(ScaArgs A) {
    constexpr int PER = (sca::CARRY_MAX + sca::NT - 1) / sca::NT;        // 11
    const int t = threadIdx.x;
    const ScaJob job = A.jobs[blockIdx.x];
    const sca::Piece p = sca::piece_first(A.J0, A.nj, job.first);
    float *carry = A.carry + (size_t)job.slot * sca::CARRY_STRIDE;
    const float *row = A.w_dem + (size_t)job.channel * (size_t)A.lin_rows;
    float v[PER];
#pragma unroll
    for (int r = 0; r < PER; r++) { const int i = t + sca::NT * r; v[r] = i < p.carry_len1 ? sca::carry_sample(p, i, carry, row) : 0.f; }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PER; r++) { const int i = t + sca::NT * r; if (i < p.carry_len1) carry[i] = v[r]; }
}

// the read-out's gather: workgroup q copies block src [q] (slot * RING + b mod RING) to out [q]: 240 audio samples, then the level
__global__ __launch_bounds__(sca::NT) void sca_gather_kernel(const float *__restrict__ audio, const float *__restrict__ level, const int32_t *__restrict__ src,
                                                             float *__restrict__ out) {
    const size_t from = (size_t)src[blockIdx.x];
    float *to = out + (size_t)blockIdx.x * (sca::BLOCK_AUDIO + 1);
    const int t = threadIdx.x;
    if (t < sca::BLOCK_AUDIO) to[t] = audio[from * sca::BLOCK_AUDIO + t];
    else if (t == sca::BLOCK_AUDIO) to[t] = level[from];
}

}  // namespace

void launch_sca(const ScaArgs &A, hipStream_t s) {
    if (A.n_jobs <= 0) return;
    if (A.nb > 0) hipLaunchKernelGGL(sca_block_kernel, dim3((unsigned)A.nb, (unsigned)A.n_jobs), dim3(sca::NT), 0, s, A);
    hipLaunchKernelGGL(sca_carry_kernel, dim3((unsigned)A.n_jobs), dim3(sca::NT), 0, s, A);
    FMX_LAUNCHED();
}

void launch_sca_gather(const float *audio, const float *level, const int32_t *src, float *out, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(sca_gather_kernel, dim3((unsigned)n), dim3(sca::NT), 0, s, audio, level, src, out);
    FMX_LAUNCHED();
}

}  // namespace fmx

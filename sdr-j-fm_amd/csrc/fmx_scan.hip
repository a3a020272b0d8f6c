// fmx_scan.hip -- scan mode (fm-processor.cpp:478-495): the fm-rate samples of the scanning channels, behind their carry, cut into blocks of
// 1024; every complete block through the pruned 1024-point transform of fmx_scan.h and into the channel's record ring as (signal_db,
// noise_db); the samples left over become the new carry.  And the mute of the scanning channels' PCM behind stage C.
//
// One workgroup per scanning channel, four waves, one block per wave at a time.  A channel's samples of the call are read from stage A's
// fm-rate ring as every reader of it does: fm sample j at ring position j - delay_fm, zero while j < delay_fm (fmx_readout.hip fmx_get_tap).
// The carry is read by the wave of block 0 only and rewritten behind a barrier.
#include "fmx_internal.h"
#include "fmx_scan.h"
#include <algorithm>

namespace fmx {

namespace {

__global__ __launch_bounds__(256) void scan_kernel(ScanArgs A) {
    __shared__ float2 sW[scan::N];
    __shared__ float2 sZ[4][scan::LDS_N];
    const ScanJob job = A.jobs[blockIdx.x];
    const int ch = job.ch, fill = job.fill;
    const int64_t nj = A.J1 - A.J0, total = (int64_t)fill + nj;
    const int64_t nblk = total / scan::N;
    const int delay = A.front_sets[A.params[ch].front_set].delay_fm;
    const float2 *__restrict__ zr = A.zring + (size_t)ch * (size_t)(A.ring_mask + 1);
    float2 *__restrict__ carry = A.carry + (size_t)ch * scan::N;
    for (int i = threadIdx.x; i < scan::N; i += 256) sW[i] = A.W[i];
    // sample i of the channel's scan stream in this call: the carry, then fm samples J0, J0 + 1, ...
    auto sample = [&](int64_t i) -> float2 {
        if (i < fill) return carry[i];
        const int64_t jv = A.J0 + (i - fill) - delay;
        return jv < 0 ? make_float2(0.f, 0.f) : zr[jv & A.ring_mask];
    };
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float2 tw[scan::PER];
#pragma unroll
    for (int q = 1; q < scan::PER; q++) tw[q] = sW[lane * q];
    tw[0] = make_float2(1.f, 0.f);
    const int64_t rounds = (nblk + 3) / 4;
    for (int64_t it = 0; it < rounds; it++) {
        const int64_t b = it * 4 + w;
        const bool active = b < nblk;
        if (active) {
            float2 x[scan::PER], z[scan::PER];
#pragma unroll
            for (int p = 0; p < scan::PER; p++) x[p] = sample(b * scan::N + lane + 64 * p);
            scan::stage1(x, sW, tw, z);
#pragma unroll
            for (int q = 0; q < scan::PER; q++) sZ[w][lane * scan::ROW + q] = z[q];
        }
        __syncthreads();
        if (active) {
            int ka, kb; float2 Xa, Xb; float sig, noi;
            scan::stage2(sZ[w], sW, lane, &ka, &Xa, &kb, &Xb);
            scan::lane_sums(ka, Xa, kb, Xb, &sig, &noi);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) { sig += __shfl_xor(sig, m, 64); noi += __shfl_xor(noi, m, 64); }
            // (a call of more than RING blocks keeps its last RING: no two waves write one slot)
            if (lane == 0 && b >= nblk - scan::RING)
                A.rec[(size_t)ch * scan::RING + (size_t)((job.slot0 + b) & (scan::RING - 1))] = make_float2(scan::get_db(sig), scan::get_db(noi));
        }
        __syncthreads();
    }
    // the new carry: the samples behind the last complete block (with no complete block: the call's samples behind the old carry)
    const int64_t base = nblk * scan::N;
    const int64_t from = nblk > 0 ? base : (int64_t)fill;
    for (int64_t i = from + threadIdx.x; i < total; i += 256) carry[i - base] = sample(i);
}

__global__ __launch_bounds__(256) void scan_mute_kernel(const int32_t *__restrict__ chans, float2 *__restrict__ pcm, int64_t pcm_stride, int64_t frames) {
    float2 *out = pcm + (size_t)chans[blockIdx.y] * (size_t)pcm_stride;
    for (int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x; f < frames; f += (int64_t)gridDim.x * 256) out[f] = make_float2(0.f, 0.f);
}

}  // namespace

void launch_scan(const ScanArgs &A, int n_jobs, hipStream_t s) {
    if (n_jobs <= 0 || A.J1 <= A.J0) return;
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)n_jobs), dim3(256), 0, s, A);
}

void launch_scan_mute(const int32_t *chans, int n, float2 *pcm, int64_t pcm_stride, int64_t frames, hipStream_t s) {
    if (n <= 0 || frames <= 0) return;
    const dim3 grid((unsigned)std::min<int64_t>((frames + 255) / 256, 64), (unsigned)n);
    hipLaunchKernelGGL(scan_mute_kernel, grid, dim3(256), 0, s, chans, pcm, pcm_stride, frames);
}

}  // namespace fmx

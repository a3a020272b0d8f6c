// fmx_rdsm.hip -- the RDS meter: per channel and window of 2560 RDS samples the maximum of the power |z|^2 of the 24 kS/s baseband behind
// the RDS path's decimator, and the sums of I I, Q Q, I Q, I and Q -- injection level, phase against the pilot's third harmonic and the cleanness of the
// sub-carrier in front of every slicer.
//
// One wave per metered channel of a piece, from a job table (fmx_rdsm.h piece); the grid is the channel's own RDS-sample count.  Sample i of a window belongs
// to lane i mod 64, as its step i div 64: a step of the wave is one coalesced read of 64 consecutive entries (512 bytes) of the channel's rds24 ring, RDS sample
// m at position m & 8191.  The kernel reads [first, m1) only, samples the piece's own rds_mix_decim wrote in front of it on the same stream.  Whole steps go
// UNROLL at a time, their loads first; a step the piece covers in part goes alone.  Every lane accumulates in step order in f32, without contraction (this
// file is compiled with -ffp-contract=off); what a channel carries from piece to piece is its lanes' six accumulators and no sample.  At a window's end the
// lanes are combined by the butterfly a [l] = a [l] op a [l xor k], k = 32 .. 1, and lane 0 writes the record.  A plain streaming read: no LDS, no atomics.
#include "fmx_internal.h"
#include "fmx_rdsm.h"
#include <cmath>

namespace fmx {

static_assert(rdsm::RING24 == RDS24_RING, "fmx_rdsm.h restates the size of the path's 24 kS/s ring");

namespace {

constexpr int WAVES = 4;               // jobs per workgroup (the waves share nothing)
constexpr int UNROLL = 8;              // whole steps whose loads are in flight together (40 steps a window: 5 rounds)

__global__ __launch_bounds__(64 * WAVES) void rdsm_kernel(RdsmArgs A, int n_jobs) {
    const int jb = (int)blockIdx.x * WAVES + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (jb >= n_jobs) return;
    const RdsmJob job = A.jobs[jb];
    const int64_t end = job.m1;
    int64_t j = job.first;
    if (j < 0 || j >= end || end - j > rdsm::RING24 || job.ch < 0 || job.ch >= A.channels) return;
    const float2 *__restrict__ zr = A.rds24 + (size_t)job.ch * rdsm::RING24;
    float *__restrict__ st = A.state + (size_t)job.ch * (rdsm::QUANT * rdsm::LANES) + lane;
    int64_t w = rdsm::window_of(j);
    float mx = -INFINITY, sii = 0.f, sqq = 0.f, siq = 0.f, si = 0.f, sq = 0.f;
    if (j != w * rdsm::WINDOW) {      // the window is in progress: its accumulators as the last piece left them
        mx = st[rdsm::Q_MX * rdsm::LANES]; sii = st[rdsm::Q_II * rdsm::LANES]; sqq = st[rdsm::Q_QQ * rdsm::LANES];
        siq = st[rdsm::Q_IQ * rdsm::LANES]; si = st[rdsm::Q_I * rdsm::LANES]; sq = st[rdsm::Q_Q * rdsm::LANES];
    }
    int k = 0;
    while (j < end) {
        const int64_t wbase = w * rdsm::WINDOW, wnext = wbase + rdsm::WINDOW;
        const int64_t stop = end < wnext ? end : wnext;
        const int i_lo = (int)(j - wbase), i_hi = (int)(stop - wbase);      // (the window's samples of this piece: RDS samples wbase + i_lo .. wbase + i_hi - 1)
        // one sample of a lane: every product and every sum rounded once
        auto accumulate = [&](const float2 z) {
            const float ii = z.x * z.x, qq = z.y * z.y;
            const float p = ii + qq;
            mx = fmaxf(mx, p);
            sii += ii; sqq += qq;
            const float iq = z.x * z.y; siq += iq;
            si += z.x; sq += z.y;
        };
        const int q_end = rdsm::step_of(i_hi - 1);
        int q = rdsm::step_of(i_lo);
        while (q <= q_end) {
            if (q * rdsm::LANES >= i_lo && (q + UNROLL) * rdsm::LANES <= i_hi) {
                float2 z[UNROLL];
#pragma unroll
                for (int t = 0; t < UNROLL; t++) z[t] = zr[(wbase + (q + t) * rdsm::LANES + lane) & (int64_t)(rdsm::RING24 - 1)];
#pragma unroll
                for (int t = 0; t < UNROLL; t++) accumulate(z[t]);
                q += UNROLL;
                continue;
            }
            const int i = q * rdsm::LANES + lane;
            if (i >= i_lo && i < i_hi) accumulate(zr[(wbase + i) & (int64_t)(rdsm::RING24 - 1)]);
            q++;
        }
        if (stop == wnext) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, m, 64));
                sii += __shfl_xor(sii, m, 64); sqq += __shfl_xor(sqq, m, 64); siq += __shfl_xor(siq, m, 64);
                si += __shfl_xor(si, m, 64); sq += __shfl_xor(sq, m, 64);
            }
            if (lane == 0) {
                fmx_rds_meter_record r;
                r.index = w; r.end_sample = wnext;
                r.p_max = mx; r.ii_mean = rdsm::finish_mean(sii); r.qq_mean = rdsm::finish_mean(sqq); r.iq_mean = rdsm::finish_mean(siq);
                r.i_mean = rdsm::finish_mean(si); r.q_mean = rdsm::finish_mean(sq);
                A.ring[(size_t)job.ch * rdsm::RING + (size_t)((job.slot0 + k) & (rdsm::RING - 1))] = r;
            }
            k++;
            mx = -INFINITY; sii = sqq = siq = si = sq = 0.f;
        }
        j = stop; w++;
    }
    st[rdsm::Q_MX * rdsm::LANES] = mx; st[rdsm::Q_II * rdsm::LANES] = sii; st[rdsm::Q_QQ * rdsm::LANES] = sqq;
    st[rdsm::Q_IQ * rdsm::LANES] = siq; st[rdsm::Q_I * rdsm::LANES] = si; st[rdsm::Q_Q * rdsm::LANES] = sq;
}

}  // namespace

void launch_rdsm(const RdsmArgs &A, int n_jobs, hipStream_t s) {
    if (n_jobs <= 0) return;
    hipLaunchKernelGGL(rdsm_kernel, dim3((unsigned)((n_jobs + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, s, A, n_jobs);
}

}  // namespace fmx

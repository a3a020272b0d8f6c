// fmx_meter.hip -- the modulation meter: per channel and 50 ms window the demodulator output's maximum, minimum, sum and sum of squares,
// and its two sums against the sine and the cosine of the pilot phase -- peak deviation, multiplex power and pilot deviation in the demodulator's units.
//
// One wave per metered channel of a piece, from a job table (fmx_meter.h meter_produce).  Sample i of a window belongs to lane i mod 64, as its step
// i div 64: a step of the wave reads 64 consecutive floats of the channel's row of w_dem and of w_cur, the rows stage B leaves behind and the RDS path reads.
// Every lane accumulates in step order in f32, without contraction (this file is compiled with -ffp-contract=off); what a channel carries from piece to piece
// is its lanes' six accumulators, so a record does not depend on how the stream is cut.  At a window's end the lanes are combined by the butterfly
// a [l] = a [l] op a [l xor m], m = 32 .. 1, and lane 0 writes the record.
#include "fmx_internal.h"
#include "fmx_meter.h"
#include <cmath>

namespace fmx {

namespace {

constexpr int WAVES = 4;               // jobs per workgroup (the waves share nothing)

__global__ __launch_bounds__(64 * WAVES) void meter_kernel(MeterArgs A, int n_jobs) {
    const int jb = (int)blockIdx.x * WAVES + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (jb >= n_jobs) return;
    const MeterJob job = A.jobs[jb];
    const int64_t end = A.J1;
    int64_t j = A.J0 + job.r0;
    if (job.r0 < 0 || j >= end) return;
    const float *__restrict__ dem = A.w_dem + (size_t)job.ch * (size_t)A.lin_rows;
    const float *__restrict__ cur = A.w_cur + (size_t)job.ch * (size_t)A.lin_rows;
    float *__restrict__ st = A.state + (size_t)job.ch * (meter::QUANT * meter::LANES) + lane;
    int64_t w = meter::window_of(j);
    float mx = -INFINITY, mn = INFINITY, s1 = 0.f, s2 = 0.f, si = 0.f, sq = 0.f;
    if (j != w * meter::WINDOW) {      // the window is in progress: its accumulators as the last piece left them
        mx = st[meter::Q_MX * meter::LANES]; mn = st[meter::Q_MN * meter::LANES]; s1 = st[meter::Q_S1 * meter::LANES];
        s2 = st[meter::Q_S2 * meter::LANES]; si = st[meter::Q_SI * meter::LANES]; sq = st[meter::Q_SQ * meter::LANES];
    }
    int k = 0;
    while (j < end) {
        const int64_t wbase = w * meter::WINDOW, wnext = wbase + meter::WINDOW;
        const int64_t stop = end < wnext ? end : wnext;
        const int i_lo = (int)(j - wbase), i_hi = (int)(stop - wbase);
        const int64_t rbase = wbase - A.J0;      // (the row of the window's sample 0: rows rbase + i_lo .. rbase + i_hi - 1 lie in [r0, J1 - J0))
        for (int q = meter::step_of(i_lo); q <= meter::step_of(i_hi - 1); q++) {
            const int i = q * meter::LANES + lane;
            if (i >= i_lo && i < i_hi) {
                const float d = dem[rbase + i], phi = cur[rbase + i];
                float S, C;
                sincosf(phi, &S, &C);
                mx = fmaxf(mx, d); mn = fminf(mn, d);
                s1 += d;
                const float dd = d * d; s2 += dd;
                const float ds = d * S; si += ds;
                const float dc = d * C; sq += dc;
            }
        }
        if (stop == wnext) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, m, 64)); mn = fminf(mn, __shfl_xor(mn, m, 64));
                s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64); si += __shfl_xor(si, m, 64); sq += __shfl_xor(sq, m, 64);
            }
            if (lane == 0) {
                fmx_mod_record r;
                r.index = w; r.end_sample = wnext;
                r.peak_pos = mx; r.peak_neg = mn; r.mean = meter::finish_mean(s1); r.mean_square = meter::finish_mean(s2);
                r.pilot_i = meter::finish_pilot(si); r.pilot_q = meter::finish_pilot(sq);
                A.ring[(size_t)job.ch * meter::RING + (size_t)((job.slot0 + k) & (meter::RING - 1))] = r;
            }
            k++;
            mx = -INFINITY; mn = INFINITY; s1 = s2 = si = sq = 0.f;
        }
        j = stop; w++;
    }
    st[meter::Q_MX * meter::LANES] = mx; st[meter::Q_MN * meter::LANES] = mn; st[meter::Q_S1 * meter::LANES] = s1;
    st[meter::Q_S2 * meter::LANES] = s2; st[meter::Q_SI * meter::LANES] = si; st[meter::Q_SQ * meter::LANES] = sq;
}

}  // namespace

void launch_meter(const MeterArgs &A, int n_jobs, hipStream_t s) {
    if (n_jobs <= 0 || A.J1 <= A.J0) return;
    hipLaunchKernelGGL(meter_kernel, dim3((unsigned)((n_jobs + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, s, A, n_jobs);
}

}  // namespace fmx

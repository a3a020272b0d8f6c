// fmx_rx.hip -- the reception meter: per channel and 50 ms window the maximum, the minimum, the sum and the sum of squares of the power
// |v|^2 of stage A's fm-rate samples, and the sum of v conj (u), u the sample before v -- level, carrier-to-noise, envelope depth and frequency offset of
// the signal in front of the limiter.
//
// One wave per metered channel of a piece, from a job table (fmx_meter.h meter_produce); the grid is the modulation meter's.  Sample i of a window belongs
// to lane i mod 64, as its step i div 64: a step of the wave reads 64 consecutive entries of the channel's ring as every reader of it does -- fm sample j
// at ring position j - delay_fm, zero while j < delay_fm -- and the one before them: lane 0 loads its predecessor, every other lane takes it from its
// neighbour.  Whole steps go UNROLL at a time, their loads first; a step the piece covers in part goes alone.  Every lane accumulates in step order in f32, without contraction (this file is compiled with -ffp-contract=off); what a channel carries
// from piece to piece is its lanes' six accumulators and no sample.  At a window's end the lanes are combined by the butterfly
// a [l] = a [l] op a [l xor m], m = 32 .. 1, and lane 0 writes the record.  A plain streaming read: no LDS, no atomics.
#include "fmx_internal.h"
#include "fmx_rx.h"
#include <cmath>

namespace fmx {

namespace {

constexpr int WAVES = 4;               // jobs per workgroup (the waves share nothing)
constexpr int UNROLL = 6;              // whole steps whose loads are in flight together (150 steps a window: 25 rounds)

__global__ __launch_bounds__(64 * WAVES) void rx_kernel(RxArgs A, int n_jobs) {
    const int jb = (int)blockIdx.x * WAVES + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (jb >= n_jobs) return;
    const RxJob job = A.jobs[jb];
    const int64_t end = A.J1;
    int64_t j = A.J0 + job.r0;
    if (job.r0 < 0 || j >= end) return;
    const int64_t delay = A.front_sets[A.params[job.ch].front_set].delay_fm;
    const float2 *__restrict__ zr = A.zring + (size_t)job.ch * (size_t)(A.ring_mask + 1);
    float *__restrict__ st = A.state + (size_t)job.ch * (rx::QUANT * meter::LANES) + lane;
    // fm sample jj as the ring holds it
    auto sample = [&](int64_t jj) -> float2 {
        const int64_t jv = jj - delay;
        return jv < 0 ? make_float2(0.f, 0.f) : zr[jv & (int64_t)A.ring_mask];
    };
    int64_t w = meter::window_of(j);
    float mx = -INFINITY, mn = INFINITY, s1 = 0.f, s2 = 0.f, cr = 0.f, ci = 0.f;
    if (j != w * meter::WINDOW) {      // the window is in progress: its accumulators as the last piece left them
        mx = st[rx::Q_MX * meter::LANES]; mn = st[rx::Q_MN * meter::LANES]; s1 = st[rx::Q_S1 * meter::LANES];
        s2 = st[rx::Q_S2 * meter::LANES]; cr = st[rx::Q_CR * meter::LANES]; ci = st[rx::Q_CI * meter::LANES];
    }
    int k = 0;
    while (j < end) {
        const int64_t wbase = w * meter::WINDOW, wnext = wbase + meter::WINDOW;
        const int64_t stop = end < wnext ? end : wnext;
        const int i_lo = (int)(j - wbase), i_hi = (int)(stop - wbase);      // (the window's samples of this piece: fm samples wbase + i_lo .. wbase + i_hi - 1)
        // one sample of a lane: every product and every sum rounded once
        auto accumulate = [&](const float2 v, const float2 u) {
            const float rr = v.x * v.x, ii = v.y * v.y;
            const float p = rr + ii;
            mx = fmaxf(mx, p); mn = fminf(mn, p);
            s1 += p;
            const float pp = p * p; s2 += pp;
            const float a = v.x * u.x, b = v.y * u.y; const float re = a + b; cr += re;
            const float c = v.y * u.x, d = v.x * u.y; const float im = c - d; ci += im;
        };
        const int q_end = meter::step_of(i_hi - 1);
        int q = meter::step_of(i_lo);
        while (q <= q_end) {
            if (q * meter::LANES >= i_lo && (q + UNROLL) * meter::LANES <= i_hi) {
                // UNROLL whole steps: their loads first, then the steps in order.  Lane 0's predecessor is loaded for the first of them and is the last
                // lane's sample of the step before for the others.
                float2 v[UNROLL];
#pragma unroll
                for (int t = 0; t < UNROLL; t++) v[t] = sample(wbase + (q + t) * meter::LANES + lane);
                float2 u0 = make_float2(0.f, 0.f);
                if (lane == 0) u0 = sample(wbase + q * meter::LANES - 1);
#pragma unroll
                for (int t = 0; t < UNROLL; t++) {
                    float2 u;
                    u.x = __shfl_up(v[t].x, 1, 64); u.y = __shfl_up(v[t].y, 1, 64);
                    if (t > 0) { u0.x = __shfl(v[t - 1].x, 63, 64); u0.y = __shfl(v[t - 1].y, 63, 64); }
                    if (lane == 0) u = u0;
                    accumulate(v[t], u);
                }
                q += UNROLL;
                continue;
            }
            const int i = q * meter::LANES + lane;
            const bool mine = i >= i_lo && i < i_hi;
            // (the sample in front of the piece's first is read too: it is its neighbour's u.  Nothing behind the piece's last sample is.)
            float2 v = make_float2(0.f, 0.f), u0 = v;
            if (i >= i_lo - 1 && i < i_hi) v = sample(wbase + i);
            if (lane == 0 && mine) u0 = sample(wbase + i - 1);
            float2 u;
            u.x = __shfl_up(v.x, 1, 64); u.y = __shfl_up(v.y, 1, 64);
            if (lane == 0) u = u0;
            if (mine) accumulate(v, u);
            q++;
        }
        if (stop == wnext) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, m, 64)); mn = fminf(mn, __shfl_xor(mn, m, 64));
                s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64); cr += __shfl_xor(cr, m, 64); ci += __shfl_xor(ci, m, 64);
            }
            if (lane == 0) {
                fmx_rx_record r;
                r.index = w; r.end_sample = wnext;
                r.p_max = mx; r.p_min = mn; r.p_mean = meter::finish_mean(s1); r.p2_mean = meter::finish_mean(s2);
                r.r1_re = meter::finish_mean(cr); r.r1_im = meter::finish_mean(ci);
                A.ring[(size_t)job.ch * rx::RING + (size_t)((job.slot0 + k) & (rx::RING - 1))] = r;
            }
            k++;
            mx = -INFINITY; mn = INFINITY; s1 = s2 = cr = ci = 0.f;
        }
        j = stop; w++;
    }
    st[rx::Q_MX * meter::LANES] = mx; st[rx::Q_MN * meter::LANES] = mn; st[rx::Q_S1 * meter::LANES] = s1;
    st[rx::Q_S2 * meter::LANES] = s2; st[rx::Q_CR * meter::LANES] = cr; st[rx::Q_CI * meter::LANES] = ci;
}

}  // namespace

void launch_rx(const RxArgs &A, int n_jobs, hipStream_t s) {
    if (n_jobs <= 0 || A.J1 <= A.J0) return;
    hipLaunchKernelGGL(rx_kernel, dim3((unsigned)((n_jobs + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, s, A, n_jobs);
}

}  // namespace fmx

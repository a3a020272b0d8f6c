// fmx_wide_rate.hip -- stage W at any receiver rate (no counterpart in the reference, whose Airspy handler interpolates 2.5 MS/s
// linearly on the host): one stream at Rw S/s feeds many outputs at Ro = 2 304 000 S/s, Rw / Ro = M / L in lowest terms.  Output j of a stream,
//     q_j = (j + 1) M - 1,  n_j = q_j div L,  p_j = q_j mod L,      y [j] = sum_i H [p_j + L i] x [n_j - i] O (P [n_j - i]),  i < NP = ceil (N_H / L),
// H the N_H = 16 M + 1 tap prototype at the rate M Ro, P [n] = (P [n - 1] - f) mod Rw the oscillator's integer phase (fmx_wide_rate.h: the integers).
//
// One workgroup per (stream, tile of 256 outputs): the tile's samples -- at most floor (255 M / L) + 2 -- and the NP - 1 in front of them are read
// from HBM once, converted to f32 and kept in LDS in sample order (neighbouring lanes, whose newest samples lie M / L = 1.04 ... 15.6 apart,
// read elements that far apart; each lane walks its own window backwards.  The bank pattern: DESIGN.md 4.10).  Thread c computes output c of
// the tile for every output of the stream, four at a time.  With a constant offset
// O (P [n_j - i]) = O (P [n_j]) O (i f), but the tap now depends on the lane: the real row H [p_j + L i] comes from a [L][NP] table in global memory
// (each lane reads its own row in order), the stations' rotators O (i f) through the scalar cache, and the product H x is formed once for the four
// stations of a group.  The sum runs in tap order, two accumulators per output, whatever the tile, the call or the position in it; the output's
// rotator O (P [n_j]) is evaluated in f64 per output (a table of Rw entries would be up to 295 MB).
//
// Behind fmx_wideband_set_offset the outputs of the call's head whose windows reach back across a change are recomputed sample by sample, each
// sample with the phase of its own run: stage W's wide_slow with n_j, p_j.
#include "fmx_internal.h"
#include "fmx_wide_rate.h"
#include "../../include/fmx.h"

namespace fmx {

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int WR_NT = wrate::TILE;                // threads: one per output of the tile
constexpr int WR_SB = 4;                          // outputs of a stream computed together

__device__ __forceinline__ float2 wr_load(const void *src, int fmt, float qs, int64_t at) {
    switch (fmt) {
    case FMX_IQ_U8: { const uchar2 v = reinterpret_cast<const uchar2 *>(src)[at]; return make_float2((float)((int)v.x - 127) * qs, (float)((int)v.y - 127) * qs); }
    case FMX_IQ_S8: { const char2 v = reinterpret_cast<const char2 *>(src)[at]; return make_float2((float)v.x * qs, (float)v.y * qs); }
    case FMX_IQ_S16: { const short2 v = reinterpret_cast<const short2 *>(src)[at]; return make_float2((float)v.x * qs, (float)v.y * qs); }
    default: return reinterpret_cast<const float2 *>(src)[at];
    }
}

// O (P [n]) of a run: P [n] = (pbase - (n - nbase + 1) f) mod Rw, (cos, sin) in f64 rounded to f32
__device__ __forceinline__ float2 wr_osc(const WideSeg &g, int64_t n, int32_t Rw) {
    int64_t q = (n - g.nbase + 1) % Rw; if (q < 0) q += Rw;
    int64_t p = ((int64_t)g.pbase - q * (int64_t)g.f) % Rw; if (p < 0) p += Rw;
    double sn, cs;
    sincos(2.0 * 3.14159265358979323846 * (double)p / (double)Rw, &sn, &cs);
    return make_float2((float)cs, (float)sn);
}

// An output of the call's head whose window crosses an offset change: every sample with the phase it was mixed with.
__device__ __noinline__ float2 wr_slow(const WideOut &o, const float *__restrict__ hp, const float2 *X, int a0, int64_t nj, int NP, int32_t Rw) {
    float ar = 0.f, ai = 0.f;
    int k = 0;
    for (int i = 0; i < NP; i++) {
        const int64_t n = nj - i;                                        // (n < 0: the zeros in front of the stream)
        while (k + 1 < o.nseg && n < o.seg[k].nbase) k++;                // (n falls: the runs are met newest first)
        const float2 O = wr_osc(o.seg[k], n, Rw);
        const float2 x = X[a0 - i];
        const float vr = x.x * O.x - x.y * O.y, vi = x.x * O.y + x.y * O.x;
        ar = fmaf(hp[i], vr, ar); ai = fmaf(hp[i], vi, ai);
    }
    return make_float2(ar, ai);
}

// (rot / phases / dst: WideRateArgs' pointers once more, as parameters the compiler knows not to alias)
__global__ __launch_bounds__(WR_NT) void wide_rate_kernel(WideRateArgs A, const float2 *__restrict__ rot, const float *__restrict__ phases,
                                                          float2 *__restrict__ dst) {
    __shared__ __attribute__((aligned(16))) float2 X[wrate::LDS_SAMPLES];
    __shared__ int sOut[WR_NT], sSlow[WR_NT];
    const int t = threadIdx.x, tile = blockIdx.x, stream = blockIdx.y;
    const int64_t L = A.L, M = A.M;
    const int NP = A.NP, HN = A.NP - 1;
    const int64_t jc0 = (int64_t)tile * wrate::TILE;                     // the tile's first output of the call
    const int n_tile = (int)(A.n_out - jc0 < wrate::TILE ? A.n_out - jc0 : wrate::TILE);
    const int64_t jt = A.j0 + jc0;                                       // ... counted from the stream's beginning
    int64_t n_first, n_last; int32_t pj;
    wrate::sample_of(jt, L, M, &n_first, &pj);
    wrate::sample_of(jt + n_tile - 1, L, M, &n_last, &pj);
    const int64_t s_lo = n_first - HN;                                   // the sample at image index 0
    const int nsamp = (int)(n_last - s_lo) + 1;                          // <= wrate::max_samples () <= wrate::LDS_SAMPLES
    const int64_t rel0 = s_lo - A.g0;                                    // ... relative to the call's first sample (>= -HN)

    // 1. the tile's samples and the NP - 1 in front of them, converted once
    const float2 *hin = A.hist_in + (size_t)stream * wrate::HIST;
    const int64_t sbase = (int64_t)stream * A.src_stride;
    for (int a = t; a < nsamp; a += WR_NT) {
        const int64_t s = rel0 + a;
        X[a] = s >= 0 ? wr_load(A.src, A.fmt, A.qs, sbase + s) : hin[HN + s];
    }
    // ... and what the next call finds in front of its first sample: the stream's last NP - 1 samples (behind the last output's newest sample
    // there may be some that no tile holds, so they are converted here once more: at most 255 per call)
    if (jc0 + n_tile == A.n_out) {
        float2 *hout = A.hist_out + (size_t)stream * wrate::HIST;
        for (int k = t; k < HN; k += WR_NT) {
            const int64_t s = A.n_wide - HN + k;
            hout[k] = s >= 0 ? wr_load(A.src, A.fmt, A.qs, sbase + s) : hin[HN + s];
        }
    }
    __syncthreads();

    // this thread's output (a ragged tile's spare threads repeat its last one and store nothing)
    int64_t nj;
    wrate::sample_of(jt + (t < n_tile ? t : n_tile - 1), L, M, &nj, &pj);
    const int a0 = (int)(nj - s_lo);                                     // its newest sample in the image, >= NP - 1
    const float *__restrict__ hp = phases + (size_t)pj * NP;

    const int st0 = A.first[stream], nst = A.first[stream + 1] - st0;
    for (int base = 0; base < nst; base += WR_NT) {
        const int cnt = nst - base < WR_NT ? nst - base : WR_NT;
        // 2. per output of the stream (one thread each): how many of the call's first outputs have a window that crosses an offset change
        __syncthreads();
        if (t < cnt) {
            const int m = A.list[st0 + base + t];
            int slow = 0;
            if (tile == 0 && A.outs[m].nseg > 1) slow = (int)wrate::crossing(A.j0, A.n_out, A.outs[m].seg[0].nbase, NP, L, M);
            sOut[t] = m; sSlow[t] = slow;
        }
        __syncthreads();
        // 3. the folded filter, WR_SB outputs of the stream at a time
        for (int sb = 0; sb < cnt; sb += WR_SB) {
            const float2 *g[WR_SB];
            int mm[WR_SB];
#pragma unroll
            for (int k = 0; k < WR_SB; k++) {
                const int at = sb + k < cnt ? sb + k : cnt - 1;          // (a short last group repeats its last output; only sb + k < cnt is stored)
                mm[k] = __builtin_amdgcn_readfirstlane(sOut[at]);
                g[k] = rot + (size_t)mm[k] * NP;
            }
            v2f a[WR_SB], b[WR_SB];
#pragma unroll
            for (int k = 0; k < WR_SB; k++) { a[k] = (v2f){0.f, 0.f}; b[k] = (v2f){0.f, 0.f}; }
#pragma unroll 4
            for (int i = 0; i < NP; i++) {
                const float h = hp[i];
                const float2 x = X[a0 - i];
                const v2f xa = (v2f){h * x.x, h * x.y}, xb = (v2f){xa.y, xa.x};
#pragma unroll
                for (int k = 0; k < WR_SB; k++) {
                    const float2 gk = g[k][i];
                    a[k] = __builtin_elementwise_fma((v2f){gk.x, gk.x}, xa, a[k]);
                    b[k] = __builtin_elementwise_fma((v2f){-gk.y, gk.y}, xb, b[k]);
                }
            }
            // 4. the output's rotator O (P [n_j]) and the store
#pragma unroll
            for (int k = 0; k < WR_SB; k++) {
                if (sb + k < cnt && t < n_tile) {
                    const v2f sum = a[k] + b[k];
                    const float2 o = wr_osc(A.outs[mm[k]].seg[0], nj, A.Rw);
                    dst[(size_t)mm[k] * A.dst_stride + jc0 + t] = make_float2(o.x * sum.x - o.y * sum.y, o.x * sum.y + o.y * sum.x);
                }
            }
        }
        // 5. behind an offset change: the outputs of the call's head whose windows cross it, again, sample by sample
        if (tile == 0 && t < n_tile) {
            for (int k = 0; k < cnt; k++)
                if (t < sSlow[k]) {
                    const int m = sOut[k];
                    dst[(size_t)m * A.dst_stride + t] = wr_slow(A.outs[m], hp, X, a0, nj, NP, A.Rw);
                }
        }
    }
}

void launch_wide_rate(const WideRateArgs &A, int streams, hipStream_t s) {
    if (A.n_out <= 0) return;
    const unsigned tiles = (unsigned)((A.n_out + wrate::TILE - 1) / wrate::TILE);
    hipLaunchKernelGGL(wide_rate_kernel, dim3(tiles, (unsigned)streams), dim3(WR_NT), 0, s, A, A.rot, A.phases, A.dst);
    FMX_LAUNCHED();
}

}  // namespace fmx

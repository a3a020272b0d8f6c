// fmx_wide.hip -- stage W, wide-band ingest (DESIGN.md "Stage W"; no counterpart in the reference): one stream at Rw = K * 2 304 000 S/s
// feeds many outputs at 2 304 000 S/s.  Output m is  y[j] = sum_i h[i] x[jK + K-1 - i] O(P[jK + K-1 - i]),  T = 16 K + 1 real taps,
// P[n] = (P[n-1] - f) mod Rw the reference oscillator's integer phase at the wide rate.
//
// One workgroup per (stream, tile of W_TILE outputs): the tile's W_TILE K samples and the 16 K in front of them are read from HBM ONCE,
// converted to f32 and kept in LDS as K rows of columns (sample s at row s mod K, column s / K), so that the 64 lanes of a wave -- 64
// consecutive outputs -- read 64 consecutive columns of one row for every tap: no bank conflicts.  Thread c computes output c of the
// tile for every output of the stream, four at a time (one LDS read feeds four complex products).  With a constant offset
// O(P[n_j - i]) = O(P[n_j]) O(i f), so the mix is folded into complex taps g[i] = h[i] O(i f) (built by the host in f64, fetched through the
// scalar cache: a workgroup's threads all work on the same outputs) and one rotator per output, O(P[n_j]).  P[n_j] is a multiple of K, so
// the rotator is an entry of the 2 304 000-point oscillator table.  The sum always runs in tap order, two accumulators per output
// (the products with Re g and with Im g), whatever the tile, the call or the position in it.
//
// The fold is exact only where a window holds samples of ONE offset.  Behind fmx_wideband_set_offset the history still holds samples
// mixed with the old offset (and with every offset before it that is less than 16 K samples old: WideOut::seg): the outputs whose
// windows reach back across a change are recomputed sample by sample with each sample's own phase (wide_slow: at most 16 per output and call).
#include "fmx_internal.h"
#include "../../include/fmx.h"

namespace fmx {

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int W_COLS = W_TILE + W_HCOLS + 1;      // 273: rows start 2 banks apart (the fill writes a sample's row = its index mod K)
constexpr int W_NT = 256;                         // threads: one per output of the tile
constexpr int W_SB = 4;                           // outputs of a stream computed together

__device__ __forceinline__ float2 wide_load(const void *src, int fmt, float qs, int64_t at) {
    switch (fmt) {
    case FMX_IQ_U8: { const uchar2 v = reinterpret_cast<const uchar2 *>(src)[at]; return make_float2((float)((int)v.x - 127) * qs, (float)((int)v.y - 127) * qs); }
    case FMX_IQ_S8: { const char2 v = reinterpret_cast<const char2 *>(src)[at]; return make_float2((float)v.x * qs, (float)v.y * qs); }
    case FMX_IQ_S16: { const short2 v = reinterpret_cast<const short2 *>(src)[at]; return make_float2((float)v.x * qs, (float)v.y * qs); }
    default: return reinterpret_cast<const float2 *>(src)[at];
    }
}

// Output column c (< 16) of a call's first tile whose window crosses an offset change: every sample with the phase it was mixed with.
template <int K>
__device__ __noinline__ float2 wide_slow(const WideOut &o, const float *__restrict__ h, const float2 (*X)[W_COLS], int64_t g0, int c) {
    constexpr int T = 16 * K + 1;
    constexpr int64_t RW = (int64_t)K * W_RATE0;
    float ar = 0.f, ai = 0.f;
    int k = 0;
    for (int i = 0; i < T; i++) {
        const int d = i / K, e = i - d * K;
        const int64_t n = g0 + (int64_t)(c + 1) * K - 1 - i;              // global index of the sample (n < 0: the zeros in front of the stream)
        while (k + 1 < o.nseg && n < o.seg[k].nbase) k++;                // (i grows, n falls: the runs are met newest first)
        int64_t q = (n - o.seg[k].nbase + 1) % RW; if (q < 0) q += RW;
        int64_t p = ((int64_t)o.seg[k].pbase - q * (int64_t)o.seg[k].f) % RW; if (p < 0) p += RW;
        double sn, cs;
        sincos(2.0 * 3.14159265358979323846 * (double)p / (double)RW, &sn, &cs);
        const float Or = (float)cs, Oi = (float)sn;
        const float2 x = X[K - 1 - e][c + W_HCOLS - d];
        const float vr = x.x * Or - x.y * Oi, vi = x.x * Oi + x.y * Or;
        ar = fmaf(h[i], vr, ar); ai = fmaf(h[i], vi, ai);
    }
    return make_float2(ar, ai);
}

// (taps / dst: WideArgs' pointers once more, as parameters the compiler knows not to alias -- the taps then come through scalar loads)
template <int K>
__global__ __launch_bounds__(W_NT) void wide_kernel(WideArgs A, const float2 *__restrict__ taps, float2 *__restrict__ dst) {
    constexpr int T = 16 * K + 1;
    __shared__ __attribute__((aligned(16))) float2 X[K][W_COLS];
    __shared__ int sOut[W_NT], sRot[W_NT], sStep[W_NT], sSlow[W_NT];
    const int t = threadIdx.x, tile = blockIdx.x, stream = blockIdx.y;
    const int64_t j0 = (int64_t)tile * W_TILE;                           // the tile's first output of the call
    const int n_tile = (int)(A.n_out - j0 < W_TILE ? A.n_out - j0 : W_TILE);
    const int64_t s0 = j0 * K - W_HCOLS * K;                             // call-relative index of the sample at X[0][0]
    const int nsamp = (n_tile + W_HCOLS) * K;

    // 1. the tile and its 16 K samples of history, converted once
    const float2 *hin = A.hist_in + (size_t)stream * W_HIST;
    const int64_t sbase = (int64_t)stream * A.src_stride;
    for (int idx = t; idx < (W_TILE + W_HCOLS) * K; idx += W_NT) {       // (a ragged tile's columns behind its last sample: zeros)
        const int64_t s = s0 + idx;
        const float2 v = idx >= nsamp ? make_float2(0.f, 0.f) : s >= 0 ? wide_load(A.src, A.fmt, A.qs, sbase + s) : hin[W_HCOLS * K + s];
        X[idx % K][idx / K] = v;
    }
    __syncthreads();
    // ... and what the next call finds in front of its first sample: the stream's last 16 K samples are the image's last 16 K
    if (j0 + n_tile == A.n_out) {
        float2 *hout = A.hist_out + (size_t)stream * W_HIST;
        for (int idx = t; idx < W_HCOLS * K; idx += W_NT) { const int at = n_tile * K + idx; hout[idx] = X[at % K][at / K]; }
    }

    const int st0 = A.first[stream], nst = A.first[stream + 1] - st0;
    const int64_t jg = A.g0 / K + j0;                                    // the tile's first output, counted from the stream's beginning
    for (int base = 0; base < nst; base += W_NT) {
        const int cnt = nst - base < W_NT ? nst - base : W_NT;
        // 2. per output of the stream (one thread each): the rotator's table index at the tile's first output and its step, and how many of
        //    the call's first outputs have a window that crosses an offset change
        __syncthreads();
        if (t < cnt) {
            const int m = A.list[st0 + base + t];
            const WideSeg g = A.outs[m].seg[0];
            const int64_t q = (jg + 1 - g.nbase / K) % W_RATE0;          // outputs since the run began, this one included
            const int step = g.f % W_RATE0;
            int64_t r = ((int64_t)(g.pbase / K) - q * step) % W_RATE0; if (r < 0) r += W_RATE0;
            int slow = 0;
            if (tile == 0 && A.outs[m].nseg > 1) {                       // output c's oldest sample g0 + (c + 1) K - T lies in front of the run:
                const int64_t lim = g.nbase - A.g0 + T;                  // (c + 1) K < lim <= T
                slow = lim > 0 ? (int)((lim - 1) / K) : 0;               // the number of such c >= 0 (at most 16)
            }
            sOut[t] = m; sRot[t] = (int)r; sStep[t] = step; sSlow[t] = slow;
        }
        __syncthreads();
        // 3. the folded filter: thread t = output column t of the tile, W_SB outputs of the stream at a time
        for (int sb = 0; sb < cnt; sb += W_SB) {
            const float2 *g[W_SB];
            int mm[W_SB];
#pragma unroll
            for (int k = 0; k < W_SB; k++) {
                const int at = sb + k < cnt ? sb + k : cnt - 1;          // (a short last group repeats its last output; only sb + k < cnt is stored)
                mm[k] = __builtin_amdgcn_readfirstlane(sOut[at]);
                g[k] = taps + (size_t)mm[k] * T;
            }
            v2f a[W_SB], b[W_SB];
#pragma unroll
            for (int k = 0; k < W_SB; k++) { a[k] = (v2f){0.f, 0.f}; b[k] = (v2f){0.f, 0.f}; }
            for (int d = 0; d < W_HCOLS; d++) {
#pragma unroll
                for (int e = 0; e < K; e++) {
                    const float2 x = X[K - 1 - e][t + W_HCOLS - d];
                    const v2f xa = (v2f){x.x, x.y}, xb = (v2f){x.y, x.x};
#pragma unroll
                    for (int k = 0; k < W_SB; k++) {
                        const float2 gk = g[k][K * d + e];
                        a[k] = __builtin_elementwise_fma((v2f){gk.x, gk.x}, xa, a[k]);
                        b[k] = __builtin_elementwise_fma((v2f){-gk.y, gk.y}, xb, b[k]);
                    }
                }
            }
            {   // the last tap, i = 16 K
                const float2 x = X[K - 1][t];
                const v2f xa = (v2f){x.x, x.y}, xb = (v2f){x.y, x.x};
#pragma unroll
                for (int k = 0; k < W_SB; k++) {
                    const float2 gk = g[k][T - 1];
                    a[k] = __builtin_elementwise_fma((v2f){gk.x, gk.x}, xa, a[k]);
                    b[k] = __builtin_elementwise_fma((v2f){-gk.y, gk.y}, xb, b[k]);
                }
            }
            // 4. the output's rotator O(P[n_j]) from the table, and the store
#pragma unroll
            for (int k = 0; k < W_SB; k++) {
                if (sb + k < cnt && t < n_tile) {
                    const v2f sum = a[k] + b[k];
                    int r = sRot[sb + k] - (int)(((unsigned)t * (unsigned)sStep[sb + k]) % (unsigned)W_RATE0);
                    if (r < 0) r += W_RATE0;
                    const float2 o = A.rot[r];
                    dst[(size_t)mm[k] * A.dst_stride + j0 + t] = make_float2(o.x * sum.x - o.y * sum.y, o.x * sum.y + o.y * sum.x);
                }
            }
        }
        // 5. behind an offset change: the outputs of the call's head whose windows cross it, again, sample by sample
        if (tile == 0 && t < W_HCOLS && t < n_tile) {
            for (int k = 0; k < cnt; k++)
                if (t < sSlow[k]) {
                    const int m = sOut[k];
                    dst[(size_t)m * A.dst_stride + t] = wide_slow<K>(A.outs[m], A.h, X, A.g0, t);
                }
        }
    }
}

template <int K> static void launch_wide_k(const WideArgs &A, int streams, hipStream_t s) {
    const unsigned tiles = (unsigned)((A.n_out + W_TILE - 1) / W_TILE);
    hipLaunchKernelGGL(wide_kernel<K>, dim3(tiles, (unsigned)streams), dim3(W_NT), 0, s, A, A.taps, A.dst);
}

void launch_wide(const WideArgs &A, int K, int streams, hipStream_t s) {
    if (A.n_out <= 0) return;
    switch (K) {
    case 2: launch_wide_k<2>(A, streams, s); break;
    case 3: launch_wide_k<3>(A, streams, s); break;
    case 4: launch_wide_k<4>(A, streams, s); break;
    case 5: launch_wide_k<5>(A, streams, s); break;
    case 6: launch_wide_k<6>(A, streams, s); break;
    case 7: launch_wide_k<7>(A, streams, s); break;
    case 8: launch_wide_k<8>(A, streams, s); break;
    case 9: launch_wide_k<9>(A, streams, s); break;
    case 10: launch_wide_k<10>(A, streams, s); break;
    case 11: launch_wide_k<11>(A, streams, s); break;
    case 12: launch_wide_k<12>(A, streams, s); break;
    case 13: launch_wide_k<13>(A, streams, s); break;
    case 14: launch_wide_k<14>(A, streams, s); break;
    case 15: launch_wide_k<15>(A, streams, s); break;
    case 16: launch_wide_k<16>(A, streams, s); break;
    default: note_hip(hipErrorInvalidValue); return;
    }
    FMX_LAUNCHED();
}

}  // namespace fmx

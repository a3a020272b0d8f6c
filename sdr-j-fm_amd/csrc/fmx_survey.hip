// fmx_survey.hip -- the band survey of stage W (the arithmetic is fmx_survey.h's): behind wide_kernel, on the call's stream,
// every stream's samples -- the carry, then the call's input, converted as wide_kernel converts them -- are cut into blocks of 4096.
//
// survey_block_kernel, one workgroup of 256 threads per (stream, completed block): sixteen samples per thread, windowed on load, three
// radix-16 passes in registers with two exchanges through LDS, Re^2 + Im^2 of the block's 4096 bins to power [stream][block][bin].  Its
// parallelism depends neither on the blocks per record nor on the number of streams.
// survey_fold_kernel, one thread per (stream, bin), behind it: the call's blocks added to the stream's accumulator in block order -- the
// order that makes a record independent of how the stream is cut into calls --, a record scaled and written to its ring slot at every
// record boundary; and one thread per (stream, carry sample): the call's samples behind its last complete block become the new carry (a
// call that completes no block appends to it).  The block kernel has read the old carry by then: one carry buffer per stream is enough.
// Traffic beside the 2 .. 8 input bytes per wide sample: 4 bytes written and 4 read of `power`.
#include "fmx_internal.h"
#include "fmx_survey.h"

namespace fmx {

namespace {

// a sample of the call's input, converted (wide_load of fmx_wide.hip: the same values)
__device__ __forceinline__ float2 survey_load(const void *src, int fmt, float qs, int64_t at) {
    switch (fmt) {
    case FMX_IQ_U8: { const uchar2 v = reinterpret_cast<const uchar2 *>(src)[at]; return make_float2((float)((int)v.x - 127) * qs, (float)((int)v.y - 127) * qs); }
    case FMX_IQ_S8: { const char2 v = reinterpret_cast<const char2 *>(src)[at]; return make_float2((float)v.x * qs, (float)v.y * qs); }
    case FMX_IQ_S16: { const short2 v = reinterpret_cast<const short2 *>(src)[at]; return make_float2((float)v.x * qs, (float)v.y * qs); }
    default: return reinterpret_cast<const float2 *>(src)[at];
    }
}

__global__ __launch_bounds__(survey::NT) void survey_block_kernel(SurveyArgs A, const float2 *__restrict__ W, float *__restrict__ power) {
    __shared__ float2 sZ[survey::LDS_N];
    const int t = threadIdx.x, stream = blockIdx.y;
    const int64_t j = blockIdx.x;
    const float2 *carry = A.carry + (size_t)stream * survey::N;
    const int64_t sbase = (int64_t)stream * A.src_stride;
    float2 x[survey::PER], y[survey::PER];
#pragma unroll
    for (int n2 = 0; n2 < survey::PER; n2++) {
        const int i = t + 256 * n2;
        const int64_t q = survey::source_index(j, i, A.fill);          // (q < 0 only in block 0: carry [i], i < fill)
        const float2 v = q < 0 ? carry[A.fill + q] : survey_load(A.src, A.fmt, A.qs, sbase + q);
        const float w = A.window[i];
        x[n2] = make_float2(v.x * w, v.y * w);
    }
    survey::pass1(t, x, W, sZ);
    __syncthreads();
    survey::pass2_load(t, sZ, y);
    __syncthreads();
    survey::pass2_store(t, y, W, sZ);
    __syncthreads();
    float p[survey::PER];
    survey::pass3(t, sZ, W, p);
    float *out = power + ((size_t)stream * (size_t)A.power_stride + (size_t)j) * survey::N;
#pragma unroll
    for (int c = 0; c < survey::PER; c++) out[t + 256 * c] = p[c];
}

__global__ __launch_bounds__(survey::NT) void survey_fold_kernel(SurveyArgs A) {
    const int i = blockIdx.x * survey::NT + threadIdx.x, stream = blockIdx.y;          // a bin, and a carry position
    float *accp = A.acc + (size_t)stream * survey::N + i;
    const float acc = A.fresh ? 0.f : *accp;
    *accp = survey::accumulate(acc, A.power + (size_t)stream * (size_t)A.power_stride * survey::N + i, A.blocks, A.phase, A.B, A.scale,
                               A.ring + (size_t)stream * survey::RING * survey::N + i, A.slot0);
    float2 *carry = A.carry + (size_t)stream * survey::N;
    const int64_t sbase = (int64_t)stream * A.src_stride;
    if (A.blocks == 0) {                                                 // fill + n_wide < 4096: the call's samples behind the old carry
        if (i < A.n_wide) carry[A.fill + i] = survey_load(A.src, A.fmt, A.qs, sbase + i);
    } else if (i < A.fill_after)                                         // the call's last fill_after samples
        carry[i] = survey_load(A.src, A.fmt, A.qs, sbase + A.n_wide - A.fill_after + i);
}

}  // namespace

void launch_survey(const SurveyArgs &A, int streams, hipStream_t s) {
    if (A.n_wide <= 0) return;
    if (A.blocks > 0)
        hipLaunchKernelGGL(survey_block_kernel, dim3((unsigned)A.blocks, (unsigned)streams), dim3(survey::NT), 0, s, A, A.W, A.power);
    hipLaunchKernelGGL(survey_fold_kernel, dim3(survey::N / survey::NT, (unsigned)streams), dim3(survey::NT), 0, s, A);
    FMX_LAUNCHED();
}

}  // namespace fmx

// fmx_spec.hip -- the spectrum meter (the arithmetic is fmx_survey.h's, the grid and the fold fmx_spec.h's): behind stage A, on the
// stream stage A ran on, the metered streams' samples of a piece -- the carry, then the piece's input, converted as stage A converts them -- are cut
// into the blocks of the S-grid.  The shape is the band survey's (fmx_survey.hip); what differs: the metered streams are a job list, the S-grid,
// the maximum beside the sum, the first-block rule, and a scratch array that the host bounds by cutting the piece's blocks into chunks.
//
// spec_block_kernel, one workgroup of 256 threads per (job, block of the chunk): sixteen samples per thread, windowed on load, three radix-16 passes in
// registers with two exchanges through the survey's 32 896-byte LDS image, Re^2 + Im^2 of the block's 4096 bins to power [job][block][bin].
// spec_fold_kernel, one thread per (job, bin), behind it: the chunk's blocks folded into the stream's sum and maximum in block order (spec::fold) --
// the order that makes a record independent of how the stream is cut into calls, pieces and chunks --, both scaled and stored to the record's ring
// slot at its last block; and, in the piece's last fold, one thread per (job, carry sample): the piece's samples of the block in progress become
// the new carry (a piece that stays inside one block appends to it).  Every block kernel of the piece that reads the old carry -- the first chunk's --
// has run by then: one carry buffer per stream is enough.  No atomics, no inline assembly.
#include "fmx_internal.h"
#include "fmx_spec.h"

namespace fmx {

namespace {

// a sample of the piece's input, converted (stage A's values: (u8 - 127) / 128, s8 / 128, s16 / denominator)
__device__ __forceinline__ float2 spec_load(const void *src, int fmt, float qs, int64_t at) {
    switch (fmt) {
    case FMX_IQ_U8: { const uchar2 v = reinterpret_cast<const uchar2 *>(src)[at]; return make_float2((float)((int)v.x - 127) * qs, (float)((int)v.y - 127) * qs); }
    case FMX_IQ_S8: { const char2 v = reinterpret_cast<const char2 *>(src)[at]; return make_float2((float)v.x * qs, (float)v.y * qs); }
    case FMX_IQ_S16: { const short2 v = reinterpret_cast<const short2 *>(src)[at]; return make_float2((float)v.x * qs, (float)v.y * qs); }
    default: return reinterpret_cast<const float2 *>(src)[at];
    }
}

__global__ __launch_bounds__(spec::NT) void spec_block_kernel(SpecArgs A) {
    __shared__ float2 sZ[survey::LDS_N];
    const int t = threadIdx.x, jl = blockIdx.y;
    const SpecJob job = A.jobs[A.job0 + jl];
    const int64_t b = A.b + (int64_t)blockIdx.x;
    const float2 *carry = A.carry + (size_t)job.slot * spec::N;
    const int64_t sbase = (int64_t)job.stream * A.src_stride;
    float2 x[spec::PER], y[spec::PER];
#pragma unroll
    for (int n2 = 0; n2 < spec::PER; n2++) {
        const int i = t + 256 * n2;
        const int64_t q = spec::source_index(b, i, A.g0, A.S);          // (q < 0 only in the piece's first block: carry [i], i < fill)
        float2 v = make_float2(0.f, 0.f);
        if (q < 0) v = carry[i];
        else if (q < A.n) v = spec_load(A.src, A.fmt, A.qs, sbase + q);  // (always: the block completes in the piece)
        const float w = A.window[i];
        x[n2] = make_float2(v.x * w, v.y * w);
    }
    survey::pass1(t, x, A.W, sZ);
    __syncthreads();
    survey::pass2_load(t, sZ, y);
    __syncthreads();
    survey::pass2_store(t, y, A.W, sZ);
    __syncthreads();
    float p[spec::PER];
    survey::pass3(t, sZ, A.W, p);
    float *out = A.power + ((size_t)jl * (size_t)A.nb + (size_t)blockIdx.x) * spec::N;
#pragma unroll
    for (int c = 0; c < spec::PER; c++) out[t + 256 * c] = p[c];
}

__global__ __launch_bounds__(spec::NT) void spec_fold_kernel(SpecArgs A) {
    const int i = blockIdx.x * spec::NT + threadIdx.x, jl = blockIdx.y;          // a bin, and a carry position
    const SpecJob job = A.jobs[A.job0 + jl];
    if (A.nb > 0) {
        float *accp = A.acc + (size_t)job.slot * 2 * spec::N + i;
        float sum = accp[0], mx = accp[spec::N];
        float *ring = A.ring + (size_t)job.slot * spec::RING * 2 * spec::N + i;
        spec::fold(sum, mx, A.power + (size_t)jl * (size_t)A.nb * spec::N + i, spec::N, A.b, A.nb, job.first, A.phase, A.B, A.c, A.c1, ring, ring + spec::N);
        accp[0] = sum; accp[spec::N] = mx;
    }
    if (!A.write_carry) return;
    float2 *carry = A.carry + (size_t)job.slot * spec::N;
    const int64_t sbase = (int64_t)job.stream * A.src_stride;
    if (A.append) {                                                      // the piece's samples behind the old carry (fill + n < 4096)
        if (i < A.n) carry[A.fill + i] = spec_load(A.src, A.fmt, A.qs, sbase + i);
    } else if (i < A.fill_after)                                         // the piece's samples from the start of the block in progress
        carry[i] = spec_load(A.src, A.fmt, A.qs, sbase + A.carry_src + i);
}

}  // namespace

void launch_spec(const SpecArgs &A, hipStream_t s) {
    if (A.n_jobs <= 0) return;
    if (A.nb > 0) hipLaunchKernelGGL(spec_block_kernel, dim3((unsigned)A.nb, (unsigned)A.n_jobs), dim3(spec::NT), 0, s, A);
    if (A.nb > 0 || A.write_carry) hipLaunchKernelGGL(spec_fold_kernel, dim3(spec::N / spec::NT, (unsigned)A.n_jobs), dim3(spec::NT), 0, s, A);
    FMX_LAUNCHED();
}

}  // namespace fmx

// fmx_mpx.hip -- the multiplex spectrum meter (the arithmetic is fmx_survey.h's, the grid fmx_spec.h's, the loader and the fold
// fmx_mpx.h's): behind stage B, on the stream on which stage_rds and the modulation meter read the rows, the metered channels' demodulator output of a
// piece -- the carry, then the piece's row of w_dem -- is cut into the blocks of the S-grid.  The shape is the spectrum meter's (fmx_spec.hip); what
// differs: a real row per channel and piece instead of a complex stream, and the 2048 bins a real input has.
//
// mpx_block_kernel, one workgroup of 256 threads per (job, block of the chunk): sixteen samples per thread, windowed on load, imaginary part zero, three
// radix-16 passes in registers with two exchanges through the survey's 32 896-byte LDS image, Re^2 + Im^2 of bins 0 .. 2047 to power [job][block][bin]
// (pass 3 leaves thread t the bins t + 256 c: c < 8 are stored, coalesced).
// mpx_fold_kernel, behind it: one thread per (job, bin) folds the chunk's blocks into the channel's sum and maximum in block order (mpx::fold) -- the
// order that makes a record independent of how the stream is cut into calls, pieces and chunks --, both scaled and stored to the record's ring slot at
// its last block; and, in the piece's last fold, one thread per (job, carry sample): the piece's samples of the block in progress become the new carry
// (a piece that stays inside one block appends to it).  Every block kernel of the piece that reads the old carry -- the first chunk's -- has run by
// then: one carry buffer per channel is enough.
// mpx_gather_kernel, for fmx_mpx_spectrum_read: the records of a range of channels into one staging array.  No atomics, no inline assembly.
#include "fmx_internal.h"
#include "fmx_mpx.h"

namespace fmx {

namespace {

__global__ __launch_bounds__(mpx::NT) void mpx_block_kernel(MpxArgs A) {
    __shared__ float2 sZ[survey::LDS_N];
    const int t = threadIdx.x, jl = blockIdx.y;
    const MpxJob job = A.jobs[A.job0 + jl];
    const int64_t b = A.b + (int64_t)blockIdx.x;
    float2 x[mpx::PER], y[mpx::PER];
    mpx::load(t, b, A.g0, A.n, A.S, A.carry + (size_t)job.slot * mpx::N, A.w_dem + (size_t)job.channel * (size_t)A.lin_rows, A.window, x);
    survey::pass1(t, x, A.W, sZ);
    __syncthreads();
    survey::pass2_load(t, sZ, y);
    __syncthreads();
    survey::pass2_store(t, y, A.W, sZ);
    __syncthreads();
    float p[mpx::PER];
    survey::pass3(t, sZ, A.W, p);
    float *out = A.power + ((size_t)jl * (size_t)A.nb + (size_t)blockIdx.x) * mpx::BINS;
#pragma unroll
    for (int c = 0; c < mpx::KEEP; c++) out[t + 256 * c] = p[c];
}

__global__ __launch_bounds__(mpx::NT) void mpx_fold_kernel(MpxArgs A) {
    const int i = blockIdx.x * mpx::NT + threadIdx.x, jl = blockIdx.y;          // a bin (i < 2048), and a carry position (i < 4096)
    const MpxJob job = A.jobs[A.job0 + jl];
    if (A.nb > 0 && i < mpx::BINS) {
        float *accp = A.acc + (size_t)job.slot * 2 * mpx::BINS + i;
        float sum = accp[0], mx = accp[mpx::BINS];
        float *ring = A.ring + (size_t)job.slot * mpx::RING * 2 * mpx::BINS + i;
        mpx::fold(sum, mx, A.power + (size_t)jl * (size_t)A.nb * mpx::BINS + i, mpx::BINS, A.b, A.nb, job.first, A.phase, A.B, A.c, A.c1, ring, ring + mpx::BINS);
        accp[0] = sum; accp[mpx::BINS] = mx;
    }
    if (!A.write_carry) return;
    float *carry = A.carry + (size_t)job.slot * mpx::N;
    const float *row = A.w_dem + (size_t)job.channel * (size_t)A.lin_rows;
    if (A.append) {                                                      // the piece's samples behind the old carry (fill + n < 4096)
        if (i < A.n) carry[A.fill + i] = row[i];
    } else if (i < A.fill_after)                                         // the piece's samples from the start of the block in progress
        carry[i] = row[A.carry_src + i];
}

// the read-out's gather: workgroup q copies ring record src [q] (slot * RING + r mod RING: 2 x 2048 floats, mean then peak) to out [q], so that a range of
// channels leaves the device in one copy
__global__ __launch_bounds__(mpx::NT) void mpx_gather_kernel(const float *__restrict__ ring, const int32_t *__restrict__ src, float *__restrict__ out) {
    const float *from = ring + (size_t)src[blockIdx.x] * 2 * mpx::BINS;
    float *to = out + (size_t)blockIdx.x * 2 * mpx::BINS;
#pragma unroll
    for (int c = 0; c < 2 * mpx::BINS / mpx::NT; c++) to[threadIdx.x + mpx::NT * c] = from[threadIdx.x + mpx::NT * c];
}

}  // namespace

void launch_mpx(const MpxArgs &A, hipStream_t s) {
    if (A.n_jobs <= 0) return;
    if (A.nb > 0) hipLaunchKernelGGL(mpx_block_kernel, dim3((unsigned)A.nb, (unsigned)A.n_jobs), dim3(mpx::NT), 0, s, A);
    // (2048 threads per job fold; only the piece's last launch of a group, which writes up to 4096 carry samples, needs the other 2048)
    const unsigned per_job = (unsigned)((A.write_carry ? mpx::N : mpx::BINS) / mpx::NT);
    if (A.nb > 0 || A.write_carry) hipLaunchKernelGGL(mpx_fold_kernel, dim3(per_job, (unsigned)A.n_jobs), dim3(mpx::NT), 0, s, A);
    FMX_LAUNCHED();
}

void launch_mpx_gather(const float *ring, const int32_t *src, float *out, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(mpx_gather_kernel, dim3((unsigned)n), dim3(mpx::NT), 0, s, ring, src, out);
    FMX_LAUNCHED();
}

}  // namespace fmx

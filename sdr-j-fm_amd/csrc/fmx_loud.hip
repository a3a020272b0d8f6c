// fmx_loud.hip -- the programme audio meter: per channel and 100 ms window each ear's peak, mean square and K-weighted mean square
// (ITU-R BS.1770-4's two biquads at 48 000 frames/s) and the mean of left x right, from the PCM the piece has just delivered.
//
// Each (channel, ear) is one sequential machine and one lane: a wave holds 32 metered channels of a piece, from a job table (fmx_loud.h audio_produce), a
// workgroup is one wave.  The lanes do not walk their rows in global memory: the wave loads a tile of 64 frames of each of its channels with one coalesced
// 512-byte load per channel, one tile ahead of the one it walks, and puts it into LDS -- rows of 65 float2, so that the 32 rows a step reads lie in 32
// different bank pairs; the two lanes of a channel read the same float2 (a broadcast), which also gives the left lane its neighbour's sample for the
// cross sum.  Every lane runs in frame order in f32 without contraction (this file is compiled with -ffp-contract=off).  What a channel carries from piece
// to piece is its 16 floats (filter states and the accumulators of the window in progress), so a record does not depend on how the stream is cut.  The
// window grid is the same for every channel: a window's end is uniform over the wave, and each lane writes its own fields of the record.
#include "fmx_internal.h"
#include "fmx_loud.h"

namespace fmx {

namespace {

constexpr int CHW = 32;                    // channels per wave
constexpr int ROW = loud::TILE + 1;        // float2 per channel and tile in LDS: 130 dwords, row i starts in bank 2 i mod 64

__global__ __launch_bounds__(64) void loud_kernel(LoudArgs A, int n_jobs) {
    __shared__ float2 tile[2][CHW * ROW];
    __shared__ int64_t rowoff[CHW];
    const int lane = (int)threadIdx.x, base = (int)blockIdx.x * CHW;
    const int nch = n_jobs - base < CHW ? n_jobs - base : CHW;      // the wave's channels (uniform)
    const int frames = A.frames;
    if (nch <= 0 || frames <= 0) return;
    const int mine = lane >> 1, ear = lane & 1;
    const bool live = mine < nch;
    LoudJob job{-1, 0, 0, 0};
    if (live) job = A.jobs[base + mine];
    // (the rows behind the wave's last channel repeat it: the tile loads below are unconditional and stay inside the piece's PCM)
    if (lane < CHW) rowoff[lane] = (int64_t)A.jobs[base + (lane < nch ? lane : nch - 1)].ch * A.pcm_stride;
    __syncthreads();

    float st[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float *__restrict__ sp = A.state + (size_t)(live ? job.ch : 0) * loud::STATE + (size_t)ear * 8;
    if (live && !job.reset) {
        const float4 a = *reinterpret_cast<const float4 *>(sp), b = *reinterpret_cast<const float4 *>(sp + 4);
        st[0] = a.x; st[1] = a.y; st[2] = a.z; st[3] = a.w; st[4] = b.x; st[5] = b.y; st[6] = b.z; st[7] = b.w;
    }
    float t1a = st[loud::S_T1A], t2a = st[loud::S_T2A], t1b = st[loud::S_T1B], t2b = st[loud::S_T2B];
    float pk = st[loud::S_PK], s2 = st[loud::S_S2], z = st[loud::S_Z], sx = st[loud::S_SX];
    const float b0a = loud::K_COEF[0][0], b1a = loud::K_COEF[0][1], b2a = loud::K_COEF[0][2], a1a = loud::K_COEF[0][3], a2a = loud::K_COEF[0][4];
    const float b0b = loud::K_COEF[1][0], b1b = loud::K_COEF[1][1], b2b = loud::K_COEF[1][2], a1b = loud::K_COEF[1][3], a2b = loud::K_COEF[1][4];

    int64_t w = loud::window_of(A.M0);
    int until = (int)((w + 1) * loud::WINDOW - A.M0);      // frames to the end of window w (uniform, 1 .. 4800)
    bool acc = job.acc != 0;                                // the window in progress has been metered from its start
    int k = 0;                                              // records this lane's channel has left in this piece

    const int ntiles = (frames + loud::TILE - 1) / loud::TILE;
    float2 r[CHW];
    // tile t of every channel of the wave into registers: lane l takes frame 64 t + l (the last tile is ragged: a lane behind the piece's frames loads
    // the piece's last frame again, which no machine walks)
    auto fetch = [&](int t) {
        const int f = t * loud::TILE + lane < frames ? t * loud::TILE + lane : frames - 1;
#pragma unroll
        for (int i = 0; i < CHW; i++) r[i] = A.pcm[rowoff[i] + f];
    };
    auto put = [&](int b) {
#pragma unroll
        for (int i = 0; i < CHW; i++) tile[b][i * ROW + lane] = r[i];
    };
    fetch(0); put(0);
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        if (t + 1 < ntiles) fetch(t + 1);
        const int nf = frames - t * loud::TILE < loud::TILE ? frames - t * loud::TILE : loud::TILE;
        {   // (every lane walks, so that the loop's bounds stay uniform: a lane without a channel walks a copy of the wave's last row and stores nothing)
            const float2 *__restrict__ row = &tile[t & 1][mine * ROW];
            int f = 0;
            while (f < nf) {
                const int stop = nf - f < until ? nf : f + until;
                until -= stop - f;
#pragma unroll 8
                for (; f < stop; f++) {
                    const float2 v = row[f];
                    const float x = ear ? v.y : v.x;
                    pk = fmaxf(pk, fabsf(x));
                    const float xx = x * x; s2 += xx;
                    const float p0 = b0a * x; const float o = p0 + t1a;
                    const float p1 = b1a * x, q1 = a1a * o; const float d1 = p1 - q1; t1a = d1 + t2a;
                    const float p2 = b2a * x, q2 = a2a * o; t2a = p2 - q2;
                    const float r0 = b0b * o; const float y = r0 + t1b;
                    const float r1 = b1b * o, u1 = a1b * y; const float e1 = r1 - u1; t1b = e1 + t2b;
                    const float r2 = b2b * o, u2 = a2b * y; t2b = r2 - u2;
                    const float yy = y * y; z += yy;
                    const float lr = v.x * v.y; sx += lr;
                }
                if (until == 0) {      // window w ends with frame f - 1
                    if (acc && live) {
                        char *rec = reinterpret_cast<char *>(A.ring + (size_t)job.ch * loud::RING + (size_t)((job.slot0 + k) & (loud::RING - 1)));
                        float *fl = reinterpret_cast<float *>(rec + 16);      // peak_l, peak_r, ms_l, ms_r, kms_l, kms_r, cross
                        fl[0 + ear] = pk; fl[2 + ear] = loud::finish_mean(s2); fl[4 + ear] = loud::finish_mean(z);
                        if (ear == 0) {
                            int64_t *ix = reinterpret_cast<int64_t *>(rec);
                            ix[0] = w; ix[1] = (w + 1) * loud::WINDOW;
                            fl[6] = loud::finish_mean(sx);
                            reinterpret_cast<int32_t *>(rec)[11] = 0;
                        }
                        k++;
                    }
                    pk = s2 = z = sx = 0.f;
                    acc = true; w++; until = loud::WINDOW;
                }
            }
        }
        if (t + 1 < ntiles) put((t + 1) & 1);
        __syncthreads();
    }
    if (live) {
        *reinterpret_cast<float4 *>(sp) = make_float4(t1a, t2a, t1b, t2b);
        *reinterpret_cast<float4 *>(sp + 4) = make_float4(pk, s2, z, sx);
    }
}

}  // namespace

static_assert(sizeof(fmx_audio_record) == 48, "the kernel writes the record's fields by their offsets");

void launch_loud(const LoudArgs &A, int n_jobs, hipStream_t s) {
    if (n_jobs <= 0 || A.frames <= 0) return;
    hipLaunchKernelGGL(loud_kernel, dim3((unsigned)((n_jobs + CHW - 1) / CHW)), dim3(64), 0, s, A, n_jobs);
}

}  // namespace fmx

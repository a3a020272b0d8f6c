// fmx_diag.hip -- the diagnostics of libfmx: the streaming-bandwidth probe and stage A's phase counters (include/fmx_debug.h), and the per-stage profile
// of a handle's calls (fmx_profile_*, include/fmx.h).  Nothing here is on a call's path: run_piece records a profiled call's events (fmx_api.hip), these
// entry points read them.
#include "fmx_host.h"

#include <cstring>

// ---- diagnostics: the practical HBM ceiling (SURVEY 8d asks for the measured device-copy bandwidth next to the nominal 8 TB/s)
namespace fmx {
typedef float f32x4_t __attribute__((ext_vector_type(4)));
// mode 0: dst[i] = src[i] (float2 copy, 16 B per lane per access);  mode 1: stage A's traffic shape: read 12 float2, write 1;  mode 2: the same reads and NO
// write (a sum that is never the sentinel): what this GPU reads at when nothing is written -- the ceiling of `roofline.frac_read_only`.
template <int MODE>
__global__ __launch_bounds__(256) void stream_probe_kernel(const f32x4_t *__restrict__ src, f32x4_t *__restrict__ dst, size_t n16) {
    const size_t stride = (size_t)gridDim.x * 256;
    if (MODE == 0) {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
    } else {
        // each lane reads 6 x 16 B (12 float2) spaced a wave apart (coalesced), sums, and writes one float2 per 12 read
        const size_t ngroups = n16 / (6 * 64);
        const size_t wave = ((size_t)blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = stride >> 6;
        const int lane = threadIdx.x & 63;
        for (size_t g = wave; g < ngroups; g += nwaves) {
            f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 6; k++) a += __builtin_nontemporal_load(src + (g * 6 + k) * 64 + lane);
            if (MODE == 2) { if (a.x + a.z == 1.2345e33f) reinterpret_cast<float2 *>(dst)[lane] = make_float2(a.y, a.w); }
            else reinterpret_cast<float2 *>(dst)[g * 64 + lane] = make_float2(a.x + a.z, a.y + a.w);
        }
    }
}
}  // namespace fmx

namespace {

// the events of the profiled calls made so far, into the handle's sums
int prof_drain(fmx_handle h) {
    for (auto &pr : h->prof) {
        HIPCHK(hipEventSynchronize(pr.e[3]));
        for (int k = 0; k < 3; k++) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, pr.e[k], pr.e[k + 1]));
            h->prof_acc.ms[k] += ms; h->prof_acc.launches[k] += 1;
        }
        h->prof_acc.input_samples += pr.in_samples; h->prof_acc.channel_samples += pr.ch_samples;
        for (int i = 0; i < 4; i++) (void)hipEventDestroy(pr.e[i]);
    }
    h->prof.clear();
    return FMX_OK;
}

}  // namespace

extern "C" {

// diagnostics (include/fmx_debug.h): streaming bandwidth of this GPU in GB/s over `bytes` of float2 data, the mean of
// `iters` launches timed with HIP events.  mode 0: copy (counts bytes read + written); mode 1: read 12, write 1 (stage A's shape).
int fmx_debug_stream_bandwidth(int32_t device, int32_t mode, int64_t bytes, int32_t iters, double *gbps) {
    if (!gbps || bytes < (1 << 20) || iters < 1 || mode < 0 || mode > 2) return fail(FMX_E_INVALID, "bad argument");
    HIPCHK(hipSetDevice(device));
    const size_t n16 = (size_t)bytes / 16 / (6 * 64) * (6 * 64);
    fmx::f32x4_t *src = nullptr, *dst = nullptr;
    HIPCHK(hipMalloc(&src, n16 * 16));
    if (hipMalloc(&dst, mode == 0 ? n16 * 16 : n16 * 16 / 12 + 64) != hipSuccess) { (void)hipFree(src); return fail(FMX_E_HIP, "hipMalloc"); }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipMemset(src, 0, n16 * 16));
    const int grid = 256 * 8;
    for (int it = -2; it < iters; it++) {
        if (it == 0) HIPCHK(hipEventRecord(e0, 0));
        if (mode == 0) hipLaunchKernelGGL(fmx::stream_probe_kernel<0>, dim3(grid), dim3(256), 0, 0, src, dst, n16);
        else if (mode == 1) hipLaunchKernelGGL(fmx::stream_probe_kernel<1>, dim3(grid), dim3(256), 0, 0, src, dst, n16);
        else hipLaunchKernelGGL(fmx::stream_probe_kernel<2>, dim3(grid), dim3(256), 0, 0, src, dst, n16);
    }
    HIPCHK(hipEventRecord(e1, 0));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    const double moved = mode == 0 ? 2.0 * n16 * 16 : (mode == 1 ? n16 * 16 * (1.0 + 1.0 / 12) : (double)n16 * 16);
    *gbps = moved * iters / (ms * 1e-3) * 1e-9;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(src); (void)hipFree(dst);
    return FMX_OK;
}

// diagnostics (include/fmx_debug.h): per-phase shader-cycle counters of front_kernel, summed over channels
int fmx_debug_phase_cycles(fmx_handle h, int32_t enable, unsigned long long *out /*[DBG_SLOTS = 96], may be null*/) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    const size_t nb = sizeof(unsigned long long) * DBG_SLOTS * (size_t)h->channels;
    if (out && h->B.dbg) {
        std::vector<unsigned long long> tmp(DBG_SLOTS * (size_t)h->channels);
        HIPCHK(hipMemcpy(tmp.data(), h->B.dbg, nb, hipMemcpyDeviceToHost));
        for (int k = 0; k < DBG_SLOTS; k++) { out[k] = 0; for (int c = 0; c < h->channels; c++) out[k] += tmp[(size_t)c * DBG_SLOTS + k]; }
    }
    if (enable && !h->B.dbg) FMXCHK(h->mem.alloc(h->B.dbg, DBG_SLOTS * (size_t)h->channels));
    if (h->B.dbg) HIPCHK(hipMemset(h->B.dbg, 0, nb));
    if (!enable) h->mem.release(h->B.dbg);
    return FMX_OK;
}

// diagnostics (include/fmx_debug.h): the scalar state of a channel's RDS slicers behind the handle's last call, a plain copy (no launch)
int fmx_debug_rds_state(fmx_handle h, int32_t channel, float *out, int32_t capacity, int32_t *n) {
    if (!h || !out || !n || channel < 0 || channel >= h->channels || capacity < FMX_DEBUG_RDS_STATE_FIELDS) return fail(FMX_E_INVALID, "bad argument");
    *n = 0;
    if (!h->rds_alloc) return FMX_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    RdsState s2; Rds1State s1; Rds3State s3;
    HIPCHK(hipMemcpy(&s2, h->R.state + channel, sizeof(s2), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&s1, h->R.state1 + channel, sizeof(s1), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&s3, h->R.state3 + channel, sizeof(s3), hipMemcpyDeviceToHost));
    const float v[FMX_DEBUG_RDS_STATE_FIELDS] = {
        (float)h->params[channel].rds_mode, (float)s2.nbits,
        s2.gain, s2.c_freq, s2.c_phase, s2.mu, (float)s2.skip, (float)s2.sample_count,
        s1.c_freq, s1.c_phase, s1.last_sync,
        s3.c_freq, s3.c_phase, s3.bit_clk_phase, (float)s3.bs_sync_err, (float)s3.bs_synced };
    std::memcpy(out, v, sizeof(v));
    *n = FMX_DEBUG_RDS_STATE_FIELDS;
    return FMX_OK;
}

int fmx_profile_enable(fmx_handle h, int32_t on) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    h->prof_on = on != 0;
    return FMX_OK;
}
int fmx_profile_read(fmx_handle h, fmx_profile *out, int32_t reset) {
    if (!h || !out) return fail(FMX_E_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    int rc = prof_drain(h);
    if (rc) return rc;
    *out = h->prof_acc;
    if (reset) std::memset(&h->prof_acc, 0, sizeof(h->prof_acc));
    return FMX_OK;
}

}  // extern "C"

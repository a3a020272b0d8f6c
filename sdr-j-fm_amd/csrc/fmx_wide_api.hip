// fmx_wide_api.hip -- the host half of stage W, wide-band ingest (fmx_wideband_* of include/fmx.h; the kernel is in fmx_wide.hip, that of a rate
// object -- fmx_wideband_create_rate, DESIGN.md 4.10 -- in fmx_wide_rate.hip with its integers and its prototype in fmx_wide_rate.h), and of its band
// survey (fmx_wideband_survey_*; kernels in fmx_survey.hip, bookkeeping and station finder in fmx_survey.h).  It shares nothing with
// fmx_handle but the error, the checking macros and the memory owner of fmx_host.h.
#include "fmx_host.h"
#include "fmx_design.h"
#include "fmx_survey.h"
#include "fmx_wide_rate.h"

#include <cmath>

// ---- stage W: wide-band ingest (fmx_wide.hip; DESIGN.md "Stage W") ------------------------------------------------------------------
// One object = `streams` inputs at K * 2 304 000 S/s and `outputs` stations at 2 304 000 S/s.  Everything an output's oscillator needs
// is integer arithmetic the host can do: the device holds, per output, the runs of samples mixed with one offset (WideOut) and the
// folded taps; both are uploaded only when an offset changes.  The samples' history has two buffers, swapped per call, because the
// workgroup that writes the new one runs beside the ones that read the old one.
struct fmx_wideband_s {
    int device = 0, streams = 0, K = 0, outputs = 0, T = 0;   // a rate object (fmx_wideband_create_rate): K = 0, T = NP, the samples of a window
    wrate::Ratio rate{};                     // ... its Rw = 2 304 000 M / L (L = 0: a factor object)
    float *d_phases = nullptr;               // [L][NP] the prototype's phases; d_taps then holds the rotators O (i f) alone
    int64_t max_block = 0, Rw = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    DevMem mem;
    std::mutex mtx;                          // guards `want` (fmx_wideband_set_offset from any thread)
    std::vector<int32_t> want, cur;          // the offsets asked for / in force
    std::vector<WideOut> outs;               // host mirror
    std::vector<float> h;                    // the low-pass, T taps
    int64_t g0 = 0;                          // wide samples per stream so far
    int parity = 0;                          // which history buffer the next call reads
    bool outs_dirty = true;
    int multi = 0;                           // outputs with more than one run inside a window
    float2 *d_hist[2] = {nullptr, nullptr}, *d_taps = nullptr, *d_rot = nullptr, *d_out = nullptr;
    float *d_h = nullptr;
    WideOut *d_outs = nullptr;
    int32_t *d_first = nullptr, *d_list = nullptr;
    char *d_in = nullptr;                    // fmx_wideband_process_host_raw's staging buffers: d_in, d_out
    // the band survey (fmx_survey.hip; allocated by the first fmx_wideband_survey_enable).  Every stream takes the same samples per call, so one
    // set of counters serves them all; the device keeps none.
    int32_t sv_B = 0, sv_fill = 0;           // blocks per record (0: off), samples in the carries
    int64_t sv_blocks = 0, sv_g0 = 0;        // blocks completed since the survey began, and the wide sample (of g0's count) it began at
    int64_t sv_cap = 0;                      // blocks of a call d_sv_power has room for, per stream
    bool sv_fresh = false;                   // no call since the survey began: the accumulators start at zero
    float sv_scale = 0.f;
    std::vector<float> sv_win;
    std::vector<int64_t> sv_read;            // per stream: the next record fmx_wideband_survey_read hands out
    float *d_sv_win = nullptr, *d_sv_power = nullptr, *d_sv_acc = nullptr, *d_sv_ring = nullptr;
    float2 *d_sv_W = nullptr, *d_sv_carry = nullptr;
    hipEvent_t ev_sv = nullptr; bool ev_sv_set = false; hipStream_t rd_stream = nullptr;   // behind the last call's survey kernels; the read-out's copies
};

namespace {

int64_t pmod(int64_t a, int64_t m) { const int64_t r = a % m; return r < 0 ? r + m : r; }

std::vector<float> wide_lowpass(int K) { return design::lowpass(16 * K + 1, 400000, K * W_RATE0); }

// the folded taps of one output: g[i] = h[i] O((i f) mod Rw), the products formed in f64 and rounded once (a rate object: O alone, the
// tap depends on the output's phase and stays with the kernel)
void wide_fold_taps(const fmx_wideband_s *w, int32_t f, float2 *g) {
    const int64_t fm = pmod(f, w->Rw);
    for (int i = 0; i < w->T; i++) {
        const double ang = 2.0 * design::kPi * (double)((i * fm) % w->Rw) / (double)w->Rw;
        if (w->rate.L) { g[i] = make_float2((float)std::cos(ang), (float)std::sin(ang)); continue; }
        g[i] = make_float2((float)((double)w->h[i] * std::cos(ang)), (float)((double)w->h[i] * std::sin(ang)));
    }
}

// rate: null for a factor object, else the accepted ratio of a rate object (cfg->factor must then be 0)
int wide_check_config(const fmx_wideband_config *cfg, const wrate::Ratio *rate = nullptr) {
    if (cfg->struct_size != (int32_t)sizeof(fmx_wideband_config)) return fail(FMX_E_INVALID, "fmx_wideband_config.struct_size mismatch");
    if (rate && cfg->factor != 0) return fail(FMX_E_INVALID, "factor must be 0 where a wide rate is given");
    if (!rate && (cfg->factor < W_MIN_K || cfg->factor > W_MAX_K)) return fail(FMX_E_INVALID, "factor must be in [2, 16]");
    if (cfg->streams < 1 || cfg->streams > 65535) return fail(FMX_E_INVALID, "streams must be in [1, 65535]");
    if (cfg->outputs < 1 || !cfg->stream_of_output) return fail(FMX_E_INVALID, "outputs must be >= 1, with a stream each");
    if (rate && cfg->max_block < rate->min_call) return fail(FMX_E_INVALID, "max_block must be at least ceil (M / L)");
    if (!rate && (cfg->max_block < cfg->factor || cfg->max_block % cfg->factor != 0)) return fail(FMX_E_INVALID, "max_block must be a positive multiple of factor");
    const int64_t lim = (rate ? rate->Rw : (int64_t)cfg->factor * W_RATE0) / 2 - 150000;
    for (int m = 0; m < cfg->outputs; m++) {
        if (cfg->stream_of_output[m] < 0 || cfg->stream_of_output[m] >= cfg->streams) return fail(FMX_E_INVALID, "stream_of_output entry out of range");
        const int64_t f = cfg->offset_hz ? cfg->offset_hz[m] : 0;
        if (f > lim || f < -lim) return fail(FMX_E_INVALID, rate ? "offset_hz: |f| must be <= wide_rate_hz / 2 - 150000" : "offset_hz: |f| must be <= factor * 1152000 - 150000");
    }
    return FMX_OK;
}

int wide_init(fmx_wideband w, const fmx_wideband_config *cfg, const wrate::Ratio *rate = nullptr) {
    w->device = cfg->device; w->streams = cfg->streams; w->K = cfg->factor; w->outputs = cfg->outputs;
    w->T = 16 * w->K + 1; w->max_block = cfg->max_block; w->Rw = (int64_t)w->K * W_RATE0;
    std::vector<float> phases;
    if (rate) {
        w->rate = *rate; w->T = rate->NP; w->Rw = rate->Rw;
        if (!wrate::fits(*rate)) return fail(FMX_E_INVALID, "wide_rate_hz: a tile's samples do not fit the workgroup's image");
        w->h = wrate::prototype(*rate);
        phases = wrate::phase_table(*rate, w->h);
    } else {
        w->h = wide_lowpass(w->K);
    }
    w->cur.assign((size_t)w->outputs, 0);
    for (int m = 0; m < w->outputs; m++) w->cur[m] = cfg->offset_hz ? cfg->offset_hz[m] : 0;
    w->want = w->cur;
    w->outs.assign((size_t)w->outputs, WideOut{});
    std::vector<int32_t> first((size_t)w->streams + 1, 0), list((size_t)w->outputs);
    for (int m = 0; m < w->outputs; m++) first[(size_t)cfg->stream_of_output[m] + 1]++;
    for (int s = 0; s < w->streams; s++) first[s + 1] += first[s];
    std::vector<int32_t> fill(first.begin(), first.end() - 1);
    std::vector<float2> taps((size_t)w->outputs * w->T);
    for (int m = 0; m < w->outputs; m++) {
        WideOut &o = w->outs[m];
        o.stream = cfg->stream_of_output[m]; o.nseg = 1;
        o.seg[0] = WideSeg{0, 0, (int32_t)pmod(w->cur[m], w->Rw)};      // P starts at 0
        list[(size_t)fill[o.stream]++] = m;
        wide_fold_taps(w, w->cur[m], taps.data() + (size_t)m * w->T);
    }
    std::vector<float2> rot((size_t)W_RATE0);                            // the oscillator table at the narrow rate (oscillator.cpp:26-35)
    for (int i = 0; i < W_RATE0; i++) rot[i] = make_float2((float)std::cos(2.0 * design::kPi * i / W_RATE0), (float)std::sin(2.0 * design::kPi * i / W_RATE0));
    HIPCHK(hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&w->ev_in, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&w->ev_out, hipEventDisableTiming));
    DevMem &M = w->mem;
    FMXCHK(M.alloc(w->d_hist[0], (size_t)w->streams * W_HIST, true));    // samples before the first call are zero
    FMXCHK(M.alloc(w->d_hist[1], (size_t)w->streams * W_HIST, true));
    FMXCHK(M.upload(w->d_taps, taps));
    FMXCHK(M.upload(w->d_h, w->h));
    FMXCHK(M.upload(w->d_rot, rot));
    if (rate) FMXCHK(M.upload(w->d_phases, phases));
    FMXCHK(M.upload(w->d_first, first));
    FMXCHK(M.upload(w->d_list, list));
    FMXCHK(M.alloc(w->d_outs, (size_t)w->outputs));
    return FMX_OK;
}

// the head of a call: offsets that changed since the last one begin a new run at this call's first sample; runs that have left every window go
int wide_flush(fmx_wideband w, hipStream_t s) {
    std::vector<int32_t> want;
    { std::lock_guard<std::mutex> lk(w->mtx); want = w->want; }
    const int64_t c = w->g0;
    if (w->multi > 0) {
        w->multi = 0;
        for (auto &o : w->outs) {
            if (o.nseg <= 1) continue;
            while (o.nseg > 1 && o.seg[o.nseg - 2].nbase <= c - (w->T - 1)) { o.nseg--; w->outs_dirty = true; }
            if (o.nseg > 1) w->multi++;
        }
    }
    std::vector<float2> g((size_t)w->T);
    for (int m = 0; m < w->outputs; m++) {
        if (want[m] == w->cur[m]) continue;
        WideOut &o = w->outs[m];
        const int32_t fm = (int32_t)pmod(want[m], w->Rw);
        if (o.seg[0].nbase == c) o.seg[0].f = fm;                        // no sample was mixed with the offset it replaces
        else {
            const WideSeg &z = o.seg[0];
            const int64_t p = pmod((int64_t)z.pbase - pmod(c - z.nbase, w->Rw) * (int64_t)z.f, w->Rw);    // P [c - 1]: the phase is kept
            if (o.nseg == 1) w->multi++;
            if (o.nseg < W_MAX_SEG) o.nseg++;
            for (int k = o.nseg - 1; k > 0; k--) o.seg[k] = o.seg[k - 1];
            o.seg[0] = WideSeg{c, (int32_t)p, fm};
        }
        w->cur[m] = want[m];
        wide_fold_taps(w, want[m], g.data());
        HIPCHK(hipMemcpyAsync(w->d_taps + (size_t)m * w->T, g.data(), sizeof(float2) * g.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (g is reused; an offset change is a rare event)
        w->outs_dirty = true;
    }
    if (w->outs_dirty) {
        HIPCHK(hipMemcpyAsync(w->d_outs, w->outs.data(), sizeof(WideOut) * w->outs.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));                                 // (the mirror may change at the next call's head)
        w->outs_dirty = false;
    }
    return FMX_OK;
}

// the outputs the next call of n_wide samples produces
int64_t wide_outputs_for(const fmx_wideband_s *w, int64_t n_wide) {
    return w->rate.L ? wrate::count(w->g0, n_wide, w->rate.L, w->rate.M) : n_wide / w->K;
}

int wide_check_call(fmx_wideband w, int32_t fmt, float s16_den, int64_t wide_stride, int64_t n_wide, int64_t narrow_stride) {
    if (const ParamCheck pc = check_iq_format(fmt, s16_den); pc.code) return fail(pc.code, pc.msg);
    if (w->rate.L) {
        if (n_wide < 0 || (n_wide > 0 && n_wide < w->rate.min_call)) return fail(FMX_E_INVALID, "n_wide must be 0 or at least ceil (M / L)");
        if (n_wide > w->max_block) return fail(FMX_E_TOO_LARGE, "n_wide > max_block");
        if (wide_stride < n_wide) return fail(FMX_E_INVALID, "wide_stride < n_wide");
        if (narrow_stride < wide_outputs_for(w, n_wide)) return fail(FMX_E_INVALID, "narrow_stride < the call's outputs (fmx_wideband_outputs_for)");
        return FMX_OK;
    }
    if (n_wide < 0 || n_wide % w->K != 0) return fail(FMX_E_INVALID, "n_wide must be a multiple of factor");
    if (n_wide > w->max_block) return fail(FMX_E_TOO_LARGE, "n_wide > max_block");
    if (wide_stride < n_wide) return fail(FMX_E_INVALID, "wide_stride < n_wide");
    if (narrow_stride < n_wide / w->K) return fail(FMX_E_INVALID, "narrow_stride < n_wide / factor");
    return FMX_OK;
}

// the band survey's share of a call, behind wide_kernel on the call's stream: which blocks and records the call completes is survey::plan's
// integer arithmetic; the event is what fmx_wideband_survey_read waits on
int survey_run(fmx_wideband w, const WideArgs &W, hipStream_t s) {
    const survey::Plan p = survey::plan(w->sv_fill, W.n_wide, w->sv_blocks, w->sv_B);
    if (p.blocks > w->sv_cap) return fail(FMX_E_TOO_LARGE, "survey: the call completes more blocks than max_block allows");
    SurveyArgs A{};
    A.src = W.src; A.fmt = W.fmt; A.qs = W.qs; A.src_stride = W.src_stride; A.n_wide = W.n_wide;
    A.blocks = p.blocks; A.fill = w->sv_fill; A.fill_after = p.fill;
    A.phase = p.phase; A.B = w->sv_B; A.slot0 = (int32_t)(p.record0 % survey::RING); A.fresh = w->sv_fresh ? 1 : 0;
    A.scale = w->sv_scale; A.power_stride = w->sv_cap;
    A.window = w->d_sv_win; A.W = w->d_sv_W; A.carry = w->d_sv_carry; A.power = w->d_sv_power; A.acc = w->d_sv_acc; A.ring = w->d_sv_ring;
    g_launch_err = hipSuccess;
    launch_survey(A, w->streams, s);
    if (g_launch_err != hipSuccess) return fail(FMX_E_HIP, std::string("survey kernels: ") + hipGetErrorString(g_launch_err));
    HIPCHK(hipEventRecord(w->ev_sv, s));
    w->ev_sv_set = true;
    w->sv_fill = p.fill; w->sv_blocks += p.blocks; w->sv_fresh = false;
    return FMX_OK;
}

int wide_run(fmx_wideband w, const void *d_wide, int32_t fmt, float s16_den, int64_t wide_stride, int64_t n_wide, float2 *d_narrow,
             int64_t narrow_stride, hipStream_t s) {
    if (n_wide == 0) return FMX_OK;
    FMXCHK(wide_flush(w, s));
    WideArgs A{};
    A.src = d_wide; A.fmt = fmt; A.qs = fmt == 3 ? 1.0f / s16_den : 1.0f / 128.0f;
    A.src_stride = wide_stride; A.n_wide = n_wide; A.g0 = w->g0;
    if (w->rate.L) {                            // (of A the survey takes the input alone)
        WideRateArgs B{};
        B.src = A.src; B.fmt = A.fmt; B.qs = A.qs; B.src_stride = wide_stride; B.n_wide = n_wide; B.g0 = w->g0;
        B.j0 = wrate::before(w->g0, w->rate.L, w->rate.M); B.n_out = wide_outputs_for(w, n_wide);
        B.dst = d_narrow; B.dst_stride = narrow_stride;
        B.hist_in = w->d_hist[w->parity]; B.hist_out = w->d_hist[w->parity ^ 1];
        B.Rw = (int32_t)w->Rw; B.L = (int32_t)w->rate.L; B.M = (int32_t)w->rate.M; B.NP = w->rate.NP;
        B.phases = w->d_phases; B.rot = w->d_taps; B.outs = w->d_outs; B.first = w->d_first; B.list = w->d_list;
        g_launch_err = hipSuccess;
        launch_wide_rate(B, w->streams, s);
        if (g_launch_err != hipSuccess) return fail(FMX_E_HIP, std::string("wide_rate_kernel: ") + hipGetErrorString(g_launch_err));
        if (w->sv_B > 0) FMXCHK(survey_run(w, A, s));
        w->g0 += n_wide; w->parity ^= 1;
        return FMX_OK;
    }
    A.n_out = n_wide / w->K;
    A.dst = d_narrow; A.dst_stride = narrow_stride;
    A.hist_in = w->d_hist[w->parity]; A.hist_out = w->d_hist[w->parity ^ 1];
    A.taps = w->d_taps; A.h = w->d_h; A.rot = w->d_rot; A.outs = w->d_outs; A.first = w->d_first; A.list = w->d_list;
    g_launch_err = hipSuccess;
    launch_wide(A, w->K, w->streams, s);
    if (g_launch_err != hipSuccess) return fail(FMX_E_HIP, std::string("wide_kernel: ") + hipGetErrorString(g_launch_err));
    if (w->sv_B > 0) FMXCHK(survey_run(w, A, s));
    w->g0 += n_wide; w->parity ^= 1;
    return FMX_OK;
}

int wide_create(const fmx_wideband_config *cfg, const wrate::Ratio *rate, fmx_wideband *out) {
    if (!cfg || !out) return fail(FMX_E_INVALID, "null argument");
    FMXCHK(wide_check_config(cfg, rate));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(FMX_E_NO_DEVICE, "no HIP device visible: libfmx has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(FMX_E_INVALID, "device ordinal out of range");
    HIPCHK(hipSetDevice(cfg->device));
    fmx_wideband w = new (std::nothrow) fmx_wideband_s();
    if (!w) return fail(FMX_E_NOMEM, "out of host memory");
    if (const int rc = wide_init(w, cfg, rate)) { const std::string msg = g_err; (void)fmx_wideband_destroy(w); g_err = msg; return rc; }
    *out = w;
    return FMX_OK;
}

}  // namespace

extern "C" {

int fmx_wideband_taps(int32_t factor, float *dst, int32_t capacity, int32_t *n) {
    if (factor < W_MIN_K || factor > W_MAX_K) return fail(FMX_E_INVALID, "factor must be in [2, 16]");
    if (!dst && capacity > 0) return fail(FMX_E_INVALID, "null argument");
    const std::vector<float> h = wide_lowpass(factor);
    if (n) *n = (int32_t)h.size();
    if (capacity < (int32_t)h.size()) return fail(FMX_E_TOO_LARGE, "capacity < 16 * factor + 1");
    std::copy(h.begin(), h.end(), dst);
    return FMX_OK;
}

int fmx_wideband_rate_taps(int32_t wide_rate_hz, float *dst, int32_t capacity, int32_t *n, int32_t *L_out, int32_t *M_out) {
    const char *why = "";
    wrate::Ratio r;
    if (wrate::ratio_of(wide_rate_hz, &r, &why)) return fail(FMX_E_INVALID, why);
    if (!dst && capacity > 0) return fail(FMX_E_INVALID, "null argument");
    if (n) *n = r.NH;
    if (L_out) *L_out = (int32_t)r.L;
    if (M_out) *M_out = (int32_t)r.M;
    if (capacity < r.NH) return fail(FMX_E_TOO_LARGE, "capacity < 16 M + 1");
    const std::vector<float> H = wrate::prototype(r);
    std::copy(H.begin(), H.end(), dst);
    return FMX_OK;
}

int64_t fmx_wideband_outputs_for(fmx_wideband w, int64_t n_wide) {
    if (!w || n_wide < 0) return 0;
    return wide_outputs_for(w, n_wide);
}

int fmx_wideband_create(const fmx_wideband_config *cfg, fmx_wideband *out) { return wide_create(cfg, nullptr, out); }

int fmx_wideband_create_rate(const fmx_wideband_config *cfg, int32_t wide_rate_hz, fmx_wideband *out) {
    if (!cfg || !out) return fail(FMX_E_INVALID, "null argument");
    const char *why = "";
    wrate::Ratio r;
    if (wrate::ratio_of(wide_rate_hz, &r, &why)) return fail(FMX_E_INVALID, why);
    return wide_create(cfg, &r, out);
}

int fmx_wideband_destroy(fmx_wideband w) {
    if (!w) return FMX_OK;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    if (w->rd_stream) { (void)hipStreamSynchronize(w->rd_stream); (void)hipStreamDestroy(w->rd_stream); }
    for (hipEvent_t e : {w->ev_in, w->ev_out, w->ev_sv}) if (e) (void)hipEventDestroy(e);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    w->mem.release_all();
    delete w;
    return FMX_OK;
}

int fmx_wideband_set_offset(fmx_wideband w, int32_t output, int32_t hz) {
    if (!w) return fail(FMX_E_INVALID, "null handle");
    if (output < 0 || output >= w->outputs) return fail(FMX_E_INVALID, "output out of range");
    const int64_t lim = w->Rw / 2 - 150000;
    if (hz > lim || hz < -lim) return fail(FMX_E_INVALID, w->rate.L ? "offset: |f| must be <= wide_rate_hz / 2 - 150000" : "offset: |f| must be <= factor * 1152000 - 150000");
    std::lock_guard<std::mutex> lk(w->mtx);
    w->want[(size_t)output] = hz;
    return FMX_OK;
}

int fmx_wideband_process_device_raw(fmx_wideband w, const void *d_wide, int32_t format, float s16_denominator, int64_t wide_stride, int64_t n_wide,
                                    float *d_narrow, int64_t narrow_stride, int64_t *n_narrow, void *hip_stream) {
    if (!w || !d_wide || !d_narrow) return fail(FMX_E_INVALID, "null argument");
    FMXCHK(wide_check_call(w, format, s16_denominator, wide_stride, n_wide, narrow_stride));
    HIPCHK(hipSetDevice(w->device));
    const int64_t n_out = wide_outputs_for(w, n_wide);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : w->stream;
    if (!hip_stream) {                          // as fmx_process_device: behind what HIP's default stream holds now ...
        HIPCHK(hipEventRecord(w->ev_in, nullptr));
        HIPCHK(hipStreamWaitEvent(w->stream, w->ev_in, 0));
    }
    FMXCHK(wide_run(w, d_wide, format, s16_denominator, wide_stride, n_wide, reinterpret_cast<float2 *>(d_narrow), narrow_stride, s));
    if (!hip_stream) {                          // ... and the default stream behind this call, so that an fmx_process_device (.., NULL) that follows finds its input
        HIPCHK(hipEventRecord(w->ev_out, w->stream));
        HIPCHK(hipStreamWaitEvent(nullptr, w->ev_out, 0));
    }
    if (n_narrow) *n_narrow = n_out;
    return FMX_OK;
}

int fmx_wideband_process_host_raw(fmx_wideband w, const void *wide, int32_t format, float s16_denominator, int64_t wide_stride, int64_t n_wide,
                                  float *narrow, int64_t narrow_stride, int64_t *n_narrow) {
    if (!w || !wide || !narrow) return fail(FMX_E_INVALID, "null argument");
    FMXCHK(wide_check_call(w, format, s16_denominator, wide_stride, n_wide, narrow_stride));
    HIPCHK(hipSetDevice(w->device));
    const int64_t cap = w->rate.L ? wrate::before(w->max_block, w->rate.L, w->rate.M) + 1 : w->max_block / w->K;   // (a rate object: floor (n L / M) or one more)
    const int64_t n_out = wide_outputs_for(w, n_wide);
    if (!w->d_in) {
        FMXCHK(w->mem.alloc(w->d_in, (size_t)w->streams * (size_t)w->max_block * 8));    // sized for the widest format
        FMXCHK(w->mem.alloc(w->d_out, (size_t)w->outputs * (size_t)cap));
    }
    if (n_narrow) *n_narrow = n_out;
    if (n_wide == 0) return FMX_OK;
    const size_t bps = (size_t)bytes_per_sample(format);
    HIPCHK(hipMemcpy2DAsync(w->d_in, bps * w->max_block, wide, bps * wide_stride, bps * n_wide, w->streams, hipMemcpyHostToDevice, w->stream));
    FMXCHK(wide_run(w, w->d_in, format, s16_denominator, w->max_block, n_wide, w->d_out, cap, w->stream));
    HIPCHK(hipMemcpy2DAsync(narrow, sizeof(float2) * narrow_stride, w->d_out, sizeof(float2) * cap, sizeof(float2) * n_out, w->outputs,
                            hipMemcpyDeviceToHost, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    return FMX_OK;
}

int fmx_wideband_survey_enable(fmx_wideband w, int32_t blocks_per_record) {
    if (!w) return fail(FMX_E_INVALID, "null handle");
    if (blocks_per_record < 0 || blocks_per_record > survey::MAX_B) return fail(FMX_E_INVALID, "blocks_per_record must be in [0, 4096]");
    if (blocks_per_record > 0 && !w->d_sv_ring) {
        HIPCHK(hipSetDevice(w->device));
        w->sv_win.resize(survey::N);
        survey::make_window(w->sv_win.data());
        std::vector<float2> W(survey::N);
        survey::make_twiddles(W.data());
        w->sv_cap = (w->max_block + survey::N - 1) / survey::N;          // (a carry of at most 4095 samples and max_block more)
        w->sv_read.assign((size_t)w->streams, 0);
        if (!w->ev_sv) HIPCHK(hipEventCreateWithFlags(&w->ev_sv, hipEventDisableTiming));
        if (!w->rd_stream) HIPCHK(hipStreamCreateWithFlags(&w->rd_stream, hipStreamNonBlocking));
        DevMem &M = w->mem;
        FMXCHK(M.upload(w->d_sv_win, w->sv_win));
        FMXCHK(M.upload(w->d_sv_W, W));
        FMXCHK(M.alloc(w->d_sv_carry, (size_t)w->streams * survey::N));
        FMXCHK(M.alloc(w->d_sv_power, (size_t)w->streams * (size_t)w->sv_cap * survey::N));
        FMXCHK(M.alloc(w->d_sv_acc, (size_t)w->streams * survey::N));
        FMXCHK(M.alloc(w->d_sv_ring, (size_t)w->streams * survey::RING * survey::N));   // (the last allocation: the test above)
    }
    w->sv_B = blocks_per_record;
    if (blocks_per_record > 0) {                                          // a new survey from the next call on
        w->sv_fill = 0; w->sv_blocks = 0; w->sv_g0 = w->g0; w->sv_fresh = true;
        w->sv_scale = survey::record_scale(w->sv_win.data(), blocks_per_record);
        std::fill(w->sv_read.begin(), w->sv_read.end(), 0);
    }
    return FMX_OK;
}

int fmx_wideband_survey_read(fmx_wideband w, int32_t stream, fmx_survey_record *recs, float *power, int32_t capacity, int32_t *n_records) {
    if (!w || !n_records) return fail(FMX_E_INVALID, "null argument");
    *n_records = 0;
    if (stream < 0 || stream >= w->streams) return fail(FMX_E_INVALID, "stream out of range");
    if (capacity < 0 || (capacity > 0 && (!recs || !power))) return fail(FMX_E_INVALID, "null argument");
    if (w->sv_B <= 0) return FMX_OK;
    const int64_t done = w->sv_blocks / w->sv_B;
    const int64_t first = std::max(w->sv_read[(size_t)stream], done - survey::RING);   // (older ones were overwritten: the gap shows in `index`)
    const int64_t n = std::min<int64_t>(capacity, done - first);
    if (n <= 0) return FMX_OK;
    HIPCHK(hipSetDevice(w->device));
    if (w->ev_sv_set) HIPCHK(hipStreamWaitEvent(w->rd_stream, w->ev_sv, 0));          // the object's last call, not the device
    for (int64_t i = 0; i < n; i++) {
        const int64_t r = first + i;
        recs[i] = fmx_survey_record{r, w->sv_g0 + (r + 1) * (int64_t)w->sv_B * survey::N, w->sv_B, 0};
        HIPCHK(hipMemcpyAsync(power + (size_t)i * survey::N, w->d_sv_ring + ((size_t)stream * survey::RING + (size_t)(r % survey::RING)) * survey::N,
                              sizeof(float) * survey::N, hipMemcpyDeviceToHost, w->rd_stream));
    }
    HIPCHK(hipStreamSynchronize(w->rd_stream));
    w->sv_read[(size_t)stream] = first + n;
    *n_records = (int32_t)n;
    return FMX_OK;
}

int fmx_wideband_survey_stations(const fmx_survey_find *cfg, const float *power, fmx_survey_station *out, int32_t capacity, int32_t *n_stations,
                                 float *floor_db) {
    const char *why = "";
    const int rc = survey::find(cfg, 0, power, out, capacity, n_stations, floor_db, &why);
    return rc == FMX_OK ? FMX_OK : fail(rc, why);
}

int fmx_wideband_survey_stations_rate(const fmx_survey_find *cfg, int32_t wide_rate_hz, const float *power, fmx_survey_station *out, int32_t capacity,
                                      int32_t *n_stations, float *floor_db) {
    const char *why = "";
    wrate::Ratio r;
    if (wrate::ratio_of(wide_rate_hz, &r, &why)) return fail(FMX_E_INVALID, why);
    const int rc = survey::find(cfg, r.Rw, power, out, capacity, n_stations, floor_db, &why);
    return rc == FMX_OK ? FMX_OK : fail(rc, why);
}

}  // extern "C"

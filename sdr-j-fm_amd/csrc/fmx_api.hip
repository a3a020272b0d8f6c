// fmx_api.hip -- the handle of libfmx's C ABI (include/fmx.h) and its call path: create / destroy, the settings mailbox, table/tap design + upload, the
// block machines, promotion and demotion, per-call geometry and the kernel launches.  A handle's device and pinned memory has one owner (DevMem,
// fmx_host.h): fmx_destroy names no buffer.  What a handle's settings mean for its next call is decided in fmx_needs.h, how the call becomes launches
// in fmx_plan.h (both pure, checked on the CPU); here are the locks, allocations, uploads and launches.  The entry points that only read a handle are
// in fmx_readout.hip, stage W's in fmx_wide_api.hip, the diagnostics in fmx_diag.hip.  No CPU fallback exists: every entry point fails when HIP is
// unavailable.
#include "fmx_host.h"
#include "fmx_fftconv.h"
#include "fmx_design.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

thread_local std::string fmx::host::g_err;

namespace {

int env_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
// The FMX_* environment switches (diagnostics: the runs two GPU tests compare the default schedule with; none is needed by a user): read ONCE, by the
// first fmx_create of the process -- nothing on the per-call path asks the environment.
struct EnvSwitches {
    bool pieces_serial;   // FMX_CALL_PIECES_SERIAL=1: the pieces of an overlapping call one after the other on the caller's stream
    bool tail_split;      // FMX_TAIL_SPLIT=0: stages B and C as one channel group
};
const EnvSwitches &env_switches() {
    static const EnvSwitches sw{env_int("FMX_CALL_PIECES_SERIAL", 0) != 0, env_int("FMX_TAIL_SPLIT", 1) != 0};
    return sw;
}

int next_pow2(int64_t v) { int64_t p = 1; while (p < v) p <<= 1; return (int)p; }

// ---- tap-set construction -----------------------------------------------------------------
// Front end = inputFilter (optional) * fmBand_1 * fmBand_2 folded into one real polyphase FIR evaluated by stage A's /12 kernel.
// `decim` = the reference's total decimation at this input rate (12: both decimators; 6: fmBand_2 does not decimate; 1: no decimators
// at all, fm-processor.cpp:471), `twins` = 12 / decim, `p` = which of the twins this set is for: twin p computes the outputs
// j = twins * m + p, whose newest input decim * j + decim - 1 - L = 12 (m - delay_p) + off_p.  Returns delay_p.
int build_front_set(int32_t bw, int32_t inputRate, int32_t fmRate, int decim, int p, float *taps /*A_TAPS_STRIDE*/, FrontSet *fs) {
    std::vector<double> g(1, 1.0);
    double S1 = 0.0, S2 = 0.0;
    if (decim > 1) {
        const int32_t IRate = inputRate / 6;                                       // fm-processor.cpp:36
        design::DecimKernel k1 = design::decim(4 * inputRate / IRate + 1, fmRate / 2, inputRate);   // :68-71
        design::DecimKernel k2 = design::decim(IRate / fmRate + 1, fmRate / 2, IRate);              // :72-75 (decimation IRate / fmRate: 2 or 1)
        const int D1 = inputRate / IRate;                                          // 6
        // y[m] = sum k1[l] x[6m+5-l]; z[j] = sum k2[i] y[D2 j + D2 - 1 - i]  (fir-filters.cpp:397-424)
        //  => z[j] = sum_k g[k] x[decim j + decim - 1 - k],  g[k] = sum_{D1*i+l=k} h2[i] h1[l]
        g.assign((size_t)(D1 * (k2.hn.size() - 1) + k1.hn.size()), 0.0);
        for (size_t i = 0; i < k2.hn.size(); i++)
            for (size_t l = 0; l < k1.hn.size(); l++) g[D1 * i + l] += (double)k2.hn[i] * (double)k1.hn[l];
        S1 = k1.sum; S2 = k2.sum;
    }
    int L = 0;                                                                 // overlap-add latency in input samples
    if (bw > 0) {
        // inputFilter.setLowPass(fmBandwidth / 2, inputRate), fftFilter(2*32768, 251) (:77,398)
        std::vector<float> hin = design::lowpass(251, bw / 2, inputRate);
        g = design::convolve(g, design::to_double(hin));
        L = 2 * 32768 - 251;                                                   // NumofSamples fft-filters.cpp:34
    }
    const int NT = (int)g.size();
    // newest input of this twin's output column m: 12 (m - delay) + off
    const int64_t e = (int64_t)decim * p + decim - 1 - L;
    int64_t delay = -(e >= 0 ? e / 12 : -((-e + 11) / 12));
    const int off = (int)(e + 12 * delay);
    fs->off = off; fs->delay_fm = (int32_t)delay; fs->zshift = 0;
    int nd = 0;
    std::fill(taps, taps + A_TAPS_STRIDE, 0.f);
    for (int d = 0; d < A_MAX_ND; d++)
        for (int r = 0; r < DECIM; r++) {
            const int k = 12 * d + off - r;
            if (k >= 0 && k < NT) { taps[(d + 1) * DECIM + r] = (float)g[k]; nd = d + 1; }
        }
    fs->nd = nd;
    // complex gain of the (h/sum, h) kernels: (1 + j S1)(1 + j S2)  (fir-filters.cpp:345-346); 1 without the decimators
    fs->gain_re = (float)(1.0 - S1 * S2); fs->gain_im = (float)(S1 + S2);
    // the FIR's response to the slowly moving RfDC value: sum of the taps (as the kernel sums them: f32 taps) times the value at
    // the taps' centre of mass.  Output column q has its newest input at sample 12 q + off; "RfDC applied to sample s" is the state
    // behind s, interpolated between the column boundaries: boundary column q - dc_k, weight dc_w towards the next boundary.
    double hs = 0, mk = 0;
    for (int d = 0; d < A_MAX_ND; d++)
        for (int r = 0; r < DECIM; r++) {
            const double v = (double)taps[(d + 1) * DECIM + r];
            hs += v; mk += v * (double)(12 * d + off - r);
        }
    fs->hsum = (float)hs;
    const double q0 = (double)off - mk / hs + 1.0;
    const int K = -(int)std::floor(q0 / 12.0);
    fs->dc_k = K; fs->dc_w = (float)((q0 + 12.0 * K) / 12.0);
    return (int)delay;
}

void build_audio_set(int32_t lf, int32_t fmRate, const std::vector<float> &rs, float *taps /*C_TAPS_STRIDE*/, AudioSet *as) {
    std::vector<double> g = design::to_double(rs);
    as->delay = 0;
    if (lf > 0) {
        // fmAudioFilter.setLowPass(lowPassFrequency, fmRate), fftFilter(2*4096, 756) (:76,404)
        std::vector<float> ha = design::lowpass(AUDIO_TAPS, lf, fmRate);
        g = design::convolve(design::to_double(ha), g);
        as->delay = AUDIO_DELAY;
    }
    as->ntaps = (int)g.size();
    std::fill(taps, taps + C_TAPS_STRIDE, 0.f);
    for (int kk = 0; kk < as->ntaps; kk++) taps[kk] = (float)g[as->ntaps - 1 - kk];   // reversed
}

}  // namespace

int fmx::host::ensure_sets(fmx_handle h) {
    // deduplicate bandwidth / lf-cutoff values into tap sets, upload when changed
    std::vector<int32_t> fk, ak;
    for (int c = 0; c < h->channels; c++) {
        int32_t b = h->user[c].bw_applied, l = h->user[c].lf_applied > 0 ? h->user[c].lf_applied : 0;      // (folded handles: see ChanUser)
        if (h->ola_mode) { b = 0; l = 0; }      // (the two filters run as block machines in front of stage A's decimators / stage C's resampler)
        auto it = std::find(fk.begin(), fk.end(), b);
        if (it == fk.end()) { fk.push_back(b); it = fk.end() - 1; }
        h->params[c].front_set = (int)(it - fk.begin()) * h->twins;          // (index of the channel's first twin set)
        auto ia = std::find(ak.begin(), ak.end(), l);
        if (ia == ak.end()) { ak.push_back(l); ia = ak.end() - 1; }
        h->params[c].audio_set = (int)(ia - ak.begin());
    }
    if (fk != h->front_keys) {
        h->front_keys = fk;
        const size_t TW = (size_t)h->twins, NS = fk.size() * TW;              // one tap set per bandwidth value and twin
        h->h_front_taps.assign(NS * A_TAPS_STRIDE, 0.f);
        h->h_front_sets.resize(NS);
        for (size_t i = 0; i < fk.size(); i++) {
            int dmin = 0x7fffffff;
            std::vector<int> dl(TW);
            for (size_t p = 0; p < TW; p++) {
                dl[p] = build_front_set(fk[i], h->cfg.inputRate, h->cfg.fmRate, h->decim, (int)p, &h->h_front_taps[(i * TW + p) * A_TAPS_STRIDE], &h->h_front_sets[i * TW + p]);
                dmin = std::min(dmin, dl[p]);
            }
            // fm sample j sits at ring position j - delay_fm: twin p's column m is j = TW (m + delay_p) + p
            for (size_t p = 0; p < TW; p++) { h->h_front_sets[i * TW + p].zshift = dl[p] - dmin; h->h_front_sets[i * TW + p].delay_fm = (int32_t)(TW * (size_t)dmin); }
        }
        if ((int)NS > h->front_cap) {
            h->mem.release(h->d_front_taps); h->mem.release(h->d_front_sets);
            h->front_cap = std::max<int>((int)NS, 4);
            FMXCHK(h->mem.alloc(h->d_front_taps, (size_t)A_TAPS_DEV * h->front_cap));
            FMXCHK(h->mem.alloc(h->d_front_sets, (size_t)h->front_cap));
        }
        HIPCHK(hipDeviceSynchronize());
        std::vector<float> dev(NS * A_TAPS_DEV, 0.f);                    // device image: [set][r][d]
        for (size_t i = 0; i < NS; i++)
            for (int d = 0; d < A_MAX_ND; d++)
                for (int r = 0; r < DECIM; r++)
                    dev[i * A_TAPS_DEV + r * A_TAPS_ROW + d] = h->h_front_taps[i * A_TAPS_STRIDE + (d + 1) * DECIM + r];
        HIPCHK(hipMemcpy(h->d_front_taps, dev.data(), sizeof(float) * dev.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_front_sets, h->h_front_sets.data(), sizeof(FrontSet) * NS, hipMemcpyHostToDevice));
        h->T.front_taps = h->d_front_taps; h->T.front_sets = h->d_front_sets;
    }
    if (ak != h->audio_keys) {
        h->audio_keys = ak;
        h->h_audio_taps.assign(ak.size() * C_TAPS_STRIDE, 0.f);
        h->h_audio_sets.resize(ak.size());
        for (size_t i = 0; i < ak.size(); i++)
            build_audio_set(ak[i], h->cfg.fmRate, h->h_rs_taps, &h->h_audio_taps[i * C_TAPS_STRIDE], &h->h_audio_sets[i]);
        if ((int)ak.size() > h->audio_cap) {
            h->mem.release(h->d_audio_taps); h->mem.release(h->d_audio_sets);
            h->audio_cap = std::max<int>((int)ak.size(), 4);
            FMXCHK(h->mem.alloc(h->d_audio_taps, (size_t)C_TAPS_STRIDE * h->audio_cap));
            FMXCHK(h->mem.alloc(h->d_audio_sets, (size_t)h->audio_cap));
        }
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(h->d_audio_taps, h->h_audio_taps.data(), sizeof(float) * h->h_audio_taps.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_audio_sets, h->h_audio_sets.data(), sizeof(AudioSet) * ak.size(), hipMemcpyHostToDevice));
        h->T.audio_taps = h->d_audio_taps; h->T.audio_sets = h->d_audio_sets;
        {   // the two factors of the folded FIR, separately (gain_fix_kernel)
            std::vector<float> lp(ak.size() * AUDIO_TAPS, 0.f);
            for (size_t i = 0; i < ak.size(); i++) if (ak[i] > 0) { const std::vector<float> ha = design::lowpass(AUDIO_TAPS, ak[i], h->cfg.fmRate); std::copy(ha.begin(), ha.end(), lp.begin() + i * AUDIO_TAPS); }
            h->mem.release(h->T.audio_lp_taps);
            FMXCHK(h->mem.upload(h->T.audio_lp_taps, lp));
            if (!h->T.rs_taps) FMXCHK(h->mem.upload(h->T.rs_taps, h->h_rs_taps));
            // spectra of the four decimation phases g_p[i] = g[4 i + p] of the folded FIR (audio_fft_kernel); h_audio_taps holds g reversed
            std::vector<float2> W(fftc::W_COUNT), spec(ak.size() * 4 * fftc::N);
            fftc::make_twiddles(W.data());
            for (size_t i = 0; i < ak.size(); i++) {
                const int nt = h->h_audio_sets[i].ntaps;
                const float *rev = &h->h_audio_taps[i * C_TAPS_STRIDE];
                for (int p = 0; p < 4; p++) {
                    std::vector<float> gp;
                    for (int kk = p; kk < nt; kk += 4) gp.push_back(rev[nt - 1 - kk]);
                    fftc::make_spectrum(gp.data(), (int)gp.size(), &spec[(i * 4 + p) * fftc::N], W.data());
                }
            }
            h->mem.release(h->T.audio_spec);
            FMXCHK(h->mem.upload(h->T.audio_spec, spec));
        }
    }
    h->sets_dirty = false;
    return FMX_OK;
}

namespace {

void refresh_derived(fmx_handle h, int c) {
    // the arithmetic of the setters themselves
    const ChanUser &u = h->user[c];
    ChanParams &p = h->params[c];
    const int32_t fmRate = h->cfg.fmRate;
    if (u.deemph_us >= 1) {                     // setDeemphasis fm-processor.cpp:291-297 (Tau is float)
        const float Tau = (float)(1000000.0 / u.deemph_us);
        p.deemph_alpha = (float)(1.0 / ((double)((float)fmRate / Tau) + 1.0));
    } else {                                    // ctor :174
        p.deemph_alpha = (float)(1.0 / (fmRate / (1000000.0 / 50.0 + 1)));
    }
    p.deemph_l2 = (float)std::log2((double)(1.0f - p.deemph_alpha));
    p.volume = u.ctor_volume ? 0.5f : std::pow(10.0f, u.volume_db / 20.0f);        // :127, :299-301
    p.left_ch = (u.balance > 0 ? (float)((100 - u.balance) / 100.0) : 1.0f);       // :282-286
    p.right_ch = (u.balance < 0 ? (float)((100 + u.balance) / 100.0) : 1.0f);
    p.panorama = (float)(int16_t)u.panorama / 100.0f;                               // :277-280
}

int ensure_lo_table(fmx_handle h) {
    if (h->T.lo_table) return FMX_OK;
    const int32_t R = h->cfg.inputRate;
    std::vector<float2> tab((size_t)R);
    for (int32_t i = 0; i < R; i++)             // Oscillator ctor oscillator.cpp:26-35
        tab[i] = make_float2((float)std::cos(2.0 * design::kPi * i / R), (float)std::sin(2.0 * design::kPi * i / R));
    return h->mem.upload(h->T.lo_table, tab);
}

int ensure_rds_body(fmx_handle h);
int ensure_rds(fmx_handle h) {
    if (h->rds_alloc) return FMX_OK;
    const int rc = ensure_rds_body(h);
    if (rc) { h->rds_mem.release_all(); h->R = RdsBuffers{}; h->d_rds_nc0 = nullptr; h->rds_stage = nullptr; }      // partial failure: give everything back, the next enable tries again
    return rc;
}
int ensure_rds_body(fmx_handle h) {
    const size_t C = (size_t)h->channels;
    const int32_t fmRate = h->cfg.fmRate;
    DevMem &M = h->rds_mem;
    RdsBuffers &R = h->R;
    FMXCHK(M.alloc(R.in_blk, C * RDS_BLK, true));
    FMXCHK(M.alloc(R.bpreal, C * 2 * RDS_BLK, true));
    FMXCHK(M.alloc(R.bp_over, 2 * C * 768, true));
    FMXCHK(M.alloc(R.hil, C * 2 * RDS_BLK, true));
    FMXCHK(M.alloc(R.hil_over, 2 * C * 768, true));
    FMXCHK(M.alloc(R.phase_ring, C * RDS_PHASE_RING, true));
    FMXCHK(M.alloc(R.U, C * 32768));
    FMXCHK(M.alloc(R.V, C * 32768));
    FMXCHK(M.alloc(R.rds24, C * RDS24_RING, true));
    R.pitch = h->pitch;
    FMXCHK(M.alloc(R.mf, (size_t)(h->work_nj / 8 + 8) * h->pitch));
    R.mfc_stride = ((h->work_nj / 8 + 8 + 2 + 7) / 8) * 8;
    FMXCHK(M.alloc(R.mfc, (size_t)R.mfc_stride * C, true));
    FMXCHK(M.alloc(R.mfm, (size_t)R.mfc_stride * C, true));
    FMXCHK(M.alloc(R.bits, C * RDS_BITS_CAP, true));
    FMXCHK(M.alloc(R.sym, C * RDS_SYM_CAP, true));
    {   // rdsDecoder_2 / AGC / Costas constructor state (rds-decoder-2.cpp:44-78, rds-decoder.cpp:41-43)
        RdsState s0; std::memset(&s0, 0, sizeof(s0));
        s0.gain = 9.0f; s0.mu = 0.f; s0.skip = 3; s0.sample_count = 0;
        s0.c_limit = (float)(2 * design::kPi * (double)10.0f / (double)(float)24000);
        std::vector<RdsState> init(C, s0);
        FMXCHK(M.upload(R.state, init));
    }
    {   // spectra: the DFT of the zero-padded band-pass kernel (fft-filters.cpp:71-82, setBand(57000 -+ 2400)), and the
        // analytic-signal mask of fftFilterHilbert::setHilbert (:177-190)
        const int N = 32768, D = 768;
        std::vector<float> k = design::bandpass(D, 3 * 19000 - 4800 / 2, 3 * 19000 + 4800 / 2, fmRate);
        std::vector<float2> S((size_t)N), Hm((size_t)N);
        std::vector<double> cs((size_t)N), sn((size_t)N);
        for (int i = 0; i < N; i++) { cs[i] = std::cos(-2 * design::kPi * i / N); sn[i] = std::sin(-2 * design::kPi * i / N); }
        for (int f = 0; f < N; f++) {
            double re = 0, im = 0;
            for (int i = 0; i < D; i++) {
                const int a = (int)(((int64_t)f * i) & (N - 1));
                re += (double)k[2 * i] * cs[a] - (double)k[2 * i + 1] * sn[a];
                im += (double)k[2 * i] * sn[a] + (double)k[2 * i + 1] * cs[a];
            }
            S[f] = make_float2((float)re, (float)im);
            Hm[f] = make_float2(f == 0 || f == N / 2 ? 1.0f : (f < N / 2 ? 2.0f : 0.0f), 0.f);
        }
        FMXCHK(M.upload(R.S_bp, S));
        FMXCHK(M.upload(R.S_hil, Hm));
        {   // the band-pass kernel is complex and only the real part of its result is kept (fm-processor.cpp:741): for a real input
            // Re (a * s) = a * Re (s), the DFT of Re (s) is the Hermitian part of S -- the filter vector of the paired transforms
            std::vector<float2> Sr((size_t)N);
            for (int f = 0; f < N; f++) {
                const float2 a = S[(size_t)f], b = S[(size_t)((N - f) & (N - 1))];
                Sr[(size_t)f] = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
            }
            FMXCHK(M.upload(R.S_bp_re, Sr));
        }
        std::vector<float> dk = design::decim_complex(11, 24000 / 2, fmRate);      // rdsDecimator fm-processor.cpp:382
        std::vector<float> rr = design::rrc(1.0, 24000, 2 * 1187.5f, 1.0, 45);       // rds-decoder-2.cpp:67-71
        float2 *dd;                                                                  // (dk: 11 (re, im) pairs as floats)
        FMXCHK(M.alloc(dd, 11));
        FMXCHK(M.upload(R.rrc, rr));
        HIPCHK(hipMemcpy(dd, dk.data(), sizeof(float2) * 11, hipMemcpyHostToDevice));
        R.dec_taps = dd;
    }
    {   // RDS_1: Costas state, rdsFilter / Match / sharpFilter coefficients (rds-decoder-1.cpp:43-100), rings at 24 kS/s
        FMXCHK(M.alloc(R.c_ring, C * RDS24_RING, true));
        FMXCHK(M.alloc(R.f_ring, C * RDS24_RING, true));
        FMXCHK(M.alloc(R.state1, C, true));
        std::vector<float> co = design::lowpass(RDS1_FIR, 2 * 2400, 24000);            // rdsFilter (21, RDS_WIDTH, rate)
        const std::vector<float> mk = design::rds1_match_kernel(24000);
        if ((int)mk.size() != RDS1_MATCH) return fail(FMX_E_HIP, "unexpected length of the RDS_1 matched filter");
        co.insert(co.end(), mk.begin(), mk.end());
        const design::Iir bp = design::iir_butterworth_bandpass(7, (int32_t)(1187.5 - 6), (int32_t)(1187.5 + 6), 24000);   // sharpFilter
        if (bp.nq != RDS1_QUADS) return fail(FMX_E_HIP, "unexpected biquad count of the RDS_1 band-pass");
        for (int i = 0; i < RDS1_QUADS; i++) { co.push_back(bp.q[i][1]); co.push_back(bp.q[i][2]); co.push_back(bp.q[i][4]); co.push_back(bp.q[i][5]); }
        co.push_back(bp.gain);
        FMXCHK(M.upload(R.rds1_coef, co));
        h->h_rds1 = co;
    }
    {   // RDS_3: state, and mySinCos (rate) of rdsDecoder_3 (rds-decoder-3.cpp:49): SinCos ctor sincos.cpp:45-54 at Rate 24000
        FMXCHK(M.alloc(R.state3, C, true));
        std::vector<float2> sc24(24000);
        for (int i = 0; i < 24000; i++) sc24[i] = make_float2((float)std::cos(2 * design::kPi * i / 24000), (float)std::sin(2 * design::kPi * i / 24000));
        FMXCHK(M.upload(R.sincos24, sc24));
    }
    FMXCHK(M.alloc(R.sync, C, true));                                  // (all zero: rdsBlockSynchronizer::reset, nothing read, no group yet)
    FMXCHK(M.alloc(R.groups, C * RDS_GROUP_RING, true));
    if (!h->ev_call) HIPCHK(hipEventCreateWithFlags(&h->ev_call, hipEventDisableTiming));
    h->rd.bits.assign(C, 0);
    {
        FMXCHK(M.alloc(h->d_rds_nc0, C, true));
        FMXCHK(M.alloc(R.chlist, C, true));
        R.nc0 = h->d_rds_nc0;
        h->rds_nc.assign(C, 0); h->rds_nc0.assign(C, -1); h->last_m0.assign(C, 0); h->last_m1.assign(C, 0);
    }
    h->rds_alloc = true;
    return FMX_OK;
}

// ---- the overlap-add block machines (fmx_ola.hip) ----------------------------------------------------------------------------------
int ola_alloc_side(fmx_handle h, fmx_handle_s::OlaSide &S, int L, int degree) {
    const size_t C = (size_t)h->channels;
    S.L = L; S.degree = degree;
    FMXCHK(h->mem.alloc(S.A, C * L, true));
    FMXCHK(h->mem.alloc(S.C, C * L, true));
    FMXCHK(h->mem.alloc(S.over, C * OLA_MAX_TAPS, true));
    FMXCHK(h->mem.alloc(S.over_new, C * OLA_MAX_TAPS, true));
    FMXCHK(h->mem.alloc(S.taps, C * OLA_MAX_TAPS, true));
    S.inp.assign(C, 0); S.on.assign(C, 0); S.key.assign(C, -1);
    return FMX_OK;
}
int ensure_ola(fmx_handle h) {
    if (h->d_v) return FMX_OK;
    const size_t C = (size_t)h->channels;
    FMXCHK(h->mem.alloc(h->d_v, C * h->cfg.max_block));
    FMXCHK(h->mem.alloc(h->d_u, C * h->cfg.max_block));
    FMXCHK(h->mem.alloc(h->d2ring, C * h->dring, true));
    h->pre_look.max_tiles = (int32_t)(h->cfg.max_block / PRE_TILE_SAMPLES + 1);
    FMXCHK(h->mem.alloc(h->pre_look.maps, C * h->pre_look.max_tiles));
    FMXCHK(h->mem.alloc(h->pre_look.flags, C * h->pre_look.max_tiles, true));
    FMXCHK(h->mem.alloc(h->pre_look.tickets, C, true));
    h->pre_look.ticket_base = 0;
    FMXCHK(ola_alloc_side(h, h->ola_in, 2 * 32768 - 251, 251));          // inputFilter (2 * 32768, 251) fm-processor.cpp:77
    return ola_alloc_side(h, h->ola_au, 2 * 4096 - AUDIO_TAPS, AUDIO_TAPS);   // fmAudioFilter (2 * 4096, 756) :76
}
// setBandwidth / setlfcutoff as the reference's loop takes them over at a block start (fm-processor.cpp:396-408): a new value designs the
// kernel and RESTARTS the block position (fftFilter::setLowPass fft-filters.cpp:84-95: inp = 0, buffers kept); "Off" / <= 0 stops using the
// filter, whose buffers stay as they are
int ola_take_settings(fmx_handle h) {
    bool synced = false;
    for (int side = 0; side < 2; side++) {
        fmx_handle_s::OlaSide &S = side ? h->ola_au : h->ola_in;
        for (int c = 0; c < h->channels; c++) {
            const int32_t want = side ? (h->user[c].lf_cutoff > 0 ? h->user[c].lf_cutoff : 0) : (h->user[c].bandwidth > 0 ? h->user[c].bandwidth : 0);
            bool &ev = side ? h->user[c].lf_event : h->user[c].bw_event;
            const bool again = ev && want != 0 && S.key[(size_t)c] >= 0;        // (the value in use selected again: the block restarts, the kernel stays)
            ev = false;
            if (want == S.key[(size_t)c]) { if (again) { S.on[(size_t)c] = 1; S.inp[(size_t)c] = 0; h->last_filter_event_g = h->g_total; } continue; }
            S.key[(size_t)c] = want;
            h->last_filter_event_g = h->g_total;
            if (want == 0) { S.on[(size_t)c] = 0; continue; }
            const std::vector<float> k = side ? design::lowpass(AUDIO_TAPS, want, h->cfg.fmRate) : design::lowpass(251, want / 2, h->cfg.inputRate);
            if (!synced) { HIPCHK(hipDeviceSynchronize()); synced = true; }      // (an earlier call may still be reading the kernels)
            HIPCHK(hipMemcpy(S.taps + (size_t)c * OLA_MAX_TAPS, k.data(), sizeof(float) * k.size(), hipMemcpyHostToDevice));
            S.on[(size_t)c] = 1; S.inp[(size_t)c] = 0;
        }
    }
    return FMX_OK;
}
// one step of every channel's block machine, as the host works it out; step_ref hands it to the launchers
struct HStep { std::vector<OlaChan> ch; };
int step_ref(fmx_handle h, const HStep &st, hipStream_t s, OlaStepRef *out) {
    *out = OlaStepRef{};
    if (h->channels <= OLA_MAX_CH) { for (int c = 0; c < h->channels; c++) out->val.ch[c] = st.ch[(size_t)c]; return FMX_OK; }
    const size_t C = (size_t)h->channels;
    if (!h->step_dev) {
        FMXCHK(h->mem.alloc(h->step_dev, C * fmx_handle_s::STEP_SLOTS));
        FMXCHK(h->mem.alloc_pinned(h->step_host, C * fmx_handle_s::STEP_SLOTS));
        for (auto &e : h->step_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const int k = h->step_next; h->step_next = (k + 1) % fmx_handle_s::STEP_SLOTS;
    if (h->step_used[k]) HIPCHK(hipEventSynchronize(h->step_ev[k]));          // (the copy that last used this slot's host side has run)
    h->step_used[k] = true;
    std::memcpy(h->step_host + (size_t)k * C, st.ch.data(), sizeof(OlaChan) * C);
    HIPCHK(hipMemcpyAsync(h->step_dev + (size_t)k * C, h->step_host + (size_t)k * C, sizeof(OlaChan) * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(h->step_ev[k], s));
    out->tab = h->step_dev + (size_t)k * C;
    return FMX_OK;
}
void ola_fill(const fmx_handle_s::OlaSide &S, OlaBuffers &O) { O.A = S.A; O.C = S.C; O.over = S.over; O.over_new = S.over_new; O.taps = S.taps; O.L = S.L; O.degree = S.degree; }
// does every channel's filter take the whole call as one run (no block boundary before its last sample)?  Then the step is returned and
// the caller's own kernel (pre_kernel / deemph_kernel) does the copy; ola_finish_single runs the block transforms that fall due behind it.
bool ola_single_step(fmx_handle h, const fmx_handle_s::OlaSide &S, int64_t len, HStep *st) {
    st->ch.assign((size_t)h->channels, OlaChan{});
    for (int c = 0; c < h->channels; c++) {
        const bool on = S.on[(size_t)c] != 0;
        if (on && S.inp[(size_t)c] + len > S.L) return false;
        OlaChan &d = st->ch[(size_t)c];
        d.off = 0; d.len = (int32_t)len; d.inp = S.inp[(size_t)c]; d.on = on ? 1 : 0; d.conv = (on && len > 0 && S.inp[(size_t)c] + len == S.L) ? 1 : 0;
    }
    return true;
}
void ola_finish_single(fmx_handle h, fmx_handle_s::OlaSide &S, const HStep &st, const OlaStepRef &ref, const OlaBuffers &O, hipStream_t s) {
    bool any_conv = false;
    for (int c = 0; c < h->channels; c++) any_conv |= st.ch[(size_t)c].conv != 0;
    if (any_conv) { launch_ola_conv(ref, O, h->channels, s); FMX_LAUNCHED(); }
    for (int c = 0; c < h->channels; c++) if (st.ch[(size_t)c].on) S.inp[(size_t)c] = st.ch[(size_t)c].conv ? 0 : S.inp[(size_t)c] + st.ch[(size_t)c].len;
}
// Pass () of every channel over `len` samples: runs up to the block boundary, the block transform where a block completes, and on
int run_ola(fmx_handle h, fmx_handle_s::OlaSide &S, OlaBuffers O, int64_t len, hipStream_t s) {
    ola_fill(S, O);
    std::vector<int64_t> off((size_t)h->channels, 0);
    for (;;) {
        HStep st; st.ch.assign((size_t)h->channels, OlaChan{});
        int maxlen = 0; bool any_conv = false;
        for (int c = 0; c < h->channels; c++) {
            const int64_t rem = len - off[(size_t)c];
            const bool on = S.on[(size_t)c] != 0;
            const int64_t run = on ? std::min<int64_t>(rem, S.L - S.inp[(size_t)c]) : rem;
            OlaChan &d = st.ch[(size_t)c];
            d.off = (int32_t)off[(size_t)c]; d.len = (int32_t)run; d.inp = S.inp[(size_t)c]; d.on = on ? 1 : 0;
            d.conv = (on && run > 0 && S.inp[(size_t)c] + run == S.L) ? 1 : 0;
            maxlen = std::max<int>(maxlen, (int)run); any_conv |= d.conv != 0;
        }
        if (maxlen <= 0) break;
        OlaStepRef ref; { const int rc = step_ref(h, st, s, &ref); if (rc) return rc; }
        launch_ola_io(ref, O, h->channels, maxlen, s); FMX_LAUNCHED();
        if (any_conv) { launch_ola_conv(ref, O, h->channels, s); FMX_LAUNCHED(); }
        for (int c = 0; c < h->channels; c++) {
            const OlaChan &d = st.ch[(size_t)c];
            off[(size_t)c] += d.len;
            if (d.on) S.inp[(size_t)c] = d.conv ? 0 : S.inp[(size_t)c] + d.len;
        }
    }
    return FMX_OK;
}

// the input side of a block-machine handle's call: pre_kernel (RF DC removal, balance, oscillator per sample) and the input filter's machine over the call's
// G.n samples; the machines' output stream is h->d_u
int ola_input_side(fmx_handle h, const CallGeom &G, const DeviceBuffers &B, const void *d_iq, hipStream_t s) {
    OlaBuffers O{}; O.src = h->d_v; O.dst = h->d_u; O.src_stride = O.dst_stride = h->cfg.max_block; O.src_mask = O.dst_mask = -1;
    HStep st1;
    int rc;
    if (ola_single_step(h, h->ola_in, G.n, &st1)) {
        OlaStepRef ref; rc = step_ref(h, st1, s, &ref); if (rc) return rc;
        ola_fill(h->ola_in, O);
        h->pre_look.epoch += 1;
        launch_pre(h->T, B, G, d_iq, h->d_v, h->cfg.max_block, h->channels, s, &ref, &O, h->pre_look); FMX_LAUNCHED();
        { const uint32_t nt = (uint32_t)((G.n + PRE_TILE_SAMPLES - 1) / PRE_TILE_SAMPLES); if (nt > 1) h->pre_look.ticket_base += nt; }
        ola_finish_single(h, h->ola_in, st1, ref, O, s);
    } else {
        h->pre_look.epoch += 1;
        launch_pre(h->T, B, G, d_iq, h->d_v, h->cfg.max_block, h->channels, s, nullptr, nullptr, h->pre_look); FMX_LAUNCHED();
        { const uint32_t nt = (uint32_t)((G.n + PRE_TILE_SAMPLES - 1) / PRE_TILE_SAMPLES); if (nt > 1) h->pre_look.ticket_base += nt; }
        rc = run_ola(h, h->ola_in, O, G.n, s); if (rc) return rc;
    }
    return FMX_OK;
}

// PROMOTION of a folded batch to the block machines at the stream position g_total (fmx_promote.hip has the story).  Rare and heavy: the device is idle around it.
int promote(fmx_handle h, hipStream_t s) {
    std::lock_guard<std::mutex> lk(h->mtx);
    const size_t C = (size_t)h->channels;
    HIPCHK(hipDeviceSynchronize());
    int rc = ensure_ola(h); if (rc) return rc;
    if (h->h_front_sets.size() > h->old_sets_cap) {
        h->mem.release(h->d_old_sets);
        h->old_sets_cap = h->h_front_sets.size() + 8;
        FMXCHK(h->mem.alloc(h->d_old_sets, h->old_sets_cap));
    }
    if (!h->d_old_set_of) {
        FMXCHK(h->mem.alloc(h->d_old_set_of, C));
        FMXCHK(h->mem.alloc(h->d_params_replay, C));
        FMXCHK(h->mem.alloc(h->d_au_tail, C * PROMO_TAIL_AU));
    }
    {   // what the folded stage A used: its tap sets' delays (the ring's newest entries move by them), and the parameters the kept samples were taken under
        std::vector<int32_t> set_of(C);
        std::vector<ChanParams> pr(h->params);
        for (size_t c = 0; c < C; c++) { set_of[c] = h->params[c].front_set; pr[c].actions = 0; }
        HIPCHK(hipMemcpy(h->d_old_sets, h->h_front_sets.data(), sizeof(FrontSet) * h->h_front_sets.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_old_set_of, set_of.data(), sizeof(int32_t) * C, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(h->d_params_replay, pr.data(), sizeof(ChanParams) * C, hipMemcpyHostToDevice));
    }
    const int64_t t0 = h->g_total, have = h->promo_have;
    const int64_t J0 = t0 / h->decim;
    // the machines as the settings in force leave them at the first kept sample / at the d ring's tail: kernels designed, block positions as the reference's
    // (both filters count from the stream's first sample: a folded handle has had no restart), buffers empty
    for (int side = 0; side < 2; side++) {
        fmx_handle_s::OlaSide &S = side ? h->ola_au : h->ola_in;
        const int64_t start = side ? J0 - PROMO_TAIL_AU : h->promo_g0;
        HIPCHK(hipMemset(S.A, 0, sizeof(float2) * C * S.L)); HIPCHK(hipMemset(S.C, 0, sizeof(float2) * C * S.L));
        HIPCHK(hipMemset(S.over, 0, sizeof(float2) * C * OLA_MAX_TAPS));
        for (size_t c = 0; c < C; c++) {
            const int32_t want = side ? (h->user[c].lf_applied > 0 ? h->user[c].lf_applied : 0) : (h->user[c].bw_applied > 0 ? h->user[c].bw_applied : 0);
            S.key[c] = want; S.on[c] = want != 0 ? 1 : 0;
            const int64_t org = (side ? h->origin_au : h->origin_in).size() == C ? (side ? h->origin_au : h->origin_in)[c] : 0;
            S.inp[c] = want != 0 ? (int32_t)((((start - org) % S.L) + S.L) % S.L) : 0;
            if (want == 0) continue;
            const std::vector<float> k = side ? design::lowpass(AUDIO_TAPS, want, h->cfg.fmRate) : design::lowpass(251, want / 2, h->cfg.inputRate);
            HIPCHK(hipMemcpy(S.taps + c * OLA_MAX_TAPS, k.data(), sizeof(float) * k.size(), hipMemcpyHostToDevice));
        }
    }
    g_launch_err = hipSuccess;
    // ---- the input side: the channels' state back to where it was at the first kept sample, then pre_kernel and the machine over the kept samples
    launch_promo_state(h->B.state, h->tail_snap, h->channels, 1, s); FMX_LAUNCHED();
    DeviceBuffers Bc = h->B; Bc.params = h->d_params_replay;
    int64_t pos = 0, last_len = 0;
    while (pos < have) {
        int64_t len = (pos == 0 && have % h->cfg.max_block) ? have % h->cfg.max_block : h->cfg.max_block;
        if (len > have - pos) len = have - pos;
        CallGeom Gc{};
        Gc.g0 = h->promo_g0 + pos; Gc.n = len; Gc.input_rate = h->cfg.inputRate; Gc.iq_format = 0; Gc.iq_scale = 1.0f; Gc.stream_stride = h->tail_cap;
        Gc.channels = h->channels; Gc.streams = h->streams; Gc.twins = h->twins; Gc.n_cus = h->n_cus;
        rc = ola_input_side(h, Gc, Bc, h->tail_iq + pos, s); if (rc) return rc;
        pos += len; last_len = len;
    }
    if (last_len < 12 * A_HIST_COLS + 12) return fail(FMX_E_HIP, "promotion: the last kept piece is shorter than the decimators' history");
    // ---- the decimators' history and the ring's newest entries
    launch_promo_hist(h->B.hist, h->d_u, h->cfg.max_block, last_len, (int)(t0 % DECIM), h->twins, h->B.zring, h->ring - 1, J0, h->d_params, h->d_old_sets, h->d_old_set_of,
                      h->channels, s); FMX_LAUNCHED();
    // ---- the audio side: the d ring's tail with the de-emphasis taken out, the audio machine over it, the de-emphasis behind the machine into the ring stage C reads
    launch_promo_inv_deemph(h->B.dring, h->dring - 1, J0, PROMO_TAIL_AU, h->d_params_replay, h->d_au_tail, h->channels, s); FMX_LAUNCHED();
    {
        OlaBuffers O{}; O.src = h->d_au_tail; O.src_stride = PROMO_TAIL_AU; O.src_mask = -1; O.src_pos = 0;
        O.dst = h->d2ring; O.dst_stride = h->dring; O.dst_mask = h->dring - 1; O.dst_pos = J0 - PROMO_TAIL_AU;
        rc = run_ola(h, h->ola_au, O, PROMO_TAIL_AU, s); if (rc) return rc;
        CallGeom Gx{}; Gx.J0 = J0 - PROMO_TAIL_AU; Gx.J1 = J0; Gx.dring_mask = h->dring - 1;
        launch_deemph(Bc, Gx, h->d2ring, h->channels, s, nullptr, nullptr); FMX_LAUNCHED();
    }
    HIPCHK(g_launch_err);
    HIPCHK(hipDeviceSynchronize());
    // ---- a block-machine handle from here on: the pending setters reach their filters through ola_take_settings, as a small handle's do
    h->ola_mode = true; h->sets_dirty = true; h->params_dirty = true;
    h->promo_pending = false; h->promo_have = 0; h->promoted = true; h->demo_capture = false; h->last_filter_event_g = t0;
    for (auto &u : h->user) { u.bw_applied = u.bandwidth; u.lf_applied = u.lf_cutoff; }
    return FMX_OK;
}

// may a promoted handle go back?  Every filter that has ever run is running and has been undisturbed for three blocks (a filter that is switched off keeps
// buffers the reference would replay when it is switched on again: such a handle stays on the machines), nothing is pending
bool demotable(fmx_handle h) {
    if (!h->promoted || !h->ola_mode || h->folded_pinned || h->twins != 1) return false;
    if (h->g_total - h->last_filter_event_g < DEMO_QUIET) return false;
    for (int side = 0; side < 2; side++) {
        const fmx_handle_s::OlaSide &S = side ? h->ola_au : h->ola_in;
        for (int c = 0; c < h->channels; c++) {
            const ChanUser &u = h->user[(size_t)c];
            if ((side ? u.lf_event : u.bw_event)) return false;
            const int32_t want = side ? (u.lf_cutoff > 0 ? u.lf_cutoff : 0) : (u.bandwidth > 0 ? u.bandwidth : 0);
            if (want != S.key[(size_t)c] && !(want == 0 && S.key[(size_t)c] <= 0)) return false;      // (a setter on its way)
            if (S.key[(size_t)c] > 0 && !S.on[(size_t)c]) return false;
            if (S.key[(size_t)c] == 0 && want == 0 && S.inp[(size_t)c] != 0) return false;             // (switched off in mid-block: stale buffers)
        }
    }
    return true;
}
// DEMOTION: the folded filters again at the stream position g_total (see DEMO_QUIET in fmx_internal.h)
int demote(fmx_handle h, hipStream_t s) {
    std::lock_guard<std::mutex> lk(h->mtx);
    const size_t C = (size_t)h->channels;
    HIPCHK(hipDeviceSynchronize());
    const int64_t t1 = h->g_total, have = h->promo_have, J1 = t1 / h->decim;
    h->origin_in.assign(C, 0); h->origin_au.assign(C, 0);
    for (size_t c = 0; c < C; c++) {
        if (h->ola_in.on[c]) h->origin_in[c] = t1 - h->ola_in.inp[c];
        if (h->ola_au.on[c]) h->origin_au[c] = J1 - h->ola_au.inp[c];
    }
    h->ola_mode = false; h->promoted = false; h->demo_capture = false; h->promo_have = 0;
    for (auto &u : h->user) { u.bw_applied = u.bandwidth; u.lf_applied = u.lf_cutoff; }
    h->sets_dirty = true;
    int rc = ensure_sets(h); if (rc) return rc;                   // (the folded tap sets of the settings in force; the channels' set indices with them)
    {
        std::vector<ChanParams> pr(h->params);
        for (auto &p : pr) p.actions = 0;
        HIPCHK(hipMemcpy(h->d_params_replay, pr.data(), sizeof(ChanParams) * C, hipMemcpyHostToDevice));
    }
    g_launch_err = hipSuccess;
    // the channels' stage-A state back to the first kept sample, an empty filter history (the run's first 24 outputs land in ring entries nobody reads any more)
    launch_promo_state(h->B.state, h->tail_snap, h->channels, 1, s); FMX_LAUNCHED();
    HIPCHK(hipMemsetAsync(h->B.hist, 0, sizeof(float2) * C * DECIM * A_HIST_COLS, s));
    HIPCHK(hipMemsetAsync(h->B.dcv_hist, 0, sizeof(float2) * C * DCV_SAVE, s));
    DeviceBuffers Bc = h->B; Bc.params = h->d_params_replay;
    int64_t pos = 0;
    while (pos < have) {
        const int64_t len = std::min<int64_t>(h->cfg.max_block, have - pos);
        CallGeom Gc{};
        Gc.g0 = h->promo_g0 + pos; Gc.n = len; Gc.J0 = Gc.g0 / h->decim; Gc.J1 = (Gc.g0 + len) / h->decim;
        Gc.ring_mask = h->ring - 1; Gc.dring_mask = h->dring - 1; Gc.sring_mask = h->sring - 1; Gc.input_rate = h->cfg.inputRate; Gc.pitch = h->pitch;
        Gc.iq_format = 0; Gc.iq_scale = 1.0f; Gc.stream_stride = h->tail_cap; Gc.channels = h->channels; Gc.streams = h->streams; Gc.twins = h->twins; Gc.n_cus = h->n_cus;
        Gc.parts = 1;
        launch_front(h->T, Bc, Gc, h->tail_iq + pos, h->channels, s); FMX_LAUNCHED();
        pos += len;
    }
    // the d ring as the folded stage B leaves it: de-emphasised (its last entries, from a standing start 2048 entries in front of what stage C reads)
    {
        CallGeom Gx{}; Gx.J0 = J1 - DEMO_TAIL_AU; Gx.J1 = J1; Gx.dring_mask = h->dring - 1;
        launch_deemph(Bc, Gx, h->B.dring, h->channels, s, nullptr, nullptr); FMX_LAUNCHED();
    }
    HIPCHK(g_launch_err);
    HIPCHK(hipDeviceSynchronize());
    h->params_dirty = true;
    return FMX_OK;
}

// scan mode's buffers (fmx_scan.hip), allocated by the first call in which a channel scans
int ensure_scan(fmx_handle h) {
    if (h->scan_alloc) return FMX_OK;
    const size_t C = (size_t)h->channels;
    HIPCHK(hipDeviceSynchronize());
    std::vector<float2> W((size_t)scan::N);
    scan::make_twiddles(W.data());
    FMXCHK(h->mem.upload(h->d_scan_W, W));
    FMXCHK(h->mem.alloc(h->d_scan_carry, C * scan::N, true));
    FMXCHK(h->mem.alloc(h->d_scan_rec, C * scan::RING, true));
    FMXCHK(h->mem.alloc(h->d_scan_jobs, C));
    FMXCHK(h->mem.alloc(h->d_scan_mute, C));
    h->scan_fill.assign(C, 0); h->scan_blocks.assign(C, 0); h->rd.scan.assign(C, 0);
    h->scan_end.assign(C * scan::RING, 0); h->scan_rec_thr.assign(C * scan::RING, 0);
    h->scan_alloc = true;
    return FMX_OK;
}

// A record meter's device side (fmx_taps.h), allocated by the first call in which a channel's meter is on: per channel `state_n` floats of the window in
// progress, `ring_n` records and a job
template <class R, class J> int ensure_record_tap(fmx_handle h, RecordTap &T, size_t state_n, size_t ring_n, float *&state, R *&ring, J *&jobs) {
    if (T.alloc) return FMX_OK;
    const size_t C = (size_t)h->channels;
    HIPCHK(hipDeviceSynchronize());
    FMXCHK(h->mem.alloc(state, C * state_n, true));
    FMXCHK(h->mem.alloc(ring, C * ring_n, true));
    FMXCHK(h->mem.alloc(jobs, C));
    T.start(C);
    return FMX_OK;
}
// ... by flush_mailbox (under mtx), where `may` allows it, and the switches of the piece being made
template <class R, class J> int flush_record_tap(fmx_handle h, RecordTap &T, bool may, size_t state_n, size_t ring_n, float *&state, R *&ring, J *&jobs) {
    if (may && !T.alloc && T.any_on()) FMXCHK(ensure_record_tap(h, T, state_n, ring_n, state, ring, jobs));
    T.take_switches();
    return FMX_OK;
}

int ensure_spec_tables(fmx_handle h) {      // (the window and the twiddles, the two spectrum meters': whichever comes first)
    if (h->d_spec_win) return FMX_OK;
    std::vector<float> win(spec::N); std::vector<float2> W(spec::N);
    survey::make_window(win.data()); survey::make_twiddles(W.data());
    FMXCHK(h->mem.upload(h->d_spec_win, win));
    return h->mem.upload(h->d_spec_W, W);
}
// The spectrum meter's memory (fmx_spec.hip), under mtx: a slot for every stream whose meter is on and has none yet.  Memory is per slot -- 32 KB of carry,
// 32 KB of sum and maximum, 128 KB of ring -- and grows to the slots in use (grow_slots).  The scratch of block
// powers holds what a call of max_block samples completes for every slot, or spec::SCRATCH_BYTES where that is less (stage_spectrum cuts the piece then).
int ensure_spectrum(fmx_handle h) {
    SlotTap &T = h->spec_tap;
    T.start((size_t)h->streams, spec::RING);
    const size_t old = (size_t)T.slots, need = old + (size_t)T.slots_needed();
    if ((int32_t)need > T.cap) {
        HIPCHK(hipDeviceSynchronize());
        FMXCHK(ensure_spec_tables(h));
        if (!h->ev_spec) HIPCHK(hipEventCreateWithFlags(&h->ev_spec, hipEventDisableTiming));
        FMXCHK(grow_slots(h->mem, h->d_spec_carry, old, need, spec::N));
        FMXCHK(grow_slots(h->mem, h->d_spec_acc, old, need, 2 * spec::N));
        FMXCHK(grow_slots(h->mem, h->d_spec_ring, old, need, spec::RING * 2 * spec::N));
        if (old > 0) HIPCHK(hipDeviceSynchronize());
        h->mem.release(h->d_spec_jobs);
        FMXCHK(h->mem.alloc(h->d_spec_jobs, need));
        const int64_t want = spec::scratch_blocks_for((int32_t)need, (h->cfg.max_block + spec::N - 1) / spec::N + 1);
        if (want > h->spec_scratch) {
            h->mem.release(h->d_spec_power);
            FMXCHK(h->mem.alloc(h->d_spec_power, (size_t)want * spec::N));
            h->spec_scratch = want;
        }
        T.cap = (int32_t)need;
    }
    T.assign_slots();
    return FMX_OK;
}

// The multiplex spectrum meter's memory (fmx_mpx.hip), under mtx, grown as ensure_spectrum grows the spectrum meter's: a slot for every channel whose meter
// is on and has none yet -- 16 KB of carry, 16 KB of sum and maximum, 64 KB of ring.  The scratch of block powers holds what a piece of work_nj fm samples
// completes for every slot, or spec::SCRATCH_BYTES where that is less (stage_mpx cuts the piece then).
int ensure_mpx(fmx_handle h) {
    SlotTap &T = h->mpx_tap;
    T.start((size_t)h->channels, mpx::RING);
    const size_t old = (size_t)T.slots, need = old + (size_t)T.slots_needed();
    if ((int32_t)need > T.cap) {
        HIPCHK(hipDeviceSynchronize());
        FMXCHK(ensure_spec_tables(h));
        if (!h->ev_mpx) HIPCHK(hipEventCreateWithFlags(&h->ev_mpx, hipEventDisableTiming));
        FMXCHK(grow_slots(h->mem, h->d_mpx_carry, old, need, mpx::N));
        FMXCHK(grow_slots(h->mem, h->d_mpx_acc, old, need, 2 * mpx::BINS));
        FMXCHK(grow_slots(h->mem, h->d_mpx_ring, old, need, mpx::RING * 2 * mpx::BINS));
        if (old > 0) HIPCHK(hipDeviceSynchronize());
        h->mem.release(h->d_mpx_jobs);
        FMXCHK(h->mem.alloc(h->d_mpx_jobs, need));
        const int64_t want = mpx::scratch_blocks_for((int32_t)need, (h->work_nj + mpx::N - 1) / mpx::N + 1);
        if (want > h->mpx_scratch) {
            h->mem.release(h->d_mpx_power);
            FMXCHK(h->mem.alloc(h->d_mpx_power, (size_t)want * mpx::BINS));
            h->mpx_scratch = want;
        }
        T.cap = (int32_t)need;
    }
    T.assign_slots();
    return FMX_OK;
}

// The sub-carrier decoder's memory (fmx_sca.hip), under mtx, grown likewise: a slot for every channel that decodes and has none yet --
// sca::BYTES_PER_CHANNEL: the ring's audio and levels, the carry, the mixed taps.  The audio filter is one per handle; a slot's mixed taps are made by
// stage_sca when its channel is switched on.
int ensure_sca(fmx_handle h) {
    SlotTap &T = h->sca_tap;
    if (!T.started()) h->sca_slot_centre.assign((size_t)h->channels, 0);
    T.start((size_t)h->channels, sca::RING);
    if (h->sca_taps_stale) {
        HIPCHK(hipDeviceSynchronize());
        h->sca_g = sca::design_band(h->sca_cfg, h->cfg.fmRate);
        h->mem.release(h->d_sca_a);
        FMXCHK(h->mem.upload(h->d_sca_a, sca::design_audio(h->sca_cfg, h->cfg.fmRate)));
        std::fill(h->sca_slot_centre.begin(), h->sca_slot_centre.end(), 0);      // (every slot's mixed taps are made anew)
        h->sca_taps_stale = false;
    }
    const size_t old = (size_t)T.slots, need = old + (size_t)T.slots_needed();
    if ((int32_t)need > T.cap) {
        HIPCHK(hipDeviceSynchronize());
        if (!h->ev_sca) HIPCHK(hipEventCreateWithFlags(&h->ev_sca, hipEventDisableTiming));
        FMXCHK(grow_slots(h->mem, h->d_sca_carry, old, need, sca::CARRY_STRIDE));
        FMXCHK(grow_slots(h->mem, h->d_sca_audio, old, need, sca::RING * sca::BLOCK_AUDIO));
        FMXCHK(grow_slots(h->mem, h->d_sca_level, old, need, sca::RING));
        FMXCHK(grow_slots(h->mem, h->d_sca_taps, old, need, sca::NG + 1));
        if (old > 0) HIPCHK(hipDeviceSynchronize());
        h->mem.release(h->d_sca_jobs);
        FMXCHK(h->mem.alloc(h->d_sca_jobs, need));
        T.cap = (int32_t)need;
    }
    T.assign_slots();
    return FMX_OK;
}

// The monitoring feed's memory (fmx_feed.hip), under mtx, grown likewise: a slot for every channel that feeds and has none yet -- feed::BYTES_PER_CHANNEL:
// the ring's audio and powers, the carry.  The taps are one array per handle, uploaded with the first slot.
int ensure_feed(fmx_handle h) {
    SlotTap &T = h->feed_tap;
    if (!T.started()) h->feed_mode.assign((size_t)h->channels, 0);
    T.start((size_t)h->channels, feed::RING);
    const size_t old = (size_t)T.slots, need = old + (size_t)T.slots_needed();
    if ((int32_t)need > T.cap) {
        HIPCHK(hipDeviceSynchronize());
        if (!h->ev_feed) HIPCHK(hipEventCreateWithFlags(&h->ev_feed, hipEventDisableTiming));
        if (!h->d_feed_h) FMXCHK(h->mem.upload(h->d_feed_h, feed::design()));
        FMXCHK(grow_slots(h->mem, h->d_feed_carry, old, need, feed::CARRY_STRIDE));
        FMXCHK(grow_slots(h->mem, h->d_feed_audio, old, need, feed::RING * feed::BLOCK));
        FMXCHK(grow_slots(h->mem, h->d_feed_power, old, need, feed::RING));
        if (old > 0) HIPCHK(hipDeviceSynchronize());
        h->mem.release(h->d_feed_jobs);
        FMXCHK(h->mem.alloc(h->d_feed_jobs, need));
        T.cap = (int32_t)need;
    }
    T.assign_slots();
    return FMX_OK;
}
// ... by flush_mailbox (under mtx) while a unit is on, and the values of the piece being made.  `live`: the tap's stage runs while SlotTap::live
template <class Ensure> int flush_slot_tap(fmx_handle h, SlotTap &T, Ensure ensure, bool live) {
    if (T.any_on()) { FMXCHK(ensure(h)); if (live) T.live = true; }
    T.take_switches();
    return FMX_OK;
}

// the tiled work arrays of the demodulator pre-pass (fmx_demod.hip): limited / unlimited samples in, demodulator output out.  (Allocated by the first call
// that needs them -- before run_call decides how the call is made: a call in pieces needs them too.)
int ensure_prepass_arrays(fmx_handle h) {
    if (h->B.w_iq) return FMX_OK;
    HIPCHK(hipDeviceSynchronize());
    FMXCHK(h->mem.alloc(h->B.w_iq, (size_t)h->work_nj * h->pitch, true));
    return h->mem.alloc(h->B.w_osc, (size_t)h->work_nj * h->pitch, true);
}
// the summary of the settings as they stand (fmx_needs.h); under mtx
CallNeeds summarize(fmx_handle h) {
    CallNeeds nd = needs_begin(h->channels, h->twins, h->ola_mode, h->scope_taps.load());
    for (size_t c = 0; c < h->params.size(); c++) {
        const ChanParams &p = h->params[c];
        const FrontSet &fs = h->h_front_sets[(size_t)p.front_set];
        needs_add(nd, ChanNeeds{p.decoder, p.squelch_mode, p.rds_mode, p.lo_freq, p.att_l, p.att_r, fs.nd, fs.dc_k, (h->mod_tap.user[c] || h->mpx_tap.user[c] || h->sca_tap.user[c]) ? 1 : 0});
    }
    return nd;
}
int flush_mailbox(fmx_handle h) {
    std::lock_guard<std::mutex> lk(h->mtx);
    if (h->gain_dirty) { h->gain_pending = true; h->gain_dirty = false; }   // (a change arriving behind this point belongs to the next call, flag and value)
    if (h->ola_mode) { int rc = ensure_ola(h); if (rc) return rc; rc = ola_take_settings(h); if (rc) return rc; }
    else if (!h->promo_pending) for (auto &u : h->user) { u.bw_event = false; u.lf_event = false; }     // (a folded handle applies a filter value, not the setter's call)
    if (h->sets_dirty) { int rc = ensure_sets(h); if (rc) return rc; h->params_dirty = true; }
    const CallNeeds nd = h->needs = summarize(h);
    if (nd.any_lo) { int rc = ensure_lo_table(h); if (rc) return rc; }
    if (nd.front4_ok && nd.any_lo) {
        // the complex-tap variant of stage A on the matrix pipe (fmx_front4lo.hip): the sum of every channel's complex taps (tap_sum_lo)
        // (computed when a channel's tap set or oscillator changes, not per call: 300 sine / cosine pairs per channel)
        h->hlo_key.resize(h->params.size(), std::make_pair(-1, 0x7fffffff));
        for (size_t ci = 0; ci < h->params.size(); ci++) {
            ChanParams &p = h->params[ci];
            const std::pair<int32_t, int32_t> key(h->front_keys[(size_t)p.front_set / (size_t)h->twins], p.lo_freq);
            if (h->hlo_key[ci] == key) continue;
            h->hlo_key[ci] = key;
            const TapSum H = tap_sum_lo(&h->h_front_taps[(size_t)p.front_set * A_TAPS_STRIDE], A_MAX_ND, h->h_front_sets[(size_t)p.front_set].off, p.lo_freq, h->cfg.inputRate);
            if (H.re != p.hlo_re || H.im != p.hlo_im) { p.hlo_re = H.re; p.hlo_im = H.im; h->params_dirty = true; }
        }
    }
    h->call_rds_mode.resize((size_t)h->channels);
    for (int c = 0; c < h->channels; c++) h->call_rds_mode[(size_t)c] = (int8_t)h->params[(size_t)c].rds_mode;
    h->call_scan.clear(); h->call_scan_thr.clear();
    for (int c = 0; c < h->channels; c++)
        if (h->user[(size_t)c].scanning) { h->call_scan.push_back(c); h->call_scan_thr.push_back(h->user[(size_t)c].scan_thr); }
    if (!h->call_scan.empty()) { const int rc = ensure_scan(h); if (rc) return rc; }
    // (any_meter says that the rows are needed: the modulation meter or the multiplex spectrum meter is on.  The modulation meter's own memory is for a handle
    // that switches it on)
    FMXCHK(flush_record_tap(h, h->mod_tap, nd.any_meter, meter::QUANT * meter::LANES, meter::RING, h->d_meter_state, h->d_meter_ring, h->d_meter_jobs));
    // (the audio meter reads the call's PCM behind everything that writes it and asks nothing of the call's plan: it is no part of CallNeeds)
    FMXCHK(flush_record_tap(h, h->audio_tap, true, loud::STATE, loud::RING, h->d_loud_state, h->d_loud_ring, h->d_loud_jobs));
    // (the reception meter reads stage A's ring, which every handle keeps in every mode: no part of CallNeeds either)
    FMXCHK(flush_record_tap(h, h->rx_tap, true, rx::QUANT * meter::LANES, rx::RING, h->d_rx_state, h->d_rx_ring, h->d_rx_jobs));
    // (a channel's RDS path runs while its decoder is on and stands still otherwise -- block filters, phase delay line, decimator and slicer
    // keep what they hold, as the reference's processor's do: nothing restarts when a decoder is switched; run_piece counts per channel)
    if (nd.any_rds) { const int rc = ensure_rds(h); if (rc) return rc; }
    // (the RDS meter reads the path's own 24 kS/s ring and switches no decoder on: no part of CallNeeds, and nothing before a decoder runs)
    FMXCHK(flush_record_tap(h, h->rdsm_tap, nd.any_rds, rdsm::QUANT * rdsm::LANES, rdsm::RING, h->d_rdsm_state, h->d_rdsm_ring, h->d_rdsm_jobs));
    // (the spectrum meter reads the call's input and its own memory: no part of CallNeeds.  fmx_spectrum_setup's grid is taken over here, while no
    // stream's meter is on: indices, cursors and what the ring held start over)
    if (h->spec_setup_dirty) { h->spec_B = h->spec_B_user; h->spec_S = h->spec_S_user; h->spec_setup_dirty = false; h->spec_tap.restart(); }
    FMXCHK(flush_slot_tap(h, h->spec_tap, ensure_spectrum, false));      // (no `live`: run_piece looks at the slots allocated)
    // (the multiplex spectrum meter reads the rows a metered channel asks for above -- ChanNeeds::metered -- and its own memory.  fmx_mpx_spectrum_setup's
    // grid is taken over here, while no channel's meter is on: indices, cursors and what the ring held start over.  live: stage_mpx has something to do --
    // a meter is on, or was and its channel's first sample has not been cleared yet)
    if (h->mpx_setup_dirty) { h->mpx_B = h->mpx_B_user; h->mpx_S = h->mpx_S_user; h->mpx_setup_dirty = false; h->mpx_tap.restart(); }
    FMXCHK(flush_slot_tap(h, h->mpx_tap, ensure_mpx, true));
    // (the sub-carrier decoder reads the rows a decoding channel asks for above -- ChanNeeds::metered -- and its own memory.  fmx_sca_setup's values are
    // taken over here, while no channel decodes: cursors and what the ring held start over.  live: stage_sca has something to do -- a channel decodes,
    // or did and its first sample has not been cleared yet)
    if (h->sca_setup_dirty) { h->sca_cfg = h->sca_cfg_user; h->sca_setup_dirty = false; h->sca_taps_stale = true; h->sca_tap.restart(); }
    FMXCHK(flush_slot_tap(h, h->sca_tap, ensure_sca, true));
    // (the monitoring feed reads the call's PCM behind everything that writes it, as the audio meter does, and its own memory: no part of CallNeeds.
    // live: stage_feed has something to do -- a channel feeds, or did and its first frame has not been cleared yet)
    FMXCHK(flush_slot_tap(h, h->feed_tap, ensure_feed, true));
    if (nd.keep_taps && !h->w_diff_mem) {
        HIPCHK(hipDeviceSynchronize());
        FMXCHK(h->mem.alloc(h->w_diff_mem, (size_t)h->work_nj * h->pitch, true));
    }
    h->B.w_diff = nd.keep_taps ? h->w_diff_mem : nullptr;
    h->taps_kept = nd.keep_taps;
    h->B.rows_on = nd.rows_on ? 1 : 0;
    h->B.peaks_on = nd.peaks_on ? 1 : 0;
    h->B.prepass_var = nd.prepass_var;
    if (nd.any_nsq && !h->T.nsq_coef) {
        // squelch ctor squelchClass.cpp:11-18 with mySquelch (1, 70000, fmRate / 20, fmRate) fm-processor.cpp:87
        const design::Iir hp = design::iir_chebyshev_lowhigh(true, 20, 70000 - 100, h->cfg.fmRate);
        const design::Iir lp = design::iir_chebyshev_lowhigh(false, 20, 70000, h->cfg.fmRate);
        h->h_nsq.assign(2 * NSQ_QUADS * 4 + 2, 0.f);
        for (int f = 0; f < 2; f++) {
            const design::Iir &F = f ? lp : hp;
            if (F.nq != NSQ_QUADS) return fail(FMX_E_HIP, "unexpected biquad count of the squelch filters");
            for (int i = 0; i < NSQ_QUADS; i++) {
                h->h_nsq[(f * NSQ_QUADS + i) * 4 + 0] = F.q[i][1]; h->h_nsq[(f * NSQ_QUADS + i) * 4 + 1] = F.q[i][2];
                h->h_nsq[(f * NSQ_QUADS + i) * 4 + 2] = F.q[i][4]; h->h_nsq[(f * NSQ_QUADS + i) * 4 + 3] = F.q[i][5];
            }
            h->h_nsq[2 * NSQ_QUADS * 4 + f] = F.gain;
        }
        HIPCHK(hipDeviceSynchronize());
        FMXCHK(h->mem.upload(h->T.nsq_coef, h->h_nsq));
    }
    if (nd.prepass) { const int rc = ensure_prepass_arrays(h); if (rc) return rc; }
    for (int c = 0; c < h->channels; c++) {            // set_squelchValue takes effect at a block start, when it differs (fm-processor.cpp:410-413)
        ChanUser &u = h->user[c];
        if (u.squelch_value != u.squelch_old) {
            u.squelch_level = u.squelch_value; u.squelch_old = u.squelch_value;
            const SquelchThr t = squelch_thresholds(u.squelch_level);
            h->params[c].squelch_thr = t.level; h->params[c].squelch_nthr = t.noise;
            h->params_dirty = true;
        }
    }
    if (h->params_dirty) {
        HIPCHK(hipDeviceSynchronize());   // the previous call may still run on the caller's stream and the side streams
        HIPCHK(hipMemcpy(h->d_params, h->params.data(), sizeof(ChanParams) * h->channels, hipMemcpyHostToDevice));
        // one-shot actions stay pending on the host until a call's kernels have consumed them (actions_consumed): an
        // upload alone -- a call that fails afterwards, or one too short to hold an fm sample -- must not lose them
        h->act_up.resize((size_t)h->channels);
        for (int c = 0; c < h->channels; c++) h->act_up[(size_t)c] = h->params[(size_t)c].actions;
        h->params_dirty = false;
    }
    return FMX_OK;
}

// The kernels of a call have been enqueued: the action bits they consume are done.  ACT_DC_RESET belongs to the input-FIR
// kernel (every call), the other two to the PSS integrator, which only looks at them in a call with at least one fm sample.
void actions_consumed(fmx_handle h, bool had_fm_samples) {
    std::lock_guard<std::mutex> lk(h->mtx);
    if (h->act_up.size() != (size_t)h->channels) return;
    const int32_t done = ACT_DC_RESET | (had_fm_samples ? (ACT_TRIGGER_FREQ | ACT_RESTART_PSS) : 0);
    for (int c = 0; c < h->channels; c++) {
        const int32_t clr = h->act_up[(size_t)c] & done;
        if (clr) { h->params[(size_t)c].actions &= ~clr; h->act_up[(size_t)c] &= ~clr; h->params_dirty = true; }   // upload the cleared bits before the next call
    }
}

void frames_geom(const fmx_handle h, int64_t n, CallGeom *G) {
    G->g0 = h->g_total; G->n = n;
    G->J0 = h->g_total / h->decim; G->J1 = (h->g_total + n) / h->decim;
    // newConverter: 192 frames in -> 48 out (newconverter.cpp:55-80, inputLimit = fmRate/1000)
    G->M0 = 48 * (G->J0 / 192); G->M1 = 48 * (G->J1 / 192);
}
// PCM frames a call of n input samples produces now
int64_t call_frames(const fmx_handle h, int64_t n) { CallGeom G{}; frames_geom(h, n, &G); return conv2_out(h, G.M1) - conv2_out(h, G.M0); }

// the handle's side streams (a call made in overlapping pieces: run_call; stage B's last round of workgroups beside stage C: run_piece), created when first wanted
int ensure_pipe_streams(fmx_handle h) {
    if (h->pipe_sA) return FMX_OK;
    // (plain streams, the recurrences' with priority.  Measured and not kept: compute units of their own for the recurrences -- CU-masked streams,
    // 16 / 32 / 64 CUs for the 64 waves, the rest for the other streams: 6.7 / 6.3 / 6.0 ms per step against 6.2 without masks.  A lone wave walks a
    // sample in 216 ns with the chip to itself and in 270-300 ns while the other stages run, on CUs of its own or not: what it loses is the
    // chip's clock under load, not its SIMD.)
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIPCHK(hipStreamCreateWithPriority(&h->pipe_sA, hipStreamNonBlocking, lo));
    HIPCHK(hipStreamCreateWithPriority(&h->pipe_sB, hipStreamNonBlocking, lo));
    HIPCHK(hipStreamCreateWithPriority(&h->pipe_sP, hipStreamNonBlocking, hi));     // (the chain everything waits for)
    for (hipEvent_t *e : {&h->pipe_ev0, &h->pipe_evA, &h->pipe_evD, &h->pipe_evP, &h->pipe_evE, &h->pipe_evB[0], &h->pipe_evB[1]}) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return FMX_OK;
}

// the arguments of an fmx_process_* call, checked once at its head (run_call; fmx_process_host_raw for the caller's PCM buffer)
int check_call(fmx_handle h, int32_t fmt, float s16_den, int64_t n, int64_t pcm_stride) {
    if (const ParamCheck pc = check_iq_format(fmt, s16_den); pc.code) return fail(pc.code, pc.msg);
    if (n <= 0 || n > h->cfg.max_block) return fail(FMX_E_TOO_LARGE, "n_complex must be in [1, max_block]");
    if (call_frames(h, n) > pcm_stride) return fail(FMX_E_TOO_LARGE, "pcm_stride smaller than the frames this call produces");
    return FMX_OK;
}

// what every piece of a call shares
struct CallArgs { int32_t fmt; float s16_den; int64_t stream_stride, pcm_stride; };

// The promotion turn of a piece.  A folded batch with a filter change pending (fmx_promote.hip) is promoted once enough of its streams is kept, else this
// piece's samples are kept too (*capture); a promoted handle whose machines have been quiet goes back to the folded filters the same way.  Either change
// happens at the head of an fmx_process_* call only, not between its pieces: fmx_filter_change_due speaks of CALLS.
int promotion_turn(fmx_handle h, bool head, hipStream_t s, bool *capture) {
    bool do_promote = false, do_demote = false;
    {
        std::lock_guard<std::mutex> lk(h->mtx);
        if (h->ola_mode) {
            const bool ok = demotable(h);      // (a quiet promoted handle keeps a block of its streams before it goes back)
            if (!ok || h->promo_recapture) { h->demo_capture = false; h->promo_have = 0; }
            else if (!h->demo_capture) { h->demo_capture = true; h->promo_have = 0; *capture = true; }
            else if (h->promo_have >= DEMO_TAIL_IN && head) do_demote = true;
            else *capture = true;
            h->promo_recapture = false;
        }
        else if (!h->promo_pending) h->promo_recapture = false;
        else if (h->promo_recapture) { h->promo_recapture = false; h->promo_have = 0; }      // (what pre_kernel applies changed: the kept samples start over, behind this call)
        else if (h->promo_have >= PROMO_TAIL_IN && head) do_promote = true;
        else *capture = true;
    }
    if (do_promote) return promote(h, s);
    if (do_demote) return demote(h, s);
    return FMX_OK;
}

// keep the piece's samples for the promotion (promotion_turn)
int capture_samples(fmx_handle h, const void *d_iq, const CallArgs &a, const CallGeom &G, hipStream_t sa) {
    if (h->tail_iq && h->promo_have + G.n > h->tail_cap) return FMX_OK;      // (cannot happen: a change is applied at the first call boundary behind PROMO_TAIL_IN samples)
    if (!h->tail_iq) {
        h->tail_cap = PROMO_TAIL_IN + h->cfg.max_block;
        FMXCHK(h->mem.alloc(h->tail_iq, (size_t)h->streams * h->tail_cap));
        FMXCHK(h->mem.alloc(h->tail_snap, (size_t)h->channels));
    }
    if (h->promo_have == 0) { h->promo_g0 = h->g_total; launch_promo_state(h->B.state, h->tail_snap, h->channels, 0, sa); FMX_LAUNCHED(); }
    launch_capture(d_iq, a.fmt, G.iq_scale, a.stream_stride, G.n, h->streams, h->tail_iq, h->tail_cap, h->promo_have, sa); FMX_LAUNCHED();
    h->promo_have += G.n;
    return FMX_OK;
}

// stage A on `sa` (the block machines: their input side and the stage on `s`): its split in time (plan_front_parts; the snapshot buffers allocated when first
// needed) and its kernel
int stage_a(fmx_handle h, CallGeom &G, const void *d_iq, hipStream_t s, hipStream_t sa) {
    const FrontParts fp = plan_front_parts(G.g0, G.n, h->front_parts.load(), h->twins, h->channels, h->n_cus);
    if (fp.parts > 1 && !h->B.fsnap) {
        const size_t C = (size_t)h->channels;
        h->B.dc_pitch = (int32_t)(h->cfg.max_block / FRONT_TILE + 2);
        FMXCHK(h->mem.alloc(h->B.dc_tiles, 2 * (size_t)h->streams * h->B.dc_pitch));
        FMXCHK(h->mem.alloc(h->B.fsnap, C));
        FMXCHK(h->mem.alloc(h->B.hist_snap, C * DECIM * A_HIST_COLS));
        FMXCHK(h->mem.alloc(h->B.dcv_snap, C * DCV_SAVE));
    }
    const FrontChoice fc = choose_front(h->needs.front4_ok, h->needs.any_lo, h->front_kernel.load(), fp.parts, h->channels, h->n_cus);
    G.parts = fc.parts; G.part_tiles = fp.part_tiles; G.front4 = fc.front4;
    // (what is reported is what runs: a call without a whole tile on the kernel's grid goes to front_kernel in launch_front)
    h->last_front_kernel = (G.front4 && front4_tiles(G, d_iq) > 0) ? 3 : 1;
    if (h->ola_mode) {
        // RF DC removal / balance / LO mix per sample, the input filter as the reference's block machine, then the decimators
        if (const int rc = ola_input_side(h, G, h->B, d_iq, s)) return rc;
        CallGeom Gp = G; Gp.pre_processed = 1; Gp.iq_format = 0; Gp.iq_scale = 1.0f; Gp.stream_stride = h->cfg.max_block; Gp.streams_private = h->twins == 1 ? 1 : 0;
        launch_front(h->T, h->B, Gp, h->d_u, h->channels, s);
    } else
    launch_front(h->T, h->B, G, d_iq, h->channels, sa);   // stage A: four waves per channel, packed-FMA FIR (fmx_front.hip)
    FMX_LAUNCHED();
    return FMX_OK;
}

// stage B (with its pre-pass for the PLL / AM decoders and the squelches): a piece of an overlapping call (piped), two channel groups (second > 0) or one
// launch sequence on `s`
int stage_b(fmx_handle h, const CallGeom &G, int k, bool piped, int second, hipStream_t s, hipStream_t sa) {
    if (piped) {
        // stage B of this piece behind its stage A.  The pre-pass of this piece: its parallel part (disc_kernel) behind the piece's stage A on that stream --
        // and behind the stage B that read the half of the work arrays it is about to overwrite --, the recurrences on theirs, the noise squelch's pipeline
        // and stage B on `s`
        HIPCHK(hipEventRecord(h->pipe_evA, sa)); HIPCHK(hipStreamWaitEvent(s, h->pipe_evA, 0));
        if (k >= 2) HIPCHK(hipStreamWaitEvent(sa, h->pipe_evB[k & 1], 0));
        DeviceBuffers Bk = h->B;
        if (k & 1) { const size_t off = (size_t)prepass_half(h->work_nj) * (size_t)h->pitch; Bk.w_iq += off; Bk.w_osc += off; }
        const PrepassStreams ps{sa, h->pipe_sP, h->pipe_evD, h->pipe_evP};
        launch_demod_fused(h->T, Bk, G, h->channels, s, &ps);
        HIPCHK(hipEventRecord(h->pipe_evB[k & 1], s));
    } else if (second > 0) {
        // (the second group on the handle's side stream, behind stage A)
        HIPCHK(hipEventRecord(h->pipe_evA, s)); HIPCHK(hipStreamWaitEvent(h->pipe_sA, h->pipe_evA, 0));
        CallGeom G1 = G, G2 = G;
        G1.ch0 = 0; G1.ch_count = h->channels - second; G2.ch0 = h->channels - second; G2.ch_count = second;
        launch_demod_fused(h->T, h->B, G1, h->channels, s);
        launch_demod_fused(h->T, h->B, G2, h->channels, h->pipe_sA);
    } else
    launch_demod_fused(h->T, h->B, G, h->channels, s);
    if (G.J1 > G.J0) {       // (stage B's bookkeeping behind the call, fmx_stageb.hip)
        int cnt = h->my_count_host + (int)(G.J1 - G.J0);
        if (cnt > (SINCOS_N >> 1)) cnt -= (SINCOS_N >> 1) + 1;
        h->my_count_host = cnt;
    }
    return FMX_OK;
}

// the RDS meter: the metered channels' 24 kS/s samples of the piece, out of the path's rds24 ring, into their lane accumulators, every window that ends in
// it into the record ring (fmx_rdsm.hip) -- on the RDS path's stream behind the piece's launch_rds, whose rds_mix_decim wrote the samples, and so ahead of the
// next piece's writes.  Channel c's path had processed rds_nc0 [c] samples in front of the piece (< 0: its decoder is off, the channel gets no job and
// nothing of its changes).  The bookkeeping is the host's (rdsm::piece); the kernel gets one job per channel that accumulates.
int stage_rds_meter(fmx_handle h, const CallGeom &G, hipStream_t s) {
    const int64_t nj = G.J1 - G.J0;
    h->rdsm_jobs.clear();
    {
        std::lock_guard<std::mutex> lk(h->mtx);      // (fmx_rds_meter_records reads the counters from any thread)
        for (int c = 0; c < h->channels; c++) {
            const int64_t a = h->rds_nc0[(size_t)c];
            if (a >= 0 && h->rdsm_tap.call[(size_t)c] && !rdsm::ring_holds(a / 8, (a + nj) / 8))
                return fail(FMX_E_TOO_LARGE, "the piece has more RDS samples than the path's 24 kS/s ring holds");
        }
        for (int c = 0; c < h->channels; c++) {
            const int64_t a = h->rds_nc0[(size_t)c];
            RecordTap &T = h->rdsm_tap;      // (on_from is rdsm::piece's, the decoder-off case included: no begin here)
            const rdsm::Piece p = rdsm::piece(T.call[(size_t)c] != 0, a >= 0, T.on_from[(size_t)c], a < 0 ? 0 : a / 8, a < 0 ? 0 : (a + nj) / 8, T.produced[(size_t)c]);
            T.on_from[(size_t)c] = p.on_from;
            if (!p.job) continue;
            h->rdsm_jobs.push_back(RdsmJob{p.first, (a + nj) / 8, c, (int32_t)p.slot(0)});
            T.produced[(size_t)c] = p.new_produced;
        }
    }
    const size_t n = h->rdsm_jobs.size();
    if (n == 0) return FMX_OK;
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_rdsm_jobs, h->rdsm_jobs.data(), sizeof(RdsmJob) * n, hipMemcpyHostToDevice, s));
    RdsmArgs A{};
    A.jobs = h->d_rdsm_jobs; A.rds24 = h->R.rds24; A.state = h->d_rdsm_state; A.ring = h->d_rdsm_ring; A.channels = h->channels;
    launch_rdsm(A, (int)n, s); FMX_LAUNCHED();
    return FMX_OK;
}

// the RDS path of the channels that decode it, each at its own block phase
int stage_rds(fmx_handle h, const CallGeom &G, hipStream_t s) {
    const int64_t nj = G.J1 - G.J0;
    int modes = 0;
    for (int c = 0; c < h->channels; c++) {
        const int m = h->call_rds_mode[(size_t)c];
        modes |= 1 << m;
        h->rds_nc0[(size_t)c] = m != 0 ? h->rds_nc[(size_t)c] : -1;
    }
    // (pageable source: the copy is staged before the call returns, the vector is free again)
    HIPCHK(hipMemcpyAsync(h->d_rds_nc0, h->rds_nc0.data(), sizeof(int64_t) * (size_t)h->channels, hipMemcpyHostToDevice, s));
    launch_rds(h->B, h->R, G, h->channels, h->rds_nc0.data(), modes, s);
    for (int c = 0; c < h->channels; c++) {
        const int64_t a = h->rds_nc0[(size_t)c];
        if (a < 0) { h->last_m0[(size_t)c] = h->last_m1[(size_t)c]; continue; }       // (decoder off in this call: no outputs, not the last on-call's)
        h->last_m0[(size_t)c] = a / 8; h->last_m1[(size_t)c] = (a + nj) / 8;
        h->rds_nc[(size_t)c] = a + nj;
    }
    return h->rdsm_tap.alloc ? stage_rds_meter(h, G, s) : FMX_OK;
}

// scan mode: the scanning channels' fm samples of the call behind their carries, every complete block of 1024 into the record ring (fmx_scan.hip), on the
// stream stage A ran on: behind this piece's stage A and ahead of the next one's.  The bookkeeping is the host's; the kernel gets one job per channel.
int stage_scan(fmx_handle h, const CallGeom &G, hipStream_t sa) {
    const int64_t nj = G.J1 - G.J0;
    const size_t n = h->call_scan.size();
    h->scan_jobs.resize(n);
    {
        std::lock_guard<std::mutex> lk(h->mtx);      // (fmx_scan_results reads the counters from any thread)
        for (size_t i = 0; i < n; i++) {
            const int c = h->call_scan[i];
            const ScanProduce sp = scan_produce(h->scan_fill[(size_t)c], h->scan_blocks[(size_t)c], nj, G.J0, scan::N, scan::RING);
            h->scan_jobs[i] = ScanJob{c, sp.job_fill, sp.job_slot0, 0};
            for (int64_t b = sp.b0; b < sp.nblk; b++) {
                const size_t slot = (size_t)c * scan::RING + (size_t)sp.slot(b);
                h->scan_end[slot] = sp.end_sample(b);
                h->scan_rec_thr[slot] = h->call_scan_thr[i];
            }
            h->scan_blocks[(size_t)c] = sp.new_blocks;
            h->scan_fill[(size_t)c] = sp.new_fill;
        }
    }
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_scan_jobs, h->scan_jobs.data(), sizeof(ScanJob) * n, hipMemcpyHostToDevice, sa));
    ScanArgs A{};
    A.jobs = h->d_scan_jobs; A.zring = h->B.zring; A.params = h->d_params; A.front_sets = h->d_front_sets; A.W = h->d_scan_W;
    A.carry = h->d_scan_carry; A.rec = h->d_scan_rec; A.J0 = G.J0; A.J1 = G.J1; A.ring_mask = G.ring_mask;
    launch_scan(A, (int)n, sa); FMX_LAUNCHED();
    return FMX_OK;
}

// the modulation meter: the metered channels' rows of the piece into their lane accumulators, every window that ends in it into the record ring
// (fmx_meter.hip), on the stream stage B ran on and behind it, where stage_rds reads the same rows.  The bookkeeping is the host's (meter_produce); the
// kernel gets one job per channel that accumulates.
int stage_meter(fmx_handle h, const CallGeom &G, hipStream_t s) {
    const int64_t nj = G.J1 - G.J0;
    if (nj > h->work_nj) return fail(FMX_E_TOO_LARGE, "the piece has more fm samples than stage B's rows hold");
    h->meter_jobs.clear();
    {
        std::lock_guard<std::mutex> lk(h->mtx);      // (fmx_mod_records reads the counters from any thread)
        for (int c = 0; c < h->channels; c++) {
            RecordTap &T = h->mod_tap;
            if (!T.begin((size_t)c, G.J0)) continue;      // (off: the window in progress is dropped)
            const meter::Produce mp = meter::meter_produce(T.on_from[(size_t)c], G.J0, nj, T.produced[(size_t)c]);
            if (mp.first >= G.J1) continue;
            h->meter_jobs.push_back(MeterJob{c, (int32_t)(mp.first - G.J0), (int32_t)mp.slot(0), 0});
            T.produced[(size_t)c] = mp.new_produced;
        }
    }
    const size_t n = h->meter_jobs.size();
    if (n == 0) return FMX_OK;
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_meter_jobs, h->meter_jobs.data(), sizeof(MeterJob) * n, hipMemcpyHostToDevice, s));
    MeterArgs A{};
    A.jobs = h->d_meter_jobs; A.w_dem = h->B.w_dem; A.w_cur = h->B.w_cur; A.state = h->d_meter_state; A.ring = h->d_meter_ring;
    A.J0 = G.J0; A.J1 = G.J1; A.lin_rows = h->B.lin_rows;
    launch_meter(A, (int)n, s); FMX_LAUNCHED();
    return FMX_OK;
}

// The multiplex spectrum meter: the metered channels' rows of the piece through fmx_mpx.hip, on the stream stage B ran on and behind it, where stage_rds and
// the modulation meter read the same rows.  What the piece's fm samples [J0, J1) mean on the grid is spec::piece's integers; the metered channels go in
// groups, a group's blocks in chunks (spec::launches), so that the scratch holds every launch's block powers; the sums stay in block order, so nothing
// depends on the cutting.  The piece's last launch of a group writes the carry: the row holds this piece's fm samples only.  The ring tags -- which record
// a slot holds -- change under mtx with the event fmx_mpx_spectrum_read waits for.
int stage_mpx(fmx_handle h, const CallGeom &G, hipStream_t s) {
    const int64_t nj = G.J1 - G.J0;
    if (nj > h->work_nj) return fail(FMX_E_TOO_LARGE, "the piece has more fm samples than stage B's rows hold");
    std::lock_guard<std::mutex> lk(h->mtx);
    const int32_t S = h->mpx_S, B = h->mpx_B;
    const spec::Piece p = spec::piece(G.J0, nj, S, B);
    h->mpx_jobs.clear();
    SlotTap &T = h->mpx_tap;
    for (int c = 0; c < h->channels; c++)
        if (T.begin((size_t)c, G.J0)) h->mpx_jobs.push_back(MpxJob{c, T.slot[(size_t)c], spec::first_block(T.on_from[(size_t)c], S)});      // (off: the record in progress is dropped)
    const int64_t n_jobs = (int64_t)h->mpx_jobs.size();
    if (n_jobs == 0) { T.live = false; return FMX_OK; }      // (every meter is off and every first sample cleared: nothing to do until one is switched on)
    if (h->mpx_c_B != B) {                    // (c follows B: fmx_mpx_spectrum_setup)
        std::vector<float> win(mpx::N);
        survey::make_window(win.data());
        h->mpx_c = survey::record_scale(win.data(), B); h->mpx_c1 = survey::record_scale(win.data(), 1); h->mpx_c_B = B;
    }
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_mpx_jobs, h->mpx_jobs.data(), sizeof(MpxJob) * (size_t)n_jobs, hipMemcpyHostToDevice, s));
    MpxArgs A{};
    A.jobs = h->d_mpx_jobs; A.w_dem = h->B.w_dem; A.lin_rows = h->B.lin_rows; A.g0 = G.J0; A.n = nj; A.S = S; A.B = B;
    A.fill = p.fill; A.fill_after = p.fill_after; A.append = p.append; A.carry_src = p.carry_src; A.c = h->mpx_c; A.c1 = h->mpx_c1;
    A.window = h->d_spec_win; A.W = h->d_spec_W; A.carry = h->d_mpx_carry; A.acc = h->d_mpx_acc; A.ring = h->d_mpx_ring; A.power = h->d_mpx_power;
    spec::launches(n_jobs, h->mpx_scratch, p.blocks, p.fill_after > 0, [&](int64_t j0, int64_t gn, int64_t done, int64_t nb, bool write_carry) {
        A.job0 = (int32_t)j0; A.n_jobs = (int32_t)gn;
        A.b = p.b0 + done; A.nb = (int32_t)nb; A.phase = (int32_t)(A.b % B);
        A.write_carry = write_carry ? 1 : 0;
        launch_mpx(A, s);
    });
    FMX_LAUNCHED();
    HIPCHK(hipEventRecord(h->ev_mpx, s)); h->ev_mpx_set = true;
    const int64_t r_end = p.record0 + p.records;
    for (const MpxJob &job : h->mpx_jobs)
        for (int64_t r = std::max(p.record0, r_end - mpx::RING); r < r_end; r++)
            if (spec::delivered(r, B, job.first)) T.tag((size_t)job.channel, r, r & (mpx::RING - 1));
    return FMX_OK;
}

// The sub-carrier decoder: the decoding channels' rows of the piece through fmx_sca.hip, on the stream stage B ran on and behind it, where stage_rds, the
// modulation meter and the multiplex spectrum meter read the same rows.  What the piece's fm samples [J0, J1) mean per channel is sca::piece's integers,
// which the kernels form again from {channel, slot, first block}.  A channel switched on -- or to another centre -- by this piece gets its mixed taps here.
// Of a piece that completes more than 128 blocks only the last 128 are formed.  The ring tags -- which block a slot holds -- change under mtx with the
// event fmx_sca_read waits for.
int stage_sca(fmx_handle h, const CallGeom &G, hipStream_t s) {
    const int64_t nj = G.J1 - G.J0;
    if (nj > h->work_nj) return fail(FMX_E_TOO_LARGE, "the piece has more fm samples than stage B's rows hold");
    std::lock_guard<std::mutex> lk(h->mtx);
    SlotTap &T = h->sca_tap;
    h->sca_jobs.clear();
    for (int c = 0; c < h->channels; c++) {
        const int32_t centre = T.call[(size_t)c], slot = T.slot[(size_t)c];
        if (centre && h->sca_slot_centre[(size_t)c] != centre) {                       // (another centre is another sub-carrier: it starts as a channel switched on does)
            std::vector<float2> taps = sca::mixed_taps(h->sca_g, centre, h->cfg.fmRate);
            taps.push_back(sca::rotation(centre, h->cfg.fmRate));
            // (pageable source: the copy is staged before the call returns)
            HIPCHK(hipMemcpyAsync(h->d_sca_taps + (size_t)slot * (sca::NG + 1), taps.data(), sizeof(float2) * taps.size(), hipMemcpyHostToDevice, s));
            h->sca_slot_centre[(size_t)c] = centre; T.restart_unit((size_t)c);
        }
        if (T.begin((size_t)c, G.J0)) h->sca_jobs.push_back(ScaJob{c, slot, sca::first_block(T.on_from[(size_t)c])});      // (off: the block in progress is dropped)
    }
    const int64_t n_jobs = (int64_t)h->sca_jobs.size();
    if (n_jobs == 0) { T.live = false; return FMX_OK; }      // (no channel decodes and every first sample is cleared: nothing to do until one is switched on)
    HIPCHK(hipMemcpyAsync(h->d_sca_jobs, h->sca_jobs.data(), sizeof(ScaJob) * (size_t)n_jobs, hipMemcpyHostToDevice, s));
    const int64_t bn = G.J0 / sca::BLOCK_FM, be = G.J1 / sca::BLOCK_FM;
    ScaArgs A{};
    A.jobs = h->d_sca_jobs; A.n_jobs = (int32_t)n_jobs; A.w_dem = h->B.w_dem; A.lin_rows = h->B.lin_rows; A.J0 = G.J0; A.nj = nj;
    A.b_lo = std::max(bn, be - sca::RING); A.nb = (int32_t)(be - A.b_lo);
    A.scale = sca::u_scale(h->sca_cfg, h->cfg.fmRate); A.a = h->d_sca_a; A.taps = h->d_sca_taps;
    A.carry = h->d_sca_carry; A.audio = h->d_sca_audio; A.level = h->d_sca_level;
    launch_sca(A, s);
    HIPCHK(hipEventRecord(h->ev_sca, s)); h->ev_sca_set = true;
    for (const ScaJob &job : h->sca_jobs)
        for (int64_t b = std::max(A.b_lo, job.first); b < be; b++) T.tag((size_t)job.channel, b, b % sca::RING);
    return FMX_OK;
}

// the reception meter: the metered channels' fm samples of the piece, out of stage A's ring, into their lane accumulators, every window that ends in it into
// the record ring (fmx_rx.hip) -- on the stream stage A ran on, behind this piece's stage A and ahead of the next one's, as stage_scan.  The sample in front
// of the piece's first comes from the ring: rx::ring_holds says that stage A has not yet written over it (with fmx_create's sizing of the ring it always
// does, as for stage B, which looks back two samples).  The bookkeeping is the host's (meter_produce); the kernel gets one job per channel that accumulates.
int stage_rx(fmx_handle h, const CallGeom &G, hipStream_t sa) {
    const int64_t nj = G.J1 - G.J0;
    h->rx_jobs.clear();
    {
        std::lock_guard<std::mutex> lk(h->mtx);      // (fmx_rx_records reads the counters from any thread)
        for (int c = 0; c < h->channels; c++)
            if (h->rx_tap.call[(size_t)c] && !rx::ring_holds(h->ring, h->h_front_sets[(size_t)h->params[(size_t)c].front_set].delay_fm, nj, h->twins))
                return fail(FMX_E_TOO_LARGE, "the piece has more fm samples than stage A's ring keeps behind the reception meter's look-back");
        for (int c = 0; c < h->channels; c++) {
            RecordTap &T = h->rx_tap;
            if (!T.begin((size_t)c, G.J0)) continue;      // (off: the window in progress is dropped)
            const meter::Produce mp = meter::meter_produce(T.on_from[(size_t)c], G.J0, nj, T.produced[(size_t)c]);
            if (mp.first >= G.J1) continue;
            h->rx_jobs.push_back(RxJob{c, (int32_t)(mp.first - G.J0), (int32_t)mp.slot(0), 0});
            T.produced[(size_t)c] = mp.new_produced;
        }
    }
    const size_t n = h->rx_jobs.size();
    if (n == 0) return FMX_OK;
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_rx_jobs, h->rx_jobs.data(), sizeof(RxJob) * n, hipMemcpyHostToDevice, sa));
    RxArgs A{};
    A.jobs = h->d_rx_jobs; A.zring = h->B.zring; A.params = h->d_params; A.front_sets = h->d_front_sets; A.state = h->d_rx_state; A.ring = h->d_rx_ring;
    A.J0 = G.J0; A.J1 = G.J1; A.ring_mask = G.ring_mask;
    launch_rx(A, (int)n, sa); FMX_LAUNCHED();
    return FMX_OK;
}

// The spectrum meter: the metered streams' input samples of the piece through fmx_spec.hip, on the stream stage A ran on.  What the piece means on the
// grid is spec::piece's integers; the metered streams go in groups, a group's blocks in chunks (spec::group_streams, spec::chunk_blocks), so that the
// scratch holds every launch's block powers; the sums stay in block order, so nothing depends on the cutting.  The piece's last launch of a group writes
// the carry.  Where stage A's stream is not the piece's own (overlapping pieces) the piece's stream waits for the meter: the caller's input buffer is
// free when the call's last stream is.  The ring tags -- which record a slot holds -- change under mtx with the event fmx_spectrum_read waits for.
int stage_spectrum(fmx_handle h, const CallGeom &G, const void *d_iq, hipStream_t s, hipStream_t sa) {
    std::lock_guard<std::mutex> lk(h->mtx);
    const int32_t S = h->spec_S, B = h->spec_B;
    const spec::Piece p = spec::piece(G.g0, G.n, S, B);
    h->spec_jobs.clear();
    SlotTap &T = h->spec_tap;
    for (int st = 0; st < h->streams; st++)
        if (T.begin((size_t)st, G.g0)) h->spec_jobs.push_back(SpecJob{st, T.slot[(size_t)st], spec::first_block(T.on_from[(size_t)st], S)});      // (off: the record in progress is dropped)
    const int64_t nj = (int64_t)h->spec_jobs.size();
    if (nj == 0) return FMX_OK;
    if (h->spec_c_B != B) {                   // (c follows B: fmx_spectrum_setup)
        std::vector<float> win(spec::N);
        survey::make_window(win.data());
        h->spec_c = survey::record_scale(win.data(), B); h->spec_c1 = survey::record_scale(win.data(), 1); h->spec_c_B = B;
    }
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_spec_jobs, h->spec_jobs.data(), sizeof(SpecJob) * (size_t)nj, hipMemcpyHostToDevice, sa));
    SpecArgs A{};
    A.jobs = h->d_spec_jobs; A.src = d_iq; A.fmt = G.iq_format; A.qs = G.iq_scale; A.src_stride = G.stream_stride; A.g0 = G.g0; A.n = G.n; A.S = S; A.B = B;
    A.fill = p.fill; A.fill_after = p.fill_after; A.append = p.append; A.carry_src = p.carry_src; A.c = h->spec_c; A.c1 = h->spec_c1;
    A.window = h->d_spec_win; A.W = h->d_spec_W; A.carry = h->d_spec_carry; A.acc = h->d_spec_acc; A.ring = h->d_spec_ring; A.power = h->d_spec_power;
    spec::launches(nj, h->spec_scratch, p.blocks, p.fill_after > 0, [&](int64_t j0, int64_t gn, int64_t done, int64_t nb, bool write_carry) {
        A.job0 = (int32_t)j0; A.n_jobs = (int32_t)gn;
        A.b = p.b0 + done; A.nb = (int32_t)nb; A.phase = (int32_t)(A.b % B);
        A.write_carry = write_carry ? 1 : 0;
        launch_spec(A, sa);
    });
    FMX_LAUNCHED();
    HIPCHK(hipEventRecord(h->ev_spec, sa)); h->ev_spec_set = true;
    if (sa != s) HIPCHK(hipStreamWaitEvent(s, h->ev_spec, 0));
    const int64_t r_end = p.record0 + p.records;
    for (const SpecJob &job : h->spec_jobs)
        for (int64_t r = std::max(p.record0, r_end - spec::RING); r < r_end; r++)
            if (spec::delivered(r, B, job.first)) T.tag((size_t)job.stream, r, r & (spec::RING - 1));
    return FMX_OK;
}

// the scanning channels' frames of the call are zeros (their chain runs on: outside the scanning calls a channel is what it would have been)
int stage_scan_mute(fmx_handle h, float2 *d_pcm, int64_t pcm_stride, int64_t frames, hipStream_t s) {
    const size_t n = h->call_scan.size();
    HIPCHK(hipMemcpyAsync(h->d_scan_mute, h->call_scan.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    launch_scan_mute(h->d_scan_mute, (int)n, d_pcm, pcm_stride, frames, s); FMX_LAUNCHED();
    return FMX_OK;
}

// the programme audio meter: the metered channels' frames of the piece, as d_pcm now holds them, through their K-weighting filters and into their window
// sums, every window that ends in the piece into the record ring (fmx_loud.hip) -- on `s`, behind both channel groups' audio kernels, the gain correction
// and the scan mute.  The bookkeeping is the host's (audio_produce); the kernel gets one job per metered channel.
int stage_audio_meter(fmx_handle h, const CallGeom &G, const float2 *d_pcm, int64_t frames, hipStream_t s) {
    h->loud_jobs.clear();
    {
        std::lock_guard<std::mutex> lk(h->mtx);      // (fmx_audio_records reads the counters from any thread)
        for (int c = 0; c < h->channels; c++) {
            RecordTap &T = h->audio_tap;
            if (!T.begin((size_t)c, G.M0)) continue;      // (off: the window in progress and the states are dropped)
            const loud::Produce ap = loud::audio_produce(T.on_from[(size_t)c], G.M0, frames, T.produced[(size_t)c]);
            h->loud_jobs.push_back(LoudJob{c, ap.first == G.M0 ? 1 : 0, (int32_t)ap.slot(0), ap.reset ? 1 : 0});
            T.produced[(size_t)c] = ap.new_produced;
        }
    }
    const size_t n = h->loud_jobs.size();
    if (n == 0) return FMX_OK;
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_loud_jobs, h->loud_jobs.data(), sizeof(LoudJob) * n, hipMemcpyHostToDevice, s));
    LoudArgs A{};
    A.jobs = h->d_loud_jobs; A.pcm = d_pcm; A.pcm_stride = G.pcm_stride; A.state = h->d_loud_state; A.ring = h->d_loud_ring;
    A.M0 = G.M0; A.frames = (int32_t)frames;
    launch_loud(A, (int)n, s); FMX_LAUNCHED();
    return FMX_OK;
}

// The monitoring feed: the feeding channels' frames of the piece, as d_pcm now holds them, through fmx_feed.hip -- on `s`, right beside the audio meter:
// behind both channel groups' audio kernels, the gain correction and the scan mute.  What the piece's frames [M0, M0 + frames) mean per channel is
// feed::piece's integers, which the kernels form again from {channel, slot, mode, first block}.  A channel found on in another mode than it runs in starts
// as a channel switched on does.  A piece without a frame only takes the switches over.  Of a piece that completes more than 128 blocks only the last 128
// are formed.  The ring tags -- which block a slot holds -- change under mtx with the event the read-outs wait for.
int stage_feed(fmx_handle h, const CallGeom &G, const float2 *d_pcm, int64_t frames, hipStream_t s) {
    std::lock_guard<std::mutex> lk(h->mtx);
    SlotTap &T = h->feed_tap;
    h->feed_jobs.clear();
    for (int c = 0; c < h->channels; c++) {
        const int32_t mode = T.call[(size_t)c];
        if (mode && h->feed_mode[(size_t)c] != mode) T.restart_unit((size_t)c);
        h->feed_mode[(size_t)c] = mode;
        if (T.begin((size_t)c, G.M0)) h->feed_jobs.push_back(FeedJob{c, T.slot[(size_t)c], mode, 0, feed::first_block(T.on_from[(size_t)c])});      // (off: the block in progress and the carry are dropped)
    }
    const int64_t n_jobs = (int64_t)h->feed_jobs.size();
    if (n_jobs == 0) { T.live = false; return FMX_OK; }      // (no channel feeds and every first frame is cleared: nothing to do until one is switched on)
    if (frames <= 0) return FMX_OK;
    if (h->ev_feed_rd_set) HIPCHK(hipStreamWaitEvent(s, h->ev_feed_rd, 0));      // (a fmx_feed_read_device still gathering on another stream reads the ring first)
    // (pageable source: the copy is staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_feed_jobs, h->feed_jobs.data(), sizeof(FeedJob) * (size_t)n_jobs, hipMemcpyHostToDevice, s));
    const int64_t be = (G.M0 + frames) / feed::BLOCK_FRAMES;
    FeedArgs A{};
    A.jobs = h->d_feed_jobs; A.n_jobs = (int32_t)n_jobs; A.pcm = d_pcm; A.pcm_stride = G.pcm_stride; A.M0 = G.M0; A.frames = (int32_t)frames;
    A.b_lo = feed::formed_from(G.M0, frames); A.nb = (int32_t)(be - A.b_lo);
    A.h = h->d_feed_h; A.carry = h->d_feed_carry; A.audio = h->d_feed_audio; A.power = h->d_feed_power;
    launch_feed(A, s);
    HIPCHK(hipEventRecord(h->ev_feed, s)); h->ev_feed_set = true;
    for (const FeedJob &job : h->feed_jobs)
        for (int64_t b = std::max(A.b_lo, job.first); b < be; b++) T.tag((size_t)job.channel, b, feed::ring_slot(b));
    return FMX_OK;
}

// stage C: the audio filter and resampler (the block machines: the audio low-pass and the de-emphasis in front of it), a gain change's correction, the
// second converter
int stage_c(fmx_handle h, CallGeom &G, float2 *d_pcm, int64_t frames, int second, hipStream_t s) {
    DeviceBuffers Bq = h->B;
    if (h->ola_mode && G.J1 > G.J0) {
        // the audio low-pass as the reference's block machine on the de-emphasised stream; the resampler reads its output
        OlaBuffers O{}; O.src = h->B.dring; O.dst = h->d2ring; O.src_stride = O.dst_stride = h->dring; O.src_mask = O.dst_mask = h->dring - 1;
        O.src_pos = O.dst_pos = G.J0;
        HStep st1;
        // de-emphasis behind the filter, as the reference orders them (:589-595)
        if (ola_single_step(h, h->ola_au, G.J1 - G.J0, &st1)) {
            OlaStepRef ref; const int rc = step_ref(h, st1, s, &ref); if (rc) return rc;
            ola_fill(h->ola_au, O);
            launch_deemph(h->B, G, h->d2ring, h->channels, s, &ref, &O); FMX_LAUNCHED();
            ola_finish_single(h, h->ola_au, st1, ref, O, s);
        } else {
            const int rc = run_ola(h, h->ola_au, O, G.J1 - G.J0, s); if (rc) return rc;
            launch_deemph(h->B, G, h->d2ring, h->channels, s, nullptr, nullptr); FMX_LAUNCHED();
        }
    }
    if (h->ola_mode) Bq.dring = h->d2ring;
    if (h->gain_pending && G.M1 > G.M0) { G.gain_fix = 1; launch_gain_fix(h->T, Bq, G, h->channels, s); FMX_LAUNCHED(); h->gain_pending = false; }
    if (second > 0) {
        CallGeom G1 = G, G2 = G;
        G1.ch0 = 0; G2.ch0 = h->channels - second;
        launch_audio(h->T, Bq, G1, d_pcm, h->channels - second, s);
        launch_audio(h->T, Bq, G2, d_pcm, second, h->pipe_sA);
        HIPCHK(hipEventRecord(h->pipe_evE, h->pipe_sA)); HIPCHK(hipStreamWaitEvent(s, h->pipe_evE, 0));
    } else if (!h->cv_nt) launch_audio(h->T, Bq, G, d_pcm, h->channels, s);
    else {
        // the audio stage writes its 48 kHz frames behind the converter's history; theConverter's output goes to the caller
        CallGeom G48 = G; G48.pcm_stride = h->x48_stride;
        launch_audio(h->T, Bq, G48, h->d_x48 + h->cv_nt, h->channels, s);
        launch_conv2(h->d_x48, h->x48_stride, h->d_cv_taps, h->cv_p, h->cv_q, h->cv_nt, G.M0, G.M1 - G.M0, conv2_out(h, G.M0), frames,
                     d_pcm, G.pcm_stride, h->channels, s);
    }
    return FMX_OK;
}

// One launch sequence: piece k of a call (fmx_plan.h plan_call), n input samples at d_iq, its frames to d_pcm, on `s`.  A piece of an overlapping call runs its
// stage A on the handle's stream pipe_sA, behind what the caller's stream held when the call began; FMX_CALL_PIECES_SERIAL=1 (a diagnostic) runs the same
// pieces one after the other on `s` -- what the overlapping run must equal bit for bit.
int run_piece(fmx_handle h, const CallArgs &a, const void *d_iq, int64_t n, float2 *d_pcm, hipStream_t s, int k, bool overlapped, int64_t *n_frames) {
    bool capture = false;
    int rc = promotion_turn(h, k == 0, s, &capture);
    if (rc || (rc = flush_mailbox(h))) return rc;
    CallGeom G{};
    frames_geom(h, n, &G);
    G.ring_mask = h->ring - 1; G.dring_mask = h->dring - 1; G.sring_mask = h->sring - 1;
    G.input_rate = h->cfg.inputRate; G.pitch = h->pitch; G.streams_private = (h->streams_private && h->twins == 1) ? 1 : 0; G.twins = h->twins; G.channels = h->channels; G.stream_stride = a.stream_stride; G.pcm_stride = a.pcm_stride;
    G.iq_format = a.fmt; G.iq_scale = (a.fmt == 3) ? 1.0f / a.s16_den : 1.0f / 128.0f; G.n_cus = h->n_cus; G.streams = h->streams;
    const int64_t frames = conv2_out(h, G.M1) - conv2_out(h, G.M0);
    const bool rds_running = h->rds_alloc && h->needs.any_rds;       // (as of this piece's flush_mailbox)
    if (rds_running && G.J1 - G.J0 > RDS_BLK)
        return fail(FMX_E_TOO_LARGE, "with RDS on, a call may cover at most 32000 fm samples (384000 input samples)");
    const bool piped = overlapped && !h->ola_mode && !env_switches().pieces_serial;
    hipStream_t sa = piped ? h->pipe_sA : s;
    G.host_count1 = piped ? h->my_count_host + 1 : 0;
    ProfRec pr{}; const bool prof = h->prof_on;
    if (prof) {
        for (int i = 0; i < 4; i++) HIPCHK(hipEventCreate(&pr.e[i]));
        pr.in_samples = n * h->streams; pr.ch_samples = n * h->channels;
        HIPCHK(hipEventRecord(pr.e[0], sa));
    }
    g_launch_err = hipSuccess;
    h->B.lin_rows = (int32_t)h->work_nj;
    if (capture && (rc = capture_samples(h, d_iq, a, G, sa))) return rc;
    if ((rc = stage_a(h, G, d_iq, s, sa))) return rc;
    if (!h->call_scan.empty() && G.J1 > G.J0 && (rc = stage_scan(h, G, sa))) return rc;
    if (h->rx_tap.alloc && G.J1 > G.J0 && (rc = stage_rx(h, G, sa))) return rc;
    if (h->spec_tap.cap > 0 && (rc = stage_spectrum(h, G, d_iq, s, sa))) return rc;
    if (prof) HIPCHK(hipEventRecord(pr.e[1], sa));
    G.stageb_form = h->stageb_form.load(); G.no_deemph = h->ola_mode ? 1 : 0;
    // a plain batch (no pre-pass, no RDS, no scope-tap rows: stage B as the whole kernel) runs stages B and C as two channel groups on two streams where it has
    // more channels than one round of stage-B workgroups (second_group_channels); FMX_TAIL_SPLIT=0: one group
    const bool plain = plain_batch(PieceFlags{piped, h->ola_mode, h->B.w_iq != nullptr, h->cv_nt != 0, h->needs.rows_on, rds_running, h->gain_pending, G.stageb_form,
                                              G.J1 > G.J0, G.M1 > G.M0});
    const int second = env_switches().tail_split && plain ? second_group_channels(h->channels, h->n_cus) : 0;
    if (second > 0 && (rc = ensure_pipe_streams(h))) return rc;
    h->last_second_group = second;
    if ((rc = stage_b(h, G, k, piped, second, s, sa))) return rc;
    if (rds_running && (rc = stage_rds(h, G, s))) return rc;
    if (h->mod_tap.alloc && G.J1 > G.J0 && (rc = stage_meter(h, G, s))) return rc;
    if (h->mpx_tap.live && G.J1 > G.J0 && (rc = stage_mpx(h, G, s))) return rc;
    if (h->sca_tap.live && G.J1 > G.J0 && (rc = stage_sca(h, G, s))) return rc;
    if (prof) HIPCHK(hipEventRecord(pr.e[2], s));
    if ((rc = stage_c(h, G, d_pcm, frames, second, s))) return rc;
    if (!h->call_scan.empty() && frames > 0 && (rc = stage_scan_mute(h, d_pcm, G.pcm_stride, frames, s))) return rc;
    if (h->audio_tap.alloc && frames > 0 && (rc = stage_audio_meter(h, G, d_pcm, frames, s))) return rc;
    if (h->feed_tap.live && (rc = stage_feed(h, G, d_pcm, frames, s))) return rc;
    if (prof) { HIPCHK(hipEventRecord(pr.e[3], s)); h->prof.push_back(pr); }
    FMX_LAUNCHED();
    HIPCHK(g_launch_err);
    actions_consumed(h, G.J1 > G.J0);
    h->last_J0 = G.J0; h->last_J1 = G.J1;
    h->g_total += n;
    if (n_frames) *n_frames = frames;
    return FMX_OK;
}

// One fmx_process_* call: checked, planned (fmx_plan.h plan_call: whole, in RDS pieces, or in overlapping pre-pass pieces), and run piece by piece.
int run_call(fmx_handle h, const void *d_iq, int32_t fmt, float s16_den, int64_t stream_stride, int64_t n, float2 *d_pcm,
             int64_t pcm_stride, int64_t *n_frames, hipStream_t s) {
    h->last_pieces = 1;
    int rc = check_call(h, fmt, s16_den, n, pcm_stride);
    if (rc) return rc;
    CallShape cs{};
    {   // (the settings as they stand now; the pieces' own decisions read what their flush_mailbox takes)
        std::lock_guard<std::mutex> lk(h->mtx);
        const CallNeeds nd = summarize(h);
        cs.any_rds = nd.any_rds; cs.prepass = nd.prepass; cs.pllc = nd.pllc; cs.am = nd.am;
    }
    // (the pre-pass's work arrays are allocated before the call is cut: the first call of such a batch runs in pieces too)
    if (!cs.any_rds && cs.prepass && !h->ola_mode && (rc = ensure_prepass_arrays(h))) return rc;
    cs.n = n; cs.decim = h->decim; cs.call_pieces = h->pipe_rows.load(); cs.channels = h->channels; cs.ola_mode = h->ola_mode; cs.conv2 = h->cv_nt != 0;
    cs.prepass_arrays = h->B.w_iq != nullptr; cs.half = prepass_half(h->work_nj);
    const CallPlan plan = plan_call(cs);
    // A batch whose channels need the demodulator pre-pass (PLL / AM decoder, a squelch: fmx_demod.hip).  Its recurrences are one wave per 64 channels walking
    // the call's fm samples one after the other -- 64 waves on 1024 SIMDs at 4096 channels, for longer than stages A, B and C together take -- and nothing else
    // can run meanwhile: stage B waits for its output, it waits for stage A.  Such a call is made in OVERLAPPING PIECES (the chain is invariant to how a stream
    // is cut into calls) on three streams: stage A of piece k + 1 and stage B / C of piece k - 1 fill the chip while the pre-pass walks piece k.  The pre-pass's
    // work arrays alternate between two halves of their allocation; an event per stage boundary orders the rest.  What the stages share beyond their hand-over
    // arrays: the myCount of the metaData snapshot (kept by stage B, read by the pre-pass: handed over by the host, CallGeom::host_count1) and the RF DC level
    // stage B's snapshot reads from stage A's state (a display value that moves by 1e-7 of its distance per sample: it may be the next piece's).
    const bool overlapped = plan.kind == CallKind::OVERLAPPED;
    hipStream_t ps = s;
    if (overlapped) {
        if ((rc = ensure_pipe_streams(h))) return rc;
        // the pieces run on the handle's three streams, behind what the caller's stream held when the call began; the caller's stream goes on behind the last of them
        HIPCHK(hipEventRecord(h->pipe_ev0, s));
        HIPCHK(hipStreamWaitEvent(h->pipe_sA, h->pipe_ev0, 0)); HIPCHK(hipStreamWaitEvent(h->pipe_sB, h->pipe_ev0, 0));
        ps = h->pipe_sB;
    }
    const CallArgs a{fmt, s16_den, stream_stride, pcm_stride};
    const int64_t bps = bytes_per_sample(fmt);
    int64_t pos = 0, total = 0;
    const bool rds_pieces = plan.lens.size() > 1 && cs.any_rds;   // (only a call that decodes RDS pays for the copy)
    std::vector<int64_t> nc_before;                               // every channel's own count of fm samples in front of such a call
    if (rds_pieces) nc_before = h->rds_alloc ? h->rds_nc : std::vector<int64_t>((size_t)h->channels, 0);
    for (size_t k = 0; k < plan.lens.size(); k++) {
        int64_t got = 0;
        rc = run_piece(h, a, reinterpret_cast<const char *>(d_iq) + pos * bps, plan.lens[k], d_pcm + total, ps, (int)k, overlapped, &got);
        if (rc) { if (overlapped) (void)hipDeviceSynchronize(); return rc; }
        pos += plan.lens[k]; total += got;
    }
    // fmx_last_rds_samples_of counts the CALL's outputs: stage_rds has left the last piece's (a call in pieces gave 1209 of its 5208)
    for (size_t c = 0; rds_pieces && h->rds_alloc && c < nc_before.size(); c++)
        if (h->rds_nc[c] != nc_before[c]) { h->last_m0[c] = nc_before[c] / 8; h->last_m1[c] = h->rds_nc[c] / 8; }
    if (overlapped) {
        HIPCHK(hipEventRecord(h->pipe_evE, h->pipe_sB)); HIPCHK(hipStreamWaitEvent(s, h->pipe_evE, 0));
        h->last_pieces = (int)plan.lens.size();
    }
    // what the batch RDS read-outs wait for instead of the whole device: the end of this call, on the stream it ran on
    if (h->rds_alloc) { HIPCHK(hipEventRecord(h->ev_call, s)); h->ev_call_set = true; }
    if (n_frames) *n_frames = total;
    return FMX_OK;
}


}  // namespace

namespace {

// ---- fmx_create, step by step -------------------------------------------------------------------------------------------
struct Conv2Design { int p = 1, q = 1, nt = 0; std::vector<float> taps; };     // the second converter (audioRate != workingRate), design::design_conv2

// 1. the configuration: what this build implements, the reference's total decimation for cfg.inputRate, the second converter
int validate_config(const fmx_config *cfg, int *decim_out, Conv2Design *cv) {
    if (cfg->struct_size != (int32_t)sizeof(fmx_config)) return fail(FMX_E_INVALID, "fmx_config.struct_size mismatch");
    if (cfg->channels < 1) return fail(FMX_E_INVALID, "channels must be >= 1");
    if (cfg->fmRate != 192000 || cfg->workingRate != 48000)
        return fail(FMX_E_UNSUPPORTED, "this build implements fmRate 192000 / workingRate 48000 (radio.cpp:68,231-233)");
    int decim = DECIM;
    {   // The reference derives its two decimators from inputRate (fm-processor.cpp:36,68-75): fmBand_1 always divides by 6, fmBand_2 by
        // (inputRate / 6) / fmRate in INTEGER arithmetic, and with inputRate / fmRate <= 1 there are no decimators at all (:471) -- whatever
        // rate that leaves is then treated as fmRate.  Stage A's kernel decimates by 12; a total of 6 or 1 runs it as 2 or 12 "twins" per
        // channel, one per output phase (CallGeom::twins).  Filters, LO table and DC constant are designed for the rate given.
        if (cfg->inputRate < 1 || cfg->inputRate > 100000000) return fail(FMX_E_INVALID, "inputRate out of range");
        if (cfg->inputRate / cfg->fmRate <= 1) decim = 1;
        else {
            const int32_t IRate = cfg->inputRate / 6;
            const int64_t d2 = IRate / cfg->fmRate;
            if ((d2 != 1 && d2 != 2) || 4 * (int64_t)cfg->inputRate / IRate + 1 != 25 || cfg->inputRate / IRate != 6)
                return fail(FMX_E_UNSUPPORTED, "inputRate: built are the rates the reference decimates by 12 (2304000 <= inputRate < 3456000), by 6 "
                                               "(1152000 <= inputRate < 2304000) and not at all (inputRate < 384000); below 1152000 the reference's "
                                               "second decimator has one tap and a zero gain (fir-filters.cpp:327-347), from 3456000 on it divides by 3+");
            decim = 6 * (int)d2;
        }
    }
    *decim_out = decim;
    if (cfg->audioRate != cfg->workingRate) {
        if (cfg->audioRate < 8000 || cfg->audioRate > 192000 ||
            !design::design_conv2(cfg->workingRate, cfg->audioRate, &cv->p, &cv->q, &cv->nt, &cv->taps))
            return fail(FMX_E_UNSUPPORTED, "audioRate: 8000 .. 192000 with audioRate / gcd (audioRate, workingRate) <= 640 (the second converter's phases)");
    }
    if (cfg->max_block < 12 || cfg->max_block > (1 << 20)) return fail(FMX_E_INVALID, "max_block must be in [12, 1048576]");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FMX_E_NO_DEVICE, "no HIP device visible: libfmx has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(FMX_E_INVALID, "device ordinal out of range");
    return FMX_OK;
}

// 2. the handle's shape, every channel's constructor defaults and its stream
int init_channels(fmx_handle h, const fmx_config *cfg, int decim, const Conv2Design &cv) {
    h->cfg = *cfg; h->cfg.stream_of_channel = nullptr;
    h->decim = decim; h->twins = DECIM / decim;
    h->channels = cfg->channels;
    h->streams = cfg->streams > 0 ? cfg->streams : cfg->channels;
    if (cv.nt) {
        h->cv_p = cv.p; h->cv_q = cv.q; h->cv_nt = cv.nt;
        h->x48_stride = cv.nt + cfg->max_block / (4 * h->decim) + 96;
    }
    h->ola_mode = filter_form(0, h->channels).ola_mode;          // FMX_P_FILTER_RESTARTS = 0 (automatic)
    h->user.assign(h->channels, ChanUser());
    h->rd.init((size_t)h->channels);
    for (RecordTap *t : {&h->mod_tap, &h->audio_tap, &h->rx_tap, &h->rdsm_tap}) t->init((size_t)h->channels);
    h->spec_tap.init((size_t)h->streams);
    for (SlotTap *t : {&h->mpx_tap, &h->sca_tap, &h->feed_tap}) t->init((size_t)h->channels);
    h->params.assign(h->channels, ChanParams());
    for (int c = 0; c < h->channels; c++) {
        ChanParams &p = h->params[c];
        std::memset(&p, 0, sizeof(p));
        int s = cfg->stream_of_channel ? cfg->stream_of_channel[c] : (cfg->streams > 0 ? c % h->streams : c);
        if (s < 0 || s >= h->streams) return fail(FMX_E_INVALID, "stream_of_channel entry out of range");
        p.stream = s;
        // constructor defaults fm-processor.cpp:110-160 / fm-demodulator.cpp:66
        p.fm_mode = 0; p.sound_sel = 0; p.decoder = 3; p.auto_mono = 1; p.pss_active = 1; p.dc_remove = 1;
        p.rds_mode = 0; p.lo_freq = 0; p.lo_period = 0; p.att_l = 1.f; p.att_r = 1.f;
        p.pll_seq = pll_seq(0, h->channels);
        const SquelchThr t = squelch_thresholds(1);              // mySquelch (1, ...) fm-processor.cpp:87
        p.squelch_mode = 0; p.squelch_thr = t.level; p.squelch_nthr = t.noise;
        refresh_derived(h, c);
    }
    std::vector<int> users((size_t)h->streams, 0);
    h->streams_private = true;
    for (auto &p : h->params) if (++users[(size_t)p.stream] > 1) h->streams_private = false;
    return FMX_OK;
}

// 3. the device's limits, the handle's stream and event
int init_device(fmx_handle h) {
    hipDeviceProp_t dp;
    HIPCHK(hipGetDeviceProperties(&dp, h->cfg.device));
    h->n_cus = dp.multiProcessorCount;
    int optin = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, h->cfg.device) != hipSuccess) optin = 0;
    h->lds_per_block = std::max((size_t)dp.sharedMemPerBlock, (size_t)optin);
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
    return FMX_OK;
}

// 4a. the trigonometric tables: SinCos and the three bit-exactness checks of what the kernels use in its place, atan, arcsine
int build_trig_tables(fmx_handle h) {
    const int32_t fmRate = h->cfg.fmRate;
    std::vector<float2> sc((size_t)SINCOS_N);                       // SinCos ctor sincos.cpp:45-54
    for (int i = 0; i < SINCOS_N; i++)
        sc[i] = make_float2((float)std::cos(2 * design::kPi * i / fmRate), (float)std::sin(2 * design::kPi * i / fmRate));
    FMXCHK(h->mem.upload(h->T.sincos, sc));
    {   // the table as two polynomials (SinPoly): accept it only if it reproduces every entry, bar a few listed exceptions
        SinPoly sp{}; sp.step = 2 * design::kPi / fmRate;
        bool fits = (fmRate == SINCOS_N);
        for (int i = 0; fits && i < SINCOS_N; i++) {
            float sn, cs;
            sincos_poly(i, sp.step, &sn, &cs);
            if (std::memcmp(&sn, &sc[i].y, 4) != 0) { if (sp.ns < 4) { sp.s_idx[sp.ns] = i; sp.s_val[sp.ns] = sc[i].y; sp.ns++; } else fits = false; }
            if (std::memcmp(&cs, &sc[i].x, 4) != 0) { if (sp.nc < 4) { sp.c_idx[sp.nc] = i; sp.c_val[sp.nc] = sc[i].x; sp.nc++; } else fits = false; }
        }
        sp.ok = fits ? 1 : 0;
        h->T.sp = sp;
    }
    {   // 2-level factorisation of the sine column for the sequential pilot PLL (LDS resident):
        // sin(2 pi idx/N) = Im(EA[a] EB[b]), idx = 256 a + b.  Used only if the f64 expression rounds to
        // exactly the reference's f32 table entry for EVERY idx (checked here with the same unfused
        // multiply/add sequence the kernel runs); otherwise the kernel reads the global table.
        std::vector<double2> tr((size_t)TRIG2_N);
        for (int a = 0; a < TRIG2_A; a++) { double t = 2 * design::kPi * (256.0 * a) / fmRate; tr[a] = make_double2(std::cos(t), std::sin(t)); }
        for (int a = 0; a < TRIG2_APAD; a++) tr[TRIG2_A + a] = tr[a];          // idx in [N, N + 512) wraps to idx - N
        for (int b = 0; b < TRIG2_B; b++) { double t = 2 * design::kPi * (double)b / fmRate; tr[TRIG2_A + TRIG2_APAD + b] = make_double2(std::cos(t), std::sin(t)); }
        bool exact = (fmRate == TRIG2_A * TRIG2_B);
        for (int i = 0; exact && i < SINCOS_N; i++) {
            const double2 ea = tr[i >> 8], eb = tr[TRIG2_A + TRIG2_APAD + (i & 255)];
            const float sn = (float)(ea.y * eb.x + ea.x * eb.y);
            if (std::memcmp(&sn, &sc[i].y, 4) != 0) exact = false;
        }
        if (exact) FMXCHK(h->mem.upload(h->T.trig2, tr));
    }
    {   // the pilot-phase wrap: (float)((double)v - 2 pi) == (v - P32) + C32 in f32 for every float v the PLL can
        // produce there, v in [P32, P32 + 0.7)?  (P32 = the float just above 2 pi.)  Checked bit for bit.
        const float P32 = 6.2831855f;
        const float C32 = (float)((double)P32 - 2 * design::kPi);
        bool ok = true;
        for (float v = P32; ok && v < P32 + 0.7f; v = std::nextafterf(v, 100.f)) {
            const float want = (float)((double)v - 2 * design::kPi);
            volatile float d = v - P32;
            const float got = d + C32;
            if (std::memcmp(&want, &got, 4) != 0) ok = false;
        }
        h->T.wrap32_c = C32; h->T.wrap32_ok = ok ? 1 : 0;
    }
    std::vector<float> at((size_t)ATAN_N + 1);                      // compAtan ctor Xtan2.cpp:28-31
    const float St = (float)design::kPi;
    for (int i = 0; i <= ATAN_N; i++) { float f = (float)i / ATAN_N; at[i] = (float)((double)(std::atan(f) * St) / design::kPi); }
    FMXCHK(h->mem.upload(h->T.atan_ppy, at));
    std::vector<float> as((size_t)ARCSINE_N + 1);                   // fm-demodulator.cpp:74-77
    for (int i = 0; i <= ARCSINE_N; i++) as[i] = (float)(std::asin(2.0 * i / ARCSINE_N - 1.0) / 2.0);
    return h->mem.upload(h->T.arcsine, as);
}

// 4b. the PSS low-pass and its spectrum, the resampler's taps, the DeviceTables scalars
int build_filter_tables(fmx_handle h) {
    const int32_t fmRate = h->cfg.fmRate;
    h->h_pss_taps = design::lowpass(PSS_TAPS, 15000, fmRate);      // stereo-separation.cpp:31,39
    FMXCHK(h->mem.upload(h->T.pss_taps, h->h_pss_taps));
    h->h_rs_taps = design::resampler(RS_TAPS);
    {   // fast-convolution form of the PSS low-pass (fmx_fftconv.h): twiddles and the taps' spectrum in the device transform's own order
        std::vector<float2> W(fftc::W_COUNT), Hs(fftc::N);
        fftc::make_twiddles(W.data());
        fftc::make_spectrum(h->h_pss_taps.data(), PSS_TAPS, Hs.data(), W.data());
        FMXCHK(h->mem.upload(h->T.fft_w, W));
        FMXCHK(h->mem.upload(h->T.pss_hs, Hs));
    }
    h->T.sincos_C = fmRate / (2 * design::kPi);
    {   // fm_Demodulator ctor fm-demodulator.cpp:57-72
        const float F_G = (float)(0.65 * fmRate / 2), Delta_F = (float)(0.95 * fmRate / 2);
        const float B_FM = 2 * (Delta_F + F_G);
        h->T.K_FM = (float)((double)(2 * B_FM) * design::kPi / (double)F_G);
        const float max_dev = (float)(0.95 * (0.5 * fmRate));
        const float fac = (float)(2.0 * design::kPi / fmRate);         // pllC ctor pllC.cpp:42-53
        h->T.pll_beta = (float)std::exp(-2.0 * design::kPi * (double)(float)(0.85 * fmRate) / 2 / fmRate);
        h->T.pll_lo = -max_dev * fac; h->T.pll_hi = max_dev * fac; h->T.pll_center = (float)(0 * 2 * design::kPi / fmRate);
    }
    // pilotRecovery / PSS ctor args fm-processor.cpp:78-82, stereo-separation.cpp:32
    h->T.pil_omega = (float)((double)((float)19000 / (float)fmRate) * (2 * design::kPi));
    h->T.pil_gain = (float)(10 * (2 * design::kPi) / fmRate);
    h->T.K_FM_rcp = 1.0f / h->T.K_FM; h->T.pil_omega_rcp = 1.0f / h->T.pil_omega;
    h->T.pss_alpha = 10.0f / (float)fmRate;
    h->T.pss_lock_alpha = 1.0f / fmRate;
    h->T.afc_l2 = (float)std::log2((double)(1 - 0.0001f));                              // fm-demodulator.cpp:197 (1 - fmDcAlpha)
    h->T.lock_l2 = (float)std::log2(1.0 - (double)(1.0f / 3000.0f));                    // pilot-recover.cpp:66 (1.0 - alpha)
    h->T.pssmean_l2 = (float)std::log2((double)(1.0f - h->T.pss_lock_alpha));          // stereo-separation.cpp:90 (1.0f - lockAlpha)
    return FMX_OK;
}

// 5. the per-channel rings, stage B's work arrays, the PCM tail's buffers, the second converter's, the channels' initial state
int alloc_channel_buffers(fmx_handle h, const Conv2Design &cv) {
    DevMem &M = h->mem;
    DeviceBuffers &B = h->B;
    const int32_t max_block = h->cfg.max_block;
    const int64_t fm_per_call = max_block / h->decim + 2;
    h->ring = next_pow2((2 * 32768 - 251) / h->decim + 1 + fm_per_call + 512);      // the input filter's latency in fm samples + a call
    // (a batch keeps three blocks of the audio filter in its d ring: what its promotion to the block machines runs the audio machine over, fmx_promote.hip)
    h->dring = next_pow2(std::max<int64_t>(AUDIO_DELAY + C_MAX_TAPS, h->channels > OLA_MAX_CH ? PROMO_TAIL_AU + 8 : 0) + fm_per_call + 192 + 4 * C_TILE);
    h->sring = 4096;
    const size_t C = (size_t)h->channels;
    const size_t CT = C * (size_t)h->twins;                    // stage-A workgroups: `twins` per channel
    if (cv.nt) {
        FMXCHK(M.upload(h->d_cv_taps, cv.taps));
        FMXCHK(M.alloc(h->d_x48, C * h->x48_stride, true));
    }
    FMXCHK(M.alloc(B.hist, CT * DECIM * A_HIST_COLS, true));
    FMXCHK(M.alloc(B.dcv_hist, CT * DCV_SAVE, true));
    if (h->twins > 1) FMXCHK(M.alloc(B.state_tw, C * (size_t)(h->twins - 1), true));
    FMXCHK(M.alloc(B.zring, C * h->ring, true));
    FMXCHK(M.alloc(B.sring, C * h->sring, true));
    FMXCHK(M.alloc(B.dring, C * h->dring, true));
    {
        const size_t NJ = (((size_t)fm_per_call + 1 + WT - 1) / WT) * WT;      // whole work-array tiles (widx)
        h->work_nj = (int64_t)NJ;
        h->pitch = ((h->channels + 63) / 64) * 64 + 64;
        const size_t P = (size_t)h->pitch;   // rows are padded (see CallGeom.pitch)
        // the recurrence kernels move whole 64-channel row blocks, pad columns included: keep those finite
        FMXCHK(M.alloc(B.w_dem, NJ * P, true));
        FMXCHK(M.alloc(B.w_cur, NJ * P, true));
        B.lockm_stride = (int32_t)(NJ / 6 + 512);
        FMXCHK(M.alloc(B.w_lockm, (size_t)B.lockm_stride * P, true));
        FMXCHK(M.alloc(B.gfix, GAIN_FIX_FRAMES * P, true));
    }
    {
        ChanState s0; std::memset(&s0, 0, sizeof(s0));
        s0.Imin1 = s0.Qmin1 = s0.Imin2 = s0.Qmin2 = (float)0.01;        // fm-demodulator.cpp:79-82
        FMXCHK(M.upload(B.state, std::vector<ChanState>(C, s0)));
    }
    FMXCHK(M.alloc(h->d_params, C));
    B.params = h->d_params;
    {   // PCM tail: one test-tone burst (fm-processor.cpp:808-813,818-821: float phase += float incr, PI_Constrain, sinf)
        // and the peak meter's per-tile maxima / window ring
        std::vector<float> tone((size_t)TT_BURST);
        float ph = 0.0f; const float inc = (float)(2 * design::kPi / h->cfg.workingRate * 1000.0f);
        for (int i = 0; i < TT_BURST; i++) {
            ph += inc;
            if (!(0 <= ph && ph < 2 * design::kPi)) ph = (float)std::fmod((double)ph, 2 * design::kPi);   // PI_Constrain fm-constants.h:149-153 (ph > 0 here)
            tone[i] = std::sin(ph);
        }
        FMXCHK(M.upload(B.tone, tone));
        B.pk_tiles = (int32_t)((max_block / (4 * h->decim) + 96) / C_TILE + 8);
        FMXCHK(M.alloc(B.pk_part, C * B.pk_tiles, true));
        FMXCHK(M.alloc(B.pk_ring, C * PK_RING, true));
    }
    return FMX_OK;
}


// a switch of the units [u, u + 1), or of all `units` of them (u < 0); under mtx
template <class T> void set_range(std::vector<T> &v, int32_t u, int32_t units, T value) {
    const int u0 = u < 0 ? 0 : u, u1 = u < 0 ? units : u + 1;
    for (int i = u0; i < u1; i++) v[(size_t)i] = value;
}
}  // namespace

extern "C" {

int fmx_abi_version(void) { return FMX_ABI_VERSION; }
const char *fmx_last_error(void) { return g_err.c_str(); }

int fmx_create(const fmx_config *cfg, fmx_handle *out) {
    if (!cfg || !out) return fail(FMX_E_INVALID, "null argument");
    (void)env_switches();                       // (the FMX_* environment switches: read here, once per process)
    int decim = DECIM;
    Conv2Design cv;
    FMXCHK(validate_config(cfg, &decim, &cv));
    HIPCHK(hipSetDevice(cfg->device));

    fmx_handle h = new (std::nothrow) fmx_handle_s();
    if (!h) return fail(FMX_E_NOMEM, "out of host memory");
    int rc = init_channels(h, cfg, decim, cv);
    if (!rc) rc = init_device(h);
    if (!rc) rc = build_trig_tables(h);
    if (!rc) rc = build_filter_tables(h);
    if (!rc) rc = alloc_channel_buffers(h, cv);
    if (!rc) rc = ensure_sets(h);
    // every failure goes through fmx_destroy: nothing of a half-built handle stays behind
    if (rc) { const std::string msg = g_err; (void)fmx_destroy(h); g_err = msg; return rc; }
    *out = h;
    return FMX_OK;
}

int fmx_destroy(fmx_handle h) {
    if (!h) return FMX_OK;
    (void)hipSetDevice(h->cfg.device);
    for (hipStream_t st : {h->stream, h->pipe_sA, h->pipe_sP, h->pipe_sB}) if (st) (void)hipStreamSynchronize(st);
    for (auto &pr : h->prof) for (int i = 0; i < 4; i++) (void)hipEventDestroy(pr.e[i]);
    for (hipEvent_t e : h->step_ev) if (e) (void)hipEventDestroy(e);
    if (h->rd_stream) { (void)hipStreamSynchronize(h->rd_stream); (void)hipStreamDestroy(h->rd_stream); }
    for (hipEvent_t e : {h->ev_call, h->ev_spec, h->ev_mpx, h->ev_sca, h->ev_feed, h->ev_feed_rd, h->ev_in, h->pipe_ev0, h->pipe_evA, h->pipe_evD, h->pipe_evP, h->pipe_evE, h->pipe_evB[0], h->pipe_evB[1]}) if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : {h->stream, h->pipe_sA, h->pipe_sP, h->pipe_sB}) if (st) (void)hipStreamDestroy(st);
    h->mem.release_all(); h->rds_mem.release_all();
    delete h;
    return FMX_OK;
}

int fmx_set_param(fmx_handle h, int32_t channel, int32_t id, double value) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (channel < -1 || channel >= h->channels) return fail(FMX_E_INVALID, "channel out of range");
    const int iv = (int)std::llround(value);
    if (const ParamCheck pc = check_param(id, value, h->cfg.inputRate); pc.code) return fail(pc.code, pc.msg);
    switch (id) {      // the handle-wide settings and scan mode's: nothing of ChanParams changes
    case FMX_P_FRONT_KERNEL: h->front_kernel.store(iv); return FMX_OK;
    case FMX_P_SCOPE_TAPS: h->scope_taps.store(iv); return FMX_OK;
    case FMX_P_CALL_PIECES: h->pipe_rows.store(iv); return FMX_OK;
    case FMX_P_FRONT_PARTS: h->front_parts.store(iv); return FMX_OK;
    case FMX_P_STAGEB_FORM: h->stageb_form.store(iv); return FMX_OK;
    case FMX_P_FILTER_RESTARTS: {
        std::lock_guard<std::mutex> lk(h->mtx);
        if (h->g_total != 0) return fail(FMX_E_UNSUPPORTED, "the filter structure of a handle is fixed by its first call");
        const FilterForm ff = filter_form(iv, h->channels);
        if (ff.ola_mode != h->ola_mode) { h->ola_mode = ff.ola_mode; h->sets_dirty = true; }
        h->folded_pinned = ff.folded_pinned;
        return FMX_OK; }
    case FMX_P_SCANNING:
    case FMX_P_SCAN_THRESHOLD: {
        std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes both at the next call; nothing on the device changes)
        const int c0 = channel < 0 ? 0 : channel, c1 = channel < 0 ? h->channels : channel + 1;
        for (int c = c0; c < c1; c++) {
            if (id == FMX_P_SCANNING) h->user[(size_t)c].scanning = value != 0.0;
            else h->user[(size_t)c].scan_thr = (int16_t)value;
        }
        return FMX_OK; }
    default: break;
    }
    std::lock_guard<std::mutex> lk(h->mtx);
    const int c0 = channel < 0 ? 0 : channel, c1 = channel < 0 ? h->channels : channel + 1;
    if (id == FMX_A_RESET_RDS || id == FMX_A_TRIGGER_FREQUENCY_CHANGE) {
        for (int c = c0; c < c1; c++) h->rd.reset_dec[(size_t)c] = h->rd.reset_dec_all[(size_t)c] = 1;      // resetRds (:862-864); triggerFrequencyChange calls it (:852); one flag per read-out path
    }
    for (int c = c0; c < c1; c++) {
        ChanUser &u = h->user[c]; ChanParams &p = h->params[c];
        switch (id) {
        case FMX_P_FM_MODE: p.fm_mode = iv; break;
        case FMX_P_FM_DECODER: p.decoder = iv; break;
        case FMX_P_SOUND_MODE: p.sound_sel = iv; break;
        case FMX_P_STEREO_PANORAMA: u.panorama = iv; break;
        case FMX_P_SOUND_BALANCE: u.balance = iv; h->gain_dirty = true; break;
        case FMX_P_DEEMPHASIS: u.deemph_us = iv; break;
        case FMX_P_VOLUME_DB: u.volume_db = (float)value; u.ctor_volume = false; h->gain_dirty = true; break;
        case FMX_P_LF_CUTOFF: case FMX_P_BANDWIDTH: {
            if (id == FMX_P_LF_CUTOFF) { u.lf_cutoff = iv > 0 ? iv : 0; u.lf_event = iv > 0; } else { u.bandwidth = iv; u.bw_event = iv > 0; }
            // (deferred: pending until the handle has kept enough of its streams to become a block-machine handle, promote)
            if (defer_filter_change(h->ola_mode, h->folded_pinned, h->g_total, h->twins, h->cfg.max_block)) { if (!h->promo_pending) { h->promo_pending = true; h->promo_have = 0; } }
            else { u.bw_applied = u.bandwidth; u.lf_applied = u.lf_cutoff; h->sets_dirty = true; }
            break; }
        case FMX_P_ATTENUATION_L: p.att_l = (float)value; h->promo_recapture = true; break;
        case FMX_P_ATTENUATION_R: p.att_r = (float)value; h->promo_recapture = true; break;
        case FMX_P_RDS_MODE: p.rds_mode = iv; break;
        case FMX_P_LOCAL_OSCILLATOR: p.lo_freq = iv; p.lo_period = lo_period(iv, h->cfg.inputRate); h->promo_recapture = true; break;
        case FMX_P_AUTO_MONO: p.auto_mono = iv != 0; break;
        case FMX_P_PSS: p.pss_active = iv != 0; break;
        case FMX_P_SQUELCH_MODE: p.squelch_mode = iv; break;
        case FMX_P_SQUELCH_VALUE: u.squelch_value = iv; break;
        case FMX_P_TEST_TONE: p.test_tone = iv != 0; break;
        case FMX_P_PLL_SOLVER: p.pll_seq = pll_seq(iv, h->channels); break;
        case FMX_P_DISP_DELAY:                       // DelayLine::set_delay_steps fm-processor.h:60-63: resize keeps what is there
            u.delay.resize((size_t)iv + 1, make_float2(-40.0f, -40.0f)); u.delay_idx = 0; break;
        case FMX_P_DC_REMOVE: p.dc_remove = iv != 0; p.actions |= ACT_DC_RESET; h->promo_recapture = true; break;
        case FMX_A_TRIGGER_FREQUENCY_CHANGE: p.actions |= ACT_TRIGGER_FREQ; break;
        case FMX_A_RESTART_PSS: p.actions |= ACT_RESTART_PSS; break;
        default: break;
        }
        refresh_derived(h, c);
    }
    h->params_dirty = true;
    return FMX_OK;
}

int fmx_mod_meter_enable(fmx_handle h, int32_t channel, int32_t on) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (channel < -1 || channel >= h->channels) return fail(FMX_E_INVALID, "channel out of range");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes it at the next call; nothing on the device changes)
    set_range<uint8_t>(h->mod_tap.user, channel, h->channels, on != 0);
    return FMX_OK;
}

int fmx_audio_meter_enable(fmx_handle h, int32_t channel, int32_t on) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (channel < -1 || channel >= h->channels) return fail(FMX_E_INVALID, "channel out of range");
    if (h->cv_nt != 0 || h->cfg.audioRate != 48000)
        return fail(FMX_E_UNSUPPORTED, "the audio meter's K-weighting coefficients are those of 48000 frames/s: not on a handle with another audioRate");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes it at the next call; nothing on the device changes)
    set_range<uint8_t>(h->audio_tap.user, channel, h->channels, on != 0);
    return FMX_OK;
}

int fmx_rx_meter_enable(fmx_handle h, int32_t channel, int32_t on) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (channel < -1 || channel >= h->channels) return fail(FMX_E_INVALID, "channel out of range");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes it at the next call; nothing on the device changes)
    set_range<uint8_t>(h->rx_tap.user, channel, h->channels, on != 0);
    return FMX_OK;
}

int fmx_rds_meter_enable(fmx_handle h, int32_t channel, int32_t on) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (channel < -1 || channel >= h->channels) return fail(FMX_E_INVALID, "channel out of range");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes it at the next call; nothing on the device changes, and no decoder is switched)
    set_range<uint8_t>(h->rdsm_tap.user, channel, h->channels, on != 0);
    return FMX_OK;
}

int fmx_spectrum_setup(fmx_handle h, int32_t blocks_per_record, int32_t every) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (blocks_per_record < 1 || blocks_per_record > spec::MAX_B) return fail(FMX_E_INVALID, "blocks_per_record must be in [1, 4096]");
    if (every < 1 || every > spec::MAX_S) return fail(FMX_E_INVALID, "every must be in [1, 4096]");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes the grid over at the next call)
    if (h->spec_tap.any_on())
        return fail(FMX_E_INVALID, "fmx_spectrum_setup: a stream's spectrum meter is on");
    h->spec_B_user = blocks_per_record; h->spec_S_user = every; h->spec_setup_dirty = true;
    return FMX_OK;
}

int fmx_spectrum_enable(fmx_handle h, int32_t stream, int32_t on) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (stream < -1 || stream >= h->streams) return fail(FMX_E_INVALID, "stream out of range");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes it at the next call; nothing on the device changes)
    set_range<int32_t>(h->spec_tap.user, stream, h->streams, on != 0);
    return FMX_OK;
}

int fmx_mpx_spectrum_setup(fmx_handle h, int32_t blocks_per_record, int32_t every) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (blocks_per_record < 1 || blocks_per_record > mpx::MAX_B) return fail(FMX_E_INVALID, "blocks_per_record must be in [1, 4096]");
    if (every < 1 || every > mpx::MAX_S) return fail(FMX_E_INVALID, "every must be in [1, 4096]");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes the grid over at the next call)
    if (h->mpx_tap.any_on())
        return fail(FMX_E_INVALID, "fmx_mpx_spectrum_setup: a channel's multiplex spectrum meter is on");
    h->mpx_B_user = blocks_per_record; h->mpx_S_user = every; h->mpx_setup_dirty = true;
    return FMX_OK;
}

int fmx_mpx_spectrum_enable(fmx_handle h, int32_t channel, int32_t on) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (channel < -1 || channel >= h->channels) return fail(FMX_E_INVALID, "channel out of range");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes it at the next call; nothing on the device changes)
    set_range<int32_t>(h->mpx_tap.user, channel, h->channels, on != 0);
    return FMX_OK;
}

int fmx_sca_setup(fmx_handle h, const fmx_sca_config *cfg) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    const fmx_sca_config want = cfg ? *cfg : sca::default_config();
    if (const char *why = sca::config_error(&want, h->cfg.fmRate)) return fail(FMX_E_INVALID, std::string("fmx_sca_setup: ") + why);
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes the values over at the next call)
    if (h->sca_tap.any_on())
        return fail(FMX_E_INVALID, "fmx_sca_setup: a channel's sub-carrier decoder is on");
    h->sca_cfg_user = want; h->sca_setup_dirty = true;
    return FMX_OK;
}

int fmx_sca_enable(fmx_handle h, int32_t channel, int32_t centre_hz) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (channel < -1 || channel >= h->channels) return fail(FMX_E_INVALID, "channel out of range");
    if (centre_hz < 0) return fail(FMX_E_INVALID, "centre_hz must not be negative");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes it at the next call; nothing on the device changes)
    const fmx_sca_config &cfg = h->sca_setup_dirty ? h->sca_cfg_user : h->sca_cfg;
    if (const char *why = sca::centre_error(centre_hz, cfg.half_band_hz, h->cfg.fmRate))
        return fail(FMX_E_INVALID, "fmx_sca_enable: centre_hz " + std::to_string(centre_hz) + " with half_band_hz " + std::to_string(cfg.half_band_hz) + " at fmRate " +
                                       std::to_string(h->cfg.fmRate) + ": " + why);
    set_range<int32_t>(h->sca_tap.user, channel, h->channels, centre_hz);
    return FMX_OK;
}

int fmx_feed_enable(fmx_handle h, int32_t channel, int32_t mode) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    if (channel < -1 || channel >= h->channels) return fail(FMX_E_INVALID, "channel out of range");
    if (mode < feed::MODE_OFF || mode > feed::MODE_RIGHT) return fail(FMX_E_INVALID, "fmx_feed_enable: mode must be 0 (off), 1 ((L + R) / 2), 2 (left) or 3 (right)");
    if (h->cv_nt != 0 || h->cfg.audioRate != 48000)
        return fail(FMX_E_UNSUPPORTED, "the feed's filter and its divide by 3 are those of 48000 frames/s: not on a handle with another audioRate");
    std::lock_guard<std::mutex> lk(h->mtx);      // (flush_mailbox takes it at the next call; nothing on the device changes)
    set_range<int32_t>(h->feed_tap.user, channel, h->channels, mode);
    return FMX_OK;
}

int64_t fmx_feed_allocated(fmx_handle h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mtx);
    return (int64_t)h->feed_tap.cap * feed::BYTES_PER_CHANNEL;
}

int64_t fmx_filter_change_due(fmx_handle h) {
    if (!h) return -1;
    std::lock_guard<std::mutex> lk(h->mtx);
    if (!h->promo_pending || h->ola_mode) return -1;
    if (h->promo_recapture) return PROMO_TAIL_IN + 1;
    return h->promo_have >= PROMO_TAIL_IN ? 0 : PROMO_TAIL_IN - h->promo_have;
}

int64_t fmx_frames_for(fmx_handle h, int64_t n) {
    if (!h || n < 0) return -1;
    return call_frames(h, n);
}

int fmx_process_device_raw(fmx_handle h, const void *d_iq, int32_t format, float s16_den, int64_t stream_stride, int64_t n,
                           float *d_pcm, int64_t pcm_stride, int64_t *n_frames, void *hip_stream) {
    if (!h || !d_iq || !d_pcm) return fail(FMX_E_INVALID, "null argument");
    if (stream_stride < n) return fail(FMX_E_INVALID, "stream_stride < n_complex");
    HIPCHK(hipSetDevice(h->cfg.device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (!hip_stream) {
        // NULL also names HIP's legacy default stream, where such a caller's producer (e.g. PyTorch's current stream) runs;
        // the handle's stream is non-blocking, so order this call behind what is queued there now.  (Measured: the default
        // stream's implicit synchronisation with the CU-masked streams of stage B costs ~0.4 ms per call at 4096 channels;
        // a caller that passes a stream of its own, as bench.py does, does not pay it.)
        HIPCHK(hipEventRecord(h->ev_in, nullptr));
        HIPCHK(hipStreamWaitEvent(h->stream, h->ev_in, 0));
    }
    return run_call(h, d_iq, format, s16_den, stream_stride, n, reinterpret_cast<float2 *>(d_pcm), pcm_stride, n_frames, s);
}
int fmx_process_device(fmx_handle h, const float *d_iq, int64_t stream_stride, int64_t n, float *d_pcm,
                       int64_t pcm_stride, int64_t *n_frames, void *hip_stream) {
    return fmx_process_device_raw(h, d_iq, FMX_IQ_F32, 0.f, stream_stride, n, d_pcm, pcm_stride, n_frames, hip_stream);
}

int fmx_process_host_raw(fmx_handle h, const void *iq, int32_t format, float s16_den, int64_t stream_stride, int64_t n,
                         float *pcm, int64_t pcm_stride, int64_t *n_frames) {
    if (!h || !iq || !pcm) return fail(FMX_E_INVALID, "null argument");
    if (stream_stride < n) return fail(FMX_E_INVALID, "stream_stride < n_complex");
    if (const int rc = check_call(h, format, s16_den, n, pcm_stride)) return rc;     // (pcm_stride: the caller's buffer; run_call checks the staging buffer's)
    HIPCHK(hipSetDevice(h->cfg.device));
    const int64_t cap = conv2_out(h, h->cfg.max_block / (4 * h->decim) + 96) + 2;
    if (!h->d_iq) {
        FMXCHK(h->mem.alloc(h->d_iq, (size_t)h->streams * h->cfg.max_block));    // sized for the widest format
        FMXCHK(h->mem.alloc(h->d_pcm, (size_t)h->channels * cap));
    }
    const size_t bps = (size_t)bytes_per_sample(format);
    // The single receiver's call (one stream, 16384 samples: 128 KB in, 2.7 KB out) spends a third of its time in the two copies' fixed costs
    // (a pageable buffer is staged by the runtime, each copy is a submission of its own).  Small calls go through pinned, device-visible
    // memory instead: the samples are copied there by the CPU and READ BY STAGE A over the bus, the PCM is written there by stage C.
    constexpr size_t ZC_MAX_IN = (size_t)1 << 20;
    const size_t in_bytes = bps * (size_t)n * (size_t)h->streams;
    if (in_bytes <= ZC_MAX_IN && (size_t)h->channels * (size_t)cap * sizeof(float2) <= ZC_MAX_IN) {
        if (!h->hp_pcm) {
            FMXCHK(h->mem.alloc_pinned(h->hp_iq, ZC_MAX_IN));
            FMXCHK(h->mem.alloc_pinned(h->hp_pcm, (size_t)h->channels * cap));
        }
        for (int sidx = 0; sidx < h->streams; sidx++)
            std::memcpy(h->hp_iq + (size_t)sidx * bps * n, (const char *)iq + (size_t)sidx * bps * stream_stride, bps * (size_t)n);
        int64_t got = 0;
        int rc = run_call(h, h->hp_iq, format, s16_den, n, n, h->hp_pcm, cap, &got, h->stream);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int c = 0; c < h->channels && got > 0; c++)
            std::memcpy(pcm + 2 * (size_t)c * pcm_stride, h->hp_pcm + (size_t)c * cap, sizeof(float2) * (size_t)got);
        if (n_frames) *n_frames = got;
        return FMX_OK;
    }
    HIPCHK(hipMemcpy2DAsync(h->d_iq, bps * h->cfg.max_block, iq, bps * stream_stride, bps * n, h->streams,
                            hipMemcpyHostToDevice, h->stream));
    int64_t got = 0;
    int rc = run_call(h, h->d_iq, format, s16_den, h->cfg.max_block, n, h->d_pcm, cap, &got, h->stream);
    if (rc) return rc;
    if (got > 0)
        HIPCHK(hipMemcpy2DAsync(pcm, sizeof(float2) * pcm_stride, h->d_pcm, sizeof(float2) * cap, sizeof(float2) * got,
                                h->channels, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n_frames) *n_frames = got;
    return FMX_OK;
}
int fmx_process_host(fmx_handle h, const float *iq, int64_t stream_stride, int64_t n, float *pcm,
                     int64_t pcm_stride, int64_t *n_frames) {
    return fmx_process_host_raw(h, iq, FMX_IQ_F32, 0.f, stream_stride, n, pcm, pcm_stride, n_frames);
}

int fmx_synchronize(fmx_handle h) {
    if (!h) return fail(FMX_E_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    return FMX_OK;
}

}  // extern "C"

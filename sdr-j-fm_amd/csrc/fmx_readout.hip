// fmx_readout.hip -- the entry points of include/fmx.h that only read a handle: metaData, peak levels, scope taps, tap sets, the RDS bits, symbols, groups
// and decoders, scan records, the modulation meter's, the audio meter's, the reception meter's and the RDS meter's records, the PLL counters, the facts about
// the last call; the host-only RDS helpers, the host-only loudness figures (fmx_audio_loudness), reception figures (fmx_rx_quality_of) and RDS meter's
// calibration and figures (fmx_rds_meter_cal, fmx_rds_meter_figures).  A per-channel read-out waits for the device, asks its ring's producer for the count, and takes [from, from + count) out of one copy of the ring (read_ring); where each reader stands is in the
// handle's Readers (fmx_host.h), for the eight taps in the tap itself (RecordTap, SlotTap: fmx_taps.h).  The two batch RDS read-outs wait for the handle's last call only and copy every channel's ring at once (rds_batch_fetch).
#include "fmx_host.h"
#include "fmx_design.h"

#include <cmath>
#include <complex>
#include <cstring>

namespace {

// the head of a read-out: this handle's device, and everything enqueued on it done
int device_idle(fmx_handle h) {
    HIPCHK(hipSetDevice(h->cfg.device));
    HIPCHK(hipDeviceSynchronize());
    return FMX_OK;
}
// ... followed by the state of the channels [c0, c1) / by a channel's RDS state
int fetch_chan_states(fmx_handle h, int c0, int c1, ChanState *st) {
    FMXCHK(device_idle(h));
    HIPCHK(hipMemcpy(st, h->B.state + c0, sizeof(ChanState) * (size_t)(c1 - c0), hipMemcpyDeviceToHost));
    return FMX_OK;
}
int fetch_rds_state(fmx_handle h, int channel, RdsState *st) {
    FMXCHK(device_idle(h));
    HIPCHK(hipMemcpy(st, h->R.state + channel, sizeof(RdsState), hipMemcpyDeviceToHost));
    return FMX_OK;
}

// The rings of `n` consecutive channels, `ring` entries each, at d_rings: of channel k the items [takes [k].from, takes [k].from + takes [k].count), oldest
// first: visit (k, i, item) for i = 0 .. count - 1, out of ONE copy of the rings.  Nothing is copied when there is nothing to take.
template <class T, class F> int read_rings(const T *d_rings, int ring, int n, const RingTake *takes, F &&visit) {
    bool any = false;
    for (int k = 0; k < n; k++) any |= takes[k].count > 0;
    if (!any) return FMX_OK;
    std::vector<T> items((size_t)ring * (size_t)n);
    HIPCHK(hipMemcpy(items.data(), d_rings, sizeof(T) * items.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < n; k++)
        for (int64_t i = 0; i < takes[k].count; i++) visit(k, i, items[(size_t)k * (size_t)ring + (size_t)ring_slot(takes[k].from + i, ring)]);
    return FMX_OK;
}
// ... of one channel: visit (i, item)
template <class T, class F> int read_ring(const T *d_ring, int ring, RingTake t, F &&visit) {
    return read_rings(d_ring, ring, 1, &t, [&](int, int64_t i, const T &item) { visit(i, item); });
}

// A record meter's read-out (RecordTap, fmx_taps.h): of the channels [first_channel, first_channel + n_channels) the records at the cursor, oldest first, at most
// `cap` each, out of one copy of their rings; the cursors move behind what was handed out (a reader that fell behind: the gap shows in `index`)
template <class R> int read_records(fmx_handle h, RecordTap fmx_handle_s::*tap, R *fmx_handle_s::*d_ring, int ring, int32_t first_channel, int32_t n_channels, R *out, int32_t cap,
                                    int32_t *n_records) {
    if (!h || first_channel < 0 || n_channels < 0 || (int64_t)first_channel + n_channels > h->channels || cap < 0 || (n_channels > 0 && (!n_records || (cap > 0 && !out))))
        return fail(FMX_E_INVALID, "bad argument");
    RecordTap &T = h->*tap;
    for (int k = 0; k < n_channels; k++) n_records[k] = 0;
    if (n_channels == 0 || !T.alloc) return FMX_OK;
    FMXCHK(device_idle(h));
    std::lock_guard<std::mutex> lk(h->mtx);
    std::vector<RingTake> takes((size_t)n_channels);
    for (int k = 0; k < n_channels; k++) takes[(size_t)k] = T.take((size_t)(first_channel + k), ring, cap);
    FMXCHK(read_rings(h->*d_ring + (size_t)first_channel * (size_t)ring, ring, n_channels, takes.data(),
                      [&](int k, int64_t i, const R &r) { out[(size_t)k * (size_t)cap + (size_t)i] = r; }));
    for (int k = 0; k < n_channels; k++) { T.commit((size_t)(first_channel + k), takes[(size_t)k]); n_records[k] = (int32_t)takes[(size_t)k].count; }
    return FMX_OK;
}

// fmx_pll_replays / fmx_pll_exact_segments: a counter of ChanState, of one channel or (channel < 0) summed over all
template <class F> int64_t sum_chan_states(fmx_handle h, int32_t channel, F counter) {
    if (!h || channel >= h->channels) return (int64_t)fail(FMX_E_INVALID, "bad argument");
    const int c0 = channel < 0 ? 0 : channel, c1 = channel < 0 ? h->channels : channel + 1;
    std::vector<ChanState> st((size_t)(c1 - c0));
    if (fetch_chan_states(h, c0, c1, st.data()) != FMX_OK) return (int64_t)fail(FMX_E_HIP, "device error");
    int64_t n = 0;
    for (auto &s : st) n += counter(s);
    return n;
}

// One read-out of the device for the channels first .. first + n - 1: their synchroniser states and group rings, behind the handle's last call, in two
// copies into the handle's pinned buffer.
int rds_batch_fetch(fmx_handle h, int first, int n, const RdsSyncChan **st, const RdsGroupRec **grp) {
    HIPCHK(hipSetDevice(h->cfg.device));
    const size_t C = (size_t)h->channels;
    if (!h->rd_stream) HIPCHK(hipStreamCreateWithFlags(&h->rd_stream, hipStreamNonBlocking));
    if (!h->rds_stage) FMXCHK(h->rds_mem.alloc_pinned(h->rds_stage, C * (sizeof(RdsSyncChan) + sizeof(RdsGroupRec) * RDS_GROUP_RING)));
    RdsGroupRec *g = reinterpret_cast<RdsGroupRec *>(h->rds_stage);                        // (the 16-byte records first: the buffer's alignment is theirs)
    RdsSyncChan *c = reinterpret_cast<RdsSyncChan *>(h->rds_stage + C * sizeof(RdsGroupRec) * RDS_GROUP_RING);
    if (h->ev_call_set) HIPCHK(hipStreamWaitEvent(h->rd_stream, h->ev_call, 0));
    HIPCHK(hipMemcpyAsync(c, h->R.sync + first, sizeof(RdsSyncChan) * (size_t)n, hipMemcpyDeviceToHost, h->rd_stream));
    HIPCHK(hipMemcpyAsync(g, h->R.groups + (size_t)first * RDS_GROUP_RING, sizeof(RdsGroupRec) * RDS_GROUP_RING * (size_t)n, hipMemcpyDeviceToHost, h->rd_stream));
    HIPCHK(hipStreamSynchronize(h->rd_stream));
    *st = c; *grp = g;
    return FMX_OK;
}

}  // namespace

extern "C" {

int fmx_get_meta(fmx_handle h, int32_t channel, fmx_meta *m) {
    if (!h || !m || channel < 0 || channel >= h->channels) return fail(FMX_E_INVALID, "bad argument");
    ChanState st;
    FMXCHK(fetch_chan_states(h, channel, channel + 1, &st));
    m->DcValRf = st.meta_dc_rf; m->DcValIf = st.meta_dc_if; m->PssPhaseShiftDegree = st.meta_pss_deg;
    m->PssPhaseChange = st.meta_pss_change; m->PssState = st.meta_pss_state;
    m->PilotPllLockStrength = st.meta_lock_strength; m->PilotPllLocked = st.meta_locked;
    m->live_pilot_locked = (h->params[channel].fm_mode != 2) ? st.pil_locked : 0;
    m->live_lock_strength = (h->params[channel].fm_mode != 2) ? st.pil_lock : 0.f;
    m->live_dc_if = st.fm_afc; m->squelch_active = (h->params[channel].squelch_mode != 0) ? st.sq_suppress : 0;
    m->fm_samples = h->g_total / h->decim; m->pcm_frames = conv2_out(h, 48 * ((h->g_total / h->decim) / 192));
    m->live_rf_dc_re = st.dc_re; m->live_rf_dc_im = st.dc_im;
    return FMX_OK;
}

int fmx_get_peaks(fmx_handle h, int32_t channel, float *lr_db, int32_t capacity, int32_t *n_events) {
    if (!h || !n_events || channel < 0 || channel >= h->channels || capacity < 0 || (capacity > 0 && !lr_db))
        return fail(FMX_E_INVALID, "bad argument");
    if (!h->taps_kept) return fail(FMX_E_UNSUPPORTED, "this handle does not run the peak-level meter: a display feed, automatic only up to 64 channels -- fmx_set_param (h, -1, FMX_P_SCOPE_TAPS, 1) and one call switch it on");
    ChanState st;
    FMXCHK(fetch_chan_states(h, channel, channel + 1, &st));
    std::lock_guard<std::mutex> lk(h->mtx);
    ChanUser &u = h->user[channel];
    const RingTake t = ring_take(st.pk_events, h->rd.peaks[channel], PK_RING, capacity);      // (a caller that fell behind: the oldest windows are gone)
    FMXCHK(read_ring(h->B.pk_ring + (size_t)channel * PK_RING, PK_RING, t, [&](int64_t k, float2 pk) {
        // fm-processor.cpp:785-794: float log10 (std::log10 of a float), -40 dB for silence, then the display delay line
        const float ldb = pk.x > 0.0f ? 20.0f * std::log10(pk.x) : -40.0f;
        const float rdb = pk.y > 0.0f ? 20.0f * std::log10(pk.y) : -40.0f;
        u.delay[u.delay_idx] = make_float2(ldb, rdb);
        u.delay_idx = (u.delay_idx + 1) % (uint32_t)u.delay.size();
        lr_db[2 * k] = u.delay[u.delay_idx].x; lr_db[2 * k + 1] = u.delay[u.delay_idx].y;
    }));
    h->rd.peaks[channel] = (int32_t)t.next();
    *n_events = (int32_t)t.count;
    return FMX_OK;
}

int fmx_get_tap(fmx_handle h, int32_t channel, int32_t tap, float *dst, int64_t n) {
    if (!h || !dst || channel < 0 || channel >= h->channels || n < 0) return fail(FMX_E_INVALID, "bad argument");
    const int64_t J1 = h->g_total / h->decim;
    if (tap != 4 && (n > J1 || n > (h->last_J1 - h->last_J0))) return fail(FMX_E_INVALID, "n exceeds the samples produced by the last call");
    FMXCHK(device_idle(h));
    const char *base; int64_t cap, elem, delay = 0;
    switch (tap) {
    case FMX_TAP_FM_IQ: base = (const char *)(h->B.zring + (size_t)channel * h->ring); cap = h->ring; elem = sizeof(float2);
        delay = h->h_front_sets[h->params[channel].front_set].delay_fm; break;
    case FMX_TAP_DEMOD: case FMX_TAP_LR_RAW: case FMX_TAP_PILOT_PHASE: {
        // these taps are read back from the last call's work arrays (channel-major rows of the call), rows [nj - n, nj)
        const int64_t nj = h->last_J1 - h->last_J0, r0 = nj - n;
        if (!h->taps_kept) return fail(FMX_E_UNSUPPORTED, "this handle does not keep the demodulator / LR / pilot-phase scope taps: display feeds, automatic only up to 64 channels -- fmx_set_param (h, -1, FMX_P_SCOPE_TAPS, 1) and one call switch them on");
        if (n == 0) return FMX_OK;
        {                            // this call's rows are contiguous per channel
            const size_t off = (size_t)channel * (size_t)h->work_nj + (size_t)r0;
            std::vector<float> a((size_t)n), b;
            HIPCHK(hipMemcpy(a.data(), (tap == FMX_TAP_PILOT_PHASE ? h->B.w_cur : h->B.w_dem) + off, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
            if (tap == FMX_TAP_LR_RAW) {
                b.resize((size_t)n);
                HIPCHK(hipMemcpy(b.data(), h->B.w_diff + off, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
                for (int64_t i = 0; i < n; i++) { dst[2 * i] = a[(size_t)i]; dst[2 * i + 1] = b[(size_t)i]; }
            } else std::memcpy(dst, a.data(), sizeof(float) * (size_t)n);
        }
        return FMX_OK; }
    case FMX_TAP_PRE_RESAMPLER: base = (const char *)((h->ola_mode && h->d2ring ? h->d2ring : h->B.dring) + (size_t)channel * h->dring); cap = h->dring; elem = sizeof(float2); break;
    case 4: {   // FMX_TAP_RDS_IQ: complex @24 kS/s after rdsDecimator (:553): the last n outputs of the last call
        if (!h->rds_alloc) return fail(FMX_E_INVALID, "RDS is off");
        const int64_t lm0 = h->last_m0[(size_t)channel], lm1 = h->last_m1[(size_t)channel];      // (the channel's own count: fmx_last_rds_samples_of)
        if (n > lm1 - lm0) return fail(FMX_E_INVALID, "n exceeds the RDS samples the channel produced in the last call");
        if (n > RDS24_RING) return fail(FMX_E_INVALID, "n exceeds the 8192 RDS samples the library keeps");      // (a call of more than 786432 input samples)
        char *o = (char *)dst;
        for (int64_t m = lm1 - n; m < lm1;) {
            const int64_t pos = m & (RDS24_RING - 1);
            const int64_t run = std::min<int64_t>(RDS24_RING - pos, lm1 - m);
            HIPCHK(hipMemcpy(o, (const char *)(h->R.rds24 + (size_t)channel * RDS24_RING) + pos * sizeof(float2), (size_t)run * sizeof(float2), hipMemcpyDeviceToHost));
            o += run * sizeof(float2); m += run;
        }
        return FMX_OK; }
    default: return fail(FMX_E_INVALID, "unknown tap id");
    }
    // samples j in [J1-n, J1) live at ring index (j - delay) & (cap-1); before the stream start they are 0
    char *out = (char *)dst;
    for (int64_t j = J1 - n; j < J1;) {
        const int64_t jv = j - delay;
        if (jv < 0) { std::memset(out, 0, elem); out += elem; j++; continue; }
        const int64_t pos = jv & (cap - 1);
        const int64_t run = std::min<int64_t>(cap - pos, J1 - j);
        HIPCHK(hipMemcpy(out, base + pos * elem, (size_t)(run * elem), hipMemcpyDeviceToHost));
        out += run * elem; j += run;
    }
    return FMX_OK;
}

int fmx_rds_bits(fmx_handle h, int32_t channel, uint8_t *bits, int32_t capacity, int32_t *n_bits) {
    if (!h || channel < 0 || channel >= h->channels || !n_bits || capacity < 0) return fail(FMX_E_INVALID, "bad argument");
    *n_bits = 0;
    if (!h->rds_alloc) return FMX_OK;
    RdsState st;
    FMXCHK(fetch_rds_state(h, channel, &st));
    const RingTake t = ring_take(st.nbits, h->rd.bits[channel], RDS_BITS_CAP, bits ? capacity : 0);   // (ring overrun: oldest bits lost)
    FMXCHK(read_ring(h->R.bits + (size_t)channel * RDS_BITS_CAP, RDS_BITS_CAP, t, [&](int64_t k, uint8_t b) { bits[k] = b; }));
    h->rd.bits[channel] = (int32_t)t.next();
    *n_bits = (int32_t)t.count;
    return FMX_OK;
}

int fmx_rds_symbols(fmx_handle h, int32_t channel, float *iq, int32_t capacity, int32_t *n_symbols) {
    if (!h || channel < 0 || channel >= h->channels || !n_symbols || capacity < 0) return fail(FMX_E_INVALID, "bad argument");
    *n_symbols = 0;
    if (!h->rds_alloc) return FMX_OK;
    RdsState st;
    FMXCHK(fetch_rds_state(h, channel, &st));
    int32_t &rd = h->rd.symbols[(size_t)channel];
    if (st.nbits < rd) rd = 0;                  // (the count went backwards: start over)
    const RingTake t = ring_take(st.nbits, rd, RDS_SYM_CAP, iq ? capacity : 0);        // (ring overrun: oldest symbols lost)
    FMXCHK(read_ring(h->R.sym + (size_t)channel * RDS_SYM_CAP, RDS_SYM_CAP, t, [&](int64_t k, float2 v) { iq[2 * k] = v.x; iq[2 * k + 1] = v.y; }));
    *n_symbols = (int32_t)t.count;
    rd = (int32_t)t.next();
    return FMX_OK;
}

int64_t fmx_last_fm_samples(fmx_handle h) { return h ? (int64_t)(h->last_J1 - h->last_J0) : 0; }
int fmx_scan_results(fmx_handle h, int32_t channel, fmx_scan_result *out, int32_t capacity, int32_t *n_results) {
    if (!h || !n_results || channel < 0 || channel >= h->channels || capacity < 0 || (capacity > 0 && !out)) return fail(FMX_E_INVALID, "bad argument");
    *n_results = 0;
    if (!h->scan_alloc) return FMX_OK;
    FMXCHK(device_idle(h));
    std::lock_guard<std::mutex> lk(h->mtx);
    const size_t c = (size_t)channel;
    const RingTake t = ring_take(h->scan_blocks[c], h->rd.scan[c], scan::RING, capacity);      // (a caller that fell behind: the oldest records are gone)
    FMXCHK(read_ring(h->d_scan_rec + c * scan::RING, scan::RING, t, [&](int64_t k, float2 rec) {
        const int64_t b = t.from + k;
        const size_t slot = c * scan::RING + (size_t)ring_slot(b, scan::RING);
        fmx_scan_result &r = out[k];
        r.block = b; r.end_sample = h->scan_end[slot];
        r.signal_db = rec.x; r.noise_db = rec.y;
        r.found = (r.signal_db - r.noise_db > (float)h->scan_rec_thr[slot]) ? 1 : 0;   // fm-processor.cpp:489 (float against int16_t)
        r.reserved = 0;
    }));
    h->rd.scan[c] = t.next();
    *n_results = (int32_t)t.count;
    return FMX_OK;
}

int fmx_mod_records(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_mod_record *out, int32_t capacity_per_channel, int32_t *n_records) {
    return read_records(h, &fmx_handle_s::mod_tap, &fmx_handle_s::d_meter_ring, meter::RING, first_channel, n_channels, out, capacity_per_channel, n_records);
}

// Hz per unit of the demodulator output, in the reference's own float order: fm_Demodulator's constructor (fm-demodulator.cpp:58-64) makes K_FM of three
// floats, demodulate () ends in res = 20 (r - afc) / K_FM (:198); r radians per sample are r fmRate / (2 pi) Hz
int fmx_mod_hz_per_unit(int32_t decoder, int32_t fmRate, double *hz) {
    if (!hz || fmRate < 1) return fail(FMX_E_INVALID, "bad argument");
    switch (decoder) {
    case 2: case 3: case 4: break;      // pllC's phaseIncr (NcoPhase += phaseIncr, pllC.cpp:80-84), the two atan2 discriminators (:169-175)
    case 1: return fail(FMX_E_UNSUPPORTED, "the AM decoder's output is the carrier's relative amplitude, not a frequency");
    case 5: return fail(FMX_E_UNSUPPORTED, "the RealBB decoder's value is half the arcsine of sin (phase step) from a table (fm-demodulator.cpp:180-186): linear in frequency only for small deviations");
    case 6: return fail(FMX_E_UNSUPPORTED, "the Diff decoder's value is a difference quotient over two samples divided by sqrt (2) (fm-demodulator.cpp:190-191), not an angle per sample");
    default: return fail(FMX_E_INVALID, "decoder must be 1..6");
    }
    const float F_G = (float)(0.65 * fmRate / 2), Delta_F = (float)(0.95 * fmRate / 2);
    const float B_FM = 2 * (Delta_F + F_G);
    const float K_FM = (float)((double)(2 * B_FM) * design::kPi / (double)F_G);
    *hz = (double)K_FM / 20.0 * (double)fmRate / (2.0 * design::kPi);
    return FMX_OK;
}

int fmx_audio_records(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_audio_record *out, int32_t capacity_per_channel, int32_t *n_records) {
    return read_records(h, &fmx_handle_s::audio_tap, &fmx_handle_s::d_loud_ring, loud::RING, first_channel, n_channels, out, capacity_per_channel, n_records);
}

// BS.1770-4 over one channel's records (include/fmx.h): blocks of 4 consecutive records, the absolute gate at -70 LUFS, the relative gate 10 LU below the
// level of what passed it
int fmx_audio_loudness(const fmx_audio_record *recs, int32_t n, fmx_loudness *out) {
    if (!out || n < 0 || (n > 0 && !recs)) return fail(FMX_E_INVALID, "bad argument");
    const auto lufs = [](double z) { return z > 0.0 ? -0.691 + 10.0 * std::log10(z) : -HUGE_VAL; };
    const auto dbfs = [](double p) { return p > 0.0 ? 20.0 * std::log10(p) : -HUGE_VAL; };
    fmx_loudness L{};
    L.momentary_lufs = L.short_term_lufs = L.integrated_lufs = -HUGE_VAL;
    std::vector<double> zb;                 // z_j of every block
    double sc = 0.0, sl = 0.0, sr = 0.0, pl = 0.0, pr = 0.0;
    int64_t run = 0;                        // records up to this one with consecutive index
    for (int32_t i = 0; i < n; i++) {
        run = (i > 0 && recs[i].index == recs[i - 1].index + 1) ? run + 1 : 1;
        if (run >= 4) {
            double z = 0.0;
            for (int k = 3; k >= 0; k--) z += (double)recs[i - k].kms_l + (double)recs[i - k].kms_r;
            zb.push_back(z / 4.0);
        }
        sc += (double)recs[i].cross; sl += (double)recs[i].ms_l; sr += (double)recs[i].ms_r;
        pl = std::max(pl, (double)recs[i].peak_l); pr = std::max(pr, (double)recs[i].peak_r);
    }
    if (run >= 4) L.momentary_lufs = lufs(zb.back());
    if (run >= 30) {
        double z = 0.0;
        for (int k = 29; k >= 0; k--) z += (double)recs[n - 1 - k].kms_l + (double)recs[n - 1 - k].kms_r;
        L.short_term_lufs = lufs(z / 30.0);
    }
    L.blocks_total = (int64_t)zb.size();
    double za = 0.0; int64_t na = 0;
    for (double z : zb) if (lufs(z) > -70.0) { za += z; na++; }
    if (na > 0) {
        const double rel = lufs(za / (double)na) - 10.0;
        double zg = 0.0; int64_t ng = 0;
        for (double z : zb) if (lufs(z) > -70.0 && lufs(z) > rel) { zg += z; ng++; }
        L.blocks_gated = ng;
        if (ng > 0) L.integrated_lufs = lufs(zg / (double)ng);
    }
    const double den = std::sqrt(sl * sr);
    L.correlation = den > 0.0 ? sc / den : 0.0;
    L.peak_dbfs_l = dbfs(pl); L.peak_dbfs_r = dbfs(pr);
    *out = L;
    return FMX_OK;
}

int fmx_rx_records(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_rx_record *out, int32_t capacity_per_channel, int32_t *n_records) {
    return read_records(h, &fmx_handle_s::rx_tap, &fmx_handle_s::d_rx_ring, rx::RING, first_channel, n_channels, out, capacity_per_channel, n_records);
}

// the reception figures of one channel's records (include/fmx.h): level, the M2M4 carrier-to-noise estimate, the envelope's depth, the lag-1 offset
int fmx_rx_quality_of(const fmx_rx_record *recs, int32_t n, int32_t fmRate, fmx_rx_quality *out) {
    if (!out || !recs || n <= 0 || fmRate < 1) return fail(FMX_E_INVALID, "bad argument");
    double s2 = 0.0, s4 = 0.0, sre = 0.0, sim = 0.0, depth = 0.0;
    for (int32_t i = 0; i < n; i++) {
        s2 += (double)recs[i].p_mean; s4 += (double)recs[i].p2_mean;
        sre += (double)recs[i].r1_re; sim += (double)recs[i].r1_im;
        if (recs[i].p_max > 0.0f) {
            const double a = std::sqrt((double)recs[i].p_max), b = std::sqrt(std::max(0.0, (double)recs[i].p_min));
            depth = std::max(depth, (a - b) / (a + b));
        }
    }
    const double M2 = s2 / (double)n, M4 = s4 / (double)n;
    fmx_rx_quality Q{};
    Q.level_dbfs = M2 > 0.0 ? 10.0 * std::log10(M2) : -HUGE_VAL;
    const double disc = 2.0 * M2 * M2 - M4;
    if (disc <= 0.0) Q.cnr_db = -HUGE_VAL;
    else {
        const double S = std::sqrt(disc), N = M2 - S;
        Q.cnr_db = N <= 0.0 ? HUGE_VAL : 10.0 * std::log10(S / N);
    }
    Q.am_depth = depth;
    Q.offset_hz = std::atan2(sim, sre) * (double)fmRate / (2.0 * design::kPi);
    Q.windows = n;
    *out = Q;
    return FMX_OK;
}

int fmx_rds_meter_records(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_rds_meter_record *out, int32_t capacity_per_channel, int32_t *n_records) {
    return read_records(h, &fmx_handle_s::rdsm_tap, &fmx_handle_s::d_rdsm_ring, rdsm::RING, first_channel, n_channels, out, capacity_per_channel, n_records);
}

// the calibration of a channel's RDS meter (include/fmx.h), from the taps the handle runs with: the 57 kHz band-pass (ensure_rds: only the real part of
// the complex kernel's result is kept), the analytic-signal filter's factor 3 (rds_spectrum), rdsDecimator's complex kernel; in front of the demodulator
// the channel's front-end taps (with the input filter as a block machine on a handle that runs it so) and the one-sample phase difference
int fmx_rds_meter_cal(fmx_handle h, int32_t channel, fmx_rds_meter_calib *out) {
    if (!h || !out || channel < 0 || channel >= h->channels) return fail(FMX_E_INVALID, "bad argument");
    // the response of real taps g [0 .. n) at `turns` cycles per sample, about the delay `centre`, in double
    auto fir_response = [](const float *g, int n, int stride, double turns, double centre) -> std::complex<double> {
        double re = 0.0, im = 0.0;
        for (int i = 0; i < n; i++) {
            const double a = -2.0 * design::kPi * turns * ((double)i - centre);
            re += (double)g[(size_t)i * (size_t)stride] * std::cos(a); im += (double)g[(size_t)i * (size_t)stride] * std::sin(a);
        }
        return {re, im};
    };
    const int32_t fmRate = h->cfg.fmRate, inRate = h->cfg.inputRate;
    std::vector<float> G;
    int32_t decoder = 0, ola_bw = 0;
    {
        std::lock_guard<std::mutex> lk(h->mtx);
        if (h->sets_dirty) { HIPCHK(hipSetDevice(h->cfg.device)); int rc = ensure_sets(h); if (rc) return rc; h->params_dirty = true; }
        decoder = h->params[(size_t)channel].decoder;
        if (h->ola_mode) ola_bw = h->user[(size_t)channel].bandwidth > 0 ? h->user[(size_t)channel].bandwidth : 0;
        const FrontSet &fs = h->h_front_sets[(size_t)h->params[(size_t)channel].front_set];
        const float *t = &h->h_front_taps[(size_t)h->params[(size_t)channel].front_set * A_TAPS_STRIDE];
        G.assign(A_TAPS_STRIDE, 0.f);       // (FIR order: G [k], k = 12 d + off - r, as fmx_get_taps hands them out)
        for (int d = 0; d < fs.nd; d++) for (int r = 0; r < DECIM; r++) {
            const int k = 12 * d + fs.off - r;
            if (k >= 0 && k < A_TAPS_STRIDE) G[(size_t)k] = t[(d + 1) * DECIM + r];
        }
    }
    double hz = 0.0;
    { const int rc = fmx_mod_hz_per_unit(decoder, fmRate, &hz); if (rc) return rc; }      // (FMX_E_UNSUPPORTED: the decoder's output is no frequency)
    fmx_rds_meter_calib K{};
    const double sub = 3.0 * 19000.0;
    const std::vector<float> bp = design::bandpass(768, 3 * 19000 - 4800 / 2, 3 * 19000 + 4800 / 2, fmRate);
    const std::complex<double> Hbp = fir_response(bp.data(), 768, 2, sub / (double)fmRate, 384.0);      // (the real parts: Re (a * s) = a * Re (s))
    const std::vector<float> dk = design::decim_complex(11, 24000 / 2, fmRate);
    std::complex<double> D0(0.0, 0.0);
    for (int i = 0; i < 11; i++) D0 += std::complex<double>((double)dk[(size_t)2 * i], (double)dk[(size_t)2 * i + 1]);
    K.gain = 3.0 * std::abs(Hbp) * std::abs(D0);
    K.phase0_deg = (std::arg(D0) + std::arg(Hbp)) * 180.0 / design::kPi;
    // the RF path: the sidebands of a small sub-carrier lie 57 kHz on either side of the carrier; the response relative to the carrier's, their mean
    const double tr = sub / (double)inRate;
    const double g0 = std::abs(fir_response(G.data(), (int)G.size(), 1, 0.0, 0.0));
    double rf = g0 > 0.0 ? 0.5 * (std::abs(fir_response(G.data(), (int)G.size(), 1, tr, 0.0)) + std::abs(fir_response(G.data(), (int)G.size(), 1, -tr, 0.0))) / g0 : 0.0;
    if (ola_bw > 0) {
        const std::vector<float> L = design::lowpass(251, ola_bw / 2, inRate);      // (ola_take_settings)
        const double l0 = std::abs(fir_response(L.data(), 251, 1, 0.0, 0.0));
        rf *= 0.5 * (std::abs(fir_response(L.data(), 251, 1, tr, 0.0)) + std::abs(fir_response(L.data(), 251, 1, -tr, 0.0))) / l0;
    }
    const double x = design::kPi * sub / (double)fmRate;
    K.path_57k = rf * std::sin(x) / x;
    *out = K;
    return FMX_OK;
}

// the figures of one channel's RDS-meter records (include/fmx.h): the covariance of I and Q, its eigenvalues and its axis
int fmx_rds_meter_figures(const fmx_rds_meter_record *recs, int32_t n, const fmx_rds_meter_calib *cal, double hz_per_unit, fmx_rds_figures *out) {
    if (!out || !recs || !cal || n <= 0) return fail(FMX_E_INVALID, "bad argument");
    double A = 0.0, B = 0.0, Cq = 0.0, mi = 0.0, mq = 0.0, pmax = 0.0;
    for (int32_t i = 0; i < n; i++) {
        A += (double)recs[i].ii_mean; B += (double)recs[i].qq_mean; Cq += (double)recs[i].iq_mean;
        mi += (double)recs[i].i_mean; mq += (double)recs[i].q_mean;
        pmax = std::max(pmax, (double)recs[i].p_max);
    }
    A /= (double)n; B /= (double)n; Cq /= (double)n; mi /= (double)n; mq /= (double)n;
    const double a = A - mi * mi, b = B - mq * mq, c = Cq - mi * mq;
    const double r = std::hypot((a - b) / 2.0, c);
    const double lp = (a + b) / 2.0 + r, lm = (a + b) / 2.0 - r;
    const double K = hz_per_unit / (cal->gain * cal->path_57k);
    fmx_rds_figures F{};
    F.injection_rms_hz = std::sqrt(std::max(lp - lm, 0.0)) * K;
    F.injection_peak_hz = std::sqrt(pmax) * K;
    F.carrier_hz = std::hypot(mi, mq) * K;
    if (lp <= 0.0) { F.phase_deg = 0.0; F.axis_db = -HUGE_VAL; }
    else {
        double ph = 0.5 * std::atan2(2.0 * c, a - b) * 180.0 / design::kPi - cal->phase0_deg;
        ph = std::fmod(ph, 180.0);                 // (an axis: modulo 180)
        if (ph <= -45.0) ph += 180.0; else if (ph > 135.0) ph -= 180.0;
        F.phase_deg = ph;
        F.axis_db = lm <= 0.0 ? HUGE_VAL : 10.0 * std::log10(lp / lm);
    }
    F.windows = n;
    *out = F;
    return FMX_OK;
}

// the spectrum meter's records of one stream: which record a ring slot holds is the host's (SlotTap::tags); behind the handle's last call only
int fmx_spectrum_read(fmx_handle h, int32_t stream, fmx_spectrum_record *recs, float *mean, float *peak, int32_t capacity, int32_t *n_records) {
    if (!h || !n_records) return fail(FMX_E_INVALID, "null argument");
    *n_records = 0;
    if (stream < 0 || stream >= h->streams) return fail(FMX_E_INVALID, "stream out of range");
    if (capacity < 0 || (capacity > 0 && (!recs || !mean))) return fail(FMX_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mtx);
    SlotTap &T = h->spec_tap;
    if (!T.started() || capacity == 0) return FMX_OK;
    std::vector<int64_t> have;
    T.pending((size_t)stream, capacity, have);      // (older ones were read, or overwritten: the gap shows in `index`)
    const int n = (int)have.size();
    if (n == 0) return FMX_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->rd_stream) HIPCHK(hipStreamCreateWithFlags(&h->rd_stream, hipStreamNonBlocking));
    if (h->ev_spec_set) HIPCHK(hipStreamWaitEvent(h->rd_stream, h->ev_spec, 0));
    const float *ring = h->d_spec_ring + (size_t)T.slot[(size_t)stream] * spec::RING * 2 * spec::N;
    for (int i = 0; i < n; i++) {
        const int64_t r = have[i];
        recs[i] = fmx_spectrum_record{r, spec::record_end(r, h->spec_B, h->spec_S), h->spec_B, h->spec_S};
        const float *slot = ring + (size_t)(r & (spec::RING - 1)) * 2 * spec::N;
        HIPCHK(hipMemcpyAsync(mean + (size_t)i * spec::N, slot, sizeof(float) * spec::N, hipMemcpyDeviceToHost, h->rd_stream));
        if (peak) HIPCHK(hipMemcpyAsync(peak + (size_t)i * spec::N, slot + spec::N, sizeof(float) * spec::N, hipMemcpyDeviceToHost, h->rd_stream));
    }
    HIPCHK(hipStreamSynchronize(h->rd_stream));
    T.commit((size_t)stream, have[(size_t)n - 1] + 1);
    *n_records = n;
    return FMX_OK;
}

int fmx_spectrum_figures(const fmx_spectrum_find *cfg, const float *mean, const float *peak, fmx_spectrum_figs *out) {
    const char *why = "";
    const int rc = spec::figures(cfg, mean, peak, out, &why);
    return rc == FMX_OK ? FMX_OK : fail(rc, why);
}

// The multiplex spectrum meter's records of a range of channels.  Which record a ring slot holds is the host's (SlotTap::tags).  The records of the
// whole range are gathered on the device into one staging array (mpx_gather_kernel) behind the handle's last call, and leave it in ONE copy to pinned
// memory (a range of more than MPX_READ_BATCH records: one copy per 4096 records, 64 MB of staging at the most).  The cursors move only when every copy
// has arrived: a read that fails loses nothing.
constexpr int64_t MPX_READ_BATCH = 4096;
int fmx_mpx_spectrum_read(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_mpx_record *recs, float *mean, float *peak,
                          int32_t capacity_per_channel, int32_t *n_records) {
    if (!h || !n_records) return fail(FMX_E_INVALID, "null argument");
    if (first_channel < 0 || n_channels < 1 || n_channels > h->channels || first_channel > h->channels - n_channels) return fail(FMX_E_INVALID, "channel range out of range");
    for (int q = 0; q < n_channels; q++) n_records[q] = 0;
    const int32_t cap = capacity_per_channel;
    if (cap < 0 || (cap > 0 && (!recs || !mean))) return fail(FMX_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mtx);
    SlotTap &T = h->mpx_tap; GatherStage &S = h->mpx_stage;
    if (!T.started() || cap == 0) return FMX_OK;
    // what the range has to hand out: per record its place in the ring and in the caller's arrays
    S.src.clear();
    std::vector<size_t> dst;
    std::vector<int64_t> next((size_t)n_channels, -1), have;
    std::vector<int32_t> count((size_t)n_channels, 0);
    for (int q = 0; q < n_channels; q++) {
        const size_t ch = (size_t)(first_channel + q);
        T.pending(ch, cap, have);      // (older ones were read, or overwritten: the gap shows in `index`)
        const int n = (int)have.size();
        for (int i = 0; i < n; i++) {
            const int64_t r = have[(size_t)i];
            const size_t at = (size_t)q * (size_t)cap + (size_t)i;
            recs[at] = fmx_mpx_record{r, spec::record_end(r, h->mpx_B, h->mpx_S), h->mpx_B, h->mpx_S};
            S.src.push_back(T.slot[ch] * mpx::RING + (int32_t)(r & (mpx::RING - 1)));
            dst.push_back(at);
        }
        if (n > 0) { next[(size_t)q] = have[(size_t)n - 1] + 1; count[(size_t)q] = n; }
    }
    const int64_t total = (int64_t)dst.size();
    if (total == 0) return FMX_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->rd_stream) HIPCHK(hipStreamCreateWithFlags(&h->rd_stream, hipStreamNonBlocking));
    if (h->ev_mpx_set) HIPCHK(hipStreamWaitEvent(h->rd_stream, h->ev_mpx, 0));
    const int64_t batch = std::min(total, MPX_READ_BATCH);
    FMXCHK(S.ensure(h->mem, batch, 2 * mpx::BINS));
    g_launch_err = hipSuccess;
    for (int64_t o = 0; o < total; o += batch) {
        const int64_t m = std::min(batch, total - o);
        HIPCHK(hipMemcpyAsync(S.d_src, S.src.data() + o, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, h->rd_stream));
        launch_mpx_gather(h->d_mpx_ring, S.d_src, S.d_stage, (int)m, h->rd_stream);
        HIPCHK(g_launch_err);
        HIPCHK(hipMemcpyAsync(S.h_stage, S.d_stage, sizeof(float) * (size_t)m * 2 * mpx::BINS, hipMemcpyDeviceToHost, h->rd_stream));
        HIPCHK(hipStreamSynchronize(h->rd_stream));
        for (int64_t i = 0; i < m; i++) {
            const float *from = S.h_stage + (size_t)i * 2 * mpx::BINS;
            std::memcpy(mean + dst[(size_t)(o + i)] * mpx::BINS, from, sizeof(float) * mpx::BINS);
            if (peak) std::memcpy(peak + dst[(size_t)(o + i)] * mpx::BINS, from + mpx::BINS, sizeof(float) * mpx::BINS);
        }
    }
    for (int q = 0; q < n_channels; q++)
        if (count[(size_t)q] > 0) { T.commit((size_t)(first_channel + q), next[(size_t)q]); n_records[q] = count[(size_t)q]; }
    return FMX_OK;
}

int fmx_mpx_figures(const fmx_mpx_find *cfg, const float *mean, const float *peak, fmx_mpx_figs *out) {
    const char *why = "";
    const int rc = mpx::figures(cfg, mean, peak, out, &why);
    return rc == FMX_OK ? FMX_OK : fail(rc, why);
}

// The sub-carrier decoder's blocks of a range of channels.  Which block a ring slot holds is the host's (SlotTap::tags).  Per channel the run of
// consecutive blocks from the oldest one not yet read; the runs of the whole range are gathered on the device into one staging array (sca_gather_kernel)
// behind the handle's last call, and leave it in ONE copy to pinned memory (a range of more than SCA_READ_BATCH blocks: one copy per 65 536 blocks, 63 MB
// of staging at the most).  The cursors move only when every copy has arrived: a read that fails loses nothing.
constexpr int64_t SCA_READ_BATCH = 65536;
int fmx_sca_read(fmx_handle h, int32_t first_channel, int32_t n_channels, int64_t *first_block, float *audio, float *level,
                 int32_t capacity_blocks_per_channel, int32_t *n_blocks) {
    if (!h || !n_blocks || !first_block) return fail(FMX_E_INVALID, "null argument");
    if (first_channel < 0 || n_channels < 1 || n_channels > h->channels || first_channel > h->channels - n_channels) return fail(FMX_E_INVALID, "channel range out of range");
    for (int q = 0; q < n_channels; q++) { n_blocks[q] = 0; first_block[q] = -1; }
    const int32_t cap = capacity_blocks_per_channel;
    if (cap < 0 || (cap > 0 && !audio)) return fail(FMX_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mtx);
    SlotTap &T = h->sca_tap; GatherStage &S = h->sca_stage;
    if (!T.started() || cap == 0) return FMX_OK;
    constexpr int REC = sca::BLOCK_AUDIO + 1;
    S.src.clear();
    std::vector<size_t> dst;
    std::vector<int64_t> from((size_t)n_channels, -1);
    std::vector<int32_t> count((size_t)n_channels, 0);
    for (int q = 0; q < n_channels; q++) {
        const size_t ch = (size_t)(first_channel + q);
        const SlotRun r = T.run(ch, cap);      // (older ones were read, or overwritten: the gap shows in first_block; the run ends at a gap)
        for (int32_t n = 0; n < r.count; n++) {
            S.src.push_back(T.slot[ch] * sca::RING + (int32_t)((r.from + n) % sca::RING));
            dst.push_back((size_t)q * (size_t)cap + (size_t)n);
        }
        from[(size_t)q] = r.from; count[(size_t)q] = r.count;
    }
    const int64_t total = (int64_t)dst.size();
    if (total == 0) return FMX_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->rd_stream) HIPCHK(hipStreamCreateWithFlags(&h->rd_stream, hipStreamNonBlocking));
    if (h->ev_sca_set) HIPCHK(hipStreamWaitEvent(h->rd_stream, h->ev_sca, 0));
    const int64_t batch = std::min(total, SCA_READ_BATCH);
    FMXCHK(S.ensure(h->mem, batch, REC));
    g_launch_err = hipSuccess;
    for (int64_t o = 0; o < total; o += batch) {
        const int64_t m = std::min(batch, total - o);
        HIPCHK(hipMemcpyAsync(S.d_src, S.src.data() + o, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, h->rd_stream));
        launch_sca_gather(h->d_sca_audio, h->d_sca_level, S.d_src, S.d_stage, (int)m, h->rd_stream);
        HIPCHK(g_launch_err);
        HIPCHK(hipMemcpyAsync(S.h_stage, S.d_stage, sizeof(float) * (size_t)m * REC, hipMemcpyDeviceToHost, h->rd_stream));
        HIPCHK(hipStreamSynchronize(h->rd_stream));
        for (int64_t i = 0; i < m; i++) {
            const float *src = S.h_stage + (size_t)i * REC;
            std::memcpy(audio + dst[(size_t)(o + i)] * sca::BLOCK_AUDIO, src, sizeof(float) * sca::BLOCK_AUDIO);
            if (level) level[dst[(size_t)(o + i)]] = src[sca::BLOCK_AUDIO];
        }
    }
    for (int q = 0; q < n_channels; q++)
        if (count[(size_t)q] > 0) {
            T.commit((size_t)(first_channel + q), from[(size_t)q] + count[(size_t)q]);
            first_block[q] = from[(size_t)q]; n_blocks[q] = count[(size_t)q];
        }
    return FMX_OK;
}

int fmx_sca_taps(const fmx_sca_config *cfg, int32_t fmRate, int32_t which, float *dst, int32_t capacity, int32_t *n) {
    if (!n) return fail(FMX_E_INVALID, "fmx_sca_taps: n is null");
    const fmx_sca_config want = cfg ? *cfg : sca::default_config();
    if (const char *why = sca::config_error(&want, fmRate)) return fail(FMX_E_INVALID, std::string("fmx_sca_taps: ") + why);
    if (which != 0 && which != 1) return fail(FMX_E_INVALID, "fmx_sca_taps: which must be 0 (g) or 1 (a)");
    if (capacity < 0 || (capacity > 0 && !dst)) return fail(FMX_E_INVALID, "fmx_sca_taps: dst is null");
    const std::vector<float> t = which == 0 ? sca::design_band(want, fmRate) : sca::design_audio(want, fmRate);
    *n = (int32_t)t.size();
    std::copy(t.begin(), t.begin() + std::min<int32_t>(capacity, *n), dst);
    return FMX_OK;
}

int fmx_sca_info(int32_t fmRate, fmx_sca_info_t *out) {
    if (!out) return fail(FMX_E_INVALID, "fmx_sca_info: out is null");
    if (fmRate < 8000 || fmRate > 1000000 || fmRate % 8 != 0) return fail(FMX_E_INVALID, "fmx_sca_info: fmRate must be a multiple of 8 in [8000, 1000000]");
    out->audio_rate_hz = fmRate / (sca::D1 * sca::D2); out->block_audio = sca::BLOCK_AUDIO; out->block_fm = sca::BLOCK_FM; out->lookback_fm = sca::LOOKBACK;
    out->delay_fm = (sca::NG - 1) / 2.0 + sca::D1 * ((sca::NLP - 1) / 2.0);
    out->ring_blocks = sca::RING; out->bytes_per_channel = (int32_t)sca::BYTES_PER_CHANNEL;
    return FMX_OK;
}

// The monitoring feed's blocks of a range of channels, for both read-outs.  Which block a ring slot holds is the host's (SlotTap::tags).  Per
// channel the run of consecutive blocks from the oldest one not yet read.  fmx_feed_read gathers the runs of the whole range on the device into one
// staging array (feed_gather_kernel, which converts the format) behind the handle's last call, and they leave it in one copy of the audio and one of the
// powers to pinned memory (a range of more than FEED_READ_BATCH blocks: a pair of copies per 65 536 blocks, 42 MB of staging at the most);
// fmx_feed_read_device gathers them straight to their places in the caller's device buffers on the caller's stream.  The cursors move only when everything
// is queued or has arrived: a read that fails loses nothing.
namespace {

constexpr int64_t FEED_READ_BATCH = 65536;

struct FeedRuns {
    std::vector<int64_t> from;                 // per channel of the range: the run's first block (-1: none)
    std::vector<int32_t> count;
};

// under mtx, lists the runs: ring block h->feed_src [i] goes to block h->feed_dst [i] (q cap + n) of the output; both lists are the handle's, so that
// an asynchronous upload never reads a vector that has gone
void feed_runs(fmx_handle h, int32_t first_channel, int32_t n_channels, int32_t cap, FeedRuns &runs) {
    runs.from.assign((size_t)n_channels, -1); runs.count.assign((size_t)n_channels, 0);
    h->feed_src.clear(); h->feed_dst.clear();
    const SlotTap &T = h->feed_tap;
    if (!T.started() || cap == 0) return;
    for (int q = 0; q < n_channels; q++) {
        const size_t ch = (size_t)(first_channel + q);
        const SlotRun r = T.run(ch, cap);      // (older ones were read, or overwritten: the gap shows in first_block; the run ends at a gap)
        for (int32_t n = 0; n < r.count; n++) {
            h->feed_src.push_back(T.slot[ch] * feed::RING + (int32_t)((r.from + n) % feed::RING));
            h->feed_dst.push_back((int32_t)((int64_t)q * cap + n));
        }
        runs.from[(size_t)q] = r.from; runs.count[(size_t)q] = r.count;
    }
}

int feed_check(fmx_handle h, int32_t first_channel, int32_t n_channels, int64_t *first_block, const void *audio, int32_t format, int32_t cap, int32_t *n_blocks,
               const char *who) {
    if (!h || !n_blocks || !first_block) return fail(FMX_E_INVALID, std::string(who) + ": null argument");
    if (first_channel < 0 || n_channels < 1 || n_channels > h->channels || first_channel > h->channels - n_channels)
        return fail(FMX_E_INVALID, std::string(who) + ": channel range out of range");
    for (int q = 0; q < n_channels; q++) { n_blocks[q] = 0; first_block[q] = -1; }
    if (format != FMX_FEED_F32 && format != FMX_FEED_S16) return fail(FMX_E_INVALID, std::string(who) + ": format must be FMX_FEED_F32 or FMX_FEED_S16");
    if (cap < 0) return fail(FMX_E_INVALID, std::string(who) + ": capacity_blocks_per_channel is negative");
    if (cap > 0 && !audio) return fail(FMX_E_INVALID, std::string(who) + ": audio is null");
    if (cap == 0 && audio) return fail(FMX_E_INVALID, std::string(who) + ": capacity_blocks_per_channel is 0 with an audio buffer");
    if ((int64_t)n_channels * cap > INT32_MAX) return fail(FMX_E_TOO_LARGE, std::string(who) + ": n_channels x capacity_blocks_per_channel exceeds 2^31 - 1 blocks");
    return FMX_OK;
}

// the index arrays of a gather: src then dst, feed_src_cap entries each, behind whatever still reads them
int feed_index_arrays(fmx_handle h, int64_t n, hipStream_t s) {
    if (h->ev_feed_rd_set) HIPCHK(hipStreamWaitEvent(s, h->ev_feed_rd, 0));
    if (n > h->feed_src_cap) {
        if (h->ev_feed_rd_set) HIPCHK(hipEventSynchronize(h->ev_feed_rd));
        h->mem.release(h->d_feed_src); h->feed_src_cap = 0;
        FMXCHK(h->mem.alloc(h->d_feed_src, (size_t)(2 * n)));
        h->feed_src_cap = n;
    }
    return FMX_OK;
}

void feed_commit(fmx_handle h, int32_t first_channel, int32_t n_channels, const FeedRuns &runs, int64_t *first_block, int32_t *n_blocks) {
    for (int q = 0; q < n_channels; q++)
        if (runs.count[(size_t)q] > 0) {
            h->feed_tap.commit((size_t)(first_channel + q), runs.from[(size_t)q] + runs.count[(size_t)q]);
            first_block[q] = runs.from[(size_t)q]; n_blocks[q] = runs.count[(size_t)q];
        }
}

}  // namespace

int fmx_feed_read(fmx_handle h, int32_t first_channel, int32_t n_channels, int64_t *first_block, void *audio, int32_t format, float *power,
                  int32_t capacity_blocks_per_channel, int32_t *n_blocks) {
    const int32_t cap = capacity_blocks_per_channel;
    FMXCHK(feed_check(h, first_channel, n_channels, first_block, audio, format, cap, n_blocks, "fmx_feed_read"));
    std::lock_guard<std::mutex> lk(h->mtx);
    FeedRuns runs;
    feed_runs(h, first_channel, n_channels, cap, runs);
    const int64_t total = (int64_t)h->feed_dst.size();
    if (total == 0) return FMX_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    if (!h->rd_stream) HIPCHK(hipStreamCreateWithFlags(&h->rd_stream, hipStreamNonBlocking));
    if (h->ev_feed_set) HIPCHK(hipStreamWaitEvent(h->rd_stream, h->ev_feed, 0));
    const int64_t batch = std::min(total, FEED_READ_BATCH);
    FMXCHK(feed_index_arrays(h, batch, h->rd_stream));
    if (batch > h->feed_stage_blocks) {
        h->mem.release(h->d_feed_stage); h->mem.release(h->h_feed_stage); h->feed_stage_blocks = 0;
        FMXCHK(h->mem.alloc(h->d_feed_stage, (size_t)batch * (feed::BLOCK + 1)));
        FMXCHK(h->mem.alloc_pinned(h->h_feed_stage, (size_t)batch * (feed::BLOCK + 1)));
        h->feed_stage_blocks = batch;
    }
    // (the staging array: the audio of the batch's blocks one behind the other in the asked format, then, from float feed_stage_blocks x 160 on, the powers)
    const size_t esize = format == FMX_FEED_S16 ? sizeof(int16_t) : sizeof(float);
    const size_t pw_at = (size_t)h->feed_stage_blocks * feed::BLOCK;
    std::vector<int32_t> seq((size_t)batch);
    for (int64_t i = 0; i < batch; i++) seq[(size_t)i] = (int32_t)i;
    g_launch_err = hipSuccess;
    for (int64_t o = 0; o < total; o += batch) {
        const int64_t m = std::min(batch, total - o);
        HIPCHK(hipMemcpyAsync(h->d_feed_src, h->feed_src.data() + o, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, h->rd_stream));
        HIPCHK(hipMemcpyAsync(h->d_feed_src + h->feed_src_cap, seq.data(), sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, h->rd_stream));
        launch_feed_gather(h->d_feed_audio, h->d_feed_power, h->d_feed_src, h->d_feed_src + h->feed_src_cap, h->d_feed_stage, format,
                           power ? h->d_feed_stage + pw_at : nullptr, (int)m, h->rd_stream);
        HIPCHK(g_launch_err);
        HIPCHK(hipMemcpyAsync(h->h_feed_stage, h->d_feed_stage, esize * (size_t)m * feed::BLOCK, hipMemcpyDeviceToHost, h->rd_stream));
        if (power) HIPCHK(hipMemcpyAsync(h->h_feed_stage + pw_at, h->d_feed_stage + pw_at, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost, h->rd_stream));
        HIPCHK(hipStreamSynchronize(h->rd_stream));
        for (int64_t i = 0; i < m; i++) {
            const size_t to = (size_t)h->feed_dst[(size_t)(o + i)];
            std::memcpy(static_cast<char *>(audio) + to * feed::BLOCK * esize, reinterpret_cast<const char *>(h->h_feed_stage) + (size_t)i * feed::BLOCK * esize,
                        esize * feed::BLOCK);
            if (power) power[to] = h->h_feed_stage[pw_at + (size_t)i];
        }
    }
    feed_commit(h, first_channel, n_channels, runs, first_block, n_blocks);
    return FMX_OK;
}

int fmx_feed_read_device(fmx_handle h, int32_t first_channel, int32_t n_channels, int64_t *first_block, void *d_audio, int32_t format, float *d_power,
                         int32_t capacity_blocks_per_channel, int32_t *n_blocks, void *hip_stream) {
    const int32_t cap = capacity_blocks_per_channel;
    FMXCHK(feed_check(h, first_channel, n_channels, first_block, d_audio, format, cap, n_blocks, "fmx_feed_read_device"));
    std::lock_guard<std::mutex> lk(h->mtx);
    FeedRuns runs;
    feed_runs(h, first_channel, n_channels, cap, runs);
    const int64_t total = (int64_t)h->feed_dst.size();
    if (total == 0) return FMX_OK;
    HIPCHK(hipSetDevice(h->cfg.device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
    if (h->ev_feed_set) HIPCHK(hipStreamWaitEvent(s, h->ev_feed, 0));
    FMXCHK(feed_index_arrays(h, total, s));
    if (!h->ev_feed_rd) HIPCHK(hipEventCreateWithFlags(&h->ev_feed_rd, hipEventDisableTiming));
    g_launch_err = hipSuccess;
    // (pageable sources: the copies are staged before the call returns)
    HIPCHK(hipMemcpyAsync(h->d_feed_src, h->feed_src.data(), sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->d_feed_src + h->feed_src_cap, h->feed_dst.data(), sizeof(int32_t) * (size_t)total, hipMemcpyHostToDevice, s));
    launch_feed_gather(h->d_feed_audio, h->d_feed_power, h->d_feed_src, h->d_feed_src + h->feed_src_cap, d_audio, format, d_power, (int)total, s);
    HIPCHK(g_launch_err);
    HIPCHK(hipEventRecord(h->ev_feed_rd, s)); h->ev_feed_rd_set = true;
    feed_commit(h, first_channel, n_channels, runs, first_block, n_blocks);
    return FMX_OK;
}

int fmx_feed_taps(float *dst, int32_t capacity, int32_t *n) {
    if (!n) return fail(FMX_E_INVALID, "fmx_feed_taps: n is null");
    if (capacity < 0 || (capacity > 0 && !dst)) return fail(FMX_E_INVALID, "fmx_feed_taps: dst is null");
    const std::vector<float> t = feed::design();
    *n = (int32_t)t.size();
    std::copy(t.begin(), t.begin() + std::min<int32_t>(capacity, *n), dst);
    return FMX_OK;
}

int fmx_feed_info(fmx_feed_info_t *out) {
    if (!out) return fail(FMX_E_INVALID, "fmx_feed_info: out is null");
    out->rate_hz = feed::RATE; out->block_samples = feed::BLOCK; out->block_frames = feed::BLOCK_FRAMES; out->lookback_frames = feed::LOOKBACK;
    out->delay_frames = feed::DELAY_FRAMES; out->ring_blocks = feed::RING; out->bytes_per_channel = (int32_t)feed::BYTES_PER_CHANNEL;
    return FMX_OK;
}

int64_t fmx_pll_replays(fmx_handle h, int32_t channel) { return sum_chan_states(h, channel, [](const ChanState &s) { return s.pll_replays; }); }
int64_t fmx_pll_exact_segments(fmx_handle h, int32_t channel) { return sum_chan_states(h, channel, [](const ChanState &s) { return s.pll_exact_segs; }); }
int32_t fmx_last_front_kernel(fmx_handle h) { return h ? h->last_front_kernel : 0; }
int32_t fmx_last_call_pieces(fmx_handle h) { return h ? h->last_pieces : 0; }
int32_t fmx_last_second_group(fmx_handle h) { return h ? h->last_second_group : 0; }
int64_t fmx_last_rds_samples_of(fmx_handle h, int32_t channel) {
    if (!h || !h->rds_alloc || channel < 0 || channel >= h->channels) return 0;
    return h->last_m1[(size_t)channel] - h->last_m0[(size_t)channel];
}
int64_t fmx_last_rds_samples(fmx_handle h) { return fmx_last_rds_samples_of(h, 0); }

int fmx_rds_decode(fmx_handle h, int32_t channel, fmx_rds_info *info) {
    if (!h || channel < 0 || channel >= h->channels || !info) return fail(FMX_E_INVALID, "bad argument");
    if ((int)h->rd.dec.size() != h->channels) h->rd.dec.assign((size_t)h->channels, fmx::RdsGroupDecoderHost());
    fmx::RdsGroupDecoderHost &D = h->rd.dec[(size_t)channel];
    bool do_reset = false;
    {
        std::lock_guard<std::mutex> lk(h->mtx);
        if (h->rd.reset_dec[(size_t)channel]) { h->rd.reset_dec[(size_t)channel] = 0; do_reset = true; }
    }
    if (h->rds_alloc) {
        RdsState st;
        FMXCHK(fetch_rds_state(h, channel, &st));
        int32_t &rd = h->rd.dec_bits[(size_t)channel];
        if (st.nbits < rd) { rd = 0; D.reset_all(); }      // (the count went backwards: start over)
        if (do_reset) {
            // rdsGroupDecoder::reset: PI / PTY / labels back to unknown.  The reference resets between two blocks of samples;
            // here the decoder runs behind the slicer, so the bits still pending belong to the time before the reset (the
            // old station after a retune) and are dropped.
            D.reset_groups(); rd = st.nbits;
        }
        const RingTake t = ring_take(st.nbits, rd, RDS_BITS_CAP, RDS_BITS_CAP);      // (ring overrun: oldest bits lost)
        FMXCHK(read_ring(h->R.bits + (size_t)channel * RDS_BITS_CAP, RDS_BITS_CAP, t, [&](int64_t, uint8_t b) { D.push_bit(b != 0); }));
        rd = (int32_t)t.next();
    }
    else if (do_reset) D.reset_groups();
    *info = D.info();
    return FMX_OK;
}

int fmx_rds_decode_all(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_rds_info *infos) {
    if (!h || first_channel < 0 || n_channels < 0 || (int64_t)first_channel + n_channels > h->channels || (n_channels > 0 && !infos)) return fail(FMX_E_INVALID, "bad argument");
    if (n_channels == 0) return FMX_OK;
    const size_t C = (size_t)h->channels;
    if (h->rd.dec_all.size() != C) h->rd.dec_all.assign(C, fmx::RdsGroupDecoderHost());
    std::vector<uint8_t> do_reset((size_t)n_channels, 0);
    {
        std::lock_guard<std::mutex> lk(h->mtx);
        for (int k = 0; k < n_channels; k++) { do_reset[(size_t)k] = h->rd.reset_dec_all[(size_t)(first_channel + k)]; h->rd.reset_dec_all[(size_t)(first_channel + k)] = 0; }
    }
    const RdsSyncChan *st = nullptr; const RdsGroupRec *grp = nullptr;
    if (h->rds_alloc) FMXCHK(rds_batch_fetch(h, first_channel, n_channels, &st, &grp));
    for (int k = 0; k < n_channels; k++) {
        const size_t c = (size_t)(first_channel + k);
        fmx::RdsGroupDecoderHost &D = h->rd.dec_all[c];
        if (!h->rds_alloc) { if (do_reset[(size_t)k]) D.reset_groups(); infos[k] = D.info(); continue; }
        const RdsSyncChan &S = st[k];
        int64_t &rd = h->rd.dec_groups[c];
        // rdsGroupDecoder::reset: PI / PTY / labels back to unknown; the groups completed before this read-out belong to the time before the reset
        // and are dropped.  The synchroniser runs on (fmx.h: where this differs from fmx_rds_decode)
        if (do_reset[(size_t)k]) { D.reset_groups(); rd = S.groups; }
        const RingTake t = ring_take(S.groups, rd, RDS_GROUP_RING, RDS_GROUP_RING);      // (a reader that fell behind: the oldest groups are lost)
        for (int64_t i = 0; i < t.count; i++) {
            int64_t end_bit; uint16_t b[4];
            if (rds_group_read(S, grp + (size_t)k * RDS_GROUP_RING, t.from + i, &end_bit, b)) D.push_group(b);
        }
        rd = t.next();
        D.set_sync_status(fmx::RdsSyncStatus{S.s.synced, S.s.n_crc_err, S.s.n_sync_err, S.s.ber_num, S.s.ber_den});
        infos[k] = D.info();
    }
    return FMX_OK;
}

int fmx_rds_groups(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_rds_group *out, int32_t capacity_per_channel, int32_t *n_groups) {
    if (!h || first_channel < 0 || n_channels < 0 || (int64_t)first_channel + n_channels > h->channels || capacity_per_channel < 0 ||
        (n_channels > 0 && (!n_groups || (capacity_per_channel > 0 && !out)))) return fail(FMX_E_INVALID, "bad argument");
    for (int k = 0; k < n_channels; k++) n_groups[k] = 0;
    if (n_channels == 0 || !h->rds_alloc) return FMX_OK;
    const RdsSyncChan *st = nullptr; const RdsGroupRec *grp = nullptr;
    FMXCHK(rds_batch_fetch(h, first_channel, n_channels, &st, &grp));
    for (int k = 0; k < n_channels; k++) {
        int64_t &rd = h->rd.groups[(size_t)(first_channel + k)];
        const RingTake t = ring_take(st[k].groups, rd, RDS_GROUP_RING, capacity_per_channel);   // (a reader that fell behind: the gap shows in `index`)
        int32_t m = 0;
        for (int64_t i = 0; i < t.count; i++) {
            fmx_rds_group &r = out[(size_t)k * (size_t)capacity_per_channel + (size_t)m];
            if (!rds_group_read(st[k], grp + (size_t)k * RDS_GROUP_RING, t.from + i, &r.end_bit, r.block)) continue;
            r.index = t.from + i; m++;
        }
        rd = t.next();
        n_groups[k] = m;
    }
    return FMX_OK;
}

// host-only entry (no device needed): run a fresh block synchroniser / group decoder over a bit array
int fmx_rds_decode_bits(const uint8_t *bits, int32_t n_bits, fmx_rds_info *info) {
    if ((!bits && n_bits > 0) || n_bits < 0 || !info) return fail(FMX_E_INVALID, "bad argument");
    fmx::RdsGroupDecoderHost D;
    for (int32_t i = 0; i < n_bits; i++) D.push_bit(bits[i] != 0);
    *info = D.info();
    return FMX_OK;
}

const char *fmx_rds_pty_name(int32_t pty_code, int32_t pty_locale) { return fmx::rds_pty_name(pty_code, pty_locale); }
uint16_t fmx_rds_map_char(uint8_t alfabet, uint8_t character) { return fmx::rds_map_char(alfabet, character); }
int32_t fmx_rds_prepare_text(const uint8_t *v, int32_t length, uint8_t *alfabet, uint16_t *out, int32_t capacity) {
    if (!v || !out || length < 0 || capacity < 0) { (void)fail(FMX_E_INVALID, "bad argument"); return -1; }
    return fmx::rds_prepare_text(v, length, alfabet, out, capacity);
}

int fmx_get_taps(fmx_handle h, int32_t channel, int32_t which, float *dst, int32_t capacity, int32_t *n) {
    if (!h || !dst || !n || channel < 0 || channel >= h->channels) return fail(FMX_E_INVALID, "bad argument");
    {   // the tap sets of the CURRENT settings; nothing is uploaded and no pending action is touched (introspection)
        std::lock_guard<std::mutex> lk(h->mtx);
        if (h->sets_dirty) { HIPCHK(hipSetDevice(h->cfg.device)); int rc = ensure_sets(h); if (rc) return rc; h->params_dirty = true; }
    }
    const float *src = nullptr; int cnt = 0;
    std::vector<float> tmp;
    switch (which) {
    case 0: {   // front-end taps back in FIR order G[k], k = 12 d + off - r
        const FrontSet &fs = h->h_front_sets[h->params[channel].front_set];
        const float *t = &h->h_front_taps[(size_t)h->params[channel].front_set * A_TAPS_STRIDE];
        int NT = 0;
        tmp.assign(A_TAPS_STRIDE, 0.f);
        for (int d = 0; d < fs.nd; d++) for (int r = 0; r < DECIM; r++) {
            int k = 12 * d + fs.off - r;
            if (k >= 0 && k < A_TAPS_STRIDE) { tmp[k] = t[(d + 1) * DECIM + r]; if (t[(d + 1) * DECIM + r] != 0.f) NT = std::max(NT, k + 1); }
        }
        src = tmp.data(); cnt = NT; break; }
    case 1: src = h->h_pss_taps.data(); cnt = PSS_TAPS; break;
    case 2: {
        const AudioSet &as = h->h_audio_sets[h->params[channel].audio_set];
        const float *t = &h->h_audio_taps[(size_t)h->params[channel].audio_set * C_TAPS_STRIDE];
        tmp.resize(as.ntaps);
        for (int k = 0; k < as.ntaps; k++) tmp[k] = t[as.ntaps - 1 - k];
        src = tmp.data(); cnt = as.ntaps; break; }
    case 3: src = h->h_rs_taps.data(); cnt = RS_TAPS; break;
    case 4: {   // noise-squelch filters as the kernel holds them: [2][10][A1 A2 B1 B2], then the two gains (high-pass first)
        const design::Iir hp = design::iir_chebyshev_lowhigh(true, 20, 70000 - 100, h->cfg.fmRate);
        const design::Iir lp = design::iir_chebyshev_lowhigh(false, 20, 70000, h->cfg.fmRate);
        tmp.assign(2 * NSQ_QUADS * 4 + 2, 0.f);
        for (int f = 0; f < 2; f++) {
            const design::Iir &F = f ? lp : hp;
            for (int i = 0; i < NSQ_QUADS; i++) { tmp[(f * NSQ_QUADS + i) * 4] = F.q[i][1]; tmp[(f * NSQ_QUADS + i) * 4 + 1] = F.q[i][2]; tmp[(f * NSQ_QUADS + i) * 4 + 2] = F.q[i][4]; tmp[(f * NSQ_QUADS + i) * 4 + 3] = F.q[i][5]; }
            tmp[2 * NSQ_QUADS * 4 + f] = F.gain;
        }
        src = tmp.data(); cnt = (int)tmp.size(); break; }
    case 5: {   // RDS_1 constants as the kernels hold them: rdsFilter taps [21], Match kernel [43], sharpFilter [8][A1 A2 B1 B2], gain
        tmp = design::lowpass(RDS1_FIR, 2 * 2400, 24000);
        const std::vector<float> mk = design::rds1_match_kernel(24000);
        tmp.insert(tmp.end(), mk.begin(), mk.end());
        const design::Iir bp = design::iir_butterworth_bandpass(7, (int32_t)(1187.5 - 6), (int32_t)(1187.5 + 6), 24000);
        for (int i = 0; i < bp.nq; i++) { tmp.push_back(bp.q[i][1]); tmp.push_back(bp.q[i][2]); tmp.push_back(bp.q[i][4]); tmp.push_back(bp.q[i][5]); }
        tmp.push_back(bp.gain);
        src = tmp.data(); cnt = (int)tmp.size(); break; }
    default: return fail(FMX_E_INVALID, "unknown tap-set id");
    }
    if (cnt > capacity) return fail(FMX_E_TOO_LARGE, "capacity too small");
    std::memcpy(dst, src, sizeof(float) * cnt);
    *n = cnt;
    return FMX_OK;
}

}  // extern "C"

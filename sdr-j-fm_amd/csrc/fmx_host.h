// fmx_host.h -- what the host files of libfmx share (private to csrc): the last error and the checking macros, the owner of device memory, the handle
// behind include/fmx.h's fmx_handle, and the few helpers that cross a file.  fmx_api.hip holds the handle's life and its call path, fmx_readout.hip every
// entry point that only reads a handle, fmx_wide_api.hip stage W's host half, fmx_diag.hip the diagnostics.  Whatever crosses a file lives in
// fmx::host, with hidden visibility: the library's dynamic symbols under the fmx_ prefix are the two public headers' functions and nothing else.
#pragma once
#include "../../include/fmx.h"
#include "../../include/fmx_debug.h"
#include "fmx_internal.h"
#include "fmx_scan.h"
#include "fmx_meter.h"
#include "fmx_loud.h"
#include "fmx_rx.h"
#include "fmx_rdsm.h"
#include "fmx_rdsgroups.h"
#include "fmx_spec.h"
#include "fmx_mpx.h"
#include "fmx_sca.h"
#include "fmx_feed.h"
#include "fmx_taps.h"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

namespace fmx {
namespace host __attribute__((visibility("hidden"))) {

extern thread_local std::string g_err;      // what fmx_last_error returns (defined in fmx_api.hip)
inline int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(FMX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

#define FMXCHK(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// The owner of a handle's device and pinned memory: every buffer is its own hipMalloc / hipHostMalloc, recorded the moment it exists, and given back
// by release (one buffer, now) or release_all (fmx_destroy).  The only place of this library that allocates or frees GPU memory for a handle.
struct DevMem {
    std::vector<void *> dev, pinned;
    template <class T> int alloc(T *&p, size_t n, bool zero = false) {
        void *q = nullptr;
        HIPCHK(hipMalloc(&q, sizeof(T) * n));
        dev.push_back(q); p = static_cast<T *>(q);
        if (zero) HIPCHK(hipMemset(q, 0, sizeof(T) * n));
        return FMX_OK;
    }
    template <class T> int upload(T *&p, const std::vector<typename std::remove_const<T>::type> &src) {
        FMXCHK(alloc(p, src.size()));
        HIPCHK(hipMemcpy(dev.back(), src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
        return FMX_OK;
    }
    template <class T> int alloc_pinned(T *&p, size_t n) {
        void *q = nullptr;
        HIPCHK(hipHostMalloc(&q, sizeof(T) * n, hipHostMallocDefault));
        pinned.push_back(q); p = static_cast<T *>(q);
        return FMX_OK;
    }
    template <class T> void release(T *&p) {          // (device or pinned; a null or unknown pointer is only nulled)
        void *q = const_cast<void *>(static_cast<const void *>(p));
        auto it = std::find(dev.begin(), dev.end(), q);
        if (it != dev.end()) { dev.erase(it); (void)hipFree(q); }
        else if ((it = std::find(pinned.begin(), pinned.end(), q)) != pinned.end()) { pinned.erase(it); (void)hipHostFree(q); }
        p = nullptr;
    }
    void release_all() {
        for (void *q : dev) (void)hipFree(q);
        for (void *q : pinned) (void)hipHostFree(q);
        dev.clear(); pinned.clear();
    }
};

// A slotted array of a slot tap (fmx_taps.h) grows: `new_slots` x `per_slot` zeroed elements, the `old_slots` in use copied, the old array released (hipFree
// waits for the copy), the new pointer stored.  The caller synchronises the device in front of a growth's first array and behind its last copy.
template <class T> int grow_slots(DevMem &mem, T *&p, size_t old_slots, size_t new_slots, size_t per_slot) {
    T *q = nullptr;
    FMXCHK(mem.alloc(q, new_slots * per_slot, true));
    if (old_slots > 0) HIPCHK(hipMemcpy(q, p, sizeof(T) * old_slots * per_slot, hipMemcpyDeviceToDevice));
    mem.release(p);
    p = q;
    return FMX_OK;
}

// The staging of a gather read-out (fmx_mpx_spectrum_read, fmx_sca_read; under mtx): which ring items to gather, where the device gathers them, and the
// pinned copy of that.  `src` is the host's list: a member, so that an asynchronous upload never reads a vector that has gone.
struct GatherStage {
    int32_t *d_src = nullptr; float *d_stage = nullptr, *h_stage = nullptr; int64_t cap = 0; std::vector<int32_t> src;
    int ensure(DevMem &mem, int64_t batch, size_t floats_per_item) {
        if (batch <= cap) return FMX_OK;
        mem.release(d_src); mem.release(d_stage); mem.release(h_stage); cap = 0;
        FMXCHK(mem.alloc(d_src, (size_t)batch));
        FMXCHK(mem.alloc(d_stage, (size_t)batch * floats_per_item));
        FMXCHK(mem.alloc_pinned(h_stage, (size_t)batch * floats_per_item));
        cap = batch;
        return FMX_OK;
    }
};

inline int bytes_per_sample(int32_t fmt) { return fmt == FMX_IQ_F32 ? 8 : (fmt == FMX_IQ_S16 ? 4 : 2); }

// per-channel user-level settings (what the fmProcessor setters store)
struct ChanUser {
    int32_t bandwidth = 0;       // 0 = Off.  NB ctor default: inputFilterOn=false (fm-processor.cpp:149)
    int32_t lf_cutoff = 0;       // <=0 = off. ctor default fmAudioFilterActive=false (:164)
    int32_t bw_applied = 0, lf_applied = 0;    // what a FOLDED handle's tap sets are built from: the setter's value -- except while a mid-stream change of a batch
                                 // is pending (fmx_handle_s::promo_pending): then the values in force when the setter arrived
    bool bw_event = false, lf_event = false;   // setBandwidth / setlfcutoff CALLED with a value since the last call: the reference sets newInputFilter /
                                 // newAudioFilter whatever the value (:232-239, :762-770), and its loop restarts the filter's block (:396-408)
    int32_t deemph_us = 0;       // 0 = ctor default alpha (:174)
    bool    ctor_volume = true;  // volumeFactor = 0.5f (:127) until setVolume
    float   volume_db = 0.f;
    int32_t balance = 0, panorama = 100;
    int32_t squelch_value = 0, squelch_old = 0, squelch_level = 1;   // fm-processor.cpp:194-195; mySquelch (1, ...) :87
    // peak meter, host half: DelayLine<DSPCOMPLEX> (fm-processor.h:54-75) over the dB pairs, windows already fetched
    std::vector<float2> delay = std::vector<float2>(1, make_float2(-40.0f, -40.0f));
    uint32_t delay_idx = 0;
    // scan mode (FMX_P_SCANNING, FMX_P_SCAN_THRESHOLD): startScanning / stopScanning, the constructor's thresHold (fm-processor.cpp:63,108,361-367)
    bool    scanning = false;
    int16_t scan_thr = 20;
};

struct ProfRec { hipEvent_t e[4]; int64_t in_samples, ch_samples; int n; };

// Where the read-outs of the audio chain, the RDS path and scan mode stand, per channel: the number of the next item its ring's producer counts (ring_take,
// fmx_needs.h), the reset requests of the two RDS decoder paths, and their group decoders.  The cursors and flags are sized by fmx_create (init); the
// decoders are large and built by the first read-out that decodes.  ensure_rds_body starts `bits` over, ensure_scan `scan`.  The eight taps keep their
// readers' cursors themselves (RecordTap::cursor, SlotTap::cursor: fmx_taps.h).
// The count of a ring runs backwards only if its producer starts over, which no producer does today (fmx_rdssync.h).  Two readers of RdsState::nbits
// provide for it all the same and start over themselves: fmx_rds_symbols (`symbols`) and fmx_rds_decode (`dec_bits`, with the decoder).  fmx_rds_bits
// (`bits`) does not: it hands out nothing until the count has passed its cursor again.  The difference is kept as it was found.
struct Readers {
    std::vector<int32_t> peaks;              // fmx_get_peaks: windows of ChanState::pk_events
    std::vector<int32_t> bits;               // fmx_rds_bits: bits of RdsState::nbits
    std::vector<int32_t> dec_bits;           // fmx_rds_decode: the same count
    std::vector<int32_t> symbols;            // fmx_rds_symbols: the same count
    std::vector<int64_t> dec_groups;         // fmx_rds_decode_all: groups of RdsSyncChan::groups
    std::vector<int64_t> groups;             // fmx_rds_groups: the same count
    std::vector<int64_t> scan;               // fmx_scan_results: blocks of fmx_handle_s::scan_blocks
    std::vector<uint8_t> reset_dec, reset_dec_all;   // resetRds / triggerFrequencyChange asked for the group decoder's reset: fmx_rds_decode's, fmx_rds_decode_all's (under mtx)
    std::vector<RdsGroupDecoderHost> dec, dec_all;   // fmx_rds_decode's decoders (the synchroniser on the host), fmx_rds_decode_all's (on the GPU: rds_sync)
    void init(size_t channels) {
        peaks.assign(channels, 0); bits.assign(channels, 0); dec_bits.assign(channels, 0); symbols.assign(channels, 0);
        dec_groups.assign(channels, 0); groups.assign(channels, 0); scan.assign(channels, 0);
        reset_dec.assign(channels, 0); reset_dec_all.assign(channels, 0);
    }
};

}  // namespace host
}  // namespace fmx

// (the host files are written inside these two namespaces; nothing else includes this header)
using namespace fmx;
using namespace fmx::host;

struct fmx_handle_s {
    fmx_config cfg{};
    int channels = 0, streams = 0;
    bool streams_private = false;                                    // no two channels listen to the same stream
    hipStream_t stream = nullptr;
    int n_cus = 256; size_t lds_per_block = 65536;     // device limits the stage-A layout choice looks at
    std::vector<int32_t> act_up;                                     // one-shot action bits uploaded with the last parameter upload
    hipEvent_t ev_in = nullptr;
    std::mutex mtx;                          // guards the mailbox (set_param from any thread)
    std::vector<ChanUser> user;
    std::vector<ChanParams> params;          // host mirror
    bool params_dirty = true, sets_dirty = true;
    bool gain_dirty = true;                                          // volume / balance set since the last call (and before the first); under mtx
    bool gain_pending = false;                                       // ... taken over by flush_mailbox together with the settings themselves (processing
                                                                     // thread only): gain_fix_kernel runs in the first call that produces frames
    DevMem mem;                              // every device / pinned buffer of the handle (the RDS path's: rds_mem)
    Readers rd;                              // the read-outs' cursors (fmx_readout.hip)
    // unique tap sets
    std::vector<int32_t> front_keys, audio_keys;
    int front_cap = 0, audio_cap = 0;
    std::vector<float> h_front_taps, h_audio_taps, h_pss_taps, h_rs_taps, h_nsq, h_rds1;
    std::vector<FrontSet> h_front_sets; std::vector<AudioSet> h_audio_sets;
    // device: what the host writes again after the allocation (the kernels' views T.front_taps, T.front_sets, T.audio_taps, T.audio_sets, B.params are const)
    float *d_front_taps = nullptr, *d_audio_taps = nullptr;
    FrontSet *d_front_sets = nullptr; AudioSet *d_audio_sets = nullptr;
    ChanParams *d_params = nullptr;
    DeviceTables T{}; DeviceBuffers B{};
    int ring = 0, dring = 0, sring = 0;
    int decim = DECIM, twins = 1;            // the reference's total decimation for cfg.inputRate (12, 6 or 1) and 12 / decim (CallGeom::twins)
    int64_t g_total = 0;                     // input samples consumed per stream
    int64_t work_nj = 0;                     // rows of the sample-major work arrays
    int pitch = 0;                           // their row pitch in elements
    // staging for the host-pointer entry point
    float2 *d_iq = nullptr, *d_pcm = nullptr;
    // second converter (audioRate != workingRate, fm-processor.cpp:89-91,825-838)
    int cv_p = 1, cv_q = 1, cv_nt = 0; float *d_cv_taps = nullptr; float2 *d_x48 = nullptr; int64_t x48_stride = 0;
    // profiling
    bool prof_on = false; std::vector<ProfRec> prof; fmx_profile prof_acc{};
    int64_t last_J0 = 0, last_J1 = 0;
    // RDS path (allocated when a channel first switches RDS on)
    bool rds_alloc = false; RdsBuffers R{}; DevMem rds_mem;     // (an owner of its own: a partial failure gives the whole path back, ensure_rds)
    // per channel: the fm samples its RDS path has processed (it stands still while the channel's decoder is off, as the reference's
    // processor leaves its block filters, phase delay line and decimator alone then: fm-processor.cpp:733-754, :551-553), what RdsBuffers::nc0
    // was in the last call, and the device copy of the latter
    std::vector<int64_t> rds_nc, rds_nc0;
    int64_t *d_rds_nc0 = nullptr;
    // the batch read-outs (fmx_rds_decode_all, fmx_rds_groups): the synchroniser runs on the GPU (rds_sync); an event behind the handle's last call, a
    // stream and a pinned buffer for the two copies of a read-out
    hipEvent_t ev_call = nullptr; bool ev_call_set = false; hipStream_t rd_stream = nullptr;
    char *rds_stage = nullptr;
    std::vector<int64_t> last_m0, last_m1;  // per channel: its 24 kS/s outputs of the last call
    // what a call needs of `params` beyond the device copy, taken under `mtx` by flush_mailbox: fmx_set_param may write `params` from another thread
    // while the processing thread enqueues the call
    std::vector<int8_t> call_rds_mode;
    CallNeeds needs{};                       // the summary of the settings the call's kernels and buffers are chosen from (fmx_needs.h)
    // scan mode (fmx_scan.hip): the call's scanning channels and their thresholds (flush_mailbox); per channel the block being collected (fill), the blocks
    // completed since fmx_create, and per record slot the fm sample behind the block and the threshold of the call that completed it
    // (the device keeps (signal_db, noise_db) per slot); allocated by the first call in which a channel scans
    std::vector<int32_t> call_scan; std::vector<int16_t> call_scan_thr;
    bool scan_alloc = false;
    float2 *d_scan_W = nullptr, *d_scan_carry = nullptr, *d_scan_rec = nullptr; ScanJob *d_scan_jobs = nullptr; int32_t *d_scan_mute = nullptr;
    std::vector<ScanJob> scan_jobs;
    std::vector<int32_t> scan_fill; std::vector<int64_t> scan_blocks, scan_end; std::vector<int16_t> scan_rec_thr;
    // The four record meters (RecordTap, fmx_taps.h: switches, on_from, produced and the reader's cursor, under mtx), each with its device side -- the
    // accumulators of the window in progress, the record ring, the jobs -- and the jobs of the piece being made.  The device side is allocated by the first
    // call in which a meter is on (ensure_record_tap): a handle that never switches a meter on has none of it.
    // the modulation meter (fmx_meter.hip, fmx_meter.h): on_from and windows in fm samples
    RecordTap mod_tap;
    float *d_meter_state = nullptr; fmx_mod_record *d_meter_ring = nullptr; MeterJob *d_meter_jobs = nullptr; std::vector<MeterJob> meter_jobs;
    // the programme audio meter (fmx_loud.hip, fmx_loud.h): in PCM frames; the device keeps each channel's 16 floats
    RecordTap audio_tap;
    float *d_loud_state = nullptr; fmx_audio_record *d_loud_ring = nullptr; LoudJob *d_loud_jobs = nullptr; std::vector<LoudJob> loud_jobs;
    // the reception meter (fmx_rx.hip, fmx_rx.h): in fm samples
    RecordTap rx_tap;
    float *d_rx_state = nullptr; fmx_rx_record *d_rx_ring = nullptr; RxJob *d_rx_jobs = nullptr; std::vector<RxJob> rx_jobs;
    // the RDS meter (fmx_rdsm.hip, fmx_rdsm.h): in RDS samples of the channel's own count, on_from that of the first piece that produced one (rdsm::piece);
    // allocated by the first call in which a meter is on and a decoder runs
    RecordTap rdsm_tap;
    float *d_rdsm_state = nullptr; fmx_rds_meter_record *d_rdsm_ring = nullptr; RdsmJob *d_rdsm_jobs = nullptr; std::vector<RdsmJob> rdsm_jobs;
    // The four slot taps (SlotTap, fmx_taps.h: the user's and the piece's values, slot, on_from, the reader's cursor, the ring tags, slots in use and
    // allocated, live; under mtx), each with its slotted device arrays, the jobs of the piece being made, the event behind the last piece's kernels -- what
    // its read-out waits for -- and whatever is its own.  The device arrays grow with the units switched on (grow_slots): a handle that never switches a
    // tap on has none of its memory.
    // the spectrum meter (fmx_spec.hip, fmx_spec.h), per STREAM, on_from in input samples: B and S in force and what fmx_spectrum_setup asked for (taken over
    // by flush_mailbox); per slot the carry, sum and maximum, and the ring of records
    SlotTap spec_tap;
    int32_t spec_B = 16, spec_S = 1, spec_B_user = 16, spec_S_user = 1; bool spec_setup_dirty = false;
    int64_t spec_scratch = 0;                                           // blocks of scratch allocated
    float spec_c = 0.f, spec_c1 = 0.f; int32_t spec_c_B = 0;            // 1 / (B sum w^2) for B = spec_c_B, 1 / sum w^2
    float2 *d_spec_carry = nullptr, *d_spec_W = nullptr; float *d_spec_acc = nullptr, *d_spec_ring = nullptr, *d_spec_power = nullptr, *d_spec_win = nullptr;
    SpecJob *d_spec_jobs = nullptr; std::vector<SpecJob> spec_jobs;
    hipEvent_t ev_spec = nullptr; bool ev_spec_set = false;
    // the multiplex spectrum meter (fmx_mpx.hip, fmx_mpx.h), per CHANNEL, on_from in fm samples: per slot the carry (16 KB), sum and maximum (16 KB) and the
    // ring (64 KB); the window and the twiddles are d_spec_win / d_spec_W, shared with the spectrum meter
    SlotTap mpx_tap;
    int32_t mpx_B = mpx::DEFAULT_B, mpx_S = 1, mpx_B_user = mpx::DEFAULT_B, mpx_S_user = 1; bool mpx_setup_dirty = false;
    int64_t mpx_scratch = 0;                                            // blocks of scratch allocated
    float mpx_c = 0.f, mpx_c1 = 0.f; int32_t mpx_c_B = 0;              // 1 / (B sum w^2) for B = mpx_c_B, 1 / sum w^2
    float *d_mpx_carry = nullptr, *d_mpx_acc = nullptr, *d_mpx_ring = nullptr, *d_mpx_power = nullptr;
    MpxJob *d_mpx_jobs = nullptr; std::vector<MpxJob> mpx_jobs;
    GatherStage mpx_stage;                                              // fmx_mpx_spectrum_read's
    hipEvent_t ev_mpx = nullptr; bool ev_mpx_set = false;
    // the sub-carrier decoder (fmx_sca.hip, fmx_sca.h), per CHANNEL, the value a centre frequency, on_from in fm samples: the centre each channel's slot's
    // taps were made for; per slot the ring's audio (120 KB) and levels, the carry (10.25 KB) and the mixed taps with the rotation (1544 bytes)
    SlotTap sca_tap;
    std::vector<int32_t> sca_slot_centre;
    fmx_sca_config sca_cfg = sca::default_config(), sca_cfg_user = sca::default_config(); bool sca_setup_dirty = false;
    bool sca_taps_stale = true;                                          // d_sca_a is not sca_cfg's (the setup changed, or nothing was uploaded yet)
    std::vector<float> sca_g;                                            // the band filter of sca_cfg (the mixed taps are made from it per centre)
    float *d_sca_a = nullptr, *d_sca_carry = nullptr, *d_sca_audio = nullptr, *d_sca_level = nullptr; float2 *d_sca_taps = nullptr;
    ScaJob *d_sca_jobs = nullptr; std::vector<ScaJob> sca_jobs;
    GatherStage sca_stage;                                               // fmx_sca_read's
    hipEvent_t ev_sca = nullptr; bool ev_sca_set = false;
    // the monitoring feed (fmx_feed.hip, fmx_feed.h), per CHANNEL, the value a mode, on_from in PCM frames: the mode each channel runs in; per slot the ring's
    // audio (80 KB) and powers and the carry (2496 bytes); the taps are one array per handle
    SlotTap feed_tap;
    std::vector<int32_t> feed_mode;
    float *d_feed_h = nullptr, *d_feed_carry = nullptr, *d_feed_audio = nullptr, *d_feed_power = nullptr;
    FeedJob *d_feed_jobs = nullptr; std::vector<FeedJob> feed_jobs;
    // the read-outs' staging (under mtx): which ring blocks to gather and where to, where the host read-out gathers them, and the pinned copy of that
    int32_t *d_feed_src = nullptr; int64_t feed_src_cap = 0; std::vector<int32_t> feed_src, feed_dst;
    float *d_feed_stage = nullptr, *h_feed_stage = nullptr; int64_t feed_stage_blocks = 0;
    hipEvent_t ev_feed = nullptr; bool ev_feed_set = false;
    hipEvent_t ev_feed_rd = nullptr; bool ev_feed_rd_set = false;        // behind the last fmx_feed_read_device's gather: what the next use of d_feed_src, and the next piece's kernels, wait for
    std::atomic<int> stageb_form{0};     // FMX_P_STAGEB_FORM
    std::atomic<int> front_parts{0};     // FMX_P_FRONT_PARTS
    std::atomic<int> front_kernel{0};    // FMX_P_FRONT_KERNEL
    std::atomic<int> scope_taps{-1};     // FMX_P_SCOPE_TAPS
    bool taps_kept = true;               // the last call kept the scope-tap rows (fmx_get_tap)
    float *w_diff_mem = nullptr;         // the LR scope tap's rows (allocated when first wanted; DeviceBuffers::w_diff is null while the tap is off)
    std::vector<std::pair<int32_t, int32_t>> hlo_key;   // per channel: the (bandwidth, oscillator) its ChanParams::hlo_* were computed for
    int last_front_kernel = 1;           // what the last call's stage A was given (FMX_P_FRONT_KERNEL numbering): fmx_last_front_kernel
    // a batch call whose channels need the demodulator pre-pass (a lone wave per 64 channels walking the call sample by sample: 6 % of the chip for
    // most of the call's time) is made in pieces whose stages overlap: run_call
    hipStream_t pipe_sA = nullptr, pipe_sP = nullptr, pipe_sB = nullptr;   // stage A (and the parallel part of the pre-pass) of piece k + 1, the recurrences of piece k, stage B / C of piece k - 1
    hipEvent_t pipe_ev0 = nullptr, pipe_evA = nullptr, pipe_evD = nullptr, pipe_evP = nullptr, pipe_evE = nullptr, pipe_evB[2] = {nullptr, nullptr};
    std::atomic<int> pipe_rows{-1};      // FMX_P_CALL_PIECES: fm samples per piece (-1 automatic, 0 never)
    int last_pieces = 1;                 // overlapping pieces the last call was made in (fmx_last_call_pieces)
    int last_second_group = 0;           // channels of the second stage-B / C group of the last call (fmx_last_second_group)
    int my_count_host = 0;               // the reference's myCount (fm-processor.cpp:662-684) as stage B keeps it in every channel's state: the same in all of them
    PreLook pre_look{};                  // pre_kernel's look-back buffers (ensure_ola)
    char *hp_iq = nullptr; float2 *hp_pcm = nullptr;   // fmx_process_host: pinned, device-visible staging of small calls
    // the reference's two overlap-add filters as the block machines they are (fmx_ola.hip): handles of up to OLA_MAX_CH channels
    bool ola_mode = false;               // FMX_P_FILTER_RESTARTS resolved (fixed once the first call has been made)
    struct OlaSide {
        int L = 0, degree = 0;
        float2 *A = nullptr, *C = nullptr, *over = nullptr, *over_new = nullptr; float *taps = nullptr;
        std::vector<int32_t> inp, on, key;   // per channel: block position, Pass () in use, the setting the kernel was designed for (-1: none yet)
    } ola_in, ola_au;
    float2 *d_v = nullptr, *d_u = nullptr, *d2ring = nullptr;   // pre_kernel's output, the input filter's output ([channels][max_block]), the audio filter's output ring
    // A batch (folded filters) whose filters are changed in mid-stream: the setter stays pending while the library keeps the streams' samples (fmx_promote.hip),
    // then the handle switches to the block machines (promote).  FMX_P_FILTER_RESTARTS = 2 pins the folded filters (the change then applies at once, as
    // rounds 1-5 applied it: a different glitch of one filter latency).
    bool folded_pinned = false;          // FMX_P_FILTER_RESTARTS = 2 was asked for
    bool promoted = false;               // a block-machine handle by promotion: goes back to the folded filters once its machines have been quiet (demote)
    bool demo_capture = false;           // ... and is keeping its streams for that
    int64_t last_filter_event_g = 0;     // stream position at which a filter setter was last applied (ola_take_settings)
    std::vector<int64_t> origin_in, origin_au;   // per channel: the stream position (input samples / fm samples) at which the filter's block counter was last 0, as far as a
                                         // FOLDED handle knows it (0 from fmx_create; the machines' own counters at a demotion)
    bool promo_pending = false;          // a filter setter arrived behind the first call
    bool promo_recapture = false;        // ... and a setter of what pre_kernel applies (RF DC removal, balance, oscillator) behind it: the kept samples start over
    int64_t promo_have = 0, promo_g0 = 0;   // samples kept per stream, and the stream position of the first
    float2 *tail_iq = nullptr; int64_t tail_cap = 0; FrontSnap *tail_snap = nullptr;
    size_t old_sets_cap = 0;
    ChanParams *d_params_replay = nullptr; FrontSet *d_old_sets = nullptr; int32_t *d_old_set_of = nullptr; float2 *d_au_tail = nullptr;
    // the block machines' steps of a handle above OLA_MAX_CH channels: tables in device memory (the launchers take a step by value up to 64 channels),
    // a ring of STEP_SLOTS tables, each copied from pinned host memory on the call's stream in front of the kernels that read it
    static constexpr int STEP_SLOTS = 32;
    OlaChan *step_dev = nullptr, *step_host = nullptr; hipEvent_t step_ev[STEP_SLOTS] = {}; bool step_used[STEP_SLOTS] = {}; int step_next = 0;
};

namespace fmx {
namespace host __attribute__((visibility("hidden"))) {

int ensure_sets(fmx_handle h);           // fmx_api.hip: the tap sets of the settings in force, designed and uploaded when they changed (under mtx)
// frames the second converter has put out after `in` frames at the working rate: outputs m with m q < in p
inline int64_t conv2_out(const fmx_handle h, int64_t in) { return h->cv_nt ? (in * h->cv_p + h->cv_q - 1) / h->cv_q : in; }

}  // namespace host
}  // namespace fmx

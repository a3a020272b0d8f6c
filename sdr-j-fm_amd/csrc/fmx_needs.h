// fmx_needs.h -- what a handle's settings mean for its next call: which values a setter accepts and what it derives from them, the one summary of the
// channels' settings a call's kernels and buffers are chosen from (CallNeeds), stage A's kernel, the plain batch, and the cursors of the rings the
// read-outs hand out.  A metered channel (fmx_mod_meter_enable, fmx_mpx_spectrum_enable or fmx_sca_enable) sets rows_on as an RDS channel does: the rows w_dem / w_cur are handle-wide, so a batch with
// one metered channel writes 8 bytes per fm sample for EVERY channel and takes the non-plain call shape.  Plain C++ (no HIP, no handle, no allocation, no lock): fmx_api.hip decides with these functions, tests/needs_check.cpp checks
// them on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/fmx.h"
#include "fmx_plan.h"

namespace fmx {

constexpr int LO_LDS_MAX = 1024;       // LO phase periods up to this are tabulated in LDS by the input-FIR kernel
constexpr int OLA_MAX_CH = 64;         // FMX_P_FILTER_RESTARTS automatic: handles up to this many channels run the block machines (fmx_ola.hip)
constexpr int PLL_SEQ_AUTO_MAX = 64;   // FMX_P_PLL_SOLVER = 0: handles up to this many channels evaluate the pilot PLL sequentially

// ---- parameter checks: a refusal's code and text (FMX_OK, null: accepted)
struct ParamCheck { int code; const char *msg; };

// fmx_set_param's value check; what depends on the handle's history (FMX_P_FILTER_RESTARTS behind the first call) stays with the handle
inline ParamCheck check_param(int32_t id, double value, int32_t inputRate) {
    const int iv = (int)std::llround(value);
    const char *bad = nullptr;
    switch (id) {
    case FMX_P_FM_MODE: if (iv < 0 || iv > 2) bad = "fm mode must be 0..2"; break;
    case FMX_P_FM_DECODER: if (iv < 1 || iv > 6) bad = "decoder must be 1..6"; break;
    case FMX_P_SOUND_MODE: if (iv < 0 || iv > 6) bad = "sound mode must be 0..6"; break;
    case FMX_P_STEREO_PANORAMA: if (iv < 0 || iv > 200) bad = "panorama must be 0..200"; break;
    case FMX_P_SOUND_BALANCE: if (iv < -100 || iv > 100) bad = "balance must be -100..100"; break;
    case FMX_P_DEEMPHASIS: if (iv < 1) bad = "de-emphasis must be >= 1 us (Q_ASSERT fm-processor.cpp:293)"; break;
    case FMX_P_BANDWIDTH: if (iv < 0 || iv > inputRate) bad = "bandwidth out of range"; break;
    case FMX_P_RDS_MODE: if (iv < 0 || iv > 3) bad = "rds mode must be 0..3"; break;
    case FMX_P_LOCAL_OSCILLATOR: if (std::abs(iv) > inputRate) bad = "|lo| must be <= inputRate (oscillator.cpp:49-58)"; break;
    case FMX_P_SQUELCH_MODE: if (iv < 0 || iv > 2) bad = "squelch mode must be 0 (off), 1 (noise squelch) or 2 (level squelch)"; break;
    case FMX_P_SQUELCH_VALUE: if (iv < 0 || iv > 100) bad = "squelch value must be 0..100"; break;
    case FMX_P_PLL_SOLVER: if (iv < 0 || iv > 3) bad = "PLL solver must be 0 (automatic), 1 (sequential), 2 (Newton, sequential around lock decisions) or 3 (Newton always)"; break;
    case FMX_P_FRONT_KERNEL:
        if (iv < 0 || iv > 3 || iv == 2) bad = "front kernel must be 0 (automatic), 1 (four waves per channel, packed f32 FMAs) or 3 (the filter on the matrix pipe); 2 was round 5's six-wave kernel, now tools/experiments/fmx_front3.hip";
        break;
    case FMX_P_SCOPE_TAPS: if (iv < -1 || iv > 1) bad = "scope taps must be -1 (automatic), 0 (not kept) or 1 (kept)"; break;
    case FMX_P_CALL_PIECES: if (iv < -1 || iv > (1 << 20)) bad = "call pieces must be -1 (automatic), 0 (never) or the fm samples per piece"; break;
    case FMX_P_FRONT_PARTS: if (iv < 0 || iv > 32) bad = "front parts must be 0 (automatic), 1 (one workgroup per channel) or 2..32"; break;
    case FMX_P_STAGEB_FORM: if (iv < 0 || iv > 2) bad = "stage B form must be 0 (automatic), 1 (one kernel) or 2 (two kernels)"; break;
    case FMX_P_FILTER_RESTARTS: if (iv < 0 || iv > 2) bad = "filter restarts must be 0 (automatic), 1 (the reference's block filters) or 2 (folded FIRs)"; break;
    case FMX_P_SCANNING: if (!(value == 0.0 || value == 1.0)) bad = "scanning must be 0 or 1"; break;
    case FMX_P_SCAN_THRESHOLD:
        if (!(value >= -32768.0 && value <= 32767.0 && value == std::floor(value))) bad = "scan threshold must be an integral number of dB in -32768..32767 (the reference's int16_t thresHold)";
        break;
    case FMX_P_DISP_DELAY: if (iv < 0 || iv > 100000) bad = "display delay must be 0..100000 steps"; break;
    case FMX_P_TEST_TONE:
    case FMX_P_VOLUME_DB: case FMX_P_LF_CUTOFF: case FMX_P_ATTENUATION_L: case FMX_P_ATTENUATION_R:
    case FMX_P_AUTO_MONO: case FMX_P_PSS: case FMX_P_DC_REMOVE:
    case FMX_A_TRIGGER_FREQUENCY_CHANGE: case FMX_A_RESTART_PSS: case FMX_A_RESET_RDS: break;
    default: bad = "unknown parameter id";
    }
    return {bad ? FMX_E_INVALID : FMX_OK, bad};
}

// the sample format of an fmx_process_*_raw / fmx_wideband_process_*_raw call
inline ParamCheck check_iq_format(int32_t fmt, float s16_den) {
    if (fmt < 0 || fmt > 3) return {FMX_E_INVALID, "unknown IQ format"};
    int ex = 0;
    if (fmt == FMX_IQ_S16 && (!(s16_den >= 1.0f) || std::frexp(s16_den, &ex) != 0.5f)) return {FMX_E_INVALID, "s16_denominator must be a power of two >= 1"};
    return {FMX_OK, nullptr};
}

// ---- derived settings
// ChanParams::lo_period: inputRate / gcd (|lo|, inputRate) when the oscillator's phase sequence repeats within LO_LDS_MAX samples, else 0
inline int32_t lo_period(int32_t lo, int32_t inputRate) {
    int64_t a = lo < 0 ? -(int64_t)lo : lo, b = inputRate;
    while (b) { const int64_t r = a % b; a = b; b = r; }
    const int64_t per = a ? inputRate / a : 0;
    return (lo != 0 && per <= LO_LDS_MAX) ? (int32_t)per : 0;
}
// ChanParams::pll_seq of FMX_P_PLL_SOLVER's value
inline int32_t pll_seq(int value, int channels) { return (value == 1 || (value == 0 && channels <= PLL_SEQ_AUTO_MAX)) ? 1 : (value == 3 ? 2 : 0); }
// set_squelchValue's two thresholds (squelchClass.cpp:33-37): ChanParams::squelch_thr, ::squelch_nthr
struct SquelchThr { float level, noise; };
inline SquelchThr squelch_thresholds(int32_t squelch_level) {
    return {std::pow(10.0f, (float)(squelch_level - 80) / 30.0f), 1.0f - (float)squelch_level / 100.0f};
}
// FMX_P_FILTER_RESTARTS resolved: the block machines or the folded filters, and whether the folded ones were asked for by name
struct FilterForm { bool ola_mode, folded_pinned; };
inline FilterForm filter_form(int value, int channels) { return {value == 1 || (value == 0 && channels <= OLA_MAX_CH), value == 2}; }
// FMX_P_BANDWIDTH / FMX_P_LF_CUTOFF on a folded handle in mid-stream: the setter stays pending until the handle has kept enough of its streams to become a
// block-machine handle; everywhere else -- before the first call, a block-machine handle, folded filters pinned -- it applies with the next call
inline bool defer_filter_change(bool ola_mode, bool folded_pinned, int64_t g_total, int twins, int64_t max_block) {
    return !ola_mode && !folded_pinned && g_total > 0 && twins >= 1 && max_block >= 4096;
}
// The sum of a channel's complex taps, Hlo = sum_m G [m] e^(j 2 pi ((m lo) mod R) / R): what the matrix-pipe input filter makes of the RF DC value
// (fmx_front4.hip).  tz: the host tap image Tz [(d + 1) * DECIM + r] = G [12 d + off - r], d = 0 .. cols - 1; (the plain tap sum, 0) without an oscillator.
struct TapSum { float re, im; };
inline TapSum tap_sum_lo(const float *tz, int cols, int32_t off, int32_t lo, int32_t inputRate) {
    const int R = inputRate;
    double hr = 0, hi = 0;
    for (int d = 0; d < cols; d++)
        for (int r = 0; r < DECIM; r++) {
            const int m = 12 * d + off - r;
            if (m < 0) continue;
            const int64_t ph = (((int64_t)m * lo) % R + R) % R;
            const double g = (double)tz[(d + 1) * DECIM + r], a = 2.0 * 3.14159265358979323846 * (double)ph / (double)R;
            hr += g * std::cos(a); hi += g * std::sin(a);
        }
    return {(float)hr, (float)hi};
}

// ---- the summary of a handle's settings: one pass over the channels (needs_begin, then needs_add per channel)
struct ChanNeeds {                     // what the summary reads of one channel: of its ChanParams ...
    int32_t decoder, squelch_mode, rds_mode, lo_freq;
    float   att_l, att_r;
    int32_t nd, dc_k;                  // ... and of its FrontSet
    int32_t metered;                   // ... and whether its modulation meter, its multiplex spectrum meter or its sub-carrier decoder is on (fmx_mod_meter_enable, fmx_mpx_spectrum_enable, fmx_sca_enable)
};
struct CallNeeds {
    bool any_lo;                       // some channel has a local oscillator (the LO table; stage A's complex-tap variant)
    bool front4_ok;                    // every channel qualifies for front4_kernel
    bool any_rds;                      // some channel decodes RDS
    bool prepass, pllc, am;            // CallShape's: the demodulator pre-pass runs (PLL / AM decoder, a squelch); pllC does; the AM decoder does
    int  prepass_var;                  // DeviceBuffers::prepass_var
    bool any_nsq;                      // some channel runs the noise squelch (its filters' coefficients)
    bool keep_taps, rows_on, peaks_on; // FMX_P_SCOPE_TAPS resolved; DeviceBuffers::rows_on, ::peaks_on
    bool any_meter;                    // some channel's modulation meter, multiplex spectrum meter or sub-carrier decoder is on
};
inline CallNeeds needs_begin(int channels, int twins, bool ola_mode, int scope_taps) {
    CallNeeds n{};
    // stage A on the matrix pipe (fmx_front4.hip): no twins, no block machines, and of every channel what needs_add asks
    n.front4_ok = twins == 1 && !ola_mode;
    // the scope taps that are rows of stage B's work arrays: display feeds, kept where there is a display; the RDS path reads two of them
    n.keep_taps = scope_taps < 0 ? channels <= 64 : scope_taps != 0;
    n.rows_on = n.keep_taps; n.peaks_on = n.keep_taps;
    return n;
}
inline void needs_add(CallNeeds &n, const ChanNeeds &c) {
    n.any_lo |= c.lo_freq != 0;
    // front4_kernel: every tap set the long fold with its RfDC taken 12 columns back.  It applies the IQ balance in front of its filter together with the
    // tile's scale and takes the RF DC recurrence's column sums back through 1 / balance: a balance of 0 (the slider's end, radio.cpp:989-995) or one no
    // slider produces goes to front_kernel's per-sample pass
    const float al = std::fabs(c.att_l), ar = std::fabs(c.att_r);
    n.front4_ok = n.front4_ok && c.nd > 4 && c.dc_k == 12 && al >= 1e-6f && al <= 1e6f && ar >= 1e-6f && ar <= 1e6f;
    n.any_rds |= c.rds_mode != 0;
    if (c.rds_mode != 0) n.rows_on = true;
    // the modulation meter reads the same two rows behind stage B (fmx_meter.hip), the multiplex spectrum meter the first of them (fmx_mpx.hip).  The rows are handle-wide: a batch with ONE metered channel writes them --
    // 8 bytes per fm sample -- for every channel, and is no plain batch any more (plain_batch below: one channel group, the rows' kernel choice)
    n.any_meter |= c.metered != 0;
    if (c.metered != 0) n.rows_on = true;
    // pllC on the fm-rate IQ; |z| for the level squelch; the general AFC body for the noise squelch
    n.pllc |= c.decoder == 2 || c.decoder == 1;
    n.am |= c.decoder == 1;
    n.prepass |= c.decoder == 2 || c.decoder == 1 || c.squelch_mode != 0;
    // (of the channels the pre-pass touches: fmx_demod.hip, afc_kernel's variants)
    n.prepass_var |= (c.decoder == 2 ? 1 : 0) | (c.decoder == 1 ? 2 : 0) | (c.squelch_mode == 2 ? 4 : 0) | ((c.decoder > 2 && c.squelch_mode != 0) ? 8 : 0);
    n.any_nsq |= c.squelch_mode == 1;
}

// ---- stage A's kernel: CallGeom::front4 (0 front_kernel, 1 front4_kernel, 2 its complex-tap variant) and the parts that remain of plan_front_parts'.
// fk: FMX_P_FRONT_KERNEL.  Automatic: the filter on the matrix pipe wherever a handle qualifies and has the channels to fill the chip without splitting
// them in time (measured at 4096 channels on one box: 1.52 ms per launch against 1.75 for the four-wave kernel and 1.84 for the six-wave VALU kernel,
// which both sit at the packed-FMA power limit); the complex-tap variant runs one channel per workgroup: a handle of one channel per
// compute unit fills the chip
struct FrontChoice { int front4, parts; };
inline FrontChoice choose_front(bool front4_ok, bool any_lo, int fk, int parts, int channels, int n_cus) {
    if (front4_ok && !any_lo && (fk == 3 || (fk == 0 && parts <= 1))) return {1, 1};
    if (front4_ok && any_lo && (fk == 3 || (fk == 0 && channels >= n_cus))) return {2, 1};
    return {0, parts};
}

// ---- a plain batch (no pre-pass, no RDS, no scope-tap rows: stage B as the whole kernel) may run stages B and C as two channel groups (second_group_channels)
struct PieceFlags {
    bool piped, ola_mode, prepass_arrays, conv2, rows_on, rds_running, gain_pending;   // rds_running: the RDS path is allocated and some channel decodes
    int  stageb_form;
    bool has_fm, has_frames;           // the piece covers an fm sample / produces a PCM frame
};
inline bool plain_batch(const PieceFlags &f) {
    return !f.piped && !f.ola_mode && !f.prepass_arrays && !f.conv2 && !f.rows_on && !f.rds_running && !f.gain_pending && f.stageb_form == 0 && f.has_fm && f.has_frames;
}

// ---- ring cursors.  A producer has made `produced` items so far into a ring of `ring` slots (a power of two; item i in slot i & (ring - 1)), the consumer
// has read `read` of them and takes at most `capacity`: items [from, from + count) are handed out and the read position becomes next ().  A consumer that
// fell behind by more than the ring has lost the oldest items: `from` is then past them.
struct RingTake {
    int64_t from, count;
    int64_t next() const { return from + count; }
};
inline RingTake ring_take(int64_t produced, int64_t read, int64_t ring, int64_t capacity) {
    if (produced - read > ring) read = produced - ring;
    int64_t count = produced - read < capacity ? produced - read : capacity;
    if (count < 0) count = 0;
    return {read, count};
}
inline int64_t ring_slot(int64_t pos, int64_t ring) { return pos & (ring - 1); }

// scan mode's producer: a channel whose carry holds `fill` samples and that has completed `blocks` blocks takes the call's nj fm samples from J0 on.
// The kernel's job, the blocks of the call that leave a record -- the last `ring` of them: b in [b0, nblk), at slot (b), ending behind fm sample
// end_sample (b) - 1 -- and the counters behind the call.
struct ScanProduce {
    int32_t job_fill, job_slot0;       // ScanJob::fill, ::slot0
    int64_t b0, nblk;
    int64_t blocks, new_blocks, J0;
    int32_t new_fill, block, ring;
    int64_t slot(int64_t b) const { return (blocks + b) & (ring - 1); }
    int64_t end_sample(int64_t b) const { return J0 + (b + 1) * block - job_fill; }      // (a complete block ends in this call: the carry holds < block)
};
inline ScanProduce scan_produce(int64_t fill, int64_t blocks, int64_t nj, int64_t J0, int block, int ring) {
    ScanProduce p{};
    p.nblk = (fill + nj) / block;
    p.b0 = p.nblk > ring ? p.nblk - ring : 0;
    p.job_fill = (int32_t)fill; p.job_slot0 = (int32_t)(blocks & (ring - 1));
    p.blocks = blocks; p.new_blocks = blocks + p.nblk; p.J0 = J0;
    p.new_fill = (int32_t)((fill + nj) % block); p.block = block; p.ring = ring;
    return p;
}

}  // namespace fmx

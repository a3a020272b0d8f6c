// fm_processor_adapter.h -- host-side C++ mirror of the reference's fmProcessor for the FM hot path.
//
// The reference wires  deviceHandler -> fmProcessor -> audioSink  (SURVEY 1); `fmProcessor` is a
// QThread whose run() loop (src/fm/fm-processor.cpp:373-687) pulls 16384-sample blocks and pushes
// PCM frames.  This header provides the same class shape WITHOUT Qt on top of the C ABI of
// include/fmx.h, so that the GUI's call sites (radio.cpp:915-948, the handle_* slots) compile
// against it unchanged in spirit: same method names, same argument meaning, same error behaviour
// (setters never throw; unsupported settings are reported through lastError()).
//
// A Qt build derives this class from QThread and emits the signals from the values returned by
// poll_meta(); see INTEGRATION.md.  Header-only; links against libfmx.so only.
#pragma once
#include <atomic>
#include <algorithm>
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/fmx.h"

namespace fmx_host {

// devices/device-handler.h:60-85 -- the two calls the processing loop uses
struct DeviceHandler {
    virtual ~DeviceHandler() {}
    virtual int32_t Samples() = 0;                                        // complex samples available
    virtual int32_t getSamples(std::complex<float> *dst, int32_t n) = 0;  // copies n interleaved (I,Q) pairs
    virtual int32_t getRate() { return 2304000; }
};
// includes/output/audiosink.h:36-76 -- real = left, imag = right, float32 at audioRate
struct AudioSink {
    virtual ~AudioSink() {}
    virtual int32_t putSamples(std::complex<float> *frames, int32_t n) = 0;
};

class FmProcessor {
public:
    enum class FM_Mode { Stereo, StereoPano, Mono };                       // fm-processor.h:83
    enum Channels { S_STEREO, S_STEREO_SWAPPED, S_LEFT, S_RIGHT, S_LEFTplusRIGHT, S_LEFTminusRIGHT,
                    S_LEFTminusRIGHT_Test };                               // fm-processor.h:88-90
    struct SMetaData {                                                     // fm-processor.h:91-101
        enum class EPssState { OFF, ANALYZING, ESTABLISHED };
        float DcValRf, DcValIf, PssPhaseShiftDegree, PssPhaseChange;
        EPssState PssState;
        float PilotPllLockStrength;
        bool PilotPllLocked;
    };

    // fm-processor.cpp:48-63 (the scope ring buffers, RadioInterface* and fm_Demodulator* of the
    // reference constructor stay on the GUI side; the decoder is selected with setFMdecoder)
    FmProcessor(DeviceHandler *theDevice, AudioSink *mySink, int32_t inputRate = 2304000, int32_t fmRate = 192000,
                int32_t workingRate = 48000, int32_t audioRate = 48000, int device = 0)
        : myRig(theDevice), theSink(mySink) {
        fmx_config c{};
        c.struct_size = (int32_t)sizeof(c); c.device = device; c.channels = 1; c.streams = 0; c.stream_of_channel = nullptr;
        c.inputRate = inputRate; c.fmRate = fmRate; c.workingRate = workingRate; c.audioRate = audioRate;
        c.max_block = bufferSize;
        if (fmx_abi_version() != FMX_ABI_VERSION) { err = "libfmx has another ABI version than this adapter was built for"; h = nullptr; return; }
        check(fmx_create(&c, &h));
        inBuf.resize(bufferSize);
        // one PCM frame per 4 fm samples; an input rate the reference does not decimate (192 kS/s devices) gives bufferSize fm samples per
        // block; the second converter makes audioRate / workingRate frames of every 48 kHz frame
        outBuf.resize((size_t)((int64_t)(bufferSize / 4 + 64) * std::max(audioRate, workingRate) / workingRate + 8));
    }
    ~FmProcessor() { stop(); if (h) fmx_destroy(h); }
    FmProcessor(const FmProcessor &) = delete;
    FmProcessor &operator=(const FmProcessor &) = delete;

    bool ok() const { return h != nullptr; }
    const std::string &lastError() const { return err; }

    // ---- the reference's setters, fm-processor.h:104-156 ----
    void setfmMode(FM_Mode m) { set(FMX_P_FM_MODE, (double)(int)m); }
    void setFMdecoder(const std::string &name) {                          // fm-demodulator.cpp:93-103
        static const char *names[] = { "AM", "FM PLL Decoder", "FM Mixed Demod", "FM Complex Baseband Delay",
                                       "FM Real Baseband Delay", "FM Difference Based" };
        int code = 2;                                                      // unknown name -> `default:` = PLL
        for (int i = 0; i < 6; i++) if (name == names[i]) code = i + 1;
        set(FMX_P_FM_DECODER, code);
    }
    void setSoundMode(uint8_t selector) { set(FMX_P_SOUND_MODE, selector); }
    void setStereoPanorama(int16_t pan) { set(FMX_P_STEREO_PANORAMA, pan); }
    void setSoundBalance(int16_t balance) { set(FMX_P_SOUND_BALANCE, balance); }
    void setDeemphasis(int16_t us) { set(FMX_P_DEEMPHASIS, us); }
    void setVolume(float gainDb) { set(FMX_P_VOLUME_DB, gainDb); }
    void setlfcutoff(int32_t hz) { set(FMX_P_LF_CUTOFF, hz); }
    void setBandwidth(const std::string &s) {                              // "165kHz" | "Off" (fm-processor.cpp:232-239)
        set(FMX_P_BANDWIDTH, s == "Off" ? 0.0 : 1000.0 * std::strtol(s.c_str(), nullptr, 10));
    }
    void setAttenuation(float l, float r) { set(FMX_P_ATTENUATION_L, l); set(FMX_P_ATTENUATION_R, r); }
    void setfmRdsSelector(int mode) { set(FMX_P_RDS_MODE, mode); }
    void triggerFrequencyChange() { set(FMX_A_TRIGGER_FREQUENCY_CHANGE, 0); }
    void restartPssAnalyzer() { set(FMX_A_RESTART_PSS, 0); }
    void resetRds() { set(FMX_A_RESET_RDS, 0); }
    void set_localOscillator(int32_t lo) { set(FMX_P_LOCAL_OSCILLATOR, lo); }
    void set_squelchMode(int m) { set(FMX_P_SQUELCH_MODE, m); }
    void setAutoMonoMode(bool b) { set(FMX_P_AUTO_MONO, b); }
    void setPSSMode(bool b) { set(FMX_P_PSS, b); }
    void setDCRemove(bool b) { set(FMX_P_DC_REMOVE, b); }
    void setTestTone(bool b) { set(FMX_P_TEST_TONE, b); }
    void setDispDelay(int steps) { set(FMX_P_DISP_DELAY, steps); }       // fm-processor.cpp:935-937
    void set_squelchValue(int v) { set(FMX_P_SQUELCH_VALUE, v); }        // :213-215
    // scan mode (fm-processor.cpp:361-367): taken over at the next block; the constructor's thresHold (:63,108) as a setter
    void startScanning() { scanning.store(true); }
    void stopScanning() { scanning.store(false); }
    void setScanThreshold(int16_t thresHold) { set(FMX_P_SCAN_THRESHOLD, thresHold); }

    bool isPilotLocked(float &oLockStrength) {                             // fm-processor.cpp:870-880
        fmx_meta m{};
        if (fmx_get_meta(h, 0, &m) != FMX_OK) { oLockStrength = 0; return false; }
        oLockStrength = m.live_lock_strength;
        return m.live_pilot_locked != 0;
    }
    float get_demodDcComponent() { fmx_meta m{}; return fmx_get_meta(h, 0, &m) == FMX_OK ? m.live_dc_if : 0.0f; }
    bool getSquelchState() { fmx_meta m{}; return fmx_get_meta(h, 0, &m) == FMX_OK && m.squelch_active != 0; }      // fm-processor.cpp:217-219

    // ---- the processing loop ----
    // One iteration of the while loop of fmProcessor::run() (fm-processor.cpp:387-686).  Returns false
    // when the device holds fewer than bufferSize samples (the reference sleeps 1 ms and retries).
    // `before_block`, when given, runs once a block is known to be waiting and before it is taken: the place to read state that belongs in
    // front of the block (the Qt adapter latches its dump flag and the RfDC value there, not on iterations that find no block)
    template <class F> bool run_block(F before_block) {
        if (!h || myRig->Samples() < bufferSize) return false;
        before_block();
        return take_block();
    }
    bool run_block() { return run_block([] {}); }
    bool take_block() {
        const int32_t amount = myRig->getSamples(inBuf.data(), bufferSize);
        lastN = amount;
        // the scanning flag is read once per block: while it is set the reference's loop feeds its scan buffer and sends nothing on (:478-495)
        const bool scan = scanning.load();
        if (scan != lastScan && !check(fmx_set_param(h, 0, FMX_P_SCANNING, scan ? 1.0 : 0.0))) return false;
        lastScan = scan;
        int64_t frames = 0;
        if (!check(fmx_process_host(h, reinterpret_cast<const float *>(inBuf.data()), amount, amount,
                                    reinterpret_cast<float *>(outBuf.data()), (int64_t)outBuf.size(), &frames)))
            return false;
        if (frames > 0 && theSink && !scan) theSink->putSamples(outBuf.data(), (int32_t)frames);
        fmCount += fmx_last_fm_samples(h);                                    // (amount / the reference's decimation at this input rate)
        return true;
    }
    // QThread::run() equivalent; stop() as fm-processor.cpp:204-211
    void run() { running.store(true); while (running.load()) { if (!run_block()) idle(); } }
    void stop() { running.store(false); }

    // what the reference emits as showMetaData every fmRate/2 samples (fm-processor.cpp:662-684)
    bool poll_meta(SMetaData &out) {
        if (fmCount - lastMeta <= 96000) return false;
        lastMeta = fmCount;
        fmx_meta m{};
        if (fmx_get_meta(h, 0, &m) != FMX_OK) return false;
        out.DcValRf = m.DcValRf; out.DcValIf = m.DcValIf; out.PssPhaseShiftDegree = m.PssPhaseShiftDegree;
        out.PssPhaseChange = m.PssPhaseChange; out.PssState = (SMetaData::EPssState)m.PssState;
        out.PilotPllLockStrength = m.PilotPllLockStrength; out.PilotPllLocked = m.PilotPllLocked != 0;
        return true;
    }

    // what the reference emits as showPeakLevel (leftDb, rightDb) every 961 PCM frames (fm-processor.cpp:772-798):
    // calls `emit_fn(leftDb, rightDb)` once per window that closed since the last poll, oldest first
    template <class F> int poll_peaks(F emit_fn) {
        float lr[2 * 64]; int32_t n = 0;
        if (fmx_get_peaks(h, 0, lr, 64, &n) != FMX_OK) return 0;
        if (lastScan) return 0;                                             // (a scanning block feeds no meter: the windows are taken and dropped)
        for (int32_t k = 0; k < n; k++) emit_fn(lr[2 * k], lr[2 * k + 1]);
        return n;
    }

    // what the reference's scan emits (fm-processor.cpp:483-493): calls `emit_fn(const fmx_scan_result &)` once per block completed since the
    // last poll, oldest first; the reference emits scanresult () for the records with `found` set
    template <class F> int poll_scan(F emit_fn) {
        fmx_scan_result r[64]; int32_t n = 0, total = 0;
        do {
            if (fmx_scan_results(h, 0, r, 64, &n) != FMX_OK) return total;
            for (int32_t k = 0; k < n; k++) emit_fn(r[k]);
            total += n;
        } while (n == 64);
        return total;
    }
    // the modulation meter (include/fmx.h fmx_mod_records; nothing of the reference's): setModulationMeter switches it with the next block, pollModulation
    // calls `emit_fn(const fmx_mod_record &)` once per 50 ms window completed since the last poll, oldest first
    void setModulationMeter(bool on) { if (h) check(fmx_mod_meter_enable(h, 0, on ? 1 : 0)); }
    template <class F> int pollModulation(F emit_fn) {
        fmx_mod_record r[64]; int32_t n = 0;
        if (!h || fmx_mod_records(h, 0, 1, r, 64, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(r[k]);
        return n;
    }
    // the programme audio meter (include/fmx.h fmx_audio_records; nothing of the reference's): setAudioMeter switches it with the next block, pollAudio
    // calls `emit_fn(const fmx_audio_record &)` once per 100 ms window completed since the last poll, oldest first (fmx_audio_loudness makes LUFS of them)
    void setAudioMeter(bool on) { if (h) check(fmx_audio_meter_enable(h, 0, on ? 1 : 0)); }
    template <class F> int pollAudio(F emit_fn) {
        fmx_audio_record r[64]; int32_t n = 0;
        if (!h || fmx_audio_records(h, 0, 1, r, 64, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(r[k]);
        return n;
    }
    // the reception meter (include/fmx.h fmx_rx_records; nothing of the reference's): setReceptionMeter switches it with the next block, pollReception
    // calls `emit_fn(const fmx_rx_record &)` once per 50 ms window completed since the last poll, oldest first (fmx_rx_quality_of makes level, C/N, envelope
    // depth and offset of them: receptionQuality over the records one poll handed out)
    void setReceptionMeter(bool on) { if (h) check(fmx_rx_meter_enable(h, 0, on ? 1 : 0)); }
    template <class F> int pollReception(F emit_fn) {
        fmx_rx_record r[64]; int32_t n = 0;
        if (!h || fmx_rx_records(h, 0, 1, r, 64, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(r[k]);
        return n;
    }
    static bool receptionQuality(const fmx_rx_record *recs, int32_t n, fmx_rx_quality *q, int32_t fmRate = 192000) { return fmx_rx_quality_of(recs, n, fmRate, q) == FMX_OK; }
    // the RDS meter (include/fmx.h fmx_rds_meter_records; nothing of the reference's): setRdsMeter switches it with the next block (it switches no RDS
    // decoder on), pollRdsMeter calls `emit_fn(const fmx_rds_meter_record &)` once per window of 2560 RDS samples completed since the last poll, oldest
    // first; rdsMeterCal is the channel's calibration from the handle's taps, rdsMeterFigures makes injection, phase and axis ratio of the records
    void setRdsMeter(bool on) { if (h) check(fmx_rds_meter_enable(h, 0, on ? 1 : 0)); }
    template <class F> int pollRdsMeter(F emit_fn) {
        fmx_rds_meter_record r[64]; int32_t n = 0;
        if (!h || fmx_rds_meter_records(h, 0, 1, r, 64, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(r[k]);
        return n;
    }
    bool rdsMeterCal(fmx_rds_meter_calib *cal) { return h && check(fmx_rds_meter_cal(h, 0, cal)); }
    static bool rdsMeterFigures(const fmx_rds_meter_record *recs, int32_t n, const fmx_rds_meter_calib *cal, double hz_per_unit, fmx_rds_figures *f) {
        return fmx_rds_meter_figures(recs, n, cal, hz_per_unit, f) == FMX_OK;
    }
    // the spectrum meter (include/fmx.h fmx_spectrum_*; the reference hands these samples to its HF scope): setSpectrumGrid sets blocks per record and
    // `every` while the meter is off, setSpectrumMeter switches it with the next block, pollSpectrum calls
    // `emit_fn(const fmx_spectrum_record &, const float *mean, const float *peak)` (4096 bins each) once per record of this processor's stream completed
    // since the last poll, oldest first; spectrumFigures makes bandwidth, adjacent-channel and mask figures of one record
    bool setSpectrumGrid(int32_t blocks_per_record, int32_t every) { return h && check(fmx_spectrum_setup(h, blocks_per_record, every)); }
    void setSpectrumMeter(bool on) { if (h) check(fmx_spectrum_enable(h, 0, on ? 1 : 0)); }
    template <class F> int pollSpectrum(F emit_fn) {
        fmx_spectrum_record r[4]; int32_t n = 0;
        std::vector<float> mean(4 * 4096), peak(4 * 4096);
        if (!h || fmx_spectrum_read(h, 0, r, mean.data(), peak.data(), 4, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(r[k], mean.data() + (size_t)k * 4096, peak.data() + (size_t)k * 4096);
        return n;
    }
    static bool spectrumFigures(const fmx_spectrum_find *cfg, const float *mean, const float *peak, fmx_spectrum_figs *f) {
        return fmx_spectrum_figures(cfg, mean, peak, f) == FMX_OK;
    }
    // the multiplex spectrum meter (include/fmx.h fmx_mpx_*; the reference's LF scope with setlfPlotType (DEMODULATOR), fm-processor.cpp:597-660):
    // setMpxSpectrumGrid sets blocks per record and `every` while the meter is off, setMpxSpectrumMeter switches it with the next block, pollMpxSpectrum
    // calls `emit_fn(const fmx_mpx_record &, const float *mean, const float *peak)` (2048 bins each, bin k at k fmRate / 4096 Hz) once per record of this
    // processor's channel completed since the last poll, oldest first; mpxFigures makes deviation, pilot, carrier and floor figures of one record
    bool setMpxSpectrumGrid(int32_t blocks_per_record, int32_t every) { return h && check(fmx_mpx_spectrum_setup(h, blocks_per_record, every)); }
    void setMpxSpectrumMeter(bool on) { if (h) check(fmx_mpx_spectrum_enable(h, 0, on ? 1 : 0)); }
    template <class F> int pollMpxSpectrum(F emit_fn) {
        fmx_mpx_record r[4]; int32_t n = 0;
        std::vector<float> mean(4 * 2048), peak(4 * 2048);
        if (!h || fmx_mpx_spectrum_read(h, 0, 1, r, mean.data(), peak.data(), 4, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(r[k], mean.data() + (size_t)k * 2048, peak.data() + (size_t)k * 2048);
        return n;
    }
    static bool mpxFigures(const fmx_mpx_find *cfg, const float *mean, const float *peak, fmx_mpx_figs *f) {
        return fmx_mpx_figures(cfg, mean, peak, f) == FMX_OK;
    }
    // the sub-carrier decoder (include/fmx.h fmx_sca_*; no counterpart in the reference): setScaSetup sets the filters and the deviation while no channel
    // decodes (NULL: the defaults), setScaDecoder switches this processor's channel on at centre_hz (67 000, 76 000, 82 000 at 192 kS/s; 0: off) with the next
    // call, pollSca calls `emit_fn(int64_t block, const float *audio, float level)` (240 samples at fmRate / 8) once per block completed since the last
    // poll, oldest first, up to a gap
    bool setScaSetup(const fmx_sca_config *cfg) { return h && check(fmx_sca_setup(h, cfg)); }
    bool setScaDecoder(int32_t centre_hz) { return h && check(fmx_sca_enable(h, 0, centre_hz)); }
    template <class F> int pollSca(F emit_fn) {
        int64_t first = -1; int32_t n = 0;
        std::vector<float> audio((size_t)128 * 240), level(128);
        if (!h || fmx_sca_read(h, 0, 1, &first, audio.data(), level.data(), 128, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(first + k, audio.data() + (size_t)k * 240, level[(size_t)k]);
        return n;
    }
    // the monitoring feed (include/fmx.h fmx_feed_*; no counterpart in the reference): setFeed switches this processor's channel's 16 kS/s mono feed with
    // the next call (0: off, 1: (L + R) / 2, 2: left, 3: right); pollFeed calls `emit_fn(int64_t block, const float *audio, float power)` (160 samples;
    // block b belongs to the PCM frames [480 b, 480 b + 480)) once per block completed since the last poll, oldest first, up to a gap; pollFeedS16 the same
    // with `const int16_t *audio`, converted on the device
    bool setFeed(int32_t mode) { return h && check(fmx_feed_enable(h, 0, mode)); }
    template <class F> int pollFeed(F emit_fn) {
        int64_t first = -1; int32_t n = 0;
        std::vector<float> audio((size_t)128 * 160), power(128);
        if (!h || fmx_feed_read(h, 0, 1, &first, audio.data(), FMX_FEED_F32, power.data(), 128, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(first + k, audio.data() + (size_t)k * 160, power[(size_t)k]);
        return n;
    }
    template <class F> int pollFeedS16(F emit_fn) {
        int64_t first = -1; int32_t n = 0;
        std::vector<int16_t> audio((size_t)128 * 160); std::vector<float> power(128);
        if (!h || fmx_feed_read(h, 0, 1, &first, audio.data(), FMX_FEED_S16, power.data(), 128, &n) != FMX_OK) return 0;
        for (int32_t k = 0; k < n; k++) emit_fn(first + k, audio.data() + (size_t)k * 160, power[(size_t)k]);
        return n;
    }
    // the RDS picture of this processor's channel(s) in one read-out of the device (fmx_rds_decode_all: the block synchroniser has run on the GPU,
    // the group decoder runs here): what the rds classes' signals carried, infos[k] for channel first + k
    bool poll_rds(fmx_rds_info *infos, int32_t first = 0, int32_t count = 1) { return h && check(fmx_rds_decode_all(h, first, count, infos)); }
    // the last block was processed while scanning: the GUI's scope feeds skip it, as the reference's loop does
    bool lastBlockScanned() const { return lastScan; }

    static constexpr int32_t bufferSize = 2 * 8192;                        // fm-processor.cpp:374

    // what the GUI side-band feeds of run() need (fm-processor.cpp:420-421, 555-563, 597-660): the raw block just processed
    // and the library handle for fmx_get_tap / fmx_rds_*
    const std::complex<float> *lastBlock() const { return inBuf.data(); }
    int32_t lastAmount() const { return lastN; }
    fmx_handle handle() const { return h; }
    void set_ptyLocale(int l) { ptyLocale = l; }                            // fm-processor.cpp:939-941 (used by the adapter's PTY names)
    int get_ptyLocale() const { return ptyLocale; }

protected:
    virtual void idle() {}                                                  // the Qt build calls msleep(1) here

private:
    bool check(int rc) { if (rc != FMX_OK) { err = fmx_last_error(); return false; } return true; }
    void set(int id, double v) { if (h) check(fmx_set_param(h, 0, id, v)); }
    fmx_handle h = nullptr;
    DeviceHandler *myRig;
    AudioSink *theSink;
    std::vector<std::complex<float>> inBuf, outBuf;
    std::atomic<bool> running{false};
    std::atomic<bool> scanning{false};
    bool lastScan = false;                                                  // the flag the last block was processed with (and handed to the library)
    std::string err;
    int64_t fmCount = 0, lastMeta = 0;
    int32_t lastN = 0;
    int ptyLocale = 0;
};

}  // namespace fmx_host

// wideband_adapter.h -- host-side C++ wrapper of stage W, the wide-band ingest stage (include/fmx.h fmx_wideband; DESIGN.md "Stage W").
//
// The stage has no counterpart in the reference: its device handlers deliver one station's 2 304 000 S/s.  A receiver of 10 - 20 MS/s
// (Airspy R2, HackRF, LimeSDR, Pluto) hands its stream to a Wideband object, which produces one 2 304 000 S/s stream per station in the
// layout fmx_process_device takes; the handle behind it is the one fm_processor_adapter.h wraps.  Header-only; links against libfmx.so
// only.  Nothing throws: a failed call returns false and lastError() holds the library's text.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fmx.h"

namespace fmx_host {

class Wideband {
public:
    // stream_of_output [m]: the wide stream station m is cut from; offset_hz [m]: its carrier relative to the stream's centre
    Wideband(int32_t factor, int32_t streams, const std::vector<int32_t> &stream_of_output, const std::vector<int32_t> &offset_hz,
             int32_t max_block, int device = 0)
        : K(factor), nOutputs((int32_t)stream_of_output.size()) {
        if (fmx_abi_version() != FMX_ABI_VERSION) { err = "libfmx has another ABI version than this adapter was built for"; return; }
        if (offset_hz.size() != stream_of_output.size()) { err = "one offset per output"; return; }
        fmx_wideband_config c{};
        c.struct_size = (int32_t)sizeof(c); c.device = device; c.streams = streams; c.factor = factor; c.outputs = nOutputs;
        c.stream_of_output = stream_of_output.data(); c.offset_hz = offset_hz.data(); c.max_block = max_block;
        if (fmx_wideband_create(&c, &w) != FMX_OK) { err = fmx_last_error(); w = nullptr; }
    }
    // A receiver whose rate is no multiple of 2 304 000 (Airspy at 2.5 / 10, SDRplay at 8, a USRP at 12.5 MS/s, a recorded file at 20): a rate
    // object (fmx_wideband_create_rate).  factor () is 0; a call's count is outputsFor (n_wide), no longer n_wide / factor ().
    struct Rate { int32_t hz; };
    Wideband(Rate wide_rate, int32_t streams, const std::vector<int32_t> &stream_of_output, const std::vector<int32_t> &offset_hz,
             int32_t max_block, int device = 0)
        : K(0), nOutputs((int32_t)stream_of_output.size()) {
        if (fmx_abi_version() != FMX_ABI_VERSION) { err = "libfmx has another ABI version than this adapter was built for"; return; }
        if (offset_hz.size() != stream_of_output.size()) { err = "one offset per output"; return; }
        fmx_wideband_config c{};
        c.struct_size = (int32_t)sizeof(c); c.device = device; c.streams = streams; c.factor = 0; c.outputs = nOutputs;
        c.stream_of_output = stream_of_output.data(); c.offset_hz = offset_hz.data(); c.max_block = max_block;
        if (fmx_wideband_create_rate(&c, wide_rate.hz, &w) != FMX_OK) { err = fmx_last_error(); w = nullptr; }
    }
    ~Wideband() { if (w) fmx_wideband_destroy(w); }
    Wideband(const Wideband &) = delete;
    Wideband &operator=(const Wideband &) = delete;

    bool ok() const { return w != nullptr; }
    const std::string &lastError() const { return err; }
    int32_t factor() const { return K; }
    int32_t outputs() const { return nOutputs; }
    static int32_t narrowRate() { return 2304000; }

    // retune station m; any thread; takes effect at the first sample of the next call
    bool setOffset(int32_t output, int32_t hz) { return check(fmx_wideband_set_offset(w, output, hz)); }

    // n_wide (a multiple of factor ()) samples per stream, device pointers, asynchronous on hip_stream: station m's n_wide / factor ()
    // samples land at d_narrow + 2 * m * narrow_stride -- fmx_process_device (h, d_narrow, narrow_stride, n_wide / factor (), ...) on the
    // same stream takes them as they lie
    bool processDevice(const void *d_wide, fmx_iq_format format, float s16_denominator, int64_t wide_stride, int64_t n_wide,
                       float *d_narrow, int64_t narrow_stride, void *hip_stream, int64_t *n_narrow = nullptr) {
        return check(fmx_wideband_process_device_raw(w, d_wide, (int32_t)format, s16_denominator, wide_stride, n_wide, d_narrow, narrow_stride,
                                                     n_narrow, hip_stream));
    }
    // the same with host buffers, synchronous
    bool processHost(const void *wide, fmx_iq_format format, float s16_denominator, int64_t wide_stride, int64_t n_wide, float *narrow,
                     int64_t narrow_stride, int64_t *n_narrow = nullptr) {
        return check(fmx_wideband_process_host_raw(w, wide, (int32_t)format, s16_denominator, wide_stride, n_wide, narrow, narrow_stride, n_narrow));
    }
    // the outputs per station that the next call will produce for n_wide samples (the processing thread's)
    int64_t outputsFor(int64_t n_wide) const { return fmx_wideband_outputs_for(w, n_wide); }
    // a rate object's prototype: 16 M + 1 real taps (needs no device); empty where the rate is refused
    static std::vector<float> rateTaps(int32_t wide_rate_hz, int32_t *L = nullptr, int32_t *M = nullptr) {
        int32_t n = 0;
        std::vector<float> h;
        if (fmx_wideband_rate_taps(wide_rate_hz, nullptr, 0, &n, L, M) != FMX_E_TOO_LARGE) return h;
        h.resize((size_t)n);
        if (fmx_wideband_rate_taps(wide_rate_hz, h.data(), n, &n, L, M) != FMX_OK) h.clear();
        return h;
    }
    // the stage's low-pass: 16 factor + 1 real taps (needs no device)
    static std::vector<float> taps(int32_t factor) {
        std::vector<float> h(16 * 16 + 1);
        int32_t n = 0;
        if (fmx_wideband_taps(factor, h.data(), (int32_t)h.size(), &n) != FMX_OK) n = 0;
        h.resize((size_t)n);
        return h;
    }

    // the band survey (fmx_wideband_survey_*): from the next call on every stream's averaged power spectrum, records of blocks_per_record
    // blocks of 4096 wide samples (1 .. 4096; 0 ends it).  The processing thread's, as readSurvey.
    bool survey(int32_t blocks_per_record) { return check(fmx_wideband_survey_enable(w, blocks_per_record)); }
    // the records of `stream` completed since its last read, oldest first, at most `capacity`: recs [i] and power [4096 i .. 4096 i + 4095]
    bool readSurvey(int32_t stream, std::vector<fmx_survey_record> &recs, std::vector<float> &power, int32_t capacity = 4) {
        recs.assign((size_t)(capacity > 0 ? capacity : 0), fmx_survey_record{});
        power.assign(recs.size() * 4096, 0.0f);
        int32_t n = 0;
        const bool ok = check(fmx_wideband_survey_read(w, stream, recs.data(), power.data(), (int32_t)recs.size(), &n));
        recs.resize((size_t)n);
        power.resize((size_t)n * 4096);
        return ok;
    }
    // the stations of one record (needs no device): the raster offsets setOffset accepts, ascending; empty where an argument is rejected
    static std::vector<fmx_survey_station> stations(const float *power, int32_t factor, int32_t raster_hz = 100000, int32_t origin_hz = 0,
                                                    float threshold_db = 10.0f, int32_t dc_guard_hz = 0, float *floor_db = nullptr) {
        fmx_survey_find f{};
        f.struct_size = (int32_t)sizeof(f); f.factor = factor; f.raster_hz = raster_hz; f.origin_hz = origin_hz; f.dc_guard_hz = dc_guard_hz;
        f.threshold_db = threshold_db;
        std::vector<fmx_survey_station> out(16);
        int32_t n = 0;
        int rc = fmx_wideband_survey_stations(&f, power, out.data(), (int32_t)out.size(), &n, floor_db);
        if (rc == FMX_E_TOO_LARGE) { out.resize((size_t)n); rc = fmx_wideband_survey_stations(&f, power, out.data(), (int32_t)out.size(), &n, floor_db); }
        out.resize(rc == FMX_OK ? (size_t)n : 0);
        return out;
    }

private:
    bool check(int rc) { if (rc != FMX_OK) err = fmx_last_error(); return rc == FMX_OK; }
    fmx_wideband w = nullptr;
    int32_t K, nOutputs;
    std::string err;
};

}  // namespace fmx_host

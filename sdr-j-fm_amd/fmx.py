"""ctypes binding of libfmx (include/fmx.h) plus a host-side mirror of the reference's
``fmProcessor`` interface (includes/fm/fm-processor.h:104-156) for the FM hot path.

This module never computes DSP itself and has no CPU fallback: if libfmx.so or a HIP device
is missing every call raises ``FmxError``.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMX_LIB") or os.path.join(HERE, "lib", "libfmx.so")      # FMX_LIB: A/B runs of two builds

# error codes (include/fmx.h)
FMX_OK, FMX_E_INVALID, FMX_E_UNSUPPORTED, FMX_E_NO_DEVICE, FMX_E_HIP, FMX_E_NOMEM, FMX_E_TOO_LARGE = 0, -1, -2, -3, -4, -5, -6

# parameter ids (include/fmx.h fmx_param_id)
ABI_VERSION = 3               # FMX_ABI_VERSION of include/fmx.h this mirror follows
P_FM_MODE, P_FM_DECODER, P_SOUND_MODE, P_STEREO_PANORAMA, P_SOUND_BALANCE, P_DEEMPHASIS = 1, 2, 3, 4, 5, 6
P_VOLUME_DB, P_LF_CUTOFF, P_BANDWIDTH, P_ATTENUATION_L, P_ATTENUATION_R, P_RDS_MODE = 7, 8, 9, 10, 11, 12
P_LOCAL_OSCILLATOR, P_AUTO_MONO, P_PSS, P_DC_REMOVE, P_SQUELCH_MODE, P_TEST_TONE, P_SQUELCH_VALUE = 13, 14, 15, 16, 17, 18, 19
P_DISP_DELAY = 20
P_STAGEB_FORM = 22            # handle-wide: 0 automatic, 1 stage B as one kernel per call, 2 as two (bit-identical results)
P_FRONT_KERNEL = 25           # handle-wide: 0 automatic, 1 fmx_front.hip (packed f32 FMAs), 3 fmx_front4.hip (f16-split matrix FIR; 2 was the six-wave kernel now in tools/experiments)
P_SCOPE_TAPS = 26             # handle-wide: -1 automatic (up to 64 channels), 0 the display feeds (demodulator / LR / pilot-phase scope taps, peak meter) are not produced, 1 produced
P_CALL_PIECES = 27            # handle-wide: -1 automatic, 0 never, n > 0 fm samples per piece of a call made in overlapping pieces (pre-pass batches)
P_FRONT_PARTS = 24            # handle-wide: 0 automatic, 1 one workgroup per channel, 2..32 parts in time per channel (bit-identical results)
P_FILTER_RESTARTS = 23        # handle-wide, before the first call: 0 automatic, 1 the reference's block filters (<= 64 channels), 2 folded FIRs
P_PLL_SOLVER = 21             # 0 automatic, 1 sequential (the reference's trajectory), 2 Newton while in lock + sequential around lock decisions, 3 Newton always
P_SCANNING = 28               # per channel: 0 / 1, startScanning / stopScanning (the channel's PCM of a scanning call is zeros; its chain runs on)
P_SCAN_THRESHOLD = 29         # per channel: the constructor's thresHold in dB, an integer in -32768..32767 (default 20)
A_TRIGGER_FREQUENCY_CHANGE, A_RESTART_PSS, A_RESET_RDS = 100, 101, 102

TAP_FM_IQ, TAP_DEMOD, TAP_LR_RAW, TAP_PRE_RESAMPLER, TAP_RDS_IQ, TAP_PILOT_PHASE = 0, 1, 2, 3, 4, 5
IQ_F32, IQ_U8, IQ_S8, IQ_S16 = 0, 1, 2, 3

EXPORTS = [
    "fmx_abi_version", "fmx_last_error", "fmx_create", "fmx_destroy", "fmx_set_param", "fmx_frames_for", "fmx_filter_change_due",
    "fmx_process_host", "fmx_process_device", "fmx_process_host_raw", "fmx_process_device_raw", "fmx_synchronize",
    "fmx_get_meta", "fmx_get_tap", "fmx_get_peaks",
    "fmx_scan_results", "fmx_mod_meter_enable", "fmx_mod_records", "fmx_mod_hz_per_unit", "fmx_audio_meter_enable", "fmx_audio_records", "fmx_audio_loudness", "fmx_rx_meter_enable", "fmx_rx_records", "fmx_rx_quality_of", "fmx_rds_meter_enable", "fmx_rds_meter_records", "fmx_rds_meter_cal", "fmx_rds_meter_figures", "fmx_spectrum_setup", "fmx_spectrum_enable", "fmx_spectrum_read", "fmx_spectrum_figures", "fmx_mpx_spectrum_setup", "fmx_mpx_spectrum_enable", "fmx_mpx_spectrum_read", "fmx_mpx_figures", "fmx_sca_setup", "fmx_sca_enable", "fmx_sca_read", "fmx_sca_taps", "fmx_sca_info", "fmx_feed_enable", "fmx_feed_read", "fmx_feed_read_device", "fmx_feed_taps", "fmx_feed_info", "fmx_feed_allocated", "fmx_rds_bits", "fmx_rds_symbols", "fmx_last_fm_samples", "fmx_pll_replays", "fmx_pll_exact_segments", "fmx_last_front_kernel", "fmx_last_call_pieces", "fmx_last_second_group", "fmx_last_rds_samples", "fmx_last_rds_samples_of", "fmx_rds_decode", "fmx_rds_decode_all", "fmx_rds_groups", "fmx_rds_decode_bits", "fmx_rds_pty_name", "fmx_rds_map_char", "fmx_rds_prepare_text", "fmx_get_taps", "fmx_profile_enable", "fmx_profile_read",
    "fmx_wideband_create", "fmx_wideband_destroy", "fmx_wideband_set_offset", "fmx_wideband_process_device_raw", "fmx_wideband_process_host_raw", "fmx_wideband_taps",
    "fmx_wideband_survey_enable", "fmx_wideband_survey_read", "fmx_wideband_survey_stations",
    "fmx_wideband_create_rate", "fmx_wideband_outputs_for", "fmx_wideband_rate_taps", "fmx_wideband_survey_stations_rate",
]


class FmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libfmx error %d: %s" % (code, msg))
        self.code = code


class FmxConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32), ("channels", C.c_int32), ("streams", C.c_int32),
        ("stream_of_channel", C.POINTER(C.c_int32)),
        ("inputRate", C.c_int32), ("fmRate", C.c_int32), ("workingRate", C.c_int32), ("audioRate", C.c_int32),
        ("max_block", C.c_int32),
    ]


class FmxWidebandConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("device", C.c_int32), ("streams", C.c_int32), ("factor", C.c_int32), ("outputs", C.c_int32),
        ("stream_of_output", C.POINTER(C.c_int32)), ("offset_hz", C.POINTER(C.c_int32)), ("max_block", C.c_int32),
    ]


class FmxSurveyRecord(C.Structure):
    _fields_ = [("index", C.c_int64), ("end_sample", C.c_int64), ("blocks", C.c_int32), ("reserved", C.c_int32)]


class FmxSurveyFind(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("factor", C.c_int32), ("raster_hz", C.c_int32), ("origin_hz", C.c_int32),
                ("dc_guard_hz", C.c_int32), ("threshold_db", C.c_float)]


class FmxSurveyStation(C.Structure):
    _fields_ = [("offset_hz", C.c_int32), ("level_db", C.c_float), ("snr_db", C.c_float), ("reserved", C.c_int32)]


# fmx_survey_record / fmx_survey_station as numpy records (Wideband.survey_read, survey_stations)
SURVEY_RECORD_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("blocks", np.int32), ("reserved", np.int32)])
SURVEY_STATION_DTYPE = np.dtype([("offset_hz", np.int32), ("level_db", np.float32), ("snr_db", np.float32), ("reserved", np.int32)])
assert SURVEY_RECORD_DTYPE.itemsize == C.sizeof(FmxSurveyRecord) and SURVEY_STATION_DTYPE.itemsize == C.sizeof(FmxSurveyStation)
SURVEY_BINS = 4096


class FmxSpectrumRecord(C.Structure):
    _fields_ = [("index", C.c_int64), ("end_sample", C.c_int64), ("blocks", C.c_int32), ("every", C.c_int32)]


class FmxSpectrumMaskPoint(C.Structure):
    _fields_ = [("offset_hz", C.c_double), ("limit_db", C.c_double)]


class FmxSpectrumFind(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rate_hz", C.c_int32), ("centre_hz", C.c_int32), ("raster_hz", C.c_int32), ("dc_guard_hz", C.c_int32),
                ("rbw_hz", C.c_int32), ("obw_fraction", C.c_double), ("x_db", C.c_double), ("mask", C.POINTER(FmxSpectrumMaskPoint)),
                ("n_mask", C.c_int32), ("reserved", C.c_int32)]


class FmxSpectrumFigs(C.Structure):
    _fields_ = [("channel_db", C.c_double), ("obw_hz", C.c_double), ("obw_lower_hz", C.c_double), ("obw_upper_hz", C.c_double), ("xdb_hz", C.c_double),
                ("centroid_hz", C.c_double), ("adj_db", C.c_double * 4), ("mask_margin_db", C.c_double), ("mask_worst_hz", C.c_double)]


# fmx_spectrum_record as a numpy record (Fmx.spectrum_read)
SPECTRUM_RECORD_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("blocks", np.int32), ("every", np.int32)])
assert SPECTRUM_RECORD_DTYPE.itemsize == C.sizeof(FmxSpectrumRecord) == 24
SPECTRUM_BINS = 4096
SPECTRUM_RING = 4             # records the library keeps per metered stream


class FmxMpxRecord(C.Structure):
    _fields_ = [("index", C.c_int64), ("end_sample", C.c_int64), ("blocks", C.c_int32), ("every", C.c_int32)]


class FmxMpxBand(C.Structure):
    _fields_ = [("lo_hz", C.c_double), ("hi_hz", C.c_double)]


class FmxMpxFind(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rate_hz", C.c_int32), ("hz_per_unit", C.c_double), ("dc_guard_hz", C.c_int32), ("line_half_hz", C.c_int32),
                ("bands", C.POINTER(FmxMpxBand)), ("n_bands", C.c_int32), ("reserved", C.c_int32)]


class FmxMpxFigs(C.Structure):
    _fields_ = [("total_hz", C.c_double), ("mono_hz", C.c_double), ("stereo_hz", C.c_double), ("rds_hz", C.c_double), ("aux_hz", C.c_double),
                ("pilot_hz", C.c_double), ("pilot_freq_hz", C.c_double), ("carrier38_hz", C.c_double), ("floor_hz_rt_hz", C.c_double),
                ("pilot_cn0_db", C.c_double), ("band_hz", C.c_double * 16), ("band_line_hz", C.c_double * 16), ("band_hold_line_hz", C.c_double * 16),
                ("band_hold_over_mean_db", C.c_double * 16)]


# fmx_mpx_record as a numpy record (Fmx.mpx_spectrum_read)
MPX_RECORD_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("blocks", np.int32), ("every", np.int32)])
assert MPX_RECORD_DTYPE.itemsize == C.sizeof(FmxMpxRecord) == 24
MPX_BINS = 2048               # bin k at k * fmRate / 4096 Hz
MPX_RING = 4                  # records the library keeps per metered channel


class FmxScaConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("half_band_hz", C.c_int32), ("audio_cut_hz", C.c_int32), ("deviation_hz", C.c_int32), ("deemphasis_us", C.c_int32)]


class FmxScaInfo(C.Structure):
    _fields_ = [("audio_rate_hz", C.c_int32), ("block_audio", C.c_int32), ("block_fm", C.c_int32), ("lookback_fm", C.c_int32), ("delay_fm", C.c_double),
                ("ring_blocks", C.c_int32), ("bytes_per_channel", C.c_int32)]


SCA_BLOCK_AUDIO = 240         # audio samples per block, at fmRate / 8
SCA_BLOCK_FM = 1920           # fm samples per block
SCA_LOOKBACK = 703            # fm samples a block reads in front of its first
SCA_RING = 128                # blocks the library keeps per decoding channel


class FmxFeedInfo(C.Structure):
    _fields_ = [("rate_hz", C.c_int32), ("block_samples", C.c_int32), ("block_frames", C.c_int32), ("lookback_frames", C.c_int32), ("delay_frames", C.c_double),
                ("ring_blocks", C.c_int32), ("bytes_per_channel", C.c_int32)]


FEED_F32, FEED_S16 = 0, 1     # fmx_feed_format
FEED_OFF, FEED_MIX, FEED_LEFT, FEED_RIGHT = 0, 1, 2, 3
FEED_BLOCK = 160              # feed samples per block, at 16 kS/s
FEED_BLOCK_FRAMES = 480       # PCM frames per block
FEED_LOOKBACK = 143           # PCM frames a block reads in front of its first
FEED_RING = 128               # blocks the library keeps per feeding channel


class FmxMeta(C.Structure):
    _fields_ = [
        ("DcValRf", C.c_float), ("DcValIf", C.c_float), ("PssPhaseShiftDegree", C.c_float),
        ("PssPhaseChange", C.c_float), ("PssState", C.c_int32), ("PilotPllLockStrength", C.c_float),
        ("PilotPllLocked", C.c_int32), ("fm_samples", C.c_int64), ("pcm_frames", C.c_int64),
        ("live_pilot_locked", C.c_int32), ("live_lock_strength", C.c_float), ("live_dc_if", C.c_float),
        ("squelch_active", C.c_int32), ("live_rf_dc_re", C.c_float), ("live_rf_dc_im", C.c_float),
    ]


class FmxRdsInfo(C.Structure):
    _fields_ = [("synchronized", C.c_int32), ("pi_code", C.c_int32), ("pty_code", C.c_int32), ("last_group_type", C.c_int32),
                ("groups_decoded", C.c_int32), ("crc_errors", C.c_int32), ("sync_errors", C.c_int32), ("bit_error_rate", C.c_float),
                ("station_label", C.c_char * 9), ("radio_text", C.c_char * 65), ("af1_khz", C.c_int32), ("af2_khz", C.c_int32),
                ("music_speech", C.c_int32), ("di_code", C.c_int32),
                ("radio_text_ucs2", C.c_uint16 * 65), ("radio_text_ucs2_len", C.c_int16)]

    @property
    def radio_text_unicode(self):
        """The radio text as the reference's setRadioText receives it (prepareText + mapEBUtoUnicode, trimmed)."""
        return "".join(chr(v) for v in self.radio_text_ucs2[:self.radio_text_ucs2_len])


class FmxScanResult(C.Structure):
    _fields_ = [("block", C.c_int64), ("end_sample", C.c_int64), ("signal_db", C.c_float), ("noise_db", C.c_float),
                ("found", C.c_int32), ("reserved", C.c_int32)]


# fmx_scan_result as a numpy record (Fmx.scan_results)
SCAN_DTYPE = np.dtype([("block", np.int64), ("end_sample", np.int64), ("signal_db", np.float32), ("noise_db", np.float32),
                       ("found", np.int32), ("reserved", np.int32)])
assert SCAN_DTYPE.itemsize == C.sizeof(FmxScanResult)


class FmxModRecord(C.Structure):
    _fields_ = [("index", C.c_int64), ("end_sample", C.c_int64), ("peak_pos", C.c_float), ("peak_neg", C.c_float), ("mean", C.c_float),
                ("mean_square", C.c_float), ("pilot_i", C.c_float), ("pilot_q", C.c_float)]


# fmx_mod_record as a numpy record (Fmx.mod_records)
MOD_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("peak_pos", np.float32), ("peak_neg", np.float32), ("mean", np.float32),
                      ("mean_square", np.float32), ("pilot_i", np.float32), ("pilot_q", np.float32)])
assert MOD_DTYPE.itemsize == C.sizeof(FmxModRecord)
MOD_WINDOW = 9600             # fm samples per record: 50 ms


class FmxAudioRecord(C.Structure):
    _fields_ = [("index", C.c_int64), ("end_frame", C.c_int64), ("peak_l", C.c_float), ("peak_r", C.c_float), ("ms_l", C.c_float), ("ms_r", C.c_float),
                ("kms_l", C.c_float), ("kms_r", C.c_float), ("cross", C.c_float), ("reserved", C.c_int32)]


# fmx_audio_record as a numpy record (Fmx.audio_records)
AUDIO_DTYPE = np.dtype([("index", np.int64), ("end_frame", np.int64), ("peak_l", np.float32), ("peak_r", np.float32), ("ms_l", np.float32),
                        ("ms_r", np.float32), ("kms_l", np.float32), ("kms_r", np.float32), ("cross", np.float32), ("reserved", np.int32)])
assert AUDIO_DTYPE.itemsize == C.sizeof(FmxAudioRecord) == 48
AUDIO_WINDOW = 4800           # PCM frames per record: 100 ms


class FmxLoudness(C.Structure):
    _fields_ = [("momentary_lufs", C.c_double), ("short_term_lufs", C.c_double), ("integrated_lufs", C.c_double), ("correlation", C.c_double),
                ("peak_dbfs_l", C.c_double), ("peak_dbfs_r", C.c_double), ("blocks_total", C.c_int64), ("blocks_gated", C.c_int64)]


class FmxRxRecord(C.Structure):
    _fields_ = [("index", C.c_int64), ("end_sample", C.c_int64), ("p_max", C.c_float), ("p_min", C.c_float), ("p_mean", C.c_float),
                ("p2_mean", C.c_float), ("r1_re", C.c_float), ("r1_im", C.c_float)]


# fmx_rx_record as a numpy record (Fmx.rx_records)
RX_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("p_max", np.float32), ("p_min", np.float32), ("p_mean", np.float32),
                     ("p2_mean", np.float32), ("r1_re", np.float32), ("r1_im", np.float32)])
assert RX_DTYPE.itemsize == C.sizeof(FmxRxRecord) == 40
RxRecord = FmxRxRecord
RX_WINDOW = 9600              # fm samples per record: 50 ms, the modulation meter's grid


class FmxRxQuality(C.Structure):
    _fields_ = [("level_dbfs", C.c_double), ("cnr_db", C.c_double), ("am_depth", C.c_double), ("offset_hz", C.c_double), ("windows", C.c_int64)]


class FmxRdsMeterRecord(C.Structure):
    _fields_ = [("index", C.c_int64), ("end_sample", C.c_int64), ("p_max", C.c_float), ("ii_mean", C.c_float), ("qq_mean", C.c_float),
                ("iq_mean", C.c_float), ("i_mean", C.c_float), ("q_mean", C.c_float)]


# fmx_rds_meter_record as a numpy record (Fmx.rds_meter_records)
RDSM_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("p_max", np.float32), ("ii_mean", np.float32), ("qq_mean", np.float32),
                       ("iq_mean", np.float32), ("i_mean", np.float32), ("q_mean", np.float32)])
assert RDSM_DTYPE.itemsize == C.sizeof(FmxRdsMeterRecord) == 40
RDSM_WINDOW = 2560            # RDS samples (24 kS/s, the channel's own count) per record: 106.7 ms


class FmxRdsMeterCal(C.Structure):
    _fields_ = [("gain", C.c_double), ("phase0_deg", C.c_double), ("path_57k", C.c_double)]


class FmxRdsFigures(C.Structure):
    _fields_ = [("injection_rms_hz", C.c_double), ("injection_peak_hz", C.c_double), ("carrier_hz", C.c_double), ("phase_deg", C.c_double),
                ("axis_db", C.c_double), ("windows", C.c_int64)]


class FmxRdsGroup(C.Structure):
    _fields_ = [("index", C.c_int64), ("end_bit", C.c_int64), ("block", C.c_uint16 * 4)]


# the fields of fmx_debug_rds_state, in its order (include/fmx_debug.h)
RDS_STATE_FIELDS = ("mode", "nbits", "rds2_gain", "rds2_freq", "rds2_phase", "rds2_mu", "rds2_skip", "rds2_sample_count",
                    "rds1_freq", "rds1_phase", "rds1_last_sync", "rds3_freq", "rds3_phase", "rds3_bit_clk_phase", "rds3_sync_err", "rds3_synced")

# fmx_rds_group as a numpy record (Fmx.rds_groups)
RDS_GROUP_DTYPE = np.dtype({"names": ["index", "end_bit", "block"], "formats": [np.int64, np.int64, (np.uint16, 4)], "offsets": [0, 8, 16],
                            "itemsize": C.sizeof(FmxRdsGroup)})


class FmxProfile(C.Structure):
    _fields_ = [("launches", C.c_int64 * 4), ("ms", C.c_double * 4), ("input_samples", C.c_int64),
                ("channel_samples", C.c_int64)]


_lib = None


def load_library(path=None):
    """Load libfmx.so and declare every symbol of include/fmx.h.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FmxError(FMX_E_NO_DEVICE, "%s not built (run `python sdr-j-fm_amd/build.py`); there is no CPU fallback" % p)
    L = C.CDLL(p)
    vp, i32, i64, f32p = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_float)
    L.fmx_abi_version.restype = C.c_int
    L.fmx_abi_version.argtypes = []
    if L.fmx_abi_version() != ABI_VERSION:     # the output structs (FmxMeta, FmxRdsInfo) carry no size field: refuse a library of another layout
        raise FmxError(FMX_E_INVALID, "%s has ABI version %d, this binding was written for %d" % (p, L.fmx_abi_version(), ABI_VERSION))
    L.fmx_last_error.restype = C.c_char_p
    L.fmx_last_error.argtypes = []
    L.fmx_create.restype = C.c_int
    L.fmx_create.argtypes = [C.POINTER(FmxConfig), C.POINTER(vp)]
    L.fmx_destroy.restype = C.c_int
    L.fmx_destroy.argtypes = [vp]
    L.fmx_set_param.restype = C.c_int
    L.fmx_set_param.argtypes = [vp, i32, i32, C.c_double]
    L.fmx_frames_for.restype = i64
    L.fmx_frames_for.argtypes = [vp, i64]
    L.fmx_process_host.restype = C.c_int
    L.fmx_process_host.argtypes = [vp, f32p, i64, i64, f32p, i64, C.POINTER(i64)]
    L.fmx_process_device.restype = C.c_int
    L.fmx_process_device.argtypes = [vp, vp, i64, i64, vp, i64, C.POINTER(i64), vp]
    L.fmx_process_host_raw.restype = C.c_int
    L.fmx_process_host_raw.argtypes = [vp, vp, i32, C.c_float, i64, i64, f32p, i64, C.POINTER(i64)]
    L.fmx_process_device_raw.restype = C.c_int
    L.fmx_process_device_raw.argtypes = [vp, vp, i32, C.c_float, i64, i64, vp, i64, C.POINTER(i64), vp]
    L.fmx_synchronize.restype = C.c_int
    L.fmx_synchronize.argtypes = [vp]
    L.fmx_get_meta.restype = C.c_int
    L.fmx_get_meta.argtypes = [vp, i32, C.POINTER(FmxMeta)]
    L.fmx_get_tap.restype = C.c_int
    L.fmx_get_tap.argtypes = [vp, i32, i32, f32p, i64]
    L.fmx_get_peaks.restype = C.c_int
    L.fmx_get_peaks.argtypes = [vp, i32, f32p, i32, C.POINTER(i32)]
    L.fmx_rds_decode.restype = C.c_int
    L.fmx_rds_decode.argtypes = [vp, i32, C.POINTER(FmxRdsInfo)]
    L.fmx_rds_decode_all.restype = C.c_int
    L.fmx_rds_decode_all.argtypes = [vp, i32, i32, C.POINTER(FmxRdsInfo)]
    L.fmx_rds_groups.restype = C.c_int
    L.fmx_rds_groups.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.fmx_rds_decode_bits.restype = C.c_int
    L.fmx_rds_decode_bits.argtypes = [C.POINTER(C.c_uint8), i32, C.POINTER(FmxRdsInfo)]
    L.fmx_rds_pty_name.restype = C.c_char_p
    L.fmx_rds_pty_name.argtypes = [i32, i32]
    L.fmx_rds_map_char.restype = C.c_uint16
    L.fmx_rds_map_char.argtypes = [C.c_uint8, C.c_uint8]
    L.fmx_rds_prepare_text.restype = i32
    L.fmx_rds_prepare_text.argtypes = [C.POINTER(C.c_uint8), i32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), i32]
    L.fmx_scan_results.restype = C.c_int
    L.fmx_scan_results.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.fmx_mod_meter_enable.restype = C.c_int
    L.fmx_mod_meter_enable.argtypes = [vp, i32, i32]
    L.fmx_mod_records.restype = C.c_int
    L.fmx_mod_records.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.fmx_audio_meter_enable.restype = C.c_int
    L.fmx_audio_meter_enable.argtypes = [vp, i32, i32]
    L.fmx_audio_records.restype = C.c_int
    L.fmx_audio_records.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.fmx_audio_loudness.restype = C.c_int
    L.fmx_audio_loudness.argtypes = [vp, i32, C.POINTER(FmxLoudness)]
    L.fmx_rx_meter_enable.restype = C.c_int
    L.fmx_rx_meter_enable.argtypes = [vp, i32, i32]
    L.fmx_rx_records.restype = C.c_int
    L.fmx_rx_records.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.fmx_rx_quality_of.restype = C.c_int
    L.fmx_rx_quality_of.argtypes = [vp, i32, i32, C.POINTER(FmxRxQuality)]
    L.fmx_rds_meter_enable.restype = C.c_int
    L.fmx_rds_meter_enable.argtypes = [vp, i32, i32]
    L.fmx_rds_meter_records.restype = C.c_int
    L.fmx_rds_meter_records.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.fmx_rds_meter_cal.restype = C.c_int
    L.fmx_rds_meter_cal.argtypes = [vp, i32, C.POINTER(FmxRdsMeterCal)]
    L.fmx_rds_meter_figures.restype = C.c_int
    L.fmx_rds_meter_figures.argtypes = [vp, i32, C.POINTER(FmxRdsMeterCal), C.c_double, C.POINTER(FmxRdsFigures)]
    L.fmx_spectrum_setup.restype = C.c_int
    L.fmx_spectrum_setup.argtypes = [vp, i32, i32]
    L.fmx_spectrum_enable.restype = C.c_int
    L.fmx_spectrum_enable.argtypes = [vp, i32, i32]
    L.fmx_spectrum_read.restype = C.c_int
    L.fmx_spectrum_read.argtypes = [vp, i32, vp, vp, vp, i32, C.POINTER(i32)]
    L.fmx_spectrum_figures.restype = C.c_int
    L.fmx_spectrum_figures.argtypes = [C.POINTER(FmxSpectrumFind), vp, vp, C.POINTER(FmxSpectrumFigs)]
    L.fmx_mpx_spectrum_setup.restype = C.c_int
    L.fmx_mpx_spectrum_setup.argtypes = [vp, i32, i32]
    L.fmx_mpx_spectrum_enable.restype = C.c_int
    L.fmx_mpx_spectrum_enable.argtypes = [vp, i32, i32]
    L.fmx_mpx_spectrum_read.restype = C.c_int
    L.fmx_mpx_spectrum_read.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp]
    L.fmx_mpx_figures.restype = C.c_int
    L.fmx_mpx_figures.argtypes = [C.POINTER(FmxMpxFind), vp, vp, C.POINTER(FmxMpxFigs)]
    L.fmx_sca_setup.restype = C.c_int
    L.fmx_sca_setup.argtypes = [vp, C.POINTER(FmxScaConfig)]
    L.fmx_sca_enable.restype = C.c_int
    L.fmx_sca_enable.argtypes = [vp, i32, i32]
    L.fmx_sca_read.restype = C.c_int
    L.fmx_sca_read.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp]
    L.fmx_sca_taps.restype = C.c_int
    L.fmx_sca_taps.argtypes = [C.POINTER(FmxScaConfig), i32, i32, vp, i32, C.POINTER(i32)]
    L.fmx_sca_info.restype = C.c_int
    L.fmx_sca_info.argtypes = [i32, C.POINTER(FmxScaInfo)]
    L.fmx_feed_enable.restype = C.c_int
    L.fmx_feed_enable.argtypes = [vp, i32, i32]
    L.fmx_feed_read.restype = C.c_int
    L.fmx_feed_read.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp]
    L.fmx_feed_read_device.restype = C.c_int
    L.fmx_feed_read_device.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, vp, vp]
    L.fmx_feed_taps.restype = C.c_int
    L.fmx_feed_taps.argtypes = [vp, i32, C.POINTER(i32)]
    L.fmx_feed_info.restype = C.c_int
    L.fmx_feed_info.argtypes = [C.POINTER(FmxFeedInfo)]
    L.fmx_feed_allocated.restype = C.c_int64
    L.fmx_feed_allocated.argtypes = [vp]
    L.fmx_mod_hz_per_unit.restype = C.c_int
    L.fmx_mod_hz_per_unit.argtypes = [i32, i32, C.POINTER(C.c_double)]
    L.fmx_rds_bits.restype = C.c_int
    L.fmx_rds_bits.argtypes = [vp, i32, C.POINTER(C.c_uint8), i32, C.POINTER(i32)]
    L.fmx_rds_symbols.restype = C.c_int
    L.fmx_rds_symbols.argtypes = [vp, i32, f32p, i32, C.POINTER(i32)]
    L.fmx_last_fm_samples.restype = C.c_int64
    L.fmx_last_fm_samples.argtypes = [vp]
    L.fmx_pll_replays.restype = C.c_int64
    L.fmx_pll_replays.argtypes = [vp, C.c_int32]
    L.fmx_pll_exact_segments.restype = C.c_int64
    L.fmx_filter_change_due.restype = C.c_int64
    L.fmx_filter_change_due.argtypes = [vp]
    L.fmx_last_front_kernel.restype = C.c_int32
    L.fmx_last_front_kernel.argtypes = [vp]
    L.fmx_last_call_pieces.restype = C.c_int32
    L.fmx_last_call_pieces.argtypes = [vp]
    L.fmx_last_second_group.restype = C.c_int32
    L.fmx_last_second_group.argtypes = [vp]
    L.fmx_pll_exact_segments.argtypes = [vp, C.c_int32]
    L.fmx_last_rds_samples.restype = C.c_int64
    L.fmx_last_rds_samples.argtypes = [vp]
    L.fmx_last_rds_samples_of.restype = C.c_int64
    L.fmx_last_rds_samples_of.argtypes = [vp, C.c_int32]
    L.fmx_debug_rds_state.restype = C.c_int                 # include/fmx_debug.h: a diagnostic, not one of EXPORTS
    L.fmx_debug_rds_state.argtypes = [vp, i32, f32p, i32, C.POINTER(i32)]
    L.fmx_get_taps.restype = C.c_int
    L.fmx_get_taps.argtypes = [vp, i32, i32, f32p, i32, C.POINTER(i32)]
    L.fmx_profile_enable.restype = C.c_int
    L.fmx_profile_enable.argtypes = [vp, i32]
    L.fmx_profile_read.restype = C.c_int
    L.fmx_profile_read.argtypes = [vp, C.POINTER(FmxProfile), i32]
    L.fmx_wideband_create.restype = C.c_int
    L.fmx_wideband_create.argtypes = [C.POINTER(FmxWidebandConfig), C.POINTER(vp)]
    L.fmx_wideband_destroy.restype = C.c_int
    L.fmx_wideband_destroy.argtypes = [vp]
    L.fmx_wideband_set_offset.restype = C.c_int
    L.fmx_wideband_set_offset.argtypes = [vp, i32, i32]
    L.fmx_wideband_process_device_raw.restype = C.c_int
    L.fmx_wideband_process_device_raw.argtypes = [vp, vp, i32, C.c_float, i64, i64, vp, i64, C.POINTER(i64), vp]
    L.fmx_wideband_process_host_raw.restype = C.c_int
    L.fmx_wideband_process_host_raw.argtypes = [vp, vp, i32, C.c_float, i64, i64, f32p, i64, C.POINTER(i64)]
    L.fmx_wideband_taps.restype = C.c_int
    L.fmx_wideband_taps.argtypes = [i32, f32p, i32, C.POINTER(i32)]
    L.fmx_wideband_survey_enable.restype = C.c_int
    L.fmx_wideband_survey_enable.argtypes = [vp, i32]
    L.fmx_wideband_survey_read.restype = C.c_int
    L.fmx_wideband_survey_read.argtypes = [vp, i32, vp, f32p, i32, C.POINTER(i32)]
    L.fmx_wideband_survey_stations.restype = C.c_int
    L.fmx_wideband_survey_stations.argtypes = [C.POINTER(FmxSurveyFind), f32p, vp, i32, C.POINTER(i32), f32p]
    L.fmx_wideband_create_rate.restype = C.c_int
    L.fmx_wideband_create_rate.argtypes = [C.POINTER(FmxWidebandConfig), i32, C.POINTER(vp)]
    L.fmx_wideband_outputs_for.restype = i64
    L.fmx_wideband_outputs_for.argtypes = [vp, i64]
    L.fmx_wideband_rate_taps.restype = C.c_int
    L.fmx_wideband_rate_taps.argtypes = [i32, f32p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.fmx_wideband_survey_stations_rate.restype = C.c_int
    L.fmx_wideband_survey_stations_rate.argtypes = [C.POINTER(FmxSurveyFind), i32, f32p, vp, i32, C.POINTER(i32), f32p]
    if path is None:
        _lib = L
    return L


def rds_decode_bits(bits):
    """Decode a recorded RDS bit stream from a fresh state (host only); returns FmxRdsInfo."""
    L = load_library()
    b = np.ascontiguousarray(bits, np.uint8)
    info = FmxRdsInfo()
    rc = L.fmx_rds_decode_bits(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size, C.byref(info))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode())
    return info


def mod_hz_per_unit(decoder=3, fmRate=192000):
    """Hz per unit of the demodulator output, and so of the modulation meter's records, for a decoder (include/fmx.h fmx_mod_hz_per_unit; host only,
    needs no device).  Raises FmxError (FMX_E_UNSUPPORTED) for the decoders whose output is no frequency."""
    L = load_library()
    hz = C.c_double()
    rc = L.fmx_mod_hz_per_unit(int(decoder), int(fmRate), C.byref(hz))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return hz.value


def loudness(records):
    """The BS.1770-4 / EBU R 128 figures of one channel's audio-meter records in order (AUDIO_DTYPE; include/fmx.h fmx_audio_loudness; host only, needs no
    device): a dict of momentary_lufs, short_term_lufs, integrated_lufs, correlation, peak_dbfs_l, peak_dbfs_r (float; -inf where there is too little
    or only silence), blocks_total and blocks_gated."""
    L = load_library()
    recs = np.ascontiguousarray(records, AUDIO_DTYPE)
    out = FmxLoudness()
    rc = L.fmx_audio_loudness(recs.ctypes.data if recs.size else None, int(recs.size), C.byref(out))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return {name: getattr(out, name) for name, _ in FmxLoudness._fields_}


def rx_quality(records, fmRate=192000):
    """The reception figures of one channel's reception-meter records (RX_DTYPE; include/fmx.h fmx_rx_quality_of; host only, needs no device): a dict of
    level_dbfs, cnr_db (-inf: no carrier, +inf: no noise), am_depth, offset_hz and windows.  Raises FmxError (FMX_E_INVALID) for no records."""
    L = load_library()
    recs = np.ascontiguousarray(records, RX_DTYPE)
    out = FmxRxQuality()
    rc = L.fmx_rx_quality_of(recs.ctypes.data if recs.size else None, int(recs.size), int(fmRate), C.byref(out))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return {name: getattr(out, name) for name, _ in FmxRxQuality._fields_}


def spectrum_figures(mean, peak=None, rate_hz=2304000, centre_hz=0, raster_hz=100000, dc_guard_hz=0, obw_fraction=0.99, x_db=26.0, rbw_hz=10000,
                     mask=None):
    """The figures of one spectrum-meter record (include/fmx.h fmx_spectrum_figures; host only, needs no device): a dict of channel_db, obw_hz,
    obw_lower_hz, obw_upper_hz, xdb_hz, centroid_hz, adj_db (a list for the offsets -2, -1, +1, +2 rasters), mask_margin_db and mask_worst_hz; frequencies
    relative to centre_hz, -inf for a quantity that cannot be formed.  mask: the caller's break points [(|offset_hz|, limit_db), ...] or None.  Raises
    FmxError (FMX_E_INVALID) for an argument the library refuses."""
    L = load_library()
    mean = np.ascontiguousarray(mean, np.float32)
    assert mean.shape == (SPECTRUM_BINS,)
    if peak is not None:
        peak = np.ascontiguousarray(peak, np.float32)
        assert peak.shape == (SPECTRUM_BINS,)
    pts = None
    if mask is not None:
        pts = (FmxSpectrumMaskPoint * max(len(mask), 1))(*[FmxSpectrumMaskPoint(float(o), float(l)) for o, l in mask])
    cfg = FmxSpectrumFind(C.sizeof(FmxSpectrumFind), int(rate_hz), int(centre_hz), int(raster_hz), int(dc_guard_hz), int(rbw_hz), float(obw_fraction),
                          float(x_db), pts, len(mask) if mask is not None else 0, 0)
    out = FmxSpectrumFigs()
    rc = L.fmx_spectrum_figures(C.byref(cfg), mean.ctypes.data, peak.ctypes.data if peak is not None else None, C.byref(out))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    figs = {name: getattr(out, name) for name, _ in FmxSpectrumFigs._fields_}
    figs["adj_db"] = list(out.adj_db)
    return figs


def mpx_figures(mean, peak=None, rate_hz=192000, hz_per_unit=1.0, dc_guard_hz=30, line_half_hz=250, bands=None):
    """The figures of one multiplex-spectrum record (include/fmx.h fmx_mpx_figures; host only, needs no device): a dict of total_hz, mono_hz, stereo_hz,
    rds_hz, aux_hz, pilot_hz, pilot_freq_hz, carrier38_hz, floor_hz_rt_hz, pilot_cn0_db and, one entry per caller band [(lo_hz, hi_hz), ...], the lists
    band_hz, band_line_hz, band_hold_line_hz and band_hold_over_mean_db; -inf for a quantity that cannot be formed.  hz_per_unit: Fmx.mod_hz_per_unit's,
    or 1.0 for the demodulator's own units.  Raises FmxError (FMX_E_INVALID) for an argument the library refuses."""
    L = load_library()
    mean = np.ascontiguousarray(mean, np.float32)
    assert mean.shape == (MPX_BINS,)
    if peak is not None:
        peak = np.ascontiguousarray(peak, np.float32)
        assert peak.shape == (MPX_BINS,)
    nb = len(bands) if bands is not None else 0
    arr = (FmxMpxBand * max(nb, 1))(*[FmxMpxBand(float(lo), float(hi)) for lo, hi in (bands or [])]) if bands is not None else None
    cfg = FmxMpxFind(C.sizeof(FmxMpxFind), int(rate_hz), float(hz_per_unit), int(dc_guard_hz), int(line_half_hz), arr, nb, 0)
    out = FmxMpxFigs()
    rc = L.fmx_mpx_figures(C.byref(cfg), mean.ctypes.data, peak.ctypes.data if peak is not None else None, C.byref(out))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    figs = {name: getattr(out, name) for name, _ in FmxMpxFigs._fields_[:10]}
    for name, _ in FmxMpxFigs._fields_[10:]:
        figs[name] = list(getattr(out, name))[:min(nb, 16)]
    return figs


def _sca_config(half_band_hz=9000, audio_cut_hz=5000, deviation_hz=6000, deemphasis_us=150):
    return FmxScaConfig(C.sizeof(FmxScaConfig), int(half_band_hz), int(audio_cut_hz), int(deviation_hz), int(deemphasis_us))


def sca_taps(which, rate_hz=192000, **setup):
    """The taps a handle with that setup (half_band_hz, audio_cut_hz, deviation_hz, deemphasis_us) runs its sub-carrier decoder with (fmx_sca_taps;
    host only, needs no device): which 0 or "g" -> the 192-tap band filter at fmRate, 1 or "a" -> the 128-tap audio filter at fmRate / 4."""
    L = load_library()
    which = {"g": 0, "a": 1}.get(which, which)
    cfg = _sca_config(**setup)
    out = np.zeros(192, np.float32)
    n = C.c_int32()
    rc = L.fmx_sca_taps(C.byref(cfg), int(rate_hz), int(which), out.ctypes.data, out.size, C.byref(n))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return out[:n.value].copy()


def sca_info(rate_hz=192000):
    """The sub-carrier decoder's numbers at fmRate (fmx_sca_info; host only): a dict of audio_rate_hz, block_audio, block_fm, lookback_fm, delay_fm,
    ring_blocks and bytes_per_channel."""
    L = load_library()
    out = FmxScaInfo()
    rc = L.fmx_sca_info(int(rate_hz), C.byref(out))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return {name: getattr(out, name) for name, _ in FmxScaInfo._fields_}


def feed_taps():
    """The monitoring feed's 144 taps at 48 000 frames/s (fmx_feed_taps; host only, needs no device)."""
    L = load_library()
    out = np.zeros(144, np.float32)
    n = C.c_int32()
    rc = L.fmx_feed_taps(out.ctypes.data, out.size, C.byref(n))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return out[:n.value].copy()


def feed_info():
    """The monitoring feed's numbers (fmx_feed_info; host only): a dict of rate_hz, block_samples, block_frames, lookback_frames, delay_frames, ring_blocks
    and bytes_per_channel."""
    L = load_library()
    out = FmxFeedInfo()
    rc = L.fmx_feed_info(C.byref(out))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return {name: getattr(out, name) for name, _ in FmxFeedInfo._fields_}


def _device_ptr(x):
    """an address, or whatever has a data_ptr () (a torch tensor on the device), or None"""
    if x is None:
        return None
    return C.c_void_p(int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x))


def rds_meter_figures(records, cal, hz_per_unit):
    """The figures of one channel's RDS-meter records (RDSM_DTYPE; include/fmx.h fmx_rds_meter_figures; host only, needs no device): a dict of
    injection_rms_hz, injection_peak_hz, carrier_hz, phase_deg, axis_db and windows.  `cal` is what Fmx.rds_meter_cal returned (a dict of gain,
    phase0_deg, path_57k), hz_per_unit what mod_hz_per_unit returned.  Raises FmxError (FMX_E_INVALID) for no records."""
    L = load_library()
    recs = np.ascontiguousarray(records, RDSM_DTYPE)
    k = FmxRdsMeterCal(float(cal["gain"]), float(cal["phase0_deg"]), float(cal["path_57k"]))
    out = FmxRdsFigures()
    rc = L.fmx_rds_meter_figures(recs.ctypes.data if recs.size else None, int(recs.size), C.byref(k), float(hz_per_unit), C.byref(out))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return {name: getattr(out, name) for name, _ in FmxRdsFigures._fields_}


class Fmx:
    """Thin object wrapper over an fmx_handle (a batch of FM channels on one GPU)."""

    def __init__(self, channels=1, streams=0, stream_of_channel=None, device=0, max_block=16384,
                 inputRate=2304000, fmRate=192000, workingRate=48000, audioRate=48000):
        self.L = load_library()
        cfg = FmxConfig()
        cfg.struct_size = C.sizeof(FmxConfig)
        cfg.device, cfg.channels, cfg.streams = device, channels, streams
        self._map = None
        if stream_of_channel is not None:
            self._map = (C.c_int32 * channels)(*[int(x) for x in stream_of_channel])
            cfg.stream_of_channel = C.cast(self._map, C.POINTER(C.c_int32))
        cfg.inputRate, cfg.fmRate, cfg.workingRate, cfg.audioRate = inputRate, fmRate, workingRate, audioRate
        cfg.max_block = max_block
        self.channels = channels
        self.streams = streams if streams > 0 else channels
        self.max_block = max_block
        self.h = C.c_void_p()
        self._check(self.L.fmx_create(C.byref(cfg), C.byref(self.h)))

    def _check(self, rc):
        if rc != FMX_OK:
            raise FmxError(rc, self.L.fmx_last_error().decode("utf-8", "replace"))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.fmx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_param(self, pid, value, channel=-1):
        self._check(self.L.fmx_set_param(self.h, channel, pid, float(value)))

    def frames_for(self, n):
        return int(self.L.fmx_frames_for(self.h, n))

    def process_host(self, iq):
        """iq: float32 [streams, n, 2] (or [n, 2] for one stream) -> pcm float32 [channels, frames, 2]."""
        iq = np.ascontiguousarray(iq, np.float32)
        if iq.ndim == 2:
            iq = iq[None]
        assert iq.shape[0] == self.streams and iq.shape[2] == 2
        n = iq.shape[1]
        frames = self.frames_for(n)
        cap = max(frames, 1)
        pcm = np.zeros((self.channels, cap, 2), np.float32)
        got = C.c_int64()
        self._check(self.L.fmx_process_host(self.h, iq.ctypes.data_as(C.POINTER(C.c_float)), n, n,
                                            pcm.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(got)))
        return pcm[:, :got.value]

    def process_host_raw(self, iq, fmt, s16_denominator=2048.0):
        """Raw device samples: iq uint8 / int8 / int16 [streams, n, 2] (or [n, 2]), fmt = IQ_U8 / IQ_S8 /
        IQ_S16; converted on the GPU exactly as the reference's device handlers do on the host."""
        dt = {IQ_U8: np.uint8, IQ_S8: np.int8, IQ_S16: np.int16, IQ_F32: np.float32}[fmt]
        iq = np.ascontiguousarray(iq, dt)
        if iq.ndim == 2:
            iq = iq[None]
        assert iq.shape[0] == self.streams and iq.shape[2] == 2
        n = iq.shape[1]
        cap = max(self.frames_for(n), 1)
        pcm = np.zeros((self.channels, cap, 2), np.float32)
        got = C.c_int64()
        self._check(self.L.fmx_process_host_raw(self.h, iq.ctypes.data_as(C.c_void_p), fmt, float(s16_denominator), n, n,
                                                pcm.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(got)))
        return pcm[:, :got.value]

    def process_device(self, d_iq_ptr, stream_stride, n, d_pcm_ptr, pcm_stride, hip_stream=None):
        got = C.c_int64()
        self._check(self.L.fmx_process_device(self.h, C.c_void_p(d_iq_ptr), stream_stride, n, C.c_void_p(d_pcm_ptr),
                                              pcm_stride, C.byref(got), C.c_void_p(hip_stream or 0)))
        return got.value

    def synchronize(self):
        self._check(self.L.fmx_synchronize(self.h))

    def meta(self, channel=0):
        m = FmxMeta()
        self._check(self.L.fmx_get_meta(self.h, channel, C.byref(m)))
        return m

    def tap(self, tap_id, n, channel=0):
        width = 1 if tap_id in (TAP_DEMOD, TAP_PILOT_PHASE) else 2
        out = np.zeros((n, width), np.float32)
        self._check(self.L.fmx_get_tap(self.h, channel, tap_id, out.ctypes.data_as(C.POINTER(C.c_float)), n))
        return out[:, 0] if width == 1 else out

    def peaks(self, channel=0, capacity=256):
        """showPeakLevel events since the last fetch as [events, 2] (leftDb, rightDb)."""
        out = np.zeros((max(capacity, 1), 2), np.float32)
        n = C.c_int32()
        self._check(self.L.fmx_get_peaks(self.h, channel, out.ctypes.data_as(C.POINTER(C.c_float)), capacity, C.byref(n)))
        return out[:n.value].copy()

    def scan_results(self, channel=0, capacity=1024):
        """Scan-mode records completed since the last read, oldest first, as a numpy structured array (SCAN_DTYPE:
        block, end_sample, signal_db, noise_db, found)."""
        out = np.zeros(max(capacity, 1), SCAN_DTYPE)
        n = C.c_int32()
        self._check(self.L.fmx_scan_results(self.h, channel, out.ctypes.data, capacity, C.byref(n)))
        return out[:n.value].copy()

    def mod_meter(self, on=True, channel=-1):
        """Switch the modulation meter of a channel (-1: of every channel) on or off, from the next call on (fmx_mod_meter_enable)."""
        self._check(self.L.fmx_mod_meter_enable(self.h, int(channel), 1 if on else 0))

    def mod_records(self, first=0, count=None, capacity=64):
        """The modulation meter's records since the last read, per channel of the range, oldest first (fmx_mod_records): a list of numpy structured
        arrays (MOD_DTYPE: index, end_sample, peak_pos, peak_neg, mean, mean_square, pilot_i, pilot_q), one per 50 ms window, in the demodulator's
        units (mod_hz_per_unit).  The library keeps the last 64 per channel."""
        count = self.channels - first if count is None else count
        out = np.zeros((max(count, 1), max(capacity, 1)), MOD_DTYPE)
        n = (C.c_int32 * max(count, 1))()
        self._check(self.L.fmx_mod_records(self.h, first, count, out.ctypes.data, capacity, n))
        return [out[k, :n[k]].copy() for k in range(count)]

    def audio_meter(self, on=True, channel=-1):
        """Switch the programme audio meter of a channel (-1: of every channel) on or off, from the next call on (fmx_audio_meter_enable)."""
        self._check(self.L.fmx_audio_meter_enable(self.h, int(channel), 1 if on else 0))

    def audio_records(self, first=0, count=None, capacity=64):
        """The audio meter's records since the last read, per channel of the range, oldest first (fmx_audio_records): a list of numpy structured arrays
        (AUDIO_DTYPE: index, end_frame, peak_l, peak_r, ms_l, ms_r, kms_l, kms_r, cross), one per 100 ms window of the delivered PCM; loudness () turns
        a channel's records into LUFS.  The library keeps the last 64 per channel."""
        count = self.channels - first if count is None else count
        out = np.zeros((max(count, 1), max(capacity, 1)), AUDIO_DTYPE)
        n = (C.c_int32 * max(count, 1))()
        self._check(self.L.fmx_audio_records(self.h, first, count, out.ctypes.data, capacity, n))
        return [out[k, :n[k]].copy() for k in range(count)]

    def rx_meter(self, on=True, channel=-1):
        """Switch the reception meter of a channel (-1: of every channel) on or off, from the next call on (fmx_rx_meter_enable)."""
        self._check(self.L.fmx_rx_meter_enable(self.h, int(channel), 1 if on else 0))

    rx_meter_enable = rx_meter

    def rx_records(self, first=0, count=None, capacity=64):
        """The reception meter's records since the last read, per channel of the range, oldest first (fmx_rx_records): a list of numpy structured arrays
        (RX_DTYPE: index, end_sample, p_max, p_min, p_mean, p2_mean, r1_re, r1_im), one per 50 ms window of the channel's fm-rate samples; rx_quality ()
        turns a channel's records into level, C/N, envelope depth and offset.  The library keeps the last 64 per channel."""
        count = self.channels - first if count is None else count
        out = np.zeros((max(count, 1), max(capacity, 1)), RX_DTYPE)
        n = (C.c_int32 * max(count, 1))()
        self._check(self.L.fmx_rx_records(self.h, first, count, out.ctypes.data, capacity, n))
        return [out[k, :n[k]].copy() for k in range(count)]

    def rds_meter_enable(self, on=True, channel=-1):
        """Switch the RDS meter of a channel (-1: of every channel) on or off, from the next call on (fmx_rds_meter_enable).  Switches no decoder."""
        self._check(self.L.fmx_rds_meter_enable(self.h, int(channel), 1 if on else 0))

    def rds_meter_records(self, first=0, count=None, capacity=64):
        """The RDS meter's records since the last read, per channel of the range, oldest first (fmx_rds_meter_records): a list of numpy structured arrays
        (RDSM_DTYPE: index, end_sample, p_max, ii_mean, qq_mean, iq_mean, i_mean, q_mean), one per window of 2560 of the channel's own 24 kS/s samples;
        rds_meter_figures () turns a channel's records into injection, phase and axis ratio.  The library keeps the last 64 per channel."""
        count = self.channels - first if count is None else count
        out = np.zeros((max(count, 1), max(capacity, 1)), RDSM_DTYPE)
        n = (C.c_int32 * max(count, 1))()
        self._check(self.L.fmx_rds_meter_records(self.h, first, count, out.ctypes.data, capacity, n))
        return [out[k, :n[k]].copy() for k in range(count)]

    def spectrum_setup(self, blocks_per_record=16, every=1):
        """The spectrum meter's grid, handle-wide (fmx_spectrum_setup): blocks of 4096 input samples per record and `every` (block b begins at input
        sample 4096 * every * b).  Only while no stream's meter is on."""
        self._check(self.L.fmx_spectrum_setup(self.h, int(blocks_per_record), int(every)))

    def spectrum_meter(self, on=True, stream=-1):
        """Switch the spectrum meter of a stream (-1: of every stream) on or off, from the next call on (fmx_spectrum_enable)."""
        self._check(self.L.fmx_spectrum_enable(self.h, int(stream), 1 if on else 0))

    spectrum_enable = spectrum_meter

    def spectrum_read(self, stream=0, capacity=SPECTRUM_RING, peak=True):
        """The records of `stream` completed since its last read, oldest first (fmx_spectrum_read) -> (records as SPECTRUM_RECORD_DTYPE, mean [n, 4096]
        f32, peak [n, 4096] f32 or None); spectrum_figures () turns one record into bandwidth, adjacent-channel and mask figures.  The library keeps the
        last 4 per metered stream."""
        recs = np.zeros(max(capacity, 1), SPECTRUM_RECORD_DTYPE)
        mean = np.zeros((max(capacity, 1), SPECTRUM_BINS), np.float32)
        pk = np.zeros((max(capacity, 1), SPECTRUM_BINS), np.float32) if peak else None
        n = C.c_int32()
        self._check(self.L.fmx_spectrum_read(self.h, int(stream), recs.ctypes.data, mean.ctypes.data, pk.ctypes.data if peak else None, int(capacity), C.byref(n)))
        return recs[:n.value].copy(), mean[:n.value].copy(), (pk[:n.value].copy() if peak else None)

    def mpx_spectrum_setup(self, blocks_per_record=48, every=1):
        """The multiplex spectrum meter's grid, handle-wide (fmx_mpx_spectrum_setup): blocks of 4096 fm samples per record and `every` (block b begins at
        fm sample 4096 * every * b).  Only while no channel's meter is on."""
        self._check(self.L.fmx_mpx_spectrum_setup(self.h, int(blocks_per_record), int(every)))

    def mpx_spectrum_meter(self, on=True, channel=-1):
        """Switch the multiplex spectrum meter of a channel (-1: of every channel) on or off, from the next call on (fmx_mpx_spectrum_enable)."""
        self._check(self.L.fmx_mpx_spectrum_enable(self.h, int(channel), 1 if on else 0))

    mpx_spectrum_enable = mpx_spectrum_meter

    def mpx_spectrum_read(self, first=0, count=1, capacity=MPX_RING, peak=True):
        """The records of channels first .. first + count - 1 completed since each one's last read, oldest first, in one read-out of the device
        (fmx_mpx_spectrum_read) -> a list with one (records as MPX_RECORD_DTYPE, mean [n, 2048] f32, peak [n, 2048] f32 or None) per channel;
        mpx_figures () turns one record into deviation, pilot, carrier and floor figures.  The library keeps the last 4 per metered channel."""
        cap = max(int(capacity), 1)
        recs = np.zeros((count, cap), MPX_RECORD_DTYPE)
        mean = np.zeros((count, cap, MPX_BINS), np.float32)
        pk = np.zeros((count, cap, MPX_BINS), np.float32) if peak else None
        n = np.zeros(count, np.int32)
        self._check(self.L.fmx_mpx_spectrum_read(self.h, int(first), int(count), recs.ctypes.data, mean.ctypes.data, pk.ctypes.data if peak else None,
                                                 int(capacity), n.ctypes.data))
        return [(recs[q, :n[q]].copy(), mean[q, :n[q]].copy(), (pk[q, :n[q]].copy() if peak else None)) for q in range(count)]

    def sca_setup(self, half_band_hz=9000, audio_cut_hz=5000, deviation_hz=6000, deemphasis_us=150):
        """The sub-carrier decoder's setup, handle-wide (fmx_sca_setup).  Only while no channel decodes."""
        cfg = _sca_config(half_band_hz, audio_cut_hz, deviation_hz, deemphasis_us)
        self._check(self.L.fmx_sca_setup(self.h, C.byref(cfg)))

    def sca_enable(self, centre_hz=67000, channel=-1):
        """Switch the sub-carrier decoder of a channel (-1: of every channel) on at centre_hz, or off with 0, from the next call on (fmx_sca_enable)."""
        self._check(self.L.fmx_sca_enable(self.h, int(channel), int(centre_hz)))

    def sca_read(self, first=0, count=1, capacity=SCA_RING, level=True):
        """The consecutive blocks of channels first .. first + count - 1 completed since each one's last read, oldest first, in one read-out of the device
        (fmx_sca_read) -> a list with one (first_block or -1, audio [n, 240] f32 at fmRate / 8, level [n] f32 or None) per channel.  A run ends at a
        gap; the rest comes with the next read.  The library keeps the last 128 blocks per decoding channel."""
        cap = max(int(capacity), 1)
        first_block = np.zeros(count, np.int64)
        audio = np.zeros((count, cap, SCA_BLOCK_AUDIO), np.float32)
        lv = np.zeros((count, cap), np.float32) if level else None
        n = np.zeros(count, np.int32)
        self._check(self.L.fmx_sca_read(self.h, int(first), int(count), first_block.ctypes.data, audio.ctypes.data, lv.ctypes.data if level else None,
                                        int(capacity), n.ctypes.data))
        return [(int(first_block[q]), audio[q, :n[q]].copy(), (lv[q, :n[q]].copy() if level else None)) for q in range(count)]

    def feed(self, mode=1, channel=-1):
        """Switch the monitoring feed of a channel (-1: of every channel) from the next call on (fmx_feed_enable): mode 0 off, 1 (L + R) / 2, 2 left,
        3 right.  16 kS/s mono in blocks of 160 samples; block b belongs to the PCM frames [480 b, 480 b + 480)."""
        self._check(self.L.fmx_feed_enable(self.h, int(channel), int(mode)))

    def feed_read(self, first=0, count=1, capacity=FEED_RING, fmt="f32", power=True, device=None):
        """The consecutive blocks of channels first .. first + count - 1 completed since each one's last read, oldest first, in one read-out of the device.
        device None (fmx_feed_read) -> a list with one (first_block or -1, audio [n, 160] f32 or int16, power [n] f32 or None) per channel.
        device = (audio, power or None[, hip_stream]) -- addresses, or torch tensors on the device, of [count, capacity x 160] samples of `fmt` and
        [count, capacity] f32 -- (fmx_feed_read_device): the same gather into those buffers, asynchronous on hip_stream -> a list with one
        (first_block or -1, n) per channel; block i of channel q is at audio [q, 160 i : 160 i + 160].  A run ends at a gap; the rest comes with the next
        read.  The library keeps the last 128 blocks per feeding channel."""
        code = {"f32": FEED_F32, "s16": FEED_S16}.get(fmt, fmt)
        first_block = np.zeros(count, np.int64)
        n = np.zeros(count, np.int32)
        if device is not None:
            d_audio, d_power, stream = (tuple(device) + (None, None))[:3] if isinstance(device, (tuple, list)) else (device, None, None)
            self._check(self.L.fmx_feed_read_device(self.h, int(first), int(count), first_block.ctypes.data, _device_ptr(d_audio), int(code), _device_ptr(d_power),
                                                    int(capacity), n.ctypes.data, _device_ptr(stream)))
            return [(int(first_block[q]), int(n[q])) for q in range(count)]
        cap = max(int(capacity), 1)
        audio = np.zeros((count, cap, FEED_BLOCK), np.int16 if code == FEED_S16 else np.float32)
        pw = np.zeros((count, cap), np.float32) if power else None
        self._check(self.L.fmx_feed_read(self.h, int(first), int(count), first_block.ctypes.data, audio.ctypes.data if capacity > 0 else None, int(code),
                                         pw.ctypes.data if power else None, int(capacity), n.ctypes.data))
        return [(int(first_block[q]), audio[q, :n[q]].copy(), (pw[q, :n[q]].copy() if power else None)) for q in range(count)]

    def feed_allocated(self):
        """the bytes of device memory the handle holds for the feed (fmx_feed_allocated; 0: it never fed)"""
        return int(self.L.fmx_feed_allocated(self.h))

    feed_taps = staticmethod(feed_taps)
    feed_info = staticmethod(feed_info)

    def rds_meter_cal(self, channel=0):
        """The calibration of a channel's RDS meter from the handle's own taps (fmx_rds_meter_cal): a dict of gain, phase0_deg and path_57k."""
        out = FmxRdsMeterCal()
        self._check(self.L.fmx_rds_meter_cal(self.h, int(channel), C.byref(out)))
        return {name: getattr(out, name) for name, _ in FmxRdsMeterCal._fields_}

    def rds_bits(self, channel=0, capacity=8192):
        buf = (C.c_uint8 * capacity)()
        n = C.c_int32()
        self._check(self.L.fmx_rds_bits(self.h, channel, buf, capacity, C.byref(n)))
        return np.frombuffer(buf, np.uint8, n.value).copy()

    def rds_symbols(self, channel=0, capacity=1024):
        """The constellation points the pending bits were decided on, [n, 2]."""
        out = np.zeros((max(capacity, 1), 2), np.float32)
        n = C.c_int32()
        self._check(self.L.fmx_rds_symbols(self.h, channel, out.ctypes.data_as(C.POINTER(C.c_float)), capacity, C.byref(n)))
        return out[:n.value].copy()

    def debug_rds_state(self, channel=0):
        """The scalar state of the channel's RDS slicers behind the last call (fmx_debug_rds_state, include/fmx_debug.h: a diagnostic) as a dict
        of RDS_STATE_FIELDS; empty on a handle whose RDS was never switched on."""
        out = np.zeros(len(RDS_STATE_FIELDS), np.float32)
        n = C.c_int32()
        self._check(self.L.fmx_debug_rds_state(self.h, channel, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n)))
        return dict(zip(RDS_STATE_FIELDS[:n.value], out.tolist()))

    def last_fm_samples(self):
        return int(self.L.fmx_last_fm_samples(self.h))

    def filter_change_due(self):
        """Input samples per stream still to come before a pending mid-stream setBandwidth / setlfcutoff of a batch takes effect (fmx_filter_change_due):
        0 = the next call applies it at its first sample, -1 = nothing pending (setters apply with the next call)."""
        return int(self.L.fmx_filter_change_due(self.h))

    def last_front_kernel(self):
        """Which kernel ran the input-filter stage of the last call (fmx_last_front_kernel: FMX_P_FRONT_KERNEL's numbering)."""
        return int(self.L.fmx_last_front_kernel(self.h))

    def last_call_pieces(self):
        """Overlapping pieces the last call was made in (fmx_last_call_pieces, P_CALL_PIECES; 1: whole)."""
        return int(self.L.fmx_last_call_pieces(self.h))

    def last_second_group(self):
        """Channels of the second of the two groups the last call's stereo / audio stages ran as (fmx_last_second_group; 0: one group)."""
        return int(self.L.fmx_last_second_group(self.h))

    def last_rds_samples(self, channel=0):
        """24 kS/s RDS samples the last call produced on `channel` (fmx_last_rds_samples_of): the n that tap(TAP_RDS_IQ, n, channel) accepts."""
        return int(self.L.fmx_last_rds_samples_of(self.h, channel))

    def pll_replays(self, channel=-1):
        """Segments of the pilot PLL that were replayed sequentially (fmx_pll_replays)."""
        n = int(self.L.fmx_pll_replays(self.h, channel))
        if n < 0:
            self._check(n)
        return n

    def pll_exact_segments(self, channel=-1):
        """Segments FMX_P_PLL_SOLVER = 2 evaluated sequentially because the pilot was not comfortably in lock (fmx_pll_exact_segments)."""
        n = int(self.L.fmx_pll_exact_segments(self.h, channel))
        if n < 0:
            self._check(n)
        return n

    def rds_decode(self, channel=0):
        """Feed the bits sliced so far into the channel's block synchroniser / group decoder; returns FmxRdsInfo."""
        info = FmxRdsInfo()
        self._check(self.L.fmx_rds_decode(self.h, channel, C.byref(info)))
        return info

    def rds_decode_all(self, first=0, count=None):
        """rds_decode for the channels first .. first + count - 1 (default: up to the last) in one read-out of the device (fmx_rds_decode_all):
        a list of FmxRdsInfo.  The block synchroniser has run on the GPU; own decoders, independent of rds_decode."""
        count = self.channels - first if count is None else count
        infos = (FmxRdsInfo * max(count, 1))()
        self._check(self.L.fmx_rds_decode_all(self.h, first, count, infos))
        return [infos[k] for k in range(count)]

    def rds_groups(self, first=0, count=None, capacity=64):
        """The complete RDS groups since the last read, per channel of the range, oldest first (fmx_rds_groups): a list of numpy structured
        arrays (RDS_GROUP_DTYPE: index, end_bit, block[4]).  The library keeps the last 64 per channel."""
        count = self.channels - first if count is None else count
        out = np.zeros((max(count, 1), max(capacity, 1)), RDS_GROUP_DTYPE)
        n = (C.c_int32 * max(count, 1))()
        self._check(self.L.fmx_rds_groups(self.h, first, count, out.ctypes.data, capacity, n))
        return [out[k, :n[k]].copy() for k in range(count)]

    def taps(self, which, channel=0):
        buf = np.zeros(1024, np.float32)
        n = C.c_int32()
        self._check(self.L.fmx_get_taps(self.h, channel, which, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size, C.byref(n)))
        return buf[:n.value].copy()

    def profile_enable(self, on=True):
        self._check(self.L.fmx_profile_enable(self.h, 1 if on else 0))

    def profile_read(self, reset=True):
        p = FmxProfile()
        self._check(self.L.fmx_profile_read(self.h, C.byref(p), 1 if reset else 0))
        return {"launches": list(p.launches), "ms": list(p.ms), "input_samples": p.input_samples,
                "channel_samples": p.channel_samples}


def wideband_taps(factor):
    """The T = 16 K + 1 low-pass taps of stage W for a factor K (host only, needs no device)."""
    L = load_library()
    h = np.zeros(16 * 16 + 1, np.float32)
    n = C.c_int32()
    rc = L.fmx_wideband_taps(int(factor), h.ctypes.data_as(C.POINTER(C.c_float)), h.size, C.byref(n))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode())
    return h[:n.value].copy()


def wideband_rate_taps(rate_hz):
    """The prototype of stage W for a wide rate in Hz (include/fmx.h fmx_wideband_rate_taps; host only, needs no device)
    -> (H [16 M + 1] f32, L, M)."""
    lib = load_library()
    n, L, M = C.c_int32(), C.c_int32(), C.c_int32()
    rc = lib.fmx_wideband_rate_taps(int(rate_hz), None, 0, C.byref(n), C.byref(L), C.byref(M))
    if rc != FMX_E_TOO_LARGE:
        raise FmxError(rc, lib.fmx_last_error().decode("utf-8", "replace"))
    h = np.zeros(n.value, np.float32)
    rc = lib.fmx_wideband_rate_taps(int(rate_hz), h.ctypes.data_as(C.POINTER(C.c_float)), h.size, C.byref(n), C.byref(L), C.byref(M))
    if rc != FMX_OK:
        raise FmxError(rc, lib.fmx_last_error().decode("utf-8", "replace"))
    return h, L.value, M.value


def survey_stations(power, factor=0, raster_hz=100000, origin_hz=0, threshold_db=10.0, dc_guard_hz=0, rate_hz=None):
    """The stations of one survey record (include/fmx.h fmx_wideband_survey_stations; host only, needs no device): power [4096] of a stream
    of `factor`, or of rate_hz S/s (fmx_wideband_survey_stations_rate; factor then stays 0)
    -> (stations as SURVEY_STATION_DTYPE records, ascending in offset_hz, floor_db)."""
    L = load_library()
    power = np.ascontiguousarray(power, np.float32)
    assert power.shape == (SURVEY_BINS,)
    cfg = FmxSurveyFind(C.sizeof(FmxSurveyFind), int(factor), int(raster_hz), int(origin_hz), int(dc_guard_hz), float(threshold_db))
    out = np.zeros(256, SURVEY_STATION_DTYPE)              # (16 * 2 304 000 / 50 000 = 737 candidates, each station beats its neighbours within 200 kHz)
    n, floor_db = C.c_int32(), C.c_float()
    if rate_hz is not None:
        rc = L.fmx_wideband_survey_stations_rate(C.byref(cfg), int(rate_hz), power.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.c_void_p),
                                                 out.size, C.byref(n), C.byref(floor_db))
    else:
        rc = L.fmx_wideband_survey_stations(C.byref(cfg), power.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.c_void_p), out.size,
                                            C.byref(n), C.byref(floor_db))
    if rc != FMX_OK:
        raise FmxError(rc, L.fmx_last_error().decode("utf-8", "replace"))
    return out[:n.value].copy(), floor_db.value


class Wideband:
    """Stage W (include/fmx.h fmx_wideband): `streams` inputs at factor * 2 304 000 S/s -> one 2 304 000 S/s complex stream per station, in the
    layout Fmx.process_device takes."""
    NARROW_RATE = 2304000

    def __init__(self, factor=0, stream_of_output=(0,), offset_hz=(0,), streams=1, max_block=None, device=0, rate_hz=None):
        """factor 2 .. 16, or rate_hz: a rate object (fmx_wideband_create_rate) for a receiver whose rate is no multiple of 2 304 000."""
        self.L = load_library()
        self.rate_hz = int(rate_hz) if rate_hz is not None else None
        self.factor, self.streams, self.outputs = (0 if rate_hz is not None else int(factor)), int(streams), len(stream_of_output)
        self.max_block = int(max_block) if max_block is not None else 16384 * (self.factor or 16)
        assert len(offset_hz) == self.outputs
        cfg = FmxWidebandConfig()
        cfg.struct_size = C.sizeof(FmxWidebandConfig)
        cfg.device, cfg.streams, cfg.factor, cfg.outputs, cfg.max_block = device, self.streams, self.factor, self.outputs, self.max_block
        self._map = (C.c_int32 * max(self.outputs, 1))(*[int(x) for x in stream_of_output])
        self._off = (C.c_int32 * max(self.outputs, 1))(*[int(x) for x in offset_hz])
        cfg.stream_of_output = C.cast(self._map, C.POINTER(C.c_int32))
        cfg.offset_hz = C.cast(self._off, C.POINTER(C.c_int32))
        self.h = C.c_void_p()
        if self.rate_hz is not None:
            self._check(self.L.fmx_wideband_create_rate(C.byref(cfg), self.rate_hz, C.byref(self.h)))
        else:
            self._check(self.L.fmx_wideband_create(C.byref(cfg), C.byref(self.h)))

    def _check(self, rc):
        if rc != FMX_OK:
            raise FmxError(rc, self.L.fmx_last_error().decode("utf-8", "replace"))

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.fmx_wideband_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_offset(self, output, hz):
        self._check(self.L.fmx_wideband_set_offset(self.h, int(output), int(hz)))

    def outputs_for(self, n_wide):
        """The outputs per station that the next call will produce for n_wide samples (processing thread)."""
        return int(self.L.fmx_wideband_outputs_for(self.h, int(n_wide)))

    def survey(self, blocks_per_record):
        """Begin a band survey at the next call (blocks of 4096 wide samples per record, 1 .. 4096), or end it (0)."""
        self._check(self.L.fmx_wideband_survey_enable(self.h, int(blocks_per_record)))

    def survey_read(self, stream, capacity=4):
        """The records of `stream` completed since its last read, oldest first -> (records as SURVEY_RECORD_DTYPE, power [n, 4096] f32)."""
        recs = np.zeros(max(capacity, 1), SURVEY_RECORD_DTYPE)
        power = np.zeros((max(capacity, 1), SURVEY_BINS), np.float32)
        n = C.c_int32()
        self._check(self.L.fmx_wideband_survey_read(self.h, int(stream), recs.ctypes.data_as(C.c_void_p), power.ctypes.data_as(C.POINTER(C.c_float)),
                                                    int(capacity), C.byref(n)))
        return recs[:n.value].copy(), power[:n.value].copy()

    def process_host(self, wide, fmt=IQ_F32, s16_denominator=2048.0):
        """wide: [streams, n_wide, 2] (or [n_wide, 2] for one stream) of float32 / uint8 / int8 / int16 according to fmt
        -> complex IQ float32 [outputs, n_wide / factor (a rate object: outputs_for (n_wide)), 2]."""
        dt = {IQ_U8: np.uint8, IQ_S8: np.int8, IQ_S16: np.int16, IQ_F32: np.float32}[fmt]
        wide = np.ascontiguousarray(wide, dt)
        if wide.ndim == 2:
            wide = wide[None]
        assert wide.shape[0] == self.streams and wide.shape[2] == 2
        n = wide.shape[1]
        cap = max(self.outputs_for(n), 1)
        out = np.zeros((self.outputs, cap, 2), np.float32)
        got = C.c_int64()
        self._check(self.L.fmx_wideband_process_host_raw(self.h, wide.ctypes.data_as(C.c_void_p), fmt, float(s16_denominator), n, n,
                                                         out.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(got)))
        return out[:, :got.value]

    def process_device(self, d_wide_ptr, wide_stride, n_wide, d_narrow_ptr, narrow_stride, fmt=IQ_F32, s16_denominator=2048.0, hip_stream=None):
        """Device pointers, asynchronous on hip_stream; returns the outputs per station (n_wide / factor; a rate object: outputs_for (n_wide)).  Fmx.process_device (d_narrow_ptr, narrow_stride, ...) on the
        same stream takes the result as it lies."""
        got = C.c_int64()
        self._check(self.L.fmx_wideband_process_device_raw(self.h, C.c_void_p(d_wide_ptr), fmt, float(s16_denominator), wide_stride, n_wide,
                                                           C.c_void_p(d_narrow_ptr), narrow_stride, C.byref(got), C.c_void_p(hip_stream or 0)))
        return got.value


class FmProcessor:
    """Host-side mirror of the reference's ``fmProcessor`` (fm-processor.h:79-156) for ONE channel
    of an :class:`Fmx` batch: same method names and argument meaning as the reference setters, so a
    test written against the reference class reads the same here.  ``run_block`` is one iteration
    of ``fmProcessor::run()`` (fm-processor.cpp:387-686): pull a block from a deviceHandler-shaped
    source (``Samples()``/``getSamples(n)``) and push PCM into an audioSink-shaped sink
    (``putSamples(array)``)."""

    FM_Mode = {"Stereo": 0, "StereoPano": 1, "Mono": 2}
    DECODERS = {"AM": 1, "FM PLL Decoder": 2, "FM Mixed Demod": 3, "FM Complex Baseband Delay": 4,
                "FM Real Baseband Delay": 5, "FM Difference Based": 6}      # fm-demodulator.cpp:36-43

    def __init__(self, theDevice=None, mySink=None, inputRate=None, fmRate=192000, workingRate=48000,
                 audioRate=48000, fmx=None, channel=0, blockSize=16384):
        self.myRig, self.theSink = theDevice, mySink
        if inputRate is None:                             # radio.cpp:836: inputRate = theDevice -> getRate ()
            inputRate = theDevice.getRate() if hasattr(theDevice, "getRate") else 2304000
        self.fmx = fmx if fmx is not None else Fmx(1, max_block=blockSize, inputRate=inputRate, fmRate=fmRate,
                                                   workingRate=workingRate, audioRate=audioRate)
        self.channel = channel
        self.bufferSize = blockSize                       # fm-processor.cpp:374
        self.scanning = False                             # startScanning / stopScanning: taken over at the next block

    def _set(self, pid, v):
        self.fmx.set_param(pid, v, self.channel)

    # --- the reference's setters (same names) ---
    def setfmMode(self, m): self._set(P_FM_MODE, self.FM_Mode[m] if isinstance(m, str) else m)

    def setFMdecoder(self, name):
        # fm_Demodulator::setDecoder: an unknown name selects -1, which falls into `default:` = PLL
        self._set(P_FM_DECODER, self.DECODERS.get(name, 2) if isinstance(name, str) else name)

    def setSoundMode(self, selector): self._set(P_SOUND_MODE, selector)
    def setStereoPanorama(self, pan): self._set(P_STEREO_PANORAMA, pan)
    def setSoundBalance(self, balance): self._set(P_SOUND_BALANCE, balance)
    def setDeemphasis(self, us): self._set(P_DEEMPHASIS, us)
    def setVolume(self, gain_db): self._set(P_VOLUME_DB, gain_db)
    def setlfcutoff(self, hz): self._set(P_LF_CUTOFF, hz)

    def setBandwidth(self, s):
        # the reference takes the GUI string "165kHz" or "Off" (fm-processor.cpp:232-239)
        if isinstance(s, str):
            v = 0 if s == "Off" else int("".join(ch for ch in s if ch.isdigit() or ch == "-") or "0") * 1000
        else:
            v = int(s)
        self._set(P_BANDWIDTH, v)

    def setAttenuation(self, l, r):
        self._set(P_ATTENUATION_L, l)
        self._set(P_ATTENUATION_R, r)

    def setfmRdsSelector(self, m): self._set(P_RDS_MODE, m)
    def triggerFrequencyChange(self): self._set(A_TRIGGER_FREQUENCY_CHANGE, 0)
    def restartPssAnalyzer(self): self._set(A_RESTART_PSS, 0)
    def resetRds(self): self._set(A_RESET_RDS, 0)
    def set_localOscillator(self, lo): self._set(P_LOCAL_OSCILLATOR, lo)
    def set_squelchMode(self, m): self._set(P_SQUELCH_MODE, m)          # ESqMode: 0 OFF, 1 NSQ, 2 LSQ
    def set_squelchValue(self, v): self._set(P_SQUELCH_VALUE, v)         # fm-processor.cpp:213-215
    def getSquelchState(self): return bool(self.fmx.meta(self.channel).squelch_active)      # :217-219
    def pollPeakLevels(self): return self.fmx.peaks(self.channel)       # what showPeakLevel was emitted with since the last poll
    def setAutoMonoMode(self, b): self._set(P_AUTO_MONO, 1 if b else 0)
    def setPSSMode(self, b): self._set(P_PSS, 1 if b else 0)
    def setDCRemove(self, b): self._set(P_DC_REMOVE, 1 if b else 0)
    def setTestTone(self, b): self._set(P_TEST_TONE, 1 if b else 0)
    def setDispDelay(self, steps): self._set(P_DISP_DELAY, steps)

    # scan mode (fm-processor.cpp:361-367, 478-495): the threshold is the constructor's thresHold, here a setting
    def startScanning(self): self.scanning = True
    def stopScanning(self): self.scanning = False
    def setScanThreshold(self, db): self._set(P_SCAN_THRESHOLD, db)

    def pollScanResults(self):
        """The scan records since the last poll; the reference emits scanresult () for each with `found` set."""
        return self.fmx.scan_results(self.channel)

    def setModulationMeter(self, on): self.fmx.mod_meter(on, self.channel)

    def pollModulation(self):
        """The modulation meter's records since the last poll (MOD_DTYPE): peak deviation, multiplex power and pilot per 50 ms window."""
        return self.fmx.mod_records(self.channel, 1)[0]

    def setAudioMeter(self, on): self.fmx.audio_meter(on, self.channel)

    def pollAudio(self):
        """The audio meter's records since the last poll (AUDIO_DTYPE): peak, mean square, K-weighted mean square and cross term per 100 ms window."""
        return self.fmx.audio_records(self.channel, 1)[0]

    def setReceptionMeter(self, on): self.fmx.rx_meter(on, self.channel)

    def pollReception(self):
        """The reception meter's records since the last poll (RX_DTYPE): power maximum, minimum, mean, mean square and lag-1 correlation per 50 ms window."""
        return self.fmx.rx_records(self.channel, 1)[0]

    def setRdsMeter(self, on): self.fmx.rds_meter_enable(on, self.channel)

    def pollRdsMeter(self):
        """The RDS meter's records since the last poll (RDSM_DTYPE): power maximum and the second and first moments of I and Q per 2560 RDS samples."""
        return self.fmx.rds_meter_records(self.channel, 1)[0]

    def setSpectrumMeter(self, on, stream=-1): self.fmx.spectrum_meter(on, stream)

    def pollSpectrum(self, stream=0):
        """The spectrum meter's records of a stream since the last poll: (records as SPECTRUM_RECORD_DTYPE, mean [n, 4096], peak [n, 4096])."""
        return self.fmx.spectrum_read(stream)

    def setMpxSpectrumMeter(self, on): self.fmx.mpx_spectrum_meter(on, self.channel)

    def pollMpxSpectrum(self):
        """The multiplex spectrum meter's records of this channel since the last poll: (records as MPX_RECORD_DTYPE, mean [n, 2048], peak [n, 2048])."""
        return self.fmx.mpx_spectrum_read(self.channel, 1)[0]

    def setScaDecoder(self, centre_hz): self.fmx.sca_enable(centre_hz, self.channel)

    def pollSca(self):
        """The sub-carrier decoder's blocks of this channel since the last poll: (first_block or -1, audio [n, 240] at fmRate / 8, level [n])."""
        return self.fmx.sca_read(self.channel, 1)[0]

    def setFeed(self, mode): self.fmx.feed(mode, self.channel)

    def pollFeed(self, fmt="f32"):
        """The monitoring feed's blocks of this channel since the last poll: (first_block or -1, audio [n, 160] at 16 kS/s, power [n])."""
        return self.fmx.feed_read(self.channel, 1, fmt=fmt)[0]

    def isPilotLocked(self):
        m = self.fmx.meta(self.channel)
        return bool(m.live_pilot_locked), m.live_lock_strength

    def get_demodDcComponent(self): return self.fmx.meta(self.channel).live_dc_if

    def run_block(self):
        """One loop iteration of fmProcessor::run(): returns False when the device has < bufferSize samples."""
        if self.myRig.Samples() < self.bufferSize:
            return False
        iq = self.myRig.getSamples(self.bufferSize)
        scanning = self.scanning                          # (read once: the flag and what the sink gets belong to the same block)
        self._set(P_SCANNING, 1 if scanning else 0)
        pcm = self.fmx.process_host(iq)
        if self.theSink is not None and pcm.shape[1] > 0 and not scanning:    # the reference's loop sends nothing while it scans (:494)
            self.theSink.putSamples(pcm[self.channel])
        return True

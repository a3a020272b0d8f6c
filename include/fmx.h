/*
 * fmx.h -- C ABI of libfmx: the MI355X (gfx950) implementation of sdr-j-fm's FM processing
 * chain (reference: /root/reference/src/fm/fm-processor.cpp:373-759 and the leaf classes in
 * src/various).  One fmx handle owns N independent FM channels ("fmProcessor" instances) that
 * are demodulated as one batch on one GPU.
 *
 * Each entry point names the reference interface it replaces (file:line relative to the
 * reference tree).  No C++, Qt or torch types cross this boundary: plain pointers and sizes.
 *
 * Threading: exactly one processing thread per handle (the adapter's QThread replacing
 * fmProcessor::run()).  fmx_set_param may be called from any thread; values take effect at the
 * next fmx_process_* call, mirroring the settings mailbox of fm-processor.cpp:396-413.
 * Ownership: the caller owns every in/out buffer; the handle owns all device memory and state.
 * Errors: 0 = FMX_OK, negative = error; text via fmx_last_error().  There is NO CPU fallback:
 * every call fails with FMX_E_NO_DEVICE / FMX_E_HIP when the GPU path is unavailable.
 */
#ifndef FMX_H
#define FMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: fmx_meta and fmx_rds_info grew (live_rf_dc_*, radio_text_ucs2*), FMX_P_PLL_SOLVER 3, fmx_pll_exact_segments.
 * 3 (round 6): handles above 64 channels keep no display feeds unless asked (FMX_P_SCOPE_TAPS: fmx_get_tap / fmx_get_peaks answer FMX_E_UNSUPPORTED there), round 5's
 * exports (fmx_last_front_kernel, fmx_last_call_pieces, fmx_last_second_group, fmx_last_rds_samples_of ...), FMX_P_FRONT_KERNEL without its value 2.  The output
 * structs are caller-allocated and carry no size field: a caller built against another version must not call in -- the adapters
 * compare fmx_abi_version () with the FMX_ABI_VERSION they were compiled with when they load the library. */
#define FMX_ABI_VERSION 3

typedef struct fmx_handle_s *fmx_handle;

enum {
    FMX_OK = 0,
    FMX_E_INVALID = -1,        /* bad argument / unknown parameter id / out-of-range value */
    FMX_E_UNSUPPORTED = -2,    /* a setting of the reference this build does not implement */
    FMX_E_NO_DEVICE = -3,      /* no HIP device: the product path never falls back to the CPU */
    FMX_E_HIP = -4,            /* HIP runtime error (text in fmx_last_error) */
    FMX_E_NOMEM = -5,
    FMX_E_TOO_LARGE = -6,      /* n > max_block, or pcm capacity too small */
};

/* Construction arguments: replaces the fmProcessor constructor
 * (fm-processor.cpp:48-63; GUI values radio.cpp:231-252,915-930).  Only the DSP-relevant
 * arguments exist here; the scope ring buffers / Qt objects stay in the adapter. */
typedef struct {
    int32_t struct_size;       /* sizeof(fmx_config), for ABI growth */
    int32_t device;            /* HIP device ordinal */
    int32_t channels;          /* number of FM channels in this batch (>=1) */
    int32_t streams;           /* number of distinct IQ input streams; 0 => one per channel */
    const int32_t *stream_of_channel; /* [channels] or NULL (identity); several channels may share a
                                  wide-band stream and differ in set_localOscillator (BASELINE config 3) */
    int32_t inputRate;         /* the device's rate (deviceHandler::getRate, radio.cpp:836): 2304000 (fm-constants.h:35), or any rate the reference
                                  decimates by 12 (2304000 <= inputRate < 3456000), by 6 (1152000 <= inputRate < 2304000: its second decimator
                                  then only filters) or not at all (inputRate / fmRate <= 1: the 192 kS/s devices) -- fm-processor.cpp:68-75,
                                  :471; what the decimation leaves is treated as fmRate, as in the reference.  Other rates: FMX_E_UNSUPPORTED */
    int32_t fmRate;            /* 192000 */
    int32_t workingRate;       /* 48000 */
    int32_t audioRate;         /* 48000 = workingRate: sendSampletoOutput's direct path (:826-829); any other rate in 8000 .. 192000
                                  with audioRate / gcd <= 640 runs the second converter (theConverter :89-91, :830-837; main.cpp:57-65 -m) */
    int32_t max_block;         /* max complex samples per stream per call (reference block = 16384, :374) */
} fmx_config;

/* One id per fmProcessor setter (fm-processor.h:104-156).  Values are passed as double. */
typedef enum {
    FMX_P_FM_MODE = 1,         /* setfmMode: 0 Stereo, 1 StereoPano, 2 Mono          (:241-243)  */
    FMX_P_FM_DECODER = 2,      /* fm_Demodulator::setDecoder: 1 AM 2 PLL 3 Mixed 4 ComplexBB 5 RealBB 6 Diff
                                  (fm-demodulator.cpp:27-44,93-103,215-241) */
    FMX_P_SOUND_MODE = 3,      /* setSoundMode: Channels enum 0..6                   (:273-275)  */
    FMX_P_STEREO_PANORAMA = 4, /* setStereoPanorama 0..200                           (:277-280)  */
    FMX_P_SOUND_BALANCE = 5,   /* setSoundBalance -100..100                          (:282-286)  */
    FMX_P_DEEMPHASIS = 6,      /* setDeemphasis, microseconds >= 1                   (:291-297)  */
    FMX_P_VOLUME_DB = 7,       /* setVolume, dB                                      (:299-301)  */
    FMX_P_LF_CUTOFF = 8,       /* setlfcutoff, Hz; <= 0 switches the audio filter off (:762-770) */
    FMX_P_BANDWIDTH = 9,       /* setBandwidth, Hz (the GUI's "165kHz" -> 165000); 0 = "Off" (:232-239) */
    FMX_P_ATTENUATION_L = 10,  /* setAttenuation (Lgain)                             (:351-359)  */
    FMX_P_ATTENUATION_R = 11,  /* setAttenuation (Rgain)                                         */
    FMX_P_RDS_MODE = 12,       /* setfmRdsSelector: 0 off, 1 = RDS_1 (rds-decoder-1.cpp), 2 = RDS_2 (rds-decoder-2.cpp),
                                  3 = RDS_3 (rds-decoder-3.cpp)                      (:840-847).  Per channel, at any time: a channel's RDS path
                                  (block filters, phase delay line, decimator, slicers) runs while its decoder is on and keeps what it holds while
                                  it is off, as the reference's processor does (:733-754, :551-553) -- nothing is restarted by a switch */
    FMX_P_LOCAL_OSCILLATOR = 13,/* set_localOscillator, Hz                           (:866-868)  */
    FMX_P_AUTO_MONO = 14,      /* setAutoMonoMode                                    (:914-916)  */
    FMX_P_PSS = 15,            /* setPSSMode                                         (:918-920)  */
    FMX_P_DC_REMOVE = 16,      /* setDCRemove (also zeroes RfDC)                     (:922-925)  */
    FMX_P_SQUELCH_MODE = 17,   /* set_squelchMode (fm-processor.cpp:882): 0 OFF, 1 NSQ (noise squelch, squelchClass.cpp:47-87: two order-20
                                  Chebyshev filters around 70 kHz on the demodulator output), 2 LSQ (level squelch, :89-113) */
    FMX_P_TEST_TONE = 18,      /* setTestTone (:931-933): 1 kHz bursts of 25 ms every 2 s at 0.9, programme at 0.1 (:800-823) */
    FMX_P_SQUELCH_VALUE = 19,  /* set_squelchValue 0..100 (:213-215): takes effect at the next call when it differs  */
    FMX_P_DISP_DELAY = 20,     /* setDispDelay (:935-937): steps of the peak-level delay line; applies to the windows
                                  fmx_get_peaks has not handed out yet */
    FMX_P_PLL_SOLVER = 21,     /* how stage B evaluates the pilot PLL loop of pilot-recover.cpp:54-61 (no counterpart in the reference, whose
                                  loop runs sample by sample): 1 = sequentially in every segment -- the reference's f32 trajectory (one thread
                                  per channel walks the recurrence, the table arithmetic is prepared by all); 2 = all samples of a segment at
                                  once by Newton's method (the trajectory to ~1e-5 rad: the loop's own f32 rounding noise, integrated) WHILE
                                  THE PILOT IS COMFORTABLY IN LOCK, sequentially otherwise -- during acquisition and whenever the lock metric
                                  came within 0.05 of its threshold in the previous segment, so that every lock decision
                                  (pilot-recover.cpp:62-80) is taken on the reference's own trajectory: what large batches use;
                                  3 = Newton's method always (diagnostic: lock decisions may then fall a few samples apart from the
                                  reference's when the metric creeps through its threshold); 0 = automatic: 1 up to 64 channels per
                                  handle, 2 above (default).  "The reference's trajectory" to this bound: every evaluation of the loop step,
                                  the sequential one included, takes the NCO sine from the GPU's sine unit, within 1.2e-7 of the
                                  reference's table entry (not that entry bit for bit, and the unit's rounding is this architecture's);
                                  the lock decisions were equal to the oracle's in every tested case, which a metric creeping at 1e-6
                                  per sample through its threshold does not guarantee to the sample. */
    FMX_P_STAGEB_FORM = 22,    /* (handle-wide: the channel argument is ignored) stage B -- limiter .. de-emphasis -- as 1 = one kernel per call,
                                  2 = two kernels (limiter .. lock detector, then PSS .. de-emphasis: four workgroups per CU instead of
                                  three); 0 = automatic (default): whichever wastes less of its last round of workgroups for the
                                  handle's channel count.  The results of the two forms are bit-identical. */
    FMX_P_FILTER_RESTARTS = 23,/* (handle-wide, before the first call) how the two overlap-add filters of the reference -- inputFilter (65536 points, 251
                                  taps, :469-470) and fmAudioFilter (8192 points, 756 taps, :589-591) -- are built: 1 = as the block machines they
                                  are (fft-filters.cpp:33-163): a setBandwidth / setlfcutoff in the middle of a stream then replays the last output
                                  block, drops the block in progress and carries the old tail over, sample for sample as the reference does (any
                                  channel count; about seven times the cost of 2 on a batch); 2 = folded into stage A's / stage C's polyphase FIRs
                                  for good -- the same filters wherever the settings were made before the first call, a different glitch of one
                                  filter latency behind a change in mid-stream; 0 = automatic (default): 1 up to 64 channels; above, folded UNTIL a
                                  filter setter arrives in mid-stream -- the handle then becomes a block-machine handle before the setter takes
                                  effect (fmx_filter_change_due), and the change is the reference's, sample for sample */
    FMX_P_FRONT_PARTS = 24,    /* (handle-wide: the channel argument is ignored) the input-filter stage runs one workgroup per channel; a handle with
                                  fewer channels than the GPU has workgroup slots splits every channel's call in time over several workgroups
                                  (each later one recomputes one 1536-sample tile to get its filter history): 0 = automatic (default), 1 = never,
                                  2..32 = that many parts wherever a call is long enough.  The results are bit-identical. */
    FMX_P_FRONT_KERNEL = 25,   /* (handle-wide: the channel argument is ignored) which kernel runs the input-filter stage.
                                  1 = fmx_front.hip: four waves per channel, the folded filter as packed f32 FMAs; every input format, local
                                  oscillators, any call.
                                  3 = fmx_front4.hip: the filter on the matrix pipe -- samples and taps split into two f16 halves each, their
                                  products exact in the f32 accumulator, the remainders' roundings at 2^-22 of a product: the fm-rate IQ
                                  agrees with kernel 1's to 5e-7 of its amplitude, PCM against the oracle is unchanged.  BLOCK FLOATING
                                  POINT: every 1536-sample tile of a channel is split behind a power-of-two scale of its own (its largest
                                  balanced sample goes to [2^14, 2^15)), so the stage is linear at any level, as the reference's f32 filter
                                  is -- nothing is clamped, weak signals keep 22 bits.  (Limit: two adjacent tiles of one channel whose
                                  largest samples differ by more than 2^126.)  The IQ balance is applied in front of the filter, where the
                                  reference has it (fm-processor.cpp:462-464).
                                  3 takes the whole 1536-sample tiles of the calls it can -- any sample format, the input filter on
                                  everywhere, a balance between 1e-6 and 1e6 in magnitude, a call that starts on a multiple of 12 samples --
                                  and leaves the rest to kernel 1.  A handle with LOCAL OSCILLATORS runs the kernel's complex-tap variant
                                  (the mix folded into a tap set per channel built from the reference's own oscillator table; one channel
                                  per workgroup: automatic for handles with at least one channel per compute unit).  (2 was round 5's six-wave VALU
                                  kernel: measured slower, now tools/experiments/fmx_front3.hip; the value is refused.)
                                  0 = automatic (default): 3 where a handle qualifies and has the channels to fill the GPU, else 1. */
    FMX_P_SCOPE_TAPS = 26,     /* (handle-wide: the channel argument is ignored) whether the DISPLAY FEEDS are produced: the three scope taps that are rows
                                  of stage B's work arrays -- FMX_TAP_DEMOD, FMX_TAP_LR_RAW, FMX_TAP_PILOT_PHASE (fm-processor.cpp:608-613 and the
                                  demodulator / pilot scopes): 12 bytes written per channel and fm sample that nothing else reads (a channel that
                                  decodes RDS keeps its demodulator and pilot rows regardless: the RDS path reads them) -- and the peak-level
                                  meter's maxima (showPeakLevel: fmx_get_peaks).  1 = produced, 0 = not (fmx_get_tap answers FMX_E_UNSUPPORTED for
                                  those taps, fmx_get_peaks likewise; FMX_TAP_FM_IQ, FMX_TAP_PRE_RESAMPLER and FMX_TAP_RDS_IQ are read from rings
                                  and always there), -1 = automatic (default): produced by handles of up to 64 channels -- the receiver with a
                                  display --, not by larger batches.  The PCM does not depend on it.  Takes effect at the next call. */
    FMX_P_CALL_PIECES = 27,    /* (handle-wide: the channel argument is ignored) fm samples per PIECE of a call that is made in overlapping pieces.  A batch
                                  whose channels run the PLL / AM decoder or a squelch (pllC.cpp:67-90, squelchClass.cpp:47-113: recurrences that walk a
                                  channel's samples one after the other, one wave per 64 channels) would leave the GPU idle for most of such a call:
                                  the library cuts the call into pieces -- the chain does not depend on how a stream is cut into calls -- and runs the
                                  input filter of piece k + 1 and the stereo / audio stages of piece k - 1 while the recurrences walk piece k.
                                  -1 = automatic (default): 3840 (AM decoder) or 4608 (PLL decoder alone) with a short last piece (19200 fm samples are cut 4608 4608 4608 3840 1536)
                                  or 4608 (squelches only) for handles of 1024 channels and more, calls of two pieces and more, no RDS decoder on, no second converter;
                                  0 = never; n > 0: pieces of n fm samples (rounded up to 16) for any handle above 64 channels.  Takes effect at the next call. */
    FMX_P_SCANNING = 28,       /* startScanning / stopScanning (fm-processor.cpp:361-367): 0 or 1, per channel.  While a channel scans, its fm-rate samples
                                  (those of FMX_TAP_FM_IQ, the value behind fmBand_2 the reference puts into scanBuffer, :478-481) are collected in
                                  blocks of 1024; every complete block goes through a 1024-point forward transform (Fft_transform, f32, no scaling)
                                  and becomes one record of fmx_scan_results: get_db (getSignal) and get_db (getNoise) (:484-493, :886-904,
                                  fm-constants.h:144) and whether their difference exceeds the threshold (the reference's scanresult ()).  A
                                  channel's SCAN CARRY (the block being collected, 0..1023 samples) starts empty at fmx_create, is advanced by the
                                  calls in which the channel scans only, and is never reset: a block may hold samples from before a pause and from
                                  after it, as the reference's scanPointer (a local of run (), :377, untouched by start / stopScanning) does.
                                  ONE DELIBERATE DIFFERENCE: the reference skips its demodulator and everything behind it while scanning (:494
                                  `continue`); here the channel's chain -- stages B and C, the RDS path -- runs on, and its PCM frames of a scanning
                                  call are written as zeros.  The channels of a handle share one sample and frame timeline, so a channel cannot skip
                                  fm samples, and the result is exact: outside its scanning calls a channel that scanned is bit-identical to one that
                                  never did.  So after a scan the chain continues from its running state, where the reference's continues from the
                                  state it froze.  Taps, meta and peaks of a scanning channel report the running chain (the adapters hold them back
                                  while scanning).  Takes effect at the next call. */
    FMX_P_SCAN_THRESHOLD = 29, /* the constructor's thresHold (fm-processor.cpp:63,108; the GUI's ini key `threshold`, default 20, radio.cpp:912-913),
                                  per channel, in dB: an integral value in -32768..32767 (int16_t), default 20.  A record takes the threshold of the
                                  call that completed its block.  Takes effect at the next call. */
    /* actions (value ignored) */
    FMX_A_TRIGGER_FREQUENCY_CHANGE = 100, /* triggerFrequencyChange (:849-855) */
    FMX_A_RESTART_PSS = 101,              /* restartPssAnalyzer     (:857-860) */
    FMX_A_RESET_RDS = 102,                /* resetRds               (:862-864) */
} fmx_param_id;

/* What fmProcessor reports upward: SMetaData (fm-processor.h:91-101, emitted :662-684) */
typedef struct {
    float   DcValRf, DcValIf, PssPhaseShiftDegree, PssPhaseChange;
    int32_t PssState;          /* 0 OFF, 1 ANALYZING, 2 ESTABLISHED */
    float   PilotPllLockStrength;
    int32_t PilotPllLocked;
    int64_t fm_samples;        /* fm-rate samples processed so far */
    int64_t pcm_frames;        /* PCM frames produced so far */
    /* live values (not the 0.5 s snapshot): what isPilotLocked() (:870-880) / get_demodDcComponent() (:221-226) read */
    int32_t live_pilot_locked;
    float   live_lock_strength;
    float   live_dc_if;
    int32_t squelch_active;    /* getSquelchState (:217-219): the level squelch is muting the demodulator output */
    float   live_rf_dc_re, live_rf_dc_im;   /* RfDC (:423-446) behind the last sample processed: what a caller needs to reproduce the
                                               DC-corrected block the reference dumps (:448-455) with the reference's own recurrence */
} fmx_meta;

typedef enum {
    FMX_TAP_FM_IQ = 0,         /* complex @fmRate after fmBand_2 (IF_FILTERED scope, :601-604)   */
    FMX_TAP_DEMOD = 1,         /* float   @fmRate after demodulate (DEMODULATOR scope, :605-607) */
    FMX_TAP_LR_RAW = 2,        /* complex @fmRate (sum,diff) (AF_SUM/AF_DIFF scopes, :608-613)   */
    FMX_TAP_PRE_RESAMPLER = 3, /* complex @fmRate after de-emphasis (:594-595), before gain.  On a handle
                                  that runs the folded filters the audio low-pass is applied AFTER this
                                  point (stage C); on a block-machine handle (FMX_P_FILTER_RESTARTS, a
                                  promoted batch) the tap holds the reference's own value, behind
                                  fmAudioFilter AND the de-emphasis (:589-595) */
    FMX_TAP_RDS_IQ = 4,        /* complex @24 kS/s after rdsDecimator (RDS_INPUT scope, :566-569)        */
    FMX_TAP_PILOT_PHASE = 5,   /* float   @fmRate currentPilotPhase (:695; the value the RDS mixer's phase buffer takes, :747) */
} fmx_tap_id;

/* One record of scan mode (FMX_P_SCANNING): what the reference computes for every block of 1024 fm samples it scans (fm-processor.cpp:483-493) */
typedef struct fmx_scan_result {
    int64_t block;        /* the channel's scan-block number since fmx_create, from 0 (a gap = records dropped) */
    int64_t end_sample;   /* fm-sample index (reference numbering, as FMX_TAP_FM_IQ) one past the block's last sample */
    float   signal_db;    /* get_db (getSignal (X, 1024), 256) */
    float   noise_db;     /* get_db (getNoise (X, 1024), 256) */
    int32_t found;        /* signal_db - noise_db > threshold: where the reference emits scanresult () */
    int32_t reserved;
} fmx_scan_result;

/* per-kernel timing collected with HIP events on the processing stream */
typedef struct {
    int64_t launches[4];       /* 0 front-end (input FIR), 1 demod/pilot/PSS, 2 audio FIR+resample, 3 reserved */
    double  ms[4];             /* accumulated GPU time of each kernel */
    int64_t input_samples;     /* complex input samples (summed over streams) covered by the timings */
    int64_t channel_samples;   /* complex input samples summed over channels */
} fmx_profile;

int  fmx_abi_version(void);
const char *fmx_last_error(void);

/* replaces `new fmProcessor(...)` (radio.cpp:915-930) */
int  fmx_create(const fmx_config *cfg, fmx_handle *out);
/* replaces fmProcessor::stop() + delete (fm-processor.cpp:200-211) */
int  fmx_destroy(fmx_handle h);

/* replaces the ~25 setters; channel = -1 addresses every channel */
int  fmx_set_param(fmx_handle h, int32_t channel, int32_t param_id, double value);

/* number of PCM frames the next call with n complex samples will produce per channel */
int64_t fmx_frames_for(fmx_handle h, int64_t n_complex);
/* replaces the moment at which the reference's loop takes a setBandwidth / setlfcutoff over (fm-processor.cpp:396-408: the next block start).  A handle
 * that runs its filters as the reference's block machines takes it with its next call: -1.  A BATCH (above 64 channels, FMX_P_FILTER_RESTARTS
 * automatic) runs the filters folded into its polyphase FIRs until a filter setter arrives in mid-stream; it then keeps what its streams deliver for
 * three blocks of the input filter (196 879 samples, 85 ms) and becomes a block-machine handle at the first call boundary behind that, where the setter
 * restarts its filter exactly as the reference's setLowPass does (fft-filters.cpp:84-95).  Returns the input samples per stream still to come before
 * that call (0: the next call applies the change at its first sample), -1 when nothing is pending. */
int64_t fmx_filter_change_due(fmx_handle h);

/* Replaces one iteration of the loop in fmProcessor::run() (fm-processor.cpp:387-686) for every
 * channel: `iq` = what deviceHandler::getSamples (device-handler.h:71-74) delivered, interleaved
 * (I,Q) float32, stream s at iq + 2*s*stream_stride; `pcm` = what is handed to
 * audioSink::putSamples (audiosink.h:45), interleaved (L,R) float32, channel c at
 * pcm + 2*c*pcm_stride.  Host buffers; synchronous. */
int  fmx_process_host(fmx_handle h, const float *iq, int64_t stream_stride, int64_t n_complex,
                      float *pcm, int64_t pcm_stride, int64_t *n_frames);
/* Same with DEVICE pointers (IQ already resident in HBM); asynchronous on `hip_stream`
 * (a hipStream_t, NULL = the handle's own stream, which first waits for the work queued on HIP's default stream -- the
 * stream NULL names -- at the time of the call, so a producer there needs no extra synchronisation; the results are
 * ordered by fmx_synchronize).  *n_frames is known on return. */
int  fmx_process_device(fmx_handle h, const float *d_iq, int64_t stream_stride, int64_t n_complex,
                        float *d_pcm, int64_t pcm_stride, int64_t *n_frames, void *hip_stream);
/* The same two calls for RAW device samples (the conversion the device handlers do on the host moves into
 * the input-FIR kernel, so 2 or 4 bytes per complex sample cross PCIe / HBM instead of 8).  Interleaved (I,Q) pairs of
 *   FMX_IQ_F32  float32, as above
 *   FMX_IQ_U8   uint8,  value = (u8 - 127) / 128        rtlsdr-handler.cpp:291-292
 *   FMX_IQ_S8   int8,   value = s8 / 128                hackrf-handler.cpp:364-365
 *   FMX_IQ_S16  int16,  value = s16 / s16_denominator   lime-handler.cpp:250, pluto-handler.cpp:578,
 *                                                       sdrplay-handler-v3.cpp:261 (2048 or 4096); 32768 for PCM16 files
 * stream_stride stays in COMPLEX SAMPLES; s16_denominator must be a power of two (the division is then exact, as in the
 * reference) and is ignored for the other formats. */
typedef enum { FMX_IQ_F32 = 0, FMX_IQ_U8 = 1, FMX_IQ_S8 = 2, FMX_IQ_S16 = 3 } fmx_iq_format;
int  fmx_process_host_raw(fmx_handle h, const void *iq, int32_t format, float s16_denominator, int64_t stream_stride,
                          int64_t n_complex, float *pcm, int64_t pcm_stride, int64_t *n_frames);
int  fmx_process_device_raw(fmx_handle h, const void *d_iq, int32_t format, float s16_denominator, int64_t stream_stride,
                            int64_t n_complex, float *d_pcm, int64_t pcm_stride, int64_t *n_frames, void *hip_stream);
int  fmx_synchronize(fmx_handle h);

/* replaces the showMetaData signal payload / isPilotLocked / get_demodDcComponent */
int  fmx_get_meta(fmx_handle h, int32_t channel, fmx_meta *meta);
/* replaces the showPeakLevel signal (fm-processor.h:293, evaluatePeakLevel fm-processor.cpp:772-798): every 961 PCM
 * frames the reference emits (leftDb, rightDb) of the window's absolute maxima, behind a display delay line.  Copies
 * the (leftDb, rightDb) pairs of the windows that closed since the last fetch, oldest first, at most `capacity` pairs
 * (the maxima are taken on the GPU next to the audio FIR; dB conversion and delay line run here).  The library keeps
 * the last 256 windows (5 s) per channel. */
int  fmx_get_peaks(fmx_handle h, int32_t channel, float *lr_db, int32_t capacity, int32_t *n_events);
/* replaces the hf/lf/iq scope ring feeds: copies the most recent n samples of a tap
 * (n * 1 or 2 floats) to host memory; n <= samples produced by the last call (fmx_last_fm_samples / fmx_last_rds_samples: while a channel
 * decodes RDS, a call of more than 31999 fm samples -- 383988 input samples at the rates the reference decimates by 12, 191994 at those it
 * decimates by 6, 31999 where it does not decimate -- is made in pieces of that length, and the taps at the fm rate hold the last piece.  FMX_TAP_RDS_IQ is read from a ring of 8192
 * samples per channel and reaches back over the whole call, pieces or not: n <= fmx_last_rds_samples_of and n <= 8192 -- of a call of more than
 * 786432 input samples only the last 8192 can be had; a larger n is FMX_E_INVALID) */
int  fmx_get_tap(fmx_handle h, int32_t channel, int32_t tap_id, float *dst, int64_t n);
/* What the reference's RDS classes tell the GUI through Qt signals (rds-groupdecoder.cpp:44-63, rds-blocksynchronizer.cpp:39-42):
 * setPiCode, setPTYCode, setStationLabel, setRadioText / clearRadioText, setAFDisplay, setMusicSpeechFlag, setGroup,
 * setRDSisSynchronized, setbitErrorRate, setCRCErrors, setSyncErrors.  station_label / radio_text hold the raw RDS characters, NUL
 * terminated (the reference shows the label as QString (stationLabel), rds-groupdecoder.cpp:185-186); radio_text_ucs2 is the text as
 * setRadioText receives it. */
typedef struct fmx_rds_info {
    int32_t synchronized;      /* block synchroniser locked (A..C received without error) */
    int32_t pi_code;           /* block A of the last group; 0 until a group has been decoded */
    int32_t pty_code;          /* programme type 0..31, -1 until known */
    int32_t last_group_type;   /* 0..15, -1 until known */
    int32_t groups_decoded;    /* complete groups so far */
    int32_t crc_errors, sync_errors;
    float   bit_error_rate;
    char    station_label[9];  /* PS name (group 0A), blank padded */
    char    radio_text[65];    /* radio text (group 2A) as the reference would display it (trimmed) */
    int32_t af1_khz, af2_khz;  /* alternative frequencies of the last 0A group, 0 = none */
    int32_t music_speech;      /* -1 unknown, else the M/S flag */
    int32_t di_code;
    /* the radio text as rdsGroupDecoder::prepareText hands it to setRadioText (rds-groupdecoder.cpp:298-315): walked pair by pair with
     * the alphabet-switch pairs 0x0F0F / 0x0E0E / 0x1B6E handled as the reference handles them (the pair's second byte is emitted, the
     * character behind it is not), every character through mapEBUtoUnicode (ebu-codetables.c:65-72), QString::trimmed; UTF-16 code
     * units, 0 terminated */
    uint16_t radio_text_ucs2[65];
    int16_t  radio_text_ucs2_len;
} fmx_rds_info;
/* replaces rdsDecoder::processBit + rdsBlockSynchronizer + rdsGroupDecoder (rds-decoder.cpp:104-131,
 * rds-blocksynchronizer.cpp:114-336, rds-groupdecoder.cpp:100-290) on the host: feeds every bit the slicer has produced
 * since the last call into the channel's block synchroniser / group decoder and returns the current picture.
 * Independent of fmx_rds_bits (own read position). */
int  fmx_rds_decode(fmx_handle h, int32_t channel, fmx_rds_info *info);
/* One complete RDS group as the block synchroniser hands it to rdsGroupDecoder::decode (the reference's setGroup feed) */
typedef struct fmx_rds_group {
    int64_t  index;      /* the channel's group number since fmx_create, from 0 (a gap = records dropped) */
    int64_t  end_bit;    /* slicer bit count (fmx_rds_bits' numbering) one past the group's last bit */
    uint16_t block[4];   /* A..D as rdsGroupDecoder::decode receives them */
} fmx_rds_group;
/* fmx_rds_decode for the channels first_channel .. first_channel + n_channels - 1 at once, infos[k] for channel first_channel + k.  For a batch the
 * block synchroniser runs on the GPU behind the bit slicers (every bit, in every call) and leaves the complete groups -- 11.4 per second and channel -- in a
 * ring of 64 per channel; this call waits for the handle's last fmx_process_* call only (not for the device), reads the range's synchroniser states and
 * group rings in two copies whatever the number of channels, and runs the group decoder (PI, PTY, PS name, radio text, AF) of each channel over its new
 * groups on the host.  The picture is fmx_rds_decode's, field for field: the same synchroniser (tests/test_rdssync_cpu.py), the same group decoder.
 * Own decoders and read positions: independent of fmx_rds_decode, fmx_rds_bits and fmx_rds_groups.  A channel that was read less often than every 5.6 s
 * has lost its oldest groups (never a bit: the synchroniser does not wait for the reader).
 * FMX_A_RESET_RDS / FMX_A_TRIGGER_FREQUENCY_CHANGE (a request of this path's own; fmx_rds_decode has its own) take effect at the next fmx_rds_decode_all:
 * the group decoder goes back to unknown and the groups completed before that read-out are dropped; the synchroniser runs on, as the reference's does.
 * The one difference from fmx_rds_decode: that call, whose synchroniser runs at read-out time, SKIPS the bits pending at a reset, so its synchroniser
 * sees a gap in the stream (and resynchronises behind it); this path never skips a bit.  The two agree wherever fmx_rds_decode had nothing pending at
 * the reset -- a caller that polls after every call.
 * A handle on which no channel ever decoded RDS returns the fresh picture fmx_rds_decode returns there.  FMX_E_INVALID: a range outside the handle's
 * channels, or infos NULL with n_channels > 0. */
int  fmx_rds_decode_all(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_rds_info *infos);
/* The setGroup feed for a channel range: the groups completed since this export's last read of the channel (own read position, at most the last 64),
 * oldest first, up to capacity_per_channel records per channel at out + k * capacity_per_channel, their number in n_groups[k]; what does not fit stays
 * for the next read.  The same single read-out of the device as fmx_rds_decode_all. */
int  fmx_rds_groups(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_rds_group *out, int32_t capacity_per_channel, int32_t *n_groups);
/* the same decoder over a caller-supplied bit array, from a fresh state (host only, needs no device): what a
 * recorded bit stream decodes to */
int  fmx_rds_decode_bits(const uint8_t *bits, int32_t n_bits, fmx_rds_info *info);
/* The byte work behind the text signals, exactly as the reference does it (tests/test_rds_text.py pins all three against the
 * reference's own code in oracle/_ref and tests/golden/ref_rds_tables.npz):
 *   fmx_rds_pty_name      pty_table [pty][locale] (ebu-codetables.c:4-37; rds-groupdecoder.cpp:115), UTF-8; NULL outside 0..31 x 0..1
 *   fmx_rds_map_char      mapEBUtoUnicode (alfabet, character) (ebu-codetables.c:65-72)
 *   fmx_rds_prepare_text  rdsGroupDecoder::prepareText (v, length) (:298-315) with alfabetSwitcher / setAlfabetTo (:317-343): writes the
 *                         trimmed text as UTF-16 code units (0 terminated when capacity allows) and returns their count; *alfabet is
 *                         the decoder's theAlfabet (in / out, may be NULL) */
const char *fmx_rds_pty_name(int32_t pty_code, int32_t pty_locale);
uint16_t fmx_rds_map_char(uint8_t alfabet, uint8_t character);
int32_t  fmx_rds_prepare_text(const uint8_t *v, int32_t length, uint8_t *alfabet, uint16_t *out, int32_t capacity);
/* replaces rdsDecoder::doDecode's bit output (rds-decoder.cpp:69-104): pending RDS bits */
int  fmx_rds_bits(fmx_handle h, int32_t channel, uint8_t *bits, int32_t capacity, int32_t *n_bits);
/* replaces doDecode's second output (`*m`, rds-decoder-2.cpp:108-114), the constellation point every bit was decided on, which
 * fmProcessor::run pushes into the IQ scope ring (fm-processor.cpp:555-563): pending symbols as interleaved (I, Q), oldest
 * first, own read position.  RDS_2 only; the library keeps the last 1024. */
int  fmx_rds_symbols(fmx_handle h, int32_t channel, float *iq, int32_t capacity, int32_t *n_symbols);
/* fm-rate samples (inputRate / the reference's decimation: 12, 6 or 1) the last fmx_process_* call produced per channel: the n that fmx_get_tap accepts for the
 * fm-rate taps, and the number of entries the reference's run() pushed into its LF scope vector for the same block.  A call the library made in pieces -- with a
 * channel decoding RDS (pieces of 31999 fm samples) or as overlapping pieces (FMX_P_CALL_PIECES) -- reports its LAST piece here, and the row taps hold that piece. */
int64_t fmx_last_fm_samples(fmx_handle h);
/* Health counter of the pilot PLL (no counterpart in the reference, whose loop is sequential): stage B finds the loop's
 * trajectory of a 1536-sample segment by Newton's method on the whole segment; a segment that does not settle within the
 * round limit is replayed sample by sample by one thread -- correct, only slower.  Returns the number of such segments
 * of `channel` since fmx_create (channel < 0: summed over all channels), or a negative fmx error code. */
int64_t fmx_pll_replays(fmx_handle h, int32_t channel);
/* Segments (of up to 1536 fm samples) that FMX_P_PLL_SOLVER = 2 evaluated sequentially because the pilot was not comfortably in lock,
 * of `channel` since fmx_create (channel < 0: summed over all channels), or a negative fmx error code: what the guard costs. */
int64_t fmx_pll_exact_segments(fmx_handle h, int32_t channel);
/* Which kernel the last fmx_process_* call gave its input-filter stage to (FMX_P_FRONT_KERNEL's numbering: 1, 2 or 3; the remainder of a call
 * that is not whole 1536-sample tiles always goes to kernel 1): what a benchmark names beside its number. */
int32_t fmx_last_front_kernel(fmx_handle h);
/* ... and the number of overlapping pieces it was made in (FMX_P_CALL_PIECES; 1: the call was made whole). */
int32_t fmx_last_call_pieces(fmx_handle h);
/* ... and the channels of the SECOND of the two channel groups its stereo / audio stages ran as (0: one group).  A batch of more channels than one round of
 * the stereo stage's workgroups, without RDS, scope taps or demodulator pre-pass, runs those stages for the channels 0 .. C - n - 1 on the caller's stream and
 * for the last n on a side stream of the handle, so that the audio stage of one group fills what the stereo stage of the other leaves free; the input
 * filter stage stays one launch.  The results do not depend on it (every channel's arithmetic is its own); FMX_TAIL_SPLIT=0 in the environment switches it off. */
int32_t fmx_last_second_group(fmx_handle h);
/* ... and 24 kS/s RDS samples (rdsDecimator outputs, fm-processor.cpp:553): the n that fmx_get_tap accepts for FMX_TAP_RDS_IQ */
int64_t fmx_last_rds_samples(fmx_handle h);
/* ... of one channel.  A channel's RDS path counts the fm samples IT has processed -- it runs while the channel's decoder is on and stands still
 * otherwise, as a processor of the reference leaves its block filters, its phase delay line and its decimator alone while rdsModus is RDS_OFF
 * (fm-processor.cpp:733-754, :551-553) -- so channels that switched their decoders on at different times divide by eight on different phases
 * and a call may give one of them an output more than another.  fmx_last_rds_samples is this for channel 0. */
int64_t fmx_last_rds_samples_of(fmx_handle h, int32_t channel);

/* replaces the scanresult () signal (fm-processor.h, emitted fm-processor.cpp:489-492): the records completed since the last read, oldest first, at most
 * `capacity`; the library keeps the last 1024 per channel (a reader that fell behind sees the gap in `block`) */
int  fmx_scan_results(fmx_handle h, int32_t channel, fmx_scan_result *out, int32_t capacity, int32_t *n_results);

/* ---- the modulation meter: what a broadcast monitor reports per station -- peak deviation over 50 ms windows (ITU-R SM.1268), multiplex
 * power (the mean square of the deviation, which a host averages over 60 s for ITU-R BS.412) and pilot deviation -- as one record per channel and window,
 * computed on the GPU behind the demodulator, for one channel and for thousands alike.
 *
 * Inputs, for fm sample j of a channel (j counts the handle's fm samples since fmx_create, as the taps number them): d [j], the demodulator output, the
 * value of FMX_TAP_DEMOD (fm-processor.cpp:497), and phi [j], currentPilotPhase, the value of FMX_TAP_PILOT_PHASE (:695).
 * Window w is the fm samples [9600 w, 9600 (w + 1)), 50 ms; every channel shares the grid.  Inside a window sample i = j - 9600 w belongs to lane
 * l = i mod 64 as its step q = i div 64 (150 steps).  Each lane accumulates in step order, in f32, without contraction into fma:
 *     mx = max (mx, d) from -inf, mn = min (mn, d) from +inf, s1 += d, s2 += f32 (d d), si += f32 (d S), sq += f32 (d C)   (sums from 0)
 * with S, C the device's f32 sine and cosine (sincosf) of the f32 phi.  At the window's end the 64 lanes are combined by the butterfly
 * a [l] = a [l] op a [l xor m] for m = 32, 16, 8, 4, 2, 1, and
 *     peak_pos = mx, peak_neg = mn, mean = s1 / 9600.0f, mean_square = s2 / 9600.0f, pilot_i = si / 4800.0f, pilot_q = sq / 4800.0f.
 * A pilot a sin (phi + e) in d gives (pilot_i, pilot_q) = a (cos e, sin e): its deviation is hypot (pilot_i, pilot_q).
 * What a channel carries between calls is its 64 x 6 lane accumulators and no sample: on the same d and phi a record is the same bit for bit however
 * the stream is cut into calls, or a call into pieces, the pilot fields included.  (d and phi themselves depend on the cut in their last bits -- the RF DC
 * removal and the AFC are evaluated in tiles and segments that begin with the call; not so the PLL decoder with RF DC removal off --, and records of
 * two cuts differ by as much: DESIGN.md 4.11.)
 * Window w of a channel leaves a record only if the channel's meter was on in every call that covered one of its samples: a meter switched on in
 * mid-window starts at the next boundary, one switched off drops the window in progress; a scanning channel's meter runs on, as its chain does.
 * The device keeps the last 64 records (3.2 s) per channel.  Everything else a handle delivers -- PCM, RDS, meta, taps, peaks, scan records -- is bit for
 * bit what it is without the meter.  The rows the meter reads are handle-wide: a batch with one metered channel writes them (8 bytes per fm sample) for
 * every channel and runs as a batch that keeps them does (see fmx_last_second_group). */
typedef struct fmx_mod_record {
    int64_t index;        /* the window w; a gap means windows that were not metered or that the reader lost */
    int64_t end_sample;   /* 9600 (w + 1): the fm sample behind the window's last */
    float   peak_pos, peak_neg, mean, mean_square, pilot_i, pilot_q;      /* in the demodulator's units (fmx_mod_hz_per_unit), mean_square in their square */
} fmx_mod_record;
/* switches the meter of a channel (-1: of every channel) on or off; from any thread, takes effect at the next call */
int  fmx_mod_meter_enable(fmx_handle h, int32_t channel, int32_t on);
/* the records the channels first_channel .. first_channel + n_channels - 1 completed since this function last read them, oldest first, at most
 * capacity_per_channel each (more stay for the next read): channel k's at out [k * capacity_per_channel ..], their number in n_records [k].  One
 * read-out of the device for the whole range. */
int  fmx_mod_records(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_mod_record *out, int32_t capacity_per_channel, int32_t *n_records);
/* Hz per unit of d (host only, needs no device) for the decoders whose discriminator value is radians per sample -- 2 the PLL decoder's phase increment
 * (pllC.cpp:80-84), 3 Mixed and 4 ComplexBB (an atan2) --: res = 20 (r - afc) / K_FM, K_FM = 2 B_FM pi / F_G (fm-demodulator.cpp:58-64,198), hence
 * hz = K_FM fmRate / (40 pi) = B_FM fmRate / (20 F_G), 47 261.5 at 192 000.  FMX_E_UNSUPPORTED for 1 (AM: no frequency), 5 (RealBB: an arcsine table's
 * half angle of a sine, no linear scale) and 6 (Diff: a difference quotient, no angle). */
int  fmx_mod_hz_per_unit(int32_t decoder, int32_t fmRate, double *hz);

/* ---- the programme audio meter: what a broadcast monitor reports of the PROGRAMME -- loudness (ITU-R BS.1770-4 / EBU R 128), level,
 * silence, a lost ear, an out-of-phase stereo signal -- as one 48-byte record per channel and 100 ms window, computed on the GPU from the PCM the call
 * delivers, so that the PCM itself can stay on the device.
 *
 * Input: the channel's PCM, exactly the values the call delivers (a scanning channel's zeros included).  Frame m counts the handle's PCM frames since
 * fmx_create (fmx_meta.pcm_frames).  Window w is the frames [4800 w, 4800 (w + 1)), 100 ms, the gating step of BS.1770; every channel shares the grid.
 * Each (channel, ear) is one sequential machine, run in frame order in IEEE f32 with subnormals and without contraction into fma; its states start at
 * zero in the piece of a call that switches the meter on, as if the programme had been silent before.  Per frame, x the ear's sample:
 *     pk = max (pk, |x|)         s2 += f32 (x x)
 *     for the two K-weighting sections in turn (transposed direct form II), v = x for the first and v = the first's o for the second:
 *         o = f32 (b0 v) + t1      t1 = f32 (f32 (b1 v) - f32 (a1 o)) + t2      t2 = f32 (b2 v) - f32 (a2 o)
 *     z += f32 (o o)   (o of the second section)          left ear only: sx += f32 (xL xR)
 * with BS.1770-4's 48 kHz coefficients rounded to f32:
 *     section 1: b 1.53512485958697, -2.69169618940638, 1.19839281085285;  a1 -1.69065929318241, a2 0.73248077421585
 *     section 2: b 1.0, -2.0, 1.0;                                          a1 -1.99004745483398, a2 0.99007225036621
 * At a window's end: peak = pk, ms = s2 / 4800.0f, kms = z / 4800.0f, cross = sx / 4800.0f; pk, s2, z and sx start again at 0, the filter states run on.
 * What a channel carries between calls is 16 floats and no sample: on the same PCM the records are the same bit for bit however the stream is cut into
 * calls, or a call into pieces.  (The PCM itself depends on the cut in its last bits: DESIGN.md 4.12.)
 * Window w of a channel leaves a record only if the channel's meter was on in every piece that covered one of its frames: the filters run from the first
 * frame of the piece that switched the meter on, accumulation starts at the first window boundary at or behind it; switching off drops the window in
 * progress and the states.  The device keeps the last 64 records (6.4 s) per channel.  Everything else a handle delivers -- PCM, RDS, meta, taps, peaks,
 * scan records, modulation records, fmx_last_second_group -- is bit for bit what it is without the meter; a handle that never switches it on allocates
 * and launches nothing for it.  The coefficients are those of 48 000 frames/s: a handle with audioRate != 48000 answers FMX_E_UNSUPPORTED. */
typedef struct fmx_audio_record {
    int64_t index;        /* the window w; a gap means windows that were not metered or that the reader lost */
    int64_t end_frame;    /* 4800 (w + 1): the PCM frame behind the window's last */
    float   peak_l, peak_r;      /* the largest |sample| (sample peak, not true peak) */
    float   ms_l, ms_r;          /* mean square, unweighted */
    float   kms_l, kms_r;        /* mean square behind the K-weighting */
    float   cross;               /* mean of left x right: cross / sqrt (ms_l ms_r) is the window's correlation */
    int32_t reserved;            /* 0 */
} fmx_audio_record;
/* switches the audio meter of a channel (-1: of every channel) on or off; from any thread, takes effect at the next call */
int  fmx_audio_meter_enable(fmx_handle h, int32_t channel, int32_t on);
/* the records the channels first_channel .. first_channel + n_channels - 1 completed since this function last read them, oldest first, at most
 * capacity_per_channel each (more stay for the next read): channel k's at out [k * capacity_per_channel ..], their number in n_records [k].  One
 * read-out of the device for the whole range. */
int  fmx_audio_records(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_audio_record *out, int32_t capacity_per_channel, int32_t *n_records);
/* BS.1770-4 for two channels of weight 1 over one channel's records in order (host only, needs no device, all arithmetic in double).
 * A block is 4 records with consecutive `index` (400 ms, 75 % overlap); a gap in `index` breaks the run.  z_j is the mean of kms_l + kms_r over block j,
 * l_j = -0.691 + 10 log10 z_j.  momentary_lufs is the last 4 records' block, short_term_lufs the same over the last 30 records (3 s), both only if those
 * records are consecutive; integrated_lufs is -0.691 + 10 log10 of the mean z_j over the blocks with l_j above -70 LUFS and above the relative threshold,
 * which lies 10 LU below the level of the mean z_j of the blocks above -70 LUFS.  blocks_total counts the blocks, blocks_gated those that passed both
 * gates.  correlation is sum cross / sqrt (sum ms_l sum ms_r) over all records, 0 where the denominator is 0; peak_dbfs_* is 20 log10 of the largest peak.
 * A quantity with too few records, or of z = 0 (of a peak of 0), reads -HUGE_VAL. */
typedef struct fmx_loudness {
    double  momentary_lufs, short_term_lufs, integrated_lufs;
    double  correlation;
    double  peak_dbfs_l, peak_dbfs_r;
    int64_t blocks_total, blocks_gated;
} fmx_loudness;
int  fmx_audio_loudness(const fmx_audio_record *recs, int32_t n, fmx_loudness *out);

/* ---- the reception meter: what a monitoring receiver reports of the RECEPTION beside modulation -- RF level, a carrier-to-noise figure,
 * the envelope's modulation depth (the multipath indicator) and the frequency offset; tuner ICs call them "level / WAM / offset" -- as one 40-byte record
 * per channel and 50 ms window, computed on the GPU from the channel's fm-rate samples in front of the limiter, where the envelope still carries the noise
 * and the multipath.
 *
 * Input, for fm sample j of a channel (j counts the handle's fm samples since fmx_create, as the taps number them): v [j], the value of FMX_TAP_FM_IQ,
 * read as every reader of stage A's ring reads it -- ring position (j - delay_fm) & ring_mask, zero while j - delay_fm < 0, delay_fm the latency of the
 * channel's input filter in force in the piece that reads -- and u [j] = v [j - 1] under the same rule: the previous sample comes from the ring and is
 * never carried.
 * The grid is the modulation meter's, so that records of the two meters pair by `index`: window w is the fm samples [9600 w, 9600 (w + 1)), 50 ms; inside
 * a window sample i = j - 9600 w belongs to lane l = i mod 64 as its step q = i div 64 (150 steps).  Each lane accumulates in step order, in f32, without
 * contraction into fma; with f32 (.) one rounding:
 *     p  = f32 (f32 (v.re v.re) + f32 (v.im v.im))
 *     mx = max (mx, p) from -inf, mn = min (mn, p) from +inf, s1 += p, s2 += f32 (p p)                                    (sums from 0)
 *     cr += f32 (f32 (v.re u.re) + f32 (v.im u.im)),  ci += f32 (f32 (v.im u.re) - f32 (v.re u.im))
 * (cr, ci) is the sum of v conj (u), the autocorrelation at lag 1.  At the window's end the 64 lanes are combined by the butterfly
 * a [l] = a [l] op a [l xor m] for m = 32, 16, 8, 4, 2, 1, and
 *     p_max = mx, p_min = mn, p_mean = s1 / 9600.0f, p2_mean = s2 / 9600.0f, r1_re = cr / 9600.0f, r1_im = ci / 9600.0f.
 * What a channel carries between calls is its 64 x 6 lane accumulators and no sample: on the same ring contents a record is the same bit for bit however
 * the stream is cut into calls, or a call into pieces.  (The ring's contents themselves depend on the cut in their last bits where the RF DC removal is on:
 * it is evaluated in tiles that begin with the call)
 * Window w of a channel leaves a record only if the channel's meter was on in every piece that covered one of its samples: a meter switched on in
 * mid-window starts at the next boundary, one switched off drops the window in progress; a scanning channel's meter runs on, as its chain does.
 * The device keeps the last 64 records (3.2 s) per channel.  Everything else a handle delivers -- PCM, RDS, meta, taps, peaks, scan records, both other
 * meters' records, fmx_last_second_group, fmx_last_call_pieces, fmx_last_front_kernel -- is bit for bit, or equal to, what it is without the meter: the
 * ring is kept by every handle in every mode, so a reception meter asks nothing of a call's plan and can be on for every channel of a batch, which stays
 * the plain batch it was.  A handle that never switches it on allocates and launches nothing for it. */
typedef struct fmx_rx_record {
    int64_t index;        /* the window w; a gap means windows that were not metered or that the reader lost */
    int64_t end_sample;   /* 9600 (w + 1): the fm sample behind the window's last */
    float   p_max, p_min, p_mean, p2_mean;      /* of the power |v|^2 (full scale 1); p2_mean in its square */
    float   r1_re, r1_im;                       /* the mean of v conj (v one sample earlier) */
} fmx_rx_record;   /* 40 bytes */
/* switches the reception meter of a channel (-1: of every channel) on or off; from any thread, takes effect at the next call */
int  fmx_rx_meter_enable(fmx_handle h, int32_t channel, int32_t on);
/* the records the channels first_channel .. first_channel + n_channels - 1 completed since this function last read them, oldest first, at most
 * capacity_per_channel each (more stay for the next read): channel k's at out [k * capacity_per_channel ..], their number in n_records [k].  One
 * read-out of the device for the whole range. */
int  fmx_rx_records(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_rx_record *out, int32_t capacity_per_channel, int32_t *n_records);
/* The reception figures of one channel's records (host only, needs no device, all arithmetic in double).  With M2 the mean of p_mean and M4 the mean of
 * p2_mean over the n records:
 *   level_dbfs = 10 log10 M2 (-HUGE_VAL for M2 = 0);
 *   cnr_db     the M2M4 estimate for a carrier of constant envelope in complex Gaussian noise: S = sqrt (2 M2^2 - M4), N = M2 - S,
 *              cnr_db = 10 log10 (S / N); -HUGE_VAL where 2 M2^2 - M4 <= 0 (no carrier: the channel is noise), +HUGE_VAL where N <= 0;
 *   am_depth   the largest over the records of (sqrt p_max - sqrt p_min) / (sqrt p_max + sqrt p_min), the envelope's modulation depth; 0 for a record
 *              with p_max = 0;
 *   offset_hz  atan2 (sum r1_im, sum r1_re) fmRate / (2 pi): the power-weighted centre of the instantaneous frequency, whatever the decoder;
 *   windows    n.
 * n = 0 (or a null pointer, or fmRate < 1) gives FMX_E_INVALID. */
typedef struct fmx_rx_quality {
    double  level_dbfs, cnr_db, am_depth, offset_hz;
    int64_t windows;
} fmx_rx_quality;
int  fmx_rx_quality_of(const fmx_rx_record *recs, int32_t n, int32_t fmRate, fmx_rx_quality *out);

/* ---- the RDS meter: the RDS sub-carrier itself, in front of every slicer -- its injection level (the RDS deviation, which regulators
 * limit), its phase against the third harmonic of the pilot (IEC 62106: 0 or 90 degrees within 10) and how clean it is -- as one 40-byte record per
 * channel and window of 2560 RDS samples (106.7 ms, about 127 bits), computed on the GPU from the 24 kS/s complex baseband behind the RDS path's decimator.
 *
 * Input, for RDS sample m of a channel: z [m] = (I, Q), the value of FMX_TAP_RDS_IQ, at position m & 8191 of the channel's ring of 24 kS/s samples.  m
 * counts the channel's own 24 kS/s outputs since fmx_create -- the count fmx_last_rds_samples_of adds up -- and stands still while the channel's decoder is
 * off: channels switched on at different times have different grids, and that is intended.
 * Window w is the channel's RDS samples [2560 w, 2560 (w + 1)); inside a window sample i = m - 2560 w belongs to lane i mod 64 as its step i div 64 (40
 * steps).  Each lane accumulates in step order, in f32, without contraction into fma; with f32 (.) one rounding:
 *     ii = f32 (I I), qq = f32 (Q Q), p = f32 (ii + qq)
 *     mx = max (mx, p) from -inf, sii += ii, sqq += qq, siq += f32 (I Q), si += I, sq += Q                               (sums from 0)
 * At the window's end the 64 lanes are combined by the butterfly a [l] = a [l] op a [l xor k] for k = 32, 16, 8, 4, 2, 1, and
 *     p_max = mx, ii_mean = sii / 2560.0f, qq_mean = sqq / 2560.0f, iq_mean = siq / 2560.0f, i_mean = si / 2560.0f, q_mean = sq / 2560.0f.
 * What a channel carries between pieces is its 64 x 6 lane accumulators and no sample: on the same ring contents a record is the same bit for bit however
 * the stream is cut into calls, or a call into pieces (the pieces of at most 31 999 fm samples that calls with RDS on are made in included).
 * Window w of a channel leaves a record only if the channel's meter was on in every piece in which the channel produced one of the window's samples: a
 * meter switched on in mid-window starts at the next boundary, one switched off drops the window in progress.  A piece in which the channel's decoder is
 * off changes nothing: a window may span a pause of the decoder, as the path's own filters do.  Enabling the meter does not switch RDS on: a metered
 * channel whose decoder never runs gets no records.  The slicer (RDS_1 / 2 / 3), FMX_A_RESET_RDS and FMX_A_TRIGGER_FREQUENCY_CHANGE do not touch the
 * meter: the front end runs on, and so does the meter.  The device keeps the last 64 records (6.8 s) per channel.  Everything else a handle delivers --
 * PCM, RDS bits, groups, fmx_rds_decode_all, meta, taps, peaks, scan records, the three other meters' records, fmx_last_second_group,
 * fmx_last_call_pieces, fmx_last_front_kernel -- is bit for bit, or equal to, what it is without the meter.  A handle that never switches it on allocates
 * and launches nothing for it. */
typedef struct fmx_rds_meter_record {
    int64_t index;        /* the window w; a gap means windows that were not metered or that the reader lost */
    int64_t end_sample;   /* 2560 (w + 1), in the channel's own RDS-sample count */
    float   p_max;                                   /* the largest I I + Q Q */
    float   ii_mean, qq_mean, iq_mean, i_mean, q_mean;   /* the sums / 2560.0f */
} fmx_rds_meter_record;   /* 40 bytes */
/* switches the RDS meter of a channel (-1: of every channel) on or off; from any thread, takes effect at the next call; switches no decoder */
int  fmx_rds_meter_enable(fmx_handle h, int32_t channel, int32_t on);
/* the records the channels first_channel .. first_channel + n_channels - 1 completed since this function last read them, oldest first, at most
 * capacity_per_channel each (more stay for the next read): channel k's at out [k * capacity_per_channel ..], their number in n_records [k].  One
 * read-out of the device for the whole range. */
int  fmx_rds_meter_records(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_rds_meter_record *out, int32_t capacity_per_channel, int32_t *n_records);
/* The calibration of a channel's RDS meter, from the handle's own designed taps (computed on the host, in double; like fmx_get_taps it brings the
 * handle's tap sets up to the current settings first, and needs no call to have been made):
 *   gain        |z| per unit of sub-carrier amplitude in the demodulator output d: the real 57 kHz band-pass's response at 57 kHz (0.5000: only the
 *               real part of the complex band-pass's result is kept), times 3 (the analytic-signal filter's factor), times the magnitude of the
 *               decimator's complex DC gain (1.9459): 2.9188 at 192 kS/s;
 *   phase0_deg  the chain's constant rotation, the argument of the decimator's complex DC gain (59.08 degrees): band-pass and analytic-signal filter are
 *               linear in phase with a delay of 384 samples, whole periods of 19 and 57 kHz, and the mixer turns by minus three times the pilot's own
 *               delayed phase.  With it phase_deg below refers to the pilot as transmitted;
 *   path_57k    the static response, relative to DC, of what lies between the antenna and d for a small sub-carrier at 57 kHz: the channel's RF path
 *               (the input filter in force with the two decimators, the mean of the sidebands at +-57 kHz) times the discriminator's own response
 *               (sin x / x for the one-sample phase difference, x = pi 57000 / fmRate: 0.861).  FMX_E_UNSUPPORTED for the decoders
 *               fmx_mod_hz_per_unit refuses. */
typedef struct fmx_rds_meter_calib {
    double gain, phase0_deg, path_57k;
} fmx_rds_meter_calib;
int  fmx_rds_meter_cal(fmx_handle h, int32_t channel, fmx_rds_meter_calib *out);
/* The figures of one channel's records (host only, needs no device, all arithmetic in double).  With A, B, C, mi, mq the means over the n records of
 * ii_mean, qq_mean, iq_mean, i_mean, q_mean:  a = A - mi^2, b = B - mq^2, c = C - mi mq (the covariance of I and Q), r = hypot ((a - b) / 2, c),
 * l+ = (a + b) / 2 + r, l- = (a + b) / 2 - r (its eigenvalues), K = hz_per_unit / (gain path_57k), hz_per_unit from fmx_mod_hz_per_unit:
 *   injection_rms_hz   sqrt (max (l+ - l-, 0)) K: the power on the sub-carrier's axis above the power across it, which is booked as noise;
 *   injection_peak_hz  sqrt (max p_max) K;
 *   carrier_hz         hypot (mi, mq) K: an unmodulated 57 kHz component (ARI, or leakage);
 *   phase_deg          atan2 (2 c, a - b) / 2 in degrees, minus phase0_deg, folded into (-45, 135]: both nominal values, 0 and 90, are interior;
 *   axis_db            10 log10 (l+ / l-); +HUGE_VAL where l- <= 0; -HUGE_VAL, with phase_deg 0, where l+ <= 0;
 *   windows            n.
 * n = 0 or a null pointer gives FMX_E_INVALID.
 * What the injection figures mean: the sub-carrier as THIS chain's demodulator sees it, corrected for the static path.  The reference's two short decimators (25 taps and 3 taps: 0.869 and 0.899 at 57 kHz)
 * make the receiver selective at 57 kHz, and a programme at full deviation moves the sidebands across that slope: under programme the figure
 * reads low by what DESIGN.md 4.14 lists.  axis_db has a ceiling of its own, the unfiltered pilot PLL's jitter, tripled. */
typedef struct fmx_rds_figures {
    double  injection_rms_hz, injection_peak_hz, carrier_hz, phase_deg, axis_db;
    int64_t windows;
} fmx_rds_figures;
int  fmx_rds_meter_figures(const fmx_rds_meter_record *recs, int32_t n, const fmx_rds_meter_calib *cal, double hz_per_unit, fmx_rds_figures *out);

/* ---- The spectrum meter (nothing of the reference's: it hands these samples to its HF scope, fm-processor.cpp:417-421; contract: DESIGN.md 4.15).
 * Per metered STREAM the power spectrum of the samples the handle is fed at inputRate -- exactly the values stage A converts (all four fmx_iq_formats,
 * s16_denominator and stream_stride honoured), in front of RF DC removal, balance and oscillator -- as a mean and a max-hold per record.
 * Grid: g counts a stream's input samples since fmx_create (all streams share it).  With S = `every` (1 .. 4096) and B = `blocks_per_record`
 * (1 .. 4096), both handle-wide, block b is the samples [4096 S b, 4096 S b + 4096) -- the other 4096 (S - 1) samples of a period are not read: S = 1
 * is the band survey's gap-free grid, S = 16 costs a sixteenth -- and record r the blocks [r B, r B + B).
 * Arithmetic: the band survey's window w (periodic Hann, f64 rounded to f32), twiddles and 4096-point transform (fmx_survey.h make_window,
 * make_twiddles, pass1 .. pass3, unchanged): p_b [k] = |sum_i w [i] x [4096 S b + i] exp (-2 pi i ik / 4096)|^2, and per bin k in f32
 *     mean_r [k] = c  (p_rB [k] + p_rB+1 [k] + ... in block order, from 0),  c  = f32 (1 / (B sum w^2))        (the survey's accumulate)
 *     peak_r [k] = c1 max_b p_b [k],                                          c1 = f32 (1 / sum w^2)
 * White noise of power s^2 reads s^2 in mean; a steady carrier reads the same in both.  Bin k lies at k inputRate / 4096 Hz (k >= 2048: minus inputRate).
 * Carried between calls per metered stream: the 0 .. 4095 samples of a block in progress, the sum and the maximum per bin, nothing else: records are bit
 * for bit the same however a stream is cut into calls and a call into pieces (RDS pieces, overlapping pre-pass pieces, calls of one sample).
 * Switch: per stream, from any thread, takes effect at the next call.  A stream's first block is the first that begins at or behind the first sample of
 * the piece that switched it on; record r is delivered only if every one of its blocks was taken while the stream was on; switching off drops the
 * record in progress.  The device keeps the last 4 records per metered stream: a reader that falls behind sees a gap in `index`.
 * Everything else a handle delivers -- PCM, RDS, meta, taps, peaks, scan records, the four other meters' records, fmx_last_second_group,
 * fmx_last_call_pieces, fmx_last_front_kernel -- is bit for bit, or equal to, what it is without the meter.  A handle that never switches it on allocates
 * and launches nothing for it; memory (192 KB per stream) is allocated for the streams that are switched on. */
typedef struct fmx_spectrum_record {
    int64_t index;        /* the record r; a gap means records that were not metered or that the reader lost */
    int64_t end_sample;   /* one past the last sample read: 4096 S ((r + 1) B - 1) + 4096, in the handle's input-sample count */
    int32_t blocks;       /* B */
    int32_t every;        /* S */
} fmx_spectrum_record;   /* 24 bytes */
/* blocks per record and `every`, handle-wide (default 16, 1); only while no stream's meter is on, else FMX_E_INVALID.  Record indices and every
 * stream's read cursor start over on the new grid, and records not yet read are lost. */
int  fmx_spectrum_setup(fmx_handle h, int32_t blocks_per_record, int32_t every);
/* switches the spectrum meter of a stream (-1: of every stream) on or off; from any thread, takes effect at the next call */
int  fmx_spectrum_enable(fmx_handle h, int32_t stream, int32_t on);
/* the records of one stream completed since this function last read that stream, oldest first, at most `capacity` (more stay for the next read):
 * recs [i], mean [4096 i ..], peak [4096 i ..] (peak may be NULL).  Waits for the handle's last call only, not for the device. */
int  fmx_spectrum_read(fmx_handle h, int32_t stream, fmx_spectrum_record *recs, float *mean, float *peak, int32_t capacity, int32_t *n_records);
/* The figures of one record (host only, needs no device, every sum in double; a bin's membership in a window is decided in integers: bin kp,
 * -2048 .. 2047, lies inside |f - f0| <= d when |kp rate_hz - 4096 f0| <= 4096 d).  Bins with |f| < dc_guard_hz are left out of every sum: the meter
 * reads in front of the RF DC removal.  A quantity that cannot be formed reads -HUGE_VAL.  All frequencies in the result are relative to centre_hz.
 *   channel_db      10 log10 of the sum of mean over |f - centre| <= 100 kHz;
 *   obw_lower_hz, obw_upper_hz, obw_hz
 *                   within the span |f - centre| <= 150 kHz: the frequencies below and above which (1 - obw_fraction) / 2 of the span's power lies, a bin's
 *                   power spread evenly over its width rate_hz / 4096 (ITU-R SM.443's beta / 2 method), and their distance;
 *   xdb_hz          the distance between the outermost bins of the span whose mean lies less than x_db below the span's largest bin;
 *   centroid_hz     the power-weighted mean of f - centre over the span;
 *   adj_db [4]      for the offsets -2, -1, +1, +2 raster_hz: the power in +-100 kHz about centre + offset, minus channel_db; -HUGE_VAL where that
 *                   window leaves |f| <= rate_hz / 2 - 50 kHz;
 *   mask_margin_db, mask_worst_hz
 *                   the smallest, over the bins with |f - centre| inside [mask [0].offset_hz, mask [n_mask - 1].offset_hz], of
 *                   limit (|f - centre|) - (10 log10 (sum of peak over the bins within rbw_hz / 2 of f) - channel_db), the limit interpolated linearly in dB
 *                   between the caller's break points, and where it is found.  Negative: violated.  Formed only when peak and mask are given.
 * FMX_E_INVALID (fmx_last_error names the argument) for: struct_size; rate_hz outside [1000, 100 000 000]; |centre_hz| > rate_hz / 2; raster_hz outside
 * [50 000, 1 000 000]; dc_guard_hz outside [0, 99 999]; obw_fraction outside (0, 1); x_db not positive and finite; rbw_hz outside [1, 200 000]; a mask of
 * one point, of offsets that are negative, not finite or not ascending, or of limits that are not finite; an entry of mean or peak that is negative or
 * not finite. */
typedef struct fmx_spectrum_mask_point { double offset_hz, limit_db; } fmx_spectrum_mask_point;
typedef struct fmx_spectrum_find {
    int32_t struct_size;       /* sizeof(fmx_spectrum_find) */
    int32_t rate_hz;           /* the stream's rate: the handle's inputRate */
    int32_t centre_hz;         /* where the channel sits in the stream: its set_localOscillator value */
    int32_t raster_hz;
    int32_t dc_guard_hz;
    int32_t rbw_hz;            /* e.g. 10 000 */
    double  obw_fraction;      /* e.g. 0.99 */
    double  x_db;              /* e.g. 26 */
    const fmx_spectrum_mask_point *mask;   /* [n_mask] ascending |offset_hz|, or NULL */
    int32_t n_mask, reserved;
} fmx_spectrum_find;
typedef struct fmx_spectrum_figs {
    double channel_db, obw_hz, obw_lower_hz, obw_upper_hz, xdb_hz, centroid_hz, adj_db[4], mask_margin_db, mask_worst_hz;
} fmx_spectrum_figs;
int  fmx_spectrum_figures(const fmx_spectrum_find *cfg, const float *mean, const float *peak, fmx_spectrum_figs *out);

/* ---- The multiplex spectrum meter (the reference draws this picture for one channel on its LF scope, setlfPlotType (DEMODULATOR),
 * fm-processor.cpp:597-660; contract: DESIGN.md 4.16).  Per metered CHANNEL the power spectrum of the demodulator output d [j] at fmRate -- exactly the
 * value of FMX_TAP_DEMOD, the row stage B leaves behind (fm-processor.cpp:497) -- as a mean and a max-hold per record.
 * Grid: j counts the handle's fm samples since fmx_create, as the taps and the modulation meter count them (all channels share it).  With S = `every`
 * (1 .. 4096) and B = `blocks_per_record` (1 .. 4096), both handle-wide, block b is the fm samples [4096 S b, 4096 S b + 4096) and record r the blocks
 * [r B, r B + B).  Default B = 48, S = 1: 1.024 s at 192 kS/s.
 * Arithmetic: one block per transform, x [i] = (f32 (d [i] w [i]), 0), the band survey's window w, twiddles and 4096-point transform (fmx_survey.h,
 * unchanged).  Bins k = 0 .. 2047 are kept, bin k at k fmRate / 4096 Hz (46.875 Hz at 192 kS/s); the Nyquist bin is dropped.  Per bin in f32
 *     mean_r [k] = c  (p_rB [k] + p_rB+1 [k] + ... in block order, from 0),  c  = f32 (1 / (B sum w^2))
 *     peak_r [k] = c1 max_b p_b [k],                                          c1 = f32 (1 / sum w^2)
 * The sum of mean over bins k1 .. k2 (0 < k1) is 4096 / 2 times the power of d in that band: a line of peak amplitude A adds 4096 A^2 / 4.
 * Carried between calls per metered channel: the 0 .. 4095 samples of a block in progress and the sum and the maximum per bin, nothing else: on the same
 * d a record is bit for bit the same however the stream is cut into calls and a call into pieces.  (d itself depends on the cut in its last bits, see the
 * modulation meter above, except with the PLL decoder and RF DC removal off.)
 * Switch: per channel, from any thread, takes effect at the next call.  A channel's first block is the first that begins at or behind the first fm sample
 * of the piece that switched it on; record r is delivered only if every one of its blocks was taken while the meter was on; switching off drops the
 * record in progress.  A scanning channel's meter runs on, as its chain does.  The device keeps the last 4 records per metered channel: a reader that
 * falls behind sees a gap in `index`.
 * Rows: a metered channel needs the handle-wide rows exactly as a modulation-metered channel does: a batch with ONE metered channel writes the rows --
 * 8 bytes per fm sample -- for EVERY channel and is no plain batch (fmx_last_second_group reads as it does with the modulation meter on).  Everything
 * else a handle delivers -- PCM, RDS, meta, taps, peaks, scan records, the five other meters' records -- is bit for bit, or equal to, what it is without
 * the meter on the same handle.  A handle that never switches it on allocates and launches nothing for it; memory (96 KB per channel) is allocated for
 * the channels that are switched on. */
typedef struct fmx_mpx_record {
    int64_t index;        /* the record r; a gap means records that were not metered or that the reader lost */
    int64_t end_sample;   /* one past the last fm sample read: 4096 S ((r + 1) B - 1) + 4096 */
    int32_t blocks;       /* B */
    int32_t every;        /* S */
} fmx_mpx_record;   /* 24 bytes */
/* blocks per record and `every`, handle-wide; only while no channel's meter is on, else FMX_E_INVALID.  Record indices and every channel's read cursor
 * start over on the new grid, and records not yet read are lost. */
int  fmx_mpx_spectrum_setup(fmx_handle h, int32_t blocks_per_record, int32_t every);
/* switches the multiplex spectrum meter of a channel (-1: of every channel) on or off; from any thread, takes effect at the next call */
int  fmx_mpx_spectrum_enable(fmx_handle h, int32_t channel, int32_t on);
/* The records of channels first_channel .. first_channel + n_channels - 1 completed since this function last read each of them, oldest first, at most
 * capacity_per_channel each (more stay for the next read), in ONE read-out of the device: channel q's record i at recs [q cap + i], its bins at
 * mean [(q cap + i) 2048 ..] and peak likewise (peak may be NULL), their number in n_records [q].  Waits for the handle's last call only.  The records
 * are gathered on the device and copied once (per 4096 records of a larger range); a read that fails leaves every cursor where it was. */
int  fmx_mpx_spectrum_read(fmx_handle h, int32_t first_channel, int32_t n_channels, fmx_mpx_record *recs, float *mean, float *peak,
                           int32_t capacity_per_channel, int32_t *n_records);
/* The figures of one record (host only, needs no device, every sum in double).  Bin k, 1 .. 2047, lies in a band [lo, hi] when
 * lo 4096 <= k rate_hz <= hi 4096 (a bound that is not integral is compared after multiplying by 4096 in double); bin 0 and the bins below dc_guard_hz
 * belong to no band.  With P (band) = 2 / 4096 x the sum of mean over the band -- the power of d in it -- and u = hz_per_unit:
 *   total_hz          u sqrt P over every usable bin: the rms deviation;
 *   mono_hz           the same over [dc_guard_hz, 15 000]: L+R;
 *   stereo_hz         over [23 000, 53 000] without the window 38 000 +- line_half_hz: L-R;
 *   rds_hz            over [54 600, 59 400]: 57 kHz +- RDS_WIDTH / 2 (fm-constants.h);
 *   aux_hz            over [61 000, min (94 000, rate_hz / 2)];
 *   pilot_hz          u sqrt (2 P) over 19 000 +- line_half_hz: the PEAK deviation of a line;
 *   pilot_freq_hz     the power-weighted mean frequency over that window;
 *   carrier38_hz      u sqrt (2 P) over 38 000 +- line_half_hz;
 *   floor_hz_rt_hz    u sqrt (P / width) over the two guards [15 500, 18 500] and [19 500, 22 500], width = the number of their bins times
 *                     rate_hz / 4096: rms deviation per root hertz;
 *   pilot_cn0_db      10 log10 of the pilot window's P over the guards' P / width;
 *   band_hz [i]       u sqrt P over the caller's band i;
 *   band_line_hz [i]  the frequency of its largest mean bin;
 *   band_hold_line_hz [i], band_hold_over_mean_db [i]
 *                     the frequency of its largest peak bin, and 10 log10 of that peak bin over the same bin's mean: 0 for a steady line, large for
 *                     one that came and went.  Formed only when peak is given.
 * What cannot be formed reads -HUGE_VAL: a band without a usable bin, a band that reaches above rate_hz / 2 (aux_hz alone is cut there), a zero
 * denominator, the entries of bands the caller did not give.
 * FMX_E_INVALID (fmx_last_error names the argument) for: struct_size; rate_hz outside [8000, 1 000 000]; hz_per_unit not positive and finite;
 * dc_guard_hz outside [0, 1000]; line_half_hz outside [50, 1000]; n_bands outside [0, 16] or bands NULL with n_bands > 0; a band without
 * 0 <= lo_hz < hi_hz <= rate_hz / 2 or with a bound that is not finite; an entry of mean or peak that is negative or not finite. */
typedef struct fmx_mpx_band { double lo_hz, hi_hz; } fmx_mpx_band;
typedef struct fmx_mpx_find {
    int32_t struct_size;       /* sizeof(fmx_mpx_find) */
    int32_t rate_hz;           /* the handle's fmRate */
    double  hz_per_unit;       /* from fmx_mod_hz_per_unit, or 1.0 for the demodulator's own units */
    int32_t dc_guard_hz;       /* e.g. 30 */
    int32_t line_half_hz;      /* e.g. 250 */
    const fmx_mpx_band *bands; /* [n_bands], or NULL */
    int32_t n_bands, reserved;
} fmx_mpx_find;
typedef struct fmx_mpx_figs {
    double total_hz, mono_hz, stereo_hz, rds_hz, aux_hz, pilot_hz, pilot_freq_hz, carrier38_hz, floor_hz_rt_hz, pilot_cn0_db;
    double band_hz[16], band_line_hz[16], band_hold_line_hz[16], band_hold_over_mean_db[16];
} fmx_mpx_figs;
int  fmx_mpx_figures(const fmx_mpx_find *cfg, const float *mean, const float *peak, fmx_mpx_figs *out);

/* ---- The sub-carrier decoder (no counterpart in the reference, which stops at 59.4 kHz; contract: DESIGN.md 4.17).  Per decoding CHANNEL the audio of
 * an FM sub-carrier (SCA) at centre_hz -- 67, 76 or 82 kHz at 192 kS/s -- of the demodulator output d [j] at R = fmRate: exactly the value of
 * FMX_TAP_DEMOD, the row stage B leaves behind.  j counts the handle's fm samples since fmx_create.
 * Taps, designed in double on the host and rounded to f32, the same for every channel (fmx_sca_taps hands them out):
 *   g [0 .. 191]  the band filter: a Kaiser (beta = 7) windowed sinc with its 6 dB point at half_band_hz + 2000 at rate R, normalised to sum 1;
 *   a [0 .. 127]  the audio filter: an 81-tap Kaiser (beta = 7) low-pass with its 6 dB point at audio_cut_hz + 1300 at rate R / 4, convolved with the
 *                 first 48 values of (1 - alpha) alpha^i, alpha = exp (-4 / (R tau)) (tau = 0: the unit impulse), normalised to sum 1.  The de-emphasis
 *                 is part of this FIR: nothing recursive is carried between calls.
 * Arithmetic:
 *     y [m] = sum_k g [k] d [4 m - k] exp (-2 pi i ((centre_hz (4 m - k)) mod R) / R)          (rate R / 4)
 *     u [m] = arg (y [m] conj (y [m - 1])) R / (8 pi deviation_hz),  arg (0) = 0
 *     s [n] = sum_k a [k] u [2 n - k]                                                           (audio, rate R / 8: 24 kS/s)
 *     level [b] = the mean of |y [m]|^2 over m in [480 b, 480 b + 480)
 * The form of the f32 arithmetic: the mix is folded into per-channel complex taps c [k] = f32 (g [k] exp (+2 pi i ((centre_hz k) mod R) / R)), formed in
 * double with the phase reduced in integers; y' [m] = sum_k c [k] d [4 m - k] (fmaf, k ascending) equals y [m] up to a rotation of modulus one, so
 * |y'|^2 = |y|^2 and y [m] conj (y [m - 1]) = y' [m] conj (y' [m - 1]) rot with the one constant rot = f32 (exp (-2 pi i ((4 centre_hz) mod R) / R)) per
 * channel.  No per-sample phase exists, so the arithmetic is the same at any j, beyond 2^32 fm samples too.
 * The peak injection of the sub-carrier is 2 sqrt (level) in d's units; times fmx_mod_hz_per_unit: in Hz.
 * Blocks: block b is the audio samples [240 b, 240 b + 240); they belong to the fm samples [1920 b, 1920 b + 1920) (10 ms at 192 kS/s).  A block is a pure
 * function of d [1920 b - 703, 1920 b + 1920) (LOOKBACK = 191 + 4 x 128 = 703) and is computed when the piece that holds its last fm sample has run.
 * Carried between pieces per decoding channel: the up to 703 + 1919 samples of d not yet consumed, nothing else: on the same d a block is bit for bit the
 * same however the stream is cut into calls and a call into pieces.
 * Switch: per channel, from any thread, takes effect at the next call.  The first delivered block is the first with 1920 b - 703 >= the first fm sample of
 * the piece that switched the channel on: every delivered sample has its whole history from real d.  Switching off drops the block in progress.  A scanning
 * channel decodes on.  The device keeps the last 128 blocks (1.28 s) per channel.
 * Rows: a decoding channel needs the handle-wide rows exactly as a modulation-metered channel does (see fmx_mod_meter_enable).  Everything else a handle
 * delivers -- PCM, RDS, meta, taps, peaks, scan records, the six meters' records -- is bit for bit, or equal to, what it is on the same handle with a
 * modulation meter instead of the decoder.  A handle that never decodes allocates and launches nothing; memory (135 432 bytes per channel: 128 blocks of
 * 240 + 1 f32, the carry, the mixed taps) is allocated for the channels that are switched on. */
typedef struct fmx_sca_config {
    int32_t struct_size;       /* sizeof(fmx_sca_config) */
    int32_t half_band_hz;      /* half width of the band filter, default 9000 */
    int32_t audio_cut_hz;      /* audio low-pass cut-off, default 5000 */
    int32_t deviation_hz;      /* the deviation that maps to an output of +-1.0, default 6000 */
    int32_t deemphasis_us;     /* de-emphasis time constant, default 150; 0: none */
} fmx_sca_config;
typedef struct fmx_sca_info_t {
    int32_t audio_rate_hz;     /* fmRate / 8 */
    int32_t block_audio;       /* 240 audio samples per block */
    int32_t block_fm;          /* 1920 fm samples per block */
    int32_t lookback_fm;       /* 703 */
    double  delay_fm;          /* the linear-phase delay in fm samples: 95.5 + 4 x 40 (the de-emphasis adds its own, frequency-dependent) */
    int32_t ring_blocks;       /* 128 */
    int32_t bytes_per_channel; /* device memory per decoding channel */
} fmx_sca_info_t;
/* the setup, handle-wide (cfg NULL: the defaults); only while no channel decodes, else FMX_E_INVALID.  Blocks not yet read are lost. */
int  fmx_sca_setup(fmx_handle h, const fmx_sca_config *cfg);
/* switches the decoder of a channel (-1: of every channel) on at centre_hz, or off with centre_hz = 0; from any thread, takes effect at the next call.
 * FMX_E_INVALID unless centre_hz - half_band_hz + 2000 >= 59 400 (the pass band's lower edge may come within the filter's 2000 Hz transition of the top of
 * the RDS band: with the defaults 66 400 Hz and up) and centre_hz + half_band_hz + 2000 <= fmRate / 2 (with the defaults at 192 kS/s 85 000 Hz and down:
 * 67, 76 and 82 kHz are admitted, 92 kHz is refused); fmx_last_error says which.  At 67 kHz the filter's skirt overlaps the RDS band (54.6 .. 59.4 kHz):
 * under a programme with RDS about 0.02 rms of the output is that band. */
int  fmx_sca_enable(fmx_handle h, int32_t channel, int32_t centre_hz);
/* The consecutive blocks of channels first_channel .. first_channel + n_channels - 1 completed since this function last read each of them, oldest first,
 * at most capacity_blocks_per_channel each, in ONE read-out of the device: channel q's run begins at block first_block [q] and has n_blocks [q] blocks,
 * block i's audio at audio [(q cap + i) 240 ..], its level at level [q cap + i] (level may be NULL).  A run ends at a gap -- blocks the reader lost, or
 * that fell while the channel was off --; the rest comes with the next read, and the gap shows in first_block.  Waits for the handle's last call only.
 * A read that fails moves no cursor. */
int  fmx_sca_read(fmx_handle h, int32_t first_channel, int32_t n_channels, int64_t *first_block, float *audio, float *level,
                  int32_t capacity_blocks_per_channel, int32_t *n_blocks);
/* host only, no device: the taps a handle with that setup runs at fmRate (cfg NULL: the defaults).  which 0: g (192), 1: a (128).  Copies
 * min (capacity, count) floats to dst (dst may be NULL with capacity 0) and stores the count in *n. */
int  fmx_sca_taps(const fmx_sca_config *cfg, int32_t fmRate, int32_t which, float *dst, int32_t capacity, int32_t *n);
/* host only, no device */
int  fmx_sca_info(int32_t fmRate, fmx_sca_info_t *out);

/* ---- The monitoring feed (no counterpart in the reference; contract: DESIGN.md 4.18).  Per feeding CHANNEL 16 kS/s mono audio, the form speech-to-text,
 * music and advert recognition and logging recorders take, so that the 48 kHz stereo PCM can stay on the device.
 * Input: the feeding channel's PCM, exactly the frames the call delivers, as d_pcm holds them behind both channel groups' audio kernels, the gain
 * correction and the scan mute -- where the programme audio meter reads them.  A scanning channel's zeros are included.  Frame m counts the handle's PCM
 * frames since fmx_create (fmx_meta.pcm_frames).  A handle with audioRate != 48000 answers FMX_E_UNSUPPORTED, as the audio meter does.
 * Taps: one filter h [0 .. 143], designed in double on the host and rounded to f32, the same for every channel and every handle (fmx_feed_taps hands it
 * out): a Kaiser (beta = 8) windowed sinc with its 6 dB point at 8000 Hz at 48 000 frames/s, normalised to sum 1 -- within +-0.0006 dB up to 7 kHz,
 * -81.96 dB and below from 9 kHz (the band that folds onto 0 .. 7 kHz), sum of |h| = 2.112.
 * Arithmetic (IEEE f32, subnormals kept, no contraction other than the fmaf written here):
 *     v [m] = 0.5f * (xL [m] + xR [m])   mode 1 (one rounding: the sum);   xL [m]: mode 2;   xR [m]: mode 3
 *     y [n] = sum_k h [k] v [3 n - k]     fmaf, k ascending from an accumulator of 0.0f;  feed sample n <-> frame 3 n
 *     power [b] = the mean of y [n]^2 over n in [160 b, 160 b + 160): the products rounded to f32 and summed in one fixed tree (csrc/fmx_feed.h states it)
 * No per-sample phase and no recursion: the arithmetic is the same at any m, beyond 2^32 frames too.
 * Blocks: block b is the feed samples [160 b, 160 b + 160), 10 ms; they belong to the frames [480 b, 480 b + 480).  A block is a pure function of
 * v [480 b - 143, 480 b + 480) (LOOKBACK = 143) and is computed when the piece that holds its last frame has run.  Carried between pieces per feeding
 * channel: the up to 143 + 479 values of v not yet consumed, nothing else: on the same PCM a block is bit for bit the same however the stream is cut into
 * calls and a call into pieces.  (The PCM itself depends on the cut in its last bits: DESIGN.md 4.12.)
 * Switch: per channel, from any thread, takes effect at the next call.  The first delivered block is the first with 480 b - 143 >= the first frame of the
 * piece that switched the channel on: every delivered sample has its whole history from real PCM.  Switching off drops the block in progress and the
 * carry.  A call that finds a channel on in another mode than it runs in restarts it at that piece, as if it had been switched off and on.
 * Ring: the device keeps the last 128 blocks (1.28 s) per channel.  A handle that never feeds allocates and launches nothing; memory (84 928 bytes per
 * channel: 128 blocks of 160 + 1 f32, the carry) is allocated for the channels that are switched on.
 * Isolation: everything else a handle delivers -- PCM, RDS, meta, taps, peaks, scan records, every meter's records, SCA blocks -- is bit for bit what it
 * is without the feed. */
typedef enum { FMX_FEED_F32 = 0, FMX_FEED_S16 = 1 } fmx_feed_format;
typedef struct fmx_feed_info_t {
    int32_t rate_hz;           /* 16000 */
    int32_t block_samples;     /* 160 feed samples per block */
    int32_t block_frames;      /* 480 PCM frames per block */
    int32_t lookback_frames;   /* 143 */
    double  delay_frames;      /* the linear-phase delay in PCM frames: 71.5 */
    int32_t ring_blocks;       /* 128 */
    int32_t bytes_per_channel; /* device memory per feeding channel */
} fmx_feed_info_t;
/* switches the feed of a channel (-1: of every channel): mode 0 off, 1 (L + R) / 2, 2 left, 3 right; from any thread, takes effect at the next call.
 * FMX_E_INVALID for another mode or a channel out of range, FMX_E_UNSUPPORTED on a handle with audioRate != 48000. */
int  fmx_feed_enable(fmx_handle h, int32_t channel, int32_t mode);
/* The consecutive blocks of channels first_channel .. first_channel + n_channels - 1 completed since fmx_feed_read or fmx_feed_read_device last read each
 * of them, oldest first, at most capacity_blocks_per_channel each, in ONE read-out of the device: channel q's run begins at block first_block [q] (-1:
 * none) and has n_blocks [q] blocks; block i of channel q is at element (q cap + i) 160 of audio, its power at power [q cap + i] (power may be NULL).
 * format FMX_FEED_F32: the ring's values; FMX_FEED_S16: (int16) min (32767, max (-32768, rintf (y * 32768.0f))), round half to even, converted on the
 * device, so that two bytes per sample cross to the host.  A run ends at a gap -- blocks the reader lost, or that fell while the channel was off --; the
 * rest comes with the next read, and the gap shows in first_block.  Waits for the handle's last call only.  A read that fails -- a range outside the
 * handle's channels, a null first_block or n_blocks, a negative capacity, a capacity with a null audio or a capacity of 0 with an audio, an unknown format:
 * FMX_E_INVALID; n_channels x capacity_blocks_per_channel above 2^31 - 1 blocks: FMX_E_TOO_LARGE -- moves no cursor. */
int  fmx_feed_read(fmx_handle h, int32_t first_channel, int32_t n_channels, int64_t *first_block, void *audio, int32_t format,
                   float *power, int32_t capacity_blocks_per_channel, int32_t *n_blocks);
/* The same gather written to the caller's DEVICE buffers d_audio and d_power (d_power may be NULL), asynchronous on hip_stream (NULL: the handle's own
 * stream), with the stream rule of fmx_process_device: the gather runs behind the handle's last call and behind what hip_stream holds; what reads the
 * buffers runs on hip_stream behind it, or synchronises.  first_block and n_blocks are HOST arrays and are known on return: they come from the host's
 * tags.  A consumer on the device -- a PyTorch tensor [channels, blocks x 160] -- takes the feed without the audio ever leaving the device's memory. */
int  fmx_feed_read_device(fmx_handle h, int32_t first_channel, int32_t n_channels, int64_t *first_block, void *d_audio, int32_t format,
                          float *d_power, int32_t capacity_blocks_per_channel, int32_t *n_blocks, void *hip_stream);
/* host only, no device: the feed's 144 taps.  Copies min (capacity, 144) floats to dst (dst may be NULL with capacity 0) and stores 144 in *n. */
int  fmx_feed_taps(float *dst, int32_t capacity, int32_t *n);
/* host only, no device */
int  fmx_feed_info(fmx_feed_info_t *out);
/* the bytes of device memory the handle has allocated for the feed's rings and carries (0: it never fed) */
int64_t fmx_feed_allocated(fmx_handle h);

/* introspection used by the parity tests: the filter taps the kernels run with.
 * which: 0 front-end polyphase taps, 1 PSS low-pass, 2 audio+resampler FIR, 3 resampler alone,
 * 4 the noise squelch's two order-20 filters: [2][10] x (A1, A2, B1, B2), then the two gains (high-pass first),
 * 5 the RDS_1 decoder's constants: rdsFilter taps [21], matched filter [43], band-pass [8] x (A1, A2, B1, B2), gain */
int  fmx_get_taps(fmx_handle h, int32_t channel, int32_t which, float *dst, int32_t capacity, int32_t *n);

int  fmx_profile_enable(fmx_handle h, int32_t on);
int  fmx_profile_read(fmx_handle h, fmx_profile *out, int32_t reset);

/* ---- Stage W: wide-band ingest (no counterpart in the reference, whose device handlers deliver one station's 2 304 000 S/s; contract: DESIGN.md
 * "Stage W").  One object takes `streams` inputs at Rw = factor * 2 304 000 S/s (factor K = 2 .. 16: what a 10 - 20 MS/s receiver delivers) and
 * produces `outputs` complex f32 streams at 2 304 000 S/s -- one per station -- in exactly the layout fmx_process_device takes: every wide
 * sample is read from device memory once for all the stations of its stream.  Output m, offset f_m (integer Hz, |f_m| <= Rw / 2 - 150 000):
 *     v_m [n] = x [n] O (P_m [n]),  P_m [n] = (P_m [n - 1] - f_m) mod Rw,  O (p) = (cos, sin) (2 pi p / Rw) in f64 rounded to f32
 *                                   (the reference oscillator's integer phase, oscillator.cpp:26-35,49-58, at the wide rate; P_m starts at 0)
 *     y_m [j] = sum_{i < T} h [i] v_m [jK + K - 1 - i],  T = 16 K + 1,  h = the reference's Blackman low-pass (fir-filters.cpp:41-62) at 400 kHz
 * f32 accumulation.  The samples in front of the first call are zeros; the last T - 1 samples of every stream and every P_m carry from call to
 * call, so the outputs do not depend on how a stream is cut into calls (bit for bit).  One processing thread per object. */
typedef struct fmx_wideband_s *fmx_wideband;
typedef struct {
    int32_t struct_size;       /* sizeof(fmx_wideband_config) */
    int32_t device;            /* HIP device ordinal */
    int32_t streams;           /* wide input streams (>= 1) */
    int32_t factor;            /* K: 2 .. 16 */
    int32_t outputs;           /* stations (>= 1) */
    const int32_t *stream_of_output;  /* [outputs] */
    const int32_t *offset_hz;  /* [outputs] f_m, or NULL: all 0 */
    int32_t max_block;         /* max wide samples per stream per call, a multiple of K */
} fmx_wideband_config;
int  fmx_wideband_create(const fmx_wideband_config *cfg, fmx_wideband *out);
int  fmx_wideband_destroy(fmx_wideband w);
/* Any thread.  Takes effect at the first sample of the next call: the samples of the history were mixed with the old offset and stay so, P_m is
 * kept (never reset).  The call that applies a change waits on its stream once per changed output while the new taps are uploaded (a retune is a rare event); calls without a change
 * stay asynchronous. */
int  fmx_wideband_set_offset(fmx_wideband w, int32_t output, int32_t hz);
/* Formats and conversion rules of fmx_process_device_raw; strides in complex samples.  n_wide must be a multiple of K (else FMX_E_INVALID) and at
 * most max_block; *n_narrow = n_wide / K.  Output m at d_narrow + 2 * m * narrow_stride: what fmx_process_device takes as its d_iq with
 * stream_stride = narrow_stride -- called on the same hip_stream behind this call it needs no copy and no synchronisation.  hip_stream NULL: the
 * object's own stream, behind the work queued on HIP's default stream at the time of the call, and the default stream waits for the result. */
int  fmx_wideband_process_device_raw(fmx_wideband w, const void *d_wide, int32_t format, float s16_denominator, int64_t wide_stride, int64_t n_wide,
                                     float *d_narrow, int64_t narrow_stride, int64_t *n_narrow, void *hip_stream);
/* The same with host buffers; synchronous. */
int  fmx_wideband_process_host_raw(fmx_wideband w, const void *wide, int32_t format, float s16_denominator, int64_t wide_stride, int64_t n_wide,
                                   float *narrow, int64_t narrow_stride, int64_t *n_narrow);
/* The T = 16 K + 1 taps h for a factor (host only, needs no device); *n = T, FMX_E_TOO_LARGE when capacity < T. */
int  fmx_wideband_taps(int32_t factor, float *dst, int32_t capacity, int32_t *n);

/* ---- The band survey of a wide-band object (contract: DESIGN.md 4.9): where are the stations of a stream?  While a survey is on, every call
 * also feeds each wide stream -- the very values stage W converts -- into an averaged power spectrum on the GPU; stage W's outputs are bit for
 * bit what they are without it, and an object that never enables it allocates and launches nothing for it.
 *   blocks   survey sample 0 of a stream is the first sample of the first call behind the enable; block b = survey samples [4096 b, 4096 (b + 1)),
 *            no overlap; the 0 .. 4095 samples a call leaves over are carried, so the records do not depend on how a stream is cut into calls
 *            (bit for bit)
 *   window   w [i] = 0.5 - 0.5 cos (2 pi i / 4096), evaluated in f64, rounded to f32
 *   power    p_b [k] = |sum_i w [i] x [4096 b + i] exp (-2 pi i ik / 4096)|^2 in f32
 *   record   r covers blocks r B .. r B + B - 1 (B = blocks_per_record): P_r [k] = c * (the f32 sum of p_b [k] in block order),
 *            c = 1 / (B sum w^2) formed in f64 and rounded to f32 -- white noise of power s^2 reads s^2 in every bin.  Bin k lies at k' Rw / 4096 Hz
 *            from the stream's centre, k' = k for k < 2048 and k - 4096 otherwise.  The device keeps the last 4 records of every stream.
 * A record sees the band for B * 4096 / Rw seconds: it should span the slowest modulation one cares about (a record shorter than a period of
 * the modulating tone sees a carrier's instantaneous frequency and may put a station one raster line off).
 * Both calls below belong to the processing thread. */
/* blocks_per_record 1 .. 4096: a new survey begins at the next call (carry empty, sums zero, no records, index from 0), also while one is
 * running.  0 ends the survey; its memory stays allocated.  Other values: FMX_E_INVALID. */
int  fmx_wideband_survey_enable(fmx_wideband w, int32_t blocks_per_record);
typedef struct fmx_survey_record {
    int64_t index;       /* record number of the stream since the survey was enabled, from 0 (a gap = records dropped) */
    int64_t end_sample;  /* wide-sample index since fmx_wideband_create, one past the record's last sample */
    int32_t blocks;      /* B */
    int32_t reserved;
} fmx_survey_record;
/* The records of `stream` completed since the last read of that stream, oldest first, at most `capacity` (and at most the 4 the device keeps):
 * recs [i] and power [4096 i .. 4096 i + 4095], *n_records of them.  Waits for the object's last call only.  With the survey off, or before a
 * record is complete: FMX_OK and 0 records.  FMX_E_INVALID: stream out of range; recs or power NULL with capacity > 0. */
int  fmx_wideband_survey_read(fmx_wideband w, int32_t stream, fmx_survey_record *recs, float *power, int32_t capacity, int32_t *n_records);
/* The stations of a record (host only, needs no device; all sums in f64, a bin's membership in a window decided in integers):
 *   candidates  f_j = origin_hz + j raster_hz for every j with |f_j| <= Rw / 2 - 150 000: what fmx_wideband_set_offset accepts
 *   usable bins |f_k| >= dc_guard_hz (a zero-IF receiver's LO leak sits at bin 0)
 *   level       c_j = the mean of P over the usable bins with |f_k - f_j| <= 100 000 Hz, the whole channel
 *   floor       F = the element at index n / 10 of the n usable bins with |f_k| <= Rw / 2 - 50 000, sorted ascending; *floor_db = 10 log10 F
 *               (a lower decile of an average of B periodograms: it reads below the true noise, 3.6 dB at B = 4, 1.6 dB at B = 16)
 *   station     snr_db = 10 log10 (c_j / F) > threshold_db, and c_j >= c_j' for every earlier and c_j > c_j' for every later candidate j'
 *               with |f_j' - f_j| < 200 000
 * Stations ascending in offset_hz, level_db = 10 log10 c_j; *n_stations = the number found; FMX_E_TOO_LARGE when capacity is smaller (nothing is
 * written beyond it).  A record whose F is 0 has no stations.  FMX_E_INVALID: struct_size mismatch, factor outside 2 .. 16, raster_hz outside
 * 50 000 .. 1 000 000, |origin_hz| >= raster_hz, dc_guard_hz outside 0 .. 99 999, a power entry that is negative or not finite. */
typedef struct fmx_survey_find {
    int32_t struct_size;       /* sizeof(fmx_survey_find) */
    int32_t factor;            /* K of the stream the record is of */
    int32_t raster_hz;         /* the broadcast raster, e.g. 100 000 */
    int32_t origin_hz;         /* the offset of any raster line from the stream's centre */
    int32_t dc_guard_hz;
    float   threshold_db;
} fmx_survey_find;
typedef struct fmx_survey_station { int32_t offset_hz; float level_db, snr_db; int32_t reserved; } fmx_survey_station;
int  fmx_wideband_survey_stations(const fmx_survey_find *cfg, const float *power, fmx_survey_station *out, int32_t capacity, int32_t *n_stations,
                                  float *floor_db);

/* ---- Stage W at any receiver rate (contract: DESIGN.md 4.10): a *rate object* is a fmx_wideband created with its wide rate Rw in Hz instead of
 * a factor -- what a fixed-rate receiver (2.5, 8, 10, 12.5, 20 MS/s ...) or a recorded IQ file delivers.  Ro = 2 304 000, g = gcd (Rw, Ro),
 * L = Ro / g, M = Rw / g.
 *   accepted   Ro < Rw <= 16 Ro, Rw no multiple of Ro (those stay with `factor`: one configuration has one answer), L <= 576.  E.g. 2 400 000
 *              (24/25), 2 500 000 (576/625), 3 000 000, 6 000 000, 8 000 000 (36/125), 10 000 000 (144/625), 12 500 000 (576/3125), 20 000 000
 *              (72/625), 36 000 000 (8/125).  Everything else: FMX_E_INVALID, the text names the rule.
 *   mix        stage W's: v_m [n] = x [n] O (P_m [n]), P_m [n] = (P_m [n - 1] - f_m) mod Rw, O in f64 rounded to f32, P_m from 0 and never reset,
 *              |f_m| <= Rw / 2 - 150 000; a change takes effect at the first sample of the next call
 *   prototype  N_H = 16 M + 1 taps at the rate M Ro: tmp = the reference's Blackman low-pass (fir-filters.cpp:41-62) with
 *              f = (float) 400000 / (float) (M Ro), H [k] = f32 (tmp [k] L / sum tmp), the sum in f64
 *   outputs    output j of a stream, from its first sample: q_j = (j + 1) M - 1, n_j = q_j div L, p_j = q_j mod L,
 *              y_m [j] = sum_{i >= 0, p_j + L i < N_H} H [p_j + L i] v_m [n_j - i], f32 accumulation in tap order; zeros in front of the stream.
 *              After N samples a stream has produced floor (N L / M) outputs: a call's count differs by one from call to call.
 *   calls      n_wide = 0 is a no-op; otherwise ceil (M / L) <= n_wide <= max_block (FMX_E_INVALID / FMX_E_TOO_LARGE) and narrow_stride at least
 *              the call's count.  History and every P_m carry across calls: the outputs do not depend on how a stream is cut, bit for bit.
 * cfg->factor must be 0, cfg->max_block any value >= ceil (M / L).  fmx_wideband_set_offset, both process calls, the survey calls and
 * fmx_wideband_destroy take a rate object as they take a factor object (the survey's bins then lie at k' Rw / 4096 Hz). */
int  fmx_wideband_create_rate(const fmx_wideband_config *cfg, int32_t wide_rate_hz, fmx_wideband *out);
/* Processing thread: the outputs per station that the next call will produce for n_wide samples (a factor object: n_wide / K). */
int64_t fmx_wideband_outputs_for(fmx_wideband w, int64_t n_wide);
/* The prototype H for a rate (host only, needs no device); *n = 16 M + 1, *L_out and *M_out the ratio (each may be NULL); FMX_E_TOO_LARGE when
 * capacity is smaller (n, L_out, M_out are still set). */
int  fmx_wideband_rate_taps(int32_t wide_rate_hz, float *dst, int32_t capacity, int32_t *n, int32_t *L_out, int32_t *M_out);
/* fmx_wideband_survey_stations for a record of a stream at wide_rate_hz (an accepted rate); cfg->factor must be 0. */
int  fmx_wideband_survey_stations_rate(const fmx_survey_find *cfg, int32_t wide_rate_hz, const float *power, fmx_survey_station *out, int32_t capacity,
                                       int32_t *n_stations, float *floor_db);

#ifdef __cplusplus
}
#endif
#endif

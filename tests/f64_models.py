"""Plain float64 models of stage C (audio low-pass, gain, 192 -> 48 kS/s resampler, start-up fade), of the second converter
and of the RDS front end (band-pass, Hilbert filter, mix with three times the delayed pilot phase, 11-tap decimator by 8), for
frame-by-frame comparisons: numpy only, direct or f64-FFT convolution.  A helper module (not a conftest): tests/test_f64_models_cpu.py
checks the models against the oracle, tests/test_gpu_worst_sample.py checks the kernels against the models.

Every model takes the f32 samples the stage under test read (a tap of the chain) and evaluates the same operation in float64: what
happens upstream of the tap -- atan-table index flips, lock instants, the input filter's rounding -- is common to both sides and drops out.

Frame and sample numbering (oracle/fm_oracle.c process_block; fmx_api.hip frames_geom):
  * fm samples j = 0, 1, ... at fmRate (192 kS/s); a call of the library covers j in [J0, J1) and delivers the PCM frames
    m in [48 (J0 div 192), 48 (J1 div 192)): the reference's converter hands 192 samples at a time to its resampler (:1559).
  * PCM frame m is the resampler's output whose newest input is fm sample 4 m + 3 (resampler_push).
  * the overlap-add audio filter (8192 points, 756 taps) answers 8192 - 756 = 7436 samples late (fmo_fftfilter_pass_c returns the
    block before); with the audio filter off there is no such delay and the filter is the 128-tap resampler alone.
"""
import ctypes as C

import numpy as np

FM_BLOCK = 192                 # fm samples the converter collects before it runs the resampler (fmRate / 1000)
AUDIO_TAPS = 756               # fm-processor.cpp:76
AUDIO_DELAY = 8192 - 756       # overlap-add latency of the audio filter
RS_TAPS = 128
FADE_FRAMES = 24000            # workingRate / 2 (fm_oracle.c suppressMax)
RDS_FFT = 2 * 16384            # FFT_SIZE_RDS
RDS_DEGREE = 2 * 384           # PILOTFILTER_SIZE
RDS_BLOCK = RDS_FFT - RDS_DEGREE            # 32000: samples per block of the two RDS overlap-add filters
RDS_SAMPLE_DELAY = 2 * RDS_BLOCK            # 64000
RDS_WIDTH = 2 * 2400
C_TILE = 256                   # frames per tile of audio_fft_kernel
C_BLOCK = 7 * C_TILE           # frames per workgroup of audio_fft_kernel (1792)


# ------------------------------------------------------------------------------------------------ convolution
def fftconv(x, h):
    """Full linear convolution of x [n] or [n, k] (along axis 0) with the real or complex taps h, in float64 / complex128."""
    x = np.asarray(x)
    h = np.asarray(h)
    cplx = np.iscomplexobj(x) or np.iscomplexobj(h)
    x = x.astype(np.complex128 if cplx else np.float64)
    h = h.astype(np.complex128 if np.iscomplexobj(h) else np.float64)
    n = x.shape[0] + h.shape[0] - 1
    if x.shape[0] == 0:
        return np.zeros((0,) + x.shape[1:], x.dtype)
    if x.shape[0] * h.shape[0] <= 1 << 16:       # short: direct
        if x.ndim == 1:
            return np.convolve(x, h)
        return np.stack([np.convolve(x[:, k], h) for k in range(x.shape[1])], axis=1)
    nfft = 1 << int(np.ceil(np.log2(n)))
    hs = h.reshape((-1,) + (1,) * (x.ndim - 1))
    if cplx:
        return np.fft.ifft(np.fft.fft(x, nfft, axis=0) * np.fft.fft(hs, nfft, axis=0), axis=0)[:n]
    return np.fft.irfft(np.fft.rfft(x, nfft, axis=0) * np.fft.rfft(hs, nfft, axis=0), nfft, axis=0)[:n]


def delayed(y, delay, n):
    """y delayed by `delay` samples, n samples of it (zeros in front of the stream)."""
    out = np.zeros((n,) + y.shape[1:], y.dtype)
    k = min(n - delay, y.shape[0])
    if k > 0:
        out[delay:delay + k] = y[:k]
    return out


# ------------------------------------------------------------------------------------------------ stage C
def gain_lr(volume_db, balance):
    """(volumeFactor * leftChannel, volumeFactor * rightChannel) in f32 as fm_oracle.c:1276-1279, 1553 forms them."""
    vf = np.power(np.float32(10.0), np.float32(volume_db) / np.float32(20.0), dtype=np.float32)
    lc = np.float32((100 - balance) / 100.0) if balance > 0 else np.float32(1.0)
    rc = np.float32((100 + balance) / 100.0) if balance < 0 else np.float32(1.0)
    return np.array([np.float32(vf * lc), np.float32(vf * rc)], np.float32)


def fade(m, start=0):
    """The f32 start-up ramp of fm_oracle.c:1564-1566 for the frame numbers m (an array): frame `start` is the first faded one."""
    m = np.asarray(m, np.int64)
    since = m - start
    cnt = (FADE_FRAMES - since).astype(np.float32)
    f = (np.float32(FADE_FRAMES) - cnt) / np.float32(FADE_FRAMES)
    return np.where((since >= 0) & (since < FADE_FRAMES), f, np.float32(1.0)).astype(np.float64)


def frames_of(j_total):
    """PCM frames the chain has delivered once it has taken j_total fm samples."""
    return 48 * (j_total // FM_BLOCK)


def decimate_at(y, offset, m0, m1):
    """y[4 m + 3 - offset] for m in [m0, m1) (zero where the index lies in front of the stream); y a full convolution."""
    idx = 4 * np.arange(m0, m1, dtype=np.int64) + 3 - offset
    out = np.zeros((m1 - m0,) + y.shape[1:], y.dtype)
    ok = (idx >= 0) & (idx < y.shape[0])
    out[ok] = y[idx[ok]]
    return out


def stage_c_folded(x, g, gain, lf_on=True, m0=0, m1=None, fade_start=0):
    """pcm[m] = fade(m) gain_LR sum_k g[k] x[4 m + 3 - delay - k]: x the concatenated pre-resampler stream [n, 2] (f32), g the
    folded taps (the library's fmx_get_taps 2: low-pass * resampler, <= 883; the resampler alone with the audio filter off),
    delay = 7436 with the audio filter on, 0 without."""
    x = np.asarray(x)
    if m1 is None:
        m1 = frames_of(x.shape[0])
    y = fftconv(x, np.asarray(g, np.float64))
    p = decimate_at(y, AUDIO_DELAY if lf_on else 0, m0, m1)
    return p * np.asarray(gain, np.float64)[None, :] * fade(np.arange(m0, m1), fade_start)[:, None]


def stage_c_two_step(x, lowpass, rs, gain_of_sample, m0=0, m1=None, fade_start=0):
    """The reference's order (fm-processor.cpp:589-647): the audio low-pass (`lowpass` = its 756 taps, None = filter off), then the
    gain applied per fm sample (gain_of_sample: [n, 2], or [2] for a constant one), then the resampler `rs` at 4 m + 3, then the fade.
    A gain that changes between two calls is a gain_of_sample that steps at the call's first fm sample."""
    x = np.asarray(x)
    n = x.shape[0]
    if m1 is None:
        m1 = frames_of(n)
    a = x.astype(np.float64) if lowpass is None else delayed(fftconv(x, np.asarray(lowpass, np.float64)), AUDIO_DELAY, n)
    gs = np.asarray(gain_of_sample, np.float64)
    b = a * (gs[None, :] if gs.ndim == 1 else gs)
    p = decimate_at(fftconv(b, np.asarray(rs, np.float64)), 0, m0, m1)
    return p * fade(np.arange(m0, m1), fade_start)[:, None]


def gain_steps(n, j_starts, gains):
    """[n, 2] gain per fm sample: gains[i] from fm sample j_starts[i] on (j_starts[0] = 0)."""
    out = np.zeros((n, 2), np.float64)
    for j, g in zip(j_starts, gains):
        out[j:] = np.asarray(g, np.float64)[None, :]
    return out


# ------------------------------------------------------------------------------------------------ second converter
def conv2_design(L, in_rate, out_rate):
    """(p, q, taps [p, nt]) of fmo_conv2_design (L = oracle_lib.oracle ())."""
    p, q, nt = C.c_int32(), C.c_int32(), C.c_int32()
    rc = L.fmo_conv2_design(in_rate, out_rate, C.byref(p), C.byref(q), C.byref(nt), None)
    assert rc == 0, (in_rate, out_rate)
    taps = np.zeros((p.value, nt.value), np.float32)
    L.fmo_conv2_design(in_rate, out_rate, C.byref(p), C.byref(q), C.byref(nt), taps.ctypes.data_as(C.POINTER(C.c_float)))
    return p.value, q.value, taps


def conv2_count(frames_in, p, q):
    """Output frames once frames_in 48 kHz frames went in: the m with m q < frames_in p (conv2_push)."""
    return (frames_in * p + q - 1) // q


def conv2(x48, p, q, taps):
    """out[m] = sum_k taps[(m q) mod p][k] x48[floor (m q / p) - k] for every m whose newest input exists; x48 [n, 2] float64."""
    x48 = np.asarray(x48, np.float64)
    nt = taps.shape[1]
    m = np.arange(conv2_count(x48.shape[0], p, q), dtype=np.int64)
    n0, ph = (m * q) // p, (m * q) % p
    xp = np.concatenate([np.zeros((nt,) + x48.shape[1:]), x48])
    t = np.asarray(taps, np.float64)[ph]                     # [m, nt]
    out = np.zeros((m.size,) + x48.shape[1:])
    for k in range(nt):
        out += t[:, k, None] * xp[n0 - k + nt]
    return out


# ------------------------------------------------------------------------------------------------ RDS front end
def rds_tables(L, fm_rate=192000):
    """The coefficients of the RDS front end as the oracle designs them: (band-pass [768] complex, decimator [11] complex)."""
    fp = C.POINTER(C.c_float)
    bp = np.zeros((RDS_DEGREE, 2), np.float32)
    L.fmo_bandpass_kernel(RDS_DEGREE, 3 * 19000 - RDS_WIDTH // 2, 3 * 19000 + RDS_WIDTH // 2, fm_rate, bp.ctypes.data_as(fp))
    dk = np.zeros((11, 2), np.float32)
    L.fmo_decim_kernel(11, 24000 // 2, fm_rate, dk.ctypes.data_as(fp))
    return bp[:, 0].astype(np.float64) + 1j * bp[:, 1], dk[:, 0].astype(np.float64) + 1j * dk[:, 1]


def hilbert_blocks(x):
    """The reference's Hilbert "filter" (fft-filters.cpp:177-201 + Pass): NOT a convolution -- every block of 32000 samples is
    zero-padded to 32768 points, its negative frequencies are removed, and the 768 points behind the block are added to the head
    of the next one; the answer comes one block late.  x real or complex [n]; returns complex [n]."""
    n = x.shape[0]
    mask = np.zeros(RDS_FFT)
    mask[0] = 1.0; mask[1:RDS_FFT // 2] = 2.0; mask[RDS_FFT // 2] = 1.0
    out = np.zeros(n, np.complex128)
    over = np.zeros(RDS_DEGREE, np.complex128)
    for b in range(n // RDS_BLOCK):
        a = np.zeros(RDS_FFT, np.complex128)
        a[:RDS_BLOCK] = x[b * RDS_BLOCK:(b + 1) * RDS_BLOCK]
        c = np.fft.ifft(np.fft.fft(a) * mask)
        c[:RDS_DEGREE] += over
        over = c[RDS_BLOCK:].copy()
        k = min(RDS_BLOCK, n - (b + 1) * RDS_BLOCK)
        out[(b + 1) * RDS_BLOCK:(b + 1) * RDS_BLOCK + k] = c[:k]
    return out


def rds_front(demod, pilot_phase, bp, dk):
    """The 24 kS/s complex RDS baseband of fm_oracle.c process_signal_with_rds / process_block from the samples the path has seen
    since its decoder was switched on: demod, pilot_phase f32 [n].
      bpo[n]  = 3 Re sum_i bp[i] demod[n - 32000 - i]                   (real overlap-add pass: x 3, fft-filters.cpp:104-125)
      hil     = hilbert_blocks (bpo)                                     (another 32000 late)
      osc[n]  = exp (-j 3 phase[n - 64000]), the product 3 * phase formed in f32 (:1402); the reference takes cos / sin of libm
                here, not its table (fm-processor.cpp:748-753), so the model takes float64 cos / sin of that f32 argument
      out[m]  = sum_i dk[i] (osc hil)[8 m + 7 - i]
    """
    demod = np.asarray(demod, np.float32)
    n = demod.shape[0]
    bpo = 3.0 * delayed(fftconv(demod, bp.real), RDS_BLOCK, n)          # real input: the real part of the output needs Re bp only
    hil = hilbert_blocks(bpo)
    ph = np.zeros(n, np.float32)
    if n > RDS_SAMPLE_DELAY:
        ph[RDS_SAMPLE_DELAY:] = np.asarray(pilot_phase, np.float32)[:n - RDS_SAMPLE_DELAY]
    th = (np.float32(3.0) * ph).astype(np.float64)
    mixed = (np.cos(th) - 1j * np.sin(th)) * hil
    y = fftconv(mixed, dk)
    return y[8 * np.arange(n // 8, dtype=np.int64) + 7]


# ------------------------------------------------------------------------------------------------ comparison
class Worst:
    """Result of compare (): worst frame, where it is, rms and scale."""

    def __init__(self, worst, index, rms, scale, lane, call_starts):
        self.worst, self.index, self.rms, self.scale, self.lane = worst, index, rms, scale, lane
        self.mod256, self.mod1792 = index % C_TILE, index % C_BLOCK
        cs = np.asarray(call_starts if call_starts is not None and len(call_starts) else [0], np.int64)
        k = int(np.searchsorted(cs, index, side="right") - 1)
        self.call = max(k, 0)
        self.from_call_start = int(index - cs[self.call])
        self.in_call_mod256, self.in_call_mod1792 = self.from_call_start % C_TILE, self.from_call_start % C_BLOCK
        self.rel = worst / scale if scale > 0 else float("inf")

    def __str__(self):
        return ("worst %.3e (%.3e of the peak %.3f) at frame %d [%s]: mod 256 = %d, mod 1792 = %d; call %d, frame %d of it "
                "(mod 256 = %d, mod 1792 = %d); rms %.3e" % (self.worst, self.rel, self.scale, self.index, "LR"[self.lane] if self.lane < 2 else self.lane,
                                                            self.mod256, self.mod1792, self.call, self.from_call_start, self.in_call_mod256,
                                                            self.in_call_mod1792, self.rms))


def compare(got, ref, call_starts=None):
    """Frame-by-frame distance of `got` (the f32 output under test, [n] complex or [n, k]) to `ref` (the float64 model): the worst
    frame, its index (also modulo the 256-frame tile and the 1792-frame block of audio_fft_kernel, both in the stream's numbering and
    counted from the first frame of the call it lies in -- call_starts: first frame of every call), the rms and the scale (largest
    |ref|)."""
    g = np.asarray(got)
    r = np.asarray(ref)
    if np.iscomplexobj(g) or np.iscomplexobj(r):
        g = np.stack([g.real, g.imag], axis=1); r = np.stack([r.real, r.imag], axis=1)
    g = g.astype(np.float64).reshape(g.shape[0], -1)
    r = r.astype(np.float64).reshape(r.shape[0], -1)
    assert g.shape == r.shape and g.shape[0] > 0, (g.shape, r.shape)
    e = np.abs(g - r)
    i, lane = np.unravel_index(int(np.argmax(e)), e.shape)
    return Worst(float(e[i, lane]), int(i), float(np.sqrt(np.mean(e ** 2))), float(np.abs(r).max()), int(lane), call_starts)


def check(w, bound, what=""):
    """The worst-frame assertion: the worst frame within `bound` of the reference's peak."""
    assert w.scale > 0 and w.rel <= bound, "%s: worst frame %.3e of the peak exceeds the bound %.3e -- %s" % (what, w.rel, bound, w)


# ------------------------------------------------------------------------------------------------ the reference's own distance
# Worst frame of the oracle's f32 arithmetic against the float64 models above on identical inputs, relative to the output's peak: measured
# on the CPU by tests/test_f64_models_cpu.py, which prints each figure and fails when one leaves its record (so the records cannot drift
# or be inflated).  The GPU bounds are derived from these and from nothing else.
REF_RESAMPLER_WORST = 8.02e-7      # oracle resampler + fade against the model, configs[1] over 1 s (2.8e-7 at a peak of 0.35)
REF_STAGE_C_WORST = 1.21e-6       # oracle overlap-add audio filter (8192 points, 756 taps, f32) + f32 resampler against the folded model, 3 s
REF_CONV2_WORST = 5.84e-7         # oracle second converter against the model on the oracle's own 48 kHz frames, worst of 44100 / 96000 / 32000
REF_RDS_WORST = 1.06e-6           # oracle TAP_RDS_IQ against rds_front on the oracle's TAP_DEMOD / TAP_PILOT, 2.3 s with RDS at 0.05

STAGE_C_BOUND = 2.0 * REF_STAGE_C_WORST                  # the library: the same method with shorter transforms; 2 for another summation order
CONV2_BOUND = STAGE_C_BOUND + REF_CONV2_WORST            # stage C's figure plus the converter's own
RDS_BOUND = 2.0 * REF_RDS_WORST
PCM_RMS_TOL = 1e-5                                       # the suite's RMS bar (BASELINE.json north_star), for the seeded-glitch checks

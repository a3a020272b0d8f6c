"""Float64 model of the multiplex spectrum meter (include/fmx.h fmx_mpx_*), its plain f32 restatement, the comparison's signal and
measure, and the signals of the figure tests.

    block b = fm samples [N S b, N S b + N), N = 4096;  w and c = f32(1 / (B sum w^2)) are the band survey's (survey_model)
    p_b[k] = |sum_i w[i] d[N S b + i] exp(-2 pi i ik / N)|^2,  k = 0 .. 2047 (d is real; the Nyquist bin is dropped)
    record r: mean_r[k] = c sum_{b = rB .. rB + B - 1} p_b[k] in block order,  peak_r[k] = c1 max_b p_b[k],  c1 = f32(1 / sum w^2)

`records64` holds the window and the two scales as the contract states them (rounded to f32) and everything else in f64.  `records32` is the plain
restatement: survey_model's window multiply and radix-2 complex64 transform of (d w, 0), the sequential f32 sum and the running f32 maximum.

The measure.  The demodulator output of a tone signal spans 128 dB between the strongest and the weakest bin of a block: a per-bin relative bound is a
lottery there.  The comparisons use a noise-like multiplex (noise_mpx) and the error
    |got - P64| / max (P64, sqrt (P64 x mean of P64 over the record))
-- the relative error for bins above the record's mean, the error against the geometric mean below, which is what an f32 transform's absolute error
in X[k] amounts to.  The bound is survey_model's rule under that measure: every bin within 2 x the worst bin of the f32 restatements, the median
within 2 x theirs."""
import numpy as np

import spec_model as pm
import survey_model as sm

N = sm.N
BINS = N // 2
RING = 4
FM_RATE = 192000


def block_powers64(d, S=1):
    g = pm.gather(np.asarray(d, np.float64), S)
    X = np.fft.rfft(g * sm.window().astype(np.float64), axis=1)[:, :BINS]
    return X.real ** 2 + X.imag ** 2


def block_powers32(d, S=1, bins=BINS):
    g = pm.gather(np.asarray(d, np.float64), S).astype(np.float32)
    if g.shape[0] == 0:
        return np.zeros((0, bins), np.float32)
    X = sm._fft32((g * sm.window()).astype(np.complex64))[:, :bins]
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    return re * re + im * im


def records64(d, B, S=1, first=0):
    """d: real (exact f32 values), one channel from fm sample 0 -> (indices, mean [records, 2048], peak [records, 2048]) in float64."""
    p = block_powers64(d, S)
    idx = pm.deliverable(p.shape[0], B, first)
    c, c1 = float(sm.record_scale(B)), float(sm.record_scale(1))
    mean = np.stack([p[r * B:(r + 1) * B].sum(axis=0) * c for r in idx]) if idx else np.zeros((0, BINS))
    peak = np.stack([p[r * B:(r + 1) * B].max(axis=0) * c1 for r in idx]) if idx else np.zeros((0, BINS))
    return idx, mean, peak


def records_from_powers32(p, B, first=0):
    p = np.asarray(p, np.float32)
    idx = pm.deliverable(p.shape[0], B, first)
    c, c1 = sm.record_scale(B), sm.record_scale(1)
    mean, peak = np.zeros((len(idx), p.shape[1]), np.float32), np.zeros((len(idx), p.shape[1]), np.float32)
    for i, r in enumerate(idx):
        s, m = np.zeros(p.shape[1], np.float32), np.zeros(p.shape[1], np.float32)
        for b in range(r * B, (r + 1) * B):
            s = s + p[b]
            m = np.maximum(m, p[b])
        mean[i], peak[i] = s * c, m * c1
    return idx, mean, peak


def records32(d, B, S=1, first=0):
    return records_from_powers32(block_powers32(d, S), B, first)


# ---- the measure and the bound -------------------------------------------------------------------------------------------------------------
def bin_errors(P, P64):
    """[records, bins] each -> the errors of all bins, flat"""
    P, P64 = np.asarray(P, np.float64), np.asarray(P64, np.float64)
    assert P.shape == P64.shape and P.ndim == 2 and P.shape[0] > 0, (P.shape, P64.shape)
    den = np.maximum(P64, np.sqrt(P64 * P64.mean(axis=1, keepdims=True)))
    assert np.all(den > 0)
    e = np.abs(P - P64) / den
    e[~np.isfinite(e)] = np.inf
    return e.reshape(-1)


def levels(P64, *restatements):
    errs = [bin_errors(r, P64) for r in restatements]
    return max(float(e.max()) for e in errs), max(float(np.median(e)) for e in errs)


def check(tag, got, P64, level_worst, level_median, quiet=False):
    """every bin within 2 x level_worst, the median within 2 x level_median -> (passed, worst ratio, median ratio)"""
    if np.asarray(got).shape != np.asarray(P64).shape:
        if not quiet:
            print("[%s] shapes differ: %s against %s" % (tag, np.asarray(got).shape, np.asarray(P64).shape))
        return False, np.inf, np.inf
    e = bin_errors(got, P64)
    rw, rm = float(e.max()) / level_worst, float(np.median(e)) / level_median
    if not quiet:
        print("[%s] worst bin %.3e (level %.3e, ratio %.2f, bound 2), median %.3e (level %.3e, ratio %.2f, bound 2)"
              % (tag, float(e.max()), level_worst, rw, float(np.median(e)), level_median, rm))
    return rw <= 2.0 and rm <= 2.0, rw, rm


def span_db(P64):
    """the largest over the records of 10 log10 (strongest bin / weakest bin)"""
    P64 = np.asarray(P64, np.float64)
    return float(np.max(10 * np.log10(P64.max(axis=1) / P64.min(axis=1))))


# ---- the comparison's signal ------------------------------------------------------------------------------------------------------------------
def envelope(n_fm):
    b = np.arange(n_fm) // N
    return 0.4 + 0.6 * ((7 * b + 3) % 5) / 4.0


def noise_mpx(n_fm, seed=0, rms_hz=8000.0, oversample=1):
    """The noise-like multiplex in Hz at oversample * 192 kS/s: white Gaussian noise band-limited to 96 kHz, rms deviation rms_hz, times an amplitude
    envelope 0.4 + 0.6 ((7 b + 3) mod 5) / 4 per block b of 4096 fm samples, so that a dropped or swapped block shows."""
    rng = np.random.default_rng(seed)
    n = n_fm * oversample
    m = rng.standard_normal(n)
    if oversample > 1:
        X = np.fft.rfft(m)
        X[np.fft.rfftfreq(n, 1.0 / (FM_RATE * oversample)) > 96000.0] = 0.0
        m = np.fft.irfft(X, n)
    m *= rms_hz / np.sqrt(np.mean(m * m))
    return m * np.repeat(envelope(n_fm), oversample)


def fm_iq(m_hz, rate, amp=0.5):
    """m (Hz) frequency-modulated in float64 onto a carrier at 0 Hz of the given amplitude -> complex64"""
    ph = 2 * np.pi * np.cumsum(np.asarray(m_hz, np.float64)) / rate
    return (amp * np.exp(1j * ph)).astype(np.complex64)


def cpu_signal(seed=0):
    """d for the CPU comparisons: the noise-like multiplex at 192 kS/s, 10 blocks and 100 fm samples, in units of 75 kHz, as exact f32 values"""
    return (noise_mpx(10 * N + 100, seed) / 75000.0).astype(np.float32)


# ---- signals of the figure tests: d in Hz at 192 kS/s ------------------------------------------------------------------------------------------
def band_noise(n, lo_hz, hi_hz, rms, seed, rate=FM_RATE):
    """Gaussian noise confined to [lo_hz, hi_hz] with the given rms"""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / rate)
    X[(f < lo_hz) | (f > hi_hz)] = 0.0
    m = np.fft.irfft(X, n)
    return m * (rms / np.sqrt(np.mean(m * m)))


def tone(n, f_hz, peak, phase=0.3, rate=FM_RATE):
    return peak * np.cos(2 * np.pi * f_hz * np.arange(n) / rate + phase)


def record_of(d, B=48):
    """(mean, peak) f32 of the first record of d, as the float64 model makes it"""
    d = np.asarray(d, np.float32).astype(np.float64)
    _, mean, peak = records64(d[:N * B], B)
    return mean[0].astype(np.float32), peak[0].astype(np.float32)

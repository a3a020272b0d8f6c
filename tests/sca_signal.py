"""Signals for the sub-carrier decoder's tests, in numpy, float64: a multiplex in Hz of deviation at any sample rate -- programme (band-
limited noise in L+R and L-R, a pilot, an RDS band) and an FM sub-carrier (SCA) carrying a tone --, the same frequency-modulated onto a carrier for the
GPU tests, and what the decoder's output must then hold."""
import numpy as np

FM_RATE = 192000
UNIT_HZ = 75000.0             # the CPU tests' d is the multiplex in units of 75 kHz


def band_noise(n, lo_hz, hi_hz, rms, rng, rate):
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / rate)
    X[(f < lo_hz) | (f > hi_hz)] = 0.0
    m = np.fft.irfft(X, n)
    return m * (rms / np.sqrt(np.mean(m * m)))


def programme(n, rate=FM_RATE, seed=1):
    """band-limited noise of 15 kHz rms in L+R (30 Hz .. 15 kHz) and 10 kHz rms in L-R (23 .. 53 kHz), a 7500 Hz pilot, an RDS band (54.6 .. 59.4 kHz) of
    2000 Hz rms: Hz of deviation, numpy seed `seed`"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    return (band_noise(n, 30.0, 15000.0, 15000.0, rng, rate) + band_noise(n, 23000.0, 53000.0, 10000.0, rng, rate)
            + 7500.0 * np.cos(2 * np.pi * 19000.0 * t + 0.4) + band_noise(n, 54600.0, 59400.0, 2000.0, rng, rate))


def sca(n, rate=FM_RATE, centre_hz=67000, injection_hz=7500.0, tone_hz=1000.0, deviation_hz=6000.0, first=0):
    """the sub-carrier: injection_hz cos (2 pi centre t + (deviation / tone) sin (2 pi tone t)), t = (first + i) / rate: a tone_hz tone at +-deviation_hz"""
    t = (first + np.arange(n)) / rate
    return injection_hz * np.cos(2 * np.pi * centre_hz * t + (deviation_hz / tone_hz) * np.sin(2 * np.pi * tone_hz * t))


def multiplex(n, rate=FM_RATE, with_programme=True, seed=1, **sca_kw):
    """the comparison signal in Hz of deviation: the sub-carrier, under the programme or alone"""
    m = sca(n, rate, **sca_kw)
    return m + programme(n, rate, seed) if with_programme else m


def cpu_signal(n=12 * 1920 + 100, **kw):
    """d for the CPU comparisons: the multiplex at 192 kS/s in units of 75 kHz, as exact f32 values"""
    return (multiplex(n, FM_RATE, **kw) / UNIT_HZ).astype(np.float32)


def fm_iq(m_hz, rate, amp=0.5):
    """m (Hz) frequency-modulated in float64 onto a carrier at 0 Hz of the given amplitude -> [n, 2] f32"""
    ph = 2 * np.pi * np.cumsum(np.asarray(m_hz, np.float64)) / rate
    return np.ascontiguousarray((amp * np.exp(1j * ph)).astype(np.complex64).view(np.float32).reshape(-1, 2))


def tone_fit(s, tone_hz, rate):
    """least squares of s against cos and sin of tone_hz and a constant -> (amplitude, rms of the residual)"""
    t = np.arange(len(s)) / rate
    A = np.stack([np.cos(2 * np.pi * tone_hz * t), np.sin(2 * np.pi * tone_hz * t), np.ones(len(s))], axis=1)
    x, *_ = np.linalg.lstsq(A, np.asarray(s, np.float64), rcond=None)
    return float(np.hypot(x[0], x[1])), float(np.sqrt(np.mean((s - A @ x) ** 2)))

"""Float64 model of stage W, the wide-band ingest stage (DESIGN.md "Stage W"; include/fmx.h fmx_wideband).  One model = one wide stream.

    Rw = K * 2 304 000,  T = 16 K + 1,  h = the reference's Blackman low-pass (fir-filters.cpp:41-62) with 400 kHz at Rw, unit sum, f32 taps
    v_m[n] = x[n] O(P_m[n]),  P_m[n] = (P_m[n-1] - f_m) mod Rw,  O(p) = (cos, sin)(2 pi p / Rw) evaluated in f64 and rounded to f32
    y_m[j] = sum_{i<T} h[i] v_m[jK + K-1 - i]

P_m starts at 0 and is never reset; an offset change takes effect at the first sample of the next call, the samples already mixed stay as
they are.  `process` sums in float64; with_f32 it also restates the same arithmetic in float32 (taps, samples and oscillator in f32, the mix
as four products, accumulation in tap order): the yardstick a GPU implementation's error is set against (ask for it in every call of a
model or in none: it keeps a history of its own)."""
import math

import numpy as np

NARROW_RATE = 2304000
CUTOFF = 400000
GUARD = 150000


def n_taps(K):
    return 16 * K + 1


def offset_limit(K):
    return K * NARROW_RATE // 2 - GUARD


def taps(K):
    """design::lowpass (16 K + 1, 400000, K * 2304000) in the reference's own mixed arithmetic: f32 taps, f64 sin / cos, Blackman window on
    i / N, f32 running sum (fir-filters.cpp:45-59).  libm's sin / cos (math), as the library's host code uses."""
    if not 2 <= K <= 16:
        raise ValueError("factor must be in [2, 16]")
    f32 = np.float32
    N = n_taps(K)
    f = float(f32(CUTOFF) / f32(K * NARROW_RATE))
    tmp = np.zeros(N, f32)
    s = f32(0.0)
    for i in range(N):
        k = i - N // 2
        v = f32(2 * math.pi * f) if k == 0 else f32(math.sin(2 * math.pi * f * float(k)) / float(k))
        w = 0.42 - 0.50 * math.cos(2 * math.pi * float(i) / float(N)) + 0.08 * math.cos(4 * math.pi * float(i) / float(N))
        tmp[i] = f32(float(v) * w)
        s = f32(s + tmp[i])
    return (tmp / s).astype(f32)


def response_db(h, rate, freqs):
    """|H(f)| in dB of real taps h at `rate`, float64."""
    n = np.arange(len(h), dtype=np.float64)
    H = np.array([np.sum(h.astype(np.float64) * np.exp(-2j * np.pi * f / rate * n)) for f in np.atleast_1d(freqs)])
    return 20 * np.log10(np.maximum(np.abs(H), 1e-300))


def convert(raw, fmt, s16_denominator=2048.0):
    """The raw formats' conversion rules (include/fmx.h fmx_iq_format): [n, 2] raw -> complex128 of the exact f32 values."""
    raw = np.asarray(raw)
    if fmt == 0:
        v = raw.astype(np.float32).astype(np.float64)
    elif fmt == 1:
        v = (raw.astype(np.float64) - 127.0) / 128.0
    elif fmt == 2:
        v = raw.astype(np.float64) / 128.0
    elif fmt == 3:
        v = raw.astype(np.float64) / float(s16_denominator)
    else:
        raise ValueError("unknown format")
    return v[:, 0] + 1j * v[:, 1]


class WidebandModel:
    def __init__(self, K, offsets):
        if not 2 <= K <= 16:
            raise ValueError("factor must be in [2, 16]")
        self.K, self.T, self.Rw = K, n_taps(K), K * NARROW_RATE
        self.h = taps(K)
        self.f = [self._checked(f) for f in offsets]
        self.P = [0 for _ in offsets]
        self.hist = [np.zeros(self.T - 1, np.complex128) for _ in offsets]        # the mixed samples in front of the next call (f64)
        self.hist32 = [np.zeros(self.T - 1, np.complex64) for _ in offsets]       # ... of the f32 restatement

    def _checked(self, f):
        f = int(f)
        if abs(f) > offset_limit(self.K):
            raise ValueError("offset out of range")
        return f

    def set_offset(self, m, hz):
        self.f[m] = self._checked(hz)

    def _oscillator(self, m, n):
        """(cos, sin) as f32 for the next n samples of output m, and P_m behind them."""
        p = (self.P[m] - self.f[m] * np.arange(1, n + 1, dtype=np.int64)) % self.Rw
        ang = 2 * np.pi * p.astype(np.float64) / self.Rw
        return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32), (int(p[-1]) if n else self.P[m])

    def process(self, x, with_f32=False):
        """One call.  x: complex [n_wide] (the converted samples, exact f32 values) -> complex128 [outputs, n_wide / K]; with_f32: also the
        f32 restatement of the same call, complex64."""
        if len(x) % self.K:
            raise ValueError("n_wide must be a multiple of the factor")
        x = np.asarray(x, np.complex128)
        n, K, T = len(x), self.K, self.T
        nj = n // K
        out = np.zeros((len(self.f), nj), np.complex128)
        out32 = np.zeros((len(self.f), nj), np.complex64)
        h = self.h.astype(np.float64)
        xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
        at = T - 1 + K - 1 + K * np.arange(nj)
        for m in range(len(self.f)):
            c, s, self.P[m] = self._oscillator(m, n)
            vv = np.concatenate([self.hist[m], x * (c.astype(np.float64) + 1j * s.astype(np.float64))])
            full = np.convolve(vv, h)                                              # full[k] = sum_i h[i] vv[k - i]
            out[m] = full[T - 1 + K - 1:T - 1 + n:K]
            self.hist[m] = vv[len(vv) - (T - 1):]
            if not with_f32:
                continue
            vr, vi = xr * c - xi * s, xr * s + xi * c                              # f32, every operation rounded
            wr = np.concatenate([self.hist32[m].real.astype(np.float32), vr])
            wi = np.concatenate([self.hist32[m].imag.astype(np.float32), vi])
            ar, ai = np.zeros(nj, np.float32), np.zeros(nj, np.float32)
            for i in range(T):                                                     # accumulation in tap order
                ar = ar + self.h[i] * wr[at - i]
                ai = ai + self.h[i] * wi[at - i]
            out32[m] = ar + 1j * ai
            self.hist32[m] = (wr[len(wr) - (T - 1):] + 1j * wi[len(wi) - (T - 1):]).astype(np.complex64)
        return (out, out32) if with_f32 else out


def rel_rms(a, b):
    """RMS of a - b relative to the RMS of b."""
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / np.sqrt(np.mean(np.abs(b) ** 2)))

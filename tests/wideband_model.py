"""Float64 model of stage W, the wide-band ingest stage (DESIGN.md "Stage W"; include/fmx.h fmx_wideband).  One model = one wide stream.

    Rw = K * 2 304 000,  T = 16 K + 1,  h = the reference's Blackman low-pass (fir-filters.cpp:41-62) with 400 kHz at Rw, unit sum, f32 taps
    v_m[n] = x[n] O(P_m[n]),  P_m[n] = (P_m[n-1] - f_m) mod Rw,  O(p) = (cos, sin)(2 pi p / Rw) evaluated in f64 and rounded to f32
    y_m[j] = sum_{i<T} h[i] v_m[jK + K-1 - i]

P_m starts at 0 and is never reset; an offset change takes effect at the first sample of the next call, the samples already mixed stay as
they are.  `process` sums in float64; with_f32 it also restates the same arithmetic in float32 (taps, samples and oscillator in f32, the mix
as four products, accumulation in tap order): the yardstick a GPU implementation's error is set against (ask for it in every call of a
model or in none: it keeps a history of its own).

Three more pieces serve the per-sample tests (test_wideband_edges_cpu.py, test_gpu_wideband_edges.py): `kernel_form`, the kernel's own
fast-path arithmetic in f32 (folded taps, four accumulators, one rotator from the 2 304 000-point table); `WidebandModel.advance`, which
moves a model forward without summing; `check_per_sample`, the bound on every single sample."""
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

    def advance(self, n, tail):
        """Move the model n samples forward without summing them: P_m by integer arithmetic, the two histories from `tail`, the last
        T - 1 samples (complex, exact f32 values) in front of the new position, each mixed with its own phase.  Equal to processing the n
        samples whose last T - 1 are `tail`, provided every offset has been in force for those T - 1 samples (set_offset, then at least
        T - 1 samples, then advance -- or advance, then set_offset)."""
        n, T = int(n), self.T
        tail = np.asarray(tail, np.complex128)
        if n % self.K or n < T - 1 or len(tail) != T - 1:
            raise ValueError("advance: n must be a multiple of the factor and at least T - 1, tail must hold T - 1 samples")
        xr, xi = tail.real.astype(np.float32), tail.imag.astype(np.float32)
        back = np.arange(T - 2, -1, -1, dtype=np.int64)                           # tail [k] lies T - 2 - k samples in front of the last one
        for m in range(len(self.f)):
            self.P[m] = (self.P[m] - self.f[m] * n) % self.Rw                     # Python integers: no width to overflow
            p = (self.P[m] + self.f[m] * back) % self.Rw
            ang = 2 * np.pi * p.astype(np.float64) / self.Rw
            c, s = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
            self.hist[m] = tail * (c.astype(np.float64) + 1j * s.astype(np.float64))
            self.hist32[m] = ((xr * c - xi * s) + 1j * (xr * s + xi * c)).astype(np.complex64)

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


_ROT = []


def rotator_table():
    """(cos, sin)(2 pi i / 2304000), i < 2 304 000, evaluated in f64 and rounded to f32: the library's oscillator table."""
    if not _ROT:
        ang = 2 * np.pi * np.arange(NARROW_RATE, dtype=np.float64) / NARROW_RATE
        _ROT.append((np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)))
    return _ROT[0]


def folded_taps(K, f, h):
    """g[i] = h[i] O((i f) mod Rw), the products formed in f64 and rounded once (wide_fold_taps) -> (Re g, Im g) as f32."""
    Rw = K * NARROW_RATE
    ang = 2 * np.pi * np.array([(i * (int(f) % Rw)) % Rw for i in range(len(h))], np.float64) / Rw
    h64 = np.asarray(h, np.float32).astype(np.float64)
    return (h64 * np.cos(ang)).astype(np.float32), (h64 * np.sin(ang)).astype(np.float32)


def kernel_form(K, f, x, h, rot_lag=None, first=0):
    """What fmx_wide.hip computes on its fast path, restated in f32 for one output of constant offset f: x, complex [n] (exact f32 values), is
    the stream from its first sample on (zeros in front of it, n a multiple of K) -> complex64 [n / K].  Folded taps, four f32 accumulators in
    tap order (Re g against (xr, xi), -+ Im g against (xi, xr)), their sum, times the rotator O(P[n_j]) = table[(-(j + 1) (f mod 2304000)) mod
    2304000], `first` outputs in front of x [0].  Every product and every sum is rounded: no fma is emulated.
    rot_lag (for seeded faults): outputs j >= rot_lag take the rotator of output j - 1."""
    f32 = np.float32
    T = n_taps(K)
    x = np.asarray(x, np.complex128)
    if len(x) % K or len(h) != T:
        raise ValueError("kernel_form: n must be a multiple of the factor, h must hold 16 K + 1 taps")
    nj = len(x) // K
    gr, gi = folded_taps(K, f, h)
    xr = np.concatenate([np.zeros(T - 1, f32), x.real.astype(f32)])
    xi = np.concatenate([np.zeros(T - 1, f32), x.imag.astype(f32)])
    at = T - 1 + K - 1 + K * np.arange(nj)
    ar, ai, br, bi = (np.zeros(nj, f32) for _ in range(4))
    for i in range(T):
        wr, wi = xr[at - i], xi[at - i]
        ar = ar + gr[i] * wr
        ai = ai + gr[i] * wi
        br = br + (-gi[i]) * wi
        bi = bi + gi[i] * wr
    sr, si = ar + br, ai + bi
    j = first + np.arange(nj, dtype=np.int64)
    if rot_lag is not None:
        j = np.where(j >= rot_lag, j - 1, j)
    idx = (-(j + 1) * (int(f) % NARROW_RATE)) % NARROW_RATE
    c, s = rotator_table()
    orr, oi = c[idx], s[idx]
    return ((orr * sr - oi * si) + 1j * (orr * si + oi * sr)).astype(np.complex64)


def check_per_sample(tag, got, ref, ref32, calls=None, form=None):
    """Every sample of every output.  got, ref (the float64 model), ref32 (its f32 restatement): [outputs, n], a case's calls concatenated.
    Per output, level = max |ref32 - ref| / max |ref| over the whole case; every sample of got must lie within 2 x level of ref, relative
    to max |ref| (the factor: a kernel may round like the restatement and in another order, DESIGN.md "Stage W").  No sample is skipped, no
    output exempt, and a sample that is not finite fails.  calls: the calls' lengths in outputs, to name the worst sample's call and its
    column in the call's tile.  form: a second f32 restatement, kernel_form's, [outputs, n] with NaN where there is none (behind an offset
    change); where given, `level` is the larger of the two restatements' worst samples (DESIGN.md "Stage W": with hundreds of outputs of 333
    samples each, the folded form's own worst sample is 2.3 - 2.6 x the plain restatement's on one output in 261, on the CPU as on the GPU).
    Prints each output's worst sample and returns the worst ratio to `level` over all outputs."""
    got, ref, ref32 = (np.asarray(v, np.complex128) for v in (got, ref, ref32))
    assert got.shape == ref.shape == ref32.shape and got.ndim == 2, (got.shape, ref.shape, ref32.shape)
    edges = np.concatenate([[0], np.cumsum(calls if calls is not None else [got.shape[1]])])
    assert edges[-1] == got.shape[1], (edges, got.shape)
    worst, failed = 0.0, []
    for m in range(got.shape[0]):
        peak = float(np.max(np.abs(ref[m])))
        level = float(np.max(np.abs(ref32[m] - ref[m]))) / peak
        if form is not None and np.any(np.isfinite(form[m])):
            level = max(level, float(np.nanmax(np.abs(np.asarray(form[m], np.complex128) - ref[m]))) / peak)
        assert peak > 0 and level > 0, (tag, m, peak, level)
        err = np.abs(got[m] - ref[m]) / peak
        err[~np.isfinite(err)] = np.inf
        j = int(np.argmax(err))
        call = int(np.searchsorted(edges, j, side="right")) - 1
        ratio = float(err[j]) / level
        print("[%s, output %d] worst sample %d (call %d, tile column %d): %.3e of the peak, f32 restatement's level %.3e (ratio %.2f, bound 2)"
              % (tag, m, j, call, (j - int(edges[call])) % 256, float(err[j]), level, ratio))
        worst = max(worst, ratio)
        if not np.all(err <= 2.0 * level):
            failed.append((m, j, float(err[j]), level))
    assert not failed, (tag, failed)
    return worst


def rel_rms(a, b):
    """RMS of a - b relative to the RMS of b."""
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.sqrt(np.mean(np.abs(a - b) ** 2)) / np.sqrt(np.mean(np.abs(b) ** 2)))

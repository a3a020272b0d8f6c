"""Float64 model of stage W at any receiver rate (include/fmx.h fmx_wideband_create_rate).  One model = one wide stream.

    Ro = 2 304 000,  g = gcd (Rw, Ro),  L = Ro / g,  M = Rw / g,  N_H = 16 M + 1,  NP = ceil (N_H / L)
    tmp = the reference's Blackman low-pass (fir-filters.cpp:41-62) of N_H taps, f = f32 (400000) / f32 (M Ro);  H [k] = f32 (tmp [k] L / sum tmp)
    v_m [n] = x [n] O (P_m [n]),  P_m [n] = (P_m [n-1] - f_m) mod Rw,  O (p) = (cos, sin) (2 pi p / Rw) evaluated in f64 and rounded to f32
    output j:  q_j = (j + 1) M - 1,  n_j = q_j div L,  p_j = q_j mod L,   y_m [j] = sum_{p_j + L i < N_H} H [p_j + L i] v_m [n_j - i]

P_m starts at 0 and is never reset; an offset change takes effect at the first sample of the next call.  `process` sums in float64; with_f32
it also restates the same arithmetic in float32 (taps, samples and oscillator in f32, the mix as four products, accumulation in tap order):
the yardstick a GPU implementation's error is set against (ask for it in every call of a model or in none).  `kernel_form` is the kernel's own
fast-path arithmetic in f32 (fmx_wide_rate.hip: H x formed first, the stations' rotators O (i f) folded in, two pairs of accumulators, the
output's rotator O (P [n_j]) from f64), `advance` moves a model forward without summing.  check_per_sample, convert and rel_rms are
wideband_model's."""
import math

import numpy as np

RO = 2304000
CUTOFF = 400000
GUARD = 150000
MAX_L = 576
RATES = [2400000, 2500000, 3000000, 6000000, 8000000, 10000000, 12500000, 20000000, 36000000]     # the rows that must work
REFUSED = [2304000, 4608000, 40000000, 10000001, 2303999, 0, -2500000]


class Ratio:
    def __init__(self, Rw):
        Rw = int(Rw)
        if not RO < Rw <= 16 * RO or Rw % RO == 0:
            raise ValueError("rate outside (Ro, 16 Ro] or a multiple of Ro")
        g = math.gcd(Rw, RO)
        if RO // g > MAX_L:
            raise ValueError("L > 576")
        self.Rw, self.L, self.M = Rw, RO // g, Rw // g
        self.NH = 16 * self.M + 1
        self.NP = -(-self.NH // self.L)
        self.min_call = -(-self.M // self.L)
        self.lim = Rw // 2 - GUARD

    def before(self, X):
        """outputs whose newest sample lies in front of sample X"""
        return int(X) * self.L // self.M

    def count(self, g0, n):
        return self.before(g0 + n) - self.before(g0)

    def samples_of(self, j):
        """(n_j, p_j) for an int64 array of output indices"""
        q = (np.asarray(j, np.int64) + 1) * self.M - 1
        return q // self.L, q % self.L


_TAPS = {}


def taps(Rw):
    """The prototype H [16 M + 1] in the library's own mixed arithmetic (design::sinc_blackman: f32 taps, f64 sin / cos, Blackman window on
    i / N; libm's sin / cos), scaled by L over the f64 sum in tap order."""
    Rw = int(Rw)
    if Rw not in _TAPS:
        r = Ratio(Rw)
        f32 = np.float32
        N = r.NH
        f = float(f32(CUTOFF) / f32(r.M * RO))
        tmp = np.zeros(N, f32)
        for i in range(N):
            k = i - N // 2
            v = f32(2 * math.pi * f) if k == 0 else f32(math.sin(2 * math.pi * f * float(k)) / float(k))
            w = 0.42 - 0.50 * math.cos(2 * math.pi * float(i) / float(N)) + 0.08 * math.cos(4 * math.pi * float(i) / float(N))
            tmp[i] = f32(float(v) * w)
        s = 0.0
        for v in tmp.astype(np.float64):                                          # in tap order, as the library sums
            s += float(v)
        _TAPS[Rw] = (tmp.astype(np.float64) * float(r.L) / s).astype(f32)
    return _TAPS[Rw]


def phase_table(Rw, H=None):
    """[L, NP]: row p = H [p + L i], zeros behind the prototype's end."""
    r = Ratio(Rw)
    H = taps(Rw) if H is None else np.asarray(H, np.float32)
    t = np.zeros(r.L * r.NP, np.float32)
    t[:r.NH] = H
    return np.ascontiguousarray(t.reshape(r.NP, r.L).T)


def response_db(H, rate, freqs):
    """|H (f)| in dB of real taps at `rate`, float64 (one matrix product per 256 frequencies)."""
    H = np.asarray(H, np.float64)
    n = np.arange(len(H), dtype=np.float64)
    freqs = np.atleast_1d(np.asarray(freqs, np.float64))
    out = np.zeros(len(freqs))
    for a in range(0, len(freqs), 256):
        ph = np.exp(-2j * np.pi * np.outer(freqs[a:a + 256] / rate, n))
        out[a:a + 256] = np.abs(ph @ H)
    return 20 * np.log10(np.maximum(out, 1e-300))


def oscillator(Rw, p):
    """O (p) as two f32 arrays"""
    ang = 2 * np.pi * np.asarray(p, np.int64).astype(np.float64) / Rw
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


class WidebandRateModel:
    """All outputs of a stream at once: the state is [outputs, ...] arrays."""

    def __init__(self, Rw, offsets):
        self.r = r = Ratio(Rw)
        self.Rw = r.Rw
        self.Hp = phase_table(Rw)
        self.f = [self._checked(f) for f in offsets]
        self.P = [0 for _ in offsets]
        self.g = 0                                                                  # samples so far
        self.hist = np.zeros((len(self.f), r.NP - 1), np.complex128)                # the mixed samples in front of the next call (f64)
        self.hist32 = np.zeros((len(self.f), r.NP - 1), np.complex64)               # ... of the f32 restatement

    def _checked(self, f):
        f = int(f)
        if abs(f) > self.r.lim:
            raise ValueError("offset out of range")
        return f

    def set_offset(self, m, hz):
        self.f[m] = self._checked(hz)

    def outputs_for(self, n):
        return self.r.count(self.g, n)

    def _mix(self, x, p):
        """x [n] (or [outputs, n]) times O (p [outputs, n]): (f64 product of the f32 oscillator, the f32 restatement's four products)"""
        c, s = oscillator(self.Rw, p)
        xr, xi = x.real.astype(np.float32), x.imag.astype(np.float32)
        return x * (c.astype(np.float64) + 1j * s.astype(np.float64)), ((xr * c - xi * s) + 1j * (xr * s + xi * c)).astype(np.complex64)

    def advance(self, n, tail):
        """Move the model n samples forward without summing them: P_m and the sample count by integer arithmetic, the two histories from
        `tail`, the last NP - 1 samples (complex, exact f32 values) in front of the new position, each mixed with its own phase.  Equal to
        processing the n samples whose last NP - 1 are `tail`, provided every offset has been in force for those NP - 1 samples."""
        n, HN = int(n), self.r.NP - 1
        tail = np.asarray(tail, np.complex128)
        if n < HN or len(tail) != HN:
            raise ValueError("advance: n must be at least NP - 1, tail must hold NP - 1 samples")
        self.P = [(P - f * n) % self.Rw for P, f in zip(self.P, self.f)]            # Python integers: no width to overflow
        back = np.arange(HN - 1, -1, -1, dtype=np.int64)[None, :]
        p = (np.array(self.P, np.int64)[:, None] + np.array(self.f, np.int64)[:, None] * back) % self.Rw
        self.hist, self.hist32 = self._mix(tail, p)
        self.g += n

    def process(self, x, with_f32=False):
        """One call.  x: complex [n_wide] (the converted samples, exact f32 values) -> complex128 [outputs, outputs_for (n_wide)]; with_f32:
        also the f32 restatement of the same call, complex64."""
        r = self.r
        x = np.asarray(x, np.complex128)
        n, HN = len(x), r.NP - 1
        j0, nj = r.before(self.g), r.count(self.g, n)
        nn, pp = r.samples_of(j0 + np.arange(nj, dtype=np.int64))
        at = (nn - self.g + HN).astype(np.int64)                                    # the newest sample's place behind the history
        assert nj == 0 or (at.min() >= HN and at.max() < HN + n)
        p = (np.array(self.P, np.int64)[:, None] - np.array(self.f, np.int64)[:, None] * np.arange(1, n + 1, dtype=np.int64)[None, :]) % self.Rw
        if n:
            self.P = [int(v) for v in p[:, -1]]
        v64, v32 = self._mix(x, p)
        vv = np.concatenate([self.hist, v64], axis=1)
        Hp64 = self.Hp.astype(np.float64)
        out = np.zeros((len(self.f), nj), np.complex128)
        for i in range(r.NP):
            out += Hp64[pp, i][None, :] * vv[:, at - i]
        self.hist = vv[:, vv.shape[1] - HN:]
        self.g += n
        if not with_f32:
            return out
        ww = np.concatenate([self.hist32, v32], axis=1)
        wr, wi = np.ascontiguousarray(ww.real), np.ascontiguousarray(ww.imag)     # f32
        ar, ai = np.zeros((len(self.f), nj), np.float32), np.zeros((len(self.f), nj), np.float32)
        for i in range(r.NP):                                                       # accumulation in tap order, every operation rounded
            h = self.Hp[pp, i][None, :]
            ar = ar + h * wr[:, at - i]
            ai = ai + h * wi[:, at - i]
        self.hist32 = ww[:, ww.shape[1] - HN:]
        return out, (ar + 1j * ai).astype(np.complex64)


def offsets(Rw, k=5):
    """the first k of: 0, -412345, lim - 1, -lim, 733001, each clipped to the rate's limit"""
    lim = Ratio(Rw).lim
    return [max(-lim, min(lim, f)) for f in [0, -412345, lim - 1, -lim, 733001][:k]]


def signal(Rw, n, sof, offs, streams, fmt=0, seed=0, amp=0.2):
    """[streams, n, 2] in the raw format: per stream a carrier with a slow phase wobble at each of its outputs' offsets, and noise
    (test_gpu_wideband_edges.edge_signal's recipe at the rate Rw)."""
    rng = np.random.default_rng(Rw // 1000 + seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((streams, n), np.complex128)
    for m, f in enumerate(offs):
        x[sof[m]] += amp * np.exp(1j * (2 * np.pi * ((int(f) * np.arange(n, dtype=np.int64)) % Rw) / Rw
                                        + 3.0 * np.sin(2 * np.pi * (900.0 + 400 * (m % 7)) * t / Rw) + m))
    x += 0.02 * (rng.standard_normal((streams, n)) + 1j * rng.standard_normal((streams, n)))
    v = np.stack([x.real, x.imag], axis=-1)
    if fmt == 0:
        return v.astype(np.float32)
    if fmt == 1:
        return np.clip(np.rint(v * 128.0 + 127.0), 0, 255).astype(np.uint8)
    if fmt == 2:
        return np.clip(np.rint(v * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint(v * 2048.0), -32768, 32767).astype(np.int16)


def kernel_form(Rw, f, x, H=None, rot_lag=None, phase_off_from=None, n_off_at=(), drop_last_tap=False):
    """What fmx_wide_rate.hip computes on its fast path, restated in f32 for one output of constant offset f (or a sequence of
    offsets): x, complex [n] (exact f32 values), is the stream from its first sample on (zeros in front of it) -> complex64 [floor (n L / M)]
    (or [offsets, floor (n L / M)]).  Per tap the product H x (rounded), then
    the rotator O ((i f) mod Rw) (f64, rounded to f32) against it in two pairs of f32 accumulators in tap order (Re against (hx_r, hx_i),
    -+ Im against (hx_i, hx_r)), their sum, times the rotator O (P [n_j]), P [n_j] = (-(n_j + 1) f) mod Rw, evaluated in f64 and rounded to
    f32.  Every product and every sum is rounded: no fma is emulated.
    Seeded faults: rot_lag: outputs j >= rot_lag take the rotator of output j - 1; phase_off_from: outputs j >= it take the phase
    (p_j + 1) mod L; n_off_at: these outputs take the samples from n_j - 1 on; drop_last_tap: the longest phases lose their last tap."""
    f32 = np.float32
    r = Ratio(Rw)
    Hp = phase_table(Rw, H)
    if drop_last_tap:
        Hp = Hp.copy()
        Hp[:, r.NP - 1] = 0
    x = np.asarray(x, np.complex128)
    nj, HN = r.before(len(x)), r.NP - 1
    j = np.arange(nj, dtype=np.int64)
    nn, pp = r.samples_of(j)
    if phase_off_from is not None:
        pp = np.where(j >= phase_off_from, (pp + 1) % r.L, pp)
    at = nn + HN
    for k in n_off_at:
        at[k] -= 1
    fm = np.atleast_1d(np.asarray(f, np.int64)) % r.Rw                             # [outputs]
    gr, gi = oscillator(r.Rw, (np.arange(r.NP, dtype=np.int64)[None, :] * fm[:, None]) % r.Rw)      # [outputs, NP]
    xr = np.concatenate([np.zeros(HN, f32), x.real.astype(f32)])
    xi = np.concatenate([np.zeros(HN, f32), x.imag.astype(f32)])
    ar, ai, br, bi = (np.zeros((len(fm), nj), f32) for _ in range(4))
    for i in range(r.NP):
        h = Hp[pp, i]
        hr, hi = (h * xr[at - i])[None, :], (h * xi[at - i])[None, :]
        ar = ar + gr[:, i:i + 1] * hr
        ai = ai + gr[:, i:i + 1] * hi
        br = br + (-gi[:, i:i + 1]) * hi
        bi = bi + gi[:, i:i + 1] * hr
    sr, si = ar + br, ai + bi
    nr = nn if rot_lag is None else np.where(j >= rot_lag, r.samples_of(np.maximum(j - 1, 0))[0], nn)
    orr, oi = oscillator(r.Rw, (-(((nr + 1) % r.Rw)[None, :] * fm[:, None])) % r.Rw)
    y = ((orr * sr - oi * si) + 1j * (orr * si + oi * sr)).astype(np.complex64)
    return y if np.ndim(f) else y[0]

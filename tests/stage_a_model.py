"""A plain float64 model of stage A -- RF DC removal, IQ balance, local oscillator, input filter, fmBand_1, fmBand_2
(fm-processor.cpp:423-476) -- for sample-by-sample comparisons of FMX_TAP_FM_IQ: numpy only.  A helper module (not a conftest):
tests/test_stage_a_model_cpu.py checks the model against the oracle and its detector against seeded defects,
tests/test_gpu_stage_a_per_sample.py checks the kernels against the model.

The model restates the REFERENCE's order of operations UNFOLDED, with the reference's own f32 coefficients (taken from the oracle
library at run time) as float64.  It reads nothing from the library under test: the library's fold of the three filters into one
polyphase FIR, its alignment `off`, its pure delay `delay_fm`, its complex output gain and its RF-DC value applied behind the filter are
what is being tested.

Numbering: input sample n = 0, 1, ... of a stream; fm sample j is the j-th output of fmBand_2 (of the input filter, or the mixed
sample itself, at rates the reference does not decimate).  The overlap-add input filter answers 65536 - 251 = 65285 input samples
late, with zeros in front: the model's fm sample j is what the oracle's TAP_FM_IQ and the library's FMX_TAP_FM_IQ hold at j.

Two forms:
  front   the reference's order: the limited RfDC value is subtracted from every sample in front of balance, mix and filter.
  behind  DESIGN.md 4.1 / FrontSet: the filter runs over the samples as they are (balanced, mixed) and what the filter makes of the RF DC
          value -- hsum balance clamp (RfDC at the taps' centre of mass), interpolated between column boundaries with dc_k and dc_w --
          is subtracted from the output.  dc_k and dc_w are recomputed here from the model's own float64 fold by build_front_set's formula.
"""
import ctypes as C

import numpy as np

import f64_models as fm

TILE = 1536                    # input samples per tile of stage A's kernels
COLS = TILE // 12              # output columns per tile
IN_TAPS = 251                  # fm-processor.cpp:77
IN_DELAY = 2 * 32768 - IN_TAPS  # overlap-add latency of the input filter (fft-filters.cpp:34)
DC_LIMIT = float(np.float32(0.01))      # fm-processor.cpp:429
IQ_F32, IQ_U8, IQ_S8, IQ_S16 = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ shapes the CPU and the GPU tests share
# calls of the matrix-pipe cases, in input samples: fewer tiles than the kernel has waves, the ring of six tiles wrapping, a remainder handed to
# front_kernel and back (every call begins on the 12-sample grid); then two calls that push the samples of interest out of the filter's delay
FRONT4_CALLS = [TILE, 5 * TILE, 6 * TILE, 7 * TILE, 13 * TILE, 7 * TILE + 600, 6 * TILE - 600]
FLUSH_CALLS = [22 * TILE, 22 * TILE]           # 5632 fm samples: more than the 5440 the input filter's latency holds back


def call_starts_fm(calls, decim=12):
    """The first fm sample of every call's read-out (calls in input samples): a call returns the fm samples its input completes."""
    ends = np.cumsum(calls) // decim
    return np.concatenate([[0], ends[:-1]])


# ------------------------------------------------------------------------------------------------ the reference's coefficients
class Design:
    """The three filters of one input rate and bandwidth as the reference designs them (f32 from the oracle, kept as float64):
    h_in [251] or None (input filter off), k1, k2 complex (h / sum, h), the two decimations (integer arithmetic of fm-processor.cpp:36,
    68-75); decim == 1: the reference runs no decimator at this rate (:471)."""

    def __init__(self, L, rate, bw, fm_rate=192000):
        fp = C.POINTER(C.c_float)
        self.rate, self.bw, self.fm_rate = int(rate), int(bw), int(fm_rate)
        self.h_in = None
        if bw > 0:
            h = np.zeros(IN_TAPS, np.float32)
            L.fmo_lowpass_kernel(IN_TAPS, bw // 2, rate, h.ctypes.data_as(fp))
            self.h_in = h.astype(np.float64)
        self.latency = IN_DELAY if bw > 0 else 0
        if rate // fm_rate > 1:
            irate = rate // 6
            self.d1, self.d2 = rate // irate, irate // fm_rate
            ks = []
            for n, low, fs in ((4 * rate // irate + 1, fm_rate // 2, rate), (irate // fm_rate + 1, fm_rate // 2, irate)):
                k = np.zeros((n, 2), np.float32)
                L.fmo_decim_kernel(n, low, fs, k.ctypes.data_as(fp))
                ks.append(k[:, 0].astype(np.float64) + 1j * k[:, 1].astype(np.float64))
            self.k1, self.k2 = ks
        else:
            self.d1 = self.d2 = 1
            self.k1 = self.k2 = None
        self.decim = self.d1 * self.d2

    # ---- the fold, for the second form and the restatements only (the model's main path never folds)
    def fold(self):
        """(g [NT] float64, gain complex): z[j] = gain sum_k g[k] v[decim j + decim - 1 - latency - k].  The kernels are h (1 / S + j), so
        the real parts fold and (1 + j S1) (1 + j S2) is left over (fir-filters.cpp:345-346)."""
        g, gain = np.ones(1), 1.0 + 0j
        if self.decim > 1:
            r1, r2 = self.k1.real, self.k2.real
            up = np.zeros(self.d1 * (r2.size - 1) + 1)
            up[::self.d1] = r2
            g = np.convolve(up, r1)
            # k = (t / S, t) with S the f32 sum of t in tap order (fir-filters.cpp:331-346): k = (t / S) (1 + j S)
            s = []
            for k in (self.k1, self.k2):
                acc = np.float32(0.0)
                for t in k.imag.astype(np.float32):
                    acc = np.float32(acc + t)
                s.append(float(acc))
            gain = (1 + 1j * s[0]) * (1 + 1j * s[1])
        if self.h_in is not None:
            g = np.convolve(g, self.h_in)
        return g, gain

    def front_set(self):
        """build_front_set's derived quantities from the model's own fold, for rates decimated by 12: g32 (the f32-rounded taps as
        float64), gain, off, delay, hsum, dc_k, dc_w."""
        assert self.decim == 12
        g, gain = self.fold()
        g32 = g.astype(np.float32).astype(np.float64)
        e = self.decim - 1 - self.latency
        delay = -(e // 12)
        off = e + 12 * delay
        hs = g32.sum()
        mk = float((g32 * np.arange(g32.size)).sum())
        q0 = off - mk / hs + 1.0
        k = -int(np.floor(q0 / 12.0))
        w = float(np.float32((q0 + 12.0 * k) / 12.0))
        return dict(g32=g32, gain=gain, off=int(off), delay=int(delay), hsum=float(np.float32(hs)), dc_k=k, dc_w=w)


# ------------------------------------------------------------------------------------------------ raw formats
def convert(codes, fmt, s16_denominator=2048.0):
    """include/fmx.h fmx_process_*_raw: U8 (u8 - 127) / 128, S8 s8 / 128, S16 s16 / denominator (a power of two); -> float32 [n, 2]."""
    c = np.asarray(codes)
    if fmt == IQ_F32:
        return c.astype(np.float32)
    if fmt == IQ_U8:
        return ((c.astype(np.int32) - 127) / 128.0).astype(np.float32)
    if fmt == IQ_S8:
        return (c.astype(np.int32) / 128.0).astype(np.float32)
    return (c.astype(np.int32) / float(s16_denominator)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the per-sample part
def as_complex(x):
    x = np.asarray(x)
    return x.astype(np.complex128) if np.iscomplexobj(x) else x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)


def per_call(value, calls):
    """A setting given once, or as one value per call, as a list of (first sample, value) runs."""
    if not isinstance(value, (list, tuple)):
        return [(0, value)]
    assert calls is not None and len(value) == len(calls)
    starts = np.concatenate([[0], np.cumsum(calls)[:-1]])
    runs = []
    for s, v in zip(starts, value):
        if not runs or runs[-1][1] != v:               # (a run begins where the setter changes something)
            runs.append((int(s), v))
    return runs


def rf_dc(x, rate, dc_runs):
    """R [n + 1]: the RfDC state in front of sample n (R[0] = 0), r <- (x - r) alpha + r with alpha = f32 (1) / f32 (rate), while DC removal
    is on; a setDCRemove change zeroes it.  dc_runs: [(first sample, on)].  Exact in blocks: r[i] = d^i (r0 + alpha sum_k<=i x[k] d^-k)."""
    n = x.shape[0]
    alpha = float(np.float32(1.0) / np.float32(rate))
    d = 1.0 - alpha
    R = np.zeros(n + 1, np.complex128)
    B = 4096
    pw = d ** np.arange(1, B + 1)
    bounds = [s for s, _ in dc_runs] + [n]
    for (s0, on), s1 in zip(dc_runs, bounds[1:]):
        r = 0.0 + 0j                                  # (the first run starts from zero, every later one from the setter's zero)
        if not on:
            continue                                  # (R stays 0: nothing is subtracted, nothing is updated)
        for a in range(s0, s1, B):
            b = min(a + B, s1)
            p = pw[:b - a]
            R[a + 1:b + 1] = p * (r + alpha * np.cumsum(x[a:b] / p))
            r = R[b]
    return R


def clamp(c):
    return np.clip(c.real, -DC_LIMIT, DC_LIMIT) + 1j * np.clip(c.imag, -DC_LIMIT, DC_LIMIT)


def oscillator(n, rate, lo_runs):
    """(LO [n] complex, f32 table values as float64): P <- (P - lo) mod rate in front of every sample, P survives a change of lo
    (oscillator.cpp:26-35, 49-58).  lo_runs: [(first sample, lo)]."""
    P = np.zeros(n, np.int64)
    p0 = 0
    bounds = [s for s, _ in lo_runs] + [n]
    for (s0, lo), s1 in zip(lo_runs, bounds[1:]):
        P[s0:s1] = (p0 - int(lo) * np.arange(1, s1 - s0 + 1, dtype=np.int64)) % rate
        if s1 > s0:
            p0 = int(P[s1 - 1])
    a = 2.0 * np.pi * P / rate
    return np.cos(a).astype(np.float32).astype(np.float64) + 1j * np.sin(a).astype(np.float32).astype(np.float64), P


def balance(c, att):
    return c.real * float(np.float32(att[0])) + 1j * c.imag * float(np.float32(att[1]))


# ------------------------------------------------------------------------------------------------ the filters, unfolded
def filters(v, D, direct=False, filtered=None):
    """Input filter (a linear convolution, 65285 samples late, zeros in front), fmBand_1, fmBand_2: an output when the counter reaches
    D, y[m] = sum_l k[l] v[D m + D - 1 - l] (fir-filters.cpp:397-424).  direct: the convolutions as plain float64 sums, whose rounding is relative to an output's own terms -- a
    transform's is relative to the stream's peak and would drown a quiet stretch a million times below it (the level-step case).
    filtered: a hook for tests/ola_model.py -- the filtered stream [n] itself, or a function of v that makes it, in the place of the LTI
    input filter (the reference's block machine across restarts); the decimators then run over it as it is."""
    n = v.shape[0]
    conv = np.convolve if direct else fm.fftconv
    if filtered is not None:
        w = np.asarray(filtered(v) if callable(filtered) else filtered, np.complex128)
        assert w.shape == (n,)
        if D.decim == 1:
            return w
        y = conv(w, D.k1)[D.d1 * np.arange(n // D.d1, dtype=np.int64) + D.d1 - 1]
        return conv(y, D.k2)[D.d2 * np.arange(y.shape[0] // D.d2, dtype=np.int64) + D.d2 - 1]
    w = v if D.h_in is None else fm.delayed(conv(v, D.h_in), IN_DELAY, n)
    if D.decim == 1:
        return w
    y = conv(w, D.k1)[D.d1 * np.arange(n // D.d1, dtype=np.int64) + D.d1 - 1]
    z = conv(y, D.k2)[D.d2 * np.arange(y.shape[0] // D.d2, dtype=np.int64) + D.d2 - 1]
    # an output whose newest input lies in front of the stream is zero: the transforms' own rounding (1e-16 of the stream's peak) must not stand there
    z[D.decim * np.arange(z.shape[0], dtype=np.int64) + D.decim - 1 - D.latency < 0] = 0.0
    return z


def stage_a(D, x, calls=None, lo=0, att=(1.0, 1.0), dc_remove=1, form="front", behind=None, dc_columns_late=0, direct=False, filtered=None):
    """The fm-rate IQ [n / decim] complex128 of one channel over the whole stream x ([n, 2] f32 or complex).  lo and dc_remove: one value,
    or one per call (calls = the calls' lengths in input samples).  form: "front", "behind", or "mixed" with `behind` a boolean per fm
    sample (the outputs a kernel of the second form wrote).  dc_columns_late: a seed for the detector, the second form's RF DC value taken that many
    columns late.  filtered: filters ()'s hook, form "front" only."""
    x = as_complex(x)
    n = x.shape[0]
    assert filtered is None or form == "front"
    lo_runs, dc_runs = per_call(lo, calls), per_call(dc_remove, calls)
    LO, _ = oscillator(n, D.rate, lo_runs)
    R = rf_dc(x, D.rate, dc_runs)
    out = {}
    if form in ("front", "mixed"):
        out["front"] = filters(balance(x - clamp(R[1:]), att) * LO, D, direct, filtered)
    if form in ("behind", "mixed"):
        F = D.front_set()
        z = filters(balance(x, att) * LO, D, direct)
        nj = 12 * np.arange(z.shape[0], dtype=np.int64) + 11 - D.latency          # the output's newest input sample
        ok = nj >= 0
        b0 = nj - F["off"] - 12 * (F["dc_k"] + dc_columns_late)                                       # the column boundary in front of the centre of mass
        r0 = np.where(b0 >= 0, R[np.clip(b0, 0, n)], 0)
        r1 = np.where(b0 + 12 >= 0, R[np.clip(b0 + 12, 0, n)], 0)
        c = clamp(r0 + F["dc_w"] * (r1 - r0))
        # what the filter makes of a constant in front of the mix: the taps' sum turned with the oscillator (fmx_front4lo.hip: Hlo LO[n],
        # Hlo = sum_m g[m] table[(m lo) mod R]) -- which is the filter run over the oscillator's own sequence, and stays that where the
        # oscillator is switched between two calls and a window holds samples mixed with the old one
        m = np.arange(F["g32"].size, dtype=np.int64)
        njc = np.clip(nj, 0, n - 1)
        if len(lo_runs) == 1:
            a = 2.0 * np.pi * ((m * int(lo_runs[0][1])) % D.rate) / D.rate
            H = F["hsum"] if int(lo_runs[0][1]) == 0 else complex((F["g32"] * (np.cos(a).astype(np.float32) + 1j * np.sin(a).astype(np.float32))).sum())
            turned = F["gain"] * LO[njc] * H
        else:
            y = fm.fftconv(LO, F["g32"])
            turned = F["gain"] * y[njc]
        out["behind"] = np.where(ok, z - turned * balance(c, att), 0)
    if form == "mixed":
        return np.where(np.asarray(behind, bool), out["behind"], out["front"])
    return out[form]


# ------------------------------------------------------------------------------------------------ restatements of the kernels' forms
def premix32(D, x, calls=None, lo=0, att=(1.0, 1.0), dc_remove=1):
    """The mixed samples of the reference's order, rounded to f32 (what a kernel's history holds in its processed format)."""
    x = as_complex(x)
    LO, _ = oscillator(x.shape[0], D.rate, per_call(lo, calls))
    v = balance(x - clamp(rf_dc(x, D.rate, per_call(dc_remove, calls))[1:]), att) * LO
    return v.real.astype(np.float32), v.imag.astype(np.float32)


def window_index(D, n_out, ntaps):
    """(the output has an input at all, index of its newest input in a stream with `ntaps` zeros in front)"""
    nj = 12 * np.arange(n_out, dtype=np.int64) + 11 - D.latency
    return nj >= 0, np.clip(nj, 0, None) + ntaps


def folded_f32(D, vr, vi, g32=None):
    """front_kernel's arithmetic in its plainest form: f32 taps and samples, one f32 accumulator in tap order (newest sample first, no fma),
    then the complex gain in f32.  -> complex128 [n / 12]."""
    F = D.front_set()
    g = (F["g32"] if g32 is None else g32).astype(np.float32)
    nt = g.size
    n_out = vr.shape[0] // 12
    ok, idx = window_index(D, n_out, nt)
    pr = np.concatenate([np.zeros(nt, np.float32), vr.astype(np.float32)])
    pi = np.concatenate([np.zeros(nt, np.float32), vi.astype(np.float32)])
    ar, ai = np.zeros(n_out, np.float32), np.zeros(n_out, np.float32)
    for k in range(nt):
        ar = ar + g[k] * pr[idx - k]
        ai = ai + g[k] * pi[idx - k]
    gr, gi = np.float32(F["gain"].real), np.float32(F["gain"].imag)
    z = (ar * gr - ai * gi).astype(np.float64) + 1j * (ar * gi + ai * gr).astype(np.float64)
    return np.where(ok, z, 0)


def folded_f64(D, vr, vi, g=None, gain=None):
    """The fold in float64 with the f32-rounded taps, on f32 samples: z[j] = gain sum_k g32[k] v[12 j + 11 - latency - k]."""
    F = D.front_set()
    g = F["g32"] if g is None else g
    v = vr.astype(np.float64) + 1j * vi.astype(np.float64)
    y = fm.fftconv(v, g)
    nj = 12 * np.arange(v.shape[0] // 12, dtype=np.int64) + 11 - D.latency
    return np.where(nj >= 0, y[np.clip(nj, 0, None)], 0) * (F["gain"] if gain is None else gain)


def f16_split(a):
    """(high, low) f16 halves of a as float64: high = f16 (a), low = f16 (a - high)."""
    hi = a.astype(np.float16).astype(np.float64)
    return hi, (a - hi).astype(np.float16).astype(np.float64)


def split_f64(D, vr, vi, drop_low_every=0):
    """front4_kernel's operands: every tile of 1536 samples has its own power-of-two scale (its largest component goes to [2^14, 2^15)),
    samples and taps 2^14 are split into f16 high and low halves, three product terms th xh + th xl + tl xh; the products are exact in f32,
    so they are summed in float64 here: what is left against folded_f64 is the split alone.  drop_low_every = 8192: one sample in 2^13
    without its low half (the round-6 double-rounding tie, as a seed for the detector)."""
    F = D.front_set()
    n = vr.shape[0] // TILE * TILE
    parts = []
    for comp in (vr[:n].astype(np.float64), vi[:n].astype(np.float64)):
        parts.append(comp.reshape(-1, TILE))
    amax = np.maximum(np.abs(parts[0]).max(axis=1), np.abs(parts[1]).max(axis=1))
    e = np.where(amax > 0, 14 - np.floor(np.log2(np.where(amax > 0, amax, 1.0))), 0.0)
    sc = np.repeat(2.0 ** e, TILE)
    th, tl = f16_split(F["g32"] * 2.0 ** 14)
    acc = []
    for comp in (vr, vi):
        xs = comp[:n].astype(np.float64) * sc
        xh, xl = f16_split(xs)
        if drop_low_every:
            xl[drop_low_every - 1::drop_low_every] = 0.0
        acc.append(fm.fftconv(xh / sc, th) + fm.fftconv(xl / sc, th) + fm.fftconv(xh / sc, tl))
    y = (acc[0] + 1j * acc[1]) * 2.0 ** -14
    nj = 12 * np.arange(n // 12, dtype=np.int64) + 11 - D.latency
    return np.where(nj >= 0, y[np.clip(nj, 0, None)], 0) * F["gain"]


# ------------------------------------------------------------------------------------------------ comparison
class Worst:
    """Result of compare (): the worst sample, relative to the peak (or to its local scale), and where it fell: the call whose read-out holds it, and
    within that read-out the tile of 1536 input samples and the column of 12 input samples -- an fm sample is `decim` input samples."""

    def __init__(self, rel, err, index, lane, scale, rms, call_starts, decim=12):
        self.rel, self.err, self.index, self.lane, self.scale, self.rms = rel, err, index, lane, scale, rms
        cs = np.asarray(call_starts if call_starts is not None and len(call_starts) else [0], np.int64)
        self.call = max(int(np.searchsorted(cs, index, side="right") - 1), 0)
        self.from_call_start = int(index - cs[self.call])
        self.tile, self.column = self.from_call_start * decim // TILE, self.from_call_start * decim % TILE // 12

    def __str__(self):
        return ("worst sample %.3e (%.3e of the scale %.4g) at fm sample %d [%s]: call %d, tile %d, column %d; rms %.3e"
                % (self.err, self.rel, self.scale, self.index, "IQ"[self.lane], self.call, self.tile, self.column, self.rms))


def compare(got, ref, call_starts=None, local=None, decim=12):
    """Sample-by-sample distance of `got` ([n, 2] f32 or complex) to `ref` (complex128), per component as f64_models.compare: the worst
    sample relative to the output's peak (the largest |component| of ref) -- or, with `local` [n], every sample relative to its own
    local scale --, its fm sample (`decim` input samples each), and the call (call_starts: the first fm sample every call returned), the tile of 1536 input samples
    and the column within the call's read-out where it fell."""
    g, r = as_complex(got), np.asarray(ref, np.complex128)
    assert g.shape == r.shape and g.shape[0] > 0, (g.shape, r.shape)
    e = np.stack([np.abs(g.real - r.real), np.abs(g.imag - r.imag)], axis=1)
    peak = float(max(np.abs(r.real).max(), np.abs(r.imag).max()))
    if local is None:
        q = e / peak if peak > 0 else np.full(e.shape, np.inf)
        scale = peak
    else:
        live = np.asarray(local) > 0
        q = np.where(live[:, None], e / np.where(live, local, 1.0)[:, None], np.where(e > 0, np.inf, 0.0))
    i, lane = np.unravel_index(int(np.argmax(q)), q.shape)
    if local is not None:
        scale = float(local[i])
    return Worst(float(q[i, lane]), float(e[i, lane]), int(i), int(lane), scale, float(np.sqrt(np.mean(e ** 2))), call_starts, decim)


def check(w, bound, what=""):
    """The worst-sample assertion; a failure names the sample's call, tile and column."""
    assert w.scale > 0 and w.rel <= bound, "%s: worst sample %.3e of the scale exceeds the bound %.3e -- %s" % (what, w.rel, bound, w)


# ------------------------------------------------------------------------------------------------ the reference's own distance
# Worst sample of the oracle's f32 arithmetic (TAP_FM_IQ) against stage_a (form "front") on identical inputs, relative to the output's
# peak: the largest over the cases of tests/test_stage_a_model_cpu.py with the input filter on and off, which prints each figure and
# holds it against these records.  The GPU bounds are these doubled (what the reference arithmetic alone reaches, doubled)
# and come from nothing else.
REF_STAGE_A_WORST_ON = 1.31e-6       # input filter on: the rate the reference does not decimate (192 000; peak 0.54); 7.1e-7 ... 8.7e-7 at the decimated rates
REF_STAGE_A_WORST_OFF = 4.10e-7      # input filter off: the two decimators' f32 sums (a balance of 0.9 / 1.1)
STAGE_A_BOUND_ON = 2.0 * REF_STAGE_A_WORST_ON
STAGE_A_BOUND_OFF = 2.0 * REF_STAGE_A_WORST_OFF
FRONT_BEHIND_DOCUMENTED = 2.5e-6          # DESIGN.md 5, known deviations: RF DC removal behind the filter, the distance between the two float64 forms

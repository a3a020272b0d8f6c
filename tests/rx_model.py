"""The reception meter (include/fmx.h fmx_rx_record) restated: a float64 model of a window's six fields, the f32 restatement in the
contract's own order -- twice: whole windows at once (restate_windows, what the checker uses) and a machine that is fed calls of any length (Machine,
which also takes the seeded faults of the checker's own test) --, quality () in float64 (fmx_rx_quality_of's figures), and the checker: every field of
a record EQUALS the restatement bit for bit.  The kernel calls no library function, so there is no tolerance anywhere between device and restatement.

v is a channel's FMX_TAP_FM_IQ from fm sample 0 on, [n, 2] float32 (or complex): the values its calls' taps returned, behind each other.  u [j] = v [j - 1],
u [0] = 0: what the ring holds in front of the stream is zero."""
import numpy as np

WINDOW, LANES, STEPS, RING = 9600, 64, 150, 64
F32 = np.float32
FIELDS = ("p_max", "p_min", "p_mean", "p2_mean", "r1_re", "r1_im")
RX_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("p_max", np.float32), ("p_min", np.float32), ("p_mean", np.float32),
                     ("p2_mean", np.float32), ("r1_re", np.float32), ("r1_im", np.float32)])


# ---- what the tests assert, each twice what tests/test_rx_cpu.py measured on the oracle (DESIGN.md 4.13 lists them under these names)
# the f32 restatement against float64 on 0.5 s of the default stereo signal: 1.02e-7 / 9.6e-8 / 1.16e-7 relative (p_mean, p2_mean, |r1|)
RESTATE_REL = {"p_mean": 2.1e-7, "p2_mean": 2.0e-7, "r1": 2.4e-7}
# an unmodulated carrier of amplitude 0.5 at +10 kHz / -3.7 kHz, RF DC removal on / off, windows 1 .. 9: offset_hz 9.43e-3 Hz from the set offset at
# the most, level_dbfs 7.02e-6 dB from 20 log10 (0.5 |H (f)|), H the designed response of the two decimators and the 165 kHz input filter
OFFSET_TOL_HZ = 2 * 9.43e-3
LEVEL_TOL_DB = 2 * 7.02e-6
# the mono 1 kHz tone at +-37 500 Hz, clean: am_depth 0.0664 (the meter's floor: the filtered FM signal's own envelope ripple) and cnr_db 25.49 (its
# ceiling); twice the depth, and twice the noise-to-carrier ratio (3.01 dB) below the ceiling
AM_DEPTH_FLOOR, CNR_CEILING_DB = 0.0664, 25.49
# config 2's stereo signal in white noise, 10 windows pooled: |cnr_db - truth| = 0.158 / 1.342 / 6.615 dB at an input C/N of 10 / 20 / 30 dB in 165 kHz
# (15.66 dB at 40 dB, which lies above the ceiling and is not asserted)
NOISE_SEED = 0x5D2F1A7B
CNR_LEVELS_DB = (10, 20, 30)
CNR_TOL_DB = {10: 2 * 0.158, 20: 2 * 1.342, 30: 2 * 6.615}


def noise_sigma(cnr_db, amp=0.5, bandwidth=165000, input_rate=2304000):
    """the generator's noiseSigma (per component, at the input rate) for a carrier of amplitude `amp` at `cnr_db` over the noise in `bandwidth`"""
    return float(np.sqrt(amp * amp / (2.0 * 10.0 ** (cnr_db / 10.0)) * input_rate / bandwidth))


def as_pairs(v):
    """[n, 2] float32 of a tap in either form"""
    v = np.asarray(v)
    if np.iscomplexobj(v):
        v = np.stack([v.real, v.imag], axis=1)
    return np.ascontiguousarray(v, F32).reshape(-1, 2)


def with_previous(v):
    """(v, u) as [n, 2] float32, u [j] = v [j - 1] and u [0] = 0"""
    v = as_pairs(v)
    return v, np.concatenate([np.zeros((1, 2), F32), v[:-1]])


def model_f64(v, windows):
    """{field: [len (windows)] float64}: the six fields of the windows in exact arithmetic on the f32 inputs."""
    v, u = with_previous(v)
    out = {k: np.zeros(len(windows)) for k in FIELDS}
    for n, w in enumerate(windows):
        a, b = v[w * WINDOW:(w + 1) * WINDOW].astype(np.float64), u[w * WINDOW:(w + 1) * WINDOW].astype(np.float64)
        assert a.shape[0] == WINDOW, "window %d is not covered by the samples" % w
        p = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
        out["p_max"][n], out["p_min"][n] = p.max(), p.min()
        out["p_mean"][n], out["p2_mean"][n] = p.sum() / 9600.0, (p * p).sum() / 9600.0
        out["r1_re"][n] = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).sum() / 9600.0
        out["r1_im"][n] = (a[:, 1] * b[:, 0] - a[:, 0] * b[:, 1]).sum() / 9600.0
    return out


def butterfly(a, op):
    """a [..., 64] f32: a [l] = a [l] op a [l xor m] for m = 32 .. 1; every lane ends with the same value, lane 0's is returned"""
    idx = np.arange(LANES)
    for m in (32, 16, 8, 4, 2, 1):
        a = op(a, a[..., idx ^ m])
    return a[..., 0]


def terms(v, u):
    """the per-sample f32 terms of the contract: p, f32 (p p), the real and the imaginary part of v conj (u), every product and sum rounded once"""
    re, im, ure, uim = v[..., 0], v[..., 1], u[..., 0], u[..., 1]
    p = re * re + im * im
    out = p, p * p, re * ure + im * uim, im * ure - re * uim
    assert all(t.dtype == F32 for t in out)
    return out


def restate_windows(v, windows):
    """{field: [len (windows)] float32}: the contract's arithmetic -- lane l takes the samples i = 64 q + l in step order, in f32, products rounded to f32
    before they are added; the butterfly; the finishing divisions."""
    v, u = with_previous(v)
    W = len(windows)
    shape = (W, STEPS, LANES, 2)
    x = np.stack([v[w * WINDOW:(w + 1) * WINDOW] for w in windows]).reshape(shape) if W else np.zeros(shape, F32)
    y = np.stack([u[w * WINDOW:(w + 1) * WINDOW] for w in windows]).reshape(shape) if W else np.zeros(shape, F32)
    p, pp, re, im = terms(x, y)
    mx, mn = np.full((W, LANES), -np.inf, F32), np.full((W, LANES), np.inf, F32)
    s1, s2, cr, ci = (np.zeros((W, LANES), F32) for _ in range(4))
    for q in range(STEPS):
        mx, mn = np.maximum(mx, p[:, q]), np.minimum(mn, p[:, q])
        s1 = s1 + p[:, q]
        s2 = s2 + pp[:, q]
        cr = cr + re[:, q]
        ci = ci + im[:, q]
    add = lambda a, b: a + b
    out = {"p_max": butterfly(mx, np.maximum), "p_min": butterfly(mn, np.minimum),
           "p_mean": butterfly(s1, add) / F32(9600.0), "p2_mean": butterfly(s2, add) / F32(9600.0),
           "r1_re": butterfly(cr, add) / F32(9600.0), "r1_im": butterfly(ci, add) / F32(9600.0)}
    assert all(a.dtype == F32 for a in out.values())
    return out


class Machine:
    """The meter of one channel as a machine that is fed calls: feed (v, on) takes the next samples of the stream and returns the records the call
    completes, as (index, end_sample, {field: f32}).  What it carries between calls is the 64 x 6 accumulators; the sample in front of a call's first is the
    ring's (`last`: the ring holds it whether the meter is on or not).  `fault` seeds one of the mistakes the checker has to catch: "drop" (the first sample
    of every call but the first is not accumulated), "swap" (lanes 3 and 40 change places in front of the butterfly), "late" (the windows begin one sample
    late), "lag0" (v conj (v) for v conj (u)), "sign" (the sign of r1_im), "4800" (the sums divided by 4800)."""

    def __init__(self, fault=None):
        self.fault = fault
        self.j = 0
        self.active = False            # the window in progress has been metered from its start
        self.last = np.zeros(2, F32)
        self._reset()

    def _reset(self):
        self.mx, self.mn = np.full(LANES, -np.inf, F32), np.full(LANES, np.inf, F32)
        self.s = np.zeros((4, LANES), F32)

    def feed(self, v, on=True):
        v = as_pairs(v)
        u = np.concatenate([self.last[None], v[:-1]]) if v.shape[0] else v
        if self.fault == "lag0":
            u = v
        p, pp, re, im = terms(v, u)
        if self.fault == "sign":
            im = -im
        shift = 1 if self.fault == "late" else 0
        recs = []
        if not on:
            self.active = False
        for n in range(v.shape[0]):
            j = self.j + n
            i = (j - shift) % WINDOW
            if on and i == 0 and j >= shift:
                self.active = True
                self._reset()
            if on and self.active and not (self.fault == "drop" and n == 0 and self.j > 0):
                l = i % LANES
                self.mx[l], self.mn[l] = max(self.mx[l], p[n]), min(self.mn[l], p[n])
                self.s[0, l] = self.s[0, l] + p[n]
                self.s[1, l] = self.s[1, l] + pp[n]
                self.s[2, l] = self.s[2, l] + re[n]
                self.s[3, l] = self.s[3, l] + im[n]
            if on and self.active and i == WINDOW - 1:
                mx, mn, s = self.mx.copy(), self.mn.copy(), self.s.copy()
                if self.fault == "swap":
                    for a in (mx, mn):
                        a[[3, 40]] = a[[40, 3]]
                    s[:, [3, 40]] = s[:, [40, 3]]
                add = lambda a, b: a + b
                den = F32(4800.0) if self.fault == "4800" else F32(9600.0)
                w = (j - shift) // WINDOW
                recs.append((w, (w + 1) * WINDOW, {
                    "p_max": butterfly(mx, np.maximum), "p_min": butterfly(mn, np.minimum),
                    "p_mean": butterfly(s[0], add) / den, "p2_mean": butterfly(s[1], add) / den,
                    "r1_re": butterfly(s[2], add) / den, "r1_im": butterfly(s[3], add) / den}))
                self.active = False
        if v.shape[0]:
            self.last = v[-1].copy()
        self.j += v.shape[0]
        return recs


def as_records(recs):
    """Machine.feed's records as an RX_DTYPE array"""
    out = np.zeros(len(recs), RX_DTYPE)
    for k, (w, e, f) in enumerate(recs):
        out[k]["index"], out[k]["end_sample"] = w, e
        for name, val in f.items():
            out[k][name] = val
    return out


def records_of(fields, windows):
    """restate_windows' or model_f64's fields as an RX_DTYPE array (the model's rounded to f32)"""
    out = np.zeros(len(windows), RX_DTYPE)
    out["index"] = np.asarray(windows, np.int64)
    out["end_sample"] = (out["index"] + 1) * WINDOW
    for name in FIELDS:
        out[name] = fields[name]
    return out


def quality(fields, fmRate=192000):
    """fmx_rx_quality_of in float64: `fields` is an RX_DTYPE array or a dict of the six fields (float64 values are taken as they are)."""
    g = lambda k: np.asarray(fields[k], np.float64)
    n = g("p_mean").size
    assert n > 0
    M2, M4 = g("p_mean").sum() / n, g("p2_mean").sum() / n
    disc = 2.0 * M2 * M2 - M4
    if disc <= 0.0:
        cnr = -np.inf
    else:
        S = np.sqrt(disc)
        N = M2 - S
        cnr = np.inf if N <= 0.0 else 10.0 * np.log10(S / N)
    a, b = np.sqrt(g("p_max")), np.sqrt(np.maximum(g("p_min"), 0.0))
    depth = np.where(g("p_max") > 0.0, (a - b) / np.where(a + b > 0.0, a + b, 1.0), 0.0)
    return {"level_dbfs": 10.0 * np.log10(M2) if M2 > 0.0 else -np.inf, "cnr_db": float(cnr), "am_depth": float(depth.max()),
            "offset_hz": float(np.arctan2(g("r1_im").sum(), g("r1_re").sum()) * fmRate / (2.0 * np.pi)), "windows": n}


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_records(recs, v, expect_index=None):
    """recs: RX_DTYPE records of one channel; v: the channel's FMX_TAP_FM_IQ from fm sample 0 on, covering every record's window.  index, end_sample and
    all six fields must EQUAL the restatement's, bit for bit."""
    recs = np.asarray(recs)
    if expect_index is not None:
        assert list(recs["index"]) == list(expect_index), (list(recs["index"]), list(expect_index))
    if recs.size == 0:
        return
    windows = [int(w) for w in recs["index"]]
    assert np.array_equal(recs["end_sample"], (recs["index"] + 1) * WINDOW), "end_sample"
    r32 = restate_windows(v, windows)
    for name in FIELDS:
        bad = np.nonzero(bits(recs[name]) != bits(r32[name]))[0]
        assert bad.size == 0, "%s differs from the restatement in window %d: %r against %r" % (name, windows[bad[0]], recs[name][bad[0]], r32[name][bad[0]])

"""The modulation meter (include/fmx.h fmx_mod_record) restated: a float64 model of a window's six figures, the f32 restatement in the
contract's own order -- twice: whole windows at once (restate_windows, what the checker uses) and sample streams cut into calls (Restatement, which
also takes the seeded faults of the checker's own test) -- and the checker that compares a handle's records with both.

d and phi are the demodulator output and the pilot phase of a channel from fm sample 0 on, as FMX_TAP_DEMOD and FMX_TAP_PILOT_PHASE deliver them."""
import numpy as np

WINDOW, LANES, STEPS, RING = 9600, 64, 150, 64
F32 = np.float32
FIELDS_EXACT = ("peak_pos", "peak_neg", "mean", "mean_square")
FIELDS_PILOT = ("pilot_i", "pilot_q")
# The error of the device's sincosf in ulp.  No ROCm math documentation is installed with the toolchain; measured once on an MI355X against float64 over
# 2^20 phases in [-8, 8) (tools/ubench/sincos_ulp.hip): 1.525 ulp of the true value at the most.  Rounded up.
SINCOS_ULP = 2.0


def model_f64(d, phi, windows):
    """{field: [len (windows)] float64}: the six figures of the windows in exact arithmetic on the f32 inputs."""
    out = {k: np.zeros(len(windows)) for k in FIELDS_EXACT + FIELDS_PILOT}
    out["mean_abs"] = np.zeros(len(windows))
    for n, w in enumerate(windows):
        x = np.asarray(d[w * WINDOW:(w + 1) * WINDOW], np.float64)
        p = np.asarray(phi[w * WINDOW:(w + 1) * WINDOW], np.float64)
        assert x.size == WINDOW and p.size == WINDOW, "window %d is not covered by the samples" % w
        out["peak_pos"][n], out["peak_neg"][n] = x.max(), x.min()
        out["mean"][n], out["mean_square"][n] = x.sum() / 9600.0, (x * x).sum() / 9600.0
        out["pilot_i"][n], out["pilot_q"][n] = (x * np.sin(p)).sum() / 4800.0, (x * np.cos(p)).sum() / 4800.0
        out["mean_abs"][n] = np.abs(x).mean()
    return out


def butterfly(a, op):
    """a [..., 64] f32: a [l] = a [l] op a [l xor m] for m = 32 .. 1; every lane ends with the same value, lane 0's is returned"""
    idx = np.arange(LANES)
    for m in (32, 16, 8, 4, 2, 1):
        a = op(a, a[..., idx ^ m])
    return a[..., 0]


def restate_windows(d, phi, windows):
    """{field: [len (windows)] float32}: the contract's arithmetic -- lane l takes the samples i = 64 q + l in step order, in f32, products rounded to f32
    before they are added; the butterfly; the finishing divisions -- with numpy's f32 sine and cosine in the device's place."""
    W = len(windows)
    x = np.stack([np.asarray(d[w * WINDOW:(w + 1) * WINDOW], F32).reshape(STEPS, LANES) for w in windows]) if W else np.zeros((0, STEPS, LANES), F32)
    p = np.stack([np.asarray(phi[w * WINDOW:(w + 1) * WINDOW], F32).reshape(STEPS, LANES) for w in windows]) if W else np.zeros((0, STEPS, LANES), F32)
    S, Cc = np.sin(p), np.cos(p)
    assert S.dtype == F32
    mx, mn = np.full((W, LANES), -np.inf, F32), np.full((W, LANES), np.inf, F32)
    s1, s2, si, sq = (np.zeros((W, LANES), F32) for _ in range(4))
    for q in range(STEPS):
        v = x[:, q]
        mx, mn = np.maximum(mx, v), np.minimum(mn, v)
        s1 = s1 + v
        s2 = s2 + v * v
        si = si + v * S[:, q]
        sq = sq + v * Cc[:, q]
    add = lambda a, b: a + b
    out = {"peak_pos": butterfly(mx, np.maximum), "peak_neg": butterfly(mn, np.minimum),
           "mean": butterfly(s1, add) / F32(9600.0), "mean_square": butterfly(s2, add) / F32(9600.0),
           "pilot_i": butterfly(si, add) / F32(4800.0), "pilot_q": butterfly(sq, add) / F32(4800.0)}
    assert all(v.dtype == F32 for v in out.values())
    return out


class Restatement:
    """The meter of one channel as a machine that is fed calls: feed (d, phi, on) takes the next samples of the stream and returns the records the call
    completes, as (index, end_sample, {field: f32}).  What it carries between calls is the 64 x 6 accumulators.  `fault` seeds one of the mistakes the
    checker has to catch: "drop" (the first sample of every call but the first is not accumulated), "swap" (lanes 3 and 40 change places in front of the
    butterfly), "late" (the windows begin one sample late), "pilot9600" (the pilot sums divided by 9600)."""

    def __init__(self, fault=None):
        self.fault = fault
        self.j = 0
        self.active = False            # the window in progress has been metered from its start
        self._reset()

    def _reset(self):
        self.mx, self.mn = np.full(LANES, -np.inf, F32), np.full(LANES, np.inf, F32)
        self.s = np.zeros((4, LANES), F32)

    def feed(self, d, phi, on=True):
        d, phi = np.asarray(d, F32), np.asarray(phi, F32)
        S, Cc = np.sin(phi), np.cos(phi)
        shift = 1 if self.fault == "late" else 0
        recs = []
        if not on:
            self.active = False
        for n in range(d.size):
            j = self.j + n
            i = (j - shift) % WINDOW
            if on and i == 0 and j >= shift:
                self.active = True
                self._reset()
            if on and self.active and not (self.fault == "drop" and n == 0 and self.j > 0):
                l, v = i % LANES, d[n]
                self.mx[l], self.mn[l] = max(self.mx[l], v), min(self.mn[l], v)
                self.s[0, l] = self.s[0, l] + v
                self.s[1, l] = self.s[1, l] + v * v
                self.s[2, l] = self.s[2, l] + v * S[n]
                self.s[3, l] = self.s[3, l] + v * Cc[n]
            if on and self.active and i == WINDOW - 1:
                mx, mn, s = self.mx.copy(), self.mn.copy(), self.s.copy()
                if self.fault == "swap":
                    for a in (mx, mn):
                        a[[3, 40]] = a[[40, 3]]
                    s[:, [3, 40]] = s[:, [40, 3]]
                add = lambda a, b: a + b
                pd = F32(9600.0) if self.fault == "pilot9600" else F32(4800.0)
                w = (j - shift) // WINDOW
                recs.append((w, (w + 1) * WINDOW, {
                    "peak_pos": butterfly(mx, np.maximum), "peak_neg": butterfly(mn, np.minimum),
                    "mean": butterfly(s[0], add) / F32(9600.0), "mean_square": butterfly(s[1], add) / F32(9600.0),
                    "pilot_i": butterfly(s[2], add) / pd, "pilot_q": butterfly(s[3], add) / pd}))
                self.active = False
        self.j += d.size
        return recs


MOD_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("peak_pos", np.float32), ("peak_neg", np.float32), ("mean", np.float32),
                      ("mean_square", np.float32), ("pilot_i", np.float32), ("pilot_q", np.float32)])


def as_records(recs):
    """Restatement.feed's records as a MOD_DTYPE array"""
    out = np.zeros(len(recs), MOD_DTYPE)
    for k, (w, e, f) in enumerate(recs):
        out[k]["index"], out[k]["end_sample"] = w, e
        for name, v in f.items():
            out[k][name] = v
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_records(recs, d, phi, expect_index=None, k_ulp=SINCOS_ULP, verbose=False):
    """recs: MOD_DTYPE records of one channel; d, phi: the channel's taps from fm sample 0 on, covering every record's window.
    index and end_sample, the two peaks, the mean and the mean square must EQUAL the restatement's bit for bit.  The pilot fields must lie within
    2 x level + k 2^-23 mean |d| of the float64 model: `level` is what the restatement (numpy's f32 sine) reaches against the model on the same records --
    the rounding of 150 additions per lane and the butterfly, which the device shares --, the factor 2 the repository's rule for a restatement that
    cannot be bit-exact; the second term is the device's own sine: k ulp of a value below 1, 2^-24 k, on every product, over 4800.
    Returns the largest pilot error and its bound, for the reports."""
    recs = np.asarray(recs)
    if expect_index is not None:
        assert list(recs["index"]) == list(expect_index), (list(recs["index"]), list(expect_index))
    if recs.size == 0:
        return 0.0, 0.0
    windows = [int(w) for w in recs["index"]]
    assert np.array_equal(recs["end_sample"], (recs["index"] + 1) * WINDOW), "end_sample"
    r32, m64 = restate_windows(d, phi, windows), model_f64(d, phi, windows)
    for name in FIELDS_EXACT:
        bad = np.nonzero(bits(recs[name]) != bits(r32[name]))[0]
        assert bad.size == 0, "%s differs from the restatement in window %d: %r against %r" % (name, windows[bad[0]], recs[name][bad[0]], r32[name][bad[0]])
    worst, worst_bound = 0.0, 0.0
    for name in FIELDS_PILOT:
        level = float(np.max(np.abs(r32[name].astype(np.float64) - m64[name])))
        bound = 2.0 * level + k_ulp * 2.0 ** -23 * m64["mean_abs"]
        err = np.abs(recs[name].astype(np.float64) - m64[name])
        if verbose:
            print("meter %s: error %.3e, restatement's level %.3e, bound %.3e" % (name, err.max(), level, bound.min()))
        bad = np.nonzero(err > bound)[0]
        assert bad.size == 0, "%s of window %d: %r, model %r, error %.3e > %.3e" % (name, windows[bad[0]], recs[name][bad[0]], m64[name][bad[0]], err[bad[0]], bound[bad[0]])
        if err.max() > worst:
            worst, worst_bound = float(err.max()), float(bound[int(np.argmax(err))])
    return worst, worst_bound

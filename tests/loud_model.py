"""The programme audio meter (include/fmx.h fmx_audio_record) restated: a float64 model of a window's fields (scipy's lfilter), the f32
restatement in the contract's own order -- twice: whole windows at once (restate_windows, what the checker uses) and a machine that is fed calls
(Machine, which also takes the seeded faults of the checker's own test) --, the checker that compares a handle's records with both, and an
independent numpy implementation of the BS.1770-4 figures fmx_audio_loudness reports.

pcm is [channels, frames, 2] float32 from PCM frame 0 of the handle on: the values its calls returned, behind each other."""
import numpy as np
from scipy.signal import lfilter

WINDOW, RING = 4800, 64
F32 = np.float32
# BS.1770-4's K-weighting at 48 kHz: {b0, b1, b2, a1, a2} of the high shelf and of the high-pass
K_DECIMAL = ((1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585),
             (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621))
K32 = np.array(K_DECIMAL, F32)            # what the machines run with
K64 = K32.astype(np.float64)              # ... and the float64 model: the same numbers, so that the distance between the two is arithmetic alone
FIELDS = ("peak_l", "peak_r", "ms_l", "ms_r", "kms_l", "kms_r", "cross")
AUDIO_DTYPE = np.dtype([("index", np.int64), ("end_frame", np.int64), ("peak_l", np.float32), ("peak_r", np.float32), ("ms_l", np.float32),
                        ("ms_r", np.float32), ("kms_l", np.float32), ("kms_r", np.float32), ("cross", np.float32), ("reserved", np.int32)])


def first_window(start):
    """the first window that lies wholly at or behind frame `start`"""
    return -(-start // WINDOW)


def k_weight_f64(x, coef=K64):
    """x [..., frames] float64 through the two sections, from zero states"""
    for b0, b1, b2, a1, a2 in coef:
        x = lfilter([b0, b1, b2], [1.0, a1, a2], x, axis=-1)
    return x


def model_f64(pcm, start=0, coef=K64):
    """{field: [channels, nwin] float64} and the index of the first window: the fields in float64 on the f32 samples, the filters started from zero at
    frame `start`, for every whole window at or behind it."""
    x = np.asarray(pcm, np.float64)[:, start:, :]
    y = k_weight_f64(np.moveaxis(x, 1, 2))                      # [ch, ear, frames]
    w0 = first_window(start)
    off = w0 * WINDOW - start
    nwin = max(0, (x.shape[1] - off) // WINDOW)
    xs = x[:, off:off + nwin * WINDOW].reshape(x.shape[0], nwin, WINDOW, 2)
    ys = y[:, :, off:off + nwin * WINDOW].reshape(x.shape[0], 2, nwin, WINDOW)
    out = {}
    for e, ear in enumerate("lr"):
        out["peak_" + ear] = np.abs(xs[..., e]).max(axis=2) if nwin else np.zeros((x.shape[0], 0))
        out["ms_" + ear] = (xs[..., e] ** 2).sum(axis=2) / 4800.0
        out["kms_" + ear] = (ys[:, e] ** 2).sum(axis=2) / 4800.0
    out["cross"] = (xs[..., 0] * xs[..., 1]).sum(axis=2) / 4800.0
    return out, w0


def biquad_step(v, t1, t2, c):
    """one frame of one transposed direct form II section in f32, every product and sum a numpy operation of its own (nothing fused)"""
    b0, b1, b2, a1, a2 = c
    p = b0 * v
    o = p + t1
    p = b1 * v
    q = a1 * o
    d = p - q
    t1 = d + t2
    p = b2 * v
    q = a2 * o
    t2 = p - q
    return o, t1, t2


def restate_windows(pcm, start=0, kweight=True):
    """(AUDIO_DTYPE array [channels, nwin], index of the first window): the contract's arithmetic on whole windows.  The filters run frame by frame over all
    channels and ears at once, from zero states at frame `start`; the window sums then run position by position over all windows at once.
    (kweight = False leaves the filters out and kms_l, kms_r at zero: for streams too long to walk frame by frame in a test.)"""
    x = np.ascontiguousarray(np.asarray(pcm, F32)[:, start:, :])
    nch, n = x.shape[0], x.shape[1]
    y = np.zeros_like(x)
    t = np.zeros((4, nch, 2), F32)
    for i in range(n if kweight else 0):
        o, t[0], t[1] = biquad_step(x[:, i], t[0], t[1], K32[0])
        y[:, i], t[2], t[3] = biquad_step(o, t[2], t[3], K32[1])
    w0 = first_window(start)
    off = w0 * WINDOW - start
    nwin = max(0, (n - off) // WINDOW)
    xs = x[:, off:off + nwin * WINDOW].reshape(nch, nwin, WINDOW, 2)
    ys = y[:, off:off + nwin * WINDOW].reshape(nch, nwin, WINDOW, 2)
    pk, s2, z = (np.zeros((nch, nwin, 2), F32) for _ in range(3))
    sx = np.zeros((nch, nwin), F32)
    for i in range(WINDOW if nwin else 0):
        v, o = xs[:, :, i], ys[:, :, i]
        pk = np.maximum(pk, np.abs(v))
        s2 = s2 + v * v
        z = z + o * o
        sx = sx + v[..., 0] * v[..., 1]
    out = np.zeros((nch, nwin), AUDIO_DTYPE)
    out["index"] = w0 + np.arange(nwin)[None, :]
    out["end_frame"] = (out["index"] + 1) * WINDOW
    d = F32(4800.0)
    for e, ear in enumerate("lr"):
        out["peak_" + ear], out["ms_" + ear], out["kms_" + ear] = pk[..., e], s2[..., e] / d, z[..., e] / d
    out["cross"] = sx / d
    assert (s2 / d).dtype == F32
    return out, w0


class Machine:
    """The meter of one channel as a machine that is fed calls: feed (pcm [frames, 2], on) takes the stream's next frames and returns the records the call
    completes (an AUDIO_DTYPE array).  What it carries between calls is its 16 floats.  `fault` seeds one of the mistakes the checker has to catch:
    "drop" (the first frame of every call but the first is not walked), "swap" (the ears change places), "late" (the windows begin one frame late),
    "zero" (the filter states are zeroed at every call boundary), "w9600" (the finishing divisions' 4800 written as 9600)."""

    def __init__(self, fault=None):
        self.fault = fault
        self.m = 0
        self.running = False           # the meter was on in the last piece
        self.active = False            # the window in progress has been metered from its start
        self.t = np.zeros((4, 2), F32)
        self._clear()

    def _clear(self):
        self.pk, self.s2, self.z, self.sx = np.zeros(2, F32), np.zeros(2, F32), np.zeros(2, F32), F32(0)

    def feed(self, pcm, on=True):
        x = np.asarray(pcm, F32).reshape(-1, 2)
        if self.fault == "swap":
            x = x[:, ::-1]
        win = WINDOW
        shift = 1 if self.fault == "late" else 0
        recs = []
        if x.shape[0] == 0:            # (a piece without frames covers none: it switches nothing)
            pass
        elif not on:
            self.running = self.active = False
        else:
            if not self.running:
                self.t[:] = 0
                self._clear()
            elif self.fault == "zero":
                self.t[:] = 0
            self.running = True
            for n in range(x.shape[0]):
                m = self.m + n
                i = (m - shift) % win
                if i == 0 and m >= shift:
                    self.active = True
                    self._clear()
                if self.fault == "drop" and n == 0 and self.m > 0:
                    continue
                v = x[n]
                o, self.t[0], self.t[1] = biquad_step(v, self.t[0], self.t[1], K32[0])
                y, self.t[2], self.t[3] = biquad_step(o, self.t[2], self.t[3], K32[1])
                self.pk = np.maximum(self.pk, np.abs(v))
                self.s2 = self.s2 + v * v
                self.z = self.z + y * y
                self.sx = self.sx + v[0] * v[1]
                if self.active and i == win - 1:
                    w, d = (m - shift) // win, F32(9600.0 if self.fault == "w9600" else 4800.0)
                    r = np.zeros(1, AUDIO_DTYPE)
                    r["index"], r["end_frame"] = w, (w + 1) * win
                    for e, ear in enumerate("lr"):
                        r["peak_" + ear], r["ms_" + ear], r["kms_" + ear] = self.pk[e], self.s2[e] / d, self.z[e] / d
                    r["cross"] = self.sx / d
                    recs.append(r)
                    self.active = False
        self.m += x.shape[0]
        return np.concatenate(recs) if recs else np.zeros(0, AUDIO_DTYPE)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_channels(recs_list, pcm, expect_index=None, start=0, verbose=False, label="audio meter", kweight=True):
    """recs_list [k]: AUDIO_DTYPE records of channel k; pcm [channels, frames, 2]: the channels' PCM from frame 0 on, covering every record's window;
    start: the frame at which the filters started from zero (the first frame of the piece that switched the meter on).  Every field of every record must
    EQUAL the restatement's bit for bit -- no transcendental function is involved.  Returns the largest distance of ms / kms from the float64 model,
    relative.  (The restatement is computed once, for all channels at once; kweight = False compares every field but kms_l and kms_r.)"""
    pcm = np.asarray(pcm, F32)
    assert len(recs_list) == pcm.shape[0]
    last = max([int(r["end_frame"].max()) for r in recs_list if r.size] + [0])
    assert pcm.shape[1] >= last, "the PCM does not cover window %d" % (last // WINDOW - 1)
    r32, w0 = restate_windows(pcm[:, :last], start, kweight)
    m64, _ = model_f64(pcm[:, :last], start)
    worst = 0.0
    for c, recs in enumerate(recs_list):
        recs = np.asarray(recs)
        if expect_index is not None:
            assert list(recs["index"]) == list(expect_index), (c, list(recs["index"]), list(expect_index))
        if recs.size == 0:
            continue
        assert np.array_equal(recs["end_frame"], (recs["index"] + 1) * WINDOW), "end_frame"
        assert not np.any(recs["reserved"]), "reserved"
        k = recs["index"] - w0
        assert k.min() >= 0, "window %d lies in front of the switch-on" % recs["index"].min()
        for name in FIELDS if kweight else [f for f in FIELDS if f[0] != "k"]:
            want = r32[name][c][k]
            bad = np.nonzero(bits(recs[name]) != bits(want))[0]
            assert bad.size == 0, "channel %d: %s differs from the restatement in window %d: %r against %r (%d of %d windows differ)" % (
                c, name, recs["index"][bad[0]], recs[name][bad[0]], want[bad[0]], bad.size, recs.size)
            if name[:2] in ("ms", "km"):
                ref = m64[name][c][k]
                ok = ref > 0
                if np.any(ok):
                    worst = max(worst, float(np.max(np.abs(recs[name][ok].astype(np.float64) - ref[ok]) / ref[ok])))
    if verbose:
        print("%s: %d records equal the restatement; ms / kms within %.2e of float64, relative" % (label, sum(r.size for r in recs_list), worst))
    return worst


def check_records(recs, pcm, expect_index=None, start=0, verbose=False, label="audio meter", kweight=True):
    """... of ONE channel: recs its records, pcm [frames, 2] its PCM"""
    return check_channels([recs], np.asarray(pcm)[None], expect_index, start, verbose, label, kweight)


# ---- BS.1770-4 on records, independently of the library: every 400 ms block as a row of a matrix
def lufs(z):
    z = np.asarray(z, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(z > 0, -0.691 + 10.0 * np.log10(np.where(z > 0, z, 1.0)), -np.inf)


def loudness_numpy(recs):
    recs = np.asarray(recs)
    n = recs.size
    z = recs["kms_l"].astype(np.float64) + recs["kms_r"].astype(np.float64)
    idx = recs["index"]

    def consecutive(a, b):
        return b - a >= 1 and a >= 0 and np.array_equal(idx[a:b], idx[a] + np.arange(b - a))
    blocks = np.array([z[i - 3:i + 1].mean() for i in range(3, n) if consecutive(i - 3, i + 1)])
    out = {"momentary_lufs": float(lufs(z[n - 4:].mean())) if n >= 4 and consecutive(n - 4, n) else -np.inf,
           "short_term_lufs": float(lufs(z[n - 30:].mean())) if n >= 30 and consecutive(n - 30, n) else -np.inf,
           "integrated_lufs": -np.inf, "blocks_total": int(blocks.size), "blocks_gated": 0}
    absolute = blocks[lufs(blocks) > -70.0] if blocks.size else blocks
    if absolute.size:
        rel = float(lufs(absolute.mean())) - 10.0
        gated = absolute[lufs(absolute) > rel]
        out["blocks_gated"] = int(gated.size)
        if gated.size:
            out["integrated_lufs"] = float(lufs(gated.mean()))
    den = np.sqrt(recs["ms_l"].astype(np.float64).sum() * recs["ms_r"].astype(np.float64).sum())
    out["correlation"] = float(recs["cross"].astype(np.float64).sum() / den) if den > 0 else 0.0
    for ear in "lr":
        p = float(recs["peak_" + ear].max()) if n else 0.0
        out["peak_dbfs_" + ear] = 20.0 * np.log10(p) if p > 0 else -np.inf
    return out


def records_f64(pcm):
    """AUDIO_DTYPE records of one channel [frames, 2] from the float64 model (for signals too long to restate frame by frame)"""
    m, w0 = model_f64(np.asarray(pcm)[None], 0)
    out = np.zeros(m["cross"].shape[1], AUDIO_DTYPE)
    out["index"] = w0 + np.arange(out.size)
    out["end_frame"] = (out["index"] + 1) * WINDOW
    for name in FIELDS:
        out[name] = m[name][0]
    return out

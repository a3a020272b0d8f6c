"""Model of the demodulator pre-pass (fmx_demod.hip: disc_kernel, afc_kernel <VAR>, nsq_kernel) -- link D' of a channel on the PLL or AM decoder
or behind a squelch, from its own fm-rate IQ to FMX_TAP_DEMOD -- for sample-by-sample comparisons on the stream the kernels themselves read.  The
oracle library and numpy only; nothing is read from the library under test.  A helper module (not a conftest): tests/test_prepass_model_cpu.py
proves the model bit-identical to an oracle chain, the call list's coverage, the decision margins, and that the comparators catch and locate
seeded defects; tests/test_gpu_prepass_per_sample.py holds the kernels to it.

  D' (z)  =  fmo_demod_demodulate per sample on ONE long-lived demodulator          (fm-demodulator.cpp:111-241, pllC.cpp:67-90)
             followed by fmo_squelch_noise, or fmo_squelch_level fed the demodulator's carrier level of that sample, on ONE long-lived squelch
                                                                                  (squelchClass.cpp:33-113, fm-processor.cpp:499-509)
The oracle taps DEMOD behind the squelch (fm_oracle.c process_block), and so does FMX_TAP_DEMOD of a pre-pass channel.  Besides DEMOD the model gives
per sample fm_afc (get_DcComponent: what the metaData snapshot behind fm sample 96000 reads), the carrier level and the squelch flag, and at every
decision of a squelch (every 9600 counted samples) the deciding quantity's distance to its threshold.  A squelch slider (fmo_squelch_set_level), a
decoder and a squelch mode can change at given samples; a squelch that is off rests (its count, averages and filter memories keep their values), and
so does pllC while neither the PLL nor the AM decoder runs -- the reference's objects do.

Every number an assertion uses is a constant of the reference, a contract value of include/fmx.h, or measured here from the reference alone and
doubled (DESIGN.md section 5 repeats them).
"""
import ctypes as C

import numpy as np

import oracle_lib as ol
import stage_b_model as sb

FM_RATE = sb.FM_RATE
TILE = 16                      # rows of a work-array tile (WT): afc_kernel's and nsq_kernel's unit
HOLD = FM_RATE // 20           # a squelch decides every 9600 counted samples (mySquelch (1, 70000, fmRate / 20, fmRate) fm-processor.cpp:87)
SNAP = FM_RATE >> 1            # the metaData snapshot is taken behind fm sample 96000, the 96001st (++myCount > fmRate / 2, fm-processor.cpp:662-684)
NSQ_LAG = 9                    # nsq_kernel's cascades hand a sample on nine steps behind its entry: a call's last nine samples leave in the drain
HW_SINE = sb.HW_SINE           # include/fmx.h: the GPU's sine unit against the reference's table entry, 1.2e-7

# ------------------------------------------------------------------------------------------------ measured on the CPU from the reference alone
# (tests/test_prepass_model_cpu.py re-measures each and holds it against these records within a quarter either way)
# Decoder 2: the reference's own pllC with its SinCos table moved by up to HW_SINE per entry (three random draws and a table moved away from zero
# by the full amount, stage_b_model's one-sided table), against the unmoved reference, on every programme below; the worst sample, of the DEMOD
# peak: 7.94e-5 (stereo), 7.59e-5 (fade), 7.66e-5 (silence).  It is a matter of table entries: the median sample is bit-identical, 10 ... 14 % of the
# samples are off by one or two entries of compAtan's table times (1 - Beta) (one is 4.2e-5 of the peak) -- an index that slips moves the NCO's phase
# by 0.93 of an entry, and the next arc-tangents answer with the neighbouring entries until the two loops happen to meet again.  So the slips are not
# isolated and link D's share rule does not apply: the bound is the plain one, twice the worst sample.
REF_PLL_WORST = 7.94e-5
PLL_BOUND = 2.0 * REF_PLL_WORST
# ... and the largest distance of fm_afc (get_DcComponent) between the same runs at any sample, rad per sample: 2.09e-8 for decoder 2, 3.35e-8 for the AM
# decoder -- whose DEMOD does not pass through pllC and stays bit-identical under every table, but whose AFC is the mean of pllC's increment
REF_PLL_AFC = 3.35e-8
PLL_AFC_BOUND = 2.0 * REF_PLL_AFC

# ------------------------------------------------------------------------------------------------ decision margins
LSQ_VALUE, NSQ_VALUE = 50, 80   # set_squelchValue of the level / noise squelch kinds: thresholds 10^((50 - 80) / 30) = 0.1 and 1 - 80 / 100 = 0.2
LSQ_SLIDER, NSQ_SLIDER = 68, 95 # ... and where the `slider` kinds move them at a call boundary
LSQ_MARGIN = 1e-3               # |carrier level - levelThr| at every decision
NSQ_MARGIN = 1e-3               # the distance of avgHigh to the nearer edge of the hysteresis band avgLow * noiseThr -+ 0.001 at every decision


class Squelch8(C.Structure):    # the head of fmo_squelch (fm_oracle.h)
    _fields_ = [("noiseThr", C.c_float), ("levelThr", C.c_float), ("avgHigh", C.c_float), ("avgLow", C.c_float),
                ("hold", C.c_int32), ("rate", C.c_int32), ("count", C.c_int32), ("suppress", C.c_int32)]


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Link:
    """One channel's demodulator and squelch, long-lived as fmProcessor's are."""

    def __init__(self, decoder=3, squelch_mode=0, squelch_value=None, sincos=None):
        self.L = L = ol.oracle()
        self.d = L.fmo_demod_new(FM_RATE)
        self.q = L.fmo_squelch_new(1, 70000, HOLD, FM_RATE)
        self.sq = C.cast(self.q, C.POINTER(Squelch8)).contents
        self.decoder, self.mode = decoder, squelch_mode
        L.fmo_demod_set_decoder(self.d, decoder)
        if sincos is not None:
            L.fmo_demod_test_set_sincos(self.d, fptr(np.ascontiguousarray(sincos, np.float32)))
        if squelch_value:                                   # (a value of 0 is oldSquelchValue: nothing is set, fm-processor.cpp:410-413)
            L.fmo_squelch_set_level(self.q, squelch_value)
        self.n = 0
        self.decisions = []                                 # (sample, mode, quantity, threshold, margin, flag behind it)

    def set(self, what, value):
        if what == "decoder":
            self.decoder = value
            self.L.fmo_demod_set_decoder(self.d, value)
        elif what == "squelch_mode":
            self.mode = value
        elif what == "squelch_value":
            self.L.fmo_squelch_set_level(self.q, value)
        else:
            raise KeyError(what)

    def feed(self, z):
        """The next samples z [n, 2] -> dict of per-sample arrays: raw (in front of the squelch), demod (behind it), afc, carrier, flag."""
        z = np.ascontiguousarray(z, np.float32).reshape(-1, 2)
        n = z.shape[0]
        raw, afc, car = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.L.fmo_demod_feed(self.d, fptr(z), n, fptr(raw), fptr(afc), fptr(car))
        dem, flag = raw.copy(), np.zeros(n, np.uint8)
        i = 0
        while self.mode and i < n:                          # up to and with the next decision, then look at what decided
            m = min(n - i, self.sq.hold - self.sq.count)
            decides = m == self.sq.hold - self.sq.count
            o, fl = np.zeros(m, np.float32), np.zeros(m, np.uint8)
            self.L.fmo_squelch_run(self.q, fptr(np.ascontiguousarray(raw[i:i + m])), fptr(np.ascontiguousarray(car[i:i + m])) if self.mode == 2 else None,
                                   fptr(o), fl.ctypes.data_as(C.POINTER(C.c_uint8)), m)
            dem[i:i + m], flag[i:i + m] = o, fl
            i += m
            if decides:
                if self.mode == 2:
                    qty, thr = float(car[i - 1]), float(self.sq.levelThr)
                    margin = abs(qty - thr)
                else:
                    qty, thr = float(self.sq.avgHigh), float(np.float32(self.sq.avgLow) * np.float32(self.sq.noiseThr))
                    margin = abs(qty - thr) - 0.001 if self.sq.noiseThr >= 0.001 else np.inf
                self.decisions.append((self.n + i - 1, self.mode, qty, thr, margin, int(fl[-1])))
        self.n += n
        return dict(raw=raw, demod=dem, afc=afc, carrier=car, flag=flag)

    def close(self):
        if self.d:
            self.L.fmo_demod_free(self.d)
            self.L.fmo_squelch_free(self.q)
            self.d = self.q = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def model(z, decoder=3, squelch_mode=0, squelch_value=None, events=(), sincos=None):
    """D' over the whole stream z [n, 2] from fm sample 0.  events: (sample, what, value) with what in decoder / squelch_mode / squelch_value,
    applied in front of that sample.  -> dict of per-sample arrays (Link.feed) plus `decisions`."""
    z = np.ascontiguousarray(z, np.float32).reshape(-1, 2)
    link = Link(decoder, squelch_mode, squelch_value, sincos)
    cuts = sorted(set([0, z.shape[0]] + [int(e[0]) for e in events if 0 < e[0] < z.shape[0]]))
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        for s, what, value in events:
            if s == a:
                link.set(what, value)
        parts.append(link.feed(z[a:b]))
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["decisions"] = list(link.decisions)
    link.close()
    return out


def check_margins(m, name="", pll_peak=None):
    """Every decision of the model keeps LSQ_MARGIN / NSQ_MARGIN; behind the PLL decoder the noise squelch's margin also exceeds what REF_PLL_WORST
    can move avgHigh against avgLow * noiseThr by: both averages are of |a filter's output| with a pass-band gain of one, so 2 * PLL_BOUND of the peak."""
    for s, mode, qty, thr, margin, _ in m["decisions"]:
        need = LSQ_MARGIN if mode == 2 else NSQ_MARGIN
        assert margin >= need, "%s: the decision at fm sample %d comes within %.3e of its threshold (%.4g against %.4g): choose another input" % (name, s, margin, qty, thr)
        if pll_peak is not None and mode == 1:
            assert margin > 2.0 * PLL_BOUND * pll_peak, (name, s, margin)
    return len(m["decisions"])


# ------------------------------------------------------------------------------------------------ the kinds
KINDS = {
    "am": dict(decoder=1),
    "pll": dict(decoder=2),
    "mixed+nsq": dict(decoder=3, squelch_mode=1, squelch_value=NSQ_VALUE),
    "mixed+lsq": dict(decoder=3, squelch_mode=2, squelch_value=LSQ_VALUE),
    "real+nsq": dict(decoder=5, squelch_mode=1, squelch_value=NSQ_VALUE),
    "real+lsq": dict(decoder=5, squelch_mode=2, squelch_value=LSQ_VALUE),
    "diff+nsq": dict(decoder=6, squelch_mode=1, squelch_value=NSQ_VALUE),
    "diff+lsq": dict(decoder=6, squelch_mode=2, squelch_value=LSQ_VALUE),
    "am+lsq": dict(decoder=1, squelch_mode=2, squelch_value=LSQ_VALUE),
    "pll+nsq": dict(decoder=2, squelch_mode=1, squelch_value=NSQ_VALUE),
    "pll+lsq": dict(decoder=2, squelch_mode=2, squelch_value=LSQ_VALUE),
    # a slider moved at a call boundary (SLIDER_CALL): the new threshold holds from that call's first sample (fm-processor.cpp:410-413 at a block start)
    "slider lsq": dict(decoder=3, squelch_mode=2, squelch_value=LSQ_VALUE, slider=LSQ_SLIDER),
    "slider nsq": dict(decoder=6, squelch_mode=1, squelch_value=NSQ_VALUE, slider=NSQ_SLIDER),
}
EXACT = [k for k, v in KINDS.items() if v["decoder"] != 2]          # bit-identical to the model; the others within PLL_BOUND


def kind_model(z, kind, starts, **kw):
    kd = KINDS[kind]
    ev = [(int(starts[SLIDER_CALL]), "squelch_value", kd["slider"])] if "slider" in kd else []
    return model(z, kd["decoder"], kd.get("squelch_mode", 0), kd.get("squelch_value"), ev, **kw)


# ------------------------------------------------------------------------------------------------ the call list and its proof
SHORT = [1, 2, 9, 10, 11, 15, 16, 17, 31, 32, 33, 47, 64, 65, 80]    # shorter than the noise squelch's lag, than a tile; 1 ... 5 whole tiles for the depth-2 pipeline
SHIFT = 11
# fm samples per call.  Decisions fall behind fm samples 9599, 19199, ... 95999 (a squelch that is on from sample 0), the snapshot behind 96000:
#            start    decision / snapshot at
#  9157        433
#  4003       9590    9599: row 9 of the first tile
#  8004      13593    19199: row 5606, a whole tile in the middle
#  7214      21597    28799: row 7202 of the ragged last tile (rows 7200 ... 7213), in front of the drain
#  9589      28811    38399: the call's last sample
#  9599      38400
#     6      47999    47999: the call's first sample (a call shorter than the noise squelch's lag)
#  9597      48005    57599: row 9594, the third sample from the end: leaves nsq_kernel in the drain behind the call's end
#  9591      57602
#     8      67193    67199: row 6 of a call shorter than the lag
#  9612      67201    76799: the last whole tile
#  9586      76813
#     1      86399    86399: a call of one sample
#  9589      86400
#     9      95989
#    80      95998    95999: row 1; 96000 (snapshot): row 2 of a whole tile
#  4022      96078
LONG = [9157, 4003, 8004, 7214, 9589, 9599, 6, 9597, 9591, 8, 9612, 9586, 1, 9589, 9, 80, 4022]
CALLS_FM = SHORT + LONG                                               # 100 100 fm samples
# the second variant: one early call longer by SHIFT samples (the last one shorter): every later call starts SHIFT samples later, and the call of 9
# samples now starts AT the snapshot sample -- the snapshot on a call's first row and in a ragged tail
CALLS_FM_B = SHORT + [LONG[0] + SHIFT] + LONG[1:-1] + [LONG[-1] - SHIFT]
CALLS, CALLS_B = [12 * n for n in CALLS_FM], [12 * n for n in CALLS_FM_B]   # input samples
SLIDER_CALL = len(SHORT) + 5                                          # the call that starts at fm sample 38400: four decisions in front, six behind
N_FM = sum(CALLS_FM)


def call_starts(calls_fm):
    return np.concatenate([[0], np.cumsum(calls_fm)[:-1]]).astype(np.int64)


def place(index, calls_fm):
    """-> (call, row of the call, the call's length)."""
    st = call_starts(calls_fm)
    k = int(np.searchsorted(st, index, side="right") - 1)
    return k, int(index - st[k]), int(calls_fm[k])


def coverage(calls_fm=None, calls_fm_b=None):
    """Asserts what the call lists must contain (the module's comment at LONG); -> a description of where every decision and the snapshot fall."""
    a = CALLS_FM if calls_fm is None else calls_fm
    b = CALLS_FM_B if calls_fm_b is None else calls_fm_b
    assert sum(a) == sum(b) and sum(a) > SNAP + 2 * TILE and len(a) == len(b)
    for n in SHORT:
        assert n in a, "no call of %d fm samples" % n
    assert {n % TILE for n in a} == set(range(TILE)), "call lengths miss residues %s modulo 16" % sorted(set(range(TILE)) - {n % TILE for n in a})
    seen, lines = set(), []
    for d in range(HOLD - 1, sum(a), HOLD):
        k, r, n = place(d, a)
        whole = r < n // TILE * TILE
        tags = set()
        if r < TILE and whole: tags.add("first tile")
        if whole and TILE <= r < (n // TILE - 1) * TILE: tags.add("middle tile")
        if not whole and n >= TILE and r < n - NSQ_LAG: tags.add("ragged tail")
        if r == n - 1 and n > 1: tags.add("last sample")
        if r == 0: tags.add("first sample")
        if n - NSQ_LAG <= r < n - 1: tags.add("drain")
        seen |= tags
        lines.append("decision behind %d: call %d (%d samples), tile %d, row %d: %s" % (d, k, n, r // TILE, r % TILE, ", ".join(sorted(tags)) or "-"))
    need = {"first tile", "middle tile", "ragged tail", "last sample", "first sample", "drain"}
    assert need <= seen, "no decision in: %s" % sorted(need - seen)
    k, r, n = place(SNAP, a)
    assert r < n // TILE * TILE, "variant A: the snapshot row is not in a whole tile"
    lines.append("snapshot behind %d, variant A: call %d (%d samples), tile %d, row %d" % (SNAP, k, n, r // TILE, r % TILE))
    k, r, n = place(SNAP, b)
    assert r == 0 and n < TILE, "variant B: the snapshot row is not a call's first row in a ragged tail"
    lines.append("snapshot behind %d, variant B: call %d (%d samples), row %d" % (SNAP, k, n, r))
    diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert len(diff) == 2 and b[diff[0]] - a[diff[0]] == a[diff[1]] - b[diff[1]] and diff[1] == len(a) - 1 and call_starts(a)[diff[0]] + a[diff[0]] < HOLD
    return lines


# ------------------------------------------------------------------------------------------------ inputs
# fm samples at which the fading carrier changes level: right behind a decision, so that the next one finds settled averages (the carrier level has a
# time constant of 1000 samples, the noise squelch's averages of 1920).  High over decisions 1-2, 5-6, 9-10; low over 3-4 and 7-8: either squelch
# closes at the third decision, opens at the fifth, closes at the seventh and opens at the ninth.
FADE_EDGES = [2 * HOLD, 4 * HOLD, 6 * HOLD, 8 * HOLD]
FADE_LOW = 0.004                 # of the carrier: 0.002 at the antenna against the level squelch's 0.1 ... and below the noise
FADE_NOISE = 0.003               # per component, added behind the envelope (a fading carrier does not take the receiver's noise with it)
SILENCE = 24000                  # input samples of exact zeros in front of the `silence` programme: the limiter's 0.001 branch
PROGRAMMES = ("stereo", "fade", "silence")


def programme_iq(name, n=None):
    """Input IQ [n, 2] f32 of a programme, n input samples (default: the whole call list)."""
    n = 12 * N_FM if n is None else n
    if name == "stereo":          # a stereo programme with noise
        return ol.synth_iq(n, pilotLevel=0.12, noiseSeed=5, noiseSigma=0.004)
    if name == "fade":
        x = ol.synth_iq(n, pilotLevel=0.12, leftHz=1370.0, rightHz=630.0).astype(np.float64)
        env = np.ones(n)
        t = np.arange(n) / 12.0
        for lo, hi in zip(FADE_EDGES[0::2], FADE_EDGES[1::2]):
            env[(t >= lo + 64) & (t < hi + 64)] = FADE_LOW
        noise = np.random.default_rng(20).normal(0.0, FADE_NOISE, (n, 2))
        return (x * env[:, None] + noise).astype(np.float32)
    if name == "silence":
        x = ol.synth_iq(n, pilotLevel=0.12, leftHz=700.0, rightHz=1300.0, leftAmp=0.3, rightAmp=0.4)
        x[:SILENCE] = 0.0
        return x
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the comparator
def locate(index, starts):
    """fm sample -> 'call c, tile t, row r' of the call whose read-out holds it."""
    st = np.asarray(starts, np.int64)
    k = max(int(np.searchsorted(st, index, side="right") - 1), 0)
    r = int(index - st[k])
    return "fm sample %d = call %d, tile %d, row %d" % (index, k, r // TILE, r % TILE)


def differences(got, ref):
    g, r = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert g.shape == r.shape and g.dtype == r.dtype, (g.shape, r.shape, g.dtype, r.dtype)
    return np.flatnonzero(g.view(np.uint32) != r.view(np.uint32)) if g.dtype == np.float32 else np.flatnonzero(g != r)


def check_identical(kind, channel, got, ref, starts, what="DEMOD", limit=6):
    """Bit identity; a failure names kind, channel, call, tile of 16 and row of the first differing samples."""
    bad = differences(got, ref)
    assert bad.size == 0, "%s, channel %s: %d of %d %s samples differ from the model, the first at %s" % (
        kind, channel, bad.size, np.asarray(ref).shape[0], what,
        "; ".join("%s (got %r, model %r)" % (locate(i, starts), np.asarray(got)[i].tolist(), np.asarray(ref)[i].tolist()) for i in bad[:limit]))


def check_flags(kind, channel, got_demod, m, starts):
    """A squelch kind: DEMOD is zero wherever the model's flag is set (x * 0.000f: a zero of either sign), and follows the model elsewhere -- a
    decision taken at another sample shows as a sample muted on one side only."""
    g = np.asarray(got_demod, np.float32)
    loud = np.flatnonzero((m["flag"] != 0) & (g != 0))
    assert loud.size == 0, "%s, channel %s: %d samples are not muted where the model's squelch is closed, the first at %s" % (kind, channel, loud.size, locate(loud[0], starts))
    mute = np.flatnonzero((m["flag"] == 0) & (g == 0) & (m["demod"] != 0))
    assert mute.size == 0, "%s, channel %s: %d samples are muted where the model's squelch is open, the first at %s" % (kind, channel, mute.size, locate(mute[0], starts))


def check_pll(kind, channel, got, ref, starts, skip=None):
    """Decoder 2: every sample within PLL_BOUND of the DEMOD peak.  skip: a mask of samples not judged here (the muted ones: check_flags).
    -> (the worst sample of the peak, where it fell, the share of samples that are not bit-identical)."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    peak = sb.demod_peak(ref)
    e = np.abs(g - r)
    if skip is not None:
        e = np.where(skip, 0.0, e)
    i = int(np.argmax(e))
    where = locate(i, starts)
    print("[%s, channel %s] decoder 2: worst sample %.3e of the peak %.4g at %s (bound %.3e); %.2f %% of the samples differ at all"
          % (kind, channel, e[i] / peak, peak, where, PLL_BOUND, 100 * float((e > 0).mean())))
    assert e[i] <= PLL_BOUND * peak, "%s, channel %s: %.3e of the peak exceeds the bound %.3e at %s (got %r, model %r)" % (
        kind, channel, e[i] / peak, PLL_BOUND, where, float(g[i]), float(r[i]))
    return float(e[i] / peak), where, float((e > 0).mean())


def check_snapshot(kind, channel, got, m, exact):
    """meta.dcValIf of a call at or behind the snapshot against the model's fm_afc behind sample SNAP: bitwise, or (exact False: the PLL and AM
    decoders, whose AFC follows pllC's increment) within PLL_AFC_BOUND."""
    want = np.float32(m["afc"][SNAP])
    if exact:
        assert np.float32(got).view(np.uint32) == want.view(np.uint32), "%s, channel %s: dcValIf %r, the model's fm_afc behind fm sample %d is %r" % (kind, channel, float(got), SNAP, float(want))
    else:
        assert abs(float(got) - float(want)) <= PLL_AFC_BOUND, "%s, channel %s: dcValIf %r, the model's fm_afc behind fm sample %d is %r (%.3e apart, bound %.3e)" % (
            kind, channel, float(got), SNAP, float(want), abs(float(got) - float(want)), PLL_AFC_BOUND)
    return abs(float(got) - float(want))


# ------------------------------------------------------------------------------------------------ the handles of the GPU test
PLAIN = None                                    # a channel that is no pre-pass channel: decoder 3, no squelch (stageb_kernel demodulates it)
KIND_LIST = list(KINDS)
PREFERRED = {"am": "stereo", "pll": "silence"}  # (every other kind: the fading carrier)


def full_handle(nch):
    """Every channel a pre-pass channel: channel c on kind c mod 13; its programme the kind's preferred one, moved on by one per block of 13 channels:
    c and c + 39 are twins."""
    kinds = [KIND_LIST[c % len(KIND_LIST)] for c in range(nch)]
    prog = [PROGRAMMES[(PROGRAMMES.index(PREFERRED.get(k, "fade")) + c // len(KIND_LIST)) % 3] for c, k in enumerate(kinds)]
    return kinds, prog


def sparse_handle(nch, special):
    kinds, prog = [PLAIN] * nch, ["stereo"] * nch
    for c, (k, p) in special.items():
        kinds[c], prog[c] = k, p
    return kinds, prog


def handles():
    """name -> (kinds per channel, programme per channel, probed channels, twins, batch, the arm of launch_demod_prepass's switch the population selects)."""
    f64, f70 = full_handle(64), full_handle(70)
    return {
        "1 nsq": sparse_handle(1, {0: ("mixed+nsq", "fade")}) + ([0], [], False, "AV_MIXED"),
        "1 lsq": sparse_handle(1, {0: ("real+lsq", "fade")}) + ([0], [], False, "AV_LSQ"),
        "3 pll": sparse_handle(3, {0: ("pll", "silence"), 1: ("pll+nsq", "fade")}) + ([0, 1], [], False, "AV_PLL"),
        "3 am": sparse_handle(3, {0: ("am", "stereo"), 1: ("am", "fade")}) + ([0, 1], [], False, "AV_AM"),
        "64 all": f64 + (list(range(26)) + [63], [(c, c + 39) for c in range(25)], False, "AV_ALL (PLL with AM)"),
        # channel 64: alone in the second, partly filled wave of afc_kernel
        "65 sparse": sparse_handle(65, {7: ("am", "stereo"), 64: ("am+lsq", "fade")}) + ([7, 64], [], True, "AV_ALL (AM with the level squelch)"),
        "70 all": f70 + (list(range(13)) + list(range(52, 70)), [(c, c + 39) for c in range(31)], True, "AV_ALL (PLL with AM)"),
        # channel 129: the only noise-squelch channel of its wave's triple (129, 130, 131), in the last, partly filled waves of both kernels; 100: between plain ones
        "130 sparse": sparse_handle(130, {5: ("pll", "stereo"), 100: ("diff+nsq", "fade"), 129: ("mixed+nsq", "fade")}) + ([5, 100, 129], [], True, "AV_PLL | AV_MIXED"),
    }


def prepass_arm(kinds):
    """Which arm of launch_demod_prepass's switch a population takes (fmx_needs.h needs_add, fmx_demod.hip), restated."""
    var = 0
    for k in kinds:
        if k is None:
            continue
        d, m = KINDS[k]["decoder"], KINDS[k].get("squelch_mode", 0)
        var |= (1 if d == 2 else 0) | (2 if d == 1 else 0) | (4 if m == 2 else 0) | (8 if d > 2 and m != 0 else 0)
    if var in (0, 8): return "AV_MIXED"
    if var == 1: return "AV_PLL"
    if var == 9: return "AV_PLL | AV_MIXED"
    if var == 2: return "AV_AM"
    if var in (4, 12): return "AV_LSQ"
    return "AV_ALL (PLL with AM)" if (var & 3) == 3 else ("AV_ALL (AM with the level squelch)" if (var & 6) == 6 else "AV_ALL (other)")


ARMS = {"AV_MIXED", "AV_PLL", "AV_PLL | AV_MIXED", "AV_AM", "AV_LSQ", "AV_ALL (PLL with AM)", "AV_ALL (AM with the level squelch)"}

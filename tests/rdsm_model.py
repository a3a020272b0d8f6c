"""The RDS meter (include/fmx.h fmx_rds_meter_record) restated: a float64 model of a window's six fields, the f32 restatement in the
contract's own order -- twice: whole windows at once (restate_windows, what the checker uses) and a machine that is fed pieces [m0, m1) of any length
(Machine, which also takes the seeded faults of the checker's own test) --, figures () and cal () in float64 (fmx_rds_meter_figures, fmx_rds_meter_cal),
the checker: every field of a record EQUALS the restatement bit for bit (the kernel calls no library function, so there is no tolerance anywhere between
device and restatement), and a numpy signal generator with a band-limited RDS sub-carrier (the oracle's generator sends unfiltered biphase, about 37 % of
whose power lies outside +-2.4 kHz).

z is a channel's FMX_TAP_RDS_IQ from its RDS sample 0 on, [n, 2] float32 (or complex): the values its calls' taps returned, behind each other."""
import numpy as np

WINDOW, LANES, STEPS, RING = 2560, 64, 40, 64
F32 = np.float32
FIELDS = ("p_max", "ii_mean", "qq_mean", "iq_mean", "i_mean", "q_mean")
RDSM_DTYPE = np.dtype([("index", np.int64), ("end_sample", np.int64), ("p_max", np.float32), ("ii_mean", np.float32), ("qq_mean", np.float32),
                       ("iq_mean", np.float32), ("i_mean", np.float32), ("q_mean", np.float32)])

# ---- what the tests assert, each twice what tests/test_rdsm_cpu.py measured on the oracle (DESIGN.md 4.14 lists them under these names); the signal is
# signal () below through the oracle chain (input filter 165 kHz, RDS mode 2), windows FIRST_WINDOW and later: the path's 64 000-sample delay and the
# pilot's 0.5 s lock lie in front
FIRST_WINDOW = 6
SECONDS = 2.0
NOISE_SEED = 0x5D2F1A7B
# the f32 restatement against float64 on the clean signal, 12 windows: p_max relative to itself, the second moments to ii_mean + qq_mean, the first to
# the rms of z (their own value may be near zero).  Measured 5.59e-8 / 7.37e-8 / 3.15e-8 / 3.75e-8 / 4.74e-9 / 2.28e-9
RESTATE_REL = {"p_max": 2 * 5.59e-8, "ii_mean": 2 * 7.37e-8, "qq_mean": 2 * 3.15e-8, "iq_mean": 2 * 3.75e-8, "i_mean": 2 * 4.74e-9, "q_mean": 2 * 2.28e-9}
# injection_peak_hz / injection_rms_hz against the sent peak and rms (peak x the waveform's own rms, 0.6933), relative, at 1000 / 2250 / 7500 Hz without
# a programme: peak +0.0203 / +0.0209 / +0.0220, rms +0.0181 / +0.0181 / +0.0177
INJECTION_PEAK_REL = 2 * 0.0220
INJECTION_RMS_REL = 2 * 0.0181
# 2250 Hz under config 2's programme (two 0.5-FS tones): after correction injection_rms_hz reads 0.9240 of the sent rms -- a loss of 0.0760, documented,
# not hidden -- and injection_peak_hz 1.0483 of the sent peak; axis_db 20.24
PROGRAMME_LOSS = 0.0760
PROGRAMME_PEAK_REL = 2 * 0.0483
# phase_deg of the sub-carrier on sin (3 p) against 0 (0.276) and on cos (3 p) against 90 (90.277); their difference against 90: 0.0004 clean, 0.246 at
# noise sigma 0.05
PHASE_TOL_DEG = 2 * 0.277
PHASE_DIFF_TOL_DEG = {0.0: 2 * 0.0004, 0.05: 2 * 0.246}
# carrier_hz of an added unmodulated 57 kHz component of 1000 Hz: 1020.04 (without it the meter reads 6.5 Hz)
CARRIER_REL = 2 * 0.0200
# no RDS on the air: injection_rms_hz reads 0.347 Hz, injection_peak_hz 6.87 Hz
NO_RDS_RMS_FLOOR_HZ = 2 * 0.347
NO_RDS_PEAK_FLOOR_HZ = 2 * 6.87
# axis_db falls over these noise levels (sigma per component at the input rate): 35.90 / 20.51 / 12.87 dB
NOISE_SIGMAS = (0.0, 0.02, 0.05)
AXIS_CLEAN_DB = 35.90


def as_pairs(z):
    """[n, 2] float32 of a tap in either form"""
    z = np.asarray(z)
    if np.iscomplexobj(z):
        z = np.stack([z.real, z.imag], axis=1)
    return np.ascontiguousarray(z, F32).reshape(-1, 2)


def model_f64(z, windows):
    """{field: [len (windows)] float64}: the six fields of the windows in exact arithmetic on the f32 inputs."""
    z = as_pairs(z)
    out = {k: np.zeros(len(windows)) for k in FIELDS}
    for n, w in enumerate(windows):
        a = z[w * WINDOW:(w + 1) * WINDOW].astype(np.float64)
        assert a.shape[0] == WINDOW, "window %d is not covered by the samples" % w
        i, q = a[:, 0], a[:, 1]
        out["p_max"][n] = (i * i + q * q).max()
        out["ii_mean"][n], out["qq_mean"][n], out["iq_mean"][n] = (i * i).sum() / 2560.0, (q * q).sum() / 2560.0, (i * q).sum() / 2560.0
        out["i_mean"][n], out["q_mean"][n] = i.sum() / 2560.0, q.sum() / 2560.0
    return out


def butterfly(a, op):
    """a [..., 64] f32: a [l] = a [l] op a [l xor k] for k = 32 .. 1; every lane ends with the same value, lane 0's is returned"""
    idx = np.arange(LANES)
    for k in (32, 16, 8, 4, 2, 1):
        a = op(a, a[..., idx ^ k])
    return a[..., 0]


def terms(z):
    """the per-sample f32 terms of the contract: ii, qq, p = f32 (ii + qq), f32 (I Q), I, Q -- every product and sum rounded once"""
    i, q = z[..., 0], z[..., 1]
    ii, qq = i * i, q * q
    out = ii + qq, ii, qq, i * q, i, q
    assert all(t.dtype == F32 for t in out)
    return out


_add = lambda a, b: a + b


def restate_windows(z, windows):
    """{field: [len (windows)] float32}: the contract's arithmetic -- lane l takes the samples i = 64 s + l in step order, in f32, products rounded to f32
    before they are added; the butterfly; the finishing divisions."""
    z = as_pairs(z)
    W = len(windows)
    shape = (W, STEPS, LANES, 2)
    x = np.stack([z[w * WINDOW:(w + 1) * WINDOW] for w in windows]).reshape(shape) if W else np.zeros(shape, F32)
    t = terms(x)
    mx = np.full((W, LANES), -np.inf, F32)
    s = [np.zeros((W, LANES), F32) for _ in range(5)]
    for q in range(STEPS):
        mx = np.maximum(mx, t[0][:, q])
        for k in range(5):
            s[k] = s[k] + t[k + 1][:, q]
    out = {"p_max": butterfly(mx, np.maximum)}
    for k, name in enumerate(FIELDS[1:]):
        out[name] = butterfly(s[k], _add) / F32(2560.0)
    assert all(a.dtype == F32 for a in out.values())
    return out


class Machine:
    """The meter of one channel as a machine that is fed pieces: feed (z, on) takes the next RDS samples of the channel (none while its decoder is off: such
    a piece is not fed) and returns the records the piece completes, as (index, end_sample, {field: f32}).  What it carries between pieces is the 64 x 6
    accumulators and no sample.  A piece of no samples changes nothing, whatever `on`.  `fault` seeds one of the mistakes the checker has to catch: "drop"
    (the first sample of every piece but the first is not accumulated), "swap" (lanes 3 and 40 change places in front of the butterfly), "late" (the windows
    begin one sample late), "cross" (iq_mean of I with the Q of the sample before), "sign" (the sign of q_mean), "1280" (the sums divided by 1280)."""

    def __init__(self, fault=None):
        self.fault = fault
        self.m = 0
        self.active = False            # the window in progress has been metered from its start
        self.prev_q = F32(0.0)
        self._reset()

    def _reset(self):
        self.mx = np.full(LANES, -np.inf, F32)
        self.s = np.zeros((5, LANES), F32)

    def feed(self, z, on=True):
        z = as_pairs(z)
        if z.shape[0] == 0:
            return []
        p, ii, qq, iq, si, sq = terms(z)
        if self.fault == "cross":
            iq = z[:, 0] * np.concatenate([[self.prev_q], z[:-1, 1]]).astype(F32)
        if self.fault == "sign":
            sq = -sq
        shift = 1 if self.fault == "late" else 0
        recs = []
        if not on:
            self.active = False
        for n in range(z.shape[0]):
            m = self.m + n
            i = (m - shift) % WINDOW
            if on and i == 0 and m >= shift:
                self.active = True
                self._reset()
            if on and self.active and not (self.fault == "drop" and n == 0 and self.m > 0):
                l = i % LANES
                self.mx[l] = max(self.mx[l], p[n])
                for k, t in enumerate((ii, qq, iq, si, sq)):
                    self.s[k, l] = self.s[k, l] + t[n]
            if on and self.active and i == WINDOW - 1:
                mx, s = self.mx.copy(), self.s.copy()
                if self.fault == "swap":
                    mx[[3, 40]] = mx[[40, 3]]
                    s[:, [3, 40]] = s[:, [40, 3]]
                den = F32(1280.0) if self.fault == "1280" else F32(2560.0)
                w = (m - shift) // WINDOW
                f = {"p_max": butterfly(mx, np.maximum)}
                for k, name in enumerate(FIELDS[1:]):
                    f[name] = butterfly(s[k], _add) / den
                recs.append((w, (w + 1) * WINDOW, f))
                self.active = False
        self.prev_q = z[-1, 1]
        self.m += z.shape[0]
        return recs


def as_records(recs):
    """Machine.feed's records as an RDSM_DTYPE array"""
    out = np.zeros(len(recs), RDSM_DTYPE)
    for k, (w, e, f) in enumerate(recs):
        out[k]["index"], out[k]["end_sample"] = w, e
        for name, val in f.items():
            out[k][name] = val
    return out


def records_of(fields, windows):
    """restate_windows' or model_f64's fields as an RDSM_DTYPE array (the model's rounded to f32)"""
    out = np.zeros(len(windows), RDSM_DTYPE)
    out["index"] = np.asarray(windows, np.int64)
    out["end_sample"] = (out["index"] + 1) * WINDOW
    for name in FIELDS:
        out[name] = fields[name]
    return out


def expected_windows(pieces):
    """the pure rule, sample by sample: `pieces` is a list of (n, on) -- the RDS samples a piece produced for the channel (0 while its decoder is off) and
    the meter's switch in it.  A window is valid from its first sample if the meter is on there and stops being valid with any of its samples that a piece
    with the meter off produces; the windows that end valid, in order."""
    out, m, valid = [], 0, False
    for n, on in pieces:
        for x in range(m, m + n):
            if x % WINDOW == 0:
                valid = bool(on)
            elif not on:
                valid = False
            if valid and x % WINDOW == WINDOW - 1:
                out.append(x // WINDOW)
        m += n
    return out


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_records(recs, z, expect_index=None):
    """recs: RDSM_DTYPE records of one channel; z: the channel's FMX_TAP_RDS_IQ from its RDS sample 0 on, covering every record's window.  index,
    end_sample and all six fields must EQUAL the restatement's, bit for bit."""
    recs = np.asarray(recs)
    if expect_index is not None:
        assert list(recs["index"]) == list(expect_index), (list(recs["index"]), list(expect_index))
    if recs.size == 0:
        return
    windows = [int(w) for w in recs["index"]]
    assert np.array_equal(recs["end_sample"], (recs["index"] + 1) * WINDOW), "end_sample"
    r32 = restate_windows(z, windows)
    for name in FIELDS:
        bad = np.nonzero(bits(recs[name]) != bits(r32[name]))[0]
        assert bad.size == 0, "%s differs from the restatement in window %d: %r against %r" % (name, windows[bad[0]], recs[name][bad[0]], r32[name][bad[0]])


# ---- calibration and figures, in double
def _response(taps, turns, centre=0.0):
    taps = np.asarray(taps, np.float64)
    return np.sum(taps * np.exp(-2j * np.pi * turns * (np.arange(taps.size) - centre)))


def cal(bp_taps, dec_taps, rf_stages, fmRate=192000):
    """fmx_rds_meter_cal in float64.  bp_taps: the complex 57 kHz band-pass kernel, 768 (re, im) pairs (only the real part of its result is kept: the real
    taps); dec_taps: rdsDecimator's complex kernel, 11 (re, im) pairs; rf_stages: [(real taps, rate)] of what lies in front of the demodulator -- the
    channel's front-end taps, and the input filter where it runs as a block machine."""
    bp = np.asarray(bp_taps, np.float64).reshape(-1, 2)[:, 0]
    dk = np.asarray(dec_taps, np.float64).reshape(-1, 2)
    Hbp = _response(bp, 57000.0 / fmRate, 384.0)
    D0 = complex(dk[:, 0].sum(), dk[:, 1].sum())
    rf = 1.0
    for taps, rate in rf_stages:
        rf *= 0.5 * (abs(_response(taps, 57000.0 / rate)) + abs(_response(taps, -57000.0 / rate))) / abs(_response(taps, 0.0))
    x = np.pi * 57000.0 / fmRate
    return {"gain": 3.0 * abs(Hbp) * abs(D0), "phase0_deg": float(np.degrees(np.angle(D0) + np.angle(Hbp))), "path_57k": float(rf * np.sin(x) / x)}


def hz_per_unit(fmRate=192000):
    """fmx_mod_hz_per_unit in the reference's float order (fm-demodulator.cpp:58-64, :198)"""
    F_G, Delta_F = F32(0.65 * fmRate / 2), F32(0.95 * fmRate / 2)
    B_FM = F32(2) * (Delta_F + F_G)
    K_FM = F32(float(F32(2) * B_FM) * np.pi / float(F_G))
    return float(K_FM) / 20.0 * fmRate / (2.0 * np.pi)


def figures(recs, k, hz):
    """fmx_rds_meter_figures in float64: recs an RDSM_DTYPE array or a dict of the six fields, k = cal (...), hz = hz_per_unit ()"""
    g = lambda name: np.asarray(recs[name], np.float64)
    n = g("ii_mean").size
    assert n > 0
    A, B, C, mi, mq = (g(name).sum() / n for name in FIELDS[1:])
    a, b, c = A - mi * mi, B - mq * mq, C - mi * mq
    r = np.hypot((a - b) / 2.0, c)
    lp, lm = (a + b) / 2.0 + r, (a + b) / 2.0 - r
    K = hz / (k["gain"] * k["path_57k"])
    out = {"injection_rms_hz": float(np.sqrt(max(lp - lm, 0.0)) * K), "injection_peak_hz": float(np.sqrt(max(g("p_max").max(), 0.0)) * K),
           "carrier_hz": float(np.hypot(mi, mq) * K), "windows": n}
    if lp <= 0.0:
        out["phase_deg"], out["axis_db"] = 0.0, -np.inf
    else:
        ph = float(np.fmod(0.5 * np.degrees(np.arctan2(2.0 * c, a - b)) - k["phase0_deg"], 180.0))
        out["phase_deg"] = ph + 180.0 if ph <= -45.0 else (ph - 180.0 if ph > 135.0 else ph)
        out["axis_db"] = np.inf if lm <= 0.0 else float(10.0 * np.log10(lp / lm))
    return out


# ---- the signal
BIT_RATE = 1187.5


def rds_waveform(n, fs=2304000.0, seed=11):
    """n samples of the RDS baseband of IEC 62106: differentially encoded random bits, each an impulse pair (+e at k t_d, -e at k t_d + t_d / 2) through
    H (f) = cos (pi f t_d / 4), |f| <= 2 / t_d, built in the frequency domain (periodic over the n samples); peak normalised to 1.  Returns (s, its rms)."""
    td = 1.0 / BIT_RATE
    nbits = int(n / fs * BIT_RATE)
    data = np.random.default_rng(seed).integers(0, 2, nbits)
    e = 2.0 * (np.cumsum(data) % 2) - 1.0                            # differential encoding
    kmax = int(2.0 / td * n / fs)
    f = np.arange(kmax + 1) * fs / n
    S = np.zeros(n // 2 + 1, np.complex128)
    t0 = np.arange(nbits) * td
    acc = np.zeros(kmax + 1, np.complex128)
    for lo in range(0, nbits, 256):                                  # (in blocks: bits x bins)
        ph = np.exp(-2j * np.pi * np.outer(t0[lo:lo + 256], f))
        acc += e[lo:lo + 256] @ ph
    S[:kmax + 1] = acc * (1.0 - np.exp(-2j * np.pi * f * td / 2.0)) * np.cos(np.pi * f * td / 4.0)
    s = np.fft.irfft(S, n)
    s /= np.max(np.abs(s))
    return s, float(np.sqrt(np.mean(s * s)))


def signal(seconds=SECONDS, rds_hz=2250.0, on="cos", programme=False, carrier_hz=0.0, sigma=0.0, seed=11, fs=2304000.0):
    """([n, 2] float32 IQ at 2.304 MS/s, the waveform's rms): pilot at 0.1 on sin (p), the band-limited sub-carrier at a peak deviation of rds_hz on
    cos (3 p) or sin (3 p), optionally config 2's programme (L = 0.5 sin 1000 Hz, R = 0.5 sin 400 Hz), an unmodulated 57 kHz component of carrier_hz on the
    same axis, FM at +-75 kHz, amplitude 0.5, white noise of `sigma` per component from the fixed seed."""
    n = int(round(seconds * fs))
    t = np.arange(n) / fs
    p = 2.0 * np.pi * 19000.0 * t
    s, rms = rds_waveform(n, fs, seed) if rds_hz else (np.zeros(n), 0.0)
    axis = np.cos(3.0 * p) if on == "cos" else np.sin(3.0 * p)
    mpx = 0.1 * np.sin(p) + (rds_hz / 75000.0 * s + carrier_hz / 75000.0) * axis
    if programme:
        L, R = 0.5 * np.sin(2.0 * np.pi * 1000.0 * t), 0.5 * np.sin(2.0 * np.pi * 400.0 * t)
        mpx += 0.45 * (L + R) + 0.45 * (L - R) * np.sin(2.0 * p)
    ph = 2.0 * np.pi * 75000.0 / fs * np.cumsum(mpx)
    iq = np.stack([0.5 * np.cos(ph), 0.5 * np.sin(ph)], axis=1)
    if sigma:
        iq += sigma * np.random.default_rng(NOISE_SEED).standard_normal((n, 2))
    return iq.astype(F32), rms

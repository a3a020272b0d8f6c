"""The float64 model of the sub-carrier decoder (include/fmx.h fmx_sca_*), an independent numpy-f32 restatement of the form the header
chose, and the measure that compares blocks.

The model is the contract's arithmetic as written, in float64, with the phase reduced in integers:
    y [m] = sum_k g [k] d [4 m - k] exp (-2 pi i ((centre (4 m - k)) mod R) / R)
    u [m] = arg (y [m] conj (y [m - 1])) R / (8 pi deviation),  arg (0) = 0
    s [n] = sum_k a [k] u [2 n - k]
    level [b] = mean |y [m]|^2, m in [480 b, 480 b + 480)
The restatement (blocks32) restates fmx_sca.h's FORM -- the mix folded into complex taps c [k] = f32 (g [k] exp (+2 pi i ((centre k) mod R) / R)), formed
in float64; y' [m] = sum_k c [k] d [4 m - k]; u from y' [m] conj (y' [m - 1]) rot, rot = f32 (exp (-2 pi i ((4 centre) mod R) / R)) -- in numpy float32,
one rounding per product and per sum, k ascending (no fused multiply-add: the header's fmaf differs from it in the last bits, as any two f32 forms do).
Measure: per audio sample |s - s64|; per block |level - level64| / level64.  Bound (DESIGN 4.9's rule): every sample within 2 x the restatement's worst,
the median within 2 x its median; the same for the levels.  Condition, asserted by every user: min |y| >= 0.1 median |y| over the compared span -- where
|y| falls to nothing arg () amplifies any rounding without bound and no comparison of u means anything."""
import numpy as np

NG, NA = 192, 128
BLOCK_FM, BLOCK_Y, BLOCK_AUDIO, LOOKBACK, RING = 1920, 480, 240, 703, 128
R = 192000


# ---- the designs, restated in numpy (the C export's taps are checked against these) -----------------------------------------------------------------
def kaiser_lowpass(n, f6, rate):
    x = np.arange(n) - (n - 1) / 2.0
    return 2.0 * f6 / rate * np.sinc(2.0 * f6 / rate * x) * np.kaiser(n, 7.0)


def design_band(half_band_hz=9000, rate=R):
    h = kaiser_lowpass(NG, half_band_hz + 2000.0, rate)
    return h / h.sum()


def design_audio(audio_cut_hz=5000, deemphasis_us=150, rate=R):
    lp = kaiser_lowpass(81, audio_cut_hz + 1300.0, rate / 4.0)
    if deemphasis_us == 0:
        de = np.zeros(48); de[0] = 1.0
    else:
        alpha = np.exp(-4.0 / (rate * deemphasis_us * 1e-6))
        de = (1 - alpha) * alpha ** np.arange(48)
    h = np.convolve(lp, de)
    return h / h.sum()


def response(h, f_hz, rate):
    k = np.arange(len(h))
    return np.abs(np.sum(np.asarray(h, np.float64) * np.exp(-2j * np.pi * f_hz * k / rate)))


# ---- the float64 model ---------------------------------------------------------------------------------------------------------------------------
def first_block(on_from):
    return -((-(on_from + LOOKBACK)) // BLOCK_FM)


def model64(d, g, a, centre, rate=R, deviation=6000.0, j0=0):
    """d [i] is fm sample j0 + i (j0 a multiple of 1920) -> {b: (audio [240], level, |y| of the block's 608)} for every block whose span lies in d"""
    d = np.asarray(d, np.float64)
    g, a = np.asarray(g, np.float64), np.asarray(a, np.float64)
    n = len(d)
    j = j0 + np.arange(n, dtype=np.int64)
    x = d * np.exp(-2j * np.pi * ((centre * j) % rate).astype(np.float64) / rate)
    full = np.convolve(x, g)                                  # full [i] = sum_k g [k] x [i - k]
    m_lo, m_hi = -((-(j0 + NG - 1)) // 4), (j0 + n - 1) // 4   # y [m] for m_lo <= m <= m_hi
    y = full[4 * np.arange(m_lo, m_hi + 1) - j0]
    z = y[1:] * np.conj(y[:-1])                               # u [m], m from m_lo + 1
    u = np.where(z == 0, 0.0, np.angle(z)) * rate / (8 * np.pi * deviation)
    fu = np.convolve(u, a)                                    # fu [i] = sum_k a [k] u [m_lo + 1 + i - k]
    out = {}
    b = first_block(j0)
    while BLOCK_FM * (b + 1) <= j0 + n:
        s = fu[2 * (BLOCK_AUDIO * b + np.arange(BLOCK_AUDIO)) - (m_lo + 1)]
        yb = y[BLOCK_Y * b - NA - m_lo: BLOCK_Y * (b + 1) - m_lo]
        out[b] = (s, float(np.mean(np.abs(yb[NA:]) ** 2)), np.abs(yb))
        b += 1
    return out


def conditioning(blocks):
    """min |y| / median |y| over every block's 608 samples"""
    ya = np.concatenate([v[2] for v in blocks.values()])
    return float(ya.min() / np.median(ya))


# ---- the numpy-f32 restatement of the header's form --------------------------------------------------------------------------------------------------
def mixed_taps(g, centre, rate=R):
    k = np.arange(NG, dtype=np.int64)
    ph = 2 * np.pi * ((centre * k) % rate).astype(np.float64) / rate
    c = np.asarray(g, np.float32).astype(np.float64) * np.exp(1j * ph)
    rot = np.exp(-2j * np.pi * ((4 * centre) % rate) / rate)
    return c.real.astype(np.float32), c.imag.astype(np.float32), np.float32(rot.real), np.float32(rot.imag)


def block32(span, g, a, centre, rate=R, deviation=6000.0, lag=1):
    """one block from its 2623 samples of d -> (audio [240] f32, level f32).  lag = 2 is the seeded defect `u from y [m] and y [m - 2]`."""
    f = np.float32
    span = np.asarray(span, f)
    assert span.shape == (LOOKBACK + BLOCK_FM,)
    cr, ci, rr, ri = mixed_taps(g, centre, rate)
    a = np.asarray(a, f)
    i = np.arange(NA + BLOCK_Y)
    re, im = np.zeros(len(i), f), np.zeros(len(i), f)
    for k in range(NG):
        v = span[4 * i + (NG - 1) - k]
        re = re + cr[k] * v
        im = im + ci[k] * v
    y1r, y1i, y0r, y0i = re[lag:], im[lag:], re[:-lag], im[:-lag]
    zr, zi = y1r * y0r + y1i * y0i, y1i * y0r - y1r * y0i
    wr, wi = zr * rr - zi * ri, zr * ri + zi * rr
    u = np.where((wr == 0) & (wi == 0), f(0), np.arctan2(wi, wr).astype(f)) * f(rate / (8 * np.pi * deviation))
    u = np.concatenate([np.zeros(lag - 1, f), u])            # (lag 2: u [m] still stands at m)
    n = np.arange(BLOCK_AUDIO)
    s = np.zeros(BLOCK_AUDIO, f)
    for k in range(NA):
        s = s + a[k] * u[2 * n + (NA - 1) - k]
    p = re[NA:] * re[NA:] + im[NA:] * im[NA:]
    return s, f(p.sum(dtype=f) / f(BLOCK_Y))


def blocks32(d, g, a, centre, rate=R, deviation=6000.0, j0=0, lag=1):
    d = np.asarray(d, np.float32)
    out = {}
    b = first_block(j0)
    while BLOCK_FM * (b + 1) <= j0 + len(d):
        lo = BLOCK_FM * b - LOOKBACK - j0
        out[b] = block32(d[lo:lo + LOOKBACK + BLOCK_FM], g, a, centre, rate, deviation, lag)
        b += 1
    return out


def blocks32_f32_phase(d, g, a, centre, rate=R, deviation=6000.0, j0=0):
    """the seeded defect `the mix phase in f32`: the contract's direct form with the phase f32 (2 pi centre / R) x f32 (j) instead of the integer reduction;
    beyond 2^24 fm samples j is no f32 any more"""
    f = np.float32
    d = np.asarray(d, f)
    j = (j0 + np.arange(len(d))).astype(f)
    ph = (f(2 * np.pi * centre / rate) * j).astype(f)
    xr, xi = (d * np.cos(ph).astype(f)).astype(np.float64), (-d * np.sin(ph).astype(f)).astype(np.float64)
    # (the rest of the chain in float64: the defect alone shows)
    out = {}
    for b in range(first_block(j0), (j0 + len(d)) // BLOCK_FM):
        lo = BLOCK_FM * b - LOOKBACK - j0
        x = (xr + 1j * xi)[lo:lo + LOOKBACK + BLOCK_FM]
        i = np.arange(NA + BLOCK_Y)
        y = np.array([np.dot(np.asarray(g, np.float64), x[4 * ii + (NG - 1) - np.arange(NG)]) for ii in i])
        z = y[1:] * np.conj(y[:-1])
        u = np.where(z == 0, 0.0, np.angle(z)) * rate / (8 * np.pi * deviation)
        n = np.arange(BLOCK_AUDIO)
        s = np.array([np.dot(np.asarray(a, np.float64), u[2 * nn + (NA - 1) - np.arange(NA)]) for nn in n])
        out[b] = (s.astype(f), f(np.mean(np.abs(y[NA:]) ** 2)))
    return out


# ---- the measure and the bound -------------------------------------------------------------------------------------------------------------------
def errors(got, want, blocks=None):
    """{b: (audio, level)} against the model's {b: (audio, level, ...)} over `blocks` (default: the model's) -> (|s - s64| flat, relative level errors)"""
    blocks = sorted(want) if blocks is None else blocks
    es = np.concatenate([np.abs(np.asarray(got[b][0], np.float64) - want[b][0]) for b in blocks])
    el = np.array([abs(float(got[b][1]) - want[b][1]) / want[b][1] if want[b][1] > 0 else abs(float(got[b][1])) for b in blocks])
    es[~np.isfinite(es)] = np.inf
    el[~np.isfinite(el)] = np.inf
    return es, el


def levels(want, *restatements, blocks=None):
    """(worst, median) of s and (worst, median) of level: the larger over the restatements"""
    e = [errors(r, want, blocks) for r in restatements]
    return (max(float(x[0].max()) for x in e), max(float(np.median(x[0])) for x in e),
            max(float(x[1].max()) for x in e), max(float(np.median(x[1])) for x in e))


def check(tag, got, want, lv, blocks=None, quiet=False):
    """every sample within 2 x the level's worst and the median within 2 x its median, for s and for level -> (passed, the four ratios)"""
    es, el = errors(got, want, blocks)
    r = (float(es.max()) / lv[0], float(np.median(es)) / lv[1], float(el.max()) / lv[2], float(np.median(el)) / lv[3])
    if not quiet:
        print("[%s] s: worst %.3e (level %.3e, ratio %.2f), median %.3e (level %.3e, ratio %.2f); level: worst %.3e (level %.3e, ratio %.2f), "
              "median %.3e (level %.3e, ratio %.2f); bound 2" % (tag, es.max(), lv[0], r[0], np.median(es), lv[1], r[1], el.max(), lv[2], r[2], np.median(el), lv[3], r[3]))
    return all(x <= 2.0 for x in r), r

"""The monitoring feed's models (include/fmx.h fmx_feed_*; sdr-j-fm_amd/csrc/fmx_feed.h): 16 kS/s mono from the delivered PCM.

design64 ()       the taps' formula in numpy float64 (numpy's own Kaiser window and sinc).
blocks32 ()       THE RESTATEMENT: the contract's f32 arithmetic in numpy, bit for bit what the header's host form and the kernel give -- v with one
                  rounding, y as the one fmaf chain (fma32: an exactly rounded f32 fused multiply-add made of float64 operations), the power's tree.
model64 ()        the float64 model on the same f32 taps and PCM, and per block the bounds an f32 form must keep:
    |y32 - y64| <= 146 u sum_k |h [k]| |v [3 n - k]|,  u = 2^-24
                  -- a 144-term fma chain has the standard bound gamma_144 sum |h| |v| <= 144 u (1 + 144 u) sum |h| |v|; the one rounding of v (mode 1:
                  |v32 - v| <= u |v|) adds u sum |h| |v|; 146 u covers both and their second-order terms (145 u + 144^2 u^2 + ... < 146 u).
    |P32 - P64| <= (1 / 160) (sum_n (2 |y64| B_n + B_n^2) + 12 u sum_n (|y64| + B_n)^2)
                  -- with B_n the bound above: the squares of the computed y differ from the model's by at most 2 |y| B + B^2; each square is rounded once
                  (u), the fixed tree adds at most 8 times in a row to any term (the fold of 160 to 128 and seven halvings: 8 u), the factor 1 / 160 is
                  rounded to f32 (u) and the product with it once more (u): 11 u, 12 u with their second-order terms, on sum (|y| + B)^2 >= the computed
                  sum of squares.  Derived, not measured.  (Underflow is left out: the signals here stay far above 2^-126.)
check ()          the checker: every block present, every sample and every power within those bounds; returns the worst ratios.
"""
import numpy as np

NTAPS, DECIM, BLOCK, BLOCK_FRAMES, LOOKBACK, RING = 144, 3, 160, 480, 143, 128
RATE, FRAME_RATE = 16000, 48000
BETA, F6_HZ = 8.0, 8000.0
DELAY_FRAMES = 71.5
U = 2.0 ** -24
F32 = np.float32


def design64():
    """a Kaiser (beta = 8) windowed sinc with its 6 dB point at 8000 Hz at 48 000 frames/s, normalised to sum 1"""
    x = np.arange(NTAPS) - (NTAPS - 1) / 2.0
    fc = 2.0 * F6_HZ / FRAME_RATE
    h = fc * np.sinc(fc * x) * np.kaiser(NTAPS, BETA)
    return h / h.sum()


def response(h, f_hz, rate=FRAME_RATE):
    """|H (f)| of the taps h at rate"""
    k = np.arange(len(h))
    return abs(np.sum(np.asarray(h, np.float64) * np.exp(-2j * np.pi * f_hz * k / rate)))


def first_block(on_from):
    """the first block with 480 b - 143 >= on_from"""
    return -((-(on_from + LOOKBACK)) // BLOCK_FRAMES)


def fma32(a, b, c):
    """f32 (a b + c) rounded ONCE, for f32 arrays: the product of two f32 is exact in float64; the sum's float64 rounding is replaced by rounding to odd
    (two-sum gives the sum's exact error), after which the rounding to f32 is that of the exact value (53 >= 24 + 2 bits)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def v32(pcm, mode, defect=None):
    """v of the contract from pcm [frames, 2] f32"""
    pcm = np.asarray(pcm, F32)
    if defect == "wrong ear" and mode in (2, 3):
        mode = 5 - mode
    if mode == 1:
        s = pcm[:, 0] + pcm[:, 1]
        return s if defect == "no half" else F32(0.5) * s
    return pcm[:, 0].copy() if mode == 2 else pcm[:, 1].copy()


def power32(y):
    """the power's fixed tree over [blocks, 160] f32 (fmx_feed.h's head)"""
    p = y * y
    q = p[:, :128].copy()
    q[:, :32] = q[:, :32] + p[:, 128:160]
    s = 64
    while s > 0:
        q[:, :s] = q[:, :s] + q[:, s:2 * s]
        s //= 2
    return q[:, 0] * (F32(1.0) / F32(BLOCK))


def blocks32(pcm, h, mode=1, m0=0, on_from=None, defect=None):
    """The restatement.  pcm [frames, 2] f32 holds the frames m0 .. m0 + frames - 1 (m0 a multiple of 480); the channel was switched on by a piece that
    began at frame on_from (default m0).  -> {b: (audio [160] f32, power f32)} of every block that is delivered and complete.
    defect (for the checker's test): "taps reversed" (the filter runs forwards in time: v [3 n + k] -- h is symmetric, so reversing the taps themselves
    changes nothing), "phase" (v [3 n + 1 - k]), "block shift" (block b holds the samples [160 b + 1, 160 b + 161)), "wrong ear", "no half",
    "power window" (the power over [160 b + 1, 160 b + 161))."""
    assert m0 % BLOCK_FRAMES == 0
    h = np.asarray(h, F32)
    v = v32(pcm, mode, defect)
    on_from = m0 if on_from is None else on_from
    b0, b1 = max(first_block(on_from), first_block(m0)), (m0 + len(v)) // BLOCK_FRAMES
    shift = 1 if defect in ("block shift", "power window") else 0
    if shift or defect == "taps reversed":
        b1 -= 1                                                    # (these read behind the block's last frame)
    if b1 <= b0:
        return {}
    n = np.arange(BLOCK * b0, BLOCK * b1 + shift)                  # feed samples
    at = DECIM * n - m0 + (1 if defect == "phase" else 0)          # index of v [3 n] in the array
    y = np.zeros(len(n), F32)
    for k in range(NTAPS):
        y = fma32(np.full(len(n), h[k], F32), v[at + k] if defect == "taps reversed" else v[at - k], y)
    nb = b1 - b0
    ya = y[shift if defect == "block shift" else 0:][:BLOCK * nb].reshape(nb, BLOCK)
    yp = y[shift:][:BLOCK * nb].reshape(nb, BLOCK) if defect == "power window" else ya
    pw = power32(np.ascontiguousarray(yp))
    return {b0 + i: (ya[i].copy(), pw[i]) for i in range(nb)}


def model64(pcm, h, mode=1, m0=0, on_from=None):
    """float64 on the same f32 taps and PCM -> {b: (y64 [160], B [160], P64, BP)}: the model's samples, their bound, its power, its bound"""
    assert m0 % BLOCK_FRAMES == 0
    h = np.asarray(h, F32).astype(np.float64)
    x = np.asarray(pcm, F32).astype(np.float64)
    v = 0.5 * (x[:, 0] + x[:, 1]) if mode == 1 else (x[:, 0] if mode == 2 else x[:, 1])
    on_from = m0 if on_from is None else on_from
    b0, b1 = max(first_block(on_from), first_block(m0)), (m0 + len(v)) // BLOCK_FRAMES
    if b1 <= b0:
        return {}
    at = DECIM * np.arange(BLOCK * b0, BLOCK * b1) - m0
    idx = at[:, None] - np.arange(NTAPS)[None, :]
    y = (v[idx] * h[None, :]).sum(axis=1)
    B = 146 * U * (np.abs(v[idx]) * np.abs(h)[None, :]).sum(axis=1)
    y, B = y.reshape(-1, BLOCK), B.reshape(-1, BLOCK)
    P = (y * y).mean(axis=1)
    BP = ((2 * np.abs(y) * B + B * B).sum(axis=1) + 12 * U * ((np.abs(y) + B) ** 2).sum(axis=1)) / BLOCK
    return {b0 + i: (y[i], B[i], P[i], BP[i]) for i in range(b1 - b0)}


def same_blocks(x, y, blocks=None):
    """bit for bit"""
    if blocks is None:
        if sorted(x) != sorted(y):
            return False
        blocks = sorted(x)
    return all(b in x and b in y and np.asarray(x[b][0], F32).tobytes() == np.asarray(y[b][0], F32).tobytes() and
               F32(x[b][1]).tobytes() == F32(y[b][1]).tobytes() for b in blocks)


def check(label, got, M, blocks=None, quiet=False):
    """got {b: (audio, power)} against model64's M on `blocks` (default: the model's) -> (ok, (worst |y - y64| / B, worst |P - P64| / BP)).  A block that
    is missing, or has another shape, fails with infinite ratios."""
    blocks = sorted(M) if blocks is None else blocks
    ry = rp = 0.0
    for b in blocks:
        if b not in got or b not in M or np.shape(got[b][0]) != (BLOCK,):
            ry = rp = np.inf
            continue
        y64, B, P, BP = M[b]
        ey = np.abs(np.asarray(got[b][0], np.float64) - y64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(ey == 0, 0.0, ey / B)
        ry = max(ry, float(np.nanmax(r)))
        ep = abs(float(got[b][1]) - P)
        rp = max(rp, 0.0 if ep == 0 else (ep / BP if BP > 0 else np.inf))
    ok = bool(blocks) and ry <= 1.0 and rp <= 1.0
    if not quiet:
        print("%s: %d blocks; worst |y - y64| / bound = %.3f, worst |P - P64| / bound = %.3f" % (label, len(blocks), ry, rp))
    return ok, (ry, rp)


# ---- signals: PCM as a handle might deliver it, [frames, 2] f32 -----------------------------------------------------------------------------------------
def programme(frames, seed=1):
    """a stereo programme: band-limited noise (a different one per ear over a common one) and two tones"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / FRAME_RATE

    def band(n):
        w = rng.standard_normal(n + 63)
        return np.convolve(w, np.hanning(64) / np.hanning(64).sum(), mode="valid")
    common, left, right = band(frames), band(frames), band(frames)
    L = 0.5 * common + 0.25 * left + 0.2 * np.sin(2 * np.pi * 440.0 * t)
    R = 0.5 * common + 0.25 * right + 0.15 * np.sin(2 * np.pi * 3300.0 * t + 0.3)
    return np.stack([L, R], axis=1).astype(F32)


def tone(frames, hz=1000.0, amp=0.5, phase=0.0):
    t = np.arange(frames) / FRAME_RATE
    s = amp * np.sin(2 * np.pi * hz * t + phase)
    return np.stack([s, s], axis=1).astype(F32)


def noise(frames, seed=2, sigma=0.3):
    rng = np.random.default_rng(seed)
    return (sigma * rng.standard_normal((frames, 2))).astype(F32)


def tone_fit(s, hz, rate):
    """least squares a sin + b cos at hz -> (amplitude, rms of the residual)"""
    t = np.arange(len(s)) / rate
    A = np.stack([np.sin(2 * np.pi * hz * t), np.cos(2 * np.pi * hz * t)], axis=1)
    c, *_ = np.linalg.lstsq(A, s, rcond=None)
    return float(np.hypot(*c)), float(np.sqrt(np.mean((s - A @ c) ** 2)))


def to_s16(y):
    """FMX_FEED_S16 in numpy: (int16) min (32767, max (-32768, rint (y * 32768))), half to even"""
    r = np.rint(np.asarray(y, F32) * F32(32768.0))
    return np.clip(r, -32768, 32767).astype(np.int16)

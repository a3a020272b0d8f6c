"""Float64 model of stage W's band survey (include/fmx.h fmx_wideband_survey_*), its plain f32 restatement, the station finder
in float64 and the test signals.

    block b = samples [N b, N (b + 1)), N = 4096;  w[i] = 0.5 - 0.5 cos(2 pi i / N) in f64, rounded to f32
    p_b[k] = |sum_i w[i] x[N b + i] exp(-2 pi i ik / N)|^2;  record r: P_r[k] = c sum_{b = rB .. rB + B - 1} p_b[k],  c = f32(1 / (B sum w^2))

`records64` holds the window (rounded to f32) and c (rounded to f32) as the contract states them and everything else in f64.  `records32` is
the plain restatement: window multiply in f32, an iterative radix-2 complex64 transform with twiddles rounded from f64, Re^2 + Im^2 and the
sequential sum over the blocks in f32, one multiply by c.  `check_spectrum` is the bound of every comparison (the detector)."""
import numpy as np

import wideband_model as wm

N = 4096
RING = 4
NARROW_RATE = wm.NARROW_RATE


def window():
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N, dtype=np.float64) / N)).astype(np.float32)


def record_scale(B):
    w = window().astype(np.float64)
    return np.float32(1.0 / (B * np.sum(w * w)))


def block_powers64(x):
    x = np.asarray(x, np.complex128)
    nb = len(x) // N
    X = np.fft.fft(x[:nb * N].reshape(nb, N) * window().astype(np.float64), axis=1)
    return X.real ** 2 + X.imag ** 2


def records64(x, B):
    """x: complex (exact f32 values), one stream from the survey's first sample on -> float64 [complete records, N]."""
    p = block_powers64(x)
    nr = p.shape[0] // B
    return p[:nr * B].reshape(nr, B, N).sum(axis=1) * float(record_scale(B))


def _fft32(v):
    """Radix-2 decimation in time on complex64 rows [.., N]: every product and sum rounded to f32, twiddles rounded from f64 once."""
    v = np.asarray(v, np.complex64)
    bits = N.bit_length() - 1
    idx = np.arange(N)
    rev = np.zeros(N, np.int64)
    for b in range(bits):
        rev |= ((idx >> b) & 1) << (bits - 1 - b)
    a = v.reshape(-1, N)[:, rev]
    half = 1
    while half < N:
        tw = np.exp(-2j * np.pi * np.arange(half, dtype=np.float64) / (2 * half)).astype(np.complex64)
        g = a.reshape(-1, N // (2 * half), 2, half)
        ev, od = g[:, :, 0, :], g[:, :, 1, :] * tw
        a = np.concatenate([ev + od, ev - od], axis=-1).reshape(-1, N)
        half *= 2
    return a.reshape(v.shape)


def block_powers32(x):
    x = np.asarray(x, np.complex128)
    nb = len(x) // N
    w = window()
    xr = x.real[:nb * N].astype(np.float32).reshape(nb, N) * w
    xi = x.imag[:nb * N].astype(np.float32).reshape(nb, N) * w
    X = _fft32((xr + 1j * xi).astype(np.complex64))
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    return re * re + im * im


def records_from_powers32(p, B, scale=None):
    """The sequential f32 sum of the blocks' powers in block order and the one multiply -> float32 [records, N]."""
    p = np.asarray(p, np.float32)
    c = record_scale(B) if scale is None else np.float32(scale)
    nr = p.shape[0] // B
    out = np.zeros((nr, N), np.float32)
    for r in range(nr):
        s = np.zeros(N, np.float32)
        for b in range(r * B, (r + 1) * B):
            s = s + p[b]
        out[r] = s * c
    return out


def records32(x, B):
    return records_from_powers32(block_powers32(x), B)


def bin_errors(P, P64):
    P, P64 = np.asarray(P, np.float64), np.asarray(P64, np.float64)
    assert P.shape == P64.shape, (P.shape, P64.shape)
    ok = P64 > 0
    e = np.abs(P[ok] - P64[ok]) / P64[ok]
    e[~np.isfinite(e)] = np.inf
    return e


def levels(P64, *restatements):
    """(level_worst, level_median): the larger of the restatements' worst bins / of their medians."""
    errs = [bin_errors(r, P64) for r in restatements]
    return max(float(e.max()) for e in errs), max(float(np.median(e)) for e in errs)


def check_spectrum(tag, got, P64, level_worst, level_median, quiet=False):
    """The spectrum bound: every bin within 2 x level_worst, the median within 2 x level_median.  -> (passed, worst ratio, median ratio)."""
    e = bin_errors(got, P64)
    rw, rm = float(e.max()) / level_worst, float(np.median(e)) / level_median
    if not quiet:
        print("[%s] worst bin %.3e (level %.3e, ratio %.2f, bound 2), median %.3e (level %.3e, ratio %.2f, bound 2)"
              % (tag, float(e.max()), level_worst, rw, float(np.median(e)), level_median, rm))
    return rw <= 2.0 and rm <= 2.0, rw, rm


# ---- the station finder in float64 ------------------------------------------------------------------------------------------------------
def find_stations(P, factor, raster_hz=100000, origin_hz=0, threshold_db=10.0, dc_guard_hz=0):
    """-> ([(offset_hz, level_db, snr_db)], floor_db).  Membership of a bin in a window in Python integers, every sum in float64; the threshold
    is compared as the f32 value the C struct holds."""
    P = np.asarray(P, np.float32).astype(np.float64)
    Rw = factor * NARROW_RATE
    kp = [k if k < N // 2 else k - N for k in range(N)]
    usable = [abs(kp[k] * Rw) >= dc_guard_hz * N for k in range(N)]
    fl = sorted(P[k] for k in range(N) if usable[k] and abs(kp[k] * Rw) <= (Rw // 2 - 50000) * N)
    F = fl[len(fl) // 10] if fl else 0.0
    floor_db = 10 * np.log10(F) if F > 0 else -np.inf
    if not F > 0:
        return [], floor_db
    lim = Rw // 2 - 150000
    js = [j for j in range(-(Rw // raster_hz) - 2, Rw // raster_hz + 3) if abs(origin_hz + j * raster_hz) <= lim]
    kpRw = np.array([kp[k] * Rw for k in range(N)], dtype=object)
    level = []
    for j in js:
        fj = origin_hz + j * raster_hz
        sel = [k for k in range(N) if usable[k] and abs(kpRw[k] - fj * N) <= 100000 * N]
        level.append(float(np.sum(P[sel])) / len(sel) if sel else 0.0)
    thr = float(np.float32(threshold_db))
    out = []
    for i, j in enumerate(js):
        c = level[i]
        if not c > 0:
            continue
        snr = 10 * np.log10(c / F)
        if not snr > thr:
            continue
        wins = True
        for q in range(len(js)):
            if q != i and abs(js[q] - j) * raster_hz < 200000:
                wins = wins and (c >= level[q] if q < i else c > level[q])
        if wins:
            out.append((origin_hz + j * raster_hz, 10 * np.log10(c), snr))
    return out, floor_db


# ---- signals -------------------------------------------------------------------------------------------------------------------------------
def fm_stations(K, n, stations, noise_power=1e-4, seed=0, dc=0.0, deviation=75000.0):
    """One stream of n samples at K * 2 304 000 S/s: mono FM stations [(offset_hz, amplitude, tone_hz)] at `deviation`, complex white noise of
    the given power, a DC spike -> complex128."""
    rng = np.random.default_rng(seed)
    Rw = K * NARROW_RATE
    t = np.arange(n, dtype=np.float64)
    x = np.sqrt(noise_power / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + dc
    for m, (f, amp, tone) in enumerate(stations):
        x = x + amp * np.exp(1j * (2 * np.pi * ((f * np.arange(n, dtype=np.int64)) % Rw) / Rw + (deviation / tone) * np.sin(2 * np.pi * tone * t / Rw + m)))
    return x


def spectrum_signal(K, n, seed=0):
    """The signal of the spectrum comparisons, in which a dropped, swapped or shifted block shows: FM carriers and noise, an amplitude envelope
    that differs per block of 4096, a linear chirp that crosses the whole band once per block, and a pedestal -> complex128, |re|, |im| < 1.
    The bound is on every bin's RELATIVE error, so every bin needs power that is not an accident.  A bin that holds noise alone is, in a single
    periodogram (B = 1), exponentially distributed: the weakest of 40 960 such bins lies 46 dB below their mean, and its relative error is the
    transform's absolute error over an arbitrarily small number -- a lottery in which two correct f32 transforms differ by any factor.  Two
    deterministic components of like strength in one bin cancel somewhere just as deeply, and the window takes a chirp's power away where
    the chirp passes at a block's edge.  Hence the pedestal: one sample of 0.8 (1 + i) at the centre of every block, where the window is 1 --
    the same power in every bin of the block, 10 dB above the chirp and 23 dB above the noise, 40 dB below the carriers' bins.  The strongest
    and the weakest bin of a record are then about 60 dB apart, and what is compared is the arithmetic."""
    lim = wm.offset_limit(K)
    x = fm_stations(K, n, [(-lim + 37000, 0.15, 2500.0), (lim // 3, 0.1, 4000.0)], noise_power=4e-6, seed=100 * K + seed)
    i = (np.arange(n) % N).astype(np.float64)
    x = x + 0.009 * np.exp(2j * np.pi * (-0.5 * i + 0.5 * i * i / N))          # -0.5 .. +0.5 cycles per sample within a block
    x[np.arange(n) % N == N // 2] = 0.8 * (1 + 1j)
    env = 0.4 + 0.6 * ((np.arange(n) // N * 7 + 3) % 5) / 4.0
    return x * env


def to_raw(x, fmt):
    """complex -> [n, 2] in the raw format (f32 / u8 / s8 / s16 with denominator 2048)."""
    v = np.stack([np.real(x), np.imag(x)], axis=-1)
    if fmt == 0:
        return v.astype(np.float32)
    if fmt == 1:
        return np.clip(np.rint(v * 128.0 + 127.0), 0, 255).astype(np.uint8)
    if fmt == 2:
        return np.clip(np.rint(v * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint(v * 2048.0), -32768, 32767).astype(np.int16)


def brute_plan(fill, n_wide, blocks_so_far, B):
    """survey::plan by counting: walk the call sample by sample."""
    blocks, records, b = 0, 0, blocks_so_far
    for _ in range(n_wide):
        fill += 1
        if fill == N:
            fill, blocks, b = 0, blocks + 1, b + 1
            if b % B == 0:
                records += 1
    return blocks, fill, blocks_so_far % B, blocks_so_far // B, records


def stream_length(K):
    """10 blocks and 100 samples, rounded down to a multiple of K."""
    return (10 * N + 100) // K * K


def call_cuts(K):
    """The calls a stream of stream_length(K) samples is cut into, every length a multiple of K: three calls that complete no block (the carry
    grows), one that completes a block from the carry and leaves a tail, one of several blocks, one that ends exactly on a block boundary, one
    of K samples, and the rest."""
    rk = lambda v: max(K, v // K * K)
    cuts = [rk(1000), rk(1500), rk(1000), rk(1200), rk(3 * N + 500)]
    fill = sum(cuts) % N
    assert sum(cuts[:3]) < N < sum(cuts[:4]) and fill > 0
    m = next(m for m in range(1, K + 1) if (m * N - fill) % K == 0)          # (gcd(K, N) divides fill: a solution exists)
    cuts += [m * N - fill, K]
    rest = stream_length(K) - sum(cuts)
    assert rest > 0 and sum(cuts[:6]) % N == 0
    return cuts + [rest]

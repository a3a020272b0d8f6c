"""Float64 model of the spectrum meter (include/fmx.h fmx_spectrum_*), its plain f32 restatement, a brute-force count of the grid and
the signals of the figure tests.

    block b = samples [N S b, N S b + N), N = 4096;  w, the transform and c = f32(1 / (B sum w^2)) are the band survey's (survey_model)
    p_b[k] = |sum_i w[i] x[N S b + i] exp(-2 pi i ik / N)|^2
    record r: mean_r[k] = c sum_{b = rB .. rB + B - 1} p_b[k] in block order,  peak_r[k] = c1 max_b p_b[k],  c1 = f32(1 / sum w^2)

`records64` holds the window and the two scales as the contract states them (rounded to f32) and everything else in f64.  `records32` is the plain
restatement: survey_model's window multiply and radix-2 complex64 transform, the sequential f32 sum and the running f32 maximum, one multiply each.
The bound of every comparison is survey_model.check_spectrum."""
import numpy as np

import survey_model as sm

N = sm.N
RING = 4


def n_blocks(n, S):
    """blocks of the S-grid that lie whole inside [0, n)"""
    return 0 if n < N else (n - N) // (N * S) + 1


def gather(x, S):
    """-> [blocks, N]: the samples the grid reads"""
    x = np.asarray(x)
    nb = n_blocks(len(x), S)
    return np.stack([x[N * S * b:N * S * b + N] for b in range(nb)]) if nb else np.zeros((0, N), x.dtype)


def block_powers64(x, S=1):
    return sm.block_powers64(gather(np.asarray(x, np.complex128), S).reshape(-1))


def block_powers32(x, S=1):
    return sm.block_powers32(gather(np.asarray(x, np.complex128), S).reshape(-1))


def deliverable(nb, B, first=0):
    """the records r with every block in [first, nb)"""
    return [r for r in range(nb // B) if r * B >= first]


def records64(x, B, S=1, first=0):
    """x: complex (exact f32 values), one stream from g = 0 -> (indices, mean [records, N], peak [records, N]) in float64."""
    p = block_powers64(x, S)
    idx = deliverable(p.shape[0], B, first)
    c, c1 = float(sm.record_scale(B)), float(sm.record_scale(1))
    mean = np.stack([p[r * B:(r + 1) * B].sum(axis=0) * c for r in idx]) if idx else np.zeros((0, N))
    peak = np.stack([p[r * B:(r + 1) * B].max(axis=0) * c1 for r in idx]) if idx else np.zeros((0, N))
    return idx, mean, peak


def records_from_powers32(p, B, first=0):
    """The fold in f32: per record the sequential sum and the running maximum in block order, one multiply each -> (indices, mean, peak) f32."""
    p = np.asarray(p, np.float32)
    idx = deliverable(p.shape[0], B, first)
    c, c1 = sm.record_scale(B), sm.record_scale(1)
    mean, peak = np.zeros((len(idx), N), np.float32), np.zeros((len(idx), N), np.float32)
    for i, r in enumerate(idx):
        s, m = np.zeros(N, np.float32), np.zeros(N, np.float32)
        for b in range(r * B, (r + 1) * B):
            s = s + p[b]
            m = np.maximum(m, p[b])
        mean[i], peak[i] = s * c, m * c1
    return idx, mean, peak


def records32(x, B, S=1, first=0):
    return records_from_powers32(block_powers32(x, S), B, first)


def first_block(g, S):
    return -(-g // (N * S))


# ---- the grid by counting -----------------------------------------------------------------------------------------------------------------
class BruteGrid:
    """The S-grid walked sample by sample from a position `g` at which a record begins (a multiple of N S B).  call(n) -> what spec::piece reports for
    the next n samples: (blocks, fill, fill_after, append, carry_src, phase, record0, records); carry_src is None where nothing says what it is."""

    def __init__(self, g, S, B):
        assert g % (N * S * B) == 0
        self.g, self.S, self.B = g, S, B
        self.fill = 0                      # samples of the block in progress
        self.done = g // (N * S)           # blocks completed so far (= the index of the next block to complete)

    def call(self, n):
        P = N * self.S
        fill0, done0, g0 = self.fill, self.done, self.g
        blocks = records = 0
        src = None                         # the call's sample at which the block in progress began, if it began inside the call
        for i in range(n):
            o = self.g % P
            if o < N:
                if o == 0:
                    src = i
                self.fill += 1
                if self.fill == N:
                    self.fill, blocks, self.done = 0, blocks + 1, self.done + 1
                    src = None
                    if self.done % self.B == 0:
                        records += 1
            self.g += 1
        append = 1 if (self.fill > 0 and src is None) else 0
        return (blocks, fill0, self.fill, append, src if (self.fill > 0 and not append) else None, done0 % self.B, done0 // self.B, records), g0


# ---- signals of the figure tests ---------------------------------------------------------------------------------------------------------------
def fm_tone(n, rate, f0, amp, tone_hz, deviation, phase=0.0):
    """A carrier at f0 frequency-modulated by one tone: amp exp(i (2 pi f0 t + (deviation / tone) sin(2 pi tone t + phase)))."""
    t = np.arange(n, dtype=np.float64)
    return amp * np.exp(1j * (2 * np.pi * ((f0 * np.arange(n, dtype=np.int64)) % rate) / rate + (deviation / tone_hz) * np.sin(2 * np.pi * tone_hz * t / rate + phase)))


def fm_noise(n, rate, f0, amp, deviation_rms, audio_hz=15000.0, seed=0):
    """A carrier at f0 frequency-modulated by low-pass Gaussian noise (a noise-like programme) of the given rms deviation."""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / rate)
    X[f > audio_hz] = 0.0
    m = np.fft.irfft(X, n)
    m *= deviation_rms / np.sqrt(np.mean(m * m))
    ph = 2 * np.pi * np.cumsum(m) / rate
    return amp * np.exp(1j * (2 * np.pi * ((f0 * np.arange(n, dtype=np.int64)) % rate) / rate + ph))


def white(n, power, seed=0):
    rng = np.random.default_rng(seed)
    return np.sqrt(power / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def record_of(x, B, S=1):
    """(mean, peak) f32 of the first record of the stream x, as the model makes it"""
    x = np.asarray(x, np.complex64).astype(np.complex128)
    _, mean, peak = records64(x[:N * S * (B - 1) + N], B, S)
    return mean[0].astype(np.float32), peak[0].astype(np.float32)


def bessel_obw(beta, tone_hz, fraction):
    """The occupied bandwidth of a tone-modulated FM carrier from its lines J_n(beta)^2 at n tone_hz: the frequencies below / above which
    (1 - fraction) / 2 of the power lies, taken at the line that crosses -> (lower_hz, upper_hz)."""
    ns = np.arange(-400, 401)
    # J_n(beta) by the integral (1 / 2 pi) int exp(i (beta sin t - n t)) dt, on a grid fine enough for n <= 400
    t = 2 * np.pi * np.arange(8192) / 8192
    J = np.array([np.mean(np.exp(1j * (beta * np.sin(t) - n * t))).real for n in ns])
    p = J * J
    p /= p.sum()
    tail = 0.5 * (1 - fraction)
    lo = ns[np.searchsorted(np.cumsum(p), tail)]
    hi = ns[::-1][np.searchsorted(np.cumsum(p[::-1]), tail)]
    return lo * tone_hz, hi * tone_hz

"""Models of four feed-forward links of stage B (fmx_stageb.hip) -- the memoryless decoders' chain from the fm-rate IQ to the de-emphasised
pair -- for sample-by-sample comparisons on the stream the kernel itself read: numpy and the oracle library only.  A helper module (not a
conftest): tests/test_stage_b_model_cpu.py proves the restatements bit-identical to the oracle, re-measures the bounds' constants and shows
that the compare helpers flag planted errors; tests/test_gpu_stage_b_per_sample.py holds the kernels to the bounds.

  link D   FM_IQ -> DEMOD                       limiter, discriminator, AFC, scaling            (fm-demodulator.cpp:111-205)
  link P   5 DEMOD -> PILOT_PHASE, lock         the pilot loop and its lock detector             (pilot-recover.cpp:54-83)
  link S   (DEMOD, PILOT_PHASE, lock) -> LR_RAW the 38 kHz mix                                   (fm-processor.cpp:689-730)
  link E   LR_RAW -> PRE_RESAMPLER              stereo matrix and de-emphasis, folded handles    (fm-processor.cpp:517-549, 594-595)

ALIGNMENT.  Sample j of every one of the five taps belongs to fm sample j of the reference's numbering.  FMX_TAP_FM_IQ is read from the z
ring `delay_fm` entries back (fmx_readout.hip: ring index j - delay_fm, zero in front of the stream) and stage B's `fetch` reads the same
ring the same `delay_fm` back (zero while j - delay_fm < 0, the reference's start values 0.01 in front of sample 0), so DEMOD [j] is the
discriminator's answer to FM_IQ [j] with FM_IQ [j - 1] (and [j - 2], decoder 6) as its history; DEMOD, PILOT_PHASE and LR_RAW are rows of
one call's work arrays (row r of a call that starts at J0 is sample J0 + r), and the d ring behind FMX_TAP_PRE_RESAMPLER is written at
index J0 + r and read without a delay.  TAP_OFFSET states that, and every link's model is evaluated with it: nothing is searched for.

The reference of every link is the oracle (fmo_demod_run, fmo_pilot_run, fmo_pss_*) or a numpy restatement that the CPU test proves
bit-identical to the oracle's chain taps.  Every bound comes from the reference's own error or the number formats (see each constant).
"""
import ctypes as C

import numpy as np

import oracle_lib as ol

FM_RATE = 192000
SEG = 1536                     # fm samples per segment of stageb_kernel (FB_W)
PER_THREAD = 6                 # consecutive samples of a segment that one thread holds (FB_K = FB_W / 256 threads)
TWO_PI = 2.0 * np.pi
TAP_OFFSET = dict(fm_iq=0, demod=0, pilot_phase=0, lr_raw=0, pre_resampler=0)      # see ALIGNMENT above
AFC_ALPHA = np.float32(0.0001)                                                      # fmDcAlpha fm-demodulator.cpp:117
LOCK_THRESHOLD = np.float32(0.07)                                                   # pilot-recover.cpp:62
START_SKIP = 16                # the peak of a DEMOD stream is taken behind the first 16 samples (the start values 0.01 make sample 0 a jump)

# ------------------------------------------------------------------------------------------------ the bounds' constants
# Each is re-measured by tests/test_stage_b_model_cpu.py from the reference alone, on the CPU, and held against these records (within a
# quarter either way: the records of links D and E are the figures the bounds were set with; the re-measurements are in the comments); the
# GPU bounds are the records doubled and come from nothing else.
REF_D_AFC64 = 1.50e-7           # oracle DEMOD against afc_scale_f64 on the same discriminator output, default programme, Mixed decoder; of the peak (re-measured 1.499e-7)
REF_D_AFC64_MISTUNED = 3.56e-5  # the same on a carrier 20 kHz off tune, |afc| reaches 0.66 (re-measured 3.74e-5 over 150 186 samples)
REF_P_SINE_FREEDOM = 3.83e-6    # rad: the reference's own pilot loop with its sine table moved by up to 1.2e-7, worst wrapped difference of four
                                # variants (three random: 1.43e-6, 1.43e-6, 1.91e-6; every entry away from zero: 3.83e-6); a phase near 2 pi has an ulp of 4.8e-7
REF_E_DEEMPH = 2.06e-7          # the reference's f32 de-emphasis recurrence against float64 on the same f32 matrix output; of the peak (re-measured 2.10e-7)
D_BATCH_BOUND = 2.0 * REF_D_AFC64
D_MISTUNED_BOUND = 2.0 * REF_D_AFC64_MISTUNED
P_SEQ_BOUND = 2.0 * REF_P_SINE_FREEDOM
E_BOUND = 2.0 * REF_E_DEEMPH
D_SLIP_SHARE = 0.002            # batches: the share of samples whose table index the one-ulp limiter may move by one entry
D_SLIP_SHARE_REF = 0.001        # ... and the cap on what the reference alone shows with its input perturbed by 6e-8 relative
HW_SINE = 1.2e-7                # include/fmx.h FMX_P_PLL_SOLVER: the GPU's sine unit against the reference's table entry
S_SINE = 1.5e-7                 # what fmx_create checks the kernels' 38 kHz sines against (link S)
P_NEWTON_RMS, P_NEWTON_WORST = 1e-5, 1e-4        # include/fmx.h's contract of the Newton solver; test_newton_solver_batch_equals_single_and_reports_rounds' per-sample bound
PSS_SLIP_SHARE = 0.02           # PSS on: the share of samples that may be one table step off (the accumulator is not tapped)
LOCK_MARGIN = 1e-5              # the model's lock metric stays this far from 0.07 on both sides of every crossing (a 1.2e-7 sine moves it by 5e-7)
TABLE_STEP = TWO_PI / FM_RATE   # rad per entry of the SinCos table


# ------------------------------------------------------------------------------------------------ inputs the CPU and the GPU tests share
# A pilot of 0.12 instead of the generator's 0.10: with 0.10 the lock metric passes 0.07 at a distance of 3.0e-6 on its way up (sample 8226
# ...), nearer than LOCK_MARGIN; with 0.12 every crossing keeps 4.8e-5 and the channel locks at sample 103720 (test_stage_b_model_cpu.py).
PROGRAMMES = dict(
    default=dict(pilotLevel=0.12),
    tones=dict(pilotLevel=0.11, leftHz=1370.0, rightHz=630.0),  # (these tones with a pilot of 0.12: 4.3e-7; with 0.11: 4.2e-5, locked at 103944)
    mistuned=dict(pilotLevel=0.12, offsetHz=20000.0),           # |afc| reaches 0.66: a batch crosses AFC_EXACT_THR = 0.15 in mid-stream
    noise=dict(carrierAmp=0.0, noiseSeed=11, noiseSigma=0.1),   # never locks
    # one stream for decoders 3 - 6, each with a lock metric of its own: 4.5e-5 (Mixed, ComplexBB; locked at 103791), 2.2e-5 (RealBB; 106969), and the Diff
    # decoder's single crossing at the input filter's first output, sample 5444 (locked at 101444)
    decoders=dict(pilotLevel=0.12, leftHz=1370.0, rightHz=630.0, leftAmp=0.3, rightAmp=0.4),
)
RAGGED = [50000, 12, 13, 99999, 230400, 1, 100000]              # test_block_size_invariance's call lengths, in input samples
CALLS = RAGGED * 4                                              # 1 921 700 input samples, 160 141 fm samples: 0.83 s


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Tables:
    """The reference's tables and constants, from the oracle library: SinCos (cos, sin) [192000], its f64 index factor, the eight atan
    tables, K_FM, the pilot loop's omega and gain, the PSS alpha."""

    def __init__(self, L=None):
        self.L = L = L or ol.oracle()
        self.sc = L.fmo_sincos_new(FM_RATE)
        t = np.ctypeslib.as_array(L.fmo_sincos_table(self.sc), shape=(FM_RATE, 2)).copy()
        self.cos, self.sin = t[:, 0].copy(), t[:, 1].copy()
        self.Cc = FM_RATE / (2 * np.pi)                        # sincos.cpp: Rate / (2 * M_PI) in f64
        at = L.fmo_atan_new()
        self.atan = [np.ctypeslib.as_array(L.fmo_atan_table(at, k), shape=(8193,)).copy() for k in range(8)]
        L.fmo_atan_free(at)
        d = L.fmo_demod_new(FM_RATE)
        self.K_FM = np.float32(L.fmo_demod_kfm(d))
        L.fmo_demod_free(d)
        o, g, a = C.c_float(), C.c_float(), C.c_float()
        L.fmo_pilot_constants(FM_RATE, C.byref(o), C.byref(g), C.byref(a))
        self.omega, self.gain, self.pss_alpha = np.float32(o.value), np.float32(g.value), np.float32(a.value)

    def table_step(self, decoder):
        """The largest difference between adjacent entries of the decoder's own table, scaled by 20 / K_FM: what one slipped index is worth in
        DEMOD.  Decoders 3 and 4: compAtan's tables (the eight differ by sign and offset only); 5: the arcsine table; 6 has no table."""
        if decoder in (3, 4):
            step = float(np.abs(np.diff(self.atan[0].astype(np.float64))).max())
        elif decoder == 5:
            n = 4 * 8192
            step = float(np.abs(np.diff((np.arcsin(2.0 * np.arange(n + 1) / n - 1.0) / 2.0).astype(np.float32).astype(np.float64))).max())
        else:
            step = 0.0
        return step * 20.0 / float(self.K_FM)

    def close(self):
        if self.sc:
            self.L.fmo_sincos_free(self.sc)
            self.sc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_tables = None


def tables():
    global _tables
    if _tables is None:
        _tables = Tables()
    return _tables


# ------------------------------------------------------------------------------------------------ link D
def demod_oracle(z, decoder=3):
    """fmo_demod_run over the whole stream z [n, 2] f32 from a fresh demodulator: DEMOD [n] f32."""
    z = np.ascontiguousarray(z, np.float32).reshape(-1, 2)
    out = np.zeros(z.shape[0], np.float32)
    tables().L.fmo_demod_run(FM_RATE, int(decoder), fptr(z), z.shape[0], fptr(out), None, None)
    return out


def limiter(z):
    """fm-demodulator.cpp:119-126 in f32: (I, Q) = z / |z|, or 0.001 each where |z| <= 0.001."""
    z = np.ascontiguousarray(z, np.float32).reshape(-1, 2)
    a = np.hypot(z[:, 0], z[:, 1])                 # hypotf
    small = a.astype(np.float64) <= 0.001
    a1 = np.where(small, np.float32(1.0), a)
    i = np.where(small, np.float32(0.001), z[:, 0] / a1).astype(np.float32)
    q = np.where(small, np.float32(0.001), z[:, 1] / a1).astype(np.float32)
    return i, q


def discriminator_mixed(z):
    """The Mixed decoder's phase step in front of the AFC (:168-172): compAtan::atan2 (Q I1 - I Q1, I I1 + Q Q1), history 0.01."""
    i, q = limiter(z)
    i1 = np.concatenate([[np.float32(0.01)], i[:-1]]).astype(np.float32)
    q1 = np.concatenate([[np.float32(0.01)], q[:-1]]).astype(np.float32)
    y = (q * i1 - i * q1).astype(np.float32)
    x = (i * i1 + q * q1).astype(np.float32)
    res = np.zeros(y.shape[0], np.float32)
    tables().L.fmo_atan2_eval(fptr(np.ascontiguousarray(y)), fptr(np.ascontiguousarray(x)), y.shape[0], fptr(res))
    return res


def afc_scale_f32(res):
    """fm-demodulator.cpp:197-198 in the reference's f32, sample after sample: afc <- (1 - a) afc + a res; 20 (res - afc) * 1 / K_FM."""
    k, c1, a = tables().K_FM, np.float32(1) - AFC_ALPHA, AFC_ALPHA
    one = np.float32(1.0)
    out = np.empty(res.shape[0], np.float32)
    afc = np.float32(0.0)
    for n, r in enumerate(res):
        afc = c1 * afc + a * r
        out[n] = np.float32(20.0) * (r - afc) * one / k
    return out


def afc_scale_f64(res):
    """The same link behind the discriminator in float64, fmDcAlpha = 0.0001 and 1 - fmDcAlpha as the source states them: what the
    reference's f32 walk is measured against.  (The f32 pair (0.99989998, 9.9999997e-5) has a DC gain of 0.999834: on a mistuned carrier
    that, not the rounding, is most of the distance.)"""
    k, a = float(tables().K_FM), 0.0001
    c1 = 1.0 - a
    out = np.empty(res.shape[0], np.float64)
    afc = 0.0
    for n, r in enumerate(res.astype(np.float64).tolist()):
        afc = c1 * afc + a * r
        out[n] = 20.0 * (r - afc) / k
    return out


def demod_mixed_numpy(z):
    """Link D, Mixed decoder, restated: bit-identical to the oracle's TAP_DEMOD (tests/test_stage_b_model_cpu.py)."""
    return afc_scale_f32(discriminator_mixed(z))


def demod_peak(ref):
    return float(np.abs(np.asarray(ref, np.float64)[START_SKIP:]).max())


# ------------------------------------------------------------------------------------------------ link P
def pilot_oracle(demod):
    """fmo_pilot_run on 5 DEMOD (f32 product, fm-processor.cpp:693): (phase f32 [n], locked bool [n], lock metric f32 [n])."""
    T = tables()
    p = (np.float32(5.0) * np.ascontiguousarray(demod, np.float32)).astype(np.float32)
    n = p.shape[0]
    ph, lk, st = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
    T.L.fmo_pilot_run(FM_RATE, T.omega, T.gain, fptr(p), n, fptr(ph), lk.ctypes.data_as(C.POINTER(C.c_uint8)), fptr(st))
    return ph, lk.astype(bool), st


def pi_constrain(v):
    """PI_Constrain fm-constants.h:148-158 on an f32 scalar: compares and fmod in f64, the result back to f32."""
    d = float(v)
    if 0.0 <= d < TWO_PI:
        return v
    if d >= TWO_PI:
        return np.float32(np.fmod(d, TWO_PI))
    if d > -TWO_PI:
        return np.float32(d + TWO_PI)
    return np.float32(TWO_PI - np.fmod(-d, TWO_PI))


def pilot_numpy(pilot, sin_table=None):
    """pilot-recover.cpp:54-83 restated in numpy f32 scalars, on pilot = 5 DEMOD: (phase, locked, metric) as pilot_oracle; with
    `sin_table` another sine table than the reference's (the bound of the sequential solver: what the kernel's freedom in the NCO sine does
    to the reference's own loop)."""
    T = tables()
    tab = T.sin if sin_table is None else np.asarray(sin_table, np.float32)
    omega, gain, Cc = T.omega, T.gain, T.Cc
    alpha = np.float32(1.0) / np.float32(3000.0)
    keep = 1.0 - float(alpha)
    n = pilot.shape[0]
    ph, lk, st = np.empty(n, np.float32), np.zeros(n, bool), np.empty(n, np.float32)
    phase = old = lock = np.float32(0.0)
    locked, stable = False, 0
    for i, x in enumerate(np.asarray(pilot, np.float32)):
        osc = tab[int(float(phase) * Cc) % FM_RATE] if phase >= 0 else -tab[int(float(-phase) * Cc) % FM_RATE]
        err = x * osc
        phase = phase + err * gain
        cur = pi_constrain(phase)
        phase = pi_constrain(phase + omega)
        quad = (osc - old) / omega
        old = osc
        lock = np.float32(float(alpha * (-quad * x)) + float(lock) * keep)
        if lock > LOCK_THRESHOLD:
            stable += 0 if locked else 1
            if locked or stable > (FM_RATE >> 1):
                locked = True
        else:
            locked, stable = False, 0
        ph[i], lk[i], st[i] = cur, locked, lock
    return ph, lk, st


def perturbed_sines(seed=None):
    """The reference's sine table moved by up to HW_SINE per entry: uniformly at random (seed), or (seed None) every entry by the full
    amount away from zero -- a sine unit that errs to one side."""
    T = tables()
    s = T.sin.astype(np.float64)
    if seed is None:
        return (s + HW_SINE * np.sign(s)).astype(np.float32)
    return (s + HW_SINE * np.random.default_rng(seed).uniform(-1.0, 1.0, s.shape[0])).astype(np.float32)


def wrapped(a, b):
    """|a - b| on the circle, float64."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.abs((d + np.pi) % TWO_PI - np.pi)


def lock_crossings(metric):
    """The samples at which the lock metric changes sides of 0.07, and its smallest distance to 0.07 over the whole stream."""
    above = np.asarray(metric, np.float32) > LOCK_THRESHOLD
    cross = np.flatnonzero(above[1:] != above[:-1]) + 1
    return cross, float(np.abs(np.asarray(metric, np.float64) - float(LOCK_THRESHOLD)).min())


# ------------------------------------------------------------------------------------------------ link S
def mix_phase(cur, pdp):
    """phaseforLRDiff fm-processor.cpp:707-714: f32 (2 (cur + pi / 4) - pilotDelayPSS), the < -2 pi branch, f32 (fmod (., 2 pi))."""
    ph = (2.0 * (np.asarray(cur, np.float32).astype(np.float64) + np.pi / 4) - np.asarray(pdp, np.float32).astype(np.float64)).astype(np.float32)
    ph = np.where(ph.astype(np.float64) < -TWO_PI, (ph.astype(np.float64) + 2 * TWO_PI).astype(np.float32), ph)
    return np.fmod(ph.astype(np.float64), TWO_PI).astype(np.float32)


def mix_index(ph, selector=0):
    """The table index of the 38 kHz mix for the phases of mix_phase (never negative: cur >= 0, pilotDelayPSS <= pi / 4).  Cosine (getCos
    sincos.cpp:87-91): a second f32 (fmod (., 2 pi)) -- 6.2831855f, what the first one rounds to just below a whole turn, becomes 1.7e-7 --;
    sine, selector 6 (getSin :81-85): none, the index is taken modulo the table's length."""
    p = np.asarray(ph, np.float32)
    assert not (p < 0).any()
    if selector != 6:
        p = np.fmod(p.astype(np.float64), TWO_PI).astype(np.float32)
    return (p.astype(np.float64) * tables().Cc).astype(np.int32) % FM_RATE


def mix_index_unrounded(cur, pdp):
    """A seed for the detector: the index from the fraction of the turn in f64, without the f32 roundings of the two fmods."""
    p = (2.0 * (np.asarray(cur, np.float32).astype(np.float64) + np.pi / 4) - np.asarray(pdp, np.float32).astype(np.float64)).astype(np.float32)
    return np.minimum(((p.astype(np.float64) / TWO_PI) % 1.0 * FM_RATE).astype(np.int32), FM_RATE - 1)


def lr_diff(demod, cur, stereo, pdp=None, selector=0, cos_table=None, unrounded=False):
    """LR_RAW.im of every sample: (float)(2.0 * lut * demod) where `stereo` (not Mono, and locked or no auto-mono), else 0.  cos_table,
    unrounded: seeds for the detector."""
    T = tables()
    demod = np.asarray(demod, np.float32)
    pdp = np.zeros(demod.shape[0], np.float32) if pdp is None else pdp
    idx = mix_index_unrounded(cur, pdp) if unrounded else mix_index(mix_phase(cur, pdp), selector)
    tab = T.sin if selector == 6 else (T.cos if cos_table is None else cos_table)
    lut = tab[idx]
    d = (2.0 * lut.astype(np.float64) * demod.astype(np.float64)).astype(np.float32)
    return np.where(np.asarray(stereo, bool), d, np.float32(0.0)).astype(np.float32)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def s_bound(demod, ref):
    """Per sample: 2 |demod| S_SINE + one ulp of the value."""
    return 2.0 * np.abs(np.asarray(demod, np.float64)) * S_SINE + ulp32(ref)


class PssLoop:
    """The oracle's fmo_pss_* driven in closed loop with a handle's own DEMOD, phase and lock (fm-processor.cpp:697-716): the accumulator
    pilotDelayPSS in front of every sample and LR_RAW.im of it."""

    def __init__(self):
        T = tables()
        self.T = T
        T.L.fmo_pss_process.restype = C.c_float
        self.h = T.L.fmo_pss_new(FM_RATE, T.pss_alpha, T.sc)

    def run(self, demod, cur, locked, auto_mono=True, selector=0, perturb=0.0):
        """-> (LR_RAW.im [n] f32, pilotDelayPSS used by every sample [n] f32, ... behind every sample [n]).  perturb: added to the
        accumulator the mix reads (the CPU test's slip measurement), not to the loop's own state."""
        T, L, h = self.T, self.T.L, self.h
        n = demod.shape[0]
        used, after = np.zeros(n, np.float32), np.zeros(n, np.float32)
        ph = np.zeros(n, np.float32)
        pdp = np.float32(0.0)
        dm, cu, lk = np.asarray(demod, np.float32), np.asarray(cur, np.float32), np.asarray(locked, bool)
        for i in range(n):
            if not lk[i]:
                pdp = np.float32(0.0)
                L.fmo_pss_reset(h)
            if lk[i] or not auto_mono:
                used[i] = pdp
                p = mix_phase(cu[i:i + 1], np.array([pdp], np.float32))[0]
                ph[i] = p
                pdp = np.float32(L.fmo_pss_process(h, C.c_float(dm[i]), C.c_float(p)))
            after[i] = pdp
        stereo = lk | (not auto_mono)
        diff = lr_diff(dm, cu, stereo, (used.astype(np.float64) + perturb).astype(np.float32), selector)
        return diff, used, after

    def close(self):
        if self.h:
            self.T.L.fmo_pss_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------ link E
def deemph_alpha(us=50):
    """setDeemphasis fm-processor.cpp:291-297: Tau is a float."""
    tau = np.float32(1000000.0 / us)
    return np.float32(1.0 / (float(np.float32(FM_RATE) / tau) + 1.0))


def matrix_f32(lr_raw, selector=0, fm_mode=0, panorama=100):
    """fm-processor.cpp:517-549 in the reference's f32 expressions: [n, 2] f32."""
    s, d = np.asarray(lr_raw, np.float32)[:, 0], np.asarray(lr_raw, np.float32)[:, 1]
    pano = np.float32(np.int16(panorama)) / np.float32(100.0) if fm_mode == 1 else np.float32(1.0)
    dw = (d * pano).astype(np.float32)
    left, right = (s + dw).astype(np.float32), (s - dw).astype(np.float32)
    pair = {0: (left, right), 1: (right, left), 2: (left, left), 3: (right, right), 4: (s, s), 5: (dw, dw), 6: (dw, dw)}[int(selector)]
    return np.stack(pair, axis=1).astype(np.float32)


def one_pole_f64(x, alpha, drop_state_at=None):
    """y <- (x - y) alpha + y from y = 0, in float64 on the f32 coefficient, both columns.  drop_state_at: a seed for the detector -- the state
    zeroed in front of that sample (a segment that lost its carry)."""
    a = float(np.float32(alpha))
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    for c in range(x.shape[1]):
        y = 0.0
        col = x[:, c].tolist()
        o = [0.0] * len(col)
        for n, v in enumerate(col):
            if n == drop_state_at:
                y = 0.0
            y = (v - y) * a + y
            o[n] = y
        out[:, c] = o
    return out


def one_pole_f32(x, alpha):
    """The reference's own recurrence (:594-595) in f32."""
    a = np.float32(alpha)
    x = np.asarray(x, np.float32)
    out = np.empty_like(x)
    for c in range(x.shape[1]):
        y = np.float32(0.0)
        for n, v in enumerate(x[:, c]):
            y = (v - y) * a + y
            out[n, c] = y
    return out


def link_e(lr_raw, selector=0, fm_mode=0, panorama=100, deemph_us=50, drop_state_at=None):
    """LR_RAW [n, 2] f32 -> PRE_RESAMPLER [n, 2] float64 (folded handles: the de-emphasis straight behind the matrix, in front of the gain)."""
    return one_pole_f64(matrix_f32(lr_raw, selector, fm_mode, panorama), deemph_alpha(deemph_us), drop_state_at)


# ------------------------------------------------------------------------------------------------ comparison
class Worst:
    """The worst sample of a comparison and where the kernel made it: the call whose read-out holds it, the segment of 1536 fm samples
    within that call and the thread (six consecutive samples each) within the segment."""

    def __init__(self, link, channel, q, err, index, scale, rms, call_starts, count=0):
        self.link, self.channel, self.rel, self.err, self.index, self.scale, self.rms, self.count = link, channel, q, err, index, scale, rms, count
        cs = np.asarray(call_starts if call_starts is not None and len(call_starts) else [0], np.int64)
        self.call = max(int(np.searchsorted(cs, index, side="right") - 1), 0)
        r = int(index - cs[self.call])
        self.segment, self.thread = r // SEG, r % SEG // PER_THREAD

    def where(self):
        return "link %s, channel %s: fm sample %d = call %d, segment %d, thread %d" % (self.link, self.channel, self.index, self.call, self.segment, self.thread)

    def __str__(self):
        return "worst sample %.3e (%.3e of %.4g) at %s; rms %.3e" % (self.err, self.rel, self.scale, self.where(), self.rms)


def locate(link, channel, index, call_starts):
    return Worst(link, channel, 0.0, 0.0, int(index), 1.0, 0.0, call_starts).where()


def compare(link, channel, got, ref, call_starts=None, scale=None, allowed=None, circular=False):
    """Sample-by-sample distance of `got` to `ref` ([n] or [n, 2]).  scale: a number (default: the largest |ref|) -- the result is relative to
    it; allowed: a per-sample absolute bound instead -- the result is the worst ratio error / allowed.  circular: phases, compared on the circle."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert g.shape == r.shape and g.shape[0] > 0, (link, g.shape, r.shape)
    e = wrapped(g, r) if circular else np.abs(g - r)
    if e.ndim == 2:
        e = e.max(axis=1)
    if allowed is not None:
        al = np.asarray(allowed, np.float64)
        al = al.max(axis=1) if al.ndim == 2 else al
        q = np.where(al > 0, e / np.where(al > 0, al, 1.0), np.where(e > 0, np.inf, 0.0))
        i = int(np.argmax(q))
        return Worst(link, channel, float(q[i]), float(e[i]), i, float(al[i]), float(np.sqrt(np.mean(e ** 2))), call_starts, int((q > 1.0).sum()))
    sc = float(np.abs(r).max()) if scale is None else float(scale)
    assert sc > 0, (link, channel, "an empty reference")
    i = int(np.argmax(e))
    return Worst(link, channel, float(e[i]) / sc, float(e[i]), i, sc, float(np.sqrt(np.mean(e ** 2))), call_starts)


def check(w, bound, note=""):
    """The worst-sample assertion: a failure names link, channel, call, segment and thread."""
    assert w.rel <= bound, "%s%s exceeds the bound %.3e -- %s" % (note + ": " if note else "", "%.3e" % w.rel, bound, w)


def report(name, w, bound):
    print("\n[%s] %s (bound %.3e)" % (name, w, bound))


def first_differences(link, channel, got, ref, call_starts, limit=8):
    """Bit identity: (count, a description of the first `limit` differing samples with call, segment and thread)."""
    g, r = np.asarray(got), np.asarray(ref)
    assert g.shape == r.shape, (link, g.shape, r.shape)
    ne = g.view(np.uint32) != r.view(np.uint32) if g.dtype == np.float32 else g != r
    if ne.ndim == 2:
        ne = ne.any(axis=1)
    bad = np.flatnonzero(ne)
    lines = ["%s: got %r, reference %r" % (locate(link, channel, i, call_starts), g[i].tolist(), r[i].tolist()) for i in bad[:limit]]
    return bad.size, "; ".join(lines)


def check_identical(link, channel, got, ref, call_starts=None):
    n, text = first_differences(link, channel, got, ref, call_starts)
    assert n == 0, "link %s, channel %s: %d of %d samples differ from the reference -- %s" % (link, channel, n, np.asarray(ref).shape[0], text)


def check_d_batch(channel, got, ref, decoder, call_starts=None, name=""):
    """Link D of a batch (the fast forms): every sample within D_BATCH_BOUND of the peak, except that up to D_SLIP_SHARE of the samples may
    be off by at most one table step instead.  -> (Worst of the normal samples, share of slips, the largest slip of the peak)."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    peak = demod_peak(ref)
    e = np.abs(g - r)
    slip = e > D_BATCH_BOUND * peak
    step = tables().table_step(decoder)
    share = float(slip.mean())
    big = float(e[slip].max()) / peak if slip.any() else 0.0
    normal = np.where(slip, 0.0, e)
    w = compare("D", channel, np.where(slip, r, g), r, call_starts, scale=peak)
    print("\n[%s link D, channel %s] normal samples: %s (bound %.3e); table slips: %.4f %% of the samples (cap %.2f %%), the largest %.3e of the peak (one step %.3e)"
          % (name, channel, w, D_BATCH_BOUND, 100 * share, 100 * D_SLIP_SHARE, big, step / peak))
    if slip.any():
        i = int(np.argmax(np.where(slip, e, 0.0)))
        assert e[i] <= step, "a sample beyond one table step (%.3e > %.3e) -- %s" % (e[i], step, locate("D", channel, i, call_starts))
    assert share <= D_SLIP_SHARE, "link D, channel %s: %.4f %% of the samples beyond %.2e of the peak, first at %s" % (
        channel, 100 * share, D_BATCH_BOUND, locate("D", channel, int(np.flatnonzero(slip)[0]), call_starts))
    assert float(normal.max()) <= D_BATCH_BOUND * peak
    return w, share, big


def check_s(channel, got_im, ref_im, demod, call_starts=None, slip_share=0.0, name=""):
    """Link S: LR_RAW.im of every sample within 2 |demod| S_SINE + an ulp of the reference; with slip_share > 0 that share of the samples may
    instead be off by one table step, 2 |demod| TABLE_STEP (PSS on).  -> (Worst, share of slips)."""
    g, r, d = np.asarray(got_im, np.float64), np.asarray(ref_im, np.float64), np.abs(np.asarray(demod, np.float64))
    al = s_bound(demod, ref_im)
    e = np.abs(g - r)
    over = e > al
    share = float(over.mean())
    w = compare("S", channel, got_im, ref_im, call_starts, allowed=al)
    print("\n[%s link S, channel %s] %s -- %d of %d samples (%.4f %%) beyond 2 |demod| %.1e + 1 ulp; the largest error %.3e |demod|"
          % (name, channel, w, int(over.sum()), g.shape[0], 100 * share, S_SINE, float((e / np.maximum(d, 1e-30)).max()) if g.shape[0] else 0.0))
    if slip_share == 0.0:
        assert not over.any(), "link S: %d samples (%.4f %%) beyond the bound, the worst %.2f times its bound -- %s" % (int(over.sum()), 100 * share, w.rel, w)
        return w, share
    wide = al + 2.0 * d * TABLE_STEP
    i = int(np.argmax(e - wide))
    assert e[i] <= wide[i], "link S: beyond one table step (%.3e > %.3e) -- %s" % (e[i], wide[i], locate("S", channel, i, call_starts))
    assert share <= slip_share, "link S, channel %s: %.3f %% of the samples one table step off (cap %.1f %%)" % (channel, 100 * share, 100 * slip_share)
    return w, share

"""The RDS back end -- everything of fmx_rds.hip between the 24 kS/s baseband and the bit ring -- compared per symbol and per call:
what tests/test_rds_slicer_cpu.py (no GPU) and tests/test_gpu_rds_slicers.py share.

  reference    the oracle's slicers as an object of their own (oracle_lib.OracleRdsSlicer: rdsDecoder_1 / _2 / _3 of fm_oracle.c, unchanged),
               resumed over exactly the samples a call got: run_oracle ()
  comparison   compare (): per call the number of bits, every bit, every RDS_2 symbol, the scalar state behind every call
  yardstick    SENS: the oracle against itself with every input sample times (1 + 2^-23 u), u uniform in +-1 (test_rds_slicer_cpu.py measures
               it and holds the constants below to it).  The GPU bound is BOUND_FACTOR = 4 times SENS: the kernels differ from the oracle by
               one rounding in each of up to four places -- a possibly contracted multiply-add in the FIR sums, the gain handed from one lane's
               walk to the threads' (an f64 scan when this was written: see rds_agc), the device's sinf / cosf, and gain * |in| in place of
               |gain * in|.  Never measured on the kernels.
  admission    admit (): inputs on which the reference's own decisions are safe -- (a) mMu stays 1e-4 away from an integer at every live
               symbol (only (int) mMu is ever used: closer than that, another rounding may move a symbol by a sample), (b) every decision whose
               variable is below 1e-3 of its peak lies within 64 bit periods behind the baseband's first non-zero sample
  model        rds2_model (): rdsDecoder_2 restated in numpy, in float64 (confirms the oracle's decisions; its distance is recorded) or in
               float32 with a seeded defect of the kind the kernels' restructuring invites (the detector must detect)
"""
import collections
import functools

import numpy as np

import oracle_lib as ol

SECONDS = 2.0                      # of every signal; the GPU cases and the admission use the first GPU_SECONDS of the same signals
GPU_SECONDS = 1.5
RATE_IN, RATE_24K, BIT_RATE = 2304000, 24000, 1187.5
SPS = RATE_24K / BIT_RATE           # 20.21 samples per bit
LEAD_IN_BITS = 64
UNDECIDED = 1e-3                   # of the decision variable's peak
MU_MARGIN = 1e-4
MAX_UNDECIDED = 40
BOUND_FACTOR = 4

# the signals (oracle_lib.synth_iq keywords); the seeds are those that pass admit () for every mode (test_rds_slicer_cpu.py::test_admission)
SIGNALS = {
    "clean": dict(rds=1, rdsLevel=0.05, rdsBitsSeed=777),
    "noisy": dict(rds=1, rdsLevel=0.03, rdsBitsSeed=777, noiseSeed=4242, noiseSigma=0.02),
    "offset": dict(rds=1, rdsLevel=0.03, rdsBitsSeed=777, noiseSeed=5, noiseSigma=0.02, offsetHz=3000.0),   # (noise seeds 1 and 4242 fail check (a))
    "programme": dict(rds=1, rdsLevel=0.05, payload="programme"),   # whole groups (rds_programme_bits): RDS_3's block synchroniser locks
    # two rounds of the programme with a payload bit of block B (bit 31 of the group) flipped in the first 9 groups: RDS_3's synchroniser finds a
    # block A, fails on B and counts a sync error, the fourth resynchronises the bit clock in mid-stream (rds-decoder-3.cpp:95-100) -- twice in
    # 1.5 s --, then the groups are whole and it locks
    "sync_errors": dict(rds=1, rdsLevel=0.05, payload="sync_errors"),
}
SENS_SIGNALS = ("clean", "noisy", "offset")
# (signal, mode) as the one-receiver GPU tests use them: each passes admit ().  "programme" fails check (a) -- mMu within 7.3e-5 -- and is not used
# with RDS_2.
GPU_USES = [("clean", 2), ("noisy", 2), ("offset", 2), ("clean", 1), ("noisy", 1), ("programme", 1), ("clean", 3), ("noisy", 3), ("programme", 3),
            ("sync_errors", 3)]
# "sync_errors" is chosen like a seed.  The damage has to end: a payload that keeps RDS_3's synchroniser failing (a block A and a damaged block B,
# round and round) has the bit clock resynchronised again and again, onto phases at which up to 10 bits behind the lead-in are decided on less
# than 1e-3 of the peak -- it fails check (b) on the reference alone, from the third resynchronisation on.  Random bits give one or two sync
# errors in 1.5 s, never the fourth.

# Call lengths in input samples (12 per fm sample, 96 per 24 kS/s sample), 1.5 s in all.  In front of the baseband's first non-zero sample
# (24 kS/s sample 8000 = input sample 768000) and again behind it: 12 (no output or one), 192 (two outputs: rds_agc's branch for fewer than
# three), 288; then 245760 (2560 outputs: exactly one round of rds_agc), 245856 (a second round of one sample), 383988 (31999 fm samples),
# 500000 and 400000 (above 384000: made in pieces), and lengths off the 96-sample grid for the rest.
SIZES = [12, 192, 288, 383988, 500000, 12, 192, 288, 245760, 245856, 99991, 1939, 250001, 77777, 5, 400000, 383989, 245857, 333333, 286520]
assert sum(SIZES) == int(GPU_SECONDS * RATE_IN)

# The batch of 70: channel c on stream c % 2 ("clean", "noisy"), decoder c % 3 + 1, switched on with call 0 (channels 0-29), 2 (30-49) or 3 (50-69).
# The first two and the first three calls end on input samples 38 x 16384 and 52 x 16384 -- fm samples 51882 and 70997: with 0 three phases of the
# decimator by 8 (0, 2, 5) and of the 32000-sample blocks, and the oracle chain, which works in blocks of 16384, can be switched on at the very
# same sample for the admission (of the join points 16384 k, k = 34 ... 59 not a multiple of 3, most fail check (a) or (b) for one of the
# slicers; these two pass for all).  Channel 33 -- noisy, RDS_2, call 2 -- keeps mMu only 1.07e-4 from an integer: not a probe.
BATCH_SIZES = [383988, 238604, 229376, 500000, 12, 192, 288, 245760, 245856, 99991, 400000, 383989, 333333, 394611]
assert sum(BATCH_SIZES) == int(GPU_SECONDS * RATE_IN) and sum(BATCH_SIZES[:2]) == 38 * 16384 and sum(BATCH_SIZES[:3]) == 52 * 16384
BATCH_CHANNELS = 70
BATCH_PROBES = [0, 1, 2, 34, 35, 50, 55, 69]


def batch_channel(c):
    """-> (signal, mode, the call the decoder is switched on with)"""
    return ("clean", "noisy")[c % 2], c % 3 + 1, 0 if c < 30 else 2 if c < 50 else 3

# ---- SENS[mode]: worst distance of the oracle from itself under the perturbation above, over 16 draws and SENS_SIGNALS, relative to each
# quantity's peak ("symbol": |o|; the state fields: their largest magnitude behind a call, phases and bitClkPhase modulo 2 pi against 2 pi).
# Bits, bit times, bit counts and the integer fields did not change in any draw (asserted).  Measured by test_rds_slicer_cpu.py::test_sens,
# which fails when a constant is below what it measures or more than twice above it.
SENS = {
    2: {"symbol": 6.4e-7, "gain": 1.3e-7, "freq": 1.5e-5, "phase": 7.6e-8, "mu": 2.2e-6},
    1: {"freq": 6.5e-6, "phase": 9.5e-7, "last_sync": 1.8e-5},
    3: {"freq": 4.3e-6, "phase": 5.0e-7, "bit_clk_phase": 0.0},      # (bitClkPhase moves by a constant between resynchronisations: equal)
}
MODEL_F64_DISTANCE = 1.5e-4          # rds2_model in float64 against the oracle: worst symbol distance of the peak (test_f64_model)
INTEGER_FIELDS = ("skip", "sample_count", "sync_err", "synced")
CIRCULAR_FIELDS = ("phase", "bit_clk_phase")

Call = collections.namedtuple("Call", "n bits at vars state")       # n: 24 kS/s samples of the call; at: sample index of each bit (from the stream's start)


def samples_of(sizes, first=0):
    """24 kS/s samples each call from call `first` on produces on a channel whose decoder is switched on with that call (fmx_rds.hip: nout of a
    call; the channel counts its own fm samples from there)."""
    # a call of s input samples carries floor ((g + s) / 12) - floor (g / 12) fm samples, g the input samples so far
    n, g, res = 0, 0, []
    for k, s in enumerate(sizes):
        nj = (g + s) // 12 - g // 12
        g += s
        if k >= first:
            res.append((n + nj) // 8 - n // 8)
            n += nj
    return res


@functools.lru_cache(maxsize=None)
def signal(name):
    """SECONDS of the signal as IQ [n, 2], read-only."""
    kw = dict(SIGNALS[name])
    payload = kw.pop("payload", None)
    if payload == "programme":
        payload = ol.rds_programme_bits()
    elif payload == "sync_errors":
        payload = np.tile(ol.rds_programme_bits(), 2)
        payload[104 * np.arange(9) + 31] ^= 1
    iq = ol.synth_iq(int(SECONDS * RATE_IN), rds_payload=payload, **kw)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def chain_baseband(name, mode=2, start=0):
    """The oracle chain's own FMO_TAP_RDS_IQ over the signal and the bits its decoder `mode` sliced; the decoder is switched on in front of input
    sample `start` (the chain's RDS path stands still until then, as a channel's does)."""
    ch = ol.OracleChain(taps=[ol.TAP_RDS_IQ], inputFilterBw=165000, rdsMode=mode if start == 0 else 0, tap_seconds=SECONDS + 0.1)
    iq = signal(name)
    if start:
        ch.process(iq[:start])
        ch.configure(rdsMode=mode)
    for i in range(start, iq.shape[0], 16384 * 20):
        ch.process(iq[i:i + 16384 * 20])
    q, bits = ch.tap(ol.TAP_RDS_IQ).copy(), ch.rds_bits().copy()
    ch.close()
    q.setflags(write=False)
    return q, bits


def run_oracle(mode, iq, counts):
    """The oracle's slicer over iq [n, 2], stopped behind every call (counts: 24 kS/s samples per call) -> a list of Call."""
    s = ol.OracleRdsSlicer(mode)
    calls, pos = [], 0
    for n in counts:
        bits, at, var = s.run(iq[pos:pos + n])
        pos += n
        calls.append(Call(n, bits, at, var, s.state()))
    s.close()
    return calls


def flat(calls):
    return (np.concatenate([c.bits for c in calls]), np.concatenate([c.at for c in calls]), np.concatenate([c.vars for c in calls]))


def first_live(iq):
    """Index of the baseband's first non-zero sample."""
    nz = np.flatnonzero((np.asarray(iq).reshape(-1, 2) != 0).any(axis=1))
    assert nz.size, "the baseband is zero throughout"
    return int(nz[0])


def undecided(ref_calls, iq):
    """-> (mask over the reference's bits, live, peak): bits decided on a variable below UNDECIDED of its peak.  In front of the baseband's first non-zero
    sample nothing is undecided: every decision variable is exactly 0 there -- in any arithmetic -- and the bit follows from `>= 0`."""
    _, at, var = flat(ref_calls)
    live = first_live(iq)
    peak = float(np.abs(var[:, 0]).max())
    return (np.abs(var[:, 0]) < UNDECIDED * peak) & (at >= live), live, peak


def mu_margin(ref_calls, iq):
    """Smallest distance of rdsDecoder_2's mMu to an integer over the live symbols (vars [:, 2] is the fraction it keeps)."""
    _, at, var = flat(ref_calls)
    m = var[at >= first_live(iq), 2].astype(np.float64)
    return float(np.minimum(m, 1.0 - m).min())


def admit(mode, ref_calls, iq):
    """The two checks an input has to pass on the reference alone; -> (mMu margin or None, undecided bits).  Raises AssertionError otherwise."""
    und, live, _ = undecided(ref_calls, iq)
    _, at, _ = flat(ref_calls)
    late = at[und] >= live + LEAD_IN_BITS * SPS
    assert not late.any(), "choose another seed: RDS_%d decides %d bits on less than %.0e of the peak behind the lead-in (first at sample %d)" % (
        mode, int(late.sum()), UNDECIDED, int(at[und][late][0]))
    margin = None
    if mode == 2:
        margin = mu_margin(ref_calls, iq)
        assert margin >= MU_MARGIN, "choose another seed: mMu comes within %.2e of an integer" % margin
    return margin, int(und.sum())


def circular(a, b, period=2 * np.pi):
    d = abs(float(a) - float(b)) % period
    return min(d, period - d)


def state_distance(got, ref):
    """Per field |got - ref| (integer fields: must be equal, not returned)."""
    out = {}
    for k, r in ref.items():
        if k in INTEGER_FIELDS:
            assert got[k] == r, (k, got[k], r)
        else:
            out[k] = circular(got[k], r) if k in CIRCULAR_FIELDS else abs(float(got[k]) - float(r))
    return out


def state_peaks(ref_calls):
    pk = {}
    for k in ref_calls[0].state:
        if k not in INTEGER_FIELDS:
            pk[k] = 2 * np.pi if k in CIRCULAR_FIELDS else max(abs(c.state[k]) for c in ref_calls)
    return pk


def distances(mode, got, ref):
    """Worst distance of `got` from `ref` (lists of Call over the same calls) per quantity, relative to the quantity's peak in `ref`.  Bit counts per
    call and integer state fields must be equal (asserted); bits are not looked at.  -> {quantity: (relative distance, call)}"""
    assert len(got) == len(ref)
    pk = state_peaks(ref)
    worst = {k: (0.0, -1) for k in pk}
    if mode == 2:
        sym_peak = max(float(np.abs(c.vars[:, 0] + 1j * c.vars[:, 1]).max()) for c in ref if c.bits.size)
        worst["symbol"] = (0.0, -1)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.bits.size == r.bits.size, "call %d (%d samples): %d bits, the reference %d" % (k, r.n, g.bits.size, r.bits.size)
        try:
            d = state_distance(g.state, r.state)
        except AssertionError as e:
            raise AssertionError("call %d (%d samples): state %s" % (k, r.n, e)) from None
        for f, v in d.items():
            rel = v / pk[f] if pk[f] > 0 else (0.0 if v == 0 else np.inf)
            if rel > worst[f][0]:
                worst[f] = (rel, k)
        if mode == 2 and r.bits.size:
            dv = g.vars[:, :2].astype(np.float64) - r.vars[:, :2]
            rel = float(np.hypot(dv[:, 0], dv[:, 1]).max()) / sym_peak
            if rel > worst["symbol"][0]:
                worst["symbol"] = (rel, k)
    return worst


def compare(mode, got, ref, iq, bound=None):
    """The comparison of the GPU tests: `got` (the kernels', or a model's) against the reference over the same calls.
      * every call sliced as many bits as the reference over the same samples;
      * every bit is the reference's from the first one, but for those the reference itself marks undecided: only inside the lead-in, at most
        MAX_UNDECIDED;
      * RDS_2: every symbol within bound ["symbol"] of the peak;
      * behind every call every state field within bound [field] of its peak, the integer fields equal.
    bound: {quantity: relative bound}, default BOUND_FACTOR x SENS [mode].  -> the distances measured (for the record)."""
    if bound is None:
        bound = {k: BOUND_FACTOR * v for k, v in SENS[mode].items()}
    w = distances(mode, got, ref)
    und, live, _ = undecided(ref, iq)
    _, at, _ = flat(ref)
    assert int(und.sum()) <= MAX_UNDECIDED and not (at[und] >= live + LEAD_IN_BITS * SPS).any(), "choose another seed: %d undecided bits" % int(und.sum())
    gb, rb = np.concatenate([c.bits for c in got]), np.concatenate([c.bits for c in ref])
    bad = np.flatnonzero((gb != rb) & ~und)
    assert bad.size == 0, "RDS_%d: %d decided bits differ, the first is bit %d (sample %d)" % (mode, bad.size, bad[0], at[bad[0]])
    for k, (rel, call) in w.items():
        assert rel <= bound[k], "RDS_%d %s: %.3e of the peak in call %d (%d samples), bound %.3e" % (mode, k, rel, call, ref[call].n, bound[k])
    return w


# ------------------------------------------------------------------------------------------------ rdsDecoder_2 restated
DEFECTS = ("tap44", "lookback", "agc_round", "late_symbol", "count_off")


def rrc_taps():
    t = np.zeros(45, np.float32)
    n = ol.oracle().fmo_rrc_kernel(1.0, 24000.0, 2 * 1187.5, 1.0, 45, ol.fptr(t))
    assert n == 45
    return t


def pi_constrain(F, ph):
    v = float(ph)
    if 0.0 <= v < 2 * np.pi:
        return ph
    if v >= 2 * np.pi:
        return F(np.fmod(v, 2 * np.pi))
    if v > -2 * np.pi:
        return F(v + 2 * np.pi)
    return F(2 * np.pi - np.fmod(-v, 2 * np.pi))


def rds2_model(iq, counts, F=np.float64, defect=None, where=None):
    """rdsDecoder_2::doDecode (rds-decoder-2.cpp:83-157) in numpy arithmetic of type F, laid out as the kernels lay it out -- matched filter
    time-parallel, AGC over every sample, symbols in a second pass -- over the calls `counts`; -> a list of Call like run_oracle (2, ...).
    defect: one of DEFECTS, seeded at call / symbol `where` --
      tap44        the matched filter's last tap is dropped
      lookback     the call's first symbol sees zeros for the AGC outputs in front of the call (v [q - 2], v [q - 1])
      agc_round    the AGC's second round of 2560 samples in a call starts from the call's first gain
      late_symbol  symbol `where` is taken a sample late
      count_off    sampleCount behind call `where` is one too large"""
    assert defect is None or defect in DEFECTS
    x = np.asarray(iq, np.float32).reshape(-1, 2).astype(F)
    n = x.shape[0]
    assert sum(counts) == n
    w = rrc_taps().astype(F)
    # matched filter: tmp += mfbuf [m - i] * mf [i], i ascending, from zero
    mre, mim = np.zeros(n, F), np.zeros(n, F)
    for i in range(45):
        if defect == "tap44" and i == 44:
            continue
        mre[i:] = mre[i:] + x[:n - i, 0] * w[i]
        mim[i:] = mim[i:] + x[:n - i, 1] * w[i]
    mag = np.sqrt(mre.astype(np.float64) ** 2 + mim.astype(np.float64) ** 2).astype(F)     # |in|: cabs of the complex sample, rounded to F
    starts = np.concatenate([[0], np.cumsum(counts)])
    # AGC (2e-3, 0.38, from 9): out = in * gain; gain += rate * (ref - |out|)
    rate, ref = F(np.float32(2e-3)), F(np.float32(0.38))
    gain = F(9.0)
    are, aim = np.zeros(n, F), np.zeros(n, F)
    gain_behind = []
    for k, cnt in enumerate(counts):
        g0 = gain
        for q in range(cnt):
            m = starts[k] + q
            if defect == "agc_round" and q > 0 and q % 2560 == 0 and (where is None or where == k):
                gain = g0
            ore, oim = mre[m] * gain, mim[m] * gain
            are[m], aim[m] = ore, oim
            gain = gain + rate * (ref - F(np.sqrt(float(ore) ** 2 + float(oim) ** 2)))
        gain_behind.append(gain)
    # Mueller & Mueller, Costas (alpha 1, beta 0.02, +-10 Hz), slicer, differential decoder
    sps, alpha = F(np.float32(24000.0) / np.float32(1187.5)), F(np.float32(0.01))
    mu, skip, count, prev = F(0), 3, 0, 0
    freq, phase, lim = F(0), F(0), F(np.float32(2 * np.pi * 10.0 / 24000.0))
    one, nsym, calls = F(1), 0, []
    rail = lambda v: one if v > 0 else -one
    for k, cnt in enumerate(counts):
        bits, at, var = [], [], []
        first = True
        for q in range(cnt):
            m = starts[k] + q
            count += 1
            fire = count >= skip
            if defect == "late_symbol" and nsym == where:
                fire = count >= skip + 1
            if not fire:
                continue
            s = []
            for d in (2, 1, 0):
                j = m - d
                zero = j < 0 or (defect == "lookback" and first and (where is None or where == k) and j < starts[k])
                s.append((F(0), F(0)) if zero else (are[j], aim[j]))
            first = False
            (s0r, s0i), (s1r, s1i), (s2r, s2i) = s
            xx = (rail(s2r) - rail(s0r)) * s1r + (rail(s2i) - rail(s0i)) * s1i
            yy = (s2r - s0r) * rail(s1r) + (s2i - s0i) * rail(s1i)
            mu = mu + (sps + alpha * (yy - xx))
            skip = int(mu)
            mu = mu - F(skip)
            count = 0
            c, sn = F(np.cos(-phase)), F(np.sin(-phase))
            ore, oim = s2r * c - s2i * sn, s2r * sn + s2i * c
            err = ore * oim
            freq = freq + F(np.float32(0.02)) * err
            if abs(freq) > lim:
                freq = F(0)
            phase = pi_constrain(F, phase + (freq + err))
            bit = 1 if ore >= 0 else 0
            bits.append(bit ^ prev)
            prev = bit
            at.append(m)
            var.append((ore, oim, mu, skip))
            nsym += 1
        if defect == "count_off" and where == k:
            count += 1
        state = dict(gain=float(gain_behind[k]), freq=float(freq), phase=float(phase), mu=float(mu), skip=float(skip), sample_count=float(count))
        calls.append(Call(cnt, np.array(bits, np.uint8), np.array(at, np.int64), np.array(var, np.float64).reshape(-1, 4), state))
    return calls

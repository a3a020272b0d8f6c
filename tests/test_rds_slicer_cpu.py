"""The reference side of tests/test_gpu_rds_slicers.py, on the CPU: the oracle's slicers as an object of their own (fmo_rds_slicer), the float64
restatement of rdsDecoder_2, the yardstick SENS, the admission of the inputs, and a proof that the comparison detects what it is there to detect
(tests/rds_slicer_model.py).  Every baseband here is the oracle chain's own FMO_TAP_RDS_IQ; nothing is measured on the kernels.

Recorded here (2 s signals; `pytest -s` prints every figure):
  consistency  the stand-alone slicer on the chain's baseband gives fmo_chain_rds_bits bit for bit, modes 1, 2, 3, in one run and in ragged runs
  float64      the same 2373 bits at the same 2373 samples as the oracle; symbols within 1.5e-4 of the peak (worst inside the pull-in), mMu within 9e-5
  SENS         see rds_slicer_model.SENS; no bit, bit time, bit count or integer state changed in any of 16 draws on three signals
  margins      mMu stays 1.9e-4 (clean), 3.2e-4 (noisy, offset) away from an integer; 35-36 undecided bits per slicer, the last 47 bit periods
               behind the baseband's first non-zero sample
"""
import numpy as np
import pytest

import rds_slicer_model as rm

N15 = int(rm.GPU_SECONDS * rm.RATE_24K)
COUNTS = rm.samples_of(rm.SIZES)


def gpu_part(name, mode):
    """The first GPU_SECONDS of the chain's baseband in the GPU tests' calls, through the oracle's slicer."""
    q = rm.chain_baseband(name, mode)[0][:N15]
    return q, rm.run_oracle(mode, q, COUNTS)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("name", ["clean", "noisy", "programme"])
def test_consistency(ol, name, mode):
    """fmo_rds_slicer on the chain's own FMO_TAP_RDS_IQ gives fmo_chain_rds_bits bit for bit -- in one run, and resumed over ragged runs (some of
    no sample, of one, of two), where bit times and decision variables are the single run's too."""
    q, bits = rm.chain_baseband(name, mode)
    whole = rm.run_oracle(mode, q, [q.shape[0]])
    assert np.array_equal(whole[0].bits, bits) and bits.size > 1900
    counts = (COUNTS + [0, 1, 2, 7, 2561, 5000])
    counts.append(q.shape[0] - sum(counts))
    parts = rm.run_oracle(mode, q, counts)
    for a, b in zip(rm.flat(parts), rm.flat(whole)):
        assert np.array_equal(a, b)
    assert parts[-1].state == whole[0].state
    assert np.all(np.diff(rm.flat(whole)[1]) > 0)


def test_f64_model():
    """rdsDecoder_2 restated in float64 (matched filter, AGC, Mueller & Mueller, Costas) decides the oracle's bits at the oracle's samples; its symbols
    differ by more than SENS -- float64 is not the yardstick here -- but by less than UNDECIDED of the peak, so it confirms every decided bit."""
    worst = 0.0
    for name in ("clean", "noisy"):
        q = rm.chain_baseband(name, 2)[0]
        ref = rm.run_oracle(2, q, [q.shape[0]])
        got = rm.rds2_model(q, [q.shape[0]], np.float64)
        (gb, ga, gv), (rb, ra, rv) = rm.flat(got), rm.flat(ref)
        assert np.array_equal(ga, ra), name
        assert np.array_equal(gb, rb), name
        peak = np.abs(rv[:, 0] + 1j * rv[:, 1]).max()
        d = np.hypot(gv[:, 0] - rv[:, 0], gv[:, 1] - rv[:, 1])
        dmu = np.abs(gv[:, 2] - rv[:, 2])
        print("\n[rds2 float64 model, %s] %d bits; symbols %.2e of the peak %.3f (bit %d, baseband live from bit %d); mMu %.2e"
              % (name, rb.size, d.max() / peak, peak, d.argmax(), np.searchsorted(ra, rm.first_live(q)), dmu.max()))
        assert np.array_equal(gv[:, 3], rv[:, 3])                       # skip
        worst = max(worst, d.max() / peak)
    assert worst < rm.UNDECIDED
    assert worst <= rm.MODEL_F64_DISTANCE <= 2 * worst, worst


def test_sens():
    """The oracle against itself with every input sample times (1 + 2^-23 u): bits, bit times, counts and integer states identical in all 16 draws
    on the three signals; the worst distances are rds_slicer_model.SENS."""
    rng = np.random.default_rng(20240611)
    meas = {m: {k: 0.0 for k in rm.SENS[m]} for m in (1, 2, 3)}
    for name in rm.SENS_SIGNALS:
        q = rm.chain_baseband(name, 2)[0]                  # (the baseband does not depend on the decoder)
        counts = COUNTS + [q.shape[0] - N15]
        for mode in (1, 2, 3):
            ref = rm.run_oracle(mode, q, counts)
            for draw in range(16):
                u = rng.uniform(-1.0, 1.0, q.shape)
                p = (q.astype(np.float64) * (1.0 + 2.0 ** -23 * u)).astype(np.float32)
                got = rm.run_oracle(mode, p, counts)
                for a, b in zip(rm.flat(got)[:2], rm.flat(ref)[:2]):
                    assert np.array_equal(a, b), (name, mode, draw)
                for k, (rel, _) in rm.distances(mode, got, ref).items():
                    meas[mode][k] = max(meas[mode][k], rel)
    for mode in (1, 2, 3):
        print("\n[SENS] RDS_%d: %s" % (mode, ", ".join("%s %.3e" % kv for kv in meas[mode].items())))
    for mode in (1, 2, 3):
        for k, v in meas[mode].items():
            assert v <= rm.SENS[mode][k] <= 2 * v, (mode, k, v, rm.SENS[mode][k])


@pytest.mark.parametrize("name,mode", rm.GPU_USES)
def test_admission(name, mode):
    """Every signal the GPU tests use, on the reference alone: (a) mMu at least 1e-4 from an integer at every live symbol, (b) every decision on
    less than 1e-3 of the peak within 64 bit periods behind the baseband's first non-zero sample, at most 40 of them (34-36 here)."""
    q, ref = gpu_part(name, mode)
    margin, und = rm.admit(mode, ref, q)
    print("\n[admission] %s, RDS_%d: mMu margin %s, %d undecided bits" % (name, mode, margin, und))
    assert 30 <= und <= rm.MAX_UNDECIDED
    if name == "sync_errors":                     # what the signal is for: n_sync_err > 3 resynchronises the bit clock in mid-stream and clears the count
        _, at, var = rm.flat(ref)
        cleared = np.flatnonzero(np.diff(var[:, 3]) < 0)
        errs = [int(c.state["sync_err"]) for c in ref]
        print("            sync errors behind the calls: %s; cleared behind bits %s (samples %s); synced at the end: %d"
              % (errs, cleared.tolist(), at[cleared].tolist(), ref[-1].state["synced"]))
        assert cleared.size >= 2 and at[cleared[0]] > rm.first_live(q) + rm.LEAD_IN_BITS * rm.SPS and ref[-1].state["synced"] == 1
        assert any(b < a for a, b in zip(errs, errs[1:]))          # ... and the states behind the calls show it


@pytest.mark.parametrize("c", rm.BATCH_PROBES)
def test_admission_of_the_batch_probes(c):
    """The probe channels of the batch of 70, whose decoders are switched on with calls 0, 2 and 3: the oracle chain switched on at the same input
    sample, in the batch's calls."""
    name, mode, join = rm.batch_channel(c)
    counts = rm.samples_of(rm.BATCH_SIZES, join)
    q = rm.chain_baseband(name, mode, sum(rm.BATCH_SIZES[:join]))[0][:sum(counts)]
    assert q.shape[0] == sum(counts)
    margin, und = rm.admit(mode, rm.run_oracle(mode, q, counts), q)
    print("\n[admission] channel %d: %s, RDS_%d, on from call %d: mMu margin %s, %d undecided bits" % (c, name, mode, join, margin, und))
    assert und <= rm.MAX_UNDECIDED and (margin is None or margin >= 1.5 * rm.MU_MARGIN)


def test_f32_model_passes():
    """rds2_model in float32, unseeded, against the oracle through the GPU tests' comparison at the GPU tests' bound: the comparison does not
    fail on a restatement that is right (numpy's cos / sin for libm's, gain from another loop)."""
    q, ref = gpu_part("clean", 2)
    w = rm.compare(2, rm.rds2_model(q, COUNTS, np.float32), ref, q)
    print("\n[rds2 float32 model, unseeded] %s" % ", ".join("%s %.2e" % (k, v[0]) for k, v in w.items()))


# where: lookback -- every call's first symbol; agc_round -- call 15 (4166 samples; in call 4, where the baseband comes alive and the gain falls from 15
# to 7, the defect costs bits of the pull-in, which the existing tests leave out); late_symbol -- symbol 1200 (the baseband is live from symbol 396);
# count_off -- behind call 10.  expect: the check of compare () that has to catch it (its message) -- not just any assertion, such as an admission's
@pytest.mark.parametrize("defect,where,expect", [
    ("tap44", None, r"RDS_2 gain: .* of the peak"), ("lookback", None, r"RDS_2 (freq|phase|symbol|mu): .* of the peak"),
    ("agc_round", 15, r"RDS_2 gain: .* of the peak in call 15"), ("late_symbol", 1200, r"state \('sample_count'"),
    ("count_off", 10, r"call 10 .*state \('sample_count'")])
def test_detector_detects(defect, where, expect):
    """Each defect of the kind the kernels' restructuring invites, seeded into the float32 restatement: the bits stay what they were -- the
    existing bit comparisons cannot see it -- and the comparison of the GPU tests fails, in the check that is there for it.  (lookback shows in
    one call only -- call 17, of 2561 samples -- by 40 times the bound on freq.)"""
    q, ref = gpu_part("clean", 2)
    got = rm.rds2_model(q, COUNTS, np.float32, defect, where)
    gb, rb = rm.flat(got)[0], rm.flat(ref)[0]
    und = rm.undecided(ref, q)[0]
    # (a symbol clock moved by a sample may bring one bit more or less into the stream's last call: the existing tests allow the counts 2-3)
    n = min(gb.size, rb.size)
    assert abs(gb.size - rb.size) <= 1 and np.array_equal(gb[:n][~und[:n]], rb[:n][~und[:n]]), "the defect shows in the bits already"
    with pytest.raises(AssertionError, match=expect) as e:
        rm.compare(2, got, ref, q)
    print("\n[detector] %s: %s" % (defect, e.value))

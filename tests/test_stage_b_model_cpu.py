"""tests/stage_b_model.py against the oracle, on the CPU: the restatements of links D, P and S equal the oracle's chain taps bit for bit, the
constants the GPU bounds are made of are re-measured from the reference alone, the slip shares lie under their caps, the inputs of the GPU
cases keep the lock metric clear of its threshold, and the compare helpers flag planted errors.  Every figure is printed."""
import numpy as np
import pytest

import stage_b_model as sb

N_IN = 16384 * 110              # 0.78 s: the default programme locks at fm sample 104276, 45910 stereo samples follow


def chain_taps(ol, siggen=None, n=N_IN, **cfg):
    taps = (ol.TAP_FM_IQ, ol.TAP_DEMOD, ol.TAP_LRRAW, ol.TAP_PILOT, ol.TAP_PSS)
    ch = ol.OracleChain(taps=taps, tap_seconds=1.0, **cfg)
    ch.process(ol.synth_iq(n, **(siggen or {})))
    out = dict(zip(("z", "demod", "lr", "phase", "pdp"), (ch.tap(t).copy() for t in taps)))
    ch.close()
    return out


@pytest.fixture(scope="module")
def dflt(ol):
    """The default programme through the oracle's chain, PSS off."""
    return chain_taps(ol, pssActive=0)


@pytest.fixture(scope="module")
def dflt_pilot(dflt):
    return sb.pilot_oracle(dflt["demod"])


@pytest.fixture(scope="module")
def mistuned(ol):
    return chain_taps(ol, dict(offsetHz=20000.0), pssActive=0)


def record_holds(measured, record, what):
    """The recorded figure is the measured one to within a quarter: another libm or compiler moves the last bits of a measurement, not a quarter."""
    print("[reference alone] %s: measured %.3e, recorded %.3e" % (what, measured, record))
    assert record / 1.25 <= measured <= 1.25 * record, (what, measured, record)


# ------------------------------------------------------------------------------------------------ restatements
def test_link_d_restatement_is_the_oracle(dflt):
    """fmo_demod_run over the chain's own TAP_FM_IQ and the numpy restatement of the Mixed decoder (limiter, compAtan, f32 AFC walk) both
    equal the chain's TAP_DEMOD bit for bit, with TAP_OFFSET's alignment: DEMOD [j] answers FM_IQ [j]."""
    assert sb.TAP_OFFSET["demod"] == sb.TAP_OFFSET["fm_iq"] == 0
    assert dflt["demod"].shape[0] == N_IN // 12
    sb.check_identical("D", "oracle", sb.demod_oracle(dflt["z"]), dflt["demod"])
    sb.check_identical("D", "numpy", sb.demod_mixed_numpy(dflt["z"]), dflt["demod"])


def test_link_p_restatement_is_the_oracle(dflt, dflt_pilot):
    """fmo_pilot_run on 5 DEMOD equals the chain's TAP_PILOT; the numpy-f32 loop equals fmo_pilot_run in phase, lock and metric, bit for
    bit.  The default programme: the metric first exceeds 0.07 at sample 8226, the channel locks at 104276."""
    ph, lk, st = dflt_pilot
    sb.check_identical("P", "oracle", ph, dflt["phase"])
    p5 = (np.float32(5.0) * dflt["demod"]).astype(np.float32)
    ph2, lk2, st2 = sb.pilot_numpy(p5)
    sb.check_identical("P", "numpy phase", ph2, ph)
    sb.check_identical("P", "numpy metric", st2, st)
    assert np.array_equal(lk2, lk)
    assert int(np.argmax(st > sb.LOCK_THRESHOLD)) == 8226 and int(np.argmax(lk)) == 104276


@pytest.mark.parametrize("selector", [0, 6])
def test_link_s_restatement_is_the_oracle(ol, dflt, dflt_pilot, selector):
    """PSS off: LR_RAW.re is DEMOD, LR_RAW.im the memoryless expression of lr_diff -- both f32 roundings of the fmod, the index
    (int)((double) ph Rate / 2 pi), (float)(2.0 lut demod) -- bit for bit on the oracle's chain, cosine arm and sine arm (selector 6)."""
    t = dflt if selector == 0 else chain_taps(ol, pssActive=0, soundSelector=6)
    ph, lk, _ = sb.pilot_oracle(t["demod"])
    assert lk.sum() == 45910 and np.array_equal(t["lr"][:, 0], t["demod"])
    sb.check_identical("S", "numpy, selector %d" % selector, sb.lr_diff(t["demod"], ph, lk, selector=selector), t["lr"][:, 1])
    assert np.count_nonzero(t["lr"][:, 1]) > 45000 and not t["lr"][:104276, 1].any()


def test_link_s_closed_loop_is_the_oracle(ol):
    """PSS on: fmo_pss_* driven in closed loop with the chain's DEMOD, phase and lock reproduces the chain's pilotDelayPSS and LR_RAW.im."""
    t = chain_taps(ol, pssActive=1)
    ph, lk, _ = sb.pilot_oracle(t["demod"])
    loop = sb.PssLoop()
    diff, used, after = loop.run(t["demod"], ph, lk)
    loop.close()
    sb.check_identical("S", "closed loop, pilotDelayPSS", after, t["pdp"])
    sb.check_identical("S", "closed loop, LR_RAW.im", diff, t["lr"][:, 1])
    assert np.abs(after).max() > 1e-4                      # (the accumulator moves: the case is not the PSS-off one)


# ------------------------------------------------------------------------------------------------ the constants
def test_link_d_constants(dflt, mistuned):
    """REF_D_AFC64 and REF_D_AFC64_MISTUNED: the oracle's DEMOD against afc_scale_f64 on the same discriminator output, of the peak."""
    for t, record, what in ((dflt, sb.REF_D_AFC64, "default programme"), (mistuned, sb.REF_D_AFC64_MISTUNED, "carrier 20 kHz off tune")):
        ref = sb.afc_scale_f64(sb.discriminator_mixed(t["z"]))
        w = sb.compare("D", what, t["demod"], ref, scale=sb.demod_peak(t["demod"]))
        print(w)
        record_holds(w.rel, record, "link D, " + what)
    assert sb.D_BATCH_BOUND == 2.0 * sb.REF_D_AFC64 and sb.D_MISTUNED_BOUND == 2.0 * sb.REF_D_AFC64_MISTUNED


def test_link_p_constant(dflt, dflt_pilot):
    """REF_P_SINE_FREEDOM: the reference's loop with its sine table moved by up to 1.2e-7 per entry -- three random tables and one with
    every entry moved away from zero --, the worst wrapped phase difference to the reference's own trajectory; no lock decision moves."""
    ph, lk, st = dflt_pilot
    p5 = (np.float32(5.0) * dflt["demod"]).astype(np.float32)
    worst = 0.0
    for seed in (1, 2, 3, None):
        ph2, lk2, st2 = sb.pilot_numpy(p5, sb.perturbed_sines(seed))
        d = float(sb.wrapped(ph2, ph).max())
        print("[reference alone] link P, sine table %s: worst %.3e rad, metric moved by %.2e" % (
            "biased" if seed is None else "seed %d" % seed, d, float(np.abs(st2.astype(np.float64) - st).max())))
        assert np.array_equal(lk2, lk)
        worst = max(worst, d)
    record_holds(worst, sb.REF_P_SINE_FREEDOM, "link P, sine freedom")
    assert sb.P_SEQ_BOUND == 2.0 * sb.REF_P_SINE_FREEDOM


def test_link_e_constant(dflt):
    """REF_E_DEEMPH: the reference's f32 de-emphasis recurrence against float64 on the same f32 matrix output (selector 0), of the peak."""
    x = sb.matrix_f32(dflt["lr"])
    ref = sb.one_pole_f64(x, sb.deemph_alpha(50))
    w = sb.compare("E", "reference", sb.one_pole_f32(x, sb.deemph_alpha(50)), ref)
    print(w)
    record_holds(w.rel, sb.REF_E_DEEMPH, "link E, de-emphasis")
    assert sb.E_BOUND == 2.0 * sb.REF_E_DEEMPH
    assert float(sb.deemph_alpha(50)) == pytest.approx(1.0 / (192000 / 20000.0 + 1.0), rel=1e-7)


# ------------------------------------------------------------------------------------------------ slip shares
def test_link_d_slip_share_of_the_reference(dflt):
    """The reference with its input moved by 6e-8 relative (an ulp here and there, what a one-ulp limiter does): a table index moves in
    0.03 ... 0.04 % of the samples, by at most one table step (3.9e-5 of the peak); every other sample stays within D_BATCH_BOUND."""
    rng = np.random.default_rng(5)
    z = dflt["z"]
    z2 = (z.astype(np.float64) * (1.0 + 6e-8 * rng.uniform(-1.0, 1.0, z.shape))).astype(np.float32)
    assert 0.2 < float((z2 != z).mean()) < 0.8
    ref = dflt["demod"].astype(np.float64)
    e = np.abs(sb.demod_oracle(z2).astype(np.float64) - ref)
    peak = sb.demod_peak(ref)
    slip = e > sb.D_BATCH_BOUND * peak
    share, step = float(slip.mean()), sb.tables().table_step(3)
    print("[reference alone] link D slips: %.4f %% of the samples, the largest %.3e of the peak (one step %.3e); the others within %.3e"
          % (100 * share, float(e[slip].max()) / peak, step / peak, float(e[~slip].max()) / peak))
    assert 0 < share <= sb.D_SLIP_SHARE_REF < sb.D_SLIP_SHARE
    assert float(e[slip].max()) <= step


def test_link_s_slip_share_of_the_reference():
    """PSS on, the accumulator not tapped: the reference's own table index with its accumulator moved by up to 1e-6 rad (uniformly, either
    way) slips in about 1.5 % of the samples, by up to 1e-7 rad in 0.2 % (uniform phases); the cap of the GPU test is PSS_SLIP_SHARE = 2 %."""
    rng = np.random.default_rng(9)
    cur = rng.uniform(0.0, sb.TWO_PI, 1 << 20).astype(np.float32)
    pdp = rng.uniform(-0.05, 0.05, cur.shape[0]).astype(np.float32)
    base = sb.mix_index(sb.mix_phase(cur, pdp))
    for move, cap in ((1e-6, sb.PSS_SLIP_SHARE), (1e-7, 0.004)):
        idx = sb.mix_index(sb.mix_phase(cur, (pdp.astype(np.float64) + rng.uniform(-move, move, cur.shape[0])).astype(np.float32)))
        d = (idx - base) % sb.FM_RATE
        share = float((d != 0).mean())
        print("[reference alone] link S slips, accumulator moved by %.0e rad: %.3f %% of the samples" % (move, 100 * share))
        assert 0 < share <= cap and np.isin(d, (0, 1, sb.FM_RATE - 1)).all()


def test_unrounded_index_differs_from_the_reference_above_one_turn():
    """The index formed from fract ((double) p / 2 pi) 192000, without the f32 rounding of fmod (p, 2 pi): over phases uniform in
    (pi / 2, 4 pi + pi / 2) it differs from the reference's by one entry in 0.14 % of the samples -- none below 2 pi, 0.28 % in [2 pi, 4 pi)."""
    rng = np.random.default_rng(3)
    p = rng.uniform(np.pi / 2, 4 * np.pi + np.pi / 2, 1 << 22)
    cur = ((p - np.pi / 2) / 2).astype(np.float32)               # (2 (cur + pi / 4) = p; cur beyond 2 pi does not occur in the chain, the expression takes it)
    zero = np.zeros(cur.shape[0], np.float32)
    ph = (2.0 * (cur.astype(np.float64) + np.pi / 4)).astype(np.float32)
    d = (sb.mix_index_unrounded(cur, zero) - sb.mix_index(sb.mix_phase(cur, zero))) % sb.FM_RATE
    assert np.isin(d, (0, 1, sb.FM_RATE - 1)).all()
    low, mid = ph < np.float32(sb.TWO_PI), (ph >= np.float32(sb.TWO_PI)) & (ph < np.float32(2 * sb.TWO_PI))
    print("[restated] unrounded index: %.3f %% of all, %.3f %% in [2 pi, 4 pi), %d below 2 pi"
          % (100 * float((d != 0).mean()), 100 * float((d[mid] != 0).mean()), int((d[low] != 0).sum())))
    assert not (d[low] != 0).any() and 0.002 < float((d[mid] != 0).mean()) < 0.004


# ------------------------------------------------------------------------------------------------ the GPU cases' inputs
@pytest.mark.parametrize("name", ["default", "tones", "mistuned"])
def test_gpu_inputs_keep_the_lock_metric_clear_of_its_threshold(ol, name):
    """Every crossing of 0.07 keeps LOCK_MARGIN on both sides (a 1.2e-7 sine moves the metric by 5e-7), and the channel locks with more than
    40 000 stereo samples left in 0.78 s.  The generator's own pilot level of 0.10 does not qualify: 3.0e-6 at sample 8226."""
    t = chain_taps(ol, sb.PROGRAMMES[name], pssActive=0)
    ph, lk, st = sb.pilot_oracle(t["demod"])
    cross, _ = sb.lock_crossings(st)
    sides = np.abs(np.concatenate([st[cross - 1], st[cross]]).astype(np.float64) - float(sb.LOCK_THRESHOLD))
    print("[%s] %d crossings, the nearest side %.3e from 0.07, locked from sample %d" % (name, cross.size, float(sides.min()), int(np.argmax(lk))))
    assert cross.size > 0 and float(sides.min()) >= sb.LOCK_MARGIN
    assert lk.any() and lk.sum() > 40000


def test_decoders_input_keeps_every_decoder_clear_of_the_threshold(ol):
    """The decoders' case runs four decoders on one stream: each has a DEMOD and a lock metric of its own, all four keep LOCK_MARGIN."""
    t = chain_taps(ol, sb.PROGRAMMES["decoders"], pssActive=0)
    locks = []
    for dec in (3, 4, 5, 6):
        _, lk, st = sb.pilot_oracle(sb.demod_oracle(t["z"], dec))
        cross, _ = sb.lock_crossings(st)
        sides = np.abs(np.concatenate([st[cross - 1], st[cross]]).astype(np.float64) - float(sb.LOCK_THRESHOLD))
        print("[decoder %d] %d crossings, the nearest side %.3e from 0.07, locked from sample %d" % (dec, cross.size, float(sides.min()), int(np.argmax(lk))))
        assert cross.size > 0 and float(sides.min()) >= sb.LOCK_MARGIN and lk.sum() > 40000
        locks.append(int(np.argmax(lk)))
    assert locks == [103791, 103791, 106969, 101444]


def test_noise_input_never_locks(ol):
    t = chain_taps(ol, sb.PROGRAMMES["noise"], pssActive=0)
    _, lk, st = sb.pilot_oracle(t["demod"])
    assert not lk.any() and not t["lr"][:, 1].any() and sb.demod_peak(t["demod"]) > 0.5
    print("[noise] lock metric at most %.3e" % float(st.max()))


# ------------------------------------------------------------------------------------------------ planted errors
def test_compare_helpers_flag_planted_errors(dflt, dflt_pilot):
    """A single sample off by 1e-5 of the peak (links D exact, S and E), one segment's de-emphasis state dropped, one cosine entry shifted,
    the unrounded index: every one is flagged, and the report names the sample's call, segment and thread."""
    ph, lk, _ = dflt_pilot
    demod, lr = dflt["demod"], dflt["lr"]
    starts = np.cumsum([0] + sb.RAGGED * 2)[:-1] // 12
    j = 110000
    call = int(np.searchsorted(starts, j, side="right") - 1)
    where = "call %d, segment %d, thread %d" % (call, (j - starts[call]) // sb.SEG, (j - starts[call]) % sb.SEG // sb.PER_THREAD)
    # link D, exact: one sample off by 1e-5 of the peak
    bad = demod.copy()
    bad[j] += np.float32(1e-5 * sb.demod_peak(demod))
    with pytest.raises(AssertionError, match="1 of .* samples differ.*" + where):
        sb.check_identical("D", 0, bad, demod, starts)
    # ... in a batch the same sample counts as a table slip (1e-5 < one step of 3.9e-5): reported, and allowed up to 0.2 %
    _, share, big = sb.check_d_batch(0, bad, demod, 3, starts)
    assert share == pytest.approx(1.0 / demod.shape[0]) and big == pytest.approx(1e-5, rel=0.02)
    # ... one step and a half is not
    bad[j] = demod[j] + np.float32(1.5 * sb.tables().table_step(3))
    with pytest.raises(AssertionError, match="beyond one table step.*" + where):
        sb.check_d_batch(0, bad, demod, 3, starts)
    # link S: the same sample
    ref_im = sb.lr_diff(demod, ph, lk)
    bad = ref_im.copy()
    bad[j] += np.float32(1e-5 * float(np.abs(ref_im).max()))
    with pytest.raises(AssertionError, match="link S: 1 samples.*" + where):
        sb.check_s(0, bad, ref_im, demod, starts)
    sb.check_s(0, ref_im, ref_im, demod, starts)
    # link S: one cosine entry shifted to its neighbour's value (the entry the locked samples use most)
    idx = sb.mix_index(sb.mix_phase(ph[lk], np.zeros(int(lk.sum()), np.float32)))
    k = int(np.bincount(idx).argmax())
    tab = sb.tables().cos.copy()
    tab[k] = tab[(k + 1) % sb.FM_RATE]
    with pytest.raises(AssertionError, match="link S: .* beyond the bound"):
        sb.check_s(0, sb.lr_diff(demod, ph, lk, cos_table=tab), ref_im, demod, starts)
    # link S: the index without the f32 rounding of the fmod
    with pytest.raises(AssertionError, match="link S: .* beyond the bound"):
        sb.check_s(0, sb.lr_diff(demod, ph, lk, unrounded=True), ref_im, demod, starts)
    # link E: one sample off by 1e-5 of the peak; the state dropped in front of one segment
    ref = sb.link_e(lr)
    good = sb.one_pole_f32(sb.matrix_f32(lr), sb.deemph_alpha(50))
    sb.check(sb.compare("E", 0, good, ref, starts), sb.E_BOUND)
    bad = good.copy()
    bad[j, 1] += np.float32(1e-5 * float(np.abs(ref).max()))
    with pytest.raises(AssertionError, match="exceeds the bound.*link E.*" + where):
        sb.check(sb.compare("E", 0, bad, ref, starts), sb.E_BOUND)
    seg_start = int(starts[call]) + ((j - int(starts[call])) // sb.SEG) * sb.SEG
    with pytest.raises(AssertionError, match="exceeds the bound.*link E.*call %d, segment %d, thread 0" % (call, (j - starts[call]) // sb.SEG)):
        sb.check(sb.compare("E", 0, sb.link_e(lr, drop_state_at=seg_start), ref, starts), sb.E_BOUND)
    # link P: a phase one table step off in one sample, across the wrap
    badp = ph.copy()
    badp[j] = np.float32((float(ph[j]) + sb.TABLE_STEP) % sb.TWO_PI)
    with pytest.raises(AssertionError, match="exceeds the bound.*link P.*" + where):
        sb.check(sb.compare("P", 0, badp, ph, starts, scale=1.0, circular=True), sb.P_SEQ_BOUND)

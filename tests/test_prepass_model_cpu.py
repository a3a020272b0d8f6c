"""tests/prepass_model.py on the CPU: the model of the demodulator pre-pass equals an oracle chain bit for bit (where FMX_TAP_DEMOD sits; the order
of carrier update, squelch and snapshot; a slider, a decoder and a squelch mode changed in mid-stream), the call lists contain what the GPU test
relies on, every squelch decision of every input keeps its margin, decoder 2's bound is re-measured from the reference alone, and the comparators
catch and locate seeded defects.  No GPU and nothing of libfmx."""
import numpy as np
import pytest

import oracle_lib as ol
import prepass_model as pm
import stage_b_model as sb

BLOCK = 16384            # the reference consumes whole blocks of input samples (fm-processor.cpp:387-417)
STARTS = pm.call_starts(pm.CALLS_FM)


def chain_run(programme, cuts=(), **cfg):
    """An oracle chain over a programme with its FM_IQ and DEMOD taps.  cuts: (block, settings) -- reconfigured in front of that input block.
    -> (z, demod, meta, the fm sample each cut took effect at)."""
    iq = pm.programme_iq(programme)
    ch = ol.OracleChain(inputFilterBw=165000, taps=(ol.TAP_FM_IQ, ol.TAP_DEMOD), **cfg)
    pos, at = 0, []
    for block, kw in cuts:
        ch.process(iq[pos:block * BLOCK])
        pos = block * BLOCK
        at.append(ch.tap(ol.TAP_FM_IQ).shape[0])
        ch.configure(**kw)
    ch.process(iq[pos:])
    z, d, meta = ch.tap(ol.TAP_FM_IQ).copy(), ch.tap(ol.TAP_DEMOD).copy(), ch.meta()
    ch.close()
    return z, d, meta, at


@pytest.fixture(scope="module")
def streams():
    return {p: chain_run(p)[0] for p in pm.PROGRAMMES}


# ------------------------------------------------------------------------------------------------ the call list
def test_call_lists_contain_what_the_gpu_test_relies_on():
    lines = pm.coverage()
    print("\n" + "\n".join(lines))
    assert all(n % 12 == 0 for n in pm.CALLS + pm.CALLS_B) and sum(pm.CALLS) == sum(pm.CALLS_B) == 12 * pm.N_FM
    assert 100000 <= pm.N_FM <= 101000 and int(STARTS[pm.SLIDER_CALL]) == 4 * pm.HOLD
    # ... and the proof notices what it is there for: a list without the six-sample call, one whose snapshot call is ragged, one without a short call
    i = pm.CALLS_FM.index(6)
    merged = pm.CALLS_FM[:i - 1] + [pm.CALLS_FM[i - 1] + 6] + pm.CALLS_FM[i + 1:] + [0]
    for bad in (merged, pm.CALLS_FM[:-2] + [12, pm.CALLS_FM[-1] + 68], [3 if n == 2 else n for n in pm.CALLS_FM[:-1]] + [pm.CALLS_FM[-1] - 1]):
        with pytest.raises(AssertionError):
            pm.coverage(bad, pm.CALLS_FM_B if len(bad) == len(pm.CALLS_FM_B) else bad)


def test_handle_populations_reach_every_arm_of_the_switch():
    hs = pm.handles()
    assert sorted(len(h[0]) for h in hs.values()) == [1, 1, 3, 3, 64, 65, 70, 130]
    for name, (kinds, prog, probe, twins, batch, arm) in hs.items():
        assert pm.prepass_arm(kinds) == arm, (name, pm.prepass_arm(kinds), arm)
        assert batch == (len(kinds) > 64) and all(kinds[c] is not None for c in probe)
        for a, b in twins:
            assert kinds[a] == kinds[b] and prog[a] == prog[b]
    assert {h[5] for h in hs.values()} == pm.ARMS
    for n in ("64 all", "70 all"):
        assert set(hs[n][0]) == set(pm.KINDS) and {hs[n][0][c] for c in hs[n][2]} == set(pm.KINDS)
    k130 = hs["130 sparse"][0]
    assert k130[129] == "mixed+nsq" and 129 % 3 == 0 and 129 // 64 == 2          # alone in its triple, in the last afc wave (two lanes)
    assert hs["65 sparse"][0][64] == "am+lsq"


# ------------------------------------------------------------------------------------------------ the model is the chain
@pytest.mark.parametrize("kind", list(pm.KINDS))
def test_model_equals_the_oracle_chain(kind):
    """FM_IQ -> DEMOD of a chain, DEMOD tapped behind the squelch; the chain's metaData: dcValIf is the model's fm_afc behind fm sample 96000,
    squelchActive its flag behind the last sample.  The slider kinds: the chain applies a new value at the next block's start."""
    kd = pm.KINDS[kind]
    cfg = dict(decoder=kd["decoder"], squelchMode=kd.get("squelch_mode", 0), squelchValue=kd.get("squelch_value", 0))
    for programme in ("fade", "silence") if kind in ("am", "pll", "mixed+nsq") else ("fade",):
        cuts = [(30, dict(squelchValue=kd["slider"]))] if "slider" in kd else []
        z, d, meta, at = chain_run(programme, cuts, **cfg)
        ev = [(at[0], "squelch_value", kd["slider"])] if cuts else []
        m = pm.model(z, kd["decoder"], kd.get("squelch_mode", 0), kd.get("squelch_value"), ev)
        pm.check_identical(kind, programme, m["demod"], d, STARTS)
        assert z.shape[0] > pm.SNAP + 2 * pm.TILE
        assert np.float32(meta.dcValIf).view(np.uint32) == m["afc"][pm.SNAP].view(np.uint32)
        if kd.get("squelch_mode", 0):
            assert meta.squelchActive == int(m["flag"][-1])
            assert m["decisions"] and [s for s, *_ in m["decisions"]] == list(range(pm.HOLD - 1, z.shape[0], pm.HOLD))


@pytest.mark.parametrize("case", ["3 1 3", "3 2 3 2", "level squelch", "noise squelch"])
def test_model_equals_the_oracle_chain_across_switches(case):
    """A decoder or a squelch mode changed in mid-stream, on one long-lived demodulator and squelch: the carrier level runs whatever the decoder
    (the AM decoder starts settled), pllC rests while off, Imin1 / Qmin1 keep their pre-AM values over an AM stretch, a squelch that is off keeps its
    count, averages and memories."""
    steps = {"3 1 3": [("decoder", 1), ("decoder", 3)], "3 2 3 2": [("decoder", 2), ("decoder", 3), ("decoder", 2)],
             "level squelch": [("squelchMode", 2), ("squelchMode", 0), ("squelchMode", 2)], "noise squelch": [("squelchMode", 1), ("squelchMode", 0), ("squelchMode", 1)]}[case]
    blocks = [22, 40, 58][:len(steps)]
    value = {"level squelch": pm.LSQ_VALUE, "noise squelch": pm.NSQ_VALUE}.get(case, 0)
    programme = "fade" if value else "stereo"
    z, d, meta, at = chain_run(programme, [(b, {k: v}) for b, (k, v) in zip(blocks, steps)], decoder=3, squelchValue=value)
    names = dict(decoder="decoder", squelchMode="squelch_mode")
    m = pm.model(z, 3, 0, value or None, [(a, names[k], v) for a, (k, v) in zip(at, steps)])
    pm.check_identical(case, programme, m["demod"], d, STARTS)
    assert at[0] >= 20000
    if case == "3 1 3":       # the AM decoder finds the carrier level settled
        assert float(m["carrier"][at[0]]) > 1.0 and abs(float(m["demod"][at[0]])) < 0.5


# ------------------------------------------------------------------------------------------------ inputs and margins
def test_every_decision_keeps_its_margin(streams):
    """Every kind on every programme: the deciding quantity stays LSQ_MARGIN / NSQ_MARGIN from its threshold at every decision; on the fading
    carrier each squelch closes and opens at least twice; the silent start reaches the limiter's 0.001 branch."""
    for p, z in streams.items():
        for kind, kd in pm.KINDS.items():
            if not kd.get("squelch_mode", 0):
                continue
            m = pm.kind_model(z, kind, STARTS)
            n = pm.check_margins(m, "%s on %s" % (kind, p), sb.demod_peak(m["raw"]) if kd["decoder"] == 2 else None)
            flags = [d[5] for d in m["decisions"]]
            print("[%s on %s] %d decisions, flags %s, the smallest margin %.3e" % (kind, p, n, flags, min(d[4] for d in m["decisions"])))
            assert n == 10
            if p == "fade":
                change = np.diff(np.array([0] + flags))
                assert (change > 0).sum() >= 2 and (change < 0).sum() >= 2, (kind, flags)
    a = np.hypot(streams["silence"][:, 0].astype(np.float64), streams["silence"][:, 1])
    assert (a[:pm.SILENCE // 12 - 64] <= 0.001).all() and (a[-50000:] > 0.1).all()
    with pytest.raises(AssertionError, match="choose another input"):        # the assertion notices a decision that sits on its threshold
        m = pm.kind_model(streams["fade"], "mixed+lsq", STARTS)
        s, mode, qty, thr, _, fl = m["decisions"][3]
        m["decisions"][3] = (s, mode, thr + 1e-4, thr, 1e-4, fl)
        pm.check_margins(m, "seeded")


# ------------------------------------------------------------------------------------------------ decoder 2's bound
def moved_tables():
    T = sb.tables()
    out = []
    for seed in (1, 2, 3, None):
        if seed is None:
            c, s = (T.cos.astype(np.float64) + pm.HW_SINE * np.sign(T.cos)).astype(np.float32), sb.perturbed_sines(None)
        else:
            rng = np.random.default_rng(seed)
            c = (T.cos.astype(np.float64) + pm.HW_SINE * rng.uniform(-1, 1, T.cos.shape[0])).astype(np.float32)
            s = (T.sin.astype(np.float64) + pm.HW_SINE * rng.uniform(-1, 1, T.cos.shape[0])).astype(np.float32)
        assert np.abs(c.astype(np.float64) - T.cos).max() <= pm.HW_SINE + 6e-8 and np.abs(s.astype(np.float64) - T.sin).max() <= pm.HW_SINE + 6e-8
        out.append(np.stack([c, s], axis=1))
    return out


def test_pll_bound_from_the_reference_alone(streams):
    """The reference's decoder 2 with its SinCos table moved by up to 1.2e-7 per entry (the test hook fmo_demod_test_set_sincos) against the
    unmoved reference: worst sample of four tables and three programmes, of the DEMOD peak.  The hook with the unmoved table changes nothing."""
    T = sb.tables()
    worst, afc_worst, shares = 0.0, 0.0, []
    for p, z in streams.items():            # the AM decoder: DEMOD does not pass through pllC, its AFC does
        ref = pm.model(z, 1)
        for tab in moved_tables():
            m = pm.model(z, 1, sincos=tab)
            pm.check_identical("am, moved table", p, m["demod"], ref["demod"], STARTS)
            afc_worst = max(afc_worst, float(np.abs(m["afc"].astype(np.float64) - ref["afc"]).max()))
    print("the AM decoder's fm_afc under the moved tables: within %.3e" % afc_worst)
    for p, z in streams.items():
        ref = pm.model(z, 2)
        same = pm.model(z, 2, sincos=np.stack([T.cos, T.sin], axis=1))
        pm.check_identical("pll, hook with the reference's table", p, same["demod"], ref["demod"], STARTS)
        peak = sb.demod_peak(ref["raw"])
        for k, tab in enumerate(moved_tables()):
            m = pm.model(z, 2, sincos=tab)
            e = np.abs(m["raw"].astype(np.float64) - ref["raw"]) / peak
            shares.append(float((e > 0).mean()))
            print("[%s, table %d] worst sample %.3e of the peak %.4g at fm sample %d; %.1f %% of the samples differ; fm_afc within %.2e"
                  % (p, k, e.max(), peak, int(np.argmax(e)), 100 * shares[-1], np.abs(m["afc"].astype(np.float64) - ref["afc"]).max()))
            worst, afc_worst = max(worst, float(e.max())), max(afc_worst, float(np.abs(m["afc"].astype(np.float64) - ref["afc"]).max()))
    print("REF_PLL_WORST re-measured %.3e (record %.3e), fm_afc %.2e (record %.2e)" % (worst, pm.REF_PLL_WORST, afc_worst, pm.REF_PLL_AFC))
    assert 0.75 * pm.REF_PLL_WORST <= worst <= 1.25 * pm.REF_PLL_WORST
    assert 0.75 * pm.REF_PLL_AFC <= afc_worst <= 1.25 * pm.REF_PLL_AFC
    assert pm.PLL_BOUND == 2.0 * pm.REF_PLL_WORST and pm.PLL_AFC_BOUND == 2.0 * pm.REF_PLL_AFC
    assert min(shares) > 0.05           # not isolated slips: link D's share rule (at most 0.2 %) does not describe this loop


# ------------------------------------------------------------------------------------------------ the detector
def test_comparators_catch_and_locate_seeded_defects(streams):
    z = streams["fade"]
    m = pm.kind_model(z, "mixed+lsq", STARTS)
    dem, raw = m["demod"], m["raw"]
    assert m["flag"][28798] == 0 and m["flag"][28799] == 1 and raw[28799] != 0

    def caught(where, fn, *a):
        with pytest.raises(AssertionError) as e:
            fn(*a)
        assert where in str(e.value), (where, str(e.value)[:400])

    pm.check_identical("mixed+lsq", 0, dem, dem.copy(), STARTS)
    pm.check_flags("mixed+lsq", 0, dem, m, STARTS)
    # one sample one ulp off
    g = dem.copy(); g[50000] = np.nextafter(g[50000], np.float32(4))
    caught(pm.locate(50000, STARTS), pm.check_identical, "mixed+lsq", 0, g, dem, STARTS)
    # a squelch decision one sample late: the decision's own sample is not muted
    g = dem.copy(); g[28799] = raw[28799]
    caught("call 18, tile 450, row 2", pm.check_flags, "mixed+lsq", 0, g, m, STARTS)
    caught("call 18, tile 450, row 2", pm.check_identical, "mixed+lsq", 0, g, dem, STARTS)
    # ... and one sample early
    g = dem.copy(); g[28798] = 0
    caught("call 18, tile 450, row 1", pm.check_flags, "mixed+lsq", 0, g, m, STARTS)
    # the last nine samples of a call left unmuted (call 18 ends behind fm sample 28810, the squelch closed)
    g = dem.copy(); g[28811 - 9:28811] = raw[28811 - 9:28811]
    caught("call 18, tile 450, row 5", pm.check_flags, "mixed+lsq", 0, g, m, STARTS)
    # the snapshot's AFC value one sample late
    assert m["afc"][pm.SNAP + 1] != m["afc"][pm.SNAP]
    pm.check_snapshot("mixed+lsq", 0, m["afc"][pm.SNAP], m, True)
    caught("dcValIf", pm.check_snapshot, "mixed+lsq", 0, m["afc"][pm.SNAP + 1], m, True)
    # a call's first tile repeated (call 17 starts at fm sample 13593)
    s = int(STARTS[17]); g = dem.copy(); g[s + 16:s + 32] = dem[s:s + 16]
    caught("call 17, tile 1, row 0", pm.check_identical, "mixed+lsq", 0, g, dem, STARTS)
    # the carrier level started from 0 at a switch to the AM decoder (call 20 starts at fm sample 38400): what a fresh demodulator gives from there
    zs = streams["stereo"]; s = int(STARTS[20])
    sw = pm.model(zs, 3, events=[(s, "decoder", 1)])
    fresh = pm.model(zs[s:], 1)
    g = sw["demod"].copy(); g[s:] = fresh["demod"]
    caught("call 20, tile 0, row 0", pm.check_identical, "3 -> 1", 0, g, sw["demod"], STARTS)
    n_off = int(pm.differences(g, sw["demod"]).size)
    print("carrier level from 0 at the switch: %d samples differ, the first %d all at the +1 clamp: %s" % (n_off, 16, bool((g[s:s + 16] == 1.0).all())))
    assert n_off > 2000 and (g[s:s + 16] == 1.0).all() and abs(float(sw["demod"][s])) < 0.5
    # decoder 2: a sample beyond the bound
    p = pm.model(zs, 2)
    g = p["demod"].copy(); g[70000] += np.float32(2.5 * pm.PLL_BOUND * sb.demod_peak(p["demod"]))
    pm.check_pll("pll", 0, p["demod"], p["demod"], STARTS)
    caught(pm.locate(70000, STARTS), pm.check_pll, "pll", 0, g, p["demod"], STARTS)

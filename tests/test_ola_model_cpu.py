"""The block-machine models of tests/ola_model.py on the CPU: against the existing LTI models where nothing restarts, against the oracle's own
fmo_fftfilter and OracleChain across restarts -- the figures the GPU bounds of tests/test_gpu_block_machines_per_sample.py are the doubles of --,
the promotion's inverted de-emphasis measured, the detector against seeded defects, and what the GPU call lists make the library's host decide.
Every test prints what it measures."""
import ctypes as C

import numpy as np
import pytest

import f64_models as fm
import ola_model as om
import stage_a_model as sa
import stage_b_model as sb

ECHO = 0.01         # added to the last tap of both machines' kernels where a seeded defect sits in the tail's last entry (ola_model.with_echo)
SMEAR = 48          # input samples: an error at input sample s reaches the fm samples whose newest input is s ... s + 47 (25 taps, 3 taps at a sixth of the rate, 12 per output)


def record_holds(measured, record, what):
    """test_f64_models_cpu's rule: the recorded figure is not below the measured one and not more than a quarter above it."""
    print("[reference alone] %s: measured %.3e of the peak, recorded %.3e" % (what, measured, record))
    assert measured <= record <= 1.25 * measured, (what, measured, record)


def rel_worst(got, ref):
    g, r = np.asarray(got, np.complex128), np.asarray(ref, np.complex128)
    e = np.maximum(np.abs(g.real - r.real), np.abs(g.imag - r.imag))
    peak = float(max(np.abs(r.real).max(), np.abs(r.imag).max()))
    i = int(np.argmax(e))
    return float(e[i]) / peak, i, peak


# ------------------------------------------------------------------------------------------------ 1. no events: the LTI models
def test_without_events_the_models_are_the_lti_ones(ol):
    """No setter: the input side is stage_a (form "front") and the audio side a convolution delayed by 7436, to float64 rounding."""
    L = ol.oracle()
    calls = om.RAGGED
    n = sum(calls)
    iq = ol.synth_iq(n, dcI=0.004, dcQ=-0.003)
    kw = dict(lo=2500, att=(0.9, 1.1))
    D = sa.Design(L, om.RATE, om.BW0)
    side = om.InputSide(L, iq, calls, [(0, om.BW0)], **kw)
    ref = sa.stage_a(D, iq, calls, **kw)
    r, i, peak = rel_worst(side.z, ref)
    print("\n[no events, input side against stage_a] worst %.2e of the peak %.3g at fm sample %d" % (r, peak, i))
    assert side.z.shape == ref.shape and r <= 1e-13
    assert side.machine.block == n // om.IN_L and side.where(0) == (True, 0, 11)
    rng = np.random.default_rng(3)
    lr = (0.2 * rng.standard_normal((30000, 2))).astype(np.float32)
    au = om.AudioSide(L, lr, [(0, om.LF0)])
    x = sb.matrix_f32(lr).astype(np.float64)
    lti = sb.one_pole_f64(fm.delayed(fm.fftconv(x, om.audio_kernel(L, om.LF0)), om.AU_L, x.shape[0]), sb.deemph_alpha(50))
    e = float(np.abs(au.y - lti).max() / np.abs(lti).max())
    print("[no events, audio side against the delayed convolution] worst %.2e of the peak" % e)
    assert e <= 1e-13 and au.where(7436 + 5) == (True, 1, 5)
    off = om.AudioSide(L, lr, [(0, 0)])
    assert np.array_equal(off.filtered, x)                  # (a filter that is off: the samples as they are)


# ------------------------------------------------------------------------------------------------ 2. the oracle's filter against the machine
def schedule(L_):
    """[(position, kernel index | -1 for "Off")] of one filter, in its own samples, and the stream's length: a restart in mid-block with a new
    kernel; the kernel in use again 0.7 blocks later (two restarts less than a block apart); a restart at inp == 0; one at inp == L - 1; "Off"
    in mid-block; on again 1.3 blocks later (stale buffers played)."""
    p1 = int(1.4 * L_)
    p2 = p1 + int(0.7 * L_)
    p3 = p2 + 2 * L_
    p4 = p3 + 2 * L_ - 1
    p5 = p4 + int(1.5 * L_)
    p6 = p5 + int(1.3 * L_)
    return [(0, 0), (p1, 1), (p2, 1), (p3, 2), (p4, 0), (p5, -1), (p6, 1)], p6 + int(2.5 * L_)


@pytest.mark.parametrize("which", ["input", "audio"])
def test_oracle_filter_against_the_machine(ol, which):
    """fmo_fftfilter (f32 FFTs) against BlockMachine (float64, a plain convolution per block) over schedule (): every sample, relative to the stream's
    peak.  Measured: see ola_model.REF_OLA_IN_FILTER / REF_OLA_AU_FILTER."""
    L = ol.oracle()
    if which == "input":
        fft, deg, values, rate = om.IN_FFT, om.IN_TAPS, [165000, 120000, 130000], om.RATE
        kernel, low = (lambda v: om.input_kernel(L, v)), (lambda v: v // 2)
    else:
        fft, deg, values, rate = om.AU_FFT, om.AU_TAPS, [15000, 9000, 12000], om.FM_RATE
        kernel, low = (lambda v: om.audio_kernel(L, v)), (lambda v: v)
    ev, n = schedule(fft - deg)
    if which == "input":
        x = ol.synth_iq(n, offsetHz=20000.0)
    else:
        t = np.arange(n) / om.FM_RATE
        rng = np.random.default_rng(5)
        x = np.stack([0.4 * np.sin(2 * np.pi * 1000 * t) + 0.1 * np.sin(2 * np.pi * 19000 * t), 0.3 * np.sin(2 * np.pi * 400 * t + 1.0)], axis=1)
        x = (x + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
    xc = x[:, 0].astype(np.float64) + 1j * x[:, 1].astype(np.float64)
    # the schedule is what it says it is
    Lb = fft - deg
    inp, on, seen = 0, True, []
    for (p, k), q in zip(ev, [e[0] for e in ev[1:]] + [n]):
        seen.append((on, inp, k))
        on = k >= 0
        inp = (0 if on else inp)
        inp = (inp + (q - p)) % Lb if on else inp
    assert 0 < seen[1][1] < Lb - 1 and seen[2][2] == seen[1][2] and 0 < seen[2][1] < Lb          # mid-block, new kernel; the same again within a block
    assert seen[3][1] == 0 and seen[4][1] == Lb - 1 and 0 < seen[5][1] < Lb - 1 and ev[6][0] - ev[5][0] > Lb
    m = om.BlockMachine(fft, deg)
    ref = om.run_events(m, xc, [(p, values[k] if k >= 0 else 0) for p, k in ev], kernel)
    h = L.fmo_fftfilter_new(fft, deg)
    out = np.zeros((n, 2), np.float32)
    xin = np.ascontiguousarray(x, np.float32)
    fp = C.POINTER(C.c_float)
    for (p, k), q in zip(ev, [e[0] for e in ev[1:]] + [n]):
        if k < 0:
            out[p:q] = xin[p:q]
            continue
        L.fmo_fftfilter_set_lowpass(h, low(values[k]), rate)
        seg_in, seg_out = np.ascontiguousarray(xin[p:q]), np.zeros((q - p, 2), np.float32)
        L.fmo_fftfilter_run_c(h, seg_in.ctypes.data_as(fp), seg_out.ctypes.data_as(fp), q - p)
        out[p:q] = seg_out
    L.fmo_fftfilter_free(h)
    rep = om.judge("oracle filter against the machine, %s" % which, out, ref, [0], lambda i: om.locate(m.marks, i, Lb), 1.0, check=False)
    record_holds(rep.rel, om.REF_OLA_IN_FILTER if which == "input" else om.REF_OLA_AU_FILTER, "the %s filter across restarts" % which)


# ------------------------------------------------------------------------------------------------ 3. the oracle chain with setters in mid-stream
def oracle_effective(at_call):
    """The oracle chain works in the reference's blocks of 16384 input samples and takes a setter over at the next block it begins
    (fm-processor.cpp:387-408): a configure () behind p input samples holds from sample 16384 (p // 16384).  -> {call: input sample}."""
    b = om.boundaries(om.R_CALLS)
    return {k: int(b[k]) // 16384 * 16384 for k in at_call}


@pytest.fixture(scope="module")
def chains(ol):
    """One oracle chain per channel of case r over R_CALLS with that channel's setters: its three taps, and the models on the same events."""
    L = ol.oracle()
    iq = om.r_streams(ol)
    out = []
    for c, kd in enumerate(om.R_KINDS):
        ch = ol.OracleChain(inputFilterBw=om.BW0, lfCutoff=om.LF0, volumeDb=0.0, loFrequency=kd.get("lo", 0), attL=kd.get("att_l", 1.0), attR=kd.get("att_r", 1.0),
                            taps=[ol.TAP_FM_IQ, ol.TAP_LRRAW, ol.TAP_PRE_RS], tap_seconds=1.0)
        pos = 0
        for k, s in enumerate(om.R_CALLS):
            kw = {}
            if k in om.R_BW[c]:
                kw["inputFilterBw"] = om.R_BW[c][k]
            if k in om.R_LF[c]:
                kw["lfCutoff"] = om.R_LF[c][k]
            if kw:
                ch.configure(**kw)
            ch.process(iq[om.R_STREAM[c], pos:pos + s])
            pos += s
        taps = {t: ch.tap(t).copy() for t in (ol.TAP_FM_IQ, ol.TAP_LRRAW, ol.TAP_PRE_RS)}
        ch.close()
        eff_bw, eff_lf = oracle_effective(om.R_BW[c]), oracle_effective(om.R_LF[c])
        ev_in = [(0, om.BW0)] + [(eff_bw[k], v) for k, v in sorted(om.R_BW[c].items())]
        ev_au = [(0, om.LF0)] + [(eff_lf[k] // om.DECIM, v) for k, v in sorted(om.R_LF[c].items())]
        out.append(dict(taps=taps, ev_in=ev_in, ev_au=ev_au, x=iq[om.R_STREAM[c]], kd=kd))
    return out


def test_oracle_chain_against_the_models(ol, chains):
    """OracleChain with configure () in mid-stream over the GPU receiver case's calls, streams, kinds and setters: TAP_FM_IQ against InputSide, TAP_PRE_RS
    (volume 0 dB: the gain behind the de-emphasis is 1) against AudioSide on the oracle's own TAP_LRRAW.  Pins the wiring: "Off" lets the samples
    through undelayed and keeps the state, setters hold from a block start, the de-emphasis stands behind the audio filter."""
    L = ol.oracle()
    worst_in = worst_au = 0.0
    for c, d in enumerate(chains):
        kd = d["kd"]
        z = d["taps"][ol.TAP_FM_IQ]
        side = om.InputSide(L, d["x"], om.R_CALLS, d["ev_in"], lo=kd.get("lo", 0), att=(kd.get("att_l", 1.0), kd.get("att_r", 1.0)))
        n = z.shape[0]
        assert 0 < n <= side.z.shape[0] and side.z.shape[0] - n < 16384 // 12 + 2
        r1 = om.judge("oracle chain, channel %d, FM_IQ" % c, z, side.z[:n], om.call_starts_fm(om.R_CALLS), side.where, 1.0, check=False)
        lr, pre = d["taps"][ol.TAP_LRRAW], d["taps"][ol.TAP_PRE_RS]
        au = om.AudioSide(L, lr, d["ev_au"])
        r2 = om.judge("oracle chain, channel %d, PRE_RS" % c, pre, au.y, om.call_starts_fm(om.R_CALLS), au.where, 1.0, check=False)
        assert r2.scale > 0.05
        worst_in, worst_au = max(worst_in, r1.rel), max(worst_au, r2.rel)
    record_holds(worst_in, om.REF_OLA_IN_CHAIN, "the chain's TAP_FM_IQ across setters")
    record_holds(worst_au, om.REF_OLA_AU_CHAIN, "the chain's TAP_PRE_RS across setters")
    # stage A keeps one bound where the machines' own figures are not larger
    print("[bounds] input side %.3e (stage A's %.3e), audio side %.3e, audio side behind a promotion %.3e" % (om.OLA_IN_BOUND, sa.STAGE_A_BOUND_ON, om.OLA_AU_BOUND, om.OLA_AU_BOUND_PROMOTED))
    assert om.OLA_IN_BOUND >= 2.0 * max(worst_in, om.REF_OLA_IN_FILTER) and om.OLA_AU_BOUND >= 2.0 * worst_au


# ------------------------------------------------------------------------------------------------ 5. the promotion's inverted de-emphasis
def test_inverted_deemphasis_measured(ol, chains):
    """promo_inv_deemph_kernel takes the de-emphasis back out of the d ring in f32, x = (y [n] - y [n - 1]) / a + y [n - 1], which amplifies the
    rounding of the stored y by about 1 / a = 10.4.  Restated in numpy f32 on one_pole_f32 (matrix_f32 (LR_RAW)) of case r's programme (the control
    channel's LR_RAW, mono until the pilot locks and stereo behind it); the float64 audio machine on the reconstruction and on the true stream."""
    L = ol.oracle()
    lr = chains[0]["taps"][ol.TAP_LRRAW]
    x32 = sb.matrix_f32(lr)
    a = sb.deemph_alpha(50)
    rec = om.inverted_deemphasis_f32(sb.one_pole_f32(x32, a), a)
    direct = float(np.abs(rec.astype(np.float64) - x32).max() / np.abs(x32).max())
    true = om.AudioSide(L, lr, [(0, om.LF0)])
    got = om.AudioSide(L, lr, [(0, om.LF0)], x=rec)
    e_f = float(np.abs(got.filtered - true.filtered).max() / np.abs(true.filtered).max())
    e_y = float(np.abs(got.y - true.y).max() / np.abs(true.y).max())
    print("\n[inverted de-emphasis, 1 / a = %.2f] the reconstruction itself %.3e of the peak; the machine's output %.3e; behind the de-emphasis %.3e" % (1.0 / float(a), direct, e_f, e_y))
    record_holds(e_f, om.REF_INV_DEEMPH, "the audio machine on the f32-inverted de-emphasis")


# ------------------------------------------------------------------------------------------------ 6. seeded defects
def region(rep, side, first, last, smear):
    """The reported sample lies in [first, last + smear] of the machine's own numbering; its call, block and position are what plain arithmetic on
    the call list and the setters gives."""
    idx = rep.index * om.DECIM + om.DECIM - 1 if side == "input" else rep.index
    assert first <= idx <= last + smear, (rep.name, idx, first, last)
    b = om.boundaries(om.R_CALLS)
    starts = b[:-1] // om.DECIM
    call = int(np.searchsorted(starts, rep.index, side="right") - 1)
    assert rep.call == call and b[call] // om.DECIM <= rep.index < b[call + 1] // om.DECIM, (rep.name, rep.call, call)


def restart_of(rep, side, events):
    """(block, position) of the reported sample counted from the last setter in front of it, by plain arithmetic."""
    Lb = om.IN_L if side == "input" else om.AU_L
    idx = rep.index * om.DECIM + om.DECIM - 1 if side == "input" else rep.index
    p = max(q for q, _ in events if q <= idx)
    return (idx - p) // Lb, (idx - p) % Lb, p


@pytest.fixture(scope="module")
def seeded(ol, chains):
    """Channel 1's stream with channel 1's widths (a new width in mid-block, the same again) and channel 2's ("Off", on again); channel 0's LR_RAW
    with channel 3's cut-offs: the right models, and a function that runs a wrong one through the GPU test's own comparison."""
    L = ol.oracle()
    x = chains[1]["x"]
    v = om.premix(x, om.R_CALLS)
    lr = chains[0]["taps"][ol.TAP_LRRAW]
    n_fm = lr.shape[0]
    ev = dict(width=om.r_input_events(1), off=om.r_input_events(2), width_late=om.r_input_events(1, True),
              cut=[e for e in om.r_audio_events(3) if e[0] <= n_fm], cut_late=[e for e in om.r_audio_events(3, True) if e[0] <= n_fm])
    good = dict(width=om.InputSide(L, x, om.R_CALLS, ev["width"], v=v), off=om.InputSide(L, x, om.R_CALLS, ev["off"], v=v), cut=om.AudioSide(L, lr, ev["cut"]))

    def run(side, events, defect=None, ref=None, echo=0.0, f32=True, **kw):
        """echo: both machines, right and wrong, on the designs with that much added to the last tap (ola_model.with_echo); f32 False: the wrong
        machine's output as it is, in float64 (a measurement of a defect's own size)."""
        if side == "input":
            bad = om.InputSide(L, x, om.R_CALLS, ev[events], v=v, defect=defect, echo=echo)
            got = np.stack([bad.z.real, bad.z.imag], axis=1)
            g = om.InputSide(L, x, om.R_CALLS, ev[events], v=v, echo=echo) if echo else good[ref or events]
            return om.judge("seeded: %s, input side" % (defect or events), got.astype(np.float32) if f32 else got, g.z, om.call_starts_fm(om.R_CALLS), g.where, om.OLA_IN_BOUND, check=False)
        bad = om.AudioSide(L, lr, ev[events], defect=defect, echo=echo, **kw)
        g = om.AudioSide(L, lr, ev[events], echo=echo) if echo else good[ref or events]
        return om.judge("seeded: %s, audio side" % (defect or events), bad.y.astype(np.float32) if f32 else bad.y, g.y, om.call_starts_fm(om.R_CALLS), g.where, om.OLA_AU_BOUND, check=False)
    return dict(run=run, ev=ev, good=good)


def test_the_right_machine_passes_its_own_comparison(seeded):
    """The models rounded to f32 -- what a perfect kernel would deliver -- stay within the bounds (6e-8 of the peak)."""
    for side, events in (("input", "width"), ("input", "off"), ("audio", "cut")):
        rep = seeded["run"](side, events)
        assert rep.rel <= 0.1 * rep.bound


@pytest.mark.parametrize("side", ["input", "audio"])
@pytest.mark.parametrize("defect", ["clear_overloop", "no_replay", "position_off_by_one", "drop_overloop_entry", "drop_overloop_head", "off_clears_c", "late"])
def test_seeded_defect_is_reported_where_it_is(seeded, side, defect):
    """One wrong machine through the GPU test's own comparison (ola_model.judge with the GPU bounds): reported, and at the call, block and position
    where the defect acts.
      clear_overloop        the old tail is missing in the first block the new kernel completes: block 1 behind the restart, positions 0 ... degree - 2
      no_replay             the kernel is swapped and the block runs on (a folded handle): from the restart until both filters are LTI again, two blocks on
      position_off_by_one   the restart sets inp = 1: the replay is a sample early, A [0] is stale
      drop_overloop_entry   Overloop [degree - 2] = h [degree - 1] A [L - 1], the last entry that is not zero, is lost.  The windowed designs end in taps of
                            2.2e-8 (input filter) / 1.5e-9 (audio filter) against largest taps of 0.072 / 0.156: with them the entry carries 1.1e-8 /
                            4.7e-10 of the peak (measured below in float64, wrong machine against right), less than half an ulp of the f32 samples
                            any comparison reads -- the case would be empty.  So both machines, right and wrong, run on the designs with ECHO = 0.01
                            added to the last tap, which gives the entry weight: reported at position degree - 2 of a block behind the first
      drop_overloop_head    (added) Overloop [0], the largest entry, is lost, on the designs as they are: position 0 of a block behind the first
      off_clears_c          "Off" clears the output block: the block played when the filter comes on again is silence
      late                  every setter one call late"""
    run, ev = seeded["run"], seeded["ev"]
    events = dict(off_clears_c="off" if side == "input" else "cut").get(defect, "width" if side == "input" else "cut")
    Lb, D = (om.IN_L, om.IN_TAPS) if side == "input" else (om.AU_L, om.AU_TAPS)
    smear = SMEAR if side == "input" else 0
    if defect == "late":
        rep = run(side, events + "_late", ref=events)
    elif defect == "drop_overloop_entry":
        own = run(side, events, defect, f32=False)
        print("[seeded: drop_overloop_entry, %s side] on the designs as they are, in float64: %.3e of the peak (half an ulp of an f32 sample at the peak: %.3e)" % (side, own.rel, 2.0 ** -25))
        assert own.rel < 2.0 ** -25
        rep = run(side, events, defect, echo=ECHO)
    else:
        rep = run(side, events, defect)
    assert rep.rel > rep.bound, "not reported: %s" % rep
    setters = [p for p, _ in ev[events][1:]]
    block, position, p = restart_of(rep, side, ev[events])
    if defect == "clear_overloop":
        assert block == 1 and position < D - 1 + smear and (rep.block, rep.position) == (block, position)
        region(rep, side, p + Lb, p + Lb + D - 2, smear)
    elif defect in ("no_replay", "position_off_by_one"):
        assert p in setters and block <= 2 and (rep.block, rep.position) == (block, position)
        region(rep, side, p, p + 2 * Lb + D, smear)
    elif defect == "drop_overloop_head":
        assert rep.on and rep.position < 1 + smear and rep.block >= 1
    elif defect == "drop_overloop_entry":
        assert rep.on and rep.block >= 1 and D - 2 <= rep.position <= D - 2 + smear and (rep.block, rep.position) == (block, position)
    elif defect == "off_clears_c":
        on_again = [q for (q, v), (_, before) in zip(ev[events][1:], ev[events][:-1]) if v > 0 and before == 0][0]
        assert p == on_again and block == 0 and (rep.block, rep.position) == (0, position)
        region(rep, side, on_again, on_again + Lb - 1, smear)
    elif defect == "late":
        late_ev = ev[events + "_late"]
        pairs = [(a[0], b_[0]) for a, b_ in zip(ev[events][1:], late_ev[1:])]
        idx = rep.index * om.DECIM + om.DECIM - 1 if side == "input" else rep.index
        assert any(a <= idx <= b_ + 2 * Lb + D + smear for a, b_ in pairs), (idx, pairs)
        region(rep, side, pairs[0][0], pairs[-1][1] + 2 * Lb + D, smear)
    else:
        region(rep, side, 0, 10 ** 9, 0)


def test_deemphasis_in_front_of_the_filter_is_reported(seeded):
    """The audio side with the de-emphasis in front of the filter: the same stream while the filter is LTI, another wherever a block is played again or
    the filter is off -- reported behind channel 3's first setter."""
    rep = seeded["run"]("audio", "cut", deemph_first=True)
    first = seeded["ev"]["cut"][1][0]
    assert rep.rel > rep.bound and rep.index >= first, str(rep)
    region(rep, "audio", first, 10 ** 9, 0)


# ------------------------------------------------------------------------------------------------ 7. what the call lists make the host decide
def test_the_call_lists_cover_every_path():
    """From the models' own block counters (the kernels cannot report which path ran): case r's and case b's list (six kinds of channels) holds, on
    each side, a call every filter takes whole, one that ends on every channel's block boundary, one that crosses a boundary, one that crosses
    several, one with channels at different positions, a call of one sample -- and, on the audio side, a call without an fm sample at which a
    setter is taken over; the one-channel handle the same without `differ`.  Channel 5's setters meet its machines at inp == 0 and inp == L - 1.
    Case p's 40 calls of 49152 samples are given: which of them the machines make is the library's choice (the promotion), so their coverage cannot
    be computed in advance; with 49152 input and 4096 fm samples a call against blocks of 65285 and 7436 they alternate between the fused and the
    split path on both sides, with the kinds at different positions behind the first setter."""
    assert sum(om.R_CALLS) == 1619727 and max(om.R_CALLS) == 230400
    for name, bw, lf, need in (("six channels", om.R_BW, om.R_LF, om.REQUIRED), ("one channel", [om.R_SINGLE_BW], [om.R_SINGLE_LF], [f for f in om.REQUIRED if f != "differ"])):
        cin = om.coverage(om.R_CALLS, om.BW0, bw, om.IN_L, False)
        cau = om.coverage(om.R_CALLS, om.LF0, lf, om.AU_L, True)
        for side, cov, extra in (("input", cin, ()), ("audio", cau, ("empty",))):
            have = set().union(*cov)
            print("[coverage, %s, %s side] %s" % (name, side, {f: [k for k, s in enumerate(cov) if f in s] for f in sorted(have)}))
            assert all(f in have for f in tuple(need) + extra), (name, side, have)
        if len(bw) > 1:
            assert "exact" in cin[0] and "exact" in cau[1] and "whole" in cau[0] and "empty" in cau[9] and "several" in cin[8] and "several" in cau[8]
    at_in = om.position_at_setters(om.R_CALLS, om.BW0, om.R_BW[5], om.IN_L, False)
    at_au = om.position_at_setters(om.R_CALLS, om.LF0, om.R_LF[5], om.AU_L, True)
    assert at_in == {1: (True, 0), 3: (True, om.IN_L - 1)} and at_au == {2: (True, 0), 4: (True, om.AU_L - 1)}
    mid = om.position_at_setters(om.R_CALLS, om.BW0, om.R_BW[2], om.IN_L, False)
    assert 0 < mid[7][1] < om.IN_L - 1 and om.boundaries(om.R_CALLS)[10] - om.boundaries(om.R_CALLS)[7] > om.IN_L          # "Off" in mid-block, on again after more than a block

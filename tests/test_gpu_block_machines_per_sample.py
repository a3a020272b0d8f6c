"""The reference's two overlap-add filters as the block machines of fmx_ola.hip, and the promotion and demotion of a batch onto them and back
(fmx_promote.hip, promote () / demote () in fmx_api.hip), sample by sample across setBandwidth / setlfcutoff in mid-stream.

After EVERY call FMX_TAP_FM_IQ, FMX_TAP_LR_RAW and FMX_TAP_PRE_RESAMPLER of every probed channel are read for last_fm_samples () samples (that
may be none) and concatenated.  The references are the float64 models of tests/ola_model.py, which know nothing of the library; the oracle takes no part here:
  FM_IQ           against InputSide over the whole stream: the reference's order in front of the filter, the input machine across the setters,
                  the two decimators.  Bound 2.62e-6 of the channel's peak: stage A's (stage_a_model.STAGE_A_BOUND_ON); the machines' own
                  measurement, 2 x 9.61e-7, is not larger.
  PRE_RESAMPLER   against AudioSide on the handle's OWN LR_RAW: matrix, the audio machine across the setters, de-emphasis.  Bound 2 x 9.22e-7 =
                  1.84e-6 of the peak; the samples that depend on what a promotion reconstructs with its f32-inverted de-emphasis -- from the
                  promotion until two audio blocks, 14872 fm samples, behind it -- 1.84e-6 + 2 x 3.57e-7 = 2.56e-6.
The constants are measured on the CPU from the reference alone (tests/test_ola_model_cpu.py), never from what the kernels give.  Every case checks every
sample of every call and prints, per tap, its worst sample relative to the peak, the call, the block since the last restart and the position in the
block where it fell, and the bound it was held to.
"""
import importlib
import re

import numpy as np
import pytest

import ola_model as om
import stage_b_model as sb

pytestmark = pytest.mark.gpu

M = importlib.import_module("sdr-j-fm_amd").fmx
TAPS = (("z", M.TAP_FM_IQ), ("lr", M.TAP_LR_RAW), ("pre", M.TAP_PRE_RESAMPLER))
PID = dict(att_l=M.P_ATTENUATION_L, att_r=M.P_ATTENUATION_R, lo=M.P_LOCAL_OSCILLATOR, dc_remove=M.P_DC_REMOVE)


def handle(fmx_amd, nch, stream_of, max_block, restarts=None, scope=None, kernel=None):
    f = fmx_amd.Fmx(nch, streams=max(stream_of) + 1, stream_of_channel=stream_of, max_block=max_block)
    for pid, v in ((M.P_BANDWIDTH, om.BW0), (M.P_LF_CUTOFF, om.LF0), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 0)):
        f.set_param(pid, v)
    for pid, v in ((M.P_FILTER_RESTARTS, restarts), (M.P_SCOPE_TAPS, scope), (M.P_FRONT_KERNEL, kernel)):
        if v is not None:
            f.set_param(pid, v)
    return f


def settings(f, kind_of_channel):
    for c, kd in enumerate(kind_of_channel):
        for k, v in kd.items():
            f.set_param(PID[k], v, c)


class Run:
    """The calls of one case, as test_gpu_stage_a_per_sample.Run with three taps: the taps of every probed channel after every call, where every
    call begins, the stage-A kernel of every call; groups of channels that must be bit-identical on all three taps after every call."""

    def __init__(self, f, iq, calls, probe, before_call=None, groups=()):
        self.t = {c: {k: [] for k, _ in TAPS} for c in probe}
        self.starts, self.kernel = [], []
        pos = j = 0
        for k, s in enumerate(calls):
            if before_call is not None:
                before_call(k)
            pcm = f.process_host(iq[:, pos:pos + s])
            assert np.isfinite(pcm).all(), k
            pos += s
            self.kernel.append(f.last_front_kernel())
            nj = f.last_fm_samples()
            assert nj == pos // om.DECIM - j, (k, nj)
            self.starts.append(j)
            for c in probe:
                for name, tap in TAPS:
                    self.t[c][name].append(f.tap(tap, nj, c) if nj else np.zeros((0, 2), np.float32))
            if nj:
                for group in groups:
                    for name, tap in TAPS:
                        first = self.t[group[0]][name][-1] if group[0] in self.t else f.tap(tap, nj, group[0])
                        for c in group[1:]:
                            assert np.array_equal(f.tap(tap, nj, c), first), ("tap %s of channel %d differs from channel %d's" % (name, c, group[0]), k)
            j += nj
        self.fm_samples = j

    def stream(self, c):
        return {k: np.concatenate(v) for k, v in self.t[c].items()}


def check_all(failed):
    assert not failed, "%d comparison(s) failed\n  " % len(failed) + "\n  ".join(failed)


def held(failed, fn, *a, **kw):
    """Every comparison of a case is made and printed whatever became of the others."""
    try:
        return fn(*a, **kw)
    except AssertionError as e:
        failed.append(str(e).split("\n")[0][:600])


# ------------------------------------------------------------------------------------------------ r, b: the machines from the first call
_input_sides = {}


def r_input_side(ol, iq, c):
    """Case r's and case b's input-side model of kind c (the model is the same for both: streams, calls, settings and setters are)."""
    if c not in _input_sides:
        kd = om.R_KINDS[c]
        _input_sides[c] = om.InputSide(ol.oracle(), iq[om.R_STREAM[c]], om.R_CALLS, om.r_input_events(c), lo=kd.get("lo", 0), att=(kd.get("att_l", 1.0), kd.get("att_r", 1.0)))
    return _input_sides[c]


def r_setters(f, channels_of_kind, bw, lf):
    """before_call: kind i's setters {call: value} go to the channels channels_of_kind [i]."""
    def before(k):
        for i, chans in enumerate(channels_of_kind):
            for table, pid in ((bw[i], M.P_BANDWIDTH), (lf[i], M.P_LF_CUTOFF)):
                if k in table:
                    for c in chans:
                        f.set_param(pid, table[k], c)
    return before


def judge_r(name, ol, iq, r, probe_kind, lf=None):
    """probe_kind: {probed channel: kind}; lf: other cut-off setters per kind than case r's.  FM_IQ and PRE_RESAMPLER of every probed channel, every sample."""
    L = ol.oracle()
    failed = []
    cs = r.starts
    for c, i in probe_kind.items():
        t = r.stream(c)
        side = r_input_side(ol, iq, i)
        assert t["z"].shape[0] == side.z.shape[0] == sum(om.R_CALLS) // om.DECIM
        held(failed, om.judge, "%s, channel %d (kind %d), FM_IQ" % (name, c, i), t["z"], side.z, cs, side.where, om.OLA_IN_BOUND)
        au = om.AudioSide(L, t["lr"], om.audio_events(om.R_CALLS, om.LF0, (lf or om.R_LF)[i]))
        assert float(np.abs(au.y).max()) > 0.1, (c, "a silent channel")
        held(failed, om.judge, "%s, channel %d (kind %d), PRE_RESAMPLER" % (name, c, i), t["pre"], au.y, cs, au.where, om.OLA_AU_BOUND)
    check_all(failed)


def test_r_receiver(fmx_amd, ol):
    """A default handle of six channels on two streams (stream 1 with a DC offset of (0.004, -0.003), inside the limiter): the machines run from the
    first call; ola_model.R_CALLS, 25 calls, 1 619 727 input samples -- the input machine's first block ends with call 0, the audio machine's with
    call 1 (the fused path with the transform behind it), the 230400-sample calls cross three and two blocks, calls of 12, 13 and 1 samples, one of
    them without an fm sample while channel 3's "off" is pending (tests/test_ola_model_cpu.py asserts the list's coverage from the models' counters).
      channel 0  no setter (control)
      channel 1  width 120 kHz in mid-block (call 7), the same again (call 10)
      channel 2  "Off" in mid-block (call 7), 165 kHz again 330400 samples later (call 10: stale buffers played)
      channel 3  audio cut-off 15000 -> 9000 (call 5) -> off (call 9) -> 15000 (call 14)
      channel 4  oscillator 2500 Hz, balance 0.9 / 1.1; width 130 kHz and cut-off 12000 at one call (8)
      channel 5  restarts at inp == 0 and inp == L - 1 of both machines (calls 1, 3: widths; calls 2, 4: cut-offs)
    Then a handle of one channel with channel 1's widths and channel 3's cut-offs: every call is fused or split for one filter alone.
    Measured on the MI355X: FM_IQ 2.8e-7 ... 3.5e-7 of the peak (worst: channel 4, call 10, block 4, position 57819; bound 2.62e-6), PRE_RESAMPLER 5.1e-7 ... 6.4e-7
    (worst: channel 5, call 24, block 15, position 4433; bound 1.84e-6); the one-channel handle 3.5e-7 (bit-identical to channel 1 of the six) and 5.7e-7."""
    iq = om.r_streams(ol)
    f = handle(fmx_amd, 6, om.R_STREAM, max(om.R_CALLS))
    settings(f, om.R_KINDS)
    r = Run(f, iq, om.R_CALLS, range(6), r_setters(f, [[c] for c in range(6)], om.R_BW, om.R_LF))
    assert set(r.kernel) == {1}
    judge_r("r, six channels", ol, iq, r, {c: c for c in range(6)})
    del f
    f = handle(fmx_amd, 1, [0], max(om.R_CALLS))
    r1 = Run(f, iq[1:2], om.R_CALLS, [0], r_setters(f, [[0]], [om.R_SINGLE_BW], [om.R_SINGLE_LF]))
    judge_r("r, one channel", ol, iq, r1, {0: 1}, lf=[None, om.R_SINGLE_LF])


def test_b_machines_on_a_batch(fmx_amd, ol):
    """FMX_P_FILTER_RESTARTS = 1 and FMX_P_SCOPE_TAPS = 1 on 65 channels: every step of the machines is a table in device memory (OlaStepRef::tab).
    Case r's calls, streams, kinds and setters by c mod 6; the first channel of each kind probed and modelled, every other channel bit-identical
    to the first of its kind (and so of its stream) on all three taps after every call.
    Measured on the MI355X: FM_IQ as case r's, bit for bit; PRE_RESAMPLER 5.1e-7 ... 7.4e-7 of the peak (worst: kind 5, call 22, block 13, position 6049; bound 1.84e-6)."""
    nch = 65
    iq = om.r_streams(ol)
    kind = [c % 6 for c in range(nch)]
    f = handle(fmx_amd, nch, [om.R_STREAM[i] for i in kind], max(om.R_CALLS), restarts=1, scope=1)
    settings(f, [om.R_KINDS[i] for i in kind])
    groups = [list(range(i, nch, 6)) for i in range(6)]
    r = Run(f, iq, om.R_CALLS, range(6), r_setters(f, groups, om.R_BW, om.R_LF), groups)
    assert set(r.kernel) == {1}
    judge_r("b, 65 channels", ol, iq, r, {c: c for c in range(6)})


# ------------------------------------------------------------------------------------------------ p: promotion and demotion
P_NCH = 65


def p_streams(ol):
    n = sum(om.P_CALLS)
    return np.stack([ol.synth_iq(n, leftHz=400.0 + 300 * k, rightHz=700.0 + 200 * k, dcI=(0.0, 0.004)[k], dcQ=(0.0, -0.003)[k], pilotLevel=0.12) for k in range(2)])


class Promoted:
    """A batch through om.P_CALLS with setters that wait for the promotion: plan {call: [(pid, value, kinds)]}; a setter made in front of call k holds
    from the first call at which fmx_filter_change_due () <= 0 (a block-machine handle: at once).  applied: [(call it was made at, call it held
    from, pid, value, kinds)]."""

    def __init__(self, f, iq, kind, plan, probe, groups=(), front_kernel=None):
        self.applied, waiting = [], []
        me = self

        def before(k):
            for pid, v, kinds in plan.get(k, []):
                for c in range(len(kind)):
                    if kind[c] in kinds:
                        f.set_param(pid, v, c)
                waiting.append((k, pid, v, kinds))
            if waiting and f.filter_change_due() <= 0:
                me.applied += [(k0, k, pid, v, kinds) for k0, pid, v, kinds in waiting]
                del waiting[:]
        self.run = Run(f, iq, om.P_CALLS, probe, before, groups)
        assert not waiting and len(self.applied) == sum(len(v) for v in plan.values())
        assert all(k - k0 <= 5 for k0, k, _, _, _ in self.applied), self.applied

    def events(self, pid, i):
        """{call: value} of kind i's setters of one sort, at the calls they held from."""
        return {k: v for _, k, p, v, kinds in self.applied if p == pid and i in kinds}


def test_p1_promotion_on_the_automatic_kernel(fmx_amd, ol):
    """65 channels, automatic FMX_P_FILTER_RESTARTS and stage-A kernel (front_kernel on every call, asserted), FMX_P_SCOPE_TAPS = 1, 40 calls of 49152
    samples.  Kinds by c mod 3: plain with RF DC removal off on a stream without an offset; oscillators 2500 and -4000 Hz with RF DC removal ON on a
    stream with an offset of (0.004, -0.003) -- front_kernel takes those in the reference's order, so ONE model of the reference's order holds in
    front of, across and behind the promotion: what the promotion's run over the kept samples makes of the snapshot of RfDC and the oscillator's
    phase (promo_state_kernel) is in every sample behind it.  A width of 130 kHz for kinds 0 and 1 at call 10; kind 2 is promoted with them and
    must not notice.  FM_IQ only, every sample: nothing tells this case which form made a call's PRE_RESAMPLER (case p2 judges it).
    Measured on the MI355X: the setter made at call 10 holds from call 15; 2.5e-7 / 2.8e-7 / 3.5e-7 of the peak (worst: call 21, block 16, position 17595; bound 2.62e-6)."""
    iq = p_streams(ol)
    kinds = [dict(dc_remove=0), dict(lo=2500), dict(lo=-4000)]
    kind = [c % 3 for c in range(P_NCH)]
    f = handle(fmx_amd, P_NCH, [0 if i == 0 else 1 for i in kind], max(om.P_CALLS), scope=1)
    settings(f, [kinds[i] for i in kind])
    groups = [list(range(i, P_NCH, 3)) for i in range(3)]
    p = Promoted(f, iq, kind, {10: [(M.P_BANDWIDTH, 130000, (0, 1))]}, range(3), groups)
    print("\n[p1] setters made at / holding from call: %s; stage-A kernel per call: %s" % ([(a, b) for a, b, _, _, _ in p.applied], "".join(str(k) for k in p.run.kernel)))
    assert set(p.run.kernel) == {1}
    L = ol.oracle()
    failed = []
    for c in range(3):
        kd = kinds[c]
        side = om.InputSide(L, iq[0 if c == 0 else 1], om.P_CALLS, om.input_events(om.P_CALLS, om.BW0, p.events(M.P_BANDWIDTH, c)), lo=kd.get("lo", 0), dc_remove=kd.get("dc_remove", 1))
        held(failed, om.judge, "p1, channel %d, FM_IQ" % c, p.run.stream(c)["z"], side.z, p.run.starts, side.where, om.OLA_IN_BOUND)
    check_all(failed)


def test_p2_promotion_and_demotion_on_the_matrix_pipe(fmx_amd, ol):
    """65 channels, automatic FMX_P_FILTER_RESTARTS, FMX_P_FRONT_KERNEL = 3, FMX_P_SCOPE_TAPS = 1, 40 calls of 49152 samples (32 tiles each):
    fmx_last_front_kernel tells the folded calls (3) from the machines' (1); the sequence folded, machines, folded, machines, folded is asserted.
    Kinds by c mod 5, all with RF DC removal off (the matrix-pipe kernel applies it behind the filter: test_d's subject): 0 plain, 1 oscillator
    2500 Hz, 2 balance 0.9 / 1.1 (probed); 3 and 4 plain (not probed).  Call 2: width 130 kHz for kinds 0 and 2, "Off" for kind 3, the width in
    use again for kind 4.  The first machine call + 1: kind 3 on again (a handle with a filter switched off in mid-block stays on the machines).
    Behind the demotion: cut-off 12000 for kinds 0 and 1 -- the second promotion takes its block phase from origin_in / origin_au as demote left them.
    FM_IQ against one model for the whole stream.  PRE_RESAMPLER per call by form: stage_b_model.link_e (the de-emphasis behind the matrix, bound
    4.12e-7) on folded calls, AudioSide on the machines' calls -- it runs from sample 0: a folded handle is the machine without a restart --, with the
    widened bound for the 14872 samples behind each promotion.
    Measured on the MI355X: kernels per call 3333333111111113333333331111111333333333, the setters of calls 2, 8 and 19 hold from 7, 8 and 24; FM_IQ 2.8e-7 ... 3.2e-7 of
    the peak (bound 2.62e-6); PRE_RESAMPLER on the machines' calls 3.8e-7 ... 4.1e-7 (bound 1.84e-6), within 14872 samples behind a promotion 4.4e-7 ... 5.7e-7 (bound
    2.56e-6), on the folded calls 2.2e-7 ... 2.5e-7 (bound 4.12e-7)."""
    iq = p_streams(ol)
    kinds = [dict(dc_remove=0), dict(dc_remove=0, lo=2500), dict(dc_remove=0, att_l=0.9, att_r=1.1), dict(dc_remove=0), dict(dc_remove=0)]
    kind = [c % 5 for c in range(P_NCH)]
    f = handle(fmx_amd, P_NCH, [c % 2 for c in range(P_NCH)], max(om.P_CALLS), scope=1, kernel=3)
    settings(f, [kinds[i] for i in kind])
    plan = {2: [(M.P_BANDWIDTH, 130000, (0, 2)), (M.P_BANDWIDTH, 0, (3,)), (M.P_BANDWIDTH, om.BW0, (4,))], 8: [(M.P_BANDWIDTH, om.BW0, (3,))], 19: [(M.P_LF_CUTOFF, 12000, (0, 1))]}
    p = Promoted(f, iq, kind, plan, range(3))
    runs = "".join(str(k) for k in p.run.kernel)
    print("\n[p2] setters made at / holding from call: %s; stage-A kernel per call: %s" % ([(a, b) for a, b, _, _, _ in p.applied], runs))
    assert re.fullmatch(r"3+1+3+1+3+", runs), runs
    assert runs[8] == "1" and runs[19] == "3", "the plan's calls do not fall where they were meant to: %s" % runs
    machine = np.array([k == 1 for k in p.run.kernel])
    promoted_at = [k for k in range(1, len(runs)) if machine[k] and not machine[k - 1]]
    L = ol.oracle()
    failed = []
    cs = np.array(p.run.starts + [p.run.fm_samples])
    on_machine = np.repeat(machine, np.diff(cs))
    wide = np.zeros(p.run.fm_samples, bool)
    for k in promoted_at:
        wide[cs[k]:cs[k] + om.PROMO_REACH] = True
    for c in range(3):
        kd = kinds[c]
        t = p.run.stream(c)
        side = om.InputSide(L, iq[c % 2], om.P_CALLS, om.input_events(om.P_CALLS, om.BW0, p.events(M.P_BANDWIDTH, c)), lo=kd.get("lo", 0),
                            att=(kd.get("att_l", 1.0), kd.get("att_r", 1.0)), dc_remove=0)
        held(failed, om.judge, "p2, channel %d, FM_IQ" % c, t["z"], side.z, p.run.starts, side.where, om.OLA_IN_BOUND)
        au = om.AudioSide(L, t["lr"], om.audio_events(om.P_CALLS, om.LF0, p.events(M.P_LF_CUTOFF, c)))
        folded = sb.link_e(t["lr"])
        peak = float(np.abs(au.y).max())
        assert peak > 0.1 and float(np.abs(folded).max()) > 0.1
        # one comparison over the stream, every sample against its call's form and held to its own bound (all relative to one peak: the machines')
        ref = np.where(on_machine[:, None], au.y, folded)
        bound = np.where(on_machine, np.where(wide, om.OLA_AU_BOUND_PROMOTED, om.OLA_AU_BOUND), sb.E_BOUND * float(np.abs(folded).max()) / float(np.abs(ref).max()))
        held(failed, judge_by_sample, "p2, channel %d, PRE_RESAMPLER" % c, t["pre"], ref, p.run.starts, au.where, bound, on_machine, wide & on_machine)
    check_all(failed)


def judge_by_sample(name, got, ref, call_starts, where, bound, on_machine, wide):
    """ola_model.judge with a bound per sample; the line names the form of the call that holds the worst sample, and gives the worst of each form and of
    the samples behind a promotion (wide) beside it."""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert g.shape == r.shape
    peak = float(np.abs(r).max())
    e = np.abs(g - r).max(axis=1) / peak
    i = int(np.argmax(e / bound))
    call = int(np.searchsorted(np.asarray(call_starts), i, side="right") - 1)
    on, block, position = where(i)
    print("\n[%s] worst sample against its bound: %.3e of the peak %.4g at fm sample %d: call %d (%s), block %d since the last restart, position %d; bound %.3e; "
          "worst of the machines' calls %.3e (bound %.3e), of those within %d samples behind a promotion %.3e (bound %.3e), of the folded calls %.3e"
          % (name, e[i], peak, i, call, "machines" if on_machine[i] else "folded", block, position, bound[i], float(e[on_machine & ~wide].max()), om.OLA_AU_BOUND,
             om.PROMO_REACH, float(e[wide].max()), om.OLA_AU_BOUND_PROMOTED, float(e[~on_machine].max())))
    assert e[i] <= bound[i], "%s: worst sample %.3e of the peak beyond its bound %.3e at fm sample %d, call %d (%s), block %d, position %d" % (
        name, e[i], bound[i], i, call, "machines" if on_machine[i] else "folded", block, position)

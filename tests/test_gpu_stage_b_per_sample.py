"""Stage B (fmx_stageb.hip) sample by sample: four feed-forward links of the memoryless decoders, each on the stream the kernel itself read.

After EVERY call FMX_TAP_FM_IQ, FMX_TAP_DEMOD, FMX_TAP_PILOT_PHASE, FMX_TAP_LR_RAW and (folded handles) FMX_TAP_PRE_RESAMPLER are read for
last_fm_samples () samples and concatenated; sample j of every tap is fm sample j (stage_b_model.TAP_OFFSET: asserted through the bit identities
below, never searched for).  Every link's reference is the oracle -- or a restatement tests/test_stage_b_model_cpu.py proves bit-identical to
it -- evaluated on the handle's own upstream tap, so whatever happens upstream drops out:

  link D  FM_IQ -> DEMOD            handles of up to 64 channels: bit-identical to fmo_demod_run.  Batches (the fast forms): every sample
                                    within 2 x 1.50e-7 = 3.0e-7 of the peak, except up to 0.2 % of the samples by at most one entry of the
                                    decoder's table (the one-ulp limiter moves an index now and then: the reference alone does so in 0.025 %
                                    of the samples when its input moves by 6e-8); a carrier 20 kHz off tune within 2 x 3.56e-5 of the peak.
  link P  5 DEMOD -> PILOT_PHASE    sequential solver: 2 x 3.83e-6 = 7.66e-6 rad on the circle (what +-1.2e-7 on the NCO sine does to the
                                    reference's own loop); Newton (batches): rms 1e-5 rad, every sample 1e-4 rad, no replay.  Lock onset:
                                    LR_RAW.im is exactly zero until the sample at which fmo_pilot_run on the own DEMOD locks.
  link S  -> LR_RAW                 .re is DEMOD bit for bit; .im within 2 |demod| 1.5e-7 + one ulp at EVERY sample with PSS off; with PSS on
                                    (the oracle's fmo_pss_* in closed loop on the own taps) up to 2 % of the samples one table step off.
  link E  LR_RAW -> PRE_RESAMPLER   folded handles: the matrix in the reference's f32 expressions, the one-pole in float64; 2 x 2.06e-7 =
                                    4.1e-7 of the peak.
The constants are measured on the CPU from the reference alone (stage_b_model.py), never from what the kernels give.  Every case prints its
figures; a failure names link, channel, call, segment (1536 fm samples) and thread (6 samples) of its worst sample.
"""
import importlib

import numpy as np
import pytest

import stage_b_model as sb

pytestmark = pytest.mark.gpu

M = importlib.import_module("sdr-j-fm_amd").fmx
CALLS = sb.CALLS
LOCKING = ("default", "tones", "mistuned", "decoders")


def handle(fmx_amd, nch, stream_of, folded=None, scope=None, form=None):
    f = fmx_amd.Fmx(nch, streams=max(stream_of) + 1, stream_of_channel=stream_of, max_block=max(CALLS))
    for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 0), (M.P_FM_DECODER, 3)):
        f.set_param(pid, v)
    for pid, v in ((M.P_FILTER_RESTARTS, 2 if folded else None), (M.P_SCOPE_TAPS, scope), (M.P_STAGEB_FORM, form)):
        if v is not None:
            f.set_param(pid, v)
    return f


def settings(f, kinds):
    """kinds: per channel a dict with decoder / selector / fm_mode / panorama / pss."""
    pid = dict(decoder=M.P_FM_DECODER, selector=M.P_SOUND_MODE, fm_mode=M.P_FM_MODE, panorama=M.P_STEREO_PANORAMA, pss=M.P_PSS)
    for c, kd in enumerate(kinds):
        for k, v in kd.items():
            if k in pid:
                f.set_param(pid[k], v, c)


def programmes(ol, names):
    return np.stack([ol.synth_iq(sum(CALLS), **sb.PROGRAMMES[n]) for n in names])


TAPS = (("z", M.TAP_FM_IQ), ("demod", M.TAP_DEMOD), ("phase", M.TAP_PILOT_PHASE), ("lr", M.TAP_LR_RAW), ("pre", M.TAP_PRE_RESAMPLER))


class Run:
    """The calls of one case: the five taps of every probed channel after every call, where every call begins, the PSS shift of every
    metaData snapshot; twins (groups of channels with equal settings on one stream): PCM and taps bit-identical after every call.
    calls, taps: another call list (input samples per call) and another choice of taps than this module's (tests/test_gpu_prepass_per_sample.py);
    before_call (k), after_call (k, fm samples of the call): hooks, for a setter at a call boundary and for a per-call read-out."""

    def __init__(self, f, iq, probe, twins=(), calls=None, taps=None, before_call=None, after_call=None):
        CALLS, TAPS = (globals()["CALLS"] if calls is None else calls), (globals()["TAPS"] if taps is None else taps)
        self.t = {c: {k: [] for k, _ in TAPS} for c in probe}
        self.starts, self.shift = [], {c: [] for c in probe}
        pos = j = 0
        for k, s in enumerate(CALLS):
            if before_call is not None:
                before_call(k)
            pcm = f.process_host(iq[:, pos:pos + s])
            pos += s
            nj = f.last_fm_samples()
            self.starts.append(j)
            for c in probe:
                for name, tap in TAPS:
                    self.t[c][name].append(f.tap(tap, nj, c))
                self.shift[c].append(float(f.meta(c).PssPhaseShiftDegree))
            for group in twins:
                assert (pcm[list(group)] == pcm[group[0]]).all(), ("PCM of twins", k, group)
                for c in [c for c in group if c in self.t][:1]:          # (a probed member: its partners' taps against its own)
                    for other in group:
                        for name, tap in TAPS:
                            assert other == c or np.array_equal(f.tap(tap, nj, other), self.t[c][name][-1]), ("tap %s of twins" % name, k, c, other)
            if after_call is not None:
                after_call(k, nj)
            j += nj
        self.fm_samples = j
        assert pos == sum(CALLS) and j == pos // 12

    def stream(self, c):
        return {k: np.concatenate(v) for k, v in self.t[c].items()}


def judge(name, r, c, kd, programme, batch, folded):
    """All links of one channel, kd its settings.  Every link is judged whatever became of the others; a failure of the channel lists them
    all.  -> the figures, for the case's summary line."""
    t = r.stream(c)
    z, dem, ph, lr = t["z"], t["demod"], t["phase"], t["lr"]
    decoder, selector, pss = kd.get("decoder", 3), kd.get("selector", 0), kd.get("pss", 0)
    tag = "%s, channel %d (%s, decoder %d, selector %d%s)" % (name, c, programme, decoder, selector, ", PSS" if pss else "")
    out, failed = {}, []
    php, lk, st = sb.pilot_oracle(dem)                   # the reference's loop and lock detector on the handle's own DEMOD
    nz = np.flatnonzero(lr[:, 1])

    def link_d():
        ref = sb.demod_oracle(z, decoder)
        assert sb.demod_peak(ref) > 0.1, tag
        if not batch:
            sb.check_identical("D", c, dem, ref, r.starts)
            out["D"] = 0.0
        elif programme == "mistuned":
            w = sb.compare("D", c, dem, ref, r.starts, scale=sb.demod_peak(ref))
            sb.report(tag + ", link D across AFC_EXACT_THR", w, sb.D_MISTUNED_BOUND)
            out["D"] = w.rel
            sb.check(w, sb.D_MISTUNED_BOUND, tag)
        else:
            w, share, _ = sb.check_d_batch(c, dem, ref, decoder, r.starts, tag)
            out["D"], out["D slips"] = w.rel, share

    def link_s_sum():
        sb.check_identical("S.re", c, lr[:, 0], dem, r.starts)

    def link_p():
        w = sb.compare("P", c, ph, php, r.starts, scale=1.0, circular=True)
        out["P"], out["P rms"] = w.rel, w.rms
        if batch:
            sb.report(tag + ", link P (Newton): rms %.3e rad (bound %.0e)" % (w.rms, sb.P_NEWTON_RMS), w, sb.P_NEWTON_WORST)
            sb.check(w, sb.P_NEWTON_WORST, tag)
            assert w.rms <= sb.P_NEWTON_RMS, "%s: link P rms %.3e rad exceeds %.0e" % (tag, w.rms, sb.P_NEWTON_RMS)
        else:
            sb.report(tag + ", link P (sequential)", w, sb.P_SEQ_BOUND)
            sb.check(w, sb.P_SEQ_BOUND, tag)

    def lock_onset():
        if programme not in LOCKING:
            assert not lk.any() and nz.size == 0, "%s: a channel on noise locked" % tag
            return
        cross, _ = sb.lock_crossings(st)
        sides = np.abs(np.concatenate([st[cross - 1], st[cross]]).astype(np.float64) - float(sb.LOCK_THRESHOLD))
        assert cross.size and float(sides.min()) >= sb.LOCK_MARGIN, "%s: the lock metric comes within %.2e of 0.07: choose another input" % (tag, float(sides.min()))
        first = int(np.argmax(lk))
        assert lk.any() and lk[first:].all() and lk.sum() > 40000, tag
        print("[%s] lock onset: the model locks at fm sample %d (%d crossings of 0.07, the nearest side %.2e away); LR_RAW.im is first non-zero at %s"
              % (tag, first, cross.size, float(sides.min()), int(nz[0]) if nz.size else None))
        out["lock"] = first
        assert nz.size and int(nz[0]) == first, "%s: lock onset at %s, the reference locks at %s" % (
            tag, sb.locate("P", c, int(nz[0]), r.starts) if nz.size else None, sb.locate("P", c, first, r.starts))

    def link_s_difference():
        if not pss:
            sb.check_s(c, lr[:, 1], sb.lr_diff(dem, ph, lk, selector=selector), dem, r.starts, 0.0, tag)
            return
        loop = sb.PssLoop()
        ref_im, _, after = loop.run(dem, ph, lk, selector=selector)
        loop.close()
        at = 96000                                       # the first metaData snapshot: behind fm sample fmRate / 2 (fm-processor.cpp:662-684)
        got = r.shift[c][int(np.searchsorted(r.starts, at, side="right") - 1)]
        model_deg = float(np.float32(float(after[at]) / np.pi * 180.0))
        print("[%s] PssPhaseShiftDegree of the snapshot behind sample %d: handle %.6g, model %.6g (difference %.3e); the model's accumulator ends at %.6g rad"
              % (tag, at, got, model_deg, got - model_deg, float(after[-1])))
        _, out["S slips"] = sb.check_s(c, lr[:, 1], ref_im, dem, r.starts, sb.PSS_SLIP_SHARE, tag)
        assert abs(got - model_deg) <= 180.0 / np.pi * 1e-6, "%s: PssPhaseShiftDegree %.6g, the model's %.6g" % (tag, got, model_deg)

    def link_e():
        ref = sb.link_e(lr, selector, kd.get("fm_mode", 0), kd.get("panorama", 100))
        w = sb.compare("E", c, t["pre"], ref, r.starts)
        sb.report(tag + ", link E", w, sb.E_BOUND)
        out["E"] = w.rel
        assert w.scale > 0.1, tag
        sb.check(w, sb.E_BOUND, tag)

    for fn in (link_d, link_s_sum, link_p, lock_onset, link_s_difference) + ((link_e,) if folded else ()):
        try:
            fn()
        except AssertionError as e:
            failed.append("%s: %s" % (fn.__name__, str(e).split("\n")[0][:1500]))
    assert not failed, "%s: %d link(s) failed\n  " % (tag, len(failed)) + "\n  ".join(failed)
    return out


# ------------------------------------------------------------------------------------------------ the receiver
@pytest.mark.parametrize("folded", [False, True], ids=["block machines", "folded"])
@pytest.mark.parametrize("pss", [0, 1], ids=["PSS off", "PSS on"])
def test_receiver(fmx_amd, ol, pss, folded):
    """One channel, default settings, a pilot of 0.12 (stage_b_model.PROGRAMMES), 28 ragged calls among them 12, 13 and 1 input samples: call
    ends on every residue of the 1536-sample segment.  Link D exact, link P sequential, lock onset, link S without and with PSS; folded
    (FMX_P_FILTER_RESTARTS 2: PART 0's de-emphasis) also link E.
    Bounds: D bit-identical; P 7.66e-6 rad; S 2 |demod| 1.5e-7 + 1 ulp, no sample left out (PSS on: up to 2 % one table step off); E 4.1e-7 of the peak.
    Measured on the MI355X: D bit-identical (before the AFC fix-up's pass cap was lifted: 41 887 of 160 141 samples an ulp off, the first in call
    3, segment 1, thread 146); P 2.41e-6 rad (block machines), 1.91e-6 (folded); lock onset at sample 103720, the reference's; S with PSS off 0.83 of its
    bound, no sample beyond it (before the index fix: 0.06 % of the samples one table step off, 6.5e-5 |demod|); with PSS on 0.020 % / 0.014 % of the
    samples one step off, the snapshot behind sample 96000 at 0 degrees on both sides (the channel locks later); E 2.27e-7 / 2.15e-7 of the peak."""
    iq = programmes(ol, ["default"])
    f = handle(fmx_amd, 1, [0], folded=folded)
    kd = dict(pss=pss)
    settings(f, [kd])
    r = Run(f, iq, [0])
    out = judge("receiver, %s" % ("folded" if folded else "block machines"), r, 0, kd, "default", False, folded)
    print("\n[receiver, PSS %d, folded %d] %s" % (pss, folded, out))


# ------------------------------------------------------------------------------------------------ the decoders
def test_decoders(fmx_amd, ol):
    """Four channels on one stream (stage_b_model.PROGRAMMES "decoders": every decoder's own lock metric keeps its margin) with decoders 3
    (Mixed), 4 (ComplexBB), 5 (RealBB) and 6 (Diff), and a fifth (Mixed) on a carrier 20 kHz off tune (|afc| reaches 0.66), PSS off: link D
    bit-identical to fmo_demod_run for every one of them (the reference's divisions, the sequentially exact AFC), links P (sequential) and
    S, lock onset.
    Measured on the MI355X: D bit-identical on all five channels; P 1.19e-6 rad (Mixed, ComplexBB, the mistuned carrier), 2.4e-7 (RealBB), 9.5e-7 (Diff),
    bound 7.66e-6; lock onsets at 103791, 103791, 106969, 101444 and 103827, the reference's; S within its bound at every sample."""
    names = ["decoders", "mistuned"]
    iq = programmes(ol, names)
    kinds = [dict(decoder=d, pss=0) for d in (3, 4, 5, 6, 3)]
    stream_of = [0, 0, 0, 0, 1]
    f = handle(fmx_amd, 5, stream_of)
    settings(f, kinds)
    r = Run(f, iq, range(5))
    failed = []
    for c, kd in enumerate(kinds):
        try:
            print("\n[decoders] channel %d: %s" % (c, judge("decoders", r, c, kd, names[stream_of[c]], False, False)))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)


# ------------------------------------------------------------------------------------------------ the batch
B_NCH = 70
B_STREAMS = ["default", "tones", "mistuned", "noise"]
B_PROBE = [0, 1, 2, 3, 4, 5, 63, 64, 69]


def batch_kinds():
    """Channel c: stream c mod 4, sound selector c mod 7 (so c, c + 28 and c + 56 are twins), StereoPano with panorama 50 on the odd
    selectors, PSS on where the selector is 0 and off elsewhere."""
    return [dict(selector=c % 7, fm_mode=1 if (c % 7) % 2 else 0, panorama=50 if (c % 7) % 2 else 100, pss=1 if c % 7 == 0 else 0) for c in range(B_NCH)]


@pytest.mark.parametrize("form", [1, 2])
def test_batch(fmx_amd, ol, form):
    """70 channels on 4 streams -- default, other tones, a carrier 20 kHz off tune (crosses AFC_EXACT_THR in mid-stream and switches
    instantiations), noise only (never locks: LR_RAW.im stays zero) --, FMX_P_SCOPE_TAPS 1, folded filters, stage B as one kernel (form 1) and
    as two (form 2).  Probed: channels 0 - 5, 63, 64, 69 (every selector, both sides of the 64th channel, the last); twins (c, c + 28, c + 56)
    bit-identical in PCM and in every tap after every call.  All four links with the batch bounds (the module's docstring), no replay.
    Measured on the MI355X, the same for both forms: D 8.8e-8 of the peak on the programmes, 1.75e-7 on noise (bound 3.0e-7), table slips in 0.011 % /
    0.006 % of the samples, the largest 3.84e-5 of the peak (one step 3.89e-5); the mistuned carrier 3.35e-5 (bound 7.12e-5), its worst sample one slip at
    the signal's onset, call 3, segment 1, thread 130; P rms 2.8e-6 ... 3.1e-6 rad, worst 1.48e-5 (mistuned, on the sequential path: 1.2e-6); lock onsets
    at 103720 / 103944 / 103827, the reference's; S with PSS off 0.82 ... 0.87 of its bound (before the index fix: 102 ... 108 samples, 0.064 ... 0.067 %,
    one table step off), with PSS on 0.015 % one step off; E 1.5e-7 ... 2.8e-7 of the peak (bound 4.12e-7)."""
    iq = programmes(ol, B_STREAMS)
    kinds = batch_kinds()
    f = handle(fmx_amd, B_NCH, [c % 4 for c in range(B_NCH)], folded=True, scope=1, form=form)
    settings(f, kinds)
    twins = [tuple(range(c, B_NCH, 28)) for c in range(28)]
    r = Run(f, iq, B_PROBE, twins)
    assert f.pll_replays() == 0
    failed = []
    for c in B_PROBE:
        try:
            print("\n[batch, form %d] channel %d: %s" % (form, c, judge("batch, form %d" % form, r, c, kinds[c], B_STREAMS[c % 4], True, True)))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)

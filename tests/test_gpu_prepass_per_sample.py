"""The demodulator pre-pass (fmx_demod.hip: disc_kernel, afc_kernel <VAR>, nsq_kernel) sample by sample, on the stream the kernels themselves read.

After EVERY call FMX_TAP_FM_IQ and FMX_TAP_DEMOD of the probed channels are read for last_fm_samples () samples and concatenated (the stage-B
module's Run).  The reference of a channel is tests/prepass_model.py -- the oracle's demodulator and squelch, long-lived, on the handle's OWN FM_IQ
from fm sample 0 (tests/test_prepass_model_cpu.py proves it an oracle chain bit for bit) --, so whatever happens upstream drops out:

  every kind but those on decoder 2     DEMOD bit-identical to the model, at every handle size
  decoder 2 (the PLL decoder)           every sample within 2 x 7.94e-5 = 1.59e-4 of the DEMOD peak (the NCO comes from the GPU's sine unit, within 1.2e-7
                                        of the reference's table entry: what that does to the reference's own loop, doubled); behind a squelch the zeros
                                        are where the model's flag is set, sample by sample
  per call                              meta.squelch_active is the model's flag behind the call's last sample; meta.dcValIf, from the call that holds fm
                                        sample 96000 on, the model's fm_afc behind it: bitwise, but within 2 x 3.35e-8 rad per sample where the AFC follows
                                        pllC's increment (decoder 2, and the AM decoder -- whose DEMOD is exact and whose AFC is not)
  twins                                 channels with equal settings on one stream: PCM and both taps bit-identical after every call
  pieces                                a 70-channel handle whose calls are made in overlapping pieces (FMX_P_CALL_PIECES 1536, and 208 = 13 tiles over
                                        the first 12 000 fm samples): the DEMOD rows of every call's last piece bit-identical to the handle made whole
The call list (32 ragged calls, 100 100 fm samples: prepass_model.CALLS) puts a squelch decision into a call's first tile, a middle tile, the ragged
tail, on a call's last and first sample and into the noise squelch's drain, and the metaData snapshot into a whole tile (variant A) or onto the first
row of a nine-sample call (variant B).  The handles' populations reach every arm of launch_demod_prepass's switch (asserted on the populations).
A failure names kind, channel, call, tile of 16 and row.
"""
import importlib

import numpy as np
import pytest

import prepass_model as pm
import stage_b_model as sb
from test_gpu_stage_b_per_sample import Run

pytestmark = pytest.mark.gpu

M = importlib.import_module("sdr-j-fm_amd").fmx
TAPS = (("z", M.TAP_FM_IQ), ("demod", M.TAP_DEMOD))
HANDLES = pm.handles()
_iq = {}


def programme(name):
    """The shared input of a programme: computed once, never written to."""
    if name not in _iq:
        _iq[name] = pm.programme_iq(name)
        _iq[name].setflags(write=False)
    return _iq[name]


def make(fmx_amd, kinds, prog, batch, pieces=0):
    """A handle with kinds [c] (None: a plain channel) on programme prog [c] -> (handle, iq [streams, n, 2])."""
    names = [p for p in pm.PROGRAMMES if p in prog]
    f = fmx_amd.Fmx(len(kinds), streams=len(names), stream_of_channel=[names.index(p) for p in prog], max_block=max(pm.CALLS + pm.CALLS_B))
    for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 0), (M.P_FM_DECODER, 3)):
        f.set_param(pid, v)
    if batch:
        f.set_param(M.P_SCOPE_TAPS, 1)
        f.set_param(M.P_CALL_PIECES, pieces)
    for c, k in enumerate(kinds):
        if k is not None:
            kd = pm.KINDS[k]
            f.set_param(M.P_FM_DECODER, kd["decoder"], c)
            if kd.get("squelch_mode", 0):
                f.set_param(M.P_SQUELCH_MODE, kd["squelch_mode"], c)
                f.set_param(M.P_SQUELCH_VALUE, kd["squelch_value"], c)
    return f, np.stack([programme(p) for p in names])


def slider(f, kinds):
    def before_call(k):
        if k == pm.SLIDER_CALL:
            for c, kind in enumerate(kinds):
                if kind is not None and "slider" in pm.KINDS[kind]:
                    f.set_param(M.P_SQUELCH_VALUE, pm.KINDS[kind]["slider"], c)
    return before_call


def judge(name, r, c, kind, prog, starts, metas):
    """One probed channel against the model on its own FM_IQ.  -> its figures."""
    t = r.stream(c)
    kd = pm.KINDS[kind]
    tag = "%s, kind %s on %s" % (name, kind, prog)
    m = pm.kind_model(t["z"], kind, starts)
    assert sb.demod_peak(m["raw"]) > 0.1, tag
    exact, sq = kd["decoder"] != 2, kd.get("squelch_mode", 0)
    out = dict(kind=kind, programme=prog)
    if sq:
        out["decisions"] = pm.check_margins(m, tag, sb.demod_peak(m["raw"]) if not exact else None)
        out["flags"] = "".join(str(d[5]) for d in m["decisions"])
        assert out["decisions"] == 10, tag
    if exact:
        pm.check_identical(tag, c, t["demod"], m["demod"], starts)
    else:
        if sq:
            pm.check_flags(tag, c, t["demod"], m, starts)
        out["worst"], out["at"], out["differ"] = pm.check_pll(tag, c, t["demod"], m["demod"], starts, skip=(m["flag"] != 0) if sq else None)
    # per call: the squelch flag behind the call's last sample; the snapshot from the call that holds fm sample SNAP on
    ends = np.concatenate([starts[1:], [t["z"].shape[0]]]) - 1
    snap_call = pm.place(pm.SNAP, np.diff(np.concatenate([starts, [t["z"].shape[0]]])).tolist())[0]
    for k, (active, dc) in enumerate(metas[c]):
        want = int(m["flag"][ends[k]]) if sq else 0
        assert active == want, "%s, channel %d: squelch_active %d behind call %d (fm sample %d), the model's flag is %d" % (tag, c, active, k, ends[k], want)
        if k >= snap_call:
            out["dcValIf off by"] = pm.check_snapshot(tag + ", call %d" % k, c, dc, m, kd["decoder"] > 2)
    return out


def run_handle(fmx_amd, name, calls, calls_fm):
    kinds, prog, probe, twins, batch, arm = HANDLES[name]
    assert pm.prepass_arm(kinds) == arm
    f, iq = make(fmx_amd, kinds, prog, batch)
    metas = {c: [] for c in probe}

    def after_call(k, nj):
        for c in probe:
            mt = f.meta(c)
            metas[c].append((int(mt.squelch_active), np.float32(mt.DcValIf)))

    r = Run(f, iq, probe, twins, calls=calls, taps=TAPS, before_call=slider(f, kinds), after_call=after_call)
    starts = np.asarray(r.starts, np.int64)
    assert r.fm_samples == pm.N_FM and starts.tolist() == pm.call_starts(calls_fm).tolist()
    failed, seen = [], []
    for c in probe:
        try:
            seen.append(judge(name, r, c, kinds[c], prog[c], starts, metas))
            print("[%s] channel %d: %s" % (name, c, seen[-1]))
        except AssertionError as e:
            failed.append(str(e).split("\n")[0][:1200])
    assert not failed, "%s (%s): %d of %d probed channels failed\n  " % (name, arm, len(failed), len(probe)) + "\n  ".join(failed)
    return f, r


@pytest.mark.parametrize("name", list(HANDLES))
def test_kinds(fmx_amd, ol, name):
    """Every handle of prepass_model.handles () -- 1, 1, 3, 3 and 64 channels (small), 65, 70 and 130 (batches: FMX_P_SCOPE_TAPS 1, FMX_P_CALL_PIECES 0) --
    over variant A of the call list: every probed channel against the model (the module's docstring), twins bit-identical.
    Measured on the MI355X: DEMOD bit-identical for every exact kind on every handle; decoder 2 5.7e-5 ... 7.8e-5 of the peak (bound 1.59e-4), 8 ... 15 % of the
    samples differ at all, the worst e.g. in call 22, tile 409, row 15 (handles of 3 and 64) and call 25, tile 41, row 5 (70 and 130); dcValIf bitwise for the
    LUT decoders, 3e-9 ... 9e-9 off for decoders 1 and 2 (bound 6.7e-8); every squelch flag equal.  (First run: the AM kinds' dcValIf was asserted bitwise and
    was 4e-9 ... 9e-9 off -- the AM decoder's AFC is the mean of pllC's increment, whose NCO is the sine unit: the test's mistake, now bounded from the
    reference alone.)"""
    run_handle(fmx_amd, name, pm.CALLS, pm.CALLS_FM)


@pytest.mark.parametrize("name", ["3 pll", "64 all", "70 all"])
def test_snapshot_on_a_call_s_first_row(fmx_amd, ol, name):
    """Variant B of the call list: one early call eleven samples longer, so that the metaData snapshot falls on the first row of a nine-sample
    call (the ragged tail of afc_kernel's slow_rows) and every decision eleven rows later in its call.  Every assertion of test_kinds.
    Measured on the MI355X: as test_kinds (decoder 2 6.4e-5 ... 7.8e-5 of the peak)."""
    run_handle(fmx_amd, name, pm.CALLS_B, pm.CALLS_FM_B)


@pytest.mark.parametrize("pieces, fm_samples", [(1536, None), (208, 12000)])
def test_pieces(fmx_amd, ol, pieces, fm_samples):
    """Two 70-channel handles with equal settings: one makes its calls whole, the other in overlapping pieces of `pieces` fm samples.  After every
    call the DEMOD rows of the last piece (last_fm_samples ()) are bit-identical to the same fm samples of the whole handle: the recurrences do not
    depend on the cut.  On both, RF DC removal is off and FMX_P_FRONT_KERNEL is 1 (otherwise stage A's output depends on the cut in its last bits --
    DESIGN 4.11; the matrix-pipe kernel takes whole 1536-sample tiles only -- and so does all behind it: measured, FM_IQ differs in 39 ... 56 of a
    piece's 1860 rows); FM_IQ of the two handles is asserted equal first.  Measured on the MI355X: up to 6 pieces per call (1536) and 44 (208), every
    DEMOD row of every probed channel equal.  (PCM is not compared: the
    pilot solver's segments move with the cut.)"""
    kinds, prog, probe, twins, batch, arm = HANDLES["70 all"]
    calls, done = [], 0
    for n in pm.CALLS_FM:
        if fm_samples is not None and done + n > fm_samples:
            break
        calls.append(12 * n)
        done += n
    whole, iq = make(fmx_amd, kinds, prog, True, 0)
    cut, _ = make(fmx_amd, kinds, prog, True, pieces)
    for f in (whole, cut):          # what makes stage A's output depend on the cut, off: the RF DC removal works in tiles that begin with the piece (DESIGN
        f.set_param(M.P_DC_REMOVE, 0)               # 4.11), and the matrix-pipe kernel takes whole 1536-sample tiles only and leaves the rest of a piece to kernel 1
        f.set_param(M.P_FRONT_KERNEL, 1)
    before = (slider(whole, kinds), slider(cut, kinds))
    pos, end, counts, failed = 0, 0, [], []
    for k, s in enumerate(calls):
        before[0](k); before[1](k)
        whole.process_host(iq[:, pos:pos + s])
        cut.process_host(iq[:, pos:pos + s])
        pos += s
        nw, nc = whole.last_fm_samples(), cut.last_fm_samples()
        assert nw == s // 12 and 0 < nc <= nw, (k, nw, nc)
        end += nw
        counts.append(cut.last_call_pieces())
        for c in probe:
            a, b = whole.tap(M.TAP_DEMOD, nw, c)[nw - nc:], cut.tap(M.TAP_DEMOD, nc, c)
            bad = pm.differences(b, a)
            za, zb = whole.tap(M.TAP_FM_IQ, nw, c)[nw - nc:], cut.tap(M.TAP_FM_IQ, nc, c)
            zbad = np.flatnonzero((za.view(np.uint32) != zb.view(np.uint32)).any(axis=1))
            assert zbad.size == 0, "pieces of %d, channel %d, call %d: the two handles' FM_IQ differ in %d rows: the comparison has no common input" % (pieces, c, k, zbad.size)
            if bad.size:
                failed.append("kind %s, channel %d, call %d (%d pieces): %d of the last piece's %d DEMOD rows differ from the whole call's, the first at %s; FM_IQ differs in %d rows%s" % (
                    kinds[c], c, k, counts[-1], bad.size, nc, pm.locate(end - nc + int(bad[0]), pm.call_starts(pm.CALLS_FM)), zbad.size,
                    (", the first at row %d of the piece" % int(zbad[0])) if zbad.size else ""))
    print("[pieces of %d] pieces per call: %s" % (pieces, counts))
    assert max(counts) > 1, "no call was made in pieces"
    assert not failed, "pieces of %d: %d (channel, call) pairs differ\n  " % (pieces, len(failed)) + "\n  ".join(failed[:40])

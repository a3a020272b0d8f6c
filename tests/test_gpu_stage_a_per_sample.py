"""Stage A sample by sample against the float64 model of tests/stage_a_model.py: every kernel (front_kernel folded, split in time and with its
twins; front4_kernel with real and with complex taps; the block machines), every sample of every call.

FMX_TAP_FM_IQ is read after EVERY call -- the ring `delay_fm` back, zero in front of the stream -- and concatenated; the model knows nothing of
the library's fold, alignment, delay or gain and must reproduce the read-out from the reference's filters alone.  Bounds (stage_a_model.py, relative
to each channel's own peak, from the oracle's distance to the same model as tests/test_stage_a_model_cpu.py measures it on the CPU -- never from
what the kernels give):
  input filter on   2 x 1.31e-6 = 2.62e-6
  input filter off  2 x 4.10e-7 = 8.2e-7
Channels whose RF DC value the library applies behind the filter (no oscillator on front_kernel, every channel of the matrix-pipe kernels) are held
to the model's second form, the others to the reference's order; the remainder of a matrix-pipe call, which front_kernel makes, to front_kernel's form.
Every case prints its worst sample, where it fell (call, tile, column) and its bound.
"""
import importlib

import numpy as np
import pytest

import stage_a_model as sa
from test_gpu_worst_sample import RAGGED

pytestmark = pytest.mark.gpu

M = importlib.import_module("sdr-j-fm_amd").fmx
T = sa.TILE
PID = dict(bw=M.P_BANDWIDTH, att_l=M.P_ATTENUATION_L, att_r=M.P_ATTENUATION_R, lo=M.P_LOCAL_OSCILLATOR, dc_remove=M.P_DC_REMOVE)


def handle(fmx_amd, nch, stream_of, max_block, kernel=None, restarts=2, parts=None, bw=165000, rate=2304000):
    f = fmx_amd.Fmx(nch, streams=max(stream_of) + 1, stream_of_channel=stream_of, max_block=max_block, inputRate=rate)
    for pid, v in ((M.P_BANDWIDTH, bw), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 0)):
        f.set_param(pid, v)
    for pid, v in ((M.P_FILTER_RESTARTS, restarts), (M.P_FRONT_KERNEL, kernel), (M.P_FRONT_PARTS, parts)):
        if v is not None:
            f.set_param(pid, v)
    return f


def settings(f, kinds):
    """kinds: per channel a dict of bw / att_l / att_r / lo / dc_remove."""
    for c, kd in enumerate(kinds):
        for k, v in kd.items():
            f.set_param(PID[k], v, c)


class Run:
    """The calls of one case: FMX_TAP_FM_IQ of every probed channel after every call, the kernel that made each call asserted."""

    def __init__(self, f, iq, calls, probe, kernel, before_call=None, raw=None, twins=None):
        self.z = {c: [] for c in probe}
        self.starts, pos, j = [], 0, 0
        for k, s in enumerate(calls):
            if before_call is not None:
                before_call(k)
            if raw is None:
                f.process_host(iq[:, pos:pos + s])
            else:
                f.process_host_raw(iq[:, pos:pos + s], *raw)
            pos += s
            want = kernel(k) if callable(kernel) else kernel
            assert f.last_front_kernel() == want, (k, s, f.last_front_kernel(), want)
            nj = f.last_fm_samples()
            self.starts.append(j)
            for c in probe:
                self.z[c].append(f.tap(M.TAP_FM_IQ, nj, c))
            for group in (twins or []):                           # channels that must be bit-identical
                first = f.tap(M.TAP_FM_IQ, nj, group[0])
                for c in group[1:]:
                    assert np.array_equal(f.tap(M.TAP_FM_IQ, nj, c), first), (k, c)
            j += nj
        self.fm_samples = j

    def stream(self, c):
        return np.concatenate(self.z[c])


def remainder_mask(calls, D, active=None):
    """True for the fm samples whose newest input lies in a matrix-pipe call's remainder (what is left of a call behind its whole tiles goes
    to front_kernel); active: per call, whether the channel takes front_kernel's per-sample pass in it (default: in every call)."""
    n = sum(calls)
    rem = np.zeros(n, bool)
    pos = 0
    for k, s in enumerate(calls):
        rem[pos + s // T * T:pos + s] = True if active is None else bool(active[k])
        pos += s
    nj = 12 * np.arange(n // 12, dtype=np.int64) + 11 - D.latency
    return np.where(nj >= 0, rem[np.clip(nj, 0, n - 1)], False)


def model(D, x, calls, kd, form, remainder=None):
    """kd: the channel's settings (a value, or a list per call); form "front" / "behind"; with `remainder` (remainder_mask) the channel takes
    the reference's order there (front_kernel's per-sample pass: an oscillator or a balance) and the second form on the tiles."""
    kw = dict(lo=kd.get("lo", 0), att=(kd.get("att_l", 1.0), kd.get("att_r", 1.0)), dc_remove=kd.get("dc_remove", 1))
    if remainder is not None and form == "behind" and (kw["att"] != (1.0, 1.0) or kw["lo"] != 0):
        return sa.stage_a(D, x, calls, form="mixed", behind=~remainder, **kw)
    return sa.stage_a(D, x, calls, form=form, **kw)


def judge(name, r, refs, bound, floor=0.0, decim=12):
    """refs: channel -> model.  Every channel relative to its own peak; prints the worst channel's line, checks every channel."""
    worst = None
    for c, ref in refs.items():
        z = r.stream(c)
        assert z.shape[0] == ref.shape[0], (c, z.shape, ref.shape)
        w = sa.compare(z, ref, r.starts, decim=decim)
        assert w.scale > floor, (c, w.scale)
        if worst is None or w.rel > worst[1].rel:
            worst = (c, w)
    print("\n[%s] worst of channels %s: channel %d: %s (bound %.2e)" % (name, sorted(refs), worst[0], worst[1], bound))
    sa.check(worst[1], bound, "%s, channel %d" % (name, worst[0]))
    return worst


def streams_of(ol, n, dcs, **kw):
    return np.stack([ol.synth_iq(n, leftHz=1000.0 + 370.0 * s, rightHz=400.0 + 230.0 * s, dcI=d[0], dcQ=d[1], **kw) for s, d in enumerate(dcs)])


# ------------------------------------------------------------------------------------------------ a. front_kernel, folded
A_KINDS = [dict(), dict(lo=2500), dict(lo=-4000), dict(att_l=0.9, att_r=1.1), dict(dc_remove=0), dict(bw=130000), dict(), dict()]
A_STREAM = [0, 1, 0, 1, 0, 1, 2, 3]
A_DC = [(0.0, 0.0), (0.004, -0.003), (0.02, -0.015), (0.2, -0.1)]


@pytest.mark.parametrize("filter_on", [True, False], ids=["filter on", "filter off"])
def test_a_front_kernel_folded(fmx_amd, ol, filter_on):
    """front_kernel on the folded filters (FMX_P_FRONT_KERNEL = 1, FMX_P_FILTER_RESTARTS = 2), calls of 1, 12 and 13 samples among the ragged ones
    (off the 12-sample grid).  Six channels on two streams, stream 1 with a DC offset of (0.004, -0.003): plain, oscillators 2500 (period 4608) and
    -4000, a balance of 0.9 / 1.1, DC removal off, bandwidth 130 000 (a second tap set); a stream with (0.02, -0.015), whose RfDC value reaches
    0.0068 in these 0.42 s, and one with (0.2, -0.1), which crosses the limiter 51 ms into the stream, inside the fourth call.  With the input filter
    off: 37 taps, the fir_rows<4> path.
    Measured on the MI355X: 3.2e-7 of the peak (bound 2.62e-6) with the filter on, 2.4e-7 (bound 8.2e-7) with it off, both on the balance channel."""
    calls = RAGGED * 2
    n = sum(calls)
    iq = streams_of(ol, n, A_DC)
    kinds = [dict(kd) for kd in A_KINDS]
    if not filter_on:
        for kd in kinds:
            kd.pop("bw", None)
    f = handle(fmx_amd, len(kinds), A_STREAM, max(calls), kernel=1, bw=165000 if filter_on else 0)
    settings(f, kinds)
    r = Run(f, iq, calls, range(len(kinds)), 1)
    assert r.fm_samples == n // 12
    L = ol.oracle()
    refs = {}
    for c, kd in enumerate(kinds):
        D = sa.Design(L, 2304000, kd.get("bw", 165000) if filter_on else 0)
        per_sample = "lo" in kd or "att_l" in kd
        refs[c] = model(D, iq[A_STREAM[c]], calls, kd, "front" if per_sample else "behind")
    judge("a, front_kernel folded, input filter %s" % ("on" if filter_on else "off"), r, refs, sa.STAGE_A_BOUND_ON if filter_on else sa.STAGE_A_BOUND_OFF, 1.0)


# ------------------------------------------------------------------------------------------------ b. the same, split in time
def test_b_front_kernel_split_in_time(fmx_amd, ol):
    """FMX_P_FRONT_PARTS = 5: every channel's call is made by five workgroups, each with a warm-up tile; three channels (plain on a stream with a DC
    offset, an oscillator, a balance), calls of 40 tiles, 33 tiles + 480, 27 tiles - 480, then what pushes them out of the filter's delay.
    Measured on the MI355X: 2.6e-7 of the peak (bound 2.62e-6)."""
    calls = [40 * T, 33 * T + 480, 27 * T - 480] + sa.FLUSH_CALLS
    iq = streams_of(ol, sum(calls), [(0.004, -0.003)])
    kinds = [dict(), dict(lo=2500), dict(att_l=0.9, att_r=1.1)]
    f = handle(fmx_amd, 3, [0, 0, 0], max(calls), kernel=1, parts=5)
    settings(f, kinds)
    r = Run(f, iq, calls, range(3), 1)
    D = sa.Design(ol.oracle(), 2304000, 165000)
    refs = {c: model(D, iq[0], calls, kd, "front" if kd else "behind") for c, kd in enumerate(kinds)}
    judge("b, front_kernel split in five parts", r, refs, sa.STAGE_A_BOUND_ON, 1.0)


# ------------------------------------------------------------------------------------------------ c. twins
@pytest.mark.parametrize("filter_on", [True, False], ids=["filter on", "filter off"])
@pytest.mark.parametrize("rate", [2880000, 1920000, 192000])
def test_c_twins_at_other_input_rates(fmx_amd, ol, rate, filter_on):
    """The rates the reference decimates by 12 (2 880 000), by 6 (1 920 000: two workgroups per channel, one per output phase) and not at all
    (192 000: twelve), test_input_rates' oscillator and DC offset, five calls -- and, with the input filter on, as many more as push them out
    of its delay --, one channel (an oscillator: the reference's order).
    Measured on the MI355X, filter on / off: 2.9e-7 / 2.0e-7 (2 880 000), 2.6e-7 / 1.9e-7 (1 920 000), 5.4e-7 / 1.4e-7 (192 000); bounds 2.62e-6 / 8.2e-7."""
    decim = 1 if rate // 192000 <= 1 else 6 * ((rate // 6) // 192000)
    block = 16384 * 5 if decim > 1 else 16384
    lo = 30000 if decim > 1 else 3000
    bw = (165000 if decim > 1 else 150000) if filter_on else 0
    calls = [block] * 5
    if filter_on:
        calls = calls + [block] * -(-(sa.IN_DELAY + 1) // block)          # (what pushes the five calls out of the filter's 65285 samples of delay)
    iq = ol.synth_iq(sum(calls), offsetHz=float(lo), dcI=0.004, dcQ=-0.003)[None]
    f = handle(fmx_amd, 1, [0], block, restarts=2, bw=bw, rate=rate)
    f.set_param(M.P_LOCAL_OSCILLATOR, lo)
    r = Run(f, iq, calls, [0], 1)
    D = sa.Design(ol.oracle(), rate, bw)
    assert D.decim == decim and r.fm_samples == sum(calls) // decim
    judge("c, input rate %d (decimation %d), input filter %d" % (rate, decim, bw), r, {0: model(D, iq[0], calls, dict(lo=lo), "front")},
          sa.STAGE_A_BOUND_ON if filter_on else sa.STAGE_A_BOUND_OFF, 0.4, decim)


# ------------------------------------------------------------------------------------------------ d. front4_kernel, real taps
D_AMPS = [30.0, 0.5, 1e-6]
D_KINDS = [dict(), dict(), dict(), dict(att_l=0.9, att_r=1.1), dict(dc_remove=0)]


@pytest.mark.parametrize("nch", [5, 2])
def test_d_matrix_pipe_real_taps(fmx_amd, ol, nch):
    """front4_kernel (FMX_P_FRONT_KERNEL = 3, FMX_P_FILTER_RESTARTS = 2): five channels -- the last workgroup holds one -- on three streams at carrier
    amplitudes 30, 0.5 and 1e-6 with DC offsets scaled alike, a balance of 0.9 / 1.1 on channel 3, DC removal off on channel 4; and two channels, one
    workgroup.  Calls of 1, 5, 6, 7 and 13 tiles (fewer tiles than waves; the ring of six tiles wrapping), 7 tiles + 600 samples and 6 tiles - 600
    (the remainder handed to front_kernel and back), then two calls that push them out of the filter's delay.  Every channel against the second form;
    the balance channel's remainders against the reference's order, which front_kernel's per-sample pass follows.
    Measured on the MI355X: 2.8e-7 ... 4.4e-7 of the peak on the plain channels; 2.54e-6 on the balance channel, in the first column of the 7-tile call's
    remainder -- the hand-over of the raw history to the per-sample pass, 1 ... 2.5e-6 for thirteen columns, 3e-7 elsewhere.  Bound 2.62e-6."""
    calls = sa.FRONT4_CALLS + sa.FLUSH_CALLS
    n = sum(calls)
    iq = np.stack([ol.synth_iq(n, carrierAmp=a, leftHz=500.0 + 250 * k, rightHz=900.0 + 150 * k, dcI=0.004 * a, dcQ=-0.003 * a) for k, a in enumerate(D_AMPS)])
    kinds = D_KINDS[:nch]
    iq = iq[:min(nch, 3)]
    f = handle(fmx_amd, nch, [c % 3 for c in range(nch)], max(calls), kernel=3, parts=1)
    settings(f, kinds)
    r = Run(f, iq, calls, range(nch), 3)
    D = sa.Design(ol.oracle(), 2304000, 165000)
    rem = remainder_mask(calls, D)
    assert rem.sum() == (600 + 936) // 12
    refs = {c: model(D, iq[c % 3], calls, kd, "behind", rem) for c, kd in enumerate(kinds)}
    judge("d, front4_kernel with real taps, %d channels" % nch, r, refs, sa.STAGE_A_BOUND_ON, 4e-6)


@pytest.mark.parametrize("fmt", ["u8", "s8", "s16"])
def test_d_matrix_pipe_raw_formats(fmx_amd, ol, fmt):
    """U8, S8 and S16 / 2048 through front4_kernel on the same calls, converted by include/fmx.h's rules, the formats' extreme codes in the stream
    (in the first call's tile, in the middle of the 13-tile call and in a remainder).
    Measured on the MI355X: 3.3e-7 (U8), 3.1e-7 (S8), 1.7e-7 (S16) of the peak; bound 2.62e-6."""
    calls = sa.FRONT4_CALLS + sa.FLUSH_CALLS
    n = sum(calls)
    x = ol.synth_iq(n)
    if fmt == "u8":
        raw, lo_, hi_, args = np.clip(np.round(x * 100.0 + 127.4), 0, 255).astype(np.uint8), 0, 255, (M.IQ_U8,)
    elif fmt == "s8":
        raw, lo_, hi_, args = np.clip(np.round(x * 100.0 + 0.4), -128, 127).astype(np.int8), -128, 127, (M.IQ_S8,)
    else:
        raw, lo_, hi_, args = np.clip(np.round(x * 1500.0 + 9.0), -32768, 32767).astype(np.int16), -32768, 32767, (M.IQ_S16, 2048.0)
    for k, p in enumerate((700, 25 * T + 5, sum(calls[:5]) + 7 * T + 300)):
        raw[p] = (lo_, hi_) if k % 2 == 0 else (hi_, lo_)
        raw[p + 1] = (hi_, hi_)
    f = handle(fmx_amd, 1, [0], max(calls), kernel=3, parts=1)
    r = Run(f, raw[None], calls, [0], 3, raw=args)
    D = sa.Design(ol.oracle(), 2304000, 165000)
    code = dict(u8=sa.IQ_U8, s8=sa.IQ_S8, s16=sa.IQ_S16)[fmt]
    judge("d, front4_kernel, raw %s" % fmt, r, {0: model(D, sa.convert(raw, code, 2048.0), calls, dict(), "behind")}, sa.STAGE_A_BOUND_ON, 1.0)


# ------------------------------------------------------------------------------------------------ e. level step
def test_e_level_step_against_the_local_scale(fmx_amd, ol):
    """test_a_level_step_between_two_tiles' input -- 2^-10, a step to 2^10 in the middle of a tile and back -- through front4_kernel, every sample
    against the model relative to the LOCAL scale: the largest model magnitude within the filter's length.  The oracle's transform filter is only
    accurate to its block's scale and cannot set a local bound; the level is the worst local-scale sample of the f32 fold restated on the host on
    the same input, doubled.
    Measured on the MI355X: 4.5e-7 of the local scale; the host's f32 fold 7.3e-7, bound 1.46e-6."""
    calls = [40 * T] * 4
    n = sum(calls)
    g = np.full(n, 2.0 ** -10, np.float32)
    g[13 * T + 700:55 * T + 100] = np.float32(2.0 ** 10)
    iq = (ol.synth_iq(n) * g[:, None])[None]
    f = handle(fmx_amd, 5, [0] * 5, max(calls), kernel=3, parts=1)
    f.set_param(M.P_DC_REMOVE, 0)
    r = Run(f, iq, calls, [0, 4], 3)
    D = sa.Design(ol.oracle(), 2304000, 165000)
    ref = sa.stage_a(D, iq[0], calls, dc_remove=0, direct=True)        # (plain sums: exact to every output's own scale)
    mag = np.maximum(np.abs(ref.real), np.abs(ref.imag))
    local = np.maximum.reduce([np.roll(mag, k) for k in range(-2, 27)])
    assert (local > 0).sum() > 12000 and float(mag.max()) > 1000 * float(np.median(mag[local > 0]))
    vr, vi = sa.premix32(D, iq[0], dc_remove=0)
    level = sa.compare(sa.folded_f32(D, vr, vi), ref, r.starts, local=local)
    print("\n[e, level step] the f32 fold on the host: %s" % level)
    assert np.array_equal(r.stream(0), r.stream(4))
    w = sa.compare(r.stream(0), ref, r.starts, local=local)
    print("[e, level step, front4_kernel] %s (bound %.2e of the local scale)" % (w, 2.0 * level.rel))
    sa.check(w, 2.0 * level.rel, "e, level step")


# ------------------------------------------------------------------------------------------------ f. the complex-tap variant
F_KINDS = [dict(lo=0), dict(lo=200000), dict(lo=-400000), dict(lo=2500), dict(lo=200000, att_l=0.9, att_r=1.1), dict(lo=-400000, dc_remove=0),
           dict(lo=2500, bw=130000)]
F_DC = [(0.0, 0.0), (0.006, -0.004), (-0.02, 0.015)]


def test_f_matrix_pipe_complex_taps(fmx_amd, ol):
    """fmx_front4lo.hip (FMX_P_FRONT_KERNEL = 3 on a handle with oscillators): the kinds and streams of
    test_matrix_pipe_input_filter_with_local_oscillators -- carriers at 0, +200 kHz, -400 kHz and +2.5 kHz, oscillators 0, 200 000, -400 000, 2500,
    a balance, DC removal off, bandwidth 130 000, DC offsets on two of three streams --, calls of whole tiles and of tiles +- 480, oscillator 200 000
    switched off in front of the fourth call and channel 0's switched to 2500 in front of the fifth.
    Measured on the MI355X: 4.1e-7 ... 9.5e-7 of the peak on channels 1 - 6; 2.59e-6 on channel 0 in the first column behind its oscillator's switch-on (the
    same hand-over as case d's: thirteen columns at 1 ... 2.6e-6, 2e-7 elsewhere).  Bound 2.62e-6."""
    calls = [8 * T, 7 * T + 480, 6 * T - 480, 8 * T, 8 * T] + sa.FLUSH_CALLS
    n = sum(calls)
    iq = np.zeros((3, n, 2), np.float32)
    for s in range(3):
        acc = np.zeros((n, 2), np.float64)
        for k, o in enumerate([0.0, 200000.0, -400000.0, 2500.0]):
            acc += ol.synth_iq(n, offsetHz=o, leftHz=300.0 + 170 * k + 40 * s, rightHz=800.0 + 90 * k + 25 * s, carrierAmp=0.2)
        iq[s] = (acc + np.array(F_DC[s])).astype(np.float32)
    stream_of = [c % 3 for c in range(7)]
    f = handle(fmx_amd, 7, stream_of, max(calls), kernel=3, parts=1)
    settings(f, F_KINDS)
    events = {3: (1, 0), 4: (0, 2500)}                 # call -> (channel, oscillator)

    def before(k):
        if k in events:
            f.set_param(M.P_LOCAL_OSCILLATOR, events[k][1], events[k][0])
    r = Run(f, iq, calls, range(7), 3, before_call=before)
    L = ol.oracle()
    refs = {}
    for c, kd in enumerate(F_KINDS):
        kd = dict(kd)
        for k, (ch, v) in events.items():
            if ch == c:
                kd["lo"] = [kd["lo"] if i < k else v for i in range(len(calls))]
        D = sa.Design(L, 2304000, kd.get("bw", 165000))
        lo_of_call = kd["lo"] if isinstance(kd["lo"], list) else [kd["lo"]] * len(calls)
        per_sample = [v != 0 or "att_l" in kd for v in lo_of_call]          # (front_kernel's pass over a remainder: the reference's order)
        refs[c] = sa.stage_a(D, iq[stream_of[c]], calls, lo=kd["lo"], att=(kd.get("att_l", 1.0), kd.get("att_r", 1.0)), dc_remove=kd.get("dc_remove", 1),
                             form="mixed", behind=~remainder_mask(calls, D, per_sample))
    judge("f, front4_kernel with complex taps", r, refs, sa.STAGE_A_BOUND_ON, 0.5)


# ------------------------------------------------------------------------------------------------ g. block machines
def test_g_block_machines(fmx_amd, ol):
    """A default three-channel handle (no FMX_P_FILTER_RESTARTS, input filter on): pre_kernel in the reference's order, the input filter as the
    reference's block machine, front_kernel's decimators; ragged calls, an oscillator on channel 1, a DC offset on the stream.
    Measured on the MI355X: 3.5e-7 of the peak (bound 2.62e-6)."""
    calls = RAGGED * 2
    iq = streams_of(ol, sum(calls), [(0.004, -0.003)])
    kinds = [dict(), dict(lo=2500), dict(att_l=0.9, att_r=1.1)]
    f = handle(fmx_amd, 3, [0, 0, 0], max(calls), restarts=None)
    settings(f, kinds)
    r = Run(f, iq, calls, range(3), 1)
    D = sa.Design(ol.oracle(), 2304000, 165000)
    judge("g, block machines", r, {c: model(D, iq[0], calls, kd, "front") for c, kd in enumerate(kinds)}, sa.STAGE_A_BOUND_ON, 1.0)


# ------------------------------------------------------------------------------------------------ h. the automatic choice at batch size
def test_h_automatic_choice_at_batch_size(fmx_amd, ol):
    """600 channels on 4 streams, test_matrix_pipe_input_filter_is_linear_at_any_level's calls and streams at amplitude 1.0, the automatic choice
    (asserted: the matrix-pipe kernel), then two calls that push them out of the filter's delay: every channel bit-identical to its stream's first after every call, four channels -- one per stream, in
    different workgroups -- modelled over all calls.
    Measured on the MI355X: 4.0e-7 of the peak (bound 2.62e-6)."""
    nch, nst, amp = 600, 4, 1.0
    calls = [49152 * 2, 49152, 49152 * 2 + 600, 49152 - 600] + sa.FLUSH_CALLS          # (the last two push the four out of the filter's delay)
    n = sum(calls)
    iq = np.stack([ol.synth_iq(n, carrierAmp=amp, leftHz=500.0 + 250 * k, rightHz=900.0 + 150 * k, dcI=0.004 * amp * (k & 1), dcQ=-0.003 * amp * (k >> 1),
                               noiseSeed=7 + k, noiseSigma=0.001 * amp * k) for k in range(nst)])
    f = handle(fmx_amd, nch, [c % nst for c in range(nch)], max(calls), restarts=None)
    probe = [0, 149, 298, 599]
    assert sorted(c % nst for c in probe) == [0, 1, 2, 3]
    r = Run(f, iq, calls, probe, 3, twins=[list(range(s, nch, nst)) for s in range(nst)])
    D = sa.Design(ol.oracle(), 2304000, 165000)
    judge("h, 600 channels, automatic choice", r, {c: model(D, iq[c % nst], calls, dict(), "behind") for c in probe}, sa.STAGE_A_BOUND_ON, 1.0)

"""Stage C, the second converter and the RDS front end, frame by frame against the float64 models of tests/f64_models.py.

The parity tests assert an RMS of the PCM against the oracle (1e-5); an error of 1e-4 on one frame in every 1792 is 2.4e-6 rms and
passes them.  Here every stage is isolated on identical inputs: the model reads the very f32 samples the kernel read (the d ring through
FMX_TAP_PRE_RESAMPLER, collected after every call; FMX_TAP_DEMOD and FMX_TAP_PILOT_PHASE for the RDS path) and the coefficients the
kernels run with (fmx_get_taps), and EVERY frame of every checked channel is compared -- the first call's, the fade's, the frames behind
every call boundary.  Call lengths are ragged, so call boundaries fall on every residue of audio_fft_kernel's 256-frame tiles and
1792-frame blocks and of the resampler's 192-sample blocks; a failure names its seam (f64_models.compare).

Bounds (f64_models.py, relative to the output's own peak, derived from the reference's distance to the same models as
tests/test_f64_models_cpu.py measures it on the CPU -- never from what the kernels give):
  stage C           2 x 1.21e-6 = 2.42e-6   (oracle overlap-add audio filter + resampler against float64; 2 for another summation order)
  second converter  2.42e-6 + 5.84e-7        (plus the converter's own)
  RDS baseband      2 x 1.06e-6 = 2.12e-6
"""
import importlib

import numpy as np
import pytest

import f64_models as fm

pytestmark = pytest.mark.gpu

M = importlib.import_module("sdr-j-fm_amd").fmx

# fmx_internal.h: AUDIO_DELAY + C_MAX_TAPS = 7436 + 883 fm samples of history, PROMO_TAIL_AU = 3 (8192 - 756) + 1200 for a handle above
# OLA_MAX_CH = 64 channels, C_TILE = 256; fmx_api.hip fmx_create: the d ring holds that, a call (max_block / 12 + 2) and 192 + 4 C_TILE more,
# rounded up to a power of two
RAGGED = [50000, 12, 13, 99999, 230400, 1, 100000]          # test_block_size_invariance's


def d_ring_length(max_block, channels):
    need = max(7436 + 883, 3 * (8192 - 756) + 1200 + 8 if channels > 64 else 0) + max_block // 12 + 2 + 192 + 4 * 256
    return 1 << int(np.ceil(np.log2(need)))


def defaults(f, folded=True, lf=15000):
    for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, lf), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 0), (M.P_FM_DECODER, 3)):
        f.set_param(pid, v)
    if folded:
        f.set_param(M.P_FILTER_RESTARTS, 2)


def programmes(ol, n, streams, **kw):
    return np.stack([ol.synth_iq(n, leftHz=1000.0 + 370.0 * s, rightHz=400.0 + 230.0 * s, **kw) for s in range(streams)])


class Run:
    """The calls of one case: the PCM of every call, the pre-resampler stream of every checked channel, where every call begins."""

    def __init__(self, f, iq, sizes, channels, before_call=None, twins=None):
        self.pcm = {c: [] for c in channels}
        self.x = {c: [] for c in channels}
        self.j_starts, self.frame_starts, self.second = [], [], []
        pos = j = frames = 0
        for k, s in enumerate(sizes):
            if before_call is not None:
                before_call(k)
            self.j_starts.append(j); self.frame_starts.append(frames)
            want = f.frames_for(s)
            p = f.process_host(iq[:, pos:pos + s])
            pos += s
            assert p.shape[1] == want
            nj = f.last_fm_samples()
            self.second.append(f.last_second_group())
            for c in channels:
                self.pcm[c].append(p[c].copy())
                self.x[c].append(f.tap(M.TAP_PRE_RESAMPLER, nj, c))
            for group in (twins or []):                       # channels that must be bit-identical
                assert (p[group] == p[group[0]]).all(), (k, group[:3])
            j += nj; frames += p.shape[1]
        self.fm_samples, self.frames = j, frames
        assert pos == sum(sizes) and j == pos // 12

    def stream(self, c):
        return np.concatenate(self.x[c]), np.concatenate(self.pcm[c])


def report(name, w, bound):
    print("\n[%s] %s (bound %.2e of the peak)" % (name, w, bound))


# ------------------------------------------------------------------------------------------------ stage C
@pytest.mark.parametrize("sizes", [RAGGED * 3, [10007] * 120], ids=["ragged", "10007s"])
def test_stage_c_single_receiver_folded(fmx_amd, ol, sizes):
    """One receiver on the folded filters (FMX_P_FILTER_RESTARTS = 2), ragged calls, every frame against
    fade (m) gain sum_k g[k] x[4 m + 3 - 7436 - k], g = fmx_get_taps (2).  The d ring (32768 entries for calls of up to 230400 samples, 16384
    for calls of 10007) wraps more than twice.
    Reference alone (CPU): 1.21e-6 of the peak; bound 2.42e-6.  Measured on the MI355X: 4.6e-7 (21 ragged calls), 2.4e-7 (120 calls of 10007)."""
    n = sum(sizes)
    iq = ol.synth_iq(n)[None]
    f = fmx_amd.Fmx(1, max_block=max(sizes))
    defaults(f)
    r = Run(f, iq, sizes, [0])
    ring = d_ring_length(max(sizes), 1)
    assert ring == (32768 if max(sizes) == 230400 else 16384) and r.fm_samples >= 2 * ring + 1000, (ring, r.fm_samples)
    x, pcm = r.stream(0)
    g = f.taps(2)
    assert g.size == 883 and pcm.shape[0] == fm.frames_of(r.fm_samples) > 24000
    ref = fm.stage_c_folded(x, g, fm.gain_lr(-6.0, 0))
    w = fm.compare(pcm, ref, r.frame_starts)
    report("stage C, one receiver, folded, %d calls" % len(sizes), w, fm.STAGE_C_BOUND)
    assert w.scale > 0.1
    fm.check(w, fm.STAGE_C_BOUND, "stage C single receiver")


@pytest.mark.parametrize("nch", [70, 600, 1100])
def test_stage_c_batches(fmx_amd, ol, nch):
    """Batches on four programmes with a balance of -30 (L and R gains differ): the first and the last channel, the two on either side of
    the channel-group boundary (1100 channels run stages B and C as two groups: asserted) and a stride through the rest, every frame;
    channels on the same stream bit-identical call by call.
    Reference alone (CPU): 1.21e-6 of the peak; bound 2.42e-6.  Measured on the MI355X: 3.2e-7 (70), 3.1e-7 (600), 3.1e-7 (1100 channels)."""
    sizes = [230400, 100000, 99999, 13, 150001, 230400, 50000]
    iq = programmes(ol, sum(sizes), 4)
    f = fmx_amd.Fmx(nch, streams=4, stream_of_channel=[c % 4 for c in range(nch)], max_block=max(sizes))
    defaults(f)
    f.set_param(M.P_SOUND_BALANCE, -30)
    probe = sorted(set([0, 1, 2, 3, nch - 1] + list(range(5, nch, max(nch // 7, 1))) + ([767, 768] if nch == 1100 else [])))
    twins = [np.arange(s, nch, 4) for s in range(4)]
    r = Run(f, iq, sizes, probe, twins=twins)
    if nch == 1100:
        assert max(r.second) == 332, r.second             # 768 + 332: the boundary lies between channels 767 and 768
    else:
        assert max(r.second) == 0
    g = f.taps(2)
    gain = fm.gain_lr(-6.0, -30)
    assert gain[0] != gain[1]
    worst = None
    for c in probe:
        x, pcm = r.stream(c)
        w = fm.compare(pcm, fm.stage_c_folded(x, g, gain), r.frame_starts)
        assert w.scale > 0.1
        if worst is None or w.rel > worst[1].rel:
            worst = (c, w)
    report("stage C, %d channels (groups %s), worst of channels %s: channel %d" % (nch, r.second, probe, worst[0]), worst[1], fm.STAGE_C_BOUND)
    fm.check(worst[1], fm.STAGE_C_BOUND, "stage C batch of %d, channel %d" % (nch, worst[0]))


@pytest.mark.parametrize("lf,ntaps", [(15000, 883), (12000, 883), (0, 128)])
def test_stage_c_lf_cutoff(fmx_amd, ol, lf, ntaps):
    """FMX_P_LF_CUTOFF at 15000, at 12000 and off (the folded filter is then the 128-tap resampler alone, without the 7436-sample delay).
    Reference alone (CPU): 1.21e-6 of the peak; bound 2.42e-6.  Measured on the MI355X: 3.2e-7, 2.7e-7, 3.4e-7."""
    sizes = RAGGED + [30011, 150000]
    iq = ol.synth_iq(sum(sizes))[None]
    f = fmx_amd.Fmx(1, max_block=max(sizes))
    defaults(f, lf=lf)
    r = Run(f, iq, sizes, [0])
    x, pcm = r.stream(0)
    g = f.taps(2)
    assert g.size == ntaps
    if lf > 0:                                                 # the taps are the oracle's design at this cut-off
        h = np.zeros(fm.AUDIO_TAPS, np.float32)
        ol.oracle().fmo_lowpass_kernel(fm.AUDIO_TAPS, lf, 192000, ol.fptr(h))
        assert np.abs(g - np.convolve(h.astype(np.float64), f.taps(3).astype(np.float64))).max() < 1e-8
    w = fm.compare(pcm, fm.stage_c_folded(x, g, fm.gain_lr(-6.0, 0), lf_on=lf > 0), r.frame_starts)
    report("stage C, lf cut-off %d (%d taps)" % (lf, ntaps), w, fm.STAGE_C_BOUND)
    assert w.scale > 0.1
    fm.check(w, fm.STAGE_C_BOUND, "stage C at lf cut-off %d" % lf)


@pytest.mark.parametrize("nch", [1, 600])
def test_stage_c_gain_changes_between_calls(fmx_amd, ol, nch):
    """Volume and balance changed between calls (gain_fix_kernel), the next call starting on the resampler's 192-sample grid and off it:
    e_0 = 4 M0 + 3 - J0 of the kernel's comment is 3, -100 and -188 for the three calls behind a change.  The two-step model -- audio
    low-pass, gain as a function of the fm sample (it steps at the call's first sample), resampler -- on every frame.  600 channels on four
    streams in three kinds: volume and balance change, balance alone changes, nothing changes (their correction must be zero).
    Reference alone (CPU): 1.21e-6 of the peak; bound 2.42e-6.  Measured on the MI355X: 5.0e-7 (1 channel), 6.6e-7 (600 channels, frame 13 of the
    call that starts at e_0 = -100)."""
    sizes = [230400] * 6 + [12 * (192 * 50 + 103), 12 * (192 * 50 + 88), 100000, 50000]
    streams = 4 if nch > 1 else 1
    iq = programmes(ol, sum(sizes), streams)
    f = fmx_amd.Fmx(nch, streams=streams, stream_of_channel=[c % streams for c in range(nch)], max_block=max(sizes))
    defaults(f)
    kinds = 3 if nch > 1 else 1
    # (volume dB, balance) per kind from call k on
    plan = {6: [(-10.5, 30), (-6.0, -20), None], 7: [(-3.0, -40), (-6.0, 50), None], 8: [(-6.0, 0), None, None]}
    setting = {kd: [(0, (-6.0, 0))] for kd in range(kinds)}       # per kind: (call, (volume, balance))

    def before(k):
        for kd in range(kinds):
            s = plan.get(k, [None] * 3)[kd]
            if s is None:
                continue
            for c in range(kd, nch, kinds):
                f.set_param(M.P_VOLUME_DB, s[0], c); f.set_param(M.P_SOUND_BALANCE, s[1], c)
            setting[kd].append((k, s))
    probe = [0] if nch == 1 else [0, 1, 2, 3, 4, 5, 298, 299, 300, 597, 598, 599]
    r = Run(f, iq, sizes, probe, before_call=before)
    assert [3 - r.j_starts[k] % 192 for k in (6, 7, 8)] == [3, -100, -188]
    assert r.frame_starts[6] > fm.FADE_FRAMES                    # (the changes lie behind the fade: nothing scales the correction down)
    h = np.zeros(fm.AUDIO_TAPS, np.float32)
    ol.oracle().fmo_lowpass_kernel(fm.AUDIO_TAPS, 15000, 192000, ol.fptr(h))
    rs = f.taps(3)
    assert rs.size == fm.RS_TAPS
    worst = None
    for c in probe:
        x, pcm = r.stream(c)
        st = setting[c % kinds]
        gains = fm.gain_steps(x.shape[0], [r.j_starts[k] for k, _ in st], [fm.gain_lr(*s) for _, s in st])
        w = fm.compare(pcm, fm.stage_c_two_step(x, h, rs, gains), r.frame_starts)
        assert w.scale > 0.1
        if worst is None or w.rel > worst[1].rel:
            worst = (c, w)
    report("stage C, gain changes, %d channel(s): worst channel %d" % (nch, worst[0]), worst[1], fm.STAGE_C_BOUND)
    fm.check(worst[1], fm.STAGE_C_BOUND, "stage C with gain changes, channel %d of %d" % (worst[0], nch))


def test_stage_c_default_small_handle(fmx_amd, ol):
    """The default handle of up to 64 channels runs the reference's block machines (fmx_ola.hip): the audio low-pass and the de-emphasis
    behind it write a second ring, which the resampler reads and which FMX_TAP_PRE_RESAMPLER returns in this form (fmx_api.hip stage_c:
    Bq.dring = d2ring; fmx_get_tap) -- the tap FOLLOWS the filter and the de-emphasis, so the model is the gain and the 128-tap resampler
    alone.  Ragged calls.
    Reference alone (CPU): 1.21e-6 of the peak (resampler alone: 8.0e-7); bound 2.42e-6.  Measured on the MI355X: 3.4e-7."""
    sizes = RAGGED * 2
    iq = ol.synth_iq(sum(sizes))[None]
    f = fmx_amd.Fmx(1, max_block=max(sizes))
    defaults(f, folded=False)
    f.set_param(M.P_VOLUME_DB, -10.5); f.set_param(M.P_SOUND_BALANCE, 30)
    r = Run(f, iq, sizes, [0])
    x, pcm = r.stream(0)
    w = fm.compare(pcm, fm.stage_c_folded(x, f.taps(3), fm.gain_lr(-10.5, 30), lf_on=False), r.frame_starts)
    report("stage C, default small handle (block machines)", w, fm.STAGE_C_BOUND)
    assert w.scale > 0.1
    fm.check(w, fm.STAGE_C_BOUND, "stage C of the default handle")


@pytest.mark.parametrize("audio_rate", [44100, 96000, 32000])
def test_second_converter(fmx_amd, ol, audio_rate):
    """audioRate != workingRate, ragged calls: the float64 model of both stages -- stage C's 48 kHz frames from the d ring, not rounded,
    into out[m] = sum_k taps[(m q) mod p][k] x48[floor (m q / p) - k] -- on every output frame.
    Reference alone (CPU): converter 5.84e-7 of the peak, stage C 1.21e-6; bound 2.42e-6 + 5.84e-7.  Measured on the MI355X: 5.3e-7 (44100), 4.6e-7 (96000), 4.9e-7 (32000)."""
    sizes = RAGGED + [16384 * 4 + 1200, 30011, 150000]
    iq = ol.synth_iq(sum(sizes))[None]
    f = fmx_amd.Fmx(1, max_block=max(sizes), audioRate=audio_rate)
    defaults(f)
    r = Run(f, iq, sizes, [0])
    x, pcm = r.stream(0)
    p, q, taps = fm.conv2_design(ol.oracle(), 48000, audio_rate)
    x48 = fm.stage_c_folded(x, f.taps(2), fm.gain_lr(-6.0, 0))
    ref = fm.conv2(x48, p, q, taps)
    assert ref.shape == pcm.shape, (ref.shape, pcm.shape)
    w = fm.compare(pcm, ref, r.frame_starts)
    report("second converter %d" % audio_rate, w, fm.CONV2_BOUND)
    assert w.scale > 0.1
    fm.check(w, fm.CONV2_BOUND, "second converter at %d" % audio_rate)


# ------------------------------------------------------------------------------------------------ RDS baseband
RDS_SIZES = [383988, 200000, 300007, 383988, 123456, 383000] * 3      # <= 31999 fm samples a call (the row taps hold the whole call); 2.3 s


def rds_case(fmx_amd, ol, nch, streams, join):
    """join: channel -> the call its decoder is switched on with."""
    iq = np.stack([ol.synth_iq(sum(RDS_SIZES), rds=1, rdsLevel=0.05, rdsBitsSeed=777 + s, leftHz=1000.0 + 370.0 * s) for s in range(streams)])
    f = fmx_amd.Fmx(nch, streams=streams, stream_of_channel=[c % streams for c in range(nch)], max_block=max(RDS_SIZES))
    defaults(f, folded=nch > 1)
    if nch > 64:
        f.set_param(M.P_SCOPE_TAPS, 1)
    probe = sorted(join)
    d, ph, q, starts = ({c: [] for c in probe} for _ in range(4))
    pos = j = 0
    j_on = {}
    for k, s in enumerate(RDS_SIZES):
        for c in range(nch):
            if join.get(c, join[max(x for x in probe if x <= c)]) == k:
                f.set_param(M.P_RDS_MODE, 2, c)
        f.process_host(iq[:, pos:pos + s])
        pos += s
        nj = f.last_fm_samples()
        assert nj <= 31999 and nj % 32000 != 0
        for c in probe:
            if join[c] <= k:
                j_on.setdefault(c, j)
                d[c].append(f.tap(M.TAP_DEMOD, nj, c)); ph[c].append(f.tap(M.TAP_PILOT_PHASE, nj, c))
                starts[c].append(sum(len(a) for a in q[c]))
                nq = f.last_rds_samples(c)
                q[c].append(f.tap(M.TAP_RDS_IQ, nq, c))
        j += nj
    bp, dk = fm.rds_tables(ol.oracle())
    worst = None
    for c in probe:
        dd, pp, qq = np.concatenate(d[c]), np.concatenate(ph[c]), np.concatenate(q[c])
        assert qq.shape[0] == dd.shape[0] // 8 and dd.shape[0] > 64000 + 2 * 96000
        ref = fm.rds_front(dd, pp, bp, dk)
        w = fm.compare(qq[:, 0].astype(np.float64) + 1j * qq[:, 1], ref, starts[c])
        print("\n[RDS baseband, channel %d of %d, on from fm sample %d (mod 8 = %d)] %s; input sample of the worst mod 32000 = %d"
              % (c, nch, j_on[c], j_on[c] % 8, w, (8 * w.index + 7) % 32000))
        assert w.scale > 0.05
        if worst is None or w.rel > worst[1].rel:
            worst = (c, w)
    return j_on, worst


def test_rds_baseband_one_channel(fmx_amd, ol):
    """FMX_P_RDS_MODE = 2 on one receiver: FMX_TAP_RDS_IQ of every call against band-pass, Hilbert filter, mix with three times the pilot
    phase of 64000 samples earlier and the 11-tap decimator in float64, on FMX_TAP_DEMOD and FMX_TAP_PILOT_PHASE of the same calls;
    calls of at most 31999 fm samples whose lengths do not divide the filters' 32000-sample blocks.
    Reference alone (CPU): 1.06e-6 of the peak; bound 2.12e-6.  Measured on the MI355X: 8.2e-7 (2.1e-7 at a peak of 0.256)."""
    _, (c, w) = rds_case(fmx_amd, ol, 1, 1, {0: 0})
    fm.check(w, fm.RDS_BOUND, "RDS baseband, one channel")


def test_rds_baseband_batch_with_decoders_switched_on_at_different_calls(fmx_amd, ol):
    """70 channels on two streams, the decoders of channels 0-29 on from the first call, of 30-49 from the third, of 50-69 from the fourth:
    three phases of the decimator by 8 and of the 32000-sample blocks in one handle (each path counts its own samples).
    Reference alone (CPU): 1.06e-6 of the peak; bound 2.12e-6.  Measured on the MI355X: 8.9e-7 ... 9.2e-7 on the channels on from the start (peak 0.256),
    1.5e-6 ... 1.99e-6 on those switched on later: the same 2.3e-7 ... 2.8e-7 worst sample at a baseband peak of 0.14 ... 0.15 (no lock-in transient in it)."""
    join = {0: 0, 1: 0, 29: 0, 30: 2, 31: 2, 50: 3, 51: 3, 69: 3}
    j_on, (c, w) = rds_case(fmx_amd, ol, 70, 2, join)
    assert len({j_on[c] % 8 for c in (0, 30, 50)}) == 3 and len({j_on[c] % 32000 for c in (0, 30, 50)}) == 3
    fm.check(w, fm.RDS_BOUND, "RDS baseband, channel %d of 70" % c)

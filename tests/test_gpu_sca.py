"""The sub-carrier decoder on the GPU (fmx_sca_setup / _enable / _read; csrc/fmx_sca.hip) against the float64 model of
tests/sca_model.py on the handle's own FMX_TAP_DEMOD.

The signal is sca_signal's at 2.304 MS/s: an SCA of 7500 Hz injection carrying a 1 kHz tone at +-6 kHz under the programme (noise in L+R and L-R, pilot,
RDS band), one seed per stream, frequency-modulated in float64 onto a carrier of amplitude 0.5.  The measure and the bound are sca_model's (see its head):
|s - s64| per audio sample and the relative error of the level per block; the GPU must stay within 2 x the worst and 2 x the median of the numpy-f32
restatement on the same taps' d.  The condition min |y| >= 0.1 median |y| is asserted on the model.  Blocks of two cuts are compared bit for bit, and only
on handles whose taps do not depend on the cut (the PLL decoder, RF DC removal off), the taps' equality asserted first.
Shapes: 41 060 fm samples per channel (492 720 input samples, 21 blocks of 1920 and 740 fm samples)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import sca_model as sm
import sca_signal as sg
import survey_model as sv

pytestmark = pytest.mark.gpu

R = 12
BF, BA = sm.BLOCK_FM, sm.BLOCK_AUDIO
N_FM = sv.stream_length(1)
CUTS = [R * c for c in sv.call_cuts(1)]      # three calls that complete no block, calls that complete several, a call of one fm sample, the rest
CENTRES = {0: 67000, 1: 82000, 2: 76000}

_IQ = {}


def iq_streams(streams=3, n_fm=N_FM, with_programme=True):
    """[streams, 12 n_fm, 2] f32; stream s carries its sub-carrier at CENTRES [s mod 3], seed 1 + s"""
    key = (streams, n_fm, with_programme)
    if key not in _IQ:
        _IQ[key] = np.stack([sg.fm_iq(sg.multiplex(n_fm * R, 192000 * R, with_programme=with_programme, seed=1 + s, centre_hz=CENTRES[s % 3]), 192000 * R)
                             for s in range(streams)])
    return _IQ[key]


def cut_free(m):
    """the handles whose taps do not depend on how the stream is cut (tests/test_gpu_mod_meter.py cut_free)"""
    return [(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0)]


def expected_blocks(cuts_fm, on_call=0):
    """the blocks a channel switched on by call on_call delivers"""
    on_from = sum(cuts_fm[:on_call])
    return list(range(sm.first_block(on_from), sum(cuts_fm) // BF))


class Run:
    """One handle fed x ([streams, n, 2] f32) in calls of the given input-sample lengths; the decoding channels' blocks read behind every call (or behind
    the last): blocks [c] = {b: (audio, level)}, runs [c] = the (first_block, n) of every non-empty read; FMX_TAP_DEMOD of the channels of tap_ch read
    behind every call and concatenated: taps [c]."""

    def __init__(self, fmx_amd, x, cuts, decoding=None, channels=None, params=(), via="host", tap_ch=(), read_every_call=True, setup=None):
        m = fmx_amd.fmx
        ns, n = x.shape[0], x.shape[1]
        channels = ns if channels is None else channels
        decoding = {0: 67000, 2: 76000} if decoding is None else decoding
        assert sum(cuts) == n
        f = fmx_amd.Fmx(channels, streams=ns if channels != ns else 0, stream_of_channel=[c % ns for c in range(channels)] if channels != ns else None,
                        max_block=max(cuts))
        self.blocks, self.runs = {c: {} for c in range(channels)}, {c: [] for c in range(channels)}
        taps, self.pieces = {c: [] for c in tap_ch}, []
        try:
            for item in params:
                f.set_param(*item)
            if setup:
                f.sca_setup(**setup)
            for c, hz in decoding.items():
                f.sca_enable(hz, c)
            if via == "device":
                import torch
                d_iq = torch.from_numpy(x).cuda()
                cap = max(f.frames_for(max(cuts)) + 64, 64)
                d_pcm = torch.zeros((channels, cap, 2), dtype=torch.float32, device="cuda")
            pos = 0
            for k, ln in enumerate(cuts):
                if via == "device":
                    got = C.c_int64()
                    f._check(f.L.fmx_process_device_raw(f.h, C.c_void_p(d_iq.data_ptr() + 8 * pos), m.IQ_F32, 2048.0, n, ln, C.c_void_p(d_pcm.data_ptr()), cap,
                                                        C.byref(got), None))
                    f.synchronize()
                else:
                    f.process_host_raw(x[:, pos:pos + ln], m.IQ_F32)
                pos += ln
                self.pieces.append(f.last_call_pieces())
                nj = f.last_fm_samples()
                for c in tap_ch:
                    if nj > 0:
                        taps[c].append(f.tap(m.TAP_DEMOD, nj, c))
                if read_every_call or k == len(cuts) - 1:
                    for c in range(channels) if channels <= 3 else sorted(decoding):
                        self.take(c, f.sca_read(c, 1)[0])
            self.taps = {c: np.concatenate(v) for c, v in taps.items()}
            self.facts = (f.last_second_group(), f.last_call_pieces(), f.last_front_kernel())
        finally:
            f.close()
        self.idx = {c: sorted(v) for c, v in self.blocks.items()}

    def take(self, c, got):
        first, audio, level = got
        assert (first < 0) == (len(audio) == 0) and audio.shape == (len(level), BA)
        if len(audio):
            self.runs[c].append((first, len(audio)))
        for i in range(len(audio)):
            assert first + i not in self.blocks[c]
            self.blocks[c][first + i] = (audio[i], level[i])


def same_bits(a, b, blocks=None):
    blocks = sorted(a) if blocks is None else blocks
    return all(b_ in a and b_ in b and a[b_][0].tobytes() == b[b_][0].tobytes() and np.float32(a[b_][1]).tobytes() == np.float32(b[b_][1]).tobytes() for b_ in blocks)


def against_the_model(tag, fmx_amd, run, chans, centres, want):
    """the blocks of `chans` within the bound of the float64 model on the taps; -> the GPU's own levels"""
    g, a = fmx_amd.sca_taps("g"), fmx_amd.sca_taps("a")
    out = {}
    for c in chans:
        d = run.taps[c]
        M = sm.model64(d, g, a, centres[c])
        assert run.idx[c] == want and set(want) <= set(M), (c, run.idx[c], want)
        cond = sm.conditioning({b: M[b] for b in want})
        lv = sm.levels(M, sm.blocks32(d, g, a, centres[c]), blocks=want)
        print("\n[%s, channel %d at %d Hz] min |y| / median |y| = %.3f; restatement: s worst %.3e median %.3e, level worst %.3e median %.3e"
              % ((tag, c, centres[c], cond) + lv))
        assert cond >= 0.1, cond
        ok, r = sm.check("GPU, %s, channel %d" % (tag, c), run.blocks[c], M, lv, blocks=want)
        assert ok, r
        es, el = sm.errors(run.blocks[c], M, want)
        out[c] = (float(es.max()), float(np.median(es)), float(el.max()), float(np.median(el)))
    return out


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_blocks_against_the_float64_model_on_the_handles_taps(fmx_amd):
    """A 3-channel handle (scope taps on by default), channels 0 and 2 decoding at 67 and 76 kHz, channel 1 not; calls cut at 12 x call_cuts (1).
    (Measured on an MI355X, DESIGN.md 4.17: the GPU's own levels are printed beside the restatement's.)"""
    run = Run(fmx_amd, iq_streams(), CUTS, tap_ch=(0, 2))
    want = expected_blocks(sv.call_cuts(1))
    assert want == list(range(1, 21)) and run.idx[1] == [] and all(t.size == N_FM for t in run.taps.values())
    own = against_the_model("3 channels", fmx_amd, run, (0, 2), CENTRES, want)
    print("the GPU's own: %s" % own)
    assert not same_bits(run.blocks[0], run.blocks[2])


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_cuts_and_entry_points_are_bit_identical(fmx_amd):
    """One call against the cuts and fmx_process_host_raw against fmx_process_device_raw: the same taps, then the same blocks, byte for byte."""
    m = fmx_amd.fmx
    x = iq_streams()
    n = x.shape[1]
    whole = Run(fmx_amd, x, [n], params=cut_free(m), tap_ch=(0, 2))
    cut = Run(fmx_amd, x, CUTS, params=cut_free(m), tap_ch=(0, 2))
    dev = Run(fmx_amd, x, CUTS, params=cut_free(m), via="device", tap_ch=(0, 2))
    for c in (0, 2):
        assert whole.taps[c].tobytes() == cut.taps[c].tobytes() == dev.taps[c].tobytes(), c      # (the premise)
        assert whole.idx[c] == cut.idx[c] == dev.idx[c] == list(range(1, 21))
        assert same_bits(whole.blocks[c], cut.blocks[c]) and same_bits(cut.blocks[c], dev.blocks[c])
    assert whole.runs[0] == [(1, 20)]


def test_calls_of_one_fm_sample_across_a_block_end(fmx_amd):
    m = fmx_amd.fmx
    x = iq_streams()[:, :R * (3 * BF + 3)]
    single = Run(fmx_amd, x, [R * (2 * BF - 2), R, R, R, R, R * (BF - 3), R, R, R, R], params=cut_free(m), tap_ch=(0,))
    block = Run(fmx_amd, x, [R * (3 * BF + 3)], params=cut_free(m), tap_ch=(0,))
    assert single.taps[0].tobytes() == block.taps[0].tobytes()
    for c in (0, 2):
        assert single.idx[c] == block.idx[c] == [1, 2] and same_bits(single.blocks[c], block.blocks[c])
    assert single.runs[0] == [(1, 1), (2, 1)]


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_rds_pieces(fmx_amd):
    """One call of 400 000 input samples with the RDS decoder on is made in RDS pieces (at most 31 999 fm samples each): the blocks are those of the same
    stream in calls of 16 384."""
    m = fmx_amd.fmx
    n = 400000
    x = iq_streams(1)[:, :n]
    params = cut_free(m) + [(m.P_RDS_MODE, 2)]
    one = Run(fmx_amd, x, [n], decoding={0: 67000}, params=params)
    small = Run(fmx_amd, x, [16384] * (n // 16384) + [n % 16384], decoding={0: 67000}, params=params)
    assert n // R > 31999 and one.idx[0] == small.idx[0] == list(range(1, n // R // BF)) and len(one.idx[0]) == 16
    assert same_bits(one.blocks[0], small.blocks[0])


def test_overlapping_pieces(fmx_amd):
    """A 1024-channel PLL-decoder handle on 3 shared streams makes a call of 98 304 input samples in overlapping pieces of 1536 fm samples; channels 0, 2
    and 1023 decode.  The blocks are those of the same calls made whole."""
    m = fmx_amd.fmx
    n = 98304
    x = iq_streams()[:, :2 * n]
    dec = {0: 67000, 2: 76000, 1023: 67000}
    big, whole = (Run(fmx_amd, x, [n, n], decoding=dec, channels=1024, params=cut_free(m) + [(m.P_CALL_PIECES, pieces)]) for pieces in (1536, 0))
    assert big.pieces[0] > 1 and whole.pieces == [1, 1]
    for c in dec:
        assert big.idx[c] == whole.idx[c] == list(range(1, 2 * n // R // BF)) and same_bits(big.blocks[c], whole.blocks[c])
    assert same_bits(big.blocks[0], big.blocks[1023]) and not same_bits(big.blocks[0], big.blocks[2])      # (channels 0 and 1023 share a stream: 1023 = 3 x 341)


def test_stage_b_as_one_kernel_and_as_two(fmx_amd):
    m = fmx_amd.fmx
    n = R * (4 * BF + 100)
    x = iq_streams()[:, :n]
    dec = {0: 67000, 129: 67000}
    a, b = (Run(fmx_amd, x, [n // 2, n // 2], decoding=dec, channels=130, params=cut_free(m) + [(m.P_STAGEB_FORM, form)]) for form in (1, 2))
    for c in dec:
        assert a.idx[c] == b.idx[c] == [1, 2, 3] and same_bits(a.blocks[c], b.blocks[c])


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_without_scope_taps(fmx_amd):
    """130 channels on 3 streams, channels 0, 2 and 129 decoding, scope taps off by default: the blocks equal those of the same handle with
    FMX_P_SCOPE_TAPS = 1, and those are within the bound of the model on its taps."""
    m = fmx_amd.fmx
    x = iq_streams()
    dec = {0: 67000, 2: 76000, 129: 67000}
    off = Run(fmx_amd, x, CUTS, decoding=dec, channels=130)
    on = Run(fmx_amd, x, CUTS, decoding=dec, channels=130, params=[(m.P_SCOPE_TAPS, 1)], tap_ch=tuple(dec))
    want = expected_blocks(sv.call_cuts(1))
    for c in dec:
        assert off.idx[c] == on.idx[c] == want and same_bits(off.blocks[c], on.blocks[c])
    against_the_model("130 channels", fmx_amd, on, tuple(dec), dec, want)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------------
def everything(f, channels):
    """what a handle delivers beside the decoder"""
    some = sorted({0, min(1, channels - 1), channels - 1})
    return dict(meta=[bytes(f.meta(c)) for c in range(channels)], bits=[f.rds_bits(c).tobytes() for c in some], peaks=[f.peaks(c).tobytes() for c in some] if channels <= 64 else [b""],
                scan=[f.scan_results(c).tobytes() for c in some], mod=[r.tobytes() for r in f.mod_records()], audio=[r.tobytes() for r in f.audio_records()],
                rx=[r.tobytes() for r in f.rx_records()], rdsm=[r.tobytes() for r in f.rds_meter_records()],
                spec=[b"".join(a.tobytes() for a in f.spectrum_read(s)) for s in range(f.streams)],
                mpx=[b"".join(a.tobytes() for a in r) for r in f.mpx_spectrum_read(0, channels)],
                facts=(f.last_second_group(), f.last_call_pieces(), f.last_front_kernel()))


@pytest.mark.parametrize("channels", [1, 130])
def test_everything_else_is_undisturbed(fmx_amd, ol, channels):
    """With every channel decoding, PCM, RDS bits, meta, peaks, scan records, the six meters' records and the facts about the last call --
    fmx_last_second_group among them -- equal a twin handle's that has the modulation meter on instead, bit for bit: on a 1-channel block-machine handle
    and on a batch of 130 channels on 3 shared streams (whose last channel scans)."""
    m = fmx_amd.fmx
    blk, ncalls = 16384, 24
    streams = 1 if channels == 1 else 3
    x = np.stack([ol.synth_iq(ncalls * blk, rds=1, leftHz=500.0 + 300 * s, rightHz=900.0 + 200 * s) for s in range(streams)])
    out = []
    for decode in (False, True):
        f = fmx_amd.Fmx(channels, streams=streams if channels > 1 else 0, stream_of_channel=[c % streams for c in range(channels)] if channels > 1 else None,
                        max_block=blk)
        f.set_param(m.P_BANDWIDTH, 165000)
        f.set_param(m.P_RDS_MODE, 2)
        if channels > 1:
            f.set_param(m.P_SCANNING, 1, channels - 1)
        f.mod_meter(True); f.audio_meter(True); f.rx_meter(True); f.rds_meter_enable(True)
        f.spectrum_setup(2, 1); f.spectrum_meter(True)
        f.mpx_spectrum_setup(2, 1); f.mpx_spectrum_meter(True)
        if decode:
            f.sca_enable(67000)
        pcm = np.concatenate([f.process_host(x[:, k * blk:(k + 1) * blk]) for k in range(ncalls)], axis=1)
        e = everything(f, channels)
        e["pcm"] = pcm
        e["sca"] = f.sca_read(0, channels)
        out.append(e)
        f.close()
    a, b = out
    assert np.array_equal(a["pcm"], b["pcm"]) and a["pcm"].shape[1] > 0
    for key in ("meta", "bits", "peaks", "scan", "mod", "audio", "rx", "rdsm", "spec", "mpx", "facts"):
        assert a[key] == b[key], key
    assert len(a["bits"][0]) > 0 and len(a["mod"][0]) > 0 and len(a["audio"][0]) > 0 and len(a["rx"][0]) > 0 and len(a["rdsm"][0]) > 0 and len(a["spec"][0]) > 0 and len(a["mpx"][0]) > 0
    assert all(r[0] == -1 and len(r[1]) == 0 for r in a["sca"])
    assert all(r[0] == 1 and len(r[1]) == ncalls * blk // R // BF - 1 for r in b["sca"])       # (32 768 fm samples: blocks 1 .. 16; the scanning channel decodes on)


def test_the_second_group_is_the_modulation_meters(fmx_amd, ol):
    """a batch with ONE channel decoding writes the rows for every channel and is no plain batch: fmx_last_second_group, and the PCM, are those of a twin
    with only the modulation meter on the same channel; a twin without either is a plain batch"""
    m = fmx_amd.fmx
    blk = 49152
    x = np.stack([ol.synth_iq(3 * blk, leftHz=500.0 + 300 * s) for s in range(2)])
    res = []
    for which in ("none", "mod", "sca"):
        f = fmx_amd.Fmx(1100, streams=2, stream_of_channel=[c % 2 for c in range(1100)], max_block=blk)      # (768 + 332: tests/test_gpu_mod_meter.py)
        f.set_param(m.P_BANDWIDTH, 165000)
        if which == "mod":
            f.mod_meter(True, 5)
        if which == "sca":
            f.sca_enable(67000, 5)
        pcm = np.concatenate([f.process_host(x[:, k * blk:(k + 1) * blk]) for k in range(3)], axis=1)
        res.append((f.last_second_group(), f.last_call_pieces(), f.last_front_kernel(), pcm, len(f.sca_read(5, 1)[0][1])))
        f.close()
    none, mod, sca = res
    assert sca[:3] == mod[:3] and np.array_equal(sca[3], mod[3]) and np.array_equal(sca[3], none[3])
    assert none[0] == 332 and mod[0] == 0 and mod[4] == 0 and sca[4] == 3 * blk // R // BF - 1


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_switch_ring_and_cursors(fmx_amd):
    m = fmx_amd.fmx
    T = 10 * BF                                                 # 0.1 s
    x = iq_streams(1, 17 * T)
    ref = Run(fmx_amd, x, [R * T] * 17, decoding={0: 67000, 1: 67000, 2: 67000}, channels=3, params=cut_free(m), tap_ch=(0,))      # on throughout, read every call
    assert ref.idx[0] == list(range(1, 170)) and same_bits(ref.blocks[0], ref.blocks[2])
    f = fmx_amd.Fmx(3, streams=1, stream_of_channel=[0, 0, 0], max_block=R * T)
    try:
        taps = []
        for item in cut_free(m):
            f.set_param(*item)
        read = lambda c, **kw: f.sca_read(c, 1, **kw)[0]

        def call(g, n):
            f.process_host_raw(x[:, R * g:R * (g + n)], m.IQ_F32)
            taps.append(f.tap(m.TAP_DEMOD, f.last_fm_samples(), 0))
            return g + n

        def equal(got, first, n):
            return got[0] == first and len(got[1]) == n and all(got[1][i].tobytes() == ref.blocks[0][first + i][0].tobytes() and
                                                                np.float32(got[2][i]).tobytes() == np.float32(ref.blocks[0][first + i][1]).tobytes() for i in range(n))
        g = call(0, BF + 100)                                   # (no decoder yet: nothing is allocated, nothing is read)
        assert read(0) [0] == -1
        for hz, why in ((92000, "above"), (60000, "below")):    # what the rule refuses says why
            with pytest.raises(fmx_amd.FmxError) as e:
                f.sca_enable(hz, 0)
            assert e.value.code == m.FMX_E_INVALID and why in str(e.value) and str(hz) in str(e.value)
        f.sca_enable(82000, 1); f.sca_enable(0, 1)              # (82 kHz is admitted; off again before any call)
        f.sca_enable(67000, 0)                                  # in mid-block, at fm sample 2020: the first block with its history behind it is 2 (3840 - 703 >= 2020)
        with pytest.raises(fmx_amd.FmxError) as e:              # the setup is fixed while a channel decodes
            f.sca_setup(deviation_hz=5000)
        assert e.value.code == m.FMX_E_INVALID and "on" in str(e.value)
        g = call(g, 3 * BF)                                     # 4 BF + 100: blocks 1 (not delivered), 2, 3 complete
        assert equal(read(0), 2, 2)
        f.sca_enable(67000, 2)                                  # a second channel: its memory is added, channel 0's is kept
        g = call(g, 2 * BF - 100)                               # 6 BF: channel 0 delivers 4, 5; channel 2, on at 4 BF + 100, has block 5's history (9600 - 703 >= 7780)
        assert equal(read(0), 4, 2) and equal(read(2), 5, 1)
        f.sca_enable(0, 0)
        g = call(g, 2 * BF)                                     # 8 BF: channel 0 is off; channel 2 delivers 6, 7
        assert read(0)[0] == -1 and equal(read(2), 6, 2)
        f.sca_enable(67000, 0)
        g = call(g, BF)                                         # channel 0 on again at 8 BF: block 8 lacks its history, the first is 9
        g = call(g, 2 * BF)                                     # 11 BF
        assert equal(read(0), 9, 2)                             # a gap in first_block: 6 .. 8 fell while it was off, and nothing stale in the carry
        # off and on between two reads: a gap inside what is unread ends the run there; the rest comes with the next read
        f.sca_enable(0, 0); g = call(g, BF)                     # 12 BF
        f.sca_enable(67000, 0); g = call(g, 3 * BF)             # 15 BF: on at 12 BF: 13, 14
        f.sca_enable(0, 0); g = call(g, BF)                     # 16 BF: block 15 is dropped
        f.sca_enable(67000, 0); g = call(g, 4 * BF)             # 20 BF: on at 16 BF: 17, 18, 19
        assert equal(read(0), 13, 2) and equal(read(0), 17, 3) and read(0)[0] == -1
        g = call(g, 10 * BF)                                    # 30 BF = 3 T
        assert equal(read(2, capacity=4), 8, 4)                 # capacity smaller than what is there; independent cursors
        assert equal(read(0), 20, 10)
        # a failed read moves no cursor
        n_blocks = np.zeros(1, np.int32); first = np.zeros(1, np.int64)
        assert f.L.fmx_sca_read(f.h, 2, 1, first.ctypes.data, None, None, 8, n_blocks.ctypes.data) == m.FMX_E_INVALID and n_blocks[0] == 0
        audio = np.zeros((8, BA), np.float32)
        assert f.L.fmx_sca_read(f.h, 2, 1, first.ctypes.data, audio.ctypes.data, None, 8, None) == m.FMX_E_INVALID and not audio.any()
        assert equal(read(2, capacity=2), 12, 2)
        # 14 unread calls of 0.1 s: the oldest blocks are lost, the newest 128 are exact
        for _ in range(14):
            g = call(g, T)                                      # 17 T: blocks up to 169
        assert np.concatenate(taps).tobytes() == ref.taps[0][:g].tobytes()                  # (the premise of every comparison with ref above)
        # the range read: channel 0 decoded on, channel 1 never did, channel 2 decoded on
        got = f.sca_read(0, 3)
        assert equal(got[0], 42, 128) and got[1][0] == -1 and equal(got[2], 42, 128)
        assert all(r[0] == -1 for r in f.sca_read(0, 3)) and read(0, level=False)[2] is None
        with pytest.raises(fmx_amd.FmxError):
            f.sca_read(2, 2)                                    # (channels 2 .. 3 of 3)
        f.sca_enable(0)                                         # every decoder off: calls in which the decoder has nothing to do, a new setup, then on again
        g0 = g
        f.process_host_raw(x[:, :R * BF], m.IQ_F32); f.process_host_raw(x[:, :R * BF], m.IQ_F32)
        f.sca_setup(deviation_hz=3000)                          # cursors start over; twice the output for the same deviation
        f.sca_enable(67000, 1)
        f.process_host_raw(x[:, :R * 3 * BF], m.IQ_F32)        # on at 17 T + 2 BF = 172 BF: blocks 173, 174
        first, audio, level = read(1)
        assert first == 173 and len(audio) == 2 and np.isfinite(audio).all() and 0.5 < np.abs(audio).max() < 4.0 and g0 == 17 * T
    finally:
        f.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------------------
# (measured on the CPU, DESIGN.md 4.17: the float64 model on the CPU oracle's DEMOD tap of the same IQ; the bounds are twice the measurements)
E2E = {67000: (3.939e-4, 2928.4), 76000: (4.877e-4, 3761.6)}      # centre -> |amplitude - |A (1000)||, the worst block's |2 sqrt (level) u - 7500| in Hz


def test_end_to_end(fmx_amd):
    """The SCA under the programme at 67 and at 76 kHz, 0.2 s, the default decoder: the recovered tone's amplitude against the response of `a` at 1 kHz
    (the tone was sent at the full +-6 kHz), and 2 sqrt (level) x fmx_mod_hz_per_unit against the 7500 Hz sent.  The level reads the sub-carrier as d
    holds it: the chain's input filter and discriminator pass 0.59 of it at 67 kHz and 0.50 at 76 kHz, which the float64 model on the oracle's tap shows
    alike -- hence the size of that bound."""
    m = fmx_amd.fmx
    a = fmx_amd.sca_taps("a")
    u = m.mod_hz_per_unit(3, 192000)
    n_fm = 20 * BF
    for s, centre in ((0, 67000), (2, 76000)):
        x = sg.fm_iq(sg.multiplex(n_fm * R, 192000 * R, seed=1, centre_hz=centre), 192000 * R)[None]
        run = Run(fmx_amd, x, [R * n_fm], decoding={0: centre}, channels=1, params=[(m.P_FM_DECODER, 3)])
        bl = list(range(2, 20))
        assert run.idx[0] == list(range(1, 20))
        amp, res = sg.tone_fit(np.concatenate([run.blocks[0][b][0] for b in bl]).astype(np.float64), 1000.0, 24000)
        inj = max(abs(2 * np.sqrt(float(run.blocks[0][b][1])) * u - 7500.0) for b in bl)
        want = sm.response(a, 1000, 48000)
        print("\n%d Hz: amplitude %.5f against |A| %.5f: %.3e apart (bound %.3e); residual %.3e; injection %.1f Hz off (bound %.1f)"
              % (centre, amp, want, abs(amp - want), 2 * E2E[centre][0], res, inj, 2 * E2E[centre][1]))
        assert abs(amp - want) <= 2 * E2E[centre][0] and inj <= 2 * E2E[centre][1]


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_cpp_demo_builds_and_runs(fmx_amd, tmp_path):
    """tests/sca_demo through host/fm_processor_adapter.h: blocks of 16 384: the blocks the Python handle delivers for the same stream"""
    import test_sca_cpu
    exe, fin, fout = str(tmp_path / "sca_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "sca.bin")
    test_sca_cpu.build_demo(fmx_amd, exe)
    x = iq_streams(1)[:, :24 * 16384]
    x[0].tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    assert out.returncode == 0 and lines[-1] == "blocks 16 first 1", lines
    rows = np.fromfile(fout, np.float32).reshape(-1, 2 + BA)
    run = Run(fmx_amd, x, [16384] * 24, decoding={0: 67000}, channels=1)
    assert [int(v) for v in rows[:, 0]] == run.idx[0] == list(range(1, 17))
    assert all(rows[i, 2:].tobytes() == run.blocks[0][b][0].tobytes() and rows[i, 1].tobytes() == np.float32(run.blocks[0][b][1]).tobytes() for i, b in enumerate(run.idx[0]))

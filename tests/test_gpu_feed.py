"""The monitoring feed on the GPU (fmx_feed_enable / _read / _read_device; csrc/fmx_feed.hip).  The model's input is the handle's own
returned PCM: every sample and every power of every block must EQUAL the f32 restatement of tests/feed_model.py bit for bit (no transcendental function
is involved) and lie within the float64 model's derived bounds.  Then: the blocks' independence of how the stream is cut into calls and pieces, the
switching rules, a scanning channel's zeros, the ring and its three read-outs, the kernel's shapes, batches in two channel groups and in overlapping
pieces, the isolation of everything else a handle delivers, and the C++ adapter.

At 2.304 MS/s a call delivers frames in lumps of 48, one per 2304 input samples; the cuts go around the block of 480 frames."""
import subprocess

import numpy as np
import pytest

import feed_model as fm

pytestmark = pytest.mark.gpu

BF, BLOCK, RING = fm.BLOCK_FRAMES, fm.BLOCK, fm.RING
LUMP = 2304
# (a)'s calls in input samples: 1, 2, 9, 10, 11, 19, 20 and 21 lumps of 48 frames -- around one block and around two --, a call of no frame, the receiver's
# block, then calls of two blocks and a bit and of four
CALLS_A = [LUMP * k for k in (1, 2, 9, 10, 11, 19, 20, 21)] + [12, 16384] + [LUMP * 23] * 4 + [LUMP * 47] * 2
TONE = dict(stereo=0, leftHz=1000.0, rightHz=1000.0, leftAmp=1.0, rightAmp=1.0, deviationHz=37500.0 / 0.9)
NOISE = dict(carrierAmp=0.0, noiseSeed=11, noiseSigma=0.3)

_X = {}


def three_signals(ol, n):
    """a stereo programme, a mono tone and noise, [3, n, 2] f32; computed once per length"""
    if n not in _X:
        _X[n] = np.stack([ol.synth_iq(n), ol.synth_iq(n, **TONE), ol.synth_iq(n, **NOISE)])
    return _X[n]


def frames_at(n_samples, per_fm=12):
    """PCM frames a handle has delivered after n_samples input samples (per_fm input samples per fm sample)"""
    return 48 * ((n_samples // per_fm) // 192)


def marks(calls, per_fm=12):
    """M [k]: the frames delivered in front of call k"""
    return [frames_at(sum(calls[:k]), per_fm) for k in range(len(calls) + 1)]


def cut_free(m):
    """the settings under which the demodulator output does not depend on the cut (tests/test_gpu_audio_meter.py cut_free; the PCM behind them still does)"""
    return [(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0)]


def make(fmx_amd, channels, streams=0, max_block=16384, params=(), **kw):
    m = fmx_amd.fmx
    som = [c % streams for c in range(channels)] if streams else None
    f = fmx_amd.Fmx(channels, streams=streams, stream_of_channel=som, max_block=max_block, **kw)
    f.set_param(m.P_BANDWIDTH, 165000)
    for item in params:
        f.set_param(*item)
    return f


class Taker:
    """collects what feed_read hands out: blocks [c] = {b: (audio, power)}, runs [c] = the (first_block, n) of every non-empty read"""

    def __init__(self, channels):
        self.blocks, self.runs = {c: {} for c in channels}, {c: [] for c in channels}

    def take(self, c, got):
        first, audio, power = got
        assert (first < 0) == (len(audio) == 0) and audio.shape == (len(power), BLOCK)
        if len(audio):
            self.runs[c].append((first, len(audio)))
        for i in range(len(audio)):
            assert first + i not in self.blocks[c]
            self.blocks[c][first + i] = (audio[i], power[i])

    def read(self, f, c, **kw):
        self.take(c, f.feed_read(c, 1, **kw)[0])


def run(f, x, calls, each=None, taker=None, read_every_call=True):
    """the calls of `calls` input samples behind each other -> the PCM they returned, [channels, frames, 2]; the taker's channels read behind every call"""
    pcm, pos = [], 0
    for k, n in enumerate(calls):
        if each:
            each(f, k)
        pcm.append(f.process_host(x[:, pos:pos + n]))
        pos += n
        if taker and (read_every_call or k == len(calls) - 1):
            for c in taker.blocks:
                taker.read(f, c)
    return np.concatenate(pcm, axis=1)


def against_the_restatement(label, fmx_amd, blocks, pcm, mode, want, on_from=0, model=True):
    """the blocks `want` of one channel: present, equal to the restatement on the channel's own PCM bit for bit, and within the float64 model's bounds"""
    h = fmx_amd.feed_taps()
    assert sorted(blocks) == list(want), (label, sorted(blocks), list(want))
    if not want:
        return
    R = fm.blocks32(pcm, h, mode, on_from=on_from)
    assert set(want) <= set(R), (label, sorted(R)[:3], sorted(R)[-3:])
    diff = sum(int(np.count_nonzero(np.asarray(blocks[b][0]).view(np.uint32) != R[b][0].view(np.uint32))) for b in want)
    pdiff = sum(np.float32(blocks[b][1]).tobytes() != np.float32(R[b][1]).tobytes() for b in want)
    msg = "%s: %d blocks; %d samples and %d powers differ from the restatement" % (label, len(want), diff, pdiff)
    if model:
        ok, r = fm.check(label, blocks, fm.model64(pcm, h, mode, on_from=on_from), blocks=list(want), quiet=True)
        msg += "; against float64: worst |y - y64| / bound %.3f, worst |P - P64| / bound %.3f" % r
        assert ok, msg
    print(msg)
    assert diff == 0 and pdiff == 0, msg


# ---- a ------------------------------------------------------------------------------------------------------------------------------------------------
def test_modes_on_programme_tone_and_noise(fmx_amd, ol):
    """(a) nine channels on three streams -- programme, tone, noise --, channel c in mode 1 + c // 3, the odd cuts of CALLS_A, read behind every call"""
    x = three_signals(ol, sum(CALLS_A))
    f = make(fmx_amd, 9, streams=3, max_block=max(CALLS_A))
    for c in range(9):
        f.feed(1 + c // 3, c)
    t = Taker(range(9))
    pcm = run(f, x, CALLS_A, taker=t)
    assert all(r[0] == -1 for r in f.feed_read(0, 9))      # (read once: nothing is pending)
    assert f.feed_allocated() == 9 * fmx_amd.feed_info()["bytes_per_channel"]
    f.close()
    M = marks(CALLS_A)
    assert pcm.shape[1] == M[-1] and M[-1] // BF >= 14 and np.abs(pcm).max() > 0.05
    want = range(1, M[-1] // BF)
    print()
    for c in range(9):
        against_the_restatement("(a) %s, mode %d" % (("programme", "tone", "noise")[c % 3], 1 + c // 3), fmx_amd, t.blocks[c], pcm[c], 1 + c // 3, want)
    # every block arrived with the call that held its last frame
    done = [M[k + 1] // BF for k in range(len(CALLS_A))]
    assert t.runs[0] == [(max(1, M[k] // BF), done[k] - max(1, M[k] // BF)) for k in range(len(CALLS_A)) if done[k] > max(1, M[k] // BF)]
    assert not fm.same_blocks(t.blocks[0], t.blocks[3]) and not fm.same_blocks(t.blocks[3], t.blocks[6])      # (the programme's ears differ)


# ---- b ------------------------------------------------------------------------------------------------------------------------------------------------
def pcm_distance(label, a, b):
    d = np.nonzero(np.any(a != b, axis=(0, 2)))[0]
    print("%s: the PCM of the two cuts differs in %d of %d frames (first: %s), by %.2e at the most, of a peak of %.2f"
          % (label, d.size, a.shape[1], d[0] if d.size else None, float(np.max(np.abs(a - b))), float(np.max(np.abs(a)))))
    return d.size == 0


def block_distance(label, a, b):
    """prints how far the blocks of two runs are apart"""
    for c in a:
        common = sorted(set(a[c]) & set(b[c]))
        ya, yb = (np.concatenate([r[c][k][0] for k in common]).astype(np.float64) for r in (a, b))
        print("%s, channel %d: %d of %d samples differ, by %.2e at the most, of a peak of %.2f"
              % (label, c, int(np.count_nonzero(ya != yb)), ya.size, float(np.max(np.abs(ya - yb))), float(np.max(np.abs(ya)))))


def equal_where_the_pcm_is(label, a, pa, b, pb):
    """Per channel and block of both runs: where the 623 frames the block reads, [480 b - 143, 480 b + 480), are the same bytes in both runs' PCM, the
    block must be the same bytes too.  Prints how many blocks that held for."""
    held = total = 0
    for c in a:
        for k in sorted(set(a[c]) & set(b[c])):
            lo, hi = BF * k - fm.LOOKBACK, BF * k + BF
            total += 1
            if pa[c][lo:hi].tobytes() == pb[c][lo:hi].tobytes():
                held += 1
                assert fm.same_blocks(a[c], b[c], blocks=[k]), (label, c, k)
    print("%s: %d of %d blocks read the same PCM in both cuts, and are equal" % (label, held, total))
    return held


def test_one_call_against_many(fmx_amd, ol):
    """(b) the same stream in eleven odd calls and in one, with the constructor's settings and with cut_free's.  What the blocks of two cuts owe each
    other is equality WHERE THE PCM IS EQUAL -- asserted per block on the 623 frames it reads --; this chain's PCM depends on the cut in its last bits (tests/test_gpu_audio_meter.py
    test_one_call_against_many).  So under EITHER cut every block equals, bit for bit, the restatement -- one fixed function of the PCM and
    the frame count -- on that cut's own returned PCM.  The distances are printed."""
    m = fmx_amd.fmx
    many_calls = CALLS_A[:10] + [LUMP * 100]
    n = sum(many_calls)
    assert n <= min(1 << 20, sum(CALLS_A))
    x = three_signals(ol, sum(CALLS_A))[:, :n]
    nb = frames_at(n) // BF
    assert nb == 20
    print()
    for label, params in (("constructor's settings", []), ("cut_free", cut_free(m))):
        res = []
        for calls in (many_calls, [n]):
            f = make(fmx_amd, 3, max_block=n, params=params)
            for c in range(3):
                f.feed(1 + c, c)
            t = Taker(range(3))
            pcm = run(f, x, calls, taker=t, read_every_call=False)
            f.close()
            res.append((t.blocks, pcm))
        (many, pm), (one, po) = res
        equal = pcm_distance(label + ", eleven calls against one", pm, po)
        block_distance(label + ", eleven calls against one", many, one)
        for c in range(3):
            against_the_restatement(label + ", eleven calls, channel %d" % c, fmx_amd, many[c], pm[c], 1 + c, range(1, nb), model=False)
            against_the_restatement(label + ", one call, channel %d" % c, fmx_amd, one[c], po[c], 1 + c, range(1, nb), model=False)
        held = equal_where_the_pcm_is(label + ", eleven calls against one", many, pm, one, po)
        assert held == 3 * (nb - 1) or not equal


# ---- c ------------------------------------------------------------------------------------------------------------------------------------------------
def segments(modes):
    """[(k0, k1, mode)]: the runs of calls in one mode (a mode change ends a run as switching off does)"""
    out, k0 = [], None
    for k, v in enumerate(list(modes) + [0]):
        if k0 is not None and v != modes[k0]:
            out.append((k0, k, modes[k0]))
            k0 = None
        if v and k0 is None:
            k0 = k
    return out


def test_switching(fmx_amd, ol):
    """(c) on and off in mid-stream, a mode change, -1 for every channel: per run of calls in one mode the delivered blocks are exactly those from the
    first with 480 b - 143 >= the first frame of the call that switched the channel on to the last that ended inside the run -- the block in progress at
    the switch is dropped --, each equal to the restatement started at that frame; a reader that comes late gets one run per read, the gap in first_block"""
    ncalls, blk = 22, LUMP * 11                                  # 528 frames a call: a block and a lump
    x = three_signals(ol, ncalls * blk)
    M = marks([blk] * ncalls)
    modes = [[0 if k < 2 else 1 if k < 8 else 0 if k < 10 else 1 if k < 14 else 2 if k < 16 else 3 for k in range(ncalls)],
             [0 if k < 16 else 3 for k in range(ncalls)],
             [2 if k < 16 else 3 for k in range(ncalls)]]
    f = make(fmx_amd, 3, max_block=blk)

    def each(f, k):
        if k == 0:
            f.feed(2, 2)
        if k in (2, 10):
            f.feed(1, 0)
        if k == 8:
            f.feed(0, 0)
        if k == 5:
            assert f.feed_read(1, 1)[0][0] == -1                # (a channel that was never enabled, on a handle that feeds)
        if k == 14:
            f.feed(2, 0)
        if k == 16:
            f.feed(3, -1)
    t = Taker([2])
    pcm = run(f, x, [blk] * ncalls, each=each, taker=t)          # channel 2 is read behind every call, channels 0 and 1 at the end
    late = Taker([0, 1])
    for c in (0, 1):
        for _ in range(8):
            late.read(f, c)
    f.close()
    print()
    for c, got in ((0, late), (1, late), (2, t)):
        want_runs, seen = [], []
        for k0, k1, mode in segments(modes[c]):
            want = range(fm.first_block(M[k0]), M[k1] // BF)
            part = {b: got.blocks[c][b] for b in want if b in got.blocks[c]}
            against_the_restatement("(c) channel %d, calls %d .. %d, mode %d" % (c, k0, k1 - 1, mode), fmx_amd, part, pcm[c], mode, want, on_from=M[k0])
            want_runs.append((want[0], len(want)))
            seen += list(want)
        assert sorted(got.blocks[c]) == seen and len(seen) >= 5, (c, sorted(got.blocks[c]), seen)
        if c != 2:
            assert got.runs[c] == want_runs, (c, got.runs[c], want_runs)      # one run a read, up to the gap
    assert late.runs[0] == [(3, 5), (12, 3), (16, 1), (18, 6)] and late.runs[1] == [(18, 6)]      # (528 frames a call: on at 1056, 5280, 7392, 8448)


# ---- d ------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_scanning_channels_blocks_are_zeros(fmx_amd, ol):
    """(d) a channel that scans for a while: its PCM is zeros, its blocks are delivered and are zeros once the filter has run out of the programme"""
    m = fmx_amd.fmx
    ncalls, blk = 12, LUMP * 21
    x = three_signals(ol, ncalls * blk)[:2]
    M = marks([blk] * ncalls)
    f = make(fmx_amd, 2, max_block=blk)
    f.feed(1)
    t = Taker([0, 1])
    pcm = run(f, x, [blk] * ncalls, each=lambda f, k: f.set_param(m.P_SCANNING, 1 if 3 <= k < 8 else 0, 0), taker=t)
    f.close()
    assert not np.any(pcm[0, M[3]:M[8]]) and np.any(pcm[0, M[8]:]) and np.any(pcm[1, M[3]:M[8]])
    want = range(1, M[-1] // BF)
    print()
    for c in (0, 1):
        against_the_restatement("(d) channel %d" % c, fmx_amd, t.blocks[c], pcm[c], 1, want)
    inside = [b for b in want if BF * b - fm.LOOKBACK >= M[3] and BF * b + BF <= M[8]]
    assert len(inside) >= 8
    for b in inside:
        assert not t.blocks[0][b][0].view(np.uint32).any() and np.float32(t.blocks[0][b][1]).tobytes() == b"\0\0\0\0"
    assert np.any(t.blocks[0][inside[0] - 1][0]) and np.any(t.blocks[0][want[-1]][0]) and np.any(t.blocks[1][inside[3]][0])


# ---- e ------------------------------------------------------------------------------------------------------------------------------------------------
def ring_handle(fmx_amd, x, calls, mode=1):
    f = fmx_amd.Fmx(2, streams=1, stream_of_channel=[0, 0], max_block=max(calls), inputRate=192000)
    f.feed(mode)
    pcm = run(f, x, calls)
    return f, pcm


def test_ring_and_read_out(fmx_amd, ol):
    """(e) At inputRate 192 000 (4 input samples a frame) 141 blocks unread leave the last 128, and the loss shows in first_block; a capacity below what
    is pending leaves the rest for the next read; a failing read -- a bad range, a capacity of 0 with an audio buffer, an unknown format, null arrays --
    moves no cursor; S16 from one handle equals to_s16 of F32 from a twin on the same input; fmx_feed_read_device into device memory, as f32 and as 16 bit,
    equals fmx_feed_read of a twin."""
    import torch
    m = fmx_amd.fmx
    blk = 4 * (10 * BF + 48)                                     # ten blocks and a lump a call
    calls = [blk] * 14                                           # 67 872 frames: blocks 0 .. 140 complete
    x = ol.synth_iq(sum(calls), inputRate=192000)[None]
    fa, pcm = ring_handle(fmx_amd, x, calls)
    nb = pcm.shape[1] // BF
    assert nb == 141 and pcm.shape[1] == frames_at(sum(calls), 1)
    lost = nb - RING                                             # blocks 1 .. 12 were written over
    # a capacity below what is pending
    got = fa.feed_read(0, 2, capacity=10)
    assert [g[0] for g in got] == [lost, lost] and all(len(g[1]) == 10 for g in got) and got[0][1].tobytes() == got[1][1].tobytes()
    # failing reads move no cursor
    L = fa.L
    first, n, audio = np.zeros(2, np.int64), np.full(2, 7, np.int32), np.zeros((2, 8, BLOCK), np.float32)
    bad = [(L.fmx_feed_read(fa.h, 1, 2, first.ctypes.data, audio.ctypes.data, m.FEED_F32, None, 8, n.ctypes.data), "range"),
           (L.fmx_feed_read(fa.h, -1, 1, first.ctypes.data, audio.ctypes.data, m.FEED_F32, None, 8, n.ctypes.data), "range"),
           (L.fmx_feed_read(fa.h, 0, 2, first.ctypes.data, audio.ctypes.data, m.FEED_F32, None, 0, n.ctypes.data), "capacity"),
           (L.fmx_feed_read(fa.h, 0, 2, first.ctypes.data, audio.ctypes.data, 2, None, 8, n.ctypes.data), "format"),
           (L.fmx_feed_read(fa.h, 0, 2, first.ctypes.data, None, m.FEED_F32, None, 8, n.ctypes.data), "audio"),
           (L.fmx_feed_read(fa.h, 0, 2, first.ctypes.data, audio.ctypes.data, m.FEED_F32, None, -1, n.ctypes.data), "capacity"),
           (L.fmx_feed_read(fa.h, 0, 2, None, audio.ctypes.data, m.FEED_F32, None, 8, n.ctypes.data), "null"),
           (L.fmx_feed_read(fa.h, 0, 2, first.ctypes.data, audio.ctypes.data, m.FEED_F32, None, 8, None), "null"),
           (L.fmx_feed_read_device(fa.h, 0, 2, first.ctypes.data, None, 7, None, 8, n.ctypes.data, None), "format")]
    assert all(rc == m.FMX_E_INVALID for rc, _ in bad), bad
    assert not audio.any()
    with pytest.raises(m.FmxError) as e:
        fa.feed_read(0, 1, fmt=5)
    assert e.value.code == m.FMX_E_INVALID and "format" in str(e.value)
    with pytest.raises(m.FmxError):
        fa.feed(4, 0)
    with pytest.raises(m.FmxError):
        fa.feed(1, 2)
    rest = fa.feed_read(0, 2, capacity=RING)
    assert [g[0] for g in rest] == [lost + 10] * 2 and all(len(g[1]) == RING - 10 for g in rest)
    assert all(g[0] == -1 for g in fa.feed_read(0, 2))
    blocks = {lost + i: (a, p) for i, (a, p) in enumerate(zip(np.concatenate([got[0][1], rest[0][1]]), np.concatenate([got[0][2], rest[0][2]])))}
    print()
    against_the_restatement("(e) the ring's 128", fmx_amd, blocks, pcm[0], 1, range(lost, nb), model=False)
    assert fa.feed_read(0, 1, power=False)[0][2] is None
    fa.close()
    f32 = np.stack([blocks[b][0] for b in range(lost, nb)])
    pw = np.float32([blocks[b][1] for b in range(lost, nb)])
    # S16 from a twin
    fb, pcm_b = ring_handle(fmx_amd, x, calls)
    assert pcm_b.tobytes() == pcm.tobytes()
    s = fb.feed_read(0, 2, fmt="s16")
    assert s[0][0] == lost and s[0][1].dtype == np.int16 and s[0][1].shape == (RING, BLOCK)
    assert np.array_equal(s[0][1], fm.to_s16(f32)) and np.array_equal(s[1][1], s[0][1]) and s[0][2].tobytes() == pw.tobytes()
    assert np.abs(s[0][1]).max() > 1000
    fb.close()
    # the device read-outs of a twin: channel 0 as f32, channel 1 as 16 bit with a capacity of 100 and then the rest, powers on and off
    fc, pcm_c = ring_handle(fmx_amd, x, calls)
    assert pcm_c.tobytes() == pcm.tobytes()
    d_audio = torch.zeros((1, RING * BLOCK), dtype=torch.float32, device="cuda")
    d_power = torch.zeros((1, RING), dtype=torch.float32, device="cuda")
    assert fc.feed_read(0, 1, capacity=RING, device=(d_audio, d_power)) == [(lost, RING)]
    fc.synchronize()
    assert d_audio.cpu().numpy().reshape(RING, BLOCK).tobytes() == f32.tobytes() and d_power.cpu().numpy().tobytes() == pw.tobytes()
    d_s16 = torch.zeros((2, 100 * BLOCK), dtype=torch.int16, device="cuda")
    assert fc.feed_read(1, 1, capacity=100, fmt="s16", device=d_s16) == [(lost, 100)]
    fc.synchronize()
    assert np.array_equal(d_s16.cpu().numpy()[0].reshape(100, BLOCK), fm.to_s16(f32[:100]))
    # a range, given as an address: channel 0 has nothing pending, channel 1's rest goes to row 1
    assert fc.feed_read(0, 2, capacity=100, fmt="s16", device=d_s16.data_ptr()) == [(-1, 0), (lost + 100, RING - 100)]
    fc.synchronize()
    assert np.array_equal(d_s16.cpu().numpy()[1].reshape(100, BLOCK)[:RING - 100], fm.to_s16(f32[100:]))
    fc.close()
    # a range on the device against a twin's host read: both channels, the layout [channels, capacity x 160], three calls
    fd, _ = ring_handle(fmx_amd, x, calls[:3])
    d2 = torch.full((2, 40 * BLOCK), 7.0, dtype=torch.float32, device="cuda")
    p2 = torch.full((2, 40), 7.0, dtype=torch.float32, device="cuda")
    n3 = frames_at(3 * blk, 1) // BF - 1                      # blocks 1 .. 29
    assert n3 == 29 and fd.feed_read(0, 2, capacity=40, device=(d2, p2)) == [(1, n3), (1, n3)]
    fd.synchronize()
    h2, q2 = d2.cpu().numpy().reshape(2, 40, BLOCK), p2.cpu().numpy()
    fd.close()
    fe, _ = ring_handle(fmx_amd, x, calls[:3])
    host = fe.feed_read(0, 2, capacity=40)
    fe.close()
    for q in range(2):
        assert host[q][0] == 1 and h2[q, :n3].tobytes() == host[q][1].tobytes() and q2[q, :n3].tobytes() == host[q][2].tobytes()
        assert np.all(h2[q, n3:] == 7.0) and np.all(q2[q, n3:] == 7.0)      # (nothing is written behind a run)


def test_audio_rate_44100_is_refused(fmx_amd):
    """(h)"""
    m = fmx_amd.fmx
    f = fmx_amd.Fmx(1, max_block=16384, audioRate=44100)
    with pytest.raises(m.FmxError) as e:
        f.feed(1, 0)
    assert e.value.code == m.FMX_E_UNSUPPORTED and "48000" in str(e.value) and f.feed_allocated() == 0
    f.close()


# ---- f ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,feeding", [(1, {0: 1}), (2, {1: 2}), (65, {0: 1, 64: 3}), (130, {0: 1, 2: 2, 129: 3})])
def test_shapes(fmx_amd, ol, nch, feeding):
    """(f) 1, 2, 65 and 130 channels on at most three shared streams with a subset feeding; above 64 channels is the batch path"""
    calls = [LUMP * 21, LUMP * 9, LUMP * 31]
    x = three_signals(ol, sum(CALLS_A))[:min(nch, 3), :sum(calls)]
    f = make(fmx_amd, nch, streams=min(nch, 3) if nch > 1 else 0, max_block=max(calls))
    for c, mode in feeding.items():
        f.feed(mode, c)
    pcm = run(f, x, calls)
    got = f.feed_read(0, nch)
    assert f.feed_allocated() == len(feeding) * fmx_amd.feed_info()["bytes_per_channel"]
    f.close()
    nb = pcm.shape[1] // BF
    assert nb == 6
    print()
    for c in range(nch):
        first, audio, power = got[c]
        if c not in feeding:
            assert first == -1 and len(audio) == 0
            continue
        assert first == 1
        against_the_restatement("(f) %d channels, channel %d" % (nch, c), fmx_amd, {1 + i: (audio[i], power[i]) for i in range(len(audio))}, pcm[c], feeding[c],
                                range(1, nb))


BATCH_ON = {0: 1, 767: 2, 768: 3, 1099: 1}


def batch(fmx_amd, x, calls, feed, channels=1100, params=()):
    """a batch on shared streams -> (PCM, the second channel group of the last call, its pieces, the blocks of BATCH_ON's channels, a read of others)"""
    f = make(fmx_amd, channels, streams=x.shape[0], max_block=max(calls), params=params)
    on = {min(c, channels - 1): mode for c, mode in BATCH_ON.items()}
    for c, mode in on.items() if feed else ():
        f.feed(mode, c)
    pcm = run(f, x, calls)
    t = Taker(on)
    for c in on:
        t.read(f, c)
    out = (pcm, f.last_second_group(), f.last_call_pieces(), t.blocks, f.feed_read(1, 3), on)
    f.close()
    return out


@pytest.fixture(scope="module")
def batch_x(ol):
    return np.stack([ol.synth_iq(2 * LUMP * 32, leftHz=500.0 + 300 * s, rightHz=900.0 + 200 * s) for s in range(3)])


def test_batch_two_channel_groups(fmx_amd, batch_x):
    """(f) 1100 channels in two channel groups, the feed on for the first and the last channel of both: the blocks equal the restatement; the second
    group is the same non-zero number and every channel's PCM the same bytes with the feed and without it"""
    calls = [LUMP * 32] * 2
    off = batch(fmx_amd, batch_x, calls, False)
    on = batch(fmx_amd, batch_x, calls, True)
    print("\n1100 channels: second group %d without the feed, %d with it" % (off[1], on[1]))
    assert off[1] == on[1] == 332
    assert off[0].shape[0] == 1100 and np.array_equal(off[0], on[0])
    assert all(len(b) == 0 for b in off[3].values()) and all(r[0] == -1 for r in on[4])
    nb = on[0].shape[1] // BF
    assert nb == 6
    for c, mode in on[5].items():
        against_the_restatement("(f) 1100 channels, channel %d" % c, fmx_amd, on[3][c], on[0][c], mode, range(1, nb))


def test_batch_overlapping_pieces(fmx_amd, batch_x):
    """(f) a 1024-channel PLL-decoder handle whose calls are made in overlapping pieces of 1536 fm samples (384 frames: less than a block) against the
    same calls made whole.  The PCM of the two differs in its last bits, so the blocks of BOTH are held against the restatement on their own PCM, bit
    for bit; the distances are printed."""
    m = fmx_amd.fmx
    calls = [LUMP * 32] * 2
    whole = batch(fmx_amd, batch_x, calls, True, 1024, [(m.P_FM_DECODER, 2), (m.P_CALL_PIECES, 0)])
    cut = batch(fmx_amd, batch_x, calls, True, 1024, [(m.P_FM_DECODER, 2), (m.P_CALL_PIECES, 1536)])
    assert whole[2] == 1 and cut[2] > 1
    print()
    equal = pcm_distance("pieces against whole calls", whole[0], cut[0])
    block_distance("pieces against whole calls", whole[3], cut[3])
    nb = whole[0].shape[1] // BF
    for c, mode in whole[5].items():
        against_the_restatement("(f) whole calls, channel %d" % c, fmx_amd, whole[3][c], whole[0][c], mode, range(1, nb), model=False)
        against_the_restatement("(f) %d pieces a call, channel %d" % (cut[2], c), fmx_amd, cut[3][c], cut[0][c], mode, range(1, nb), model=False)
    held = equal_where_the_pcm_is("pieces against whole calls", whole[3], {c: whole[0][c] for c in whole[5]}, cut[3], {c: cut[0][c] for c in whole[5]})
    assert held == len(whole[5]) * (nb - 1) or not equal


# ---- g ------------------------------------------------------------------------------------------------------------------------------------------------
def everything(f, channels):
    """what a handle delivers beside the feed"""
    some = sorted({0, min(1, channels - 1), channels - 1})
    return dict(meta=[bytes(f.meta(c)) for c in range(channels)], bits=[f.rds_bits(c).tobytes() for c in some], peaks=[f.peaks(c).tobytes() for c in some] if channels <= 64 else [b""],
                groups=[g.tobytes() for g in f.rds_groups(0, channels)],
                scan=[f.scan_results(c).tobytes() for c in some], mod=[r.tobytes() for r in f.mod_records()], audio=[r.tobytes() for r in f.audio_records()],
                rx=[r.tobytes() for r in f.rx_records()], rdsm=[r.tobytes() for r in f.rds_meter_records()],
                spec=[b"".join(a.tobytes() for a in f.spectrum_read(s)) for s in range(f.streams)],
                mpx=[b"".join(a.tobytes() for a in r) for r in f.mpx_spectrum_read(0, channels)],
                sca=[(r[0], r[1].tobytes(), r[2].tobytes()) for r in f.sca_read(0, channels)],
                facts=(f.last_second_group(), f.last_call_pieces(), f.last_front_kernel()))


@pytest.mark.parametrize("channels", [1, 130])
def test_everything_else_is_undisturbed(fmx_amd, ol, channels):
    """(g) With every channel feeding, PCM, RDS bits and groups, meta, peaks, scan records, every meter's records, the SCA blocks and the facts about the
    last call equal a twin handle's that never feeds, byte for byte: on a 1-channel block-machine handle and on a batch of 130 channels on 3 shared
    streams (whose last channel scans).  The twin reports no allocation for the feed."""
    m = fmx_amd.fmx
    blk, ncalls = 16384, 24
    streams = 1 if channels == 1 else 3
    x = np.stack([ol.synth_iq(ncalls * blk, rds=1, leftHz=500.0 + 300 * s, rightHz=900.0 + 200 * s) for s in range(streams)])
    out = []
    for feed in (False, True):
        f = fmx_amd.Fmx(channels, streams=streams if channels > 1 else 0, stream_of_channel=[c % streams for c in range(channels)] if channels > 1 else None,
                        max_block=blk)
        f.set_param(m.P_BANDWIDTH, 165000)
        f.set_param(m.P_RDS_MODE, 2)
        if channels > 1:
            f.set_param(m.P_SCANNING, 1, channels - 1)
        f.mod_meter(True); f.audio_meter(True); f.rx_meter(True); f.rds_meter_enable(True)
        f.spectrum_setup(2, 1); f.spectrum_meter(True)
        f.mpx_spectrum_setup(2, 1); f.mpx_spectrum_meter(True)
        f.sca_enable(67000)
        if feed:
            f.feed(1)
        pcm = np.concatenate([f.process_host(x[:, k * blk:(k + 1) * blk]) for k in range(ncalls)], axis=1)
        e = everything(f, channels)
        e["pcm"] = pcm
        e["feed"] = f.feed_read(0, channels)
        e["allocated"] = f.feed_allocated()
        out.append(e)
        f.close()
    a, b = out
    assert np.array_equal(a["pcm"], b["pcm"]) and a["pcm"].shape[1] > 0
    for key in ("meta", "bits", "groups", "peaks", "scan", "mod", "audio", "rx", "rdsm", "spec", "mpx", "sca", "facts"):
        assert a[key] == b[key], key
    assert len(a["bits"][0]) > 0 and len(a["mod"][0]) > 0 and len(a["audio"][0]) > 0 and len(a["rx"][0]) > 0 and len(a["rdsm"][0]) > 0 and len(a["spec"][0]) > 0 and len(a["mpx"][0]) > 0
    assert a["sca"][0][0] == 1 and len(a["sca"][0][1]) > 0
    assert a["allocated"] == 0 and all(r[0] == -1 and len(r[1]) == 0 for r in a["feed"])
    assert b["allocated"] == channels * fmx_amd.feed_info()["bytes_per_channel"]
    nb = a["pcm"].shape[1] // BF
    assert all(r[0] == 1 and len(r[1]) == nb - 1 for r in b["feed"])       # (the scanning channel feeds on: its zeros)
    for c in sorted({0, channels - 1}):
        against_the_restatement("(g) %d channels, channel %d" % (channels, c), fmx_amd, {1 + i: (b["feed"][c][1][i], b["feed"][c][2][i]) for i in range(nb - 1)},
                                b["pcm"][c], 1, range(1, nb), model=False)
    if channels > 1:
        assert not b["feed"][channels - 1][1].view(np.uint32).any()


# ---- i ------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_cpp_demo_builds_and_runs(fmx_amd, ol, tmp_path):
    """(i) tests/feed_demo through host/fm_processor_adapter.h: blocks of 16 384: the blocks the Python handle delivers for the same stream"""
    import test_feed_cpu
    exe, fin, fout = str(tmp_path / "feed_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "feed.bin")
    test_feed_cpu.build_demo(fmx_amd, exe)
    x = ol.synth_iq(24 * 16384)[None]
    x[0].tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    f = fmx_amd.Fmx(1, max_block=16384)
    f.feed(1)
    t = Taker([0])
    run(f, x, [16384] * 23, taker=t)
    f.close()
    nb = frames_at(23 * 16384) // BF
    assert out.returncode == 0 and lines[-1] == "blocks %d first 1" % (nb - 1) and lines[-2].startswith("s16 blocks ") and lines[-2].endswith("peak nonzero"), lines
    rows = np.fromfile(fout, np.float32).reshape(-1, 2 + BLOCK)
    assert [int(v) for v in rows[:, 0]] == sorted(t.blocks[0]) == list(range(1, nb))
    assert all(rows[i, 2:].tobytes() == t.blocks[0][b][0].tobytes() and rows[i, 1].tobytes() == np.float32(t.blocks[0][b][1]).tobytes() for i, b in enumerate(sorted(t.blocks[0])))

"""The programme audio meter on the GPU (fmx_audio_meter_enable, fmx_audio_records; csrc/fmx_loud.hip).  The model's input is the handle's
own returned PCM: every field of every record must EQUAL the f32 restatement of tests/loud_model.py bit for bit (no transcendental function is involved);
the distance from the float64 model is printed beside it.  Then: the records' independence of how the stream is cut into calls and pieces, the switching
rules, a scanning channel's zeros, the ring and its read-out, the kernel's shapes, batches in two channel groups, the isolation of everything else a
handle delivers, and the calibration in LUFS."""
import numpy as np
import pytest

import loud_model as lm

pytestmark = pytest.mark.gpu

W = lm.WINDOW
# (a)'s calls in input samples (48 per PCM frame): around a frame, around the kernel's tile of 64 frames, around a window; a call of no frame; the
# receiver's block; then two windows and a bit, on to nine windows
CALLS_A = [48 * k for k in (1, 63, 64, 65, 4799, 4800, 4801)] + [12, 16384] + [48 * (2 * 4800 + 37)] * 3
TONE = dict(stereo=0, leftHz=1000.0, rightHz=1000.0, leftAmp=1.0, rightAmp=1.0, deviationHz=37500.0 / 0.9)
NOISE = dict(carrierAmp=0.0, noiseSeed=11, noiseSigma=0.3)


def three_signals(ol, n):
    """a stereo programme, a mono tone and noise"""
    return np.stack([ol.synth_iq(n), ol.synth_iq(n, **TONE), ol.synth_iq(n, **NOISE)])


def frames_at(n_samples):
    """PCM frames a handle at 2 304 000 S/s has delivered after n_samples input samples"""
    return 48 * ((n_samples // 12) // 192)


def make(fmx_amd, channels, streams=0, max_block=16384, params=(), **kw):
    m = fmx_amd.fmx
    som = [c % streams for c in range(channels)] if streams else None
    f = fmx_amd.Fmx(channels, streams=streams, stream_of_channel=som, max_block=max_block, **kw)
    f.set_param(m.P_BANDWIDTH, 165000)
    for item in params:
        f.set_param(*item)
    return f


def run(f, x, calls, each=None):
    """the calls of `calls` input samples behind each other -> the PCM they returned, [channels, frames, 2]"""
    pcm, pos = [], 0
    for k, n in enumerate(calls):
        if each:
            each(f, k)
        pcm.append(f.process_host(x[:, pos:pos + n]))
        pos += n
    return np.concatenate(pcm, axis=1)


def same(a, b):
    return len(a) == len(b) and all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def report_difference(label, a, b):
    """prints how far two lists of records are apart, field by field (relative to the field's largest magnitude), before a test asserts anything of them"""
    for name in lm.FIELDS:
        worst, differing, total = 0.0, 0, 0
        for p, q in zip(a, b):
            k = min(p.size, q.size)
            if k == 0:
                continue
            u, v = p[name][:k].astype(np.float64), q[name][:k].astype(np.float64)
            worst = max(worst, float(np.max(np.abs(u - v)) / max(np.max(np.abs(u)), 1e-30)))
            differing += int(np.count_nonzero(lm.bits(p[name][:k]) != lm.bits(q[name][:k])))
            total += k
        print("%s: %s differs in %d of %d records, by %.2e of its magnitude at the most" % (label, name, differing, total, worst))


def cut_free(m):
    """The settings under which the demodulator output and the pilot phase do not depend on how the stream is cut (tests/test_gpu_mod_meter.py says why:
    with the constructor's settings stage A removes the RF DC in tiles and stage B evaluates the AFC in segments that begin with the call).  The PCM
    behind them still does: test_one_call_against_many."""
    return [(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0)]


@pytest.fixture(scope="module")
def x_a(ol):
    return three_signals(ol, sum(CALLS_A))


@pytest.fixture(scope="module")
def case_a(fmx_amd, x_a):
    """three channels, every audio meter on from the first call"""
    f = make(fmx_amd, 3, max_block=max(CALLS_A))
    f.audio_meter(True)
    pcm = run(f, x_a, CALLS_A)
    recs = f.audio_records(capacity=64)
    assert f.audio_records(capacity=64)[0].size == 0      # (read once: nothing is pending)
    f.close()
    return pcm, recs


def test_odd_cuts_against_the_restatement(case_a):
    """(a) calls of 1, 63, 64, 65, 4799, 4800 and 4801 frames, of none, of the receiver's block, of two windows and a bit"""
    pcm, recs = case_a
    nwin = pcm.shape[1] // W
    assert nwin >= 8 and pcm.shape[1] == frames_at(sum(CALLS_A))
    assert np.abs(pcm).max() > 0.05
    lm.check_channels(recs, pcm, expect_index=range(nwin), verbose=True, label="(a) odd cuts")


def pcm_distance(label, a, b):
    """prints how far the PCM of two cuts is apart"""
    d = np.nonzero(np.any(a != b, axis=(0, 2)))[0]
    print("%s: the PCM of the two cuts differs in %d of %d frames (first: %s), by %.2e at the most, of a peak of %.2f"
          % (label, d.size, a.shape[1], d[0] if d.size else None, float(np.max(np.abs(a - b))), float(np.max(np.abs(a)))))
    return d.size == 0


def test_one_call_against_many(fmx_amd, x_a):
    """(b) the same stream in ten odd calls and in one (a call holds 1 048 576 input samples at the most: four windows), with the constructor's settings
    and with cut_free's.  What the records of two cuts owe each other is equality WHERE THE PCM IS EQUAL.  No setting was found under which this chain's
    PCM is: measured on an MI355X, the one call's PCM differs from the ten calls' in 20 924 of 20 928 frames from frame 1 on with the constructor's
    settings (1.7e-6 at the most) and in 20 921 under cut_free's (1.8e-7 with the block machines, 1.2e-6 with folded filters, mono and PSS off included); in every frame behind a first call the two cuts share (1.5e-7), even
    where every cut falls on a multiple of stage B's segment; a batch's overlapping pieces against whole calls in 10 223 of 10 224 frames (5.2e-8):
    DESIGN 4.12 says where that comes from.  So the test asserts what implies that equality and more: under EITHER cut every record equals, bit for bit,
    the restatement -- one fixed function of the PCM and the frame count -- on that cut's own returned PCM.  Two cuts with equal PCM therefore have equal
    records; two cuts whose PCM differs have records that differ by exactly what the PCM's difference makes of them.  The distances are printed."""
    m = fmx_amd.fmx
    many_calls = CALLS_A[:9] + [48 * 6000]
    n = sum(many_calls)
    nwin = frames_at(n) // W
    assert nwin == 4 and n <= 1 << 20
    for label, params in (("constructor's settings", []), ("cut_free", cut_free(m))):
        res = []
        for calls in (many_calls, [n]):
            f = make(fmx_amd, 3, max_block=n, params=params)
            f.audio_meter(True)
            pcm = run(f, x_a, calls)
            res.append((f.audio_records(), pcm))
            f.close()
        (many, pm), (one, po) = res
        equal = pcm_distance(label + ", ten calls against one", pm, po)
        report_difference(label + ", ten calls against one", many, one)
        lm.check_channels(many, pm, expect_index=range(nwin))
        lm.check_channels(one, po, expect_index=range(nwin))
        assert same(many, one) or not equal


def runs_of(on):
    """[(k0, k1)]: the runs of calls with the meter on"""
    out, k0 = [], None
    for k, v in enumerate(list(on) + [False]):
        if v and k0 is None:
            k0 = k
        if not v and k0 is not None:
            out.append((k0, k))
            k0 = None
    return out


def test_switching(fmx_amd, ol):
    """(c) on in mid-window, off and on again, per channel and with -1: the records are exactly the windows metered from their first frame to their last,
    and each run's equal the restatement started from zero at the first frame of the call that switched the meter on"""
    ncalls, blk = 24, 49152
    x = three_signals(ol, ncalls * blk)
    M = [frames_at(k * blk) for k in range(ncalls + 1)]
    on = [[3 <= k for k in range(ncalls)],                       # on in mid-window
          [k < 6 or 9 <= k for k in range(ncalls)],              # off, on again
          [k >= 15 for k in range(ncalls)]]                      # never enabled until -1
    res = []
    for only_first in (False, True):
        f = make(fmx_amd, 3, max_block=blk)

        def each(f, k):
            if k == 3:
                f.audio_meter(True, 0)
            if only_first:
                return
            if k == 0 or k == 9:
                f.audio_meter(True, 1)
            if k == 6:
                f.audio_meter(False, 1)
            if k == 5:
                assert f.audio_records(2, 1)[0].size == 0      # (a channel that was never enabled, on a handle whose meter runs)
            if k == 15:
                f.audio_meter(True, -1)
        pcm = run(f, x, [blk] * ncalls, each=each)
        res.append((pcm, f.audio_records()))
        f.close()
    (pcm, recs), (pcm1, recs1) = res
    assert M[-1] >= 5 * W
    for c in range(3):
        got = 0
        for k0, k1 in runs_of(on[c]):
            want = [w for w in range(M[-1] // W) if w * W >= M[k0] and (w + 1) * W <= M[k1]]
            part = recs[c][got:got + len(want)]
            lm.check_records(part, pcm[c], expect_index=want, start=M[k0])
            got += len(want)
        assert got == recs[c].size and got >= 1
    assert list(recs[0]["index"]) == [1, 2, 3, 4] and list(recs[1]["index"]) == [0, 2, 3, 4] and list(recs[2]["index"]) == [4]
    # switching the other channels leaves this one's records as they are
    assert pcm1.tobytes() == pcm.tobytes() and recs1[0].tobytes() == recs[0].tobytes() and recs1[1].size == 0 and recs1[2].size == 0


def test_scanning_channel_is_metered_as_its_zeros(fmx_amd, ol):
    """(d) a channel that scans for six windows and then stops: zeros while it scans -- the filter states walk down through the subnormals on the device
    -- and the restatement's records, bit for bit, before, during and after"""
    m = fmx_amd.fmx
    ncalls, blk = 45, 49152
    x = three_signals(ol, ncalls * blk)[:2]
    M = [frames_at(k * blk) for k in range(ncalls + 1)]
    f = make(fmx_amd, 2, max_block=blk)
    f.audio_meter(True)
    pcm = run(f, x, [blk] * ncalls, each=lambda f, k: f.set_param(m.P_SCANNING, 1 if 4 <= k < 32 else 0, 0))
    recs = f.audio_records()
    f.close()
    inside = [w for w in range(M[-1] // W) if w * W >= M[4] and (w + 1) * W <= M[32]]
    assert len(inside) >= 5 and not np.any(pcm[0, M[4]:M[32]]) and np.any(pcm[0, M[32]:]) and np.any(pcm[1, M[4]:M[32]])
    lm.check_channels(recs, pcm, expect_index=range(M[-1] // W), verbose=True, label="(d) scanning")
    r = recs[0]
    for name in ("peak_l", "peak_r", "ms_l", "ms_r", "cross"):
        assert not np.any(r[name][inside])
    assert r["kms_l"][inside[0]] > 0 and r["kms_l"][inside[-1]] == 0 and r["kms_r"][inside[-1]] == 0      # (the tail of the programme, then nothing)
    assert np.all(r["kms_l"][inside[-1] + 2:] > 1e-6)      # ... and the programme again


def test_ring_and_read_out(fmx_amd, ol):
    """(e) 70 windows unread leave the last 64; a capacity below what is pending leaves the rest for the next read; a range read equals per-channel reads
    (four channels on one stream: equal records); a range beyond the handle's channels and a handle at audioRate 44 100 are refused"""
    m = fmx_amd.fmx
    blk, ncalls = 4 * 5 * W + 192, 15                 # input samples = fm samples per call at inputRate 192 000: five windows and 48 frames
    x = ol.synth_iq(ncalls * blk, inputRate=192000)[None]
    f = fmx_amd.Fmx(4, streams=1, stream_of_channel=[0, 0, 0, 0], max_block=blk, inputRate=192000)
    f.audio_meter(True)
    pcm = run(f, x, [blk] * 14)
    assert pcm.shape[1] // W == 70
    first = f.audio_records(0, 2, capacity=10)
    assert list(first[0]["index"]) == list(range(6, 16)) and same(first, [first[1], first[0]])
    pcm = np.concatenate([pcm, run(f, x[:, 14 * blk:], [blk])], axis=1)      # (records 70 .. 74 arrive; 16 .. 69 are still there)
    rest = f.audio_records(0, 2, capacity=64)
    assert list(rest[0]["index"]) == list(range(16, 75))
    assert f.audio_records(0, 2)[0].size == 0
    single = [f.audio_records(2, 1, capacity=64)[0], f.audio_records(3, 1, capacity=64)[0]]
    assert list(single[0]["index"]) == list(range(11, 75))                  # (a reader that fell behind: the ring's 64)
    assert single[0][5:].tobytes() == rest[0].tobytes() and single[1][5:].tobytes() == rest[1].tobytes()
    for first_ch, count in ((3, 2), (4, 1), (-1, 1), (0, 5)):
        with pytest.raises(m.FmxError) as e:
            f.audio_records(first_ch, count)
        assert e.value.code == m.FMX_E_INVALID
    with pytest.raises(m.FmxError) as e:
        f.audio_meter(True, 4)
    assert e.value.code == m.FMX_E_INVALID
    f.close()
    # (75 windows are too many to walk frame by frame here: every field but the K-weighted pair against the restatement)
    lm.check_records(np.concatenate([first[0], rest[0]]), pcm[0], verbose=True, label="(e) ring", kweight=False)
    f = fmx_amd.Fmx(1, max_block=16384, audioRate=44100)
    with pytest.raises(m.FmxError) as e:
        f.audio_meter(True, 0)
    assert e.value.code == m.FMX_E_UNSUPPORTED and "48000" in str(e.value)
    f.close()


@pytest.mark.parametrize("nch,metered", [(1, None), (33, None), (65, None), (80, [79])])
def test_shapes(fmx_amd, ol, nch, metered):
    """(f) 1, 33 and 65 metered channels -- a single lane pair, a wave and one channel, two waves and one --, and 80 channels with only the last metered"""
    blk = 49152 * 5
    x = three_signals(ol, 2 * blk)
    f = make(fmx_amd, nch, streams=min(nch, 3), max_block=blk)
    if metered is None:
        f.audio_meter(True)
    for c in metered or []:
        f.audio_meter(True, c)
    pcm = run(f, x[:min(nch, 3)], [blk] * 2)
    recs = f.audio_records()
    f.close()
    on = list(range(nch)) if metered is None else metered
    assert all(recs[c].size == (2 if c in on else 0) for c in range(nch))
    lm.check_channels([recs[c] for c in on], pcm[on], expect_index=[0, 1], verbose=True, label="(f) %d channels" % nch)
    if nch > 3:
        assert recs[on[-1]].tobytes() == recs[on[-1] % 3 if metered is None else on[-1]].tobytes()


BATCH_ON = (0, 767, 768, 1099)


def batch(fmx_amd, x, calls, meter, params=()):
    """1100 channels on eight shared streams -> (PCM, the second channel group of the last call, its pieces, the records of BATCH_ON)"""
    f = make(fmx_amd, 1100, streams=8, max_block=max(calls), params=params)
    for c in BATCH_ON if meter else ():
        f.audio_meter(True, c)
    pcm = run(f, x, calls)
    out = (pcm, f.last_second_group(), f.last_call_pieces(), [f.audio_records(c, 1)[0] for c in BATCH_ON], f.audio_records(1, 3))
    f.close()
    return out


@pytest.fixture(scope="module")
def batch_x(ol):
    return np.stack([ol.synth_iq(2 * 49152 * 5, leftHz=500.0 + 300 * s, rightHz=900.0 + 200 * s) for s in range(8)])


def test_batch_two_channel_groups(fmx_amd, batch_x):
    """(g) 1100 channels, two windows and a bit, the meter on for the first and the last channel of both channel groups: the records equal the
    restatement; the second group is the same non-zero number and every channel's PCM the same bytes with the meter and without it"""
    calls = [49152 * 5] * 2
    off = batch(fmx_amd, batch_x, calls, False)
    on = batch(fmx_amd, batch_x, calls, True)
    print("1100 channels: second group %d without the audio meter, %d with it" % (off[1], on[1]))
    assert off[1] == on[1] == 332
    assert off[0].shape[0] == 1100 and np.array_equal(off[0], on[0])
    assert all(r.size == 0 for r in off[3]) and all(r.size == 0 for r in on[4])
    lm.check_channels(on[3], on[0][list(BATCH_ON)], expect_index=[0, 1], verbose=True, label="(g) 1100 channels")


def test_batch_overlapping_pieces(fmx_amd, batch_x):
    """(g) the same handle size with the PLL decoder, its calls made in overlapping pieces of 1536 fm samples against the same calls made whole.  The PCM
    of the two differs in its last bits (measured: 10 223 of 10 224 frames, 5.2e-8 at the most, with RF DC removal on or off and with either input
    filter kernel; test_one_call_against_many says what follows from that), so the records of BOTH are held against the restatement on their own PCM,
    bit for bit; the distances are printed."""
    m = fmx_amd.fmx
    calls = [49152 * 5] * 2
    whole = batch(fmx_amd, batch_x, calls, True, [(m.P_FM_DECODER, 2), (m.P_CALL_PIECES, 0)])
    cut = batch(fmx_amd, batch_x, calls, True, [(m.P_FM_DECODER, 2), (m.P_CALL_PIECES, 1536)])
    assert whole[2] == 1 and cut[2] >= 4
    equal = pcm_distance("pieces against whole calls", whole[0], cut[0])
    report_difference("pieces against whole calls", whole[3], cut[3])
    assert all(r.size == 2 for r in whole[3]) and all(r.size == 2 for r in cut[3])
    lm.check_channels(whole[3], whole[0][list(BATCH_ON)], expect_index=[0, 1])
    lm.check_channels(cut[3], cut[0][list(BATCH_ON)], expect_index=[0, 1], verbose=True, label="(g) 13 pieces per call")
    assert same(whole[3], cut[3]) or not equal


def test_other_outputs_unchanged(fmx_amd, ol):
    """(h) three channels -- one decodes RDS, one scans for a while --, the modulation meter on: PCM, modulation records, meta, peaks, scan records and
    RDS bits are bit-identical with the audio meter on and off"""
    m = fmx_amd.fmx
    ncalls, blk = 40, 16384                             # (54 613 fm samples: the RDS path has completed a block of 32 000)
    x = three_signals(ol, ncalls * blk)
    x[0] = ol.synth_iq(ncalls * blk, rds=1)
    out = []
    for meter in (False, True):
        f = make(fmx_amd, 3, max_block=blk, params=[(m.P_RDS_MODE, 2, 0)])
        f.mod_meter(True)
        if meter:
            f.audio_meter(True)
        pcm = run(f, x, [blk] * ncalls, each=lambda f, k: f.set_param(m.P_SCANNING, 1 if 4 <= k < 12 else 0, 1))
        meta = [bytes(f.meta(c)) for c in range(3)]
        out.append((pcm, meta, [f.peaks(c) for c in range(3)], f.scan_results(1), [f.rds_bits(c) for c in range(3)], f.mod_records(), f.audio_records()))
        f.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2])) and a[2][0].shape[0] > 0
    assert a[3].tobytes() == b[3].tobytes() and a[3].size >= 8
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4])) and a[4][0].size > 0
    assert same(a[5], b[5]) and a[5][0].size >= 5
    assert all(r.size == 0 for r in a[6])
    nwin = frames_at(ncalls * blk) // W
    lm.check_channels(b[6], b[0], expect_index=range(nwin))


def test_calibration(fmx_amd, case_a):
    """(i) the mono tone's loudness from the GPU's records against the float64 model's on the same PCM"""
    pcm, recs = case_a
    got = fmx_amd.fmx.loudness(recs[1])
    want = lm.loudness_numpy(lm.records_f64(pcm[1]))
    print("mono tone: momentary %.3f LUFS (float64 model %.3f), integrated %.3f (%.3f), correlation %.6f"
          % (got["momentary_lufs"], want["momentary_lufs"], got["integrated_lufs"], want["integrated_lufs"], got["correlation"]))
    assert abs(got["momentary_lufs"] - want["momentary_lufs"]) <= 0.01 and np.isfinite(got["momentary_lufs"])
    assert got["correlation"] > 0.999

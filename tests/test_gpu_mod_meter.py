"""The modulation meter on the GPU (fmx_mod_meter_enable, fmx_mod_records; csrc/fmx_meter.hip): the records against the float64 model
and the f32 restatement of tests/meter_model.py on the handle's own taps, their independence of how the stream is cut into calls and pieces, the
switching rules, the ring and its read-out, the isolation of everything else a handle delivers, and the calibration of the three figures on signals of
known deviation."""
import numpy as np
import pytest

import meter_model as mm

pytestmark = pytest.mark.gpu

W = mm.WINDOW
HZ = 47261.5
TONE_PEAK_TOL_HZ = 2 * 816.3          # twice the oracle's own distance from 37 500 Hz on this signal (tests/test_meter_cpu.py)
# (a)'s calls in input samples: the receiver's block, one fm sample, around a step of 64, one sample short of a window, two windows and a bit; then on
# to eleven windows
CALLS_A = [16384, 12, 12 * 63, 12 * 64, 12 * 65, 12 * 9599, 12 * (2 * 9600 + 37)] + [12 * (2 * 9600 + 37)] * 4
TONE = dict(stereo=0, leftHz=1000.0, rightHz=1000.0, leftAmp=1.0, rightAmp=1.0, deviationHz=37500.0 / 0.9)
NOISE = dict(carrierAmp=0.0, noiseSeed=11, noiseSigma=0.3)


def three_signals(ol, n):
    """a stereo signal, a mono tone at +-37 500 Hz and noise"""
    return np.stack([ol.synth_iq(n), ol.synth_iq(n, **TONE), ol.synth_iq(n, **NOISE)])


def make(fmx_amd, channels, streams=0, max_block=16384, params=(), **kw):
    m = fmx_amd.fmx
    som = [c % streams for c in range(channels)] if streams else None
    f = fmx_amd.Fmx(channels, streams=streams, stream_of_channel=som, max_block=max_block, **kw)
    f.set_param(m.P_BANDWIDTH, 165000)
    for item in params:
        f.set_param(*item)
    return f


def run(f, m, x, calls, tap_ch=(), each=None):
    """the calls of `calls` input samples behind each other; returns (pcm, {ch: (d, phi)} read from the two taps after every call)"""
    taps = {c: ([], []) for c in tap_ch}
    pcm, pos = [], 0
    for k, n in enumerate(calls):
        if each:
            each(f, k)
        pcm.append(f.process_host(x[:, pos:pos + n]))
        pos += n
        nj = f.last_fm_samples()
        for c in tap_ch:
            if nj > 0:
                taps[c][0].append(f.tap(m.TAP_DEMOD, nj, c))
                taps[c][1].append(f.tap(m.TAP_PILOT_PHASE, nj, c))
    return np.concatenate(pcm, axis=1), {c: (np.concatenate(v[0]), np.concatenate(v[1])) for c, v in taps.items()}


def same(a, b):
    return len(a) == len(b) and all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def report_difference(label, a, b):
    """prints how far two lists of records are apart, field by field (relative to the field's largest magnitude), before a test asserts that they are equal"""
    for name in mm.FIELDS_EXACT + mm.FIELDS_PILOT:
        worst, differing, total = 0.0, 0, 0
        for p, q in zip(a, b):
            k = min(p.size, q.size)
            if k == 0:
                continue
            u, v = p[name][:k].astype(np.float64), q[name][:k].astype(np.float64)
            worst = max(worst, float(np.max(np.abs(u - v)) / max(np.max(np.abs(u)), 1e-30)))
            differing += int(np.count_nonzero(mm.bits(p[name][:k]) != mm.bits(q[name][:k])))
            total += k
        print("%s: %s differs in %d of %d records, by %.2e of its magnitude at the most" % (label, name, differing, total, worst))


@pytest.fixture(scope="module")
def case_a(fmx_amd, ol):
    """three channels, scope taps on by default (the block machines), every meter on from the first call"""
    m = fmx_amd.fmx
    x = three_signals(ol, sum(CALLS_A))
    f = make(fmx_amd, 3, max_block=max(CALLS_A))
    f.mod_meter(True)
    _, taps = run(f, m, x, CALLS_A, tap_ch=(0, 1, 2))
    recs = f.mod_records(capacity=64)
    assert f.mod_records(capacity=64)[0].size == 0      # (read once: nothing is pending)
    f.close()
    return x, taps, recs


def test_records_against_the_model_on_the_handles_taps(case_a):
    """(a) calls of 16384, 12, 12 x 63, 12 x 64, 12 x 65, 12 x 9599 and 12 x (2 x 9600 + 37) input samples and on"""
    _, taps, recs = case_a
    nwin = (sum(CALLS_A) // 12) // W
    assert nwin >= 5
    for c in range(3):
        err, bound = mm.check_records(recs[c], taps[c][0], taps[c][1], expect_index=range(nwin), verbose=True)
        assert err <= bound


def cut_free(m):
    """Settings under which the meter's INPUTS do not depend on how the stream is cut, so that records of two cuts can be compared bit for bit.  A record is
    a function of d, phi and the window grid alone.  With the constructor's settings d itself depends on the cut in its last bits: stage A removes the RF
    DC in tiles that begin with the call, stage B evaluates the AFC as a scan over segments that do (measured, eleven calls against one, 80 800 fm
    samples: FMX_TAP_DEMOD differs in 11 811 samples, FMX_TAP_FM_IQ in 6 546; the records then differ in their last bits too -- mean by 2.3e-6 of its
    magnitude at the most, the small pilot component by 2.2e-5).  The PLL decoder's demodulator runs in the pre-pass, a recurrence in sample
    order whatever the call, and without RF DC removal the input side has no tiles: those handles' taps are bit-identical across cuts (asserted below)."""
    return [(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0)]


def test_one_call_against_many(fmx_amd, case_a):
    """(b) the same stream in eleven calls and in one call: the records are bit-identical (on handles whose taps are: cut_free).  With the constructor's
    settings the one call's records are checked on the one call's own taps, and their distance from the eleven calls' is printed."""
    m = fmx_amd.fmx
    x, _, recs = case_a
    n = 12 * (8 * W + 4000)
    f = make(fmx_amd, 3, max_block=n)
    f.mod_meter(True)
    _, taps = run(f, m, x, [n], tap_ch=(0, 1, 2))
    one = f.mod_records()
    f.close()
    for c in range(3):
        mm.check_records(one[c], taps[c][0], taps[c][1], expect_index=range(8))
    report_difference("constructor's settings, one call against many", one, [r[:8] for r in recs])
    res = []
    for calls in (CALLS_A, [n]):
        f = make(fmx_amd, 3, max_block=max(calls), params=cut_free(m))
        f.mod_meter(True)
        _, taps = run(f, m, x, calls, tap_ch=(0, 1, 2))
        res.append((f.mod_records(), taps))
        f.close()
    (many, tm), (one, to) = res
    for c in range(3):
        for k in range(2):
            assert tm[c][k][:n // 12].tobytes() == to[c][k].tobytes(), (c, k)      # (the premise: the same d and phi from both cuts)
        mm.check_records(one[c], to[c][0], to[c][1], expect_index=range(8))
        assert one[c].size == 8 and one[c].tobytes() == many[c][:8].tobytes(), c


def expected_windows(J, on):
    """the windows that leave a record: complete, and the meter on in every call that covered one of their samples"""
    out = []
    for w in range(J[-1] // W):
        cover = [k for k in range(len(on)) if J[k] < (w + 1) * W and J[k + 1] > w * W]
        if all(on[k] for k in cover):
            out.append(w)
    return out


def test_switching(fmx_amd, ol):
    """(c) on in mid-window, off and on again, per channel and with -1, a channel never enabled until then"""
    m = fmx_amd.fmx
    ncalls, blk = 36, 16384
    x = three_signals(ol, ncalls * blk)
    J = [(k * blk) // 12 for k in range(ncalls + 1)]
    on = [[3 <= k for k in range(ncalls)],                               # on in mid-window
          [k < 10 or 14 <= k < 20 or k >= 28 for k in range(ncalls)],   # off, on again; off again, then on by -1
          [k >= 28 for k in range(ncalls)]]                             # never enabled until -1
    f = make(fmx_amd, 3, max_block=blk)

    def each(f, k):
        if k == 0:
            f.mod_meter(True, 1)
        if k == 3:
            f.mod_meter(True, 0)
        if k == 10 or k == 20:
            f.mod_meter(False, 1)
        if k == 14:
            f.mod_meter(True, 1)
        if k == 5:
            assert f.mod_records(2, 1)[0].size == 0      # (a channel that was never enabled, on a handle whose meter runs)
        if k == 28:
            f.mod_meter(True, -1)
    _, taps = run(f, m, x, [blk] * ncalls, tap_ch=(0, 1, 2), each=each)
    recs = f.mod_records()
    f.close()
    for c in range(3):
        want = expected_windows(J, on[c])
        assert len(want) >= 1
        mm.check_records(recs[c], taps[c][0], taps[c][1], expect_index=want)
    assert recs[0]["index"][0] == 1 and recs[2]["index"][0] == -(-J[28] // W)
    assert list(recs[1]["index"]) == [0, 4]                              # (the gaps in `index`: windows 1 .. 3 met a call with the meter off)


def test_ring_keeps_64_and_capacity_leaves_the_rest(fmx_amd, ol):
    """(d) 70 windows unread leave the last 64; a capacity below what is pending leaves the rest for the next read.  (j) a handle at inputRate 192 000:
    the records against the model on its taps."""
    m = fmx_amd.fmx
    blk, ncalls = 5 * W + 40, 15                      # 48 040 fm samples = input samples per call: 75 windows and a bit in all
    x = ol.synth_iq(ncalls * blk, inputRate=192000)[None]
    f = fmx_amd.Fmx(1, max_block=blk, inputRate=192000)
    f.mod_meter(True, 0)
    _, taps = run(f, m, x, [blk] * 14, tap_ch=(0,))
    assert (14 * blk) // W == 70
    first = f.mod_records(0, 1, capacity=10)[0]
    assert list(first["index"]) == list(range(6, 16))
    run(f, m, x[:, 14 * blk:], [blk])                 # (records 70 .. 74 arrive; 16 .. 69 are still there)
    rest = f.mod_records(0, 1, capacity=64)[0]
    assert list(rest["index"]) == list(range(16, 75))
    assert f.mod_records(0, 1)[0].size == 0
    f.close()
    mm.check_records(np.concatenate([first, rest[:54]]), taps[0][0], taps[0][1], verbose=True)


def test_other_outputs_unchanged_three_channels(fmx_amd, ol):
    """(e) PCM, meta, peaks, scan records and RDS bits of three channels -- one decodes RDS, one scans for a while -- are bit-identical with the meter on
    and off.  (k) the scanning channel's meter runs on."""
    m = fmx_amd.fmx
    ncalls, blk = 40, 16384                             # (54 613 fm samples: the RDS path has completed a block of 32 000)
    x = three_signals(ol, ncalls * blk)
    x[0] = ol.synth_iq(ncalls * blk, rds=1)
    out = []
    for meter in (False, True):
        f = make(fmx_amd, 3, max_block=blk, params=[(m.P_RDS_MODE, 2, 0)])
        if meter:
            f.mod_meter(True)
        pcm, taps = run(f, m, x, [blk] * ncalls, tap_ch=(1,), each=lambda f, k: f.set_param(m.P_SCANNING, 1 if 4 <= k < 12 else 0, 1))
        meta = [bytes(f.meta(c)) for c in range(3)]
        out.append((pcm, meta, [f.peaks(c) for c in range(3)], f.scan_results(1), [f.rds_bits(c) for c in range(3)], f.mod_records(), taps))
        f.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2])) and a[2][0].shape[0] > 0
    assert a[3].tobytes() == b[3].tobytes() and a[3].size >= 8
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4])) and a[4][0].size > 0
    assert all(r.size == 0 for r in a[5])
    nwin = (ncalls * blk // 12) // W
    assert all(list(r["index"]) == list(range(nwin)) for r in b[5])
    mm.check_records(b[5][1], b[6][1][0], b[6][1][1])                 # the scanning channel


@pytest.mark.parametrize("nch", [800, 1100])
def test_other_outputs_unchanged_batch(fmx_amd, ol, nch):
    """(e) PCM of 800 channels on four shared streams with one channel metered: bit-identical.  The metered handle keeps the rows and runs its stereo /
    audio stages as one channel group.  Whether the handle WITHOUT the meter runs two groups is fmx_plan.h's arithmetic: 768 workgroup slots on 256 compute
    units and a second group of 128 channels at the least -- 800 channels leave 32 and stay one group (measured: fmx_last_second_group () == 0), so
    the same comparison is made at 1100 channels as well, where the unmetered handle does run two groups (768 + 332) and the metered one does not."""
    m = fmx_amd.fmx
    blk, ncalls = 49152, 3
    x = np.stack([ol.synth_iq(ncalls * blk, leftHz=500.0 + 300 * s, rightHz=900.0 + 200 * s) for s in range(4)])
    res = []
    for meter in (False, True):
        f = make(fmx_amd, nch, streams=4, max_block=blk)
        if meter:
            f.mod_meter(True, 517)
        pcm, _ = run(f, m, x, [blk] * ncalls)
        res.append((pcm, f.last_second_group(), f.mod_records(510, 10)))
        f.close()
    print("%d channels: second group %d without the meter, %d with it" % (nch, res[0][1], res[1][1]))
    assert res[0][1] == (332 if nch == 1100 else 0) and res[1][1] == 0
    assert np.array_equal(res[0][0], res[1][0])
    assert [r.size for r in res[1][2]] == [0] * 7 + [1] + [0] * 2 and res[1][2][7]["index"][0] == 0


def batch_records(fmx_amd, x, calls, params, tap_ch=(), max_block=None):
    """130 channels on three streams, every meter on -> (records of every channel, taps, the handle's last call in pieces)"""
    m = fmx_amd.fmx
    f = make(fmx_amd, 130, streams=3, max_block=max_block or max(calls), params=params)
    f.mod_meter(True)
    _, taps = run(f, m, x, calls, tap_ch=tap_ch)
    recs, pieces = f.mod_records(), f.last_call_pieces()
    f.close()
    return recs, taps, pieces


@pytest.fixture(scope="module")
def batch_x(ol):
    return three_signals(ol, 6 * 49152)


def test_batch_taps_off_by_default(fmx_amd, batch_x):
    """(f) 130 channels, the scope taps off by default: the records equal those of the same handle with FMX_P_SCOPE_TAPS = 1, and those the model"""
    m = fmx_amd.fmx
    calls = [49152] * 6
    off, _, _ = batch_records(fmx_amd, batch_x, calls, [])
    on, taps, _ = batch_records(fmx_amd, batch_x, calls, [(m.P_SCOPE_TAPS, 1)], tap_ch=(0, 1, 2, 129))
    assert all(r.size == 2 for r in off) and same(off, on)
    for c in (0, 1, 2, 129):
        mm.check_records(on[c], taps[c][0], taps[c][1], expect_index=[0, 1], verbose=c == 0)
    assert on[0].tobytes() == on[3].tobytes() and on[0].tobytes() != on[1].tobytes()


def test_batch_overlapping_pieces(fmx_amd, batch_x):
    """(g) the PLL decoder's batch, calls made in overlapping pieces of 1536 fm samples, against the same calls made whole"""
    m = fmx_amd.fmx
    calls = [98304] * 3
    whole, _, p0 = batch_records(fmx_amd, batch_x, calls, [(m.P_FM_DECODER, 2), (m.P_CALL_PIECES, 0)])
    cut, _, p1 = batch_records(fmx_amd, batch_x, calls, [(m.P_FM_DECODER, 2), (m.P_CALL_PIECES, 1536)])
    assert p0 == 1 and p1 >= 4
    report_difference("pieces against whole calls", whole, cut)
    assert all(r.size == 2 for r in whole) and same(whole, cut)


def test_batch_stage_b_forms(fmx_amd, batch_x):
    """(i) stage B as one kernel against two"""
    m = fmx_amd.fmx
    calls = [49152] * 6
    one, _, _ = batch_records(fmx_amd, batch_x, calls, [(m.P_STAGEB_FORM, 1)])
    two, _, _ = batch_records(fmx_amd, batch_x, calls, [(m.P_STAGEB_FORM, 2)])
    assert all(r.size == 2 for r in one) and same(one, two)


def test_rds_pieces(fmx_amd, ol):
    """(h) one RDS channel, one call of 400 000 input samples (made in RDS pieces) against the same stream in small calls: bit-identical records, on a
    handle whose taps do not depend on the cut (cut_free; with the constructor's settings the two cuts' records differ in their last bits, as (b)'s:
    measured, mean by 3.6e-7 of its magnitude, the pilot fields by 5.1e-8, peaks and mean_square equal)"""
    m = fmx_amd.fmx
    n = 400000
    x = ol.synth_iq(n, rds=1)[None]
    res = []
    for calls in ([n], [16384] * (n // 16384) + [n % 16384]):
        f = make(fmx_amd, 1, max_block=n, params=[(m.P_RDS_MODE, 2)] + cut_free(m))
        f.mod_meter(True, 0)
        run(f, m, x, calls)
        res.append(f.mod_records(0, 1)[0])
        f.close()
    report_difference("one call in RDS pieces against small calls", [res[0]], [res[1]])
    assert list(res[0]["index"]) == [0, 1, 2] and res[0].tobytes() == res[1].tobytes()


def test_calibration(case_a):
    """(l) the GPU's own records of a stereo signal (pilot 7 500 Hz) and of a mono 1 kHz tone at +-37 500 Hz"""
    _, _, recs = case_a
    st, tone = recs[0], recs[1]
    pilot_hz = np.hypot(st["pilot_i"].astype(np.float64), st["pilot_q"]) * HZ
    print("pilot %s Hz, |I| / |Q| %s" % (np.round(pilot_hz[6:], 1), np.abs(st["pilot_i"][6:] / st["pilot_q"][6:])))
    assert st.size >= 10 and np.all(np.abs(pilot_hz[6:] - 7500.0) <= 750.0)
    assert np.all(np.abs(st["pilot_i"][6:]) <= 0.01 * np.abs(st["pilot_q"][6:]))
    pos, neg = tone["peak_pos"][1:10].astype(np.float64) * HZ, -tone["peak_neg"][1:10].astype(np.float64) * HZ
    print("tone peaks %s / %s Hz" % (np.round(pos, 1), np.round(neg, 1)))
    assert np.all(np.abs(pos - 37500.0) <= TONE_PEAK_TOL_HZ) and np.all(np.abs(neg - 37500.0) <= TONE_PEAK_TOL_HZ)

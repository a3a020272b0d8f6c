"""The reception meter on the GPU (fmx_rx_meter_enable, fmx_rx_records, fmx_rx_quality_of; csrc/fmx_rx.hip): the records against the f32
restatement of tests/rx_model.py on the handle's own FMX_TAP_FM_IQ -- bit for bit, every field --, their independence of how the stream is cut into calls
and pieces, the switching rules, the ring and its read-out, every form of stage A, and the isolation of everything else a handle delivers: a batch with
every channel metered stays the plain batch it was."""
import os
import subprocess

import numpy as np
import pytest

import rx_model as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = rm.WINDOW
# the calls in input samples: the receiver's block, then cuts inside a step and inside a window -- 1, 63, 64, 65, 9599 and 19 237 fm samples --, then on
CALLS = [16384, 12, 12 * 63, 12 * 64, 12 * 65, 12 * 9599, 12 * 19237, 12 * 19237, 12 * 9000]
CARRIER = dict(stereo=0, leftAmp=0.0, rightAmp=0.0, offsetHz=10000.0)


def three_signals(ol, n):
    """clean stereo, the same in noise at 20 dB (tests/test_rx_cpu.py's), an unmodulated carrier at +10 kHz"""
    return np.stack([ol.synth_iq(n), ol.synth_iq(n, noiseSeed=rm.NOISE_SEED, noiseSigma=rm.noise_sigma(20)), ol.synth_iq(n, **CARRIER)])


def make(fmx_amd, channels, streams=0, max_block=16384, bandwidth=165000, params=(), som=None, **kw):
    m = fmx_amd.fmx
    if som is None and streams:
        som = [c % streams for c in range(channels)]
    f = fmx_amd.Fmx(channels, streams=streams, stream_of_channel=som, max_block=max_block, **kw)
    if bandwidth:
        f.set_param(m.P_BANDWIDTH, bandwidth)
    for item in params:
        f.set_param(*item)
    return f


def run(f, m, x, calls, tap_ch=(), each=None):
    """the calls of `calls` input samples behind each other; returns (pcm, {ch: FM_IQ read after every call, behind each other})"""
    taps = {c: [] for c in tap_ch}
    pcm, pos = [], 0
    for k, n in enumerate(calls):
        if each:
            each(f, k)
        pcm.append(f.process_host(x[:, pos:pos + n]))
        pos += n
        nj = f.last_fm_samples()
        for c in tap_ch:
            if nj > 0:
                taps[c].append(f.tap(m.TAP_FM_IQ, nj, c))
    return np.concatenate(pcm, axis=1), {c: np.concatenate(v) for c, v in taps.items()}


def same(a, b):
    return len(a) == len(b) and all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


@pytest.fixture(scope="module")
def x3(ol):
    return three_signals(ol, sum(CALLS))


@pytest.mark.parametrize("bandwidth", [165000, 0])
def test_records_against_the_restatement_on_the_handles_tap(fmx_amd, x3, bandwidth):
    """three channels (the block machines), the input filter at 165 kHz and "Off", calls that cut steps and windows: every field bit for bit"""
    m = fmx_amd.fmx
    f = make(fmx_amd, 3, max_block=max(CALLS), bandwidth=bandwidth)
    f.rx_meter(True)
    _, taps = run(f, m, x3, CALLS, tap_ch=(0, 1, 2))
    recs = f.rx_records(capacity=64)
    assert f.rx_records()[0].size == 0      # (read once: nothing is pending)
    f.close()
    nwin = (sum(CALLS) // 12) // W
    assert nwin >= 6
    for c in range(3):
        rm.check_records(recs[c], taps[c], expect_index=range(nwin))
    assert recs[0].tobytes() != recs[1].tobytes()


def cut_free(m):
    """the tap does not depend on the cut with the PLL decoder and RF DC removal off (tests/test_gpu_mod_meter.py cut_free)"""
    return [(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0)]


def test_one_call_against_many(fmx_amd, x3):
    """the same stream in nine calls and in one: the taps are equal (the premise), then the records are"""
    m = fmx_amd.fmx
    n = sum(CALLS) - sum(CALLS) % 12
    res = []
    for calls in (CALLS, [n]):
        f = make(fmx_amd, 3, max_block=n, params=cut_free(m))
        f.rx_meter(True)
        _, taps = run(f, m, x3, calls, tap_ch=(0, 1, 2))
        res.append((f.rx_records(), taps))
        f.close()
    (many, tm), (one, to) = res
    nwin = (n // 12) // W
    for c in range(3):
        assert tm[c][:n // 12].tobytes() == to[c].tobytes(), c
        rm.check_records(one[c], to[c], expect_index=range(nwin))
        assert one[c].tobytes() == many[c][:nwin].tobytes(), c


def expected_windows(J, on):
    """the windows that leave a record: complete, and the meter on in every call that covered one of their samples"""
    out = []
    for w in range(J[-1] // W):
        cover = [k for k in range(len(on)) if J[k] < (w + 1) * W and J[k + 1] > w * W]
        if all(on[k] for k in cover):
            out.append(w)
    return out


def test_switching_and_a_scanning_channel(fmx_amd, ol):
    """on in mid-window, off and on again, per channel and with -1, a channel never enabled until then; channel 0 scans for a while and its meter runs on"""
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
            f.rx_meter(True, 1)
        if k == 3:
            f.rx_meter(True, 0)
        if k == 10 or k == 20:
            f.rx_meter(False, 1)
        if k == 14:
            f.rx_meter(True, 1)
        if k == 5:
            assert f.rx_records(2, 1)[0].size == 0      # (a channel that was never enabled, on a handle whose meter runs)
        if k == 28:
            f.rx_meter(True, -1)
        f.set_param(m.P_SCANNING, 1 if 8 <= k < 18 else 0, 0)
    pcm, taps = run(f, m, x, [blk] * ncalls, tap_ch=(0, 1, 2), each=each)
    recs = f.rx_records()
    assert f.scan_results(0).size >= 8
    f.close()
    for c in range(3):
        want = expected_windows(J, on[c])
        assert len(want) >= 1
        rm.check_records(recs[c], taps[c], expect_index=want)
    assert recs[0]["index"][0] == 1 and recs[2]["index"][0] == -(-J[28] // W)
    assert list(recs[1]["index"]) == [0, 4]                              # (the gap in `index`: windows 1 .. 3 met a call with the meter off)


def test_ring_keeps_64_and_capacity_leaves_the_rest(fmx_amd, ol):
    """70 windows unread leave the last 64; a capacity below what is pending leaves the rest for the next read (a handle at inputRate 192 000)"""
    m = fmx_amd.fmx
    blk, ncalls = 5 * W + 40, 15
    x = ol.synth_iq(ncalls * blk, inputRate=192000)[None]
    f = fmx_amd.Fmx(1, max_block=blk, inputRate=192000)
    f.rx_meter(True, 0)
    _, taps = run(f, m, x, [blk] * 14, tap_ch=(0,))
    assert (14 * blk) // W == 70
    first = f.rx_records(0, 1, capacity=10)[0]
    assert list(first["index"]) == list(range(6, 16))
    run(f, m, x[:, 14 * blk:], [blk])
    rest = f.rx_records(0, 1, capacity=64)[0]
    assert list(rest["index"]) == list(range(16, 75))
    assert f.rx_records(0, 1)[0].size == 0
    f.close()
    rm.check_records(np.concatenate([first, rest[:54]]), taps[0])


@pytest.mark.parametrize("kernel", [1, 3])
def test_front_kernels(fmx_amd, x3, kernel):
    """a folded handle (FMX_P_FILTER_RESTARTS = 2) with stage A as fmx_front.hip and as fmx_front4.hip: each handle's records on its own tap"""
    m = fmx_amd.fmx
    calls = [98304, 12 * 65, 98304, 98304, 98304]
    f = make(fmx_amd, 3, max_block=98304, params=[(m.P_FILTER_RESTARTS, 2), (m.P_FRONT_KERNEL, kernel)])
    f.rx_meter(True)
    _, taps = run(f, m, x3, calls, tap_ch=(0, 1, 2))
    recs, used = f.rx_records(), f.last_front_kernel()
    f.close()
    assert used == kernel
    for c in range(3):
        rm.check_records(recs[c], taps[c], expect_index=range(3))


def test_local_oscillator(fmx_amd, ol):
    """three channels on one stream that differ in FMX_P_LOCAL_OSCILLATOR: the carrier at +10 kHz is seen at 10, -40 and +60 kHz"""
    m = fmx_amd.fmx
    calls = [98304, 12 * 63, 98304, 98304, 98304]
    x = ol.synth_iq(sum(calls), **CARRIER)[None]
    f = make(fmx_amd, 3, streams=1, max_block=98304, params=[(m.P_LOCAL_OSCILLATOR, 50000, 1), (m.P_LOCAL_OSCILLATOR, -50000, 2)])
    f.rx_meter(True)
    _, taps = run(f, m, x, calls, tap_ch=(0, 1, 2))
    recs = f.rx_records()
    f.close()
    nwin = (sum(calls) // 12) // W
    assert nwin == 3
    offs = []
    for c in range(3):
        rm.check_records(recs[c], taps[c], expect_index=range(nwin))
        offs.append(m.rx_quality(recs[c][1:])["offset_hz"])
    print("offsets seen: %s" % np.round(offs, 2))
    assert abs(offs[0] - 10000.0) <= rm.OFFSET_TOL_HZ and abs(abs(offs[1] - 10000.0) - 50000.0) < 1.0 and abs(abs(offs[2] - 10000.0) - 50000.0) < 1.0 and offs[1] * offs[2] < 0


def test_block_machines_with_a_bandwidth_change(fmx_amd, x3):
    """FMX_P_FILTER_RESTARTS = 1 with setBandwidth in mid-stream (the input filter's block restarts): the records on the tap as read"""
    m = fmx_amd.fmx
    calls = [16384] * 16

    def each(f, k):
        if k == 6:
            f.set_param(m.P_BANDWIDTH, 120000)
        if k == 11:
            f.set_param(m.P_BANDWIDTH, 0, 1)
    f = make(fmx_amd, 3, max_block=16384, params=[(m.P_FILTER_RESTARTS, 1)])
    f.rx_meter(True)
    _, taps = run(f, m, x3, calls, tap_ch=(0, 1, 2), each=each)
    recs = f.rx_records()
    f.close()
    for c in range(3):
        rm.check_records(recs[c], taps[c], expect_index=range((sum(calls) // 12) // W))


def batch_records(fmx_amd, x, calls, params, tap_ch=()):
    m = fmx_amd.fmx
    f = make(fmx_amd, 130, streams=3, max_block=max(calls), params=params)
    f.rx_meter(True)
    _, taps = run(f, m, x, calls, tap_ch=tap_ch)
    recs, pieces = f.rx_records(), f.last_call_pieces()
    f.close()
    return recs, taps, pieces


def test_batch_overlapping_pieces(fmx_amd, ol):
    """the PLL decoder's batch of 130 channels, calls made in overlapping pieces of 1536 fm samples, against the same calls made whole: the meter's kernel
    runs on stage A's stream between one piece's stage A and the next one's"""
    m = fmx_amd.fmx
    calls = [98304] * 3
    x = three_signals(ol, sum(calls))
    whole, tw, p0 = batch_records(fmx_amd, x, calls, [(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0), (m.P_CALL_PIECES, 0)], tap_ch=(0, 129))
    cut, _, p1 = batch_records(fmx_amd, x, calls, [(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0), (m.P_CALL_PIECES, 1536)])
    assert p0 == 1 and p1 >= 4
    assert all(r.size == 2 for r in whole) and same(whole, cut)
    for c in (0, 129):                      # (the tap covers a whole call only where the call is one piece)
        rm.check_records(cut[c], tw[c], expect_index=[0, 1])
    assert cut[0].tobytes() == cut[3].tobytes() and cut[0].tobytes() != cut[1].tobytes()


def test_other_outputs_unchanged_three_channels(fmx_amd, ol):
    """PCM, meta, peaks, scan records, the two other meters' records and the RDS bits of three channels -- one decodes RDS, one scans for a while -- are
    bit-identical with the reception meter on and off"""
    m = fmx_amd.fmx
    ncalls, blk = 40, 16384
    x = three_signals(ol, ncalls * blk)
    x[0] = ol.synth_iq(ncalls * blk, rds=1)
    out = []
    for meter in (False, True):
        f = make(fmx_amd, 3, max_block=blk, params=[(m.P_RDS_MODE, 2, 0)])
        f.mod_meter(True)
        f.audio_meter(True)
        if meter:
            f.rx_meter(True)
        pcm, _ = run(f, m, x, [blk] * ncalls, each=lambda f, k: f.set_param(m.P_SCANNING, 1 if 4 <= k < 12 else 0, 1))
        meta = [bytes(f.meta(c)) for c in range(3)]
        out.append((pcm, meta, [f.peaks(c) for c in range(3)], f.scan_results(1), [f.rds_bits(c) for c in range(3)], f.mod_records(), f.audio_records(),
                    f.rx_records(), (f.last_second_group(), f.last_call_pieces(), f.last_front_kernel())))
        f.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2])) and a[2][0].shape[0] > 0
    assert a[3].tobytes() == b[3].tobytes() and a[3].size >= 8
    assert all(np.array_equal(p, q) for p, q in zip(a[4], b[4])) and a[4][0].size > 0
    assert same(a[5], b[5]) and a[5][0].size > 0 and same(a[6], b[6]) and a[6][0].size > 0
    assert a[8] == b[8]
    nwin = (ncalls * blk // 12) // W
    assert all(r.size == 0 for r in a[7]) and all(list(r["index"]) == list(range(nwin)) for r in b[7])


@pytest.mark.parametrize("nch", [800, 1100])
def test_other_outputs_unchanged_batch_with_every_channel_metered(fmx_amd, ol, nch):
    """800 and 1100 channels on four shared streams, the reception meter on for ALL of them: the PCM is bit-identical and the handle runs the channel
    groups the unmetered handle runs -- at 1100 channels 768 + 332 in both (the modulation meter makes one group of them, tests/test_gpu_mod_meter.py)"""
    m = fmx_amd.fmx
    blk, ncalls = 49152, 3
    x = np.stack([ol.synth_iq(ncalls * blk, leftHz=500.0 + 300 * s, rightHz=900.0 + 200 * s) for s in range(4)])
    res = []
    for meter in (False, True):
        f = make(fmx_amd, nch, streams=4, max_block=blk)
        if meter:
            f.rx_meter(True)
        pcm, _ = run(f, m, x, [blk] * ncalls)
        res.append((pcm, f.last_second_group(), f.last_front_kernel(), f.last_call_pieces(), f.rx_records()))
        f.close()
    print("%d channels: second group %d without the meter, %d with it" % (nch, res[0][1], res[1][1]))
    assert res[0][1] == (332 if nch == 1100 else 0) and res[1][1:4] == res[0][1:4]
    assert np.array_equal(res[0][0], res[1][0])
    assert all(r.size == 0 for r in res[0][4]) and all(list(r["index"]) == [0] for r in res[1][4])
    assert res[1][4][0].tobytes() == res[1][4][4].tobytes() and res[1][4][0].tobytes() != res[1][4][1].tobytes()      # (channels 0 and 4 share a stream)


def test_physical_figures(fmx_amd, ol):
    """the offset carrier's offset_hz and the noisy channel's cnr_db on the GPU within the CPU test's bounds (rx_model.py): signal + noise, signal and noise
    as three channels, the truth from their own records as tests/test_rx_cpu.py takes it from the oracle's taps; a fourth channel carries the carrier"""
    m = fmx_amd.fmx
    n = 12 * 11 * W
    s = rm.noise_sigma(20)
    x = np.stack([ol.synth_iq(n, noiseSeed=rm.NOISE_SEED, noiseSigma=s), ol.synth_iq(n), ol.synth_iq(n, noiseSeed=rm.NOISE_SEED, noiseSigma=s, carrierAmp=0.0),
                  ol.synth_iq(n, **CARRIER)])
    f = make(fmx_amd, 4, max_block=n // 11)
    f.rx_meter(True)
    run(f, m, x, [n // 11] * 11)
    recs = [r[1:] for r in f.rx_records()]
    f.close()
    assert all(r.size == 10 for r in recs)
    mean_p = lambda r: float(r["p_mean"].astype(np.float64).mean())
    truth = 10.0 * np.log10(mean_p(recs[1]) / mean_p(recs[2]))
    q = [m.rx_quality(r) for r in recs]
    print("truth %.3f dB, cnr_db %.3f; noise alone %s; carrier offset_hz %+.4e from 10 kHz" % (truth, q[0]["cnr_db"], q[2]["cnr_db"], q[3]["offset_hz"] - 10000.0))
    assert abs(mean_p(recs[0]) / (mean_p(recs[1]) + mean_p(recs[2])) - 1.0) <= 0.01
    assert abs(q[0]["cnr_db"] - truth) <= rm.CNR_TOL_DB[20]
    assert abs(q[3]["offset_hz"] - 10000.0) <= rm.OFFSET_TOL_HZ


def build_demo(fmx_amd, exe):
    host = os.path.join(ROOT, "sdr-j-fm_amd", "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + host, os.path.join(ROOT, "tests", "rx_demo", "rx_adapter_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])


def test_mirrors(fmx_amd, ol, tmp_path):
    """fmx.py's FmProcessor mirror (setReceptionMeter / pollReception) returns the records the handle's rx_records returns, and rx_quality of them is
    quality () of the model; the C++ adapter (host/fm_processor_adapter.h: setReceptionMeter, pollReception, receptionQuality) returns the same records
    and the same figures"""
    m = fmx_amd.fmx
    blocks = 36
    n = 16384 * blocks
    x = ol.synth_iq(n)
    res = []
    for mirror in (False, True):
        f = fmx_amd.Fmx(1, max_block=16384)
        f.set_param(m.P_BANDWIDTH, 165000)
        if mirror:
            class Rig:
                pos = 0

                def Samples(self):
                    return n - self.pos

                def getSamples(self, k):
                    self.pos += k
                    return x[self.pos - k:self.pos]
            p = fmx_amd.FmProcessor(theDevice=Rig(), mySink=None, inputRate=2304000, fmx=f, channel=0, blockSize=16384)
            p.setReceptionMeter(True)
            while p.run_block():
                pass
            res.append(p.pollReception())
        else:
            f.rx_meter(True, 0)
            for k in range(blocks):
                f.process_host(x[k * 16384:(k + 1) * 16384])
            res.append(f.rx_records(0, 1)[0])
        f.close()
    assert res[0].size == 5 and res[0].tobytes() == res[1].tobytes()
    got, want = m.rx_quality(res[0]), rm.quality(res[0])
    assert all(abs(got[k] - want[k]) <= 1e-12 * abs(want[k]) for k in ("level_dbfs", "cnr_db", "am_depth", "offset_hz"))
    # the C++ adapter on the same samples (tests/rx_demo)
    exe, fin, fout = str(tmp_path / "rx_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "records.bin")
    build_demo(fmx_amd, exe)
    x.tofile(fin)
    out = subprocess.check_output([exe, fin, fout], timeout=120).decode().split()
    assert int(out[1]) == 5 and np.fromfile(fout, rm.RX_DTYPE).tobytes() == res[0].tobytes(), out
    for k, name in ((3, "level_dbfs"), (5, "cnr_db"), (7, "am_depth"), (9, "offset_hz")):
        assert float(out[k]) == got[name], (name, out)

"""Scan mode on the GPU (FMX_P_SCANNING, fmx_scan_results; csrc/fmx_scan.hip): the records against the reference's scan restated on the
oracle's fm-rate samples (FMX_TAP_FM_IQ of OracleChain, fmo_fft_radix2 = the reference's Fft_transform bit for bit, getSignal / getNoise /
get_db in f32, fm-processor.cpp:478-495, 886-904), their independence of how a call is cut, and the isolation of the chain: a scanning
channel's PCM is zeros in its scanning calls and bit-identical to a never-scanning twin elsewhere; its neighbours do not notice."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
SIG = [5 + i for i in range(20)] + [N - 1 - (5 + i) for i in range(20)]
NOI = [N // 2 - 1 - (5 + i) for i in range(20)] + [N // 2 + 1 + (5 + i) for i in range(20)]
BLOCK = 16384                 # 1365.33 fm samples per call: never a multiple of 1024
P_SCANNING = 28


def ref_records(ol, fm_iq, spans, thr=20):
    """What the reference's scan computes: the fm samples of the scanned spans [(J0, J1), ...] behind each other, blocks of 1024 through the
    reference's FFT, its float sums and get_db.  Returns [(end_sample, signal_db, noise_db, found)]."""
    O = ol.oracle()
    idx = np.concatenate([np.arange(a, b) for a, b in spans]) if spans else np.zeros(0, np.int64)
    out = []
    for b in range(len(idx) // N):
        sel = idx[b * N:(b + 1) * N]
        v = np.ascontiguousarray(fm_iq[sel], np.float32).copy()
        assert O.fmo_fft_radix2(ol.fptr(v), N, 0) == 1
        X = v.view(np.complex64).reshape(-1)
        db = []
        for bins in (SIG, NOI):
            s = np.float32(0)
            for k in bins:
                s = np.float32(s + np.float32(abs(X[k])))
            m = np.float32(s / np.float32(40))
            db.append(np.float32(np.float32(20) * np.log10(np.float32((m + np.float32(1)) / np.float32(256)))))
        out.append((int(sel[-1]) + 1, db[0], db[1], bool(np.float32(db[0] - db[1]) > np.float32(thr))))
    return out


def check_parity(recs, ref, first_block=0):
    assert len(recs) == len(ref), (len(recs), len(ref))
    for i, (r, e) in enumerate(zip(recs, ref)):
        assert r["block"] == first_block + i
        assert r["end_sample"] == e[0], (i, r["end_sample"], e[0])
        assert abs(r["signal_db"] - e[1]) <= 1e-3 and abs(r["noise_db"] - e[2]) <= 1e-3, (i, r, e)
        margin = float(e[1]) - float(e[2])
        if abs(margin - 20.0) > 0.01:
            assert bool(r["found"]) == e[3], (i, r, e)


def oracle_fm(ol, iq, **cfg):
    ch = ol.OracleChain(taps=[ol.TAP_FM_IQ], tap_seconds=(len(iq) / 2304000.0) + 1.0, **cfg)
    ch.process(np.concatenate([iq, np.zeros((16384, 2), np.float32)]))     # (the oracle works in 16384-sample blocks: flush the last one)
    return ch.tap(ol.TAP_FM_IQ)


def spans_of(calls, scanning, block=BLOCK):
    """fm-sample spans [(J0, J1)] of the calls in `scanning` (12-fold decimation)"""
    return [((k * block) // 12, ((k + 1) * block) // 12) for k in range(calls) if k in scanning]


def run(f, x, calls, block=BLOCK, scan_ch=(0,), scanning=None, each=None):
    """calls of `block` samples of x ([streams, n, 2] or [n, 2]); scan_ch scan in the calls of `scanning` (all when None)"""
    pcm = []
    for k in range(calls):
        on = scanning is None or k in scanning
        for c in scan_ch:
            f.set_param(P_SCANNING, 1 if on else 0, c)
        if each:
            each(f, k)
        seg = x[..., k * block:(k + 1) * block, :]
        pcm.append(f.process_host(seg))
    return np.concatenate(pcm, axis=1)


def test_parity_receiver(fmx_amd, ol):
    """one channel: the block machines (FMX_P_FILTER_RESTARTS automatic)"""
    m = fmx_amd.fmx
    calls = 12
    iq = ol.synth_iq(calls * BLOCK)
    f = fmx_amd.Fmx(1, max_block=BLOCK, device=0)
    f.set_param(m.P_BANDWIDTH, 165000)
    run(f, iq, calls)
    recs = f.scan_results(0)
    ref = ref_records(ol, oracle_fm(ol, iq, inputFilterBw=165000), spans_of(calls, range(calls)))
    assert len(ref) == (calls * BLOCK // 12) // N
    check_parity(recs, ref)
    assert len(f.scan_results(0)) == 0                       # read once


def test_parity_batch_matrix_pipe(fmx_amd, ol):
    """a batch of 256 channels on two streams, stage A on the matrix pipe (fmx_front4.hip: whole 1536-sample tiles of calls that start on
    a multiple of 12 samples, so calls of 12 tiles here: 1536 fm samples, still not a multiple of 1024)"""
    m = fmx_amd.fmx
    calls, nch, block = 12, 256, 12 * 1536
    x = np.stack([ol.synth_iq(calls * block), ol.synth_iq(calls * block, leftHz=700.0, rightHz=1300.0, offsetHz=20000.0)])
    f = fmx_amd.Fmx(nch, streams=2, stream_of_channel=[c % 2 for c in range(nch)], max_block=block, device=0)
    f.set_param(m.P_BANDWIDTH, 165000)
    f.set_param(m.P_FRONT_KERNEL, 3)
    run(f, x, calls, block=block, scan_ch=(0, 1, nch - 1))
    assert f.last_front_kernel() == 3
    spans = spans_of(calls, range(calls), block=block)
    for c in (0, 1, nch - 1):
        ref = ref_records(ol, oracle_fm(ol, x[c % 2], inputFilterBw=165000), spans)
        check_parity(f.scan_results(c), ref)
    assert len(f.scan_results(2)) == 0


def test_parity_shared_stream_with_local_oscillators(fmx_amd, ol):
    """a batch of 96 channels on one wide-band stream, each at its own local oscillator"""
    calls, nch = 12, 96
    x = ol.synth_iq(calls * BLOCK, offsetHz=300000.0)
    los = [(c % 23 - 11) * 100000 for c in range(nch)]
    f = fmx_amd.Fmx(nch, streams=1, stream_of_channel=[0] * nch, max_block=BLOCK, device=0)
    f.set_param(fmx_amd.fmx.P_BANDWIDTH, 165000)              # (the oracle's default, radio.cpp:2099)
    for c, lo in enumerate(los):
        f.set_param(fmx_amd.fmx.P_LOCAL_OSCILLATOR, lo, c)
    picks = (14, 15, 30)                                      # lo 300 kHz (on the station), 400 kHz, -300 kHz
    run(f, x, calls, scan_ch=picks)
    spans = spans_of(calls, range(calls))
    for c in picks:
        check_parity(f.scan_results(c), ref_records(ol, oracle_fm(ol, x, loFrequency=los[c]), spans))


def test_pause_and_resume(fmx_amd, ol):
    """the carry is kept over a pause: a block made of samples from both sides of it"""
    calls = 12
    iq = ol.synth_iq(calls * BLOCK)
    scanning = {0, 1, 5, 6, 7, 8, 9, 10}
    f = fmx_amd.Fmx(1, max_block=BLOCK, device=0)
    f.set_param(fmx_amd.fmx.P_BANDWIDTH, 165000)
    run(f, iq, calls, scanning=scanning)
    spans = spans_of(calls, scanning)
    ref = ref_records(ol, oracle_fm(ol, iq), spans)
    recs = f.scan_results(0)
    check_parity(recs, ref)
    # calls 0 and 1 leave a carry: the third block holds samples of call 1 and of call 5
    before = spans[1][1] - spans[0][0]
    assert before % N != 0 and recs[before // N]["end_sample"] > spans[2][0]


def test_piece_invariance(fmx_amd, ol):
    """calls made in RDS pieces (an RDS neighbour) and in overlapping pre-pass pieces (a PLL-decoder neighbour, FMX_P_CALL_PIECES) give the
    records of whole calls; a mid-stream FMX_P_BANDWIDTH change while scanning included"""
    m = fmx_amd.fmx
    big = 400000                                             # 33333 fm samples: two RDS pieces
    calls = 4
    x = ol.synth_iq(calls * big, rds=1)

    def records(nch, setup, each=None):
        f = fmx_amd.Fmx(nch, streams=1, stream_of_channel=[0] * nch, max_block=big, device=0)
        f.set_param(m.P_BANDWIDTH, 165000)
        setup(f)
        run(f, x, calls, block=big, each=each)
        return f.scan_results(0), f.last_call_pieces(), f.last_fm_samples()

    def same(a, b):
        # (the fm-rate samples themselves agree to rounding, not bit for bit, between calls cut differently: stage A's RF DC recurrence is
        # evaluated per tile as a composition of affine maps whose grouping follows the call boundaries)
        assert len(a) == len(b) == (calls * big // 12) // N
        assert np.array_equal(a["block"], b["block"]) and np.array_equal(a["end_sample"], b["end_sample"])
        assert np.abs(a["signal_db"] - b["signal_db"]).max() <= 1e-4 and np.abs(a["noise_db"] - b["noise_db"]).max() <= 1e-4
        margin = a["signal_db"] - a["noise_db"]
        clear = np.abs(margin - 20.0) > 0.01
        assert np.array_equal(a["found"][clear], b["found"][clear])

    whole, _, n_whole = records(2, lambda f: None)
    rds, _, n_rds = records(2, lambda f: f.set_param(m.P_RDS_MODE, 1, 1))
    assert n_whole == big // 12 and n_rds < big // 12            # (the RDS handle's calls were made in two pieces; the last is reported)
    same(whole, rds)

    def bw(f, k):
        if k == 2:
            f.set_param(m.P_BANDWIDTH, 120000)

    def pll(f):
        f.set_param(m.P_FM_DECODER, 2, 1)
        f.set_param(m.P_CALL_PIECES, 4608)
    whole_b, p0, _ = records(96, lambda f: f.set_param(m.P_CALL_PIECES, 0), each=bw)
    piped_b, p1, _ = records(96, pll, each=bw)
    assert p0 == 1 and p1 > 1
    same(whole_b, piped_b)


def test_isolation(fmx_amd, ol):
    """zeros while scanning, the never-scanning twin's PCM elsewhere; the neighbours (taps, RDS bits) equal a handle where nothing scans"""
    m = fmx_amd.fmx
    calls = 12
    iq = ol.synth_iq(calls * BLOCK, rds=1)
    scanning = {2, 3, 4, 5, 9}

    def handle():
        f = fmx_amd.Fmx(3, streams=1, stream_of_channel=[0, 0, 0], max_block=BLOCK, device=0)
        f.set_param(m.P_BANDWIDTH, 165000)
        f.set_param(m.P_RDS_MODE, 2, 2)
        return f
    a, b = handle(), handle()
    taps_a, taps_b, bits_a, bits_b, pcm_a, pcm_b = [], [], [], [], [], []
    for k in range(calls):
        a.set_param(m.P_SCANNING, 1 if k in scanning else 0, 0)
        seg = iq[k * BLOCK:(k + 1) * BLOCK]
        pa, pb = a.process_host(seg), b.process_host(seg)
        pcm_a.append(pa); pcm_b.append(pb)
        nfm = a.last_fm_samples()
        for c in (1, 2):
            taps_a.append(np.concatenate([a.tap(t, nfm, c).reshape(-1) for t in (m.TAP_FM_IQ, m.TAP_DEMOD, m.TAP_PRE_RESAMPLER)]))
            taps_b.append(np.concatenate([b.tap(t, nfm, c).reshape(-1) for t in (m.TAP_FM_IQ, m.TAP_DEMOD, m.TAP_PRE_RESAMPLER)]))
        bits_a.append(a.rds_bits(2)); bits_b.append(b.rds_bits(2))
        if k in scanning:
            assert pa.shape[1] > 0 and not np.any(pa[0]), k
        else:
            assert np.array_equal(pa[0], pa[1]), k                  # the twin on the same stream
        assert np.array_equal(pa[1:], pb[1:]), k
    for u, v in zip(taps_a, taps_b):
        assert np.array_equal(u, v)
    assert np.array_equal(np.concatenate(bits_a), np.concatenate(bits_b)) and sum(len(v) for v in bits_a) > 0
    assert len(a.scan_results(0)) == (len(scanning) * BLOCK // 12) // N
    assert len(a.scan_results(1)) == 0 and len(b.scan_results(0)) == 0


def test_threshold_validation_and_gap(fmx_amd, ol):
    m = fmx_amd.fmx
    f = fmx_amd.Fmx(1, max_block=1 << 20, device=0)
    for pid, bad in ((m.P_SCAN_THRESHOLD, 32768), (m.P_SCAN_THRESHOLD, -32769), (m.P_SCAN_THRESHOLD, 2.5), (m.P_SCAN_THRESHOLD, float("nan")),
                     (m.P_SCANNING, 2), (m.P_SCANNING, 0.5), (m.P_SCANNING, float("nan"))):
        with pytest.raises(fmx_amd.FmxError) as e:
            f.set_param(pid, bad, 0)
        assert e.value.code == m.FMX_E_INVALID, (pid, bad)
    f.set_param(m.P_SCAN_THRESHOLD, -32768, 0)
    f.set_param(m.P_SCAN_THRESHOLD, 32767, 0)
    # the threshold of the call that completed a block decides `found`
    iq = ol.synth_iq(3 * BLOCK)
    f.set_param(m.P_SCANNING, 1, 0)
    recs = []
    for k, thr in enumerate((-32768, 32767, 5)):
        f.set_param(m.P_SCAN_THRESHOLD, thr, 0)
        f.process_host(iq[k * BLOCK:(k + 1) * BLOCK])
        r = f.scan_results(0)
        margin = r["signal_db"] - r["noise_db"]
        assert np.array_equal(r["found"].astype(bool), margin > np.float32(thr)), (thr, r)
        recs.append(r)
    assert recs[0]["found"].all() and not recs[1]["found"].any()
    # 1024 unread records and more: the oldest are gone, `block` shows the gap
    rng = np.random.default_rng(1)
    big = 1000000
    for _ in range(14):
        f.process_host((rng.standard_normal((big, 2)) * 0.1).astype(np.float32))
    done = (3 * BLOCK + 14 * big) // 12 // N
    r = f.scan_results(0, capacity=2048)
    assert len(r) == 1024 and r["block"][0] == done - 1024 and r["block"][-1] == done - 1
    assert np.all(np.diff(r["block"]) == 1) and np.all(np.diff(r["end_sample"]) == N)


def test_band_scan(fmx_amd, ol):
    """one 2.304 MS/s stream with three stations and noise, 23 channels from -1.1 to +1.1 MHz: each station's channel hits in at least 90 % of
    its blocks, no channel 200 kHz or more from every station ever does"""
    n = 12 * BLOCK
    stations = (-700000, 200000, 900000)
    x = ol.synth_iq(n, offsetHz=float(stations[0]), noiseSigma=0.01, noiseSeed=7).astype(np.float64)
    for s, (l, r) in zip(stations[1:], ((700.0, 1300.0), (400.0, 2000.0))):
        x += ol.synth_iq(n, offsetHz=float(s), leftHz=l, rightHz=r)
    x = x.astype(np.float32)
    los = [k * 100000 for k in range(-11, 12)]
    f = fmx_amd.Fmx(len(los), streams=1, stream_of_channel=[0] * len(los), max_block=BLOCK, device=0)
    for c, lo in enumerate(los):
        f.set_param(fmx_amd.fmx.P_LOCAL_OSCILLATOR, lo, c)
    f.set_param(fmx_amd.fmx.P_SCANNING, 1)
    for k in range(12):
        f.process_host(x[k * BLOCK:(k + 1) * BLOCK])
    for c, lo in enumerate(los):
        r = f.scan_results(c)
        assert len(r) == n // 12 // N
        r = r[2:]                                             # (the first blocks hold the filters' start)
        d = min(abs(lo - s) for s in stations)
        if d == 0:
            assert r["found"].mean() >= 0.9, (lo, r["signal_db"] - r["noise_db"])
        elif d >= 200000:
            assert not r["found"].any(), (lo, r["signal_db"] - r["noise_db"])


def test_cpp_adapter_scan(fmx_amd, ol, tmp_path):
    """the C++ adapter while scanning: the sink gets no frames, the scan callback sees the station's records with `found` (scanresult ())"""
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    host = os.path.join(os.path.dirname(fmx_amd.__file__), "host")
    exe = str(tmp_path / "scan_adapter_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + host, os.path.join(here, "scan_demo", "scan_adapter_demo.cpp"),
                           "-L" + os.path.dirname(fmx_amd.LIB_PATH), "-lfmx", "-Wl,-rpath," + os.path.dirname(fmx_amd.LIB_PATH), "-o", exe])
    iq = ol.synth_iq(24 * BLOCK)
    iq.tofile(str(tmp_path / "iq.f32"))
    out = subprocess.check_output([exe, str(tmp_path / "iq.f32")]).decode().split()
    f0, f1, f2, records, found = int(out[1]), int(out[2]), int(out[3]), int(out[5]), int(out[7])
    assert f0 > 0 and f1 == 0 and f2 > 0, out
    assert records == (8 * BLOCK // 12) // N, out
    assert found >= 0.9 * records, out

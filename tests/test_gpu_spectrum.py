"""The spectrum meter on the GPU (fmx_spectrum_setup / _enable / _read / _figures; csrc/fmx_spec.hip) against the float64 model of
tests/spec_model.py.

The bound of every spectrum comparison (survey_model.check_spectrum): a bin's error is |P - P64| / P64; per case, level_worst is the larger
of the worst bins of the two f32 restatements of the same records -- the plain one (radix-2, complex64) and kernel_form (the header's own stage functions
and fold on the host, tests/spec_check.cpp) --, level_median the larger of their medians; the GPU must stay within 2 x level_worst on every bin and
within 2 x level_median in the median -- mean and peak each.  Shapes: 3 streams of 10 blocks of 4096 and 100 samples."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import spec_model as pm
import survey_model as sm
import wideband_model as wm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = pm.N
FMT_NAMES = {0: "F32", 1: "U8", 2: "S8", 3: "S16/2048"}
GAP = 37                              # stream_stride - n of the device input
GAP_CODE = {0: np.nan, 1: 255, 2: -128, 3: -32768}
CUTS = sm.call_cuts(1)                # a carry that grows over three calls, a block completed from it with a tail left, several blocks, a call that
                                      # ends on a block end, a call of one sample, the rest


@pytest.fixture(scope="module")
def kernel_form(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("spec")
    exe = str(d / "spec_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "spec_check.cpp")])

    def run(x, B, S):
        """-> {index: (mean, peak)} of every record of the stream (one call per record's worth: nothing is lost to the ring)"""
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.asarray(x, np.complex64).tofile(fi)
        step = N * S * B
        cuts = [step] * (len(x) // step) + ([len(x) % step] if len(x) % step else [])
        subprocess.check_call([exe, "spectrum", fi, fo, str(B), str(S), "0", "64"] + [str(c) for c in cuts])
        raw = np.fromfile(fo, np.float32).reshape(-1, 1 + 2 * N)
        return {int(row[0]): (row[1:1 + N], row[1 + N:]) for row in raw}
    return run


_RAW = {}


def raw_streams(fmt, n=None, streams=3):
    """[streams, n, 2] in the raw format: different streams of survey_model.spectrum_signal (power in every bin: tests/test_spec_cpu.py checks it)."""
    n = sm.stream_length(1) if n is None else n
    if (fmt, n, streams) not in _RAW:
        _RAW[fmt, n, streams] = np.stack([sm.to_raw(sm.spectrum_signal(2, n, seed=s), fmt) for s in range(streams)])
    return _RAW[fmt, n, streams]


def expected_indices(cuts, B, S, first=0, g=0, read_every_call=True):
    """the records a reader gets that reads behind every call (or behind the last only): of the records a call completes the ring keeps the last four"""
    out, ring = [], {}
    for n in cuts:
        r_lo, r_hi = pm.n_blocks(g, S) // B, pm.n_blocks(g + n, S) // B
        for r in range(r_lo, r_hi):
            if r * B >= first:
                ring[r % pm.RING] = r
        g += n
        if read_every_call:
            out += sorted(r for r in ring.values() if r not in out and (not out or r > out[-1]))
    if not read_every_call:
        out = sorted(ring.values())
    return out


class Run:
    """One handle fed `raw` ([streams, n, 2]) in calls of the given lengths, the metered streams' records read behind every call (or behind the last):
    idx [s], mean [s], peak [s], recs [s] and what a last read returns (after [s]).  via: fmx_process_device_raw (input with a stride, the gap filled
    with NaN or extreme codes) or fmx_process_host_raw."""

    def __init__(self, fmx_amd, raw, fmt, cuts, B=2, S=1, metered=(0, 2), via="device", channels=None, som=None, params=(), each=None, read_every_call=True,
                 capacity=4, keep_pcm=False, **kw):
        m = fmx_amd.fmx
        streams, n = raw.shape[0], raw.shape[1]
        channels = streams if channels is None else channels
        assert sum(cuts) == n
        self.recs, self.mean, self.peak = ([[] for _ in range(streams)] for _ in range(3))
        self.pieces, pcm = [], []
        f = fmx_amd.Fmx(channels, streams=streams if (som is not None or channels != streams) else 0, stream_of_channel=som, max_block=max(cuts), **kw)
        try:
            for item in params:
                f.set_param(*item)
            f.spectrum_setup(B, S)
            for s in metered:
                f.spectrum_meter(True, s)
            if via == "device":
                import torch
                padded = np.full((streams, n + GAP, 2), GAP_CODE[fmt], raw.dtype)
                padded[:, :n] = raw
                d_iq = torch.from_numpy(padded).cuda()
                cap = max(f.frames_for(max(cuts)) + 64, 64)
                d_pcm = torch.zeros((channels, cap, 2), dtype=torch.float32, device="cuda")
                bps = raw.dtype.itemsize * 2
            pos = 0
            for k, ln in enumerate(cuts):
                if each:
                    each(f, k)
                if via == "device":
                    got = C.c_int64()
                    f._check(f.L.fmx_process_device_raw(f.h, C.c_void_p(d_iq.data_ptr() + bps * pos), fmt, 2048.0, n + GAP, ln, C.c_void_p(d_pcm.data_ptr()),
                                                        cap, C.byref(got), None))
                    if keep_pcm:
                        pcm.append(d_pcm[:, :got.value].cpu().numpy().copy())
                else:
                    p = f.process_host_raw(raw[:, pos:pos + ln], fmt, 2048.0)
                    if keep_pcm:
                        pcm.append(p)
                pos += ln
                self.pieces.append(f.last_call_pieces())
                if read_every_call or k == len(cuts) - 1:
                    for s in range(streams):
                        r, mean, peak = f.spectrum_read(s, capacity)
                        self.recs[s] += list(r)
                        self.mean[s] += list(mean)
                        self.peak[s] += list(peak)
            if via == "device":
                torch.cuda.synchronize()
            self.after = [f.spectrum_read(s)[0] for s in range(streams)]
            self.pcm = np.concatenate(pcm, axis=1) if keep_pcm else None
            self.f_facts = (f.last_second_group(), f.last_call_pieces(), f.last_front_kernel())
        finally:
            f.close()
        self.idx = [[int(r["index"]) for r in rs] for rs in self.recs]
        self.mean = [np.array(v, np.float32).reshape(-1, N) for v in self.mean]
        self.peak = [np.array(v, np.float32).reshape(-1, N) for v in self.peak]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def common(a, b, s):
    """the records of stream s both runs delivered -> (indices, a's mean, peak, b's mean, peak)"""
    idx = [r for r in a.idx[s] if r in b.idx[s]]
    ia, ib = [a.idx[s].index(r) for r in idx], [b.idx[s].index(r) for r in idx]
    return idx, a.mean[s][ia], a.peak[s][ia], b.mean[s][ib], b.peak[s][ib]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("B,S", [(1, 1), (2, 1), (2, 3)])
def test_records_against_the_float64_model(fmx_amd, kernel_form, B, S, fmt):
    """A 3-stream handle, streams 0 and 2 metered, stream 1 not; device input with stream_stride > n, the gap filled with NaN / extreme codes; the cuts
    of survey_model.call_cuts."""
    raw = raw_streams(fmt)
    run = Run(fmx_amd, raw, fmt, CUTS, B, S)
    want = expected_indices(CUTS, B, S)
    assert len(want) >= 2 and run.idx[1] == [] and len(run.after[1]) == 0
    M64, K64, M32, K32, MKF, KKF, GM, GK = ([] for _ in range(8))
    for s in (0, 2):
        x = wm.convert(raw[s], fmt)
        idx, m64, k64 = pm.records64(x, B, S)
        _, m32, k32 = pm.records32(x, B, S)
        kf = kernel_form(x, B, S)
        assert run.idx[s] == want and set(want) <= set(idx) and sorted(kf) == idx
        recs = run.recs[s]
        assert [int(r["end_sample"]) for r in recs] == [N * S * ((r + 1) * B - 1) + N for r in want]
        assert all(int(r["blocks"]) == B and int(r["every"]) == S for r in recs) and len(run.after[s]) == 0
        M64.append(m64[want]); K64.append(k64[want]); M32.append(m32[want]); K32.append(k32[want])
        MKF.append(np.stack([kf[r][0] for r in want])); KKF.append(np.stack([kf[r][1] for r in want]))
        GM.append(run.mean[s]); GK.append(run.peak[s])
    M64, K64, M32, K32, MKF, KKF, GM, GK = (np.concatenate(v) for v in (M64, K64, M32, K32, MKF, KKF, GM, GK))
    assert GM.shape == (2 * len(want), N) and np.all(np.isfinite(GM)) and np.all(np.isfinite(GK))
    print()
    ok, rw, rm = sm.check_spectrum("GPU mean, B = %d, S = %d, %s" % (B, S, FMT_NAMES[fmt]), GM, M64, *sm.levels(M64, M32, MKF))
    assert ok, (rw, rm)
    ok, rw, rm = sm.check_spectrum("GPU peak, B = %d, S = %d, %s" % (B, S, FMT_NAMES[fmt]), GK, K64, *sm.levels(K64, K32, KKF))
    assert ok, (rw, rm)
    if B == 1:
        assert same_bits(GM, GK)                                # (one block a record: c = c1, the sum of one is the maximum of one)


@pytest.mark.parametrize("B,S", [(2, 1), (2, 3)])
def test_cuts_are_bit_identical(fmx_amd, B, S):
    """One call against the cuts, and fmx_process_host_raw against fmx_process_device_raw: the same records, byte for byte."""
    raw = raw_streams(0)
    n = raw.shape[1]
    whole = Run(fmx_amd, raw, 0, [n], B, S)
    cut = Run(fmx_amd, raw, 0, CUTS, B, S)
    host = Run(fmx_amd, raw, 0, CUTS, B, S, via="host")
    single = Run(fmx_amd, raw[:, :N + 3], 0, [N - 1, 1, 1, 1, 1], 1, 1)          # calls of one sample across a block end
    block = Run(fmx_amd, raw[:, :N], 0, [N], 1, 1)
    for s in (0, 2):
        assert cut.idx[s] == host.idx[s] == expected_indices(CUTS, B, S) and whole.idx[s] == expected_indices([n], B, S)
        assert same_bits(cut.mean[s], host.mean[s]) and same_bits(cut.peak[s], host.peak[s])
        idx, am, ak, bm, bk = common(whole, cut, s)
        assert len(idx) >= 2 and same_bits(am, bm) and same_bits(ak, bk)
        assert single.idx[s] == [0] and same_bits(single.mean[s][0], block.mean[s][0])
    assert not same_bits(cut.mean[0], cut.mean[2])


def test_rds_pieces(fmx_amd):
    """One call of 400 000 input samples with the RDS decoder on is made in RDS pieces (at most 384 000 input samples each): the records are those of
    the same stream in calls of 16 384."""
    m = fmx_amd.fmx
    n = 400000
    raw = raw_streams(0, n, 1)
    params = [(m.P_RDS_MODE, 2)]
    one = Run(fmx_amd, raw, 0, [n], 4, 3, metered=(0,), via="host", params=params)
    small = Run(fmx_amd, raw, 0, [16384] * (n // 16384) + [n % 16384], 4, 3, metered=(0,), via="host", params=params)
    assert small.idx[0] == list(range(pm.n_blocks(n, 3) // 4)) and one.idx[0] == small.idx[0][-4:] and len(one.idx[0]) == 4
    idx, am, ak, bm, bk = common(one, small, 0)
    assert idx == one.idx[0] and same_bits(am, bm) and same_bits(ak, bk)


def test_overlapping_pieces(fmx_amd):
    """A 1024-channel PLL-decoder handle on 2 shared streams makes a call of 98 304 samples in overlapping pieces of 1536 fm samples; the meter runs on
    stage A's stream of every piece.  The records are those of the same streams in calls of 16 384 on a handle of two channels."""
    m = fmx_amd.fmx
    n = 98304
    raw = raw_streams(0, n, 2)
    big = Run(fmx_amd, raw, 0, [n], 2, 1, metered=(0, 1), via="host", channels=1024, som=[c % 2 for c in range(1024)],
              params=[(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0), (m.P_CALL_PIECES, 1536)])
    assert big.pieces[0] > 1
    small = Run(fmx_amd, raw, 0, [16384] * 6, 2, 1, metered=(0, 1), via="host")
    for s in (0, 1):
        assert small.idx[s] == list(range(12)) and big.idx[s] == [8, 9, 10, 11]
        idx, am, ak, bm, bk = common(big, small, s)
        assert idx == big.idx[s] and same_bits(am, bm) and same_bits(ak, bk)


def everything(f, m, channels):
    """what a handle delivers beside the spectrum meter"""
    return dict(meta=[bytes(f.meta(c)) for c in range(channels)], bits=[f.rds_bits(c).tobytes() for c in range(min(channels, 3))],
                mod=[r.tobytes() for r in f.mod_records()], audio=[r.tobytes() for r in f.audio_records()], rx=[r.tobytes() for r in f.rx_records()],
                rdsm=[r.tobytes() for r in f.rds_meter_records()], facts=(f.last_second_group(), f.last_call_pieces(), f.last_front_kernel()))


@pytest.mark.parametrize("channels", [1, 130])
def test_everything_else_is_undisturbed(fmx_amd, ol, channels):
    """With the spectrum meter on for every stream, PCM, RDS bits, meta, the four other meters' records and the facts about the last call equal a twin
    handle's without it, bit for bit: on a 1-channel block-machine handle and on a batch of 130 channels on 3 shared streams."""
    m = fmx_amd.fmx
    blk, ncalls = 16384, 24
    streams = 1 if channels == 1 else 3
    x = np.stack([ol.synth_iq(ncalls * blk, rds=1, leftHz=500.0 + 300 * s, rightHz=900.0 + 200 * s) for s in range(streams)])
    out = []
    for meter in (False, True):
        f = fmx_amd.Fmx(channels, streams=streams if channels > 1 else 0, stream_of_channel=[c % streams for c in range(channels)] if channels > 1 else None,
                        max_block=blk)
        f.set_param(m.P_BANDWIDTH, 165000)
        f.set_param(m.P_RDS_MODE, 2)
        f.mod_meter(True); f.audio_meter(True); f.rx_meter(True); f.rds_meter_enable(True)
        if meter:
            f.spectrum_setup(2, 1)
            f.spectrum_meter(True)
        pcm = np.concatenate([f.process_host(x[:, k * blk:(k + 1) * blk]) for k in range(ncalls)], axis=1)
        e = everything(f, m, channels)
        e["pcm"] = pcm
        e["spec"] = [f.spectrum_read(s)[0] for s in range(streams)]
        out.append(e)
        f.close()
    a, b = out
    assert np.array_equal(a["pcm"], b["pcm"]) and a["pcm"].shape[1] > 0
    for key in ("meta", "bits", "mod", "audio", "rx", "rdsm", "facts"):
        assert a[key] == b[key], key
    assert len(a["bits"][0]) > 0 and len(a["mod"][0]) > 0 and len(a["audio"][0]) > 0 and len(a["rx"][0]) > 0 and len(a["rdsm"][0]) > 0
    assert all(r.size == 0 for r in a["spec"]) and all(list(r["index"]) == [44, 45, 46, 47] for r in b["spec"])


def test_switch_ring_and_cursors(fmx_amd):
    raw = raw_streams(0, 24 * N, 3)
    m = fmx_amd.fmx
    B, S = 2, 1
    ref = Run(fmx_amd, raw, 0, [2 * N] * 12, B, S, via="host")       # the meter on throughout: records 0 .. 11, what a switched meter's records must equal
    assert ref.idx[0] == list(range(12))
    f = fmx_amd.Fmx(3, max_block=4 * N)
    try:
        f.spectrum_setup(B, S)
        call = lambda k, n=2 * N: f.process_host_raw(raw[:, k:k + n], 0)
        g = 0
        call(g, N + 100); g += N + 100                          # (no meter yet: nothing is allocated, nothing is read)
        assert f.spectrum_read(0)[0].size == 0
        f.spectrum_meter(True, 0)                               # in mid-stream, inside block 1: the first block is 2, the first whole record 1
        with pytest.raises(fmx_amd.FmxError) as e:              # the grid is fixed while a meter is on
            f.spectrum_setup(4, 1)
        assert e.value.code == m.FMX_E_INVALID
        call(g, 3 * N); g += 3 * N                              # blocks 1 (not taken), 2, 3 complete
        r, mean, peak = f.spectrum_read(0)
        assert list(r["index"]) == [1] and int(r["end_sample"][0]) == 4 * N
        assert same_bits(mean[0], ref.mean[0][1]) and same_bits(peak[0], ref.peak[0][1])
        f.spectrum_meter(True, 2)                               # a second stream: its memory is added, stream 0's is kept
        call(g, 2 * N - 100); g += 2 * N - 100                  # g = 6 N: record 2 complete for stream 0; stream 2 switched on inside block 4
        assert list(f.spectrum_read(0)[0]["index"]) == [2] and f.spectrum_read(2)[0].size == 0
        f.spectrum_meter(False, 0)
        call(g, 2 * N); g += 2 * N                              # record 3: stream 0 is off, stream 2's first whole record
        assert f.spectrum_read(0)[0].size == 0 and list(f.spectrum_read(2)[0]["index"]) == [3]
        f.spectrum_meter(True, 0)
        call(g, N); g += N                                      # stream 0 on again at 8 N: block 8 taken, record 4 begun
        call(g, 5 * N // 2)
        g += 5 * N // 2                                         # 11.5 N: records 4 complete
        r, mean, peak = f.spectrum_read(0)
        assert list(r["index"]) == [4]                          # a gap in index: record 3 was not metered
        assert same_bits(mean[0], ref.mean[0][4]) and same_bits(peak[0], ref.peak[0][4])      # no stale sums
        # five records unread: the oldest is lost, and index shows it; capacity smaller than what is there; independent cursors
        call(g, N // 2); g += N // 2                            # 12 N: record 5
        for _ in range(4):
            call(g, 2 * N); g += 2 * N                          # records 6 .. 9
        r2 = f.spectrum_read(2, capacity=1)[0]
        assert list(r2["index"]) == [6]                         # stream 2 never read 4 and 5: of 4 .. 9 the ring holds 6 .. 9
        assert list(f.spectrum_read(0, capacity=3)[0]["index"]) == [6, 7, 8]
        assert list(f.spectrum_read(0)[0]["index"]) == [9] and list(f.spectrum_read(2)[0]["index"]) == [7, 8, 9]
        assert f.spectrum_read(0)[0].size == 0 and f.spectrum_read(1)[0].size == 0
        rec, mean, none = f.spectrum_read(0, peak=False)
        assert none is None
        f.spectrum_meter(False)
        f.spectrum_setup(1, 2)                                  # a new grid: indices and cursors start over
        f.spectrum_meter(True, 1)
        call(g, 2 * N)
        r, _, _ = f.spectrum_read(1)
        assert list(r["index"]) == [10] and int(r["every"][0]) == 2 and int(r["end_sample"][0]) == 21 * N       # (block 10 begins at 20 N)
    finally:
        f.close()


def test_input_rate_192000(fmx_amd, kernel_form):
    """inputRate 192 000: the handle does not decimate (twelve twins per channel); the meter reads the same input"""
    raw = raw_streams(0)[:1]
    run = Run(fmx_amd, raw, 0, CUTS, 2, 1, metered=(0,), inputRate=192000)
    x = wm.convert(raw[0], 0)
    idx, m64, k64 = pm.records64(x, 2, 1)
    _, m32, k32 = pm.records32(x, 2, 1)
    kf = kernel_form(x, 2, 1)
    assert run.idx[0] == idx == expected_indices(CUTS, 2, 1)
    ok, rw, rm = sm.check_spectrum("GPU mean, 192 kS/s", run.mean[0], m64, *sm.levels(m64, m32, np.stack([kf[r][0] for r in idx])))
    assert ok, (rw, rm)
    ok, rw, rm = sm.check_spectrum("GPU peak, 192 kS/s", run.peak[0], k64, *sm.levels(k64, k32, np.stack([kf[r][1] for r in idx])))
    assert ok, (rw, rm)


def test_eleven_channels_on_one_stream(fmx_amd):
    """2 304 000 S/s, eleven channels on one stream at -1000 .. +1000 kHz, amplitudes alternating by 12 dB: ONE record of the stream, and the figures at
    each channel's centre_hz find each neighbour."""
    m = fmx_amd.fmx
    B = 8
    n = N * B
    centres = [200000 * (i - 5) for i in range(11)]
    amp = [0.02 * (4.0 if i % 2 else 1.0) for i in range(11)]
    x = sum(pm.fm_noise(n, 2304000, fc, a, 8000.0, seed=20 + i) for i, (fc, a) in enumerate(zip(centres, amp))) + pm.white(n, 1e-10, seed=19)
    raw = sm.to_raw(x, 0)[None]
    run = Run(fmx_amd, raw, 0, [n // 2, n // 2], B, 1, metered=(0,), via="host", channels=11, som=[0] * 11,
              each=lambda f, k: [f.set_param(m.P_LOCAL_OSCILLATOR, fc, c) for c, fc in enumerate(centres)] if k == 0 else None)
    assert run.idx[0] == [0]
    # The generator's levels alternate by 12.04 dB.  A figure finds a neighbour when it tells one 12 dB up from an equal one and from one 12 dB down:
    # within 6 dB, half the step.  The same for a channel's own level.
    step = 10 * np.log10(16.0)
    for i, fc in enumerate(centres):
        g = fmx_amd.spectrum_figures(run.mean[0][0], run.peak[0][0], rate_hz=2304000, centre_hz=fc, raster_hz=200000)
        print("[%+8d Hz] channel %.2f dB (sent %.2f), adj %s" % (fc, g["channel_db"], 10 * np.log10(amp[i] ** 2 * N), ["%.2f" % v for v in g["adj_db"]]))
        assert abs(g["channel_db"] - 10 * np.log10(amp[i] ** 2 * N)) < step / 2, (fc, g)
        for j, k in ((0, i - 2), (1, i - 1), (2, i + 1), (3, i + 2)):
            if 0 <= k < 11:
                assert abs(g["adj_db"][j] - 20 * np.log10(amp[k] / amp[i])) < step / 2, (fc, j, g["adj_db"])
            else:                                               # (beyond +-1000 kHz the window leaves |f| <= rate / 2 - 50 kHz)
                assert g["adj_db"][j] == -np.inf, (fc, j, g["adj_db"])


def build_demo(fmx_amd, exe):
    import test_spec_cpu
    test_spec_cpu.build_demo(fmx_amd, exe)


def test_the_cpp_demo_builds_and_runs(fmx_amd, tmp_path):
    """tests/spec_demo through host/fm_processor_adapter.h: blocks of 16 384, B = 2: the records the Python handle delivers for the same stream"""
    exe, fin, fout = str(tmp_path / "spec_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "spec.bin")
    build_demo(fmx_amd, exe)
    raw = raw_streams(0, 6 * 16384, 1)
    raw[0].tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    assert out.returncode == 0 and lines[-1].startswith("records 12 "), lines
    rows = np.fromfile(fout, np.float32).reshape(-1, 1 + 2 * N)
    run = Run(fmx_amd, raw, 0, [16384] * 6, 2, 1, metered=(0,), via="host")
    assert [int(v) for v in rows[:, 0]] == run.idx[0] == list(range(12))
    assert same_bits(rows[:, 1:1 + N], run.mean[0]) and same_bits(rows[:, 1 + N:], run.peak[0])

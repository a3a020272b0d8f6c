"""Stage W's band survey (fmx_survey.hip, include/fmx.h fmx_wideband_survey_*) on the GPU against the float64 model of tests/survey_model.py.

The bound of every spectrum comparison: a bin's error is |P - P64| / P64; per case, level_worst is the larger of the worst
bins of the two f32 restatements of the same records -- the plain one (radix-2, complex64) and kernel_form (fmx_survey.h's own stage
functions on the host, tests/survey_check.cpp) --, level_median the larger of their medians; the GPU must stay within 2 x level_worst on
every bin and within 2 x level_median in the median.  Shapes: 2 streams of 10 blocks of 4096 and 100 samples, B = 3."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import survey_model as sm
import wideband_model as wm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = sm.N
B = 3
FACTORS = [2, 5, 16]
FMT_NAMES = {0: "F32", 1: "U8", 2: "S8", 3: "S16/2048"}
GAP = 37                              # wide_stride - n_wide of the device input
GAP_CODE = {0: np.nan, 1: 255, 2: -128, 3: -32768}
OFFSETS = [100000, -300000]           # one output per stream


@pytest.fixture(scope="module")
def kernel_form(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("survey")
    exe = str(d / "survey_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "survey_check.cpp")])

    def run(x, blocks_per_record):
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.asarray(x, np.complex64).tofile(fi)
        subprocess.check_call([exe, "spectrum", fi, fo, str(blocks_per_record)])
        return np.fromfile(fo, np.float32).reshape(-1, N + 1)[:, 1:]
    return run


_RAW = {}


def raw_streams(K, fmt):
    """[2, n, 2] in the raw format: two different streams of survey_model.spectrum_signal."""
    if (K, fmt) not in _RAW:
        n = sm.stream_length(K)
        _RAW[K, fmt] = np.stack([sm.to_raw(sm.spectrum_signal(K, n, seed=s), fmt) for s in range(2)])
    return _RAW[K, fmt]


class Run:
    """One object of 2 streams fed `raw` in calls of the given lengths, every stream's records read behind every call: recs [s], power [s]
    ([records, N]), narrow ([2, n / K, 2]) and what a last read returns (after [s]).  via: the device entry point (input with a stride, the gap
    filled with NaN or extreme codes) or the host entry point.  survey: blocks per record, or 0: never enabled."""

    def __init__(self, fmx_amd, K, raw, fmt, cuts, via="device", survey=B, capacity=4):
        n = raw.shape[1]
        assert sum(cuts) == n
        self.recs, self.power, narrow = [[], []], [[], []], []
        w = fmx_amd.Wideband(K, [0, 1], OFFSETS, streams=2, max_block=max(cuts))
        try:
            if survey:
                w.survey(survey)
            if via == "device":
                import torch
                padded = np.full((2, n + GAP, 2), GAP_CODE[fmt], raw.dtype)
                padded[:, :n] = raw
                d_wide = torch.from_numpy(padded).cuda()
                d_narrow = torch.zeros((2, n // K, 2), dtype=torch.float32, device="cuda")
                bps = raw.dtype.itemsize * 2
            pos = 0
            for ln in cuts:
                if via == "device":
                    got = w.process_device(d_wide.data_ptr() + bps * pos, n + GAP, ln, d_narrow.data_ptr() + 8 * (pos // K), n // K, fmt=fmt)
                    assert got == ln // K
                else:
                    narrow.append(w.process_host(raw[:, pos:pos + ln], fmt, 2048.0))
                pos += ln
                for s in range(2):
                    r, p = w.survey_read(s, capacity)
                    self.recs[s] += list(r)
                    self.power[s] += list(p)
            if via == "device":
                torch.cuda.synchronize()
                self.narrow = d_narrow.cpu().numpy()
            else:
                self.narrow = np.concatenate(narrow, axis=1)
            self.after = [w.survey_read(s)[0] for s in range(2)]
        finally:
            w.close()
        self.power = [np.array(p, np.float32).reshape(-1, N) for p in self.power]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("K", FACTORS)
def test_records_against_the_float64_model(fmx_amd, kernel_form, K, fmt):
    """The cuts of survey_model.call_cuts: calls that complete no block (the carry grows across three), a block completed from the carry with a
    tail left, a call of several blocks, a call that ends on a block boundary, a call of K samples.  Device input with wide_stride > n_wide, the
    gap filled with NaN / extreme codes."""
    raw = raw_streams(K, fmt)
    run = Run(fmx_amd, K, raw, fmt, sm.call_cuts(K))
    n_rec = 10 // B
    P64, P32, PKF = [], [], []
    for s in range(2):
        x = wm.convert(raw[s], fmt)
        P64.append(sm.records64(x, B))
        P32.append(sm.records32(x, B))
        PKF.append(kernel_form(x, B))
        recs = run.recs[s]
        assert [int(r["index"]) for r in recs] == list(range(n_rec))
        assert [int(r["end_sample"]) for r in recs] == [(r + 1) * B * N for r in range(n_rec)]
        assert all(int(r["blocks"]) == B and int(r["reserved"]) == 0 for r in recs)
        assert len(run.after[s]) == 0
    P64, P32, PKF, got = (np.concatenate(v) for v in (P64, P32, PKF, run.power))
    assert got.shape == (2 * n_rec, N) and np.all(np.isfinite(got))
    lw, lm = sm.levels(P64, P32, PKF)
    print()
    ok, rw, rm = sm.check_spectrum("GPU, K = %d, %s" % (K, FMT_NAMES[fmt]), got, P64, lw, lm)
    assert ok, (rw, rm)


@pytest.mark.parametrize("K", FACTORS)
def test_cuts_are_bit_identical(fmx_amd, K):
    """One call against the cuts, and the host-buffer entry point against the device-buffer one: the same records, byte for byte."""
    raw = raw_streams(K, 0)
    n = raw.shape[1]
    whole = Run(fmx_amd, K, raw, 0, [n])
    cut = Run(fmx_amd, K, raw, 0, sm.call_cuts(K))
    host = Run(fmx_amd, K, raw, 0, sm.call_cuts(K), via="host")
    for s in range(2):
        assert whole.power[s].shape == (10 // B, N)
        assert same_bits(whole.power[s], cut.power[s]) and same_bits(whole.power[s], host.power[s]), s
        for other in (cut, host):
            assert [tuple(r) for r in whole.recs[s]] == [tuple(r) for r in other.recs[s]]
    assert same_bits(cut.narrow, host.narrow) and same_bits(whole.narrow, cut.narrow)


@pytest.mark.parametrize("K", FACTORS)
def test_stage_w_is_undisturbed(fmx_amd, K):
    """Stage W's outputs with the survey on are those of a twin that never enabled it; an object that enabled and then disabled the survey reads
    no records afterwards."""
    raw = raw_streams(K, 1)
    on = Run(fmx_amd, K, raw, 1, sm.call_cuts(K))
    off = Run(fmx_amd, K, raw, 1, sm.call_cuts(K), survey=0)
    assert len(on.recs[0]) == 10 // B and off.recs == [[], []]
    assert np.any(on.narrow != 0) and same_bits(on.narrow, off.narrow)
    w = fmx_amd.Wideband(K, [0, 1], OFFSETS, streams=2, max_block=raw.shape[1])
    try:
        cut = -(-2 * N // K) * K
        w.survey(1)
        w.process_host(raw[:, :cut], 1)                                # two records, unread
        w.survey(0)
        a = w.process_host(raw[:, cut:], 1)
        for s in range(2):
            assert len(w.survey_read(s)[0]) == 0
    finally:
        w.close()
    assert same_bits(a, off.narrow[:, cut // K:])


def test_ring_and_cursor(fmx_amd):
    K = 2
    raw = raw_streams(K, 0)
    M = fmx_amd.fmx
    P64 = [sm.records64(wm.convert(raw[s], 0), 1) for s in range(2)]
    w = fmx_amd.Wideband(K, [0, 1], OFFSETS, streams=2, max_block=6 * N)

    def close_to(P, s, block):                                         # (which block a record is of: far inside any f32 bound)
        return np.max(np.abs(P - P64[s][block]) / P64[s][block]) < 1e-3
    try:
        w.survey(1)
        w.process_host(raw[:, :6 * N])                                 # six records between two reads: the newest four, the gap shows in `index`
        for s in range(2):
            r, p = w.survey_read(s, 8)
            assert [int(v) for v in r["index"]] == [2, 3, 4, 5]
            assert [int(v) for v in r["end_sample"]] == [3 * N, 4 * N, 5 * N, 6 * N]
            assert all(close_to(p[i], s, 2 + i) for i in range(4))
        w.process_host(raw[:, 6 * N:9 * N])                            # three more, read in pieces
        for i in range(3):
            r, p = w.survey_read(0, 1)
            assert [int(v) for v in r["index"]] == [6 + i] and close_to(p[0], 0, 6 + i)
        assert len(w.survey_read(0, 1)[0]) == 0
        r, _ = w.survey_read(1, 2)                                     # (every stream has its own read position)
        assert [int(v) for v in r["index"]] == [6, 7]
        w.survey(2)                                                    # a new survey: stream 1's record 8 is dropped, `index` starts over
        w.process_host(raw[:, 9 * N:10 * N])
        assert len(w.survey_read(1)[0]) == 0
        w.process_host(raw[:, :3 * N])
        x = wm.convert(np.concatenate([raw[1, 9 * N:10 * N], raw[1, :3 * N]]), 0)
        r, p = w.survey_read(1)
        assert [(int(v["index"]), int(v["end_sample"]), int(v["blocks"])) for v in r] == [(0, 11 * N, 2), (1, 13 * N, 2)]
        ref = sm.records64(x, 2)
        assert np.max(np.abs(p - ref) / ref) < 1e-3
        # rejected arguments
        for bad in (-1, 4097):
            with pytest.raises(fmx_amd.FmxError) as e:
                w.survey(bad)
            assert e.value.code == M.FMX_E_INVALID
        for bad in (-1, 2):
            with pytest.raises(fmx_amd.FmxError) as e:
                w.survey_read(bad)
            assert e.value.code == M.FMX_E_INVALID
        n = C.c_int32(-1)
        assert w.L.fmx_wideband_survey_read(w.h, 0, None, None, 1, C.byref(n)) == M.FMX_E_INVALID
        assert w.L.fmx_wideband_survey_read(w.h, 0, None, None, 0, C.byref(n)) == M.FMX_OK and n.value == 0
    finally:
        w.close()


# ---- cold start, end to end -----------------------------------------------------------------------------------------------------------
CS_K = 4
CS_STATIONS = [(-1200000, 0.2, 2000.0), (300000, 0.02, 3000.0), (2100000, 0.1, 5000.0)]      # (offset, amplitude, audio tone)
CS_BLOCK = 49152                      # narrow samples per call
CS_CALLS = 4                          # 0.085 s of signal through the chain: its PCM begins 0.064 s in (the reference's start-up)
CS_TAIL = 768                         # frames read at the end: every tone a whole number of 62.5 Hz bins


def test_cold_start(fmx_amd):
    """An object created with all offsets 0 finds its stations: one record of B = 16, survey_stations, set_offset, and every channel's strongest
    PCM tone -- read from the last 16 ms of 85 ms through stage W and a 3-channel handle -- is its own station's."""
    M = fmx_amd.fmx
    n_survey = 16 * N
    n = n_survey + CS_CALLS * CS_BLOCK * CS_K
    x = sm.fm_stations(CS_K, n, CS_STATIONS, noise_power=1e-4, seed=5, deviation=50000.0)      # noise at 0.01
    wide = sm.to_raw(x, 0)[None]
    w = fmx_amd.Wideband(CS_K, [0, 0, 0], [0, 0, 0], streams=1, max_block=CS_BLOCK * CS_K)
    f = fmx_amd.Fmx(3, max_block=CS_BLOCK)
    for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 2)):
        f.set_param(pid, v)
    try:
        w.survey(16)
        w.process_host(wide[:, :n_survey])
        recs, power = w.survey_read(0, 1)
        assert len(recs) == 1 and int(recs[0]["end_sample"]) == n_survey
        stations, floor_db = fmx_amd.survey_stations(power[0], CS_K, threshold_db=10.0)
        print("\n[cold start] floor %.2f dB, stations %s" % (floor_db, [(int(s["offset_hz"]), round(float(s["snr_db"]), 1)) for s in stations]))
        assert [int(s["offset_hz"]) for s in stations] == [f0 for f0, _, _ in CS_STATIONS]
        w.survey(0)
        for m, s in enumerate(stations):
            w.set_offset(m, int(s["offset_hz"]))
        pcm = []
        for k in range(CS_CALLS):
            a = n_survey + k * CS_BLOCK * CS_K
            pcm.append(f.process_host(w.process_host(wide[:, a:a + CS_BLOCK * CS_K])))
    finally:
        w.close()
        f.close()
    pcm = np.concatenate(pcm, axis=1)
    for c, (f0, _, tone) in enumerate(CS_STATIONS):
        seg = pcm[c][-CS_TAIL:, 0].astype(np.float64)
        spec = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
        spec[:4] = 0.0
        peak_hz = float(np.argmax(spec)) * 48000.0 / len(seg)
        print("[cold start, station at %+d Hz] strongest PCM tone %.1f Hz (sent %.0f)" % (f0, peak_hz, tone))
        assert len(seg) == CS_TAIL and np.sqrt(np.mean(seg ** 2)) > 0.001 and abs(peak_hz - tone) <= 48000.0 / len(seg) * 1.5, (c, peak_hz)


# ---- the C++ wrapper -------------------------------------------------------------------------------------------------------------------
def build_demo(fmx_amd, exe):
    host = os.path.join(ROOT, "sdr-j-fm_amd", "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + host, os.path.join(ROOT, "tests", "survey_demo", "survey_adapter_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])


def test_cpp_adapter(fmx_amd, tmp_path):
    """host/wideband_adapter.h: survey, processHost in two calls, readSurvey and stations write what fmx_amd computes for the same input, byte for
    byte."""
    M = fmx_amd.fmx
    K, blocks_per_record, n_first, threshold = 4, 2, 1000 * 4, 10.0
    x = sm.fm_stations(K, 5 * N, [(-800000, 0.2, 2500.0), (1500000, 0.05, 4000.0)], seed=9)
    wide = sm.to_raw(x, 0)
    exe, fin, fout = str(tmp_path / "survey_adapter_demo"), str(tmp_path / "wide.f32"), str(tmp_path / "survey.bin")
    build_demo(fmx_amd, exe)
    wide.tofile(fin)
    out = subprocess.run([exe, fin, fout, str(K), str(blocks_per_record), str(n_first), str(threshold)], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=120)
    text = out.stdout.decode()
    assert out.returncode == 0 and "finder 0" in text and "ok 1" in text and "records 2" in text, text
    w = fmx_amd.Wideband(K, [0], [0], streams=1, max_block=5 * N)
    try:
        w.survey(blocks_per_record)
        w.process_host(wide[None, :n_first])
        w.process_host(wide[None, n_first:])
        recs, power = w.survey_read(0)
    finally:
        w.close()
    assert len(recs) == 2
    want = b""
    for r, p in zip(recs, power):
        st, floor_db = fmx_amd.survey_stations(p, K, threshold_db=threshold)
        assert [int(s["offset_hz"]) for s in st] == [-800000, 1500000]
        want += r.tobytes() + p.tobytes() + np.int32(len(st)).tobytes() + np.float32(floor_db).tobytes() + st.tobytes()
    assert M.SURVEY_RECORD_DTYPE.itemsize == 24 and M.SURVEY_STATION_DTYPE.itemsize == 16
    assert open(fout, "rb").read() == want

"""CPU checks of stage W's band survey (sdr-j-fm_amd/csrc/fmx_survey.h): the header's own stage functions compiled for the
host and driven thread by thread (tests/survey_check.cpp, "kernel_form") against the float64 model of tests/survey_model.py; the detector
of the spectrum bound against seeded defects; the per-call bookkeeping against a brute-force count; the station finder through the C export
(which needs no device) against the model's finder."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import survey_model as sm
import wideband_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = sm.N


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("survey")
    exe = str(d / "survey_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "survey_check.cpp")])

    def spectrum(x, B, cuts=()):
        """-> {record index: P [N] f32} of the records still in the ring behind the call that completed them"""
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.asarray(x, np.complex64).tofile(fi)
        subprocess.check_call([exe, "spectrum", fi, fo, str(B)] + [str(c) for c in cuts])
        raw = np.fromfile(fo, np.float32).reshape(-1, N + 1)
        return {int(row[0]): row[1:] for row in raw}

    def plan(quads):
        out = subprocess.run([exe, "plan"] + [str(v) for q in quads for v in q], capture_output=True, text=True, check=True).stdout
        return [tuple(int(v) for v in line.split()) for line in out.splitlines()]
    return spectrum, plan


_SIGNALS = {}


def signal(K):
    """The spectrum comparisons' stream, as the exact f32 values the library converts to."""
    if K not in _SIGNALS:
        _SIGNALS[K] = wm.convert(sm.to_raw(sm.spectrum_signal(K, sm.stream_length(K)), 0), 0)
    return _SIGNALS[K]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [2, 5, 16])
def test_kernel_form_against_the_float64_model(check, K, B):
    """The bound of DESIGN.md 4.9 with the level taken from the plain restatement alone."""
    spectrum, _ = check
    x = signal(K)
    P64, P32 = sm.records64(x, B), sm.records32(x, B)
    assert P64.shape == (10 // B, N)
    lw, lm = sm.levels(P64, P32)
    cut, whole = spectrum(x, B, sm.call_cuts(K)), spectrum(x, B)
    assert len(cut) >= 6 // B and max(cut) == 10 // B - 1
    for r, P in whole.items():                                        # however the stream is cut: the same bits
        if r in cut:
            assert np.array_equal(P.view(np.uint32), cut[r].view(np.uint32)), r
    idx = sorted(cut)
    print()
    ok, rw, rm = sm.check_spectrum("kernel_form, K = %d, B = %d, %d records" % (K, B, len(idx)), np.stack([cut[r] for r in idx]), P64[idx], lw, lm)
    assert ok, (rw, rm)


def test_the_detector_catches_seeded_defects(check):
    """Each defect in a restated record must break the bound whose level both restatements set."""
    spectrum, _ = check
    K, B = 5, 3
    x = signal(K)
    P64 = sm.records64(x, B)
    p = sm.block_powers32(x)
    good = sm.records_from_powers32(p, B)
    kf = spectrum(x, B)
    lw, lm = sm.levels(P64, good, np.stack([kf[r] for r in range(3)]))
    print("\n[levels, K = %d, B = %d] worst %.3e, median %.3e" % (K, B, lw, lm))
    assert sm.check_spectrum("no defect", good, P64, lw, lm)[0]
    left_out = p.copy()
    left_out[4] = 0.0
    swapped = p.copy()
    swapped[[B - 1, B]] = swapped[[B, B - 1]]
    cut = 2 * N + 1234                                                # a call boundary whose carry lost its last sample
    short = sm.block_powers32(np.concatenate([x[:cut - 1], x[cut:]]))
    defects = {
        "one block left out of a record": sm.records_from_powers32(left_out, B),
        "two blocks swapped across a record boundary": sm.records_from_powers32(swapped, B),
        "the carry one sample short": sm.records_from_powers32(short, B),
        "bins mirrored": good[:, (N - np.arange(N)) % N],
        "the scale of B + 1": sm.records_from_powers32(p, B, scale=sm.record_scale(B + 1)),
    }
    for name, rec in defects.items():
        ok, rw, rm = sm.check_spectrum(name, rec[:3], P64, lw, lm)
        assert not ok, name


def test_bookkeeping_against_a_brute_force_count(check):
    _, plan = check
    quads = [(fill, n, blocks, B) for fill in (0, 1, N - 1) for n in (2, 5, 16, N - 1, N, N + 1, 3 * N + 17) for B in (1, 3, 4096)
             for blocks in (0, 2, 4095, 3 * 4096 - 1)]
    got = plan(quads)
    assert len(got) == len(quads)
    for q, g in zip(quads, got):
        assert g == sm.brute_plan(*q), (q, g)


# ---- the station finder -------------------------------------------------------------------------------------------------------------------
def record_of(K, stations, B=16, **kw):
    x = sm.fm_stations(K, B * N, stations, **kw)
    return sm.records64(wm.convert(sm.to_raw(x, kw.pop("fmt", 0)), 0), B)[0].astype(np.float32)


FIND_CASES = {
    # name: (K, stations (offset, amplitude, tone), signal options, finder options)
    "K = 2": (2, [(-900000, 0.3, 2000.0), (-500000, 0.02, 3000.0), (400000, 0.1, 5000.0)], {}, {}),
    # (K = 4, K = 16: a station of 0.015, 26 dB below its neighbour of 0.3, 400 kHz away)
    "K = 4": (4, [(-4400000, 0.1, 2000.0), (-1200000, 0.3, 2500.0), (-800000, 0.015, 3000.0), (300000, 0.05, 4000.0), (4458000 // 100000 * 100000, 0.02, 6000.0)], {}, {}),
    "K = 16": (16, [(-18200000, 0.02, 2000.0), (-100000, 0.3, 3000.0), (300000, 0.015, 2500.0), (9900000, 0.1, 8000.0)], {}, {}),
    "dense band, K = 8": (8, [(-8800000 + 400000 * i, 0.02 + 0.28 * ((i * 7) % 11) / 10.0, 2000.0 + 250.0 * i) for i in range(45)], {}, {}),
    "DC spike, no guard": (4, [(200000, 0.05, 3000.0)], {"dc": 0.05}, {}),
    "DC spike, guard": (4, [(200000, 0.05, 3000.0)], {"dc": 0.05}, {"dc_guard_hz": 20000}),
    "raster origin": (4, [(-1470000, 0.1, 2500.0), (230000, 0.05, 4000.0)], {}, {"origin_hz": 30000}),
}
_RECORDS = {}


def case_record(name):
    if name not in _RECORDS:
        K, stations, sig, _ = FIND_CASES[name]
        _RECORDS[name] = record_of(K, stations, seed=len(name), **sig)
    return _RECORDS[name]


@pytest.mark.parametrize("threshold", [6.0, 10.0, 20.0])
@pytest.mark.parametrize("name", list(FIND_CASES))
def test_stations_through_the_c_export_against_the_model(fmx_amd, name, threshold):
    K, stations, _, opts = FIND_CASES[name]
    P = case_record(name)
    ref, ref_floor = sm.find_stations(P, K, threshold_db=threshold, **opts)
    got, floor_db = fmx_amd.survey_stations(P, K, threshold_db=threshold, **opts)
    print("\n[%s, threshold %g dB] floor %.2f dB, found %s" % (name, threshold, floor_db, [int(f) for f in got["offset_hz"]]))
    assert [int(f) for f in got["offset_hz"]] == [f for f, _, _ in ref]
    assert abs(floor_db - ref_floor) <= 1e-3
    for g, (_, level, snr) in zip(got, ref):
        assert abs(float(g["level_db"]) - level) <= 1e-3 and abs(float(g["snr_db"]) - snr) <= 1e-3, (g, level, snr)
    lim = wm.offset_limit(K)
    assert all(abs(int(f)) <= lim for f in got["offset_hz"])             # what fmx_wideband_set_offset accepts
    if name != "DC spike, no guard":                                     # (the LO leak moves that station: what the guard is for)
        assert [int(f) for f in got["offset_hz"]] == sorted(f for f, _, _ in stations), name


def test_a_u8_stream_finds_the_same_stations(fmx_amd):
    K, stations, _, _ = FIND_CASES["K = 4"]
    x = sm.fm_stations(K, 16 * N, stations, seed=4)
    P = sm.records64(wm.convert(sm.to_raw(x, 1), 1), 16)[0].astype(np.float32)
    got, _ = fmx_amd.survey_stations(P, K, dc_guard_hz=20000)            # (U8's zero is code 127.5: an offset of 1 / 256 at bin 0)
    assert [int(f) for f in got["offset_hz"]] == sorted(f for f, _, _ in stations)


def test_every_candidate_is_an_offset_set_offset_accepts(fmx_amd):
    """A record that is a station everywhere: all candidates compete, and the extreme ones returned lie inside the limit."""
    for K in (2, 7, 16):
        for raster, origin in ((100000, 0), (50000, -49999), (1000000, 999999), (100000, 30000)):
            P = np.ones(N, np.float32)
            P[::7] = 1e-6                                                # the lower decile: a floor far below
            got, _ = fmx_amd.survey_stations(P, K, raster_hz=raster, origin_hz=origin, threshold_db=3.0)
            ref, _ = sm.find_stations(P, K, raster_hz=raster, origin_hz=origin, threshold_db=3.0)
            assert [int(f) for f in got["offset_hz"]] == [f for f, _, _ in ref] and len(ref) >= 1
            lim = wm.offset_limit(K)
            assert all(abs(int(f)) <= lim and (int(f) - origin) % raster == 0 for f in got["offset_hz"])


def test_capacity_and_rejected_arguments(fmx_amd):
    import ctypes as C
    M = fmx_amd.fmx
    L = fmx_amd.load_library()
    P = case_record("K = 4")
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def call(P, capacity=8, **kw):
        f = dict(struct_size=C.sizeof(M.FmxSurveyFind), factor=4, raster_hz=100000, origin_hz=0, dc_guard_hz=0, threshold_db=10.0)
        f.update(kw)
        cfg = M.FmxSurveyFind(**f)
        out = np.full(8, -1, M.SURVEY_STATION_DTYPE)
        n, fl = C.c_int32(-7), C.c_float()
        rc = L.fmx_wideband_survey_stations(C.byref(cfg), fp(P), out.ctypes.data_as(C.c_void_p), capacity, C.byref(n), C.byref(fl))
        return rc, n.value, out

    rc, n, out = call(P)
    assert rc == M.FMX_OK and n == 5
    rc, n, small = call(P, capacity=2)
    assert rc == M.FMX_E_TOO_LARGE and n == 5
    assert np.array_equal(small[:2], out[:2]) and np.all(small["offset_hz"][2:] == -1)      # nothing written beyond the capacity
    for bad in (dict(struct_size=8), dict(factor=1), dict(factor=17), dict(raster_hz=49999), dict(raster_hz=1000001), dict(origin_hz=100000),
                dict(origin_hz=-100000), dict(dc_guard_hz=-1), dict(dc_guard_hz=100000)):
        assert call(P, **bad)[0] == M.FMX_E_INVALID, bad
    for v in (-1e-9, np.nan, np.inf):
        Q = P.copy()
        Q[1000] = v
        assert call(Q)[0] == M.FMX_E_INVALID, v
    rc, n, _ = call(np.zeros(N, np.float32))                             # the all-zero record: no floor, no stations
    assert rc == M.FMX_OK and n == 0
    assert sm.find_stations(np.zeros(N), 4)[0] == []


def test_cpp_adapter_builds_and_finds_without_a_device(fmx_amd, tmp_path):
    """host/wideband_adapter.h's survey methods under -Wall -Werror, in the demo of tests/survey_demo.  stations () needs no device; without one
    the demo then reports ok () == false and the library's text.  (What it writes with a device is checked in tests/test_gpu_survey.py.)"""
    import test_gpu_survey as gs
    exe, fin, fout = str(tmp_path / "survey_adapter_demo"), str(tmp_path / "wide.f32"), str(tmp_path / "survey.bin")
    gs.build_demo(fmx_amd, exe)
    sm.to_raw(sm.fm_stations(4, 2 * N, [(300000, 0.1, 3000.0)]), 0).tofile(fin)
    out = subprocess.run([exe, fin, fout, "4", "1", "4096", "10"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    assert lines and lines[0] == "finder 0", lines
    if out.returncode == 3:
        assert lines[1].startswith("ok 0 error") and "no CPU fallback" in lines[1], lines
    else:
        assert out.returncode == 0 and lines[1].startswith("ok 1") and lines[-1] == "records 2", lines

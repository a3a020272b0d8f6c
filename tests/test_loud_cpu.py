"""The programme audio meter on the CPU: the integers of sdr-j-fm_amd/csrc/fmx_loud.h (tests/loud_check.cpp) against a counter stepped
frame by frame; the float64 model, the f32 restatement and the checker of tests/loud_model.py -- the restatement against float64, the checker against
seeded faults --; and the host-only BS.1770-4 figures of fmx_audio_loudness against an independent numpy implementation and EBU Tech 3341's cases."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import loud_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = lm.WINDOW
# The f32 restatement against float64 on this file's own signals, ms and kms of every window, relative (test_restatement_against_float64 prints them):
# tone 2.33e-6, noise on a DC offset 4.13e-6, programme and silence 1.84e-6 (`distance` says of what).  The bound is twice the largest (DESIGN 5's rule
# for a restatement).
RESTATEMENT_REL = 2 * 4.13e-6


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("loud") / "loud_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "loud_check.cpp")])

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [json.loads(line) for line in out]
    return run


def test_constants_coefficients_division(check):
    g = check(["const"])[0]
    assert (g["window"], g["ring"], g["tile"], g["state"]) == (4800, 64, 64, 16)
    assert g["coef"] == [int(v) for v in lm.K32.reshape(-1).view(np.uint32)]      # the header's literals are the decimal values rounded to f32
    assert g["window_of"] == [0, 1, (2 ** 40 + 4800 * 7 - 1) // 4800]
    vals = [0.0, 1.0, -3.25, 4800.0, 1234.5678, 1e-30, 1e-42, 7.1e5]
    for v, r in zip(vals, check(["finish %d" % struct.unpack("<I", struct.pack("<f", v))[0] for v in vals])):
        assert r["mean"] == int(np.float32(np.float32(v) / np.float32(4800.0)).view(np.uint32))


@pytest.mark.parametrize("base", [0, 1, 4799, 4800, 12345678, 2 ** 32 - 20000, 2 ** 32 + 12345, 2 ** 40 + 4800 * 7 - 3])
def test_audio_produce_against_a_counter(check, base):
    """random cuts and random switch times: whether the states reset, the first frame a piece accumulates, the windows it completes and their ring slots"""
    res = check(["walk %d %d 500" % (seed, base) for seed in range(1, 9)])
    for r in res:
        assert r["ok"] == 1, r
    assert sum(r["records"] for r in res) > 500 and sum(r["resets"] for r in res) > 100 and sum(r["empty"] for r in res) > 20


# ---- signals: [frames, 2] float32
def tone(n, hz=997.0, left=1.0, right=0.0, phase=0.0):
    s = np.sin(2 * np.pi * hz / 48000.0 * np.arange(n) + phase)
    return np.stack([left * s, right * s], axis=1).astype(np.float32)


def noise_on_dc(n, seed=5):
    rng = np.random.default_rng(seed)
    return (0.25 + 0.2 * rng.standard_normal((n, 2))).astype(np.float32)


def programme(n, seed=7):
    """a stereo-like programme: a tone in both ears, another in the left, noise that differs between them"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 48000.0
    mid, side = 0.4 * np.sin(2 * np.pi * 440.0 * t), 0.15 * np.sin(2 * np.pi * 1700.0 * t + 0.4)
    x = np.stack([mid + side, mid - side], axis=1) + 0.02 * rng.standard_normal((n, 2))
    return x.astype(np.float32)


def programme_then_silence():
    return np.concatenate([programme(3 * W), np.zeros((7 * W, 2), np.float32)])


def distance(r32, m64, tail_from=10):
    """the largest distance of ms and kms from float64 over the windows, relative to the window's own value; from window `tail_from` on -- the digital
    silence behind a programme -- relative to the signal's largest window.  (What those windows hold is the decay of the states the programme left in
    the high-pass, a double pole at 38 Hz, 0.005 from the unit circle: the f32 error of those states is 1e-7 of the PROGRAMME, amplified by the
    pole's 1 / 0.005^2.  Measured here: the first window of silence lies 31 dB below the programme and 1.1e-3 of its own value from float64, which
    is 5.5e-7 of the programme's.)"""
    worst = 0.0
    for name in ("ms_l", "ms_r", "kms_l", "kms_r"):
        a, b = r32[name][0].astype(np.float64), m64[name][0]
        den = b.copy()
        den[tail_from:] = b.max()
        worst = max(worst, float(np.max(np.abs(a - b) / den)))
    return worst


def test_restatement_against_float64():
    """a 997 Hz tone at full scale, noise on a DC offset, a programme followed by 0.7 s of digital silence in which the filter states walk down through
    the subnormals: the restatement's ms and kms against float64, and its peaks and window numbers exactly"""
    for name, x, tail in (("tone", tone(10 * W, left=1.0, right=0.5), 10), ("noise on DC", noise_on_dc(10 * W), 10), ("programme, silence", programme_then_silence(), 3)):
        r32, w0 = lm.restate_windows(x[None])
        m64, _ = lm.model_f64(x[None])
        assert w0 == 0 and r32.shape == (1, 10) and list(r32["index"][0]) == list(range(10))
        for ear in "lr":
            assert np.array_equal(r32["peak_" + ear][0].astype(np.float64), m64["peak_" + ear][0])
        rel = distance(r32, m64, tail)
        cross = float(np.max(np.abs(r32["cross"][0] - m64["cross"][0])) / max(np.max(np.abs(m64["cross"][0])), 1e-30))
        print("restatement against float64, %s: ms / kms %.2e relative, cross %.2e of its magnitude" % (name, rel, cross))
        assert rel <= RESTATEMENT_REL and cross <= RESTATEMENT_REL
    # (the last signal: its K-weighted power in the windows of silence, where the states leave the normal range: f32 beside float64)
    print("kms_l of the programme's tail: %s\n                     float64: %s" % (r32["kms_l"][0][3:], m64["kms_l"][0][3:]))
    assert np.all(r32["ms_l"][0][3:] == 0) and r32["kms_l"][0][3] > 0 and np.all(r32["kms_l"][0][7:] < 1e-30)


def test_calibration_of_the_model():
    """BS.1770-4: a 997 Hz sine at 0 dBFS in one ear reads -3.01 LKFS"""
    m64, _ = lm.model_f64(tone(20 * W)[None])
    assert abs(float(lm.lufs(m64["kms_l"][0][10:].mean() + m64["kms_r"][0][10:].mean())) + 3.01) < 0.01


# ---- the checker
CUTS = [1365, 1366, 2731, 4799, 4800, 4801, 9637, 15000, 21605]


def feed_in_calls(machine, x, cuts):
    recs, pos = [], 0
    for c in list(cuts) + [x.shape[0]]:
        recs.append(machine.feed(x[pos:c]))
        pos = c
    return np.concatenate(recs)


@pytest.fixture(scope="module")
def prog():
    return programme(5 * W + 777)


def test_checker_accepts_the_restatement_however_the_stream_is_cut(prog):
    whole = feed_in_calls(lm.Machine(), prog, [])
    cut = feed_in_calls(lm.Machine(), prog, CUTS)
    assert whole.tobytes() == cut.tobytes() and list(whole["index"]) == [0, 1, 2, 3, 4]
    assert lm.check_records(cut, prog, expect_index=range(5), verbose=True) <= RESTATEMENT_REL


@pytest.mark.parametrize("fault", ["drop", "swap", "late", "zero", "w9600"])
def test_checker_catches_seeded_faults(prog, fault):
    """a frame dropped at a call boundary, the ears swapped, a window one frame late, filter states zeroed at a call boundary, 4800 written as 9600"""
    recs = feed_in_calls(lm.Machine(fault), prog, CUTS)
    assert recs.size >= 4
    with pytest.raises(AssertionError):
        lm.check_records(recs, prog)


def test_switching_in_the_restatement(prog):
    """on in mid-window starts the filters there and the sums at the next boundary; off drops the window in progress and the states"""
    x = np.concatenate([prog, prog])[:10 * W]
    M = lm.Machine()
    spans = [(0, 2500, False), (2500, 10000, True), (10000, 10000, False), (10000, 15000, True), (15000, 23000, False), (23000, 23001, True), (23001, 48000, True)]
    recs = np.concatenate([M.feed(x[a:b], on) for a, b, on in spans])
    assert list(recs["index"]) == [1, 2, 5, 6, 7, 8, 9]      # (the empty piece with the meter off covers no frame: window 2 stands)
    lm.check_records(recs[:2], x, start=2500)
    lm.check_records(recs[2:], x, start=23000)
    with pytest.raises(AssertionError):
        lm.check_records(recs[2:], x, start=0)               # (the filters did start again at frame 23 000)


# ---- fmx_audio_loudness
def lib_loudness(m, recs):
    return m.loudness(recs)


def compare_with_numpy(m, recs):
    got, want = lib_loudness(m, recs), lm.loudness_numpy(recs)
    for k, v in want.items():
        if isinstance(v, int) or np.isinf(v):
            assert got[k] == v, (k, got[k], v)
        else:
            assert abs(got[k] - v) <= 1e-9 * max(1.0, abs(v)), (k, got[k], v)
    return got


def db(x):
    return 10.0 ** (x / 20.0)


def test_loudness_one_ear_full_scale(fmx_amd):
    g = compare_with_numpy(fmx_amd.fmx, lm.records_f64(tone(50 * W)))
    assert abs(g["integrated_lufs"] + 3.01) <= 0.01 and abs(g["momentary_lufs"] + 3.01) <= 0.01 and abs(g["short_term_lufs"] + 3.01) <= 0.01
    assert g["correlation"] == 0.0 and abs(g["peak_dbfs_l"]) < 1e-3 and g["peak_dbfs_r"] == -np.inf
    assert g["blocks_total"] == 47 and g["blocks_gated"] >= 45


def test_loudness_tech_3341_case_1(fmx_amd):
    """both ears in phase at 1 kHz, -23 dBFS: -23.0 +-0.1 integrated, momentary and short-term"""
    g = compare_with_numpy(fmx_amd.fmx, lm.records_f64(tone(200 * W, hz=1000.0, left=db(-23), right=db(-23))))
    for k in ("integrated_lufs", "momentary_lufs", "short_term_lufs"):
        assert abs(g[k] + 23.0) <= 0.1, (k, g[k])
    assert g["correlation"] > 0.999999


def test_loudness_tech_3341_case_3_relative_gate(fmx_amd):
    """-36 / -23 / -36 dBFS for 10 / 60 / 10 s: the relative gate removes the quiet parts, -23.0 +-0.1"""
    amp = np.concatenate([np.full(100 * W, db(-36)), np.full(600 * W, db(-23)), np.full(100 * W, db(-36))])
    x = tone(800 * W, hz=1000.0, left=1.0, right=1.0) * amp[:, None].astype(np.float32)
    g = compare_with_numpy(fmx_amd.fmx, lm.records_f64(x))
    assert abs(g["integrated_lufs"] + 23.0) <= 0.1 and g["blocks_total"] == 797 and 590 <= g["blocks_gated"] <= 606
    assert abs(g["momentary_lufs"] + 36.0) <= 0.1


def test_loudness_correlation_silence_gaps_and_too_few(fmx_amd):
    m = fmx_amd.fmx
    assert abs(compare_with_numpy(m, lm.records_f64(tone(40 * W, left=0.5, right=-0.5)))["correlation"] + 1.0) < 1e-6      # R = -L
    assert compare_with_numpy(m, lm.records_f64(tone(40 * W, left=0.5, right=0.0)))["correlation"] == 0.0                  # one dead ear
    g = compare_with_numpy(m, lm.records_f64(np.zeros((40 * W, 2), np.float32)))                                          # digital silence
    assert g["integrated_lufs"] == -np.inf and g["momentary_lufs"] == -np.inf and g["short_term_lufs"] == -np.inf
    assert g["blocks_total"] == 37 and g["blocks_gated"] == 0 and g["peak_dbfs_l"] == -np.inf and g["correlation"] == 0.0
    recs = lm.records_f64(programme(40 * W))
    assert compare_with_numpy(m, recs)["blocks_total"] == 37
    gap = np.concatenate([recs[:17], recs[18:]])                     # a gap in `index` breaks the blocks
    assert compare_with_numpy(m, gap)["blocks_total"] == 14 + 19
    g = compare_with_numpy(m, np.concatenate([recs[:30], recs[31:]]))
    assert g["short_term_lufs"] == -np.inf and np.isfinite(g["momentary_lufs"])       # (only 9 consecutive records at the end)
    g = compare_with_numpy(m, recs[:3])                              # too few
    assert g["integrated_lufs"] == g["momentary_lufs"] == g["short_term_lufs"] == -np.inf and g["blocks_total"] == 0
    g = compare_with_numpy(m, recs[:29])
    assert g["short_term_lufs"] == -np.inf and np.isfinite(g["momentary_lufs"]) and np.isfinite(g["integrated_lufs"])
    g = compare_with_numpy(m, recs[:0])
    assert g["integrated_lufs"] == -np.inf and g["blocks_total"] == 0 and g["correlation"] == 0.0


def test_loudness_and_entry_points_refuse_bad_arguments(fmx_amd):
    m = fmx_amd.fmx
    L = m.load_library()
    out = m.FmxLoudness()
    recs = lm.records_f64(programme(5 * W))
    assert L.fmx_audio_loudness(recs.ctypes.data, 5, None) == m.FMX_E_INVALID
    assert L.fmx_audio_loudness(None, 5, C.byref(out)) == m.FMX_E_INVALID
    assert L.fmx_audio_loudness(recs.ctypes.data, -1, C.byref(out)) == m.FMX_E_INVALID
    assert L.fmx_audio_loudness(None, 0, C.byref(out)) == m.FMX_OK
    n = (C.c_int32 * 1)()
    assert L.fmx_audio_meter_enable(None, 0, 1) == m.FMX_E_INVALID
    assert L.fmx_audio_records(None, 0, 1, None, 0, n) == m.FMX_E_INVALID
    assert lm.AUDIO_DTYPE == m.AUDIO_DTYPE and m.AUDIO_WINDOW == W

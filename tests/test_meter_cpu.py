"""The modulation meter on the CPU: the integers of sdr-j-fm_amd/csrc/fmx_meter.h (tests/meter_check.cpp) against a counter stepped
sample by sample; the float64 model, the f32 restatement and the checker of tests/meter_model.py -- the checker against seeded faults, the model on the
oracle's taps against what the signal generator sent --; and the host-only unit conversion fmx_mod_hz_per_unit."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import meter_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HZ = 47261.5                  # Hz per unit of the demodulator output at fmRate 192 000 (fmx_mod_hz_per_unit)
# the oracle's peak for a mono 1 kHz tone at +-37 500 Hz, measured on 0.5 s with the input filter at 165 kHz and every other setting at the constructor's:
# 37 662 Hz in window 1, rising to 38 316 Hz in window 9 -- 816.3 Hz from the nominal value at the most (the chain's own doing: the RF DC removal in front
# of the filters settles over seconds and takes the carrier's residue with it).  The tests allow twice that distance.
TONE_PEAK_TOL_HZ = 2 * 816.3


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("meter") / "meter_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "meter_check.cpp")])

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [json.loads(line) for line in out]
    return run


def test_constants_lanes_steps_divisions(check):
    assert check(["const"])[0] == {"window": 9600, "lanes": 64, "steps": 150, "ring": 64, "quant": 6}
    idx = [0, 1, 63, 64, 65, 4799, 9535, 9536, 9599]
    for i, g in zip(idx, check(["map %d" % i for i in idx])):
        assert (g["lane"], g["step"]) == (i % 64, i // 64)
    vals = [0.0, 1.0, -3.25, 9600.0, 4800.0, 1234.5678, 1e-30, -7.1e5]
    for v, g in zip(vals, check(["finish %d" % struct.unpack("<I", struct.pack("<f", v))[0] for v in vals])):
        f = np.float32(v)
        assert g["mean"] == int(np.float32(f / np.float32(9600.0)).view(np.uint32)) and g["pilot"] == int(np.float32(f / np.float32(4800.0)).view(np.uint32))


@pytest.mark.parametrize("base", [0, 1, 9599, 9600, 12345678, 2 ** 32 - 20000, 2 ** 32 + 12345, 2 ** 40 + 9600 * 7 - 3])
def test_meter_produce_against_a_counter(check, base):
    """random cuts and random switch times: the first sample a piece accumulates, the windows it completes and their ring slots"""
    res = check(["walk %d %d 600" % (seed, base) for seed in range(1, 9)])
    for r in res:
        assert r["ok"] == 1, r
    assert sum(r["records"] for r in res) > 500      # (the walks do complete windows, beyond the ring's 64)


# ---- the checker
def synthetic(n, seed=3):
    """a stereo-like demodulator output in its units: a 1 kHz tone, a pilot of 0.15 at the phase the PLL reports plus a small error, noise"""
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.float64)
    ph = (2 * np.pi * 19000.0 / 192000.0 * j + 0.3) % (2 * np.pi)
    d = 0.6 * np.sin(2 * np.pi * 1000.0 / 192000.0 * j) + 0.15 * np.sin(ph + 0.02) + 0.01 * rng.standard_normal(n)
    return d.astype(np.float32), ph.astype(np.float32)


def feed_in_calls(machine, d, phi, cuts):
    recs, pos = [], 0
    for c in list(cuts) + [d.size]:
        recs += machine.feed(d[pos:c], phi[pos:c])
        pos = c
    return mm.as_records(recs)


CUTS = [1365, 1366, 2731, 9599, 9600, 9601, 19237, 30000, 43210]


def test_checker_accepts_the_restatement_however_the_stream_is_cut():
    d, phi = synthetic(5 * mm.WINDOW + 777)
    whole = feed_in_calls(mm.Restatement(), d, phi, [])
    cut = feed_in_calls(mm.Restatement(), d, phi, CUTS)
    assert whole.tobytes() == cut.tobytes() and list(whole["index"]) == [0, 1, 2, 3, 4]
    mm.check_records(cut, d, phi, expect_index=range(5), k_ulp=0.0)      # (numpy's own sine on both sides: the restatement's level alone)
    # the pilot the model finds is the one that was put in: 0.15 at 0.02 rad
    m = mm.model_f64(d, phi, [2])
    assert abs(np.hypot(m["pilot_i"][0], m["pilot_q"][0]) - 0.15) < 1e-3 and abs(np.arctan2(m["pilot_q"][0], m["pilot_i"][0]) - 0.02) < 2e-3


@pytest.mark.parametrize("fault", ["drop", "swap", "late", "pilot9600"])
def test_checker_catches_seeded_faults(fault):
    """a sample dropped at a call boundary, two lanes swapped, a window one sample late, 4800 written as 9600"""
    d, phi = synthetic(5 * mm.WINDOW + 777)
    recs = feed_in_calls(mm.Restatement(fault), d, phi, CUTS)
    assert recs.size >= 4
    with pytest.raises(AssertionError):
        mm.check_records(recs, d, phi, k_ulp=mm.SINCOS_ULP)


def test_switching_in_the_restatement():
    """on in mid-window starts at the next boundary; off drops the window in progress"""
    d, phi = synthetic(6 * mm.WINDOW)
    M = mm.Restatement()
    spans = [(0, 5000, False), (5000, 20000, True), (20000, 30000, False), (30000, 57600, True)]
    recs = []
    for a, b, on in spans:
        recs += M.feed(d[a:b], phi[a:b], on)
    recs = mm.as_records(recs)
    assert list(recs["index"]) == [1, 4, 5]
    mm.check_records(recs, d, phi, k_ulp=0.0)


# ---- the model on the oracle's taps
def oracle_taps(ol, iq, **cfg):
    ch = ol.OracleChain(taps=[ol.TAP_DEMOD, ol.TAP_PILOT], tap_seconds=(len(iq) / 2304000.0) + 1.0, **cfg)
    ch.process(np.concatenate([iq, np.zeros((16384, 2), np.float32)]))     # (the oracle works in 16384-sample blocks: flush the last one)
    n = len(iq) // 12
    return ch.tap(ol.TAP_DEMOD)[:n].copy(), ch.tap(ol.TAP_PILOT)[:n].copy()


def test_model_on_the_oracles_stereo_signal(ol):
    """1 s of the default stereo signal (pilot 7 500 Hz, peak deviation 75 000 x 0.55), input filter at 165 kHz"""
    d, phi = oracle_taps(ol, ol.synth_iq(2304000), inputFilterBw=165000)
    windows = list(range(20))
    r32, m64 = mm.restate_windows(d, phi, windows), mm.model_f64(d, phi, windows)
    for name in mm.FIELDS_EXACT[:2]:
        assert np.array_equal(r32[name].astype(np.float64), m64[name])
    rel_s2 = np.max(np.abs(r32["mean_square"] - m64["mean_square"]) / m64["mean_square"])
    pil = max(np.max(np.abs(r32[n] - m64[n])) for n in mm.FIELDS_PILOT)
    pilot_hz = np.hypot(m64["pilot_i"], m64["pilot_q"]) * HZ
    peak_hz = max(m64["peak_pos"][6:].max(), -m64["peak_neg"][6:].min()) * HZ      # (window 0 holds the filters' start-up)
    print("restatement against float64: s2 %.2e relative, pilot %.2e; pilot %.1f Hz, |I| / |Q| %.1e, peak %.1f Hz"
          % (rel_s2, pil, pilot_hz[-1], np.max(np.abs(m64["pilot_i"][6:]) / np.abs(m64["pilot_q"][6:])), peak_hz))
    assert rel_s2 < 2e-7 and pil < 1e-7                                   # (f32 sums of 9600 terms in 64 lanes: a few ulp)
    assert np.all(np.abs(pilot_hz[6:] - 7500.0) <= 750.0)                 # the chain's own response at 19 kHz: within 10 % of the nominal value
    assert np.all(np.abs(m64["pilot_i"][6:]) <= 0.01 * np.abs(m64["pilot_q"][6:]))      # the PLL's phase is the pilot's cosine
    assert abs(peak_hz - 41100.0) < 500.0


def test_model_on_a_mono_tone(ol):
    """a mono 1 kHz tone at +-37 500 Hz: the peak the meter reports is the deviation that was sent"""
    iq = ol.synth_iq(1152000, stereo=0, leftHz=1000.0, rightHz=1000.0, leftAmp=1.0, rightAmp=1.0, deviationHz=37500.0 / 0.9)
    d, phi = oracle_taps(ol, iq, inputFilterBw=165000)
    m = mm.model_f64(d, phi, list(range(1, 10)))
    pos, neg = m["peak_pos"] * HZ, -m["peak_neg"] * HZ
    print("mono tone: peaks %.1f .. %.1f / %.1f .. %.1f Hz" % (pos.min(), pos.max(), neg.min(), neg.max()))
    assert np.all(np.abs(pos - 37500.0) <= TONE_PEAK_TOL_HZ) and np.all(np.abs(neg - 37500.0) <= TONE_PEAK_TOL_HZ)
    assert np.all(np.abs(np.sqrt(2.0 * m["mean_square"]) * HZ - 37500.0) <= TONE_PEAK_TOL_HZ)      # a sine's mean square is half its peak's square


# ---- units
def test_hz_per_unit_and_refusals(fmx_amd):
    m = fmx_amd.fmx
    F_G, D_F = np.float32(0.65 * 192000 / 2), np.float32(0.95 * 192000 / 2)
    B_FM = np.float32(2) * np.float32(D_F + F_G)
    K_FM = np.float32(float(np.float32(2) * B_FM) * np.pi / float(F_G))
    want = float(K_FM) / 20.0 * 192000.0 / (2.0 * np.pi)
    for dec in (2, 3, 4):
        hz = m.mod_hz_per_unit(dec, 192000)
        assert hz == want and abs(hz - 47261.5) < 0.05, (dec, hz)
    for dec in (1, 5, 6):
        with pytest.raises(m.FmxError) as e:
            m.mod_hz_per_unit(dec)
        assert e.value.code == m.FMX_E_UNSUPPORTED and len(str(e.value)) > 40
    for dec in (0, 7):
        with pytest.raises(m.FmxError) as e:
            m.mod_hz_per_unit(dec)
        assert e.value.code == m.FMX_E_INVALID
    L = m.load_library()
    assert L.fmx_mod_hz_per_unit(3, 192000, None) == m.FMX_E_INVALID
    n = (C.c_int32 * 1)()
    assert L.fmx_mod_meter_enable(None, 0, 1) == m.FMX_E_INVALID
    assert L.fmx_mod_records(None, 0, 1, None, 0, n) == m.FMX_E_INVALID

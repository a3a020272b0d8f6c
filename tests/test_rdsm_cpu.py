"""The RDS meter on the CPU: the integers of sdr-j-fm_amd/csrc/fmx_rdsm.h (tests/rdsm_check.cpp) against a walk sample by sample; the
float64 model, the f32 restatement, the machine and the checker of tests/rdsm_model.py -- the machine's independence of the cut, the checker against
seeded faults, the restatement against float64 on the oracle's RDS_IQ tap --; the figures of figures () on that tap against what the signal generator
sent; and the host-only fmx_rds_meter_figures against figures ().  Every bound is twice what was measured here (rdsm_model.py)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rdsm_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = rm.WINDOW


# ---- the integers
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rdsm") / "rdsm_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "rdsm_check.cpp")])

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [json.loads(line) for line in out]
    return run


def test_constants(check):
    assert check(["const"])[0] == {"window": 2560, "lanes": 64, "steps": 40, "ring": 64, "ring24": 8192, "quant": 6, "order": [0, 1, 2, 3, 4, 5],
                                   "lane_2559": 63, "step_2559": 39, "lane_64": 0, "step_64": 1, "window_of_2560": 1, "window_of_2559": 0,
                                   "mean_2560": 1.0, "holds_8192": 1, "holds_8193": 0}
    assert (rm.WINDOW, rm.LANES, rm.STEPS, rm.RING) == (2560, 64, 40, 64)


def script(seed, n_pieces):
    """pieces (meter, decoder, n) with everything the rule distinguishes: pieces of 0 samples, of one, around a step and around a window, 4000; the meter
    and the decoder switched at any of them"""
    rng = np.random.default_rng(seed)
    sizes = [0, 0, 1, 1, 63, 64, 65, 640, 2559, 2560, 2561, 4000]
    meter, dec, out = 1, 1, []
    for _ in range(n_pieces):
        if rng.random() < 0.05:
            meter ^= 1
        if rng.random() < 0.05:
            dec ^= 1
        out.append((meter, dec, int(sizes[rng.integers(len(sizes))])))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_piece_against_a_walk_sample_by_sample(check, seed):
    """rdsm::piece stepped piece by piece against the brute-force walk of rdsm_check.cpp and against rm.expected_windows: switching on and off in
    mid-window, pieces of 0 samples, a decoder pause, more than 64 records (the slots modulo 64)"""
    pieces = script(seed, 1200)
    res = check(["reset"] + ["piece %d %d %d" % p for p in pieces])[1:]
    windows, m, n_switched = [], 0, 0
    for (meter, dec, n), r in zip(pieces, res):
        assert r["m0"] == m and r["m1"] == m + (n if dec else 0), r
        m = r["m1"]
        assert r["nwin"] == len(r["b_w"]) and r["produced"] == r["b_produced"], r
        assert (r["first"] if r["job"] else -1) == r["b_first"], r
        if r["nwin"]:
            assert r["b_w"] == list(range(r["w0"], r["w0"] + r["nwin"])) and r["end0"] == (r["w0"] + 1) * W, r
            assert r["b_slots"] == [(r["slot0"] + k) % 64 for k in range(r["nwin"])], r
        if not (meter and dec):
            assert r["job"] == 0 and r["nwin"] == 0
            n_switched += 1
        windows += r["b_w"]
    assert len(windows) > 64 and n_switched > 20
    assert windows == rm.expected_windows([(n if dec else 0, meter) for meter, dec, n in pieces])
    assert windows != list(range(windows[0], windows[0] + len(windows)))          # (some window was dropped)


def test_piece_spans_a_decoder_pause_and_ignores_empty_pieces(check):
    """a window spans pieces in which the decoder is off, whatever the meter's switch there, and pieces of no samples with the meter off; a piece WITH
    samples and the meter off drops it"""
    r = check(["reset", "piece 1 1 1000", "piece 0 0 500", "piece 1 0 500", "piece 0 1 0", "piece 1 1 1560", "piece 1 1 1000", "piece 0 1 1", "piece 1 1 1559",
               "piece 1 1 2560"])[1:]
    assert r[4]["b_w"] == [0] and r[4]["nwin"] == 1 and r[4]["m0"] == 1000
    assert r[7]["nwin"] == 0 and r[7]["job"] == 0 and r[8]["nwin"] == 1 and r[8]["w0"] == 2 and r[8]["slot0"] == 1


# ---- the machine and the checker
def synthetic(n, seed=5):
    """a BPSK-like baseband on an axis at 59 degrees, with an offset and noise"""
    rng = np.random.default_rng(seed)
    m = np.arange(n, dtype=np.float64)
    s = np.sin(2 * np.pi * 1187.5 / 24000.0 * m) * np.sign(np.sin(2 * np.pi * 97.0 / 24000.0 * m))
    z = 0.08 * s * np.exp(1j * np.radians(59.0)) + (0.003 - 0.002j) + 0.004 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return rm.as_pairs(z.astype(np.complex64))


def feed_in_pieces(machine, z, lengths):
    recs, pos = [], 0
    for n in list(lengths) + [z.shape[0]]:
        recs += machine.feed(z[pos:pos + n])
        pos += n
        if pos >= z.shape[0]:
            break
    return rm.as_records(recs)


PIECES = [0, 1, 63, 64, 65, 2559, 2560, 2561, 4000]


def test_machine_does_not_depend_on_the_cut():
    """pieces of 0, 1, 63, 64, 65, 2559, 2560, 2561 and 4000 samples and the rest, against one piece; and both against the whole-window restatement"""
    z = synthetic(sum(PIECES) + 2 * W + 77)
    whole = feed_in_pieces(rm.Machine(), z, [])
    cut = feed_in_pieces(rm.Machine(), z, PIECES)
    nwin = z.shape[0] // W
    assert nwin >= 6 and whole.tobytes() == cut.tobytes() and list(whole["index"]) == list(range(nwin))
    rm.check_records(cut, z, expect_index=range(nwin))
    f = rm.figures(cut, {"gain": 1.0, "phase0_deg": 0.0, "path_57k": 1.0}, 1.0)
    assert abs(f["phase_deg"] - 59.0) < 0.5 and abs(f["carrier_hz"] - np.hypot(0.003, 0.002)) < 3e-4      # the figures find what was put in


@pytest.mark.parametrize("fault", ["drop", "swap", "late", "cross", "sign", "1280"])
def test_checker_catches_seeded_faults(fault):
    """a sample dropped at a piece boundary, two lanes swapped, a window one sample late, iq_mean with I and Q of different samples, the sign of q_mean,
    1280 written for 2560"""
    z = synthetic(3 * W + 777)
    recs = feed_in_pieces(rm.Machine(fault), z, [1365, 731, 2559, 2561])
    assert recs.size >= 2
    with pytest.raises(AssertionError):
        rm.check_records(recs, z)


def test_switching_in_the_machine():
    """on in mid-window starts at the next boundary; off drops the window in progress; a piece of no samples with the meter off drops nothing"""
    z = synthetic(6 * W)
    M = rm.Machine()
    recs, pieces = [], [(0, 1000, False), (1000, 2 * W, True), (2 * W, 2 * W, False), (2 * W, 3 * W + 5, True), (3 * W + 5, 3 * W + 9, False), (3 * W + 9, 6 * W, True)]
    for a, b, on in pieces:
        recs += M.feed(z[a:b], on)
    recs = rm.as_records(recs)
    assert list(recs["index"]) == [1, 2, 4, 5] == rm.expected_windows([(b - a, on) for a, b, on in pieces])
    rm.check_records(recs, z)


# ---- the oracle's RDS_IQ tap
def rds_iq(ol, iq, **cfg):
    ch = ol.OracleChain(taps=[ol.TAP_RDS_IQ], tap_seconds=(len(iq) / 2304000.0) + 1.0, inputFilterBw=165000, rdsMode=2, **cfg)
    ch.process(np.concatenate([iq, np.zeros((16384, 2), np.float32)]))     # (the oracle works in 16384-sample blocks: flush the last one)
    return ch.tap(ol.TAP_RDS_IQ)[:len(iq) // 96].copy()


@pytest.fixture(scope="module")
def oracle_cal(ol):
    """cal () on the oracle's own kernels: the 57 kHz band-pass, rdsDecimator, and in front of the demodulator the two decimators (25 taps at 2 304 000,
    3 taps at 384 000: the real taps, the complex kernel is they times a constant) and the 251-tap input low-pass at 165 000 / 2"""
    L = ol.oracle()
    bp, dk = np.zeros(2 * 768, np.float32), np.zeros(22, np.float32)
    k1, k2, h = np.zeros(50, np.float32), np.zeros(6, np.float32), np.zeros(251, np.float32)
    L.fmo_bandpass_kernel(768, 57000 - 2400, 57000 + 2400, 192000, ol.fptr(bp))
    L.fmo_decim_kernel(11, 12000, 192000, ol.fptr(dk))
    L.fmo_decim_kernel(25, 96000, 2304000, ol.fptr(k1))
    L.fmo_decim_kernel(3, 96000, 384000, ol.fptr(k2))
    L.fmo_lowpass_kernel(251, 165000 // 2, 2304000, ol.fptr(h))
    return rm.cal(bp, dk, [(k1.reshape(-1, 2)[:, 0], 2304000.0), (k2.reshape(-1, 2)[:, 0], 384000.0), (h, 2304000.0)])


def test_calibration_from_the_designed_taps(oracle_cal):
    """gain = 3 x 0.5000 x 1.9459 = 2.9188, phase0 = the argument of the decimator's complex DC gain, 59.08 degrees (the band-pass adds nothing: its delay
    of 384 samples is whole periods of 57 kHz); the discriminator's own response at 57 kHz is 0.861, the path with the 165 kHz input filter 0.6727"""
    k = oracle_cal
    print("cal: %s" % k)
    assert abs(k["gain"] - 2.9188) < 5e-5 and abs(k["phase0_deg"] - 59.08) < 0.01
    x = np.pi * 57000.0 / 192000.0
    assert abs(np.sin(x) / x - 0.861) < 5e-4 and abs(k["path_57k"] - 0.6727) < 5e-5
    assert abs(rm.hz_per_unit() - 47261.54) < 0.01


@pytest.fixture(scope="module")
def runs(ol, oracle_cal):
    """signal () through the oracle chain, once per case: (figures of windows FIRST_WINDOW and later, the waveform's rms, the tap)"""
    hz, cache = rm.hz_per_unit(), {}

    def get(**kw):
        key = tuple(sorted(kw.items()))
        if key not in cache:
            iq, rms = rm.signal(rm.SECONDS, **kw)
            z = rds_iq(ol, iq)
            windows = list(range(rm.FIRST_WINDOW, z.shape[0] // W))
            assert len(windows) >= 12
            cache[key] = (rm.figures(rm.records_of(rm.restate_windows(z, windows), windows), oracle_cal, hz), rms, z)
        return cache[key]
    return get


def test_restatement_against_float64(runs):
    """2 s of the clean signal, RDS mode 2, windows 6 and later: the relative distance per field (p_max to itself, the second moments to ii_mean + qq_mean,
    the first to the rms of z).  Measured 5.59e-8 / 7.37e-8 / 3.15e-8 / 3.75e-8 / 4.74e-9 / 2.28e-9; the bounds are twice that"""
    z = runs()[2]
    windows = list(range(rm.FIRST_WINDOW, z.shape[0] // W))
    r32, m64 = rm.restate_windows(z, windows), rm.model_f64(z, windows)
    pw = m64["ii_mean"] + m64["qq_mean"]
    den = {"p_max": m64["p_max"], "ii_mean": pw, "qq_mean": pw, "iq_mean": pw, "i_mean": np.sqrt(pw), "q_mean": np.sqrt(pw)}
    err = {k: float(np.max(np.abs(r32[k] - m64[k]) / den[k])) for k in rm.FIELDS}
    print("restatement against float64: " + ", ".join("%s %.3e" % (k, err[k]) for k in rm.FIELDS))
    for k in rm.FIELDS:
        assert err[k] <= rm.RESTATE_REL[k], (k, err[k])


@pytest.mark.parametrize("dev", [1000.0, 2250.0, 7500.0])
def test_injection_against_what_was_sent(runs, dev):
    """deviations of 1000, 2250 and 7500 Hz without a programme: injection_peak_hz against the sent peak, injection_rms_hz against the sent rms.
    Measured: peak +0.0203 / +0.0209 / +0.0220, rms +0.0181 / +0.0181 / +0.0177 relative"""
    f, rms, _ = runs(rds_hz=dev)
    print("%.0f Hz: peak %+.4f, rms %+.4f relative (the waveform's rms %.4f); %s" % (dev, f["injection_peak_hz"] / dev - 1.0, f["injection_rms_hz"] / (dev * rms) - 1.0, rms, f))
    assert abs(rms - 0.693) < 0.002
    assert abs(f["injection_peak_hz"] / dev - 1.0) <= rm.INJECTION_PEAK_REL
    assert abs(f["injection_rms_hz"] / (dev * rms) - 1.0) <= rm.INJECTION_RMS_REL


def test_injection_under_programme(runs):
    """2250 Hz with config 2's programme (two 0.5-FS tones): the residual after correction.  Measured: injection_rms_hz 0.9240 of the sent rms (a loss of
    0.0760: the programme moves the sidebands across the second decimator's slope), injection_peak_hz 1.0483 of the sent peak, axis_db 20.24 (36 without)"""
    f, rms, _ = runs(programme=True)
    loss = 1.0 - f["injection_rms_hz"] / (2250.0 * rms)
    print("programme: rms loss %.4f, peak %+.4f relative, axis_db %.2f; %s" % (loss, f["injection_peak_hz"] / 2250.0 - 1.0, f["axis_db"], f))
    assert 0.0 < loss <= 2 * rm.PROGRAMME_LOSS
    assert abs(f["injection_peak_hz"] / 2250.0 - 1.0) <= rm.PROGRAMME_PEAK_REL
    assert f["axis_db"] < runs()[0]["axis_db"]


@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_phase_sin_against_cos(runs, sigma):
    """the sub-carrier on sin (3 p) of the pilot sin (p) -- its third harmonic -- reads 0 degrees, on cos (3 p) 90.  Measured 0.276 and 90.277 clean;
    their difference 90 within 0.0004 clean and 0.246 at noise sigma 0.05"""
    kw = {"sigma": sigma} if sigma else {}
    s, c = runs(on="sin", **kw)[0]["phase_deg"], runs(**kw)[0]["phase_deg"]
    print("sigma %.2f: sin %.4f, cos %.4f, difference %.4f" % (sigma, s, c, c - s))
    if sigma == 0.0:
        assert abs(s) <= rm.PHASE_TOL_DEG and abs(c - 90.0) <= rm.PHASE_TOL_DEG
    assert abs(c - s - 90.0) <= rm.PHASE_DIFF_TOL_DEG[sigma]


def test_carrier_of_an_unmodulated_component(runs):
    """an unmodulated 57 kHz component of 1000 Hz beside the 2250 Hz sub-carrier: carrier_hz 1020.04 (6.5 without it), injection_rms_hz unchanged"""
    f, rms, _ = runs(carrier_hz=1000.0)
    print("carrier: %s; without: %.2f Hz" % (f, runs()[0]["carrier_hz"]))
    assert abs(f["carrier_hz"] / 1000.0 - 1.0) <= rm.CARRIER_REL
    assert runs()[0]["carrier_hz"] < 0.05 * 1000.0
    assert abs(f["injection_rms_hz"] / runs()[0]["injection_rms_hz"] - 1.0) < 1e-3


def test_axis_falls_with_noise(runs):
    """axis_db over three noise levels: 35.90 / 20.51 / 12.87 dB -- monotonically down; injection_rms_hz stays (the off-axis power is booked as noise)"""
    f = [runs(**({"sigma": s} if s else {}))[0] for s in rm.NOISE_SIGMAS]
    print("axis_db %s, injection_rms_hz %s" % ([round(x["axis_db"], 2) for x in f], [round(x["injection_rms_hz"], 1) for x in f]))
    assert f[0]["axis_db"] > f[1]["axis_db"] > f[2]["axis_db"] > 0.0
    assert f[0]["axis_db"] >= rm.AXIS_CLEAN_DB - 10.0 * np.log10(2.0)
    assert all(abs(x["injection_rms_hz"] / f[0]["injection_rms_hz"] - 1.0) < 0.01 for x in f)


def test_no_rds_on_the_air(runs):
    """pilot alone: injection_rms_hz 0.347 Hz, injection_peak_hz 6.87 Hz -- below twice that"""
    f = runs(rds_hz=0.0)[0]
    print("no RDS: %s" % f)
    assert f["injection_rms_hz"] <= rm.NO_RDS_RMS_FLOOR_HZ and f["injection_peak_hz"] <= rm.NO_RDS_PEAK_FLOOR_HZ


# ---- the library
def close(a, b):
    return a == b or (np.isfinite(a) and np.isfinite(b) and abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1e-300))


NAMES = ("injection_rms_hz", "injection_peak_hz", "carrier_hz", "phase_deg", "axis_db")


def test_figures_against_the_model(fmx_amd):
    """fmx_rds_meter_figures (host only, no device) against figures () to 1e-12 relative: axes all round the circle (the fold into (-45, 135]), one record
    and many, two calibrations"""
    m = fmx_amd.fmx
    assert m.RDSM_DTYPE == rm.RDSM_DTYPE and m.RDSM_WINDOW == rm.WINDOW
    assert close(m.mod_hz_per_unit(3, 192000), rm.hz_per_unit())
    folded = []
    for seed, deg in enumerate((-80.0, -46.0, -44.0, 0.0, 59.0, 91.0, 134.0, 136.0, 179.0)):
        z = rm.as_pairs((synthetic(4 * W, seed=seed).view(np.complex64).ravel() * np.exp(1j * np.radians(deg - 59.0))).astype(np.complex64))
        recs = rm.records_of(rm.restate_windows(z, [0, 1, 2]), [0, 1, 2])
        for sub, k, hz in ((recs, {"gain": 2.9188, "phase0_deg": 59.08, "path_57k": 0.6727}, 47261.5), (recs[:1], {"gain": 1.0, "phase0_deg": 0.0, "path_57k": 1.0}, 1.0)):
            got, want = m.rds_meter_figures(sub, k, hz), rm.figures(sub, k, hz)
            assert got["windows"] == sub.size == want["windows"]
            for name in NAMES:
                assert close(got[name], want[name]), (deg, name, got[name], want[name])
            assert -45.0 < got["phase_deg"] <= 135.0
            folded.append(got["phase_deg"])
    assert min(folded) < -30.0 and max(folded) > 120.0


def test_figures_edge_cases(fmx_amd):
    """n = 0, null pointers, all-zero records, l- = 0 (a sub-carrier with nothing across it), and the argument checks of the handle's entry points"""
    m = fmx_amd.fmx
    L = m.load_library()
    out, k = m.FmxRdsFigures(), m.FmxRdsMeterCal(2.0, 10.0, 0.5)
    unit = {"gain": 2.0, "phase0_deg": 10.0, "path_57k": 0.5}
    zero = np.zeros(3, rm.RDSM_DTYPE)
    with pytest.raises(m.FmxError) as e:
        m.rds_meter_figures(zero[:0], unit, 1.0)
    assert e.value.code == m.FMX_E_INVALID
    assert L.fmx_rds_meter_figures(zero.ctypes.data, 0, C.byref(k), 1.0, C.byref(out)) == m.FMX_E_INVALID
    assert L.fmx_rds_meter_figures(None, 3, C.byref(k), 1.0, C.byref(out)) == m.FMX_E_INVALID
    assert L.fmx_rds_meter_figures(zero.ctypes.data, 3, None, 1.0, C.byref(out)) == m.FMX_E_INVALID
    assert L.fmx_rds_meter_figures(zero.ctypes.data, 3, C.byref(k), 1.0, None) == m.FMX_E_INVALID
    q = m.rds_meter_figures(zero, unit, 1.0)
    assert q == {"injection_rms_hz": 0.0, "injection_peak_hz": 0.0, "carrier_hz": 0.0, "phase_deg": 0.0, "axis_db": -np.inf, "windows": 3} == rm.figures(zero, unit, 1.0)
    line = zero.copy()                      # everything on the I axis: a = 0.25, b = c = 0 -- l+ = 0.25, l- = 0
    line["ii_mean"], line["p_max"] = 0.25, 1.0
    q, want = m.rds_meter_figures(line, unit, 3.0), rm.figures(line, unit, 3.0)
    assert q["axis_db"] == np.inf and close(q["phase_deg"], -10.0) and close(q["injection_rms_hz"], 0.5 * 3.0) and close(q["injection_peak_hz"], 3.0)
    assert all(close(q[name], want[name]) for name in NAMES)
    const = zero.copy()                     # an unmodulated component alone: the covariance is zero, the mean is not
    const["ii_mean"], const["i_mean"], const["p_max"] = 0.25, 0.5, 0.25
    q = m.rds_meter_figures(const, unit, 1.0)
    assert q["injection_rms_hz"] == 0.0 and close(q["carrier_hz"], 0.5) and q["axis_db"] == -np.inf and q["phase_deg"] == 0.0
    n = (C.c_int32 * 1)()
    assert L.fmx_rds_meter_enable(None, 0, 1) == m.FMX_E_INVALID
    assert L.fmx_rds_meter_records(None, 0, 1, None, 0, n) == m.FMX_E_INVALID
    assert L.fmx_rds_meter_cal(None, 0, C.byref(k)) == m.FMX_E_INVALID


def test_cpp_adapter_compiles(fmx_amd, tmp_path):
    """host/fm_processor_adapter.h's RDS-meter methods under -Wall -Werror, in the demo of tests/rdsm_demo; rdsMeterFigures needs no device and refuses no
    records (exit code 4 if it did not); without a device the demo then reports that the processor could not be created"""
    import test_gpu_rds_meter as gr
    exe = str(tmp_path / "rdsm_adapter_demo")
    gr.build_demo(fmx_amd, exe)
    np.zeros((16384, 2), np.float32).tofile(str(tmp_path / "iq.f32"))
    out = subprocess.run([exe, str(tmp_path / "iq.f32"), str(tmp_path / "records.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode in (0, 3), out.stdout

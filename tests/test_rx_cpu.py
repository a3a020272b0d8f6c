"""The reception meter on the CPU: the look-back bound of sdr-j-fm_amd/csrc/fmx_rx.h (tests/rx_check.cpp) against a ring stepped position
by position; the float64 model, the f32 restatement, the machine and the checker of tests/rx_model.py -- the restatement against float64, the machine's
independence of the cut, the checker against seeded faults --; the figures of quality () on the oracle's FM_IQ tap against what the signal generator sent;
and the host-only fmx_rx_quality_of against quality ().  Every bound is twice what was measured here (rx_model.py)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import rx_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = rm.WINDOW


# ---- the look-back bound
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rx") / "rx_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "rx_check.cpp")])

    def run(queries):
        out = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(queries)
        return [json.loads(line) for line in out]
    return run


def test_constants(check):
    assert check(["const"])[0] == {"ring": 64, "quant": 6, "window": 9600, "lanes": 64, "order": [0, 1, 2, 3, 4, 5]}


def test_ring_holds_against_a_stepped_ring(check):
    """around the bound, for every twin count, at stream positions in front of and far behind the filter latency"""
    q, n_yes, n_no = [], 0, 0
    for ring in (64, 1024, 16384):
        for twins in (1, 2, 12):
            for delay in (0, 1, 17, ring // 3):
                edge = ring - delay - 2 - 2 * twins          # the largest nj that holds
                for nj in (1, 2, edge - 1, edge, edge + 1, edge + 7, ring, 2 * ring + 3):
                    if nj >= 1:
                        for J0 in (0, 5, delay + 1, 2 ** 33 + 11):
                            q.append("holds %d %d %d %d %d" % (ring, delay, nj, twins, J0))
    for line, r in zip(q, check(q)):
        assert r["holds"] == r["stepped"], (line, r)
        n_yes += r["holds"]
        n_no += 1 - r["holds"]
    assert n_yes > 100 and n_no > 100


@pytest.mark.parametrize("decim", [12, 6, 1])
def test_fmx_creates_ring_always_holds(check, decim):
    """the ring as fmx_create sizes it -- the input filter's latency in fm samples, a call, 512 -- holds the look-back for the longest piece a handle takes"""
    q = []
    for max_block in (12, 16384, 230400, 1 << 22):
        per_call = max_block // decim + 2
        ring = 1
        while ring < (2 * 32768 - 251) // decim + 1 + per_call + 512:
            ring *= 2
        delay = -(-(2 * 32768 - 251) // decim)               # (the folded input filter's latency, rounded up; 0 without the filter)
        for d in (0, delay):
            q.append("holds %d %d %d %d %d" % (ring, d, per_call, 12 // decim, 10 * ring + 3))
    assert all(r == {"holds": 1, "stepped": 1} for r in check(q))


# ---- the machine and the checker
def synthetic(n, seed=5, cnr_db=25.0, offset_hz=4000.0):
    """an FM signal of amplitude 0.5 with an offset, in complex noise"""
    rng = np.random.default_rng(seed)
    j = np.arange(n, dtype=np.float64)
    ph = 2 * np.pi * offset_hz / 192000.0 * j + 30.0 * np.sin(2 * np.pi * 1000.0 / 192000.0 * j)
    s = 0.5 * 10.0 ** (-cnr_db / 20.0) / np.sqrt(2.0)
    x = 0.5 * np.exp(1j * ph) + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return rm.as_pairs(x.astype(np.complex64))


def feed_in_calls(machine, v, lengths):
    recs, pos = [], 0
    for n in list(lengths) + [v.shape[0]]:
        recs += machine.feed(v[pos:pos + n])
        pos += n
        if pos >= v.shape[0]:
            break
    return rm.as_records(recs)


CALLS = [1, 63, 64, 65, 9599, 19237]


def test_machine_does_not_depend_on_the_cut():
    """calls of 1, 63, 64, 65, 9599 and 19 237 fm samples and the rest, against one call; and both against the whole-window restatement"""
    v = synthetic(sum(CALLS) + 2 * W + 77)
    whole = feed_in_calls(rm.Machine(), v, [])
    cut = feed_in_calls(rm.Machine(), v, CALLS)
    nwin = v.shape[0] // W
    assert nwin >= 5 and whole.tobytes() == cut.tobytes() and list(whole["index"]) == list(range(nwin))
    rm.check_records(cut, v, expect_index=range(nwin))
    q = rm.quality(cut)
    assert abs(q["offset_hz"] - 4000.0) < 20.0 and abs(q["cnr_db"] - 25.0) < 0.5      # the figures find what was put in


@pytest.mark.parametrize("fault", ["drop", "swap", "late", "lag0", "sign", "4800"])
def test_checker_catches_seeded_faults(fault):
    """a sample dropped at a call boundary, two lanes swapped, a window one sample late, lag 0 for lag 1, the sign of r1_im, 4800 written for 9600"""
    v = synthetic(3 * W + 777)
    recs = feed_in_calls(rm.Machine(fault), v, [1365, 2731, 9599, 9601])
    assert recs.size >= 2
    with pytest.raises(AssertionError):
        rm.check_records(recs, v)


def test_switching_in_the_machine():
    """on in mid-window starts at the next boundary; off drops the window in progress; the sample in front of a window is the ring's whatever the switch"""
    v = synthetic(6 * W)
    M = rm.Machine()
    recs = []
    for a, b, on in [(0, 5000, False), (5000, 19200, True), (19200, 30000, False), (30000, 38400, True), (38400, 57600, True)]:
        recs += M.feed(v[a:b], on)
    recs = rm.as_records(recs)
    assert list(recs["index"]) == [1, 4, 5]
    rm.check_records(recs, v)


# ---- the oracle's FM_IQ tap
def fm_iq(ol, iq, **cfg):
    ch = ol.OracleChain(taps=[ol.TAP_FM_IQ], tap_seconds=(len(iq) / 2304000.0) + 1.0, inputFilterBw=165000, **cfg)
    ch.process(np.concatenate([iq, np.zeros((16384, 2), np.float32)]))     # (the oracle works in 16384-sample blocks: flush the last one)
    return ch.tap(ol.TAP_FM_IQ)[:len(iq) // 12].copy()


def figures(v, windows):
    return rm.quality(rm.records_of(rm.restate_windows(v, windows), windows))


def test_restatement_against_float64(ol):
    """0.5 s of the default stereo signal: measured 1.02e-7 (p_mean), 9.6e-8 (p2_mean), 1.16e-7 (|r1|) relative; the bounds are twice that"""
    v = fm_iq(ol, ol.synth_iq(1152000))
    windows = list(range(10))
    r32, m64 = rm.restate_windows(v, windows), rm.model_f64(v, windows)
    err = {k: float(np.max(np.abs(r32[k] - m64[k]) / m64[k])) for k in ("p_mean", "p2_mean")}
    err["r1"] = float(np.max(np.hypot(r32["r1_re"] - m64["r1_re"], r32["r1_im"] - m64["r1_im"]) / np.hypot(m64["r1_re"], m64["r1_im"])))
    print("restatement against float64: p_mean %.3e, p2_mean %.3e, |r1| %.3e relative" % (err["p_mean"], err["p2_mean"], err["r1"]))
    for k, e in err.items():
        assert e <= rm.RESTATE_REL[k], (k, e)
    # (the power of an f32 pair is itself rounded: the extremes are within an ulp of the model's, not equal)
    assert np.all(np.abs(r32["p_max"] - m64["p_max"]) <= 2.0 ** -23 * m64["p_max"]) and np.all(np.abs(r32["p_min"] - m64["p_min"]) <= 2.0 ** -23 * m64["p_max"])


def designed_gain(ol, f):
    """|H (f)| of the chain up to FM_IQ as designed: the two decimators' complex kernels (fir-filters.cpp:327-347, 25 taps at 2 304 000 and 3 taps at
    384 000) and the 251-tap input low-pass at 165 000 / 2"""
    L = ol.oracle()
    k1, k2, h = np.zeros(50, np.float32), np.zeros(6, np.float32), np.zeros(251, np.float32)
    L.fmo_decim_kernel(25, 96000, 2304000, ol.fptr(k1))
    L.fmo_decim_kernel(3, 96000, 384000, ol.fptr(k2))
    L.fmo_lowpass_kernel(251, 165000 // 2, 2304000, ol.fptr(h))
    resp = lambda k, fs: abs(np.sum(k * np.exp(-2j * np.pi * f / fs * np.arange(k.size))))
    return resp(k1.astype(np.float64).view(np.complex128), 2304000.0) * resp(k2.astype(np.float64).view(np.complex128), 384000.0) * resp(h.astype(np.float64), 2304000.0)


@pytest.mark.parametrize("offset,dc", [(10000.0, 1), (10000.0, 0), (-3700.0, 1), (-3700.0, 0)])
def test_unmodulated_carrier(ol, offset, dc):
    """amplitude 0.5 at +10 kHz and at -3.7 kHz, RF DC removal on and off: the offset that was set, the level the designed filters give.  Measured: 9.43e-3 Hz
    and 7.02e-6 dB at the most; the envelope is flat (am_depth below 5e-5, the C/N estimate above 57 dB)."""
    v = fm_iq(ol, ol.synth_iq(1152000, stereo=0, leftAmp=0.0, rightAmp=0.0, offsetHz=offset), dcRemove=dc)
    q = figures(v, list(range(1, 10)))
    want = 20.0 * np.log10(0.5 * designed_gain(ol, offset))
    print("carrier at %+.0f Hz, DC removal %d: offset_hz %+.3e from it, level_dbfs %.6f, %+.3e from the design; am_depth %.2e, cnr_db %.1f"
          % (offset, dc, q["offset_hz"] - offset, q["level_dbfs"], q["level_dbfs"] - want, q["am_depth"], q["cnr_db"]))
    assert abs(q["offset_hz"] - offset) <= rm.OFFSET_TOL_HZ
    assert abs(q["level_dbfs"] - want) <= rm.LEVEL_TOL_DB
    assert q["am_depth"] < 1e-3 and q["cnr_db"] > rm.CNR_CEILING_DB + 20.0


def test_clean_tone_floor_and_ceiling(ol):
    """the mono 1 kHz tone at +-37 500 Hz, clean: am_depth 0.0664 and cnr_db 25.49 are what the meter reads without noise or multipath -- the filtered FM
    signal's own envelope ripple: the floor of am_depth, the ceiling of cnr_db"""
    iq = ol.synth_iq(1152000, stereo=0, leftHz=1000.0, rightHz=1000.0, leftAmp=1.0, rightAmp=1.0, deviationHz=37500.0 / 0.9)
    q = figures(fm_iq(ol, iq), list(range(1, 10)))
    print("clean tone: am_depth %.4f, cnr_db %.2f, offset_hz %+.3f" % (q["am_depth"], q["cnr_db"], q["offset_hz"]))
    assert q["am_depth"] <= 2 * rm.AM_DEPTH_FLOOR and q["cnr_db"] >= rm.CNR_CEILING_DB - 10.0 * np.log10(2.0)
    assert rm.CNR_CEILING_DB < 40.0 + 6.0          # (why the truth test stops at 30 dB)


@pytest.fixture(scope="module")
def noise_runs(ol):
    """config 2's stereo signal alone, and per level the noise alone and their sum (the same seed: the same noise), each through the oracle"""
    n = 12 * 11 * W
    out = {"signal": fm_iq(ol, ol.synth_iq(n))}
    for level in rm.CNR_LEVELS_DB:
        s = rm.noise_sigma(level)
        out[level] = (fm_iq(ol, ol.synth_iq(n, noiseSeed=rm.NOISE_SEED, noiseSigma=s)), fm_iq(ol, ol.synth_iq(n, noiseSeed=rm.NOISE_SEED, noiseSigma=s, carrierAmp=0.0)))
    return out


@pytest.mark.parametrize("level", rm.CNR_LEVELS_DB)
def test_cnr_against_the_truth(noise_runs, level):
    """AWGN (the generator's xorshift64*, seed 0x5D2F1A7B) at 10 / 20 / 30 dB over the noise in 165 kHz.  The chain up to FM_IQ is linear but for the DC clamp:
    mean p of the sum is the sum of the two to 1 %, so the true C/N at the fm rate is mean p (signal) / mean p (noise).  Measured |cnr_db - truth| over windows
    1 .. 10 pooled: 0.158 / 1.342 / 6.615 dB -- the estimate sinks towards the clean signal's own 25.7 dB as the noise does.  40 dB is not a case: the ceiling
    lies below 40 + 6 dB (measured there: 15.66 dB off)."""
    windows = list(range(1, 11))
    both, noise = noise_runs[level]
    mean_p = lambda v: float(rm.model_f64(v, windows)["p_mean"].mean())
    ps, pn, pb = mean_p(noise_runs["signal"]), mean_p(noise), mean_p(both)
    truth = 10.0 * np.log10(ps / pn)
    q = figures(both, windows)
    print("C/N %d dB at the input: mean p of the sum %.3e from the sum of the two; truth %.3f dB, cnr_db %.3f, %.3f off; am_depth %.3f"
          % (level, pb / (ps + pn) - 1.0, truth, q["cnr_db"], q["cnr_db"] - truth, q["am_depth"]))
    assert abs(pb / (ps + pn) - 1.0) <= 0.01
    assert abs(q["cnr_db"] - truth) <= rm.CNR_TOL_DB[level]


def test_noise_only_reads_no_carrier(noise_runs):
    """carrier amplitude 0: cnr_db reads -inf, no carrier.  (Complex Gaussian noise has M4 = 2 M2^2; the band-limited noise of this seed lies on the
    no-carrier side of it at every level, which is the same noise scaled.)"""
    for level in rm.CNR_LEVELS_DB:
        assert figures(noise_runs[level][1], list(range(1, 11)))["cnr_db"] == -np.inf, level


def test_f32_limit_of_the_estimate():
    """the C/N at which the f32 restatement's cnr_db and the float64 model's first differ by 1 dB, on a constant-envelope carrier in white noise, 10 windows:
    72 dB with this seed (0.4 dB at 66, 0.9 dB at 68) -- far above the 25.7 dB a filtered FM signal allows.  Asserted: not below 60 dB, where the window
    sums' rounding (2^-24 per addition, 150 per lane) is still 30 dB below N / S."""
    rng = np.random.default_rng(7)
    n, windows = 11 * W, list(range(1, 11))
    ph = np.cumsum(2 * np.pi * 30000.0 / 192000.0 * np.sin(2 * np.pi * 1000.0 / 192000.0 * np.arange(n)))
    limit = None
    for cnr in range(30, 90, 2):
        s = 0.5 * 10.0 ** (-cnr / 20.0) / np.sqrt(2.0)
        v = rm.as_pairs((0.5 * np.exp(1j * ph) + s * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64))
        a, b = figures(v, windows)["cnr_db"], rm.quality(rm.model_f64(v, windows))["cnr_db"]
        if not abs(a - b) < 1.0:
            limit = cnr
            break
    print("f32 limit of cnr_db: %s dB" % limit)
    assert limit is not None and limit >= 60


def test_cpp_adapter_compiles(fmx_amd, tmp_path):
    """host/fm_processor_adapter.h's reception-meter methods under -Wall -Werror, in the demo of tests/rx_demo; receptionQuality needs no device and
    refuses no records (exit code 4 if it did not); without a device the demo then reports that the processor could not be created"""
    import test_gpu_rx_meter as gr
    exe = str(tmp_path / "rx_adapter_demo")
    gr.build_demo(fmx_amd, exe)
    np.zeros((16384, 2), np.float32).tofile(str(tmp_path / "iq.f32"))
    out = subprocess.run([exe, str(tmp_path / "iq.f32"), str(tmp_path / "records.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode in (0, 3), out.stdout


# ---- fmx_rx_quality_of
def lib_quality(m, recs, fmRate=192000):
    return m.rx_quality(recs, fmRate)


def close(a, b):
    return a == b or (np.isfinite(a) and np.isfinite(b) and abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1e-300))


def test_quality_of_against_the_model(fmx_amd):
    """fmx_rx_quality_of (host only, no device) against quality () to 1e-12 relative, on noisy and clean records, one record and many, two rates"""
    m = fmx_amd.fmx
    assert m.RX_DTYPE == rm.RX_DTYPE
    for seed, cnr, off in ((1, 12.0, -8000.0), (2, 35.0, 2500.0), (3, 90.0, 60000.0)):
        v = synthetic(4 * W, seed=seed, cnr_db=cnr, offset_hz=off)
        recs = rm.records_of(rm.restate_windows(v, [1, 2, 3]), [1, 2, 3])
        for sub, rate in ((recs, 192000), (recs[:1], 192000), (recs, 96000)):
            got, want = lib_quality(m, sub, rate), rm.quality(sub, rate)
            assert got["windows"] == sub.size
            for k in ("level_dbfs", "cnr_db", "am_depth", "offset_hz"):
                assert close(got[k], want[k]), (seed, k, got[k], want[k])


def test_quality_of_edge_cases(fmx_amd):
    """n = 0, all-zero records, p_max = 0, noise (no carrier), a flat envelope (no noise), and the argument checks"""
    m = fmx_amd.fmx
    L = m.load_library()
    out = m.FmxRxQuality()
    zero = np.zeros(3, rm.RX_DTYPE)
    with pytest.raises(m.FmxError) as e:
        m.rx_quality(zero[:0])
    assert e.value.code == m.FMX_E_INVALID
    assert L.fmx_rx_quality_of(zero.ctypes.data, 0, 192000, C.byref(out)) == m.FMX_E_INVALID
    assert L.fmx_rx_quality_of(None, 3, 192000, C.byref(out)) == m.FMX_E_INVALID
    assert L.fmx_rx_quality_of(zero.ctypes.data, 3, 192000, None) == m.FMX_E_INVALID
    assert L.fmx_rx_quality_of(zero.ctypes.data, 3, 0, C.byref(out)) == m.FMX_E_INVALID
    q = m.rx_quality(zero)
    assert q == {"level_dbfs": -np.inf, "cnr_db": -np.inf, "am_depth": 0.0, "offset_hz": 0.0, "windows": 3} and q == rm.quality(zero)
    one = zero.copy()                       # one window with a signal, two silent ones (p_max = 0 counts as depth 0)
    one[1]["p_max"], one[1]["p_min"], one[1]["p_mean"], one[1]["p2_mean"], one[1]["r1_re"], one[1]["r1_im"] = 0.5625, 0.0625, 0.25, 0.0625, 0.0, -0.25
    q, want = m.rx_quality(one), rm.quality(one)
    assert close(q["am_depth"], 0.5) and close(q["offset_hz"], -48000.0) and all(close(q[k], want[k]) for k in want)
    flat = zero.copy()                      # a constant envelope: M4 = M2^2, N = 0
    flat["p_max"] = flat["p_min"] = flat["p_mean"] = 0.25
    flat["p2_mean"] = 0.0625
    flat["r1_re"] = 0.25
    assert m.rx_quality(flat)["cnr_db"] == np.inf and m.rx_quality(flat)["am_depth"] == 0.0
    noise = flat.copy()                     # complex Gaussian noise: M4 = 2 M2^2
    noise["p2_mean"] = 0.125
    assert m.rx_quality(noise)["cnr_db"] == -np.inf
    n = (C.c_int32 * 1)()
    assert L.fmx_rx_meter_enable(None, 0, 1) == m.FMX_E_INVALID
    assert L.fmx_rx_records(None, 0, 1, None, 0, n) == m.FMX_E_INVALID

"""CPU checks of the sub-carrier decoder (sdr-j-fm_amd/csrc/fmx_sca.h): sca::piece against a sample-by-sample brute force; the two
designs through the C export (which needs no device); the header's host form (tests/sca_check.cpp: carry, span and per-sample functions driven piece by
piece as the kernels drive them) and an independent numpy-f32 restatement against the float64 model of tests/sca_model.py; the detector against seeded
defects; the truth figures against what tests/sca_signal.py sent.

The comparison signal (sca_signal.cpu_signal): an SCA of 7500 Hz injection at 67 kHz carrying a 1 kHz tone at +-6 kHz, under band-limited noise of
15 kHz rms in L+R and 10 kHz rms in L-R, a 7500 Hz pilot and an RDS band of 2000 Hz rms, numpy seed 1, 192 kS/s, 12 blocks and 100 fm samples."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sca_model as sm
import sca_signal as sg
import survey_model as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, LB = sm.BLOCK_FM, sm.LOOKBACK

# measured with the numpy-f32 restatement on the comparison signal (re-measured by test_host_form_and_restatement_against_float64, which prints them)
RESTATEMENT_S_WORST, RESTATEMENT_S_MEDIAN, RESTATEMENT_LEVEL_WORST = 5.7e-7, 6.6e-8, 1.1e-7


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"          # (the compile is the check: without the compiler the tests fail)
    d = tmp_path_factory.mktemp("sca")
    exe = str(d / "sca_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "sca_check.cpp")])

    class Check:
        @staticmethod
        def blocks(x, centre=67000, j_start=0, cuts=(), on_call=0, defect=0):
            """-> {b: (audio, level)} of the blocks delivered, in the order of delivery"""
            fi, fo = str(d / "in.bin"), str(d / "out.bin")
            np.asarray(x, np.float32).tofile(fi)
            subprocess.check_call([exe, "blocks", fi, fo, str(centre), str(j_start), str(on_call), str(defect)] + [str(c) for c in cuts])
            raw = np.fromfile(fo, np.float32).reshape(-1, 2 + sm.BLOCK_AUDIO)
            return {int(row[0]) + j_start // BF: (row[2:], row[1]) for row in raw}

        @staticmethod
        def pieces(triples):
            out = subprocess.run([exe, "piece"] + [str(v) for q in triples for v in q], capture_output=True, text=True, check=True).stdout.splitlines()
            return [tuple(int(v) for v in ln.split()) for ln in out]
    return Check


_CACHE = {}


def taps(fmx_amd):
    if "g" not in _CACHE:
        _CACHE["g"], _CACHE["a"] = fmx_amd.sca_taps("g"), fmx_amd.sca_taps("a")
    return _CACHE["g"], _CACHE["a"]


def signal():
    if "d" not in _CACHE:
        _CACHE["d"] = sg.cpu_signal()
    return _CACHE["d"]


def reference(fmx_amd):
    """the float64 model and the restatement's levels on the comparison signal, computed once"""
    if "M" not in _CACHE:
        g, a = taps(fmx_amd)
        _CACHE["M"] = sm.model64(signal(), g, a, 67000)
        _CACHE["B32"] = sm.blocks32(signal(), g, a, 67000)
        _CACHE["lv"] = sm.levels(_CACHE["M"], _CACHE["B32"])
    return _CACHE["M"], _CACHE["B32"], _CACHE["lv"]


def same_blocks(x, y):
    return sorted(x) == sorted(y) and all(np.array_equal(x[b][0].view(np.uint32), y[b][0].view(np.uint32)) and
                                          np.float32(x[b][1]).tobytes() == np.float32(y[b][1]).tobytes() for b in x)


# ---- 1: the integers --------------------------------------------------------------------------------------------------------------------------------
def brute(J0, nj, on_from):
    """sample by sample: which blocks have their last fm sample in [J0, J0 + nj) and their first read sample at or behind on_from; which samples in front
    of J0 (and of J0 + nj) a block not yet complete there, and delivered, still reads"""
    b_lo = max(J0 // BF - 2, 0)
    first = next(b for b in range(max(on_from // BF - 1, 0), on_from // BF + 3) if BF * b - LB >= on_from)
    done = [b for b in range(b_lo, (J0 + nj) // BF + 2) if b >= first and J0 <= BF * b + BF - 1 < J0 + nj]

    def carried(J):
        later = [b for b in range(max(J // BF - 2, 0), max(J // BF, first) + 2) if b >= first and BF * b + BF - 1 >= J]
        lo = min(BF * b - LB for b in later)
        return lo, max(J - lo, 0)
    c0, c1 = carried(J0), carried(J0 + nj)
    return first, (done[0] if done else None), len(done), c0, c1


def test_piece_against_a_sample_by_sample_brute_force(check):
    """calls of one fm sample across a block end, on_from inside a block, long pieces, J0 beyond 2^32 and 2^40"""
    cases = []
    for base in (0, BF * 5, BF * 2236963, BF * 572662307):                  # (1920 x 2 236 963 > 2^32, 1920 x 572 662 307 > 2^40)
        for on in (base, base + 1, base + 700, base + BF - LB, base + BF - LB + 1, base + BF - 1):
            for J0 in (on, on + 1, base + BF - 2, base + BF - 1, base + BF, base + 2 * BF - 1, base + 2 * BF, base + 3 * BF - 1, base + 3 * BF + 5, base + 4 * BF - 1):
                if J0 < on:
                    continue
                for nj in (1, 2, 100, BF - 1, BF, BF + 1, 3 * BF + 7, 19200):
                    cases.append((J0, nj, on))
    got = check.pieces(cases)
    assert len(got) == len(cases) > 1000
    for (J0, nj, on), (first, b0, blocks, cf0, cl0, cf1, cl1, from_carry, row_src) in zip(cases, got):
        w_first, w_b0, w_blocks, (w_cf0, w_cl0), (w_cf1, w_cl1) = brute(J0, nj, on)
        assert first == w_first and blocks == w_blocks and (blocks == 0 or b0 == w_b0), (J0, nj, on)
        assert cl0 == w_cl0 and cl1 == w_cl1 and (cl0 == 0 or cf0 == w_cf0) and (cl1 == 0 or cf1 == w_cf1), (J0, nj, on)
        assert 0 <= cl0 <= LB + BF - 1 and 0 <= cl1 <= LB + BF - 1
        assert from_carry == (max(J0 - cf1, 0) if cl1 else 0) and row_src == max(cf1 - J0, 0)
        assert from_carry == 0 or (cf1 >= cf0 and cf1 - cf0 + from_carry <= cl0)          # (what comes out of the old carry lies in it)


# ---- 2: the designs ---------------------------------------------------------------------------------------------------------------------------------
def test_the_designs(fmx_amd):
    g, a = taps(fmx_amd)
    assert g.shape == (192,) and a.shape == (128,) and g.dtype == a.dtype == np.float32
    assert abs(g.sum(dtype=np.float64) - 1) < 192 * 2.0 ** -25 and abs(a.sum(dtype=np.float64) - 1) < 128 * 2.0 ** -25      # (one f32 rounding a tap)
    assert np.abs(g - sm.design_band()).max() < 2.0 ** -24 and np.abs(a - sm.design_audio()).max() < 2.0 ** -24              # (numpy's own Kaiser and sinc)
    assert np.array_equal(g, g[::-1])
    # g: flat to the pass edge, 6 dB at half_band + 2000, gone from half_band + 4400 on (Kaiser beta = 7: side lobes below -70 dB)
    assert sm.response(g, 9000, 192000) > 0.99 and abs(sm.response(g, 11000, 192000) - 0.5) < 1e-3
    assert max(sm.response(g, f, 192000) for f in range(13400, 96001, 100)) < 10 ** (-70 / 20)
    # a against LP (f) / sqrt (1 + (2 pi f tau)^2): the sampled exponential's pole against the analogue one differs by 0.7 % at 3 kHz and 48 kS/s (computed:
    # 0.3357 against 0.3334), its truncation at 48 values by alpha^48 = 0.13 %: bound 1 %
    lp = sm.kaiser_lowpass(81, 6300.0, 48000.0)
    lp /= lp.sum()
    for f in (400, 1000, 3000):
        want = sm.response(lp, f, 48000) / np.sqrt(1 + (2 * np.pi * f * 150e-6) ** 2)
        assert abs(sm.response(a, f, 48000) / want - 1) < 0.01, f
    assert abs(sm.response(lp, 6300, 48000) - 0.5) < 2e-3
    # tau = 0: the low-pass alone, padded
    a0 = fmx_amd.sca_taps("a", deemphasis_us=0)
    assert np.array_equal(a0[:81], lp.astype(np.float32)) and not a0[81:].any()
    # another setup and rate reach the design
    assert np.abs(fmx_amd.sca_taps("g", rate_hz=256000, half_band_hz=7000) - sm.design_band(7000, 256000)).max() < 2.0 ** -24
    info = fmx_amd.sca_info(192000)
    assert info == dict(audio_rate_hz=24000, block_audio=240, block_fm=1920, lookback_fm=703, delay_fm=95.5 + 4 * 40, ring_blocks=128, bytes_per_channel=135432)


def test_every_refusal_names_its_argument(fmx_amd):
    m = fmx_amd.fmx
    for kw, name in ((dict(half_band_hz=500), "half_band_hz"), (dict(half_band_hz=30000), "half_band_hz"), (dict(audio_cut_hz=100), "audio_cut_hz"),
                     (dict(audio_cut_hz=20000), "audio_cut_hz"), (dict(deviation_hz=0), "deviation_hz"), (dict(deemphasis_us=-1), "deemphasis_us"),
                     (dict(deemphasis_us=5000), "deemphasis_us"), (dict(rate_hz=1000), "fmRate"), (dict(rate_hz=192001), "fmRate"),
                     (dict(rate_hz=24000, half_band_hz=10000), "half_band_hz"), (dict(rate_hz=48000, audio_cut_hz=5000), "audio_cut_hz")):
        with pytest.raises(fmx_amd.FmxError) as e:
            fmx_amd.sca_taps("g", **kw)
        assert e.value.code == m.FMX_E_INVALID and name in str(e.value), (kw, str(e.value))
    with pytest.raises(fmx_amd.FmxError) as e:
        fmx_amd.sca_taps(2)
    assert "which" in str(e.value)
    with pytest.raises(fmx_amd.FmxError) as e:
        fmx_amd.sca_info(1000)
    assert "fmRate" in str(e.value)
    L = m.load_library()
    cfg = m.FmxScaConfig(4, 9000, 5000, 6000, 150)
    import ctypes as C
    n = C.c_int32()
    assert L.fmx_sca_taps(C.byref(cfg), 192000, 0, None, 0, C.byref(n)) == m.FMX_E_INVALID and b"struct_size" in L.fmx_last_error()
    assert L.fmx_sca_taps(None, 192000, 0, None, 4, C.byref(n)) == m.FMX_E_INVALID and b"dst" in L.fmx_last_error()
    assert L.fmx_sca_taps(None, 192000, 1, None, 0, C.byref(n)) == m.FMX_OK and n.value == 128


# ---- 3: the two f32 forms against float64 -------------------------------------------------------------------------------------------------------------
def test_host_form_and_restatement_against_float64(fmx_amd, check):
    M, B32, lv = reference(fmx_amd)
    cond = sm.conditioning(M)
    print("\nblocks %s; min |y| / median |y| = %.3f" % (sorted(M), cond))
    assert sorted(M) == list(range(1, 12)) and cond >= 0.1
    print("numpy-f32 restatement: s worst %.3e, median %.3e; level worst %.3e, median %.3e (relative)" % lv)
    # (the recorded levels hold: the bound of everything below is no accident of this run)
    assert lv[0] <= 2 * RESTATEMENT_S_WORST and lv[1] <= 2 * RESTATEMENT_S_MEDIAN and lv[2] <= 2 * RESTATEMENT_LEVEL_WORST
    H = check.blocks(signal())
    assert sorted(H) == sorted(M)
    ok, r = sm.check("host form", H, M, lv)
    assert ok, r
    assert not same_blocks(H, B32)                                          # (two forms: fmaf against a rounding per product)


def test_the_host_form_does_not_depend_on_the_cut(fmx_amd, check):
    d = signal()
    n = len(d)
    whole = check.blocks(d)
    cuts = list(sv.call_cuts(1))
    cuts = cuts[:4] + [n - sum(cuts[:4])]                                   # (1000, 1500, 1000, 1200: calls that complete no block, then the rest)
    assert same_blocks(whole, check.blocks(d, cuts=cuts))
    assert same_blocks(whole, check.blocks(d, cuts=[2 * BF - 2, 1, 1, 1, 1, BF - 3, 1, 1, 1, n - 3 * BF - 2]))      # (one fm sample a call across two block ends)
    assert same_blocks(whole, check.blocks(d, cuts=[700] * (n // 700) + [n % 700]))
    # switched on in mid-block: the first delivered block is the first with its whole history behind the switch, and equals the whole run's
    late = check.blocks(d, cuts=[BF + 1218, n - BF - 1218], on_call=1)      # (on at 3138 = 2 x 1920 - 702: block 2 reads from 3137)
    assert sorted(late) == list(range(3, 12)) and same_blocks(late, {b: whole[b] for b in late})
    at = check.blocks(d, cuts=[BF + 1217, n - BF - 1217], on_call=1)        # (on at 3137 exactly: block 2 is delivered)
    assert sorted(at) == list(range(2, 12)) and same_blocks(at, {b: whole[b] for b in at})


def test_beyond_2_to_the_32_fm_samples(fmx_amd, check):
    """the same d placed at fm sample 1920 x 2 236 963 > 2^32: the mixed taps know no j, so the blocks are the same bits -- 67 000 x 1920 is a multiple
    of 192 000, so the contract's phase is the same too -- and the float64 model with its integer phase agrees"""
    g, a = taps(fmx_amd)
    d = signal()[:5 * BF]
    j0 = BF * 2236963
    assert j0 > 2 ** 32 and (67000 * BF) % 192000 == 0
    far, near = check.blocks(d, j_start=j0, cuts=[BF + 5, 1, len(d) - BF - 6]), check.blocks(d)
    assert sorted(far) == [2236963 + b for b in sorted(near)] and same_blocks(near, {b - 2236963: v for b, v in far.items()})
    M = sm.model64(d, g, a, 67000, j0=j0)
    ok, r = sm.check("beyond 2^32", far, M, reference(fmx_amd)[2])
    assert ok, r


# ---- 4: the detector ----------------------------------------------------------------------------------------------------------------------------------
def test_the_measure_flags_seeded_defects(fmx_amd, check):
    g, a = taps(fmx_amd)
    M, _, lv = reference(fmx_amd)
    d = signal()
    cuts = [2 * BF + 400, 3 * BF, len(d) - 5 * BF - 400]
    clean = check.blocks(d, cuts=cuts)
    ok, r = sm.check("no defect", clean, M, lv, quiet=True)
    assert ok
    ratios = {}
    for name, kind in (("a stale carry sample", 1), ("the row read one sample late in the second piece", 2), ("a block left out", 3)):
        bad = check.blocks(d, cuts=cuts, defect=kind)
        ok, r = sm.check(name, bad, M, lv, quiet=True)
        ratios[name] = max(r)
        assert not ok and sorted(bad) == sorted(M), name
    ok, r = sm.check("lag 2", sm.blocks32(d, g, a, 67000, lag=2), M, lv, quiet=True)
    ratios["u from y [m] and y [m - 2]"] = max(r)
    assert not ok
    # the mix phase in f32: harmless at fm sample 0, wrong beyond 2^24
    j0 = BF * 8739
    assert j0 > 2 ** 24
    short = d[:4 * BF]
    ok, r = sm.check("f32 phase", sm.blocks32_f32_phase(short, g, a, 67000, j0=j0), sm.model64(short, g, a, 67000, j0=j0), lv, quiet=True)
    ratios["the mix phase in f32 beyond 2^24 samples"] = max(r)
    assert not ok
    ok, r = sm.check("the header's form there", check.blocks(short, j_start=j0), sm.model64(short, g, a, 67000, j0=j0), lv, quiet=True)
    assert ok, r
    print("\nworst ratio per seeded defect (bound 2): " + "; ".join("%s: %.3g" % kv for kv in ratios.items()))
    assert min(ratios.values()) > 10


def test_an_all_zero_input_gives_exactly_zero(check):
    z = check.blocks(np.zeros(4 * BF, np.float32), cuts=[BF + 3, 3 * BF - 3])
    assert sorted(z) == [1, 2, 3]
    for audio, level in z.values():
        assert not audio.view(np.uint32).any() and np.float32(level).tobytes() == b"\0\0\0\0"      # (+0.0, not -0.0)


# ---- 5: the truth ---------------------------------------------------------------------------------------------------------------------------------------
# tone Hz, under programme -> bounds on |amplitude - |A (f)||, the residual's rms, |2 sqrt (level) x 75 000 - 7500| (worst block): twice what the float64
# model measures on the same signal (1.062e-4, 4.512e-6, 0.45; 5.226e-4, 1.642e-4, 0.62; 3.468e-3, 4.027e-7, 10.57; 1.100e-4, 1.995e-2,
# 389.99; 4.365e-4, 2.064e-2, 386.50; 2.929e-3, 1.971e-2, 408.88).  Under programme the residual and the level's excess are the RDS band inside the filter.
TRUTH = {(400, False): (2.124e-4, 9.024e-6, 0.90), (1000, False): (1.0452e-3, 3.284e-4, 1.24), (3000, False): (6.936e-3, 8.054e-7, 21.14),
         (400, True): (2.200e-4, 3.990e-2, 779.98), (1000, True): (8.730e-4, 4.128e-2, 773.0), (3000, True): (5.858e-3, 3.942e-2, 817.76)}


@pytest.mark.parametrize("tone_hz,prog", sorted(TRUTH))
def test_figures_against_what_the_generator_sent(fmx_amd, check, tone_hz, prog):
    """the header's host form on the C export's taps: the fitted amplitude of the tone against the response of `a` (a tone at the full +-6 kHz reads
    |A (f)|), the residual, and 2 sqrt (level) against the 7500 Hz sent"""
    g, a = taps(fmx_amd)
    d = sg.cpu_signal(with_programme=prog, tone_hz=float(tone_hz))
    H = check.blocks(d)
    s = np.concatenate([H[b][0] for b in sorted(H)]).astype(np.float64)
    amp, res = sg.tone_fit(s, tone_hz, 24000)
    inj = max(abs(2 * np.sqrt(float(H[b][1])) * sg.UNIT_HZ - 7500.0) for b in H)
    want = sm.response(a, tone_hz, 48000)
    b_amp, b_res, b_inj = TRUTH[tone_hz, prog]
    print("\n%d Hz%s: amplitude %.6f against |A| %.6f: %.3e apart (bound %.3e); residual %.3e rms (bound %.3e); injection %.2f Hz off (bound %.2f)"
          % (tone_hz, " under programme" if prog else "", amp, want, abs(amp - want), b_amp, res, b_res, inj, b_inj))
    assert len(H) == 11 and abs(amp - want) <= b_amp and res <= b_res and inj <= b_inj


# ---- 6: the C++ adapter ---------------------------------------------------------------------------------------------------------------------------------
def build_demo(fmx_amd, exe):
    host = os.path.join(ROOT, "sdr-j-fm_amd", "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + host, os.path.join(ROOT, "tests", "sca_demo", "sca_adapter_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])


def test_cpp_adapter_builds_and_reads_the_designs_without_a_device(fmx_amd, tmp_path):
    """host/fm_processor_adapter.h's methods under -Wall -Werror, in the demo of tests/sca_demo.  fmx_sca_info and fmx_sca_taps need no device; without one
    the demo then reports ok 0 and the library's text.  (What it writes with a device is checked in tests/test_gpu_sca.py.)"""
    exe, fin, fout = str(tmp_path / "sca_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "sca.bin")
    build_demo(fmx_amd, exe)
    sg.fm_iq(sg.multiplex(3 * 16384, 2304000), 2304000).tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    assert lines and lines[0] == "info rate 24000 block 240 fm 1920 lookback 703 delay 255.5 ring 128 bytes 135432 taps 192 sum 1.000000", lines
    if out.returncode == 3:
        assert lines[1].startswith("ok 0 error"), lines
    else:
        assert out.returncode == 0 and lines[-1].startswith("blocks "), lines

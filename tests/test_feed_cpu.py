"""CPU checks of the monitoring feed (sdr-j-fm_amd/csrc/fmx_feed.h): feed::piece against a frame-by-frame brute force; the design
through the C export (which needs no device); the header's host form (tests/feed_check.cpp: carry, span and per-sample functions driven piece by piece as
the kernels drive them) and the numpy-f32 restatement of tests/feed_model.py against each other bit for bit and against the float64 model within its derived
bounds; the checker against seeded defects; the figures of a tone, of an aliasing tone, the delay and the 16-bit conversion.

The comparison signals (feed_model): a stereo programme (band-limited noise per ear over a common one, two tones), a 1 kHz tone and white noise, as PCM
[frames, 2] f32, 12 blocks and 100 frames each."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import feed_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, LB, BLOCK, RING = fm.BLOCK_FRAMES, fm.LOOKBACK, fm.BLOCK, fm.RING
FRAMES = 12 * BF + 100


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"          # (the compile is the check: without the compiler the tests fail)
    d = tmp_path_factory.mktemp("feed")
    exe = str(d / "feed_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "feed_check.cpp")])

    class Check:
        @staticmethod
        def blocks(pcm, mode=1, m_start=0, cuts=(), on_call=0):
            """-> {b: (audio, power)} of the blocks delivered"""
            fi, fo = str(d / "in.bin"), str(d / "out.bin")
            np.ascontiguousarray(pcm, np.float32).tofile(fi)
            subprocess.check_call([exe, "blocks", fi, fo, str(mode), str(m_start), str(on_call)] + [str(c) for c in cuts])
            raw = np.fromfile(fo, np.float32).reshape(-1, 2 + BLOCK)
            return {int(row[0]) + m_start // BF: (row[2:], row[1]) for row in raw}

        @staticmethod
        def pieces(triples):
            out = []
            for k in range(0, len(triples), 2000):
                txt = subprocess.run([exe, "piece"] + [str(v) for q in triples[k:k + 2000] for v in q], capture_output=True, text=True, check=True).stdout
                out += [tuple(int(v) for v in ln.split()) for ln in txt.splitlines()]
            return out

        @staticmethod
        def s16(y):
            fi, fo = str(d / "y.bin"), str(d / "s.bin")
            np.asarray(y, np.float32).tofile(fi)
            subprocess.check_call([exe, "s16", fi, fo])
            return np.fromfile(fo, np.int16)

        @staticmethod
        def taps():
            fo = str(d / "h.bin")
            subprocess.check_call([exe, "taps", fo])
            return np.fromfile(fo, np.float32)
    return Check


_CACHE = {}


def taps(fmx_amd):
    if "h" not in _CACHE:
        _CACHE["h"] = fmx_amd.feed_taps()
    return _CACHE["h"]


def signals():
    if "x" not in _CACHE:
        _CACHE["x"] = {"programme": fm.programme(FRAMES), "tone": fm.tone(FRAMES), "noise": fm.noise(FRAMES)}
    return _CACHE["x"]


def reference(fmx_amd, name, mode):
    """the float64 model and the restatement on a comparison signal, computed once"""
    key = ("ref", name, mode)
    if key not in _CACHE:
        _CACHE[key] = (fm.model64(signals()[name], taps(fmx_amd), mode), fm.blocks32(signals()[name], taps(fmx_amd), mode))
    return _CACHE[key]


# ---- 1: the integers --------------------------------------------------------------------------------------------------------------------------------
def brute(M0, frames, on_from):
    """frame by frame: the blocks whose last frame lies in [M0, M0 + frames) and whose first read frame lies at or behind on_from; the frames in front of
    M0 (and of M0 + frames) that a delivered block not yet complete there still reads; the ring after every delivered block was written in turn"""
    first = next(b for b in range(max(on_from // BF - 1, 0), on_from // BF + 3) if BF * b - LB >= on_from)
    m = np.arange(M0, M0 + frames, dtype=np.int64)
    done = [int(b) for b in m[m % BF == BF - 1] // BF if b >= first]

    def carried(M):
        b = next(b for b in range(max(M // BF - 1, 0), max(M // BF, first) + 2) if b >= first and BF * b + BF - 1 >= M)
        return BF * b - LB, max(M - (BF * b - LB), 0)
    ring = {}
    for b in done:
        ring[b % RING] = b
    return first, (done[0] if done else None), len(done), carried(M0), carried(M0 + frames), ring


def test_piece_against_a_frame_by_frame_brute_force(check):
    """random on_from, M0 and piece lengths -- one frame, 479, 480, 481, longer than the ring --, starts beyond 2^32 and 2^40 frames"""
    rng = np.random.default_rng(5)
    cases = []
    for base in (0, BF * 7, BF * 8947849, BF * 2290649225):                    # (480 x 8 947 849 > 2^32, 480 x 2 290 649 225 > 2^40)
        assert base == 0 or base == BF * 7 or base > 2 ** 32
        for on in [base, base + 1, base + BF - LB, base + BF - LB + 1, base + BF - 1] + [base + int(v) for v in rng.integers(0, 3 * BF, 6)]:
            for M0 in [on, on + 1, base + BF - 1, base + BF, base + 2 * BF - 1, base + 3 * BF + 5] + [on + int(v) for v in rng.integers(0, 4 * BF, 6)]:
                if M0 < on:
                    continue
                for frames in [1, 2, BF - 1, BF, BF + 1, 4800, RING * BF + 3 * BF + 17] + [int(v) for v in rng.integers(1, 3 * BF, 3)]:
                    cases.append((M0, frames, on))
    got = check.pieces(cases)
    assert len(got) == len(cases) > 3000
    for (M0, frames, on), (first, b0, blocks, cf0, cl0, cf1, cl1, from_carry, row_src, formed, slot0) in zip(cases, got):
        w_first, w_b0, w_blocks, (w_cf0, w_cl0), (w_cf1, w_cl1), ring = brute(M0, frames, on)
        assert first == w_first and blocks == w_blocks and (blocks == 0 or b0 == w_b0), (M0, frames, on)
        assert cl0 == w_cl0 and cl1 == w_cl1 and (cl0 == 0 or cf0 == w_cf0) and (cl1 == 0 or cf1 == w_cf1), (M0, frames, on)
        assert 0 <= cl0 <= LB + BF - 1 and 0 <= cl1 <= LB + BF - 1
        assert from_carry == (max(M0 - cf1, 0) if cl1 else 0) and row_src == max(cf1 - M0, 0)
        assert from_carry == 0 or (cf1 >= cf0 and cf1 - cf0 + from_carry <= cl0)          # (what comes out of the old carry lies in it)
        assert cl1 - from_carry <= max(frames - row_src, 0)                               # (the rest lies in the piece's frames)
        # the ring: forming only the blocks from formed_from on leaves what forming every block in turn leaves
        assert {b % RING: b for b in range(max(formed, b0), b0 + blocks)} == ring and slot0 == b0 % RING, (M0, frames, on)
        assert formed >= M0 // BF and (M0 + frames) // BF - formed <= RING


# ---- 2: the design ----------------------------------------------------------------------------------------------------------------------------------
def db(x):
    return 20 * np.log10(x)


def test_the_design(fmx_amd, check):
    h = taps(fmx_amd)
    h64 = fm.design64()
    assert h.shape == (144,) and h.dtype == np.float32 and np.array_equal(h, check.taps())
    # within 1 ulp of numpy's float64 design of the same formula; the sum is 1 to f32 rounding (half an ulp a tap)
    assert np.all(np.abs(h.astype(np.float64) - h64) <= np.spacing(np.abs(h64).astype(np.float32)).astype(np.float64))
    assert abs(h.sum(dtype=np.float64) - 1) < 144 * 2.0 ** -25
    assert np.array_equal(h, h[::-1])
    assert abs(fm.response(h64, 8000) - 0.5) < 1e-3                         # the 6 dB point
    # the f32 taps' response: the issue's conditions (its own measurements of the double design: +-0.0006 dB, -81.96 dB, sum |h| = 2.112)
    ripple = max(abs(db(fm.response(h, f))) for f in range(0, 7001, 50))
    stop = max(db(fm.response(h, f)) for f in range(9000, 24001, 25))
    print("\nf32 taps: pass band 0 .. 7 kHz within %.5f dB, stop band from 9 kHz %.2f dB, sum |h| = %.4f" % (ripple, stop, np.abs(h).sum(dtype=np.float64)))
    assert ripple <= 0.002 and stop <= -80.0
    assert abs(np.abs(h).sum(dtype=np.float64) - 2.112) < 1e-3
    info = fmx_amd.feed_info()
    assert info == dict(rate_hz=16000, block_samples=160, block_frames=480, lookback_frames=143, delay_frames=71.5, ring_blocks=128, bytes_per_channel=84928)
    assert info["bytes_per_channel"] == 4 * (128 * 161 + 624)


def test_the_exports_refuse_bad_arguments(fmx_amd):
    m = fmx_amd.fmx
    L = m.load_library()
    n = C.c_int32()
    assert L.fmx_feed_taps(None, 4, C.byref(n)) == m.FMX_E_INVALID and b"dst" in L.fmx_last_error()
    assert L.fmx_feed_taps(None, 0, None) == m.FMX_E_INVALID
    assert L.fmx_feed_taps(None, 0, C.byref(n)) == m.FMX_OK and n.value == 144
    few = np.zeros(10, np.float32)
    assert L.fmx_feed_taps(few.ctypes.data, 10, C.byref(n)) == m.FMX_OK and n.value == 144 and np.array_equal(few, taps(fmx_amd)[:10])
    assert L.fmx_feed_info(None) == m.FMX_E_INVALID
    assert L.fmx_feed_enable(None, 0, 1) == m.FMX_E_INVALID and L.fmx_feed_allocated(None) == 0
    assert {"fmx_feed_enable", "fmx_feed_read", "fmx_feed_read_device", "fmx_feed_taps", "fmx_feed_info"} <= set(m.EXPORTS)


# ---- 3: the two f32 forms against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("programme", 1), ("programme", 2), ("programme", 3), ("tone", 1), ("noise", 1), ("noise", 3)])
def test_host_form_and_restatement_against_float64(fmx_amd, check, name, mode):
    M, B32 = reference(fmx_amd, name, mode)
    H = check.blocks(signals()[name], mode)
    assert sorted(M) == sorted(B32) == sorted(H) == list(range(1, 12))
    assert fm.same_blocks(H, B32)                                           # the two f32 forms: bit for bit
    print()
    ok, r = fm.check("host form, %s, mode %d" % (name, mode), H, M)
    assert ok, r
    assert r[0] > 0 and r[1] > 0                                            # (the comparison is no identity)


def test_the_modes_differ_and_mode_one_is_the_mix(fmx_amd, check):
    x = signals()["programme"]
    mix, left, right = (check.blocks(x, mode) for mode in (1, 2, 3))
    assert not fm.same_blocks(mix, left) and not fm.same_blocks(left, right)
    mono = np.stack([fm.v32(x, 1)] * 2, axis=1)
    assert fm.same_blocks(mix, check.blocks(mono, 2))                       # v is formed first, with one rounding, then filtered


def test_the_host_form_does_not_depend_on_the_cut(fmx_amd, check):
    x = signals()["programme"]
    n = len(x)
    whole = check.blocks(x)
    assert fm.same_blocks(whole, check.blocks(x, cuts=[100, 200, 150, n - 450]))                                        # calls that complete no block, then the rest
    assert fm.same_blocks(whole, check.blocks(x, cuts=[2 * BF - 2, 1, 1, 1, 1, BF - 3, 1, 1, 1, n - 3 * BF - 2]))      # one frame a call across two block ends
    assert fm.same_blocks(whole, check.blocks(x, cuts=[BF - 1, BF, BF + 1, n - 3 * BF]))
    assert fm.same_blocks(whole, check.blocks(x, cuts=[48] * (n // 48) + [n % 48]))                                     # the lumps a handle delivers
    assert fm.same_blocks(whole, check.blocks(x, cuts=[170] * (n // 170) + [n % 170]))
    # switched on in mid-block: the first delivered block is the first with its whole history behind the switch, and equals the whole run's
    late = check.blocks(x, cuts=[2 * BF - LB + 1, n - 2 * BF + LB - 1], on_call=1)                                     # (on at 818: block 2 reads from 817)
    assert sorted(late) == list(range(3, 12)) and fm.same_blocks(late, whole, blocks=sorted(late))
    at = check.blocks(x, cuts=[2 * BF - LB, n - 2 * BF + LB], on_call=1)                                               # (on at 817 exactly: block 2 is delivered)
    assert sorted(at) == list(range(2, 12)) and fm.same_blocks(at, whole, blocks=sorted(at))


def test_beyond_2_to_the_32_frames(fmx_amd, check):
    """the same PCM placed at frame 480 x 8 947 849 > 2^32: no phase is formed per sample, so the blocks are the same bits"""
    x = signals()["noise"][:5 * BF]
    m0 = BF * 8947849
    assert m0 > 2 ** 32
    far, near = check.blocks(x, m_start=m0, cuts=[BF + 5, 1, len(x) - BF - 6]), check.blocks(x)
    assert sorted(near) == [1, 2, 3, 4] and sorted(far) == [8947849 + b for b in sorted(near)]
    assert fm.same_blocks(near, {b - 8947849: v for b, v in far.items()})
    assert fm.same_blocks(far, fm.blocks32(x, taps(fmx_amd), m0=m0))
    ok, r = fm.check("beyond 2^32", far, fm.model64(x, taps(fmx_amd), m0=m0), quiet=True)
    assert ok, r


def test_an_all_zero_input_gives_exactly_zero(check):
    z = check.blocks(np.zeros((4 * BF, 2), np.float32), cuts=[BF + 3, 3 * BF - 3])
    assert sorted(z) == [1, 2, 3]
    for audio, power in z.values():
        assert not audio.view(np.uint32).any() and np.float32(power).tobytes() == b"\0\0\0\0"      # (+0.0, not -0.0)


def test_fma32_is_a_single_rounding():
    """the restatement's fused multiply-add against exact rational arithmetic, on cases picked to sit on float64's and f32's ties"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 3, 4000)).astype(np.float32)
    # a b = 2^-24 (1 - 2^-46) under c = 1 + 2^-23: the exact sum lies just below f32's tie and rounds down; a float64 sum lands on the tie and a second
    # rounding takes it up to the even neighbour 1 + 2^-22
    a = np.concatenate([a, np.float32([2.0 ** -24 + 2.0 ** -47, 2.0 ** -24 + 2.0 ** -47])])
    b = np.concatenate([b, np.float32([1 - 2.0 ** -23, -(1 - 2.0 ** -23)])])
    c = np.concatenate([c, np.float32([1 + 2.0 ** -23, -(1 + 2.0 ** -23)])])
    got = fm.fma32(a, b, c)
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert got[-2] == np.float32(1 + 2.0 ** -23) and naive[-2] == np.float32(1 + 2.0 ** -22)      # (the case does what it is there for)

    def exact(x, y, z):
        v = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(v))                                           # (a double rounding at worst one ulp off: pick the nearest of three)
        cand = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cand, key=lambda q: (abs(Fraction(float(q)) - v), int(np.float32(q).view(np.uint32)) & 1))
        return np.float32(best)
    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 4: the checker -------------------------------------------------------------------------------------------------------------------------------------
def test_the_checker_flags_seeded_defects(fmx_amd):
    h = taps(fmx_amd)
    ratios = {}
    for name, mode in (("programme", 1), ("programme", 2), ("noise", 1)):
        x = signals()[name]
        M = fm.model64(x, h, mode)
        ok, r = fm.check("no defect", fm.blocks32(x, h, mode), M, quiet=True)
        assert ok, r
        for defect in ("taps reversed", "phase", "block shift", "wrong ear", "no half", "power window"):
            if (defect == "wrong ear" and mode == 1) or (defect == "no half" and mode != 1):
                continue                                                    # (the ear is a defect of modes 2 and 3, the missing half of mode 1)
            bad = fm.blocks32(x, h, mode, defect=defect)
            blocks = sorted(set(bad) & set(M))
            assert len(blocks) >= 9
            ok, r = fm.check(defect, bad, M, blocks=blocks, quiet=True)
            ratios[name, mode, defect] = max(r)
            assert not ok, (name, mode, defect)
            if defect == "power window":                                    # (the samples are right, the power alone is not)
                assert r[0] <= 1.0 < r[1]
    # a missing block
    x = signals()["programme"]
    M, good = fm.model64(x, h), fm.blocks32(x, h)
    del good[5]
    assert not fm.check("a block left out", good, M, quiet=True)[0]
    print("\nworst ratio per seeded defect (bound 1): " + "; ".join("%s/%d/%s: %.3g" % (k + (v,)) for k, v in ratios.items()))
    assert min(ratios.values()) > 10


# ---- 5: the figures -------------------------------------------------------------------------------------------------------------------------------------
def feed_of(check, x, mode=1):
    H = check.blocks(x, mode)
    return np.concatenate([H[b][0] for b in sorted(H)]).astype(np.float64), min(H)


def test_a_1_khz_tone_keeps_its_amplitude_and_frequency(check):
    x = fm.tone(21 * BF, hz=1000.0, amp=0.5)
    y, b0 = feed_of(check, x)
    assert len(y) == 20 * BLOCK
    amp, res = fm.tone_fit(y, 1000.0, fm.RATE)
    spec = np.abs(np.fft.rfft(y[:3200] * np.hanning(3200)))                 # 5 Hz a bin
    print("\n1 kHz at 0.5: amplitude %.7f (%.5f dB), residual %.2e rms, spectrum's peak at %d Hz" % (amp, db(amp / 0.5), res, 5 * int(np.argmax(spec))))
    assert abs(db(amp / 0.5)) <= 0.002 and 5 * int(np.argmax(spec)) == 1000 and res < 1e-6


def test_a_10_khz_tone_leaves_at_most_minus_80_db_at_its_alias(check):
    x = fm.tone(21 * BF, hz=10000.0, amp=0.5)
    y, _ = feed_of(check, x)
    amp, _ = fm.tone_fit(y, 6000.0, fm.RATE)                                # 16 000 - 10 000
    print("\n10 kHz at 0.5: %.2f dB at 6 kHz" % db(max(amp, 1e-30) / 0.5))
    assert db(max(amp, 1e-30) / 0.5) <= -80.0


def test_the_delay_is_71_5_frames(check):
    hz = 100.0                                                              # (a period of 480 frames: the phase is unambiguous)
    x = fm.tone(21 * BF, hz=hz, amp=0.5)
    y, b0 = feed_of(check, x)
    t = (np.arange(len(y)) + BLOCK * b0) / fm.RATE                          # feed sample n <-> frame 3 n
    A = np.stack([np.sin(2 * np.pi * hz * t), np.cos(2 * np.pi * hz * t)], axis=1)
    c, *_ = np.linalg.lstsq(A, y, rcond=None)
    delay = -np.arctan2(c[1], c[0]) / (2 * np.pi * hz) * fm.FRAME_RATE
    print("\ndelay %.4f frames" % delay)
    assert abs(delay - fm.DELAY_FRAMES) < 0.01


def test_to_s16(check):
    y = np.float32([1.0, -1.0, 0.0, 0.5, -0.5, 1.5 / 32768, 2.5 / 32768, -1.5 / 32768, -2.5 / 32768, 0.5 / 32768, -0.5 / 32768, 32766.5 / 32768, 32767.5 / 32768,
                    2.0, -2.0, 1e9, -1e9, 32767.0 / 32768, -32767.5 / 32768, -32768.5 / 32768, 0.4999 / 32768, np.inf, -np.inf])
    want = np.int16([32767, -32768, 0, 16384, -16384, 2, 2, -2, -2, 0, 0, 32766, 32767,
                     32767, -32768, 32767, -32768, 32767, -32768, -32768, 0, 32767, -32768])
    got = check.s16(y)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(fm.to_s16(y), want)                               # the numpy form the GPU test uses
    r = np.random.default_rng(4).standard_normal(5000).astype(np.float32)
    assert np.array_equal(check.s16(r), fm.to_s16(r))


# ---- 6: the C++ adapter ---------------------------------------------------------------------------------------------------------------------------------
def build_demo(fmx_amd, exe):
    host = os.path.join(ROOT, "sdr-j-fm_amd", "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + host, os.path.join(ROOT, "tests", "feed_demo", "feed_adapter_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])


def test_cpp_adapter_builds_and_reads_the_design_without_a_device(fmx_amd, tmp_path, ol):
    """host/fm_processor_adapter.h's methods under -Wall -Werror, in the demo of tests/feed_demo.  fmx_feed_info and fmx_feed_taps need no device; without
    one the demo then reports ok 0 and the library's text.  (What it writes with a device is checked in tests/test_gpu_feed.py.)"""
    exe, fin, fout = str(tmp_path / "feed_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "feed.bin")
    build_demo(fmx_amd, exe)
    ol.synth_iq(3 * 16384).tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    assert lines and lines[0] == "info rate 16000 block 160 frames 480 lookback 143 delay 71.5 ring 128 bytes 84928 taps 144 sum 1.000000", lines
    if out.returncode == 3:
        assert lines[1].startswith("ok 0 error"), lines
    else:
        assert out.returncode == 0 and lines[-1].startswith("blocks "), lines

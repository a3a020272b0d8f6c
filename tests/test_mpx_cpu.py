"""CPU checks of the multiplex spectrum meter (sdr-j-fm_amd/csrc/fmx_mpx.h): the header's loader, the survey's stage functions and the
meter's fold compiled for the host and driven launch by launch, thread by thread (tests/mpx_check.cpp, "kernel_form") against the float64 model of
tests/mpx_model.py; the detector against seeded defects; the plan the meter takes over from the spectrum meter at fm-sample counts beyond 2^32 and
with its own 8 KB blocks; the figures through the C export (which needs no device) against what a numpy generator sent.

The comparisons' signal is mpx_model.noise_mpx and their measure mpx_model.bin_errors: see the head of mpx_model.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mpx_model as mm
import spec_model as pm
import survey_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BINS = mm.N, mm.BINS
GRIDS = ((1, 1), (2, 1), (3, 1), (2, 3))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"          # (the compile is the check: without the compiler the tests fail)
    d = tmp_path_factory.mktemp("mpx")
    exe = str(d / "mpx_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "mpx_check.cpp")])

    class Check:
        @staticmethod
        def spectrum(x, B, S, cuts=(), on_call=0, scratch=2, defect=0):
            """-> {record index: (mean, peak)} of the records delivered, as they stood in the ring behind the piece that completed them; defect: one of
            the driver's seeded defects (the head of mpx_check.cpp)"""
            fi, fo = str(d / "in.bin"), str(d / "out.bin")
            np.asarray(x, np.float32).tofile(fi)
            subprocess.check_call([exe] + (["defect", str(defect)] if defect else ["spectrum"]) + [fi, fo, str(B), str(S), str(on_call), str(scratch)] + [str(c) for c in cuts])
            raw = np.fromfile(fo, np.float32).reshape(-1, 1 + 2 * BINS)
            return {int(row[0]): (row[1:1 + BINS], row[1 + BINS:]) for row in raw}

        @staticmethod
        def lines(mode, tuples):
            return subprocess.run([exe, mode] + [str(v) for q in tuples for v in q], capture_output=True, text=True, check=True).stdout.splitlines()
    return Check


_CACHE = {}


def signal():
    if "d" not in _CACHE:
        _CACHE["d"] = mm.cpu_signal(0)
    return _CACHE["d"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def stacked(recs, idx):
    return np.stack([recs[r][0] for r in idx]), np.stack([recs[r][1] for r in idx])


# ---- 1, 2: the kernel form against float64, the cuts bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", GRIDS)
def test_kernel_form_against_the_float64_model(check, B, S):
    d = signal()
    idx, mean64, peak64 = mm.records64(d, B, S)
    _, mean32, peak32 = mm.records32(d, B, S)
    got = check.spectrum(d, B, S)
    assert sorted(got) == idx[-mm.RING:] or sorted(got) == idx              # (one piece: the ring keeps the last four)
    keep = sorted(got)
    rows = [idx.index(r) for r in keep]
    gm, gp = stacked(got, keep)
    print("[B=%d S=%d] a record's bins span %.1f dB" % (B, S, mm.span_db(mean64)))
    for tag, g, P64, P32 in (("mean", gm, mean64[rows], mean32[rows]), ("peak", gp, peak64[rows], peak32[rows])):
        lw, lm = mm.levels(P64, P32, g)
        print("[B=%d S=%d %s] levels: worst %.3e, median %.3e" % (B, S, tag, lw, lm))
        # (the kernel form is one of the restatements that set the level: the check is that both restatements agree to within a factor of two)
        for name, r in (("kernel form", g), ("numpy f32", P32)):
            ok, _, _ = mm.check("%s %s" % (name, tag), r, P64, *mm.levels(P64, P32 if name == "kernel form" else g))
            assert ok
    if B == 1:
        assert same_bits(gm, gp)
    # the cuts: every record as it stood behind the piece that completed it, bit for bit the whole's
    cut = check.spectrum(d, B, S, cuts=sm.call_cuts(1))
    have = sorted(cut)                                  # (a piece that completes five records leaves four in the ring: B = 1, the last piece)
    assert set(keep) <= set(have) <= set(idx) and (B == 1 or have == idx) and len(have) >= len(idx) - 1
    for r in keep:
        assert same_bits(cut[r][0], got[r][0]) and same_bits(cut[r][1], got[r][1]), r
    one = check.spectrum(d, B, S, cuts=[N - 3] + [1] * 6 + [len(d) - N - 3], scratch=1)      # (pieces of one fm sample across a block end)
    for r in keep:
        assert same_bits(one[r][0], got[r][0]) and same_bits(one[r][1], got[r][1]), r
    at = [idx.index(r) for r in have]
    cm, cp = stacked(cut, have)
    assert mm.check("cuts mean", cm, mean64[at], *mm.levels(mean64[at], mean32[at]))[0]
    assert mm.check("cuts peak", cp, peak64[at], *mm.levels(peak64[at], peak32[at]))[0]


def test_a_meter_switched_on_in_mid_block_takes_the_next_block(check):
    d = signal()
    cuts = sm.call_cuts(1)
    for B, S in ((2, 1), (2, 3)):
        got = check.spectrum(d, B, S, cuts=cuts, on_call=2)
        first = pm.first_block(sum(cuts[:2]), S)
        idx, mean64, peak64 = mm.records64(d, B, S, first=first)
        _, mean32, _ = mm.records32(d, B, S, first=first)
        assert first == 1 and sorted(got) == idx and idx and idx[0] == 1
        gm, _ = stacked(got, idx)
        assert mm.check("switched on", gm, mean64, *mm.levels(mean64, mean32))[0]


# ---- 3: the detector ----------------------------------------------------------------------------------------------------------------------------
def test_the_measure_flags_defects_seeded_into_the_driver(check):
    """the same detector on the header's own loader, carry and fold: tests/mpx_check.cpp run with one defect seeded into how it drives them"""
    d = signal()
    cuts = sm.call_cuts(1)
    idx, mean64, peak64 = mm.records64(d, 2, 1)
    _, mean32, peak32 = mm.records32(d, 2, 1)
    clean = check.spectrum(d, 2, 1, cuts=cuts)
    gm, gp = stacked(clean, idx)
    assert mm.check("clean mean", gm, mean64, *mm.levels(mean64, mean32))[0] and mm.check("clean peak", gp, peak64, *mm.levels(peak64, peak32))[0]
    for kind, name in ((1, "a stale carry sample"), (2, "a row read one sample late in the second piece"), (3, "a block left out")):
        got = check.spectrum(d, 2, 1, cuts=cuts, defect=kind)
        assert sorted(got) == idx
        bm, bp = stacked(got, idx)
        okm, rwm, rmm = mm.check("m", bm, mean64, *mm.levels(mean64, mean32), quiet=True)
        okp, rwp, rmp = mm.check("p", bp, peak64, *mm.levels(peak64, peak32), quiet=True)
        print("[driver defect: %s] mean: worst ratio %.3g, median ratio %.3g; peak: worst ratio %.3g, median ratio %.3g (bound 2)" % (name, rwm, rmm, rwp, rmp))
        assert not okm and not okp, name


def test_the_measure_flags_seeded_defects():
    d = signal().astype(np.float64)
    flagged = {}

    def judge(name, B, S, bad_idx, bad_mean, bad_peak, first=0):
        idx, mean64, peak64 = mm.records64(d, B, S, first=first)
        _, mean32, peak32 = mm.records32(d, B, S, first=first)
        if list(bad_idx) != idx:
            print("[defect: %s] index list %s against %s" % (name, list(bad_idx), idx))
            flagged[name] = True
            return
        okm, rwm, rmm = mm.check("m", bad_mean, mean64, *mm.levels(mean64, mean32), quiet=True)
        okp, rwp, rmp = mm.check("p", bad_peak, peak64, *mm.levels(peak64, peak32), quiet=True)
        print("[defect: %s] mean: worst ratio %.3g, median ratio %.3g; peak: worst ratio %.3g, median ratio %.3g (bound 2)" % (name, rwm, rmm, rwp, rmp))
        flagged[name] = not (okm and okp)

    # a block left out (B = 2: block 3 does not reach its record's sum and maximum)
    p = mm.block_powers32(d, 1)
    p_bad = p.copy(); p_bad[3] = 0
    judge("a block left out", 2, 1, *mm.records_from_powers32(p_bad, 2))
    # peak filled with the mean
    i, m, _ = mm.records32(d, 2, 1)
    judge("peak filled with the mean", 2, 1, i, m, m)
    # the grid off by one fm sample at S = 3
    judge("grid off by one fm sample at S = 3", 2, 3, *mm.records32(np.concatenate([d[1:], [0.0]]), 2, 3))
    # a stale carry sample: one sample of a block is the one a block earlier
    stale = d.copy(); stale[2 * N + 700] = d[N + 700]
    judge("a stale carry sample", 2, 1, *mm.records32(stale, 2, 1))
    # a record let in from in front of the first block
    judge("a record from in front of the first block", 2, 1, *mm.records32(d, 2, 1, first=0), first=1)
    # bin 2047 written from bin 2048
    p49 = mm.block_powers32(d, 1, bins=BINS + 1)
    p_bad = p49[:, :BINS].copy(); p_bad[:, BINS - 1] = p49[:, BINS]
    judge("bin 2047 written from bin 2048", 1, 1, *mm.records_from_powers32(p_bad, 1))
    # a row read one sample late in the second piece
    n1 = sm.call_cuts(1)[0]
    late = d.copy(); late[n1:-1] = d[n1 + 1:]
    judge("a row read one sample late in the second piece", 2, 1, *mm.records32(late, 2, 1))
    assert len(flagged) == 7 and all(flagged.values()), flagged


# ---- 4: the plan the meter takes over ------------------------------------------------------------------------------------------------------------
def test_the_plan_at_fm_sample_counts_beyond_2_to_the_32(check):
    for S, B in ((1, 48), (3, 2), (16, 1)):
        P = N * S
        g_far = ((1 << 32) // (P * B) + 1) * P * B
        grid = pm.BruteGrid(g_far, S, B)
        calls = [N - 2, 1, 1, 1, 1000, 31999, 16000, P, 2 * P + 17, 1]
        want, quads = [], []
        for n in calls:
            w, g0 = grid.call(n)
            want.append(w); quads.append((g0, n, S, B))
        got = [tuple(int(v) for v in l.split()) for l in check.lines("plan", quads)]
        for q, g, (blocks, fill, fill_after, append, src, phase, record0, records) in zip(quads, got, want):
            b0, gblocks, gfill, gfill_after, gappend, gsrc, gphase, grecord0, grecords = g
            assert (gblocks, gfill, gfill_after, gappend, gphase, grecord0, grecords) == (blocks, fill, fill_after, append, phase, record0, records), (q, g)
            assert b0 == record0 * B + phase and (src is None or gsrc == src), (q, g)


def test_the_chunks_cover_every_block_once_within_32768_blocks_of_8_kb(check):
    cap = 32768
    triples = [(ch, blocks, carries) for ch in (1, 3, 4096, 32768, 32769, 40000) for blocks in (0, 1, 5, 9) for carries in (0, 1)]
    it = iter(check.lines("launches", triples))
    for ch, blocks, carries in triples:
        seen, carried = np.zeros(ch, np.int64), np.zeros(ch, np.int64)
        for line in it:
            if line == "end":
                break
            j0, gn, done, nb, wc = (int(v) for v in line.split())
            assert gn * max(nb, 1) <= cap and gn * nb * BINS * 4 <= 256 << 20 and 0 < gn and j0 + gn <= ch
            assert np.all(seen[j0:j0 + gn] == done)               # (a channel's blocks in order, none twice)
            seen[j0:j0 + gn] += nb
            if wc:
                assert np.all(seen[j0:j0 + gn] == blocks)        # (the carry behind the channel's last block)
                carried[j0:j0 + gn] += 1
        assert np.all(seen == blocks) and np.all(carried == (1 if carries else 0)), (ch, blocks, carries)


# ---- 5: the figures through the C export ------------------------------------------------------------------------------------------------------
# (figure, truth -- what the generator sent --, the error measured on the CPU, the bound asserted: twice the measurement, DESIGN.md 4.16's table)
FIGURE_BOUNDS = {
    ("pilot at 19000.0", "pilot_hz"): 0.033,                  # measured 0.01602 Hz of 7500
    ("pilot at 19000.0", "pilot_freq_hz"): 0.00066,           # measured 0.0003287 Hz
    ("pilot at 19000.0", "mono_hz"): 176.0,                   # measured 87.81 Hz of 15 000: 48 Hann-weighted blocks of noise are what they are
    ("pilot at 19000.0", "total_hz"): 167.0,                  # measured 83.39 Hz of 15 909.9
    ("pilot at 19001.5", "pilot_hz"): 0.036,                  # measured 0.018 Hz
    ("pilot at 19001.5", "pilot_freq_hz"): 0.00081,           # measured 0.0004008 Hz
    ("pilot at 19001.5", "mono_hz"): 176.0,                   # measured 87.81 Hz
    ("pilot at 19001.5", "total_hz"): 167.0,                  # measured 83.39 Hz
    ("L-R", "stereo_hz"): 6.9,                                # measured 3.439 Hz of 10 000
    ("L-R", "carrier38_hz"): 0.22,                            # measured 0.1081 Hz of 0: the skirts of the programme a kilohertz away
    ("L-R with a 38 kHz leak", "stereo_hz"): 6.9,             # measured 3.439 Hz
    ("L-R with a 38 kHz leak", "carrier38_hz"): 0.0031,       # measured 0.001518 Hz of 750
    ("RDS-shaped band", "rds_hz"): 26.4,                      # measured 13.18 Hz of 2000
    ("FM sub-carrier at 67 kHz", "aux_hz"): 74.3,             # measured 37.12 Hz of 5303.3: the sidebands below 61 kHz are the band's loss
    ("FM sub-carrier at 67 kHz", "band_hz"): 1.33,            # measured 0.6606 Hz of 5303.3 over [59 000, 75 000]
    ("white noise", "floor_hz_rt_hz"): 0.0098,                # measured 0.004868 of 3.22749 Hz / sqrt (Hz)
    ("white noise and a pilot", "floor_hz_rt_hz"): 0.0102,    # measured 0.005057
    ("white noise and a pilot", "pilot_cn0_db"): 0.0145,      # measured 0.007238 dB of 64.3136
    ("a tone in 1 block of 48", "band_hold_over_mean_db"): 4.8e-7,      # measured 2.352e-07 dB of 10 log10 48: c1 / c in f32
    ("a tone in 1 block of 48", "band_hold_line_hz"): 31.3,   # measured 15.62 Hz: the bin beside 70 000 Hz, a third of 46.875 Hz away
    ("a tone in 1 block of 48", "band_line_hz"): 31.3,        # measured 15.62 Hz
    ("a tone in 1 block of 48", "band_hz"): 0.00026,          # measured 0.00013 Hz of 102.062
}


def figure_cases():
    """-> [(case, figure, truth, mean, peak, bands)]"""
    if "figs" in _CACHE:
        return _CACHE["figs"]
    n, B = 48 * N, 48
    cases = []
    prog = mm.band_noise(n, 30.0, 15000.0, 15000.0, 1)
    for f0 in (19000.0, 19001.5):
        m, p = mm.record_of(prog + mm.tone(n, f0, 7500.0), B)
        tag = "pilot at %.1f" % f0
        cases += [(tag, "pilot_hz", 7500.0, m, p, None), (tag, "pilot_freq_hz", f0, m, p, None), (tag, "mono_hz", 15000.0, m, p, None),
                  (tag, "total_hz", float(np.hypot(15000.0, 7500.0 / np.sqrt(2))), m, p, None)]
    diff = mm.band_noise(n, 23000.0, 37000.0, 10000.0 / np.sqrt(2), 2) + mm.band_noise(n, 39000.0, 53000.0, 10000.0 / np.sqrt(2), 3)
    m, p = mm.record_of(diff, B)
    cases += [("L-R", "stereo_hz", 10000.0, m, p, None), ("L-R", "carrier38_hz", 0.0, m, p, None)]
    m, p = mm.record_of(diff + mm.tone(n, 38000.0, 750.0), B)
    cases += [("L-R with a 38 kHz leak", "stereo_hz", 10000.0, m, p, None), ("L-R with a 38 kHz leak", "carrier38_hz", 750.0, m, p, None)]
    m, p = mm.record_of(mm.band_noise(n, 55000.0, 59000.0, 2000.0, 4), B)
    cases += [("RDS-shaped band", "rds_hz", 2000.0, m, p, None)]
    t = np.arange(n) / mm.FM_RATE
    sub = 7500.0 * np.cos(2 * np.pi * 67000.0 * t + 5.0 * np.sin(2 * np.pi * 1000.0 * t))
    m, p = mm.record_of(sub, B)
    cases += [("FM sub-carrier at 67 kHz", "aux_hz", 7500.0 / np.sqrt(2), m, p, None), ("FM sub-carrier at 67 kHz", "band_hz", 7500.0 / np.sqrt(2), m, p, [(59000.0, 75000.0)])]
    rng = np.random.default_rng(5)
    white = 1000.0 * rng.standard_normal(n)
    density = 1000.0 ** 2 / (mm.FM_RATE / 2)
    m, p = mm.record_of(white, B)
    cases += [("white noise", "floor_hz_rt_hz", float(np.sqrt(density)), m, p, None)]
    m, p = mm.record_of(white + mm.tone(n, 19000.0, 7500.0), B)
    cases += [("white noise and a pilot", "floor_hz_rt_hz", float(np.sqrt(density)), m, p, None),
              ("white noise and a pilot", "pilot_cn0_db", float(10 * np.log10(7500.0 ** 2 / 2 / density)), m, p, None)]
    burst = np.zeros(n)
    burst[5 * N:6 * N] = mm.tone(N, 70000.0, 1000.0)
    m, p = mm.record_of(burst + 1e-3 * white, B)
    band = [(69000.0, 71000.0)]
    cases += [("a tone in 1 block of 48", "band_hold_over_mean_db", float(10 * np.log10(48.0)), m, p, band),
              ("a tone in 1 block of 48", "band_hold_line_hz", 70000.0, m, p, band), ("a tone in 1 block of 48", "band_line_hz", 70000.0, m, p, band),
              ("a tone in 1 block of 48", "band_hz", 1000.0 / np.sqrt(2) / np.sqrt(48.0), m, p, band)]
    _CACHE["figs"] = cases
    return cases


def figure_of(fmx_amd, name, m, p, bands):
    figs = fmx_amd.mpx_figures(m, p, rate_hz=mm.FM_RATE, hz_per_unit=1.0, dc_guard_hz=30, line_half_hz=250, bands=bands)
    v = figs[name]
    return v[0] if isinstance(v, list) else v


def test_figures_against_what_the_generator_sent(fmx_amd):
    missing, failed = [], []
    for case, name, truth, m, p, bands in figure_cases():
        got = figure_of(fmx_amd, name, m, p, bands)
        err = abs(got - truth)
        bound = FIGURE_BOUNDS.get((case, name))
        print("[%s] %s: truth %.6g, got %.6g, error %.4g, bound %s" % (case, name, truth, got, err, "%.4g" % bound if bound is not None else "none"))
        if bound is None:
            missing.append((case, name))
        elif not err <= bound:
            failed.append((case, name, err, bound))
    assert not missing and not failed, (missing, failed)


def test_what_cannot_be_formed_reads_minus_infinity(fmx_amd):
    m = np.ones(BINS, np.float32)
    f = fmx_amd.mpx_figures(m, None, rate_hz=48000, bands=[(0.0, 1.0), (100.0, 24000.0)])
    assert f["rds_hz"] == -np.inf and f["aux_hz"] == -np.inf and f["stereo_hz"] == -np.inf and f["carrier38_hz"] == -np.inf
    assert f["mono_hz"] > 0 and f["pilot_hz"] > 0 and np.isfinite(f["floor_hz_rt_hz"])
    assert f["band_hz"][0] == -np.inf and f["band_hz"][1] > 0                       # (no usable bin in [0, 1] Hz)
    assert f["band_hold_line_hz"] == [-np.inf, -np.inf] and f["band_hold_over_mean_db"] == [-np.inf, -np.inf]      # (needs peak)
    z = fmx_amd.mpx_figures(np.zeros(BINS, np.float32), np.zeros(BINS, np.float32), bands=[(1000.0, 2000.0)])
    assert z["pilot_freq_hz"] == -np.inf and z["pilot_cn0_db"] == -np.inf and z["band_hold_over_mean_db"] == [-np.inf] and z["total_hz"] == 0.0
    # membership in integers: at 192 kS/s bin 320 lies at 15 000 Hz exactly and belongs to [.., 15 000]; bin 0 and the bins below the guard to no band
    one = np.zeros(BINS, np.float32); one[320] = 1.0
    assert fmx_amd.mpx_figures(one)["mono_hz"] > 0 and fmx_amd.mpx_figures(one, bands=[(15000.000001, 16000.0)])["band_hz"] == [0.0]
    dc = np.zeros(BINS, np.float32); dc[0] = 1.0
    assert fmx_amd.mpx_figures(dc, dc_guard_hz=0)["total_hz"] == 0.0
    lowest = np.zeros(BINS, np.float32); lowest[1] = 1.0
    assert fmx_amd.mpx_figures(lowest, dc_guard_hz=46)["total_hz"] > 0 and fmx_amd.mpx_figures(lowest, dc_guard_hz=47)["total_hz"] == 0.0


def test_every_refusal_names_its_argument(fmx_amd):
    m = np.ones(BINS, np.float32)
    bad = m.copy(); bad[7] = -1.0
    nan = m.copy(); nan[9] = np.nan
    for kw, word in ((dict(rate_hz=7999), "rate_hz"), (dict(rate_hz=1000001), "rate_hz"), (dict(hz_per_unit=0.0), "hz_per_unit"),
                     (dict(hz_per_unit=float("inf")), "hz_per_unit"), (dict(hz_per_unit=float("nan")), "hz_per_unit"),
                     (dict(dc_guard_hz=-1), "dc_guard_hz"), (dict(dc_guard_hz=1001), "dc_guard_hz"), (dict(line_half_hz=49), "line_half_hz"),
                     (dict(line_half_hz=1001), "line_half_hz"), (dict(bands=[(0.0, 1.0)] * 17), "n_bands"), (dict(bands=[(5.0, 5.0)]), "bands"),
                     (dict(bands=[(-1.0, 5.0)]), "bands"), (dict(bands=[(1.0, 96000.5)]), "bands"), (dict(bands=[(1.0, float("nan"))]), "bands")):
        with pytest.raises(fmx_amd.FmxError) as e:
            fmx_amd.mpx_figures(m, m, **kw)
        assert word in str(e.value), (kw, str(e.value))
    for mean, peak, word in ((bad, None, "mean"), (nan, None, "mean"), (m, bad, "peak"), (m, nan, "peak")):
        with pytest.raises(fmx_amd.FmxError) as e:
            fmx_amd.mpx_figures(mean, peak)
        assert word in str(e.value)
    L, fx = fmx_amd.load_library(), fmx_amd.fmx
    cfg = fx.FmxMpxFind(4, 192000, 1.0, 30, 250, None, 0, 0)
    out = fx.FmxMpxFigs()
    import ctypes as C
    assert L.fmx_mpx_figures(C.byref(cfg), m.ctypes.data, None, C.byref(out)) != 0 and b"struct_size" in L.fmx_last_error()


def build_demo(fmx_amd, exe):
    host = os.path.join(ROOT, "sdr-j-fm_amd", "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + host, os.path.join(ROOT, "tests", "mpx_demo", "mpx_adapter_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])


def test_cpp_adapter_builds_and_forms_figures_without_a_device(fmx_amd, tmp_path):
    """host/fm_processor_adapter.h's four methods under -Wall -Werror, in the demo of tests/mpx_demo.  mpxFigures needs no device; without one the demo
    then reports ok 0 and the library's text.  (What it writes with a device is checked in tests/test_gpu_mpx_spectrum.py.)"""
    exe, fin, fout = str(tmp_path / "mpx_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "mpx.bin")
    build_demo(fmx_amd, exe)
    mm.fm_iq(mm.noise_mpx(3 * 16384 // 12, 0, oversample=12), 2304000).tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    assert lines and lines[0].startswith("figures 1 pilot_freq 18984.375")      # (bins 400 .. 410 of a flat record: bin 405), lines
    if out.returncode == 3:
        assert lines[1].startswith("ok 0 error"), lines
    else:
        assert out.returncode == 0 and lines[-1].startswith("records "), lines

"""CPU checks of the spectrum meter (sdr-j-fm_amd/csrc/fmx_spec.h): the grid's bookkeeping against a sample-by-sample count; the
survey's stage functions and the meter's fold compiled for the host and driven launch by launch, thread by thread (tests/spec_check.cpp,
"kernel_form") against the float64 model of tests/spec_model.py; the detector against seeded defects; the figures through the C export (which needs
no device) against what a numpy generator sent.

The spectrum comparisons' signal is survey_model.spectrum_signal: the bound is on every bin's RELATIVE error, so every bin needs power that is no
accident -- the pedestal of that signal gives it; test_kernel_form_against_the_float64_model checks that it does."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import spec_model as pm
import survey_model as sm
import wideband_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = pm.N
RATE = 2304000


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("spec")
    exe = str(d / "spec_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "spec_check.cpp")])

    def rows(path):
        raw = np.fromfile(path, np.float32).reshape(-1, 1 + 2 * N)
        return {int(row[0]): (row[1:1 + N], row[1 + N:]) for row in raw}

    class Check:
        @staticmethod
        def spectrum(x, B, S, cuts=(), on_call=0, scratch=2):
            """-> {record index: (mean, peak)} of the records delivered, as they stood in the ring behind the call that completed them"""
            fi, fo = str(d / "in.bin"), str(d / "out.bin")
            np.asarray(x, np.complex64).tofile(fi)
            subprocess.check_call([exe, "spectrum", fi, fo, str(B), str(S), str(on_call), str(scratch)] + [str(c) for c in cuts])
            return rows(fo)

        @staticmethod
        def fold(p, B, first=0, chunk=1 << 30):
            fi, fo = str(d / "p.bin"), str(d / "fold.bin")
            np.asarray(p, np.float32).tofile(fi)
            subprocess.check_call([exe, "fold", fi, fo, str(B), str(first), str(chunk)])
            return rows(fo)

        @staticmethod
        def lines(mode, quads):
            out = subprocess.run([exe, mode] + [str(v) for q in quads for v in q], capture_output=True, text=True, check=True).stdout
            return out.splitlines()
    return Check


_SIGNAL = {}


def signal():
    """The spectrum comparisons' stream (10 blocks of 4096 and 100 samples), as the exact f32 values the library converts to."""
    if "x" not in _SIGNAL:
        _SIGNAL["x"] = wm.convert(sm.to_raw(sm.spectrum_signal(2, sm.stream_length(1)), 0), 0)
    return _SIGNAL["x"]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------------
def piece_of(line):
    b0, blocks, fill, fill_after, append, carry_src, phase, record0, records = (int(v) for v in line.split())
    return dict(b0=b0, blocks=blocks, fill=fill, fill_after=fill_after, append=append, carry_src=carry_src, phase=phase, record0=record0, records=records)


def walk(check, g_start, S, B, calls):
    """spec::piece for consecutive calls from g_start against the count"""
    grid = pm.BruteGrid(g_start, S, B)
    want, quads = [], []
    for n in calls:
        w, g0 = grid.call(n)
        want.append(w)
        quads.append((g0, n, S, B))
    got = [piece_of(l) for l in check.lines("plan", quads)]
    assert len(got) == len(want)
    for q, g, (blocks, fill, fill_after, append, src, phase, record0, records) in zip(quads, got, want):
        assert (g["blocks"], g["fill"], g["fill_after"], g["append"], g["phase"], g["record0"], g["records"]) == \
            (blocks, fill, fill_after, append, phase, record0, records), (q, g)
        assert g["b0"] == record0 * B + phase, (q, g)
        if src is not None:
            assert g["carry_src"] == src, (q, g)
    return got


def test_the_plan_against_a_brute_force_count(check):
    rng = np.random.default_rng(7)
    for S, B in ((1, 3), (2, 2), (3, 2)):
        P = N * S
        # n = 1 repeated across a block end, n < 4096 repeated, calls ending exactly on a block end and on a period end, random lengths
        calls = [N - 2, 1, 1, 1, 1, 1000, 1000, 1000, 1000, 1000]
        pos = sum(calls)
        calls.append((-(pos - N)) % P or P)                   # ends exactly on a block end
        pos += calls[-1]
        assert pos % P == N % P
        calls.append(P - N if S > 1 else P)                   # ends exactly on a period end
        calls += [int(v) for v in rng.integers(1, 2 * P, 6)] + [1, 1, N, P, 2 * P + 17]
        walk(check, 0, S, B, calls)
        g_far = ((1 << 32) // (P * B) + 1) * P * B            # g beyond 2^32, at a record's first sample
        walk(check, g_far, S, B, calls)


def test_at_every_1_the_plan_is_the_surveys(check, tmp_path):
    """S = 1: blocks, fill, phase, record0 and records are survey::plan's (tests/survey_check.cpp plan) for the same stream position."""
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "survey_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "survey_check.cpp")])
    quads_spec, quads_sv = [], []
    for B in (1, 3, 4096):
        for g0 in (0, 1, N - 1, N, 5 * N + 77, (1 << 32) + 12345):
            for n in (1, 2, N - 1, N, N + 1, 3 * N + 17):
                quads_spec.append((g0, n, 1, B))
                quads_sv.append((g0 % N, n, g0 // N, B))
    got = [piece_of(l) for l in check.lines("plan", quads_spec)]
    out = subprocess.run([exe, "plan"] + [str(v) for q in quads_sv for v in q], capture_output=True, text=True, check=True).stdout
    sv = [tuple(int(v) for v in l.split()) for l in out.splitlines()]
    assert len(got) == len(sv) == len(quads_spec)
    for q, g, (blocks, fill, phase, record0, records) in zip(quads_spec, got, sv):
        assert (g["blocks"], g["fill_after"], g["phase"], g["record0"], g["records"]) == (blocks, fill, phase, record0, records), (q, g)
        assert g["fill"] == q[0] % N


def test_the_chunks_cover_every_block_once_within_the_cap(check):
    cap = 16384                                               # spec::SCRATCH_BLOCKS: 256 MiB of 16 KB blocks
    quads = [(streams, scratch, blocks, carries) for streams in (1, 2, 3, 64, 4096, 16384, 16385, 40000) for scratch in (1, 2, 7, 600, cap)
             for blocks in (0, 1, 5, 57) for carries in (0, 1) if streams * blocks <= 2000 * scratch]          # (at most some thousand launches a case)
    lines = check.lines("launches", quads)
    it = iter(lines)
    for streams, scratch, blocks, carries in quads:
        seen = np.zeros(streams, np.int64)                    # blocks visited per stream, which must arrive in order
        carried = np.zeros(streams, np.int64)
        for line in it:
            if line == "end":
                break
            j0, gn, done, nb, wc = (int(v) for v in line.split())
            assert gn * max(nb, 1) <= max(scratch, gn) and (gn <= scratch or scratch < 1) and gn * nb * N * 4 <= 256 << 20
            assert np.all(seen[j0:j0 + gn] == done)
            seen[j0:j0 + gn] += nb
            carried[j0:j0 + gn] += wc
            assert not wc or done + nb == blocks              # the carry is written behind the stream's last block
        assert np.all(seen == blocks) and np.all(carried == carries), (streams, scratch, blocks, carries)


def test_first_block_and_delivery_rules(check):
    for g, S, B, r in ((0, 1, 2, 0), (1, 1, 2, 0), (1, 1, 2, 1), (N, 1, 2, 0), (N + 1, 3, 2, 0), (3 * N, 3, 2, 1), (3 * N + 1, 3, 2, 1), ((1 << 33) + 5, 16, 4, 40000)):
        first, deliv, end = (int(v) for v in check.lines("rules", [(g, S, B, r)])[0].split())
        assert first == pm.first_block(g, S) and first * N * S >= g and (first == 0 or (first - 1) * N * S < g)      # the first block at or behind g
        assert deliv == (1 if r * B >= first else 0)
        assert end == N * S * ((r + 1) * B - 1) + N


# ---- the stage functions and the fold on the host ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(1, 1), (2, 1), (3, 1), (2, 3)])
def test_kernel_form_against_the_float64_model(check, B, S):
    x = signal()
    idx, M64, K64 = pm.records64(x, B, S)
    _, M32, K32 = pm.records32(x, B, S)
    assert len(idx) == pm.n_blocks(len(x), S) // B >= 2
    # the signal has real power in every bin: the weakest bin of any record within 80 dB of the strongest (spectrum_signal: about 60 dB)
    assert M64.min() > 1e-8 * M64.max() and K64.min() > 1e-8 * K64.max()
    whole = check.spectrum(x, B, S, scratch=64)
    cut = check.spectrum(x, B, S, sm.call_cuts(1), scratch=2)
    # (at most two blocks per launch, one sample in one call.  A call that completes more than four records leaves the last four: B = 1)
    assert set(cut) <= set(idx) and (sorted(cut) == idx if B > 1 else len(cut) >= 6) and max(cut) == idx[-1]
    idx = sorted(cut)
    M64, K64, M32, K32 = (v[idx] for v in (M64, K64, M32, K32))
    for r, (m, k) in whole.items():                           # however the stream is cut, and the call into chunks: the same bits
        assert same_bits(m, cut[r][0]) and same_bits(k, cut[r][1]), r
    lw, lm = sm.levels(M64, M32)
    kw, km = sm.levels(K64, K32)
    print()
    ok, rw, rm = sm.check_spectrum("kernel_form mean, B = %d, S = %d" % (B, S), np.stack([cut[r][0] for r in idx]), M64, lw, lm)
    assert ok, (rw, rm)
    ok, rw, rm = sm.check_spectrum("kernel_form peak, B = %d, S = %d" % (B, S), np.stack([cut[r][1] for r in idx]), K64, kw, km)
    assert ok, (rw, rm)


def test_switched_on_in_mid_stream(check):
    """The meter switched on by the call that begins at sample 2500 (inside block 0): the first block is 1, and with B = 2 the first record is 1."""
    x = signal()
    B, S = 2, 1
    cuts = sm.call_cuts(1)
    assert sum(cuts[:2]) == 2500
    got = check.spectrum(x, B, S, cuts, on_call=2)
    idx, M64, K64 = pm.records64(x, B, S, first=pm.first_block(2500, S))
    assert idx == [1, 2, 3, 4] and sorted(got) == idx
    whole = check.spectrum(x, B, S, scratch=64)
    for r in idx:
        assert same_bits(got[r][0], whole[r][0]) and same_bits(got[r][1], whole[r][1])


def test_the_fold_is_the_sequential_f32_sum_however_it_is_chunked(check):
    p = pm.block_powers32(signal())
    for B, first in ((3, 0), (2, 1), (1, 4)):
        idx, mean, peak = pm.records_from_powers32(p, B, first)
        for chunk in (1, 2, 7, 1 << 30):
            got = check.fold(p, B, first, chunk)
            keep = []                                         # a call's records: the last four it completes, those delivered
            for b in range(0, len(p), chunk):
                done = list(range(b // B, min(b + chunk, len(p)) // B))[-pm.RING:]
                keep += [r for r in done if r * B >= first]
            assert sorted(got) == keep and set(keep) <= set(idx) and len(keep) >= min(len(idx), pm.RING)
            for r in keep:
                i = idx.index(r)
                assert same_bits(got[r][0], mean[i]) and same_bits(got[r][1], peak[i]), (B, first, chunk, r)


# ---- the detector ------------------------------------------------------------------------------------------------------------------------------
def test_the_detector_catches_seeded_defects(check):
    """Each defect must break the check that guards against it, on inputs that make it visible (shown per defect)."""
    x = signal()
    B, S = 2, 3
    idx, M64, K64 = pm.records64(x, B, S)
    p = pm.block_powers32(x, S)
    _, good_m, good_k = pm.records_from_powers32(p, B)
    kf = check.spectrum(x, B, S)
    lw, lm = sm.levels(M64, good_m, np.stack([kf[r][0] for r in idx]))
    kw, km = sm.levels(K64, good_k, np.stack([kf[r][1] for r in idx]))
    print("\n[levels, B = %d, S = %d] mean: worst %.3e, median %.3e; peak: worst %.3e, median %.3e" % (B, S, lw, lm, kw, km))
    assert sm.check_spectrum("no defect, mean", good_m, M64, lw, lm)[0] and sm.check_spectrum("no defect, peak", good_k, K64, kw, km)[0]

    # a block left out of a record (the block's power is that of its neighbours: it is missed)
    left_out = p.copy()
    left_out[1] = 0.0
    assert np.median(p[1] / p[0]) > 0.1
    assert not sm.check_spectrum("a block left out", pm.records_from_powers32(left_out, B)[1], M64, lw, lm)[0]

    # peak filled with the mean (the blocks of a record differ in level: the envelope of spectrum_signal)
    assert np.median(np.abs(good_k - good_m) / good_k) > 0.05
    assert not sm.check_spectrum("peak filled with the mean", good_m, K64, kw, km)[0]

    # the grid off by one sample at S = 3 (the signal changes from sample to sample: chirp and noise)
    shifted = sm.block_powers32(np.concatenate([x[N * S * b + 1:N * S * b + 1 + N] for b in range(p.shape[0] - 1)]))
    assert not sm.check_spectrum("the grid off by one sample", pm.records_from_powers32(shifted, B)[1][:1], M64[:1], lw, lm)[0]

    # a stale carry sample: a call boundary inside block 1 whose carry kept, at one position, the sample of the block before.  The stream must change
    # inside the block for that to show: the two samples differ by more than a thousandth of full scale
    pos = N * S + 1234
    assert abs(x[pos] - x[pos - N * S]) > 1e-3
    stale = x.copy()
    stale[pos] = x[pos - N * S]
    assert not sm.check_spectrum("a stale carry sample", pm.records32(stale, B, S)[1], M64, lw, lm)[0]

    # a block in front of the first-block rule let in: switched on at sample 1 (inside block 0) the stream's first block is 1 and record 0 must not
    # arrive.  The detector is the list of indices; the input that shows it is a switch that is no record boundary
    first = pm.first_block(1, S)
    assert first == 1 and first % B != 0
    assert pm.records64(x, B, S, first=first)[0] == idx[1:] != pm.records64(x, B, S, first=0)[0]
    assert sorted(check.spectrum(x, B, S, [1, len(x) - 1], on_call=1)) == idx[1:]

    # two blocks swapped in the sum: the mean in float64 is the same, so the bound cannot see it; the detector is the bit comparison of the fold with the
    # sequential f32 sum, on powers whose f32 sum depends on the order: (1 + e) + e = 1 in f32 for e = 2^-24, (e + e) + 1 = 1 + 2^-23
    e = np.float32(2.0 ** -24)
    q = np.stack([np.full(N, 1.0, np.float32), np.full(N, e, np.float32), np.full(N, e, np.float32)])
    swapped = q[[1, 2, 0]]
    a, b = pm.records_from_powers32(q, 3)[1], pm.records_from_powers32(swapped, 3)[1]
    assert not same_bits(a, b)                                                       # the inputs make the order visible
    got = check.fold(q, 3)[0][0]
    assert same_bits(got, a[0]) and not same_bits(got, b[0])
    benign = np.stack([np.full(N, v, np.float32) for v in (1.0, 2.0, 4.0)])         # (exact sums: no order to see)
    assert same_bits(pm.records_from_powers32(benign, 3)[1], pm.records_from_powers32(benign[[1, 2, 0]], 3)[1])


# ---- the figures -------------------------------------------------------------------------------------------------------------------------------
B_FIG = 16
# Asserted bounds: twice the error measured here against the generator's truth (DESIGN.md 4.15 lists both).
BOUNDS = {
    "tone obw_hz": 2 * 386.712, "tone obw edges": 2 * 202.652, "tone channel_db": 2 * 1.7406e-06, "tone centroid_hz": 2 * 316.602, "tone xdb_hz": 2 * 12250.0,
    "noise obw_hz": 2 * 4891.78, "noise channel_db": 2 * 7.91973e-06, "noise centroid_hz": 2 * 392.648,
    "adj_db": 2 * 0.274173, "offset centroid_hz": 2 * 150.843, "dc channel_db guarded": 2 * 1.46856e-05,
}


def within(name, err):
    print("[figures] %-24s error %.6g (bound %.6g)" % (name, err, BOUNDS[name]))
    return err <= BOUNDS[name]


def figs_of(fmx_amd, x, **kw):
    mean, peak = pm.record_of(x, B_FIG)
    return fmx_amd.spectrum_figures(mean, peak, rate_hz=RATE, **kw), mean, peak


def test_figures_of_a_tone_modulated_carrier(fmx_amd):
    """1 kHz at +-75 kHz: the 99 % bandwidth against the value computed from the carrier's Bessel lines."""
    n = N * B_FIG
    x = pm.fm_tone(n, RATE, 0, 0.5, 1000.0, 75000.0) + pm.white(n, 1e-8, seed=1)
    f, _, _ = figs_of(fmx_amd, x)
    lo, hi = pm.bessel_obw(75.0, 1000.0, 0.99)
    print("\n[tone] obw %.1f Hz (Bessel lines: %.1f .. %.1f), xdb %.1f, centroid %.2f, channel %.4f dB" % (f["obw_hz"], lo, hi, f["xdb_hz"], f["centroid_hz"], f["channel_db"]))
    assert within("tone obw_hz", abs(f["obw_hz"] - (hi - lo)))
    assert within("tone obw edges", max(abs(f["obw_lower_hz"] - lo), abs(f["obw_upper_hz"] - hi)))
    assert within("tone channel_db", abs(f["channel_db"] - 10 * np.log10(0.25 * N)))
    assert within("tone centroid_hz", abs(f["centroid_hz"]))
    # the x dB bandwidth of such a carrier: its lines fall off steeply beyond the deviation -- Carson's 2 (75 + 1) kHz is the yardstick
    assert within("tone xdb_hz", abs(f["xdb_hz"] - 152000.0))


def test_figures_of_a_noise_like_programme(fmx_amd):
    """A carrier modulated by low-pass noise of 19 kHz rms deviation: in the quasi-static limit its spectrum is the Gaussian density of the
    instantaneous frequency, whose central 99 % is 2 * 2.5758 sigma wide."""
    n = N * B_FIG
    x = pm.fm_noise(n, RATE, 0, 0.3, 19000.0, seed=3) + pm.white(n, 1e-8, seed=2)
    f, _, _ = figs_of(fmx_amd, x)
    print("\n[noise] obw %.1f Hz (quasi-static %.1f), centroid %.2f, channel %.4f dB" % (f["obw_hz"], 2 * 2.5758 * 19000.0, f["centroid_hz"], f["channel_db"]))
    assert within("noise obw_hz", abs(f["obw_hz"] - 2 * 2.5758 * 19000.0))
    assert within("noise channel_db", abs(f["channel_db"] - 10 * np.log10(0.09 * N)))
    assert within("noise centroid_hz", abs(f["centroid_hz"]))


def test_adjacent_channels(fmx_amd):
    """A station 20 dB up at +200 kHz and one 10 dB down at -100 kHz, all three noise-modulated (sigma 8 kHz: symmetric, inside +-50 kHz).  With a raster
    of 100 kHz the +-100 kHz windows overlap: the window about -200 kHz holds the lower half of the -100 kHz station (0.05), the one about -100 kHz that
    station and the channel's lower half (0.1 + 0.5), the one about +100 kHz the channel's upper half and the strong station's lower half (0.5 + 50),
    the one about +200 kHz the strong station (100)."""
    n = N * B_FIG
    a = 0.03
    x = pm.fm_noise(n, RATE, 0, a, 8000.0, seed=5) + pm.fm_noise(n, RATE, 200000, 10 * a, 8000.0, seed=6) + \
        pm.fm_noise(n, RATE, -100000, a / np.sqrt(10.0), 8000.0, seed=7) + pm.white(n, 1e-10, seed=4)
    f, _, _ = figs_of(fmx_amd, x, raster_hz=100000)
    # channel_db itself holds the halves of both neighbours' ... no: |f| <= 100 kHz holds the -100 kHz station's upper half only
    truth_ch = 1.0 + 0.05
    truth = [10 * np.log10(v / truth_ch) for v in (0.05, 0.6, 50.5, 100.0)]
    print("\n[adjacent] adj_db %s, truth %s" % (["%.3f" % v for v in f["adj_db"]], ["%.3f" % v for v in truth]))
    assert within("adj_db", max(abs(g - t) for g, t in zip(f["adj_db"], truth)))
    # a channel at the band's edge: the windows that leave |f| <= rate / 2 - 50 kHz read -inf
    g = fmx_amd.spectrum_figures(*pm.record_of(x, B_FIG), rate_hz=RATE, centre_hz=900000, raster_hz=100000)
    assert g["adj_db"][2] > -np.inf and g["adj_db"][3] == -np.inf and g["adj_db"][0] > -np.inf


def test_a_carrier_offset_reads_in_the_centroid(fmx_amd):
    n = N * B_FIG
    x = pm.fm_noise(n, RATE, 403000, 0.3, 3000.0, seed=8) + pm.white(n, 1e-8, seed=9)
    f, _, _ = figs_of(fmx_amd, x, centre_hz=400000)
    print("\n[offset] centroid %.2f Hz" % f["centroid_hz"])
    assert within("offset centroid_hz", abs(f["centroid_hz"] - 3000.0))


def test_a_dc_spike_with_and_without_the_guard(fmx_amd):
    """A channel 50 kHz above a DC spike 6 dB stronger than itself: without the guard channel_db reads the spike (10 log10 5 = 7 dB high); with a guard
    of 3 kHz it reads the channel."""
    n = N * B_FIG
    x = pm.fm_noise(n, RATE, 50000, 0.1, 8000.0, seed=10) + 0.2 + pm.white(n, 1e-10, seed=11)
    open_, _, _ = figs_of(fmx_amd, x, centre_hz=50000)
    guarded, _, _ = figs_of(fmx_amd, x, centre_hz=50000, dc_guard_hz=3000)
    print("\n[dc] channel_db %.3f without the guard, %.3f with it; centroid %.1f / %.1f" % (open_["channel_db"], guarded["channel_db"], open_["centroid_hz"], guarded["centroid_hz"]))
    assert abs(open_["channel_db"] - 10 * np.log10(0.05 * N)) < 0.1 and open_["centroid_hz"] < -35000
    assert within("dc channel_db guarded", abs(guarded["channel_db"] - 10 * np.log10(0.01 * N)))
    assert abs(guarded["centroid_hz"]) < 1000


def test_a_callers_mask_just_met_and_just_violated(fmx_amd):
    """An exact record: a flat channel of 1 per bin inside +-100 kHz and a spur; the level of the spur relative to the channel is known exactly, and a
    mask 0.01 dB above it is met by 0.01 dB, one 0.01 dB below it violated by 0.01 dB -- at the spur.  rbw_hz = 1: a bin alone."""
    kp = np.arange(N)
    kp[kp >= N // 2] -= N
    f_hz = kp * (RATE / N)
    mean = np.where(np.abs(kp * RATE) <= 100000 * N, 1.0, 1e-9).astype(np.float32)
    peak = mean.copy()
    k_spur = int(round(150000 * N / RATE))
    peak[k_spur] = 0.02
    rel = 10 * np.log10(float(peak[k_spur]) / float(np.sum(mean[np.abs(kp * RATE) <= 100000 * N].astype(np.float64))))
    for delta in (0.01, -0.01):
        g = fmx_amd.spectrum_figures(mean, peak, rate_hz=RATE, rbw_hz=1, mask=[(120000, rel + delta), (200000, rel + delta)])
        assert abs(g["mask_margin_db"] - delta) < 1e-9 and g["mask_worst_hz"] == f_hz[k_spur], (delta, g)
    # a sloped mask: the limit at the spur is interpolated linearly in dB between the break points
    f_spur = f_hz[k_spur]
    g = fmx_amd.spectrum_figures(mean, peak, rate_hz=RATE, rbw_hz=1, mask=[(120000, rel + 10.0), (f_spur + 30000, rel - 5.0)])
    want = 10.0 - 15.0 * (f_spur - 120000) / (f_spur + 30000 - 120000)
    assert abs(g["mask_margin_db"] - want) < 1e-9 and g["mask_worst_hz"] == f_spur
    # a wider resolution bandwidth sums the neighbours: three bins of 1e-9 beside the spur change nothing visible, five bins of the channel do
    g = fmx_amd.spectrum_figures(mean, peak, rate_hz=RATE, rbw_hz=2500, mask=[(0, 0.0), (50000, 0.0)])
    assert abs(g["mask_margin_db"] - (0.0 - 10 * np.log10(5.0 / float(np.sum(mean[np.abs(kp * RATE) <= 100000 * N].astype(np.float64)))))) < 1e-9
    # without peak or without a mask the margin is not formed
    assert fmx_amd.spectrum_figures(mean, None, rate_hz=RATE, mask=[(0, 0.0), (50000, 0.0)])["mask_margin_db"] == -np.inf
    assert fmx_amd.spectrum_figures(mean, peak, rate_hz=RATE)["mask_margin_db"] == -np.inf


def test_refusals(fmx_amd):
    M = fmx_amd.fmx
    mean = np.ones(N, np.float32)
    L = fmx_amd.load_library()

    def refused(expect, mean=mean, peak=None, **kw):
        with pytest.raises(fmx_amd.FmxError) as e:
            fmx_amd.spectrum_figures(mean, peak, **kw)
        assert e.value.code == M.FMX_E_INVALID and expect in str(e.value), (expect, str(e.value))

    assert fmx_amd.spectrum_figures(mean)["channel_db"] > 0
    refused("rate_hz", rate_hz=999)
    refused("rate_hz", rate_hz=100000001)
    refused("centre_hz", centre_hz=1152001)
    refused("raster_hz", raster_hz=49999)
    refused("raster_hz", raster_hz=1000001)
    refused("dc_guard_hz", dc_guard_hz=-1)
    refused("dc_guard_hz", dc_guard_hz=100000)
    for v in (0.0, 1.0, -0.5, np.nan):
        refused("obw_fraction", obw_fraction=v)
    for v in (0.0, -3.0, np.inf, np.nan):
        refused("x_db", x_db=v)
    refused("rbw_hz", rbw_hz=0)
    refused("mask", mask=[(0, 0.0)])
    refused("mask", mask=[(10000, 0.0), (10000, -10.0)])
    refused("mask", mask=[(-1, 0.0), (10000, -10.0)])
    refused("mask", mask=[(0, np.nan), (10000, -10.0)])
    refused("mask", mask=[(0, 0.0), (np.inf, -10.0)])
    for v in (-1e-9, np.nan, np.inf):
        bad = mean.copy()
        bad[1000] = v
        refused("mean", mean=bad)
        refused("peak", peak=bad)
    import ctypes as C
    cfg = M.FmxSpectrumFind(8, RATE, 0, 100000, 0, 10000, 0.99, 26.0, None, 0, 0)
    out = M.FmxSpectrumFigs()
    assert L.fmx_spectrum_figures(C.byref(cfg), mean.ctypes.data, None, C.byref(out)) == M.FMX_E_INVALID
    assert b"struct_size" in L.fmx_last_error()
    # what cannot be formed reads -inf: an all-zero record
    z = fmx_amd.spectrum_figures(np.zeros(N, np.float32))
    assert z["channel_db"] == -np.inf and z["obw_hz"] == -np.inf and z["centroid_hz"] == -np.inf and all(v == -np.inf for v in z["adj_db"])


def test_cpp_adapter_builds_and_forms_figures_without_a_device(fmx_amd, tmp_path):
    """host/fm_processor_adapter.h's spectrum methods under -Wall -Werror, in the demo of tests/spec_demo.  spectrumFigures needs no device; without one
    the demo then reports ok 0 and the library's text.  (What it writes with a device is checked in tests/test_gpu_spectrum.py.)"""
    exe, fin, fout = str(tmp_path / "spec_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "spec.bin")
    build_demo(fmx_amd, exe)
    sm.to_raw(signal()[:3 * 16384], 0).tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    assert lines and lines[0].startswith("figures 1 centroid"), lines
    if out.returncode == 3:
        assert lines[1].startswith("ok 0 error"), lines
    else:
        assert out.returncode == 0 and lines[-1].startswith("records "), lines


def build_demo(fmx_amd, exe):
    host = os.path.join(ROOT, "sdr-j-fm_amd", "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + host, os.path.join(ROOT, "tests", "spec_demo", "spec_adapter_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])

"""Stage W's per-sample check without a GPU: that the detector of tests/test_gpu_wideband_edges.py and its shapes can catch what they are
for.  `kernel_form` (the kernel's fast-path arithmetic in f32) stays within check_per_sample for every factor, `advance` equals processing
the samples it skips, seeded faults on the GPU tests' own shapes fail the check, and host/wideband_adapter.h compiles."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_wideband_edges as ge
import wideband_model as wm

N_OUT = 549                                      # two tiles of 256 outputs and a ragged one: the first call of case a


def offsets(K):
    lim = wm.offset_limit(K)
    return [0, -412345, lim - 1, -lim, 733001]


_CASES = {}


def case(K):
    """One stream, five outputs, 549 outputs each: (converted samples, f64 model, f32 restatement, kernel_form).  Computed once per K."""
    if K not in _CASES:
        offs = offsets(K)
        x = wm.convert(ge.edge_signal(K, N_OUT * K, [0] * 5, offs, 1)[0], 0)
        mod = wm.WidebandModel(K, offs)
        ref, ref32 = mod.process(x, with_f32=True)
        form = np.stack([wm.kernel_form(K, f, x, mod.h) for f in offs])
        for v in (x, ref, ref32, form):
            v.setflags(write=False)
        _CASES[K] = (x, ref, ref32, form)
    return _CASES[K]


def fails(tag, got, ref, ref32, **kw):
    with pytest.raises(AssertionError):
        wm.check_per_sample(tag, got, ref, ref32, **kw)
    return True


@pytest.mark.parametrize("K", range(2, 17))
def test_kernel_form_against_the_model(K):
    """Folded taps, four accumulators and the table rotator are within the bound the GPU is held to; the ratios are printed."""
    x, ref, ref32, form = case(K)
    print()
    ratio = wm.check_per_sample("kernel_form, K = %d" % K, form, ref, ref32)
    level = max(float(np.max(np.abs(ref32[m] - ref[m])) / np.max(np.abs(ref[m]))) for m in range(len(ref)))
    print("[kernel_form, K = %d] worst ratio %.2f; the restatement's worst sample %.2e of the peak" % (K, ratio, level))


@pytest.mark.parametrize("K", [2, 7, 16])
def test_advance_equals_processing(K):
    """An offset change, 300 outputs that are either processed or skipped with `advance`, another change, 50 outputs: the same to 1e-13."""
    lim = wm.offset_limit(K)
    offs = [0, -412345, lim]
    cuts = [40 * K, 300 * K, 50 * K]
    x = wm.convert(ge.edge_signal(K, sum(cuts), [0] * 3, offs, 1, seed=3)[0], 0)
    a, b, c = x[:cuts[0]], x[cuts[0]:cuts[0] + cuts[1]], x[cuts[0] + cuts[1]:]
    walked, skipped = wm.WidebandModel(K, offs), wm.WidebandModel(K, offs)
    for mod in (walked, skipped):
        mod.process(a, with_f32=True)
        mod.set_offset(1, 733001)
        mod.set_offset(2, -lim)
    walked.process(b, with_f32=True)
    skipped.advance(len(b), b[-16 * K:])
    for mod in (walked, skipped):
        mod.set_offset(0, 250000)
    assert walked.P == skipped.P
    y, y32 = walked.process(c, with_f32=True)
    z, z32 = skipped.process(c, with_f32=True)
    assert np.max(np.abs(y - z)) <= 1e-13 * np.max(np.abs(y))
    assert np.array_equal(y32, z32)
    with pytest.raises(ValueError):
        skipped.advance(K, b[-16 * K:])                                  # shorter than a window: the tail would not be the whole history


# ---- seeded faults --------------------------------------------------------------------------------------------------------------------
def test_seeded_single_sample_passes_the_rms_rule():
    """1e-5 of the peak on one sample of 549 (K = 16, output 1, column 44 of the second tile) passes `rel_rms <= 3 x the restatement's` and
    fails check_per_sample.  (The RMS rule is at its loosest where the restatement's error is largest: on this signal the fault passes it
    from K = 9 on, ratio 2.4 at K = 16, and stands out at K = 2, ratio 5.6.  The per-sample check catches it at every K.)"""
    for K in range(2, 17):
        x, ref, ref32, form = case(K)
        got = form.astype(np.complex128)
        got[1, 300] += 1e-5 * np.max(np.abs(ref[1]))
        e_got, e_f32 = wm.rel_rms(got[1], ref[1]), wm.rel_rms(ref32[1], ref[1])
        print("\n[seeded 1e-5, K = %d] rel_rms %.3e, restatement %.3e (ratio %.2f, the RMS rule allows 3)" % (K, e_got, e_f32, e_got / e_f32))
        if K == 16:
            assert e_got <= 3.0 * e_f32
        assert fails("seeded 1e-5, K = %d" % K, got, ref, ref32)


@pytest.mark.parametrize("K", [2, 16])
def test_seeded_late_rotator(K):
    """The rotator one output late from column 0 of the second tile on."""
    x, ref, ref32, form = case(K)
    offs = offsets(K)
    got = np.stack([wm.kernel_form(K, f, x, wm.taps(K), rot_lag=256) for f in offs])
    assert np.array_equal(got[:, :256], form[:, :256])
    assert np.array_equal(got[0], form[0])                               # offset 0 has no rotation: the fault shows on the others
    assert fails("late rotator, K = %d" % K, got[1:], ref[1:], ref32[1:])


def test_seeded_dropped_last_tap():
    """The tap i = 16 K dropped.  The Blackman window leaves it 4e-5 of the sum at K = 2 and 9e-8 at K = 16, under an f32 sum's rounding:
    the check catches it where it is above the restatement's level (asserted for K <= 4), and no f32 bound can at K = 16."""
    for K in range(2, 17):
        x, ref, ref32, form = case(K)
        h = wm.taps(K).copy()
        weight = abs(float(h[-1]))
        h[-1] = 0.0
        got = np.stack([wm.kernel_form(K, f, x, h) for f in offsets(K)])
        err = max(float(np.max(np.abs(got[m] - ref[m])) / np.max(np.abs(ref[m]))) for m in range(len(ref)))
        print("\n[dropped last tap, K = %d] |h[16 K]| = %.2e, worst sample %.2e of the peak" % (K, weight, err))
        if K <= 4:
            assert fails("dropped last tap, K = %d" % K, got, ref, ref32)


def run_lists(K, plan, start, keep):
    """The run lists of wide_flush for one output, restated with Python integers: per call the runs (first sample, phase in front of it,
    offset), newest first, at most `keep` of them (the oldest are dropped)."""
    T, Rw = wm.n_taps(K), K * wm.NARROW_RATE
    runs, cur, c, per_call = [(0, 0, start % Rw)], start, 0, []
    for nj, want in plan:
        while len(runs) > 1 and runs[-2][0] <= c - (T - 1):
            runs.pop()
        if want != cur:
            nbase, pbase, f = runs[0]
            if nbase == c:
                runs[0] = (nbase, pbase, want % Rw)
            else:
                runs.insert(0, (c, (pbase - ((c - nbase) % Rw) * f) % Rw, want % Rw))
            cur = want
        del runs[keep:]
        per_call.append(list(runs))
        c += nj * K
    return per_call


def by_runs(K, x, plan, start, keep):
    """wide_slow restated in f64: every output of every call of the plan, each sample with the phase of its run."""
    T, Rw = wm.n_taps(K), K * wm.NARROW_RATE
    h = wm.taps(K).astype(np.float64)
    out, j = [], 0
    for (nj, _), runs in zip(plan, run_lists(K, plan, start, keep)):
        for _ in range(nj):
            acc = 0.0
            for i in range(T):
                n = (j + 1) * K - 1 - i
                if n < 0:
                    break
                k = 0
                while k + 1 < len(runs) and n < runs[k][0]:
                    k += 1
                nbase, pbase, f = runs[k]
                p = (pbase - ((n - nbase + 1) % Rw) * f) % Rw
                ang = 2 * np.pi * p / Rw
                acc += h[i] * x[n] * complex(np.float32(np.cos(ang)), np.float32(np.sin(ang)))
            out.append(acc)
            j += 1
    return np.array(out)[None]


def test_seeded_short_run_list():
    """Case c's calls at K = 2 (a change in front of each of 18 calls of K samples: the window of call 16 holds 17 runs), output 0.

    With all 17 runs the restatement of wide_slow equals the model.  With 16 -- the oldest run dropped, its samples given the phase the next
    run's formula gives them -- it STILL equals the model: runs are at least K samples long, so 16 of them cover 16 K of a window's 16 K + 1
    samples, the seventeenth holds one sample, the last in front of run 16, and its phase is that run's `pbase` itself.  The seventeenth entry
    of W_MAX_SEG is never needed for the result, and a list one short cannot be told from a full one by any test.  With 15 runs two and more
    samples get a wrong phase, and check_per_sample fails."""
    K = 2
    plan = ge.c_plan(K)
    calls = [nj for nj, _ in plan]
    start = ge.C_START[0]
    x = wm.convert(ge.edge_signal(K, sum(calls) * K, [0, 0, 0], ge.C_START, 1)[0], 0)
    mod = wm.WidebandModel(K, [start])
    ref, ref32, want, cur = [], [], [], start
    for nj, sets in plan:
        for m, f in sets:
            if m == 0:
                cur = f
        want.append((nj, cur))
        mod.set_offset(0, cur)
        a, b = mod.process(x[sum(c for c, _ in want[:-1]) * K:sum(c for c, _ in want) * K], with_f32=True)
        ref.append(a)
        ref32.append(b)
    ref, ref32 = np.concatenate(ref, axis=1), np.concatenate(ref32, axis=1)
    assert max(len(r) for r in run_lists(K, want, start, 99)) == 17
    print()
    full = by_runs(K, x, want, start, 17)
    assert wm.check_per_sample("17 runs", full, ref, ref32, calls=calls) < 0.01
    one_short = by_runs(K, x, want, start, 16)
    assert np.array_equal(one_short, full)
    assert fails("15 runs", by_runs(K, x, want, start, 15), ref, ref32, calls=calls)


def test_seeded_group_index():
    """A group's second output stored under the first one's index, on case a's stream 0 (five outputs, a NaN-filled buffer)."""
    K = 5
    x, ref, ref32, form = case(K)
    got = form.astype(np.complex128)
    got[0], got[1] = form[1], complex(np.nan, np.nan)
    assert fails("group index", got, ref, ref32)
    got[1] = form[1]                                                     # ... and where the buffer held the right values from an earlier call
    assert fails("group index, stale buffer", got, ref, ref32)


# ---- the C++ wrapper ------------------------------------------------------------------------------------------------------------------
def test_wideband_adapter_compiles_and_reports_a_missing_device(fmx_amd, tmp_path):
    """host/wideband_adapter.h under -Wall -Werror, in the demo of tests/wideband_demo.  Without a device the demo reports ok () == false and the
    library's text; taps () needs none.  (On a machine with a device the object is created and the demo runs through; what it writes is
    checked in tests/test_gpu_wideband_edges.py.)"""
    K, n_out = 5, 40
    exe, fin, fout = str(tmp_path / "wideband_adapter_demo"), str(tmp_path / "wide.f32"), str(tmp_path / "narrow.f32")
    ge.build_demo(fmx_amd, exe)
    ge.edge_signal(K, n_out * K, [0, 0], [0, 100000], 1)[0].tofile(fin)
    out = subprocess.run([exe, fin, fout, str(K), str(7 * K), "1", "733001", "0", "100000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         timeout=120)
    text = out.stdout.decode()
    lines = text.splitlines()
    assert lines and lines[0] == "taps5 81", text
    if out.returncode == 3:
        assert lines[1].startswith("ok 0 error ") and len(lines[1]) > len("ok 0 error "), text
        assert not os.path.exists(fout)
    else:
        assert out.returncode == 0 and lines[1].startswith("ok 1"), text
        assert os.path.getsize(fout) == 2 * n_out * 2 * 4

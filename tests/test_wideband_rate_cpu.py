"""Stage W at any receiver rate without a GPU: which rates are accepted, the prototype bit for bit against the model and its
frequency response, the integer bookkeeping of sdr-j-fm_amd/csrc/fmx_wide_rate.h (tests/wide_rate_check.cpp, a host program without HIP)
against a brute-force count, the argument that a window meets at most 16 call boundaries, and that the per-sample detector of
tests/test_gpu_wideband_rate.py catches what it is for: seeded defects on `kernel_form`, the kernel's own fast-path arithmetic in f32."""
import math
import os
import subprocess

import numpy as np
import pytest

import wideband_model as wm
import wideband_rate_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OUT = 549                                      # two tiles of 256 outputs and a ragged one


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wide_rate") / "wide_rate_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "wide_rate_check.cpp")])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
        return [line.split() for line in out.splitlines()]
    return run


# ---- accepted and refused rates -------------------------------------------------------------------------------------------------------
def create(fmx_amd, rate, **kw):
    """fmx_wideband_create_rate's answer: 0, or the error's (code, text).  The configuration is checked before the device is looked for."""
    try:
        fmx_amd.Wideband(rate_hz=rate, **kw).close()
        return 0, ""
    except fmx_amd.fmx.FmxError as e:
        return e.code, str(e)


@pytest.mark.parametrize("rate", rm.RATES)
def test_listed_rates_are_accepted(fmx_amd, check, rate):
    m = fmx_amd.fmx
    r = rm.Ratio(rate)
    code, text = create(fmx_amd, rate, max_block=r.min_call)
    assert code in (0, m.FMX_E_NO_DEVICE), text                          # (without a device: past every check of the configuration)
    h, L, M = m.wideband_rate_taps(rate)
    assert (L, M, len(h)) == (r.L, r.M, 16 * r.M + 1) and math.gcd(L, M) == 1 and L * rate == M * rm.RO
    row = check("ratio", rate)[0]
    assert row[0] == "ok" and [int(v) for v in row[1:6]] == [r.L, r.M, r.NH, r.NP, r.min_call]
    assert int(row[6]) == 255 * r.M // r.L + 1 + r.NP <= 4352 and r.NP - 1 <= 255  # the image of a tile fits the workgroup's LDS
    # refusals that belong to an accepted rate: a factor beside it, a max_block below ceil (M / L), an offset beyond the limit
    assert create(fmx_amd, rate, factor=0, max_block=r.min_call - 1)[0] == m.FMX_E_INVALID
    assert create(fmx_amd, rate, offset_hz=[r.lim + 1], max_block=4096)[0] == m.FMX_E_INVALID
    cfg = m.FmxWidebandConfig()
    cfg.struct_size, cfg.streams, cfg.factor, cfg.outputs, cfg.max_block = m.C.sizeof(m.FmxWidebandConfig), 1, 2, 1, 4096
    sof = (m.C.c_int32 * 1)(0)
    cfg.stream_of_output = m.C.cast(sof, m.C.POINTER(m.C.c_int32))
    lib, h = m.load_library(), m.C.c_void_p()
    assert lib.fmx_wideband_create_rate(m.C.byref(cfg), rate, m.C.byref(h)) == m.FMX_E_INVALID and b"factor must be 0" in lib.fmx_last_error()


@pytest.mark.parametrize("rate", rm.REFUSED)
def test_other_rates_are_refused(fmx_amd, check, rate):
    m = fmx_amd.fmx
    code, text = create(fmx_amd, rate, max_block=4096)
    assert code == m.FMX_E_INVALID, text
    rule = "above 2304000" if rate <= rm.RO else "multiple of 2304000" if rate % rm.RO == 0 else "at most 16" if rate > 16 * rm.RO else "at most 576"
    assert rule in text, text
    with pytest.raises(m.FmxError) as e:
        m.wideband_rate_taps(rate)
    assert e.value.code == m.FMX_E_INVALID and rule in str(e.value)
    with pytest.raises(m.FmxError) as e:
        m.survey_stations(np.ones(4096, np.float32), rate_hz=rate)
    assert e.value.code == m.FMX_E_INVALID and rule in str(e.value)
    assert check("ratio", rate)[0][0] == "refused"
    with pytest.raises(ValueError):
        rm.Ratio(rate)


# ---- the prototype --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", rm.RATES)
def test_taps_and_response(fmx_amd, rate):
    """The C taps equal the model's bit for bit; droop over +-150 kHz below 0.25 dB, attenuation from 1.152 MHz to Rw / 2 above 80 dB (scanned
    every 2 kHz: a side lobe is M Ro / N_H = 144 kHz wide), every phase sums to 1 within 1e-4.  Measured: 0.221 - 0.224 dB, 82.36 - 82.76 dB,
    7e-9 (36 MS/s) - 1.4e-5 (2.4 MS/s)."""
    r = rm.Ratio(rate)
    h, _, _ = fmx_amd.fmx.wideband_rate_taps(rate)
    H = rm.taps(rate)
    assert np.array_equal(h.view(np.uint32), H.view(np.uint32))
    unit = 20 * math.log10(r.L)                                           # the prototype's DC gain is L: each phase has gain 1
    droop = unit - float(rm.response_db(H, r.M * rm.RO, np.linspace(-150000.0, 150000.0, 61)).min())
    stop = unit - float(rm.response_db(H, r.M * rm.RO, np.arange(1152000.0, rate / 2 + 1.0, 2000.0)).max())
    sums = float(np.max(np.abs(rm.phase_table(rate).astype(np.float64).sum(axis=1) - 1.0)))
    print("\n[prototype, %d S/s] L = %d, M = %d, N_H = %d, NP = %d: droop %.3f dB, attenuation %.2f dB, phase sums within %.1e of 1"
          % (rate, r.L, r.M, r.NH, r.NP, droop, stop, sums))
    assert droop < 0.25 and stop > 80.0 and sums < 1e-4


# ---- the integers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", rm.RATES)
def test_counts_against_brute_force(check, rate):
    """Random cuts of a stream from sample 0 and from a sample beyond 2^32: the header's count, first output, n_j and p_j against an
    accumulator that is stepped output by output (q += M from a sample k M, where exactly k L outputs lie behind) and counts the outputs whose
    newest sample lies in front of each call's end: no floor (X L / M) in it."""
    r = rm.Ratio(rate)
    rng = np.random.default_rng(rate // 1000)
    for start_k in (0, (1 << 32) // r.M + 7):
        g, j, acc = start_k * r.M, start_k * r.L, r.M - 1                # at sample k M exactly k L outputs lie behind: q_j - g L = M - 1
        cuts = [r.min_call, r.min_call, r.min_call + 1] + [int(v) for v in rng.integers(r.min_call, 40 * r.min_call + 3, size=60)]
        want, args, g0 = [], [], g
        for n in cuts:
            first, cnt = None, 0
            while acc < (g0 + n - g) * r.L:                              # output j's newest sample g + acc div L lies in front of the call's end
                if first is None:
                    first = (g + acc // r.L, acc % r.L)
                cnt, j, acc = cnt + 1, j + 1, acc + r.M
            assert cnt >= 1
            want.append((j - cnt, cnt) + first)
            args += [g0, n]
            g0 += n
        got = [tuple(int(v) for v in row) for row in check("count", r.L, r.M, *args)]
        assert got == want
        assert {c for _, c, _, _ in want} <= {n * r.L // r.M for n in cuts} | {n * r.L // r.M + 1 for n in cuts}
        # the model's integers are the same ones
        assert [(r.before(a), r.count(a, n)) for a, n in zip(args[::2], args[1::2])] == [(a, b) for a, b, _, _ in want]
    # outputs of a call's head whose window of NP samples reaches in front of a change
    j0, n_out = r.before(10 ** 6), r.count(10 ** 6, 4000)
    nn, _ = r.samples_of(j0 + np.arange(n_out))
    changes = [10 ** 6, 10 ** 6 - 1, 10 ** 6 - r.NP + 2, 10 ** 6 - r.NP + 1, 10 ** 6 - r.NP, 0, 10 ** 6 - 3 * r.min_call]
    got = [int(row[0]) for row in check("crossing", r.L, r.M, r.NP, *[v for c in changes for v in (j0, n_out, c)])]
    assert got == [int(np.sum(nn - (r.NP - 1) < c)) for c in changes] and got[0] > 0 and got[4] == 0


def test_a_window_meets_at_most_16_call_boundaries(check):
    """A window of NP samples has NP - 1 gaps and calls are at least ceil (M / L) samples long, so it holds at most
    ceil ((NP - 1) / ceil (M / L)) boundaries.  L does not divide M, hence ceil (M / L) >= (M + 1) / L and
    16 ceil (M / L) >= (16 M + 16) / L >= N_H / L: NP <= 16 ceil (M / L) and the count is at most 16 -- 17 runs, W_MAX_SEG, as DESIGN 4.8 has
    it for K.  Walked here for every ratio M / L in lowest terms with 1 < L <= 576 and L < M < 16 L, with the largest window (NP - 1 <= 255:
    the history a stream keeps), the largest image of a tile (<= 4352 float2) and the most outputs whose windows can cross one change
    (<= 256: they lie in the call's first tile)."""
    ratios, max_np, max_bound, max_image, max_cross, misfits = (int(v) for v in check("all")[0])
    print("\n[all ratios] %d ratios: NP <= %d, boundaries in a window <= %d, image <= %d float2, crossing outputs <= %d"
          % (ratios, max_np, max_bound, max_image, max_cross))
    assert ratios > 10 ** 6 and misfits == 0
    assert max_bound == 16 and max_np <= 256 and max_image <= 4352 and max_cross <= 256
    for rate in rm.RATES:
        r = rm.Ratio(rate)
        assert -(-(r.NP - 1) // r.min_call) <= 16 and r.NP <= 16 * r.min_call


# ---- the detector on restated outputs --------------------------------------------------------------------------------------------------
_CASES = {}


def case(rate):
    """One stream, five outputs, 549 outputs each: (converted samples, offsets, f64 model, f32 restatement, kernel_form).  Once per rate."""
    if rate not in _CASES:
        r = rm.Ratio(rate)
        offs = rm.offsets(rate)
        n = -(-N_OUT * r.M // r.L)
        x = wm.convert(rm.signal(rate, n, [0] * 5, offs, 1)[0], 0)
        assert r.before(n) == N_OUT
        ref, ref32 = rm.WidebandRateModel(rate, offs).process(x, with_f32=True)
        form = rm.kernel_form(rate, offs, x)
        for v in (x, ref, ref32, form):
            v.setflags(write=False)
        _CASES[rate] = (x, offs, ref, ref32, form)
    return _CASES[rate]


def caught(tag, got, ref, ref32):
    try:
        wm.check_per_sample(tag, got, ref, ref32)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("rate", rm.RATES)
def test_kernel_form_against_the_model(rate):
    """H x formed first, the folded rotators, two pairs of accumulators and the f64 output rotator are within the bound the GPU is held to:
    every sample of kernel_form within 2 x the plain restatement's worst sample (measured: ratio 1.00 - 1.35 over the nine rates)."""
    x, offs, ref, ref32, form = case(rate)
    print()
    ratio = wm.check_per_sample("kernel_form, %d S/s" % rate, form, ref, ref32)
    level = max(float(np.max(np.abs(ref32[m] - ref[m])) / np.max(np.abs(ref[m]))) for m in range(len(ref)))
    print("[kernel_form, %d S/s] worst ratio %.2f; the restatement's worst sample %.2e of the peak" % (rate, ratio, level))


@pytest.mark.parametrize("rate", rm.RATES)
def test_cuts_and_advance(rate):
    """The model does not depend on how the stream is cut (f64 to 1e-13, the f32 restatement bit for bit), calls of ceil (M / L) samples
    included, and `advance` equals processing the samples it skips."""
    r = rm.Ratio(rate)
    x, offs, ref, ref32, _ = case(rate)
    cut = rm.WidebandRateModel(rate, offs)
    a, b, pos = [], [], 0
    for n in [r.min_call] * 5 + [r.min_call + 1, 7 * r.min_call, len(x)]:
        n = min(n, len(x) - pos)
        assert cut.outputs_for(n) == r.count(pos, n)
        y, y32 = cut.process(x[pos:pos + n], with_f32=True)
        a.append(y)
        b.append(y32)
        pos += n
    assert np.max(np.abs(np.concatenate(a, axis=1) - ref)) <= 1e-13 * np.max(np.abs(ref))
    assert np.array_equal(np.concatenate(b, axis=1), ref32)
    walked, skipped = rm.WidebandRateModel(rate, offs), rm.WidebandRateModel(rate, offs)
    n0, n1 = 40 * r.min_call, len(x) - 60 * r.min_call
    for mod in (walked, skipped):
        mod.process(x[:n0], with_f32=True)
        mod.set_offset(1, offs[4])
    walked.process(x[n0:n1], with_f32=True)
    skipped.advance(n1 - n0, x[n1 - (r.NP - 1):n1])
    assert walked.P == skipped.P and walked.g == skipped.g
    y, y32 = walked.process(x[n1:], with_f32=True)
    z, z32 = skipped.process(x[n1:], with_f32=True)
    assert np.max(np.abs(y - z)) <= 1e-13 * np.max(np.abs(y)) and np.array_equal(y32, z32)


# What the detector catches (check_per_sample, bound 2) of the five seeded defects, per rate.  "last tap" drops the tap i = NP - 1 of every
# phase that has one, p < N_H - L (NP - 1): 17 of 24 phases at 2.4 MS/s, 209 of 576 at 2.5 MS/s, caught -- down to the single phase 0 at
# 36 MS/s, whose last tap is H [N_H - 1] itself: the Blackman window leaves it 1.5e-9 of a phase's sum, under an f32 sum's rounding, and no
# f32 bound can see it (as DESIGN 4.8 says of the tap i = 16 K at K = 16).  Everything else is caught at every rate (the late rotator on
# the outputs whose offset is not 0: offset 0 has no rotation).
DEFECTS = ["one sample", "phase", "sample index", "last tap", "late rotator"]
NOT_CAUGHT = {"last tap": {36000000}}


@pytest.mark.parametrize("rate", rm.RATES)
def test_seeded_defects(rate):
    """1e-5 of the peak on one sample; the phase p_j one too far from the second tile on; n_j one too small at a call boundary (output 300);
    the tap i = NP - 1 of the longest phases dropped; the rotator one output late from the second tile on."""
    r = rm.Ratio(rate)
    x, offs, ref, ref32, form = case(rate)
    got = {}
    one = form.astype(np.complex128)
    one[1, 300] += 1e-5 * np.max(np.abs(ref[1]))
    got["one sample"] = one
    got["phase"] = rm.kernel_form(rate, offs, x, phase_off_from=256)
    got["sample index"] = rm.kernel_form(rate, offs, x, n_off_at=[300])
    got["last tap"] = rm.kernel_form(rate, offs, x, drop_last_tap=True)
    got["late rotator"] = rm.kernel_form(rate, offs, x, rot_lag=256)
    for name in ("phase", "late rotator"):
        assert np.array_equal(got[name][:, :256], form[:, :256])
    assert np.array_equal(got["late rotator"][0], form[0])              # offset 0 has no rotation: the fault shows on the others
    dropped = np.abs(rm.taps(rate)[r.L * (r.NP - 1):])
    print("\n[seeded, %d S/s] %d of %d phases have a tap i = NP - 1; the largest is %.1e of a phase's sum, the last %.1e"
          % (rate, len(dropped), r.L, float(dropped.max()), float(dropped[-1])))
    for name in DEFECTS:
        rows = slice(1, None) if name == "late rotator" else slice(None)
        hit = caught("seeded %s, %d S/s" % (name, rate), got[name][rows], ref[rows], ref32[rows])
        print("[seeded, %d S/s] %s: %s" % (rate, name, "caught" if hit else "not caught"))
        assert hit == (rate not in NOT_CAUGHT.get(name, set())), (name, rate)

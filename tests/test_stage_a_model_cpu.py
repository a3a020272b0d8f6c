"""The float64 model of stage A (tests/stage_a_model.py) on the CPU: against the oracle's TAP_FM_IQ -- the figures the GPU bounds of
tests/test_gpu_stage_a_per_sample.py are derived from --, the kernels' forms restated on the host, the documented distance between RF DC
removal in front of the filter and behind it, and the detector against defects seeded into restated outputs on the GPU tests' own shapes.
Every test prints what it measures."""
import numpy as np
import pytest

import stage_a_model as sa

N = 491520                     # 30 of the oracle's 16384-sample blocks: 40960 fm samples at a decimation of 12

# (settings of the oracle chain and the model, settings of the signal generator)
CASES = {
    "dc inside the limiter": (dict(), dict(dcI=0.004, dcQ=-0.003)),
    "dc beyond the limiter": (dict(), dict(dcI=0.02, dcQ=-0.015)),
    "balance 0.9 / 1.1": (dict(att=(0.9, 1.1)), dict()),
    "oscillator 200000": (dict(lo=200000), dict(offsetHz=200000.0)),
    "oscillator 2500": (dict(lo=2500), dict(offsetHz=2500.0)),
    "amplitude 30": (dict(), dict(carrierAmp=30.0)),
    "amplitude 1e-6": (dict(), dict(carrierAmp=1e-6)),
    "2880000": (dict(rate=2880000, lo=30000), dict(offsetHz=30000.0, dcI=0.004, dcQ=-0.003)),
    "1920000": (dict(rate=1920000, lo=30000), dict(offsetHz=30000.0, dcI=0.004, dcQ=-0.003)),
    "192000": (dict(rate=192000, lo=3000), dict(offsetHz=3000.0, dcI=0.004, dcQ=-0.003)),
}


def record_holds(measured, record, what):
    """test_f64_models_cpu's rule: the recorded figure is not below the measured one and not more than a quarter above it."""
    print("[reference alone] %s: measured %.3e of the peak, recorded %.3e" % (what, measured, record))
    assert measured <= record <= 1.25 * measured, (what, measured, record)


def oracle_fm_iq(ol, iq, rate, bw, lo=0, att=(1.0, 1.0)):
    ch = ol.OracleChain(inputRate=rate, inputFilterBw=bw, loFrequency=lo, attL=att[0], attR=att[1], taps=[ol.TAP_FM_IQ], tap_seconds=3.0)
    ch.process(iq)
    z = ch.tap(ol.TAP_FM_IQ).copy()
    ch.close()
    return z


@pytest.mark.parametrize("filter_on", [True, False], ids=["filter on", "filter off"])
def test_the_oracle_against_the_model(ol, filter_on):
    """The level: the oracle chain's TAP_FM_IQ against the unfolded float64 model, every sample, relative to the peak, over DC offsets inside
    and beyond the limiter, a balance, oscillators on the 200 kHz raster and off it, carrier amplitudes 30 and 1e-6 and the rates the
    reference decimates by 12 (2 880 000), by 6 (1 920 000) and not at all (192 000).  The largest figure is the record
    REF_STAGE_A_WORST_ON / _OFF; the GPU bounds are the records doubled, so the oracle stays within the bounds' halves.
    Measured, filter on: 7.1e-7 ... 8.7e-7 at the decimated rates (peak 2.0 ... 2.6 for a carrier of 0.5), 1.30e-6 at 192 000, where no
    decimator's gain stands behind the overlap-add filter's noise (peak 0.54); filter off: 2.3e-7 ... 4.1e-7."""
    L = ol.oracle()
    level = 0.0
    for name, (kw, sig) in CASES.items():
        kw = dict(kw)
        rate = kw.pop("rate", 2304000)
        bw = (150000 if rate == 192000 else 165000) if filter_on else 0
        iq = ol.synth_iq(N, **sig)
        z = oracle_fm_iq(ol, iq, rate, bw, **kw)
        D = sa.Design(L, rate, bw)
        ref = sa.stage_a(D, iq, **kw)
        assert z.shape[0] == ref.shape[0] == N // D.decim
        w = sa.compare(z, ref)
        print("\n[oracle against float64, %s, filter %d] %s" % (name, bw, w))
        assert w.scale > 2e-6
        level = max(level, w.rel)
    record = sa.REF_STAGE_A_WORST_ON if filter_on else sa.REF_STAGE_A_WORST_OFF
    record_holds(level, record, "stage A, input filter %s" % ("on" if filter_on else "off"))
    assert level <= 0.5 * (sa.STAGE_A_BOUND_ON if filter_on else sa.STAGE_A_BOUND_OFF)


def test_the_model_owes_the_library_nothing(ol):
    """What build_front_set derives, derived again from the reference's kernels alone: 287 taps (37 with the input filter off), the newest input of
    fm sample j at 12 j + 11 - 65285 = 12 (j - 5440) + 6, the centre of mass 12 columns back."""
    L = ol.oracle()
    on, off = sa.Design(L, 2304000, 165000).front_set(), sa.Design(L, 2304000, 0).front_set()
    assert on["g32"].size == 287 and off["g32"].size == 37
    assert (on["delay"], on["off"], on["dc_k"]) == (5440, 6, 12) and (off["delay"], off["off"]) == (0, 11)
    assert abs(on["hsum"] - 1.0) < 1e-5 and 0.0 <= on["dc_w"] < 1.0 and 0.0 <= off["dc_w"] < 1.0
    assert on["gain"] == off["gain"]                            # (1 + j S1) (1 + j S2): the decimators' alone
    assert 4.0 < abs(on["gain"]) < 6.0                          # (a carrier of 0.5 peaks at 2.5)


# ------------------------------------------------------------------------------------------------ the kernels' forms, restated
@pytest.fixture(scope="module")
def shapes(ol):
    """The matrix-pipe case's shape: its calls, a stream with a DC offset that is still settling, the model of both forms."""
    L = ol.oracle()
    calls = sa.FRONT4_CALLS + sa.FLUSH_CALLS
    n = sum(calls)
    iq = ol.synth_iq(n, dcI=0.004, dcQ=-0.003)
    D = sa.Design(L, 2304000, 165000)
    vr, vi = sa.premix32(D, iq)
    return dict(L=L, calls=calls, n=n, iq=iq, D=D, vr=vr, vi=vi, front=sa.stage_a(D, iq), behind=sa.stage_a(D, iq, form="behind"),
                starts=sa.call_starts_fm(calls))


def test_restatements_of_the_kernel_forms(ol, shapes):
    """front_kernel's form (f32 taps and samples, one accumulator in tap order, then the gain), front4_kernel's split alone (a tile's
    power-of-two scale, samples and taps 2^14 as f16 halves, three product terms, exact sums) and the fold with f32-rounded taps, each
    against the unfolded model: the bounds leave room for them and are not met by accident.
    Measured: f32 fold 8.4e-7 of the peak (1.31e-6 is the reference's level, 2.62e-6 the bound), the split alone 4.4e-8, the float64 fold
    with f32 taps 3.5e-8."""
    D, vr, vi, ref = shapes["D"], shapes["vr"], shapes["vi"], shapes["front"]
    f64 = sa.folded_f64(D, vr, vi)
    w_f32 = sa.compare(sa.folded_f32(D, vr, vi), ref, shapes["starts"])
    w_split = sa.compare(sa.split_f64(D, vr, vi), f64, shapes["starts"])
    w_fold = sa.compare(f64, ref, shapes["starts"])
    print("\n[f32 fold against the model] %s\n[front4's split alone, against the float64 fold] %s\n[float64 fold, f32 taps, against the model] %s"
          % (w_f32, w_split, w_fold))
    assert w_f32.scale > 2.0
    assert w_f32.rel <= sa.REF_STAGE_A_WORST_ON          # (a 287-tap f32 sum is no worse than the reference's 65536-point f32 transforms)
    assert w_split.rel <= 2.0 ** -22                     # (a sample keeps 22 bits)
    assert w_fold.rel <= 2.0 ** -24                      # (every tap and every mixed sample rounded once)


def test_rf_dc_in_front_of_the_filter_and_behind_it(ol):
    """The documented deviation: the distance between the two float64 forms on streams with a DC offset -- inside the limiter,
    beyond it, with a balance, at amplitude 1e-6 -- and with constant oscillators of 200 000 and 2500 Hz stays under the 2.5e-6 of the fm-rate
    IQ's peak stated there.
    Measured: 3.3e-7 ... 3.5e-7 with the input filter on, 2.3e-7 ... 2.4e-7 off (the first outputs of a stream, whose windows begin in front of it);
    oscillator 200 000: 8.7e-7 on, 9.2e-7 off -- RfDC carries a ripple of alpha |x| at the carrier's offset, which the reference's order mixes to
    0 Hz and the column boundaries do not sample --, oscillator 2500: 4.1e-7 on, 2.9e-7 off."""
    L = ol.oracle()
    worst = 0.0
    for bw in (165000, 0):
        D = sa.Design(L, 2304000, bw)
        for att, lo, sig in (((1.0, 1.0), 0, dict(dcI=0.004, dcQ=-0.003)), ((1.0, 1.0), 0, dict(dcI=0.02, dcQ=-0.015)),
                             ((0.9, 1.1), 0, dict(dcI=0.02, dcQ=-0.015)), ((1.0, 1.0), 0, dict(carrierAmp=1e-6, dcI=4e-9, dcQ=-3e-9)),
                             ((1.0, 1.0), 200000, dict(offsetHz=200000.0)), ((1.0, 1.0), 2500, dict(offsetHz=2500.0))):
            iq = ol.synth_iq(N, **sig)
            w = sa.compare(sa.stage_a(D, iq, att=att, lo=lo, form="behind"), sa.stage_a(D, iq, att=att, lo=lo))
            print("\n[DC behind the filter against DC in front of it, filter %d, balance %s, oscillator %d, %s] %s" % (bw, att, lo, sig, w))
            worst = max(worst, w.rel)
    assert 0.0 < worst <= sa.FRONT_BEHIND_DOCUMENTED


def test_the_two_forms_across_an_oscillator_switch(ol):
    """An oscillator switched on, and another switched off, between two calls: windows behind the switch hold samples mixed with the old
    oscillator.  The second form's RF DC term is the filter run over the oscillator's own sequence; with the NEW oscillator turned back over
    those samples it would be misplaced by gain |RfDC| -- 1.1e-3 of the peak on this stream, whose RfDC value follows its 0 Hz carrier.  The two
    forms stay within the documented 2.5e-6 across both switches.  Measured: 5.2e-7 and 4.6e-7."""
    T = sa.TILE
    calls = [8 * T, 7 * T + 480, 6 * T - 480, 8 * T, 8 * T] + sa.FLUSH_CALLS
    iq = (ol.synth_iq(sum(calls), carrierAmp=0.2).astype(np.float64) + ol.synth_iq(sum(calls), carrierAmp=0.2, offsetHz=2500.0, leftHz=470.0)).astype(np.float32)
    D = sa.Design(ol.oracle(), 2304000, 165000)
    for lo in ([0, 0, 0, 0, 2500, 2500, 2500], [200000, 200000, 200000, 0, 0, 0, 0]):
        w = sa.compare(sa.stage_a(D, iq, calls, lo=lo, form="behind"), sa.stage_a(D, iq, calls, lo=lo), sa.call_starts_fm(calls))
        print("\n[the two forms across an oscillator switch %s] %s" % (lo, w))
        assert w.scale > 0.5 and w.rel <= sa.FRONT_BEHIND_DOCUMENTED


# ------------------------------------------------------------------------------------------------ the detector
def caught(got, ref, bound, starts):
    w = sa.compare(got, ref, starts)
    try:
        sa.check(w, bound, "seed")
    except AssertionError as e:
        assert "call %d, tile %d, column %d" % (w.call, w.tile, w.column) in str(e)
        return w
    return None


def test_the_detector_catches_seeded_defects(ol, shapes):
    """Defects seeded into RESTATED outputs (never into a kernel) on the matrix-pipe case's calls; `check` must fail on each and name the
    sample.  The clean restatements pass."""
    D, vr, vi, ref, starts, calls = shapes["D"], shapes["vr"], shapes["vi"], shapes["front"], shapes["starts"], shapes["calls"]
    B = sa.STAGE_A_BOUND_ON
    clean = sa.folded_f32(D, vr, vi)
    assert caught(clean, ref, B, starts) is None
    peak = float(np.abs(ref.real).max())
    # 1e-5 of the peak on one sample
    s = clean.copy(); j = int(starts[7]) + 3 * sa.COLS + 77; s[j] += 1e-5 * peak
    w = caught(s, ref, B, starts)
    assert w is not None and w.index == j and (w.call, w.tile, w.column) == (7, 3, 77)
    # one tile's outputs one column late (the third tile of the 13-tile call, as its read-out shows it: outputs in flight are 5440 old)
    s = clean.copy(); a = 5440 + int(starts[4]) + 2 * sa.COLS; s[a:a + sa.COLS] = clean[a - 1:a + sa.COLS - 1]
    w = caught(s, ref, B, starts)
    assert w is not None and a <= w.index < a + sa.COLS
    # the gain's imaginary part negated
    F = D.front_set()
    assert caught(sa.folded_f64(D, vr, vi, gain=np.conj(F["gain"])), ref, B, starts) is not None
    # the oscillator's phase one sample off behind a call boundary (an oscillator of 2500 Hz: a step of 0.0068 rad)
    x = sa.as_complex(shapes["iq"])
    LO, P = sa.oscillator(x.shape[0], D.rate, [(0, 2500)])
    v = sa.balance(x - sa.clamp(sa.rf_dc(x, D.rate, [(0, 1)])[1:]), (1.0, 1.0))
    slip = LO.copy(); b = sum(calls[:4]); slip[b:-1] = LO[b + 1:]
    assert caught(sa.filters(v * LO, D), sa.stage_a(D, shapes["iq"], lo=2500), B, starts) is None
    w = caught(sa.filters(v * slip, D), sa.stage_a(D, shapes["iq"], lo=2500), B, starts)
    assert w is not None and w.index >= b // 12 + 5440 - 24
    # one sample in 2^13 without its f16 low half (the double-rounding tie of round 6)
    assert caught(sa.split_f64(D, vr, vi), ref, B, starts) is None
    w = caught(sa.split_f64(D, vr, vi, drop_low_every=8192), ref, B, starts)
    assert w is not None
    print("\n[a sample in 2^13 without its low half] %s" % w)


def test_the_detector_and_the_newest_taps(ol, shapes):
    """The newest tap dropped.  The reference's Blackman window is zero at i = 0 (fir-filters.cpp:45-59: cos (2 pi i / N), not N - 1), so the
    fold's newest taps are zero or next to it: g[0] = g[1] = 0 with the input filter on, g[0 ... 6] = 0 with it off (37 taps).  One dropped tap
    there is under an f32 sum's rounding, as stage W's seventeenth tap is; what the check sees is a dropped COLUMN.  Measured: with the filter on,
    caught from the newest 22 taps on (they weigh 3.9e-6 of the sum), asserted for the newest two columns; with the filter off from the newest 8
    on (3.6e-5 of the sum), asserted for the newest column."""
    L = shapes["L"]
    for bw, m_caught, bound in ((165000, 24, sa.STAGE_A_BOUND_ON), (0, 12, sa.STAGE_A_BOUND_OFF)):
        D = sa.Design(L, 2304000, bw)
        vr, vi = sa.premix32(D, shapes["iq"])
        ref = sa.stage_a(D, shapes["iq"])
        g = D.front_set()["g32"]
        first = None
        for m in range(1, 40):
            gm = g.copy(); gm[:m] = 0.0
            if caught(sa.folded_f64(D, vr, vi, g=gm), ref, bound, shapes["starts"]) is not None:
                first = m
                break
        assert first is not None and first <= m_caught
        print("\n[newest taps dropped, filter %d] caught from the newest %d on; they weigh %.2e of the sum" % (bw, first, abs(g[:first]).sum() / g.sum()))


def test_the_detector_and_a_late_rf_dc_value(ol, shapes):
    """The second form's RF DC value taken one column late, on the matrix-pipe case's own stream, whose RfDC value is still settling.  RfDC follows
    the carrier itself, not only the offset: per column it moves by 12 alpha |x - RfDC| = 5.2e-6 of the carrier, the gain makes 2.5e-5 of that,
    and the peak is 4.8 times the carrier: 5e-6 of the peak, twice the bound.  Measured: 5.1e-6, caught."""
    D, starts = shapes["D"], shapes["starts"]
    assert caught(shapes["behind"].astype(np.complex64), shapes["behind"], sa.STAGE_A_BOUND_ON, starts) is None
    w = caught(sa.stage_a(D, shapes["iq"], form="behind", dc_columns_late=1), shapes["behind"], sa.STAGE_A_BOUND_ON, starts)
    print("\n[RF DC one column late] %s" % w)
    assert w is not None

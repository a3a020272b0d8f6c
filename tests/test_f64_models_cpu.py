"""The float64 models of tests/f64_models.py against the oracle, on the CPU: a GPU failure of tests/test_gpu_worst_sample.py can then be
blamed on the kernel and not on the model.  Every test prints the reference-alone figure it measures -- the worst frame of the oracle's
f32 arithmetic against the model on identical inputs, relative to the output's peak -- and holds it against its record in f64_models.py
(REF_*), from which the GPU bounds are derived."""
import ctypes as C

import numpy as np
import pytest

import f64_models as fm


def record_holds(measured, record, what):
    """The recorded figure is the measured one: not below it (the GPU bound would be too tight for the reference itself) and not more
    than a quarter above (it would be inflated).  Another libm or compiler moves the last bits of the measurement, not a quarter."""
    print("[reference alone] %s: measured %.3e of the peak, recorded %.3e" % (what, measured, record))
    assert measured <= record <= 1.25 * measured, (what, measured, record)


@pytest.fixture(scope="module")
def config2(ol):
    """configs[1] (stereo, 165 kHz, PSS) over 3 s: PCM and the taps the models read."""
    n = 16384 * 422
    iq = ol.synth_iq(n)
    ch = ol.OracleChain(taps=[ol.TAP_LRRAW, ol.TAP_PRE_RS], inputFilterBw=165000, tap_seconds=3.1)
    pcm = ch.process(iq)
    return dict(iq=iq, pcm=pcm, pre=ch.tap(ol.TAP_PRE_RS).copy(), lr=ch.tap(ol.TAP_LRRAW).copy())


def resampler_taps(ol):
    r = np.zeros(fm.RS_TAPS, np.float32)
    ol.oracle().fmo_resampler_taps(ol.fptr(r))
    return r


def test_resampler_fade_and_gain_against_the_oracle(ol, config2):
    """The oracle's TAP_PRE_RS sits behind the gain, so its PCM is fade (m) sum_k r[k] pre[4 m + 3 - k]: frame by frame over the first
    second (the fade's 24000 frames and as many behind it).  Measured: worst frame 2.8e-7 at a peak of 0.35 (8.0e-7 of it), rms 3.7e-8.
    Bound 1e-6 of the peak: 1.25 x the measured figure, for other signals and gains."""
    pcm, pre = config2["pcm"][:48000], config2["pre"]
    ref = fm.stage_c_folded(pre, resampler_taps(ol), [1.0, 1.0], lf_on=False, m1=pcm.shape[0])
    w = fm.compare(pcm, ref)
    print("\n[resampler + fade, oracle against float64] %s" % w)
    assert pcm.shape[0] == 48000 and w.scale > 0.3
    record_holds(w.rel, fm.REF_RESAMPLER_WORST, "resampler + fade")
    fm.check(w, 1e-6, "oracle resampler + fade")


@pytest.mark.parametrize("volume_db,balance", [(-6.0, 0), (-10.5, 30), (3.25, -45), (-20.0, 100)])
def test_gain_is_formed_as_the_oracle_forms_it(ol, volume_db, balance):
    """gain_lr () bit for bit: with 0 dB and no balance the oracle's gain is exactly 1, so the pre-resampler tap of a chain at
    (volume, balance) is the f32 product of gain_lr and the tap of the chain at (0 dB, 0)."""
    iq = ol.synth_iq(16384 * 12)
    taps = []
    for v, b in ((0.0, 0), (volume_db, balance)):
        ch = ol.OracleChain(taps=[ol.TAP_PRE_RS], inputFilterBw=165000, volumeDb=v, balance=b, tap_seconds=0.2)
        ch.process(iq)
        taps.append(ch.tap(ol.TAP_PRE_RS).copy())
    g = fm.gain_lr(volume_db, balance)
    assert np.abs(taps[0]).max() > 0.1 and g.dtype == np.float32
    assert np.array_equal(taps[1], taps[0] * g[None, :])


def test_audio_low_pass_reference_alone(ol, config2):
    """The oracle's own f32 overlap-add audio filter (fmo_fftfilter: 8192 points, 756 taps, 15 kHz) over the 192 kS/s stereo stream the
    reference's audio filter reads (left / right from TAP_LRRAW of configs[1], 3 s: programme, pilot and the 38 kHz products), then the
    oracle's f32 resampler (128 taps, summed in its order), against the float64 model -- the filter alone at 192 kS/s, and filter +
    resampler at the 48 kHz instants in the folded and in the two-step form (which are one model: 1e-12).
    THE figure the GPU bound of stage C is derived from (f64_models.REF_STAGE_C_WORST, STAGE_C_BOUND = 2 x).
    Measured: filter alone 1.33e-6 of the peak, filter + resampler 1.29e-6 of the peak (0.73)."""
    L = ol.oracle()
    lr = config2["lr"]
    x = np.ascontiguousarray(np.stack([lr[:, 0] + lr[:, 1], lr[:, 0] - lr[:, 1]], axis=1), np.float32)
    n = x.shape[0] // 4 * 4
    x = x[:n]
    assert n >= 3 * 190000
    f = L.fmo_fftfilter_new(8192, fm.AUDIO_TAPS)
    L.fmo_fftfilter_set_lowpass(f, 15000, 192000)
    y = np.zeros_like(x)
    L.fmo_fftfilter_run_c(f, ol.fptr(x), ol.fptr(y), n)
    L.fmo_fftfilter_free(f)
    h = np.zeros(fm.AUDIO_TAPS, np.float32)
    L.fmo_lowpass_kernel(fm.AUDIO_TAPS, 15000, 192000, ol.fptr(h))
    w_lp = fm.compare(y, fm.delayed(fm.fftconv(x, h), fm.AUDIO_DELAY, n))
    print("\n[audio low-pass, oracle overlap-add against float64] %s" % w_lp)
    # the oracle's resampler on the oracle's filter output (resampler_push: k ascending, f32, unfused)
    r = resampler_taps(ol)
    m = n // 4
    yp = np.concatenate([np.zeros((fm.RS_TAPS - 1, 2), np.float32), y])
    idx = 4 * np.arange(m) + 3 + fm.RS_TAPS - 1
    acc = np.zeros((m, 2), np.float32)
    for k in range(fm.RS_TAPS):
        acc = acc + r[k] * yp[idx - k]
    g = np.convolve(h.astype(np.float64), r.astype(np.float64))
    never = -10 ** 9                                              # (no fade: the stage alone)
    folded = fm.stage_c_folded(x, g, [1.0, 1.0], lf_on=True, m1=m, fade_start=never)
    two = fm.stage_c_two_step(x, h, r, [1.0, 1.0], m1=m, fade_start=never)
    assert np.abs(folded - two).max() <= 1e-12 * np.abs(folded).max()
    w = fm.compare(acc, folded)
    print("[audio low-pass + resampler, oracle f32 against float64] %s" % w)
    assert w.scale > 0.3
    record_holds(w.rel, fm.REF_STAGE_C_WORST, "overlap-add audio filter + resampler")
    assert fm.STAGE_C_BOUND == 2.0 * fm.REF_STAGE_C_WORST


def test_two_step_model_with_a_gain_step_equals_the_folded_model_away_from_it(ol, config2):
    """A gain that steps at fm sample J: frames whose 128-tap resampler window lies wholly on one side of J are the folded model at
    that side's gain; the frames that straddle it are neither (the case gain_fix_kernel exists for)."""
    L = ol.oracle()
    x = config2["pre"][:60000]
    h = np.zeros(fm.AUDIO_TAPS, np.float32)
    L.fmo_lowpass_kernel(fm.AUDIO_TAPS, 15000, 192000, ol.fptr(h))
    r = resampler_taps(ol)
    g = np.convolve(h.astype(np.float64), r.astype(np.float64))
    g0, g1 = fm.gain_lr(-6.0, 0), fm.gain_lr(-10.5, 30)
    J = 192 * 200 + 103
    two = fm.stage_c_two_step(x, h, r, fm.gain_steps(x.shape[0], [0, J], [g0, g1]))
    f0, f1 = fm.stage_c_folded(x, g, g0), fm.stage_c_folded(x, g, g1)
    m_before, m_after = (J - 3) // 4, (J + fm.RS_TAPS + 3) // 4          # 4 m + 3 < J  /  4 m + 3 - 127 >= J
    s = np.abs(f0).max()
    assert np.abs(two[:m_before] - f0[:m_before]).max() <= 1e-12 * s and np.abs(two[m_after:] - f1[m_after:]).max() <= 1e-12 * s
    mid = slice(m_before + 4, m_after - 4)
    assert np.abs(two[mid] - f0[mid]).max() > 1e-4 * s and np.abs(two[mid] - f1[mid]).max() > 1e-4 * s


def test_rds_front_end_model_against_the_oracle(ol):
    """rds_front () on the oracle's TAP_DEMOD and TAP_PILOT against the oracle's TAP_RDS_IQ, 2.3 s with RDS at 0.05: every one of the
    56320 baseband samples, the 64000-sample start-up included.  Measured: worst sample 2.7e-7 at a peak of 0.256 (1.05e-6 of it), rms 5.0e-8.
    (The reference mixes with cos / sin of libm here, not with its table -- fm-processor.cpp:748-753 says why -- and so does the model.)"""
    n = 16384 * 330
    iq = ol.synth_iq(n, rds=1, rdsLevel=0.05)
    ch = ol.OracleChain(taps=[ol.TAP_DEMOD, ol.TAP_PILOT, ol.TAP_RDS_IQ], inputFilterBw=165000, rdsMode=2, tap_seconds=2.6)
    ch.process(iq)
    d, p, q = ch.tap(ol.TAP_DEMOD), ch.tap(ol.TAP_PILOT), ch.tap(ol.TAP_RDS_IQ)
    assert d.shape[0] >= 2 * 192000 and q.shape[0] == d.shape[0] // 8
    bp, dk = fm.rds_tables(ol.oracle())
    ref = fm.rds_front(d, p, bp, dk)
    w = fm.compare(q[:, 0].astype(np.float64) + 1j * q[:, 1], ref)
    print("\n[RDS front end, oracle against float64] %s" % w)
    assert w.scale > 0.05
    record_holds(w.rel, fm.REF_RDS_WORST, "RDS baseband")
    assert fm.RDS_BOUND == 2.0 * fm.REF_RDS_WORST


def test_second_converter_model_against_the_oracle(ol, config2):
    """conv2 () stage-local: the oracle's 48 kHz frames are those of the same chain at audioRate = 48000, so the model runs on them (f32)
    and is compared with the oracle's PCM at 44100, 96000 and 32000, every frame.  Measured worst frame, of the peak (0.35): 6.6e-7, 3.9e-7, 5.5e-7."""
    iq = config2["iq"][:2304000]
    o48 = ol.OracleChain(inputFilterBw=165000).process(iq)
    worst = 0.0
    for rate in (44100, 96000, 32000):
        o = ol.OracleChain(inputFilterBw=165000, audioRate=rate).process(iq)
        p, q, taps = fm.conv2_design(ol.oracle(), 48000, rate)
        ref = fm.conv2(o48, p, q, taps)
        assert ref.shape == o.shape and o.shape[0] == fm.conv2_count(o48.shape[0], p, q)
        w = fm.compare(o, ref)
        print("\n[second converter %d = 48000 x %d / %d, oracle against float64] %s" % (rate, p, q, w))
        assert w.scale > 0.3
        worst = max(worst, w.rel)
    record_holds(worst, fm.REF_CONV2_WORST, "second converter")
    assert fm.CONV2_BOUND == fm.STAGE_C_BOUND + fm.REF_CONV2_WORST


@pytest.mark.parametrize("where", ["one frame in every 1792", "the first frame of a call"])
def test_the_detector_detects_what_the_rms_bar_does_not(ol, config2, where):
    """A synthetic kernel output: the float64 model of stage C rounded to f32, plus 1e-4 on one frame in every 1792 (a workgroup's block
    of audio_fft_kernel) or on the single first frame of a call.  It passes the suite's bar, rms <= 1e-5, and fails the worst-frame
    assertion, which names the seam."""
    L = ol.oracle()
    x = config2["pre"][:192000]
    h = np.zeros(fm.AUDIO_TAPS, np.float32)
    L.fmo_lowpass_kernel(fm.AUDIO_TAPS, 15000, 192000, ol.fptr(h))
    g = np.convolve(h.astype(np.float64), resampler_taps(ol).astype(np.float64))
    ref = fm.stage_c_folded(x, g, fm.gain_lr(-6.0, 0))
    calls = [0, 4176, 4176 + 48 * 13, 20000 // 48 * 48]
    clean = ref.astype(np.float32)
    w = fm.compare(clean, ref, calls)
    fm.check(w, fm.STAGE_C_BOUND, "the model rounded to f32")
    bad = clean.copy()
    if where == "one frame in every 1792":
        bad[1791::fm.C_BLOCK, 0] += np.float32(1e-4)
    else:
        bad[calls[2], 1] += np.float32(1e-4)
    w = fm.compare(bad, ref, calls)
    print("\n[seeded glitch, %s] %s" % (where, w))
    assert w.rms <= fm.PCM_RMS_TOL                                 # the existing bar does not see it
    with pytest.raises(AssertionError, match="worst frame"):
        fm.check(w, fm.STAGE_C_BOUND, "seeded glitch")
    if where == "one frame in every 1792":
        assert w.mod1792 == 1791 and w.mod256 == 255 and w.lane == 0
    else:
        assert w.call == 2 and w.from_call_start == 0 and w.lane == 1


@pytest.mark.parametrize("back,frames,exact", [(320, 80, True), (128, 32, False)], ids=["GAIN_FIX_BACK=320", "GAIN_FIX_BACK=128"])
def test_the_detector_sees_a_gain_correction_that_is_too_short(ol, config2, back, frames, exact):
    """gain_fix_kernel's arithmetic in float64 (fmx_audio.hip: the folded filter at the new gain plus (g_old - g_new) sum_q h_rs[e_r + q]
    a[J0 - q] on the call's first frames), for a call that starts 103 samples into a resampler block (e_0 = -100): with the kernel's
    GAIN_FIX_BACK = 320 entries and 80 frames it IS the two-step model; with rounds 2-5's 128 entries and 32 frames -- the mutation a reviewer
    can make in fmx_internal.h -- frames 32 ... 78 of the call go without their part: the worst-frame assertion fails and
    names a frame right behind the call's first (frame 40 here, half the signal's size: a volume step of 7.5 dB)."""
    L = ol.oracle()
    x = config2["pre"][96000:96000 + 60000]                      # (behind the oracle's fade: full level)
    n = x.shape[0]
    h = np.zeros(fm.AUDIO_TAPS, np.float32)
    L.fmo_lowpass_kernel(fm.AUDIO_TAPS, 15000, 192000, ol.fptr(h))
    r = resampler_taps(ol)
    g = np.convolve(h.astype(np.float64), r.astype(np.float64))
    g0, g1 = fm.gain_lr(-6.0, 0), fm.gain_lr(-10.5, 30)
    J0 = 192 * 200 + 103
    M0 = fm.frames_of(J0)
    never = -10 ** 9
    ref = fm.stage_c_two_step(x, h, r, fm.gain_steps(n, [0, J0], [g0, g1]), m0=M0, fade_start=never)
    got = fm.stage_c_folded(x, g, g1, m0=M0, fade_start=never)
    a = fm.delayed(fm.fftconv(x, h), fm.AUDIO_DELAY, n)
    for fr in range(frames):
        e = 4 * (M0 + fr) + 3 - J0
        assert fr > 0 or e == -100
        for q in range(max(1, -e), back):
            if e + q < fm.RS_TAPS:
                got[fr] += (g0.astype(np.float64) - g1) * r[e + q] * a[J0 - q]
    w = fm.compare(got.astype(np.float32), ref, [0])
    print("\n[gain correction with %d entries and %d frames] %s" % (back, frames, w))
    assert w.scale > 0.1
    if exact:
        fm.check(w, fm.STAGE_C_BOUND, "gain correction as the kernel makes it")
    else:
        with pytest.raises(AssertionError, match="worst frame"):
            fm.check(w, fm.STAGE_C_BOUND, "gain correction of rounds 2-5")
        assert w.call == 0 and 32 <= w.from_call_start < 80

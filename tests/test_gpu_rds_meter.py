"""The RDS meter on the GPU (fmx_rds_meter_enable, fmx_rds_meter_records, fmx_rds_meter_cal, fmx_rds_meter_figures; csrc/fmx_rdsm.hip):
the records against the f32 restatement of tests/rdsm_model.py on the handle's own FMX_TAP_RDS_IQ gathered call by call -- bit for bit, every field --,
their independence of how the stream is cut into calls and pieces, a channel's own grid with a late and a paused decoder, the switching rules, the ring
and its read-out, one channel and an odd batch with the three slicers mixed, the isolation of everything else a handle delivers, the figures within the
CPU test's bounds, and the mirrors."""
import os
import subprocess

import numpy as np
import pytest

import rdsm_model as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = rm.WINDOW
R = 96          # input samples per RDS sample at 2 304 000 S/s: 12 x 8
# the calls in input samples.  Two calls of 3999 RDS samples lead past the path's delay; then pieces that produce 0, 1, 63, 64, 65, 2559 and 2561 RDS samples
# (4 fm samples, then 4 more: the first output falls into the second call); one call of 40 000 fm samples, which is made in pieces of at most 31 999; then on
CALLS = [R * 3999, R * 3999, 48, 48, R * 63, R * 64, R * 65, R * 2559, R * 2561, 12 * 40000, R * 3999, R * 3999]
RDS_PER_CALL = [3999, 3999, 0, 1, 63, 64, 65, 2559, 2561, 5000, 3999, 3999]


@pytest.fixture(scope="module")
def x3():
    """the clean signal (2250 Hz on cos (3 p)), the same at noise sigma 0.05, and one without RDS"""
    sec = (sum(CALLS) + 2304) / 2304000.0
    return np.stack([rm.signal(sec)[0], rm.signal(sec, sigma=0.05)[0], rm.signal(sec, rds_hz=0.0)[0]])


def make(fmx_amd, channels, streams=0, max_block=16384, rds=2, params=(), **kw):
    m = fmx_amd.fmx
    som = [c % streams for c in range(channels)] if streams else None
    f = fmx_amd.Fmx(channels, streams=streams, stream_of_channel=som, max_block=max_block, **kw)
    f.set_param(m.P_BANDWIDTH, 165000)
    if rds:
        f.set_param(m.P_RDS_MODE, rds)
    for item in params:
        f.set_param(*item)
    return f


def run(f, m, x, calls, tap_ch=(), each=None):
    """the calls of `calls` input samples behind each other; returns (pcm, {ch: RDS_IQ read after every call, behind each other}, {ch: [RDS samples per
    call]}) -- a channel's tap is in its own count: a call in which its decoder is off adds nothing"""
    taps, counts = {c: [np.zeros((0, 2), np.float32)] for c in tap_ch}, {c: [] for c in tap_ch}
    pcm, pos = [], 0
    for k, n in enumerate(calls):
        if each:
            each(f, k)
        pcm.append(f.process_host(x[:, pos:pos + n]))
        pos += n
        for c in tap_ch:
            nr = f.last_rds_samples(c)
            counts[c].append(nr)
            if nr > 0:
                taps[c].append(f.tap(m.TAP_RDS_IQ, nr, c))
    return np.concatenate(pcm, axis=1), {c: np.concatenate(v) for c, v in taps.items()}, counts


def same(a, b):
    return len(a) == len(b) and all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def test_records_against_the_restatement_on_the_handles_tap(fmx_amd, x3):
    """three channels (clean, noisy, no RDS), calls whose pieces produce 0, 1, 63, 64, 65, 2559 and 2561 RDS samples and one call made in pieces: every
    field of every record bit for bit"""
    m = fmx_amd.fmx
    f = make(fmx_amd, 3, max_block=max(CALLS))
    f.rds_meter_enable(True)
    _, taps, counts = run(f, m, x3, CALLS, tap_ch=(0, 1, 2))
    recs = f.rds_meter_records(capacity=64)
    assert f.rds_meter_records()[0].size == 0      # (read once: nothing is pending)
    f.close()
    assert counts[0] == RDS_PER_CALL and max(RDS_PER_CALL) > 4000       # (a piece of a call with RDS on has at most 31 999 fm samples: 4000 RDS samples)
    nwin = sum(RDS_PER_CALL) // W
    assert nwin >= 10
    for c in range(3):
        rm.check_records(recs[c], taps[c], expect_index=range(nwin))
    assert recs[0].tobytes() != recs[1].tobytes() and recs[0].tobytes() != recs[2].tobytes()
    assert float(recs[0]["ii_mean"][-1] + recs[0]["qq_mean"][-1]) > 100.0 * float(recs[2]["ii_mean"][-1] + recs[2]["qq_mean"][-1])      # (RDS on the air, and not)


def test_one_call_against_many(fmx_amd, x3):
    """behind three calls that lead past the path's delay, the same 8000 RDS samples in ONE call (768 000 input samples, made in pieces; the most the tap
    hands out of one call is 8192) and in eight calls that cut steps and windows, with RF DC removal off and the PLL decoder: the taps are equal (the
    premise), then the records are"""
    m = fmx_amd.fmx
    lead = [R * 3999] * 3
    many = [48, 48, R * 63, R * 64, R * 65, R * 2559, R * 2561, R * 2687]
    assert sum(many) == R * 8000
    res = []
    for calls in (lead + many, lead + [R * 8000]):
        f = make(fmx_amd, 3, max_block=R * 8000, params=[(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0)])
        f.rds_meter_enable(True)
        _, taps, counts = run(f, m, x3, calls, tap_ch=(0, 1, 2))
        res.append((f.rds_meter_records(), taps, counts))
        f.close()
    (rm_, tm, _), (ro, to, co) = res
    assert co[0][-1] == 8000
    nwin = (3 * 3999 + 8000) // W
    assert nwin == 7
    for c in range(3):
        assert tm[c].tobytes() == to[c].tobytes(), c
        rm.check_records(ro[c], to[c], expect_index=range(nwin))
        assert ro[c].tobytes() == rm_[c].tobytes(), c


def test_late_and_paused_decoder_and_switched_meter(fmx_amd, x3):
    """channel 0's decoder is switched on 12 060 input samples late: end_sample is in its own count and its grid its own (its records equal the restatement
    on ITS tap from its sample 0).  Channel 1's decoder is switched off and on again in mid-window: the window spans the pause.  Channel 2's meter is
    switched off and on in mid-window: the window in progress is dropped, the next starts at a boundary.  A call in which a decoder is off leaves the
    channel's count where it was.  Expected indices from the pure rule (rm.expected_windows)."""
    m = fmx_amd.fmx
    blk = R * 640               # a quarter window per call (5120 fm samples: one piece)
    calls = [12060] + [blk] * 36
    f = make(fmx_amd, 3, max_block=blk, rds=0)
    f.rds_meter_enable(True)
    on = []

    def each(f, k):
        if k == 0:
            f.set_param(m.P_RDS_MODE, 2, 1)
            f.set_param(m.P_RDS_MODE, 3, 2)
        if k == 1:
            f.set_param(m.P_RDS_MODE, 2, 0)
        if k == 10:
            f.set_param(m.P_RDS_MODE, 0, 1)       # (a pause in mid-window ...)
        if k == 15:
            f.set_param(m.P_RDS_MODE, 2, 1)       # (... of five calls)
        if k == 18:
            f.rds_meter_enable(False, 2)
        if k == 20:
            f.rds_meter_enable(True, 2)
        on.append([True, True, not 18 <= k < 20])
    _, taps, counts = run(f, m, x3, calls, tap_ch=(0, 1, 2), each=each)
    recs = f.rds_meter_records()
    f.close()
    assert counts[0][0] == 0 and counts[0][1] == 640 and counts[1][0] == 12060 // R and all(n == 0 for n in counts[1][10:15])
    for c in range(3):
        want = rm.expected_windows([(counts[c][k], on[k][c]) for k in range(len(calls))])
        assert len(want) >= 5
        rm.check_records(recs[c], taps[c], expect_index=want)
    assert list(recs[0]["index"]) == list(range(9)) and recs[0]["end_sample"][-1] == 9 * W == sum(counts[0])
    assert list(recs[1]["index"]) == list(range(sum(counts[1]) // W))                  # (the pause costs no window)
    assert 4 not in list(recs[2]["index"]) and 3 in list(recs[2]["index"]) and 5 in list(recs[2]["index"])


def test_meter_without_a_decoder_and_resets(fmx_amd, x3):
    """a metered channel whose decoder never runs gets no records (the meter switches no RDS on); FMX_A_RESET_RDS and FMX_A_TRIGGER_FREQUENCY_CHANGE in
    mid-stream do not touch the meter: the records stay on the tap's grid"""
    m = fmx_amd.fmx
    calls = [R * 3999] * 4
    f = make(fmx_amd, 2, max_block=calls[0], rds=0, params=[(m.P_RDS_MODE, 2, 0)])
    f.rds_meter_enable(True)

    def each(f, k):
        if k == 1:
            f.set_param(m.A_RESET_RDS, 0, 0)
        if k == 2:
            f.set_param(m.A_TRIGGER_FREQUENCY_CHANGE, 0, 0)
    _, taps, _ = run(f, m, x3[:2], calls, tap_ch=(0,), each=each)
    recs = f.rds_meter_records()
    f.close()
    rm.check_records(recs[0], taps[0], expect_index=range(4 * 3999 // W))
    assert recs[1].size == 0


def test_ring_keeps_64_and_capacity_leaves_the_rest(fmx_amd, ol):
    """70 windows unread leave the last 64; a capacity below what is pending leaves the rest for the next read (a handle at inputRate 192 000)"""
    m = fmx_amd.fmx
    blk, ncalls = 8 * (W + 8), 75
    x = ol.synth_iq(ncalls * blk, inputRate=192000, rds=1)[None]
    f = fmx_amd.Fmx(1, max_block=blk, inputRate=192000)
    f.set_param(m.P_RDS_MODE, 2)
    f.rds_meter_enable(True, 0)
    taps = []
    for k in range(70):
        f.process_host(x[:, k * blk:(k + 1) * blk])
        taps.append(f.tap(m.TAP_RDS_IQ, f.last_rds_samples(0), 0))
    assert (70 * blk // 8) // W == 70
    first = f.rds_meter_records(0, 1, capacity=10)[0]
    assert list(first["index"]) == list(range(6, 16))
    for k in range(70, 75):
        f.process_host(x[:, k * blk:(k + 1) * blk])
    rest = f.rds_meter_records(0, 1, capacity=64)[0]
    assert list(rest["index"]) == list(range(16, 75))
    assert f.rds_meter_records(0, 1)[0].size == 0
    f.close()
    rm.check_records(np.concatenate([first, rest[:54]]), np.concatenate(taps))


def test_handle_sizes(fmx_amd, x3):
    """one channel (the block-machine handle) and 65 channels (a batch, odd: the last channel has no partner in the paired transforms) with RDS_1, 2 and 3
    mixed, every channel metered: each handle's records on its own taps.  The slicer does not affect the meter: the one channel's records are the same
    with RDS_2, RDS_1 and RDS_3"""
    m = fmx_amd.fmx
    calls = [R * 3999] * 5
    nwin = 5 * 3999 // W
    single = []
    for mode in (2, 1, 3):
        f = make(fmx_amd, 1, max_block=calls[0], rds=mode)
        f.rds_meter_enable(True)
        _, taps, _ = run(f, m, x3[:1], calls, tap_ch=(0,))
        single.append(f.rds_meter_records()[0])
        rm.check_records(single[-1], taps[0], expect_index=range(nwin))
        f.close()
    assert single[0].tobytes() == single[1].tobytes() == single[2].tobytes()
    f = make(fmx_amd, 65, streams=3, max_block=calls[0], rds=0, params=[(m.P_RDS_MODE, 1 + (c // 3) % 3, c) for c in range(65)])
    f.rds_meter_enable(True)
    _, taps, _ = run(f, m, x3, calls, tap_ch=(0, 1, 2, 3, 30, 64))
    recs = f.rds_meter_records()
    f.close()
    for c in (0, 1, 2, 3, 30, 64):
        rm.check_records(recs[c], taps[c], expect_index=range(nwin))
    assert all(list(r["index"]) == list(range(nwin)) for r in recs)
    # (channels of one stream ride through the block transforms with different partners: their taps, and so their records, agree but for the last bits)
    assert recs[0].tobytes() != recs[1].tobytes() and np.allclose(recs[0]["ii_mean"], recs[3]["ii_mean"], rtol=1e-3)


def info_fields(info):
    """an fmx_rds_info field by field (the struct's padding and what lies behind a text's terminator are not part of what the library delivers)"""
    return tuple(tuple(v[:info.radio_text_ucs2_len + 1]) if name == "radio_text_ucs2" else v for name, v in ((name, getattr(info, name)) for name, _ in info._fields_))


@pytest.mark.parametrize("nch", [3, 65])
def test_other_outputs_unchanged(fmx_amd, ol, nch):
    """PCM, RDS bits, groups, fmx_rds_decode_all, meta, the three other meters' records, fmx_last_second_group and fmx_last_call_pieces of 3 and of 65
    channels are equal with the RDS meter on and off"""
    m = fmx_amd.fmx
    calls = [R * 3999, R * 3999, 12 * 40000] + [R * 3999] * 8
    n = sum(calls)
    # (a programme with groups to decode, the default stereo signal, and the generator's random RDS bits)
    x = np.stack([ol.synth_iq(n, rds=1, rdsLevel=0.05, rds_payload=ol.rds_programme_bits(pi=0xD3A1, ps="FMX-AMD ", text="THE RDS METER")), ol.synth_iq(n),
                  ol.synth_iq(n, rds=1)])
    out = []
    for meter in (False, True):
        f = make(fmx_amd, nch, streams=3, max_block=max(calls), rds=0, params=[(m.P_RDS_MODE, 1 + (c + 1) % 3, c) for c in range(nch)])
        f.mod_meter(True)
        f.audio_meter(True)
        f.rx_meter(True)
        if meter:
            f.rds_meter_enable(True)
        pcm, _, _ = run(f, m, x, calls)
        sel = range(nch) if nch == 3 else (0, 1, 2, 32, 64)
        out.append((pcm, [bytes(f.meta(c)) for c in sel], [f.rds_bits(c) for c in sel], f.rds_groups(), [info_fields(i) for i in f.rds_decode_all()],
                    f.mod_records(), f.audio_records(), f.rx_records(), (f.last_second_group(), f.last_call_pieces(), f.last_front_kernel()),
                    f.rds_meter_records()))
        f.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2])) and a[2][0].size > 0
    assert same(a[3], b[3]) and a[3][0].size > 0 and a[4] == b[4] and a[4][0][4] > 0      # (groups_decoded)
    assert same(a[5], b[5]) and a[5][0].size > 0 and same(a[6], b[6]) and a[6][0].size > 0 and same(a[7], b[7]) and a[7][0].size > 0
    assert a[8] == b[8]
    nwin = (sum(calls) // R) // W
    assert all(r.size == 0 for r in a[9]) and all(list(r["index"]) == list(range(nwin)) for r in b[9])


def oracle_kernels(ol):
    L = ol.oracle()
    bp, dk = np.zeros(2 * 768, np.float32), np.zeros(22, np.float32)
    L.fmo_bandpass_kernel(768, 57000 - 2400, 57000 + 2400, 192000, ol.fptr(bp))
    L.fmo_decim_kernel(11, 12000, 192000, ol.fptr(dk))
    return bp, dk


def test_figures_and_calibration(fmx_amd, ol):
    """the clean signal's figures, from the GPU's records, lie within the CPU test's bounds (rdsm_model.py); fmx_rds_meter_cal equals cal () of the model on
    the handle's own front-end taps to 1e-12 -- on the block-machine handle (the input filter a stage of its own) and on a folded one --, and refuses the
    decoders fmx_mod_hz_per_unit refuses"""
    m = fmx_amd.fmx
    x, rms = rm.signal(rm.SECONDS)
    n = x.shape[0] // 8 * 8
    bp, dk = oracle_kernels(ol)
    f = make(fmx_amd, 1, max_block=n // 8)
    f.rds_meter_enable(True)
    for k in range(8):
        f.process_host(x[k * (n // 8):(k + 1) * (n // 8)])
    recs = f.rds_meter_records()[0]
    k1 = f.rds_meter_cal(0)
    lp = np.zeros(251, np.float32)
    ol.oracle().fmo_lowpass_kernel(251, 165000 // 2, 2304000, ol.fptr(lp))
    want1 = rm.cal(bp, dk, [(f.taps(0, 0), 2304000.0), (lp, 2304000.0)])
    f.set_param(m.P_FM_DECODER, 5)
    with pytest.raises(m.FmxError) as e:
        f.rds_meter_cal(0)
    assert e.value.code == m.FMX_E_UNSUPPORTED
    f.close()
    f = make(fmx_amd, 2, max_block=16384, params=[(m.P_FILTER_RESTARTS, 2)])
    k2 = f.rds_meter_cal(1)
    want2 = rm.cal(bp, dk, [(f.taps(0, 1), 2304000.0)])
    f.close()
    for got, want in ((k1, want1), (k2, want2)):
        for name in ("gain", "phase0_deg", "path_57k"):
            assert abs(got[name] - want[name]) <= 1e-12 * abs(want[name]), (name, got[name], want[name])
    assert abs(k1["path_57k"] - k2["path_57k"]) < 1e-4 * k1["path_57k"]
    recs = recs[recs["index"] >= rm.FIRST_WINDOW]
    assert recs.size >= 8
    fig, mod = m.rds_meter_figures(recs, k1, m.mod_hz_per_unit(3, 192000)), rm.figures(recs, k1, rm.hz_per_unit())
    print("GPU figures: %s" % fig)
    for name in ("injection_rms_hz", "injection_peak_hz", "carrier_hz", "phase_deg", "axis_db"):
        assert abs(fig[name] - mod[name]) <= 1e-12 * abs(mod[name]), name
    assert abs(fig["injection_peak_hz"] / 2250.0 - 1.0) <= rm.INJECTION_PEAK_REL
    assert abs(fig["injection_rms_hz"] / (2250.0 * rms) - 1.0) <= rm.INJECTION_RMS_REL
    assert abs(fig["phase_deg"] - 90.0) <= rm.PHASE_TOL_DEG
    assert fig["axis_db"] >= rm.AXIS_CLEAN_DB - 10.0 * np.log10(2.0)


def build_demo(fmx_amd, exe):
    host = os.path.join(ROOT, "sdr-j-fm_amd", "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-I" + host, os.path.join(ROOT, "tests", "rdsm_demo", "rdsm_adapter_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])


def test_mirrors(fmx_amd, tmp_path):
    """fmx.py's FmProcessor mirror (setRdsMeter / pollRdsMeter) returns the records the handle's rds_meter_records returns; the C++ adapter
    (host/fm_processor_adapter.h: setRdsMeter, pollRdsMeter, rdsMeterCal, rdsMeterFigures) returns the same records and the same figures"""
    m = fmx_amd.fmx
    blocks = 60
    n = 16384 * blocks
    x = rm.signal(n / 2304000.0)[0][:n]
    res = []
    for mirror in (False, True):
        f = fmx_amd.Fmx(1, max_block=16384)
        f.set_param(m.P_BANDWIDTH, 165000)
        f.set_param(m.P_RDS_MODE, 2)
        if mirror:
            class Rig:
                pos = 0

                def Samples(self):
                    return n - self.pos

                def getSamples(self, k):
                    self.pos += k
                    return x[self.pos - k:self.pos]
            p = fmx_amd.FmProcessor(theDevice=Rig(), mySink=None, inputRate=2304000, fmx=f, channel=0, blockSize=16384)
            p.setRdsMeter(True)
            while p.run_block():
                pass
            res.append(p.pollRdsMeter())
        else:
            f.rds_meter_enable(True, 0)
            for k in range(blocks):
                f.process_host(x[k * 16384:(k + 1) * 16384])
            res.append(f.rds_meter_records(0, 1)[0])
            cal = f.rds_meter_cal(0)
        f.close()
    nwin = (n // R) // W
    assert nwin == 4 and res[0].size == nwin and res[0].tobytes() == res[1].tobytes()
    got = m.rds_meter_figures(res[0], cal, m.mod_hz_per_unit(3, 192000))
    exe, fin, fout = str(tmp_path / "rdsm_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "records.bin")
    build_demo(fmx_amd, exe)
    x.tofile(fin)
    out = subprocess.check_output([exe, fin, fout], timeout=120).decode().split()
    assert int(out[1]) == nwin and np.fromfile(fout, rm.RDSM_DTYPE).tobytes() == res[0].tobytes(), out
    for k, name in ((3, "injection_rms_hz"), (5, "injection_peak_hz"), (7, "carrier_hz"), (9, "phase_deg"), (11, "axis_db")):
        assert float(out[k]) == got[name], (name, out)

"""The multiplex spectrum meter on the GPU (fmx_mpx_spectrum_setup / _enable / _read, fmx_mpx_figures; csrc/fmx_mpx.hip) against the
float64 model of tests/mpx_model.py on the handle's own FMX_TAP_DEMOD.

The signal and the measure are mpx_model's (see its head): a noise-like multiplex, and per bin |P - P64| / max (P64, sqrt (P64 x the record's mean)).
Per case, level_worst is the larger of the worst bins of the two f32 restatements of the same records -- the plain one (radix-2, complex64) and
kernel_form (the header's own loader, stage functions and fold on the host, tests/mpx_check.cpp) --, level_median the larger of their medians; the GPU
must stay within 2 x level_worst on every bin and within 2 x level_median in the median -- mean and peak each.  Records of two cuts are compared bit
for bit, and only on handles whose taps do not depend on the cut (the PLL decoder, RF DC removal off), the taps' equality asserted first.
Shapes: 10 blocks of 4096 fm samples and 100 fm samples per channel (492 720 input samples)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mpx_model as mm
import spec_model as pm
import survey_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BINS, R = mm.N, mm.BINS, 12
N_FM = sm.stream_length(1)
CUTS = [R * c for c in sm.call_cuts(1)]      # three calls that complete no block, a block completed from the carry with a tail left, several blocks, a call
                                             # that ends exactly on a block end, a call of one fm sample, the rest


@pytest.fixture(scope="module")
def kernel_form(tmp_path_factory):
    cc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = tmp_path_factory.mktemp("mpx")
    exe = str(d / "mpx_check")
    subprocess.check_call([cc, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "mpx_check.cpp")])

    def run(x, B, S):
        """-> {index: (mean, peak)} of every record of the channel (one piece per record's worth: nothing is lost to the ring)"""
        fi, fo = str(d / "in.bin"), str(d / "out.bin")
        np.asarray(x, np.float32).tofile(fi)
        step = N * S * B
        cuts = [step] * (len(x) // step) + ([len(x) % step] if len(x) % step else [])
        subprocess.check_call([exe, "spectrum", fi, fo, str(B), str(S), "0", "64"] + [str(c) for c in cuts])
        raw = np.fromfile(fo, np.float32).reshape(-1, 1 + 2 * BINS)
        return {int(row[0]): (row[1:1 + BINS], row[1 + BINS:]) for row in raw}
    return run


_IQ = {}


def iq_streams(streams=3, n_fm=N_FM):
    """[streams, 12 n_fm, 2] f32: the noise-like multiplex with one seed per stream, frequency-modulated in float64 onto a carrier of amplitude 0.5"""
    if (streams, n_fm) not in _IQ:
        x = np.stack([mm.fm_iq(mm.noise_mpx(n_fm, seed=s, oversample=R), 192000 * R) for s in range(streams)])
        _IQ[streams, n_fm] = np.ascontiguousarray(x.view(np.float32).reshape(streams, n_fm * R, 2))
    return _IQ[streams, n_fm]


def cut_free(m):
    """the handles whose taps do not depend on how the stream is cut (tests/test_gpu_mod_meter.py cut_free)"""
    return [(m.P_FM_DECODER, 2), (m.P_DC_REMOVE, 0)]


def expected_indices(cuts_fm, B, S, first=0, read_every_call=True):
    """the records a reader gets that reads behind every call (or behind the last only): of the records a call completes the ring keeps the last four"""
    out, ring, g = [], {}, 0
    for n in cuts_fm:
        for r in range(pm.n_blocks(g, S) // B, pm.n_blocks(g + n, S) // B):
            if r * B >= first:
                ring[r % mm.RING] = r
        g += n
        if read_every_call:
            out += sorted(r for r in ring.values() if not out or r > out[-1])
    return out if read_every_call else sorted(ring.values())


class Run:
    """One handle fed x ([streams, n, 2] f32) in calls of the given input-sample lengths; the metered channels' records read behind every call (or behind
    the last) in one range read per channel: idx [c], mean [c], peak [c], recs [c]; FMX_TAP_DEMOD of the channels of tap_ch read behind every call with
    fmx_last_fm_samples and concatenated: taps [c]."""

    def __init__(self, fmx_amd, x, cuts, B=2, S=1, metered=(0, 2), channels=None, streams=None, params=(), via="host", tap_ch=(), read_every_call=True,
                 each=None, keep_pcm=False):
        m = fmx_amd.fmx
        ns, n = x.shape[0], x.shape[1]
        channels = ns if channels is None else channels
        assert sum(cuts) == n
        f = fmx_amd.Fmx(channels, streams=ns if channels != ns else 0, stream_of_channel=[c % ns for c in range(channels)] if channels != ns else None,
                        max_block=max(cuts))
        read = sorted(set(metered))
        self.recs, self.mean, self.peak = ({c: [] for c in range(channels)} for _ in range(3))
        taps, pcm, self.pieces = {c: [] for c in tap_ch}, [], []
        try:
            for item in params:
                f.set_param(*item)
            f.mpx_spectrum_setup(B, S)
            for c in metered:
                f.mpx_spectrum_meter(True, c)
            if via == "device":
                import torch
                d_iq = torch.from_numpy(x).cuda()
                cap = max(f.frames_for(max(cuts)) + 64, 64)
                d_pcm = torch.zeros((channels, cap, 2), dtype=torch.float32, device="cuda")
            pos = 0
            for k, ln in enumerate(cuts):
                if each:
                    each(f, k)
                if via == "device":
                    got = C.c_int64()
                    f._check(f.L.fmx_process_device_raw(f.h, C.c_void_p(d_iq.data_ptr() + 8 * pos), m.IQ_F32, 2048.0, n, ln, C.c_void_p(d_pcm.data_ptr()), cap,
                                                        C.byref(got), None))
                    f.synchronize()
                else:
                    p = f.process_host_raw(x[:, pos:pos + ln], m.IQ_F32)
                    if keep_pcm:
                        pcm.append(p.copy())
                pos += ln
                self.pieces.append(f.last_call_pieces())
                nj = f.last_fm_samples()
                for c in tap_ch:
                    if nj > 0:
                        taps[c].append(f.tap(m.TAP_DEMOD, nj, c))
                if read_every_call or k == len(cuts) - 1:
                    for c in range(channels) if channels <= 3 else read:
                        r, mean, peak = f.mpx_spectrum_read(c, 1)[0]
                        self.recs[c] += list(r); self.mean[c] += list(mean); self.peak[c] += list(peak)
            self.taps = {c: np.concatenate(v) for c, v in taps.items()}
            self.pcm = np.concatenate(pcm, axis=1) if keep_pcm else None
            self.facts = (f.last_second_group(), f.last_call_pieces(), f.last_front_kernel())
        finally:
            f.close()
        self.idx = {c: [int(r["index"]) for r in rs] for c, rs in self.recs.items()}
        self.mean = {c: np.array(v, np.float32).reshape(-1, BINS) for c, v in self.mean.items()}
        self.peak = {c: np.array(v, np.float32).reshape(-1, BINS) for c, v in self.peak.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def common(a, b, c, cb=None):
    """the records of channel c both runs delivered -> (indices, a's mean, peak, b's mean, peak)"""
    cb = c if cb is None else cb
    idx = [r for r in a.idx[c] if r in b.idx[cb]]
    ia, ib = [a.idx[c].index(r) for r in idx], [b.idx[cb].index(r) for r in idx]
    return idx, a.mean[c][ia], a.peak[c][ia], b.mean[cb][ib], b.peak[cb][ib]


def against_the_model(tag, run, taps, kernel_form, chans, B, S, want):
    """the records of `chans` within the bound of the float64 model on the taps"""
    M64, K64, M32, K32, MKF, KKF, GM, GK = ([] for _ in range(8))
    for c in chans:
        d = taps[c]
        idx, m64, k64 = mm.records64(d, B, S)
        _, m32, k32 = mm.records32(d, B, S)
        kf = kernel_form(d, B, S)
        assert run.idx[c] == want and set(want) <= set(idx) and sorted(kf) == idx, (c, run.idx[c], want, idx)
        M64.append(m64[want]); K64.append(k64[want]); M32.append(m32[want]); K32.append(k32[want])
        MKF.append(np.stack([kf[r][0] for r in want])); KKF.append(np.stack([kf[r][1] for r in want]))
        GM.append(run.mean[c]); GK.append(run.peak[c])
    M64, K64, M32, K32, MKF, KKF, GM, GK = (np.concatenate(v) for v in (M64, K64, M32, K32, MKF, KKF, GM, GK))
    assert GM.shape == (len(chans) * len(want), BINS) and np.all(np.isfinite(GM)) and np.all(np.isfinite(GK))
    print("\n[%s] a record's bins span %.1f dB" % (tag, mm.span_db(M64)))
    lw, lm = mm.levels(M64, M32, MKF)
    ok, rw, rm = mm.check("GPU mean, " + tag, GM, M64, lw, lm)
    assert ok, (rw, rm)
    ok, rw, rm = mm.check("GPU peak, " + tag, GK, K64, *mm.levels(K64, K32, KKF))
    assert ok, (rw, rm)
    return GM, GK


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(1, 1), (2, 1), (2, 3)])
def test_records_against_the_float64_model_on_the_handles_taps(fmx_amd, kernel_form, B, S):
    """A 3-channel handle (scope taps on by default), channels 0 and 2 metered, channel 1 not; calls cut at 12 x survey_model.call_cuts (1)."""
    run = Run(fmx_amd, iq_streams(), CUTS, B, S, tap_ch=(0, 2))
    want = expected_indices(sm.call_cuts(1), B, S)
    assert len(want) >= 2 and run.idx[1] == [] and all(t.size == N_FM for t in run.taps.values())
    for c in (0, 2):
        recs = run.recs[c]
        assert [int(r["end_sample"]) for r in recs] == [N * S * ((r + 1) * B - 1) + N for r in want]
        assert all(int(r["blocks"]) == B and int(r["every"]) == S for r in recs)
    GM, GK = against_the_model("B = %d, S = %d" % (B, S), run, run.taps, kernel_form, (0, 2), B, S, want)
    if B == 1:
        assert same_bits(GM, GK)                                # (one block a record: c = c1, the sum of one is the maximum of one)


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S", [(2, 1), (2, 3)])
def test_cuts_are_bit_identical(fmx_amd, B, S):
    """One call against the cuts -- which hold three calls in a row that complete no block, a call that ends exactly on a block end and a call of one
    fm sample --, and fmx_process_host_raw against fmx_process_device_raw: the same taps, then the same records, byte for byte."""
    m = fmx_amd.fmx
    x = iq_streams()
    n = x.shape[1]
    whole = Run(fmx_amd, x, [n], B, S, params=cut_free(m), tap_ch=(0, 2))
    cut = Run(fmx_amd, x, CUTS, B, S, params=cut_free(m), tap_ch=(0, 2))
    dev = Run(fmx_amd, x, CUTS, B, S, params=cut_free(m), via="device", tap_ch=(0, 2))
    for c in (0, 2):
        assert whole.taps[c].tobytes() == cut.taps[c].tobytes() == dev.taps[c].tobytes(), c      # (the premise)
        assert cut.idx[c] == dev.idx[c] == expected_indices(sm.call_cuts(1), B, S) and whole.idx[c] == expected_indices([N_FM], B, S)
        assert same_bits(cut.mean[c], dev.mean[c]) and same_bits(cut.peak[c], dev.peak[c])
        idx, am, ak, bm, bk = common(whole, cut, c)
        assert len(idx) >= 2 and same_bits(am, bm) and same_bits(ak, bk)
    assert not same_bits(cut.mean[0], cut.mean[2])


def test_calls_of_one_fm_sample_across_a_block_end(fmx_amd):
    m = fmx_amd.fmx
    x = iq_streams()
    single = Run(fmx_amd, x[:, :R * (N + 3)], [R * (N - 1), R, R, R, R], 1, 1, params=cut_free(m), tap_ch=(0,))
    block = Run(fmx_amd, x[:, :R * (N + 3)], [R * (N + 3)], 1, 1, params=cut_free(m), tap_ch=(0,))
    assert single.taps[0].tobytes() == block.taps[0].tobytes()
    for c in (0, 2):
        assert single.idx[c] == block.idx[c] == [0] and same_bits(single.mean[c], block.mean[c]) and same_bits(single.peak[c], block.peak[c])
        assert int(single.recs[c][0]["end_sample"]) == N


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_rds_pieces(fmx_amd):
    """One call of 400 000 input samples with the RDS decoder on is made in RDS pieces (at most 31 999 fm samples each): the records are those of the same
    stream in calls of 16 384."""
    m = fmx_amd.fmx
    n = 400000
    x = iq_streams(1, N_FM)[:, :n]
    params = cut_free(m) + [(m.P_RDS_MODE, 2)]
    one = Run(fmx_amd, x, [n], 2, 1, metered=(0,), params=params)
    small = Run(fmx_amd, x, [16384] * (n // 16384) + [n % 16384], 2, 1, metered=(0,), params=params)
    assert n // R > 31999 and small.idx[0] == list(range((n // R) // N // 2)) == one.idx[0] and len(one.idx[0]) == 4
    assert same_bits(one.mean[0], small.mean[0]) and same_bits(one.peak[0], small.peak[0])


def test_overlapping_pieces(fmx_amd):
    """A 1024-channel PLL-decoder handle on 2 shared streams makes a call of 98 304 input samples in overlapping pieces of 1536 fm samples; channels 0, 1
    and 1023 metered.  The records are those of the same calls made whole."""
    m = fmx_amd.fmx
    n = 98304
    x = iq_streams(2, N_FM)[:, :2 * n]
    res = []
    for pieces in (1536, 0):
        res.append(Run(fmx_amd, x, [n, n], 1, 1, metered=(0, 1, 1023), channels=1024, params=cut_free(m) + [(m.P_CALL_PIECES, pieces)]))
    big, whole = res
    assert big.pieces[0] > 1 and whole.pieces == [1, 1]
    for c in (0, 1, 1023):
        assert big.idx[c] == whole.idx[c] == [0, 1, 2, 3]
        assert same_bits(big.mean[c], whole.mean[c]) and same_bits(big.peak[c], whole.peak[c])
    assert same_bits(big.mean[1], big.mean[1023]) and not same_bits(big.mean[0], big.mean[1])      # (channels 1 and 1023 share a stream)


def test_stage_b_as_one_kernel_and_as_two(fmx_amd):
    m = fmx_amd.fmx
    n = R * (2 * N + 100)
    x = iq_streams(3)[:, :n]
    a, b = (Run(fmx_amd, x, [n // 2, n // 2], 1, 1, metered=(0, 129), channels=130, params=cut_free(m) + [(m.P_STAGEB_FORM, form)]) for form in (1, 2))
    for c in (0, 129):
        assert a.idx[c] == b.idx[c] == [0, 1] and same_bits(a.mean[c], b.mean[c]) and same_bits(a.peak[c], b.peak[c])


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_without_scope_taps(fmx_amd, kernel_form):
    """130 channels on 3 streams, channels 0, 1 and 129 metered, scope taps off by default: the records equal those of the same handle with
    FMX_P_SCOPE_TAPS = 1, and those are within the bound of the model on its taps."""
    m = fmx_amd.fmx
    x = iq_streams()
    off = Run(fmx_amd, x, CUTS, 2, 1, metered=(0, 1, 129), channels=130)
    on = Run(fmx_amd, x, CUTS, 2, 1, metered=(0, 1, 129), channels=130, params=[(m.P_SCOPE_TAPS, 1)], tap_ch=(0, 1, 129))
    want = expected_indices(sm.call_cuts(1), 2, 1)
    for c in (0, 1, 129):
        assert off.idx[c] == on.idx[c] == want and same_bits(off.mean[c], on.mean[c]) and same_bits(off.peak[c], on.peak[c])
    against_the_model("130 channels", on, on.taps, kernel_form, (0, 1, 129), 2, 1, want)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------------
def everything(f, channels):
    """what a handle delivers beside the multiplex spectrum meter"""
    some = sorted({0, min(1, channels - 1), channels - 1})
    return dict(meta=[bytes(f.meta(c)) for c in range(channels)], bits=[f.rds_bits(c).tobytes() for c in some], peaks=[f.peaks(c).tobytes() for c in some] if channels <= 64 else [b""],      # (a display feed: up to 64 channels)
                scan=[f.scan_results(c).tobytes() for c in some], mod=[r.tobytes() for r in f.mod_records()], audio=[r.tobytes() for r in f.audio_records()],
                rx=[r.tobytes() for r in f.rx_records()], rdsm=[r.tobytes() for r in f.rds_meter_records()],
                spec=[b"".join(a.tobytes() for a in f.spectrum_read(s)) for s in range(f.streams)],
                facts=(f.last_second_group(), f.last_call_pieces(), f.last_front_kernel()))


@pytest.mark.parametrize("channels", [1, 130])
def test_everything_else_is_undisturbed(fmx_amd, ol, channels):
    """With the meter on for every channel, PCM, RDS bits, meta, peaks, scan records, the five other meters' records and the facts about the last call
    equal a twin handle's without it, bit for bit: on a 1-channel block-machine handle and on a batch of 130 channels on 3 shared streams (whose last
    channel scans)."""
    m = fmx_amd.fmx
    blk, ncalls = 16384, 24
    streams = 1 if channels == 1 else 3
    x = np.stack([ol.synth_iq(ncalls * blk, rds=1, leftHz=500.0 + 300 * s, rightHz=900.0 + 200 * s) for s in range(streams)])
    out = []
    for meter in (False, True):
        f = fmx_amd.Fmx(channels, streams=streams if channels > 1 else 0, stream_of_channel=[c % streams for c in range(channels)] if channels > 1 else None,
                        max_block=blk)
        f.set_param(m.P_BANDWIDTH, 165000)
        f.set_param(m.P_RDS_MODE, 2)
        if channels > 1:
            f.set_param(m.P_SCANNING, 1, channels - 1)
        f.mod_meter(True); f.audio_meter(True); f.rx_meter(True); f.rds_meter_enable(True)
        f.spectrum_setup(2, 1); f.spectrum_meter(True)
        if meter:
            f.mpx_spectrum_setup(2, 1)
            f.mpx_spectrum_meter(True)
        pcm = np.concatenate([f.process_host(x[:, k * blk:(k + 1) * blk]) for k in range(ncalls)], axis=1)
        e = everything(f, channels)
        e["pcm"] = pcm
        e["mpx"] = [r[0] for r in f.mpx_spectrum_read(0, channels)]
        out.append(e)
        f.close()
    a, b = out
    assert np.array_equal(a["pcm"], b["pcm"]) and a["pcm"].shape[1] > 0
    for key in ("meta", "bits", "peaks", "scan", "mod", "audio", "rx", "rdsm", "spec", "facts"):
        assert a[key] == b[key], key
    assert len(a["bits"][0]) > 0 and len(a["mod"][0]) > 0 and len(a["audio"][0]) > 0 and len(a["rx"][0]) > 0 and len(a["rdsm"][0]) > 0 and len(a["spec"][0]) > 0
    assert (len(a["scan"][-1]) > 0) == (channels > 1) and (len(a["peaks"][0]) > 0) == (channels == 1)
    assert all(r.size == 0 for r in a["mpx"]) and all(list(r["index"]) == [0, 1, 2, 3] for r in b["mpx"])      # (32 768 fm samples: 8 blocks)


def test_the_second_group_is_the_modulation_meters(fmx_amd, ol):
    """a batch with ONE channel's meter on writes the rows for every channel and is no plain batch: fmx_last_second_group, and the PCM, are those of a twin
    with only the modulation meter on the same channel; a twin without either is a plain batch"""
    m = fmx_amd.fmx
    blk = 49152                                     # (three calls: 12 288 fm samples, one window of the modulation meter)
    x = np.stack([ol.synth_iq(3 * blk, leftHz=500.0 + 300 * s) for s in range(2)])
    res = []
    for which in ("none", "mod", "mpx"):
        f = fmx_amd.Fmx(1100, streams=2, stream_of_channel=[c % 2 for c in range(1100)], max_block=blk)      # (768 + 332: tests/test_gpu_mod_meter.py)
        f.set_param(m.P_BANDWIDTH, 165000)
        if which == "mod":
            f.mod_meter(True, 5)
        if which == "mpx":
            f.mpx_spectrum_meter(True, 5)
        pcm = np.concatenate([f.process_host(x[:, k * blk:(k + 1) * blk]) for k in range(3)], axis=1)
        res.append((f.last_second_group(), f.last_call_pieces(), f.last_front_kernel(), pcm, f.mod_records(5, 1)[0].size))
        f.close()
    none, mod, mpx = res
    assert mpx[:3] == mod[:3] and np.array_equal(mpx[3], mod[3]) and np.array_equal(mpx[3], none[3])
    assert none[0] == 332 and mod[0] == 0 and mod[4] > 0 and mpx[4] == 0


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_switch_ring_and_cursors(fmx_amd):
    m = fmx_amd.fmx
    x = iq_streams(3, 24 * N)
    B, S = 2, 1
    ref = Run(fmx_amd, x, [R * 2 * N] * 12, B, S, metered=(0, 1, 2), params=cut_free(m), tap_ch=(0,))      # on throughout: records 0 .. 11
    assert ref.idx[0] == list(range(12))
    f = fmx_amd.Fmx(3, max_block=R * 4 * N)
    twin = fmx_amd.Fmx(3, max_block=R * 4 * N)
    try:
        taps = []
        for h in (f, twin):
            for item in cut_free(m):
                h.set_param(*item)
            h.mpx_spectrum_setup(B, S)
        twin.mpx_spectrum_meter(True)
        read = lambda c, **kw: f.mpx_spectrum_read(c, 1, **kw)[0]

        def call(g, n):
            for h in (f, twin):
                h.process_host_raw(x[:, R * g:R * (g + n)], m.IQ_F32)
            taps.append(f.tap(m.TAP_DEMOD, f.last_fm_samples(), 0))
            return g + n
        g = call(0, N + 100)                                    # (no meter yet: nothing is allocated, nothing is read)
        assert read(0)[0].size == 0
        f.mpx_spectrum_meter(True, 0)                           # in mid-stream, inside block 1: the first block is 2, the first whole record 1
        with pytest.raises(fmx_amd.FmxError) as e:              # the grid is fixed while a meter is on
            f.mpx_spectrum_setup(4, 1)
        assert e.value.code == m.FMX_E_INVALID and "on" in str(e.value)
        g = call(g, 3 * N)                                      # blocks 1 (not taken), 2, 3 complete
        r, mean, peak = read(0)
        assert list(r["index"]) == [1] and int(r["end_sample"][0]) == 4 * N
        assert same_bits(mean[0], ref.mean[0][1]) and same_bits(peak[0], ref.peak[0][1])
        f.mpx_spectrum_meter(True, 2)                           # a second channel: its memory is added, channel 0's is kept
        g = call(g, 2 * N - 100)                                # g = 6 N: record 2 complete for channel 0; channel 2 switched on inside block 4
        r, mean, peak = read(0)
        assert list(r["index"]) == [2] and same_bits(mean[0], ref.mean[0][2]) and read(2)[0].size == 0
        f.mpx_spectrum_meter(False, 0)
        g = call(g, 2 * N)                                      # record 3: channel 0 is off, channel 2's first whole record
        r, mean, peak = read(2)
        assert read(0)[0].size == 0 and list(r["index"]) == [3] and same_bits(mean[0], ref.mean[2][3]) and same_bits(peak[0], ref.peak[2][3])
        f.mpx_spectrum_meter(True, 0)
        g = call(g, N)                                          # channel 0 on again at 8 N: block 8 taken, record 4 begun
        g = call(g, 5 * N // 2)                                 # 11.5 N: record 4 complete
        r, mean, peak = read(0)
        assert list(r["index"]) == [4]                          # a gap in index: record 3 was not metered
        assert same_bits(mean[0], ref.mean[0][4]) and same_bits(peak[0], ref.peak[0][4])      # no stale sums
        # five records unread: the oldest is lost, and index shows it; capacity smaller than what is there; independent cursors
        g = call(g, N // 2)                                     # 12 N: record 5
        for _ in range(4):
            g = call(g, 2 * N)                                  # records 6 .. 9
        assert np.concatenate(taps).tobytes() == ref.taps[0][:g].tobytes()                  # (the premise of every comparison with ref above)
        assert list(read(2, capacity=1)[0]["index"]) == [6]     # channel 2 never read 4 and 5: of 4 .. 9 the ring holds 6 .. 9
        assert list(read(0, capacity=3)[0]["index"]) == [6, 7, 8]
        # a range read of channels 0 .. 2 equals three single reads on the twin (every channel on throughout there; f's channel 1 never was)
        got = f.mpx_spectrum_read(0, 3)
        singles = [twin.mpx_spectrum_read(c, 1)[0] for c in range(3)]
        assert [list(r[0]["index"]) for r in got] == [[9], [], [7, 8, 9]] and all(list(s[0]["index"]) == [6, 7, 8, 9] for s in singles)
        for c in (0, 2):
            k = len(got[c][0])
            assert got[c][0].tobytes() == singles[c][0][-k:].tobytes() and same_bits(got[c][1], singles[c][1][-k:]) and same_bits(got[c][2], singles[c][2][-k:])
            assert same_bits(singles[c][1], ref.mean[c][6:10])
        assert all(r[0].size == 0 for r in f.mpx_spectrum_read(0, 3))
        assert read(0, peak=False)[2] is None
        with pytest.raises(fmx_amd.FmxError):
            f.mpx_spectrum_read(2, 2)                           # (channels 2 .. 3 of 3)
        f.mpx_spectrum_meter(False)
        g = call(g, N)                                          # every meter off: two calls in which the meter has nothing to do, then on again
        g = call(g, N)
        assert all(r[0].size == 0 for r in f.mpx_spectrum_read(0, 3))
        f.mpx_spectrum_setup(1, 2)                              # a new grid: indices and cursors start over
        f.mpx_spectrum_meter(True, 1)
        f.process_host_raw(x[:, R * g:R * (g + 2 * N)], m.IQ_F32)
        r, _, _ = read(1)
        assert list(r["index"]) == [11] and int(r["every"][0]) == 2 and int(r["end_sample"][0]) == 23 * N       # (block 11 begins at 22 N)
    finally:
        f.close(); twin.close()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------------------------
# (measured on an MI355X; the bounds are twice the measurements)
PILOT_HZ_BOUND = 190.0          # measured 94.857 Hz: 7115.725 against the modulation meter's 7210.582
PILOT_FREQ_BOUND = 0.182        # measured 0.0907 Hz
RDS_HZ_BOUND = 1099.3           # measured 549.628 Hz: 695.924 against the RDS meter's 1245.552 -- two different quantities, see the test
RDS_CAL_BOUND = 435.2           # measured 217.565 Hz: rds_hz sqrt (2) / path_57k = 1463.117 against the same 1245.552, like for like


def test_figures_end_to_end(fmx_amd, ol):
    """The oracle generator's default stereo signal with RDS, 1.28 s in calls of 196 608 input samples, B = 48: pilot_hz against the modulation meter's
    hypot (pilot_i, pilot_q) over the same second on the same handle, pilot_freq_hz against 19 000, rds_hz against the RDS meter's rms injection."""
    m = fmx_amd.fmx
    blk, ncalls = 196608, 15
    x = ol.synth_iq(ncalls * blk, rds=1)
    f = fmx_amd.Fmx(1, max_block=blk)
    try:
        f.set_param(m.P_BANDWIDTH, 165000)
        f.set_param(m.P_RDS_MODE, 2)
        f.mod_meter(True); f.rds_meter_enable(True); f.mpx_spectrum_meter(True)       # (the default grid: B = 48, S = 1)
        mod, rdsm = [], []
        for k in range(ncalls):
            f.process_host(x[k * blk:(k + 1) * blk])
            mod += list(f.mod_records(0, 1)[0]); rdsm += list(f.rds_meter_records(0, 1)[0])
        recs, mean, peak = f.mpx_spectrum_read(0, 1)[0]
        cal = f.rds_meter_cal(0)
    finally:
        f.close()
    assert list(recs["index"]) == [0] and int(recs["end_sample"][0]) == 48 * N and int(recs["blocks"][0]) == 48
    u = m.mod_hz_per_unit(3, 192000)
    figs = fmx_amd.mpx_figures(mean[0], peak[0], rate_hz=192000, hz_per_unit=u)
    print("\nfigures: %s" % figs)
    mod = np.array(mod)
    inside = mod[(mod["end_sample"] <= 48 * N) & (mod["index"] >= 4)]          # (the windows of the record's second, behind the PLL's first 0.2 s)
    pilot_mod = float(np.mean(np.hypot(inside["pilot_i"].astype(np.float64), inside["pilot_q"].astype(np.float64)))) * u
    rdsm = np.array(rdsm)
    rds_fig = m.rds_meter_figures(rdsm[rdsm["index"] >= 2], cal, u)
    d_pilot, d_freq, d_rds = abs(figs["pilot_hz"] - pilot_mod), abs(figs["pilot_freq_hz"] - 19000.0), abs(figs["rds_hz"] - rds_fig["injection_rms_hz"])
    print("pilot_hz %.3f against the modulation meter's %.3f: %.3f apart (bound %s)" % (figs["pilot_hz"], pilot_mod, d_pilot, PILOT_HZ_BOUND))
    print("pilot_freq_hz %.4f against 19 000: %.4f apart (bound %s)" % (figs["pilot_freq_hz"], d_freq, PILOT_FREQ_BOUND))
    # (rds_hz is the rms deviation of the band as d holds it; the RDS meter's figure is the rms of the sub-carrier's AMPLITUDE -- sqrt (2) more --, referred to
    # the antenna through path_57k, and reads low under programme.  Both comparisons are asserted: the plain difference, and like for like)
    rds_cal = figs["rds_hz"] * np.sqrt(2.0) / cal["path_57k"]
    d_cal = abs(rds_cal - rds_fig["injection_rms_hz"])
    print("rds_hz sqrt (2) / path_57k (%.6f) = %.3f against the same: %.3f apart (bound %s)" % (cal["path_57k"], rds_cal, d_cal, RDS_CAL_BOUND))
    print("rds_hz %.3f against the RDS meter's rms injection %.3f: %.3f apart (bound %s)" % (figs["rds_hz"], rds_fig["injection_rms_hz"], d_rds, RDS_HZ_BOUND))
    assert inside.size >= 15 and d_pilot <= PILOT_HZ_BOUND and d_freq <= PILOT_FREQ_BOUND and d_rds <= RDS_HZ_BOUND and d_cal <= RDS_CAL_BOUND


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_cpp_demo_builds_and_runs(fmx_amd, tmp_path):
    """tests/mpx_demo through host/fm_processor_adapter.h: blocks of 16 384, B = 2: the records the Python handle delivers for the same stream"""
    import test_mpx_cpu
    exe, fin, fout = str(tmp_path / "mpx_adapter_demo"), str(tmp_path / "iq.f32"), str(tmp_path / "mpx.bin")
    test_mpx_cpu.build_demo(fmx_amd, exe)
    x = iq_streams(1, N_FM)[:, :24 * 16384]
    x[0].tofile(fin)
    out = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    lines = out.stdout.decode().splitlines()
    assert out.returncode == 0 and lines[-1].startswith("records 4 "), lines
    rows = np.fromfile(fout, np.float32).reshape(-1, 1 + 2 * BINS)
    run = Run(fmx_amd, x, [16384] * 24, 2, 1, metered=(0,))
    assert [int(v) for v in rows[:, 0]] == run.idx[0] == [0, 1, 2, 3]
    assert same_bits(rows[:, 1:1 + BINS], run.mean[0]) and same_bits(rows[:, 1 + BINS:], run.peak[0])
    figs = fmx_amd.mpx_figures(run.mean[0][-1], run.peak[0][-1], hz_per_unit=1.0)
    assert [float(v) for v in lines[-1].split()[3::2]] == [figs["total_hz"], figs["pilot_hz"], figs["pilot_freq_hz"]]

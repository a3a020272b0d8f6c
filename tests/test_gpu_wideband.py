"""Stage W, the wide-band ingest stage (fmx_wide.hip, include/fmx.h fmx_wideband), on the GPU against the float64 model of
tests/wideband_model.py.

The bound of every comparison with the model: the GPU's error (RMS relative to the output's RMS, per output) may be at most 3 x the error
of the model's f32 restatement of the same call (taps, samples and oscillator in f32, accumulation in tap order); the factor covers
another summation order and the folded-tap form.  Shapes: 2 streams, 3 outputs each, three tiles of 256 outputs and a ragged rest."""
import ctypes as C

import numpy as np
import pytest

import wideband_model as wm

pytestmark = pytest.mark.gpu

TILE = 256
N_OUT = 3 * TILE + 37
FACTORS = [2, 5, 16]
FMT_NAMES = {0: "F32", 1: "U8", 2: "S8", 3: "S16/2048"}
SOF = [0, 0, 0, 1, 1, 1]


def offsets(K):
    lim = wm.offset_limit(K)
    return [0, -412345, lim - 1, -lim, 733001, 100000]


def wide_signal(K, n, fmt, seed=0):
    """Two streams [2, n, 2] in the raw format: a carrier with a slow phase wobble at every output's offset, and noise."""
    rng = np.random.default_rng(1000 * K + seed)
    Rw = K * wm.NARROW_RATE
    t = np.arange(n, dtype=np.float64)
    offs = offsets(K)
    x = np.zeros((2, n), np.complex128)
    for m, f in enumerate(offs):
        x[SOF[m]] += 0.2 * np.exp(1j * (2 * np.pi * f * t / Rw + 3.0 * np.sin(2 * np.pi * (900.0 + 400 * m) * t / Rw) + m))
    x += 0.02 * (rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n)))
    v = np.stack([x.real, x.imag], axis=-1)
    if fmt == 0:
        return v.astype(np.float32)
    if fmt == 1:
        return np.clip(np.rint(v * 128.0 + 127.0), 0, 255).astype(np.uint8)
    if fmt == 2:
        return np.clip(np.rint(v * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint(v * 2048.0), -32768, 32767).astype(np.int16)


def models(K):
    offs = offsets(K)
    return [wm.WidebandModel(K, [offs[m] for m in range(6) if SOF[m] == s]) for s in range(2)]


def model_call(mods, raw, fmt):
    """-> (f64 model, f32 restatement), each [6, n / K]"""
    ys = [mods[s].process(wm.convert(raw[s], fmt), with_f32=True) for s in range(2)]
    return np.concatenate([ys[0][0], ys[1][0]]), np.concatenate([ys[0][1], ys[1][1]])


def cplx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def check_bound(tag, got, ref, ref32):
    worst = 0.0
    for m in range(got.shape[0]):
        e_gpu, e_f32 = wm.rel_rms(got[m], ref[m]), wm.rel_rms(ref32[m], ref[m])
        print("[%s, output %d] GPU vs f64 model %.3e, f32 restatement vs f64 model %.3e (ratio %.2f)" % (tag, m, e_gpu, e_f32, e_gpu / e_f32))
        worst = max(worst, e_gpu / e_f32)
        assert e_gpu <= 3.0 * e_f32, (tag, m, e_gpu, e_f32)
    return worst


def run_against_model(fmx_amd, K, fmt):
    raw = wide_signal(K, N_OUT * K, fmt)
    w = fmx_amd.Wideband(K, SOF, offsets(K), streams=2, max_block=N_OUT * K)
    try:
        got = cplx(w.process_host(raw, fmt, 2048.0))
    finally:
        w.close()
    assert got.shape == (6, N_OUT)
    ref, ref32 = model_call(models(K), raw, fmt)
    print()
    check_bound("K = %d, %s" % (K, FMT_NAMES[fmt]), got, ref, ref32)


@pytest.mark.parametrize("K", FACTORS)
def test_against_the_float64_model(fmx_amd, K):
    run_against_model(fmx_amd, K, 0)


@pytest.mark.parametrize("fmt", [1, 2, 3])
@pytest.mark.parametrize("K", FACTORS)
def test_raw_formats(fmx_amd, K, fmt):
    """U8, S8 and S16 / 2048, each against the model fed the converted values."""
    run_against_model(fmx_amd, K, fmt)


@pytest.mark.parametrize("K", FACTORS)
def test_cuts_are_bit_identical(fmx_amd, K):
    """One call against the same samples in calls of K, 7 K and the rest."""
    raw = wide_signal(K, N_OUT * K, 0)
    w = fmx_amd.Wideband(K, SOF, offsets(K), streams=2, max_block=N_OUT * K)
    whole = w.process_host(raw)
    w.close()
    w = fmx_amd.Wideband(K, SOF, offsets(K), streams=2, max_block=N_OUT * K)
    parts = [w.process_host(raw[:, :K]), w.process_host(raw[:, K:8 * K]), w.process_host(raw[:, 8 * K:])]
    w.close()
    cut = np.concatenate(parts, axis=1)
    assert cut.shape == whole.shape
    assert np.array_equal(cut.view(np.uint32), whole.view(np.uint32))


@pytest.mark.parametrize("K", FACTORS)
def test_call_length_must_be_a_multiple_of_the_factor(fmx_amd, K):
    """n_wide not a multiple of K answers FMX_E_INVALID (the check needs an object, hence a device) and leaves the stream where it was."""
    raw = wide_signal(K, 40 * K, 0)
    w = fmx_amd.Wideband(K, SOF, offsets(K), streams=2, max_block=40 * K)
    ref = fmx_amd.Wideband(K, SOF, offsets(K), streams=2, max_block=40 * K)
    try:
        a = w.process_host(raw[:, :20 * K])
        for bad in (1, K - 1, K + 1, 20 * K - 1):
            with pytest.raises(fmx_amd.FmxError) as e:
                w.process_host(raw[:, :bad])
            assert e.value.code == fmx_amd.fmx.FMX_E_INVALID and "multiple" in str(e.value)
        with pytest.raises(fmx_amd.FmxError) as e:
            w.process_host(np.concatenate([raw, raw], axis=1))
        assert e.value.code == fmx_amd.fmx.FMX_E_TOO_LARGE
        b = w.process_host(raw[:, 20 * K:])
        whole = ref.process_host(raw)
    finally:
        w.close()
        ref.close()
    assert np.array_equal(np.concatenate([a, b], axis=1).view(np.uint32), whole.view(np.uint32))


@pytest.mark.parametrize("K", FACTORS)
def test_offset_change_between_calls(fmx_amd, K):
    """Offsets change between calls -- once behind a long call, again behind a call of 3 K samples and again behind one of K samples, so
    that the windows of the following outputs hold samples of up to four offsets: the T - 1 samples that straddle the changes, and the
    outputs behind them, must meet the bound against the model with the same switches."""
    n_a = TILE + 11
    cuts = [n_a * K, 3 * K, K, (N_OUT - n_a - 4) * K]
    lim = wm.offset_limit(K)
    changes = [{1: 250000, 4: -lim + 1}, {1: -90001, 5: 0}, {1: lim}]
    raw = wide_signal(K, N_OUT * K, 0)
    w = fmx_amd.Wideband(K, SOF, offsets(K), streams=2, max_block=N_OUT * K)
    mods = models(K)
    local = {m: (SOF[m], [q for q in range(6) if SOF[q] == SOF[m]].index(m)) for m in range(6)}
    got, ref, ref32, pos = [], [], [], 0
    try:
        for k, ln in enumerate(cuts):
            if k > 0:
                for m, f in changes[k - 1].items():
                    w.set_offset(m, f)
                    mods[local[m][0]].set_offset(local[m][1], f)
            got.append(cplx(w.process_host(raw[:, pos:pos + ln])))
            a, b = model_call(mods, raw[:, pos:pos + ln], 0)
            ref.append(a)
            ref32.append(b)
            pos += ln
        with pytest.raises(fmx_amd.FmxError) as e:
            w.set_offset(0, lim + 1)
        assert e.value.code == fmx_amd.fmx.FMX_E_INVALID
        with pytest.raises(fmx_amd.FmxError) as e:                   # a call's length must be a multiple of K
            w.process_host(raw[:, :K + 1])
        assert e.value.code == fmx_amd.fmx.FMX_E_INVALID
    finally:
        w.close()
    got, ref, ref32 = (np.concatenate(v, axis=1) for v in (got, ref, ref32))
    head = slice(n_a, n_a + 4 + 16)                                  # every output whose window holds samples of more than one offset
    behind = slice(n_a + 4 + 16, N_OUT)
    print()
    check_bound("K = %d, before the change" % K, got[:, :n_a], ref[:, :n_a], ref32[:, :n_a])
    check_bound("K = %d, across the changes" % K, got[:, head], ref[:, head], ref32[:, head])
    check_bound("K = %d, behind the changes" % K, got[:, behind], ref[:, behind], ref32[:, behind])


# ---- chained into a handle ------------------------------------------------------------------------------------------------------
CH_K = 4
CH_BLOCK = 49152                      # narrow samples per call
CH_CALLS = 4
CH_OFFS = [-1200000, 300000, 2100000]
CH_TONES = [700.0, 1300.0, 1900.0]


@pytest.fixture(scope="module")
def chained_signal():
    """One K = 4 stream (9.216 MS/s) that holds three mono FM stations, 50 kHz deviation, a tone each."""
    Rw = CH_K * wm.NARROW_RATE
    n = CH_CALLS * CH_BLOCK * CH_K
    t = np.arange(n, dtype=np.float64)
    x = np.zeros(n, np.complex128)
    for f, tone in zip(CH_OFFS, CH_TONES):
        x += 0.25 * np.exp(1j * (2 * np.pi * ((f * np.arange(n, dtype=np.int64)) % Rw) / Rw + (50000.0 / tone) * np.sin(2 * np.pi * tone * t / Rw)))
    return np.stack([x.real, x.imag], axis=-1).astype(np.float32)[None]


def _handle(fmx_amd):
    M = fmx_amd.fmx
    f = fmx_amd.Fmx(3, max_block=CH_BLOCK)
    for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 2)):
        f.set_param(pid, v)
    return f


def test_chained_into_a_handle(fmx_amd, ol, chained_signal):
    import torch
    wide = chained_signal
    nw = CH_BLOCK * CH_K
    # (a) on the device, no copy in between: Wideband -> Fmx on one stream ...
    dev = torch.device("cuda:0")
    d_wide = torch.from_numpy(wide).to(dev)
    d_narrow = torch.zeros((3, CH_BLOCK, 2), dtype=torch.float32, device=dev)
    cap = CH_BLOCK // 48 + 96
    d_pcm = torch.zeros((3, cap, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    w = fmx_amd.Wideband(CH_K, [0, 0, 0], CH_OFFS, streams=1, max_block=nw)
    f = _handle(fmx_amd)
    pcm_dev = []
    try:
        for k in range(CH_CALLS):
            got = w.process_device(d_wide.data_ptr() + 8 * k * nw, wide.shape[1], nw, d_narrow.data_ptr(), CH_BLOCK, hip_stream=stream.cuda_stream)
            assert got == CH_BLOCK
            frames = f.process_device(d_narrow.data_ptr(), CH_BLOCK, CH_BLOCK, d_pcm.data_ptr(), cap, hip_stream=stream.cuda_stream)
            stream.synchronize()
            pcm_dev.append(d_pcm[:, :frames].cpu().numpy())
    finally:
        w.close()
        f.close()
    pcm_dev = np.concatenate(pcm_dev, axis=1)
    # ... against the same handle fed the channeliser's output through fmx_process_host
    w = fmx_amd.Wideband(CH_K, [0, 0, 0], CH_OFFS, streams=1, max_block=nw)
    f = _handle(fmx_amd)
    pcm_host, narrow = [], []
    try:
        for k in range(CH_CALLS):
            y = w.process_host(wide[:, k * nw:(k + 1) * nw])
            narrow.append(y)
            pcm_host.append(f.process_host(y))
    finally:
        w.close()
        f.close()
    pcm_host = np.concatenate(pcm_host, axis=1)
    assert pcm_dev.shape == pcm_host.shape and pcm_dev.shape[1] > 3000
    assert np.array_equal(pcm_dev.view(np.uint32), pcm_host.view(np.uint32))
    # (b) within the project's 1e-5 RMS of the oracle run on the model's output rounded to f32
    ref = wm.WidebandModel(CH_K, CH_OFFS).process(wm.convert(wide[0], 0))
    print()
    for c in range(3):
        iq = np.stack([ref[c].real, ref[c].imag], axis=-1).astype(np.float32)
        po = ol.OracleChain(inputFilterBw=165000, fmMode=2).process(iq)
        assert po.shape == pcm_dev[c].shape, (po.shape, pcm_dev[c].shape)
        err = float(np.sqrt(np.mean((pcm_dev[c].astype(np.float64) - po) ** 2)))
        # (c) the strongest PCM tone is the station's own
        seg = pcm_dev[c][1024:, 0].astype(np.float64)
        spec = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
        spec[:4] = 0.0
        peak_hz = float(np.argmax(spec)) * 48000.0 / len(seg)
        print("[chained, station %d at %+d Hz] PCM RMS diff vs oracle on the model's output %.3e, level %.3f, strongest tone %.1f Hz (sent %.0f)"
              % (c, CH_OFFS[c], err, float(np.sqrt(np.mean(seg ** 2))), peak_hz, CH_TONES[c]))
        assert err <= 1e-5, (c, err)
        assert abs(peak_hz - CH_TONES[c]) <= 48000.0 / len(seg) * 1.5, (c, peak_hz)
        assert np.sqrt(np.mean(seg ** 2)) > 0.01


def test_create_destroy_cycles_give_their_memory_back(fmx_amd):
    """The method of tests/test_gpu_lifecycle.py: free device memory before and after ten create / process / destroy cycles differs by less
    than one object's footprint."""
    import torch

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    K = 5
    raw = wide_signal(K, N_OUT * K, 0)

    def one():
        before = free_bytes()
        w = fmx_amd.Wideband(K, SOF, offsets(K), streams=2, max_block=N_OUT * K)
        footprint = before - free_bytes()
        try:
            w.process_host(raw)                         # (the host call's staging buffers)
            w.set_offset(2, 12345)
            w.process_host(raw[:, :7 * K])
        finally:
            w.close()
        return footprint

    prints = [one() for _ in range(2)]
    start = free_bytes()
    prints += [one() for _ in range(10)]
    lost = start - free_bytes()
    footprint = min(prints)
    print("\n[wideband lifecycle] footprint at creation %.1f MB, free memory lost over 10 cycles: %.3f MB" % (footprint / 1e6, lost / 1e6))
    assert footprint > 0
    assert lost < footprint, (lost, footprint)

"""Stage W (wide-band ingest) without a GPU: the taps, their frequency response, the float64 model's independence of how a stream is cut,
and the argument checks the library makes before it looks for a device."""
import ctypes as C

import numpy as np
import pytest

import wideband_model as wm


@pytest.mark.parametrize("K", range(2, 17))
def test_library_taps_equal_the_models_bit_for_bit(fmx_amd, K):
    h = fmx_amd.fmx.wideband_taps(K)
    ref = wm.taps(K)
    assert h.dtype == np.float32 and h.shape == (16 * K + 1,)
    assert np.array_equal(h.view(np.uint32), ref.view(np.uint32))
    assert abs(float(np.sum(h.astype(np.float64))) - 1.0) < 1e-6


@pytest.mark.parametrize("K", range(2, 17))
def test_response_of_the_taps(fmx_amd, K):
    """Droop of at most 0.25 dB over +-150 kHz, at least 80 dB down at and above 1.152 MHz, where the images of the division by K begin
    (measured at design time: 0.22 dB and 83 dB)."""
    h = fmx_amd.fmx.wideband_taps(K)
    rate = K * wm.NARROW_RATE
    passband = wm.response_db(h, rate, np.linspace(0.0, 150000.0, 61))
    droop = float(passband.max() - passband.min())
    stop = wm.response_db(h, rate, np.arange(1152000.0, rate / 2 + 1.0, 2000.0))
    att = float(passband[0] - stop.max())
    print("\n[wideband taps, K = %d] droop over +-150 kHz %.3f dB, attenuation from 1.152 MHz %.1f dB" % (K, droop, att))
    assert droop <= 0.25
    assert att >= 80.0


@pytest.mark.parametrize("K", [2, 5, 16])
def test_model_does_not_depend_on_the_cuts(K):
    rng = np.random.default_rng(K)
    n = 700 * K
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    lim = wm.offset_limit(K)
    offs = [0, -412345, lim - 1, -lim]
    whole = wm.WidebandModel(K, offs).process(x)
    cut = wm.WidebandModel(K, offs)
    parts, pos = [], 0
    for ln in (K, 7 * K, 33 * K, 2 * K, n - 43 * K):
        parts.append(cut.process(x[pos:pos + ln]))
        pos += ln
    assert pos == n
    got = np.concatenate(parts, axis=1)
    # (float64 sums of the same products; the summation order inside numpy's convolution may differ with the length: a few ulp of f64)
    assert np.max(np.abs(got - whole)) <= 1e-13 * np.max(np.abs(whole))
    with pytest.raises(ValueError):
        cut.process(x[:K + 1])


def _create(L, M, K, streams, sof, offs, max_block):
    cfg = M.FmxWidebandConfig()
    cfg.struct_size = C.sizeof(M.FmxWidebandConfig)
    cfg.device, cfg.streams, cfg.factor, cfg.outputs, cfg.max_block = 0, streams, K, len(sof), max_block
    a = (C.c_int32 * len(sof))(*sof)
    b = (C.c_int32 * len(offs))(*offs)
    cfg.stream_of_output, cfg.offset_hz = C.cast(a, C.POINTER(C.c_int32)), C.cast(b, C.POINTER(C.c_int32))
    h = C.c_void_p()
    rc = L.fmx_wideband_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.fmx_wideband_destroy(h)
    return rc, L.fmx_last_error().decode()


def test_argument_checks_that_need_no_device(fmx_amd):
    """The configuration is checked before the device is looked for: on a host without a GPU these answer FMX_E_INVALID, not FMX_E_NO_DEVICE.
    (The length of a call can only be checked against an object, which needs a device: the rule `a multiple of K` is checked here on
    max_block, where fmx_wideband_create applies it, and on n_wide in tests/test_gpu_wideband.py.)"""
    M = fmx_amd.fmx
    L = fmx_amd.load_library()
    for K in (1, 17, 0, -3):
        rc, msg = _create(L, M, K, 1, [0], [0], 1024 * 16)
        assert rc == M.FMX_E_INVALID and "factor" in msg, (K, rc, msg)
        n = C.c_int32()
        assert L.fmx_wideband_taps(K, None, 0, C.byref(n)) == M.FMX_E_INVALID
    for K in (2, 5, 16):
        lim = wm.offset_limit(K)
        for f in (lim + 1, -lim - 1):
            rc, msg = _create(L, M, K, 1, [0, 0], [0, f], 1024 * K)
            assert rc == M.FMX_E_INVALID and "offset" in msg, (K, f, rc, msg)
        rc, msg = _create(L, M, K, 1, [0], [lim], 1024 * K + 1)                 # not a multiple of K
        assert rc == M.FMX_E_INVALID and "multiple" in msg, (K, rc, msg)
        rc, msg = _create(L, M, K, 1, [0], [-lim], 1024 * K)                    # everything in range: only the device can be missing
        assert rc in (M.FMX_OK, M.FMX_E_NO_DEVICE), (rc, msg)
    rc, msg = _create(L, M, 4, 2, [0, 2], [0, 0], 4096)
    assert rc == M.FMX_E_INVALID and "stream_of_output" in msg
    assert L.fmx_wideband_set_offset(None, 0, 0) == M.FMX_E_INVALID
    assert L.fmx_wideband_destroy(None) == 0
    got = C.c_int64()
    assert L.fmx_wideband_process_host_raw(None, None, 0, 0.0, 0, 0, None, 0, C.byref(got)) == M.FMX_E_INVALID
    h = np.zeros(10, np.float32)
    n = C.c_int32()
    assert L.fmx_wideband_taps(2, h.ctypes.data_as(C.POINTER(C.c_float)), 10, C.byref(n)) == M.FMX_E_TOO_LARGE and n.value == 33

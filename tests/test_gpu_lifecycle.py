"""A handle gives back the device memory of every subsystem it allocated lazily (fmx_host.h: DevMem; fmx_api.hip: fmx_destroy)."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCH, NST, BLOCK = 72, 2, 16384 * 3
WARMUP, CYCLES = 2, 16


def _one_handle(fmx_amd, ol, iq, free_bytes):
    """Create a batch handle above the block machines' 64 channels, switch everything on that allocates when first used, run it through a
    mid-stream promotion, destroy it.  Returns the handle's footprint at creation."""
    M = fmx_amd.fmx
    L = fmx_amd.load_library()
    L.fmx_debug_phase_cycles.restype = C.c_int
    L.fmx_debug_phase_cycles.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_ulonglong)]
    before = free_bytes()
    f = fmx_amd.Fmx(NCH, streams=NST, stream_of_channel=[c % NST for c in range(NCH)], max_block=BLOCK)
    footprint = before - free_bytes()
    try:
        for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0)):
            f.set_param(pid, v)
        f.set_param(M.P_RDS_MODE, 2, 0)                      # the RDS path's buffers
        f.set_param(M.P_SCANNING, 1, 1)                      # scan mode's
        f.set_param(M.P_SQUELCH_MODE, 1, 2)                  # the noise squelch: its coefficients, the pre-pass arrays, the side streams
        f.set_param(M.P_LOCAL_OSCILLATOR, 2500, 3)           # the oscillator table
        f.set_param(M.P_SCOPE_TAPS, 1)                       # the LR scope tap's rows
        assert L.fmx_debug_phase_cycles(f.h, 1, None) == 0   # the diagnostic counters: enabled and LEFT enabled
        calls = 0
        pcm = f.process_host(iq[:, :BLOCK])                  # (process_host: the staging buffers, device and pinned)
        calls += 1
        assert pcm.shape[0] == NCH
        assert len(f.tap(M.TAP_LR_RAW, 64, 4)) == 64
        for c in range(1, NCH, 2):                           # a mid-stream width change: the handle keeps its streams, then is promoted
            f.set_param(M.P_BANDWIDTH, 130000, c)
        assert f.filter_change_due() > 0
        while f.filter_change_due() > 0:
            assert calls < 10, "the filter change never fell due"
            f.process_host(iq[:, calls * BLOCK:(calls + 1) * BLOCK])
            calls += 1
        f.process_host(iq[:, calls * BLOCK:(calls + 1) * BLOCK])      # (this call's head promotes the handle: the block machines' buffers)
        assert f.filter_change_due() == -1 and f.last_front_kernel() == 1
        assert len(f.scan_results(1)) > 0
    finally:
        f.close()
    return footprint


def test_create_destroy_cycles_give_their_memory_back(fmx_amd, ol):
    """Handles that exercise every lazily allocated subsystem must give their memory back: in one process, WARMUP + CYCLES times, a 72-channel
    handle is created, gets RDS, scan mode, the noise squelch, a local oscillator, the LR scope tap and fmx_debug_phase_cycles (left enabled)
    switched on, is fed through fmx_process_host, has its input filter changed in mid-stream (the promotion's buffers) and is destroyed.  Free
    device memory behind the warm-up cycles and behind CYCLES more may differ by less than ONE handle's footprint (free before fmx_create
    minus free behind it; the smallest seen): a buffer leaked per cycle accumulates linearly, the runtime's own caching does not.

    Leaks much smaller than a handle -- such as the 768 bytes per channel of DeviceBuffers::dbg, which fmx_destroy did not free before
    the handle had one owner for its memory -- are below what this can see; that every allocation goes through that owner is what covers
    those."""
    import torch

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    iq = np.stack([ol.synth_iq(10 * BLOCK, leftHz=400.0 + 300 * k, rightHz=700.0 + 200 * k) for k in range(NST)])
    prints = [_one_handle(fmx_amd, ol, iq, free_bytes) for _ in range(WARMUP)]
    start = free_bytes()
    prints += [_one_handle(fmx_amd, ol, iq, free_bytes) for _ in range(CYCLES)]
    lost = start - free_bytes()
    footprint = min(prints)
    print("\n[lifecycle, %d channels] footprint at creation %.1f MB (smallest of %d), free memory lost over %d cycles: %.3f MB"
          % (NCH, footprint / 1e6, len(prints), CYCLES, lost / 1e6))
    assert footprint > 0
    assert lost < footprint, (lost, footprint)

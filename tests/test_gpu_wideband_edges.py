"""Stage W (fmx_wide.hip, fmx_wideband_* in fmx_wide_api.hip) sample by sample on the GPU: every factor, the edges of tiles, groups and the run
list, strides, positions beyond 2^31 and 2^32 samples, the raw formats' extreme codes, and the C++ wrapper.

Every comparison goes through wideband_model.check_per_sample against the float64 model: each sample of each output within 2 x the worst
sample of the model's f32 restatement, relative to the output's peak.  The signal is the recipe of test_gpu_wideband.wide_signal: a carrier
with a slow phase wobble at every output's offset, and noise.  tests/test_wideband_edges_cpu.py shows on these shapes that the check
catches what it is for."""
import os
import subprocess
import time

import numpy as np
import pytest

import wideband_model as wm

pytestmark = pytest.mark.gpu

FMT_NAMES = {0: "F32", 1: "U8", 2: "S8", 3: "S16"}
A_SOF = [0, 0, 0, 0, 0, 1, 2, 2, 2, 2]           # case a: a full group and a short one, one output, one full group, a stream with none
A_STREAMS = 4
A_CALLS = [549, 257, 5, 16]                      # outputs: two tiles and a ragged one; a tile of one column; n_tile < 16 twice


def a_offsets(K):
    lim = wm.offset_limit(K)
    return [0, -412345, lim - 1, -lim, 733001, 100000, lim, -1, -(lim // 2), 1]


def edge_signal(K, n, sof, offs, streams, fmt=0, seed=0, amp=0.2):
    """[streams, n, 2] in the raw format: per stream a carrier with a slow phase wobble at each of its outputs' offsets, and noise."""
    rng = np.random.default_rng(7000 * K + seed)
    Rw = K * wm.NARROW_RATE
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((streams, n), np.complex128)
    for m, f in enumerate(offs):
        x[sof[m]] += amp * np.exp(1j * (2 * np.pi * ((int(f) * np.arange(n, dtype=np.int64)) % Rw) / Rw
                                        + 3.0 * np.sin(2 * np.pi * (900.0 + 400 * (m % 7)) * t / Rw) + m))
    x += 0.02 * (rng.standard_normal((streams, n)) + 1j * rng.standard_normal((streams, n)))
    v = np.stack([x.real, x.imag], axis=-1)
    if fmt == 0:
        return v.astype(np.float32)
    if fmt == 1:
        return np.clip(np.rint(v * 128.0 + 127.0), 0, 255).astype(np.uint8)
    if fmt == 2:
        return np.clip(np.rint(v * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint(v * 2048.0), -32768, 32767).astype(np.int16)


class Models:
    """One float64 model per stream that has outputs; rows come back in the library's order of outputs."""

    def __init__(self, K, sof, offs, streams):
        self.sof = list(sof)
        self.members = [[m for m in range(len(sof)) if sof[m] == s] for s in range(streams)]
        self.mods = [wm.WidebandModel(K, [offs[m] for m in mem]) if mem else None for mem in self.members]

    def set_offset(self, m, hz):
        s = self.sof[m]
        self.mods[s].set_offset(self.members[s].index(m), hz)

    def advance(self, n, tails):
        for s, mod in enumerate(self.mods):
            if mod is not None:
                mod.advance(n, tails[s])

    def process(self, raw, fmt=0, den=2048.0):
        """raw [streams, n, 2] -> (f64 model, f32 restatement), each [outputs, n / K]"""
        nj = raw.shape[1] // self.mods[self.sof[0]].K
        ref, ref32 = np.zeros((len(self.sof), nj), np.complex128), np.zeros((len(self.sof), nj), np.complex64)
        for s, mod in enumerate(self.mods):
            if mod is not None:
                a, b = mod.process(wm.convert(raw[s], fmt, den), with_f32=True)
                ref[self.members[s]], ref32[self.members[s]] = a, b
        return ref, ref32


def cplx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def device_call(torch, w, raw, K, outputs, stream, pad_wide=0, pad_narrow=0):
    """One fmx_wideband_process_device call on torch buffers with wide_stride = n_wide + pad_wide and narrow_stride = n_out + pad_narrow.
    Both paddings are NaN before the call; the output rows must come back finite in front of n_out and still NaN behind it."""
    dev = torch.device("cuda:0")
    streams, n = raw.shape[0], raw.shape[1]
    host = np.full((streams, n + pad_wide, 2), np.nan, np.float32)
    host[:, :n] = raw
    d_wide = torch.from_numpy(host).to(dev)
    d_out = torch.full((outputs, n // K + pad_narrow, 2), float("nan"), dtype=torch.float32, device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    got = w.process_device(d_wide.data_ptr(), n + pad_wide, n, d_out.data_ptr(), n // K + pad_narrow, hip_stream=stream.cuda_stream)
    stream.synchronize()
    assert got == n // K
    out = d_out.cpu().numpy()
    assert np.all(np.isfinite(out[:, :n // K])), "a sample in front of n_out was not written"
    assert np.all(np.isnan(out[:, n // K:])), "the kernel wrote behind a row's n_out"
    return out[:, :n // K].copy()


# ---- a. every factor: groups, tiles, strides ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", range(2, 17))
def test_every_factor(fmx_amd, K):
    """Four streams with 5, 1, 4 and no outputs, calls of 549, 257, 5 and 16 outputs through process_device with wide_stride = n_wide + 3 K and
    narrow_stride = n_out + 7 on NaN-filled buffers; the same samples through process_host in one call are bit-identical."""
    import torch
    offs, total = a_offsets(K), sum(A_CALLS)
    raw = edge_signal(K, total * K, A_SOF, offs, A_STREAMS)
    mods = Models(K, A_SOF, offs, A_STREAMS)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    w = fmx_amd.Wideband(K, A_SOF, offs, streams=A_STREAMS, max_block=total * K)
    whole = fmx_amd.Wideband(K, A_SOF, offs, streams=A_STREAMS, max_block=total * K)
    got, ref, ref32, pos = [], [], [], 0
    try:
        for nj in A_CALLS:
            seg = raw[:, pos * K:(pos + nj) * K]
            got.append(device_call(torch, w, seg, K, len(A_SOF), stream, pad_wide=3 * K, pad_narrow=7))
            a, b = mods.process(seg)
            ref.append(a)
            ref32.append(b)
            pos += nj
        one = whole.process_host(raw)
    finally:
        w.close()
        whole.close()
    got = np.concatenate(got, axis=1)
    assert np.array_equal(got.view(np.uint32), one.view(np.uint32))
    print()
    ratio = wm.check_per_sample("a, K = %d" % K, cplx(got), np.concatenate(ref, axis=1), np.concatenate(ref32, axis=1), calls=A_CALLS)
    print("[a, K = %d] worst sample: %.2f of the f32 restatement's level" % (K, ratio))


# ---- b. more than 256 outputs on a stream ---------------------------------------------------------------------------------------------
B_OUTPUTS = 261                                  # 256, then a full group, then a short one
B_CALLS = [293, 40]
B_CHANGED = [3, 255, 256, 260]                   # 256 and 260: slow-path outputs in the second pass of the loop over a stream's outputs


def b_offsets(K):
    lim = wm.offset_limit(K)
    v = np.random.default_rng(40 + K).integers(-lim, lim + 1, size=B_OUTPUTS + len(B_CHANGED))
    v[1], v[258] = lim, -lim
    return [int(f) for f in v[:B_OUTPUTS]], [int(f) for f in v[B_OUTPUTS:]]


@pytest.mark.parametrize("K", [2, 16])
def test_more_outputs_than_threads(fmx_amd, K):
    """One stream with 261 outputs, calls of 293 and 40 outputs, offset changes on outputs 3, 255, 256 and 260 in front of the second.

    Measured on the MI355X against the plain restatement alone: every output within 2 x but one, output 158 at K = 2 (sample 189: 2.39 x) and
    output 199 at K = 16 (sample 44: 2.69 x), both fast-path samples of the first call.  kernel_form on the CPU is 2.34 x and 2.58 x on the
    same two outputs and within 2 x on the other 260: the folded form's own rounding against a restatement whose worst of 333 samples came
    out low (its level spreads 1.15 - 3.05e-7 over the outputs at K = 2), not the kernel.  So here `level` is the larger of the two CPU
    restatements' worst samples, kernel_form's over the samples in front of an output's offset change; the factor 2 stays."""
    offs, new = b_offsets(K)
    sof = [0] * B_OUTPUTS
    raw = edge_signal(K, sum(B_CALLS) * K, sof, offs, 1, amp=0.02)
    mods = Models(K, sof, offs, 1)
    w = fmx_amd.Wideband(K, sof, offs, streams=1, max_block=sum(B_CALLS) * K)
    got, ref, ref32, pos = [], [], [], 0
    try:
        for k, nj in enumerate(B_CALLS):
            if k == 1:
                for m, f in zip(B_CHANGED, new):
                    w.set_offset(m, f)
                    mods.set_offset(m, f)
            seg = raw[:, pos * K:(pos + nj) * K]
            got.append(cplx(w.process_host(seg)))
            a, b = mods.process(seg)
            ref.append(a)
            ref32.append(b)
            pos += nj
    finally:
        w.close()
    x = wm.convert(raw[0], 0)
    form = np.full((B_OUTPUTS, sum(B_CALLS)), np.nan, np.complex128)
    for m, f in enumerate(offs):
        n = B_CALLS[0] if m in B_CHANGED else sum(B_CALLS)
        form[m, :n] = wm.kernel_form(K, f, x[:n * K], wm.taps(K))
    print()
    wm.check_per_sample("b, K = %d" % K, np.concatenate(got, axis=1), np.concatenate(ref, axis=1), np.concatenate(ref32, axis=1), calls=B_CALLS,
                        form=form)


# ---- c. seventeen runs ----------------------------------------------------------------------------------------------------------------
def c_plan(K):
    """The calls of case c and the set_offset calls in front of each: [(outputs of the call, [(output, hz), ...])].  A change on output 0 in
    front of the first call (nothing was mixed with the offset it replaces) and of each of 20 calls of K samples, on output 1 in front of
    every third; in front of call 7 output 1 is set twice (the last value wins), in front of call 18 output 0 is set to the value in
    force (nothing happens): calls 0 ... 17 are an unbroken chain of changes.  Then one call of 40 outputs."""
    lim = wm.offset_limit(K)
    rng = np.random.default_rng(300 + K)
    draw = lambda: int(rng.integers(-lim, lim + 1))
    plan, cur0 = [], None
    for k in range(20):
        sets = [(0, cur0 if k == 18 else draw())]
        cur0 = sets[0][1]
        if k % 3 == 0:
            sets.append((1, draw()))
        if k == 7:
            sets += [(1, draw()), (1, draw())]
        plan.append((1, sets))
    plan.append((40, []))
    return plan


C_START = [250000, -90001, 412345]


@pytest.mark.parametrize("K", [2, 7, 16])
def test_seventeen_runs(fmx_amd, K):
    """Twenty calls of K samples with a new offset in front of each: the windows behind them hold 17 runs, the run list is full, trimmed and
    shifted.  Every sample of every call against the model with the same switches; output 2, which never changes, is also bit-identical
    to a fresh object that never saw a change."""
    plan = c_plan(K)
    calls = [nj for nj, _ in plan]
    sof = [0, 0, 0]
    raw = edge_signal(K, sum(calls) * K, sof, C_START, 1)
    mods = Models(K, sof, C_START, 1)
    w = fmx_amd.Wideband(K, sof, C_START, streams=1, max_block=40 * K)
    fresh = fmx_amd.Wideband(K, [0], C_START[2:], streams=1, max_block=40 * K)
    got, alone, ref, ref32, pos = [], [], [], [], 0
    try:
        for nj, sets in plan:
            for m, f in sets:
                w.set_offset(m, f)
                mods.set_offset(m, f)
            seg = raw[:, pos * K:(pos + nj) * K]
            got.append(w.process_host(seg))
            alone.append(fresh.process_host(seg))
            a, b = mods.process(seg)
            ref.append(a)
            ref32.append(b)
            pos += nj
    finally:
        w.close()
        fresh.close()
    got, alone = np.concatenate(got, axis=1), np.concatenate(alone, axis=1)
    assert np.array_equal(got[2].view(np.uint32), alone[0].view(np.uint32))
    print()
    wm.check_per_sample("c, K = %d" % K, cplx(got), np.concatenate(ref, axis=1), np.concatenate(ref32, axis=1), calls=calls)


# ---- d. one second of outputs ---------------------------------------------------------------------------------------------------------
D_K = 2
D_EDGE = 600                                     # outputs of the first and of the last call
D_BULK, D_BULK_CALLS = 76770, 30                 # 30 x 76 770 = 2 304 000 - 300 - 600 outputs from one reused buffer


def test_one_second_of_outputs(fmx_amd):
    """K = 2: 600 outputs, an offset change on output 1, whole calls from a reused device buffer until 2 304 000 - 300 outputs have passed, then
    600 outputs across the 1 s mark, where the count of outputs since a run began wraps (output 0) and does not (output 1)."""
    import torch
    K, sof, offs = D_K, [0, 0], [733001, -412345]
    assert D_EDGE + D_BULK * D_BULK_CALLS == wm.NARROW_RATE - 300
    raw = edge_signal(K, (2 * D_EDGE + D_BULK) * K, [0, 0, 0], offs + [1900001], 1)
    first, bulk, last = raw[:, :D_EDGE * K], raw[:, D_EDGE * K:(D_EDGE + D_BULK) * K], raw[:, (D_EDGE + D_BULK) * K:]
    mods = Models(K, sof, offs, 1)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    w = fmx_amd.Wideband(K, sof, offs, streams=1, max_block=D_BULK * K)
    try:
        got = [device_call(torch, w, first, K, 2, stream)]
        ref, ref32 = mods.process(first)
        w.set_offset(1, 1900001)
        mods.set_offset(1, 1900001)
        d_bulk = torch.from_numpy(bulk).to(dev)
        d_out = torch.zeros((2, D_BULK, 2), dtype=torch.float32, device=dev)
        stream.wait_stream(torch.cuda.current_stream())
        for _ in range(D_BULK_CALLS):
            w.process_device(d_bulk.data_ptr(), D_BULK * K, D_BULK * K, d_out.data_ptr(), D_BULK, hip_stream=stream.cuda_stream)
        stream.synchronize()
        mods.advance(D_BULK * D_BULK_CALLS * K, [wm.convert(bulk[0], 0)[-16 * K:]])
        got.append(device_call(torch, w, last, K, 2, stream))
        a, b = mods.process(last)
    finally:
        w.close()
    print()
    wm.check_per_sample("d, first and last call", cplx(np.concatenate(got, axis=1)), np.concatenate([ref, a], axis=1),
                        np.concatenate([ref32, b], axis=1), calls=[D_EDGE, D_EDGE])


# ---- e. beyond 2^31 and 2^32 samples --------------------------------------------------------------------------------------------------
E_K = 16
E_BUF = 1 << 24                                  # samples of the reused device buffer (U8: 32 MB)
E_EDGE = 600                                     # outputs of a compared call


def test_beyond_2_to_the_31_and_32_samples(fmx_amd):
    """K = 16, one stream, two outputs, U8: the first call, the call across sample 2^31, the call across sample 2^32 with an offset change on
    output 0 in front of it, and the call behind it with a change on output 1 in front (a run that begins beyond 2^32); 600 outputs each,
    the boundary in the middle of its call.  In between one device buffer of 2^24 samples is fed again and again (256 launches, 2^28
    outputs per station) while the model skips with `advance`.  Prints the time the launches in between took."""
    import torch
    K, sof, offs = E_K, [0, 0], [-412345, wm.offset_limit(E_K)]
    n_edge = E_EDGE * K
    part = edge_signal(K, 1 << 20, [0, 0, 0, 0], offs + [733001, -5000000], 1, fmt=1)
    buf = np.ascontiguousarray(np.tile(part, (1, E_BUF >> 20, 1)))
    mods = Models(K, sof, offs, 1)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    d_buf = torch.from_numpy(buf).to(dev)
    d_out = torch.zeros((2, E_BUF // K, 2), dtype=torch.float32, device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    w = fmx_amd.Wideband(K, sof, offs, streams=1, max_block=E_BUF)
    state = {"pos": 0, "seconds": 0.0}
    got, ref, ref32 = [], [], []

    def compared(at):
        """600 outputs from sample `at` of the buffer"""
        w.process_device(d_buf.data_ptr() + 2 * at, E_BUF, n_edge, d_out.data_ptr(), E_BUF // K, fmt=1, hip_stream=stream.cuda_stream)
        stream.synchronize()
        got.append(d_out[:, :E_EDGE].cpu().numpy())
        a, b = mods.process(buf[:, at:at + n_edge], fmt=1)
        ref.append(a)
        ref32.append(b)
        state["pos"] += n_edge

    def skip_to(target):
        """whole buffers, then a part of one, until `target` samples have passed"""
        n = target - state["pos"]
        assert n > 0 and n % K == 0
        last, t0 = E_BUF, time.perf_counter()
        for _ in range(n // E_BUF):
            w.process_device(d_buf.data_ptr(), E_BUF, E_BUF, d_out.data_ptr(), E_BUF // K, fmt=1, hip_stream=stream.cuda_stream)
        if n % E_BUF:
            last = n % E_BUF
            w.process_device(d_buf.data_ptr(), E_BUF, last, d_out.data_ptr(), E_BUF // K, fmt=1, hip_stream=stream.cuda_stream)
        stream.synchronize()
        state["seconds"] += time.perf_counter() - t0
        mods.advance(n, [wm.convert(buf[0, last - 16 * K:last], 1)])
        state["pos"] = target

    try:
        compared(0)
        skip_to((1 << 31) - n_edge // 2)
        compared(16000)
        skip_to((1 << 32) - n_edge // 2)
        w.set_offset(0, 733001)
        mods.set_offset(0, 733001)
        compared(32000)
        assert state["pos"] > 1 << 32
        w.set_offset(1, -5000000)
        mods.set_offset(1, -5000000)
        compared(48000)
    finally:
        w.close()
    print("\n[e] %d samples per stream; the 256 launches between the compared calls took %.2f s" % (state["pos"], state["seconds"]))
    wm.check_per_sample("e, first call / across 2^31 / across 2^32 / behind it", cplx(np.concatenate(got, axis=1)), np.concatenate(ref, axis=1),
                        np.concatenate(ref32, axis=1), calls=[E_EDGE] * 4)


# ---- f. the raw formats' extreme codes ------------------------------------------------------------------------------------------------
def extreme_codes(fmt, n, seed):
    """[1, n, 2] uniform over every code of the format, the extreme codes among them"""
    rng = np.random.default_rng(seed)
    lo, hi, dt = {1: (0, 255, np.uint8), 2: (-128, 127, np.int8), 3: (-32768, 32767, np.int16)}[fmt]
    v = rng.integers(lo, hi + 1, size=(1, n, 2)).astype(dt)
    v[0, 5, 0], v[0, 6, 1], v[0, n // 2, 1], v[0, n - 1, 0] = lo, hi, lo, hi
    assert v.min() == lo and v.max() == hi
    return v


@pytest.mark.parametrize("fmt,den", [(1, 2048.0), (2, 2048.0), (3, 1.0), (3, 2048.0), (3, 32768.0)])
def test_extreme_raw_codes(fmx_amd, fmt, den):
    """K = 5, 300 outputs at offsets 0 and lim of samples uniform over every code: U8 0 and 255, S8 -128, S16 -32768, denominators 1 and 32768."""
    K, n_out = 5, 300
    offs = [0, wm.offset_limit(K)]
    raw = extreme_codes(fmt, n_out * K, 10 * fmt + int(den) % 7)
    w = fmx_amd.Wideband(K, [0, 0], offs, streams=1, max_block=n_out * K)
    try:
        got = cplx(w.process_host(raw, fmt, den))
    finally:
        w.close()
    ref, ref32 = Models(K, [0, 0], offs, 1).process(raw, fmt, den)
    print()
    wm.check_per_sample("f, %s / %g" % (FMT_NAMES[fmt], den if fmt == 3 else 128.0), got, ref, ref32)


# ---- the C++ wrapper ------------------------------------------------------------------------------------------------------------------
def build_demo(fmx_amd, exe):
    here = os.path.dirname(os.path.abspath(__file__))
    host = os.path.join(os.path.dirname(fmx_amd.__file__), "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + host, os.path.join(here, "wideband_demo", "wideband_adapter_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])


def test_cpp_adapter(fmx_amd, tmp_path):
    """host/wideband_adapter.h: processHost in two calls with setOffset between them writes what fmx_amd.Wideband computes, bit for bit."""
    K, n_out, n_first = 5, 300, 77
    offs = [0, -412345, wm.offset_limit(K)]
    raw = edge_signal(K, n_out * K, [0, 0, 0], offs, 1)
    exe, fin, fout = str(tmp_path / "wideband_adapter_demo"), str(tmp_path / "wide.f32"), str(tmp_path / "narrow.f32")
    build_demo(fmx_amd, exe)
    raw[0].tofile(fin)
    out = subprocess.run([exe, fin, fout, str(K), str(n_first * K), "1", "733001"] + [str(f) for f in offs], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0, out.stdout.decode()
    assert "taps5 81" in out.stdout.decode() and "ok 1" in out.stdout.decode(), out.stdout.decode()
    w = fmx_amd.Wideband(K, [0, 0, 0], offs, streams=1, max_block=n_out * K)
    try:
        a = w.process_host(raw[:, :n_first * K])
        w.set_offset(1, 733001)
        b = w.process_host(raw[:, n_first * K:])
    finally:
        w.close()
    want = np.concatenate([a, b], axis=1)
    got = np.fromfile(fout, np.float32).reshape(3, n_out, 2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

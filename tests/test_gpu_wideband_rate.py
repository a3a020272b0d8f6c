"""Stage W at any receiver rate (fmx_wide_rate.hip, fmx_wideband_create_rate in fmx_wide_api.hip) sample by sample on the GPU:
every listed rate, the edges of tiles, groups and the run list, strides, positions beyond 2^31 and 2^32 samples, the raw formats' extreme
codes, the refusals that need an object, the chain behind a rate object, its band survey and the C++ wrapper.

Every comparison of stage W's outputs goes through wideband_model.check_per_sample against the float64 model of tests/wideband_rate_model.py:
each sample of each output within 2 x the worst sample of the model's f32 restatement, relative to the output's peak.  No sample is skipped
and no output is exempt.  tests/test_wideband_rate_cpu.py shows on these shapes that the check catches what it is for."""
import os
import subprocess
import time

import numpy as np
import pytest

import wideband_model as wm
import wideband_rate_model as rm

pytestmark = pytest.mark.gpu

A_SOF = [0, 0, 0, 0, 0, 1, 2, 2, 2, 2]           # case a: a full group and a short one, one output, one full group, a stream with none
A_STREAMS = 4
A_TARGETS = [549, 257, 256, 255, 5, 1]           # outputs of the calls: two tiles and a ragged one, a tile of one column, a full tile, ...


def a_offsets(rate):
    lim = rm.Ratio(rate).lim
    return rm.offsets(rate) + [max(-lim, min(lim, f)) for f in [100000, lim, -1, -(lim // 2), 1]]


def plan_calls(r, targets, g0=0):
    """Call lengths in samples from sample g0 on that produce `targets` outputs, in this order; where no call of at least ceil (M / L) samples
    produces a (small) target at the place the stream has reached, a filler call moves it on.  Then one call of exactly ceil (M / L).
    -> (the calls' lengths, the places of the target calls among them)"""
    calls, places, g = [], [], g0
    for t in targets:
        for fill in [0] + list(range(r.min_call, r.min_call + 2 * r.M)):
            j = r.before(g + fill) + t
            n = -(-j * r.M // r.L) - (g + fill)                          # the first sample count that completes t outputs
            if n >= r.min_call and r.count(g + fill, n) == t and (fill == 0 or r.count(g, fill) >= 1):
                break
        else:
            raise AssertionError("no call produces %d outputs" % t)
        if fill:
            calls.append(fill)
        places.append(len(calls))
        calls.append(n)
        g += fill + n
    return calls + [r.min_call], places


class Models:
    """One float64 model per stream that has outputs; rows come back in the library's order of outputs."""

    def __init__(self, rate, sof, offs, streams):
        self.sof = list(sof)
        self.members = [[m for m in range(len(sof)) if sof[m] == s] for s in range(streams)]
        self.mods = [rm.WidebandRateModel(rate, [offs[m] for m in mem]) if mem else None for mem in self.members]

    def set_offset(self, m, hz):
        s = self.sof[m]
        self.mods[s].set_offset(self.members[s].index(m), hz)

    def advance(self, n, tails):
        for s, mod in enumerate(self.mods):
            if mod is not None:
                mod.advance(n, tails[s])

    def process(self, raw, fmt=0, den=2048.0):
        """raw [streams, n, 2] -> (f64 model, f32 restatement), each [outputs, the call's count]"""
        nj = self.mods[self.sof[0]].outputs_for(raw.shape[1])
        ref, ref32 = np.zeros((len(self.sof), nj), np.complex128), np.zeros((len(self.sof), nj), np.complex64)
        for s, mod in enumerate(self.mods):
            if mod is not None:
                a, b = mod.process(wm.convert(raw[s], fmt, den), with_f32=True)
                ref[self.members[s]], ref32[self.members[s]] = a, b
        return ref, ref32


def cplx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def device_call(torch, w, raw, outputs, stream, pad_wide=0, pad_narrow=0):
    """One fmx_wideband_process_device call on torch buffers with wide_stride = n_wide + pad_wide and narrow_stride = count + pad_narrow.
    Both paddings are NaN before the call; the output rows must come back finite in front of the count and still NaN behind it, and the
    count the call reports is the one outputs_for announced."""
    dev = torch.device("cuda:0")
    streams, n = raw.shape[0], raw.shape[1]
    host = np.full((streams, n + pad_wide, 2), np.nan, np.float32)
    host[:, :n] = raw
    d_wide = torch.from_numpy(host).to(dev)
    cnt = w.outputs_for(n)
    d_out = torch.full((outputs, cnt + pad_narrow, 2), float("nan"), dtype=torch.float32, device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    got = w.process_device(d_wide.data_ptr(), n + pad_wide, n, d_out.data_ptr(), cnt + pad_narrow, hip_stream=stream.cuda_stream)
    stream.synchronize()
    assert got == cnt
    out = d_out.cpu().numpy()
    assert np.all(np.isfinite(out[:, :cnt])), "a sample in front of the count was not written"
    assert np.all(np.isnan(out[:, cnt:])), "the kernel wrote behind a row's count"
    return out[:, :cnt].copy()


# ---- a. every listed rate: groups, tiles, strides ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", rm.RATES)
def test_every_rate(fmx_amd, rate):
    """Four streams with 5, 1, 4 and no outputs; calls producing 549, 257, 256, 255, 5 and 1 outputs and one of exactly ceil (M / L) samples
    through process_device with wide_stride = n_wide + 37 and narrow_stride = count + 7 on NaN-filled buffers; the same samples through
    process_host in one call are bit-identical."""
    import torch
    r = rm.Ratio(rate)
    offs, (calls, places) = a_offsets(rate), plan_calls(r, A_TARGETS)
    total = sum(calls)
    raw = rm.signal(rate, total, A_SOF, offs, A_STREAMS)
    mods = Models(rate, A_SOF, offs, A_STREAMS)
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    w = fmx_amd.Wideband(rate_hz=rate, stream_of_output=A_SOF, offset_hz=offs, streams=A_STREAMS, max_block=total)
    whole = fmx_amd.Wideband(rate_hz=rate, stream_of_output=A_SOF, offset_hz=offs, streams=A_STREAMS, max_block=total)
    got, ref, ref32, counts, pos = [], [], [], [], 0
    try:
        for n in calls:
            seg = raw[:, pos:pos + n]
            got.append(device_call(torch, w, seg, len(A_SOF), stream, pad_wide=37, pad_narrow=7))
            a, b = mods.process(seg)
            ref.append(a)
            ref32.append(b)
            counts.append(a.shape[1])
            pos += n
        assert whole.outputs_for(total) == sum(counts)
        one = whole.process_host(raw)
    finally:
        w.close()
        whole.close()
    assert [counts[k] for k in places] == A_TARGETS and calls[-1] == r.min_call
    got = np.concatenate(got, axis=1)
    assert np.array_equal(got.view(np.uint32), one.view(np.uint32))
    print()
    ratio = wm.check_per_sample("a, %d S/s" % rate, cplx(got), np.concatenate(ref, axis=1), np.concatenate(ref32, axis=1), calls=counts)
    print("[a, %d S/s] calls of %s samples: worst sample %.2f of the f32 restatement's level" % (rate, calls, ratio))


# ---- b. more than 256 outputs on a stream ---------------------------------------------------------------------------------------------
B_OUTPUTS = 261                                  # 256, then a full group, then a short one
B_TARGETS = [293, 40]
B_CHANGED = [3, 255, 256, 260]                   # 256 and 260: slow-path outputs in the second pass of the loop over a stream's outputs


def b_offsets(rate):
    lim = rm.Ratio(rate).lim
    v = np.random.default_rng(40 + rate // 1000).integers(-lim, lim + 1, size=B_OUTPUTS + len(B_CHANGED))
    v[1], v[258] = lim, -lim
    return [int(f) for f in v[:B_OUTPUTS]], [int(f) for f in v[B_OUTPUTS:]]


@pytest.mark.parametrize("rate", [2500000, 36000000])
def test_more_outputs_than_threads(fmx_amd, rate):
    """One stream with 261 outputs, calls of 293 and 40 outputs, offset changes on outputs 3, 255, 256 and 260 in front of the second.

    With 261 outputs of 333 samples each, kernel_form on the CPU is above twice the plain restatement's worst sample on single outputs: 2 at
    2.5 MS/s (worst 2.34 x, output 181) and 4 at 36 MS/s (worst 2.48 x, output 252), whose plain levels lie at the low end of a spread of
    0.9 - 2.3e-7 and 3.3 - 9.6e-7.  That is the form's rounding, so DESIGN 4.8 case b's rule holds here: `level` is the larger of the two CPU
    restatements' worst samples, kernel_form's over the samples in front of an output's offset change; the factor 2 stays.  Measured on the
    MI355X with it: worst ratio 1.79 (2.5 MS/s) and 1.37 (36 MS/s)."""
    r = rm.Ratio(rate)
    offs, new = b_offsets(rate)
    sof = [0] * B_OUTPUTS
    calls = plan_calls(r, B_TARGETS)[0][:2]
    raw = rm.signal(rate, sum(calls), sof, offs, 1, amp=0.02)
    mods = Models(rate, sof, offs, 1)
    w = fmx_amd.Wideband(rate_hz=rate, stream_of_output=sof, offset_hz=offs, streams=1, max_block=sum(calls))
    got, ref, ref32, pos = [], [], [], 0
    try:
        for k, n in enumerate(calls):
            if k == 1:
                for m, f in zip(B_CHANGED, new):
                    w.set_offset(m, f)
                    mods.set_offset(m, f)
            seg = raw[:, pos:pos + n]
            got.append(cplx(w.process_host(seg)))
            a, b = mods.process(seg)
            ref.append(a)
            ref32.append(b)
            pos += n
    finally:
        w.close()
    form = rm.kernel_form(rate, offs, wm.convert(raw[0], 0)).astype(np.complex128)
    assert form.shape == (B_OUTPUTS, sum(B_TARGETS))
    form[B_CHANGED, B_TARGETS[0]:] = np.nan
    print()
    wm.check_per_sample("b, %d S/s" % rate, np.concatenate(got, axis=1), np.concatenate(ref, axis=1), np.concatenate(ref32, axis=1),
                        calls=B_TARGETS, form=form)


# ---- c. seventeen runs ----------------------------------------------------------------------------------------------------------------
def c_plan(rate):
    """The set_offset calls in front of each of 20 calls of ceil (M / L) samples: a change on output 0 in front of every call (the first:
    nothing was mixed with the offset it replaces), on output 1 in front of every third; in front of call 7 output 1 is set twice (the last
    value wins), in front of call 18 output 0 is set to the value in force (nothing happens).  Then one call of 40 ceil (M / L) samples."""
    r = rm.Ratio(rate)
    rng = np.random.default_rng(300 + rate // 1000)
    draw = lambda: int(rng.integers(-r.lim, r.lim + 1))
    plan, cur0 = [], None
    for k in range(20):
        sets = [(0, cur0 if k == 18 else draw())]
        cur0 = sets[0][1]
        if k % 3 == 0:
            sets.append((1, draw()))
        if k == 7:
            sets += [(1, draw()), (1, draw())]
        plan.append((r.min_call, sets))
    plan.append((40 * r.min_call, []))
    return plan


@pytest.mark.parametrize("rate", [2400000, 10000000, 36000000])
def test_seventeen_runs(fmx_amd, rate):
    """Twenty minimal calls with a new offset in front of each: the windows behind them hold 17 runs, the run list is full, trimmed and
    shifted.  Every sample of every call against the model with the same switches; output 2, which never changes, is also bit-identical to
    a fresh object that never saw a change."""
    r = rm.Ratio(rate)
    plan = c_plan(rate)
    start = [250000, -90001, 412345]
    sof = [0, 0, 0]
    total = sum(n for n, _ in plan)
    raw = rm.signal(rate, total, sof, start, 1)
    mods = Models(rate, sof, start, 1)
    w = fmx_amd.Wideband(rate_hz=rate, stream_of_output=sof, offset_hz=start, streams=1, max_block=40 * r.min_call)
    fresh = fmx_amd.Wideband(rate_hz=rate, stream_of_output=[0], offset_hz=start[2:], streams=1, max_block=40 * r.min_call)
    got, alone, ref, ref32, counts, pos = [], [], [], [], [], 0
    try:
        for n, sets in plan:
            for m, f in sets:
                w.set_offset(m, f)
                mods.set_offset(m, f)
            seg = raw[:, pos:pos + n]
            got.append(w.process_host(seg))
            alone.append(fresh.process_host(seg))
            a, b = mods.process(seg)
            ref.append(a)
            ref32.append(b)
            counts.append(a.shape[1])
            pos += n
    finally:
        w.close()
        fresh.close()
    got, alone = np.concatenate(got, axis=1), np.concatenate(alone, axis=1)
    assert got.shape[1] == sum(counts) == r.before(total)
    assert np.array_equal(got[2].view(np.uint32), alone[0].view(np.uint32))
    print()
    wm.check_per_sample("c, %d S/s" % rate, cplx(got), np.concatenate(ref, axis=1), np.concatenate(ref32, axis=1), calls=counts)


# ---- d. beyond 2^31 and 2^32 samples --------------------------------------------------------------------------------------------------
D_RATE = 20000000
D_BUF = 1 << 24                                  # samples of the reused device buffer (U8: 32 MB)
D_EDGE = 5200                                    # samples of a compared call: 599 outputs


def test_beyond_2_to_the_31_and_32_samples(fmx_amd):
    """20 MS/s, one stream, two outputs, U8: the first call, the call across sample 2^31, the call across sample 2^32 with an offset change on
    output 0 in front of it, and the call behind it with a change on output 1 in front (a run that begins beyond 2^32); 5200 samples each,
    the boundary in the middle of its call.  In between one device buffer of 2^24 samples is fed again and again (256 launches) while the
    model skips with `advance`.  Prints the time the launches in between took."""
    import torch
    rate, r = D_RATE, rm.Ratio(D_RATE)
    sof, offs = [0, 0], [-412345, r.lim]
    part = rm.signal(rate, 1 << 20, [0, 0, 0, 0], offs + [733001, -5000000], 1, fmt=1)
    buf = np.ascontiguousarray(np.tile(part, (1, D_BUF >> 20, 1)))
    mods = Models(rate, sof, offs, 1)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    d_buf = torch.from_numpy(buf).to(dev)
    cap = r.before(D_BUF) + 1
    d_out = torch.zeros((2, cap, 2), dtype=torch.float32, device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    w = fmx_amd.Wideband(rate_hz=rate, stream_of_output=sof, offset_hz=offs, streams=1, max_block=D_BUF)
    state = {"pos": 0, "seconds": 0.0}
    got, ref, ref32, counts = [], [], [], []

    def compared(at):
        """D_EDGE samples from sample `at` of the buffer"""
        cnt = w.outputs_for(D_EDGE)
        assert w.process_device(d_buf.data_ptr() + 2 * at, D_BUF, D_EDGE, d_out.data_ptr(), cap, fmt=1, hip_stream=stream.cuda_stream) == cnt
        stream.synchronize()
        got.append(d_out[:, :cnt].cpu().numpy())
        a, b = mods.process(buf[:, at:at + D_EDGE], fmt=1)
        assert a.shape[1] == cnt
        ref.append(a)
        ref32.append(b)
        counts.append(cnt)
        state["pos"] += D_EDGE

    def skip_to(target):
        """whole buffers, then a part of one, until `target` samples have passed"""
        n = target - state["pos"]
        assert n > 0
        last, t0 = D_BUF, time.perf_counter()
        for _ in range(n // D_BUF):
            w.process_device(d_buf.data_ptr(), D_BUF, D_BUF, d_out.data_ptr(), cap, fmt=1, hip_stream=stream.cuda_stream)
        if n % D_BUF:
            last = n % D_BUF
            w.process_device(d_buf.data_ptr(), D_BUF, last, d_out.data_ptr(), cap, fmt=1, hip_stream=stream.cuda_stream)
        stream.synchronize()
        state["seconds"] += time.perf_counter() - t0
        mods.advance(n, [wm.convert(buf[0, last - (r.NP - 1):last], 1)])
        state["pos"] = target

    try:
        compared(0)
        skip_to((1 << 31) - D_EDGE // 2)
        compared(16000)
        skip_to((1 << 32) - D_EDGE // 2)
        w.set_offset(0, 733001)
        mods.set_offset(0, 733001)
        compared(32000)
        assert state["pos"] > 1 << 32
        w.set_offset(1, -5000000)
        mods.set_offset(1, -5000000)
        compared(48000)
    finally:
        w.close()
    print("\n[d] %d samples per stream; the launches between the compared calls took %.2f s" % (state["pos"], state["seconds"]))
    wm.check_per_sample("d, first call / across 2^31 / across 2^32 / behind it", cplx(np.concatenate(got, axis=1)), np.concatenate(ref, axis=1),
                        np.concatenate(ref32, axis=1), calls=counts)


# ---- e. the raw formats' extreme codes ------------------------------------------------------------------------------------------------
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
    """10 MS/s, 300 outputs at offsets 0 and lim of samples uniform over every code: U8 0 and 255, S8 -128, S16 -32768, denominators 1 and 32768."""
    rate = 10000000
    r = rm.Ratio(rate)
    n = -(-300 * r.M // r.L)
    offs = [0, r.lim]
    raw = extreme_codes(fmt, n, 10 * fmt + int(den) % 7)
    w = fmx_amd.Wideband(rate_hz=rate, stream_of_output=[0, 0], offset_hz=offs, streams=1, max_block=n)
    try:
        got = cplx(w.process_host(raw, fmt, den))
    finally:
        w.close()
    ref, ref32 = Models(rate, [0, 0], offs, 1).process(raw, fmt, den)
    assert got.shape[1] == 300
    print()
    wm.check_per_sample("e, %s / %g" % ({1: "U8", 2: "S8", 3: "S16"}[fmt], den if fmt == 3 else 128.0), got, ref, ref32)


# ---- f. the refusals that need an object ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [2500000, 36000000])
def test_refusals_of_a_call(fmx_amd, rate):
    """A call shorter than ceil (M / L), one longer than max_block, a narrow_stride one short; n_wide = 0 is a no-op, and none of the refused
    calls moved the stream: the next call gives what a fresh object gives."""
    import torch
    m = fmx_amd.fmx
    r = rm.Ratio(rate)
    n = 40 * r.min_call
    raw = rm.signal(rate, n, [0], [0], 1)
    dev = torch.device("cuda:0")
    d_wide = torch.from_numpy(raw).to(dev)
    cnt = r.before(n)
    d_out = torch.zeros((1, cnt, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    w = fmx_amd.Wideband(rate_hz=rate, max_block=n)
    fresh = fmx_amd.Wideband(rate_hz=rate, max_block=n)
    try:
        assert w.outputs_for(n) == cnt and w.outputs_for(0) == 0
        for n_wide, stride, code in ((r.min_call - 1, cnt, m.FMX_E_INVALID), (n + 1, cnt + 1, m.FMX_E_TOO_LARGE), (n, cnt - 1, m.FMX_E_INVALID)):
            with pytest.raises(m.FmxError) as e:
                w.process_device(d_wide.data_ptr(), n + 1, n_wide, d_out.data_ptr(), stride)
            assert e.value.code == code, str(e.value)
        assert w.process_device(d_wide.data_ptr(), n, 0, d_out.data_ptr(), 0) == 0
        assert w.process_device(d_wide.data_ptr(), n, n, d_out.data_ptr(), cnt) == cnt
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), fresh.process_host(raw).view(np.uint32))
    finally:
        w.close()
        fresh.close()


# ---- g. the chain behind a rate object ------------------------------------------------------------------------------------------------
G_RATE = 10000000
G_OFFS = [-1200000, 300000, 2100000]
G_TONES = [700.0, 1300.0, 1900.0]
G_CALLS = [212510, 212490, 212500, 107917, 107917]   # 85.3 ms: 48 962, 48 958, 48 960, ... outputs, 196 608 = 12 x 16 384 in all (the oracle
                                                 # works in the reference's blocks of 16 384 and keeps a partial one pending)
G_BLOCK = 49152                                  # narrow samples the handle takes per call, at most


def stations_signal(n, noise=0.0, seed=0):
    """One 10 MS/s stream that holds three mono FM stations, 50 kHz deviation, a tone each (and white noise) -> [1, n, 2] f32."""
    t = np.arange(n, dtype=np.float64)
    x = np.zeros(n, np.complex128)
    for f, tone in zip(G_OFFS, G_TONES):
        x += 0.25 * np.exp(1j * (2 * np.pi * ((f * np.arange(n, dtype=np.int64)) % G_RATE) / G_RATE + (50000.0 / tone) * np.sin(2 * np.pi * tone * t / G_RATE)))
    if noise:
        rng = np.random.default_rng(seed)
        x += noise * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return np.stack([x.real, x.imag], axis=-1).astype(np.float32)[None]


def _handle(fmx_amd):
    M = fmx_amd.fmx
    f = fmx_amd.Fmx(3, max_block=G_BLOCK)
    for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 2)):
        f.set_param(pid, v)
    return f


def test_chained_into_a_handle(fmx_amd, ol):
    """A 10 MS/s stream with three mono FM stations through a rate object into a 3-channel handle on the same stream, 85 ms: device chain and
    host calls agree bit for bit, the PCM is within 1e-5 RMS of the oracle run on the model's output, each channel's strongest tone is its
    own station's."""
    import torch
    wide = stations_signal(sum(G_CALLS))
    dev = torch.device("cuda:0")
    d_wide = torch.from_numpy(wide).to(dev)
    d_narrow = torch.zeros((3, G_BLOCK, 2), dtype=torch.float32, device=dev)
    cap = G_BLOCK // 48 + 96
    d_pcm = torch.zeros((3, cap, 2), dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    w = fmx_amd.Wideband(rate_hz=G_RATE, stream_of_output=[0, 0, 0], offset_hz=G_OFFS, streams=1, max_block=max(G_CALLS))
    f = _handle(fmx_amd)
    pcm_dev, counts, pos = [], [], 0
    try:
        for n in G_CALLS:
            got = w.process_device(d_wide.data_ptr() + 8 * pos, wide.shape[1], n, d_narrow.data_ptr(), G_BLOCK, hip_stream=stream.cuda_stream)
            frames = f.process_device(d_narrow.data_ptr(), G_BLOCK, got, d_pcm.data_ptr(), cap, hip_stream=stream.cuda_stream)
            stream.synchronize()
            pcm_dev.append(d_pcm[:, :frames].cpu().numpy())
            counts.append(got)
            pos += n
    finally:
        w.close()
        f.close()
    pcm_dev = np.concatenate(pcm_dev, axis=1)
    assert len(set(counts)) > 1 and sum(counts) == rm.Ratio(G_RATE).before(sum(G_CALLS))
    w = fmx_amd.Wideband(rate_hz=G_RATE, stream_of_output=[0, 0, 0], offset_hz=G_OFFS, streams=1, max_block=max(G_CALLS))
    f = _handle(fmx_amd)
    pcm_host, pos = [], 0
    try:
        for n in G_CALLS:
            pcm_host.append(f.process_host(w.process_host(wide[:, pos:pos + n])))
            pos += n
    finally:
        w.close()
        f.close()
    pcm_host = np.concatenate(pcm_host, axis=1)
    assert pcm_dev.shape == pcm_host.shape and pcm_dev.shape[1] > 3000
    assert np.array_equal(pcm_dev.view(np.uint32), pcm_host.view(np.uint32))
    ref = rm.WidebandRateModel(G_RATE, G_OFFS).process(wm.convert(wide[0], 0))
    print()
    for c in range(3):
        iq = np.stack([ref[c].real, ref[c].imag], axis=-1).astype(np.float32)
        po = ol.OracleChain(inputFilterBw=165000, fmMode=2).process(iq)
        assert po.shape == pcm_dev[c].shape, (po.shape, pcm_dev[c].shape)
        err = float(np.sqrt(np.mean((pcm_dev[c].astype(np.float64) - po) ** 2)))
        seg = pcm_dev[c][1024:, 0].astype(np.float64)
        spec = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
        spec[:4] = 0.0
        peak_hz = float(np.argmax(spec)) * 48000.0 / len(seg)
        print("[g, station %d at %+d Hz] PCM RMS diff vs oracle on the model's output %.3e, level %.3f, strongest tone %.1f Hz (sent %.0f)"
              % (c, G_OFFS[c], err, float(np.sqrt(np.mean(seg ** 2))), peak_hz, G_TONES[c]))
        assert err <= 1e-5, (c, err)
        assert abs(peak_hz - G_TONES[c]) <= 48000.0 / len(seg) * 1.5, (c, peak_hz)
        assert np.sqrt(np.mean(seg ** 2)) > 0.01


# ---- h. the band survey of a rate object ----------------------------------------------------------------------------------------------
H_CALLS = [50000, 40000, 45000]                  # multiples of 4: a factor-4 object takes the same calls; two records of 16 blocks


def test_survey_on_a_rate_object(fmx_amd):
    """The survey's block transform does not know the rate: the records of a rate object are byte-identical to those of a factor object fed
    the same samples, stage W's outputs are bit-identical with the survey on and off, and the finder for a 10 MS/s stream finds the three
    stations and nothing else at 10 dB."""
    wide = stations_signal(sum(H_CALLS), noise=0.007, seed=5)
    objs = {"rate, survey": fmx_amd.Wideband(rate_hz=G_RATE, stream_of_output=[0, 0, 0], offset_hz=G_OFFS, max_block=max(H_CALLS)),
            "rate": fmx_amd.Wideband(rate_hz=G_RATE, stream_of_output=[0, 0, 0], offset_hz=G_OFFS, max_block=max(H_CALLS)),
            "factor, survey": fmx_amd.Wideband(4, [0], [0], max_block=max(H_CALLS))}
    out = {k: [] for k in objs}
    try:
        objs["rate, survey"].survey(16)
        objs["factor, survey"].survey(16)
        pos = 0
        for n in H_CALLS:
            for k, w in objs.items():
                out[k].append(w.process_host(wide[:, pos:pos + n]))
            pos += n
        recs_r, pow_r = objs["rate, survey"].survey_read(0)
        recs_f, pow_f = objs["factor, survey"].survey_read(0)
        assert len(objs["rate"].survey_read(0)[0]) == 0
    finally:
        for w in objs.values():
            w.close()
    assert len(recs_r) == 2 and recs_r.tobytes() == recs_f.tobytes() and pow_r.tobytes() == pow_f.tobytes()
    a, b = np.concatenate(out["rate, survey"], axis=1), np.concatenate(out["rate"], axis=1)
    assert a.shape[1] == rm.Ratio(G_RATE).before(sum(H_CALLS)) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for rec in pow_r:
        st, floor_db = fmx_amd.fmx.survey_stations(rec, rate_hz=G_RATE, threshold_db=10.0)
        print("\n[h] floor %.1f dB, stations %s" % (floor_db, [(int(s["offset_hz"]), round(float(s["snr_db"]), 1)) for s in st]))
        assert [int(s["offset_hz"]) for s in st] == G_OFFS
    with pytest.raises(fmx_amd.fmx.FmxError):
        fmx_amd.fmx.survey_stations(pow_r[0], factor=4, rate_hz=G_RATE)      # cfg->factor must be 0 beside a rate


# ---- i. the C++ wrapper ---------------------------------------------------------------------------------------------------------------
def build_demo(fmx_amd, exe):
    here = os.path.dirname(os.path.abspath(__file__))
    host = os.path.join(os.path.dirname(fmx_amd.__file__), "host")
    lib = os.path.dirname(fmx_amd.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + host, os.path.join(here, "wideband_rate_demo", "wideband_rate_demo.cpp"),
                           "-L" + lib, "-lfmx", "-Wl,-rpath," + lib, "-o", exe])


def test_cpp_adapter(fmx_amd, tmp_path):
    """host/wideband_adapter.h with a rate: processHost in two calls with setOffset between them, the counts from outputsFor, writes what
    fmx_amd.Wideband computes, bit for bit."""
    rate, n, n_first = 2500000, 330, 77
    r = rm.Ratio(rate)
    offs = [0, -412345, r.lim]
    raw = rm.signal(rate, n, [0, 0, 0], offs, 1)
    exe, fin, fout = str(tmp_path / "wideband_rate_demo"), str(tmp_path / "wide.f32"), str(tmp_path / "narrow.f32")
    build_demo(fmx_amd, exe)
    raw[0].tofile(fin)
    out = subprocess.run([exe, fin, fout, str(rate), str(n_first), "1", "733001"] + [str(f) for f in offs], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=120)
    text = out.stdout.decode()
    assert out.returncode == 0, text
    assert "taps %d %d %d" % (r.NH, r.L, r.M) in text and "ok 1 factor 0 outputs 3" in text, text
    assert "counts %d %d" % (r.count(0, n_first), r.count(n_first, n - n_first)) in text, text
    w = fmx_amd.Wideband(rate_hz=rate, stream_of_output=[0, 0, 0], offset_hz=offs, streams=1, max_block=n)
    try:
        a = w.process_host(raw[:, :n_first])
        w.set_offset(1, 733001)
        b = w.process_host(raw[:, n_first:])
    finally:
        w.close()
    want = np.concatenate([a, b], axis=1)
    got = np.fromfile(fout, np.float32).reshape(3, r.before(n), 2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

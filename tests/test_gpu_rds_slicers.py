"""The RDS back end of fmx_rds.hip -- rds_matched, rds_agc, rds_symbols; rds1_costas, rds1_fir, rds1_slicer; rds3_slicer -- per symbol and per call
on the kernels' own baseband.

After EVERY call the test reads what the call's slicers were given (FMX_TAP_RDS_IQ, fmx_last_rds_samples_of) and what they made of it: the bits
(fmx_rds_bits), RDS_2's symbols (fmx_rds_symbols) and the scalar state (fmx_debug_rds_state).  The reference is the oracle's slicer as an object
of its own (fmo_rds_slicer: the oracle's decoders, unchanged), resumed over exactly those samples call by call.  Asserted
(rds_slicer_model.compare):
  * every call slices as many bits as the oracle over the same samples -- which pins the bit times to the call grid;
  * every bit is the oracle's from the first one, but for those the oracle itself decides on less than 1e-3 of the decision variable's peak:
    only within 64 bit periods behind the baseband's first non-zero sample, at most 40 per channel (35-36 on the CPU);
  * mMu, recomputed on the kernels' baseband, stays 1e-4 away from an integer ("choose another seed" otherwise; never a skip);
  * every RDS_2 symbol within 4 x SENS of the peak; behind every call every state field within 4 x SENS of its peak, integer fields equal.
SENS is the oracle's own sensitivity to one rounding of its input (tests/test_rds_slicer_cpu.py::test_sens measures it, on the CPU); the factor
of four and the admission of the signals are derived in tests/rds_slicer_model.py.  None of the bounds was taken from the kernels.

Calls (rds_slicer_model.SIZES, input samples): 12, 192 (two outputs: rds_agc's branch for fewer than three) and 288 both in front of the live
baseband and inside it, 245760 (exactly one AGC round of 2560), 245856 (a second round of one sample), 383988 (31999 fm samples), 500000 and
400000 (made in pieces), the rest off the 96-sample grid.
"""
import importlib

import numpy as np
import pytest

import rds_slicer_model as rm

pytestmark = pytest.mark.gpu

M = importlib.import_module("sdr-j-fm_amd").fmx
N = int(rm.GPU_SECONDS * rm.RATE_IN)
STATE_OF = {2: dict(gain="rds2_gain", freq="rds2_freq", phase="rds2_phase", mu="rds2_mu", skip="rds2_skip", sample_count="rds2_sample_count"),
            1: dict(freq="rds1_freq", phase="rds1_phase", last_sync="rds1_last_sync"),
            3: dict(freq="rds3_freq", phase="rds3_phase", bit_clk_phase="rds3_bit_clk_phase", sync_err="rds3_sync_err", synced="rds3_synced")}


def defaults(f):
    for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 0), (M.P_FM_DECODER, 3)):
        f.set_param(pid, v)


def run(fmx_amd, iq, sizes, modes, join=None, probes=None, twins=()):
    """iq [streams, n, 2] through a handle of len (modes) channels (channel c on stream c % streams, decoder modes [c] switched on with call
    join [c]) in calls of `sizes`; after every call the observables of every probe channel.  -> {channel: (baseband, [Call])}.
    twins: groups of channels that must be bit-identical in bits and symbols, call by call."""
    nch, streams = len(modes), iq.shape[0]
    join = join or [0] * nch
    probes = list(range(nch)) if probes is None else probes
    watched = sorted(set(probes) | {c for g in twins for c in g})
    f = fmx_amd.Fmx(nch, streams=streams, stream_of_channel=[c % streams for c in range(nch)], max_block=max(sizes))
    defaults(f)
    base, calls = {c: [] for c in probes}, {c: [] for c in probes}
    pos = 0
    for k, s in enumerate(sizes):
        for c in range(nch):
            if join[c] == k:
                f.set_param(M.P_RDS_MODE, modes[c], c)
        f.process_host(iq[:, pos:pos + s])
        pos += s
        seen = {}
        for c in watched:
            if join[c] > k:
                continue
            seen[c] = (f.rds_bits(c), f.rds_symbols(c) if modes[c] == 2 else None)
        for g in twins:
            g = [c for c in g if c in seen]
            for c in g[1:]:
                assert np.array_equal(seen[c][0], seen[g[0]][0]), "call %d: the bits of channels %d and %d differ" % (k, g[0], c)
                assert modes[c] != 2 or np.array_equal(seen[c][1], seen[g[0]][1]), "call %d: the symbols of channels %d and %d differ" % (k, g[0], c)
        for c in probes:
            if join[c] > k:
                continue
            n = f.last_rds_samples(c)
            base[c].append(f.tap(M.TAP_RDS_IQ, n, c).reshape(-1, 2))
            bits, sym = seen[c]
            st = f.debug_rds_state(c)
            assert st["mode"] == modes[c]
            var = np.zeros((bits.size, 4))
            if modes[c] == 2:
                assert sym.shape[0] == bits.size, "call %d, channel %d: %d bits and %d symbols" % (k, c, bits.size, sym.shape[0])
                var[:, :2] = sym
            calls[c].append(rm.Call(n, bits, None, var, {k2: st[v] for k2, v in STATE_OF[modes[c]].items()}))
    assert pos == iq.shape[1]
    return {c: (np.concatenate(base[c]), calls[c]) for c in probes}


def check(what, mode, q, got):
    """One channel against the oracle's slicer over the same calls; prints what it measured."""
    ref = rm.run_oracle(mode, q, [c.n for c in got])
    und = rm.undecided(ref, q)[0]
    gb, rb = np.concatenate([c.bits for c in got]), rm.flat(ref)[0]
    nb = min(gb.size, rb.size)
    try:
        d = ", ".join("%s %.2e (%.2e)" % (k, v[0], rm.BOUND_FACTOR * rm.SENS[mode][k]) for k, v in rm.distances(mode, got, ref).items())
    except AssertionError as e:
        d = "no distances: %s" % e
    print("\n[%s, RDS_%d] %d samples, live from %d; bits %d, the oracle's %d (%d of them undecided), %d differ; mMu margin %s; of the peak (bound): %s"
          % (what, mode, q.shape[0], rm.first_live(q), gb.size, rb.size, int(und.sum()), int((gb[:nb] != rb[:nb]).sum()),
             rm.mu_margin(ref, q) if mode == 2 else None, d))
    rm.admit(mode, ref, q)
    return rm.compare(mode, got, ref, q)


def one_receiver(fmx_amd, name, mode):
    iq = rm.signal(name)[None, :N]
    q, got = run(fmx_amd, iq, rm.SIZES, [mode])[0]
    assert [c.n for c in got] == rm.samples_of(rm.SIZES)
    return check("one receiver, %s" % name, mode, q, got), got


@pytest.mark.parametrize("name", ["clean", "noisy"])
def test_rds2_one_receiver(fmx_amd, ol, name):
    """a. One receiver, RDS_2, the calls above: rds_matched's look-back into the ring across every call, rds_agc's one, two and three rounds, its
    hand-over of three samples and its branch for fewer than three, rds_symbols' jump across calls of no symbol.
    Reference alone (CPU): SENS symbol 6.4e-7, gain 1.3e-7, freq 1.5e-5, phase 7.6e-8, mMu 2.2e-6 of their peaks; bounds four times that.
    Measured on the MI355X: symbol 1.3e-7 (clean), 1.8e-7 (noisy); gain and mMu equal; freq 5.8e-6 / 1.1e-6; phase 3.8e-8 / equal; no bit differs.
    With rds_agc's gain from an f64 scan of affine maps (before this test): gain 4.3e-5, symbol 1.5e-4 (clean) / 4.3e-5 (noisy), mMu 8.1e-5,
    phase 8.7e-6, freq 1.1e-4 of their peaks, from the call in which the baseband comes alive -- the bits were the oracle's all the same."""
    w, got = one_receiver(fmx_amd, name, 2)
    assert sum(c.bits.size for c in got) > 1700


@pytest.mark.parametrize("name,mode", [(n, m) for n, m in rm.GPU_USES if m != 2])
def test_rds1_rds3_one_receiver(fmx_amd, ol, name, mode):
    """b. The same with RDS_1 (Costas, two time-parallel FIRs over the rings, the band-pass and slope detector) and RDS_3 (Costas, bit clock,
    integrate and dump, the block synchroniser's reaction on the bit clock).  On whole groups ("programme") RDS_3's synchroniser locks; on random
    bits it hunts and counts the sync errors of chance matches (one or two in 1.5 s); on "sync_errors" -- nine groups with a damaged block B, then
    whole ones -- the fourth sync error resynchronises the bit clock in mid-stream, twice, and the synchroniser locks behind it (asserted on the
    kernel's state; bitClkPhase and the counts equal the oracle's after every call).
    Reference alone (CPU): SENS RDS_1 freq 6.5e-6, phase 9.5e-7, lastSync 1.8e-5; RDS_3 freq 4.3e-6, phase 5.0e-7, bitClkPhase equal.
    Measured on the MI355X: RDS_1 freq 6.0e-7 ... 1.5e-6, phase 3.8e-8 ... 1.1e-7, lastSync 4.7e-6 ... 1.1e-5; RDS_3 freq and phase the same figures,
    on "sync_errors" freq 3.4e-6, phase 3.8e-7; bitClkPhase and the sync-error counts equal, across both resynchronisations; no bit differs."""
    w, got = one_receiver(fmx_amd, name, mode)
    assert sum(c.bits.size for c in got) > 1300
    if name == "programme" and mode == 3:
        assert got[-1].state["synced"] == 1 and max(c.state["sync_err"] for c in got) <= 3
    if name == "sync_errors":
        # rds3_slicer's `bs_sync_err > 3` branch in mid-stream: 21 rdsFilter outputs rebuilt from c_ring, bit_clk_phase and the synchroniser's state
        # rewritten.  The kernel's own count goes back to 0 behind a call (twice: 2, 2, 2, 3, 0, 0, 3, 1 ... on the CPU) and it locks afterwards.
        errs = [c.state["sync_err"] for c in got]
        live = [k for k, e in enumerate(errs) if e > 0]
        assert live and any(errs[k] == 0 for k in range(live[0], len(errs))) and sum(b < a for a, b in zip(errs, errs[1:])) >= 2, errs
        assert got[-1].state["synced"] == 1


def test_tap_reaches_back_8192_samples(fmx_amd):
    """A call of 800000 input samples (three pieces) gives 8333 baseband samples, counted over the whole call; the ring the tap is read from keeps
    8192: more is refused, 8192 are handed out and end in the ring's newest."""
    f = fmx_amd.Fmx(1, max_block=800000)
    defaults(f)
    f.set_param(M.P_RDS_MODE, 2)
    f.process_host(rm.signal("clean")[None, :800000])
    assert f.last_rds_samples(0) == 800000 // 12 // 8 == 8333
    with pytest.raises(fmx_amd.FmxError) as e:
        f.tap(M.TAP_RDS_IQ, 8333, 0)
    assert e.value.code == M.FMX_E_INVALID
    assert np.array_equal(f.tap(M.TAP_RDS_IQ, 8192, 0)[-100:], f.tap(M.TAP_RDS_IQ, 100, 0))


def test_rds2_offset(fmx_amd, ol):
    """d. A carrier 3 kHz off with noise: the Costas loop works (freq and phase move), one RDS_2 receiver.
    Measured on the MI355X: symbol 1.9e-7, gain 1.2e-7, freq 7.2e-6, mMu 2.1e-6 of their peaks (bounds 2.6e-6, 5.2e-7, 6.0e-5, 8.8e-6); phase equal."""
    one_receiver(fmx_amd, "offset", 2)


def test_batch_of_70(fmx_amd, ol):
    """c. 70 channels on two streams (clean, noisy), RDS_1 / _2 / _3 interleaved, the decoders of channels 0-29 on from the first call, of 30-49
    from the third, of 50-69 from the fourth (rds_slicer_model.BATCH_SIZES): lanes of one wave at three phases of the decimator and the blocks,
    three slicers sharing RdsState::nbits and the bit ring.  Eight probe channels against the oracle; channels of equal stream, mode and start
    bit-identical in bits and symbols after every call.
    Measured on the MI355X, worst of the eight: RDS_2 symbol 5.1e-7 (channel 55, on from call 3; bound 2.6e-6), gain 3.2e-8, freq 8.9e-6, phase and
    mMu equal; RDS_1 freq 2.1e-6, phase 7.6e-8, lastSync 1.4e-5 (bound 7.2e-5); RDS_3 freq 2.6e-6, phase 1.5e-7 (bound 2.0e-6), bitClkPhase equal;
    no bit differs, 1-3 undecided bits on the channels switched on later (their filters start inside the signal), 35-36 on the others."""
    nch, sizes = rm.BATCH_CHANNELS, rm.BATCH_SIZES
    modes = [rm.batch_channel(c)[1] for c in range(nch)]
    join = [rm.batch_channel(c)[2] for c in range(nch)]
    starts = {k: sum(sizes[:k]) // 12 for k in (0, 2, 3)}
    assert len({j % 8 for j in starts.values()}) == 3 and len({j % 32000 for j in starts.values()}) == 3
    groups = {}
    for c in range(nch):
        groups.setdefault(rm.batch_channel(c), []).append(c)
    probes = rm.BATCH_PROBES
    assert sorted({modes[c] for c in probes}) == [1, 2, 3] and sorted({join[c] for c in probes}) == [0, 2, 3]
    assert all(len({modes[c] for c in probes if join[c] == j}) >= 2 for j in (0, 2, 3))
    iq = np.stack([rm.signal("clean")[:N], rm.signal("noisy")[:N]])
    out = run(fmx_amd, iq, sizes, modes, join, probes, twins=list(groups.values()))
    for c in probes:
        q, got = out[c]
        assert [x.n for x in got] == rm.samples_of(sizes, join[c])
        check("channel %d of 70, %s, on from call %d" % (c, rm.batch_channel(c)[0], join[c]), modes[c], q, got)

"""The read cursors of the per-channel read-outs (fmx_rds_symbols, fmx_rds_bits, fmx_get_peaks) and the two PLL counters' channel ranges: a reader
that takes less than is there goes on where it stopped, a reader that fell behind a ring gets the ring's last entries, and a read-out with nothing
new returns nothing.  The GPU is compared with itself: a handle of two channels on one stream with the same settings is read only at the end, and
what it hands out then is what a reader that kept up has collected.  For the peak levels that reader is the twin channel, read once with room for
everything.  For the RDS symbols and bits it is the same channel of a second handle, made and fed alike, and read after every call: the twins' PCM is
equal bit for bit, but their RDS symbols are not (measured: they differ in the last bits, 2e-6 at most, from the first symbol that is not zero on, and 16
of the bits decided on the 30 faint symbols of the onset differ), while a channel repeats itself bit for bit from handle to handle.  The signal is
1.15 s long: the shortest that puts more symbols into the symbol ring than its 1024 entries (1187.5 symbols per second, behind the RDS band-pass's
block of 32000 fm samples)."""
import importlib

import numpy as np
import pytest

import rds_streams as rs

pytestmark = pytest.mark.gpu

M = importlib.import_module("sdr-j-fm_amd").fmx
BLOCK = 49152
CALLS = 54
SYM_CAP = 1024              # RDS_SYM_CAP (fmx_internal.h)


@pytest.fixture(scope="module")
def run(fmx_amd, ol):
    """The handle that nobody has read, after its last call; channel 1's symbols, read call by call, and its bits, read in one go, of the handle that
    was read all along."""
    iq = ol.synth_iq(CALLS * BLOCK, rds=1, rdsLevel=0.05, rds_payload=rs.programme(**rs.PROG_A))

    def handle():
        f = fmx_amd.Fmx(2, streams=1, stream_of_channel=[0, 0], max_block=BLOCK)
        for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_RDS_MODE, 2),
                       (M.P_SCOPE_TAPS, 1), (M.P_DISP_DELAY, 4), (M.P_PLL_SOLVER, 2)):
            f.set_param(pid, v)
        return f

    kept_up, sym = handle(), []
    for i in range(0, CALLS * BLOCK, BLOCK):
        kept_up.process_host(iq[i:i + BLOCK])
        sym.append(kept_up.rds_symbols(1))
    bits = kept_up.rds_bits(1)
    kept_up.close()
    f = handle()
    for i in range(0, CALLS * BLOCK, BLOCK):
        f.process_host(iq[i:i + BLOCK])
    yield f, np.concatenate(sym), bits
    f.close()


def test_symbols_behind_the_ring(run):
    """Channel 1's first read comes after more symbols than the ring holds: it gets the last 1024 of those read call by call, bit for bit, and then
    nothing."""
    f, sym, _ = run
    print("\n[readout cursors] %d symbols read call by call" % sym.shape[0])
    assert sym.shape[0] > SYM_CAP
    late = f.rds_symbols(1, SYM_CAP)
    assert late.shape == (SYM_CAP, 2)
    assert late.tobytes() == sym[-SYM_CAP:].tobytes()
    assert f.rds_symbols(1, SYM_CAP).shape[0] == 0


def test_bits_in_small_reads(run):
    """Seven bits at a time until nothing is left: the same bits as a single read."""
    f, sym, whole = run
    parts = []
    while True:
        b = f.rds_bits(1, 7)
        if b.size == 0:
            break
        assert b.size <= 7
        parts.append(b)
    got = np.concatenate(parts)
    print("\n[readout cursors] %d bits in %d reads" % (got.size, len(parts)))
    assert whole.size == sym.shape[0]                   # (a symbol per bit: both count RdsState::nbits)
    assert all(p.size == 7 for p in parts[:-1])
    assert np.array_equal(got, whole)
    assert f.rds_bits(1, 7).size == 0 and f.rds_bits(1).size == 0


def test_peaks_in_small_reads(run):
    """Three windows at a time: the display delay line (four steps) is carried from read to read, so the pieces are the twin's single read."""
    f = run[0]
    whole = f.peaks(0)
    parts = []
    while True:
        p = f.peaks(1, 3)
        if p.shape[0] == 0:
            break
        assert p.shape[0] <= 3
        parts.append(p)
    got = np.concatenate(parts)
    print("\n[readout cursors] %d peak windows in %d reads" % (got.shape[0], len(parts)))
    assert whole.shape[0] > 3 * 4                        # (more reads than the delay line has steps)
    assert np.any(whole[4:] != -40.0) and np.all(whole[:4] == -40.0)      # (the first four are the delay line's initial entries)
    assert got.tobytes() == whole.tobytes()
    assert f.peaks(0).shape[0] == 0 and f.peaks(1, 3).shape[0] == 0


def test_pll_counters_over_all_channels(run):
    """Channel -1 is the sum over the channels."""
    f = run[0]
    replays = [f.pll_replays(c) for c in range(2)]
    exact = [f.pll_exact_segments(c) for c in range(2)]
    print("\n[readout cursors] PLL replays %s, exact segments %s" % (replays, exact))
    assert f.pll_replays(-1) == sum(replays)
    assert f.pll_exact_segments(-1) == sum(exact)
    assert replays[0] == replays[1] and exact[0] == exact[1]

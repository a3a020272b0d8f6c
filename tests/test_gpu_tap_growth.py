"""Unread items survive a growth.  A slot tap (the spectrum and multiplex spectrum meters, the sub-carrier decoder, the monitoring feed: fmx_taps.h) gives a
unit its slot of device memory when it is first switched on: the slotted arrays are allocated anew and the slots in use copied (grow_slots, fmx_host.h).
Here unit 0 has unread items in its ring, and a record or block in progress, when unit 1 is switched on; what unit 0 then reads must be what it reads on a
twin handle that never grows, and unit 1's first item what it is on a twin where unit 1 alone was switched on by the same call.  Equalities between two
runs of the same kernels: indices and payload bytes, no tolerance."""
import numpy as np
import pytest

import sca_signal as sg

pytestmark = pytest.mark.gpu

R = 12                                        # input samples per fm sample
CALLS = (2.25, 2.25, 3.75)                    # in blocks (whole fm samples for every tap): two calls with unit 0 alone, the growth, one more call


def spec_read(f, u):
    r, mean, peak = f.spectrum_read(u)
    return [int(i) for i in r["index"]], [mean[k].tobytes() + peak[k].tobytes() for k in range(len(r))]


def mpx_read(f, u):
    r, mean, peak = f.mpx_spectrum_read(u, 1)[0]
    return [int(i) for i in r["index"]], [mean[k].tobytes() + peak[k].tobytes() for k in range(len(r))]


def sca_read(f, u):
    first, audio, level = f.sca_read(u, 1)[0]
    return [first + k for k in range(len(audio))], [audio[k].tobytes() + np.float32(level[k]).tobytes() for k in range(len(audio))]


def feed_read(f, u):
    first, audio, power = f.feed_read(u, 1)[0]
    return [first + k for k in range(len(audio))], [audio[k].tobytes() + np.float32(power[k]).tobytes() for k in range(len(audio))]


# tap: (input samples per block, setup, switch a unit on, read a unit, the items unit 0 holds unread at the growth, all it reads behind the last call,
# unit 1's first item).  The memory grows 4.5 blocks into the streams, the last call ends at 8.25.  Two blocks per record for the two spectrum meters:
# records 0 and 1 are complete and half of block 4 is carried when the memory grows; unit 1, on from block 5, delivers record 3 first.  The decoder and
# the feed look back less than a block (703 fm samples, 143 frames): unit 0 delivers from block 1, unit 1, on at 4.5 blocks, from block 5.
TAPS = {
    "spectrum": (4096, lambda f: f.spectrum_setup(2, 1), lambda f, u: f.spectrum_meter(True, u), spec_read, 2, [0, 1, 2, 3], 3),
    "mpx": (4096 * R, lambda f: f.mpx_spectrum_setup(2, 1), lambda f, u: f.mpx_spectrum_meter(True, u), mpx_read, 2, [0, 1, 2, 3], 3),
    "sca": (1920 * R, lambda f: None, lambda f, u: f.sca_enable(67000, u), sca_read, 3, [1, 2, 3, 4, 5, 6, 7], 5),
    "feed": (1920 * R, lambda f: None, lambda f, u: f.feed(1, u), feed_read, 3, [1, 2, 3, 4, 5, 6, 7], 5),
}

_IQ = {}


def iq_streams(n):
    """[2, n, 2] f32: two FM streams with a programme and a sub-carrier at 67 kHz (tests/sca_signal.py), seeds 1 and 2"""
    if n not in _IQ:
        n_fm = (n + R - 1) // R
        _IQ[n] = np.stack([sg.fm_iq(sg.multiplex(n_fm * R, 192000 * R, with_programme=True, seed=1 + s, centre_hz=67000), 192000 * R)[:n] for s in range(2)])
    return _IQ[n]


@pytest.mark.parametrize("tap", sorted(TAPS))
def test_unread_items_survive_a_growth(fmx_amd, tap):
    m = fmx_amd.fmx
    block, setup, switch_on, read, unread_at_growth, want0, want1 = TAPS[tap]
    cuts = [int(c * block) for c in CALLS]
    x = iq_streams(sum(cuts))
    # the handle that grows; the twin with unit 0 on throughout; the twin on which unit 1 alone is switched on by the last call
    handles = [fmx_amd.Fmx(2, max_block=max(cuts)) for _ in range(3)]
    grows, only0, only1 = handles
    try:
        for f in handles:
            setup(f)
        switch_on(grows, 0); switch_on(only0, 0)
        g = 0
        for k, n in enumerate(cuts):
            if k == len(cuts) - 1:
                switch_on(grows, 1); switch_on(only1, 1)      # (the memory of `grows` grows from one slot to two with two calls' items unread in slot 0)
            for f in handles:
                f.process_host_raw(x[:, g:g + n], m.IQ_F32)
            g += n
        got0, got1, twin0, twin1 = read(grows, 0), read(grows, 1), read(only0, 0), read(only1, 1)
        assert len([i for i in want0 if (i + 1) * (2 if tap in ("spectrum", "mpx") else 1) * block <= cuts[0] + cuts[1]]) == unread_at_growth >= 2
        assert got0[0] == want0 and twin0[0] == want0, (got0[0], twin0[0])
        assert got0[1] == twin0[1], [k for k in range(len(want0)) if got0[1][k] != twin0[1][k]]
        assert got1[0] and got1[0][0] == want1 and twin1[0][0] == want1, (got1[0], twin1[0])
        assert got1[1][0] == twin1[1][0]
        assert read(only1, 0)[0] == [] and read(only0, 1)[0] == []
    finally:
        for f in handles:
            f.close()

"""The block synchroniser on the GPU (kernel rds_sync, fmx_rds.hip) and the batch read-outs fmx_rds_decode_all / fmx_rds_groups against the
per-channel path (fmx_rds_decode: the synchroniser on the host over the bit ring) and against the generator's own groups.  Chosen bit sequences --
clean programmes, and one with a payload bit error, a five-bit burst, a checkword error, a sync error, a type-B group, PI changes, a dropped and an
inserted bit (tests/rds_streams.py) -- reach the synchroniser through the whole chain, as the 57 kHz sub-carrier of synthetic FM streams of 3.6 s."""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest

import rds_streams as rs

pytestmark = pytest.mark.gpu

M = importlib.import_module("sdr-j-fm_amd").fmx
BLOCK = 16384 * 20
N = int(3.6 * 2304000) // BLOCK * BLOCK
FIELDS = [name for name, _ in M.FmxRdsInfo._fields_]


@pytest.fixture(scope="module")
def streams(ol):
    """Three streams: programme A clean, the faulty payload, programme B clean -- IQ [3, N, 2], the payloads, and the bits the generator sent."""
    payloads = [rs.programme(**rs.PROG_A), rs.faulty_payload(), rs.programme(**rs.PROG_B)]
    made = [ol.synth_iq(N, return_rds_bits=True, rds=1, rdsLevel=0.05, rds_payload=p) for p in payloads]
    iq = np.stack([m[0] for m in made])
    iq.setflags(write=False)
    return iq, payloads, [m[1] for m in made]


def gui_defaults(f):
    for pid, v in ((M.P_BANDWIDTH, 165000), (M.P_LF_CUTOFF, 15000), (M.P_DEEMPHASIS, 50), (M.P_VOLUME_DB, -6.0), (M.P_FM_MODE, 0), (M.P_FM_DECODER, 3)):
        f.set_param(pid, v)


def value(info, name):
    v = getattr(info, name)
    if name == "bit_error_rate":
        return struct.pack("<f", v)                       # bit for bit
    if name == "radio_text_ucs2":
        return list(v)
    return v


def same_info(a, b, what):
    for name in FIELDS:
        assert value(a, name) == value(b, name), (what, name, value(a, name), value(b, name))


def words(payload):
    """The (A, B, C, D) payload words of a stream of whole groups."""
    g = np.asarray(payload, np.int64).reshape(-1, 4, rs.BLOCK)[:, :, :16]
    return (g << np.arange(15, -1, -1)).sum(axis=2)


def pull_in(rx, tx):
    """Where the received bits become the transmitted ones for good: (p, shift) with rx[i] == tx[i + shift] for every i >= p.  The chain delays the
    bits (filter latency, some hundred bit periods), so shift is negative and p >= -shift: the received bits in front of that answer to nothing sent.
    The payloads repeat, so the end of rx occurs in tx once per round: the last occurrence is the one the chain's delay leaves room for."""
    tail = rx[-400:]
    hits = [k for k in range(tx.size - tail.size + 1) if np.array_equal(tx[k:k + tail.size], tail)]
    assert hits, "the received bits do not end in what the generator sent"
    shift = hits[-1] - (rx.size - tail.size)
    lo, hi = max(0, -shift), min(rx.size, tx.size - shift)
    assert hi == rx.size, (shift, rx.size, tx.size)                     # (nothing received that was not yet sent)
    bad = np.flatnonzero(rx[lo:hi] != tx[lo + shift:hi + shift])
    return (lo if bad.size == 0 else lo + int(bad[-1]) + 1), shift


def test_batch_equals_per_channel(fmx_amd, streams):
    """130 channels on 3 streams -- three waves of lanes, the last part-filled -- RDS_2 on all but two, one switched on three calls late:
    after every call fmx_rds_decode_all equals fmx_rds_decode channel by channel, field by field; at the end both equal the host decoder
    over the bits the slicer produced, those bits are the generator's behind the pull-in, and the injected faults were met."""
    iq, payloads, sent = streams
    nch, off, late = 130, (5, 77), 64
    f = fmx_amd.Fmx(nch, streams=3, stream_of_channel=[c % 3 for c in range(nch)], max_block=BLOCK)
    gui_defaults(f)
    f.set_param(M.P_RDS_MODE, 2)
    for c in off + (late,):
        f.set_param(M.P_RDS_MODE, 0, c)
    for k, i in enumerate(range(0, N, BLOCK)):
        if k == 3:
            f.set_param(M.P_RDS_MODE, 2, late)
        f.process_host(iq[:, i:i + BLOCK, :])
        infos = f.rds_decode_all()
        assert len(infos) == nch
        for c in range(nch):
            same_info(infos[c], f.rds_decode(c), (k, c))
    same_info(f.rds_decode_all(nch - 1, 1)[0], infos[nch - 1], "the last channel alone")
    same_info(f.rds_decode_all(7, 1)[0], infos[7], "a range of one")
    for c in off:
        assert infos[c].groups_decoded == 0 and infos[c].synchronized == 0 and f.rds_bits(c).size == 0
    for c in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        rx = f.rds_bits(c)
        cpu = fmx_amd.fmx.rds_decode_bits(rx)
        same_info(infos[c], cpu, ("host decoder over the sliced bits", c))
        p, shift = pull_in(rx, sent[c % 3])
        assert p < 1500, (c, p)
        # the CPU run over what was sent starts at the first group boundary behind the pull-in: a synchroniser that starts in mid-group may take
        # a chance match for block A and count a sync error that says nothing about the payload
        q = -(-(p + shift) // rs.GROUP) * rs.GROUP
        tail = fmx_amd.fmx.rds_decode_bits(sent[c % 3][q:shift + rx.size])
        whole = (shift + rx.size - q) // rs.GROUP
        print("\n[rds batch] ch %d: %d bits, pull-in %d, lag %d; groups %d crc %d sync %d (the %d whole groups sent behind the pull-in alone: %d / %d / %d)"
              % (c, rx.size, p, -shift, infos[c].groups_decoded, infos[c].crc_errors, infos[c].sync_errors, whole, tail.groups_decoded, tail.crc_errors, tail.sync_errors))
        if c % 3 == 1:
            # the payload was chosen for this: the faults cost CRC and sync errors, in the CPU run over what was sent and on the GPU
            assert tail.crc_errors >= 3 and tail.sync_errors >= 1
            assert infos[c].crc_errors >= 3 and infos[c].sync_errors >= 1 and infos[c].groups_decoded >= 15
            assert infos[c].pi_code in (rs.PROG_A["pi"], rs.PROG_B["pi"])
        else:
            prog = rs.PROG_A if c % 3 == 0 else rs.PROG_B
            assert tail.crc_errors == 0 and tail.sync_errors == 0 and tail.groups_decoded == whole
            assert infos[c].crc_errors == 0 and infos[c].groups_decoded >= whole - 1
            assert infos[c].pi_code == prog["pi"] and infos[c].pty_code == prog["pty"] and infos[c].synchronized == 1
            if c != late:
                assert infos[c].station_label.decode() == prog["ps"] and infos[c].radio_text.decode() == prog["text"]
                assert infos[c].groups_decoded >= 20


def run_three(fmx_amd, iq, sizes, mode=2, max_block=BLOCK, after_call=None):
    """A handle of three channels, one per stream, fed in calls of the given sizes (in turn) until the streams end."""
    f = fmx_amd.Fmx(3, streams=3, stream_of_channel=[0, 1, 2], max_block=max_block)
    gui_defaults(f)
    f.set_param(M.P_RDS_MODE, mode)
    pos = k = 0
    while pos < iq.shape[1]:
        n = min(sizes[k % len(sizes)], iq.shape[1] - pos)
        f.process_host(iq[:, pos:pos + n, :])
        pos += n
        if after_call:
            after_call(f, k)
        k += 1
    return f


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_every_slicer(fmx_amd, streams, mode):
    """rds_sync runs behind rds1_slicer, rds_symbols and rds3_slicer alike (a block-machine handle of three channels): the same equality."""
    def poll(f, k):
        infos = f.rds_decode_all()
        for c in range(3):
            same_info(infos[c], f.rds_decode(c), (mode, k, c))
    f = run_three(fmx_amd, streams[0], [BLOCK], mode=mode, after_call=poll)
    infos = f.rds_decode_all()
    for c in range(3):
        same_info(infos[c], fmx_amd.fmx.rds_decode_bits(f.rds_bits(c)), (mode, c))
    assert all(f.rds_decode(c).groups_decoded == infos[c].groups_decoded for c in range(3))
    if mode == 2:
        assert infos[0].groups_decoded >= 15 and infos[0].pi_code == rs.PROG_A["pi"]
        assert infos[2].groups_decoded >= 15 and infos[2].pi_code == rs.PROG_B["pi"]


def test_cuts(fmx_amd, streams):
    """Whole blocks, and ragged calls -- one fm sample (12 input samples, far less than a bit), 400000 samples (above 383988: made in RDS pieces),
    odd lengths: the group records are the same, and each clean stream's are the generator's groups in order behind the pull-in."""
    iq, payloads, _ = streams
    ragged = [12, 99991, 400000, 5, BLOCK, 1939, 250001, 24, 383989, 77777]
    recs = []
    for sizes, mb in (([BLOCK], BLOCK), (ragged, 400000)):
        got = [[], [], []]

        def take(f, k, got=got):
            if k % 3 == 0:
                for c, r in enumerate(f.rds_groups()):
                    got[c].append(r)
        f = run_three(fmx_amd, iq, sizes, max_block=mb, after_call=take)
        take(f, 0)
        assert all(r.size == 0 for r in f.rds_groups())
        recs.append([np.concatenate(g) for g in got])
    for c in range(3):
        a, b = recs[0][c], recs[1][c]
        assert a.size >= 20 and a.size == b.size
        for name in ("index", "end_bit", "block"):
            assert np.array_equal(a[name], b[name]), (c, name)
        assert np.array_equal(a["index"], np.arange(a.size))
    for c in (0, 2):
        a, want = recs[0][c], words(payloads[c])
        first = [g for g in range(want.shape[0]) if np.array_equal(want[g], a["block"][0])]
        assert first, "the first record is no group of the programme"
        assert any(all(np.array_equal(a["block"][i], want[(g + i) % want.shape[0]]) for i in range(a.size)) for g in first)
        assert np.all(np.diff(a["end_bit"]) == rs.GROUP)


def test_ring_keeps_the_last_64(fmx_amd, streams):
    """The streams three times over without a read: more than 64 groups complete, fmx_rds_groups hands out the last 64, the gap shows in `index`,
    a second read returns nothing; fmx_rds_decode_all, read for the first time, decodes those 64."""
    iq = streams[0]
    f = fmx_amd.Fmx(3, streams=3, stream_of_channel=[0, 1, 2], max_block=BLOCK)
    gui_defaults(f)
    f.set_param(M.P_RDS_MODE, 2)
    for _ in range(3):
        for i in range(0, N, BLOCK):
            f.process_host(iq[:, i:i + BLOCK, :])
    few = f.rds_groups(capacity=10)
    rest = f.rds_groups()
    again = f.rds_groups()
    infos = f.rds_decode_all()
    for c in (0, 2):
        r = np.concatenate([few[c], rest[c]])
        assert few[c].size == 10 and r.size == 64 and again[c].size == 0
        # (three passes of 41 groups each, less the pull-ins: well above 64 complete, so the first record kept is not the channel's first)
        assert r["index"][0] > 0 and np.array_equal(r["index"], r["index"][0] + np.arange(64))
        assert np.all(np.diff(r["end_bit"]) >= rs.GROUP) and r["end_bit"][-1] <= 3 * (N * 1187.5 / 2304000 + 1)
        assert infos[c].groups_decoded == 64 and infos[c].pi_code == (rs.PROG_A, None, rs.PROG_B)[c]["pi"]


def test_reset(fmx_amd, streams):
    """Both paths polled after every call, FMX_A_RESET_RDS in the middle (nothing pending in either): they stay equal, PI goes through 0 and returns."""
    seen = []

    def poll(f, k):
        infos = f.rds_decode_all()
        for c in range(3):
            same_info(infos[c], f.rds_decode(c), (k, c))
        seen.append(infos[0].pi_code)
        if k == 16:
            assert infos[0].pi_code == rs.PROG_A["pi"] and infos[0].station_label.decode().strip() != ""
            f.set_param(M.A_RESET_RDS, 1)
            infos = f.rds_decode_all()
            for c in range(3):
                same_info(infos[c], f.rds_decode(c), ("reset", c))
                assert infos[c].pi_code == 0 and infos[c].pty_code == -1 and infos[c].station_label == b" " * 8
            seen.append(infos[0].pi_code)
    run_three(fmx_amd, streams[0], [BLOCK], after_call=poll)
    assert seen[17] == 0 and seen[16] == rs.PROG_A["pi"] and seen[-1] == rs.PROG_A["pi"]


def test_edges(fmx_amd):
    """A handle whose RDS was never switched on; ranges of one; bad ranges and null pointers."""
    f = fmx_amd.Fmx(5, streams=1, stream_of_channel=[0] * 5, max_block=16384)
    gui_defaults(f)
    f.process_host(np.zeros((1, 16384, 2), np.float32))
    infos = f.rds_decode_all()
    assert len(infos) == 5
    for c in range(5):
        same_info(infos[c], f.rds_decode(c), c)
        assert infos[c].pi_code == 0 and infos[c].pty_code == -1 and infos[c].groups_decoded == 0
    assert [g.size for g in f.rds_groups()] == [0] * 5
    same_info(f.rds_decode_all(4, 1)[0], infos[4], "the last channel alone")
    assert f.rds_decode_all(2, 0) == [] and len(f.rds_decode_all(3)) == 2
    for first, count in ((-1, 1), (0, 6), (5, 1), (4, 2), (0, -1)):
        with pytest.raises(fmx_amd.FmxError) as e:
            f.rds_decode_all(first, count)
        assert e.value.code == M.FMX_E_INVALID
        with pytest.raises(fmx_amd.FmxError) as e:
            f.rds_groups(first, count)
        assert e.value.code == M.FMX_E_INVALID
    n = (C.c_int32 * 5)()
    assert f.L.fmx_rds_decode_all(f.h, 0, 5, None) == M.FMX_E_INVALID
    assert f.L.fmx_rds_groups(f.h, 0, 5, None, 4, n) == M.FMX_E_INVALID
    assert f.L.fmx_rds_groups(f.h, 0, 5, None, 0, None) == M.FMX_E_INVALID
    assert f.L.fmx_rds_decode_all(None, 0, 1, None) == M.FMX_E_INVALID

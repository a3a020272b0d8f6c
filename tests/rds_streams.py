"""RDS bit streams with chosen faults, built from the generators of tests/oracle_lib.py (rds_group_bits, rds_programme_bits): what
tests/test_rdssync_cpu.py feeds the block synchronisers and tests/test_gpu_rds_batch.py sends through the whole chain as synth_iq's rds_payload."""
import numpy as np

import oracle_lib as ol

GROUP = 104                 # bits per group: four blocks of 16 payload + 10 checkword bits
BLOCK = 26
PROG_A = dict(pi=0xD3A1, pty=10, ps="FMX-AMD ", text="HIP KERNELS ON MI355X - RDS OK")
PROG_B = dict(pi=0x2468, pty=3, ps="CHAN TWO", text="SECOND STREAM")


def programme(**kw):
    return ol.rds_programme_bits(**kw)


def bit_index(group, block, bit):
    """Position in a stream of whole groups: bit 0 .. 15 of a block is its payload (MSB first), 16 .. 25 its checkword."""
    return GROUP * group + BLOCK * block + bit


def flip(bits, positions):
    out = np.array(bits, np.uint8)
    for p in positions:
        out[p] ^= 1
    return out


def type_b_group(pi=0xD3A1, pty=10):
    """A 0B group: block B's version bit set, block C under offset word C'."""
    b = (0 << 12) | (1 << 11) | (pty << 5) | (1 << 3)
    return np.array(ol.rds_group_bits(pi, b, pi, (ord("T") << 8) | ord("B"), type_b=True), np.uint8)


def faulty_payload():
    """24 groups sent round and round: programme A with a payload bit error (group 2, block C), a five-bit burst in a payload (group 5, block D), a
    checkword error (group 8, block B) and -- while the synchroniser is still hunting behind it -- a payload error in the next group's block B (a sync
    error); then programme B (a PI change, and another at the wrap) with a type-B group in place of group 14, a bit dropped from group 17 and a bit
    inserted into group 20."""
    a = programme(**PROG_A)
    b = programme(**PROG_B)
    assert a.size == 12 * GROUP and b.size >= 8 * GROUP
    b = np.concatenate([b, b])[:12 * GROUP]
    bits = np.concatenate([a, b])
    bits = flip(bits, [bit_index(2, 2, 5)])
    bits = flip(bits, [bit_index(5, 3, 6 + k) for k in (0, 2, 3, 4)])          # a burst spanning five bits
    bits = flip(bits, [bit_index(8, 1, 20)])
    bits = flip(bits, [bit_index(9, 1, 3)])
    bits[GROUP * 14:GROUP * 15] = type_b_group(PROG_B["pi"], PROG_B["pty"])
    drop, ins = bit_index(17, 2, 9), bit_index(20, 1, 12)
    bits = np.concatenate([bits[:drop], bits[drop + 1:ins], [1 - bits[ins]], bits[ins:]])
    assert bits.size == 24 * GROUP
    return bits.astype(np.uint8)

// fmx_rdssync.h -- the RDS block synchroniser as one function for host and device.
// A restatement of RdsGroupDecoderHost::push_bit's synchroniser half (fmx_rdsgroups.h: push, syndrome, offset_word, decode_block, meggitt,
// resync and the zeroing of the blocks behind a complete group; rds-blocksynchronizer.cpp:57-336, rds-decoder.cpp:104-131) on a POD state, so that
// the kernel rds_sync (fmx_rds.hip) can run it where the slicers leave their bits.  RdsGroupDecoderHost's own synchroniser stays what this one is
// measured against (tests/rdssync_check.cpp: every field after every bit).  Integer work only: the bit error rate is kept as the numerator and
// denominator it was last computed from, and the host forms the float.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FMX_HD __host__ __device__
#else
#define FMX_HD
#endif

namespace fmx {

struct RdsSync {
    uint32_t stream;                         // the running shift register (32 bits: the synchronised path hands it over unmasked)
    int32_t  synced, cur;                    // crcFifoFilled / the block expected next (0 .. 3)
    uint32_t bits_in_blk, bits_done, bit_err;
    int32_t  n_crc_err, n_sync_err;
    uint32_t ber_num, ber_den;               // bit_err / bits_done as decode_block last divided them (den == 0: never; the rate is 0)
    uint16_t blk[4];                         // the blocks received so far; zeroed behind a complete group
};
// (all zero = rdsBlockSynchronizer::reset / sync_reset)

enum RdsSyncRes { RDS_WAITING_A, RDS_BUFFERING, RDS_NO_SYNC, RDS_NO_CRC, RDS_COMPLETE };
// which paths a run took (tests/rdssync_check.cpp asserts that its streams reach every one); null in the kernel
struct RdsSyncCover { uint64_t waiting_a, found_a, no_sync, no_crc, complete, meggitt_flip, meggitt_run, ber_wrap, type_b_offset; };

namespace rdssync {
constexpr uint32_t NCRC = 10, NPAY = 16, NBLK = 26, POLY = 0x5B9, REM = 0x31B, BER_RESET = 4000;

// the reference's 26-step loop (rds-blocksynchronizer.cpp:126-142) on block = bits ^ offset word
constexpr uint32_t syndrome_loop(uint32_t block) {
    uint32_t reg = 0;
    for (int k = (int)NBLK - 1; k >= 0; k--) {
        const uint32_t msb = reg & (1u << (NCRC - 1));
        reg <<= 1;
        if (msb) reg ^= POLY;
        if ((block >> k) & 1u) reg ^= REM;
    }
    return reg;
}
// The loop is linear over GF(2) in `block` (reg starts at 0; shift, conditional POLY on reg's own bit and conditional REM on a block bit are all
// XOR-linear): syndrome (block) = XOR of syndrome (1 << k) over the set bits k.  Bit j of the result is therefore the parity of block & MASK_j,
// MASK_j = the bits k whose unit syndrome has bit j set -- ten masked popcounts.  Bits 26 .. 31 of `block` are in no mask, as the loop ignores them.
constexpr uint32_t syndrome_mask(int j) {
    uint32_t m = 0;
    for (int k = 0; k < (int)NBLK; k++) if ((syndrome_loop(1u << k) >> j) & 1u) m |= 1u << k;
    return m;
}
template <int J> struct SynMask { static constexpr uint32_t v = syndrome_mask(J); };
FMX_HD inline uint32_t parity32(uint32_t v) { return (uint32_t)__builtin_popcount(v) & 1u; }
FMX_HD inline uint32_t syndrome(uint32_t bits, uint32_t off) {
    const uint32_t b = bits ^ off;
    return parity32(b & SynMask<0>::v) | parity32(b & SynMask<1>::v) << 1 | parity32(b & SynMask<2>::v) << 2 | parity32(b & SynMask<3>::v) << 3 |
           parity32(b & SynMask<4>::v) << 4 | parity32(b & SynMask<5>::v) << 5 | parity32(b & SynMask<6>::v) << 6 | parity32(b & SynMask<7>::v) << 7 |
           parity32(b & SynMask<8>::v) << 8 | parity32(b & SynMask<9>::v) << 9;
}
FMX_HD inline uint32_t offset_word(int blk, bool typeB) {              // rds-blocksynchronizer.cpp:197-213
    return blk == 1 ? 0x198u : blk == 2 ? (typeB ? 0x350u : 0x168u) : blk == 3 ? 0x1B4u : 0xFCu;
}
// blk[1] as it stands: a stale or zeroed value while the synchroniser hunts for block A
FMX_HD inline bool type_b(const RdsSync &s) { return ((s.blk[1] >> 11) & 1) != 0; }
// blk[i] = v without a run-time index (the state lives in registers in the kernel)
FMX_HD inline void set_blk(RdsSync &s, int i, uint16_t v) {
    s.blk[0] = i == 0 ? v : s.blk[0]; s.blk[1] = i == 1 ? v : s.blk[1]; s.blk[2] = i == 2 ? v : s.blk[2]; s.blk[3] = i == 3 ? v : s.blk[3];
}
FMX_HD inline void resync(RdsSync &s) { s.cur = 0; s.synced = 0; s.bits_in_blk = 0; }   // :101-106

// doMeggit (:176-195): flips bits of the running register and counts them; its result is discarded by the caller
FMX_HD inline void meggitt(RdsSync &s, uint32_t syn, RdsSyncCover *cv) {
    uint32_t mask = 1u << (NBLK - 1);
    if (cv) cv->meggitt_run++;
    for (uint32_t i = 0; i < NPAY; i++) {
        if (syn & 0x200) {
            if ((syn & 0x1f) == 0) { s.stream ^= mask; s.bit_err++; if (cv) cv->meggitt_flip++; }
            else syn ^= POLY;
        }
        syn <<= 1; mask >>= 1;
    }
}
FMX_HD inline bool decode_block(RdsSync &s, int b, uint32_t bits, RdsSyncCover *cv) {   // :144-173
    const bool tb = type_b(s);
    if (cv && b == 2 && tb) cv->type_b_offset++;
    const uint32_t syn = syndrome(bits, offset_word(b, tb));
    if (!s.synced) return syn == 0;
    s.bits_done += NPAY;
    if (syn != 0) { meggitt(s, syn, cv); s.bit_err += NPAY; }          // (the block still counts as failed)
    s.ber_num = s.bit_err; s.ber_den = s.bits_done;
    if (s.bits_done >= BER_RESET) { s.bit_err = 0; s.bits_done = 0; if (cv) cv->ber_wrap++; }
    return syn == 0;
}
FMX_HD inline RdsSyncRes push(RdsSync &s, bool bit, RdsSyncCover *cv) {                  // :215-336
    s.stream = (s.stream << 1) | (bit ? 1u : 0u);
    if (s.synced) {
        if (++s.bits_in_blk < NBLK) return RDS_BUFFERING;
        s.bits_in_blk = 0;
        if (!decode_block(s, s.cur, s.stream, cv)) { s.n_crc_err++; return RDS_NO_CRC; }
        set_blk(s, s.cur, (uint16_t)(s.stream >> NCRC));
        const RdsSyncRes r = s.cur == 3 ? RDS_COMPLETE : RDS_BUFFERING;
        s.cur = (s.cur + 1) & 3;
        return r;
    }
    if (s.cur == 0) {                                                  // slide bit by bit until a clean block A appears
        if (syndrome(s.stream & 0x3FFFFFF, offset_word(0, type_b(s))) != 0) { if (cv) cv->waiting_a++; return RDS_WAITING_A; }
        s.blk[0] = (uint16_t)(s.stream >> NCRC);
        s.bits_in_blk = 0; s.cur = 1;
        if (cv) cv->found_a++;
        return RDS_BUFFERING;
    }
    if (s.bits_in_blk < NBLK - 1) { s.bits_in_blk++; return RDS_BUFFERING; }
    s.bits_in_blk = 0;
    {
        const bool tb = type_b(s);
        if (cv && s.cur == 2 && tb) cv->type_b_offset++;
        if (syndrome(s.stream, offset_word(s.cur, tb)) != 0) { s.n_sync_err++; return RDS_NO_SYNC; }
    }
    set_blk(s, s.cur, (uint16_t)(s.stream >> NCRC));
    if (s.cur < 2) { s.cur++; return RDS_BUFFERING; }                  // SYNC_END_BLOCK = BLOCK_C
    s.synced = 1;
    const RdsSyncRes r = s.cur == 3 ? RDS_COMPLETE : RDS_BUFFERING;
    s.cur = (s.cur + 1) & 3;
    return r;
}
}  // namespace rdssync

// One sliced bit, as rdsDecoder::processBit reacts to the synchroniser (rds-decoder.cpp:104-131).  True when the bit completes a group: its four blocks,
// as rdsGroupDecoder::decode receives them, are in out[0 .. 3], and the synchroniser's own copies are zeroed.
FMX_HD inline bool rds_sync_bit(RdsSync &s, bool bit, uint16_t out[4], RdsSyncCover *cv = nullptr) {
    switch (rdssync::push(s, bit, cv)) {
    case RDS_WAITING_A: case RDS_BUFFERING: return false;
    case RDS_NO_SYNC: if (cv) cv->no_sync++; rdssync::resync(s); return false;
    case RDS_NO_CRC: if (cv) cv->no_crc++; rdssync::resync(s); return false;
    case RDS_COMPLETE: break;
    }
    if (cv) cv->complete++;
    for (int i = 0; i < 4; i++) { out[i] = s.blk[i]; s.blk[i] = 0; }
    return true;
}

// ---- what the kernel keeps per channel, and the record it leaves per complete group
constexpr int RDS_GROUP_RING = 64;          // records kept per channel: 5.6 s of groups at 11.4 per second
struct RdsSyncChan {
    RdsSync s;
    int32_t rd;                              // RdsState::nbits up to which the synchroniser has read the channel's bit ring
    int32_t pad;
    int64_t bits;                            // ... the same count since fmx_create in 64 bits (fmx_rds_bits' numbering)
    int64_t groups;                          // complete groups since fmx_create: the next record's number
};
// 16 bytes, one vector store: the group's number and the bit count one past its last bit by their low halves (the host widens them against
// RdsSyncChan::groups / ::bits, which a kept record lies at most 64 groups behind)
struct alignas(16) RdsGroupRec { uint16_t blk[4]; uint32_t index_lo, end_bit_lo; };
static_assert(sizeof(RdsGroupRec) == 16 && sizeof(RdsGroupRec) * RDS_GROUP_RING == 1024, "the group ring is 1 KB per channel");
static_assert(sizeof(RdsSyncChan) == 72, "RdsSyncChan is copied to the host as it is");

// A lane's work in rds_sync: the channel's bits from its read position up to the slicer's count `nbits` (RdsState::nbits), out of the bit ring
// `ring` (bits_cap bytes, a power of two and a multiple of 8, 8-byte aligned; one bit per byte, at count & (bits_cap - 1)), a record into
// grp[number & 63] for every complete group.  The ring is read eight bits per load.
// nbits never runs backwards: the slicers only count up, the RDS buffers are allocated once per handle and never re-initialised, and the
// difference is taken modulo 2^32, so the count's wrap (after 41 days of bits) passes unnoticed.  It never runs away either: rds_sync is
// launched behind every launch of a slicer, and a launch covers at most 32000 fm samples (198 bits) -- so there is no "start over" case here.
FMX_HD inline void rds_sync_walk(RdsSyncChan &c, const uint8_t *ring, uint32_t bits_cap, int32_t nbits, RdsGroupRec *grp, RdsSyncCover *cv = nullptr) {
    const uint32_t pending = (uint32_t)nbits - (uint32_t)c.rd;
    const uint64_t *ring8 = reinterpret_cast<const uint64_t *>(ring);
    uint32_t pos = (uint32_t)c.rd;
    uint64_t w = 0;
    for (uint32_t i = 0; i < pending; i++, pos++) {
        const uint32_t slot = pos & (bits_cap - 1);
        if (i == 0 || (slot & 7) == 0) w = ring8[slot >> 3];
        const bool bit = ((w >> (8 * (slot & 7))) & 0xFF) != 0;
        uint16_t b[4];
        c.bits++;
        if (rds_sync_bit(c.s, bit, b, cv)) {
            RdsGroupRec r;
            r.blk[0] = b[0]; r.blk[1] = b[1]; r.blk[2] = b[2]; r.blk[3] = b[3];
            r.index_lo = (uint32_t)c.groups; r.end_bit_lo = (uint32_t)c.bits;
            grp[c.groups & (RDS_GROUP_RING - 1)] = r;
            c.groups++;
        }
    }
    c.rd = nbits;
}
// the record of group `index` (c.groups - 64 <= index < c.groups) out of a channel's ring, widened
inline bool rds_group_read(const RdsSyncChan &c, const RdsGroupRec *grp, int64_t index, int64_t *end_bit, uint16_t blk[4]) {
    const RdsGroupRec &r = grp[index & (RDS_GROUP_RING - 1)];
    if (r.index_lo != (uint32_t)index) return false;                 // (not the record the counter promises: never, short of a torn copy)
    *end_bit = c.bits - (int64_t)((uint32_t)c.bits - r.end_bit_lo);
    for (int i = 0; i < 4; i++) blk[i] = r.blk[i];
    return true;
}

}  // namespace fmx

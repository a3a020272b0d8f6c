// Host check of sdr-j-fm_amd/csrc/fmx_rdssync.h (run by tests/test_rdssync_cpu.py): one query per line on stdin, one JSON object per query on stdout.
//   syndrome                 -> rdssync::syndrome against the reference's 26-step loop (RdsGroupDecoderHost::syndrome's text, repeated here) on all
//                               2^26 words, for each of the five offset words: {"checked": n, "mismatches": m}
//   stream name 0101...      -> the bit string through (a) RdsGroupDecoderHost::push_bit, the yardstick, and (b) rds_sync_bit + push_group +
//                               set_sync_status: every field of info () compared after every bit.  Then the same bits through rds_sync_walk -- the
//                               kernel's loop over a bit ring of 8192 bytes -- cut into chunks of 1, 25, 26, 27, 119 bits and of 0, 1, 25, 26, 27, 119
//                               bits in turn: the state behind every run and the records it left (number, end bit, blocks) against (b)'s.
//                               -> {"bits": n, "field_mismatches": m, "first": "...", "groups": g, "chunk_mismatches": m, the paths taken, the final info}
#include "../sdr-j-fm_amd/csrc/fmx_rdsgroups.h"
#include "../sdr-j-fm_amd/csrc/fmx_rdssync.h"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>
using namespace fmx;

static uint32_t loop26(uint32_t bits, uint32_t off) {                 // fmx_rdsgroups.h syndrome (), rds-blocksynchronizer.cpp:126-142
    const uint32_t block = bits ^ off;
    uint32_t reg = 0;
    for (int k = 25; k >= 0; k--) {
        const uint32_t msb = reg & (1u << 9);
        reg <<= 1;
        if (msb) reg ^= 0x5B9;
        if ((block >> k) & 1u) reg ^= 0x31B;
    }
    return reg;
}

// the first field of fmx_rds_info in which a and b differ (null: none), field by field: the struct has padding.  The float by its bit pattern; the two
// character arrays as the NUL-terminated strings they are (the decoder does not define radio_text behind its terminator)
static const char *diff(const fmx_rds_info &a, const fmx_rds_info &b) {
#define F(x) if (std::memcmp(&a.x, &b.x, sizeof(a.x)) != 0) return #x;
#define S(x) if (std::strncmp(a.x, b.x, sizeof(a.x)) != 0 || std::memchr(a.x, 0, sizeof(a.x)) == nullptr) return #x;
    F(synchronized) F(pi_code) F(pty_code) F(last_group_type) F(groups_decoded) F(crc_errors) F(sync_errors) F(bit_error_rate)
    S(station_label) S(radio_text) F(af1_khz) F(af2_khz) F(music_speech) F(di_code) F(radio_text_ucs2) F(radio_text_ucs2_len)
#undef F
#undef S
    return nullptr;
}
static RdsSyncStatus status_of(const RdsSync &s) { return RdsSyncStatus{s.synced, s.n_crc_err, s.n_sync_err, s.ber_num, s.ber_den}; }

struct Rec { int64_t index, end_bit; uint16_t blk[4]; };
static bool same(const Rec &a, const Rec &b) { return a.index == b.index && a.end_bit == b.end_bit && std::memcmp(a.blk, b.blk, 8) == 0; }

constexpr uint32_t CAP = 8192;                                        // RDS_BITS_CAP (fmx_internal.h)
// the bits through rds_sync_walk in chunks (sizes in turn), the slicer's side played by the loop that fills the ring; the records are read out
// behind every chunk as fmx_rds_groups reads them.  start: the slicer's count in front of the first bit (the ring's and the count's wraps)
static int run_chunked(const std::vector<uint8_t> &bits, const std::vector<int> &sizes, uint32_t start, const RdsSync &want, const std::vector<Rec> &recs) {
    alignas(8) static uint8_t ring[CAP];
    static RdsGroupRec grp[RDS_GROUP_RING];
    std::memset(ring, 0, sizeof(ring)); std::memset(grp, 0, sizeof(grp));
    RdsSyncChan c; std::memset(&c, 0, sizeof(c));
    c.rd = (int32_t)start;
    uint32_t nbits = start;
    int64_t read = 0; size_t k = 0, pos = 0; int bad = 0;
    std::vector<Rec> got;
    while (pos < bits.size() || k % sizes.size() != 0) {
        size_t take = (size_t)sizes[k++ % sizes.size()];
        if (take > bits.size() - pos) take = bits.size() - pos;
        for (size_t i = 0; i < take; i++) ring[nbits++ & (CAP - 1)] = bits[pos++];
        rds_sync_walk(c, ring, CAP, (int32_t)nbits, grp);
        if (c.groups - read > RDS_GROUP_RING) { bad++; read = c.groups - RDS_GROUP_RING; }      // (the chunks are far too short for that)
        for (; read < c.groups; read++) {
            Rec r; r.index = read;
            if (!rds_group_read(c, grp, read, &r.end_bit, r.blk)) bad++;
            got.push_back(r);
        }
    }
    if (std::memcmp(&c.s, &want, sizeof(RdsSync)) != 0) bad++;
    if (c.bits != (int64_t)bits.size() || c.groups != (int64_t)recs.size() || c.rd != (int32_t)nbits) bad++;
    if (got.size() != recs.size()) bad++;
    else for (size_t i = 0; i < got.size(); i++) if (!same(got[i], recs[i])) bad++;
    return bad;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string q;
        in >> q;
        if (q == "syndrome") {
            const uint32_t offs[5] = {0xFC, 0x198, 0x168, 0x350, 0x1B4};
            unsigned long long checked = 0, bad = 0;
            {   // (every word, on a few threads: 3.4e8 runs of the 26-step loop)
                constexpr int NT = 8;
                unsigned long long tbad[NT] = {};
                std::vector<std::thread> th;
                for (int t = 0; t < NT; t++)
                    th.emplace_back([&, t]() {
                        const uint32_t w0 = (uint32_t)t * ((1u << 26) / NT), w1 = w0 + (1u << 26) / NT;
                        for (uint32_t off : offs)
                            for (uint32_t w = w0; w < w1; w++) if (rdssync::syndrome(w, off) != loop26(w, off)) tbad[t]++;
                    });
                for (auto &x : th) x.join();
                for (int t = 0; t < NT; t++) bad += tbad[t];
                checked += 5ull << 26;
            }
            // the synchronised path hands the 32-bit register over unmasked: bits 26 .. 31 must not count
            for (uint32_t w = 0; w < (1u << 20); w++) {
                const uint32_t v = w * 2654435761u;
                checked++; if (rdssync::syndrome(v, 0x198) != loop26(v, 0x198) || rdssync::syndrome(v, 0x198) != rdssync::syndrome(v & 0x3FFFFFF, 0x198)) bad++;
            }
            printf("{\"checked\": %llu, \"mismatches\": %llu}\n", checked, bad);
        } else if (q == "stream") {
            std::string name, text;
            in >> name >> text;
            std::vector<uint8_t> bits(text.size());
            for (size_t i = 0; i < text.size(); i++) bits[i] = text[i] == '1';
            RdsGroupDecoderHost ref, grpdec;
            RdsSync s; std::memset(&s, 0, sizeof(s));
            RdsSyncCover cv; std::memset(&cv, 0, sizeof(cv));
            std::vector<Rec> recs;
            unsigned long long bad = 0; std::string first;
            {   // nothing pushed yet: the overlay of an all-zero synchroniser is the fresh picture
                grpdec.set_sync_status(status_of(s));
                if (const char *f = diff(ref.info(), grpdec.info())) { bad++; first = std::string("fresh:") + f; }
            }
            for (size_t i = 0; i < bits.size(); i++) {
                ref.push_bit(bits[i] != 0);
                uint16_t b[4];
                if (rds_sync_bit(s, bits[i] != 0, b, &cv)) {
                    grpdec.push_group(b);
                    Rec r; r.index = (int64_t)recs.size(); r.end_bit = (int64_t)i + 1; std::memcpy(r.blk, b, 8);
                    recs.push_back(r);
                }
                grpdec.set_sync_status(status_of(s));
                if (const char *f = diff(ref.info(), grpdec.info())) { if (!bad) first = std::to_string(i) + ":" + f; bad++; }
            }
            int cbad = 0;
            for (int c : {1, 25, 26, 27, 119}) cbad += run_chunked(bits, {c}, 0, s, recs);
            cbad += run_chunked(bits, {0, 1, 25, 26, 27, 119}, 0, s, recs);
            cbad += run_chunked(bits, {119, 0, 27}, CAP - 61, s, recs);                 // the ring's wrap inside a chunk
            cbad += run_chunked(bits, {0, 1, 25, 26, 27, 119}, 0xFFFFFFFFu - 1000, s, recs);   // ... and the 32-bit count's
            cbad += run_chunked(bits, {26, 119}, 0x7FFFFFFFu - 500, s, recs);
            const fmx_rds_info &I = ref.info();
            unsigned ber; std::memcpy(&ber, &I.bit_error_rate, 4);
            printf("{\"name\": \"%s\", \"bits\": %zu, \"field_mismatches\": %llu, \"first\": \"%s\", \"groups\": %zu, \"chunk_mismatches\": %d, "
                   "\"waiting_a\": %llu, \"found_a\": %llu, \"no_sync\": %llu, \"no_crc\": %llu, \"complete\": %llu, \"meggitt_run\": %llu, \"meggitt_flip\": %llu, "
                   "\"ber_wrap\": %llu, \"type_b_offset\": %llu, "
                   "\"synchronized\": %d, \"pi_code\": %d, \"pty_code\": %d, \"last_group_type\": %d, \"groups_decoded\": %d, \"crc_errors\": %d, \"sync_errors\": %d, \"ber_bits\": %u}\n",
                   name.c_str(), bits.size(), bad, first.c_str(), recs.size(), cbad,
                   (unsigned long long)cv.waiting_a, (unsigned long long)cv.found_a, (unsigned long long)cv.no_sync, (unsigned long long)cv.no_crc, (unsigned long long)cv.complete,
                   (unsigned long long)cv.meggitt_run, (unsigned long long)cv.meggitt_flip, (unsigned long long)cv.ber_wrap, (unsigned long long)cv.type_b_offset,
                   I.synchronized, I.pi_code, I.pty_code, I.last_group_type, I.groups_decoded, I.crc_errors, I.sync_errors, ber);
        } else {
            printf("{\"error\": \"unknown query\"}\n");
        }
        fflush(stdout);
    }
    return 0;
}

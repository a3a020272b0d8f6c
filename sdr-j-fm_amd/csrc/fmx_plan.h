// fmx_plan.h -- how one fmx_process_* call becomes launches: the pieces it is made in, stage A's split in time, stage B's form and its
// channel groups.  Plain C++ (no HIP): fmx_api.hip and fmx_stageb.hip decide with these functions, tests/call_plan_check.cpp checks them on the CPU.
#pragma once
#include <cstdint>
#include <vector>

namespace fmx {

constexpr int DECIM = 12;                 // inputRate / fmRate (2304000 / 192000): stage A's decimation
constexpr int RDS_BLK = 32000;            // overlap-add block of the two 32768-pt filters of the RDS path (fft-filters.cpp:34)
constexpr int STAGEB_SEG = 1536;          // fm samples per segment of stage B (fmx_stageb.hip FB_W)
constexpr int STAGEB_WG_PER_CU = 3;       // workgroups per CU of stage B as one kernel (its launch bounds; the two kernels run 4)

constexpr int PIPE_ROWS_AUTO = 3072;      // fm samples per piece of an overlapping call where pllC runs (two of stage B's segments; measured at 4096 channels:
                                          // 2048 / 3072 / 4608 / 6400 fm samples per piece give 6.37 / 6.18 / 6.46 / 6.79 ms per step, the call made whole 8.24)
constexpr int PIPE_ROWS_AUTO_PLL = 4608;  // ... where pllC runs for the PLL decoder only (round 6: its chain is 66 issue slots per sample instead of 80 and the launches' own cost counts more:
                                          // pieces of 3072 x 6 / 4608 x 4 / 5376 x 3 + 3072 / 4608 x 3 + 3072 + 2304 / 4608 x 3 + 3840 + 1536 give 5.29 / 5.21 / 4.92 / 4.82 / 4.83 ms per step)
constexpr int PIPE_ROWS_AUTO_AM = 3840;   // ... where the AM decoder runs (its chain is longer per sample): 3072 x 6 / 3840 x 4 + 2304 + 1536 / 3840 x 4 + 1536 + 2304 / 3072 x 5 + 2304 + 1536 give 6.0-6.1 / 5.72 / 5.93 / 5.77 ms per step
constexpr int PIPE_ROWS_AUTO_SQ = 4608;   // ... where only squelches do (noise squelch 6.61 / 5.73 / 5.46 / 5.54 against 5.90 whole, level squelch 5.43 / 4.73 / 4.59 / 4.72 against 5.23)
constexpr int PIPE_MIN_CHANNELS = 1024;   // automatic: batches that fill the chip
constexpr int TAIL_MIN_CHANNELS = 128;    // the second stage-B / C channel group: at least this many channels

// rows of one half of the pre-pass work arrays (work_nj rows in all): an overlapping call's pieces alternate between the two halves
inline int64_t prepass_half(int64_t work_nj) { return (work_nj / 2) & ~(int64_t)15; }

// ---- the pieces of a call.  The caller has checked the call: n is in [1, max_block], the format is valid.
struct CallShape {
    int64_t n; int decim;                   // input samples per stream; input samples per fm sample at the handle's rate (12, 6 or 1)
    bool any_rds;                           // some channel decodes RDS
    bool prepass, pllc, am;                 // some channel runs the demodulator pre-pass (fmx_demod.hip): the PLL / AM decoder or a squelch; pllC (either decoder); the AM decoder
    int call_pieces, channels;              // FMX_P_CALL_PIECES (-1 automatic, 0 never, else fm samples per piece); the handle's channels
    bool ola_mode, conv2, prepass_arrays;   // the block machines run (fmx_ola.hip); the second converter does; the pre-pass work arrays are allocated
    int64_t half;                           // prepass_half
};
// WHOLE: one launch sequence on the caller's stream.  RDS_PIECES: pieces of (RDS_BLK - 1) * decim one after the other on the caller's stream (a launch
// sequence covers at most one RDS block boundary per channel, whatever the call's phase in the fm-rate grid).  OVERLAPPED: pre-pass pieces on the handle's
// three streams (fmx_api.hip run_call).
enum class CallKind { WHOLE, RDS_PIECES, OVERLAPPED };
struct CallPlan { CallKind kind; std::vector<int64_t> lens; };   // lens: input samples per stream of each piece, in order; they sum to n

inline CallPlan plan_call(const CallShape &c) {
    const int64_t n = c.n, d = c.decim;
    if (c.any_rds) {
        const int64_t piece = (int64_t)(RDS_BLK - 1) * d;
        if (n <= piece) return {CallKind::WHOLE, {n}};
        CallPlan p{CallKind::RDS_PIECES, {}};
        for (int64_t pos = 0; pos < n; pos += piece) p.lens.push_back(n - pos < piece ? n - pos : piece);
        return p;
    }
    const int want = c.call_pieces;
    const int64_t auto_rows = c.am ? PIPE_ROWS_AUTO_AM : PIPE_ROWS_AUTO_PLL;
    // (a call too short for two of pllC's longer pieces is cut into the shorter ones)
    const int64_t rows = want > 0 ? ((want + 15) / 16) * 16 : (c.pllc ? (n < 2 * auto_rows * d ? PIPE_ROWS_AUTO : auto_rows) : PIPE_ROWS_AUTO_SQ);
    const int64_t piece = rows * d;
    // (only these batches.  Measured: the headline's batch -- no pre-pass; stage A bound by HBM, stage B by instruction issue -- made in 13 / 6 / 4 / 3 overlapping
    // pieces takes 4.97 / 3.89 / 3.60 / 3.60 ms per step against 3.46 whole: stage B's workgroups fill the register files, the stages do not share a CU)
    if (!(c.prepass && c.prepass_arrays && want != 0 && !c.ola_mode && !c.conv2 && (want > 0 || c.channels >= PIPE_MIN_CHANNELS) && rows + 2 <= c.half && n >= 2 * piece))
        return {CallKind::WHOLE, {n}};
    CallPlan p{CallKind::OVERLAPPED, {}};
    if (want < 0 && c.pllc) {
        // pllC's chain: whole pieces, then the rest (between one and two pieces) as a multiple of half a segment of stage B's and a SHORT last piece of one segment
        // to one and a half.  What the call pays beyond the chain of the lone waves is its last piece's stages B and C (the chain has ended)
        // (19200 fm samples: 4608 4608 4608 3840 1536; AM decoder: 3840 x 4, 2304, 1536)
        const int64_t seg = (int64_t)STAGEB_SEG * d;
        int64_t pos = 0;
        while (n - pos >= 2 * piece) { p.lens.push_back(piece); pos += piece; }
        const int64_t R = n - pos;
        int64_t a = ((R - seg) / (seg / 2)) * (seg / 2);
        if (a > piece) a = piece;
        if (a >= seg) { p.lens.push_back(a); p.lens.push_back(R - a); } else p.lens.push_back(R);
        bool fits = true;
        for (int64_t l : p.lens) fits = fits && l > 0 && l / d + 2 <= c.half;
        if (fits) return p;
        p.lens.clear();
    }
    // equal pieces; a last piece shorter than half a piece rides with the one before it (the arrays' halves hold a piece and a half)
    for (int64_t pos = 0; pos < n;) {
        int64_t len = (n - pos < piece) ? n - pos : piece;
        if (n - pos - len > 0 && n - pos - len < piece / 2 && (rows * 3) / 2 + 2 <= c.half) len = n - pos;
        p.lens.push_back(len); pos += len;
    }
    return p;
}

// ---- stage A split in time.  Stage A runs one workgroup per channel, two per CU: a handle with fewer channels than that leaves compute units idle while each
// workgroup walks its channel's tiles one after the other.  Such a call splits every channel in time (fmx_front.hip, CallGeom::parts): as many parts as fill the
// chip, none shorter than FRONT_MIN_PART_TILES tiles (every later part computes one tile twice).  The results are the same bit for bit.
constexpr int FRONT_MIN_PART_TILES = 6, FRONT_MAX_PARTS = 32, FRONT_TILE = 128 * DECIM;
struct FrontParts { int parts, part_tiles; };   // parts <= 1: one workgroup per channel
// g0, n: the call's first input sample and its length; want: FMX_P_FRONT_PARTS
inline FrontParts plan_front_parts(int64_t g0, int64_t n, int want, int twins, int channels, int n_cus) {
    const FrontParts one{1, 0};
    if (twins != 1 || want == 1) return one;
    const int64_t r0 = g0 % DECIM;
    const int NT = (int)((r0 + n - 1) / FRONT_TILE) + 1;
    int parts = want > 1 ? want : (2 * n_cus) / channels;
    if (want <= 1 && parts > NT / FRONT_MIN_PART_TILES) parts = NT / FRONT_MIN_PART_TILES;
    if (parts > FRONT_MAX_PARTS) parts = FRONT_MAX_PARTS;
    if (parts > NT / 2) parts = NT / 2;              // (forced: at least two tiles per part)
    if (parts < 2) return one;
    const int pt = (NT + parts - 1) / parts;
    parts = (NT + pt - 1) / pt;
    if (parts < 2) return one;
    return {parts, pt};
}

// ---- stage B as one kernel or two.  Per channel both forms cost the same (measured, 256 ... 4096 channels: the kernel is bound by instruction issue, a fourth
// workgroup per CU adds nothing), what differs is the tail: the whole kernel runs wg_per_cu workgroups per CU, its halves 4, and a batch that does not fill
// the last round of either leaves CUs idle.  The form whose rounds waste less wins; a tie goes to the single launch.  (4096 channels on 256 CUs: 5.33 rounds
// of 768 against 4 of 1024 -- 2.05 against 1.91 ms.)  A batch that keeps no scope taps and decodes no RDS (rows_on == 0): the whole kernel leaves the rows
// unwritten -- 0.63 GB per call at 4096 channels, and writes are the expensive direction on this GPU -- and is then the faster form where the halves were:
// 1.60 against 1.69 ms.  form: FMX_P_STAGEB_FORM (1 one kernel, 2 two, 0 this arithmetic).
inline bool stageb_two_kernels(int channels, int n_cus, bool rows_on, int form, int wg_per_cu) {
    if (form) return form == 2;
    const int cus = n_cus > 0 ? n_cus : 256;
    const long whole = (long)((channels + wg_per_cu * cus - 1) / (wg_per_cu * cus)) * wg_per_cu * 100;
    const long halves = (long)((channels + 4 * cus - 1) / (4 * cus)) * 4 * 102;          // (two launches, the hand-over through HBM: 2 %)
    return rows_on && halves < whole;
}

// ---- stages B and C of a plain batch as two channel groups: the channels of the second group (0: one group).  Stage B is bound by instruction issue and
// leaves its last round of workgroups partly filled (4096 channels are 5.33 rounds of 768); stage C moves the d ring and the PCM.  With the second group's
// stage B finished while the first group's still runs, its stage C fills what stage B leaves free: 3.48 -> 3.32 ms per step at 4096 channels.
// (the first group: 2304 of 4096 channels on 256 CUs -- three whole rounds.  Measured there, second group of 256 / 512 / 1024 / 1792 / 2048 / 3072 channels:
// 3.47 / 3.45 / 3.35 / 3.32 / 3.39 / 3.43 ms per step against 3.47-3.55 with one group.)  Other counts, one group -> two, ms per step: 3840 (2304 + 1536)
// 3.20 -> 3.12, 3000 (2304 + 696) 2.51 -> 2.43 (1536 + 1464: 2.51), 2048 (1536 + 512) 1.68 -> 1.63, 1536 (768 + 768) 1.30 -> 1.27, 1024 (768 + 256)
// 0.915 -> 0.910: the first group is two thirds of the rounds, in whole rounds.
inline int second_group_channels(int channels, int n_cus) {
    const int slots = STAGEB_WG_PER_CU * (n_cus > 0 ? n_cus : 256);
    if (channels <= slots) return 0;
    int first_rounds = (int)(0.65 * (double)channels / (double)slots + 0.5);
    if (first_rounds < 1) first_rounds = 1;
    const int tail = channels - first_rounds * slots;
    return tail < TAIL_MIN_CHANNELS ? 0 : tail;     // (a second group of a few dozen channels is three launches for nothing)
}

}  // namespace fmx

// fmx_spec.h -- the spectrum meter (include/fmx.h fmx_spectrum_*; the reference hands these samples to its HF scope, fm-processor.cpp:417-421):
// a windowed 4096-point power spectrum of a handle's own streams at inputRate, mean and max-hold per record, and the host's figures over a record.  The
// window, the twiddles and the transform are the band survey's (fmx_survey.h, included unchanged).  What is the meter's own is here, as pure functions --
// fmx_api.hip decides with them, fmx_spec.hip runs them, tests/spec_check.cpp drives them on the CPU:
//   the grid: g counts a stream's input samples since fmx_create; with S = `every` and B = blocks per record, block b is the samples
//     [4096 S b, 4096 S b + 4096), record r the blocks [r B, r B + B).  The other 4096 (S - 1) samples of a period are not read;
//   piece (): what a piece [g0, g0 + n) of a call means on that grid -- the blocks it completes, what the first of them draws on the carry, what is carried
//     behind it, the phase in the record, the records completed;
//   chunk_blocks (), group_streams (): how a piece's (stream, block) pairs are cut so that the scratch of block powers stays within SCRATCH_BYTES;
//   fold (): one bin of one stream over a chunk's blocks in block order -- one add and one max per block, both skipped in front of the stream's first block,
//     the scaled store of both at a record's last block;
//   first_block (), delivered (): the switch's rules;
//   figures (): occupied bandwidth, x-dB bandwidth, centroid, adjacent channels and the mask margin of one record, all sums in f64, membership of a bin
//     in a window decided in integers as survey::find decides it.
#pragma once
#include "fmx_survey.h"

namespace fmx {
namespace spec {

constexpr int N = survey::N, NT = survey::NT, PER = survey::PER;
constexpr int RING = 4;                                   // records kept per metered stream
constexpr int MAX_B = 4096, MAX_S = 4096;                 // blocks per record, every
constexpr int64_t SCRATCH_BYTES = (int64_t)256 << 20;     // the cap of the block powers' scratch array
constexpr int64_t SCRATCH_BLOCKS = SCRATCH_BYTES / ((int64_t)N * (int64_t)sizeof(float));      // 16 384 blocks of 4096 f32

// ---- the grid ------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int64_t period(int32_t S) { return (int64_t)N * S; }
// samples of a block that lie in front of position g: 0 where g is a block's first sample or lies in a period's unread part
__host__ __device__ __forceinline__ int32_t in_progress(int64_t g, int32_t S) { const int64_t o = g % period(S); return o < N ? (int32_t)o : 0; }
// one past the last sample of record r (fmx_spectrum_record::end_sample)
__host__ __device__ __forceinline__ int64_t record_end(int64_t r, int32_t B, int32_t S) { return period(S) * ((r + 1) * (int64_t)B - 1) + N; }

// the first block of a stream switched on by a piece that begins at g: the first that begins at or behind g
__host__ __device__ __forceinline__ int64_t first_block(int64_t g, int32_t S) { return (g + period(S) - 1) / period(S); }
// record r is delivered when every one of its blocks was taken: its first block is at or behind the stream's first
__host__ __device__ __forceinline__ bool delivered(int64_t r, int32_t B, int64_t first) { return r * (int64_t)B >= first; }

struct Piece {
    int64_t b0;              // the first block that can complete in the piece: the one in progress at g0, else the next to begin
    int64_t blocks;          // blocks the piece completes: b0 .. b0 + blocks - 1
    int32_t fill;            // samples of block b0 carried in front of the piece (0 .. N - 1)
    int32_t fill_after;      // samples carried behind it (0 .. N - 1)
    int32_t append;          // 1: the piece ends inside the block it began in -- its n samples go behind the carry's `fill`
    int32_t phase;           // b0 mod B
    int64_t carry_src;       // append == 0 and fill_after > 0: the piece's sample that becomes carry [0]
    int64_t record0;         // b0 div B: the record block b0 belongs to
    int64_t records;         // records the piece completes: record0 .. record0 + records - 1
};
__host__ __device__ inline Piece piece(int64_t g0, int64_t n, int32_t S, int32_t B) {
    Piece p;
    const int64_t P = period(S), g1 = g0 + n;
    p.fill = in_progress(g0, S);
    p.b0 = g0 % P < N ? g0 / P : g0 / P + 1;
    const int64_t b_end = g1 >= N ? (g1 - N) / P + 1 : 0;          // blocks b with P b + N <= g1
    p.blocks = b_end > p.b0 ? b_end - p.b0 : 0;
    p.fill_after = in_progress(g1, S);
    const int64_t start = g1 / P * P;                              // where the block in progress at g1 began
    p.append = (p.fill_after > 0 && start < g0) ? 1 : 0;
    p.carry_src = (p.fill_after > 0 && !p.append) ? start - g0 : 0;
    p.phase = (int32_t)(p.b0 % B);
    p.record0 = p.b0 / B;
    p.records = (p.b0 + p.blocks) / B - p.record0;
    return p;
}
// Where sample i of block b lies: >= 0: index into the piece's samples; < 0: carry [i] (block b0 alone, i < fill)
__host__ __device__ __forceinline__ int64_t source_index(int64_t b, int i, int64_t g0, int32_t S) { return period(S) * b + i - g0; }

// ---- bounded scratch: `streams` metered streams go in groups of at most group_streams, a group's blocks in chunks of chunk_blocks ----------------
__host__ __device__ __forceinline__ int64_t group_streams(int64_t streams, int64_t scratch_blocks) { return streams < scratch_blocks ? streams : scratch_blocks; }
__host__ __device__ __forceinline__ int64_t chunk_blocks(int64_t streams_in_group, int64_t scratch_blocks) {
    const int64_t c = scratch_blocks / (streams_in_group > 0 ? streams_in_group : 1);
    return c > 0 ? c : 1;
}
// the scratch a handle allocates: enough for `streams` streams of `blocks` blocks each, never above the cap, never below one block
inline int64_t scratch_blocks_for(int64_t streams, int64_t blocks) {
    const int64_t want = streams * (blocks > 0 ? blocks : 1);
    return want < SCRATCH_BLOCKS ? (want > 0 ? want : 1) : SCRATCH_BLOCKS;
}

// The launches of a piece that completes `blocks` blocks for `streams` metered streams: visit (first stream of the group, streams in it, blocks of the
// piece in front of the chunk, blocks in the chunk, write_carry).  Every (stream, block) is visited once, a stream's blocks in order; no visit holds
// more than scratch_blocks (stream, block) pairs; the carry is written by the last visit of every group (`carries`: the piece carries samples behind it),
// which is a visit of no block where the piece completes none.
template <class F> inline void launches(int64_t streams, int64_t scratch_blocks, int64_t blocks, bool carries, F &&visit) {
    const int64_t group = group_streams(streams, scratch_blocks);
    for (int64_t j0 = 0; j0 < streams; j0 += group) {
        const int64_t gn = group < streams - j0 ? group : streams - j0, chunk = chunk_blocks(gn, scratch_blocks);
        int64_t done = 0;
        do {
            const int64_t nb = chunk < blocks - done ? chunk : blocks - done;
            const bool last = done + nb == blocks;
            if (nb > 0 || (carries && last)) visit(j0, gn, done, nb, carries && last);
            done += nb;
        } while (done < blocks);
    }
}

// ---- the fold: one bin of one stream over nb blocks from block b on, in block order; p [j * pstride] is block b + j's power -----------------------
// `phase` = b mod B.  A record's first block clears sum and maximum; at its last block both are scaled and stored to mean [slot * 2 N] and
// peak [slot * 2 N] (slot = record mod RING) if the record is delivered.
__host__ __device__ __forceinline__ void fold(float &sum, float &mx, const float *p, int64_t pstride, int64_t b, int64_t nb, int64_t first, int phase, int B,
                                              float c, float c1, float *mean, float *peak) {
    int64_t r = b / B;
    for (int64_t j = 0; j < nb; j++) {
        if (phase == 0) { sum = 0.f; mx = 0.f; }
        if (b + j >= first) { const float v = p[j * pstride]; sum += v; mx = fmaxf(mx, v); }
        if (++phase == B) {
            if (delivered(r, B, first)) { const size_t at = (size_t)(r & (RING - 1)) * 2 * N; mean[at] = sum * c; peak[at] = mx * c1; }
            phase = 0; r++;
        }
    }
}

// ---- the figures (include/fmx.h fmx_spectrum_figures) ---------------------------------------------------------------------------------------------
inline int figures(const fmx_spectrum_find *cfg, const float *mean, const float *peak, fmx_spectrum_figs *out, const char **why) {
    *why = "";
    if (!cfg || !mean || !out) { *why = "null argument"; return FMX_E_INVALID; }
    if (cfg->struct_size != (int32_t)sizeof(fmx_spectrum_find)) { *why = "fmx_spectrum_find.struct_size mismatch"; return FMX_E_INVALID; }
    if (cfg->rate_hz < 1000 || cfg->rate_hz > 100000000) { *why = "rate_hz must be in [1000, 100000000]"; return FMX_E_INVALID; }
    const int64_t R = cfg->rate_hz, C = cfg->centre_hz;
    if (2 * (C < 0 ? -C : C) > R) { *why = "|centre_hz| must be <= rate_hz / 2"; return FMX_E_INVALID; }
    if (cfg->raster_hz < 50000 || cfg->raster_hz > 1000000) { *why = "raster_hz must be in [50000, 1000000]"; return FMX_E_INVALID; }
    if (cfg->dc_guard_hz < 0 || cfg->dc_guard_hz > 99999) { *why = "dc_guard_hz must be in [0, 99999]"; return FMX_E_INVALID; }
    if (!(cfg->obw_fraction > 0.0 && cfg->obw_fraction < 1.0)) { *why = "obw_fraction must lie inside (0, 1)"; return FMX_E_INVALID; }
    if (!(cfg->x_db > 0.0) || !std::isfinite(cfg->x_db)) { *why = "x_db must be positive and finite"; return FMX_E_INVALID; }
    if (cfg->rbw_hz < 1 || cfg->rbw_hz > 200000) { *why = "rbw_hz must be in [1, 200000]"; return FMX_E_INVALID; }
    if (cfg->n_mask < 0 || cfg->n_mask == 1 || (cfg->n_mask > 0) != (cfg->mask != nullptr)) { *why = "mask / n_mask: none, or at least two break points"; return FMX_E_INVALID; }
    for (int i = 0; i < cfg->n_mask; i++) {
        const fmx_spectrum_mask_point &m = cfg->mask[i];
        if (!std::isfinite(m.offset_hz) || !std::isfinite(m.limit_db) || m.offset_hz < 0.0 || (i > 0 && !(m.offset_hz > cfg->mask[i - 1].offset_hz))) {
            *why = "mask: offsets must be finite, not negative and ascending, limits finite"; return FMX_E_INVALID;
        }
    }
    for (int k = 0; k < N; k++) {
        if (!(mean[k] >= 0.f) || !std::isfinite(mean[k])) { *why = "mean holds a negative or non-finite entry"; return FMX_E_INVALID; }
        if (peak && (!(peak[k] >= 0.f) || !std::isfinite(peak[k]))) { *why = "peak holds a negative or non-finite entry"; return FMX_E_INVALID; }
    }
    // bin kp (-N/2 .. N/2 - 1) lies at kp R / N Hz; every comparison with a frequency is made on kp R against the frequency times N
    auto at = [](int kp) { return kp < 0 ? kp + N : kp; };
    auto iabs = [](int64_t v) { return v < 0 ? -v : v; };
    auto usable = [&](int kp) { return iabs((int64_t)kp * R) >= (int64_t)cfg->dc_guard_hz * N; };
    auto within = [&](int kp, int64_t f, int64_t half) { return iabs((int64_t)kp * R - f * N) <= half * N; };
    auto window_sum = [&](const float *P, int64_t f, int64_t half) {
        double s = 0.0;
        for (int kp = -N / 2; kp < N / 2; kp++) if (usable(kp) && within(kp, f, half)) s += (double)P[at(kp)];
        return s;
    };
    auto db = [](double v) { return v > 0.0 ? 10.0 * std::log10(v) : -HUGE_VAL; };
    const double df = (double)R / N;
    auto off = [&](int kp) { return (double)kp * df - (double)C; };          // f - centre
    fmx_spectrum_figs F;
    F.channel_db = db(window_sum(mean, C, 100000));
    F.obw_hz = F.obw_lower_hz = F.obw_upper_hz = F.xdb_hz = F.centroid_hz = F.mask_margin_db = F.mask_worst_hz = -HUGE_VAL;
    // the span |f - centre| <= 150 kHz, ascending
    int lo = N, hi = -N;
    for (int kp = -N / 2; kp < N / 2; kp++) if (within(kp, C, 150000)) { if (kp < lo) lo = kp; if (kp > hi) hi = kp; }
    double total = 0.0, moment = 0.0, largest = 0.0;
    for (int kp = lo; kp <= hi; kp++) if (usable(kp)) {
        const double v = (double)mean[at(kp)];
        total += v; moment += v * off(kp); if (v > largest) largest = v;
    }
    if (total > 0.0) {
        F.centroid_hz = moment / total;
        const double tail = 0.5 * (1.0 - cfg->obw_fraction) * total;
        double cum = 0.0;
        for (int kp = lo; kp <= hi; kp++) {
            const double v = usable(kp) ? (double)mean[at(kp)] : 0.0;
            if (v > 0.0 && cum + v >= tail) { F.obw_lower_hz = off(kp) - 0.5 * df + df * (tail - cum) / v; break; }
            cum += v;
        }
        cum = 0.0;
        for (int kp = hi; kp >= lo; kp--) {
            const double v = usable(kp) ? (double)mean[at(kp)] : 0.0;
            if (v > 0.0 && cum + v >= tail) { F.obw_upper_hz = off(kp) + 0.5 * df - df * (tail - cum) / v; break; }
            cum += v;
        }
        F.obw_hz = F.obw_upper_hz - F.obw_lower_hz;
        const double thr = largest * std::pow(10.0, -cfg->x_db / 10.0);
        int first = N, last = -N;
        for (int kp = lo; kp <= hi; kp++) if (usable(kp) && (double)mean[at(kp)] > thr) { if (kp < first) first = kp; last = kp; }
        if (first <= last) F.xdb_hz = (double)(last - first) * df;
    }
    static const int offs[4] = {-2, -1, 1, 2};
    for (int i = 0; i < 4; i++) {
        const int64_t f = C + (int64_t)offs[i] * cfg->raster_hz;
        const double s = window_sum(mean, f, 100000);
        const bool inside = iabs(f) + 100000 <= R / 2 - 50000;
        F.adj_db[i] = (inside && s > 0.0 && F.channel_db > -HUGE_VAL) ? db(s) - F.channel_db : -HUGE_VAL;
    }
    if (peak && cfg->n_mask > 0 && F.channel_db > -HUGE_VAL) {
        const double m_lo = cfg->mask[0].offset_hz, m_hi = cfg->mask[cfg->n_mask - 1].offset_hz;
        bool any = false;
        double worst = 0.0, worst_hz = 0.0;
        for (int kp = -N / 2; kp < N / 2; kp++) {
            const double d = std::fabs(off(kp));
            if (!usable(kp) || d < m_lo || d > m_hi) continue;
            int seg = 0;
            while (seg + 2 < cfg->n_mask && d > cfg->mask[seg + 1].offset_hz) seg++;
            const fmx_spectrum_mask_point &a = cfg->mask[seg], &b = cfg->mask[seg + 1];
            const double limit = a.limit_db + (b.limit_db - a.limit_db) * (d - a.offset_hz) / (b.offset_hz - a.offset_hz);
            double s = 0.0;                                                // the bins within rbw_hz / 2 of this one: 2 |k' - k| R <= rbw N
            const int reach = (int)((int64_t)cfg->rbw_hz * N / (2 * R)) + 1;
            for (int q = std::max(-N / 2, kp - reach); q <= std::min(N / 2 - 1, kp + reach); q++) if (usable(q)&& 2 * iabs((int64_t)(q - kp) * R) <= (int64_t)cfg->rbw_hz * N) s += (double)peak[at(q)];
            if (!(s > 0.0)) continue;
            const double margin = limit - (db(s) - F.channel_db);
            if (!any || margin < worst) { any = true; worst = margin; worst_hz = off(kp); }
        }
        if (any) { F.mask_margin_db = worst; F.mask_worst_hz = worst_hz; }
    }
    *out = F;
    return FMX_OK;
}

}  // namespace spec
}  // namespace fmx

// fmx_rdsm.h -- the RDS meter's integers: the window grid of a channel's own 24 kS/s count, the lane / step a sample of a window goes to,
// the order of the six accumulators, the division that finishes a record, and what a piece of a call means for one channel (piece).  The grid is in the
// channel's own RDS-sample count, which stands still while its decoder is off: the modulation meter's meter_produce (fmx_meter.h) is restated here for a
// window of 2560 and a count that a piece may leave where it was.  Plain C++ (no HIP, no handle, no allocation): fmx_api.hip decides with these functions,
// fmx_rdsm.hip runs them, tests/rdsm_check.cpp checks them on the CPU.
#pragma once
#include <cstdint>

namespace fmx {
namespace rdsm {

constexpr int WINDOW = 2560;           // RDS samples per window: 106.7 ms at 24 000 S/s, about 127 bits; window w is [2560 w, 2560 (w + 1))
constexpr int LANES = 64;              // sample i of a window is accumulated by lane i mod 64 ...
constexpr int STEPS = WINDOW / LANES;  // ... as its step i div 64 (40 steps: a window is whole steps)
constexpr int RING = 64;               // records kept per channel (6.8 s)
constexpr int RING24 = 8192;           // the path's ring of 24 kS/s samples per channel (RDS24_RING of fmx_internal.h): what a piece may span
constexpr int QUANT = 6;               // accumulators per lane, in this order in a channel's state [QUANT][LANES]
enum { Q_MX = 0, Q_II = 1, Q_QQ = 2, Q_IQ = 3, Q_I = 4, Q_Q = 5 };
static_assert(STEPS * LANES == WINDOW && (RING & (RING - 1)) == 0 && RING24 % LANES == 0 && (RING24 & (RING24 - 1)) == 0,
              "the window is whole steps, the rings are powers of two, a step never straddles the ring's end");

#if defined(__HIPCC__)
#define FMX_RDSM_HD __host__ __device__
#else
#define FMX_RDSM_HD
#endif
FMX_RDSM_HD inline int64_t window_of(int64_t m) { return m / WINDOW; }
FMX_RDSM_HD inline int lane_of(int i) { return i % LANES; }
FMX_RDSM_HD inline int step_of(int i) { return i / LANES; }
// a record's mean of a combined sum over the window's 2560 samples
FMX_RDSM_HD inline float finish_mean(float s) { return s / 2560.0f; }

// One channel and one piece of a call.  In the piece the channel's decoder is on or off and its RDS meter is on or off; the piece's rds_mix_decim writes the
// channel's RDS samples [m0, m1) (m0 = (nc0 + row0) / 8 of the channel's own count; m1 = m0 where the piece is shorter than the next output is away).  The
// meter has been on in every piece that produced a sample since the one that began at on_from (-1: it has not) and has completed `produced` records.
//   - a piece that produces nothing for the channel (decoder off, or m1 = m0) changes nothing, whatever the meter's switch: a window may span it;
//   - a piece that produces samples with the meter off drops the window in progress (on_from = -1);
//   - a window counts only if the meter was on for all of it: accumulation begins at the first window boundary at or behind on_from.
//   job:      the channel accumulates in this piece: the samples [first, m1)
//   w0, nwin: the windows the piece completes, w0 .. w0 + nwin - 1; window w0 + k leaves its record in ring slot slot (k)
struct Piece {
    int64_t on_from, first, w0, nwin, produced, new_produced;
    bool    job;
    int64_t slot(int64_t k) const { return (produced + k) & (RING - 1); }
    int64_t end_sample(int64_t k) const { return (w0 + k + 1) * WINDOW; }
};
inline Piece piece(bool meter_on, bool decoder_on, int64_t on_from, int64_t m0, int64_t m1, int64_t produced) {
    Piece p{};
    p.on_from = on_from; p.first = m1; p.produced = p.new_produced = produced;
    if (!decoder_on || m1 <= m0) return p;
    if (!meter_on) { p.on_from = -1; return p; }
    if (p.on_from < 0) p.on_from = m0;
    const int64_t bound = (p.on_from + WINDOW - 1) / WINDOW * WINDOW;
    p.first = bound > m0 ? bound : m0;
    if (p.first >= m1) { p.first = m1; return p; }
    p.job = true;
    p.w0 = p.first / WINDOW;                       // the window `first` lies in: it is metered from its start
    p.nwin = m1 / WINDOW - p.w0;
    p.new_produced = produced + p.nwin;
    return p;
}
// the kernel reads the ring positions of [m0, m1) only, which the piece's own rds_mix_decim wrote: they are all there while the piece is no longer than the ring
FMX_RDSM_HD inline bool ring_holds(int64_t m0, int64_t m1) { return m1 - m0 <= RING24; }

}  // namespace rdsm
}  // namespace fmx

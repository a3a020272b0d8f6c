// fmx_rx.h -- the reception meter's integers.  The window grid, the lanes, the steps and what a piece of a call means for one metered
// channel are the modulation meter's (fmx_meter.h: WINDOW, LANES, lane_of, step_of, meter_produce), so that records of the two meters pair by `index`.
// What is the reception meter's own: the order of its six accumulators, and the look-back of one sample into stage A's fm-rate ring.  Plain C++ (no HIP,
// no handle, no allocation): fmx_api.hip decides with these functions, fmx_rx.hip runs them, tests/rx_check.cpp checks them on the CPU.
#pragma once
#include "fmx_meter.h"

namespace fmx {
namespace rx {

constexpr int RING = meter::RING;      // records kept per channel (3.2 s)
constexpr int QUANT = 6;               // accumulators per lane, in this order in a channel's state [QUANT][LANES]
enum { Q_MX = 0, Q_MN = 1, Q_S1 = 2, Q_S2 = 3, Q_CR = 4, Q_CI = 5 };

// fm sample j of a channel sits at ring position j - delay_fm (zero while that is negative).  The oldest position a piece of nj fm samples from J0 on reads
// is J0 - 1 - delay_fm: u [J0] = v [J0 - 1] comes from the ring and is never carried.
FMX_METER_HD inline int64_t oldest_position(int64_t J0, int64_t delay_fm) { return J0 - 1 - delay_fm; }
// The position behind the newest one stage A can have written when the piece's reader runs: the piece's own columns end below J1 + 1 (a column is complete
// with the input sample 12 q + off, off in 0 .. 11), a twin's columns are interleaved and shifted by at most one column of `twins`.
FMX_METER_HD inline int64_t newest_bound(int64_t J0, int64_t nj, int64_t twins) { return J0 + nj + 1 + 2 * twins; }
// The ring still holds v [J0 - 1] when the piece runs: no position stage A has written by then is the oldest one read, one turn of the ring later.
FMX_METER_HD inline bool ring_holds(int64_t ring, int64_t delay_fm, int64_t nj, int64_t twins) {
    return delay_fm >= 0 && nj > 0 && newest_bound(0, nj, twins) - oldest_position(0, delay_fm) <= ring;
}

}  // namespace rx
}  // namespace fmx

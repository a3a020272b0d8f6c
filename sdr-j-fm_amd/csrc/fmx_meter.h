// fmx_meter.h -- the modulation meter's integers: the window grid every channel shares, the lane / step a sample of a window goes to, the
// divisions that finish a record, and what a piece of a call means for one metered channel (meter_produce).  Plain C++ (no HIP, no handle, no
// allocation): fmx_api.hip decides with these functions, fmx_meter.hip runs them, tests/meter_check.cpp checks them on the CPU.
#pragma once
#include <cstdint>

namespace fmx {
namespace meter {

constexpr int WINDOW = 9600;           // fm samples per window: 50 ms at 192 000 S/s (ITU-R SM.1268); window w is [9600 w, 9600 (w + 1))
constexpr int LANES = 64;              // sample i of a window is accumulated by lane i mod 64 ...
constexpr int STEPS = WINDOW / LANES;  // ... as its step i div 64 (150 steps: a window is whole steps)
constexpr int RING = 64;               // records kept per channel (3.2 s)
constexpr int QUANT = 6;               // accumulators per lane, in this order in a channel's state [QUANT][LANES]
enum { Q_MX = 0, Q_MN = 1, Q_S1 = 2, Q_S2 = 3, Q_SI = 4, Q_SQ = 5 };
static_assert(STEPS * LANES == WINDOW && (RING & (RING - 1)) == 0, "the window is whole steps, the ring a power of two");

#if defined(__HIPCC__)
#define FMX_METER_HD __host__ __device__
#else
#define FMX_METER_HD
#endif
FMX_METER_HD inline int64_t window_of(int64_t j) { return j / WINDOW; }
FMX_METER_HD inline int lane_of(int i) { return i % LANES; }
FMX_METER_HD inline int step_of(int i) { return i / LANES; }
// the record's fields of the combined sums: mean and mean square over the window's 9600 samples; the pilot's two components as amplitudes -- a pilot
// a sin (phi) in d gives sum d sin (phi) = a 9600 / 2
FMX_METER_HD inline float finish_mean(float s) { return s / 9600.0f; }
FMX_METER_HD inline float finish_pilot(float s) { return s / 4800.0f; }

// One metered channel and one piece of nj > 0 fm samples from J0 on.  The channel's meter has been on in every piece since the one that began at fm sample
// on_from (<= J0) and has completed `produced` records since fmx_create.  A window counts only if the meter was on for all of it: accumulation begins at the
// first window boundary at or behind on_from.
//   first:   the first fm sample the piece accumulates (>= J0; >= J0 + nj: none -- the channel gets no job)
//   w0, nwin: the windows the piece completes, w0 .. w0 + nwin - 1; window w0 + k leaves its record in ring slot slot (k)
struct Produce {
    int64_t first, w0, nwin, produced, new_produced;
    bool    any() const { return nwin > 0; }
    int64_t slot(int64_t k) const { return (produced + k) & (RING - 1); }
    int64_t end_sample(int64_t k) const { return (w0 + k + 1) * WINDOW; }
};
inline Produce meter_produce(int64_t on_from, int64_t J0, int64_t nj, int64_t produced = 0) {
    Produce p{};
    const int64_t end = J0 + nj;
    const int64_t bound = (on_from + WINDOW - 1) / WINDOW * WINDOW;      // (on_from >= 0)
    p.first = bound > J0 ? bound : J0;
    const int64_t wa = p.first / WINDOW, wb = end / WINDOW;              // the window `first` lies in (it is metered from its start), the one `end` lies in
    p.w0 = wa;
    p.nwin = (p.first < end && wb > wa) ? wb - wa : 0;
    p.produced = produced; p.new_produced = produced + p.nwin;
    return p;
}

}  // namespace meter
}  // namespace fmx

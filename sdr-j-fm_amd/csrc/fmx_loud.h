// fmx_loud.h -- the programme audio meter's integers and constants: the window grid every channel shares, the K-weighting coefficients
// as the f32 the machines run with, the divisions that finish a record, and what a piece of a call means for one metered channel (audio_produce).
// Plain C++ (no HIP, no handle, no allocation): fmx_api.hip decides with these functions, fmx_loud.hip runs them, tests/loud_check.cpp checks them on
// the CPU.
#pragma once
#include <cstdint>

namespace fmx {
namespace loud {

constexpr int WINDOW = 4800;           // PCM frames per window: 100 ms at 48 000 frames/s, the gating step of ITU-R BS.1770; window w is [4800 w, 4800 (w + 1))
constexpr int RING = 64;               // records kept per channel (6.4 s)
constexpr int TILE = 64;               // frames a wave stages per channel and step (512 B of a channel's row)
constexpr int STATE = 16;              // floats a channel carries between pieces: [ear][8], in this order per ear
enum { S_T1A = 0, S_T2A = 1, S_T1B = 2, S_T2B = 3, S_PK = 4, S_S2 = 5, S_Z = 6, S_SX = 7 };      // (S_SX: the left ear's; the right ear's is unused)
static_assert((RING & (RING - 1)) == 0, "the ring is a power of two");

// BS.1770-4's K-weighting for 48 000 frames/s, rounded to f32: section 1 the high shelf, section 2 the high-pass (RLB); {b0, b1, b2, a1, a2}
constexpr float K_COEF[2][5] = {
    {1.53512485958697f, -2.69169618940638f, 1.19839281085285f, -1.69065929318241f, 0.73248077421585f},
    {1.0f, -2.0f, 1.0f, -1.99004745483398f, 0.99007225036621f},
};

#if defined(__HIPCC__)
#define FMX_LOUD_HD __host__ __device__
#else
#define FMX_LOUD_HD
#endif
FMX_LOUD_HD inline int64_t window_of(int64_t m) { return m / WINDOW; }
// the record's fields of a window's sums: means over its 4800 frames
FMX_LOUD_HD inline float finish_mean(float s) { return s / 4800.0f; }

// One metered channel and one piece of `frames` > 0 PCM frames from M0 on.  The channel's meter has been on in every piece since the one that began at
// frame on_from (<= M0) and has completed `produced` records since fmx_create.  The filters run over every frame of the piece, from zero states in the
// piece that switched the meter on; a window counts only if the meter was on for all of it: accumulation begins at the first window boundary at or behind
// on_from.
//   reset:   the piece is the one that switched the meter on: the channel's 16 floats start at zero
//   first:   the first frame the piece accumulates (>= M0; >= M0 + frames: none, the piece only runs the filters)
//   w0, nwin: the windows the piece completes, w0 .. w0 + nwin - 1; window w0 + k leaves its record in ring slot slot (k)
struct Produce {
    bool    reset;
    int64_t first, w0, nwin, produced, new_produced;
    bool    any() const { return nwin > 0; }
    int64_t slot(int64_t k) const { return (produced + k) & (RING - 1); }
    int64_t end_frame(int64_t k) const { return (w0 + k + 1) * WINDOW; }
};
inline Produce audio_produce(int64_t on_from, int64_t M0, int64_t frames, int64_t produced = 0) {
    Produce p{};
    const int64_t end = M0 + frames;
    const int64_t bound = (on_from + WINDOW - 1) / WINDOW * WINDOW;      // (on_from >= 0)
    p.reset = on_from == M0;
    p.first = bound > M0 ? bound : M0;
    const int64_t wa = p.first / WINDOW, wb = end / WINDOW;              // the window `first` lies in (it is metered from its start), the one `end` lies in
    p.w0 = wa;
    p.nwin = (p.first < end && wb > wa) ? wb - wa : 0;
    p.produced = produced; p.new_produced = produced + p.nwin;
    return p;
}

}  // namespace loud
}  // namespace fmx

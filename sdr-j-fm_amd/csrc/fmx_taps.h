// fmx_taps.h -- the host side of the eight taps beside the audio chain, in the two kinds they come in.  A RECORD TAP (the modulation, programme audio,
// reception and RDS meters) keeps a record ring per channel: the switches, the sample since which a channel has been on, the records it has produced and
// the reader's cursor.  A SLOT TAP (the spectrum and multiplex spectrum meters, the sub-carrier decoder, the monitoring feed) gives a unit -- a stream or
// a channel -- a slot in device memory the first time it is switched on and tags each ring slot with the item it holds.  Three rules live here and nowhere
// else: a unit found off drops the item in progress (on_from = -1); a unit keeps its slot; a setup taken over starts indices and cursors over.  What a
// window, a record or a block is stays with each tap's own header (meter_produce, audio_produce, rdsm::piece, spec::piece ...).  Plain C++ (no HIP, no
// handle, no lock): fmx_api.hip and fmx_readout.hip keep their books with these functions, under the handle's mutex; tests/taps_check.cpp checks them on
// the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "fmx_needs.h"

namespace fmx {

// `on`: the unit is on in the piece being made.  Off drops what was in progress; the first piece on starts at `pos`; staying on changes nothing.
inline bool tap_begin(bool on, int64_t &on_from, int64_t pos) {
    if (!on) { on_from = -1; return false; }
    if (on_from < 0) on_from = pos;
    return true;
}

struct RecordTap {
    std::vector<uint8_t> user;               // the user's switch (fmx_*_enable)
    std::vector<uint8_t> call;               // the switch of the piece being made
    std::vector<int64_t> on_from;            // the sample since which the channel has been on in every piece (-1: off)
    std::vector<int64_t> produced;           // records completed since fmx_create
    std::vector<int64_t> cursor;             // the next record the read-out hands out
    bool alloc = false;                      // the device side exists: state, ring and jobs (a handle that never switches the meter on has none of it)

    void init(size_t channels) { user.assign(channels, 0); cursor.assign(channels, 0); }      // (what exists from fmx_create on)
    void start(size_t channels) {            // (the device side has just been allocated)
        call.assign(channels, 0); on_from.assign(channels, -1); produced.assign(channels, 0); cursor.assign(channels, 0);
        alloc = true;
    }
    bool any_on() const { return std::any_of(user.begin(), user.end(), [](uint8_t on) { return on != 0; }); }
    void take_switches() { if (alloc) call = user; }
    // false: the channel is off in this piece and gets no job
    bool begin(size_t c, int64_t pos) { return tap_begin(call[c] != 0, on_from[c], pos); }
    RingTake take(size_t c, int64_t ring, int64_t capacity) const { return ring_take(produced[c], cursor[c], ring, capacity); }
    void commit(size_t c, const RingTake &t) { cursor[c] = t.next(); }
};

struct SlotRun { int64_t from; int32_t count; };      // items [from, from + count); from -1: none

struct SlotTap {
    std::vector<int32_t> user;               // the user's value: on / off, a centre, a mode (0: off)
    std::vector<int32_t> call;               // the value of the piece being made
    std::vector<int32_t> slot;               // the unit's slot in the tap's device memory (-1: none yet; a unit keeps its slot)
    std::vector<int64_t> on_from;            // the sample of the piece that switched the unit on (-1: off)
    std::vector<int64_t> cursor;             // the next item the read-out hands out
    std::vector<int64_t> tags;               // [unit * ring + k]: the item ring slot k holds (-1: none)
    int32_t ring = 0;
    int32_t slots = 0, cap = 0;              // slots in use, slots allocated
    bool live = false;                       // some unit is on, or was in the last piece that looked

    void init(size_t units) { user.assign(units, 0); }      // (what exists from fmx_create on)
    void start(size_t units, int32_t ring_slots) {           // (first use; later calls change nothing)
        if (!slot.empty()) return;
        slot.assign(units, -1); on_from.assign(units, -1); cursor.assign(units, 0); call.assign(units, 0);
        tags.assign(units * (size_t)ring_slots, -1); ring = ring_slots;
    }
    bool started() const { return !slot.empty(); }
    bool any_on() const { return std::any_of(user.begin(), user.end(), [](int32_t v) { return v != 0; }); }
    bool wants_slot(size_t u) const { return user[u] != 0 && slot[u] < 0; }
    int32_t slots_needed() const { int32_t n = 0; for (size_t u = 0; u < slot.size(); u++) n += wants_slot(u) ? 1 : 0; return n; }
    void assign_slots() { for (size_t u = 0; u < slot.size(); u++) if (wants_slot(u)) slot[u] = slots++; }
    // a setup taken over: what the rings held is gone, indices and cursors start over; the slots stay
    void restart() { std::fill(on_from.begin(), on_from.end(), -1); std::fill(tags.begin(), tags.end(), -1); std::fill(cursor.begin(), cursor.end(), 0); }
    void take_switches() { if (started()) call = user; }
    // false: the unit is off in this piece and gets no job
    bool begin(size_t u, int64_t pos) { return tap_begin(call[u] != 0, on_from[u], pos); }
    void restart_unit(size_t u) { on_from[u] = -1; }      // (another centre, another mode: the next begin starts as a unit switched on does)
    void tag(size_t u, int64_t item, int64_t ring_slot) { tags[u * (size_t)ring + (size_t)ring_slot] = item; }
    // the tagged items at or past the cursor, ascending, at most `capacity`: older ones were read or overwritten, and a gap is a gap
    void pending(size_t u, int64_t capacity, std::vector<int64_t> &out) const {
        out.clear();
        for (int32_t k = 0; k < ring; k++) if (tags[u * (size_t)ring + (size_t)k] >= cursor[u]) out.push_back(tags[u * (size_t)ring + (size_t)k]);
        std::sort(out.begin(), out.end());
        if ((int64_t)out.size() > capacity) out.resize((size_t)(capacity < 0 ? 0 : capacity));
    }
    // the oldest tagged item at or past the cursor and the consecutive items behind it (item i in ring slot i mod ring): the run ends at a gap
    SlotRun run(size_t u, int64_t capacity) const {
        const int64_t *t = tags.data() + u * (size_t)ring;
        int64_t oldest = -1;
        for (int32_t k = 0; k < ring; k++) if (t[k] >= cursor[u] && (oldest < 0 || t[k] < oldest)) oldest = t[k];
        if (oldest < 0) return {-1, 0};
        int32_t n = 0;
        while (n < capacity && n < ring && t[(oldest + n) % ring] == oldest + n) n++;
        return {oldest, n};
    }
    void commit(size_t u, int64_t next) { cursor[u] = next; }
};

}  // namespace fmx

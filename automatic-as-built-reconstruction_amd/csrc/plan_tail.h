// plan_tail.h -- ticket bookkeeping of the deferred-join tail of a launch plan (plan.hip: AABR_PLAN_TAIL records).
// Host-only and free of HIP calls, like the *_tiles.h decision headers: tests/plan_tail_host_harness.cpp compiles it
// alone (with sanitizers) and walks the join / release orders a caller can produce.
//
// A ticket stands for "everything a call issued on the tail stream".  It names one slot of a grow-only table plus
// the slot's generation at the time it was handed out:  ticket = generation << kSlotBits | (slot + 1);  0 = no tail.
// Releasing bumps the generation, so every copy of a released ticket is stale from then on: `find` answers -1 for it
// (join / sync on a stale ticket are no-ops: its owner has joined it -- that is what entitles one to release), a second
// release does nothing.  The slot keeps its `event` (an opaque handle the caller created for `device`) across
// releases: that is the pool -- the next ticket of the same device reuses it.
#pragma once
#include <stdint.h>
#include <mutex>
#include <vector>

namespace aabr {

struct TailTickets {
  static constexpr int kSlotBits = 20;
  static constexpr uint64_t kSlotMask = (1ull << kSlotBits) - 1;
  struct Slot {
    uint64_t gen = 1;        // generation of the ticket that is or will next be handed out for this slot
    bool live = false;
    void *event = nullptr;   // pooled handle; stays with the slot
    int device = -1;         // the device `event` belongs to (-1: no event yet)
  };
  std::mutex m;              // held by the caller around every call below AND the use it makes of slot(..).event
  std::vector<Slot> slots;

  // a free slot whose pooled event belongs to `device` (or that has none yet); 0 when the table is full
  uint64_t acquire(int device, int *slot_out) {
    int s = -1;
    for (size_t i = 0; i < slots.size() && s < 0; ++i)
      if (!slots[i].live && (slots[i].device == device || slots[i].event == nullptr)) s = (int)i;
    if (s < 0) {
      if (slots.size() >= (size_t)kSlotMask) return 0;
      slots.push_back(Slot());
      s = (int)slots.size() - 1;
    }
    slots[s].live = true;
    *slot_out = s;
    return (slots[s].gen << kSlotBits) | (uint64_t)(s + 1);
  }
  // the live slot of `ticket`; -1 for 0, a value never handed out, or a released ticket
  int find(uint64_t ticket) const {
    const uint64_t idx = ticket & kSlotMask;
    if (ticket == 0 || idx == 0 || idx > slots.size()) return -1;
    const Slot &sl = slots[idx - 1];
    return (sl.live && sl.gen == (ticket >> kSlotBits)) ? (int)(idx - 1) : -1;
  }
  // true when THIS call released the ticket (its event went back to the pool)
  bool release(uint64_t ticket) {
    const int s = find(ticket);
    if (s < 0) return false;
    slots[s].live = false;
    ++slots[s].gen;
    return true;
  }
  size_t live_count() const {
    size_t n = 0;
    for (const Slot &sl : slots) n += sl.live ? 1 : 0;
    return n;
  }
};

} // namespace aabr

// Stand-alone host program for csrc/plan_tail.h (the ticket table of the deferred-join tail): built with the host
// sanitizers by tests/test_plan_tail_host.py and run directly.  Walks the orders a ticket's holder can produce -- join
// twice, release twice, join after release, a copy of a ticket outliving the slot's reuse -- and the pool.
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include "../automatic-as-built-reconstruction_amd/csrc/plan_tail.h"

using aabr::TailTickets;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
  } while (0)

// what plan.hip does around the table: the "event" is created when a slot has none, and stays with the slot
static int g_events_made = 0;
static uint64_t take(TailTickets &t, int device) {
  std::lock_guard<std::mutex> l(t.m);
  int s = -1;
  const uint64_t tk = t.acquire(device, &s);
  if (tk && t.slots[s].event == nullptr) {
    t.slots[s].event = malloc(8);
    t.slots[s].device = device;
    ++g_events_made;
  }
  return tk;
}
static bool joinable(TailTickets &t, uint64_t tk) {   // aabr_plan_tail_join: waits only for a live ticket
  std::lock_guard<std::mutex> l(t.m);
  const int s = t.find(tk);
  return s >= 0 && t.slots[s].event != nullptr;
}
static bool give_back(TailTickets &t, uint64_t tk) {
  std::lock_guard<std::mutex> l(t.m);
  return t.release(tk);
}

int main() {
  TailTickets t;
  CHECK(!joinable(t, 0) && !give_back(t, 0));                  // 0 = "the list had no tail"
  CHECK(!joinable(t, 12345) && !give_back(t, 12345));          // never handed out
  CHECK(!joinable(t, ~0ull) && !give_back(t, ~0ull));

  const uint64_t a = take(t, 0);
  CHECK(a != 0 && t.live_count() == 1);
  CHECK(joinable(t, a) && joinable(t, a));                     // join twice
  CHECK(give_back(t, a) && !give_back(t, a));                  // release twice: the second does nothing
  CHECK(!joinable(t, a));                                      // join after release: a no-op
  CHECK(t.live_count() == 0);

  const uint64_t b = take(t, 0);                               // the pool: same slot, same event, another generation
  CHECK(b != 0 && b != a && (b & TailTickets::kSlotMask) == (a & TailTickets::kSlotMask) && g_events_made == 1);
  CHECK(joinable(t, b) && !joinable(t, a) && !give_back(t, a));   // the stale copy touches nothing of the new holder's
  CHECK(joinable(t, b));

  const uint64_t c = take(t, 0);                               // two in flight: two slots
  CHECK(c != 0 && (c & TailTickets::kSlotMask) != (b & TailTickets::kSlotMask) && g_events_made == 2);
  CHECK(give_back(t, b) && joinable(t, c) && !joinable(t, b));

  const uint64_t d = take(t, 1);                               // a pooled event is never handed to another device
  CHECK(d != 0 && g_events_made == 3 && (d & TailTickets::kSlotMask) != (b & TailTickets::kSlotMask));
  const uint64_t e = take(t, 0);
  CHECK((e & TailTickets::kSlotMask) == (b & TailTickets::kSlotMask) && g_events_made == 3);
  CHECK(give_back(t, c) && give_back(t, d) && give_back(t, e) && t.live_count() == 0);

  // forward thread takes, "autograd" threads join and release, all at once
  {
    TailTickets u;
    std::thread th[4];
    int bad[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; ++k)
      th[k] = std::thread([&u, &bad, k] {
        for (int i = 0; i < 2000; ++i) {
          const uint64_t tk = take(u, k & 1);
          if (!tk || !joinable(u, tk)) ++bad[k];
          std::thread other([&u, &bad, k, tk] {
            if (!joinable(u, tk) || !give_back(u, tk) || give_back(u, tk) || joinable(u, tk)) ++bad[k];
          });
          other.join();
        }
      });
    for (auto &x : th) x.join();
    CHECK(bad[0] + bad[1] + bad[2] + bad[3] == 0 && u.live_count() == 0 && u.slots.size() <= 8);
    for (auto &sl : u.slots) free(sl.event);
  }
  for (auto &sl : t.slots) free(sl.event);
  printf("ok\n");
  return 0;
}

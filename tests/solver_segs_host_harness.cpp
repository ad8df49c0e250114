// Stand-alone host program over csrc/solver_segs.h: the segment-to-chunk cutter against a brute-force enumeration of
// (segment, element), and the step entry's refusals -- meant to be built with the host address / undefined-behaviour
// sanitizers (tests/test_solver_host.py).  No device code exists in the header.  Exit status 0 and a last line "ok" when
// every expectation holds; otherwise one line per failed expectation.
#include "../automatic-as-built-reconstruction_amd/csrc/solver_segs.h"

#include <stdio.h>
#include <string.h>
#include <vector>

using namespace aabr;

static int g_failed = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++g_failed; } \
  } while (0)

// segments of the given sizes packed back to back from flat offset `first`; heap vectors of the exact size, so that a
// read or write past either end is an error the sanitizer reports
static void check_packing(const std::vector<int64_t> &sizes, int64_t first) {
  const int64_t n_segs = (int64_t)sizes.size();
  std::vector<int64_t> off(sizes.size()), numel(sizes);
  std::vector<int32_t> group(sizes.size());
  int64_t n = first;
  for (int64_t s = 0; s < n_segs; ++s) {
    off[s] = n;
    group[s] = (int32_t)(s % kSgdMaxGroups);
    n += sizes[s];
  }
  off.shrink_to_fit(); numel.shrink_to_fit(); group.shrink_to_fit();
  const char *why = nullptr;
  const int64_t count = sgd_cut_segments(off.data(), numel.data(), group.data(), n_segs, n, nullptr, 0, &why);
  EXPECT(count >= 0);
  if (count < 0) { printf("  refused: %s\n", why); return; }
  std::vector<SgdChunk> tab((size_t)count);
  tab.shrink_to_fit();
  EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), n_segs, n, tab.data(), count, &why) == count);
  if (count > 1) {   // one record short: refused, nothing written past the end
    std::vector<SgdChunk> small((size_t)count - 1);
    small.shrink_to_fit();
    EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), n_segs, n, small.data(), count - 1, &why) == -1);
    EXPECT(strstr(why, "too small") != nullptr);
  }
  // brute force: the owner of every flat element, by walking the segments
  std::vector<int64_t> owner((size_t)n, -1), covered((size_t)n, 0);
  for (int64_t s = 0; s < n_segs; ++s)
    for (int64_t e = 0; e < sizes[s]; ++e) owner[(size_t)(off[s] + e)] = s;
  int64_t prev_end = 0, chunks_of_empty = 0;
  for (int64_t c = 0; c < count; ++c) {
    const SgdChunk &k = tab[(size_t)c];
    const int64_t s = k.seg_group / kSgdMaxGroups;
    EXPECT(k.n >= 1 && k.n <= kSgdChunkElems);
    EXPECT(k.off >= prev_end && k.off + k.n <= n);
    EXPECT(s >= 0 && s < n_segs);
    if (s < 0 || s >= n_segs || k.off < 0 || k.off + k.n > n) continue;
    EXPECT(k.seg_group % kSgdMaxGroups == group[(size_t)s]);
    EXPECT(k.seg_first == off[(size_t)s]);
    if (sizes[(size_t)s] == 0) ++chunks_of_empty;
    // a chunk's two ends are its segment's ends or multiples of 4 of the flat offset
    EXPECT(k.off == off[(size_t)s] || k.off % 4 == 0);
    EXPECT(k.off + k.n == off[(size_t)s] + sizes[(size_t)s] || (k.off + k.n) % 4 == 0);
    for (int64_t e = k.off; e < k.off + k.n; ++e) {
      EXPECT(owner[(size_t)e] == s);
      ++covered[(size_t)e];
    }
    prev_end = k.off + k.n;
  }
  EXPECT(chunks_of_empty == 0);
  for (int64_t e = 0; e < n; ++e) EXPECT(covered[(size_t)e] == (owner[(size_t)e] >= 0 ? 1 : 0));
}

static void check_bad_segments() {
  const char *why = nullptr;
  std::vector<int64_t> off = {0, 8}, numel = {8, 8};
  std::vector<int32_t> group = {0, 1};
  EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), 2, 16, nullptr, 0, &why) == 2);
  EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), 2, 15, nullptr, 0, &why) == -1 && strstr(why, "past n"));
  EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), -1, 16, nullptr, 0, &why) == -1 && strstr(why, "negative"));
  EXPECT(sgd_cut_segments(nullptr, numel.data(), group.data(), 2, 16, nullptr, 0, &why) == -1 && strstr(why, "null"));
  off[1] = 7;
  EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), 2, 16, nullptr, 0, &why) == -1 && strstr(why, "overlap"));
  off[1] = 8; group[1] = 8;
  EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), 2, 16, nullptr, 0, &why) == -1 && strstr(why, "group"));
  group[1] = 1; numel[0] = -1;
  EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), 2, 16, nullptr, 0, &why) == -1 && strstr(why, "negative"));
  numel[0] = 8; numel[1] = INT64_MAX;     // first + len would overflow: refused by the subtraction form of the check
  EXPECT(sgd_cut_segments(off.data(), numel.data(), group.data(), 2, 16, nullptr, 0, &why) == -1 && strstr(why, "past n"));
  EXPECT(sgd_cut_segments(nullptr, nullptr, nullptr, 0, 0, nullptr, 0, &why) == 0);
  EXPECT(sgd_cut_segments(nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr) == 0);
}

static void check_step_refusals() {
  alignas(16) static float buf[64];
  const void *p = buf, *m = buf + 32, *tab = buf, *g = buf;
  const float lr[8] = {0}, wd[8] = {0};
  SgdChunk last{28, 24, 4, 3 * kSgdMaxGroups + 1};
  auto R = [&](const void *flat, const void *mom, int64_t n, const void *table, const SgdChunk *l, int64_t n_chunks,
               int64_t n_segs, const void *gf, const void *gt, int bf16, const float *a, const float *b, int groups,
               float mu) { return sgd_step_refusal(flat, mom, n, table, l, n_chunks, n_segs, gf, gt, bf16, a, b, groups, mu); };
  EXPECT(R(p, m, 32, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f) == nullptr);
  EXPECT(R(p, m, 32, tab, &last, 5, 4, nullptr, g, 1, lr, wd, 8, 0.9f) == nullptr);
  EXPECT(R(p, nullptr, 32, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 1, 0.0f) == nullptr);   // no buffer without momentum
  EXPECT(R(nullptr, nullptr, 0, nullptr, nullptr, 0, 0, g, nullptr, 0, lr, wd, 1, 0.9f) == nullptr);   // nothing to do
  const char *w;
  EXPECT((w = R(p, m, 32, tab, &last, 5, 4, g, g, 0, lr, wd, 2, 0.9f)) && strstr(w, "both"));
  EXPECT((w = R(p, m, 32, tab, &last, 5, 4, nullptr, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "neither"));
  EXPECT((w = R(p, m, 32, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 0, 0.9f)) && strstr(w, "n_groups"));
  EXPECT((w = R(p, m, 32, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 9, 0.9f)) && strstr(w, "n_groups"));
  EXPECT((w = R(nullptr, m, 32, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "null"));
  EXPECT((w = R(p, nullptr, 32, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "null"));
  EXPECT((w = R(p, m, 32, nullptr, &last, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "null"));
  EXPECT((w = R(p, m, 32, tab, nullptr, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "null"));
  EXPECT((w = R(p, m, 32, tab, &last, 5, 4, g, nullptr, 0, nullptr, wd, 2, 0.9f)) && strstr(w, "null"));
  EXPECT((w = R(p, m, -1, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "negative"));
  EXPECT((w = R(p, m, 32, tab, &last, -5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "negative"));
  EXPECT((w = R(p, m, 31, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "past n"));
  EXPECT((w = R(p, m, 32, tab, &last, 5, 3, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "n_segs"));
  EXPECT((w = R(buf + 1, m, 32, tab, &last, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "aligned"));
  EXPECT((w = R(p, m, 32, tab, &last, 5, 4, g, nullptr, 2, lr, wd, 2, 0.9f)) && strstr(w, "grad_is_bf16"));
  SgdChunk huge{INT64_MAX - 2, 0, 4, 0};     // off + n would overflow
  EXPECT((w = R(p, m, 32, tab, &huge, 5, 4, g, nullptr, 0, lr, wd, 2, 0.9f)) && strstr(w, "past n"));
}

int main() {
  const int64_t C = kSgdChunkElems;
  const std::vector<int64_t> sizes = {0, 1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, 0, 5, 1, 4, 3, 2 * C + 3, C + 1, C, C - 1, 0};
  for (int64_t first = 0; first < 4; ++first) check_packing(sizes, first);
  // every size at every flat phase, alone
  for (int64_t s : sizes)
    for (int64_t first = 0; first < 8; ++first) check_packing({s}, first);
  check_packing({}, 0);
  check_bad_segments();
  check_step_refusals();
  if (g_failed) { printf("%d expectation(s) failed\n", g_failed); return 1; }
  printf("ok\n");
  return 0;
}

// Stand-alone host program over csrc/anchor_list.h: fill_anchor_segs on good and bad tables, meant to be built with the
// host address / undefined-behaviour sanitizers (tests/test_anchor_list_host.py).  No device code runs.  Exit status 0
// and a last line "ok" when every expectation holds; otherwise one line per failed expectation.
#include "../automatic-as-built-reconstruction_amd/csrc/anchor_list.h"

#include <stdarg.h>
#include <string.h>
#include <string>
#include <vector>

static std::string g_error;
namespace aabr {
void set_error(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_error = buf;
}
}  // namespace aabr
using namespace aabr;

static int g_failed = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++g_failed; } \
  } while (0)

// the flat tables of counts[m][b] sites, as rpn_glue._anchor_tables lays them out; heap vectors of the exact size, so that
// a read past either end is an error the sanitizer reports
static void tables(const std::vector<std::vector<int>> &counts, int A, std::vector<int32_t> &seg, std::vector<int32_t> &site) {
  const int n_maps = (int)counts.size(), nb = (int)counts[0].size();
  std::vector<int> row(n_maps, 0);
  seg.clear(); site.clear();
  for (int b = 0; b < nb; ++b) {
    seg.push_back(0);
    for (int m = 0; m < n_maps; ++m) {
      seg.push_back(seg.back() + counts[m][b] * A);
      site.push_back(row[m]);
      row[m] += counts[m][b];
    }
  }
  seg.shrink_to_fit(); site.shrink_to_fit();
}

static void expect_refused(const std::vector<int32_t> &seg, const std::vector<int32_t> &site, int n_maps, int A, int nb,
                           const char *what) {
  AnchorSegs s;
  g_error.clear();
  EXPECT(fill_anchor_segs(s, "entry_under_test", n_maps, A, 0, nb, seg.data(), site.data(), nullptr) == AABR_EINVAL);
  EXPECT(g_error.find("entry_under_test") != std::string::npos);
  EXPECT(g_error.find(what) != std::string::npos);
}

int main() {
  // map 1 empty for example 1, map 2 empty for all, example 2 without sites
  const std::vector<std::vector<int>> counts = {{5, 2, 0, 4}, {3, 0, 0, 1}, {0, 0, 0, 0}};
  const int A = 3, n_maps = 3, nb = 4;
  std::vector<int32_t> seg, site;
  tables(counts, A, seg, site);
  for (int b0 = 0; b0 < nb; ++b0) {
    AnchorSegs s;
    memset(&s, 0xff, sizeof s);
    int64_t nmax = -1;
    EXPECT(fill_anchor_segs(s, "good", n_maps, A, b0, nb - b0, seg.data(), site.data(), &nmax) == AABR_OK);
    EXPECT(s.n_maps == n_maps && s.nb == nb - b0 && s.A == A);
    int64_t longest = 0;
    for (int b = 0; b < kAnchorMaxBatch; ++b)
      for (int m = 0; m <= kAnchorMaxMaps; ++m) {
        const bool on = b < nb - b0;
        EXPECT(s.seg[b][m] == (on ? seg[(b0 + b) * (n_maps + 1) + (m < n_maps ? m : n_maps)] : 0));
        if (m < kAnchorMaxMaps) EXPECT(s.site[b][m] == (on && m < n_maps ? site[(b0 + b) * n_maps + m] : 0));
        if (on && s.seg[b][m] > longest) longest = s.seg[b][m];
      }
    EXPECT(nmax == longest);
  }
  {  // no site table: the flat-list mode, all rows 0
    AnchorSegs s;
    EXPECT(fill_anchor_segs(s, "flat", n_maps, A, 0, nb, seg.data(), nullptr, nullptr) == AABR_OK);
    for (int b = 0; b < kAnchorMaxBatch; ++b)
      for (int m = 0; m < kAnchorMaxMaps; ++m) EXPECT(s.site[b][m] == 0);
  }
  {  // the largest table: 8 maps, 16 examples, nothing to pad
    std::vector<std::vector<int>> full(kAnchorMaxMaps, std::vector<int>(kAnchorMaxBatch));
    for (int m = 0; m < kAnchorMaxMaps; ++m)
      for (int b = 0; b < kAnchorMaxBatch; ++b) full[m][b] = (m * 7 + b * 3) % 5;
    std::vector<int32_t> fseg, fsite;
    tables(full, 1, fseg, fsite);
    AnchorSegs s;
    int64_t nmax = 0;
    EXPECT(fill_anchor_segs(s, "full", kAnchorMaxMaps, 1, 0, kAnchorMaxBatch, fseg.data(), fsite.data(), &nmax) == AABR_OK);
    for (int b = 0; b < kAnchorMaxBatch; ++b) {
      for (int m = 0; m <= kAnchorMaxMaps; ++m) EXPECT(s.seg[b][m] == fseg[b * (kAnchorMaxMaps + 1) + m]);
      for (int m = 0; m < kAnchorMaxMaps; ++m) EXPECT(s.site[b][m] == fsite[b * kAnchorMaxMaps + m]);
    }
    expect_refused(fseg, fsite, kAnchorMaxMaps + 1, 1, 1, "maps");
    AnchorSegs t;
    EXPECT(fill_anchor_segs(t, "full", kAnchorMaxMaps, 1, 0, kAnchorMaxBatch + 1, fseg.data(), fsite.data(), nullptr) == AABR_EINVAL);
    EXPECT(fill_anchor_segs(t, "full", kAnchorMaxMaps, 0, 0, kAnchorMaxBatch, fseg.data(), fsite.data(), nullptr) == AABR_EINVAL);
    EXPECT(fill_anchor_segs(t, "full", kAnchorMaxMaps, 1, 0, 1, nullptr, fsite.data(), nullptr) == AABR_EINVAL);
  }
  // the three bad tables, each in the LAST example so that every earlier row is walked first
  std::vector<int32_t> bad = seg;
  bad[3 * (n_maps + 1) + 2] = bad[3 * (n_maps + 1) + 1] - A;   // decreasing
  expect_refused(bad, site, n_maps, A, nb, "non-decreasing");
  bad = seg;
  for (int m = 0; m <= n_maps; ++m) bad[3 * (n_maps + 1) + m] += A;   // first entry not 0
  expect_refused(bad, site, n_maps, A, nb, "starts at 0");
  bad = seg;
  for (int m = 1; m <= n_maps; ++m) bad[3 * (n_maps + 1) + m] += 1;   // a segment that is no multiple of A
  expect_refused(bad, site, n_maps, A, nb, "multiple of A");
  if (g_failed) return 1;
  printf("ok\n");
  return 0;
}

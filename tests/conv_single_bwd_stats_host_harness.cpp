// Compiles the PRODUCT's decision for the backward-statistics form of the single-rule convolution
// (automatic-as-built-reconstruction_amd/csrc/conv_single_tiles.h: single_bwd_stats_refusal, single_bwd_stats_launch) for the
// host: tests/test_conv_single_bwd_stats_host.py compares it with a plain restatement in Python.  With -DHARNESS_MAIN it is
// a stand-alone program that sweeps the same header and checks its invariants: the form run under the sanitizers.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../automatic-as-built-reconstruction_amd/csrc/conv_single_tiles.h"
// cases[n][11]: bf16, n_in, n_out, rows_in, rows_out, vol, flags, the three SingleKnobs, the SINGLE_BWD_STATS knob
// out[n][13]: route refused, chunk of the route (0 when refused), launch refused, kg, chunk_pairs, grid_x, grid_y, lds_bytes,
//             wflip, wp_bytes, parts, stats_doubles, the plain route asked with has_stats = true refused
// msgs[n][3][128]: the route's, the launch's and the plain route's (has_stats = true) refusal texts
extern "C" void host_single_bwd_stats(const int64_t *cases, int64_t n, int64_t *out, char *msgs) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t *c = cases + 11 * i;
    int64_t *o = out + 13 * i;
    const aabr::SingleKnobs kn{(int)c[7], (int)c[8], (int)c[9]};
    const bool bf16 = c[0] != 0;
    const int n_in = (int)c[1], n_out = (int)c[2], vol = (int)c[5];
    const char *m = aabr::single_bwd_stats_refusal(bf16, n_in, n_out, c[3], c[4], vol, kn, (int)c[10]);
    strncpy(msgs + 384 * i, m ? m : "", 127);
    o[0] = m != nullptr;
    o[1] = m ? 0 : aabr::single_chunk_pairs(kn);
    aabr::SingleBwdStatsLaunch t;
    const char *l = aabr::single_bwd_stats_launch(n_in, n_out, c[3], c[4], vol, (int)c[6], kn, t);
    strncpy(msgs + 384 * i + 128, l ? l : "", 127);
    const int64_t r[10] = {l != nullptr, t.l.kg,    t.l.chunk_pairs, t.l.grid_x, t.l.grid_y, t.l.lds_bytes,
                           t.l.wflip,    t.l.wp_bytes, t.parts,      t.stats_doubles};
    for (int j = 0; j < 10; ++j) o[2 + j] = r[j];
    const char *old = aabr::single_refusal(bf16, true, n_in, n_out, c[3], c[4], vol, kn);
    strncpy(msgs + 384 * i + 256, old ? old : "", 127);
    o[12] = old != nullptr;
  }
}
extern "C" int64_t host_single_min_rows(void) { return aabr::kSingleMinRows; }
extern "C" int host_single_default_on(void) { return aabr::kSingleDefaultOn; }
extern "C" int host_single_bwd_stats_default_on(void) { return aabr::kSingleBwdStatsDefaultOn; }

#ifdef HARNESS_MAIN
#define EXPECT(cond)                                                                                  \
  do {                                                                                                \
    if (!(cond)) { printf("FAILED %s (case %lld)\n", #cond, (long long)i); return 1; }               \
  } while (0)
int main() {
  const int64_t U = aabr::kKnobUnset;
  const int64_t n_ins[] = {0, 32, 48, 64, 128, 160}, n_outs[] = {32, 64, 128, 192}, vols[] = {1, 8, 27, 70000};
  const int64_t rows[] = {-1, 0, 1, 255, 256, 1000, 32767, 32768, 84077, 281622, (1ll << 25) - 1, 1ll << 25};
  const int64_t knobs[][4] = {{U, U, U, U}, {1, 0, U, 1}, {1, 0, 1024, U}, {0, U, U, U}, {U, U, U, 0}, {U, 100000, 512, 1}};
  int64_t taken = 0, i = 0;
  for (int64_t bf16 = 0; bf16 < 2; ++bf16)
    for (int64_t n_in : n_ins)
      for (int64_t n_out : n_outs)
        for (int64_t vol : vols)
          for (int64_t r : rows)
            for (const auto &kn : knobs) {
              const int64_t c[11] = {bf16, n_in, n_out, r + 3, r, vol, (i & 1) * 2, kn[0], kn[1], kn[2], kn[3]};
              int64_t o[13];
              char msgs[384];
              memset(msgs, 0, sizeof(msgs));
              host_single_bwd_stats(c, 1, o, msgs);
              ++i;
              EXPECT(o[12] == 1);                                    // the plain route never delivers statistics
              EXPECT((o[0] != 0) == (msgs[0] != 0) && (o[2] != 0) == (msgs[128] != 0));
              if (o[0] == 0) {                                       // routed: the launch exists and its buffer holds the parts
                ++taken;
                EXPECT(o[2] == 0 && o[4] == o[1] && (o[1] == 256 || o[1] == 1024));
                EXPECT(o[10] == o[5] && o[10] == r / o[1] + vol && o[11] == o[10] * 2 * n_out);
                EXPECT(o[7] >= aabr::kSingleReduceBytes && o[7] >= 2 * 32 * n_in * 4 && o[6] == n_out / 64);
                const int64_t min_rows = kn[1] == U ? aabr::kSingleMinRows : kn[1];
                EXPECT(r >= min_rows && (min_rows < aabr::kSingleMinRows || o[10] <= r / 64 + 1));
              }
              if (o[2] != 0 || r <= 0) EXPECT(o[10] == 0 && o[11] == 0 && o[5] == 0);
            }
  printf("%lld cases, %lld routed\n", (long long)i, (long long)taken);
  return taken > 50 ? 0 : 1;
}
#endif

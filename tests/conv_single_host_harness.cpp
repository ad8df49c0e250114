// Compiles the PRODUCT's single-rule route decision (automatic-as-built-reconstruction_amd/csrc/conv_single_tiles.h) for the
// host: tests/test_conv_single_host.py compares it with a plain restatement in Python.
#include <stdint.h>
#include <string.h>
#include "../automatic-as-built-reconstruction_amd/csrc/conv_single_tiles.h"
// cases[n][11]: bf16, has_stats, n_in, n_out, rows_in, rows_out, vol, flags, then the three SingleKnobs
// out[n][10]: route refused, chunk of the route (0 when refused), launch refused, kg, chunk_pairs, grid_x, grid_y, lds_bytes,
//             wflip, wp_bytes; msgs[n][2][128]: the route's and the launch's refusal texts
extern "C" void host_single(const int64_t *cases, int64_t n, int64_t *out, char *msgs) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t *c = cases + 11 * i;
    int64_t *o = out + 10 * i;
    const aabr::SingleKnobs kn{(int)c[8], (int)c[9], (int)c[10]};
    const bool bf16 = c[0] != 0, stats = c[1] != 0;
    const int n_in = (int)c[2], n_out = (int)c[3], vol = (int)c[6];
    const char *m = aabr::single_refusal(bf16, stats, n_in, n_out, c[4], c[5], vol, kn);
    strncpy(msgs + 256 * i, m ? m : "", 127);
    o[0] = m != nullptr;
    o[1] = m ? 0 : aabr::single_chunk_pairs(kn);
    aabr::SingleLaunch t;
    const char *l = aabr::single_launch(n_in, n_out, c[4], c[5], vol, (int)c[7], kn, t);
    strncpy(msgs + 256 * i + 128, l ? l : "", 127);
    const int64_t r[8] = {l != nullptr, t.kg, t.chunk_pairs, t.grid_x, t.grid_y, t.lds_bytes, t.wflip, t.wp_bytes};
    for (int j = 0; j < 8; ++j) o[2 + j] = r[j];
  }
}
extern "C" int64_t host_single_min_rows(void) { return aabr::kSingleMinRows; }
extern "C" int host_single_default_on(void) { return aabr::kSingleDefaultOn; }

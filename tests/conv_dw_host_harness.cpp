// Compiles the PRODUCT's weight-gradient launch decision (automatic-as-built-reconstruction_amd/csrc/conv_dw_tiles.h) for
// the host: tests/test_conv_dw_host.py compares it with the rule restated in tests/conv_dw_rule.py.
#include <stdint.h>
#include "../automatic-as-built-reconstruction_amd/csrc/conv_dw_tiles.h"
// cases[n][10]: bf16, n_in, n_out, V_out, vol, max_chunks, aligned16, then the three DwKnobs values;
// out[n][12]: kind, bf16, cb, nb, chunk_pairs, direct, grid_x, grid_y, n_wg, reduce, to_scratch, tiles
extern "C" void host_conv_dw_launch(const int64_t *cases, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t *c = cases + 10 * i;
    const aabr::DwKnobs kn{(int)c[7], (int)c[8], (int)c[9]};
    const aabr::DwLaunch d = aabr::conv_dw_launch(c[0] != 0, (int)c[1], (int)c[2], c[3], (int)c[4], c[5], c[6] != 0, kn);
    const int64_t r[12] = {d.k.kind, d.k.bf16, d.k.cb, d.k.nb, d.chunk_pairs, d.direct,
                           d.grid_x, d.grid_y, d.n_wg, d.reduce, d.to_scratch, d.tiles};
    for (int j = 0; j < 12; ++j) out[12 * i + j] = r[j];
  }
}

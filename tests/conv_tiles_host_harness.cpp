// Compiles the PRODUCT's 64-row-tile launch decision (automatic-as-built-reconstruction_amd/csrc/conv_tiles.h) for the
// host: tests/test_conv_tiles_host.py compares it with the rule restated in tests/conv_tiles_rule.py.
#include <stdint.h>
#include "../automatic-as-built-reconstruction_amd/csrc/conv_tiles.h"
// cases[n][15]: bf16, n_in, n_out, V_out, vol, flags, in_bytes, wp_bytes, words_bytes, then the six TileKnobs values;
// out[n][11]: kind, nbw, wpb, nkc, kg, aligned, adj, grid_x, grid_y, block, lds
extern "C" void host_conv_tile_launch(const int64_t *cases, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t *c = cases + 15 * i;
    const aabr::TileKnobs kn{(int)c[9], (int)c[10], (int)c[11], (int)c[12], (int)c[13], (int)c[14]};
    const aabr::TileLaunch t = (c[0] ? aabr::conv_tile_launch_bf16 : aabr::conv_tile_launch)(
        (int)c[1], (int)c[2], c[3], (int)c[4], (int)c[5], c[6], c[7], c[8], kn);
    const int64_t r[11] = {t.k.kind, t.k.nbw, t.k.wpb, t.k.nkc, t.k.kg, t.k.aligned, t.k.adj,
                           t.grid_x, t.grid_y, t.block, t.lds};
    for (int j = 0; j < 11; ++j) out[11 * i + j] = r[j];
  }
}

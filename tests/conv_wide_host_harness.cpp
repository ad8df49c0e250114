// Compiles the PRODUCT's wide-kernel launch decision (automatic-as-built-reconstruction_amd/csrc/conv_wide_tiles.h) for
// the host, without and with -DAABR_DEV: tests/test_conv_wide_host.py compares it with the rule restated in
// tests/conv_wide_rule.py.
#include <stdint.h>
#include <string.h>
#include "../automatic-as-built-reconstruction_amd/csrc/conv_wide_tiles.h"
// cases[n][21]: storage, parts, n_in, n_out, rows_in, V_out, tile_rows, vol, flags, has_stats, then the eleven WideKnobs
// what 0: wide_tile_rows -> out[n][14] = {T}; 1: wide_split -> {(P << 16) | T}; 2: wide_launch ->
// out[n][14]: refused, kg, dbg, nbuf, bf16, ncb, split, grid_x, grid_y, lds_bytes, wflip, in_bytes, words_bytes, wp_bytes
// and msgs[n][128]: the refusal's text
extern "C" void host_wide(int what, const int64_t *cases, int64_t n, int64_t *out, char *msgs) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t *c = cases + 21 * i;
    int64_t *o = out + 14 * i;
    const aabr::WideKnobs kn{(int)c[10], (int)c[11], (int)c[12], (int)c[13], (int)c[14], (int)c[15],
                             (int)c[16], (int)c[17], (int)c[18], (int)c[19], (int)c[20]};
    const int st = (int)c[0], n_in = (int)c[2], n_out = (int)c[3], vol = (int)c[7];
    for (int j = 0; j < 14; ++j) o[j] = 0;
    if (what == 0) { o[0] = aabr::wide_tile_rows(st, n_in, n_out, c[4], c[5], vol, kn); continue; }
    if (what == 1) { o[0] = aabr::wide_split(st, n_in, n_out, c[4], c[5], vol, kn); continue; }
    aabr::WideLaunch t;
    const char *m = aabr::wide_launch(st, (int)c[1], n_in, n_out, c[4], c[5], (int)c[6], vol, (int)c[8], c[9] != 0, kn, t);
    strncpy(msgs + 128 * i, m ? m : "", 127);
    const int64_t r[14] = {m != nullptr, t.k.kg, t.k.dbg, t.k.nbuf, t.k.bf16, t.k.ncb, t.k.split, t.grid_x, t.grid_y,
                           t.lds_bytes, t.wflip, t.in_bytes, t.words_bytes, t.wp_bytes};
    for (int j = 0; j < 14; ++j) o[j] = r[j];
  }
}
extern "C" int host_wide_dev(void) { return aabr::kWideDev; }
// the loaded library's four dispatch queries over the same cases (fns: tile_rows, tile_rows_bf16, split, split_bf16, handed
// over as addresses so that a grid of this size costs no Python call per case); out[n][2] = {tile rows, split word}
typedef int (*WideQuery)(int, int, int64_t, int64_t, int);
extern "C" void host_library_queries(void *const *fns, const int64_t *cases, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t *c = cases + 21 * i;
    const int bf = c[0] != 0;
    out[2 * i] = ((WideQuery)fns[bf])((int)c[2], (int)c[3], c[4], c[5], (int)c[7]);
    out[2 * i + 1] = ((WideQuery)fns[2 + bf])((int)c[2], (int)c[3], c[4], c[5], (int)c[7]);
  }
}

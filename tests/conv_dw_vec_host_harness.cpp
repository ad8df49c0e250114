// Compiles the PRODUCT's choice of the weight gradient's gather form (automatic-as-built-reconstruction_amd/csrc/
// conv_dw_tiles.h: dw_vec_operands and the accumulator -> channel maps dw_tile_row / dw_tile_col) for the host:
// tests/test_conv_dw_vec_host.py compares it with a Python restatement.  With -DDW_VEC_HOST_MAIN it is a program of its own
// that walks the same grid and checks the maps (built with -fsanitize=address,undefined by the test).
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../automatic-as-built-reconstruction_amd/csrc/conv_dw_tiles.h"

// cases[n][6]: bf16, n_in, n_out, align_in, align_dout, knob DW_VEC; out[n][3]: cb, nb (dw_tiling), mask
extern "C" void host_dw_vec_operands(const int64_t *cases, int64_t n, int64_t *out) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t *c = cases + 6 * i;
    int cb, nb, tiles;
    aabr::dw_tiling((int)c[1], (int)c[2], cb, nb, tiles);
    out[3 * i] = cb;
    out[3 * i + 1] = nb;
    out[3 * i + 2] = aabr::dw_vec_operands(c[0] != 0, (int)c[1], (int)c[2], cb, nb, (uint64_t)c[3], (uint64_t)c[4], (int)c[5]);
  }
}
// rows[g][r][a] (4 x 4 x cb) and cols[c16][b] (16 x nb): channel inside the tile
extern "C" void host_dw_tile_maps(int vec, int cb, int nb, int32_t *rows, int32_t *cols) {
  for (int g = 0; g < 4; ++g)
    for (int r = 0; r < 4; ++r)
      for (int a = 0; a < cb; ++a) rows[(g * 4 + r) * cb + a] = aabr::dw_tile_row(vec != 0, cb, g, r, a);
  for (int c16 = 0; c16 < 16; ++c16)
    for (int b = 0; b < nb; ++b) cols[c16 * nb + b] = aabr::dw_tile_col(vec != 0, nb, c16, b);
}

#ifdef DW_VEC_HOST_MAIN
int main() {
  const int planes[] = {9, 16, 32, 33, 48, 64, 80, 96, 128, 256};
  const int64_t offs[] = {0, 4, 8, 16};
  int bad = 0;
  long n = 0;
  for (int bf = 0; bf < 2; ++bf)
    for (int ci : planes)
      for (int co : planes)
        for (int64_t oi : offs)
          for (int64_t oo : offs) {
            const int64_t c[6] = {bf, ci, co, 0x7f0000001000ll + oi, 0x7f0000002000ll + oo, aabr::kKnobUnset};
            int64_t o[3];
            host_dw_vec_operands(c, 1, o);
            const int cb = (int)o[0], nb = (int)o[1], m = (int)o[2];
            ++n;
            // a vector-loaded operand has only full tiles and an address the load's width divides
            if ((m & aabr::kDwVecIn) && (bf || cb == 1 || ci % (16 * cb) || (c[3] % (4 * cb)))) ++bad;
            if ((m & aabr::kDwVecOut) && (bf || nb == 1 || co % (16 * nb) || (c[4] % (4 * nb)))) ++bad;
            int64_t c0[6] = {bf, ci, co, c[3], c[4], 0};
            host_dw_vec_operands(c0, 1, o);
            if (o[2] != 0) ++bad;
          }
  for (int vec = 0; vec < 2; ++vec)
    for (int cb = 1; cb <= 4; cb *= 2)
      for (int nb = 1; nb <= 4; nb *= 2) {
        std::vector<int32_t> rows(16 * cb), cols(16 * nb), seen_r(16 * cb, 0), seen_c(16 * nb, 0);
        host_dw_tile_maps(vec, cb, nb, rows.data(), cols.data());
        for (int32_t v : rows) {
          if (v < 0 || v >= 16 * cb) { ++bad; continue; }
          ++seen_r[v];
        }
        for (int32_t v : cols) {
          if (v < 0 || v >= 16 * nb) { ++bad; continue; }
          ++seen_c[v];
        }
        for (int32_t v : seen_r) bad += v != 1;
        for (int32_t v : seen_c) bad += v != 1;
      }
  printf("dw_vec host harness: %ld decisions, %d violations\n", n, bad);
  return bad ? 1 : 0;
}
#endif

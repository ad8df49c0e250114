// conv_tiles.h -- which 64-row-tile kernel instance aabr_conv_forward / _bf16 launch (conv.hip only carries it out), with
// what grid.  Free of HIP headers: tests/conv_tiles_host_harness.cpp compiles it with g++ and pins the decision.
#pragma once
#include <stdint.h>
#ifndef AABR_HD
#ifdef __HIPCC__
#define AABR_HD __host__ __device__ inline
#else
#define AABR_HD static inline
#endif
#endif

namespace aabr {

constexpr int kKnobUnset = -2147483647 - 1;   // knob(): neither the environment nor aabr_set_knob gave a value
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

constexpr int kKC = 32; // channels per K-chunk: 4 lane groups x 8 consecutive channels

AABR_HD int nkc_of(int ci) { return (ci + kKC - 1) / kKC; }
AABR_HD int nnb_of(int co) { return (co + 15) / 16; }

enum TileKind { kTileWlds, kTileSmall, kTileWpipe, kTileBuf, kTileGeneric, kTileBf16 };

// knobs CONV_WLDS, CONV_SMALL, SMALL_WPB, SMALL_MAX, CONV_NBW, CONV_WPB (tuning experiments and tests; kKnobUnset = none)
struct TileKnobs { int wlds, small, small_wpb, small_max, nbw, wpb; };

// One launch: the kernel and its template arguments (0 / false where the kernel has no such argument), grid, block
// threads, dynamic LDS bytes.
//   kTileWlds    k_conv_blocks_mfma_wlds<nbw, nkc, aligned>
//   kTileSmall   k_conv_blocks_mfma_small<wpb>
//   kTileWpipe   k_conv_blocks_mfma_wpipe<nbw, wpb, true, adj>
//   kTileBuf     k_conv_blocks_mfma_buf<nbw, wpb, adj, aligned>
//   kTileGeneric k_conv_blocks_mfma<nbw, wpb, aligned>
//   kTileBf16    k_conv_blocks_mfma_bf16<nbw, wpb, kg, adj>
struct TileKernel {
  int kind, nbw, wpb, nkc, kg;
  bool aligned, adj;
};
inline bool operator==(const TileKernel &a, const TileKernel &b) {
  return a.kind == b.kind && a.nbw == b.nbw && a.wpb == b.wpb && a.nkc == b.nkc && a.kg == b.kg &&
         a.aligned == b.aligned && a.adj == b.adj;
}
struct TileLaunch {
  TileKernel k;
  int64_t grid_x, grid_y;
  int block;
  int64_t lds;
};

// WPB waves share the blocks of one 64-row tile.  Pick the split that minimises (rounds of resident workgroups) x
// (blocks per wave): a grid one workgroup larger than what fits on the chip at once would otherwise pay a whole second
// round.  `waves`: the waves per CU the kernel's registers allow (4 SIMDs); ties go to more waves.  Knob CONV_WPB forces it.
inline int tile_wpb(int64_t wgs, int vol, int nbw, int waves, int knob_wpb) {
  const int max_wpb = nbw == 4 ? 3 : 4;
  if (knob_wpb >= 2 && knob_wpb <= max_wpb) return knob_wpb;   // tuning experiments only
  int best_wpb = 2;
  int64_t best_cost = -1;
  for (int wpb = 2; wpb <= max_wpb; ++wpb) {
    int64_t per_cu = (160 * 1024) / ((int64_t)wpb * 64 * (nbw * 16) * 4);
    if (per_cu > waves / wpb) per_cu = waves / wpb;
    if (per_cu < 1) per_cu = 1;
    const int64_t cost = ceil_div(wgs, 256 * per_cu) * ceil_div(vol, wpb);
    if (best_cost < 0 || cost <= best_cost) { best_cost = cost; best_wpb = wpb; }
  }
  return best_wpb;
}

// a streaming kernel over (64-row tile, nbw-block column slab) workgroups
inline TileLaunch tile_slabs(int kind, int nbw, int wpb, int64_t V_out, int nnb) {
  return {{kind, nbw, wpb, 0, 0, false, false}, ceil_div(V_out, 64), ceil_div(nnb, nbw), 64 * wpb,
          (int64_t)wpb * 64 * (nbw * 16) * 4};
}

// fp32.  flags: bit 0 transpose, bit 1 flip, bit 2 prepacked, bits 8+ timing experiments (generic kernel only).
// in_bytes / wp_bytes / words_bytes: input features, packed weights, tile blocks.
inline TileLaunch conv_tile_launch(int n_in, int n_out, int64_t V_out, int vol, int flags, int64_t in_bytes,
                                   int64_t wp_bytes, int64_t words_bytes, const TileKnobs &kn) {
  const int nkc = nkc_of(n_in), nnb = nnb_of(n_out);
  const bool aligned = (n_in % kKC) == 0, exp = (flags >> 8) != 0;
  const int64_t T = ceil_div(V_out, 64);
  // lean buffer-descriptor kernels: every buffer below 2 GiB (32-bit offsets)
  const bool lean_any = in_bytes < (1ll << 31) && wp_bytes < (1ll << 31) && words_bytes < (1ll << 31) && !exp;
  const bool lean = aligned && lean_any;
  // LDS-resident weights: the slab's packed filter bank + enough per-wave output tiles fit in 160 KiB
  if (nkc <= 2 && in_bytes < (1ll << 31) && words_bytes < (1ll << 31) && !exp) {
    const int forced = kn.wlds == kKnobUnset ? -1 : kn.wlds;   // tuning only: 0 disables, 1/2/4 forces the slab width
    // Measured (tools_conv_bench.py, S80k and 1.5 M points): 16-column slabs with 8 waves per CU beat
    // wider slabs (fewer waves fit beside the larger filter bank) and beat the streaming kernel when the
    // layer is at least 64 planes wide; narrow layers (<= 32 output planes) stay on the streaming kernel.
    int nbw = 0, nw = 0;
    for (int cand = 1; cand <= 4; cand <<= 1) {
      if (forced > 0 ? cand != forced : (cand != 1 || nnb < 4)) continue;
      if (cand > 1 && cand / 2 >= nnb) continue; // no wider than the layer
      const int64_t w_lds = (int64_t)vol * nkc * cand * 2048, tile_lds = (int64_t)64 * cand * 16 * 4;
      int64_t fit = (160 * 1024 - w_lds) / tile_lds;
      if (fit > 8) fit = 8; // 512 threads: two waves per SIMD, 256 VGPRs each
      if (fit < 4) continue;
      nbw = cand; nw = (int)fit;
      break;
    }
    if (nbw > 0 && forced != 0) {
      const int64_t slabs = ceil_div(nnb, nbw);
      int64_t wgx = ceil_div(T, nw);
      const int64_t cap = 256 / slabs > 0 ? 256 / slabs : 1; // persistent: about one workgroup per CU
      if (wgx > cap) wgx = cap;
      // a small tile count spreads over more CUs with fewer waves each
      while (nw > 4 && wgx < cap && ceil_div(T, nw - 1) <= cap) { --nw; wgx = ceil_div(T, nw); }
      return {{kTileWlds, nbw, 0, nkc, 0, aligned, false}, wgx, slabs, 64 * nw,
              (int64_t)vol * nkc * nbw * 2048 + nw * ((int64_t)64 * nbw * 16 * 4)};
    }
  }
  // tiny rule books with wide layers (coarse FPN scales): (pair, chunk) items over 8 waves x 16-column slabs
  const int smax = kn.small_max == kKnobUnset ? 512 : kn.small_max;
  if (lean && nkc >= 2 && T * nnb < smax && kn.small != 0) {   // CONV_SMALL=0 disables
    // 16 waves per workgroup when the grid alone cannot fill the chip (each wave's chain of dependent (pair,
    // chunk) items halves; 94 VGPRs: four waves per SIMD fit): SMALL_WPB forces 8 / 16
    int wpb = T * nnb < 1024 ? 16 : 8;
    if (kn.small_wpb == 8 || kn.small_wpb == 16) wpb = kn.small_wpb;
    return {{kTileSmall, 0, wpb, 0, 0, false, false}, T, nnb, 64 * wpb, (int64_t)wpb * 64 * 16 * 4};
  }
  // widest column slab the layer allows (fewest re-gathers of the input rows) -- unless the rule book is so
  // small that the launch would leave most CUs idle (the coarse FPN scales: 1-50 tiles): then narrower
  // slabs, i.e. more and shorter workgroups; at that size the gathers are latency, not bandwidth
  int nbw = nnb <= 1 ? 1 : (nnb == 2 ? 2 : 4);
  while (nbw > 1 && T * ceil_div(nnb, nbw) < 512) nbw >>= 1;
  // throughput-bound launches: 32-column slabs of the streaming kernel (twice the waves per CU beside half
  // the private LDS tile) edge out the 64-column weight-prefetch kernel: 39.4 -> 40.3 % / 41.9 -> 42.8 % of
  // the fp32 MFMA peak at 128 / 256 planes, 1.5 M points.  So NBW 4 launches have fewer than 8192 workgroups.
  if (nbw == 4 && T * ceil_div(nnb, 4) >= 8192) nbw = 2;
  if ((kn.nbw == 1 || kn.nbw == 2 || kn.nbw == 4) && kn.nbw <= nbw) nbw = kn.nbw;   // tuning experiments only
  // register budget: 3 (164 VGPRs, weight prefetch) resp. 5 waves per SIMD
  const int wpb = tile_wpb(T * ceil_div(nnb, nbw), vol, nbw, nbw == 4 ? 12 : 20, kn.wpb);
  TileLaunch t = tile_slabs(kTileGeneric, nbw, wpb, V_out, nnb);
  if (lean && nbw == 4) {           // weight prefetch; no adjacent-pair sharing (it pays from 8192 workgroups, see above)
    t.k.kind = kTileWpipe;
    return t;
  }
  t.k.aligned = aligned;
  if (lean_any) {                   // element gathers when the plane count is not a multiple of 32
    t.k.kind = kTileBuf;
    t.k.adj = true;                 // adjacent-pair weight sharing pays at every size in the streaming kernel
  }
  return t;                         // generic: flat 64-bit addressing, timing experiments
}

// bf16 storage: the same inputs; plane counts are multiples of 32 and every buffer is below 2 GiB (the entry point
// checks both), so neither the flags nor the byte sizes change the choice
inline TileLaunch conv_tile_launch_bf16(int n_in, int n_out, int64_t V_out, int vol, int /*flags*/, int64_t /*in_bytes*/,
                                        int64_t /*wp_bytes*/, int64_t /*words_bytes*/, const TileKnobs &kn) {
  const int nkc = nkc_of(n_in), nnb = nnb_of(n_out);
  const int64_t T = ceil_div(V_out, 64);
  int nbw = nnb == 2 ? 2 : 4;
  if (nbw == 4 && T * ceil_div(nnb, 4) < 512) nbw = 2; // small rule book: more, shorter workgroups
  if ((kn.nbw == 2 || kn.nbw == 4) && kn.nbw <= nbw) nbw = kn.nbw;   // tuning experiments only
  TileLaunch t = tile_slabs(kTileBf16, nbw, tile_wpb(T * ceil_div(nnb, nbw), vol, nbw, 16, kn.wpb), V_out, nnb);
  t.k.kg = nkc >= 3 ? 4 : nkc;
  t.k.adj = true;
  return t;
}

} // namespace aabr

// conv_wide_tiles.h -- what the wide kernel k_conv_cs is launched with (conv_wide.hip only carries it out): rows per tile,
// offset split, kernel instance (channel groups, stage buffers, slab width), grid, LDS bytes and the wflip word, for both
// feature storages.  Free of HIP headers: tests/conv_wide_host_harness.cpp compiles it with g++ and pins the decision.
#pragma once
#include <stdint.h>
#include "conv_tiles.h"   // ceil_div, kKnobUnset

namespace aabr {

constexpr int kWS = 64;            // tile row stride in floats = slab width
constexpr int kMaxVol = 63;        // vol + 1 prefix entries live in the lanes of one VGPR
constexpr int kMaxTileRows = 240;  // (240 + 1) rows x 256 B + 16 KiB stage = 76 KiB: two workgroups per CU
#ifdef AABR_DEV
constexpr bool kWideDev = true;    // `make DEV=1`: the timing-experiment variants (flags >> 8) are compiled
#else
constexpr bool kWideDev = false;
#endif

inline int64_t wide_words(int64_t V, int vol, int T) {
  const int64_t nt = (V + T - 1) / T;
  return nt * (vol + 1) + nt * (int64_t)(T / 16) * vol * 16;
}

// knobs WIDE_ROWS, CONV_WIDE, CONV_WIDE_BF16, WIDE_SPLIT, SPLIT_ROWS, SPLIT_MIN_ITEMS, SPLIT_TARGET, WIDE_NBUF, SPLIT_NBUF,
// WIDE_NCB, WIDE_PRIO (tuning experiments and tests; kKnobUnset = none)
struct WideKnobs {
  int wide_rows, conv_wide, conv_wide_bf16, wide_split, split_rows, split_min_items, split_target, wide_nbuf, split_nbuf,
      wide_ncb, wide_prio;
};

// The two feature storages.  bf16 rows hold 64 channels per 128-byte chunk where fp32 rows hold 32, so every channel
// count of the kernel doubles; a packed 32-channel x 16-column weight block halves.
enum WideStorage { kWideF32 = 0, kWideBf16 = 1 };
struct WideStorageDesc {
  int elem;        // bytes per stored feature
  int chunk;       // channels per 128-byte row chunk: n_in is a multiple of it
  int group;       // channels of the largest channel group (4 chunks): above it n_in is a multiple of it, so that
                   // every load of the inner loop is unconditional
  int wp_block;    // bytes of one packed weight block
  int res_align;   // alignment of the residual rows the write-out reads (four features)
  const char *planes_msg, *group_msg;
};
inline const WideStorageDesc &wide_storage(int storage) {
  static const WideStorageDesc d[2] = {
      {4, 32, 128, 2048, 16, "plane counts: n_in % 32, n_out % 64", "n_in above 128 must be a multiple of 128"},
      {2, 64, 256, 1024, 8, "plane counts: n_in % 64, n_out % 64", "n_in above 256 must be a multiple of 256"}};
  return d[storage == kWideBf16];
}
inline int64_t wide_wp_bytes(const WideStorageDesc &s, int n_in, int n_out, int vol) {
  return (int64_t)vol * (n_in / 32) * (n_out / 16) * s.wp_block;
}

// 16-column blocks per wave: 1 = 64-column slabs.  bf16 storage takes 2 (128-column slabs) for n_out % 128 == 0 up to 128
// input channels (two weight register sets of 16 x NCB x KG registers); WIDE_NCB knob: 1 forces 64-column slabs
inline int wide_ncb(int storage, int n_in, int n_out, const WideKnobs &kn) {
  if (storage != kWideBf16 || kn.wide_ncb == 1) return 1;
  return ((n_out & 127) == 0 && n_in <= 128) ? 2 : 1;
}

// rows per tile before the one-round rule and the knobs
inline int wide_default_rows(int storage, int n_in, int ncb) {
  // fp32: 128, except: up to 64 input channels (channel groups of 32 / 64: 8 KiB of stage, ~100 registers) 112-row tiles
  // with a single stage buffer fit FOUR workgroups per CU (36.9 KiB each): 64->64 at 200k rows 204 -> 190 us, at 282k rows
  // 180 -> 171 (round 4, measured with AABR_WIDE_NBUF / AABR_WIDE_ROWS); 128-channel groups stay at 128 rows / three per CU
  if (storage != kWideBf16) return n_in <= 64 ? 112 : 128;
  // bf16: two MFMAs per block and 64-channel chunk -- the gather / stage / barrier skeleton sets the pace, so more
  // resident workgroups pay: 96-row tiles with a single stage buffer (measured on the bench's rule books: convolution
  // time of a bf16 step 5.25 -> 5.01 ms against 128 rows + two buffers; 64 rows: 5.24)
  // 128-column slabs when the layer has them: the kernel is bound by the CU's random-row gather rate and a 64-column
  // slab gathers every row once per slab.  Their fp32 tile is 512 B per row: 64 rows (33 KiB + 8 KiB of stage) keep
  // three workgroups per CU; 64-column slabs keep the 96-row tiles of round 2.
  return ncb == 2 ? 64 : 96;
}

// what both dispatch queries refuse: shapes the kernel or its 32-bit buffer offsets cannot serve
inline bool wide_supported(const WideStorageDesc &s, int n_in, int n_out, int64_t rows_in, int vol) {
  if (n_in <= 0 || n_out <= 0 || (n_in % s.chunk) || (n_out & 63) || vol <= 0 || vol > kMaxVol) return false;
  if (rows_in >= (1ll << 23) || rows_in * n_in * s.elem >= (1ll << 31)) return false;
  return n_in <= s.group || (n_in % s.group) == 0;
}

// 0: use the 64-row-tile kernels of conv.hip; otherwise rows per tile of the block stream the wide launch wants
inline int wide_tile_rows(int storage, int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, const WideKnobs &kn) {
  const WideStorageDesc &s = wide_storage(storage);
  if (!wide_supported(s, n_in, n_out, rows_in, vol)) return 0;
  const int ncb = wide_ncb(storage, n_in, n_out, kn);
  const int64_t slabs = n_out / (64 * ncb);
  // the default, except when the whole launch fits the chip in ONE round (512 resident workgroups, 2 per
  // CU): then its time is the longest workgroup, so take the smallest tile (>= 64 rows) that still fits one round
  // (measured, profiles/r02_conv_wide_ab.txt: 22k rows x 2 slabs, 128 -> 96 rows: 184 -> 133 us; with several rounds
  // smaller tiles only lower the block fill: 84k rows 385 -> 400 us)
  int T = wide_default_rows(storage, n_in, ncb);
  if (ceil_div(V_out, T) * slabs <= 512)
    for (int t = 64; t < T; t += 16)
      if (ceil_div(V_out, t) * slabs <= 512) { T = t; break; }
  if (kn.wide_rows >= 16 && kn.wide_rows <= kMaxTileRows && (kn.wide_rows & 15) == 0) T = kn.wide_rows;   // tuning experiments only
  if (wide_words(V_out, vol, T) * 4 >= (1ll << 31)) return 0;
  if (wide_wp_bytes(s, n_in, n_out, vol) >= (1ll << 31)) return 0;
  {                                                // tuning experiments / tests only: 0 = never, 1 = whenever supported
    const int v = storage == kWideBf16 ? kn.conv_wide_bf16 : kn.conv_wide;
    if (v == 0) return 0;
    if (v == 1) return T;
  }
  // enough workgroups to fill the chip twice over (measured, profiles/r02_conv_wide_ab.txt: wins from ~340
  // workgroups up, loses below ~180)
  return ceil_div(V_out, T) * slabs >= 320 ? T : 0;
}

// (P << 16) | tile_rows when this launch should go to the offset split (conv_wide.hip), else 0.  Asked after
// wide_tile_rows declined (fewer than 320 (tile, slab) items).
inline int wide_split(int storage, int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, const WideKnobs &kn) {
  const WideStorageDesc &s = wide_storage(storage);
  if (!wide_supported(s, n_in, n_out, rows_in, vol) || vol <= 1 || V_out <= 0 || n_in < 64) return 0;
  if (kn.wide_split == 0) return 0;
  // CONV_WIDE_BF16 = 0 keeps bf16 launches off the split as well; CONV_WIDE = 0 leaves the fp32 split on
  if (storage == kWideBf16 && kn.conv_wide_bf16 == 0) return 0;
  if (ceil_div(V_out, 64) * (n_out / 64) >= 320) return 0;
  // fp32, round 5: 96-row tiles from ~1 k rows on (5,565 rows 54 -> 49 us, 1,382 rows 57 -> 53; 332 rows 27 vs 29)
  int T = (storage != kWideBf16 && V_out >= 1024) ? 96 : 64;
  if (kn.split_rows >= 64 && kn.split_rows <= 128 && (kn.split_rows & 15) == 0) T = kn.split_rows;   // (A/B)
  const int64_t items = ceil_div(V_out, T) * (n_out / 64);
  const int min_items = kn.split_min_items == kKnobUnset ? 8 : kn.split_min_items;   // below: the 16-column item kernel wins
  if (items < min_items) return 0;
  // workgroups aimed at (round 5: 512 .. 1536 re-measured; 768 and 1280 best by ~3 %)
  // (bf16: 768 / 1024 / 1280 -> 1156 / 1192 / 1204 us of coarse-scale convolutions per step)
  const int target = kn.split_target == kKnobUnset ? 768 : kn.split_target;
  int P = (int)((target + items - 1) / items);
  if (P > vol) P = vol;
  if (P > 32) P = 32;
  if (kn.wide_split >= 2 && kn.wide_split <= 32) P = kn.wide_split < vol ? kn.wide_split : vol;   // tuning experiments only
  if (P < 2) return 0;
  if (wide_words(V_out, vol, T) * 4 >= (1ll << 31) || wide_wp_bytes(s, n_in, n_out, vol) >= (1ll << 31)) return 0;
  return (P << 16) | T;
}

// k_conv_cs<kg, dbg, nbuf, bf16, ncb>; `split`: the launch writes partial tiles for k_split_reduce (same instance, its
// own name in aabr_conv_last_variant)
struct WideKernel {
  int kg, dbg, nbuf;
  bool bf16;
  int ncb;
  bool split;
};
inline bool operator==(const WideKernel &a, const WideKernel &b) {
  return a.kg == b.kg && a.dbg == b.dbg && a.nbuf == b.nbuf && a.bf16 == b.bf16 && a.ncb == b.ncb && a.split == b.split;
}
struct WideLaunch {
  WideKernel k;
  int64_t grid_x, grid_y;
  int64_t lds_bytes;
  int wflip;       // bit 0: flipped filter, bit 1: raised wave priority in the matrix phase, bits 8..15: parts of a split
  int64_t in_bytes, words_bytes, wp_bytes;
};

// One launch of k_conv_cs.  parts == 0: the plain launch; otherwise the offset split in `parts` parts.  Returns nullptr or
// the first violated condition; V_out == 0 is no error and leaves `out` zero (nothing to launch), as a refusal does.
inline const char *wide_launch(int storage, int parts, int n_in, int n_out, int64_t rows_in, int64_t V_out, int tile_rows,
                               int vol, int flags, bool has_stats, const WideKnobs &kn, WideLaunch &out) {
  const WideStorageDesc &s = wide_storage(storage);
  const bool bf16 = storage == kWideBf16, split = parts != 0;
  out = WideLaunch{};   // what a refusal and V_out == 0 leave
  WideLaunch t{};
  if (split && !(parts >= 2 && parts <= 32 && parts <= vol))
    return "2 <= parts <= min(32, vol) and a 16-byte aligned scratch of parts x V_out x n_out floats";
  if (has_stats && tile_rows < 64) return "statistics need tiles of >= 64 rows";
  if (!(n_in > 0 && n_out > 0 && (n_in % s.chunk) == 0 && (n_out & 63) == 0)) return s.planes_msg;
  if (!(vol > 0 && vol <= kMaxVol && V_out >= 0 && rows_in >= 0)) return "bad sizes";
  if (!(tile_rows >= 16 && tile_rows <= kMaxTileRows && (tile_rows & 15) == 0)) return "tile_rows: multiple of 16, <= 240";
  if (V_out == 0) return nullptr;
  if (rows_in <= 0) return "null pointer / empty input";
  if (rows_in >= (1ll << 23)) return "too many input rows for the wide block format";
  t.in_bytes = rows_in * n_in * s.elem;
  t.words_bytes = wide_words(V_out, vol, tile_rows) * 4;
  if (!(t.in_bytes < (1ll << 31) && t.words_bytes < (1ll << 31))) return "buffers must be < 2 GiB";
  t.wp_bytes = wide_wp_bytes(s, n_in, n_out, vol);
  if (t.wp_bytes >= (1ll << 31)) return "packed weights must be < 2 GiB";
  if (n_in > s.group && (n_in % s.group)) return s.group_msg;
  const int nkc = n_in / s.chunk, kg = nkc >= 4 ? 4 : nkc;
  // the fp32 split compiles no 32-channel instance (aabr_conv_wide_split never asks for one: n_in >= 64)
  if (split && !bf16 && kg < 2) return "the fp32 offset split needs n_in >= 64";
  const int exp = flags >> 8;   // timing experiments (tools/, `make DEV=1`)
  int dbg = 0;
  if (!split && !bf16 && (exp & 7)) {   // only the 128-channel-group instance carries the debug variants
    if (!kWideDev) return "the timing-experiment variants of k_conv_cs exist in a `make DEV=1` build only";
    if (kg != 4) return "debug variants exist for n_in >= 128 only";
    dbg = (exp & 4) ? 4 : (exp & 3);
  }
  if (!split && bf16 && kWideDev && (exp & 4)) {   // tools/tools_cs_phases.py bf16: phase clocks of the 128-channel instance
    if (kg != 2) return "the bf16 phase-clock variant exists for n_in = 128 only";
    dbg = 4;
  }
  // LDS stage buffers, one decision per family:
  int nbuf = 1;
  if (split) {
    // single stage buffer: three workgroups per CU (latency-bound launches, profiles/r04_conv_split_ab.txt: -10 %).  The fp32
    // split follows SPLIT_NBUF; the bf16 split compiles the single-buffer instances only.
    if (!bf16 && kn.split_nbuf == 2) nbuf = 2;
  } else {
    // fp32: with 128-channel groups the double-buffered stage (32 KiB) allows two workgroups per CU, a
    // single buffer three (49 KiB each) at the price of a second barrier per pair: measured +4...+10 % (128->128 at 84k
    // rows 380 -> 367 us, 256->256 1366 -> 1272 us); narrower groups fit three workgroups with the double buffer;
    // kg <= 2: single buffer + 112-row tiles = four workgroups per CU (wide_default_rows).  bf16: always one (ibid.)
    if (!bf16) nbuf = (kg == 4 || kg <= 2) ? 1 : 2;
    if (kn.wide_nbuf == 1 || kn.wide_nbuf == 2) nbuf = kn.wide_nbuf;   // tuning experiments only
    if (dbg) nbuf = bf16 ? 1 : 2;   // the debug variants run with these buffers whatever the knob says
  }
  const int ncb = split ? 1 : wide_ncb(storage, n_in, n_out, kn);
  t.k = WideKernel{kg, dbg, nbuf, bf16, ncb, split};
  t.grid_x = ceil_div(V_out, tile_rows);
  t.grid_y = (int64_t)(n_out / (64 * ncb)) * (split ? parts : 1);
  t.lds_bytes = ((int64_t)(tile_rows + 1) * kWS * ncb + nbuf * 2 * 16 * kg * 32) * 4;
  // bit 1: the waves raise their priority for the matrix phase of a step (s_setprio): the wave that holds its operands
  // gets the pipe, the others issue their gathers -- measured 331 -> 323.5 us on the dominant instance.  fp32 (plain and
  // split): on unless WIDE_PRIO is 0.  bf16: only on request (WIDE_PRIO = 1); the bf16 split: never.
  const bool prio = bf16 ? (!split && kn.wide_prio == 1) : kn.wide_prio != 0;
  t.wflip = ((flags >> 1) & 1) | (prio ? 2 : 0) | (parts << 8);
  out = t;
  return nullptr;
}

} // namespace aabr

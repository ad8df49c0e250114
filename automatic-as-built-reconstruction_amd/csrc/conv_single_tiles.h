// conv_single_tiles.h -- when a forward-form launch whose rule book gives every output row EXACTLY ONE rule goes to
// k_conv_single (conv_single.hip only carries it out), and what that kernel is launched with: shape conditions, the least
// number of output rows, pairs per chunk, grid, LDS bytes.  Free of HIP headers: tests/conv_single_host_harness.cpp compiles
// it with g++ and pins the decision.  The one-rule property itself is the CALLER's knowledge (a 1x1x1 submanifold
// convolution, a deconvolution with filter == stride, the input gradient of a convolution with filter == stride): nothing
// here can see it.
// Two decisions: `single_refusal` / `single_launch` for the plain launch (k_conv_single<KG>), whose `has_stats` means
// FORWARD statistics -- the following BatchNorm's sums of the stored values, which the kernel does not form -- and, since
// that flag cannot tell the two apart, is also what a caller without the backward form passes for backward ones; and
// `single_bwd_stats_refusal` / `single_bwd_stats_launch` for the input-gradient launch whose write-out forms the BACKWARD
// statistics of the BatchNorm whose d_out it writes (k_conv_single<KG, true>: one fp64 part per chunk).
#pragma once
#include <stdint.h>
#include "conv_tiles.h"   // ceil_div, kKnobUnset

namespace aabr {

// Least number of output rows for the route to be taken by default (SINGLE_ROWS knob: another value, 0 = every book).
// From the A/B of both routes on every qualifying rule book of the bench workload (profiles/conv_single_ab.txt): every
// launch wins from 84k rows up (deconvolutions 1.6 - 1.9x, laterals 1.15 - 1.3x); at 22k rows the deconvolution wins 7 us
// and each lateral loses 2; below, the laterals lose to the 64-row-tile kernels.  From 32,768 rows up the launch this
// route replaces is always a k_conv_cs one (conv_wide_tiles.h: >= 320 workgroups), so results stay what they were.
constexpr int64_t kSingleMinRows = 32768;
constexpr int kSingleStepPairs = 32;   // pairs the workgroup gathers and multiplies per pipeline step (two 16-pair blocks)

// knobs CONV_SINGLE (0: route off; 1: on; unset: the shipped default), SINGLE_ROWS, SINGLE_CHUNK (1024: the pair list's
// longer chunks) -- A/B runs and tests; kKnobUnset = none
struct SingleKnobs {
  int conv_single, single_rows, single_chunk;
};
constexpr bool kSingleDefaultOn = true;   // what an unset CONV_SINGLE means

// The shapes the kernel serves, or the first condition violated.  fp32 storage; `has_stats`: forward statistics wanted in
// the write-out (see above; the backward form has its own decision below).
inline const char *single_unsupported(bool bf16, bool has_stats, int n_in, int n_out, int64_t rows_in, int64_t rows_out,
                                      int vol) {
  if (bf16) return "fp32 storage only (bf16 rows stay on their kernels)";
  if (has_stats) return "no BatchNorm statistics in the write-out (their partial sums are per tile of k_conv_cs)";
  if (!(n_in > 0 && n_out > 0 && vol > 0 && vol <= 65535 && rows_in >= 0 && rows_out >= 0)) return "bad sizes";
  if (n_in > 128) return "n_in <= 128 (the offset's weight slice stays in registers)";
  if (n_out % 64) return "n_out must be a multiple of 64";
  if (n_in % 32) return "n_in must be a multiple of 32";
  if (rows_in >= (1ll << 23) || rows_in * n_in * 4 >= (1ll << 31)) return "input rows must be < 2^23 and < 2 GiB";
  if (rows_out >= (1ll << 25)) return "too many output rows for the pair list";
  if ((int64_t)vol * (n_in / 32) * (n_out / 16) * 2048 >= (1ll << 31)) return "packed weights must be < 2 GiB";
  return nullptr;
}

// Pairs per chunk: one of the two chunk tables the pair list carries.  256: measured ahead of 1024 on every book of the
// bench workload (ibid.: 309k rows 123 vs 138 us, 84k rows 39 vs 57) -- four workgroups per CU hide a chunk's weight load
// behind the others' steps, and 1024-pair chunks leave the chip with 2.4 workgroups per CU at best, a ragged last round.
inline int single_chunk_pairs(const SingleKnobs &kn) { return kn.single_chunk == 1024 ? 1024 : 256; }
// Upper bound on the chunks of a one-rule-per-row book, without reading its counts: the offsets share rows_out pairs, and
// every offset adds at most one partly filled chunk.  Workgroups past the true count exit at once.
inline int64_t single_chunk_bound(int64_t rows_out, int vol, int chunk_pairs) { return rows_out / chunk_pairs + vol; }

// The decision `SCN.single_route` reads: nullptr = take the route, else why not.
inline const char *single_refusal(bool bf16, bool has_stats, int n_in, int n_out, int64_t rows_in, int64_t rows_out, int vol,
                                  const SingleKnobs &kn) {
  if (kn.conv_single == 0 || (kn.conv_single == kKnobUnset && !kSingleDefaultOn)) return "CONV_SINGLE is off";
  if (const char *m = single_unsupported(bf16, has_stats, n_in, n_out, rows_in, rows_out, vol)) return m;
  if (rows_out == 0) return "no output rows";
  const int64_t min_rows = kn.single_rows == kKnobUnset ? kSingleMinRows : kn.single_rows;
  if (rows_out < min_rows) return "too few output rows: k_conv_cs or its offset split is faster";
  return nullptr;
}

struct SingleLaunch {
  int kg;                // 32-channel chunks per input row = the kernel instance
  int chunk_pairs;
  int64_t grid_x, grid_y;
  int64_t lds_bytes;     // the double-buffered stage: 2 x 32 rows x n_in floats
  int wflip;             // bit 0: flipped filter
  int64_t in_bytes, wp_bytes;
};

// One launch of k_conv_single<kg>.  Returns nullptr or the first violated condition; rows_out == 0 is no error (nothing to
// launch).  The row threshold is the route's, not the kernel's: an entry point called directly serves any supported book.
inline const char *single_launch(int n_in, int n_out, int64_t rows_in, int64_t rows_out, int vol, int flags,
                                 const SingleKnobs &kn, SingleLaunch &out) {
  out = SingleLaunch{};
  if (const char *m = single_unsupported(false, false, n_in, n_out, rows_in, rows_out, vol)) return m;
  if (rows_out == 0) return nullptr;
  if (rows_in <= 0) return "null pointer / empty input";
  SingleLaunch t{};
  t.kg = n_in / 32;
  t.chunk_pairs = single_chunk_pairs(kn);
  t.grid_x = single_chunk_bound(rows_out, vol, t.chunk_pairs);
  t.grid_y = n_out / 64;
  if (t.grid_x * t.grid_y >= (1ll << 31)) return "too many workgroups";
  t.lds_bytes = 2ll * kSingleStepPairs * n_in * 4;
  t.wflip = (flags >> 1) & 1;
  t.in_bytes = rows_in * n_in * 4;
  t.wp_bytes = (int64_t)vol * (n_in / 32) * (n_out / 16) * 2048;
  out = t;
  return nullptr;
}

// ---- the backward-statistics form -------------------------------------------------------------------------------------
// knob SINGLE_BWD_STATS (0: off, 1: on, unset: the shipped default); everything else -- CONV_SINGLE, the row threshold,
// the chunk length -- is the plain route's.  On: with the route the fp32 training step took 12.085 - 12.125 ms against
// 12.216 - 12.240 without, four runs each, interleaved on one GPU (profiles/conv_single_bwd_stats_bench_lines.txt).
constexpr bool kSingleBwdStatsDefaultOn = true;

// nullptr = the input-gradient launch that owes a BatchNorm its backward statistics goes to k_conv_single<KG, true>, else
// why not: every condition of the plain route but the statistics one.
inline const char *single_bwd_stats_refusal(bool bf16, int n_in, int n_out, int64_t rows_in, int64_t rows_out, int vol,
                                            const SingleKnobs &kn, int bwd_stats_knob) {
  if (bwd_stats_knob == 0 || (bwd_stats_knob == kKnobUnset && !kSingleBwdStatsDefaultOn)) return "SINGLE_BWD_STATS is off";
  return single_refusal(bf16, false, n_in, n_out, rows_in, rows_out, vol, kn);
}

struct SingleBwdStatsLaunch {
  SingleLaunch l;         // grid, chunk length, weight orientation as the plain launch; lds_bytes also holds the sums
  int64_t parts;          // fp64 parts [2][n_out] the launch writes = grid_x: one per chunk, surplus chunks write zeros
  int64_t stats_doubles;  // parts x 2 x n_out
};
constexpr int64_t kSingleReduceBytes = 256 * 8 * 8;   // a workgroup's 256 x 8 fp64 sums, combined through LDS after the last step

inline const char *single_bwd_stats_launch(int n_in, int n_out, int64_t rows_in, int64_t rows_out, int vol, int flags,
                                           const SingleKnobs &kn, SingleBwdStatsLaunch &out) {
  out = SingleBwdStatsLaunch{};
  if (const char *m = single_launch(n_in, n_out, rows_in, rows_out, vol, flags, kn, out.l)) return m;
  if (rows_out == 0) return nullptr;
  if (out.l.lds_bytes < kSingleReduceBytes) out.l.lds_bytes = kSingleReduceBytes;
  out.parts = single_chunk_bound(rows_out, vol, out.l.chunk_pairs);
  out.stats_doubles = out.parts * 2 * n_out;
  return nullptr;
}

} // namespace aabr

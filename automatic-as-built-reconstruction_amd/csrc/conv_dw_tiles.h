// conv_dw_tiles.h -- which weight-gradient kernel instance aabr_conv_backward_weight / _bf16 launch (conv_dw.hip only
// carries it out), with what grid, and which reduce follows.  Free of HIP headers: tests/conv_dw_host_harness.cpp
// compiles it with g++ and pins the decision.
#pragma once
#include <stdint.h>
#include "conv_tiles.h"   // AABR_HD, kKnobUnset, ceil_div, nnb_of

namespace aabr {

// pairs per weight-gradient chunk (one workgroup = 4 waves x chunk/4).  1024 keeps the partial-sum
// traffic small (a partial is nIn*nOut floats per chunk); 256 gives a small rule book ~4x more workgroups
// than CUs -- at 1024 the S80k launch ran one wave per SIMD and was pure gather latency.  Both chunk tables
// are compiled into the pair list; the launch picks by rule-book size and layer width.
AABR_HD int dw_chunk(int64_t V, int vol, int n_in, int n_out) {
  return ((int64_t)vol * V <= (1ll << 21) && (int64_t)n_in * n_out <= 64 * 64) ? 256 : 1024;
}

// knobs DW_FULL, DW_FULL_MIN, DW_FULL_WGS (A/B experiments and tests; kKnobUnset = none)
struct DwKnobs { int full, full_min, full_wgs; };

enum DwKind { kDwPairs, kDwPairsMfma, kDwFull };
enum DwReduce { kDwReduceNone, kDwReduceChunks, kDwReduceRanges };

// One kernel instance: the kernel, its storage type and its template arguments (0 where the kernel has none).
//   kDwPairs      k_conv_dw_pairs<cb, nb, float | bf16>   one 64 x 64 block (cb x nb blocks of 16) of dW per workgroup
//   kDwPairsMfma  k_conv_dw_pairs_bf16<cb, nb>            the same on bf16 MFMA with LDS-transposed operands
//   kDwFull       k_conv_dw_full_f32 / _bf16              whole 128 x 128 blocks
struct DwKernel {
  int kind;
  bool bf16;
  int cb, nb;
};
inline bool operator==(const DwKernel &a, const DwKernel &b) {
  return a.kind == b.kind && a.bf16 == b.bf16 && a.cb == b.cb && a.nb == b.nb;
}
// One launch: the kernel with its grid, then `reduce` (kDwReduceNone: the kernel wrote dW itself; kDwReduceChunks:
// k_conv_dw_reduce over chunk_pairs-pair chunks; kDwReduceRanges: k_conv_dw_reduce_ranges over n_wg workgroups' ranges).
// to_scratch: the kernel writes partial blocks into the caller's scratch buffer, not dW.  tiles: 64 x 64-block tiles of
// dW, what the entry point bounds by 65535 whichever kernel runs.
struct DwLaunch {
  DwKernel k;
  int chunk_pairs, direct;
  int64_t grid_x, grid_y;
  int n_wg;
  int reduce;
  bool to_scratch;
  int tiles;
};

// bf16 rows of 32-plane multiples at 16-byte-aligned addresses: bf16 MFMA with LDS-transposed operands
inline bool dw_mfma16(bool bf16, int n_in, int n_out, bool aligned16) {
  return bf16 && n_in % 32 == 0 && n_out % 32 == 0 && aligned16;
}

// the full-tile kernels (k_conv_dw_full_*): whole 128 x 128 blocks, 16-byte row loads; knob DW_FULL = 0 keeps the
// 64 x 64-block kernels (A/B)
// Returns the number of workgroups per 128 x 128 block, or 0 when the 64 x 64-block kernels should run.  Measured on
// the bench's rule books (tools/tools_dw_ab.py): the full-tile kernels win from ~250 k rules on and lose below (few, heavy
// workgroups: latency-bound); a workgroup count that is a multiple of the 256 CUs (every CU the same number of equal
// ranges) beats anything in between by 10-25 %; two per CU pay from ~600 k rules.  The rule count is on the device: it
// is estimated from the table's size (a 3^3 submanifold table of a scene is about a third full, vol 1 is full).
inline int dw_full_workgroups(int ci, int co, bool aligned16, int64_t max_chunks, int vol, int64_t V_out, bool bf,
                              const DwKnobs &kn) {
  if (ci % 128 || co % 128 || !aligned16 || kn.full == 0) return 0;
  const int tiles = (ci >> 7) * (co >> 7);
  const int64_t slots = max_chunks - vol;                  // n_wg + vol partial blocks must fit the caller's scratch buffer
  const int knob_min = kn.full_min, knob_wgs = kn.full_wgs;
  if (knob_wgs > 0) return knob_wgs <= slots ? knob_wgs : 0;             // (A/B: a given number of workgroups)
  if (knob_min > 0) {                                                    // (tests: small rule books through the kernel)
    const int64_t n = slots < 256 / tiles ? slots : 256 / tiles;
    return n >= knob_min ? (int)n : 0;
  }
  const int64_t r_est = vol == 1 ? V_out : (int64_t)vol * V_out / 3;
  if (r_est < (bf ? 150000 : 250000)) return 0;            // (bf16: 232 k rules 46 -> 38 us; fp32: 112 -> 116)
  int64_t n = (r_est >= 600000 ? 512 : 256) / tiles;
  if (n > slots) n = 256 / tiles;
  return n >= 1 && n <= slots ? (int)n : 0;
}
inline void dw_tiling(int ci, int co, int &cb, int &nb, int &tiles) {
  int ncb = nnb_of(ci), nnb = nnb_of(co);
  cb = ncb >= 4 ? 4 : (ncb >= 2 ? 2 : 1);
  nb = nnb >= 4 ? 4 : (nnb >= 2 ? 2 : 1);
  tiles = (int)(ceil_div(ncb, cb) * ceil_div(nnb, nb));
}

// ---- k_conv_dw_pairs<cb, nb, float>: which operand rows are gathered with one load per lane ------------------------------
// The MFMA's row index is only a name for a channel.  Scalar form: lane (g, c16) loads channel 16 a + c16 of block a, one
// dword per block -- a 64-channel row slice is four load instructions of half a cache line per row each.  Vector form:
// the lane loads the cb CONSECUTIVE channels cb c16 + a, a = 0 .. cb-1, in one instruction (dwordx4 / dwordx2) and register
// a is block a's operand as before, so block a holds the channels {cb i + a} instead of {16 a + i}.  Every element of dW
// is still the sum over the same pairs in the same wave, step and k-slot of the same MFMA chain: bit-identical, only the
// accumulator that holds it differs, and the write-out maps back.  The same for the output gradients with nb.
// An operand is vector-loaded when every tile is full (planes a multiple of 16 cb: no channel masks) and its pointer is
// aligned to the load (4 cb bytes); fp32 storage only; cb = 1 is the scalar form by construction.
enum { kDwVecIn = 1, kDwVecOut = 2 };
// align_in / align_dout: the pointers' addresses (or their low four bits).  knob_vec: DW_VEC (0: scalar form everywhere)
inline int dw_vec_operands(bool bf16, int n_in, int n_out, int cb, int nb, uint64_t align_in, uint64_t align_dout,
                           int knob_vec = kKnobUnset) {
  if (bf16 || knob_vec == 0) return 0;
  int m = 0;
  if (cb > 1 && n_in % (16 * cb) == 0 && align_in % (4 * cb) == 0) m |= kDwVecIn;
  if (nb > 1 && n_out % (16 * nb) == 0 && align_dout % (4 * nb) == 0) m |= kDwVecOut;
  return m;
}
// Channel (row of dW / column of dW) inside the workgroup's tile of 16 cb x 16 nb that accumulator register r of block
// (a, b) holds in lane (g, c16): the MFMA's D[i = 4 g + r][j = c16].
AABR_HD int dw_tile_row(bool vec, int cb, int g, int r, int a) { return vec ? cb * (4 * g + r) + a : 16 * a + 4 * g + r; }
AABR_HD int dw_tile_col(bool vec, int nb, int c16, int b) { return vec ? nb * c16 + b : 16 * b + c16; }

// aligned16: both feature pointers (input features, output gradients) are 16-byte aligned.  V_out > 0, max_chunks > 0.
inline DwLaunch conv_dw_launch(bool bf16, int n_in, int n_out, int64_t V_out, int vol, int64_t max_chunks, bool aligned16,
                               const DwKnobs &kn) {
  DwLaunch d{};
  dw_tiling(n_in, n_out, d.k.cb, d.k.nb, d.tiles);         // (mfma16: 2 or 4 column blocks each way)
  d.chunk_pairs = dw_chunk(V_out, vol, n_in, n_out);
  // an offset has at most V_out rules: with V_out <= chunk_pairs every offset is one chunk at most, workgroup x is offset
  // x, writes dW[x] itself and no reduce follows
  d.direct = V_out <= d.chunk_pairs ? 1 : 0;
  d.n_wg = d.direct ? 0 : dw_full_workgroups(n_in, n_out, aligned16, max_chunks, vol, V_out, bf16, kn);
  d.to_scratch = !d.direct;
  if (d.n_wg) {                                             // (bf16: only where mfma16 holds)
    d.k = {kDwFull, bf16, 0, 0};
    d.grid_x = d.n_wg;
    d.grid_y = (n_in >> 7) * (n_out >> 7);
    d.reduce = kDwReduceRanges;
    return d;
  }
  d.k.kind = dw_mfma16(bf16, n_in, n_out, aligned16) && d.k.cb > 1 && d.k.nb > 1 ? kDwPairsMfma : kDwPairs;
  d.k.bf16 = bf16;
  d.grid_x = d.direct ? vol : max_chunks;
  d.grid_y = d.tiles;
  d.reduce = d.direct ? kDwReduceNone : kDwReduceChunks;
  return d;
}

} // namespace aabr

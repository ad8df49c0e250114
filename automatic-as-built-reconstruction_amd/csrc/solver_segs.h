// solver_segs.h -- the host side of the fused SGD step (solver.hip): the cutter that turns the parameter segments of a
// flat buffer into the chunk table the kernel strides over, and the argument checks of the step entry.  No HIP in here
// (the style of anchor_list.h's host part and conv_tiles.h), so a stand-alone program can run all of it under the host
// sanitizers (tests/solver_segs_host_harness.cpp).
//
// A parameter is a segment (flat offset, numel, group); a group is one (lr, weight_decay) pair.  A chunk is at most
// kSgdChunkElems consecutive elements of ONE segment.  Every cut INSIDE a segment lies on a multiple of 4 elements of the
// flat offset: the first chunk of a segment runs from the segment's start to the last multiple of 4 within
// kSgdChunkElems of it, every later chunk starts on a multiple of 4.  The 16-byte accesses of p and m (both 16-byte
// aligned at flat offset 0) are then aligned in every chunk; only the up to 3 elements before a segment's first multiple
// of 4 and the up to 3 behind its last are touched one by one.  A segment of 0 elements gives no chunk.
#pragma once
#include <stdint.h>

namespace aabr {

constexpr int kSgdChunkElems = 2048;      // 8 KiB of p per chunk: two passes of 256 threads x 16 bytes
constexpr int kSgdChunkWords = 4;         // int64 words per chunk record
constexpr int kSgdMaxGroups = 8;
constexpr int64_t kSgdMaxSegs = (int64_t)1 << 28;

// one record of the chunk table, as the kernel reads it (4 int64 words)
struct SgdChunk {
  int64_t off;         // flat offset of the chunk's first element
  int64_t seg_first;   // flat offset of its segment's first element (the gradient of element e is g_seg[e - seg_first])
  int64_t n;           // elements, 1 .. kSgdChunkElems
  int64_t seg_group;   // segment index * kSgdMaxGroups + group
};
static_assert(sizeof(SgdChunk) == kSgdChunkWords * sizeof(int64_t), "SgdChunk is 4 words");

// end (exclusive) of the chunk that starts at flat offset `cur` inside a segment ending at `end`
inline int64_t sgd_chunk_end(int64_t cur, int64_t end) {
  const int64_t cut = (cur + kSgdChunkElems) & ~(int64_t)3;
  return cut < end ? cut : end;
}

// Cuts n_segs segments into chunks.  out == nullptr: count only.  Returns the number of chunks, or -1 with *why set:
// a null array, a negative offset or size, a group outside 0 .. 7, segments that overlap or are not in ascending flat
// order, a segment that ends past n, or more chunks than `cap` (only when out != nullptr).
inline int64_t sgd_cut_segments(const int64_t *seg_off, const int64_t *seg_numel, const int32_t *seg_group,
                                int64_t n_segs, int64_t n, SgdChunk *out, int64_t cap, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  if (n_segs < 0 || n < 0 || cap < 0) { *why = "negative size"; return -1; }
  if (n_segs > kSgdMaxSegs) { *why = "more than 2^28 segments"; return -1; }
  if (n_segs > 0 && (!seg_off || !seg_numel || !seg_group)) { *why = "null segment array"; return -1; }
  int64_t count = 0, prev_end = 0;
  for (int64_t s = 0; s < n_segs; ++s) {
    const int64_t first = seg_off[s], len = seg_numel[s];
    if (first < 0 || len < 0) { *why = "negative segment offset or size"; return -1; }
    if (seg_group[s] < 0 || seg_group[s] >= kSgdMaxGroups) { *why = "segment group outside 0 .. 7"; return -1; }
    if (first < prev_end) { *why = "segments overlap or are not in ascending flat order"; return -1; }
    if (len > n || first > n - len) { *why = "segment ends past n"; return -1; }
    const int64_t end = first + len;
    for (int64_t cur = first; cur < end;) {
      const int64_t e = sgd_chunk_end(cur, end);
      if (out) {
        if (count >= cap) { *why = "chunk table too small"; return -1; }
        out[count] = SgdChunk{cur, first, e - cur, s * kSgdMaxGroups + seg_group[s]};
      }
      ++count;
      cur = e;
    }
    prev_end = end;
  }
  return count;
}

// everything aabr_sgd_momentum_step refuses before it launches; nullptr = the call is fine.  `last` is the last record of
// the host copy of the chunk table (records ascend in flat offset, so the last one bounds them all); nullptr when
// n_chunks == 0.
inline const char *sgd_step_refusal(const void *flat, const void *momentum_buf, int64_t n, const void *chunk_table,
                                    const SgdChunk *last, int64_t n_chunks, int64_t n_segs, const void *grad_flat,
                                    const void *grad_ptr_table, int grad_is_bf16, const float *lr, const float *wd,
                                    int n_groups, float momentum) {
  if (n < 0 || n_chunks < 0 || n_segs < 0) return "negative size";
  if (n_groups < 1 || n_groups > kSgdMaxGroups) return "n_groups outside 1 .. 8";
  if (!lr || !wd) return "null lr or wd array";
  if (grad_flat && grad_ptr_table) return "both gradient sources given: flat buffer and address table";
  if (!grad_flat && !grad_ptr_table) return "neither gradient source given";
  if (grad_is_bf16 != 0 && grad_is_bf16 != 1) return "grad_is_bf16 is 0 or 1";
  if (n_chunks == 0) return nullptr;
  if (!flat) return "null parameter buffer";
  if (momentum != 0.0f && !momentum_buf) return "null momentum buffer with momentum != 0";
  if (!chunk_table || !last) return "null chunk table";
  if (((uintptr_t)flat | (uintptr_t)momentum_buf) & 15) return "parameter or momentum buffer not 16-byte aligned";
  if (last->off < 0 || last->n < 1 || last->n > kSgdChunkElems || last->off > n - last->n)
    return "chunk table: the last chunk ends past n";
  if (last->seg_group < 0 || last->seg_group / kSgdMaxGroups >= n_segs) return "chunk table: segment index past n_segs";
  return nullptr;
}

} // namespace aabr

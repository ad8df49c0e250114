// merge_corners.hip -- merge_walls_by_corners of the reference (maskrcnn_benchmark/structures/bounding_box_3d.py:843-923)
// for every scene of a call in ONE launch: one workgroup per scene, the statements of merge_corners.h.
//
// The reference walks the 2W corners of a scene in a Python loop; every iteration issues about a dozen small torch
// kernels and two nonzero() host reads, and depends on the corners the earlier ones moved.  Here the scene's corners stay
// in LDS (x, y, z of 4096 corners: 48 KiB) for the whole loop:
//   rows     the scene's rows pass in chunks of 256; a wall's number is the count of walls before it (wave ballot, the
//            four waves' counts through LDS).  The same pass runs twice: the prologue fills the corner arrays, the
//            epilogue writes every row -- walls rebuilt, other rows copied bit for bit.
//   step i   lane t takes walls t, t + 256, ...: both corners of a wall are on one lane, so "the whole wall is in S" is a
//            lane-local test.  Per pass of 256 walls lane 0 of each wave publishes one word, members in the wave |
//            whole-wall flag << 16; ONE barrier later every lane reads the words: |S| and the skip decision are
//            workgroup-uniform.  The words are double-buffered by the step's parity, so a step that does not merge (most
//            of them) costs that one barrier and nothing else.  A merging step compacts S in ascending corner
//            order -- rank inside the wave from the ballots, the waves' bases from the words --, three lanes sum one axis
//            each in that order, and the members take the mean: three more barriers, each in front of a statement that
//            reads what other lanes wrote.
// No float atomics, no atomics at all: bit-identical run to run.  No host read.
#include "common.h"
#include "merge_corners.h"

namespace aabr {

namespace {

constexpr int kMergeThreads = 256;
constexpr int kMergeWaves = kMergeThreads / 64;
constexpr int kMergeMaxCorners = 2 * kMergeMaxWalls;
constexpr int kMergeMaxPasses = kMergeMaxWalls / kMergeThreads;

struct MergeLds {
  float x[kMergeMaxCorners], y[kMergeMaxCorners], z[kMergeMaxCorners];
  union {
    merge_id_t ids[kMergeMaxCorners];       // the loop: S in ascending order
    float z0[kMergeMaxWalls];               // the prologue: z0 of every wall, until the scene's mean is taken
  } u;
  unsigned char merged[kMergeMaxCorners];
  int words[2][kMergeMaxPasses * kMergeWaves];
  int wave_cnt[kMergeWaves];
  float mean[3];
  float z0_mean;
};
static_assert(sizeof(MergeLds) <= 64 * 1024, "the scene's image must fit the static LDS limit");

// The scene's rows in chunks of 256 in ascending order; fn(row, is_wall, w) with w = the number of walls before the row.
// Returns the scene's wall count on every lane.  Ends behind a barrier.
template <class F>
__device__ inline int merge_rows(MergeLds &s, const int64_t *__restrict__ labels, int64_t r0, int64_t n,
                                 int64_t wall_label, F fn) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int base = 0;
  for (int64_t c0 = 0; c0 < n; c0 += kMergeThreads) {
    const int64_t r = c0 + t;
    const bool wall = r < n && (labels == nullptr || labels[r0 + r] == wall_label);
    const unsigned long long b = __ballot(wall);
    if (lane == 0) s.wave_cnt[wave] = __popcll(b);
    __syncthreads();                                   // the waves' counts
    int before = base, total = 0;
#pragma unroll
    for (int v = 0; v < kMergeWaves; ++v) {
      const int c = s.wave_cnt[v];
      before += v < wave ? c : 0;
      total += c;
    }
    if (r < n) fn(r0 + r, wall, before + __popcll(b & ((1ull << lane) - 1ull)));
    base += total;
    __syncthreads();                                   // wave_cnt is rewritten by the next chunk
  }
  return base;
}

__global__ __launch_bounds__(kMergeThreads) void k_merge_walls_by_corners(
    const float *__restrict__ boxes, const int64_t *__restrict__ labels, int64_t n_rows,
    const int64_t *__restrict__ scene_begin, int64_t wall_label, float threshold, float *__restrict__ boxes_out,
    int32_t *__restrict__ merged_out) {
  __shared__ MergeLds s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int64_t r0 = scene_begin[blockIdx.x], r1 = scene_begin[blockIdx.x + 1];
  r0 = r0 < 0 ? 0 : (r0 > n_rows ? n_rows : r0);
  r1 = r1 < r0 ? r0 : (r1 > n_rows ? n_rows : r1);
  const int64_t n = r1 - r0;
  for (int k = t; k < kMergeMaxCorners; k += kMergeThreads) s.merged[k] = 0;

  // 1. the walls' corners (a wall beyond the built limit writes nothing: the scene is then passed through below)
  const int W = merge_rows(s, labels, r0, n, wall_label, [&](int64_t row, bool wall, int w) {
    if (!wall || w >= kMergeMaxWalls) return;
    float b[7];
#pragma unroll
    for (int d = 0; d < 7; ++d) b[d] = boxes[7 * row + d];
    s.u.z0[w] = merge_wall_prologue(b, w, s.x, s.y, s.z);
  });
  const bool pass_through = W > kMergeMaxWalls;        // refused on the host; never truncated here either
  if (t == 0 && W > 0 && !pass_through) s.z0_mean = merge_mean_serial(s.u.z0, W);
  __syncthreads();                                     // z0_mean; u.z0 is dead, u.ids may be written

  // 2. the loop over the corners
  if (W > 1 && !pass_through) {
    const int passes = (W + kMergeThreads - 1) / kMergeThreads, n_words = passes * kMergeWaves;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i = 0; i < 2 * W; ++i) {
      int *words = s.words[i & 1];
      for (int p = 0; p < passes; ++p) {
        const int w = p * kMergeThreads + t;
        const int m = w < W ? merge_wall_members(s.x, s.y, s.z, i, w, threshold) : 0;
        const unsigned long long b0 = __ballot(m & 1), b1 = __ballot(m & 2), bw = __ballot(m == 3);
        if (lane == 0) words[p * kMergeWaves + wave] = (__popcll(b0) + __popcll(b1)) | (bw != 0ull ? 1 << 16 : 0);
      }
      __syncthreads();                                 // the step's words
      int total = 0, whole = 0;
      for (int q = 0; q < n_words; ++q) {
        const int c = words[q];
        total += c & 0xffff;
        whole |= c >> 16;
      }
      if (whole || total <= 1) continue;               // uniform: every lane read the same words
      for (int p = 0; p < passes; ++p) {
        const int w = p * kMergeThreads + t;
        const int m = w < W ? merge_wall_members(s.x, s.y, s.z, i, w, threshold) : 0;
        const unsigned long long b0 = __ballot(m & 1), b1 = __ballot(m & 2);
        int at = __popcll(b0 & below) + __popcll(b1 & below);
        for (int q = 0; q < p * kMergeWaves + wave; ++q) at += words[q] & 0xffff;
        if (m & 1) s.u.ids[at++] = (merge_id_t)(2 * w);
        if (m & 2) s.u.ids[at] = (merge_id_t)(2 * w + 1);
      }
      __syncthreads();                                 // ids
      if (t < 3) s.mean[t] = merge_mean_axis(t == 0 ? s.x : (t == 1 ? s.y : s.z), s.u.ids, total);
      __syncthreads();                                 // mean; every lane has read the corners of this step
      for (int j = t; j < total; j += kMergeThreads)
        merge_assign(s.x, s.y, s.z, s.merged, s.u.ids[j], s.mean[0], s.mean[1], s.mean[2]);
      __syncthreads();                                 // the moved corners
    }
  }

  // 3. every row of the scene
  merge_rows(s, labels, r0, n, wall_label, [&](int64_t row, bool wall, int w) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(boxes) + 7 * row;
    int32_t f0 = 0, f1 = 0;
    if (wall && !pass_through) {
      float b[7], o[7];
#pragma unroll
      for (int d = 0; d < 7; ++d) b[d] = boxes[7 * row + d];
      merge_wall_epilogue(b, w, s.x, s.y, s.z, s.z0_mean, o);
#pragma unroll
      for (int d = 0; d < 7; ++d) boxes_out[7 * row + d] = o[d];
      f0 = s.merged[2 * w];
      f1 = s.merged[2 * w + 1];
    } else {
      uint32_t v[7];
#pragma unroll
      for (int d = 0; d < 7; ++d) v[d] = src[d];
      uint32_t *dst = reinterpret_cast<uint32_t *>(boxes_out) + 7 * row;
#pragma unroll
      for (int d = 0; d < 7; ++d) dst[d] = v[d];
    }
    if (merged_out) {
      merged_out[2 * row] = f0;
      merged_out[2 * row + 1] = f1;
    }
  });
}

}  // namespace

}  // namespace aabr

using namespace aabr;

extern "C" int aabr_merge_corners_max_walls(void) { return kMergeMaxWalls; }

extern "C" int aabr_merge_walls_by_corners(const float *boxes, const int64_t *labels, int64_t n,
                                           const int64_t *scene_begin, int64_t n_scenes, int64_t max_scene_rows,
                                           int64_t wall_label, float threshold, float *boxes_out, int32_t *merged,
                                           void *stream) {
  AABR_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 28), "need 0 <= rows < 2^28");
  AABR_CHECK_ARG(n_scenes >= 0 && n_scenes < ((int64_t)1 << 31), "need 0 <= scenes < 2^31");
  AABR_CHECK_ARG(max_scene_rows >= 0 && max_scene_rows <= n, "need 0 <= max_scene_rows <= rows");
  static_assert(kMergeMaxWalls == 2048, "the message below names the limit");
  AABR_CHECK_ARG(max_scene_rows <= kMergeMaxWalls,
                 "a scene has more rows than the 2048 walls per scene this library is built for (kMergeMaxWalls); "
                 "a scene's wall count is known on the device only, so its row count is held to that limit");
  if (n_scenes == 0) {
    AABR_CHECK_ARG(n == 0, "rows without a scene");
    return AABR_OK;
  }
  AABR_CHECK_ARG(scene_begin, "null pointer");
  AABR_CHECK_ARG(n == 0 || (boxes && boxes_out), "null pointer");
  AABR_CHECK_ARG(n == 0 || boxes != boxes_out, "boxes_out must not be boxes: the rows are read again after the loop");
  hipLaunchKernelGGL(k_merge_walls_by_corners, dim3((unsigned)n_scenes), dim3(kMergeThreads), 0, (hipStream_t)stream,
                     boxes, labels, n, scene_begin, wall_label, threshold, boxes_out, merged);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

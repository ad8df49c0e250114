// nms_shared.h -- device code that more than one translation unit runs and that must give the same bits in each:
// the tile of the rotated suppression mask, the greedy scan of one sorted list, and the box decode / encode of BoxCoder3D.
// iou_nms.hip wraps them into the one-list entry points (aabr_rotate_nms_sorted, aabr_box_decode, aabr_box_encode);
// roi_post.hip runs the mask, scan and decode over many (scene, class) lists in one launch, roi_loss.hip the encode per
// proposal.  Nothing here is copied: both files call these functions.
#pragma once
#include "common.h"
#include "iou_math.h"
#include "corner_box.h"   // the corner form of the coder: box_encode7_corner / box_decode7_corner, host + device

namespace aabr {

// BoxCoder3D.decode_centroid_box (modeling/box_coder_3d.py:53-80) of one encoding against its anchor: encodings /
// weights, sizes clamped at `clip`, second_box_decode with smooth_dim (second/pytorch/core/box_torch_ops.py:118-154),
// yaw through limit_period(., 0.5, pi) -- the fp32 operations of the torch expressions in their order.
struct BoxEncodeW { float w[7]; };
__device__ __forceinline__ void box_decode7(const float *__restrict__ enc, const float *__restrict__ an,
                                            const BoxEncodeW &w, float clip, float *o) {
  float e[7];
#pragma unroll
  for (int d = 0; d < 7; ++d) e[d] = enc[d] / w.w[d];
#pragma unroll
  for (int d = 3; d < 6; ++d) e[d] = e[d] > clip ? clip : e[d];
  const float diagonal = sqrtf(an[4] * an[4] + an[3] * an[3]);
  o[0] = e[0] * diagonal + an[0];
  o[1] = e[1] * diagonal + an[1];
  o[2] = e[2] * an[5] + an[2];
  o[3] = (e[3] + 1) * an[3];
  o[4] = (e[4] + 1) * an[4];
  o[5] = (e[5] + 1) * an[5];
  const float period = 3.14159274101257324f;
  const float rg = e[6] + an[6];
  o[6] = rg - floorf(rg / period + 0.5f) * period;
}

// BoxCoder3D.encode_centroid_box (modeling/box_coder_3d.py:46-51) = second_box_encode(targets, anchors, smooth_dim=True)
// (second/pytorch/core/box_torch_ops.py:82-116; both boxes split positionally as x, y, z, w, l, h, r), the yaw difference
// wrapped by limit_period(., 0.5, pi) (utils3d/geometric_torch.py:4-10), times the coder's weights -- the same fp32
// operations in the same order as the torch expressions (no contraction: -ffp-contract=off)
__device__ __forceinline__ void box_encode7(const float *g, const float *a, const float *w, float *o) {
  const float diagonal = sqrtf(a[4] * a[4] + a[3] * a[3]);
  float e[7];
  e[0] = (g[0] - a[0]) / diagonal;
  e[1] = (g[1] - a[1]) / diagonal;
  e[2] = (g[2] - a[2]) / a[5];
  e[3] = g[3] / a[3] - 1.0f;
  e[4] = g[4] / a[4] - 1.0f;
  e[5] = g[5] / a[5] - 1.0f;
  const float kPi = 3.14159274101257324f;             // (float)math.pi
  const float rt = g[6] - a[6];
  e[6] = rt - floorf(rt / kPi + 0.5f) * kPi;
#pragma unroll
  for (int d = 0; d < 7; ++d) o[d] = e[d] * w[d];
}

// Rotated boxes, round 4.  The decision of the reference's loop is `pre-filter matrix > 0 and exact polygon IoU >=
// thresh` (spconv 1.x behind nms_cpu.py:43); evaluated in that order every overlapping pair pays both the numba-style
// IoU (vertex collection + sort, ~4x the cost of the clip) and the clip.  Here: a workgroup (256 threads) owns 16 rows x
// 64 columns; the corners of its 80 boxes are computed ONCE (fp64 sin / cos per box instead of per pair) and shared
// through LDS; per pair: circumscribed circles apart -> no hit; else the exact clip (registers only); only a pair that
// WOULD suppress (clip >= thresh: a few per cent) evaluates the pre-filter value.  Same verdicts as the order above.
// The tile is (rows i0 .. i0 + 15, column block cb) of the list `boxes` [n, 7]; i0 and cb are workgroup-uniform.
constexpr int kNmsRows = 16;
__device__ __forceinline__ void nms_mask_rot_tile(const float *__restrict__ boxes, int64_t n, float thresh, int only_xy,
                                                  int colblocks, unsigned long long *__restrict__ mask, int64_t i0,
                                                  int cb) {
  using namespace aabr_iou;
  __shared__ double s_cx[64 + kNmsRows][4], s_cy[64 + kNmsRows][4];
  __shared__ float s_b[64 + kNmsRows][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (cb < (int)(i0 >> 6)) {                           // wholly below the diagonal: a lower-scored box suppresses nothing
    if (threadIdx.x < kNmsRows && i0 + threadIdx.x < n) mask[(i0 + threadIdx.x) * colblocks + cb] = 0ull;
    return;
  }
  if (threadIdx.x < 64 + kNmsRows) {                   // slots 0..63: the column boxes; 64..79: the row boxes
    const int64_t q = threadIdx.x < 64 ? (int64_t)cb * 64 + threadIdx.x : i0 + (threadIdx.x - 64);
    float b7[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (q < n)
#pragma unroll
      for (int d = 0; d < 7; ++d) b7[d] = boxes[q * 7 + d];
    const float r5[5] = {b7[0], b7[1], b7[3], b7[4], b7[6]};
    double cx[4], cy[4];
    clip_corners(r5, cx, cy);
#pragma unroll
    for (int k = 0; k < 4; ++k) { s_cx[threadIdx.x][k] = cx[k]; s_cy[threadIdx.x][k] = cy[k]; }
#pragma unroll
    for (int d = 0; d < 7; ++d) s_b[threadIdx.x][d] = b7[d];
  }
  __syncthreads();
  const int64_t j = (int64_t)cb * 64 + lane;
  float c[7];
#pragma unroll
  for (int d = 0; d < 7; ++d) c[d] = s_b[lane][d];
  double jx[4], jy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { jx[k] = s_cx[lane][k]; jy[k] = s_cy[lane][k]; }
  const double area_j = fabs((double)c[3] * (double)c[4]);
  const float rj = 0.5f * sqrtf(c[3] * c[3] + c[4] * c[4]);
  for (int t = 0; t < kNmsRows / 4; ++t) {
    const int rs = wave * (kNmsRows / 4) + t;
    const int64_t i = i0 + rs;
    if (i >= n) break;                                 // wave-uniform
    bool hit = false;
    if (cb >= (int)(i >> 6) && j < n && j > i) {
      const float *b = s_b[64 + rs];
      const float dx = b[0] - c[0], dy = b[1] - c[1];
      const float ri = 0.5f * sqrtf(b[3] * b[3] + b[4] * b[4]);
      const float rr = (ri + rj) * 1.0001f + 1e-6f;    // conservative: never rejects a pair the clip would count
      if (dx * dx + dy * dy <= rr * rr) {
        double ix[4], iy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { ix[k] = s_cx[64 + rs][k]; iy[k] = s_cy[64 + rs][k]; }
        const double e = clip_iou_corners(ix, iy, jx, jy, fabs((double)b[3] * (double)b[4]), area_j);
        if (e >= (double)thresh) {
          const float bi[5] = {b[0], b[1], b[3], b[4], b[6]};
          const float bj[5] = {c[0], c[1], c[3], c[4], c[6]};
          float v = iou_eval_entry(bi, bj, -1);        // matrix entry [i][j] of boxes_iou_3d(dets, dets)
          if (!only_xy) {
            const float z0 = b[2], z1 = b[2] + b[5], a0 = c[2], a1 = c[2] + c[5];
            v = v * ((fminf(a1, z1) - fmaxf(a0, z0)) / (fmaxf(a1, z1) - fminf(a0, z0)));
          }
          hit = v > 0.0f;
        }
      }
    }
    const unsigned long long bits = __ballot(hit);
    if (lane == 0) mask[i * colblocks + cb] = bits;
  }
}

// Greedy scan of one sorted list by one workgroup of 256 threads.  `remv`: colblocks words of LDS owned by the caller.
__device__ __forceinline__ void nms_scan_block(const unsigned long long *__restrict__ mask, int64_t n, int colblocks,
                                               int64_t post_max, int64_t *__restrict__ keep,
                                               int32_t *__restrict__ meta, unsigned long long *remv) {
  __shared__ unsigned long long s_kept;
  __shared__ int s_nk;
  const int tid = threadIdx.x;
  for (int w = tid; w < colblocks; w += blockDim.x) remv[w] = 0ull;
  if (tid == 0) s_nk = 0;
  __syncthreads();
  const int wl = tid & 31, slice = tid >> 5;
  for (int rb = 0; rb < colblocks; ++rb) {
    const int64_t r0 = (int64_t)rb * 64;
    const int rows = (int)((n - r0) < 64 ? (n - r0) : 64);
    // speculative fetch, before the block's kept set is known: this thread's 8 rows (b = slice mod 8) of the
    // first 32 words to the right of the diagonal.  The loads overlap the serial chain below; rows that
    // turn out suppressed are simply not OR-ed in.
    unsigned long long pre[8];
    {
      const int w = rb + 1 + wl;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t row = r0 + slice + 8 * i;
        pre[i] = (w < colblocks && row < n) ? mask[row * colblocks + w] : 0ull;
      }
    }
    if (tid < 64) { // first wave: resolve the chain inside the block on the diagonal bits
      unsigned long long diag = (tid < rows) ? mask[(r0 + tid) * colblocks + rb] : 0ull;
      unsigned long long cur = remv[rb], kept = 0ull;
      for (int b = 0; b < rows; ++b) {
        unsigned long long db = __shfl(diag, b); // wave-uniform trip
        if (!((cur >> b) & 1ull)) { kept |= 1ull << b; cur |= db; }
      }
      // kept rows go to the list at their rank (all lanes at once)
      const int nk0 = s_nk;
      if ((kept >> tid) & 1ull) {
        const int64_t pos = nk0 + __popcll(kept & ((1ull << tid) - 1ull));
        if (pos < post_max) keep[pos] = r0 + tid;
      }
      if (tid == 0) {
        s_nk = nk0 + (int)__popcll(kept);
        s_kept = kept;
      }
    }
    __syncthreads();
    const unsigned long long kept = s_kept;
    if (s_nk >= post_max) break; // uniform
    // OR the kept rows' words into remv: 32 words x 8 row slices per pass (rows b = slice mod 8), loads of
    // a thread are independent; slices meet in LDS with a 64-bit atomic OR
    {
      const unsigned long long mine = kept & (0x0101010101010101ull << slice);
      if (mine) {
        unsigned long long acc0 = 0ull;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if ((mine >> (slice + 8 * i)) & 1ull) acc0 |= pre[i];
        if (acc0) atomicOr(&remv[rb + 1 + wl], acc0);
      }
      if (mine)
        for (int w = rb + 1 + wl + 32; w < colblocks; w += 32) {
          unsigned long long acc = 0ull, kb = mine;
          while (kb) {
            const int b = __ffsll((long long)kb) - 1;
            kb &= kb - 1;
            acc |= mask[(r0 + b) * colblocks + w];
          }
          if (acc) atomicOr(&remv[w], acc);
        }
    }
    __syncthreads();
  }
  if (tid == 0) meta[0] = (int32_t)(s_nk < post_max ? s_nk : post_max);
}

} // namespace aabr

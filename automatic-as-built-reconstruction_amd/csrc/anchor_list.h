// anchor_list.h -- an example's anchor list and the arithmetic on it, for every RPN stage that reads one: the proposal
// stage (iou_nms.hip: padded logits, fused top-k, decode), the label generation (iou_nms.hip) and the loss with its
// sampler (sample_shared.h, rpn_loss.hip).  The list is the anchors of all maps laid end to end as [map][site][yaw]
// (cat_scales_anchor, rpn_sparse3d.py:19-77); neither it nor the regrouped head outputs are ever materialised.  Two host
// tables address it: seg[b][m] = the first list index of map m in example b, site[b][m] = the first site row of example b
// in map m.  The sampler's key, the regression targets and the decoded boxes are promised bit-identical across the
// stages, so the table, its checks, the locate, the anchor and the float key exist here and nowhere else.
#pragma once
#include "common.h"

namespace aabr {

constexpr int kAnchorMaxMaps = 8, kAnchorMaxBatch = 16;
// a kernel's arguments (its parameter struct and everything passed beside it) must fit the 4 KiB kernel-argument segment
constexpr size_t kKernelArgBytes = 4096;

struct AnchorSegs {
  int32_t n_maps, nb, A;
  int32_t seg[kAnchorMaxBatch][kAnchorMaxMaps + 1];   // in anchors; slots past n_maps repeat the example's length
  int32_t site[kAnchorMaxBatch][kAnchorMaxMaps];      // in site rows; unused slots 0
};
struct AnchorLoc {
  int m, a;        // map, yaw
  int64_t row;     // site row in map m; row * A + a indexes the map's objectness / regression vectors
};
// the maps' site lists and what turns a site into its anchors (anchor_generator_sparse3d.py:88-104)
struct AnchorGeom {
  const int32_t *coords[kAnchorMaxMaps];   // [V_m, 4]
  float stride[kAnchorMaxMaps][3];
  float voxel_scale;
};

// map of list index j (0 <= j < seg[b][n_maps]) of example b: the last map that begins at or before j, empty maps skipped
__device__ __forceinline__ int anchor_map(const AnchorSegs &s, int b, int64_t j) {
  int m = 0;
  while (m + 1 < s.n_maps && j >= s.seg[b][m + 1]) ++m;
  return m;
}
__device__ __forceinline__ AnchorLoc anchor_locate(const AnchorSegs &s, int b, int64_t j) {
  const int m = anchor_map(s, b, j);
  const int32_t q = (int32_t)(j - s.seg[b][m]);
  return {m, q % s.A, (int64_t)s.site[b][m] + q / s.A};
}
// L.row * A + L.a of anchor_locate(s, b, j) without its division -- (site + q / A) * A + q % A = site * A + q -- for the
// passes that read one logit per list entry (padded logits, top-k); the map comes from the same anchor_map
__device__ __forceinline__ int64_t anchor_flat(const AnchorSegs &s, int b, int64_t j, int &m) {
  m = anchor_map(s, b, j);
  return (int64_t)s.site[b][m] * s.A + (j - s.seg[b][m]);
}

// AnchorGenerator.grid_anchors for one anchor: (location.float() + 0) / voxel_scale * stride + base, sizes and yaw
// 0 + base -- the fp32 operations of the torch expression in their order.  base_anchors: [n_maps * A, 7]
__device__ __forceinline__ void anchor_box7(const AnchorGeom &g, const float *__restrict__ base_anchors, int A,
                                            const AnchorLoc &L, float an[7]) {
  const int32_t *sc = g.coords[L.m] + 4 * L.row;
  const float *ba = base_anchors + 7 * ((int64_t)L.m * A + L.a);
#pragma unroll
  for (int d = 0; d < 3; ++d) an[d] = (float)sc[d] / g.voxel_scale * g.stride[L.m][d] + ba[d];
#pragma unroll
  for (int d = 3; d < 7; ++d) an[d] = 0.0f + ba[d];
}

// order-preserving float -> uint32 key (0 = below every float; -0 < +0: harmless) and back: maxima and top-k cuts are
// taken on integers
__device__ __forceinline__ uint32_t float_order_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_order_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// host side: the table of examples [b0, b0 + nbc) out of the caller's flat lists (seg_host: n_maps + 1 per example,
// site_host: n_maps per example, or null = all 0, the flat-list mode of aabr_sample_list), checked for every entry point
// alike -- each device function above relies on all of it.  `fn` names the entry in the error; *nmax = the longest list.
// "A non-empty segment needs this entry's map pointers" stays with the entry.
inline int fill_anchor_segs(AnchorSegs &out, const char *fn, int n_maps, int A, int b0, int nbc, const int32_t *seg_host,
                            const int32_t *site_host, int64_t *nmax) {
  AABR_CHECK_ARG_AS(fn, n_maps >= 1 && n_maps <= kAnchorMaxMaps && nbc >= 1 && nbc <= kAnchorMaxBatch && A > 0 && b0 >= 0,
                   "anchor table: 1 .. 8 maps, 1 .. 16 examples, at least one anchor per site");
  AABR_CHECK_ARG_AS(fn, seg_host, "null segment table");
  out.n_maps = n_maps; out.nb = nbc; out.A = A;
  int64_t longest = 0;
  for (int b = 0; b < kAnchorMaxBatch; ++b) {
    const bool on = b < nbc;
    for (int m = 0; m <= kAnchorMaxMaps; ++m)
      out.seg[b][m] = on ? seg_host[(int64_t)(b0 + b) * (n_maps + 1) + (m <= n_maps ? m : n_maps)] : 0;
    for (int m = 0; m < kAnchorMaxMaps; ++m)
      out.site[b][m] = on && m < n_maps && site_host ? site_host[(int64_t)(b0 + b) * n_maps + m] : 0;
    if (!on) continue;
    AABR_CHECK_ARG_AS(fn, out.seg[b][0] == 0, "an example's segment table starts at 0");
    for (int m = 0; m < n_maps; ++m) {
      AABR_CHECK_ARG_AS(fn, out.seg[b][m + 1] >= out.seg[b][m], "segment table must be non-decreasing");
      AABR_CHECK_ARG_AS(fn, (out.seg[b][m + 1] - out.seg[b][m]) % A == 0, "a map's segment is not a multiple of A");
    }
    if (out.seg[b][n_maps] > longest) longest = out.seg[b][n_maps];
  }
  if (nmax) *nmax = longest;
  return AABR_OK;
}
// the maps' site lists and strides (strides_host: 3 per map); unused slots null / 0
inline void fill_anchor_geom(AnchorGeom &g, int n_maps, const void *const *coords_ptrs, const float *strides_host,
                             float voxel_scale) {
  for (int m = 0; m < kAnchorMaxMaps; ++m) {
    g.coords[m] = m < n_maps ? (const int32_t *)coords_ptrs[m] : nullptr;
    for (int d = 0; d < 3; ++d) g.stride[m][d] = m < n_maps ? strides_host[3 * m + d] : 0.f;
  }
  g.voxel_scale = voxel_scale;
}

static_assert(sizeof(AnchorSegs) == 1100, "AnchorSegs: 3 + 16 * 9 + 16 * 8 words");

} // namespace aabr

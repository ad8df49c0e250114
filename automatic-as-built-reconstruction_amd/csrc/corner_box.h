// corner_box.h -- the two-corner box form of the ROI heads and its coder (reference: MODEL.CORNER_ROI = True), as plain
// functions that the HIP kernels run per box and that a host harness compiles unchanged (tests/corner_box_host_harness.cpp),
// the way iou_math.h is shared.
//
//   yx_zb box   [xc, yc, z_bottom, thickness, length, height, yaw - pi/2]     (what every list of this package holds)
//   two corners [x0, y0, x1, y1, z0, z1, thickness]                           (end points of the bottom centre line)
//
// Behavioural contract:
//   yxzb_to_2corners    utils3d/bbox3d_ops_torch.py:115-135 (Box3D_Torch.from_yxzb_to_2corners) ->
//                       utils3d/bbox3d_ops.py:127-157,524-559,623-653 (convert_from_yx_zb_boxes, bbox_corners,
//                       bboxes_corners_xz_central_surface) -> bbox3d_ops_torch.py:8-19 (adjust_corner_order)
//   corners_to_yxzb     bbox3d_ops_torch.py:29-55,93-112 (from_2corners_to_yxzb) -> utils3d/geometric_torch.py:23-84
//   box_encode7_corner  second/pytorch/core/box_torch_ops.py:14-45 (smooth_dim) x weights (box_coder_3d.py:82-91)
//   box_decode7_corner  box_coder_3d.py:93-122 -> box_torch_ops.py:51-79 (smooth_dim) -> from_2corners_to_yxzb
// The reference walks the boxes in a Python loop on the host for the first of these; here it is a few operations per box.
// Compile with -ffp-contract=off: every product / sum is rounded separately, as numpy and CPU torch round them.
#pragma once
#include <math.h>
#ifndef AABR_HD
#ifdef __HIPCC__
#define AABR_HD __host__ __device__ inline
#else
#define AABR_HD static inline
#endif
#endif

namespace aabr {

constexpr float kCornerPi = 3.14159274101257324f;      // (float)math.pi
constexpr float kCornerHalfPi = 1.57079637050628662f;  // (float)(math.pi * 0.5)

// val - floor(val / pi + offset) * pi (geometric_torch.py:4-10; the numpy one of geometric_util.py is the same in fp32)
AABR_HD float corner_limit_period(float v, float offset) { return v - floorf(v / kCornerPi + offset) * kCornerPi; }

// One yx_zb box to its two-corner form.
//   1. convert_from_yx_zb_boxes in numpy fp32: z centre, (length, thickness) as (x size, y size), yaw + pi/2 limited to
//      [0, pi).
//   2. bbox_corners: the unit corner table is float64, so the rotation R (p - h) + h (h: half sizes, R = Rz(yaw)) is
//      evaluated in fp64 -- fp64 sin / cos, fp64 products and sums -- and rounded ONCE to fp32 (`astype(bbox.dtype)`); the
//      shift by centroid - h is an fp32 addition.  Yaw exactly 0 skips the rotation: p + (centroid - h), whose fp64 sum
//      rounded to fp32 (`np.array(..., float32)`) is the fp32 sum.
//   3. the y-mid-plane: (corner k + corner k+2) / 2 in fp32 for k = 0 (x low end) and 1 (x high end); z0 is the bottom,
//      z1 = height + bottom, thickness is b[3] itself.
//   4. adjust_corner_order in torch fp32: corner 0 is the end whose offset from the centroid has a component sum > 0
//      (strict: a tie swaps), selected through the reference's multiply-by-mask blend.
AABR_HD void yxzb_to_2corners(const float b[7], float c[7]) {
  const float zc = b[2] + b[5] * 0.5f;
  const float sx = b[4], sy = b[3], sz = b[5];
  const float yaw = corner_limit_period(b[6] + kCornerHalfPi, 0.0f);
  const float hx = sx * 0.5f, hy = sy * 0.5f, hz = sz * 0.5f;
  const float zx = b[0] - hx, zy = b[1] - hy, zz = zc - hz;   // `zero = centroid - bsize * 0.5`
  float kx[4], ky[4];                                          // bottom corners (0,0) (1,0) (0,1) (1,1) of the unit table
  float zb, zt;
  if (yaw != 0.0f) {
    const double cs = cos((double)yaw), sn = sin((double)yaw);
    const double dhx = (double)hx, dhy = (double)hy, dhz = (double)hz;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double dx = ((k & 1) ? (double)sx : 0.0) - dhx, dy = ((k & 2) ? (double)sy : 0.0) - dhy;
      kx[k] = (float)(cs * dx + sn * dy + dhx) + zx;
      ky[k] = (float)(-sn * dx + cs * dy + dhy) + zy;
    }
    zb = (float)((0.0 - dhz) + dhz) + zz;
    zt = (float)(((double)sz - dhz) + dhz) + zz;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      kx[k] = ((k & 1) ? sx : 0.0f) + zx;
      ky[k] = ((k & 2) ? sy : 0.0f) + zy;
    }
    zb = 0.0f + zz;
    zt = sz + zz;
  }
  const float ax = (kx[0] + kx[2]) / 2.0f, ay = (ky[0] + ky[2]) / 2.0f;
  const float bx = (kx[1] + kx[3]) / 2.0f, by = (ky[1] + ky[3]) / 2.0f;
  const float mx = (ax + bx) / 2.0f, my = (ay + by) / 2.0f;
  const float m = ((ax - mx) + (ay - my)) > 0.0f ? 1.0f : 0.0f, n = 1.0f - m;
  c[0] = ax * m + bx * n;
  c[1] = ay * m + by * n;
  c[2] = bx * m + ax * n;
  c[3] = by * m + ay * n;
  c[4] = (zb + zb) / 2.0f;
  c[5] = (zt + zt) / 2.0f;
  c[6] = b[3];
}

// The two top corners (x0, y0, z1), (x1, y1, z1) of a two-corner box, each moved towards the pair's midpoint by half the
// thickness (bounding_box_3d.py:270-291, get_2top_corners_offseted), in the fp32 operations of the torch expressions:
// centroid = (p0 + p1) / 2, offset = centroid - p, offset / |offset| * thickness * 0.5 from left to right, p + offset.
// o = [corner 0 xyz, corner 1 xyz].  A zero-length box divides by zero and gives the IEEE result.
AABR_HD void corners_top_offseted(const float c[7], float o[6]) {
  const float p[2][3] = {{c[0], c[1], c[5]}, {c[2], c[3], c[5]}};
  float cen[3];
  for (int d = 0; d < 3; ++d) cen[d] = (p[0][d] + p[1][d]) / 2.0f;
  for (int k = 0; k < 2; ++k) {
    float off[3];
    for (int d = 0; d < 3; ++d) off[d] = cen[d] - p[k][d];
    const float nrm = sqrtf(off[0] * off[0] + off[1] * off[1] + off[2] * off[2]);
    for (int d = 0; d < 3; ++d) o[3 * k + d] = p[k][d] + off[d] / nrm * c[6] * 0.5f;
  }
}

// One two-corner box back to yx_zb, in the fp32 operations of the torch expressions:
//   corner_box_to_standard: centroid = (p0 + p1) / 2, length = |p1 - p0|, height = z1 - z0, yaw = angle_with_x(p1 - p0);
//   angle_with_x against (1, 0): the cross term is the normalised y component and the cosine the normalised x component
//   (their other products are with the exact 1 and 0 of the x axis); the |cz| > 1 guard, asin, the branch blend by the
//   cosine's sign and limit_period(., 0, pi) follow geometric_torch.py:63-81 literally.  asin is evaluated in fp64 and
//   narrowed, as iou_math.h does with sin / cos: host and device then give the same bits.
//   convert_to_yx_zb_boxes: z bottom, yaw - pi/2, limit_period(., 0.5, pi).
AABR_HD void corners_to_yxzb(const float c[7], float b[7]) {
  const float cx = (c[0] + c[2]) / 2.0f, cy = (c[1] + c[3]) / 2.0f, cz = (c[4] + c[5]) / 2.0f;
  const float dx = c[2] - c[0], dy = c[3] - c[1];
  const float len = sqrtf(fmaf(dy, dy, dx * dx));       // torch.norm over two fp32 elements on the CPU: one fused step
  const float zs = c[5] - c[4];
  const float vx = dx / len, vy = dy / len;
  float cr = 1.0f * vy - 0.0f * vx;
  const float g = fabsf(cr) > 1.0f ? 1.0f : 0.0f;
  cr = cr * (1.0f - g * 1e-7f);
  float ang = -(float)asin((double)cr);
  const float cosa = 1.0f * vx + 0.0f * vy + 0.0f * 0.0f;
  const float m = cosa >= 0.0f ? 1.0f : 0.0f;
  ang = ang * m + (kCornerPi - ang) * (1.0f - m);
  ang = corner_limit_period(ang, 0.0f);
  b[0] = cx;
  b[1] = cy;
  b[2] = cz - zs * 0.5f;
  b[3] = c[6];
  b[4] = len;
  b[5] = zs;
  b[6] = corner_limit_period(ang - kCornerHalfPi, 0.5f);
}

// BoxCoder3D.encode_corner_box of one (target, anchor) pair of yx_zb boxes: both to two corners, then
// second_corner_box_encode with smooth_dim, times the coder's weights.  A zero-length or zero-height anchor divides by
// zero and gives the IEEE result.
AABR_HD void box_encode7_corner(const float *g_yxzb, const float *a_yxzb, const float *w, float *o) {
  float g[7], a[7], e[7];
  yxzb_to_2corners(g_yxzb, g);
  yxzb_to_2corners(a_yxzb, a);
  const float axs = a[0] - a[2], ays = a[1] - a[3];
  const float xydis = sqrtf(axs * axs + ays * ays);
  const float azs = fabsf(a[4] - a[5]);
  e[0] = (g[0] - a[0]) / xydis;
  e[1] = (g[1] - a[1]) / xydis;
  e[2] = (g[2] - a[2]) / xydis;
  e[3] = (g[3] - a[3]) / xydis;
  e[4] = (g[4] - a[4]) / azs;
  e[5] = (g[5] - a[5]) / azs;
  e[6] = g[6] / a[6] - 1.0f;
  for (int d = 0; d < 7; ++d) o[d] = e[d] * w[d];
}

// BoxCoder3D.decode_corner_box of one encoding against its proposal (yx_zb): encoding / weights, elements 3..5 clamped
// at `clip` (the reference clamps those positions in the corner layout too: y1, z0, z1), second_corner_box_decode with
// smooth_dim against the proposal's two corners, back to yx_zb.
AABR_HD void box_decode7_corner(const float *enc, const float *an_yxzb, const float *w, float clip, float *o) {
  float a[7], e[7], c[7];
  yxzb_to_2corners(an_yxzb, a);
  for (int d = 0; d < 7; ++d) e[d] = enc[d] / w[d];
  for (int d = 3; d < 6; ++d) e[d] = e[d] > clip ? clip : e[d];
  const float axs = a[0] - a[2], ays = a[1] - a[3];
  const float xydis = sqrtf(axs * axs + ays * ays);
  const float azs = fabsf(a[4] - a[5]);
  c[0] = e[0] * xydis + a[0];
  c[1] = e[1] * xydis + a[1];
  c[2] = e[2] * xydis + a[2];
  c[3] = e[3] * xydis + a[3];
  c[4] = azs * e[4] + a[4];
  c[5] = azs * e[5] + a[5];
  c[6] = (e[6] + 1.0f) * a[6];
  corners_to_yxzb(c, o);
}

} // namespace aabr

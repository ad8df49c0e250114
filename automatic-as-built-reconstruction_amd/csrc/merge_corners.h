// merge_corners.h -- merging the walls of one scene by their corners (reference: maskrcnn_benchmark/structures/
// bounding_box_3d.py:843-923, merge_by_corners / merge_walls_by_corners), as plain functions that the HIP kernel
// (merge_corners.hip) runs and that a host harness compiles unchanged (tests/merge_corners_host_harness.cpp), the way
// corner_box.h is shared.
//
// The walls of a scene are numbered 0 .. W-1; wall w owns corners 2w and 2w+1, the partner of corner k is k ^ 1.  The
// corners live in three arrays x[2W], y[2W], z[2W] for the whole run:
//   1. merge_wall_prologue   per wall: yxzb_to_2corners, corners_top_offseted (get_2top_corners_offseted, :270-291) -> the
//                            two top corners pulled in by half the thickness; returns z0 of the wall's two-corner row.
//   2. the loop over i = 0 .. 2W-1 on the CURRENT corners (:865-883).  One step is
//        merge_wall_members  for every wall: which of its two corners lie closer than the threshold to corner i (the
//                            partner of i never does): the set S.  A wall with BOTH corners in S skips the step;
//        merge_mean_axis     otherwise, with |S| > 1: the mean of S per axis, summed in ascending corner index, one fp32
//                            addition at a time from 0, one division by |S| (CPU torch's x[ids].mean(dim=0) gives these
//                            bits up to |S| = 4; beyond that torch's own summation order is not followed);
//        merge_assign        every corner of S takes the mean and is flagged.
//      merge_step_serial is the step as a loop over the walls; the kernel spreads the same three functions over its lanes.
//   3. merge_wall_epilogue   per wall (:905-917): both corners pushed outward from their midpoint by half the thickness,
//                            x0 y0 x1 y1 from the pushed corners, z1 the mean of their z, z0 the scene's mean z0
//                            (merge_mean_serial over the walls in ascending order), corners_to_yxzb.
// A wall whose two corners end at the same point divides by zero and gives the IEEE result.
// Compile with -ffp-contract=off: every product / sum is rounded separately except where fmaf is written.
#pragma once
#include "corner_box.h"

namespace aabr {

constexpr int kMergeMaxWalls = 2048;      // walls of one scene the corner arrays are built for (4096 corners)

typedef unsigned short merge_id_t;        // a corner index (< 2 * kMergeMaxWalls)

// dif.norm(dim=1) of one [3] fp32 row on the CPU: torch accumulates the squares with fused steps
AABR_HD float merge_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

AABR_HD float merge_wall_prologue(const float b[7], int w, float *x, float *y, float *z) {
  float c[7], o[6];
  yxzb_to_2corners(b, c);
  corners_top_offseted(c, o);
  x[2 * w] = o[0]; y[2 * w] = o[1]; z[2 * w] = o[2];
  x[2 * w + 1] = o[3]; y[2 * w + 1] = o[4]; z[2 * w + 1] = o[5];
  return c[4];
}

// bit 0: corner 2w is in S of step i, bit 1: corner 2w+1 is.  3 = the whole wall (never the wall of i itself: its
// other corner is the partner).  A NaN distance is not < threshold.
AABR_HD int merge_wall_members(const float *x, const float *y, const float *z, int i, int w, float threshold) {
  const float xi = x[i], yi = y[i], zi = z[i];
  int m = 0;
  for (int c = 0; c < 2; ++c) {
    const int k = 2 * w + c;
    if (k != (i ^ 1) && merge_dist(xi, yi, zi, x[k], y[k], z[k]) < threshold) m |= 1 << c;
  }
  return m;
}

AABR_HD float merge_mean_axis(const float *v, const merge_id_t *ids, int n) {
  float s = 0.0f;
  for (int j = 0; j < n; ++j) s += v[ids[j]];
  return s / (float)n;
}

AABR_HD float merge_mean_serial(const float *v, int n) {
  float s = 0.0f;
  for (int j = 0; j < n; ++j) s += v[j];
  return s / (float)n;
}

AABR_HD void merge_assign(float *x, float *y, float *z, unsigned char *merged, int k, float mx, float my, float mz) {
  x[k] = mx; y[k] = my; z[k] = mz;
  merged[k] = 1;
}

// One step over n_walls walls; ids: room for 2 n_walls entries.  Returns |S| when the step merged, 0 when it did not.
AABR_HD int merge_step_serial(float *x, float *y, float *z, unsigned char *merged, int n_walls, int i, float threshold,
                              merge_id_t *ids) {
  int n = 0;
  bool whole = false;
  for (int w = 0; w < n_walls; ++w) {
    const int m = merge_wall_members(x, y, z, i, w, threshold);
    whole = whole || m == 3;
    if (m & 1) ids[n++] = (merge_id_t)(2 * w);
    if (m & 2) ids[n++] = (merge_id_t)(2 * w + 1);
  }
  if (whole || n <= 1) return 0;
  const float mx = merge_mean_axis(x, ids, n), my = merge_mean_axis(y, ids, n), mz = merge_mean_axis(z, ids, n);
  for (int j = 0; j < n; ++j) merge_assign(x, y, z, merged, ids[j], mx, my, mz);
  return n;
}

// top_2corners.mean(dim=1) of two rows: torch's sum starts from 0
AABR_HD float merge_mean2(float a, float b) { return ((0.0f + a) + b) / 2.0f; }

AABR_HD void merge_wall_epilogue(const float b[7], int w, const float *x, const float *y, const float *z, float z0_mean,
                                 float out[7]) {
  const float p[2][3] = {{x[2 * w], y[2 * w], z[2 * w]}, {x[2 * w + 1], y[2 * w + 1], z[2 * w + 1]}};
  float cen[3], q[2][3], c[7];
  for (int d = 0; d < 3; ++d) cen[d] = merge_mean2(p[0][d], p[1][d]);
  for (int k = 0; k < 2; ++k) {
    float off[3];
    for (int d = 0; d < 3; ++d) off[d] = p[k][d] - cen[d];
    // offset.norm(dim=2) over [W, 2, 3] fp32 on the CPU (torch 2.10): fused like merge_dist -- 30000 random rows matched
    // sqrt(fma(z, z, fma(y, y, x * x))) bit for bit, and about one in ten differed from the separately rounded sum
    const float nrm = sqrtf(fmaf(off[2], off[2], fmaf(off[1], off[1], off[0] * off[0])));
    for (int d = 0; d < 3; ++d) q[k][d] = p[k][d] + off[d] / nrm * b[3] * 0.5f;
  }
  c[0] = q[0][0]; c[1] = q[0][1]; c[2] = q[1][0]; c[3] = q[1][1];
  c[4] = z0_mean;
  c[5] = merge_mean2(q[0][2], q[1][2]);
  c[6] = b[3];
  corners_to_yxzb(c, out);
}

} // namespace aabr

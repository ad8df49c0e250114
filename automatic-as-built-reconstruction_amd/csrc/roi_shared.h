// roi_shared.h -- what the single-level fused ROI-align (roi.hip, k_roi_align_rot3d_sparse) and the multi-level pooler
// (roi_pool.hip, k_roi_pool) both compile and that must give the same bits in each: the geometry record, the workgroup's
// tile constants and the corner arithmetic of one sample point.  Nothing here is copied: both files include this code.
#pragma once
#include "common.h"

namespace aabr {

struct RoiGeom {
  int channels, height, width, zsize, ph, pw, pz, sampling;
  float scale;
};

constexpr int kRoiPlanes = 128; // planes per workgroup (lanes)
constexpr int kRoiBins = 96;    // bins staged in LDS per pass: 128 x 96 x 4 B = 48 KiB

// geometry of one sample point: the 8 corner cells and weights exactly as the dense kernels compute them
struct RoiCorner { int64_t o[8]; float w[8]; bool ok; };

__device__ inline RoiCorner roi_corners(const RoiGeom &g, float y, float x, float z, bool backward) {
  RoiCorner r;
  r.ok = !(y < -1.0f || y > g.height || x < -1.0f || x > g.width || z < -1.0f || (backward && z > g.zsize));
  if (!r.ok) return r;
  if (y <= 0) y = 0;
  if (x <= 0) x = 0;
  if (z <= 0) z = 0;
  int y_low = (int)y, x_low = (int)x, z_low = (int)z, y_high, x_high, z_high;
  if (y_low >= g.height - 1) { y_high = y_low = g.height - 1; y = (float)y_low; } else y_high = y_low + 1;
  if (x_low >= g.width - 1) { x_high = x_low = g.width - 1; x = (float)x_low; } else x_high = x_low + 1;
  if (z_low >= g.zsize - 1) { z_high = z_low = g.zsize - 1; z = (float)z_low; } else z_high = z_low + 1;
  const float ly = y - y_low, lx = x - x_low, lz = z - z_low;
  const float hy = 1.f - ly, hx = 1.f - lx, hz = 1.f - lz;
  r.w[0] = hy * hx * hz; r.w[1] = hy * lx * hz; r.w[2] = ly * hx * hz; r.w[3] = ly * lx * hz;
  r.w[4] = hy * hx * lz; r.w[5] = hy * lx * lz; r.w[6] = ly * hx * lz; r.w[7] = ly * lx * lz;
  r.o[0] = ((int64_t)y_low * g.width + x_low) * g.zsize + z_low;
  r.o[1] = ((int64_t)y_low * g.width + x_high) * g.zsize + z_low;
  r.o[2] = ((int64_t)y_high * g.width + x_low) * g.zsize + z_low;
  r.o[3] = ((int64_t)y_high * g.width + x_high) * g.zsize + z_low;
  r.o[4] = ((int64_t)y_low * g.width + x_low) * g.zsize + z_high;
  r.o[5] = ((int64_t)y_low * g.width + x_high) * g.zsize + z_high;
  r.o[6] = ((int64_t)y_high * g.width + x_low) * g.zsize + z_high;
  r.o[7] = ((int64_t)y_high * g.width + x_high) * g.zsize + z_high;
  return r;
}

} // namespace aabr

// point_reader.h -- how the voxel-scatter kernels are handed point i of the caller's coordinate tensor.
//
// The input layer has two coordinate layouts (SparseConvNet/sparseconvnet/ioLayers.py:15-65 InputLayer, :92-136
// BLInputLayer; IOLayersRules.h:18-125 inputLayerRules, :127-297 blRules).  The insert, numbering and prepare kernels
// (voxel_scatter.hip, brick.hip) are the same for both; what differs is where a point's (x, y, z, batch) comes from and
// when the layer skips the point.  That difference lives HERE and nowhere else: the kernels take a reader as a template
// parameter and call load() / classify() (pt_read: both).
//
//   FlatReader  int64 [n, ncols] rows (ncols 3 or 4, 4th column = batch index).  A row is skipped when x == y == z == -1,
//               the sentinel aabr_quantize_points gives a point outside FULL_SCALE (the reference drops those on the host).
//               FlatReader16: the same list with ncols == 4 at a 16-byte aligned address, read with 16-byte loads.
//   BLReader    int64 [B, L, 3] read where it lies: point i is flat row i = b * L + l, batch index = i / L (no [B L, 4]
//               copy).  A row is skipped if and only if x < 0, whatever y and z hold -- the reference's `if (p[0] >= 0)`
//               (IOLayersRules.h:188,203,256).
// Both report every other coordinate outside [0, 65534] as an error (kPtBad): the reference would create a site outside
// the grid for it.
#pragma once
#include "common.h"

namespace aabr {

enum { kPtOk = 0, kPtSkip = 1, kPtBad = 2 };

__device__ inline bool pt_out_of_range(int64_t x, int64_t y, int64_t z, int64_t b) {
  return x < 0 || y < 0 || z < 0 || b < 0 || x > kMaxCoord || y > kMaxCoord || z > kMaxCoord || b > kMaxCoord;
}

struct FlatRule {   // when the flat list's layer skips a row
  __device__ inline int classify(int64_t x, int64_t y, int64_t z, int64_t b) const {
    if (x == -1 && y == -1 && z == -1) return kPtSkip;
    return pt_out_of_range(x, y, z, b) ? kPtBad : kPtOk;
  }
};
struct FlatReader : FlatRule {
  int ncols;
  __device__ inline void load(const int64_t *__restrict__ coords, int64_t i, int64_t &x, int64_t &y, int64_t &z,
                              int64_t &b) const {
    const int64_t *c = coords + i * ncols;
    x = c[0]; y = c[1]; z = c[2]; b = ncols == 4 ? c[3] : 0;
  }
};
// ncols == 4 and a 16-byte aligned list: 32 bytes per point in two 16-byte loads
struct FlatReader16 : FlatRule {
  __device__ inline void load(const int64_t *__restrict__ coords, int64_t i, int64_t &x, int64_t &y, int64_t &z,
                              int64_t &b) const {
    const int64_t *c = coords + i * 4;
    const longlong2 a = *reinterpret_cast<const longlong2 *>(c), b2 = *reinterpret_cast<const longlong2 *>(c + 2);
    x = a.x; y = a.y; z = b2.x; b = b2.y;
  }
};
__host__ __device__ inline FlatReader flat_reader(int ncols) {
  FlatReader r;
  r.ncols = ncols;
  return r;
}

struct BLReader {
  uint32_t L;     // row length; n = B * L < 2^31, so the batch index is one 32-bit division
  __device__ inline void load(const int64_t *__restrict__ coords, int64_t i, int64_t &x, int64_t &y, int64_t &z,
                              int64_t &b) const {
    const int64_t *c = coords + i * 3;
    x = c[0]; y = c[1]; z = c[2];
    b = (int64_t)((uint32_t)i / L);
  }
  __device__ inline int classify(int64_t x, int64_t y, int64_t z, int64_t b) const {
    if (x < 0) return kPtSkip;
    return pt_out_of_range(x, y, z, b) ? kPtBad : kPtOk;
  }
};

// load + classify in one call
template <typename Reader>
__device__ inline int pt_read(const Reader &rd, const int64_t *__restrict__ coords, int64_t i, int64_t &x, int64_t &y,
                              int64_t &z, int64_t &b) {
  rd.load(coords, i, x, y, z, b);
  return rd.classify(x, y, z, b);
}

} // namespace aabr

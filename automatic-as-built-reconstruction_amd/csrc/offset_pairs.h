// offset_pairs.h -- layout of the offset-major compacted pair list (built by k_offset_bases / k_fill_offset_pairs in
// conv.hip) and the chunk-to-workgroup scheme its readers share: the weight-gradient kernels of conv_dw.hip and the
// single-rule convolution of conv_single.hip.
//   words: [vol] R_k | [vol+1] first 1024-pair chunk of offset k | [vol+1] first 256-pair chunk |
//          [vol][nb256] block bases | [vol][V][2] pairs (partner row, row), ascending row order per offset
#pragma once
#include "common.h"

namespace aabr {

__host__ __device__ inline int64_t op_hdr(int vol) { return (int64_t)vol + 2 * (vol + 1); }
__host__ __device__ inline int64_t op_nb256(int64_t V) { return (V + 255) / 256; }

// The offset k and pair range [p0, p1) of chunk `chunk` (chunk_pairs = 1024 or 256; `direct`: chunk = offset, all of its
// pairs).  The grid is a host-side bound on the chunk count: false = a surplus workgroup (workgroup-uniform), which exits.
__device__ inline bool dw_chunk_range(const int32_t *__restrict__ words, int vol, int chunk_pairs, int direct, int chunk,
                                      int lane, int &k, int &p0, int &p1) {
  if (direct) {
    k = chunk;
    p0 = 0;
    p1 = words[k];
    return true;
  }
  const int32_t *cstart = words + vol + (chunk_pairs == 256 ? vol + 1 : 0);
  if (chunk >= cstart[vol]) return false;                  // workgroup-uniform
  k = 0;
  for (int k0 = 0; k0 < vol; k0 += 64) {
    int kk = k0 + lane;
    bool mine = kk < vol && cstart[kk] <= chunk && chunk < cstart[kk + 1];
    unsigned long long m = __ballot(mine);
    if (m) { k = k0 + (__ffsll((long long)m) - 1); break; }
  }
  const int rk = words[k];
  p0 = (chunk - cstart[k]) * chunk_pairs;
  p1 = p0 + chunk_pairs;
  if (p1 > rk) p1 = rk;
  return true;
}

} // namespace aabr

// roi_pool.hip -- the multi-level ROI pooler of the box head (Pooler.forward, maskrcnn_benchmark/modeling/poolers_3d.py:
// 73-168, with FPN2MLPFeatureExtractor.convert_metric_to_pixel, roi_box_feature_extractors.py:108-114), gfx950.
//
// The reference runs, per call: a chain of small torch ops that turn the yx_zb proposals into ROI rows and pick a level
// per box, then per level a torch.nonzero (a host read), an index, one ROIAlignRotated3D and an indexed write into a
// zero-filled result.  Here it is two launches whatever the level count, and no host read:
//   k_roi_pool_prepare  all scenes' boxes -> rois [N, 8] and levels [N]
//   k_roi_pool<false>   one ROI x 128 planes per workgroup, as k_roi_align_rot3d_sparse (roi.hip); the workgroup reads
//                       its ROI's level and takes that level's features, cell map, extent and scale from a by-value
//                       table in the kernel arguments.  Every output element is written: no zero fill.
// and backward one memset of the levels' gradient rows (ONE allocation, sliced per level by the caller) + k_roi_pool<true>.
// The walk over bins and samples, the LDS staging and the corner arithmetic (roi_shared.h) are k_roi_align_rot3d_sparse's,
// statement for statement, so the forward result is bit-identical to running that kernel on each level's ROI subset.
//
// Feature storage FT (float, __bf16; aabr_roi_pool_*_bf16): the forward's eight corner loads widen a bf16 value (exact),
// nothing else knows the storage, and the output stays fp32.  The backward kernel never reads the features: the bf16
// entry runs the SAME k_roi_pool<true> with its fp32 atomics into a caller-provided fp32 buffer and rounds that once
// into the bf16 gradient rows (aabr_cast_storage): 1 memset + 2 launches.  Nothing is accumulated in bf16.
//
// Pooled storage OT (float, __bf16; aabr_roi_pool_*_pooled_bf16) of top / top_diff: the forward's final store out of
// stage[] (and the zero fill of a missing level) rounds the fp32 value once, nearest even; the backward's staging loads
// of top_diff widen (exact).  Forward instances FT x OT = 4, backward OT = 2 (FT plays no part there).
#include "common.h"
#include "roi_shared.h"

namespace aabr {

constexpr int kPoolMaxLevels = 8;  // levels per call (the reference's configurations use 1 .. 3)
constexpr int kPoolMaxScenes = 16; // scenes per call, as roi_post / roi_loss (their prefix table travels by value too)

struct PoolPrepare {
  int64_t end[kPoolMaxScenes]; // end[b] = first row after scene b
  float scales[kPoolMaxLevels];
  int nb, n_levels;
  float box_scale, canonical_size;
};

// One thread per box: what convert_metric_to_pixel (roi_box_feature_extractors.py:108-114), Pooler.convert_to_roi_format
// (poolers_3d.py:107-124) with BoxList3D.convert('standard') (bounding_box_3d.py:293-312) and the constructor's limit_yaw
// (bounding_box_3d.py:203, utils3d/geometric_torch.py:4-10,88-97), and LevelMapper_3d.__call__ (poolers_3d.py:57-69)
// compute -- the fp32 operations of those torch expressions in their order, as CPU torch evaluates them.  `/` and sqrtf
// are the correctly rounded forms under this build's flags (hipcc's default for HIP; nms_shared.h relies on the same),
// -ffp-contract=off keeps every product and sum apart.  CUDA torch divides a tensor by a CPU scalar as a multiplication
// with the reciprocal; this follows the CPU form, a true division, as nms_shared.h does for limit_period.
__global__ __launch_bounds__(256) void k_roi_pool_prepare(const float *__restrict__ boxes, int64_t N, PoolPrepare pp,
                                                          float *__restrict__ rois, int32_t *__restrict__ levels) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int scene = 0;
  while (scene + 1 < pp.nb && i >= pp.end[scene]) ++scene;
  const float *b = boxes + 7 * i;
  float p[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) p[d] = b[d] * pp.box_scale;                 // prop.bbox3d[:, 0:6] *= voxel_scale
  const float period = 3.14159274101257324f;                              // (float)pi
  float t = b[6] + 1.57079637050628662f;                                  // bbox3d1[:, -1] += math.pi * 0.5
  t = t - floorf(t / period + 0.f) * period;                              // limit_period(yaws, 0, math.pi): [0, pi)
  float *r = rois + 8 * i;
  r[0] = (float)scene;
  r[1] = p[1];                                                            // rois[:, [0, 2, 1, 3, 5, 4, 6, 7]]
  r[2] = p[0];
  r[3] = p[2] + p[5] * 0.5f;                                              // bbox3d1[:, 2] += bbox3d0[:, 5] * 0.5
  r[4] = p[3];
  r[5] = p[4];
  r[6] = p[5];
  r[7] = t * 57.2957801818847656f;                                        // rois[:, -1] *= 180.0 / math.pi
  // LevelMapper_3d: torch.max(dim=1) hands a NaN on (fmaxf would drop it), sqrt of a negative size is NaN
  const float m = (p[3] != p[3] || p[4] != p[4]) ? __builtin_nanf("") : (p[3] > p[4] ? p[3] : p[4]);
  const float rate = sqrtf(m) / pp.canonical_size;
  // torch.argmin: the first index of the minimum; a NaN is the minimum, the first one by index
  int best = 0;
  float bd = fabsf(pp.scales[0] - rate);
  for (int l = 1; l < pp.n_levels; ++l) {
    const float d = fabsf(pp.scales[l] - rate);
    if (bd == bd && (d != d || d < bd)) { bd = d; best = l; }             // bd NaN: it stays the minimum
  }
  levels[i] = best;
}

struct PoolLevel {
  const void *feats;         // [V, C] in the storage FT of the forward instance; null: a level without sites
  const int32_t *cellmap;    // [nb, height, width, zsize]
  float *d_feats;            // backward: this level's rows of the shared gradient allocation
  int32_t height, width, zsize, nb;
  float scale;
  int32_t pad_;
};
struct PoolLevels {
  PoolLevel l[kPoolMaxLevels];
  int n;
};

template <bool BACKWARD, typename FT, typename OT>
__global__ __launch_bounds__(256) void k_roi_pool(PoolLevels lv, int C, const float *__restrict__ rois,
                                                  const int32_t *__restrict__ levels, int ph_, int pw_, int pz_,
                                                  int sampling, OT *__restrict__ top,
                                                  const OT *__restrict__ top_diff) {
  extern __shared__ float stage[]; // [kRoiPlanes][kRoiBins] bins of this pass (forward: results; backward: top_diff)
  const int64_t n = blockIdx.x;
  const int c0 = blockIdx.y * kRoiPlanes;
  const int nbins = ph_ * pw_ * pz_;
  const int64_t obase = (n * C + c0) * (int64_t)nbins; // top[n][c0 + .][bin]
  const int level = levels[n];                         // workgroup-uniform
  const bool level_ok = level >= 0 && level < lv.n;
  // the table is indexed with the clamped level only: an index outside it cannot come out of prepare, and reads nothing
  const PoolLevel &L = lv.l[level_ok ? level : 0];
  if (!level_ok || L.feats == nullptr) { // no such level / a level without sites: zeros forward, nothing backward
    if (!BACKWARD) {
      for (int i = threadIdx.x; i < kRoiPlanes * nbins; i += 256) {
        const int pc = i / nbins, pb = i - pc * nbins;
        if (c0 + pc < C) top[obase + (int64_t)pc * nbins + pb] = (OT)0.f;
      }
    }
    return;
  }
  RoiGeom g;
  g.channels = C; g.height = L.height; g.width = L.width; g.zsize = L.zsize;
  g.ph = ph_; g.pw = pw_; g.pz = pz_; g.sampling = sampling; g.scale = L.scale;
  const FT *__restrict__ feats = (const FT *)L.feats;
  const int32_t *__restrict__ cellmap = L.cellmap;
  float *d_feats = L.d_feats;
  const int B = L.nb;
  // ---- from here on: k_roi_align_rot3d_sparse (roi.hip), statement for statement
  const int lane_c = threadIdx.x & (kRoiPlanes - 1), half = threadIdx.x >> 7; // two bin streams per workgroup
  const int c = c0 + lane_c;
  const bool c_ok = c < C;
  const float *r = rois + n * 8;
  const int b = (int)r[0];
  const float cw = r[1] * g.scale, ch = r[2] * g.scale, cz = r[3] * g.scale;
  float rw = r[4] * g.scale, rh = r[5] * g.scale, rz = r[6] * g.scale;
  const float theta = (float)(r[7] * 3.14159265358979323846 / 180.0);
  rw = fmaxf(rw, 1.f); rh = fmaxf(rh, 1.f); rz = fmaxf(rz, 1.f);
  const float bh = rh / (float)g.ph, bw = rw / (float)g.pw, bz = rz / (float)g.pz;
  const int gh = g.sampling > 0 ? g.sampling : (int)ceilf(rh / g.ph);
  const int gw = g.sampling > 0 ? g.sampling : (int)ceilf(rw / g.pw);
  const int gz = g.sampling > 0 ? g.sampling : (int)ceilf(rz / g.pz);
  const float sh = -rh / 2.0f, sw = -rw / 2.0f, sz = -rz / 2.0f;
  const float ct = cosf(theta), st = sinf(theta);
  const float count = (float)(gh * gw * gz);
  const bool b_ok = b >= 0 && b < B;
  const int32_t *cm = cellmap + (int64_t)(b_ok ? b : 0) * g.height * g.width * g.zsize;

  for (int bin0 = 0; bin0 < nbins; bin0 += kRoiBins) {
    const int nb = (nbins - bin0) < kRoiBins ? (nbins - bin0) : kRoiBins;
    if (BACKWARD) { // stage this pass's output gradients: contiguous runs per plane
      for (int i = threadIdx.x; i < kRoiPlanes * nb; i += 256) {
        const int pc = i / nb, pb = i - pc * nb;
        stage[pc * kRoiBins + pb] = (c0 + pc < C) ? (float)top_diff[obase + (int64_t)pc * nbins + bin0 + pb] : 0.f;
      }
      __syncthreads();
    }
    for (int lb = half; lb < nb; lb += 2) {
      const int bin = bin0 + lb;
      const int pz = bin % g.pz, pw = (bin / g.pz) % g.pw, ph = bin / g.pz / g.pw;
      const float tdiff = BACKWARD ? stage[lane_c * kRoiBins + lb] : 0.f;
      float acc = 0.f;
      for (int iy = 0; iy < gh; iy++) {
        const float yy = sh + ph * bh + (iy + .5f) * bh / (float)gh;
        for (int ix = 0; ix < gw; ix++) {
          const float xx = sw + pw * bw + (ix + .5f) * bw / (float)gw;
          for (int iz = 0; iz < gz; iz++) {
            const float zz = sz + pz * bz + (iz + .5f) * bz / (float)gz;
            const float x = xx * ct + yy * st + cw;
            const float y = yy * ct - xx * st + ch;
            const float z = zz + cz;
            const RoiCorner q = roi_corners(g, y, x, z, BACKWARD);
            if (!q.ok) continue; // forward: trilinear() returns 0, acc += 0 changes nothing
            if (!BACKWARD) {
              float v[8];
#pragma unroll
              for (int t = 0; t < 8; ++t) {
                const int32_t row = b_ok ? cm[q.o[t]] : -1; // workgroup-uniform address: one broadcast load
                v[t] = (row >= 0 && c_ok) ? (float)feats[(int64_t)row * C + c] : 0.f;
              }
              acc += (q.w[0] * v[0] + q.w[1] * v[1] + q.w[2] * v[2] + q.w[3] * v[3] + q.w[4] * v[4] + q.w[5] * v[5] +
                      q.w[6] * v[6] + q.w[7] * v[7]);
            } else {
#pragma unroll
              for (int t = 0; t < 8; ++t) {
                const int32_t row = b_ok ? cm[q.o[t]] : -1;
                if (row >= 0 && c_ok) atomicAdd(d_feats + (int64_t)row * C + c, tdiff * q.w[t] / count);
              }
            }
          }
        }
      }
      if (!BACKWARD) stage[lane_c * kRoiBins + lb] = acc / count;
    }
    __syncthreads();
    if (!BACKWARD) {
      for (int i = threadIdx.x; i < kRoiPlanes * nb; i += 256) {
        const int pc = i / nb, pb = i - pc * nb;
        if (c0 + pc < C) top[obase + (int64_t)pc * nbins + bin0 + pb] = (OT)stage[pc * kRoiBins + pb];
      }
      __syncthreads();
    }
  }
}

} // namespace aabr
using namespace aabr;

extern "C" int aabr_roi_pool_prepare(const float *boxes, int nb, const int64_t *n_host, float box_scale, int n_levels,
                                     const float *scales_host, float canonical_size, float *rois, int32_t *levels,
                                     void *stream_) {
  AABR_CHECK_ARG(n_levels >= 1 && n_levels <= kPoolMaxLevels, "n_levels must be 1 .. 8");
  AABR_CHECK_ARG(nb >= 1 && nb <= kPoolMaxScenes, "nb must be 1 .. 16");
  AABR_CHECK_ARG(n_host && scales_host, "null host array");
  PoolPrepare pp;
  int64_t N = 0;
  for (int b = 0; b < kPoolMaxScenes; ++b) {
    if (b < nb) {
      AABR_CHECK_ARG(n_host[b] >= 0, "negative count");
      N += n_host[b];
    }
    pp.end[b] = N;
  }
  for (int l = 0; l < kPoolMaxLevels; ++l) pp.scales[l] = l < n_levels ? scales_host[l] : 0.f;
  pp.nb = nb; pp.n_levels = n_levels; pp.box_scale = box_scale; pp.canonical_size = canonical_size;
  if (N == 0) return AABR_OK;
  AABR_CHECK_ARG(boxes && rois && levels, "null pointer");
  hipLaunchKernelGGL(k_roi_pool_prepare, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, (hipStream_t)stream_, boxes, N,
                     pp, rois, levels);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// the checks both gather entry points share; fills the device table
static int pool_levels(PoolLevels &lv, const AabrRoiLevel *d, int n_levels, int channels, int batch_size, int64_t num_rois,
                       int ph, int pw, int pz, bool backward, float *d_feats_all, int64_t total_rows,
                       const char **why) {
  *why = "n_levels must be 1 .. 8";
  if (n_levels < 1 || n_levels > kPoolMaxLevels) return -1;
  *why = "negative count / bad geometry";
  if (num_rois < 0 || channels <= 0 || batch_size < 0 || ph <= 0 || pw <= 0 || pz <= 0 || total_rows < 0) return -1;
  *why = "null level table";
  if (!d) return -1;
  lv.n = n_levels;
  for (int l = 0; l < kPoolMaxLevels; ++l) {
    PoolLevel &L = lv.l[l];
    L = PoolLevel{nullptr, nullptr, nullptr, 1, 1, 1, 0, 1.f, 0};
    if (l >= n_levels) continue;
    *why = "negative V";
    if (d[l].V < 0) return -1;
    if (d[l].V == 0) continue; // a level without sites: zeros for its ROIs
    *why = "nb must be 1 .. batch_size";
    if (d[l].nb < 1 || d[l].nb > batch_size) return -1;
    *why = "bad extent";
    if (d[l].height <= 0 || d[l].width <= 0 || d[l].zsize <= 0) return -1;
    *why = "null feats / cellmap";
    if (!d[l].feats || !d[l].cellmap) return -1;
    L.feats = d[l].feats; L.cellmap = d[l].cellmap;
    L.height = d[l].height; L.width = d[l].width; L.zsize = d[l].zsize; L.nb = d[l].nb;
    L.scale = d[l].spatial_scale;
    if (backward) {
      *why = "row_offset + V outside total_rows";
      if (d[l].row_offset < 0 || d[l].row_offset > total_rows - d[l].V) return -1;
      L.d_feats = d_feats_all + d[l].row_offset * channels;
    }
  }
  *why = "too many planes";
  if (ceil_div(channels, kRoiPlanes) > 65535) return -1;
  return 0;
}

template <typename FT, typename OT>
static int roi_pool_forward(const char *fn, const AabrRoiLevel *levels_desc_host, int n_levels, int channels,
                            int batch_size, const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h,
                            int pooled_w, int pooled_z, int sampling_ratio, OT *output, hipStream_t st) {
  PoolLevels lv;
  const char *why = "";
  const int rc = pool_levels(lv, levels_desc_host, n_levels, channels, batch_size, num_rois, pooled_h, pooled_w,
                             pooled_z, false, nullptr, 0, &why);
  AABR_CHECK_ARG_AS(fn, rc == 0, why);
  if (num_rois == 0) return AABR_OK;
  AABR_CHECK_ARG_AS(fn, rois && levels && output, "null pointer");
  hipLaunchKernelGGL((k_roi_pool<false, FT, OT>), dim3((unsigned)num_rois, (unsigned)ceil_div(channels, kRoiPlanes)),
                     dim3(256), (size_t)kRoiPlanes * kRoiBins * sizeof(float), st, lv, channels, rois, levels, pooled_h,
                     pooled_w, pooled_z, sampling_ratio, output, (const OT *)nullptr);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_pool_forward(const AabrRoiLevel *levels_desc_host, int n_levels, int channels, int batch_size,
                                     const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h,
                                     int pooled_w, int pooled_z, int sampling_ratio, float *output, void *stream_) {
  return roi_pool_forward<float, float>(__func__, levels_desc_host, n_levels, channels, batch_size, rois, levels, num_rois,
                                 pooled_h, pooled_w, pooled_z, sampling_ratio, output, (hipStream_t)stream_);
}

extern "C" int aabr_roi_pool_forward_bf16(const AabrRoiLevel *levels_desc_host, int n_levels, int channels,
                                          int batch_size, const float *rois, const int32_t *levels, int64_t num_rois,
                                          int pooled_h, int pooled_w, int pooled_z, int sampling_ratio, float *output,
                                          void *stream_) {
  for (int l = 0; levels_desc_host && l < n_levels && l < kPoolMaxLevels; ++l)
    AABR_CHECK_ARG(((uintptr_t)levels_desc_host[l].feats & 3) == 0, "feats must be 4-byte aligned");
  return roi_pool_forward<__bf16, float>(__func__, levels_desc_host, n_levels, channels, batch_size, rois, levels, num_rois,
                                  pooled_h, pooled_w, pooled_z, sampling_ratio, output, (hipStream_t)stream_);
}

// the memset + launch of the backward entry points; OT: the storage of grad_output
template <typename OT>
static int roi_pool_backward(const char *fn, const AabrRoiLevel *levels_desc_host, int n_levels, int channels,
                             int batch_size, const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h,
                             int pooled_w, int pooled_z, int sampling_ratio, const OT *grad_output, float *d_feats_all,
                             int64_t total_rows, hipStream_t st) {
  PoolLevels lv;
  const char *why = "";
  const int rc = pool_levels(lv, levels_desc_host, n_levels, channels, batch_size, num_rois, pooled_h, pooled_w,
                             pooled_z, true, d_feats_all, total_rows, &why);
  AABR_CHECK_ARG_AS(fn, rc == 0, why);
  AABR_CHECK_ARG_AS(fn, d_feats_all || total_rows == 0, "null d_feats_all");
  if (total_rows > 0) hipMemsetAsync(d_feats_all, 0, (size_t)total_rows * channels * sizeof(float), st);
  if (num_rois == 0 || total_rows == 0) return AABR_OK;
  AABR_CHECK_ARG_AS(fn, rois && levels && grad_output, "null pointer");
  hipLaunchKernelGGL((k_roi_pool<true, float, OT>), dim3((unsigned)num_rois, (unsigned)ceil_div(channels, kRoiPlanes)),
                     dim3(256), (size_t)kRoiPlanes * kRoiBins * sizeof(float), st, lv, channels, rois, levels, pooled_h,
                     pooled_w, pooled_z, sampling_ratio, (OT *)nullptr, grad_output);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_pool_backward(const AabrRoiLevel *levels_desc_host, int n_levels, int channels, int batch_size,
                                      const float *rois, const int32_t *levels, int64_t num_rois, int pooled_h,
                                      int pooled_w, int pooled_z, int sampling_ratio, const float *grad_output,
                                      float *d_feats_all, int64_t total_rows, void *stream_) {
  return roi_pool_backward<float>(__func__, levels_desc_host, n_levels, channels, batch_size, rois, levels, num_rois,
                                  pooled_h, pooled_w, pooled_z, sampling_ratio, grad_output, d_feats_all, total_rows,
                                  (hipStream_t)stream_);
}

extern "C" int aabr_roi_pool_backward_bf16(const AabrRoiLevel *levels_desc_host, int n_levels, int channels,
                                           int batch_size, const float *rois, const int32_t *levels, int64_t num_rois,
                                           int pooled_h, int pooled_w, int pooled_z, int sampling_ratio,
                                           const float *grad_output, float *accum_f32, void *d_feats_all_bf16,
                                           int64_t total_rows, void *stream_) {
  AABR_CHECK_ARG(total_rows <= 0 || (accum_f32 && d_feats_all_bf16), "null accum_f32 / d_feats_all_bf16");
  AABR_CHECK_ARG((((uintptr_t)accum_f32 | (uintptr_t)d_feats_all_bf16) & 3) == 0,
                 "accum_f32 / d_feats_all_bf16 must be 4-byte aligned");
  const int rc = aabr_roi_pool_backward(levels_desc_host, n_levels, channels, batch_size, rois, levels, num_rois, pooled_h,
                                        pooled_w, pooled_z, sampling_ratio, grad_output, accum_f32, total_rows, stream_);
  if (rc != AABR_OK || total_rows == 0) return rc;
  return aabr_cast_storage(accum_f32, d_feats_all_bf16, total_rows * channels, 1, stream_);
}

// ---- the pooled side in bf16 (OT = __bf16): the forward's last store rounds once, the backward widens top_diff ----

extern "C" int aabr_roi_pool_forward_pooled_bf16(const AabrRoiLevel *levels_desc_host, int n_levels, int channels,
                                                 int batch_size, const float *rois, const int32_t *levels,
                                                 int64_t num_rois, int pooled_h, int pooled_w, int pooled_z,
                                                 int sampling_ratio, int feats_bf16, void *output_bf16, void *stream_) {
  AABR_CHECK_ARG(levels_desc_host, "null levels_desc_host");
  AABR_CHECK_ARG(num_rois <= 0 || rois, "null rois");
  AABR_CHECK_ARG(num_rois <= 0 || levels, "null levels");
  AABR_CHECK_ARG(num_rois <= 0 || output_bf16, "null output_bf16");
  AABR_CHECK_ARG(((uintptr_t)output_bf16 & 3) == 0, "output_bf16 must be 4-byte aligned");
  for (int l = 0; feats_bf16 && l < n_levels && l < kPoolMaxLevels; ++l)
    AABR_CHECK_ARG(((uintptr_t)levels_desc_host[l].feats & 3) == 0, "feats must be 4-byte aligned");
  if (feats_bf16)
    return roi_pool_forward<__bf16, __bf16>(__func__, levels_desc_host, n_levels, channels, batch_size, rois, levels,
                                            num_rois, pooled_h, pooled_w, pooled_z, sampling_ratio,
                                            (__bf16 *)output_bf16, (hipStream_t)stream_);
  return roi_pool_forward<float, __bf16>(__func__, levels_desc_host, n_levels, channels, batch_size, rois, levels,
                                         num_rois, pooled_h, pooled_w, pooled_z, sampling_ratio, (__bf16 *)output_bf16,
                                         (hipStream_t)stream_);
}

extern "C" int aabr_roi_pool_backward_pooled_bf16(const AabrRoiLevel *levels_desc_host, int n_levels, int channels,
                                                  int batch_size, const float *rois, const int32_t *levels,
                                                  int64_t num_rois, int pooled_h, int pooled_w, int pooled_z,
                                                  int sampling_ratio, int feats_bf16, const void *grad_output_bf16,
                                                  float *accum_f32, void *d_feats_all_bf16_or_null, int64_t total_rows,
                                                  void *stream_) {
  AABR_CHECK_ARG(levels_desc_host, "null levels_desc_host");
  AABR_CHECK_ARG(num_rois <= 0 || rois, "null rois");
  AABR_CHECK_ARG(num_rois <= 0 || levels, "null levels");
  AABR_CHECK_ARG(num_rois <= 0 || total_rows <= 0 || grad_output_bf16, "null grad_output_bf16");
  AABR_CHECK_ARG(((uintptr_t)grad_output_bf16 & 3) == 0, "grad_output_bf16 must be 4-byte aligned");
  AABR_CHECK_ARG(total_rows <= 0 || accum_f32, "null accum_f32");
  AABR_CHECK_ARG(((uintptr_t)accum_f32 & 3) == 0, "accum_f32 must be 4-byte aligned");
  if (feats_bf16) {
    AABR_CHECK_ARG(total_rows <= 0 || d_feats_all_bf16_or_null, "null d_feats_all_bf16 (feats_bf16 = 1)");
    AABR_CHECK_ARG(((uintptr_t)d_feats_all_bf16_or_null & 3) == 0, "d_feats_all_bf16 must be 4-byte aligned");
  }
  const int rc = roi_pool_backward<__bf16>(__func__, levels_desc_host, n_levels, channels, batch_size, rois, levels,
                                           num_rois, pooled_h, pooled_w, pooled_z, sampling_ratio,
                                           (const __bf16 *)grad_output_bf16, accum_f32, total_rows, (hipStream_t)stream_);
  if (rc != AABR_OK || total_rows <= 0 || !feats_bf16) return rc;
  return aabr_cast_storage(accum_f32, d_feats_all_bf16_or_null, total_rows * channels, 1, stream_);
}

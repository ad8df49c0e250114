// corner_loss.hip -- the corner-connection losses of the corner-ROI box head (reference: the `*_corsem.yaml` configurations,
// MODEL.LOSS.WEIGHTS[4:7]): geometric_pull_loss, semantic_pull_loss, semantic_push_loss over the top corners of the sampled
// positive proposals.
//
// Label side, aabr_corner_tables (bounding_box_3d.py:270-291,451-477 get_2top_corners_offseted / get_connect_corner_ids;
// box_head_3d/loss.py:22-99 get_prop_ids_per_targ; :276-292 the remap to the sampled list).  The reference builds, per
// scene and on the host side of torch, a dense [2t, 2t] distance matrix, nonzero, three extract_order_ids passes, a sort of
// the positives and a loop over etpn = 4.  Here, for the whole batch (<= 16 scenes) and from the outputs of aabr_roi_targets:
//   C1 k_corner_tg_xyz      one thread per ground-truth box: yxzb_to_2corners + corners_top_offseted (corner_box.h);
//   C2 k_corner_tg_connect  one thread per ground-truth corner walks its scene's corners in ascending index and keeps the
//                           first three others closer than 0.1 (the diagonal is excluded; missing entries are -1);
//   C3 k_corner_prop_tables one workgroup per scene: the sampled rows with matched_idx >= 0 are the positives; each finds its
//                           place in the order (matched target, sampled position) by counting the positives before it
//                           (<= 512 of them in LDS: no per-target array, whatever the ground-truth count); a target's run
//                           of positives is then two binary searches in the sorted target list, its "first four" the first
//                           four of that run.  Per proposal corner the 16 candidate slots (own target corner + up to three
//                           connected target corners, four positives each, same corner parity) are sorted descending in
//                           registers and cut to 8; the corner's xyz comes from the sampled box.
// 3 launches whatever nb; no host read; every element of the padded outputs is written.
//
// Loss, aabr_corner_loss_forward / _backward (loss.py:384-499 corner_connection_loss).  The reference materialises
// [n, n, 8] and [n, n, 3] differences per scene (n = 2p corners) in a Python loop over scenes.  Here the pair (a, i) is
// visited by the threads that own column i: a workgroup owns kCornerTile columns of one scene, four threads per column
// sharing the rows a = r mod 4, and the scene's corners pass through LDS in tiles of kCornerTile rows.
//   L1 k_corner_loss_partial  pull / push / geometric sums in fp32 (per tile, then per thread, then a fixed tree per
//                             workgroup) and the three counts as integers;
//   L2 k_corner_loss_final    the workgroups' partials in workgroup order, the three means per scene, the mean over the
//                             scenes in scene order; the per-scene counts stay in device memory for the backward.
//   B1 k_corner_loss_backward gather form: column i's threads add the terms of (a, i) and of (i, a) -- the connected mask
//                             is not symmetric, so row a's table entries are staged too -- and write d corners_semantic of
//                             the positive rows; further workgroups of the same launch write zeros to the sampled rows that
//                             are no positive.  Every element is written.
// No float atomics: bit-identical run to run.
#include "common.h"
#include "corner_box.h"

namespace aabr {

namespace {

constexpr int kCornerMaxBatch = 16;      // scenes per call, as aabr_roi_targets
constexpr int kCornerMaxB = 512;         // sampled rows per scene, as aabr_roi_targets (batch_size_per_image)
constexpr int kCornerTile = 64;          // corners per tile of the loss kernels
constexpr int kCornerMaxTiles = 2 * kCornerMaxB / kCornerTile;
constexpr int kCornerIds = 8;            // table entries per proposal corner (loss.py:89)
constexpr int kCornerTgIds = 3;          // connected corners per ground-truth corner (bounding_box_3d.py:469)
constexpr int kCornerEtpn = 4;           // positives kept per target (loss.py:39)
constexpr int kCornerInfoWords = 8;
constexpr int kCornerPartWords = 6;
constexpr float kCornerTgThreshold = 0.1f;     // get_connect_corner_ids(threshold=0.1)
constexpr float kCornerActive = 0.2f;          // corner_connection_loss(active_threshold=0.2)
constexpr float kCornerClose = 0.5f;           // cor_semantic_loss_f(geo_close_threshold=0.5)
constexpr float kCornerDelta = 1.0f;           // cor_semantic_loss_f(delta=1.0)

struct CornerTableParams {
  int64_t prop_begin[kCornerMaxBatch];   // first proposal row of scene b (matched_idx)
  int64_t gt_begin[kCornerMaxBatch + 1]; // first ground-truth row of scene b; [nb] = the total
  int32_t n[kCornerMaxBatch];
  int nb, B;
};

__global__ __launch_bounds__(256) void k_corner_tg_xyz(int64_t total, const float *__restrict__ targets,
                                                       float *__restrict__ tg_xyz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float b[7], c[7], o[6];
#pragma unroll
  for (int d = 0; d < 7; ++d) b[d] = targets[7 * i + d];
  yxzb_to_2corners(b, c);
  corners_top_offseted(c, o);
#pragma unroll
  for (int d = 0; d < 6; ++d) tg_xyz[6 * i + d] = o[d];
}

__global__ __launch_bounds__(256) void k_corner_tg_connect(CornerTableParams p, const float *__restrict__ tg_xyz,
                                                           int32_t *__restrict__ tg_connect) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // corner of the batch
  if (i >= 2 * p.gt_begin[p.nb]) return;
  int b = 0;
  while (b + 1 < p.nb && i >= 2 * p.gt_begin[b + 1]) ++b;
  const int64_t c0 = 2 * p.gt_begin[b], m = 2 * (p.gt_begin[b + 1] - p.gt_begin[b]);
  const float x = tg_xyz[3 * i], y = tg_xyz[3 * i + 1], z = tg_xyz[3 * i + 2];
  int found = 0;
  for (int64_t j = 0; j < m && found < kCornerTgIds; ++j) {
    if (c0 + j == i) continue;
    const float dx = x - tg_xyz[3 * (c0 + j)], dy = y - tg_xyz[3 * (c0 + j) + 1], dz = z - tg_xyz[3 * (c0 + j) + 2];
    if (sqrtf(dx * dx + dy * dy + dz * dz) < kCornerTgThreshold) tg_connect[kCornerTgIds * i + found++] = (int32_t)j;
  }
  for (; found < kCornerTgIds; ++found) tg_connect[kCornerTgIds * i + found] = -1;
}

__global__ __launch_bounds__(256) void k_corner_prop_tables(CornerTableParams p, const int64_t *__restrict__ matched_idx,
                                                            const int64_t *__restrict__ samp_rows,
                                                            const float *__restrict__ samp_boxes,
                                                            const int32_t *__restrict__ tg_connect,
                                                            int64_t *__restrict__ pos_pos, int32_t *__restrict__ connect_ids,
                                                            float *__restrict__ corner_xyz, int32_t *__restrict__ info) {
  __shared__ int s_tgt[kCornerMaxB];        // matched target of sampled position s, -1: no positive
  __shared__ int s_sorted_tgt[kCornerMaxB]; // matched target of the k-th positive in (target, position) order
  __shared__ int s_sorted_pos[kCornerMaxB]; // its sampled position
  __shared__ int s_p;
  const int b = blockIdx.x, t = threadIdx.x, B = p.B;
  const int64_t G = p.gt_begin[b + 1] - p.gt_begin[b];
  if (t == 0) s_p = 0;
  for (int s = t; s < B; s += 256) {
    const int64_t row = samp_rows[(int64_t)b * B + s];
    int64_t tg = -1;
    if (row >= 0 && row < p.n[b]) tg = matched_idx[p.prop_begin[b] + row];
    s_tgt[s] = (tg >= 0 && tg < G) ? (int)tg : -1;
  }
  __syncthreads();
  for (int s = t; s < B; s += 256) {
    const int tg = s_tgt[s];
    if (tg < 0) continue;
    int k = 0;
    for (int q = 0; q < B; ++q) {
      const int o = s_tgt[q];
      k += (o >= 0 && (o < tg || (o == tg && q < s))) ? 1 : 0;
    }
    s_sorted_tgt[k] = tg;
    s_sorted_pos[k] = s;
    atomicAdd(&s_p, 1);
  }
  __syncthreads();
  const int np = s_p;
  const int32_t *conn = tg_connect + kCornerTgIds * 2 * p.gt_begin[b];
  for (int k = t; k < B; k += 256) pos_pos[(int64_t)b * B + k] = k < np ? s_sorted_pos[k] : -1;
  for (int i = t; i < 2 * B; i += 256) {
    int32_t *ids = connect_ids + ((int64_t)b * 2 * B + i) * kCornerIds;
    float *xyz = corner_xyz + ((int64_t)b * 2 * B + i) * 3;
    const int k = i >> 1, cc = i & 1;
    if (k >= np) {
#pragma unroll
      for (int q = 0; q < kCornerIds; ++q) ids[q] = -1;
      xyz[0] = xyz[1] = xyz[2] = 0.f;
      continue;
    }
    const int tc = 2 * s_sorted_tgt[k] + cc;           // this corner's ground-truth corner
    int cand[(1 + kCornerTgIds) * kCornerEtpn];
#pragma unroll
    for (int g = 0; g < 1 + kCornerTgIds; ++g) {
      const int e = g == 0 ? tc : conn[kCornerTgIds * tc + (g - 1)];
      int lo = 0, cnt = 0;
      if (e >= 0 && e < 2 * G) {
        const int x = e >> 1;
        int l = 0, h = np;
        while (l < h) { const int m = (l + h) >> 1; if (s_sorted_tgt[m] < x) l = m + 1; else h = m; }
        lo = l;
        h = np;
        while (l < h) { const int m = (l + h) >> 1; if (s_sorted_tgt[m] <= x) l = m + 1; else h = m; }
        cnt = l - lo;
      }
#pragma unroll
      for (int j = 0; j < kCornerEtpn; ++j) cand[g * kCornerEtpn + j] = j < cnt ? 2 * (lo + j) + (e & 1) : -1;
    }
    // descending, in registers: 16 slots
#pragma unroll
    for (int u = 0; u < (1 + kCornerTgIds) * kCornerEtpn - 1; ++u)
#pragma unroll
      for (int v = 0; v < (1 + kCornerTgIds) * kCornerEtpn - 1 - u; ++v) {
        const int lo_ = cand[v] < cand[v + 1] ? cand[v] : cand[v + 1], hi_ = cand[v] < cand[v + 1] ? cand[v + 1] : cand[v];
        cand[v] = hi_;
        cand[v + 1] = lo_;
      }
#pragma unroll
    for (int q = 0; q < kCornerIds; ++q) ids[q] = cand[q];
    float bx[7], c2[7], o[6];
    const float *src = samp_boxes + ((int64_t)b * B + s_sorted_pos[k]) * 7;
#pragma unroll
    for (int d = 0; d < 7; ++d) bx[d] = src[d];
    yxzb_to_2corners(bx, c2);
    corners_top_offseted(c2, o);
    xyz[0] = o[3 * cc]; xyz[1] = o[3 * cc + 1]; xyz[2] = o[3 * cc + 2];
  }
  if (t == 0) {
    int32_t *inf = info + b * kCornerInfoWords;
    inf[0] = np;
    inf[1] = (int32_t)G;
#pragma unroll
    for (int q = 2; q < kCornerInfoWords; ++q) inf[q] = 0;
  }
}

// ---- the loss -----------------------------------------------------------------------------------------------------------
struct CornerLossParams {
  const int64_t *pos_pos[kCornerMaxBatch];   // [p_b]: sampled position of the k-th positive
  const int32_t *ids[kCornerMaxBatch];       // [2 p_b, 8]
  const float *xyz[kCornerMaxBatch];         // [2 p_b, 3]
  int64_t seg_begin[kCornerMaxBatch];        // first row of scene b's sample in corners_semantic
  int32_t m[kCornerMaxBatch];                // rows of scene b's sample
  int32_t p[kCornerMaxBatch];                // its positives
  int nb;
};

// what the threads of column i keep of their own corner
struct CornerOwn {
  float sem[8], xyz[3];
  int ids[kCornerIds];
  int64_t row;          // row of corners_semantic, -1: none
  bool valid;
};

__device__ inline CornerOwn corner_own(const CornerLossParams &p, int b, int i, int n, const float *__restrict__ sem) {
  CornerOwn o;
  o.valid = i < n;
  o.row = -1;
#pragma unroll
  for (int q = 0; q < 8; ++q) { o.sem[q] = 0.f; o.ids[q] = -1; }
  o.xyz[0] = o.xyz[1] = o.xyz[2] = 0.f;
  if (!o.valid) return o;
  const int64_t pos = p.pos_pos[b][i >> 1];
  if (pos >= 0 && pos < p.m[b]) {
    o.row = p.seg_begin[b] + pos;
#pragma unroll
    for (int q = 0; q < 8; ++q) o.sem[q] = sem[o.row * 16 + (i & 1) * 8 + q];
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) o.xyz[d] = p.xyz[b][3 * (int64_t)i + d];
#pragma unroll
  for (int q = 0; q < kCornerIds; ++q) {
    const int e = p.ids[b][kCornerIds * (int64_t)i + q];
    o.ids[q] = (e >= 0 && e < n) ? e : -1;
  }
  return o;
}

struct CornerTileLds {
  float sem[kCornerTile][8];
  float xyz[kCornerTile][4];
  int ids[kCornerTile][kCornerIds];
};

// rows a0 .. a0 + kCornerTile of scene b into LDS: thread (row, part) brings 4 + 4 semantic floats, the coordinates, and
// (kIds) the row's table entries
template <bool kIds>
__device__ inline void corner_stage(CornerTileLds &s, const CornerLossParams &p, int b, int a0, int n,
                                    const float *__restrict__ sem) {
  const int row = threadIdx.x >> 2, part = threadIdx.x & 3, a = a0 + row;
  if (a >= n) return;
  if (part < 2) {
    const int64_t pos = p.pos_pos[b][a >> 1];
    const bool ok = pos >= 0 && pos < p.m[b];
    const float *src = sem + (p.seg_begin[b] + (ok ? pos : 0)) * 16 + (a & 1) * 8 + 4 * part;
#pragma unroll
    for (int q = 0; q < 4; ++q) s.sem[row][4 * part + q] = ok ? src[q] : 0.f;
  } else if (part == 2) {
#pragma unroll
    for (int d = 0; d < 3; ++d) s.xyz[row][d] = p.xyz[b][3 * (int64_t)a + d];
  } else if (kIds) {
#pragma unroll
    for (int q = 0; q < kCornerIds; ++q) s.ids[row][q] = p.ids[b][kCornerIds * (int64_t)a + q];
  }
}

__device__ inline float corner_sem_dist(const float *a, const float *b) {
  float d2 = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) { const float d = a[q] - b[q]; d2 += d * d; }
  return sqrtf(d2);
}

__device__ inline float corner_geo_dist(const float *a, const float *b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

__device__ inline bool corner_in(const int *ids, int a) {
  bool in = false;
#pragma unroll
  for (int q = 0; q < kCornerIds; ++q) in = in || ids[q] == a;
  return in;
}

__global__ __launch_bounds__(256) void k_corner_loss_partial(CornerLossParams p, const float *__restrict__ sem,
                                                             int32_t *__restrict__ partial) {
  __shared__ CornerTileLds s;
  __shared__ float s_f[3][256];
  __shared__ int s_i[3][256];
  const int b = blockIdx.y, n = 2 * p.p[b], tile0 = blockIdx.x * kCornerTile;
  if (tile0 >= n) return;                                    // (workgroup-uniform; the final stage reads ceil(n / tile))
  const int t = threadIdx.x, r = t & 3, i = tile0 + (t >> 2);
  const CornerOwn own = corner_own(p, b, i, n, sem);
  float pull = 0.f, push = 0.f, geo = 0.f;
  int n_conn = 0, n_push = 0, n_geo = 0;
  for (int a0 = 0; a0 < n; a0 += kCornerTile) {
    __syncthreads();
    corner_stage<false>(s, p, b, a0, n, sem);
    __syncthreads();
    const int rows = n - a0 < kCornerTile ? n - a0 : kCornerTile;
    float t_pull = 0.f, t_push = 0.f;
    if (own.valid)
      for (int al = r; al < rows; al += 4) {
        const int a = a0 + al;
        const float d = corner_sem_dist(s.sem[al], own.sem);
        if (a == i || corner_in(own.ids, a)) {               // mask_connect[a, i]: a is i or one of i's table entries
          t_pull += d;
          ++n_conn;
        } else if (corner_geo_dist(s.xyz[al], own.xyz) < kCornerClose) {
          const float v = kCornerDelta - d;
          t_push += v < 0.f ? 0.f : v;
          ++n_push;
        }
      }
    pull += t_pull;
    push += t_push;
  }
  // the geometric pull over the table entries of corner i: thread r takes entries r and r + 4
#pragma unroll
  for (int q = 0; q < kCornerIds; ++q) {
    const int e = own.ids[q];
    if ((q & 3) == r && e >= 0) {
      float o[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) o[d] = p.xyz[b][3 * (int64_t)e + d];
      const float d = corner_geo_dist(o, own.xyz);
      if (d < kCornerActive) { geo += d; ++n_geo; }
    }
  }
  s_f[0][t] = pull; s_f[1][t] = push; s_f[2][t] = geo;
  s_i[0][t] = n_conn; s_i[1][t] = n_push; s_i[2][t] = n_geo;
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { s_f[k][t] += s_f[k][t + w]; s_i[k][t] += s_i[k][t + w]; }
    }
  }
  __syncthreads();
  if (t == 0) {
    int32_t *o = partial + ((int64_t)b * kCornerMaxTiles + blockIdx.x) * kCornerPartWords;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = __float_as_int(s_f[k][0]); o[3 + k] = s_i[k][0]; }
  }
}

// counts [nb][4]: geometric entries below the threshold, connected pairs, push pairs, corners
__global__ __launch_bounds__(64) void k_corner_loss_final(CornerLossParams p, const int32_t *__restrict__ partial,
                                                          float *__restrict__ losses, int32_t *__restrict__ counts) {
  __shared__ float s_l[3][kCornerMaxBatch];
  const int b = threadIdx.x;
  if (b < p.nb) {
    const int n = 2 * p.p[b], tiles = (n + kCornerTile - 1) / kCornerTile;
    float f[3] = {0.f, 0.f, 0.f};
    int c[3] = {0, 0, 0};
    for (int k = 0; k < tiles; ++k) {
      const int32_t *o = partial + ((int64_t)b * kCornerMaxTiles + k) * kCornerPartWords;
#pragma unroll
      for (int q = 0; q < 3; ++q) { f[q] += __int_as_float(o[q]); c[q] += o[3 + q]; }
    }
    const int d_pull = c[0] - n > 1 ? c[0] - n : 1, d_push = c[1] > 1 ? c[1] : 1, d_geo = c[2] - n > 1 ? c[2] - n : 1;
    s_l[0][b] = f[2] / (float)d_geo;
    s_l[1][b] = f[0] / (float)d_pull;
    s_l[2][b] = f[1] / (float)d_push;
    counts[4 * b] = c[2]; counts[4 * b + 1] = c[0]; counts[4 * b + 2] = c[1]; counts[4 * b + 3] = n;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float sum = 0.f;
    for (int k = 0; k < p.nb; ++k) sum += s_l[threadIdx.x][k];
    losses[threadIdx.x] = sum / (float)p.nb;
  }
}

__global__ __launch_bounds__(256) void k_corner_loss_backward(CornerLossParams p, int tiles_max,
                                                              const float *__restrict__ sem,
                                                              const int32_t *__restrict__ counts,
                                                              const float *__restrict__ g_pull_loss,
                                                              const float *__restrict__ g_push_loss,
                                                              float *__restrict__ d_sem) {
  __shared__ CornerTileLds s;
  const int b = blockIdx.y, n = 2 * p.p[b], t = threadIdx.x;
  if ((int)blockIdx.x >= tiles_max) {
    // zeros for the sampled rows of the scene that are no positive
    const int row = ((int)blockIdx.x - tiles_max) * 256 + t;
    if (row >= p.m[b]) return;
    for (int k = 0; k < p.p[b]; ++k)
      if (p.pos_pos[b][k] == row) return;
    float *o = d_sem + (p.seg_begin[b] + row) * 16;
#pragma unroll
    for (int q = 0; q < 16; ++q) o[q] = 0.f;
    return;
  }
  const int tile0 = blockIdx.x * kCornerTile;
  if (tile0 >= n) return;
  const int r = t & 3, i = tile0 + (t >> 2);
  const CornerOwn own = corner_own(p, b, i, n, sem);
  const int d_pull = counts[4 * b + 1] - n > 1 ? counts[4 * b + 1] - n : 1;
  const int d_push = counts[4 * b + 2] > 1 ? counts[4 * b + 2] : 1;
  const float gp = *g_pull_loss / (float)p.nb / (float)d_pull;      // d loss / d (one connected distance)
  const float gs = *g_push_loss / (float)p.nb / (float)d_push;      // d loss / d (one active push term)
  float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int a0 = 0; a0 < n; a0 += kCornerTile) {
    __syncthreads();
    corner_stage<true>(s, p, b, a0, n, sem);
    __syncthreads();
    const int rows = n - a0 < kCornerTile ? n - a0 : kCornerTile;
    float tg[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (own.valid)
      for (int al = r; al < rows; al += 4) {
        const int a = a0 + al;
        if (a == i) continue;                                // the diagonal's distance is 0: no gradient
        const float d = corner_sem_dist(s.sem[al], own.sem);
        if (!(d > 0.f)) continue;                            // torch's norm: the gradient of a zero distance is 0
        const bool act = corner_geo_dist(s.xyz[al], own.xyz) < kCornerClose && kCornerDelta - d >= 0.f;
        const float w_push = act ? -gs : 0.f;
        const float w = (corner_in(own.ids, a) ? gp : w_push)        // term (a, i): a among i's entries
                        + (corner_in(s.ids[al], i) ? gp : w_push);   // term (i, a): i among a's entries
        const float coef = w / d;
#pragma unroll
        for (int q = 0; q < 8; ++q) tg[q] += coef * (own.sem[q] - s.sem[al][q]);
      }
#pragma unroll
    for (int q = 0; q < 8; ++q) g[q] += tg[q];
  }
  // the four threads of a column: (r0 + r1) + (r2 + r3) on every one of them
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    g[q] += __shfl_xor(g[q], 1);
    g[q] += __shfl_xor(g[q], 2);
  }
  if (own.valid && own.row >= 0) {
    float *o = d_sem + own.row * 16 + (i & 1) * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if ((q >> 1) == r) o[q] = g[q];
  }
}

int fill_loss_params(CornerLossParams &p, const char *fn, int nb, const int64_t *m_host, const int64_t *p_host,
                     const void *const *pos_pos_ptrs, const void *const *ids_ptrs, const void *const *xyz_ptrs,
                     int64_t n_rows, int *p_max, int64_t *m_max) {
  AABR_CHECK_ARG_AS(fn, nb >= 1 && nb <= kCornerMaxBatch, "nb must be 1 .. 16");
  AABR_CHECK_ARG_AS(fn, m_host && p_host && pos_pos_ptrs && ids_ptrs && xyz_ptrs, "null pointer");
  p = {};
  p.nb = nb;
  int64_t rows = 0;
  *p_max = 0;
  *m_max = 0;
  for (int b = 0; b < nb; ++b) {
    AABR_CHECK_ARG_AS(fn, m_host[b] >= 0 && m_host[b] < ((int64_t)1 << 31), "row count out of range");
    AABR_CHECK_ARG_AS(fn, p_host[b] >= 0 && p_host[b] <= kCornerMaxB && p_host[b] <= m_host[b],
                      "need 0 <= positives <= 512 and <= the scene's sampled rows");
    AABR_CHECK_ARG_AS(fn, p_host[b] == 0 || (pos_pos_ptrs[b] && ids_ptrs[b] && xyz_ptrs[b]), "null pointer");
    p.pos_pos[b] = (const int64_t *)pos_pos_ptrs[b];
    p.ids[b] = (const int32_t *)ids_ptrs[b];
    p.xyz[b] = (const float *)xyz_ptrs[b];
    p.seg_begin[b] = rows;
    p.m[b] = (int32_t)m_host[b];
    p.p[b] = (int32_t)p_host[b];
    rows += m_host[b];
    *p_max = p_host[b] > *p_max ? (int)p_host[b] : *p_max;
    *m_max = m_host[b] > *m_max ? m_host[b] : *m_max;
  }
  AABR_CHECK_ARG_AS(fn, rows == n_rows, "the scenes' sampled rows do not add up to the rows of corners_semantic");
  AABR_CHECK_ARG_AS(fn, n_rows * 16 < ((int64_t)1 << 31), "16 n must stay below 2^31");
  return AABR_OK;
}

}  // namespace

}  // namespace aabr

using namespace aabr;

extern "C" int aabr_corner_loss_tile(void) { return kCornerTile; }

extern "C" int64_t aabr_corner_loss_scratch_words(int nb) {
  if (nb < 1 || nb > kCornerMaxBatch) return -1;
  return (int64_t)nb * kCornerMaxTiles * kCornerPartWords;
}

extern "C" int aabr_corner_tables(const float *targets, int nb, const int64_t *n_host, const int64_t *g_host,
                                  const int64_t *matched_idx, const int64_t *samp_rows, const float *samp_boxes,
                                  int batch_size_per_image, float *tg_xyz, int32_t *tg_connect, int64_t *pos_pos,
                                  int32_t *connect_ids, float *corner_xyz, int32_t *info, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  AABR_CHECK_ARG(nb >= 1 && nb <= kCornerMaxBatch, "nb must be 1 .. 16");
  AABR_CHECK_ARG(batch_size_per_image >= 1 && batch_size_per_image <= kCornerMaxB, "need 1 <= batch_size_per_image <= 512");
  AABR_CHECK_ARG(n_host && g_host && samp_rows && samp_boxes && pos_pos && connect_ids && corner_xyz && info, "null pointer");
  CornerTableParams p = {};
  p.nb = nb;
  p.B = batch_size_per_image;
  int64_t N = 0;
  for (int b = 0; b < nb; ++b) {
    AABR_CHECK_ARG(n_host[b] >= 0 && g_host[b] >= 0 && n_host[b] < ((int64_t)1 << 31) && g_host[b] < ((int64_t)1 << 29),
                   "row count out of range");
    p.prop_begin[b] = N;
    p.n[b] = (int32_t)n_host[b];
    p.gt_begin[b + 1] = p.gt_begin[b] + g_host[b];
    N += n_host[b];
  }
  const int64_t G = p.gt_begin[nb];
  AABR_CHECK_ARG(N < ((int64_t)1 << 31), "more than 2^31 - 1 proposals per call");
  AABR_CHECK_ARG(G < ((int64_t)1 << 29), "more than 2^29 - 1 ground-truth boxes per call");
  AABR_CHECK_ARG(N == 0 || matched_idx, "null pointer");
  AABR_CHECK_ARG(G == 0 || (targets && tg_xyz && tg_connect), "null pointer");
  if (G > 0) {
    hipLaunchKernelGGL(k_corner_tg_xyz, dim3((unsigned)ceil_div(G, (int64_t)256)), dim3(256), 0, st, G, targets, tg_xyz);
    hipLaunchKernelGGL(k_corner_tg_connect, dim3((unsigned)ceil_div(2 * G, (int64_t)256)), dim3(256), 0, st, p, tg_xyz,
                       tg_connect);
  }
  hipLaunchKernelGGL(k_corner_prop_tables, dim3((unsigned)nb), dim3(256), 0, st, p, matched_idx, samp_rows, samp_boxes,
                     tg_connect, pos_pos, connect_ids, corner_xyz, info);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_corner_loss_forward(const float *corners_semantic, int64_t n, int nb, const int64_t *m_host,
                                        const int64_t *p_host, const void *const *pos_pos_ptrs,
                                        const void *const *ids_ptrs, const void *const *xyz_ptrs, float *losses,
                                        int32_t *counts, int32_t *scratch, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  CornerLossParams p;
  int p_max;
  int64_t m_max;
  int rc = fill_loss_params(p, __func__, nb, m_host, p_host, pos_pos_ptrs, ids_ptrs, xyz_ptrs, n, &p_max, &m_max);
  if (rc != AABR_OK) return rc;
  AABR_CHECK_ARG(losses && counts && scratch, "null pointer");
  AABR_CHECK_ARG(n == 0 || corners_semantic, "null pointer");
  if (p_max > 0) {
    const dim3 grid((unsigned)ceil_div(2 * p_max, kCornerTile), (unsigned)nb);
    hipLaunchKernelGGL(k_corner_loss_partial, grid, dim3(256), 0, st, p, corners_semantic, scratch);
  }
  hipLaunchKernelGGL(k_corner_loss_final, dim3(1), dim3(64), 0, st, p, scratch, losses, counts);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_corner_loss_backward(const float *corners_semantic, int64_t n, int nb, const int64_t *m_host,
                                         const int64_t *p_host, const void *const *pos_pos_ptrs,
                                         const void *const *ids_ptrs, const void *const *xyz_ptrs, const int32_t *counts,
                                         const float *grad_pull_loss, const float *grad_push_loss,
                                         float *grad_corners_semantic, void *stream_) {
  CornerLossParams p;
  int p_max;
  int64_t m_max;
  int rc = fill_loss_params(p, __func__, nb, m_host, p_host, pos_pos_ptrs, ids_ptrs, xyz_ptrs, n, &p_max, &m_max);
  if (rc != AABR_OK) return rc;
  AABR_CHECK_ARG(counts && grad_pull_loss && grad_push_loss, "null pointer");
  if (n == 0) return AABR_OK;
  AABR_CHECK_ARG(corners_semantic && grad_corners_semantic, "null pointer");
  const int tiles_max = (int)ceil_div(2 * p_max, kCornerTile);
  const dim3 grid((unsigned)(tiles_max + ceil_div(m_max, (int64_t)256)), (unsigned)nb);
  hipLaunchKernelGGL(k_corner_loss_backward, grid, dim3(256), 0, (hipStream_t)stream_, p, tiles_max, corners_semantic,
                     counts, grad_pull_loss, grad_push_loss, grad_corners_semantic);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

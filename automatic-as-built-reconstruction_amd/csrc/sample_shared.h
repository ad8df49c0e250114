// sample_shared.h -- the balanced positive / negative sampler and the loss terms that more than one translation unit
// runs and that must give the same bits in each: the selection key, the two-level histogram cut, the candidate compaction
// and the exact select (K1 .. K4 of the scheme rpn_loss.hip describes), with their host-side launcher.  rpn_loss.hip wraps
// them into aabr_rpn_loss_forward / aabr_sample_list; roi_loss.hip runs the same kernels over the box head's labels.
// Nothing here is copied: both files compile this code (the kernels sit in an unnamed namespace, one instance per file).
// The anchor table (LossParams::s), its host-side checks and the locate behind the key are anchor_list.h's.
#pragma once
#include "common.h"
#include "anchor_list.h"

#include <vector>

namespace aabr {

namespace {
constexpr int kLossBins = 4096, kLossCand = 1024, kLossMaxB = 512;
constexpr int kLossCtl = 16;
// scratch: per example hist1[class][4096], hist2[class][4096], ctl[16] (one block, cleared by one memset per call); then
// per example the candidates, uint64 [class][kLossCand]; then the per-example loss sums, float [nb][2]
constexpr int kLossZeroWords = 4 * kLossBins + kLossCtl;
constexpr int kLossCandWords = 4 * kLossCand;
// ctl words: k (2), level-1 bin (2), count below it (2), candidates (2), overflow, totals P / N (2)
enum { kCtlK = 0, kCtlBin1 = 2, kCtlBelow1 = 4, kCtlCount = 6, kCtlOverflow = 8, kCtlTotal = 9 };
// info words per example (int32 [nb][8]): num_pos, num_neg, P, N, candidates pos, candidates neg, overflow, N_s of the batch
constexpr int kInfoWords = 8;

struct LossParams {
  AnchorSegs s;                    // the chunk's examples; flat: one map, A = 1, list index = row
  int32_t nb_total, flat, with_loss, label_mode, bf16, example0, k_pos0, B;
  uint32_t seed;
  float beta;
  const void *obj[kAnchorMaxMaps];
  const void *reg[kAnchorMaxMaps];
  const int32_t *coords[kAnchorMaxMaps];
  const int64_t *labels[kAnchorMaxBatch];
  const float *targets[kAnchorMaxBatch];
  int64_t out_begin[kAnchorMaxBatch];
  uint8_t *pos_mask[kAnchorMaxBatch];
  uint8_t *neg_mask[kAnchorMaxBatch];
  // separated-classifier groups (aabr_rpn_loss_grouped_*; G = 0: none).  Example e = scene * G + group is a SEGMENT: its
  // tables are its scene's, its head values sit group[b] * rows[m] * A behind the plain index in map m's group-major
  // allocation, and the sampler's key hashes the scene, so a segment selects what the plain call selects for its scene
  int32_t G, group[kAnchorMaxBatch];
  int64_t rows[kAnchorMaxMaps];
};
// the largest set beside it: k_loss_backward (rpn_loss.hip), 4 pointers and GradPtrs, 2 x 8 pointers
static_assert(sizeof(LossParams) + (4 + 2 * kAnchorMaxMaps) * 8 <= kKernelArgBytes, "k_loss_*: the struct and 20 pointers");

__device__ inline uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
// 0 positive, 1 negative, -1 ignored.  label_mode 0: matched indices (>= 0 / -1 / -2, loss_3d.py:180-187);
// 1: sampler labels (>= 1 / 0 / other, balanced_positive_negative_sampler.py:39-40)
__device__ inline int class_of(const LossParams &p, int64_t v) {
  if (p.label_mode == 0) return v >= 0 ? 0 : (v == -1 ? 1 : -1);
  return v >= 1 ? 0 : (v == 0 ? 1 : -1);
}
__device__ inline AnchorLoc locate(const LossParams &p, int b, int64_t j) {
  if (p.flat) return {0, 0, j};
  return anchor_locate(p.s, b, j);
}
__device__ inline uint32_t key_of(const LossParams &p, int b, int64_t j, const AnchorLoc &L) {
  uint32_t h = fmix32(p.seed ^ 0x9E3779B9u);
  h = fmix32(h ^ (uint32_t)(p.G ? (p.example0 + b) / p.G : p.example0 + b));
  if (p.flat) return fmix32(h ^ (uint32_t)j);
  const int32_t *c = p.coords[L.m] + L.row * 4;
  h = fmix32(h ^ (uint32_t)L.m);
  h = fmix32(h ^ (uint32_t)c[0]);
  h = fmix32(h ^ (uint32_t)c[1]);
  h = fmix32(h ^ (uint32_t)c[2]);
  return fmix32(h ^ (uint32_t)L.a);
}
// candidate = key << 32 | index in the example's list; padding = ~0 (after everything)
__device__ inline bool cand_less(const LossParams &p, int b, unsigned long long x, unsigned long long y) {
  if ((x >> 32) != (y >> 32)) return (x >> 32) < (y >> 32);
  const uint32_t jx = (uint32_t)x, jy = (uint32_t)y;
  if (p.flat || jx == jy || jx == 0xffffffffu || jy == 0xffffffffu) return jx < jy;
  const AnchorLoc lx = locate(p, b, jx), ly = locate(p, b, jy);
  if (lx.m != ly.m) return lx.m < ly.m;
  const int32_t *cx = p.coords[lx.m] + lx.row * 4, *cy = p.coords[ly.m] + ly.row * 4;
  for (int d = 0; d < 3; ++d)
    if (cx[d] != cy[d]) return cx[d] < cy[d];
  return lx.a < ly.a;
}

// index of anchor L of example b in map L.m's objectness vector (times 7: its regression row)
__device__ inline int64_t head_index(const LossParams &p, int b, const AnchorLoc &L) {
  const int64_t oi = L.row * p.s.A + L.a;
  return p.G ? oi + p.group[b] * p.rows[L.m] * p.s.A : oi;
}
__device__ inline float ld(const void *base, int64_t i, int bf16) {
  return bf16 ? (float)reinterpret_cast<const __bf16 *>(base)[i] : reinterpret_cast<const float *>(base)[i];
}
__device__ inline void st(void *base, int64_t i, float v, int bf16) {
  if (bf16) reinterpret_cast<__bf16 *>(base)[i] = (__bf16)v;
  else reinterpret_cast<float *>(base)[i] = v;
}
// the loss terms and their derivatives (shared by the maps form and the list form)
__device__ inline float smooth_l1_term(float d, float beta) {     // d = |pred - target|
  return d < beta ? 0.5f * (d * d) / beta : d - 0.5f * beta;
}
__device__ inline float smooth_l1_grad(float diff, float beta) {  // d/d pred, diff = pred - target
  const float d = fabsf(diff);
  return d < beta ? diff / beta : (diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f));
}
__device__ inline float bce_term(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))); }

__device__ inline int32_t *ex_scratch(int32_t *scratch, const LossParams &p, int b) {
  return scratch + (int64_t)(p.example0 + b) * kLossZeroWords;
}
__device__ inline unsigned long long *ex_cand(int32_t *scratch, const LossParams &p, int b) {
  return reinterpret_cast<unsigned long long *>(scratch + (int64_t)p.nb_total * kLossZeroWords +
                                                (int64_t)(p.example0 + b) * kLossCandWords);
}

// the bin (from the bottom) in which the running count of a 4096-bin histogram reaches `need` (>= 1); the count below it
// through `below`.  Called by thread `t0` of the workgroup after s_part[256] holds the 16-bin partial sums.
__device__ inline int find_bin_low(const int32_t *__restrict__ hist, const int *s_part, int need, int &below) {
  int run = 0, bt = 255;
  for (int i = 0; i < 256; ++i) {
    if (run + s_part[i] >= need) { bt = i; break; }
    run += s_part[i];
  }
  for (int q = 0; q < 16; ++q) {
    const int c = hist[16 * bt + q];
    if (run + c >= need || q == 15) { below = run; return 16 * bt + q; }
    run += c;
  }
  below = run;
  return 16 * bt + 15;
}

template <int LEVEL>   // 1: leading 12 bits of every key; 2: the next 12 bits of the keys inside the level-1 bin
__global__ __launch_bounds__(256) void k_loss_hist(LossParams p, int32_t *__restrict__ scratch) {
  __shared__ int32_t s_hist[2][kLossBins];
  __shared__ int s_part[2][256], s_bin[2];
  const int b = blockIdx.y, t = threadIdx.x;
  int32_t *sc = ex_scratch(scratch, p, b);
  int32_t *ctl = sc + 4 * kLossBins;
  const int64_t n = p.s.seg[b][p.s.n_maps];
  if (LEVEL == 2) {
    // num_pos = min(P, int(B * f)), num_neg = min(N, B - num_pos) from the level-1 totals, then the level-1 bins
    for (int c = 0; c < 2; ++c) {
      int sum = 0;
      for (int q = 0; q < 16; ++q) sum += sc[c * kLossBins + 16 * t + q];
      s_part[c][t] = sum;
    }
    __syncthreads();
    if (t == 0) {
      int P = 0, N = 0;
      for (int i = 0; i < 256; ++i) { P += s_part[0][i]; N += s_part[1][i]; }
      const int kp = P < p.k_pos0 ? P : p.k_pos0;
      const int kn = N < p.B - kp ? N : p.B - kp;
      const int ks[2] = {kp, kn};
      for (int c = 0; c < 2; ++c) {
        int below = 0;
        s_bin[c] = ks[c] > 0 ? find_bin_low(sc + c * kLossBins, s_part[c], ks[c], below) : -1;
        if (blockIdx.x == 0) {
          ctl[kCtlK + c] = ks[c];
          ctl[kCtlBin1 + c] = s_bin[c];
          ctl[kCtlBelow1 + c] = below;
        }
      }
      if (blockIdx.x == 0) { ctl[kCtlTotal] = P; ctl[kCtlTotal + 1] = N; }
    }
  }
  for (int q = t; q < 2 * kLossBins; q += 256) (&s_hist[0][0])[q] = 0;
  __syncthreads();
  for (int64_t j = (int64_t)blockIdx.x * 256 + t; j < n; j += (int64_t)gridDim.x * 256) {
    const int c = class_of(p, p.labels[b][j]);
    if (c < 0) continue;
    if (LEVEL == 2 && s_bin[c] < 0) continue;
    const AnchorLoc L = locate(p, b, j);
    const uint32_t key = key_of(p, b, j, L);
    if (LEVEL == 1) atomicAdd(&s_hist[c][key >> 20], 1);
    else if ((int)(key >> 20) == s_bin[c]) atomicAdd(&s_hist[c][(key >> 8) & 4095u], 1);
  }
  __syncthreads();
  int32_t *h = sc + (LEVEL == 1 ? 0 : 2 * kLossBins);
  for (int q = t; q < 2 * kLossBins; q += 256) {
    const int v = (&s_hist[0][0])[q];
    if (v) atomicAdd(&h[q], v);
  }
}

__global__ __launch_bounds__(256) void k_loss_compact(LossParams p, int32_t *__restrict__ scratch) {
  __shared__ int s_part[2][256];
  __shared__ uint32_t s_thr[2];
  __shared__ int s_k[2];
  const int b = blockIdx.y, t = threadIdx.x;
  int32_t *sc = ex_scratch(scratch, p, b);
  int32_t *ctl = sc + 4 * kLossBins;
  unsigned long long *cand = ex_cand(scratch, p, b);
  const int64_t n = p.s.seg[b][p.s.n_maps];
  for (int c = 0; c < 2; ++c) {
    int sum = 0;
    for (int q = 0; q < 16; ++q) sum += sc[2 * kLossBins + c * kLossBins + 16 * t + q];
    s_part[c][t] = sum;
  }
  __syncthreads();
  if (t == 0) {
    for (int c = 0; c < 2; ++c) {
      s_k[c] = ctl[kCtlK + c];
      if (s_k[c] > 0) {
        int below2 = 0;
        const int bin2 = find_bin_low(sc + 2 * kLossBins + c * kLossBins, s_part[c], s_k[c] - ctl[kCtlBelow1 + c], below2);
        s_thr[c] = ((uint32_t)ctl[kCtlBin1 + c] << 12) | (uint32_t)bin2;
      }
    }
  }
  __syncthreads();
  for (int64_t j = (int64_t)blockIdx.x * 256 + t; j < n; j += (int64_t)gridDim.x * 256) {
    const int c = class_of(p, p.labels[b][j]);
    if (c < 0 || s_k[c] == 0) continue;
    const AnchorLoc L = locate(p, b, j);
    const uint32_t key = key_of(p, b, j, L);
    if ((key >> 8) <= s_thr[c]) {
      const int pos = atomicAdd(&ctl[kCtlCount + c], 1);
      if (pos < kLossCand) cand[c * kLossCand + pos] = ((unsigned long long)key << 32) | (unsigned long long)(uint32_t)j;
      else ctl[kCtlOverflow] = 1;
    }
  }
}

// one workgroup per example: exact cut of each class, the selected list (example-major label indices, positives then
// negatives, -1 padded to B), optional uint8 masks, and the example's sums of the loss terms
__global__ __launch_bounds__(256) void k_loss_select(LossParams p, int32_t *__restrict__ scratch, int64_t *__restrict__ sel,
                                                     int32_t *__restrict__ info, float *__restrict__ partial) {
  __shared__ unsigned long long s[kLossCand];
  __shared__ float s_red[2][256];
  const int b = blockIdx.x, t = threadIdx.x, e = p.example0 + b;
  int32_t *sc = ex_scratch(scratch, p, b);
  const int32_t *ctl = sc + 4 * kLossBins;
  const unsigned long long *cand = ex_cand(scratch, p, b);
  const int kp = ctl[kCtlK], kn = ctl[kCtlK + 1];
  const bool loss = p.with_loss != 0;
  int64_t *out = sel + (int64_t)e * p.B;
  float bce = 0.f, box = 0.f;
  for (int c = 0; c < 2; ++c) {
    const int k = c == 0 ? kp : kn, o = c == 0 ? 0 : kp;
    if (k == 0) continue;
    int C = ctl[kCtlCount + c];
    C = C < kLossCand ? C : kLossCand;
    int n2 = 2;
    while (n2 < C) n2 <<= 1;
    __syncthreads();
    for (int i = t; i < n2; i += 256) s[i] = i < C ? cand[c * kLossCand + i] : ~0ull;
    for (int size = 2; size <= n2; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        __syncthreads();
        for (int i = t; i < n2; i += 256) {
          const int j = i ^ stride;
          if (j > i) {
            const unsigned long long x = s[i], y = s[j];
            const bool up = (i & size) == 0;
            if (cand_less(p, b, y, x) == up) { s[i] = y; s[j] = x; }
          }
        }
      }
    __syncthreads();
    uint8_t *mask = c == 0 ? p.pos_mask[b] : p.neg_mask[b];
    for (int i = t; i < k; i += 256) {
      if (i >= C) { out[o + i] = -1; continue; }     // (C >= k by construction; never an index out of the list)
      const int64_t j = (int64_t)(uint32_t)s[i];
      out[o + i] = p.out_begin[b] + j;
      if (mask) mask[j] = 1;
      if (loss) {
        const AnchorLoc L = locate(p, b, j);
        const int64_t oi = head_index(p, b, L);
        bce += bce_term(ld(p.obj[L.m], oi, p.bf16), c == 0 ? 1.f : 0.f);
        if (c == 0)
          for (int d = 0; d < 7; ++d)
            box += smooth_l1_term(fabsf(ld(p.reg[L.m], oi * 7 + d, p.bf16) - p.targets[b][j * 7 + d]), p.beta);
      }
    }
  }
  for (int i = kp + kn + t; i < p.B; i += 256) out[i] = -1;
  s_red[0][t] = bce;
  s_red[1][t] = box;
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) { s_red[0][t] += s_red[0][t + w]; s_red[1][t] += s_red[1][t + w]; }
  }
  if (t == 0) {
    if (partial) { partial[2 * e] = s_red[0][0]; partial[2 * e + 1] = s_red[1][0]; }
    int32_t *inf = info + (int64_t)e * kInfoWords;
    inf[0] = kp; inf[1] = kn; inf[2] = ctl[kCtlTotal]; inf[3] = ctl[kCtlTotal + 1];
    inf[4] = ctl[kCtlCount]; inf[5] = ctl[kCtlCount + 1]; inf[6] = ctl[kCtlOverflow]; inf[7] = 0;
  }
}

// host side: the tables of chunk [b0, b0 + nbc) (<= 16 examples); `fn` names the entry point in an error
int fill_chunk(LossParams &p, const char *fn, int b0, int nbc, const int32_t *seg_begin_host, const int32_t *site_begin_host,
               const void *const *label_ptrs, const void *const *target_ptrs, const int64_t *out_begin,
               void *const *pos_masks, void *const *neg_masks, bool need_labels, int64_t &nmax) {
  int rc = fill_anchor_segs(p.s, fn, p.s.n_maps, p.s.A, b0, nbc, seg_begin_host, site_begin_host, &nmax);
  if (rc != AABR_OK) return rc;
  p.example0 = b0;
  for (int b = 0; b < kAnchorMaxBatch; ++b) {
    const bool on = b < nbc;
    const int g = b0 + b;
    p.labels[b] = on && label_ptrs ? (const int64_t *)label_ptrs[g] : nullptr;
    p.targets[b] = on && target_ptrs ? (const float *)target_ptrs[g] : nullptr;
    p.out_begin[b] = on ? out_begin[g] : 0;
    p.pos_mask[b] = on && pos_masks ? (uint8_t *)pos_masks[g] : nullptr;
    p.neg_mask[b] = on && neg_masks ? (uint8_t *)neg_masks[g] : nullptr;
    p.group[b] = on && p.G ? g % p.G : 0;
    if (!on) continue;
    const int64_t n = p.s.seg[b][p.s.n_maps];
    AABR_CHECK_ARG_AS(fn, n == 0 || !need_labels || p.labels[b], "null label list");
    AABR_CHECK_ARG_AS(fn, n == 0 || !p.with_loss || p.targets[b], "null regression-target list");
    for (int m = 0; m < p.s.n_maps; ++m)
      AABR_CHECK_ARG_AS(fn, p.flat || p.s.seg[b][m + 1] == p.s.seg[b][m] ||
                               ((p.coords[m] || !need_labels) && p.obj[m] && p.reg[m]), "null map pointer");
  }
  return AABR_OK;
}

// where example b's list (length n) begins in the concatenation the selected indices refer to; `total` runs over the
// examples in order.  With groups the concatenation is the GROUP's own, scene-major (what a plain call on that group's
// labels sees): the segments of a scene share its list length and begin at the same index.
inline int64_t select_out_begin(int G, int b, int64_t n, int64_t &total) {
  const int64_t begin = total;
  if (G == 0 || (b + 1) % G == 0) total += n;
  return begin;
}

// the per-example loss sums of k_loss_select (float [nb][2]) behind the sampler's words
inline float *select_partials(int32_t *scratch, int nb) {
  return reinterpret_cast<float *>(scratch + (int64_t)nb * (kLossZeroWords + kLossCandWords));
}

// the select of every chunk: 1 memset + 4 launches per chunk of 16 examples
int run_select_chunks(LossParams &p, const char *fn, int nb, const int32_t *seg_begin_host, const int32_t *site_begin_host,
                      const void *const *label_ptrs, const void *const *target_ptrs, void *const *pos_masks,
                      void *const *neg_masks, int64_t *selected, int32_t *info, int32_t *scratch, hipStream_t st) {
  AABR_CHECK_ARG_AS(fn, ((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
  std::vector<int64_t> out_begin(nb);
  int64_t total = 0;
  for (int b = 0; b < nb; ++b) {
    const int64_t n = seg_begin_host[b * (p.s.n_maps + 1) + p.s.n_maps];
    AABR_CHECK_ARG_AS(fn, n >= 0, "negative list length");
    out_begin[b] = select_out_begin(p.G, b, n, total);
  }
  AABR_CHECK_ARG_AS(fn, total < ((int64_t)1 << 31), "more than 2^31 - 1 entries per call");
  p.nb_total = nb;
  for (int b0 = 0; b0 < nb; b0 += kAnchorMaxBatch) {   // every chunk's table, before anything is enqueued
    AnchorSegs t;
    int rc = fill_anchor_segs(t, fn, p.s.n_maps, p.s.A, b0, nb - b0 < kAnchorMaxBatch ? nb - b0 : kAnchorMaxBatch,
                              seg_begin_host, site_begin_host, nullptr);
    if (rc != AABR_OK) return rc;
  }
  AABR_CHECK_HIP(hipMemsetAsync(scratch, 0, (size_t)nb * kLossZeroWords * sizeof(int32_t), st));
  float *partial = select_partials(scratch, nb);
  for (int b0 = 0; b0 < nb; b0 += kAnchorMaxBatch) {
    const int nbc = nb - b0 < kAnchorMaxBatch ? nb - b0 : kAnchorMaxBatch;
    int64_t nmax = 0;
    int rc = fill_chunk(p, fn, b0, nbc, seg_begin_host, site_begin_host, label_ptrs, target_ptrs, out_begin.data(),
                        pos_masks, neg_masks, true, nmax);
    if (rc != AABR_OK) return rc;
    int64_t gx = ceil_div(nmax, 256 * 8);
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    hipLaunchKernelGGL(k_loss_hist<1>, dim3((unsigned)gx, (unsigned)nbc), dim3(256), 0, st, p, scratch);
    hipLaunchKernelGGL(k_loss_hist<2>, dim3((unsigned)gx, (unsigned)nbc), dim3(256), 0, st, p, scratch);
    hipLaunchKernelGGL(k_loss_compact, dim3((unsigned)gx, (unsigned)nbc), dim3(256), 0, st, p, scratch);
    hipLaunchKernelGGL(k_loss_select, dim3((unsigned)nbc), dim3(256), 0, st, p, scratch, selected, info,
                       p.with_loss ? partial : nullptr);
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

}  // namespace

}  // namespace aabr

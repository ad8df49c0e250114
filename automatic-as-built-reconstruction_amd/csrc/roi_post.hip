// roi_post.hip -- the ROI box post-processor on the device: class logits + box regression + proposals of a batch of
// scenes -> per scene the labelled, scored, NMS-filtered rotated boxes (gfx950).
//
// Replaces PostProcessor.forward / filter_results of the reference's box head
// (maskrcnn_benchmark/modeling/roi_heads/box_head_3d/inference.py:44-162), which loops in Python over scenes and over
// classes (nonzero, gather, topk, one NMS and one host read per turn).  Contract, for nb scenes whose proposals are
// concatenated scene-major (n_b rows for scene b, N rows in all), C classes with class 0 = background:
//   1. prob = softmax(class_logits, -1)                                                         inference.py:57
//   2. boxes = BoxCoder3D.decode_centroid_box(box_regression, proposals): one box per (row, class) when the regression
//      is class specific [N, 7 C], else the row's one box for all its classes (inference.py:102-104)
//                                                                                box_coder_3d.py:53-80, inference.py:64
//   3. per scene and class j = 1 .. C-1: candidates = rows with prob[:, j] > score_thresh (strict); on an NMS-only copy
//      of their boxes with the boxlist_nms_3d clamps (sizes 3:5 >= nms_min_yx, size 5 >= nms_min_z;
//      structures/boxlist_ops_3d.py:42-44) rotate_nms_3d(pre_max, post_max, nms_thresh): the pre_max best candidates in
//      descending score, greedy suppression (pre-filter matrix > 0, exact polygon IoU >= thresh: the rule of
//      k_nms_mask_rot), the first post_max survivors                                            inference.py:125-141
//      EQUAL SCORES: ascending proposal row, in the order of the list and at the pre_max cut.  torch.topk leaves both
//      open; this is this project's rule (the one aabr_rpn_topk_maps states for the RPN side).
//   4. per scene: the classes in ascending order, each in survivor order; if the count M > detections_per_img = D > 0,
//      t = the D-th largest score (kthvalue(scores, M - D + 1)) and every detection with score >= t stays, in place --
//      ties at the cut all stay, so more than D can remain; D <= 0 keeps everything           inference.py:153-161
//   5. per detection: box (the unclamped one), score, label and the scene-local proposal row it came from.
//
// Five launches whatever nb and C are, no host read between them, integer atomics in LDS only (counts and positions
// that a sort or a scan orders afterwards): results are bit-identical run to run.
//   k_roi_post_rows    one thread per row: softmax (row max, expf, sum in class order, divide) and the row's decodes;
//   k_roi_post_select  one workgroup per (scene, class): count the candidates, radix-select the pre_max-th score when
//                      there are more, collect, bitonic sort by (score descending, row ascending) in LDS, write the
//                      sorted rows / scores / NMS-copy boxes and the segment's size;
//   k_roi_post_mask    the suppression words of every segment: grid = worst case over the host-known list lengths,
//                      surplus workgroups leave on the device-side size; the tile is nms_mask_rot_tile (nms_shared.h),
//                      the body of k_nms_mask_rot itself;
//   k_roi_post_scan    one workgroup per segment, all segments concurrently: nms_scan_block, the body of k_nms_scan;
//   k_roi_post_scene   one workgroup per scene: the D-th largest score by radix select, ordered compaction, info.
// Limits (validated): 2 <= C <= 32, 1 <= nb <= 16, 1 <= post_max <= pre_max <= 2048, N * C * 7 < 2^31.
// A scene with n_b = 0, a segment without a candidate and N = 0 are legal and give empty lists.
// With separated-classifier groups (sep_groups.h, aabr_roi_post_detections_grouped) the same five launches: the row
// kernel's softmax runs over the row's group columns (k_roi_post_rows<.., true>), a segment is a foreground column of a group,
// candidates are tested for group membership, and the detections_per_img cut is taken per (scene, group).
#include "common.h"
#include "nms_shared.h"
#include "sep_groups.h"

namespace aabr {

constexpr int kRoiMaxBatch = 16, kRoiMaxClasses = 32, kRoiMaxPre = 2048, kRoiInfoWords = 8;

struct RoiPostParams {
  int32_t row_begin[kRoiMaxBatch + 1];   // first row of scene b in the concatenated lists
  int nb, C, reg_classes;                // reg_classes: C (class specific) or 1
  int pre_max, post_max, D, only_xy;
  int P, cbmax, keep_stride;             // per-segment strides: sorted list (rows), mask row words, keep list
  float score_thresh, nms_thresh, clip, min_yx, min_z;
  BoxEncodeW w;
};

// device buffers of one call: outputs of the caller or pieces of its scratch
struct RoiPostBufs {
  float *prob, *boxes;                   // [N, C], [N, C, 7]
  int32_t *seg_m, *seg_cnt, *seg_kept;   // [S]: sorted-list size, candidates, survivors
  int32_t *sel_row;                      // [S][P] scene-local row of sorted entry k
  float *sel_score, *nms_boxes;          // [S][P], [S][P][7]
  int64_t *keep;                         // [S][keep_stride] sorted positions of the survivors
  unsigned long long *mask;              // [S][P * cbmax]
};

// exclusive prefix sum of one int per thread over the workgroup (any multiple of 64 threads up to 1024)
__device__ __forceinline__ int block_excl_scan(int v, int *s_wave, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                                     // s_wave is free again
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
  for (int w = 0; w < nw; ++w) {
    const int t = s_wave[w];
    if (w < wave) base += t;
    total += t;
  }
  return base + inc - v;
}

// The `need`-th largest of the 32-bit keys get(i, key) yields for i < n (false: entry i does not take part), by four
// 8-bit histogram passes of the whole workgroup.  Returns the key; need_eq = how many entries EQUAL to it the top
// `need` contain.  Integer LDS atomics only feed counts: the result does not depend on their order.
template <class F>
__device__ __forceinline__ uint32_t block_select_kth(int n, int need, F get, int *s_hist, int *s_ctl, int &need_eq) {
  uint32_t prefix = 0, have = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    __syncthreads();
    for (int q = threadIdx.x; q < 256; q += blockDim.x) s_hist[q] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      uint32_t key;
      if (get(i, key) && (key & have) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int cum = 0, bin = 0;
      for (int q = 255; q >= 0; --q) {
        if (cum + s_hist[q] >= need) { bin = q; break; }
        cum += s_hist[q];
      }
      s_ctl[0] = bin;
      s_ctl[1] = need - cum;
    }
    __syncthreads();
    prefix |= (uint32_t)s_ctl[0] << shift;
    have |= 255u << shift;
    need = s_ctl[1];
  }
  need_eq = need;
  return prefix;
}

// One thread per row: the row's softmax (row_softmax, sep_groups.h) and its decodes.
// kCorner: the regressions are decoded with BoxCoder3D(is_corner_roi=True).decode (box_decode7_corner, corner_box.h).
// kSep false: prob [N, C] over all columns; one decode per row when reg_classes == 1, else one per class; boxes [N, C, 7].
// kSep (SeperateClassifier.post_processor): row i belongs to group sep_id[i]; its softmax runs over that group's columns
// only, summed in group-local order, and every other column of prob is an exact 0.  The regression is class agnostic:
// one decode, boxes [N, 7].  A sep_id outside [0, G) is never used as an index: the row's prob is all 0, it is no group's
// candidate, and word 5 of its scene's info block is raised.
template <bool kCorner, bool kSep>
__global__ __launch_bounds__(256) void k_roi_post_rows(const float *__restrict__ logits, const float *__restrict__ reg,
                                                       const float *__restrict__ props,
                                                       const int32_t *__restrict__ sep_id, int64_t N, RoiPostParams p,
                                                       SepGroups sg, float *__restrict__ prob, float *__restrict__ boxes,
                                                       int32_t *__restrict__ info) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int C = p.C;
  const float *x = logits + i * C;
  const auto softmax_over = [&](const auto &cols) {
    const RowSoftmax r = row_softmax(cols, [&](int c) { return x[c]; });
    for (int k = 0; k < cols.cn; ++k) prob[i * C + cols.col(k)] = r.prob(x[cols.col(k)]);
  };
  if (kSep) {
    for (int c = 0; c < C; ++c) prob[i * C + c] = 0.0f;
    const int g = sep_id[i];
    if (g >= 0 && g < sg.G) {
      softmax_over(RowCols<true>(sg, g));
    } else {
      int b = 0;
      while (b + 1 < p.nb && i >= p.row_begin[b + 1]) ++b;
      atomicOr(&info[b * kRoiInfoWords + 5], 1);
    }
  } else {
    softmax_over(RowCols<false>{C});
  }
  float an[7], o[7];
#pragma unroll
  for (int d = 0; d < 7; ++d) an[d] = props[7 * i + d];
  const auto decode = [&](const float *e) {
    if (kCorner) box_decode7_corner(e, an, p.w.w, p.clip, o);
    else box_decode7(e, an, p.w, p.clip, o);
  };
  const bool per_class = !kSep && p.reg_classes != 1;
  const int nbox = kSep ? 1 : C;                       // boxes stored per row
  if (!per_class) decode(reg + 7 * i);
  for (int c = 0; c < nbox; ++c) {
    if (per_class) decode(reg + 7 * (i * C + c));
#pragma unroll
    for (int d = 0; d < 7; ++d) boxes[7 * (i * nbox + c) + d] = o[d];
  }
}

// kSep: the segments of a scene are the foreground columns of all groups (sg.fg_col, in (group, group-local) order); the
// candidates of column j are the rows OF ITS GROUP above the threshold -- membership is tested, a foreign row's zero
// probability is not relied on (score_thresh may be negative) -- and the boxes are one per row.
template <bool kSep>
__global__ __launch_bounds__(1024) void k_roi_post_select(RoiPostParams p, RoiPostBufs u, SepGroups sg,
                                                          const int32_t *__restrict__ sep_id) {
  __shared__ unsigned long long s_key[kRoiMaxPre];
  __shared__ int s_hist[256], s_wave[16], s_ctl[4];
  const int tid = threadIdx.x;
  const int nseg = kSep ? sg.nf : p.C - 1;
  const int s = blockIdx.x, b = s / nseg, j = kSep ? sg.fg_col[s % nseg] : 1 + s % nseg;
  const int grp = kSep ? sg.fg_group[s % nseg] : 0;
  const int r0 = p.row_begin[b], n = p.row_begin[b + 1] - r0;
  const float *col = u.prob + (int64_t)r0 * p.C + j;
  const int C = p.C;
  const float thr = p.score_thresh;
  const auto is_cand = [&](int r, float v) { return v > thr && (!kSep || sep_id[r0 + r] == grp); };
  if (tid == 0) { s_ctl[2] = 0; s_ctl[3] = 0; }
  __syncthreads();
  {
    int c = 0;
    for (int r = tid; r < n; r += 1024) c += is_cand(r, col[(int64_t)r * C]) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((tid & 63) == 0 && c) atomicAdd(&s_ctl[2], c);
  }
  __syncthreads();
  const int cnt = s_ctl[2];
  const int m = cnt < p.pre_max ? cnt : p.pre_max;
  const bool cut = cnt > p.pre_max;                    // the pre-NMS cut acts: uniform
  uint32_t T = 0;
  int need_eq = 0;
  if (cut)
    T = block_select_kth(n, p.pre_max,
                         [&](int r, uint32_t &key) {
                           const float v = col[(int64_t)r * C];
                           key = __float_as_uint(v);     // probabilities are >= +0: the bit order is the value order
                           return is_cand(r, v);
                         },
                         s_hist, s_ctl, need_eq);
  // collect: every candidate above the cut score and the first need_eq rows AT it (ascending row: ordered by a scan);
  // the positions come from an LDS counter, the sort below makes the order final
  int eq_base = 0;
  for (int base = 0; base < n; base += 1024) {
    const int r = base + tid;
    const float v = r < n ? col[(int64_t)r * C] : 0.0f;
    const bool cand = r < n && is_cand(r, v);
    const uint32_t bits = __float_as_uint(v);
    bool take = cand;
    if (cut) {
      const bool eq = cand && bits == T;
      int total;
      const int rank = eq_base + block_excl_scan(eq ? 1 : 0, s_wave, total);
      eq_base += total;
      take = cand && (bits > T || (eq && rank < need_eq));
    }
    if (take) {
      const int pos = atomicAdd(&s_ctl[3], 1);
      if (pos < kRoiMaxPre) s_key[pos] = ((unsigned long long)(~bits) << 32) | (unsigned long long)(uint32_t)r;
    }
  }
  int Pw = 2;
  while (Pw < m) Pw <<= 1;
  __syncthreads();
  for (int i = m + tid; i < Pw; i += 1024) s_key[i] = ~0ull;
  for (int size = 2; size <= Pw; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = tid; i < Pw; i += 1024) {
        const int q = i ^ stride;
        if (q > i) {
          const unsigned long long a = s_key[i], c = s_key[q];
          const bool up = (i & size) == 0;
          if ((a > c) == up) { s_key[i] = c; s_key[q] = a; }
        }
      }
    }
  __syncthreads();
  for (int k = tid; k < m; k += 1024) {
    const unsigned long long key = s_key[k];
    const int r = (int)(uint32_t)key;
    const int64_t q = (int64_t)s * p.P + k;
    u.sel_row[q] = r;
    u.sel_score[q] = __uint_as_float(~(uint32_t)(key >> 32));
    const float *src = u.boxes + 7 * (kSep ? (int64_t)(r0 + r) : (int64_t)(r0 + r) * C + j);
    float o[7];
#pragma unroll
    for (int d = 0; d < 7; ++d) o[d] = src[d];
    o[3] = o[3] < p.min_yx ? p.min_yx : o[3];          // boxlist_nms_3d clamps (boxlist_ops_3d.py:42-44)
    o[4] = o[4] < p.min_yx ? p.min_yx : o[4];
    o[5] = o[5] < p.min_z ? p.min_z : o[5];
#pragma unroll
    for (int d = 0; d < 7; ++d) u.nms_boxes[7 * q + d] = o[d];
  }
  if (tid == 0) { u.seg_m[s] = m; u.seg_cnt[s] = cnt; }
}

// grid (row tiles, column blocks, segments) sized by the longest list the host can know of; a workgroup beyond its
// segment's device-side size leaves at once
__global__ __launch_bounds__(256) void k_roi_post_mask(RoiPostParams p, RoiPostBufs u) {
  const int s = blockIdx.z;
  const int m = u.seg_m[s];
  const int64_t i0 = (int64_t)blockIdx.x * kNmsRows;
  const int cb = blockIdx.y;
  if (i0 >= m || cb * 64 >= m) return;                 // workgroup-uniform
  nms_mask_rot_tile(u.nms_boxes + 7 * (int64_t)s * p.P, m, p.nms_thresh, p.only_xy, (m + 63) / 64,
                    u.mask + (int64_t)s * p.P * p.cbmax, i0, cb);
}

__global__ __launch_bounds__(256) void k_roi_post_scan(RoiPostParams p, RoiPostBufs u) {
  __shared__ unsigned long long remv[kRoiMaxPre / 64];
  const int s = blockIdx.x;
  const int m = u.seg_m[s];
  nms_scan_block(u.mask + (int64_t)s * p.P * p.cbmax, m, (m + 63) / 64, p.post_max,
                 u.keep + (int64_t)s * p.keep_stride, u.seg_kept + s, remv);
}

// kSep: the scene's list is the groups in ascending order, each group's columns in group-local order; the
// detections_per_img cut is taken PER GROUP (each group went through a post-processor pass of its own in the reference),
// and the label is the column index, which is the original label.
template <bool kSep>
__global__ __launch_bounds__(1024) void k_roi_post_scene(RoiPostParams p, RoiPostBufs u, SepGroups sg, int64_t cap,
                                                         int64_t *__restrict__ det_rows,
                                                         int64_t *__restrict__ det_labels,
                                                         float *__restrict__ det_scores, float *__restrict__ det_boxes,
                                                         int32_t *__restrict__ info) {
  __shared__ int s_off[kRoiMaxClasses + 1], s_hist[256], s_wave[16], s_ctl[4];
  __shared__ uint32_t s_cut[kSepMaxGroups];
  const int tid = threadIdx.x, b = blockIdx.x, nc = kSep ? sg.nf : p.C - 1;
  const int s0 = b * nc;
  if (tid == 0) {
    int run = 0;
    for (int j = 0; j < nc; ++j) { s_off[j] = run; run += u.seg_kept[s0 + j]; }
    s_off[nc] = run;
  }
  __syncthreads();
  const int M = s_off[nc];
  // entry e of the scene's concatenated list (classes ascending, survivors in order) -> its sorted-list slot
  auto slot_of = [&](int e, int &label, int &grp) {
    int j = 0;
    while (j + 1 < nc && e >= s_off[j + 1]) ++j;
    label = kSep ? sg.fg_col[j] : j + 1;
    grp = kSep ? sg.fg_group[j] : 0;
    return (int64_t)(s0 + j) * p.P + u.keep[(int64_t)(s0 + j) * p.keep_stride + (e - s_off[j])];
  };
  uint32_t T = 0;                                      // keep score >= T; +0 keeps everything
  if (!kSep && p.D > 0 && M > p.D) {
    int need_eq;
    T = block_select_kth(M, p.D,
                         [&](int e, uint32_t &key) {
                           int label, grp;
                           key = __float_as_uint(u.sel_score[slot_of(e, label, grp)]);
                           return true;
                         },
                         s_hist, s_ctl, need_eq);
  }
  if (kSep) {
    for (int g = 0; g < sg.G; ++g) {                    // workgroup-uniform: group g's entries are e0 .. e1 of the list
      const int e0 = s_off[sg.fg_begin[g]], e1 = s_off[sg.fg_begin[g + 1]];
      uint32_t Tg = 0;
      if (p.D > 0 && e1 - e0 > p.D) {
        int need_eq;
        Tg = block_select_kth(e1 - e0, p.D,
                              [&](int e, uint32_t &key) {
                                int label, grp;
                                key = __float_as_uint(u.sel_score[slot_of(e0 + e, label, grp)]);
                                return true;
                              },
                              s_hist, s_ctl, need_eq);
      }
      if (tid == 0) s_cut[g] = Tg;
    }
    __syncthreads();
  }
  int out = 0;
  for (int base = 0; base < M; base += 1024) {
    const int e = base + tid;
    int label = 0, grp = 0;
    int64_t k = 0;
    bool take = false;
    if (e < M) {
      k = slot_of(e, label, grp);
      take = __float_as_uint(u.sel_score[k]) >= (kSep ? s_cut[grp] : T);
    }
    int total;
    const int64_t pos = (int64_t)b * cap + out + block_excl_scan(take ? 1 : 0, s_wave, total);
    out += total;
    if (take) {
      const int r = u.sel_row[k];
      det_rows[pos] = r;
      det_labels[pos] = label;
      det_scores[pos] = u.sel_score[k];
      const float *src = u.boxes + 7 * (kSep ? (int64_t)(p.row_begin[b] + r) : (int64_t)(p.row_begin[b] + r) * p.C + label);
#pragma unroll
      for (int d = 0; d < 7; ++d) det_boxes[7 * pos + d] = src[d];
    }
  }
  if (tid == 0) {
    int cand = 0, big = 0, most = 0;
    for (int j = 0; j < nc; ++j) {
      const int c = u.seg_cnt[s0 + j], k = u.seg_kept[s0 + j];
      cand += c;
      big = c > big ? c : big;
      most = k > most ? k : most;
    }
    int32_t *w = info + (int64_t)b * kRoiInfoWords;
    w[0] = out; w[1] = M; w[2] = cand; w[3] = big; w[4] = most; w[6] = 0; w[7] = 0;
    if (!kSep) w[5] = 0;                               // (kSep: k_roi_post_rows's flag for a sep_id out of range)
  }
}

// scratch layout in int32 words (8-byte items first); n_cap bounds N, n_max the longest scene
struct RoiPostLayout {
  int64_t S, P, cbmax, keep_stride;
  int64_t o_mask, o_keep, o_prob, o_boxes, o_row, o_score, o_nms, o_seg, words;
};
static RoiPostLayout roi_post_layout(int nb, int64_t n_max, int64_t n_cap, int C, int pre_max) {
  RoiPostLayout L;
  L.S = (int64_t)nb * (C - 1);
  const int64_t longest = n_max < pre_max ? n_max : pre_max;
  L.P = ceil_div(longest > 0 ? longest : 1, (int64_t)64) * 64;
  L.cbmax = L.P / 64;
  L.keep_stride = L.P;
  int64_t o = 0;
  L.o_mask = o;  o += 2 * L.S * L.P * L.cbmax;
  L.o_keep = o;  o += 2 * L.S * L.keep_stride;
  L.o_prob = o;  o += n_cap * C;
  L.o_boxes = o; o += n_cap * C * 7;
  L.o_row = o;   o += L.S * L.P;
  L.o_score = o; o += L.S * L.P;
  L.o_nms = o;   o += L.S * L.P * 7;
  L.o_seg = o;   o += 3 * L.S;
  L.words = o + (o & 1);
  return L;
}

static int roi_post_check_shape(const char *fn, int nb, int C, int pre_max) {
  if (C < 2 || C > kRoiMaxClasses) { set_error("%s: C must be 2 .. 32 (class 0 = background)", fn); return AABR_EINVAL; }
  if (nb < 1 || nb > kRoiMaxBatch) { set_error("%s: nb must be 1 .. 16", fn); return AABR_EINVAL; }
  if (pre_max < 1 || pre_max > kRoiMaxPre) { set_error("%s: pre_max must be 1 .. 2048", fn); return AABR_EINVAL; }
  return AABR_OK;
}

} // namespace aabr
using namespace aabr;

extern "C" int64_t aabr_roi_post_scratch_words(int nb, int64_t n_max, int C, int pre_max) {
  if (roi_post_check_shape("aabr_roi_post_scratch_words", nb, C, pre_max) != AABR_OK || n_max < 0 ||
      n_max * nb * C * 7 >= (int64_t)1 << 31)
    return -1;
  return roi_post_layout(nb, n_max, n_max * nb, C, pre_max).words;
}

// `groups`: null, or the separated-classifier groups (aabr_roi_post_detections_grouped): C = C_tot, class-agnostic
// regression, `sep_id` int32 [N], boxes [N, 7], nf = C_tot - G segments per scene
static int roi_post_detections(const char *fn, const SepGroups *groups, const int32_t *sep_id, const float *class_logits,
                               const float *box_regression,
                               const float *proposals, int nb, const int64_t *n_host, int C, int class_specific,
                               const float *weights_host, int corner_coder, float clip, float score_thresh,
                               float nms_thresh, float nms_min_yx, float nms_min_z, int only_xy, int pre_max,
                               int post_max, int detections_per_img, float *prob, float *boxes, int64_t *det_rows,
                               int64_t *det_labels, float *det_scores, float *det_boxes, int32_t *info,
                               int32_t *scratch, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  int rc = roi_post_check_shape(fn, nb, C, pre_max);
  if (rc != AABR_OK) return rc;
  AABR_CHECK_ARG_AS(fn, corner_coder == 0 || corner_coder == 1, "corner_coder must be 0 (centroid) or 1 (two corners)");
  AABR_CHECK_ARG_AS(fn, post_max >= 1 && post_max <= pre_max, "post_max must be 1 .. pre_max");
  AABR_CHECK_ARG_AS(fn, n_host && weights_host, "null host table");
  RoiPostParams p;
  int64_t N = 0, n_max = 0;
  for (int b = 0; b <= kRoiMaxBatch; ++b) {
    p.row_begin[b] = (int32_t)N;
    if (b < nb) {
      AABR_CHECK_ARG_AS(fn, n_host[b] >= 0, "negative scene length");
      N += n_host[b];
      n_max = n_host[b] > n_max ? n_host[b] : n_max;
      AABR_CHECK_ARG_AS(fn, N * C * 7 < (int64_t)1 << 31, "too many rows (N * C * 7 must stay below 2^31)");
    }
  }
  AABR_CHECK_ARG_AS(fn, info, "null pointer (info)");
  AABR_CHECK_HIP(hipMemsetAsync(info, 0, (size_t)nb * kRoiInfoWords * sizeof(int32_t), st));
  if (N == 0) return AABR_OK;
  AABR_CHECK_ARG_AS(fn, class_logits && box_regression && proposals && det_rows && det_labels && det_scores && det_boxes &&
                     scratch, "null pointer");
  AABR_CHECK_ARG_AS(fn, ((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
  AABR_CHECK_ARG_AS(fn, !groups || sep_id, "null pointer (sep_id)");
  const RoiPostLayout L = roi_post_layout(nb, n_max, N, C, pre_max);   // (groups: sized for C_tot - 1 >= nf segments)
  const SepGroups q = groups ? *groups : SepGroups();
  const int64_t S = groups ? (int64_t)nb * q.nf : L.S;
  p.nb = nb; p.C = C; p.reg_classes = class_specific ? C : 1;
  p.pre_max = pre_max; p.post_max = post_max; p.D = detections_per_img; p.only_xy = only_xy ? 1 : 0;
  p.P = (int)L.P; p.cbmax = (int)L.cbmax; p.keep_stride = (int)L.keep_stride;
  p.score_thresh = score_thresh; p.nms_thresh = nms_thresh; p.clip = clip; p.min_yx = nms_min_yx; p.min_z = nms_min_z;
  for (int d = 0; d < 7; ++d) p.w.w[d] = weights_host[d];
  RoiPostBufs u;
  u.prob = prob ? prob : reinterpret_cast<float *>(scratch + L.o_prob);
  u.boxes = boxes ? boxes : reinterpret_cast<float *>(scratch + L.o_boxes);
  u.mask = reinterpret_cast<unsigned long long *>(scratch + L.o_mask);
  u.keep = reinterpret_cast<int64_t *>(scratch + L.o_keep);
  u.sel_row = scratch + L.o_row;
  u.sel_score = reinterpret_cast<float *>(scratch + L.o_score);
  u.nms_boxes = reinterpret_cast<float *>(scratch + L.o_nms);
  u.seg_m = scratch + L.o_seg;
  u.seg_cnt = u.seg_m + L.S;
  u.seg_kept = u.seg_cnt + L.S;
  const int64_t cap = (int64_t)(groups ? q.nf : C - 1) * post_max;
  const int64_t longest = n_max < pre_max ? n_max : pre_max;     // no sorted list is longer
  const dim3 row_grid((unsigned)ceil_div(N, (int64_t)256));
  if (groups && S == 0) return AABR_OK;                // no group has a foreground column: nothing can be detected
  const auto launch = [&](auto corner, auto sep) {     // the five launches of one (coder, groups) form
    constexpr bool kCorner = decltype(corner)::value, kSep = decltype(sep)::value;
    hipLaunchKernelGGL((k_roi_post_rows<kCorner, kSep>), row_grid, dim3(256), 0, st, class_logits, box_regression,
                       proposals, sep_id, N, p, q, u.prob, u.boxes, info);
    hipLaunchKernelGGL(k_roi_post_select<kSep>, dim3((unsigned)S), dim3(1024), 0, st, p, u, q, sep_id);
    hipLaunchKernelGGL(k_roi_post_mask,
                       dim3((unsigned)ceil_div(longest, (int64_t)kNmsRows), (unsigned)ceil_div(longest, (int64_t)64),
                            (unsigned)S),
                       dim3(256), 0, st, p, u);
    hipLaunchKernelGGL(k_roi_post_scan, dim3((unsigned)S), dim3(256), 0, st, p, u);
    hipLaunchKernelGGL(k_roi_post_scene<kSep>, dim3((unsigned)nb), dim3(1024), 0, st, p, u, q, cap, det_rows, det_labels,
                       det_scores, det_boxes, info);
  };
  const std::true_type yes;
  const std::false_type no;
  if (groups) corner_coder ? launch(yes, yes) : launch(no, yes);
  else corner_coder ? launch(yes, no) : launch(no, no);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_post_detections(const float *class_logits, const float *box_regression, const float *proposals,
                                        int nb, const int64_t *n_host, int C, int class_specific,
                                        const float *weights_host, float clip, float score_thresh, float nms_thresh,
                                        float nms_min_yx, float nms_min_z, int only_xy, int pre_max, int post_max,
                                        int detections_per_img, float *prob, float *boxes, int64_t *det_rows,
                                        int64_t *det_labels, float *det_scores, float *det_boxes, int32_t *info,
                                        int32_t *scratch, void *stream_) {
  return roi_post_detections("aabr_roi_post_detections", nullptr, nullptr, class_logits, box_regression, proposals, nb, n_host, C,
                             class_specific, weights_host, 0, clip, score_thresh, nms_thresh, nms_min_yx, nms_min_z, only_xy,
                             pre_max, post_max, detections_per_img, prob, boxes, det_rows, det_labels, det_scores, det_boxes,
                             info, scratch, stream_);
}

// the same with the coder's form chosen by the caller: corner_coder 0 = centroid (the entry above), 1 = two corners
extern "C" int aabr_roi_post_detections_coder(const float *class_logits, const float *box_regression,
                                              const float *proposals, int nb, const int64_t *n_host, int C,
                                              int class_specific, const float *weights_host, int corner_coder, float clip,
                                              float score_thresh, float nms_thresh, float nms_min_yx, float nms_min_z,
                                              int only_xy, int pre_max, int post_max, int detections_per_img, float *prob,
                                              float *boxes, int64_t *det_rows, int64_t *det_labels, float *det_scores,
                                              float *det_boxes, int32_t *info, int32_t *scratch, void *stream_) {
  return roi_post_detections("aabr_roi_post_detections_coder", nullptr, nullptr, class_logits, box_regression, proposals, nb, n_host, C,
                             class_specific, weights_host, corner_coder, clip, score_thresh, nms_thresh, nms_min_yx,
                             nms_min_z, only_xy, pre_max, post_max, detections_per_img, prob, boxes, det_rows, det_labels,
                             det_scores, det_boxes, info, scratch, stream_);
}

// the separated-classifier form: C_tot columns shared by G groups, class-agnostic regression [N, 7], sep_id int32 [N]
extern "C" int aabr_roi_post_detections_grouped(const float *class_logits, const float *box_regression,
                                                const float *proposals, const int32_t *sep_id, int nb,
                                                const int64_t *n_host, int G, int C_tot, const int32_t *class_nums_host,
                                                const int32_t *cols_host, const float *weights_host, int corner_coder,
                                                float clip, float score_thresh, float nms_thresh, float nms_min_yx,
                                                float nms_min_z, int only_xy, int pre_max, int post_max,
                                                int detections_per_img, float *prob, float *boxes, int64_t *det_rows,
                                                int64_t *det_labels, float *det_scores, float *det_boxes, int32_t *info,
                                                int32_t *scratch, void *stream_) {
  SepGroups q;
  int rc = fill_sep_groups(q, __func__, G, C_tot, class_nums_host, cols_host);
  if (rc != AABR_OK) return rc;
  return roi_post_detections(__func__, &q, sep_id, class_logits, box_regression, proposals, nb, n_host, C_tot, 0,
                             weights_host, corner_coder, clip, score_thresh, nms_thresh, nms_min_yx, nms_min_z, only_xy,
                             pre_max, post_max, detections_per_img, prob, boxes, det_rows, det_labels, det_scores,
                             det_boxes, info, scratch, stream_);
}

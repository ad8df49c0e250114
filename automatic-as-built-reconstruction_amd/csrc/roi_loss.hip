// roi_loss.hip -- the training half of the box head: FastRCNNLossComputation (modeling/roi_heads/box_head_3d/loss.py:137-382,
// the non-separated path) in two stages, mirroring its `subsample` and `__call__`.
//
// Stage 1, aabr_roi_targets (loss.py:163-293).  The reference loops over the scenes and, per scene, materialises the
// [G, n] IoU matrix, takes torch.max, gathers the matched boxes, encodes, runs the sampler (two nonzero + two randperm)
// and a third nonzero for the compaction.  Here, for the whole batch (<= 16 scenes):
//   R1 k_roi_match     16 lanes per proposal (wave64, 256 threads = 16 proposals per workgroup, grid.y = scene): the
//                      scene's ground-truth boxes pass through LDS in chunks of 128 (thickness clamps applied once per
//                      box when staged), the 16 lanes share a chunk's boxes, every pair goes through iou_eval_entry and
//                      the z-overlap factor -- the arithmetic of aabr_boxes_iou_3d -- and the lanes' running maxima are
//                      folded across the wave into the first maximum (a NaN entry wins, as in torch.max); then the
//                      Matcher's two thresholds, the label and BoxCoder3D.encode (box_encode7, the function behind
//                      aabr_box_encode) against the matched box.  The matrix is stored only when the caller asks for it.
//   S1..S4             the sampler over the labels: K1 .. K4 of sample_shared.h, the code aabr_sample_list runs
//                      (list form: key over (seed, scene, row); >= 1 positive, 0 negative, everything else ignored);
//   R2 k_roi_compact   one workgroup per scene sorts the <= 512 selected rows ascending in LDS (bitonic) -- the order of
//                      nonzero(pos | neg), loss.py:279-281 -- and gathers labels, regression targets and boxes.
// 1 memset + 6 launches whatever nb, G and the class count; no host read; no float atomics.
//
// Stage 2, aabr_roi_box_loss_forward / _backward (loss.py:295-382): F.cross_entropy over the sampled rows and the
// per-class smooth-L1 of the positives, both / N_s.  One thread per row: the C logits are read once (fp32 or bf16),
// max -> sum of expf in class order -> logf; the row's seven regression columns are those of its label.  Per-thread sums in
// row order, a fixed tree per workgroup, the workgroups' sums added in order by one thread: bit-identical run to run.
// The backward writes every element of both gradients (zeros included), so the caller fills nothing.
// A label outside [0, C) is never used as an index: the row is skipped and a flag word is raised.
//
// With separated-classifier groups (sep_groups.h; the reference's seperate_classifier.py loops over the groups around the
// code above) both stages have a grouped form of the same launch counts: stage 1 runs over (scene, group) segments with
// the scene's ground truth filtered by group on the device (k_roi_gt_keys, the caller's stable sort, k_roi_match<.., true>);
// stage 2 is the same three kernels with one accumulator set per group (k_roi_loss_*<true>).
#include "common.h"
#include "iou_math.h"
#include "nms_shared.h"
#include "sample_shared.h"
#include "sep_groups.h"

namespace aabr {

namespace {

using namespace aabr_iou;

constexpr int kRoiMaxBatch = 16;
constexpr int kRoiTgtChunk = 128;
constexpr int kRoiInfoWords = 8;
constexpr int kRoiLossBlocks = 512;

struct RoiTargetParams {
  int64_t prop_begin[kRoiMaxBatch];   // first proposal row of scene b
  int64_t gt_begin[kRoiMaxBatch];     // first ground-truth row of scene b
  int64_t iou_begin[kRoiMaxBatch];    // first float of scene b's [G_b, n_b] matrix
  int32_t n[kRoiMaxBatch], g[kRoiMaxBatch];
  float aug[4];                       // target_Y, target_Z, anchor_Y, anchor_Z
  float w[7];
  float fg, bg;
  int criterion, only_xy, B;
};

// kRoiLanes adjacent lanes of a wave share one proposal: lane j takes the ground-truth boxes j, j + kRoiLanes, ... of
// every staged chunk, so the serial chain per lane is ceil(G_b / kRoiLanes) pairs and a workgroup of 256 threads serves
// 256 / kRoiLanes proposals.  Each lane keeps the first maximum of its own ascending subsequence; the lanes' candidates
// are then folded with roi_better (iou_math.h), which prefers the lower index among equal values, so the result is the first maximum
// over all G_b whatever the lane count.  A NaN entry (0 / 0 in the z factor when only_xy is off: two zero heights at the
// same z with no thickness clamp) behaves as in torch.max / np.argmax: it wins, the first one by index, matched_val is
// NaN and, since both threshold comparisons are false for it, the proposal is matched to that box.
constexpr int kRoiLanes = 16;
constexpr int kRoiPropsPerBlock = 256 / kRoiLanes;

// kCorner: the regression targets are BoxCoder3D(is_corner_roi=True).encode (box_encode7_corner, corner_box.h) instead of
// the centroid encode; matching and labels are the same statements in both instances.
// kGrouped (aabr_roi_targets_grouped): a "scene" is a segment s = scene * groups + group, p.gt_begin[s] is its SCENE's
// first ground-truth row, and the segment's ground truth is a run of the batch's ground truth sorted by group key
// (k_roi_gt_keys): sorted positions lo .. lo + G of gt.keys, found here by two binary searches -- the host never
// learns a group's count.  Sorted position k stands for the ground-truth row gt.perm[k] of the batch and carries its
// group-local label in the key's low bits; matched_idx reports the row in the scene's own list.
struct RoiGroupedGt {
  const int64_t *keys, *perm;        // [total], ascending keys; null when not grouped
  int64_t total;
};
template <bool kCorner, bool kGrouped>
__global__ __launch_bounds__(256) void k_roi_match(RoiTargetParams p, const float *__restrict__ proposals,
                                                   const float *__restrict__ targets,
                                                   const int64_t *__restrict__ target_labels, RoiGroupedGt gt,
                                                   int64_t *__restrict__ matched_idx, float *__restrict__ matched_val,
                                                   int64_t *__restrict__ labels, float *__restrict__ reg_targets,
                                                   float *__restrict__ iou_out) {
  __shared__ float s_t5[kRoiTgtChunk][5];
  __shared__ float s_tz[kRoiTgtChunk][2];
  __shared__ int64_t s_rng[2];
  const int b = blockIdx.y;
  const int64_t N = p.n[b];
  if ((int64_t)blockIdx.x * kRoiPropsPerBlock >= N) return;   // grid.x is sized for the largest scene (workgroup-uniform)
  const int lane = threadIdx.x % kRoiLanes;
  const int64_t t = (int64_t)blockIdx.x * kRoiPropsPerBlock + threadIdx.x / kRoiLanes;
  int64_t lo = 0;                                      // kGrouped: the segment's first sorted position
  int G = p.g[b];
  if (kGrouped) {
    if (threadIdx.x < 2) {                             // lower_bound of the segment's first key and of the next one's
      const int64_t want = (int64_t)(b + (int)threadIdx.x) * kSepMaxCols;
      int64_t l = 0, h = gt.total;
      while (l < h) {
        const int64_t m = (l + h) >> 1;
        if (gt.keys[m] < want) l = m + 1; else h = m;
      }
      s_rng[threadIdx.x] = l;
    }
    __syncthreads();
    lo = s_rng[0];
    G = (int)(s_rng[1] - s_rng[0]);
  }
  const float *tg = kGrouped ? targets : targets + 7 * p.gt_begin[b];
  const auto gt_row = [&](int64_t k) -> int64_t { return kGrouped ? gt.perm[lo + k] : k; };   // row of `tg`
  float an[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float a5[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, az0 = 0.f, az1 = 0.f;
  if (t < N) {
    const float *pr = proposals + 7 * (p.prop_begin[b] + t);
#pragma unroll
    for (int d = 0; d < 7; ++d) an[d] = pr[d];
    // k_box7_to_2d on the proposal side (rotate_nms_3d_torch.py:59-66)
    const float th = an[3] < p.aug[2] ? p.aug[2] : an[3];
    const float h = an[5] < p.aug[3] ? p.aug[3] : an[5];
    a5[0] = an[0]; a5[1] = an[1]; a5[2] = th; a5[3] = an[4]; a5[4] = an[6];
    az0 = an[2]; az1 = an[2] + h;
  }
  float best = -__builtin_inff();
  int best_g = 0x7fffffff;                             // (a lane that saw no box loses every fold)
  for (int g0 = 0; g0 < G; g0 += kRoiTgtChunk) {
    const int gn = G - g0 < kRoiTgtChunk ? G - g0 : kRoiTgtChunk;
    __syncthreads();
    if ((int)threadIdx.x < gn) {
      const float *tb = tg + 7 * gt_row(g0 + threadIdx.x);
      const float th = tb[3] < p.aug[0] ? p.aug[0] : tb[3];
      const float h = tb[5] < p.aug[1] ? p.aug[1] : tb[5];
      s_t5[threadIdx.x][0] = tb[0]; s_t5[threadIdx.x][1] = tb[1]; s_t5[threadIdx.x][2] = th;
      s_t5[threadIdx.x][3] = tb[4]; s_t5[threadIdx.x][4] = tb[6];
      s_tz[threadIdx.x][0] = tb[2]; s_tz[threadIdx.x][1] = tb[2] + h;
    }
    __syncthreads();
    if (t < N)
      for (int g = lane; g < gn; g += kRoiLanes) {
        float t5[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) t5[d] = s_t5[g][d];
        float v = iou_eval_entry(t5, a5, p.criterion);
        if (!p.only_xy) {
          const float t0 = s_tz[g][0], t1 = s_tz[g][1];
          const float overlap = fminf(az1, t1) - fmaxf(az0, t0);
          const float common = fmaxf(az1, t1) - fminf(az0, t0);
          v = v * (overlap / common);
        }
        if (iou_out) iou_out[p.iou_begin[b] + (int64_t)(g0 + g) * N + t] = v;
        if (roi_better(v, g0 + g, best, best_g)) { best = v; best_g = g0 + g; }
      }
  }
  // fold the kRoiLanes candidates of a proposal (every lane of the wave takes part; lane 0 of each group ends with the
  // group's result, the groups being aligned runs of kRoiLanes lanes)
#pragma unroll
  for (int w = kRoiLanes / 2; w > 0; w >>= 1) {
    const float ov = __shfl_xor(best, w);
    const int og = __shfl_xor(best_g, w);
    if (roi_better(ov, og, best, best_g)) { best = ov; best_g = og; }
  }
  if (t >= N || lane != 0) return;
  const int64_t o = p.prop_begin[b] + t;
  if (G == 0) {                                        // loss.py:200-206
    matched_idx[o] = -1;
    matched_val[o] = 0.f;
    labels[o] = 0;
#pragma unroll
    for (int d = 0; d < 7; ++d) reg_targets[7 * o + d] = 0.f;
    return;
  }
  const int64_t mi = best < p.bg ? -1 : (best < p.fg ? -2 : best_g);   // BELOW_LOW_THRESHOLD / BETWEEN_THRESHOLDS
  matched_idx[o] = kGrouped && mi >= 0 ? gt_row(mi) - p.gt_begin[b] : mi;
  matched_val[o] = best;
  if (kGrouped) labels[o] = mi >= 0 ? (gt.keys[lo + mi] & (kSepMaxCols - 1)) : (mi == -1 ? 0 : -1);
  else labels[o] = mi >= 0 ? target_labels[p.gt_begin[b] + mi] : (mi == -1 ? 0 : -1);
  const float *tb = tg + 7 * gt_row(mi < 0 ? 0 : mi);  // target[matched_idxs.clamp(min=0)]: the un-thickened boxes
  float g7[7], e[7];
#pragma unroll
  for (int d = 0; d < 7; ++d) g7[d] = tb[d];
  if (kCorner) box_encode7_corner(g7, an, p.w, e);
  else box_encode7(g7, an, p.w, e);
#pragma unroll
  for (int d = 0; d < 7; ++d) reg_targets[7 * o + d] = e[d];
}

// one workgroup per scene: the sampler's list (positives then negatives, selection order, indices into the batch's
// concatenated labels) -> ascending scene-local rows, with the rows' labels, regression targets and boxes
__global__ __launch_bounds__(256) void k_roi_compact(RoiTargetParams p, const int64_t *__restrict__ sel,
                                                     const int32_t *__restrict__ sinfo,
                                                     const float *__restrict__ proposals,
                                                     const int64_t *__restrict__ labels,
                                                     const float *__restrict__ reg_targets,
                                                     int64_t *__restrict__ samp_rows, int64_t *__restrict__ samp_labels,
                                                     float *__restrict__ samp_targets, float *__restrict__ samp_boxes,
                                                     int32_t *__restrict__ info) {
  __shared__ uint32_t s[kLossMaxB];
  __shared__ int s_cnt;
  const int b = blockIdx.x, t = threadIdx.x, B = p.B;
  const int32_t *si = sinfo + b * kInfoWords;
  const int kp = si[0], kn = si[1];
  int n2 = 2;
  while (n2 < kp + kn) n2 <<= 1;                       // kp + kn <= B <= 512
  if (t == 0) s_cnt = 0;
  __syncthreads();
  int mine = 0;
  for (int i = t; i < n2; i += 256) {
    const int64_t v = i < kp + kn ? sel[(int64_t)b * B + i] : -1;
    s[i] = v >= 0 ? (uint32_t)(v - p.prop_begin[b]) : 0xffffffffu;   // (-1 only after the sampler's overflow)
    mine += v >= 0;
  }
  if (mine) atomicAdd(&s_cnt, mine);
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = t; i < n2; i += 256) {
        const int j = i ^ stride;
        if (j > i) {
          const uint32_t x = s[i], y = s[j];
          if ((y < x) == ((i & size) == 0)) { s[i] = y; s[j] = x; }
        }
      }
    }
  __syncthreads();
  const int cnt = s_cnt;
  for (int i = t; i < B; i += 256) {
    const int64_t o = (int64_t)b * B + i;
    if (i < cnt) {
      const int64_t r = p.prop_begin[b] + s[i];
      samp_rows[o] = s[i];
      samp_labels[o] = labels[r];
#pragma unroll
      for (int d = 0; d < 7; ++d) {
        samp_targets[7 * o + d] = reg_targets[7 * r + d];
        samp_boxes[7 * o + d] = proposals[7 * r + d];
      }
    } else {
      samp_rows[o] = -1;
      samp_labels[o] = -1;
#pragma unroll
      for (int d = 0; d < 7; ++d) { samp_targets[7 * o + d] = 0.f; samp_boxes[7 * o + d] = 0.f; }
    }
  }
  if (t == 0) {
    int32_t *inf = info + b * kRoiInfoWords;
    inf[0] = cnt; inf[1] = kp; inf[2] = kn; inf[3] = si[2]; inf[4] = si[3];
    inf[5] = p.n[b] - si[2] - si[3]; inf[6] = si[6]; inf[7] = 0;
  }
}

// ---- stage 2 -------------------------------------------------------------------------------------------------------
// One partial, one finalize and one backward kernel, each instantiated for the plain loss and for the loss with
// separated-classifier groups (SeperateClassifier.roi_cross_entropy_seperated / roi_box_loss_seperated).  What differs
// between the two travels in RoiLossForm<kGrouped>; the statements are the same.
//   plain    one accumulator set; the row's columns are all C in order (no table: C has no upper limit); the regression
//            is [n, 7 C] (class specific: the row's seven columns are those of its label) or [n, 7]; divisor n -- a row
//            whose label is outside [0, C) counts in it.
//   grouped  row i belongs to group sep_id[i]; its cross-entropy runs over that group's columns of the C_tot logits in
//            group-local order with the target column cols[g][label]; the regression is [n, 7]; one accumulator set per
//            group (a register per group, no dynamically indexed array) and the divisor is the group's row count n_g,
//            counted here: a row whose label is outside [0, class_nums[g]) counts in n_g, a row whose sep_id is outside
//            [0, G) is in no group.
// Neither out-of-range value is used as an index; both raise the flag, add nothing and get exact zero gradients.
// A workgroup's partial sums: cls [kSets], box [kSets], grouped only rows [kSets] (int32 bits), then the flag.
template <bool kGrouped> struct RoiLossForm;
template <> struct RoiLossForm<false> {
  static constexpr bool kIsGrouped = false;
  static constexpr int kSets = 1, kPartWords = 3;
  int C, class_specific;
  __device__ int groups() const { return 1; }
  __device__ int width() const { return C; }                       // row stride of the logits
  __device__ bool specific() const { return class_specific != 0; }
  __device__ bool group_of(int64_t, int &g) const { g = 0; return true; }
  __device__ RowCols<false> cols(int) const { return {C}; }
};
template <> struct RoiLossForm<true> {
  static constexpr bool kIsGrouped = true;
  static constexpr int kSets = kSepMaxGroups, kPartWords = 3 * kSepMaxGroups + 1;
  SepGroups q;
  const int32_t *sep_id;
  __device__ int groups() const { return q.G; }
  __device__ int width() const { return q.C_tot; }
  __device__ bool specific() const { return false; }
  __device__ bool group_of(int64_t i, int &g) const { g = sep_id[i]; return g >= 0 && g < q.G; }
  __device__ RowCols<true> cols(int g) const { return RowCols<true>(q, g); }
};

// Per-thread sums in row order (the seven smooth-L1 terms of a row first, then the row), a fixed tree per workgroup
template <bool kGrouped>
__global__ __launch_bounds__(256) void k_roi_loss_partial(const void *__restrict__ logits, const void *__restrict__ reg,
                                                          int bf16, int64_t n, RoiLossForm<kGrouped> f,
                                                          const int64_t *__restrict__ labels,
                                                          const float *__restrict__ targets, float beta,
                                                          float *__restrict__ partial) {
  constexpr int kSets = RoiLossForm<kGrouped>::kSets, kWords = RoiLossForm<kGrouped>::kPartWords;
  __shared__ float s_red[2][256];
  __shared__ int s_cnt[kGrouped ? 256 : 1];            // (the row counts: grouped only, unused and absent when plain)
  __shared__ int s_bad;
  const int t = threadIdx.x, C = f.width();
  if (t == 0) s_bad = 0;
  float cls[kSets], box[kSets];
  int cnt[kSets];
#pragma unroll
  for (int g = 0; g < kSets; ++g) { cls[g] = 0.f; box[g] = 0.f; cnt[g] = 0; }
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256) {
    int sid;
    if (!f.group_of(i, sid)) { bad = true; continue; }
    const auto cols = f.cols(sid);
    const int64_t l = labels[i];
    float c = 0.f, b = 0.f;
    if (l < 0 || l >= cols.cn) {
      bad = true;
    } else {
      const auto x = [&](int k) { return ld(logits, i * C + k, bf16); };
      const RowSoftmax r = row_softmax(cols, x);
      c = (r.m + logf(r.s)) - x(cols.col((int)l));
      if (l > 0) {
        const int64_t c0 = f.specific() ? i * 7 * C + 7 * l : i * 7;
        for (int d = 0; d < 7; ++d) b += smooth_l1_term(fabsf(ld(reg, c0 + d, bf16) - targets[i * 7 + d]), beta);
      }
    }
#pragma unroll
    for (int g = 0; g < kSets; ++g)                    // (a register per group: no dynamically indexed array)
      if (g == sid) { cls[g] += c; box[g] += b; cnt[g] += 1; }
  }
  __syncthreads();
  if (bad) s_bad = 1;                                  // (every writer stores the same value)
  float *out = partial + (int64_t)kWords * blockIdx.x;
#pragma unroll
  for (int g = 0; g < kSets; ++g) {
    if (g >= f.groups()) break;                        // workgroup-uniform
    __syncthreads();
    s_red[0][t] = cls[g];
    s_red[1][t] = box[g];
    if constexpr (kGrouped) s_cnt[t] = cnt[g];
    for (int w = 128; w > 0; w >>= 1) {
      __syncthreads();
      if (t < w) {
        s_red[0][t] += s_red[0][t + w];
        s_red[1][t] += s_red[1][t + w];
        if constexpr (kGrouped) s_cnt[t] += s_cnt[t + w];
      }
    }
    if (t == 0) {
      out[g] = s_red[0][0];
      out[kSets + g] = s_red[1][0];
      if constexpr (kGrouped) out[2 * kSets + g] = __int_as_float(s_cnt[0]);
    }
  }
  __syncthreads();
  if (t == 0) out[kWords - 1] = s_bad ? 1.f : 0.f;
}

// thread g: set g's sums in workgroup order, / its divisor (0 / 0 = NaN for an empty sample or a group without rows, like
// aabr_rpn_loss_forward); grouped: rows[g] = n_g for the backward
template <bool kGrouped>
__global__ __launch_bounds__(64) void k_roi_loss_finalize(int nblocks, int G, const float *__restrict__ partial, int64_t n,
                                                          float *__restrict__ cls_loss, float *__restrict__ box_loss,
                                                          int32_t *__restrict__ rows, int32_t *__restrict__ flag) {
  constexpr int kSets = RoiLossForm<kGrouped>::kSets, kWords = RoiLossForm<kGrouped>::kPartWords;
  const int g = threadIdx.x;
  if (g >= G) return;
  float cls = 0.f, box = 0.f;
  int cnt = 0, bad = 0;
  for (int i = 0; i < nblocks; ++i) {
    const float *in = partial + (int64_t)kWords * i;
    cls += in[g];
    box += in[kSets + g];
    if (kGrouped) cnt += __float_as_int(in[2 * kSets + g]);
    bad |= in[kWords - 1] != 0.f;
  }
  const float div = kGrouped ? (float)cnt : (float)n;
  cls_loss[g] = cls / div;
  box_loss[g] = box / div;
  if (kGrouped) rows[g] = cnt;
  if (g == 0) *flag = bad;
}

// one thread per row writes the row's logit gradients and its regression gradients, zeros included.  Plain: each of the
// C + 7 C (or 7) elements is stored once.  Grouped: zeros over the C_tot columns, then the group's own columns over them.
template <bool kGrouped>
__global__ __launch_bounds__(256) void k_roi_loss_backward(const void *__restrict__ logits, const void *__restrict__ reg,
                                                           int bf16, int64_t n, RoiLossForm<kGrouped> f,
                                                           const int64_t *__restrict__ labels,
                                                           const float *__restrict__ targets, float beta,
                                                           const int32_t *__restrict__ rows,
                                                           const float *__restrict__ g_cls, const float *__restrict__ g_box,
                                                           void *__restrict__ grad_logits, void *__restrict__ grad_reg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int C = f.width();
  const int64_t l = labels[i];
  int sid;
  const bool ok = f.group_of(i, sid) && l >= 0 && l < f.cols(sid).cn;
  if (kGrouped)
    for (int k = 0; k < C; ++k) st(grad_logits, i * C + k, 0.f, bf16);
  float gb = 0.f;
  if (ok) {
    const auto cols = f.cols(sid);
    const float div = kGrouped ? (float)rows[sid] : (float)n;
    const auto x = [&](int k) { return ld(logits, i * C + k, bf16); };
    const RowSoftmax r = row_softmax(cols, x);
    const float gc = g_cls[sid] / div;
    gb = g_box[sid] / div;
    for (int k = 0; k < cols.cn; ++k) {
      const int c = cols.col(k);
      st(grad_logits, i * C + c, (r.prob(x(c)) - (k == l ? 1.f : 0.f)) * gc, bf16);
    }
  } else if (!kGrouped) {
    for (int k = 0; k < C; ++k) st(grad_logits, i * C + k, 0.f, bf16);
  }
  const int W = f.specific() ? 7 * C : 7;
  const int c0 = ok && l > 0 ? (f.specific() ? 7 * (int)l : 0) : -7;   // first column of the row's own box, or none
  for (int c = 0; c < W; ++c) {
    float v = 0.f;
    if (c >= c0 && c < c0 + 7 && c0 >= 0) v = smooth_l1_grad(ld(reg, i * W + c, bf16) - targets[i * 7 + (c - c0)], beta) * gb;
    st(grad_reg, i * W + c, v, bf16);
  }
}

}  // namespace

}  // namespace aabr

using namespace aabr;

extern "C" int64_t aabr_roi_targets_scratch_words(int nb) {
  // the sampler's words, its selected list (int64 [nb][512]) and its info block
  if (nb < 1 || nb > kRoiMaxBatch) return -1;
  return aabr_rpn_loss_scratch_words(nb) + (int64_t)nb * (2 * kLossMaxB + kInfoWords) + 2;
}

// The body of every aabr_roi_targets* entry point, reported under the caller's name `fn`.  groups == 0: nb scenes, g_host
// their ground-truth counts.  groups >= 2 (aabr_roi_targets_grouped): nb = scenes x groups segments (scene-major), n_host
// the segments' proposal counts, g_host the SCENES' ground-truth counts, gt_keys / gt_perm the batch's ground truth
// sorted by group key (RoiGroupedGt); target_labels is not read.
static int roi_targets_run(const char *fn, const float *proposals, const float *targets, const int64_t *target_labels,
                           int nb, int groups, const int64_t *n_host, const int64_t *g_host, const int64_t *gt_keys,
                           const int64_t *gt_perm, const float *aug_host, int criterion, int only_xy, float fg_iou,
                           float bg_iou, const float *weights_host, int corner_coder, uint32_t seed,
                           int batch_size_per_image, int num_pos_max, int64_t *matched_idx, float *matched_val,
                           int64_t *labels, float *regression_targets, float *iou_out, int64_t *samp_rows,
                           int64_t *samp_labels, float *samp_targets, float *samp_boxes, int32_t *info, int32_t *scratch,
                           hipStream_t st) {
  AABR_CHECK_ARG_AS(fn, corner_coder == 0 || corner_coder == 1, "corner_coder must be 0 (centroid) or 1 (two corners)");
  AABR_CHECK_ARG_AS(fn, nb >= 1 && nb <= kRoiMaxBatch, groups ? "scenes x groups must be 1 .. 16" : "nb must be 1 .. 16");
  AABR_CHECK_ARG_AS(fn, batch_size_per_image >= 1 && batch_size_per_image <= kLossMaxB && num_pos_max >= 0 &&
                            num_pos_max <= batch_size_per_image,
                    "need 1 <= batch_size_per_image <= 512, 0 <= num_pos_max <= batch_size_per_image");
  AABR_CHECK_ARG_AS(fn, bg_iou <= fg_iou, "need bg_iou <= fg_iou");
  AABR_CHECK_ARG_AS(fn, n_host && g_host && aug_host && weights_host && samp_rows && samp_labels && samp_targets &&
                            samp_boxes && info && scratch, "null pointer");
  AABR_CHECK_ARG_AS(fn, ((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
  RoiTargetParams p = {};
  int64_t N = 0, G = 0, M = 0, nmax = 0;
  std::vector<int32_t> seg(2 * (size_t)nb);
  for (int b = 0; b < nb; ++b) {
    const bool scene_start = !groups || b % groups == 0;            // g_host has one entry per scene
    const int64_t gb = g_host[groups ? b / groups : b];
    AABR_CHECK_ARG_AS(fn, n_host[b] >= 0 && gb >= 0 && n_host[b] < ((int64_t)1 << 31) && gb < ((int64_t)1 << 31),
                      "row count out of range");
    p.prop_begin[b] = N; p.iou_begin[b] = M;
    p.gt_begin[b] = scene_start ? G : p.gt_begin[b - 1];
    p.n[b] = (int32_t)n_host[b]; p.g[b] = groups ? 0 : (int32_t)gb;   // (a segment's count is found on the device)
    seg[2 * b] = 0; seg[2 * b + 1] = (int32_t)n_host[b];
    N += n_host[b]; M += n_host[b] * gb;
    if (scene_start) G += gb;
    nmax = n_host[b] > nmax ? n_host[b] : nmax;
  }
  AABR_CHECK_ARG_AS(fn, N < ((int64_t)1 << 31), "more than 2^31 - 1 proposals per call");
  AABR_CHECK_ARG_AS(fn, G < ((int64_t)1 << 31), "more than 2^31 - 1 ground-truth boxes per call");
  AABR_CHECK_ARG_AS(fn, N == 0 || (proposals && matched_idx && matched_val && labels && regression_targets), "null pointer");
  AABR_CHECK_ARG_AS(fn, G == 0 || (targets && (groups ? gt_keys && gt_perm : target_labels != nullptr)), "null pointer");
  AABR_CHECK_ARG_AS(fn, !groups || !iou_out, "the grouped form does not store the IoU matrices");
  for (int d = 0; d < 4; ++d) p.aug[d] = aug_host[d];
  for (int d = 0; d < 7; ++d) p.w[d] = weights_host[d];
  p.fg = fg_iou; p.bg = bg_iou; p.criterion = criterion; p.only_xy = only_xy ? 1 : 0; p.B = batch_size_per_image;
  if (nmax > 0) {
    const dim3 grid((unsigned)ceil_div(nmax, kRoiPropsPerBlock), (unsigned)nb);
    const RoiGroupedGt gt = {gt_keys, gt_perm, G};
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, p, proposals, targets, target_labels, gt, matched_idx, matched_val,
                         labels, regression_targets, iou_out);
    };
    if (groups) corner_coder ? launch(k_roi_match<true, true>) : launch(k_roi_match<false, true>);
    else corner_coder ? launch(k_roi_match<true, false>) : launch(k_roi_match<false, false>);
  }
  // the sampler over the labels just written: the list form of aabr_sample_list, one chunk (nb <= 16)
  int64_t *sel = reinterpret_cast<int64_t *>(scratch + aabr_rpn_loss_scratch_words(nb) + (aabr_rpn_loss_scratch_words(nb) & 1));
  int32_t *sinfo = reinterpret_cast<int32_t *>(sel + (int64_t)nb * kLossMaxB);
  std::vector<const void *> label_ptrs(nb);
  for (int b = 0; b < nb; ++b) label_ptrs[b] = n_host[b] ? (const void *)(labels + p.prop_begin[b]) : nullptr;
  LossParams sp = {};
  sp.s.n_maps = 1; sp.s.A = 1; sp.flat = 1; sp.with_loss = 0; sp.label_mode = 1; sp.k_pos0 = num_pos_max;
  sp.B = batch_size_per_image; sp.seed = seed; sp.beta = 1.f;
  int rc = run_select_chunks(sp, fn, nb, seg.data(), nullptr, label_ptrs.data(), nullptr, nullptr, nullptr, sel, sinfo, scratch,
                             st);
  if (rc != AABR_OK) return rc;
  hipLaunchKernelGGL(k_roi_compact, dim3((unsigned)nb), dim3(256), 0, st, p, sel, sinfo, proposals, labels,
                     regression_targets, samp_rows, samp_labels, samp_targets, samp_boxes, info);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_targets_coder(const float *proposals, const float *targets, const int64_t *target_labels, int nb,
                                      const int64_t *n_host, const int64_t *g_host, const float *aug_host, int criterion,
                                      int only_xy, float fg_iou, float bg_iou, const float *weights_host,
                                      int corner_coder, uint32_t seed, int batch_size_per_image, int num_pos_max,
                                      int64_t *matched_idx, float *matched_val, int64_t *labels,
                                      float *regression_targets, float *iou_out, int64_t *samp_rows,
                                      int64_t *samp_labels, float *samp_targets, float *samp_boxes, int32_t *info,
                                      int32_t *scratch, void *stream_) {
  return roi_targets_run(__func__, proposals, targets, target_labels, nb, 0, n_host, g_host, nullptr, nullptr, aug_host,
                         criterion, only_xy, fg_iou, bg_iou, weights_host, corner_coder, seed, batch_size_per_image,
                         num_pos_max, matched_idx, matched_val, labels, regression_targets, iou_out, samp_rows, samp_labels,
                         samp_targets, samp_boxes, info, scratch, (hipStream_t)stream_);
}

// ---- the separated-classifier groups: stage 1 ---------------------------------------------------------------------------
// key of ground-truth row i of scene b: (b groups + g) kSepMaxCols + i_local when its label is column cols[g][i_local] of
// group g, nb groups kSepMaxCols (behind every segment) when no group owns the label.  A stable ascending sort of the keys
// puts every segment's ground truth in one run, ordered (group-local label, row): the order the reference's
// _seperating_ids gives a group's targets.
namespace {
struct RoiKeyParams {
  int64_t gt_begin[kRoiMaxBatch + 1];
  int nb;
};
__global__ __launch_bounds__(256) void k_roi_gt_keys(RoiKeyParams p, SepGroups q, const int64_t *__restrict__ target_labels,
                                                     int64_t *__restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.gt_begin[p.nb]) return;
  int b = 0;
  while (b + 1 < p.nb && i >= p.gt_begin[b + 1]) ++b;
  const int64_t l = target_labels[i];
  int64_t key = (int64_t)p.nb * q.G * kSepMaxCols;
  for (int g = 0; g < q.G; ++g)
    for (int k = 0; k < q.class_nums[g]; ++k)
      if (q.cols[g][k] == l) key = ((int64_t)b * q.G + g) * kSepMaxCols + k;
  keys[i] = key;
}
}  // namespace

extern "C" int aabr_roi_gt_group_keys(const int64_t *target_labels, int nb, const int64_t *g_host, int G, int C_tot,
                                      const int32_t *class_nums_host, const int32_t *cols_host, int64_t *keys,
                                      void *stream_) {
  SepGroups q;
  int rc = fill_sep_groups(q, __func__, G, C_tot, class_nums_host, cols_host);
  if (rc != AABR_OK) return rc;
  AABR_CHECK_ARG(nb >= 1 && (int64_t)nb * G <= kRoiMaxBatch, "scenes x groups must be 1 .. 16");
  AABR_CHECK_ARG(g_host, "null pointer");
  RoiKeyParams p = {};
  p.nb = nb;
  for (int b = 0; b < nb; ++b) {
    AABR_CHECK_ARG(g_host[b] >= 0 && g_host[b] < ((int64_t)1 << 31), "row count out of range");
    p.gt_begin[b + 1] = p.gt_begin[b] + g_host[b];
  }
  const int64_t total = p.gt_begin[nb];
  AABR_CHECK_ARG(total < ((int64_t)1 << 31), "more than 2^31 - 1 ground-truth boxes per call");
  if (total == 0) return AABR_OK;
  AABR_CHECK_ARG(target_labels && keys, "null pointer");
  hipLaunchKernelGGL(k_roi_gt_keys, dim3((unsigned)ceil_div(total, (int64_t)256)), dim3(256), 0, (hipStream_t)stream_, p, q,
                     target_labels, keys);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_targets_grouped(const float *proposals, const float *targets, const int64_t *gt_keys,
                                        const int64_t *gt_perm, int nb, int G, const int64_t *n_host,
                                        const int64_t *g_host, const float *aug_host, int criterion, int only_xy,
                                        float fg_iou, float bg_iou, const float *weights_host, int corner_coder,
                                        uint32_t seed, int batch_size_per_image, int num_pos_max, int64_t *matched_idx,
                                        float *matched_val, int64_t *labels, float *regression_targets,
                                        int64_t *samp_rows, int64_t *samp_labels, float *samp_targets, float *samp_boxes,
                                        int32_t *info, int32_t *scratch, void *stream_) {
  AABR_CHECK_ARG(G >= 2 && G <= kSepMaxGroups, "the group count must be 2 .. 8");
  AABR_CHECK_ARG(nb >= 1 && (int64_t)nb * G <= kRoiMaxBatch, "scenes x groups must be 1 .. 16");
  return roi_targets_run(__func__, proposals, targets, nullptr, nb * G, G, n_host, g_host, gt_keys, gt_perm, aug_host,
                         criterion, only_xy, fg_iou, bg_iou, weights_host, corner_coder, seed, batch_size_per_image,
                         num_pos_max, matched_idx, matched_val, labels, regression_targets, nullptr, samp_rows, samp_labels,
                         samp_targets, samp_boxes, info, scratch, (hipStream_t)stream_);
}

// the centroid coder: the signature of before aabr_roi_targets_coder
extern "C" int aabr_roi_targets(const float *proposals, const float *targets, const int64_t *target_labels, int nb,
                                const int64_t *n_host, const int64_t *g_host, const float *aug_host, int criterion,
                                int only_xy, float fg_iou, float bg_iou, const float *weights_host, uint32_t seed,
                                int batch_size_per_image, int num_pos_max, int64_t *matched_idx, float *matched_val,
                                int64_t *labels, float *regression_targets, float *iou_out, int64_t *samp_rows,
                                int64_t *samp_labels, float *samp_targets, float *samp_boxes, int32_t *info,
                                int32_t *scratch, void *stream_) {
  return aabr_roi_targets_coder(proposals, targets, target_labels, nb, n_host, g_host, aug_host, criterion, only_xy, fg_iou,
                                bg_iou, weights_host, 0, seed, batch_size_per_image, num_pos_max, matched_idx, matched_val,
                                labels, regression_targets, iou_out, samp_rows, samp_labels, samp_targets, samp_boxes, info,
                                scratch, stream_);
}

// ---- stage 2: the four entry points, one runner per direction ------------------------------------------------------------
extern "C" int64_t aabr_roi_box_loss_scratch_floats(void) { return RoiLossForm<false>::kPartWords * kRoiLossBlocks; }
extern "C" int64_t aabr_roi_box_loss_grouped_scratch_floats(void) {
  return (int64_t)RoiLossForm<true>::kPartWords * kRoiLossBlocks;
}

static int roi_loss_blocks(int64_t n) {
  int64_t nblk = ceil_div(n, 256);
  return (int)(nblk < 1 ? 1 : (nblk > kRoiLossBlocks ? kRoiLossBlocks : nblk));
}

// The body of both forward entry points, reported under the caller's name `fn`.  `groups` null: the plain loss over C
// columns.  Else the grouped one: C = C_tot, class-agnostic regression, `sep_id` int32 [n], group_rows int32 [G].
static int roi_loss_forward_run(const char *fn, const SepGroups *groups, const int32_t *sep_id, const void *class_logits,
                                const void *box_regression, int input_bf16, int64_t n, int C, int class_specific,
                                const int64_t *labels, const float *regression_targets, float beta, float *cls_loss,
                                float *box_loss, int32_t *group_rows, int32_t *flag, float *scratch, hipStream_t st) {
  AABR_CHECK_ARG_AS(fn, n >= 0 && C >= 1 && beta > 0.f, groups ? "need n >= 0, beta > 0" : "need n >= 0, C >= 1, beta > 0");
  AABR_CHECK_ARG_AS(fn, n * 7 * (int64_t)C < ((int64_t)1 << 31),
                    groups ? "n * 7 C_tot must stay below 2^31" : "n * 7 C must stay below 2^31");
  AABR_CHECK_ARG_AS(fn, cls_loss && box_loss && (!groups || group_rows) && flag && scratch, "null pointer");
  AABR_CHECK_ARG_AS(fn, n == 0 || (class_logits && box_regression && (!groups || sep_id) && labels && regression_targets),
                    "null pointer");
  const int nblk = roi_loss_blocks(n);
  const auto launch = [&](auto f, int G) {
    constexpr bool kGrouped = decltype(f)::kIsGrouped;
    hipLaunchKernelGGL(k_roi_loss_partial<kGrouped>, dim3((unsigned)nblk), dim3(256), 0, st, class_logits, box_regression,
                       input_bf16 ? 1 : 0, n, f, labels, regression_targets, beta, scratch);
    hipLaunchKernelGGL(k_roi_loss_finalize<kGrouped>, dim3(1), dim3(64), 0, st, nblk, G, scratch, n, cls_loss, box_loss,
                       group_rows, flag);
  };
  if (groups) launch(RoiLossForm<true>{*groups, sep_id}, groups->G);
  else launch(RoiLossForm<false>{C, class_specific ? 1 : 0}, 1);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

static int roi_loss_backward_run(const char *fn, const SepGroups *groups, const int32_t *sep_id, const void *class_logits,
                                 const void *box_regression, int input_bf16, int64_t n, int C, int class_specific,
                                 const int64_t *labels, const float *regression_targets, float beta,
                                 const int32_t *group_rows, const float *grad_cls_loss, const float *grad_box_loss,
                                 void *grad_logits, void *grad_regression, hipStream_t st) {
  AABR_CHECK_ARG_AS(fn, n >= 0 && C >= 1 && beta > 0.f, groups ? "need n >= 0, beta > 0" : "need n >= 0, C >= 1, beta > 0");
  AABR_CHECK_ARG_AS(fn, n * 7 * (int64_t)C < ((int64_t)1 << 31),
                    groups ? "n * 7 C_tot must stay below 2^31" : "n * 7 C must stay below 2^31");
  AABR_CHECK_ARG_AS(fn, (!groups || group_rows) && grad_cls_loss && grad_box_loss, "null pointer");
  if (n == 0) return AABR_OK;
  AABR_CHECK_ARG_AS(fn, class_logits && box_regression && (!groups || sep_id) && labels && regression_targets &&
                            grad_logits && grad_regression, "null pointer");
  const auto launch = [&](auto f) {
    hipLaunchKernelGGL(k_roi_loss_backward<decltype(f)::kIsGrouped>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st,
                       class_logits, box_regression, input_bf16 ? 1 : 0, n, f, labels, regression_targets, beta, group_rows,
                       grad_cls_loss, grad_box_loss, grad_logits, grad_regression);
  };
  if (groups) launch(RoiLossForm<true>{*groups, sep_id});
  else launch(RoiLossForm<false>{C, class_specific ? 1 : 0});
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_box_loss_forward(const void *class_logits, const void *box_regression, int input_bf16, int64_t n,
                                         int C, int class_specific, const int64_t *labels,
                                         const float *regression_targets, float beta, float *cls_loss, float *box_loss,
                                         int32_t *flag, float *scratch, void *stream_) {
  return roi_loss_forward_run(__func__, nullptr, nullptr, class_logits, box_regression, input_bf16, n, C, class_specific,
                              labels, regression_targets, beta, cls_loss, box_loss, nullptr, flag, scratch,
                              (hipStream_t)stream_);
}

extern "C" int aabr_roi_box_loss_backward(const void *class_logits, const void *box_regression, int input_bf16, int64_t n,
                                          int C, int class_specific, const int64_t *labels,
                                          const float *regression_targets, float beta, const float *grad_cls_loss,
                                          const float *grad_box_loss, void *grad_logits, void *grad_regression,
                                          void *stream_) {
  return roi_loss_backward_run(__func__, nullptr, nullptr, class_logits, box_regression, input_bf16, n, C, class_specific,
                               labels, regression_targets, beta, nullptr, grad_cls_loss, grad_box_loss, grad_logits,
                               grad_regression, (hipStream_t)stream_);
}

extern "C" int aabr_roi_box_loss_grouped_forward(const void *class_logits, const void *box_regression, int input_bf16,
                                                 int64_t n, int G, int C_tot, const int32_t *class_nums_host,
                                                 const int32_t *cols_host, const int32_t *sep_id, const int64_t *labels,
                                                 const float *regression_targets, float beta, float *cls_loss,
                                                 float *box_loss, int32_t *group_rows, int32_t *flag, float *scratch,
                                                 void *stream_) {
  SepGroups q;
  int rc = fill_sep_groups(q, __func__, G, C_tot, class_nums_host, cols_host);
  if (rc != AABR_OK) return rc;
  return roi_loss_forward_run(__func__, &q, sep_id, class_logits, box_regression, input_bf16, n, C_tot, 0, labels,
                              regression_targets, beta, cls_loss, box_loss, group_rows, flag, scratch, (hipStream_t)stream_);
}

extern "C" int aabr_roi_box_loss_grouped_backward(const void *class_logits, const void *box_regression, int input_bf16,
                                                  int64_t n, int G, int C_tot, const int32_t *class_nums_host,
                                                  const int32_t *cols_host, const int32_t *sep_id, const int64_t *labels,
                                                  const float *regression_targets, float beta, const int32_t *group_rows,
                                                  const float *grad_cls_loss, const float *grad_box_loss,
                                                  void *grad_logits, void *grad_regression, void *stream_) {
  SepGroups q;
  int rc = fill_sep_groups(q, __func__, G, C_tot, class_nums_host, cols_host);
  if (rc != AABR_OK) return rc;
  return roi_loss_backward_run(__func__, &q, sep_id, class_logits, box_regression, input_bf16, n, C_tot, 0, labels,
                               regression_targets, beta, group_rows, grad_cls_loss, grad_box_loss, grad_logits,
                               grad_regression, (hipStream_t)stream_);
}

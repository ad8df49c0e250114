// det_eval.hip -- detection evaluation on the device: eval_detection_suncg of the reference
// (data3d/evaluation/suncg/suncg_eval.py:733-986, use_07_metric=True) without its Python loops over scenes and classes,
// which launch one IoU kernel and read one matrix back per scene and class.
//
// aabr_det_eval_match, for S scenes (any S >= 1: the per-scene offsets are device arrays, not a by-value table):
//   E1 k_eval_prep    one thread per ground-truth box: its index among the boxes of its class in its scene (the
//                     reference's gt_index counts inside `gt_bbox[gt_label == l]`) and the reset of its claim word;
//   E2 k_eval_match   the structure of k_roi_match (roi_loss.hip): 16 lanes per detection, 16 detections per workgroup,
//                     grid.y = scene; the scene's ground truth passes through LDS in chunks of 128 with its label, a lane
//                     skips boxes of another class, every remaining pair goes through iou_eval_entry and the z factor
//                     (the arithmetic of aabr_boxes_iou_3d), candidates are folded with roi_better (first maximum, a NaN
//                     wins); then the threshold, the 64-bit integer atomicMin of the detection's claim key on the matched
//                     box, and the key of the global ordering;
//   E3 k_eval_flag    one thread per detection: flag 1 iff its key is the minimum its box received.
// The claim is an integer minimum rather than one thread per ground-truth box scanning its scene's detections: the
// minimum costs one atomic per matched detection and is independent of their order, the scan would read every detection
// of the scene once per box.
// Between the two entries the caller sorts the keys (a stable sort: equal scores stay in ascending row).
// aabr_det_eval_curves:
//   E4 k_eval_curve   one workgroup per class walks its run of the sorted order in chunks of 256: integer prefix sums of
//                     the flags (wave shuffles, wave totals through LDS, an integer carry), rec / prec as float64
//                     quotients of exact integers, and the maxima / last positions of det_eval.h's EvalAcc, which are
//                     exact and order-independent, so the chunk size changes no bit.
//                     One workgroup per class is serial in the class's detection count (one CU; not timed beyond a few
//                     thousand detections per class).
// A whole evaluation is 4 library launches + the caller's sort, whatever S, C and the list lengths; one host read.
// No float atomics anywhere: bit-identical run to run.
#include "common.h"
#include "det_eval.h"
#include "iou_math.h"

namespace aabr {

namespace {

using namespace aabr_iou;
using namespace aabr_eval;

constexpr int kEvalTgtChunk = 128;
constexpr int kEvalLanes = 16;
constexpr int kEvalDetsPerBlock = 256 / kEvalLanes;
constexpr int kEvalScanChunk = 256;
constexpr unsigned long long kEvalNoClaim = 0xffffffffffffffffull;

struct EvalMatchParams {
  float aug[4];                       // target_Y, target_Z, anchor_Y, anchor_Z
  float thresh;
  int only_xy, C;
  int64_t S, N, G;
};

// scene of ground-truth row g: the last b with begin[b] <= g (empty scenes share a begin with their successor)
__device__ inline int64_t eval_scene_of(const int64_t *__restrict__ begin, int64_t S, int64_t g) {
  int64_t lo = 0, hi = S;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (begin[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_eval_prep(int64_t S, int64_t G, const int64_t *__restrict__ gt_begin,
                                                   const int64_t *__restrict__ gt_labels, int32_t *__restrict__ gt_rank,
                                                   unsigned long long *__restrict__ claim) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  const int64_t b = eval_scene_of(gt_begin, S, g);
  const int64_t l = gt_labels[g];
  int32_t rank = 0;
  for (int64_t r = gt_begin[b]; r < g; ++r) rank += gt_labels[r] == l;
  gt_rank[g] = rank;
  claim[g] = kEvalNoClaim;
}

__global__ __launch_bounds__(256) void k_eval_match(EvalMatchParams p, const int64_t *__restrict__ det_begin,
                                                    const int64_t *__restrict__ gt_begin, const float *__restrict__ dets,
                                                    const int64_t *__restrict__ det_labels,
                                                    const float *__restrict__ det_scores, const float *__restrict__ gts,
                                                    const int64_t *__restrict__ gt_labels,
                                                    const int32_t *__restrict__ gt_rank,
                                                    unsigned long long *__restrict__ claim, int64_t *__restrict__ gt_index,
                                                    float *__restrict__ pred_iou, int32_t *__restrict__ gt_row,
                                                    int64_t *__restrict__ sort_key, float *__restrict__ iou_out,
                                                    const int64_t *__restrict__ iou_begin) {
  __shared__ float s_t5[kEvalTgtChunk][5];
  __shared__ float s_tz[kEvalTgtChunk][2];
  __shared__ int s_lab[kEvalTgtChunk];
  const int64_t b = blockIdx.y;
  const int64_t d0 = det_begin[b], g_first = gt_begin[b];
  int64_t N = det_begin[b + 1] - d0, G64 = gt_begin[b + 1] - g_first;
  if (N > p.N - d0) N = p.N - d0;                      // (offsets that disagree with the totals read nothing outside)
  if (G64 > p.G - g_first) G64 = p.G - g_first;
  if ((int64_t)blockIdx.x * kEvalDetsPerBlock >= N) return;   // grid.x is sized for the largest scene (workgroup-uniform)
  const int G = (int)G64;
  const int lane = threadIdx.x % kEvalLanes;
  const int64_t t = (int64_t)blockIdx.x * kEvalDetsPerBlock + threadIdx.x / kEvalLanes;
  const float *tg = gts + 7 * g_first;
  float a5[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, az0 = 0.f, az1 = 0.f;
  int my_lab = -2;                                     // matches no staged label (a bad ground-truth label is staged as -1)
  if (t < N) {
    const float *pr = dets + 7 * (d0 + t);
    float an[7];
#pragma unroll
    for (int d = 0; d < 7; ++d) an[d] = pr[d];
    const float th = an[3] < p.aug[2] ? p.aug[2] : an[3];
    const float h = an[5] < p.aug[3] ? p.aug[3] : an[5];
    a5[0] = an[0]; a5[1] = an[1]; a5[2] = th; a5[3] = an[4]; a5[4] = an[6];
    az0 = an[2]; az1 = an[2] + h;
    const int64_t l = det_labels[d0 + t];
    if (l >= 0 && l < p.C) my_lab = (int)l;
  }
  float best = -__builtin_inff();
  int best_g = 0x7fffffff;                             // (a lane that saw no box of the class loses every fold)
  for (int g0 = 0; g0 < G; g0 += kEvalTgtChunk) {
    const int gn = G - g0 < kEvalTgtChunk ? G - g0 : kEvalTgtChunk;
    __syncthreads();
    if ((int)threadIdx.x < gn) {
      const float *tb = tg + 7 * (int64_t)(g0 + threadIdx.x);
      const float th = tb[3] < p.aug[0] ? p.aug[0] : tb[3];
      const float h = tb[5] < p.aug[1] ? p.aug[1] : tb[5];
      s_t5[threadIdx.x][0] = tb[0]; s_t5[threadIdx.x][1] = tb[1]; s_t5[threadIdx.x][2] = th;
      s_t5[threadIdx.x][3] = tb[4]; s_t5[threadIdx.x][4] = tb[6];
      s_tz[threadIdx.x][0] = tb[2]; s_tz[threadIdx.x][1] = tb[2] + h;
      const int64_t l = gt_labels[g_first + g0 + threadIdx.x];
      s_lab[threadIdx.x] = l >= 0 && l < p.C ? (int)l : -1;
    }
    __syncthreads();
    if (t < N)
      for (int g = lane; g < gn; g += kEvalLanes) {
        if (s_lab[g] != my_lab) continue;
        float t5[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) t5[d] = s_t5[g][d];
        float v = iou_eval_entry(t5, a5, -1);
        if (!p.only_xy) {
          const float t0 = s_tz[g][0], t1 = s_tz[g][1];
          const float overlap = fminf(az1, t1) - fmaxf(az0, t0);
          const float common = fmaxf(az1, t1) - fminf(az0, t0);
          v = v * (overlap / common);
        }
        if (iou_out) iou_out[iou_begin[b] + (int64_t)(g0 + g) * N + t] = v;
        if (roi_better(v, g0 + g, best, best_g)) { best = v; best_g = g0 + g; }
      }
  }
  // fold the kEvalLanes candidates of a detection (every lane of the wave takes part; lane 0 of each aligned group of
  // kEvalLanes lanes ends with the group's result)
#pragma unroll
  for (int w = kEvalLanes / 2; w > 0; w >>= 1) {
    const float ov = __shfl_xor(best, w);
    const int og = __shfl_xor(best_g, w);
    if (roi_better(ov, og, best, best_g)) { best = ov; best_g = og; }
  }
  if (t >= N || lane != 0) return;
  const int64_t o = d0 + t;
  const float score = det_scores[o];
  int64_t gi = -1;
  int32_t row = -1;
  float v = 0.f;                                       // no ground truth of the class in the scene: iou 0, no match
  if (best_g != 0x7fffffff) {
    v = best;
    if (!(best < p.thresh)) {                          // strict: IoU == thresh matches, and so does a NaN
      row = (int32_t)(g_first + best_g);
      gi = gt_rank[row];
      atomicMin(&claim[row], (unsigned long long)eval_claim_key(score, (uint32_t)o));
    }
  }
  gt_index[o] = gi;
  pred_iou[o] = v;
  gt_row[o] = row;
  sort_key[o] = eval_sort_key(my_lab >= 0 ? my_lab : p.C, score);
}

__global__ __launch_bounds__(256) void k_eval_flag(int64_t N, const float *__restrict__ det_scores,
                                                   const int32_t *__restrict__ gt_row,
                                                   const unsigned long long *__restrict__ claim,
                                                   int8_t *__restrict__ match) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= N) return;
  const int32_t row = gt_row[o];
  match[o] = row >= 0 && claim[row] == (unsigned long long)eval_claim_key(det_scores[o], (uint32_t)o) ? 1 : 0;
}

// first position of `keys` (ascending) that is >= v
__device__ inline int64_t eval_lower_bound(const int64_t *__restrict__ keys, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kEvalScanChunk) void k_eval_curve(int C, int64_t N, int64_t G,
                                                               const int64_t *__restrict__ sorted_key,
                                                               const int64_t *__restrict__ order,
                                                               const int8_t *__restrict__ match,
                                                               const float *__restrict__ pred_iou,
                                                               const float *__restrict__ det_scores,
                                                               const int64_t *__restrict__ gt_labels,
                                                               double *__restrict__ rows, int64_t *__restrict__ cls) {
  constexpr int kWaves = kEvalScanChunk / 64;
  __shared__ int64_t s_range[2];
  __shared__ unsigned long long s_cnt[2];              // ground truth of this class, ground-truth labels out of range
  __shared__ int s_wave[kWaves];
  __shared__ double s_pick[3][2];                      // prec, rec at the 0.5 pick, the 0.7 pick, the last position
  __shared__ int s_has[2];
  __shared__ EvalAcc s_acc[kWaves];
  const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    s_range[0] = eval_lower_bound(sorted_key, N, (int64_t)l << 32);
    s_range[1] = eval_lower_bound(sorted_key, N, (int64_t)(l + 1) << 32);
    s_cnt[0] = s_cnt[1] = 0;
    s_has[0] = s_has[1] = 0;
  }
  __syncthreads();
  const int64_t begin = s_range[0], end = s_range[1];
  {
    unsigned long long mine = 0, bad = 0;
    for (int64_t g = tid; g < G; g += kEvalScanChunk) {
      const int64_t gl = gt_labels[g];
      mine += gl == l;
      bad += gl < 0 || gl >= C;
    }
    if (mine) atomicAdd(&s_cnt[0], mine);              // (integer sums in LDS: order-independent)
    if (bad) atomicAdd(&s_cnt[1], bad);
  }
  __syncthreads();
  const int64_t n_pos = (int64_t)s_cnt[0], n_det = end - begin;
  EvalAcc acc;
  eval_acc_init(acc);
  int64_t carry = 0;                                   // flags set before this chunk
  for (int64_t base = begin; base < end; base += kEvalScanChunk) {
    const int64_t i = base + tid;
    const bool valid = i < end;
    const int64_t src = valid ? order[i] : 0;
    const int m = valid ? (match[src] == 1) : 0;
    int incl = m;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    __syncthreads();                                   // (the previous chunk's s_wave has been read)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      before += w < wave ? s_wave[w] : 0;
      total += s_wave[w];
    }
    if (valid) {
      const int64_t pos = i - begin, tp = carry + before + incl;
      const float score = det_scores[src];
      double rec, prec;
      eval_acc_point(acc, pos, tp, n_pos, (double)pred_iou[src], &rec, &prec);
      rows[4 * i] = rec;
      rows[4 * i + 1] = prec;
      rows[4 * i + 2] = (double)score;
      rows[4 * i + 3] = (double)pred_iou[src];
      // pr_of_score_threshold: k = count(score > th) - 1.  The scores descend (NaN last), so the count is a prefix and
      // position k is the one that passes while its successor does not; k = -1 reads the last position.
      const bool last = i + 1 == end;
      const float next = last ? 0.f : det_scores[order[i + 1]];
      if ((double)score > 0.5 && (last || !((double)next > 0.5))) { s_pick[0][0] = prec; s_pick[0][1] = rec; s_has[0] = 1; }
      if ((double)score > 0.7 && (last || !((double)next > 0.7))) { s_pick[1][0] = prec; s_pick[1][1] = rec; s_has[1] = 1; }
      if (last) { s_pick[2][0] = prec; s_pick[2][1] = rec; }
    }
    carry += total;
  }
  // the threads' accumulators -> one: maxima and ORs, so the tree's shape changes nothing
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    EvalAcc o;
    for (int j = 0; j < kEvalSteps; ++j) {
      o.p[j] = __shfl_xor(acc.p[j], d);
      o.u[j] = __shfl_xor(acc.u[j], d);
      o.last_le[j] = __shfl_xor(acc.last_le[j], d);
    }
    o.ge = __shfl_xor(acc.ge, d);
    eval_acc_merge(acc, o);
  }
  if (lane == 0) s_acc[wave] = acc;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < kWaves; ++w) eval_acc_merge(acc, s_acc[w]);
  int64_t *ci = cls + (int64_t)l * kEvalClassWords;
  double *cd = reinterpret_cast<double *>(ci);
  for (int j = 0; j < kEvalClassWords; ++j) ci[j] = 0;
  ci[kEvalWordNPos] = n_pos;
  ci[kEvalWordNDet] = n_det;
  ci[kEvalWordTp] = carry;
  ci[kEvalWordBegin] = begin;
  if (l == 0) {
    ci[kEvalWordBadGt] = (int64_t)s_cnt[1];
    ci[kEvalWordBadDet] = N - eval_lower_bound(sorted_key, N, (int64_t)C << 32);
  }
  const double nan = __builtin_nan("");
  if (n_det == 0) {                                    // prec[l] is None: AP and the rows are NaN (suncg_eval.py:939-942)
    for (int j = kEvalWordAp; j < kEvalWordTh7 + 2; ++j) cd[j] = nan;
    return;
  }
  double s_le[kEvalSteps];
  for (int j = 0; j < kEvalSteps; ++j)
    s_le[j] = acc.last_le[j] >= 0 ? (double)det_scores[order[begin + acc.last_le[j]]] : 0.0;
  // np.max of the scores: the first of the descending run, NaN if any score is NaN (those are last)
  const float s_first = det_scores[order[begin]], s_last = det_scores[order[end - 1]];
  const double max_score = s_last != s_last ? (double)s_last : (double)s_first;
  cd[kEvalWordAp] = eval_finish(acc, s_le, max_score, cd + kEvalWordTable);
  for (int k = 0; k < 2; ++k) {
    const int src = s_has[k] ? k : 2;
    cd[(k ? kEvalWordTh7 : kEvalWordTh5)] = s_pick[src][0];
    cd[(k ? kEvalWordTh7 : kEvalWordTh5) + 1] = s_pick[src][1];
  }
}

}  // namespace

}  // namespace aabr

using namespace aabr;

extern "C" int64_t aabr_det_eval_scratch_words(int64_t n_det, int64_t n_gt) {
  // claim words (64-bit, first), the ground truth's class-local indices, the detections' matched rows
  if (n_det < 0 || n_gt < 0 || n_det >= ((int64_t)1 << 31) || n_gt >= ((int64_t)1 << 31)) return -1;
  return 2 * n_gt + n_gt + n_det + 2;
}

extern "C" int aabr_det_eval_match(const float *det_boxes, const int64_t *det_labels, const float *det_scores,
                                   const float *gt_boxes, const int64_t *gt_labels, int64_t n_scenes,
                                   const int64_t *det_begin, const int64_t *gt_begin, int64_t n_det, int64_t n_gt,
                                   int64_t n_det_max, int C, float iou_thresh, const float *aug_host, int only_xy,
                                   int64_t *gt_index, float *pred_iou, int8_t *match, int64_t *sort_key, float *iou_out,
                                   const int64_t *iou_begin, int32_t *scratch, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  AABR_CHECK_ARG(C >= 2 && C <= 32, "need 2 <= C <= 32");
  AABR_CHECK_ARG(n_scenes >= 1 && n_scenes <= 65535, "need 1 <= n_scenes <= 65535");
  AABR_CHECK_ARG(n_det >= 0 && n_gt >= 0 && n_det_max >= 0 && n_det_max <= n_det, "negative count, or n_det_max > n_det");
  AABR_CHECK_ARG(n_det < ((int64_t)1 << 31) && n_gt < ((int64_t)1 << 31), "more than 2^31 - 1 rows per call");
  AABR_CHECK_ARG(det_begin && gt_begin && aug_host && scratch, "null pointer");
  AABR_CHECK_ARG(n_det == 0 || (det_boxes && det_labels && det_scores && gt_index && pred_iou && match && sort_key),
                 "null pointer");
  AABR_CHECK_ARG(n_gt == 0 || (gt_boxes && gt_labels), "null pointer");
  AABR_CHECK_ARG(!iou_out || iou_begin, "iou_out needs iou_begin");
  AABR_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "scratch must be 8-byte aligned");
  AABR_CHECK_ARG(n_det == 0 || n_det_max >= 1, "n_det_max is 0 with detections present");
  unsigned long long *claim = reinterpret_cast<unsigned long long *>(scratch);
  int32_t *gt_rank = scratch + 2 * n_gt;
  int32_t *gt_row = gt_rank + n_gt;
  EvalMatchParams p = {};
  for (int d = 0; d < 4; ++d) p.aug[d] = aug_host[d];
  p.thresh = iou_thresh; p.only_xy = only_xy ? 1 : 0; p.C = C; p.S = n_scenes; p.N = n_det; p.G = n_gt;
  if (n_gt > 0)
    hipLaunchKernelGGL(k_eval_prep, dim3((unsigned)ceil_div(n_gt, 256)), dim3(256), 0, st, n_scenes, n_gt, gt_begin,
                       gt_labels, gt_rank, claim);
  if (n_det > 0) {
    hipLaunchKernelGGL(k_eval_match, dim3((unsigned)ceil_div(n_det_max, kEvalDetsPerBlock), (unsigned)n_scenes), dim3(256),
                       0, st, p, det_begin, gt_begin, det_boxes, det_labels, det_scores, gt_boxes, gt_labels, gt_rank,
                       claim, gt_index, pred_iou, gt_row, sort_key, iou_out, iou_begin);
    hipLaunchKernelGGL(k_eval_flag, dim3((unsigned)ceil_div(n_det, 256)), dim3(256), 0, st, n_det, det_scores, gt_row,
                       claim, match);
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_det_eval_curves(const int64_t *sorted_key, const int64_t *order, const int8_t *match,
                                    const float *pred_iou, const float *det_scores, const int64_t *gt_labels,
                                    int64_t n_det, int64_t n_gt, int C, double *rows, int64_t *cls, void *stream_) {
  AABR_CHECK_ARG(C >= 2 && C <= 32, "need 2 <= C <= 32");
  AABR_CHECK_ARG(n_det >= 0 && n_gt >= 0, "negative count");
  AABR_CHECK_ARG(n_det < ((int64_t)1 << 31) && n_gt < ((int64_t)1 << 31), "more than 2^31 - 1 rows per call");
  AABR_CHECK_ARG(cls, "null pointer");
  AABR_CHECK_ARG(n_det == 0 || (sorted_key && order && match && pred_iou && det_scores && rows), "null pointer");
  AABR_CHECK_ARG(n_gt == 0 || gt_labels, "null pointer");
  hipLaunchKernelGGL(k_eval_curve, dim3((unsigned)C), dim3(kEvalScanChunk), 0, (hipStream_t)stream_, C, n_det, n_gt,
                     sorted_key, order, match, pred_iou, det_scores, gt_labels, rows, cls);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_det_eval_scan_chunk(void) { return kEvalScanChunk; }

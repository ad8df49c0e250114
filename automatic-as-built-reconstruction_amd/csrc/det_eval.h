// det_eval.h -- the element-level pieces of the detection evaluation (det_eval.hip) that the kernels and a host program
// must compute alike: the descending-score order key, the claim key of the match flag, the threshold table of the
// 11-point metric and its accumulation.  No HIP in here beyond the AABR_HD qualifier (the style of iou_math.h), so a
// stand-alone program runs all of it under the host sanitizers (tests/det_eval_host_harness.cpp).
//
// Behavioural contract: data3d/evaluation/suncg/suncg_eval.py:733-986 of the reference with use_07_metric=True.
#pragma once
#include <stdint.h>
#ifndef AABR_HD
#ifdef __HIPCC__
#define AABR_HD __host__ __device__ inline
#else
#define AABR_HD static inline
#endif
#endif

namespace aabr_eval {

constexpr int kEvalSteps = 11;            // recall thresholds 0.0, 0.1, .. 1.0
constexpr int kEvalClassWords = 64;       // 64-bit words of one class's result row
// word offsets inside a class's row: doubles first, integers from kEvalWordNPos on
constexpr int kEvalWordAp = 0;            // AP
constexpr int kEvalWordTable = 1;         // [11][4] = threshold, precision, score, IoU
constexpr int kEvalWordTh5 = 45;          // precision, recall at score > 0.5
constexpr int kEvalWordTh7 = 47;          // precision, recall at score > 0.7
constexpr int kEvalWordNPos = 56;         // ground-truth boxes of the class
constexpr int kEvalWordNDet = 57;         // detections of the class
constexpr int kEvalWordTp = 58;           // detections flagged 1
constexpr int kEvalWordBegin = 59;        // first row of the class's run in the sorted order
constexpr int kEvalWordBadGt = 60;        // (row of class 0 only) ground-truth labels outside [0, C)
constexpr int kEvalWordBadDet = 61;       // (row of class 0 only) detection labels outside [0, C)

AABR_HD uint32_t eval_f32_bits(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return u;
}

// Unsigned key whose ASCENDING order is DESCENDING score: +inf first, then the finite values downwards (-0.0 and +0.0
// share one key), -inf, and every NaN last under the single key 0xffffffff (no other score maps there).  Equal keys
// are left to the caller's tie rule (ascending detection row).
AABR_HD uint32_t eval_score_key(float s) {
  if (s != s) return 0xffffffffu;
  if (s == 0.0f) s = 0.0f;                                  // -0.0 -> +0.0
  const uint32_t u = eval_f32_bits(s);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

// What the detections matched to one ground-truth box compete with: the smallest key is the first in score order, the
// lower detection row among equal scores.  Its minimum over any set is independent of the order of the comparisons.
AABR_HD uint64_t eval_claim_key(float score, uint32_t det_row) {
  return ((uint64_t)eval_score_key(score) << 32) | (uint64_t)det_row;
}

// Key of the global ordering: class-major, then descending score; a stable sort adds "ascending row among equals".
// cls = C for a detection whose label lies outside [0, C): those rows sort behind every class.
AABR_HD int64_t eval_sort_key(int cls, float score) {
  return (int64_t)(((uint64_t)(uint32_t)cls << 32) | (uint64_t)eval_score_key(score));
}

// threshold i of np.arange(0.0, 1.1, 0.1): start + i * step in double
AABR_HD double eval_threshold(int i) { return 0.0 + (double)i * 0.1; }

// np.nan_to_num of a double
AABR_HD double eval_nan_to_num(double v) {
  if (v != v) return 0.0;
  if (v > 1.7976931348623157e308) return 1.7976931348623157e308;
  if (v < -1.7976931348623157e308) return -1.7976931348623157e308;
  return v;
}

// What one class's curve contributes to the 11 rows, gathered over its detections in ANY order: every member is a
// maximum or an OR, so splitting the detections among threads or chunks changes no bit.
struct EvalAcc {
  double p[kEvalSteps];        // max nan_to_num(prec) over rec >= t (only meaningful where bit i of `ge` is set)
  double u[kEvalSteps];        // max nan_to_num(pred_iou) over rec >= t
  int64_t last_le[kEvalSteps]; // largest position with rec <= t, -1: none
  uint32_t ge;                 // bit i: some position has rec >= t_i
};

AABR_HD void eval_acc_init(EvalAcc &a) {
  for (int i = 0; i < kEvalSteps; ++i) { a.p[i] = 0.0; a.u[i] = 0.0; a.last_le[i] = -1; }
  a.ge = 0;
}

// position `pos` (0-based in the class's sorted run) with tp true positives among the first pos + 1 detections
AABR_HD void eval_acc_point(EvalAcc &a, int64_t pos, int64_t tp, int64_t n_pos, double pred_iou, double *rec_out,
                            double *prec_out) {
  const double rec = (double)tp / (double)n_pos;            // 0 / 0 = NaN for a class without ground truth
  const double prec = (double)tp / (double)(pos + 1);       // tp + fp = pos + 1: every flag is 0 or 1
  const double pn = eval_nan_to_num(prec), un = eval_nan_to_num(pred_iou);
  for (int i = 0; i < kEvalSteps; ++i) {
    const double t = eval_threshold(i);
    if (rec >= t) {
      const bool first = !((a.ge >> i) & 1u);
      if (first || pn > a.p[i]) a.p[i] = pn;
      if (first || un > a.u[i]) a.u[i] = un;
      a.ge |= 1u << i;
    }
    if (rec <= t && pos > a.last_le[i]) a.last_le[i] = pos;
  }
  *rec_out = rec;
  *prec_out = prec;
}

AABR_HD void eval_acc_merge(EvalAcc &a, const EvalAcc &b) {
  for (int i = 0; i < kEvalSteps; ++i) {
    if ((b.ge >> i) & 1u) {
      const bool first = !((a.ge >> i) & 1u);
      if (first || b.p[i] > a.p[i]) a.p[i] = b.p[i];
      if (first || b.u[i] > a.u[i]) a.u[i] = b.u[i];
    }
    if (b.last_le[i] > a.last_le[i]) a.last_le[i] = b.last_le[i];
  }
  a.ge |= b.ge;
}

// The 11 rows [t, p, s, iou] and the AP of one class from its accumulator (suncg_eval.py:946-967).  score_at_last_le[i]
// is the score at position a.last_le[i] (unused where that is -1); max_score is np.max of the class's scores.
// The AP adds p / 11 in threshold order.
AABR_HD double eval_finish(const EvalAcc &a, const double *score_at_last_le, double max_score, double *table) {
  double ap = 0.0;
  for (int i = 0; i < kEvalSteps; ++i) {
    const bool any = (a.ge >> i) & 1u;
    const double p = any ? a.p[i] : 0.0;
    const double iou = any ? a.u[i] : 0.0;
    const double s = a.last_le[i] >= 0 ? score_at_last_le[i] : max_score + 0.01;
    ap += p / 11;
    table[4 * i] = eval_threshold(i);
    table[4 * i + 1] = p;
    table[4 * i + 2] = s;
    table[4 * i + 3] = iou;
  }
  return ap;
}

} // namespace aabr_eval

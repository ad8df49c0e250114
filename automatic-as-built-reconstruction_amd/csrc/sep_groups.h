// sep_groups.h -- the separated-classifier groups of the box head (MODEL.SEPARATE_CLASSES; the reference's
// modeling/seperate_classifier.py) as the kernels of roi_loss.hip and roi_post.hip see them: ONE record that travels by
// value in the kernel arguments, and the host-side checks every grouped entry point runs before its first HIP call.
//
// G groups share the C_tot columns of class_logits.  Group g owns class_nums[g] columns, cols[g][0 .. class_nums[g]), in
// group-local order; cols[g][0] is the group's background column (column 0 for group 0, num_input_classes + g - 1 for a
// separated group), every other column index is that class's original label.  No column belongs to two groups.
#pragma once
#include "common.h"

namespace aabr {

constexpr int kSepMaxGroups = 8, kSepMaxCols = 32;

struct SepGroups {
  int32_t G, C_tot, nf;                        // nf: the foreground columns of all groups together
  uint8_t class_nums[kSepMaxGroups];
  uint8_t cols[kSepMaxGroups][kSepMaxCols];
  uint8_t fg_col[kSepMaxCols], fg_group[kSepMaxCols];   // foreground column f in (group, group-local) order
  uint8_t fg_begin[kSepMaxGroups + 1];         // group g's foreground columns are fg_begin[g] .. fg_begin[g + 1]
};

// The columns one row's softmax runs over.  Plain (RowCols<false>): all cn = C columns, column k is k -- no table, so C
// has no upper limit here.  Grouped (RowCols<true>): group g's cn = class_nums[g] columns, column k is cols[g][k].
template <bool kGrouped> struct RowCols;
template <> struct RowCols<false> {
  int cn;
  __device__ int col(int k) const { return k; }
};
template <> struct RowCols<true> {
  const SepGroups &q;
  int g, cn;
  __device__ RowCols(const SepGroups &q_, int g_) : q(q_), g(g_), cn(q_.class_nums[g_]) {}
  __device__ int col(int k) const { return q.cols[g][k]; }
};

// The softmax statistics of one row, the one statement of them for the loss kernels (roi_loss.hip: x reads fp32 or bf16)
// and the post-processor (roi_post.hip: fp32): x(c) is the row's logit in column c; the maximum over the view's columns
// in order, then the sum of expf(x - m) in the same order.
struct RowSoftmax {
  float m, s;
  __device__ float prob(float x) const { return expf(x - m) / s; }
};
template <class Cols, class Load>
__device__ inline RowSoftmax row_softmax(const Cols &c, Load x) {
  RowSoftmax r;
  r.m = x(c.col(0));
  for (int k = 1; k < c.cn; ++k) r.m = fmaxf(r.m, x(c.col(k)));
  r.s = 0.f;
  for (int k = 0; k < c.cn; ++k) r.s += expf(x(c.col(k)) - r.m);
  return r;
}

// class_nums_host int32 [G], cols_host int32 [sum of class_nums]: the groups' column lists one after the other
inline int fill_sep_groups(SepGroups &q, const char *fn, int G, int C_tot, const int32_t *class_nums_host,
                           const int32_t *cols_host) {
  AABR_CHECK_ARG_AS(fn, G >= 2 && G <= kSepMaxGroups, "the group count must be 2 .. 8");
  AABR_CHECK_ARG_AS(fn, C_tot >= 2 && C_tot <= kSepMaxCols, "C_tot must be 2 .. 32");
  AABR_CHECK_ARG_AS(fn, class_nums_host && cols_host, "null group table");
  q = SepGroups();
  q.G = G; q.C_tot = C_tot;
  bool used[kSepMaxCols] = {};
  int o = 0, f = 0;
  for (int g = 0; g < G; ++g) {
    const int cn = class_nums_host[g];
    AABR_CHECK_ARG_AS(fn, cn >= 1 && cn <= C_tot, "a group needs 1 .. C_tot columns (its background column first)");
    q.class_nums[g] = (uint8_t)cn;
    q.fg_begin[g] = (uint8_t)f;
    for (int i = 0; i < cn; ++i, ++o) {
      const int c = cols_host[o];
      AABR_CHECK_ARG_AS(fn, c >= 0 && c < C_tot, "a column index is outside [0, C_tot)");
      AABR_CHECK_ARG_AS(fn, !used[c], "a column belongs to two groups");
      used[c] = true;
      q.cols[g][i] = (uint8_t)c;
      if (i > 0) { q.fg_col[f] = (uint8_t)c; q.fg_group[f] = (uint8_t)g; ++f; }
    }
  }
  q.fg_begin[G] = (uint8_t)f;
  q.nf = f;
  return AABR_OK;
}

} // namespace aabr

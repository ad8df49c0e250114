// rpn_loss.hip -- the RPN loss of the training step: RPNLossComputation.__call__ (modeling/rpn/loss_3d.py:201-251) for one
// objectness group, i.e. BalancedPositiveNegativeSampler (modeling/balanced_positive_negative_sampler.py:19-68), then
// smooth_l1_loss over the sampled positives (layers/smooth_l1_loss.py:34-52, yaw mode 'Diff') and
// binary_cross_entropy_with_logits over every sampled anchor, both divided by the batch's sampled count N_s.
//
// The reference concatenates the scales example-major (cat_scales_obj_reg), runs two torch.nonzero (host syncs) and two
// randperm per example and gathers.  Here nothing is concatenated: anchor (b, m, row r, a) is read where the RPN head
// wrote it, objectness / regression index (site_begin[b][m] + r) * A + a of map m, label / target index
// seg_begin[b][m] + r * A + a of example b's lists (the tables aabr_rpn_label_generation_targets takes; anchor_list.h).
//
// Selection rule (restated in include/aabr_hip.h): every anchor gets a 32-bit key, a chain of murmur3's finaliser
//   h = fmix32(seed ^ 0x9E3779B9); h = fmix32(h ^ v) for v in (example, map, x, y, z, anchor)
// (x, y, z: the site's coordinates), and the sample of a class is its k anchors with the smallest (key, map, x, y, z, a).
// A uniform random subset per seed, independent of the grid's row order.  Per chunk of <= 16 examples:
//   K1 12-bit histogram of the keys' leading bits, per (example, class);
//   K2 every workgroup resolves num_pos / num_neg from the histogram totals, finds the bin where the count from the
//      bottom reaches k, histogram of the next 12 bits inside it;
//   K3 the same one level down; every key whose 24-bit prefix is <= the threshold prefix becomes a candidate (k plus
//      the anchors sharing one 24-bit prefix: far below kLossCand for any list that fits in 31 bits of index);
//   K4 one workgroup per example sorts the candidates of each class (bitonic, in LDS, full tie-break), keeps k, writes
//      the selected list and the per-example sums of the loss terms of those <= B anchors;
// then K5 adds the per-example sums in example order and divides by N_s.  No float atomics: bit-identical run to run.
// K1 .. K4 and the loss terms live in sample_shared.h: the box head (roi_loss.hip) samples with the same code.
//
// Separated-classifier groups (aabr_rpn_loss_grouped_*): segment e = scene * G + group is an example of the same
// kernels.  Its anchor tables are its scene's, its head values sit group * V_m * A behind the plain index in the
// group-major allocations of the grouped RPN head (LossParams::G, group[], rows[]), its labels and targets are its own,
// and the key hashes the scene: a group's selection, sums and gradients are the plain call's on that group.  The
// finalize adds each group's sums in scene order; the losses and the upstream gradients are [G].
#include "common.h"
#include "sample_shared.h"

namespace aabr {

namespace {

// the sums in example order, / N_s (0 / 0 = NaN for an empty sample, like the reference's mean of nothing): thread g
// adds group g's segments (scene * G + g) in scene order; G = 1 without groups, every example one segment
__global__ __launch_bounds__(64) void k_loss_finalize(int nb, int G, const float *__restrict__ partial,
                                                      int32_t *__restrict__ info, float *__restrict__ obj_loss,
                                                      float *__restrict__ box_loss) {
  const int g = threadIdx.x;
  if (g >= G) return;
  float bce = 0.f, box = 0.f;
  int ns = 0;
  for (int e = g; e < nb * G; e += G) {
    bce += partial[2 * e];
    box += partial[2 * e + 1];
    ns += info[e * kInfoWords] + info[e * kInfoWords + 1];
  }
  obj_loss[g] = bce / (float)ns;
  box_loss[g] = box / (float)ns;
  for (int e = g; e < nb * G; e += G) info[e * kInfoWords + 7] = ns;
}

// the select of every chunk, then (with the loss) the finalize: 1 memset + 4 launches per chunk + 1
int run_select(LossParams &p, const char *fn, int nb, const int32_t *seg_begin_host, const int32_t *site_begin_host,
               const void *const *label_ptrs, const void *const *target_ptrs, void *const *pos_masks,
               void *const *neg_masks, int64_t *selected, int32_t *info, float *obj_loss, float *box_loss,
               int32_t *scratch, hipStream_t st) {
  int rc = run_select_chunks(p, fn, nb, seg_begin_host, site_begin_host, label_ptrs, target_ptrs, pos_masks, neg_masks, selected,
                             info, scratch, st);
  if (rc != AABR_OK) return rc;
  if (p.with_loss) {
    const int G = p.G > 1 ? p.G : 1;
    hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(64), 0, st, nb / G, G, select_partials(scratch, nb), info, obj_loss,
                       box_loss);
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

constexpr int kLossMaxGroups = 16;

struct GradPtrs {
  void *obj[kAnchorMaxMaps];
  void *reg[kAnchorMaxMaps];
};
// gradients at the sampled anchors (the caller has zeroed the gradient buffers)
__global__ __launch_bounds__(256) void k_loss_backward(LossParams p, const int64_t *__restrict__ sel,
                                                       const int32_t *__restrict__ info, const float *__restrict__ g_obj,
                                                       const float *__restrict__ g_box, GradPtrs grads) {
  const int b = blockIdx.y, e = p.example0 + b;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int32_t *inf = info + (int64_t)e * kInfoWords;
  const int kp = inf[0], ns = inf[7];
  if (i >= inf[0] + inf[1] || ns == 0) return;
  const int64_t s_i = sel[(int64_t)e * p.B + i];
  if (s_i < 0) return;
  const int64_t j = s_i - p.out_begin[b];
  const AnchorLoc L = locate(p, b, j);
  const int64_t oi = head_index(p, b, L);
  const float x = ld(p.obj[L.m], oi, p.bf16);
  const float y = i < kp ? 1.f : 0.f;
  const float go = g_obj[p.group[b]] / (float)ns;
  st(grads.obj[L.m], oi, (1.f / (1.f + expf(-x)) - y) * go, p.bf16);
  if (i < kp) {
    const float gb = g_box[p.group[b]] / (float)ns;
    for (int d = 0; d < 7; ++d) {
      const float diff = ld(p.reg[L.m], oi * 7 + d, p.bf16) - p.targets[b][j * 7 + d];
      st(grads.reg[L.m], oi * 7 + d, smooth_l1_grad(diff, p.beta) * gb, p.bf16);
    }
  }
}

// the list form of smooth_l1_loss (layers/smooth_l1_loss.py:34-52, 'Diff'): sum over n elements / divisor, per-block sums
// in a fixed grid, then added in block order
constexpr int kL1Blocks = 512;
__global__ __launch_bounds__(256) void k_smooth_l1_partial(const void *__restrict__ input, const float *__restrict__ target,
                                                           int64_t n, int bf16, float beta, float *__restrict__ partial) {
  __shared__ float s_red[256];
  const int t = threadIdx.x;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + t; i < n; i += (int64_t)gridDim.x * 256)
    acc += smooth_l1_term(fabsf(ld(input, i, bf16) - target[i]), beta);
  s_red[t] = acc;
  for (int w = 128; w > 0; w >>= 1) {
    __syncthreads();
    if (t < w) s_red[t] += s_red[t + w];
  }
  if (t == 0) partial[blockIdx.x] = s_red[0];
}
__global__ __launch_bounds__(64) void k_smooth_l1_finalize(int nblocks, const float *__restrict__ partial, float divisor,
                                                           float *__restrict__ out) {
  if (threadIdx.x != 0) return;
  float s = 0.f;
  for (int i = 0; i < nblocks; ++i) s += partial[i];
  *out = s / divisor;
}
__global__ __launch_bounds__(256) void k_smooth_l1_backward(const void *__restrict__ input, const float *__restrict__ target,
                                                            int64_t n, int bf16, float beta, float divisor,
                                                            const float *__restrict__ g, void *__restrict__ grad) {
  const float gs = *g / divisor;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    st(grad, i, smooth_l1_grad(ld(input, i, bf16) - target[i], beta) * gs, bf16);
}

// the gradient launch of every chunk: 1 per chunk of 16 examples
int run_backward(LossParams &p, const GradPtrs &g, const char *fn, int nb, const int32_t *seg_begin_host,
                 const int32_t *site_begin_host, const void *const *target_ptrs, const int64_t *selected,
                 const int32_t *info, const float *grad_obj_loss, const float *grad_box_loss, hipStream_t st) {
  const int n_maps = p.s.n_maps;
  std::vector<int64_t> out_begin(nb);
  int64_t total = 0;
  for (int b = 0; b < nb; ++b)
    out_begin[b] = select_out_begin(p.G, b, seg_begin_host[b * (n_maps + 1) + n_maps], total);
  for (int b0 = 0; b0 < nb; b0 += kAnchorMaxBatch) {
    const int nbc = nb - b0 < kAnchorMaxBatch ? nb - b0 : kAnchorMaxBatch;
    int64_t nmax = 0;
    int rc = fill_chunk(p, fn, b0, nbc, seg_begin_host, site_begin_host, nullptr, target_ptrs, out_begin.data(), nullptr,
                        nullptr, false, nmax);
    if (rc != AABR_OK) return rc;
    for (int m = 0; m < n_maps; ++m)
      for (int b = 0; b < nbc; ++b)
        AABR_CHECK_ARG_AS(fn, p.s.seg[b][m + 1] == p.s.seg[b][m] || (g.obj[m] && g.reg[m]), "null gradient pointer");
    hipLaunchKernelGGL(k_loss_backward, dim3((unsigned)ceil_div(p.B, 256), (unsigned)nbc), dim3(256), 0, st, p, selected,
                       info, grad_obj_loss, grad_box_loss, g);
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// a scene's rows of the two host tables repeated for its G segments; checks the groups' arguments
int expand_group_tables(const char *fn, int n_maps, int A, int nb, int G, const int32_t *seg_begin_host,
                        const int32_t *site_begin_host, const int64_t *rows_host, LossParams &p, std::vector<int32_t> &seg,
                        std::vector<int32_t> &site) {
  AABR_CHECK_ARG_AS(fn, n_maps >= 1 && n_maps <= kAnchorMaxMaps && nb >= 1, "bad arguments (1 .. 8 maps, >= 1 scene)");
  AABR_CHECK_ARG_AS(fn, G >= 2 && G <= kLossMaxGroups, "groups: 2 <= G <= 16");
  AABR_CHECK_ARG_AS(fn, (int64_t)nb * G < ((int64_t)1 << 24), "too many segments");
  AABR_CHECK_ARG_AS(fn, seg_begin_host && site_begin_host && rows_host, "null pointer");
  p.G = G;
  for (int m = 0; m < n_maps; ++m) {
    AABR_CHECK_ARG_AS(fn, rows_host[m] >= 0, "negative row count");
    p.rows[m] = rows_host[m];
  }
  seg.resize((size_t)nb * G * (n_maps + 1));
  site.resize((size_t)nb * G * n_maps);
  for (int b = 0; b < nb; ++b)
    for (int g = 0; g < G; ++g) {
      const size_t e = (size_t)b * G + g;
      for (int m = 0; m <= n_maps; ++m) seg[e * (n_maps + 1) + m] = seg_begin_host[(size_t)b * (n_maps + 1) + m];
      for (int m = 0; m < n_maps; ++m) {
        site[e * n_maps + m] = site_begin_host[(size_t)b * n_maps + m];
        const int64_t sites = (seg[e * (n_maps + 1) + m + 1] - seg[e * (n_maps + 1) + m]) / (A > 0 ? A : 1);
        AABR_CHECK_ARG_AS(fn, site[e * n_maps + m] >= 0 && site[e * n_maps + m] + sites <= rows_host[m],
                         "a scene's sites reach past the map's rows");
      }
    }
  return AABR_OK;
}

// the fields and per-map pointers the four loss entries share (n_maps has been checked).  A forward entry passes the
// coords and no gradient table; a backward entry the gradient table, no coords, and 0 for the sampler's k_pos0 and seed
void fill_loss_params(LossParams &p, GradPtrs *g, int n_maps, const void *const *coords_ptrs, const void *const *obj_ptrs,
                      const void *const *reg_ptrs, void *const *grad_obj_ptrs, void *const *grad_reg_ptrs, int input_bf16,
                      int num_anchors, int batch_size_per_image, int num_pos_max, uint32_t seed, float beta) {
  p.s.n_maps = n_maps; p.s.A = num_anchors; p.with_loss = 1; p.bf16 = input_bf16 ? 1 : 0; p.B = batch_size_per_image;
  p.k_pos0 = num_pos_max; p.seed = seed; p.beta = beta;
  for (int m = 0; m < n_maps; ++m) {
    p.obj[m] = obj_ptrs[m];
    p.reg[m] = reg_ptrs[m];
    if (coords_ptrs) p.coords[m] = (const int32_t *)coords_ptrs[m];
    if (g) g->obj[m] = grad_obj_ptrs[m], g->reg[m] = grad_reg_ptrs[m];
  }
}

}  // namespace

}  // namespace aabr

using namespace aabr;

extern "C" int64_t aabr_rpn_loss_scratch_words(int nb) {
  return nb > 0 ? (int64_t)nb * (kLossZeroWords + kLossCandWords + 2) : 0;
}

extern "C" int aabr_rpn_loss_forward(int n_maps, const void *const *coords_ptrs, const void *const *obj_ptrs,
                                     const void *const *reg_ptrs, int input_bf16, int num_anchors, int nb,
                                     const int32_t *seg_begin_host, const int32_t *site_begin_host,
                                     const void *const *label_ptrs, const void *const *target_ptrs, uint32_t seed,
                                     int batch_size_per_image, int num_pos_max, float beta, int64_t *selected,
                                     int32_t *info, float *obj_loss, float *box_loss, int32_t *scratch, void *stream_) {
  AABR_CHECK_ARG(n_maps >= 1 && n_maps <= kAnchorMaxMaps && nb >= 1 && num_anchors > 0, "bad arguments (1 .. 8 maps, >= 1 example)");
  AABR_CHECK_ARG(batch_size_per_image >= 1 && batch_size_per_image <= kLossMaxB && num_pos_max >= 0 &&
                     num_pos_max <= batch_size_per_image && beta > 0.f,
                 "need 1 <= batch_size_per_image <= 512, 0 <= num_pos_max <= batch_size_per_image, beta > 0");
  AABR_CHECK_ARG(coords_ptrs && obj_ptrs && reg_ptrs && seg_begin_host && site_begin_host && label_ptrs && target_ptrs &&
                     selected && info && obj_loss && box_loss && scratch, "null pointer");
  LossParams p = {};
  fill_loss_params(p, nullptr, n_maps, coords_ptrs, obj_ptrs, reg_ptrs, nullptr, nullptr, input_bf16, num_anchors,
                   batch_size_per_image, num_pos_max, seed, beta);
  return run_select(p, __func__, nb, seg_begin_host, site_begin_host, label_ptrs, target_ptrs, nullptr, nullptr, selected, info,
                    obj_loss, box_loss, scratch, (hipStream_t)stream_);
}

extern "C" int aabr_rpn_loss_backward(int n_maps, const void *const *obj_ptrs, const void *const *reg_ptrs, int input_bf16,
                                      int num_anchors, int nb, const int32_t *seg_begin_host,
                                      const int32_t *site_begin_host, const void *const *target_ptrs,
                                      int batch_size_per_image, float beta, const int64_t *selected,
                                      const int32_t *info, const float *grad_obj_loss, const float *grad_box_loss,
                                      void *const *grad_obj_ptrs, void *const *grad_reg_ptrs, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  AABR_CHECK_ARG(n_maps >= 1 && n_maps <= kAnchorMaxMaps && nb >= 1 && num_anchors > 0 && batch_size_per_image >= 1 &&
                     batch_size_per_image <= kLossMaxB && beta > 0.f, "bad arguments");
  AABR_CHECK_ARG(obj_ptrs && reg_ptrs && seg_begin_host && site_begin_host && target_ptrs && selected && info &&
                     grad_obj_loss && grad_box_loss && grad_obj_ptrs && grad_reg_ptrs, "null pointer");
  LossParams p = {};
  GradPtrs g = {};
  fill_loss_params(p, &g, n_maps, nullptr, obj_ptrs, reg_ptrs, grad_obj_ptrs, grad_reg_ptrs, input_bf16, num_anchors,
                   batch_size_per_image, 0, 0, beta);
  return run_backward(p, g, __func__, nb, seg_begin_host, site_begin_host, target_ptrs, selected, info, grad_obj_loss,
                      grad_box_loss, st);
}

extern "C" int64_t aabr_rpn_loss_grouped_scratch_words(int nb, int G) {
  return nb > 0 && G >= 2 && G <= kLossMaxGroups ? aabr_rpn_loss_scratch_words(nb * G) : 0;
}

extern "C" int aabr_rpn_loss_grouped_forward(int n_maps, const void *const *coords_ptrs, const void *const *obj_ptrs,
                                             const void *const *reg_ptrs, const int64_t *rows_host, int input_bf16,
                                             int num_anchors, int nb, int G, const int32_t *seg_begin_host,
                                             const int32_t *site_begin_host, const void *const *label_ptrs,
                                             const void *const *target_ptrs, uint32_t seed, int batch_size_per_image,
                                             int num_pos_max, float beta, int64_t *selected, int32_t *info,
                                             float *obj_loss, float *box_loss, int32_t *scratch, void *stream_) {
  AABR_CHECK_ARG(num_anchors > 0, "bad arguments (at least one anchor per site)");
  AABR_CHECK_ARG(batch_size_per_image >= 1 && batch_size_per_image <= kLossMaxB && num_pos_max >= 0 &&
                     num_pos_max <= batch_size_per_image && beta > 0.f,
                 "need 1 <= batch_size_per_image <= 512, 0 <= num_pos_max <= batch_size_per_image, beta > 0");
  AABR_CHECK_ARG(coords_ptrs && obj_ptrs && reg_ptrs && label_ptrs && target_ptrs && selected && info && obj_loss &&
                     box_loss && scratch, "null pointer");
  LossParams p = {};
  std::vector<int32_t> seg, site;
  const int rc = expand_group_tables(__func__, n_maps, num_anchors, nb, G, seg_begin_host, site_begin_host, rows_host, p, seg,
                                     site);
  if (rc != AABR_OK) return rc;
  fill_loss_params(p, nullptr, n_maps, coords_ptrs, obj_ptrs, reg_ptrs, nullptr, nullptr, input_bf16, num_anchors,
                   batch_size_per_image, num_pos_max, seed, beta);
  return run_select(p, __func__, nb * G, seg.data(), site.data(), label_ptrs, target_ptrs, nullptr, nullptr, selected, info,
                    obj_loss, box_loss, scratch, (hipStream_t)stream_);
}

extern "C" int aabr_rpn_loss_grouped_backward(int n_maps, const void *const *obj_ptrs, const void *const *reg_ptrs,
                                              const int64_t *rows_host, int input_bf16, int num_anchors, int nb, int G,
                                              const int32_t *seg_begin_host, const int32_t *site_begin_host,
                                              const void *const *target_ptrs, int batch_size_per_image, float beta,
                                              const int64_t *selected, const int32_t *info, const float *grad_obj_loss,
                                              const float *grad_box_loss, void *const *grad_obj_ptrs,
                                              void *const *grad_reg_ptrs, void *stream_) {
  AABR_CHECK_ARG(num_anchors > 0 && batch_size_per_image >= 1 && batch_size_per_image <= kLossMaxB && beta > 0.f,
                 "bad arguments");
  AABR_CHECK_ARG(obj_ptrs && reg_ptrs && target_ptrs && selected && info && grad_obj_loss && grad_box_loss &&
                     grad_obj_ptrs && grad_reg_ptrs, "null pointer");
  LossParams p = {};
  GradPtrs g = {};
  std::vector<int32_t> seg, site;
  const int rc = expand_group_tables(__func__, n_maps, num_anchors, nb, G, seg_begin_host, site_begin_host, rows_host, p, seg,
                                     site);
  if (rc != AABR_OK) return rc;
  fill_loss_params(p, &g, n_maps, nullptr, obj_ptrs, reg_ptrs, grad_obj_ptrs, grad_reg_ptrs, input_bf16, num_anchors,
                   batch_size_per_image, 0, 0, beta);
  return run_backward(p, g, __func__, nb * G, seg.data(), site.data(), target_ptrs, selected, info, grad_obj_loss,
                      grad_box_loss, (hipStream_t)stream_);
}

extern "C" int aabr_sample_list(int nb, const void *const *label_ptrs, const int64_t *n_host, uint32_t seed,
                                int batch_size_per_image, int num_pos_max, int64_t *selected, int32_t *info,
                                void *const *pos_masks, void *const *neg_masks, int32_t *scratch, void *stream_) {
  AABR_CHECK_ARG(nb >= 1 && batch_size_per_image >= 1 && batch_size_per_image <= kLossMaxB && num_pos_max >= 0 &&
                     num_pos_max <= batch_size_per_image, "need nb >= 1, 1 <= batch_size_per_image <= 512, "
                                                          "0 <= num_pos_max <= batch_size_per_image");
  AABR_CHECK_ARG(label_ptrs && n_host && selected && info && scratch, "null pointer");
  std::vector<int32_t> seg(2 * (size_t)nb);
  for (int b = 0; b < nb; ++b) {
    AABR_CHECK_ARG(n_host[b] >= 0 && n_host[b] < ((int64_t)1 << 31), "list length out of range");
    seg[2 * b] = 0;
    seg[2 * b + 1] = (int32_t)n_host[b];
  }
  LossParams p = {};
  p.s.n_maps = 1; p.s.A = 1; p.flat = 1; p.with_loss = 0; p.label_mode = 1; p.k_pos0 = num_pos_max;
  p.B = batch_size_per_image; p.seed = seed; p.beta = 1.f;
  return run_select(p, __func__, nb, seg.data(), nullptr, label_ptrs, nullptr, pos_masks, neg_masks, selected, info, nullptr, nullptr,
                    scratch, (hipStream_t)stream_);
}

extern "C" int64_t aabr_smooth_l1_scratch_floats(void) { return kL1Blocks; }

extern "C" int aabr_smooth_l1_forward(const void *input, const float *target, int64_t n, int input_bf16, float beta,
                                      float divisor, float *out, float *scratch, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  AABR_CHECK_ARG(n >= 0 && beta > 0.f && out && scratch && (n == 0 || (input && target)), "bad arguments");
  int64_t nblk = ceil_div(n, 256 * 4);
  nblk = nblk < 1 ? 1 : (nblk > kL1Blocks ? kL1Blocks : nblk);
  hipLaunchKernelGGL(k_smooth_l1_partial, dim3((unsigned)nblk), dim3(256), 0, st, input, target, n, input_bf16 ? 1 : 0, beta,
                     scratch);
  hipLaunchKernelGGL(k_smooth_l1_finalize, dim3(1), dim3(64), 0, st, (int)nblk, scratch, divisor, out);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_smooth_l1_backward(const void *input, const float *target, int64_t n, int input_bf16, float beta,
                                       float divisor, const float *grad_out, void *grad_input, void *stream_) {
  AABR_CHECK_ARG(n >= 0 && beta > 0.f && grad_out && (n == 0 || (input && target && grad_input)), "bad arguments");
  if (n == 0) return AABR_OK;
  int64_t nblk = ceil_div(n, 256 * 4);
  nblk = nblk < 1 ? 1 : (nblk > 1024 ? 1024 : nblk);
  hipLaunchKernelGGL(k_smooth_l1_backward, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream_, input, target, n,
                     input_bf16 ? 1 : 0, beta, divisor, grad_out, grad_input);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

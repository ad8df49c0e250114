// solver.hip -- the optimizer step on the device: SGD with momentum and weight decay (torch.optim.SGD, dampening 0, no
// Nesterov form: the reference's optimizer, maskrcnn_benchmark/solver/build.py:7-20) over ALL parameters in ONE launch.
// The parameters live in one flat fp32 buffer (dp.FlatParams.flat) with a momentum buffer of the same layout; the kernel
// grid-strides over a device-resident chunk table (solver_segs.h) that is built once per optimizer, and takes what
// changes from step to step -- the per-group lr and weight decay, the momentum, the gradient scale -- BY VALUE in its
// arguments, so a new learning rate costs no device write and no copy.
//
// Per element, fp32, in this order (the Makefile's -ffp-contract=off: no operation is fused with another):
//   g  = widen(grad)                    ; g = g * grad_scale   only when grad_scale != 1
//   d  = g + wd * p                     only when wd != 0      (else d = g: an infinite p stays infinite, not NaN)
//   m' = mu * m + d                     only when mu != 0      (else no buffer is read or written, the step uses d)
//   p' = p - lr * m'
// p, m and g are each read once, p and m written once; no atomics, no LDS.  The momentum buffer starts as zeros:
// mu * 0 + d has the value of torch's first-step clone(d) (only the sign of a zero can differ).
#include "common.h"
#include "solver_segs.h"

namespace aabr {

struct SgdHyper {
  float lr[kSgdMaxGroups], wd[kSgdMaxGroups];
  float mu, grad_scale;
  int32_t n_groups;
};

__device__ __forceinline__ float sgd_widen(float v) { return v; }
// bf16 -> fp32 is exact: the 16 bits become the high half of the word
__device__ __forceinline__ float sgd_widen(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

template <bool kMu>
__device__ __forceinline__ void sgd_elem(float &p, float &m, float g, float lr, float wd, float mu, float gs) {
  if (gs != 1.0f) g = g * gs;
  float d = g;
  if (wd != 0.0f) d = g + wd * p;
  if (kMu) {
    m = mu * m + d;
    d = m;
  }
  p = p - lr * d;
}

template <typename G> struct SgdVec;
template <> struct SgdVec<float> { typedef float4 type; };
template <> struct SgdVec<uint16_t> { typedef ushort4 type; };

// GradT: float, or uint16_t holding bf16 bits.  kMu: momentum != 0.
// One workgroup of 256 threads per chunk, grid-striding.  A record that does not lie inside [0, n) or names a group or
// segment that does not exist is skipped, so a damaged table cannot make the kernel write outside the two buffers.
template <typename GradT, bool kMu>
__global__ void __launch_bounds__(256) k_sgd_momentum(float *__restrict__ p, float *__restrict__ m, int64_t n,
                                                       const int64_t *__restrict__ table, int64_t n_chunks,
                                                       const GradT *__restrict__ gflat,
                                                       const uint64_t *__restrict__ gptrs, int64_t n_segs, SgdHyper hy) {
  typedef typename SgdVec<GradT>::type GVec;
  const int tid = threadIdx.x;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t off = table[kSgdChunkWords * c], seg_first = table[kSgdChunkWords * c + 1];
    const int64_t len = table[kSgdChunkWords * c + 2], sg = table[kSgdChunkWords * c + 3];
    if (off < 0 || len < 1 || len > kSgdChunkElems || off > n - len || seg_first < 0 || seg_first > off || sg < 0) continue;
    const int64_t seg = sg / kSgdMaxGroups;
    const int grp = (int)(sg % kSgdMaxGroups);
    if (grp >= hy.n_groups) continue;
    const GradT *g;
    if (gptrs) {
      if (seg >= n_segs) continue;
      const uint64_t a = gptrs[seg];
      if (a == 0) continue;              // no gradient for this parameter: p and m stay bit for bit
      g = reinterpret_cast<const GradT *>(a) + (off - seg_first);
    } else {
      g = gflat + off;
    }
    float lr = hy.lr[0], wd = hy.wd[0];
#pragma unroll
    for (int q = 1; q < kSgdMaxGroups; ++q) {
      lr = grp == q ? hy.lr[q] : lr;
      wd = grp == q ? hy.wd[q] : wd;
    }
    const float mu = hy.mu, gs = hy.grad_scale;
    const int n_el = (int)len;
    int head = (int)((-off) & 3);        // elements before the first multiple of 4 of the flat offset
    if (head > n_el) head = n_el;
    const int nvec = (n_el - head) >> 2, tail = n_el - head - 4 * nvec;
    float *pc = p + off, *mc = m + off;
    // scalar head and tail: at most 3 elements each, at a segment's two ends
    if (tid < head || (tid >= 64 && tid - 64 < tail)) {
      const int i = tid < head ? tid : head + 4 * nvec + (tid - 64);
      float pv = pc[i], mv = kMu ? mc[i] : 0.0f;
      sgd_elem<kMu>(pv, mv, sgd_widen(g[i]), lr, wd, mu, gs);
      if (kMu) mc[i] = mv;
      pc[i] = pv;
    }
    // 16-byte body; the gradient is loaded 4 elements at a time only when its address has the matching phase
    const bool gvec = (reinterpret_cast<uintptr_t>(g + head) & (sizeof(GVec) - 1)) == 0;
    for (int v = tid; v < nvec; v += 256) {
      const int i = head + 4 * v;
      const f32x4 p4 = *reinterpret_cast<const f32x4 *>(pc + i);
      f32x4 m4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if (kMu) m4 = *reinterpret_cast<const f32x4 *>(mc + i);
      float gq[4];
      if (gvec) {
        const GVec gv = *reinterpret_cast<const GVec *>(g + i);
        gq[0] = sgd_widen(gv.x); gq[1] = sgd_widen(gv.y); gq[2] = sgd_widen(gv.z); gq[3] = sgd_widen(gv.w);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) gq[q] = sgd_widen(g[i + q]);
      }
      float pq[4] = {p4.x, p4.y, p4.z, p4.w}, mq[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) sgd_elem<kMu>(pq[q], mq[q], gq[q], lr, wd, mu, gs);
      const f32x4 mo = {mq[0], mq[1], mq[2], mq[3]}, po = {pq[0], pq[1], pq[2], pq[3]};
      if (kMu) *reinterpret_cast<f32x4 *>(mc + i) = mo;
      *reinterpret_cast<f32x4 *>(pc + i) = po;
    }
  }
}

template <typename GradT>
static void launch_sgd(float *p, float *m, int64_t n, const int64_t *table, int64_t n_chunks, const void *gflat,
                       const uint64_t *gptrs, int64_t n_segs, const SgdHyper &hy, hipStream_t st) {
  const unsigned grid = (unsigned)(n_chunks < 2048 ? n_chunks : 2048);
  if (hy.mu != 0.0f)
    hipLaunchKernelGGL((k_sgd_momentum<GradT, true>), dim3(grid), dim3(256), 0, st, p, m, n, table, n_chunks,
                       (const GradT *)gflat, gptrs, n_segs, hy);
  else
    hipLaunchKernelGGL((k_sgd_momentum<GradT, false>), dim3(grid), dim3(256), 0, st, p, m, n, table, n_chunks,
                       (const GradT *)gflat, gptrs, n_segs, hy);
}

} // namespace aabr

extern "C" int aabr_sgd_chunk_elems(void) { return aabr::kSgdChunkElems; }

extern "C" int64_t aabr_sgd_chunk_table(const int64_t *seg_off, const int64_t *seg_numel, const int32_t *seg_group,
                                        int64_t n_segs, int64_t n, int64_t *table_host, int64_t cap_chunks) {
  static_assert(sizeof(aabr::SgdChunk) == 4 * sizeof(int64_t), "the table is int64[chunks][4]");
  const char *why = "";
  const int64_t r = aabr::sgd_cut_segments(seg_off, seg_numel, seg_group, n_segs, n,
                                           reinterpret_cast<aabr::SgdChunk *>(table_host), cap_chunks, &why);
  if (r < 0) aabr::set_error("%s: %s", __func__, why);
  return r;
}

extern "C" int aabr_sgd_momentum_step(float *flat, float *momentum_buf, int64_t n, const int64_t *chunk_table,
                                      const int64_t *chunk_table_host, int64_t n_chunks, int64_t n_segs,
                                      const void *grad_flat, const void *grad_ptr_table, int grad_is_bf16,
                                      const float *lr, const float *wd, int n_groups, float momentum, float grad_scale,
                                      void *stream) {
  using namespace aabr;
  AABR_CHECK_ARG(n_chunks <= 0 || chunk_table_host, "null host copy of the chunk table");
  const SgdChunk *last =
      n_chunks > 0 ? reinterpret_cast<const SgdChunk *>(chunk_table_host) + (n_chunks - 1) : nullptr;
  const char *why = sgd_step_refusal(flat, momentum_buf, n, chunk_table, last, n_chunks, n_segs, grad_flat,
                                     grad_ptr_table, grad_is_bf16, lr, wd, n_groups, momentum);
  AABR_CHECK_ARG(why == nullptr, why);
  if (n_chunks == 0) return AABR_OK;
  SgdHyper hy;
  for (int q = 0; q < kSgdMaxGroups; ++q) {
    hy.lr[q] = q < n_groups ? lr[q] : 0.0f;
    hy.wd[q] = q < n_groups ? wd[q] : 0.0f;
  }
  hy.mu = momentum;
  hy.grad_scale = grad_scale;
  hy.n_groups = n_groups;
  hipStream_t st = (hipStream_t)stream;
  const uint64_t *gptrs = reinterpret_cast<const uint64_t *>(grad_ptr_table);
  if (grad_is_bf16)
    launch_sgd<uint16_t>(flat, momentum_buf, n, chunk_table, n_chunks, grad_flat, gptrs, n_segs, hy, st);
  else
    launch_sgd<float>(flat, momentum_buf, n, chunk_table, n_chunks, grad_flat, gptrs, n_segs, hy, st);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

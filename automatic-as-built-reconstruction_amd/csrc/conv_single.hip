// conv_single.hip -- the forward-form sparse convolution for rule books in which EVERY OUTPUT ROW HAS EXACTLY ONE RULE
// (gfx950, fp32 storage): out[o] = W[k(o)] . in[i(o)] (+ bias, + residual).  The FPN's top-down path is made of them: the
// Deconvolution with filter == stride and the 1x1x1 SubmanifoldConvolution, forward and input gradient.
//
// Nothing is summed over filter offsets, so nothing of k_conv_cs' output-tile machinery (conv_wide.hip) is needed: no
// fp32 tile in LDS, no read-add-write per 16-pair block, no weight reload per (tile, offset).  Instead the work item is
// (filter offset k, chunk of that offset's pair list, 64-column slab), read from the offset-major pair list the weight
// gradient already builds (offset_pairs.h), with its chunk-to-workgroup scheme: a bounded grid, no host read of counts.
//
//   k_conv_single<KG> -- a workgroup (4 waves) takes one chunk of 256 or 1024 pairs of ONE offset; wave w owns the 16
//   output columns w of the slab and loads W[k]'s slice for them ONCE into registers (KG x 8 VGPRs x 2).  Per step the
//   workgroup gathers 32 partner rows through a double-buffered, granule-swizzled LDS stage (the gather / stage / operand
//   code of k_conv_cs: each wave a quarter of the rows, 16-byte loads, rows of step s + 2 requested while step s is
//   multiplied), every wave chains v_mfma_f32_16x16x4_f32 from zero accumulators over the staged rows in the K order of
//   k_conv_cs, and writes its 16 x 16 result straight from registers to the rows the pairs name, adding bias and residual
//   on the way.  One barrier per step (the stage hand-over).  Only the last step of a chunk is padded: padding entries
//   gather from beyond the buffer descriptor's range (zeros, no memory access) and store nothing.
//
// One chain per output element from a zero accumulator, then + bias, then + residual: bit for bit what k_conv_cs writes
// for such a book (its tile's 0 + x is exact).  Every output row is written by exactly one lane group: no atomics.
// THE CALLER GUARANTEES the one-rule property; a row named by two pairs would hold whichever was written last, a row
// named by none is not written.
//
//   k_conv_single<KG, true> -- the input-gradient launch of a convolution with filter == stride (every fine row has one
//   parent), whose output is the d_out of the BatchNorm(+leaky ReLU) in front of that convolution: the write-out also
//   forms that BatchNorm's BACKWARD statistics, with exactly the terms of k_conv_cs' write-out (conv_wide.hip, `bn.x`):
//   d = the stored value masked by the sign of the activation recomputed from the BatchNorm's input x, fp64 sums of d and
//   (x - mean) * d.  The x rows are requested with the residual rows, ahead of the gathers; a lane keeps the eight sums of
//   its four columns in registers over the chunk's steps (padding pairs add nothing), and after the last step the
//   workgroup combines them through LDS (the stage is free by then) in lane order into ONE part [2][64 columns] per
//   (chunk, slab): stats[(chunk * 2 + s) * n_out + column].  A workgroup without pairs writes zeros, so the BatchNorm
//   backward sums all gridDim.x parts in part order (aabr_bn_backward_parts) and the result does not depend on which
//   workgroup ran when: no atomics.  `out` is what k_conv_single<KG> writes, bit for bit.
#include "common.h"
#include "conv_single_tiles.h"
#include "offset_pairs.h"

namespace aabr {


extern thread_local const char *g_last_variant; // conv.hip

__device__ inline float bcs_(unsigned int v) { return __builtin_bit_cast(float, v); }

// BS instances: the BatchNorm whose backward statistics the write-out forms (x its input, the saved statistics, its affine
// coefficients or nullptr) and the parts buffer [gridDim.x][2][co]; all nullptr for the plain instances
struct SingleBwdStats {
  double *stats;
  const float *x, *mean, *invstd, *weight, *bias;
  float leak;
};

template <int KG, bool BS = false>
__global__ __launch_bounds__(256, (BS && KG == 4) ? 3 : 2) void k_conv_single(const float *__restrict__ in, int ci, int64_t in_bytes,
                                                        float *__restrict__ out, int co, int64_t V_out,
                                                        const int32_t *__restrict__ words, int vol, int chunk_pairs,
                                                        int wflip, const float *__restrict__ Wp, int64_t wp_bytes,
                                                        const float *__restrict__ bias, const float *__restrict__ res,
                                                        SingleBwdStats bn) {
  constexpr int NW = 4;                    // waves per workgroup
  constexpr int LPR = 8;                   // lanes per gathered pair row: 256 threads, 32 rows
  constexpr int RF = KG * 32;              // floats per staged row
  constexpr int RG = KG * 8;               // 16-byte granules per staged row
  constexpr int SWZ = (RG >= 16 && (RG & 15) == 0) ? 15 : 7; // XOR must stay inside the row's granules
  constexpr int STAGE = 2 * 16 * RF;       // floats per stage buffer (two blocks)
  constexpr int NGL = KG;                  // 16-byte gather loads per lane and step
  extern __shared__ __align__(16) float St[];   // [2][32][RF]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int g = lane >> 4, c16 = lane & 15;
  const int pr = wave * (64 / LPR) + lane / LPR, seg = lane % LPR;   // gather role: pair row 0..31, 16-byte segment
  const int nnb = co >> 4;
  // every XCD a contiguous range of (chunk, slab) items, as in k_conv_cs: the slabs of a chunk gather the same rows
  int chunk, nb0;
  {
    const unsigned ny = gridDim.y, total = gridDim.x * ny;
    const unsigned lin = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned per = total >> 3, rem = total & 7u, x = lin & 7u;
    const unsigned wi = x * per + (x < rem ? x : rem) + (lin >> 3);
    chunk = (int)(wi / ny);
    nb0 = (int)(wi % ny) * NW;
  }
  int k, p0, p1;
  bool work = dw_chunk_range(words, vol, chunk_pairs, 0, chunk, lane, k, p0, p1);    // false: surplus workgroup
  work = work && p0 < p1;                                                            // (workgroup-uniform)
  if (!work) {
    if (BS && threadIdx.x < 128)           // its part of the statistics: zeros
      bn.stats[((int64_t)chunk * 2 + (threadIdx.x >> 6)) * co + nb0 * 16 + (threadIdx.x & 63)] = 0.0;
    return;
  }
  const int last = words[k] - 1;           // >= p0: clamps the entry loads of the padded tail and of the steps past the end
  // the offset's (partner row, row) pairs, read word by word (the list is 4-byte aligned)
  const int32_t *__restrict__ pairs = words + op_hdr(vol) + (int64_t)vol * op_nb256(V_out) + 2 * (int64_t)k * V_out;
  const __amdgpu_buffer_rsrc_t rin =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(in), 0, (int)in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Wp), 0, (int)wp_bytes, 0x00020000);
  const unsigned rowbytes = (unsigned)ci * 4u;

  struct GReg { u32x4 v[NGL]; };
  struct Ent { int tg, oa, ob; };          // as loaded: partner row of pair row `pr` (gather role), output rows of this
                                           // lane's pair in block A and block B (compute role)
  // Entries of step s (pairs p0 + 32 s ...): unconditional loads from clamped indices.  They are masked where they are
  // USED (pad_g / pad_c), steps later: a select on a value just loaded would make the wave wait for it -- and, loads
  // returning in order, for the gathers issued before it.
  auto load_ent = [&](int s) {
    const int q = p0 + s * kSingleStepPairs;
    const int qg = q + pr, qa = q + c16, qb = q + 16 + c16;
    Ent e;
    e.tg = pairs[2 * (int64_t)(qg < last ? qg : last)];
    e.oa = pairs[2 * (int64_t)(qa < last ? qa : last) + 1];
    e.ob = pairs[2 * (int64_t)(qb < last ? qb : last) + 1];
    return e;
  };
  auto pad_g = [&](int s) { return p0 + s * kSingleStepPairs + pr >= p1; };          // gather role: a padding row
  auto pad_c = [&](int s, int b) { return p0 + s * kSingleStepPairs + b * 16 + c16 >= p1; };   // compute role, block b
  auto gather = [&](GReg &q, int tg, bool pad) {
    // a padding row's address lies beyond the descriptor's range (in_bytes < 2^31): the loads return zeros
    const unsigned va = (pad ? 0x80000000u : (unsigned)tg * rowbytes) + (unsigned)seg * 16u;
#pragma unroll
    for (int i = 0; i < NGL; ++i) q.v[i] = __builtin_amdgcn_raw_buffer_load_b128(rin, va, (unsigned)i * (unsigned)(LPR * 16), 0);
  };
  auto stage_store = [&](const GReg &q, int buf) {
    float *rowp = St + buf * STAGE + pr * RF;
#pragma unroll
    for (int i = 0; i < NGL; ++i)
      *reinterpret_cast<u32x4 *>(rowp + (((seg + LPR * i) ^ (pr & SWZ)) << 2)) = q.v[i];
  };
  auto wg_barrier = [&]() {                // LDS traffic of this wave retired, then the workgroup barrier; unlike
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // __syncthreads() it does not drain the prefetches
  };
  const int colo = (nb0 + wave) * 16 + g * 4;        // this lane's four output columns
  f32x4 bv = {0.f, 0.f, 0.f, 0.f};
  if (bias) bv = *reinterpret_cast<const f32x4 *>(bias + colo);
  // BS: the BatchNorm's forward coefficients of this lane's four columns (k_conv_cs' write-out forms them the same way) and
  // the lane's sums over the chunk
  float bmu[4] = {0.f, 0.f, 0.f, 0.f}, bwc[4] = {0.f, 0.f, 0.f, 0.f}, bbc[4] = {0.f, 0.f, 0.f, 0.f};
  double sd[4] = {0.0, 0.0, 0.0, 0.0}, sxd[4] = {0.0, 0.0, 0.0, 0.0};   // sums of d, of (x - mean) * d
  if (BS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bmu[j] = bn.mean[colo + j];
      bwc[j] = bn.invstd[colo + j] * (bn.weight ? bn.weight[colo + j] : 1.0f);
      bbc[j] = -bmu[j] * bwc[j] + (bn.bias ? bn.bias[colo + j] : 0.0f);
    }
  }

  const int nsteps = (p1 - p0 + kSingleStepPairs - 1) / kSingleStepPairs;
  // Software pipeline over the chunk's steps: entries three steps ahead (registers), gathered rows two steps ahead
  // (registers -> the other stage buffer after this step's MFMAs).  Past the chunk's end the loads repeat clamped
  // entries as padding: they gather nothing and their results are dropped.
  // The first three steps' entries go out FIRST and stay first (sched_barrier): every later wait for one of them is then
  // a counted one on the way into the loop as it is around it -- the loop header takes the stricter of the two.
  Ent ea = load_ent(0), eb = load_ent(1), ec = load_ent(2), ed;
  __builtin_amdgcn_sched_barrier(0);
  // the offset's weight slice of this wave's 16 columns, in the pack's order (k_conv_cs load_w)
  u32x4 w0[KG], w1[KG];
  {
    const int kW = (wflip & 1) ? vol - 1 - k : k;
#pragma unroll
    for (int c = 0; c < KG; ++c) {
      const unsigned so = (unsigned)((((int64_t)kW * KG + c) * nnb + nb0 + wave) * 2048);
      w0[c] = __builtin_amdgcn_raw_buffer_load_b128(rw, (unsigned)lane * 32u, so, 0);
      w1[c] = __builtin_amdgcn_raw_buffer_load_b128(rw, (unsigned)lane * 32u + 16u, so, 0);
    }
  }
  __builtin_amdgcn_sched_barrier(0);       // ... and the weights ahead of the gathers: the wait for the first rows covers them
  GReg gq0, gq1;
  gather(gq0, ea.tg, pad_g(0));
  gather(gq1, eb.tg, pad_g(1));
  stage_store(gq0, 0);
  wg_barrier();
  int par = 0, s = 0;
  // one step: rows of step s are in stage[par], its entries in e0; g_store holds the rows of step s + 1, g_issue takes
  // those of step s + 2 (entries e2), e3 takes the entries of step s + 3
  auto step = [&](const Ent &e0, const Ent &e2, Ent &e3, GReg &g_issue, GReg &g_store) __attribute__((always_inline)) {
    // the residual rows of this step first: the write-out's wait for them must not cover the gathers issued below
    f32x4 ra = {0.f, 0.f, 0.f, 0.f}, rb = ra;
    const bool pa = pad_c(s, 0), pb = pad_c(s, 1);
    const int64_t ia = (int64_t)(pa ? 0 : e0.oa) * co + colo, ib = (int64_t)(pb ? 0 : e0.ob) * co + colo;
    if (res) {                             // (kernel-uniform)
      ra = *reinterpret_cast<const f32x4 *>(res + ia);
      rb = *reinterpret_cast<const f32x4 *>(res + ib);
    }
    f32x4 xa = {0.f, 0.f, 0.f, 0.f}, xb = xa;   // BS: the BatchNorm's input at the same (row, columns), requested with them
    if (BS) {
      xa = *reinterpret_cast<const f32x4 *>(bn.x + ia);
      xb = *reinterpret_cast<const f32x4 *>(bn.x + ib);
    }
    // entries before the gather: loads return in order, and the next step's wait for these entries (its gather's
    // addresses) must not cover the rows requested here
    e3 = load_ent(s + 3);
    gather(g_issue, e2.tg, pad_g(s + 2));
    __builtin_amdgcn_sched_barrier(0);     // the prefetches are issued HERE, ahead of the MFMAs
    const float *sa = St + par * STAGE + c16 * RF;
    const float *sb = sa + 16 * RF;
    f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = accA;
    {
      u32x4 a0[KG], a1[KG], b0[KG], b1[KG];
#pragma unroll
      for (int c = 0; c < KG; ++c) {       // the lane's 8 consecutive channels of a 32-channel chunk = granules 2g, 2g+1
        const int q0 = ((c * 8 + g * 2) ^ (c16 & SWZ)) << 2, q1 = ((c * 8 + g * 2 + 1) ^ (c16 & SWZ)) << 2;
        a0[c] = *reinterpret_cast<const u32x4 *>(sa + q0);
        b0[c] = *reinterpret_cast<const u32x4 *>(sb + q0);
        a1[c] = *reinterpret_cast<const u32x4 *>(sa + q1);
        b1[c] = *reinterpret_cast<const u32x4 *>(sb + q1);
      }
#pragma unroll
      for (int c = 0; c < KG; ++c) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          accA = __builtin_amdgcn_mfma_f32_16x16x4f32(bcs_(w0[c][t]), bcs_(a0[c][t]), accA, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          accA = __builtin_amdgcn_mfma_f32_16x16x4f32(bcs_(w1[c][t]), bcs_(a1[c][t]), accA, 0, 0, 0);
      }
      if (p0 + s * kSingleStepPairs + 16 < p1) {                      // wave-uniform, covers nothing but MFMAs: only a chunk's last step lacks block B
#pragma unroll
        for (int c = 0; c < KG; ++c) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            accB = __builtin_amdgcn_mfma_f32_16x16x4f32(bcs_(w0[c][t]), bcs_(b0[c][t]), accB, 0, 0, 0);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            accB = __builtin_amdgcn_mfma_f32_16x16x4f32(bcs_(w1[c][t]), bcs_(b1[c][t]), accB, 0, 0, 0);
        }
      }
    }
    // lane (g, c16) holds out[row of pair c16][colo .. colo + 3]: the order of k_conv_cs' write-out (+ bias, + residual)
    if (bias) { accA += bv; accB += bv; }
    if (res) { accA += ra; accB += rb; }
    if (!pa) *reinterpret_cast<f32x4 *>(out + ia) = accA;
    if (!pb) *reinterpret_cast<f32x4 *>(out + ib) = accB;
    if (BS) {                              // the terms of k_conv_cs' write-out, from the values just stored
      auto add = [&](const f32x4 &v, const f32x4 &xv) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float o = xv[j] * bwc[j] + bbc[j];
          const float d = (o > 0.0f) ? v[j] : v[j] * bn.leak;
          sd[j] += (double)d;
          sxd[j] += (double)(xv[j] - bmu[j]) * (double)d;
        }
      };
      if (!pa) add(accA, xa);
      if (!pb) add(accB, xb);
    }
    stage_store(g_store, par ^ 1);         // the next step's rows, gathered a step ago
    wg_barrier();
    par ^= 1;
    ++s;
  };
  // The two register sets of gathered rows and the four of entries rotate statically: four copies of the step body, no
  // register moves (a move of a value just loaded would wait for it, and so for the gathers in flight).
  // The loop body is four whole steps and nothing leaves it half way: an exit between the copies would share the
  // loop's latch, and the header's waits would be counted along that path (two loads behind an entry = a full drain).
  while (s + 4 <= nsteps) {
    step(ea, ec, ed, gq0, gq1);
    step(eb, ed, ea, gq1, gq0);
    step(ec, ea, eb, gq0, gq1);
    step(ed, eb, ec, gq1, gq0);
  }
  if (s < nsteps) {                        // the last one to three steps
    step(ea, ec, ed, gq0, gq1);
    if (s < nsteps) {
      step(eb, ed, ea, gq1, gq0);
      if (s < nsteps) step(ec, ea, eb, gq0, gq1);
    }
  }
  if (BS) {
    // The last step's barrier is behind every wave: nobody reads the stage any more, and it holds the sums now, [8][256]
    // doubles.  Column c of the slab belongs to wave c / 16, lane group (c / 4) % 4, register c % 4; its 16 lanes hold
    // the chunk's rows: added in lane order by one thread per column and sum.
    double *red = reinterpret_cast<double *>(St);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      red[j * 256 + threadIdx.x] = sd[j];
      red[(4 + j) * 256 + threadIdx.x] = sxd[j];
    }
    __syncthreads();
    if (threadIdx.x < 128) {
      const int which = threadIdx.x >> 6, c = threadIdx.x & 63;
      const double *col = red + (which * 4 + (c & 3)) * 256 + (c >> 4) * 64 + ((c >> 2) & 3) * 16;
      double a = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) a += col[r];
      bn.stats[((int64_t)chunk * 2 + which) * co + nb0 * 16 + c] = a;
    }
  }
}

} // namespace aabr
using namespace aabr;

static SingleKnobs single_knobs() { return {knob(K_CONV_SINGLE), knob(K_SINGLE_ROWS), knob(K_SINGLE_CHUNK)}; }

// ---- the dispatch query: conv_single_tiles.h decides, with the knobs as they stand ------------------------------------
// pairs per chunk (256; 1024 on request) when a one-rule-per-row launch of this shape should go to aabr_conv_forward_single, else 0
extern "C" int aabr_conv_single_chunk(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, int bf16, int has_stats) {
  const SingleKnobs kn = single_knobs();
  if (single_refusal(bf16 != 0, has_stats != 0, n_in, n_out, rows_in, V_out, vol, kn)) return 0;
  return single_chunk_pairs(kn);
}
// why the query above returned 0 ("" when it did not)
extern "C" const char *aabr_conv_single_refusal(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, int bf16,
                                                int has_stats) {
  const char *m = single_refusal(bf16 != 0, has_stats != 0, n_in, n_out, rows_in, V_out, vol, single_knobs());
  return m ? m : "";
}

// the same for the input-gradient launch that owes a BatchNorm its backward statistics (aabr_conv_forward_single_bwd_stats)
extern "C" int aabr_conv_single_bwd_stats_chunk(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol, int bf16) {
  const SingleKnobs kn = single_knobs();
  if (single_bwd_stats_refusal(bf16 != 0, n_in, n_out, rows_in, V_out, vol, kn, knob(K_SINGLE_BWD_STATS))) return 0;
  return single_chunk_pairs(kn);
}
extern "C" const char *aabr_conv_single_bwd_stats_refusal(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol,
                                                          int bf16) {
  const char *m = single_bwd_stats_refusal(bf16 != 0, n_in, n_out, rows_in, V_out, vol, single_knobs(),
                                           knob(K_SINGLE_BWD_STATS));
  return m ? m : "";
}
// parts [2][n_out] of fp64 sums that launch writes, for the chunk length the query above returned
extern "C" int64_t aabr_conv_single_bwd_stats_parts(int64_t V_out, int vol, int chunk_pairs) {
  if (V_out <= 0 || vol <= 0 || (chunk_pairs != 256 && chunk_pairs != 1024)) return 0;
  return single_chunk_bound(V_out, vol, chunk_pairs);
}

// ---- the launch ---------------------------------------------------------------------------------------------------------
typedef decltype(&k_conv_single<1>) SingleFn;      // every instantiation has this type
struct SingleInst { const char *name; SingleFn fn; };
static const SingleInst kSingle[4] = {{"k_conv_single<1>", k_conv_single<1>}, {"k_conv_single<2>", k_conv_single<2>},
                                      {"k_conv_single<3>", k_conv_single<3>}, {"k_conv_single<4>", k_conv_single<4>}};
static const SingleInst kSingleBwdStats[4] = {{"k_conv_single<1,bwd_stats>", k_conv_single<1, true>},
                                              {"k_conv_single<2,bwd_stats>", k_conv_single<2, true>},
                                              {"k_conv_single<3,bwd_stats>", k_conv_single<3, true>},
                                              {"k_conv_single<4,bwd_stats>", k_conv_single<4, true>}};

extern "C" int aabr_conv_forward_single(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                                        int64_t V_out, const int32_t *pairs, int vol, const float *bias, int flags,
                                        const float *wpack, const float *residual, void *stream_) {
  SingleLaunch t;
  const char *refused = single_launch(n_in, n_out, rows_in, V_out, vol, flags, single_knobs(), t);
  AABR_CHECK_ARG(!refused, refused);
  if (V_out == 0) return AABR_OK;
  AABR_CHECK_ARG(in_feats && out_feats && pairs && wpack, "null pointer / empty input");
  AABR_CHECK_ARG((((uintptr_t)in_feats | (uintptr_t)out_feats | (uintptr_t)wpack | (uintptr_t)residual |
                   (uintptr_t)bias) & 15) == 0, "feature / weight / residual / bias pointers must be 16-byte aligned");
  const SingleInst &e = kSingle[t.kg - 1];
  g_last_variant = e.name;
  hipLaunchKernelGGL(e.fn, dim3((unsigned)t.grid_x, (unsigned)t.grid_y), dim3(256), (size_t)t.lds_bytes,
                     (hipStream_t)stream_, in_feats, n_in, t.in_bytes, out_feats, n_out, V_out, pairs, vol, t.chunk_pairs,
                     t.wflip, wpack, t.wp_bytes, bias, residual, SingleBwdStats{});
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// The input-gradient form whose write-out forms the backward statistics of the BatchNorm whose d_out it writes: `stats`
// takes single_bwd_stats_launch's parts x [2][n_out] doubles; the BatchNorm arguments as aabr_conv_forward_wide_bwd_stats.
extern "C" int aabr_conv_forward_single_bwd_stats(const float *in_feats, int n_in, int64_t rows_in, float *out_feats,
                                                  int n_out, int64_t V_out, const int32_t *pairs, int vol,
                                                  const float *bias, int flags, const float *wpack, const float *residual,
                                                  double *stats, const float *bn_in, const float *save_mean,
                                                  const float *save_invstd, const float *bn_weight, const float *bn_bias,
                                                  float leakiness, void *stream_) {
  SingleBwdStatsLaunch t;
  const char *refused = single_bwd_stats_launch(n_in, n_out, rows_in, V_out, vol, flags, single_knobs(), t);
  AABR_CHECK_ARG(!refused, refused);
  if (V_out == 0) return AABR_OK;
  AABR_CHECK_ARG(in_feats && out_feats && pairs && wpack, "null pointer / empty input");
  AABR_CHECK_ARG(stats && bn_in && save_mean && save_invstd, "null pointer");
  AABR_CHECK_ARG(leakiness >= 0.0f, "the activation sign is recomputed from the BatchNorm input: leakiness >= 0");
  AABR_CHECK_ARG((((uintptr_t)in_feats | (uintptr_t)out_feats | (uintptr_t)wpack | (uintptr_t)residual |
                   (uintptr_t)bias | (uintptr_t)bn_in) & 15) == 0,
                 "feature / weight / residual / bias / BatchNorm input pointers must be 16-byte aligned");
  AABR_CHECK_ARG(((uintptr_t)stats & 7) == 0, "the statistics must be 8-byte aligned");
  const SingleInst &e = kSingleBwdStats[t.l.kg - 1];
  g_last_variant = e.name;
  hipLaunchKernelGGL(e.fn, dim3((unsigned)t.l.grid_x, (unsigned)t.l.grid_y), dim3(256), (size_t)t.l.lds_bytes,
                     (hipStream_t)stream_, in_feats, n_in, t.l.in_bytes, out_feats, n_out, V_out, pairs, vol,
                     t.l.chunk_pairs, t.l.wflip, wpack, t.l.wp_bytes, bias, residual,
                     SingleBwdStats{stats, bn_in, save_mean, save_invstd, bn_weight, bn_bias, leakiness});
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

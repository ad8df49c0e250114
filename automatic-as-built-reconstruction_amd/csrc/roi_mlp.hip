// roi_mlp.hip -- the dense layers of the box head (FPN2MLPFeatureExtractor after its pooler, roi_box_feature_extractors.py:
// 46-169, and FPNPredictor, roi_box_predictors.py:34-109), gfx950: a dense fp32 GEMM family on v_mfma_f32_32x32x2_f32 with
// LDS-tiled operands and fused epilogues.  fp32 storage, except the pooled tensor and its gradient, which the
// _pooled_bf16 entry points read and write in place in bf16 (template parameter PT of the kernel: the loader's fetch
// widens one element, the LDS image and everything after it are the fp32 form's, the pooled write-out of the input
// gradient rounds once on store).  Only the instances with a pooled layout exist in bf16: plain rows, windows, dY, Y, W,
// dW and db are fp32.
//
// ONE kernel template, k_mlp_gemm<BT, LA, LB, DW>, serves the four products of a layer Y = act(A W^T + bias), W [N, K]:
//   forward          Y  [M, N] = A (rows m, reduce k)        x  W (cols n, reduce k)      + bias, ReLU
//   input gradient   dA [M, K] = dY.mask (rows m, reduce n)  x  W (cols k, reduce n)      stored row-major or pooled
//   weight gradient  dW [N, K] = dY.mask (rows n, reduce m)  x  A (cols k, reduce m)      (+ db, the column sums of dY.mask)
// Each operand is an `outer x reduce` matrix whose element address is off_out(outer) + off_red(reduce) -- true of every
// layout here: plain rows with either index contiguous (kRed / kOut), and the pooler's [n, C, hw, pz] tensor read in
// place as rows m = n hw + s, columns k = c pz + z (kPoolM: the rows are the outer index, forward; kPoolK: the columns
// are, weight gradient).  A workgroup (256 threads, 2 x 2 waves) owns a BT x BT output tile (BT = 128: 2 x 2 MFMA tiles
// of 32 x 32 per wave; BT = 64: one), walks the reduction in chunks of kBK = 32, keeps the next chunk's global loads in
// registers while the MFMAs of the current one run from LDS (one buffer, two barriers per chunk).  Plain-row operands are
// read along whichever index is contiguous in memory.  The pooled layouts are NOT fully coalesced: the lanes run along
// k = c pz + z (kPoolM) or read one row's k range (kPoolK), so a wave instruction reads runs of pz floats (16 bytes at
// the default pz = 4) that lie hw pz floats apart, a quarter of each cache line it touches, and the pooled input
// gradient is stored in the same fragments.  The neighbouring rows' instructions hit the same lines in cache; lanes along
// a ROI's contiguous (s, z) block for a fixed c would be the coalesced form and is left for when this is timed.
// A partial tile is zero-filled, so any M >= 1, N >= 1, K work.
//
// The corner form of the box head (MODEL.CORNER_ROI) runs fc6 over WINDOWS of the convolution rows X [n ph pw, R]: the
// feature extractor cuts the pw = 11 axis into cor0 = w 0..2, body = w 2..8 and cor1 = w 8..10
// (roi_box_feature_extractors.py:122-147) and gives each part its own fc6.  A window [w0, w0 + wlen) of ROI n is ph runs
// of wlen R contiguous floats, pw R apart, so it is one more outer x reduce operand (kWinM: the rows are the outer index;
// kWinK: the columns are): row m -> n pw ph R + w0 R, column k = (h wlen + wl) R + r -> h pw R + (wl R + r).  Forward
// and weight gradient read the windows in place, the input gradient writes them in place (OW); nothing is copied.
// Rows come in up to two blocks with a w0 each (rows < nsplit: w0a, the rest: w0b and ROI m - nsplit), so the two
// corner windows, which share their weights, are ONE GEMM with M = 2 n.  Lanes run along k in both layouts: runs of
// wlen R floats, coalesced.
// The windows overlap at w = 2 and w = 8, so the input gradient dX receives two contributions there.  Order: the body
// GEMM goes first and STORES w 2..8; the corner GEMM, next on the same stream, stores w 0, 1, 9, 10 and ADDS into w 2 and
// w 8 (one thread per element, a plain load-add-store: dX = corner term + body term).  Every element of dX is written
// once or stored-then-added, there is no zero fill and no atomic, and two runs give the same bits.
// LDS rows are BT + 2 floats: the reduce-fast store (row = lane & 31) and the MFMA read (lanes 32..63 read row kk + 16,
// 16 (BT + 2) = 32 mod 64 banks from lanes 0..31) are both conflict-free.
//
// mask = (Y > 0) of a ReLU forward is folded into the dY operand load (Y has dY's layout).  The pooled input gradient
// is stored straight into the pooled layout (every element once, plain stores).  The weight gradient of fc6 is stored
// through the column permutation k' = s R + r -> r hw + s, so the parameter's gradient is in the reference's layout
// while the GEMM runs on the packed weight (k_mlp_pack_fc6, one launch per forward).
//
// Determinism: no float atomics anywhere.  Where the weight gradient's reduction over M is split across workgroups
// (aabr_roi_mlp_dw_splits > 1), each writes its partial tile (and partial column sums) to scratch and k_mlp_dw_reduce adds
// the partials in split order.  The column sums ride in the weight-gradient kernel (the workgroups of column tile 0 add
// the rows of their staged dY tile in row order).
//
// Launches: forward 1; input gradient 1; weight + bias gradient 1, or 2 when split; fc6's weight pack 1.
#include "common.h"
#include <type_traits>

namespace aabr {

constexpr int kBK = 32;                      // reduction elements per chunk
enum { kRed = 0, kOut = 1, kPoolM = 2, kPoolK = 3, kWinM = 4, kWinK = 5 };

// a window of the convolution rows [n ph pw, R] as an outer x reduce matrix [blocks n, ph wlen R]
struct MlpWindow {
  uint32_t R, wR;          // R, wlen R
  uint32_t nsplit;         // rows below it use w0a, the rest w0b and ROI m - nsplit
  uint32_t w0a, w0b;
  int64_t pwR, nstride;    // pw R, ph pw R
};
__device__ inline int64_t mlp_win_row(const MlpWindow &w, uint32_t m, uint32_t &w0) {
  const bool first = m < w.nsplit;
  w0 = first ? w.w0a : w.w0b;
  return (int64_t)(first ? m : m - w.nsplit) * w.nstride + (int64_t)w0 * w.R;
}
__device__ inline int64_t mlp_win_col(const MlpWindow &w, uint32_t k, uint32_t &rem) {
  const uint32_t h = k / w.wR;
  rem = k - h * w.wR;
  return (int64_t)h * w.pwR + rem;
}

struct MlpOperand {
  const float *p;          // fp32 elements -- EXCEPT the pooled operand of a PT = __bf16 instance (k_mlp_gemm), where the
                           // _pooled_bf16 entry points pass bf16 elements through this pointer and MlpLoader::fetch reads
                           // it as const ST *.  Nothing else may dereference p: a new (vectorised) load goes through ST
  const float *mask;       // same layout as p, or NULL: the element counts where mask > 0
  int64_t ld;              // kRed: outer stride; kOut: reduce stride
  uint32_t hw, pz;         // pooled layouts
  int64_t hwpz, nstride;   // hw * pz, C * hw * pz
  MlpWindow win;           // window layouts
};

struct MlpArgs {
  MlpOperand a, b;
  int64_t rows, cols, red;        // the output is [rows, cols]
  int64_t red_per_split;          // multiple of kBK
  uint32_t tiles_c, tiles_r, splits;
  float *out;                     // fp32 -- except the pooled input gradient of a PT = __bf16 instance: bf16 elements,
                                  // stored as (PT *)out at the kernel's one write-out statement (kOutPT)
  int64_t ldo;
  uint32_t o_hw, o_pz;            // o_pz > 0: the output is stored in the pooled layout (rows m, cols k)
  int64_t o_hwpz, o_nstride;
  MlpWindow o_win;                // OW: the output is stored into windows of the convolution rows (rows m, cols k) ...
  uint32_t o_acc_w[2];            // ... and ADDED to what is there at these two absolute w positions (~0u: none)
  uint32_t perm_R, perm_hw;       // perm_hw > 0: output column k' = s R + r is stored at column r hw + s
  const float *bias;
  int relu;
  float *db;                      // DW: column sums of the A operand over the reduction, or NULL
  float *scratch;                 // DW with splits > 1: [splits][rows * cols + rows]
};

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the two halves of an element's address
template <int L> __device__ inline int64_t mlp_off_out(const MlpOperand &q, uint32_t o) {
  if (L == kRed) return (int64_t)o * q.ld;
  if (L == kOut) return (int64_t)o;
  if (L == kPoolM) {                                 // outer = m = n hw + s
    const uint32_t n = o / q.hw, s = o - n * q.hw;
    return (int64_t)n * q.nstride + (int64_t)s * q.pz;
  }
  uint32_t x;
  if (L == kWinM) return mlp_win_row(q.win, o, x);
  if (L == kWinK) return mlp_win_col(q.win, o, x);
  const uint32_t c = o / q.pz, z = o - c * q.pz;     // outer = k = c pz + z
  return (int64_t)c * q.hwpz + z;
}
template <int L> __device__ inline int64_t mlp_off_red(const MlpOperand &q, uint32_t r) {
  if (L == kRed) return (int64_t)r;
  if (L == kOut) return (int64_t)r * q.ld;
  if (L == kPoolM) {                                 // reduce = k
    const uint32_t c = r / q.pz, z = r - c * q.pz;
    return (int64_t)c * q.hwpz + z;
  }
  uint32_t x;
  if (L == kWinM) return mlp_win_col(q.win, r, x);
  if (L == kWinK) return mlp_win_row(q.win, r, x);
  const uint32_t n = r / q.hw, s = r - n * q.hw;     // reduce = m
  return (int64_t)n * q.nstride + (int64_t)s * q.pz;
}

// One operand's BT x kBK tile: global -> registers -> LDS image [kBK][BT + 2].  Thread t serves, for i < NI,
//   reduce-fast layouts (kRed, kPoolM, kWinM):  reduce t & 31, outer (t >> 5) + 8 i
//   outer-fast layouts  (kOut, kPoolK, kWinK):  outer t % BT,  reduce t / BT + (256 / BT) i
// ST is the storage of the operand's elements: float, or __bf16 for the pooled layouts (q.p then points at bf16)
template <int BT, int L, typename ST = float> struct MlpLoader {
  static constexpr int NI = BT * kBK / 256;
  static constexpr bool kRedFast = (L == kRed || L == kPoolM || L == kWinM);
  static constexpr bool kOutTab = (L == kPoolM || L == kWinM);   // one off_out per outer index of the thread
  static constexpr int LDT = BT + 2;
  int64_t oo[kOutTab ? NI : 1];  // off_out of this thread's outer indices, -1 outside the matrix (kRed: of the first)
  int64_t ld8;                       // kRed: 8 rows further
  int left;                          // kRed: outer indices from the thread's first to the matrix's end (clamped)
  float v[NI];

  __device__ inline void init(const MlpOperand &q, int64_t o0, int64_t n_out, int t) {
    ld8 = 8 * q.ld, left = 0;
    if (L == kRed) {
      const int64_t o = o0 + (t >> 5), n = n_out - o;
      oo[0] = o * q.ld;
      left = n < 0 ? 0 : n > BT ? BT : (int)n;
    } else if (kOutTab) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int64_t o = o0 + (t >> 5) + 8 * i;
        oo[i] = o < n_out ? mlp_off_out<L>(q, (uint32_t)o) : -1;
      }
    } else {
      const int64_t o = o0 + t % BT;
      oo[0] = o < n_out ? mlp_off_out<L>(q, (uint32_t)o) : -1;
    }
  }
  __device__ inline float fetch(const MlpOperand &q, int64_t off) const {
    float x = (float)((const ST *)q.p)[off];           // bf16: widened here (exact), fp32 from here on
    if (q.mask) x = q.mask[off] > 0.f ? x : 0.f;
    return x;
  }
  __device__ inline void load(const MlpOperand &q, int64_t r0, int64_t r_end, int t) {
    if (kRedFast) {
      const int64_t r = r0 + (t & 31);
      const bool rv = r < r_end;
      const int64_t ro = rv ? mlp_off_red<L>(q, (uint32_t)r) : 0;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        if (L == kRed) v[i] = (rv && 8 * i < left) ? fetch(q, oo[0] + i * ld8 + ro) : 0.f;
        else v[i] = (rv && oo[kOutTab ? i : 0] >= 0) ? fetch(q, oo[kOutTab ? i : 0] + ro) : 0.f;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int64_t r = r0 + t / BT + (256 / BT) * i;
        v[i] = (r < r_end && oo[0] >= 0) ? fetch(q, oo[0] + mlp_off_red<L>(q, (uint32_t)r)) : 0.f;
      }
    }
  }
  __device__ inline void store(float *lds, int t) const {
    if (kRedFast) {
#pragma unroll
      for (int i = 0; i < NI; ++i) lds[(t & 31) * LDT + (t >> 5) + 8 * i] = v[i];
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i) lds[(t / BT + (256 / BT) * i) * LDT + t % BT] = v[i];
    }
  }
};

// PT: the storage of whatever is in a pooled layout in this instance -- the kPoolM / kPoolK operand, or, in an instance
// without one, the pooled write-out (g.o_pz > 0: the input gradient).  float everywhere but in the _pooled_bf16 entries.
template <int BT, int LA, int LB, bool DW, bool OW = false, typename PT = float>
__global__ __launch_bounds__(256) void k_mlp_gemm(const MlpArgs g) {
  constexpr int LDT = BT + 2, TW = BT / 64;          // TW x TW MFMA tiles of 32 x 32 per wave
  constexpr bool kPoolA = LA == kPoolM || LA == kPoolK, kPoolB = LB == kPoolM || LB == kPoolK;
  constexpr bool kOutPT = !std::is_same<PT, float>::value && !kPoolA && !kPoolB;
  static_assert(std::is_same<PT, float>::value || (!OW && (kPoolA || kPoolB || !DW)), "bf16: pooled layouts only");
  __shared__ float sA[kBK * LDT];
  __shared__ float sB[kBK * LDT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  uint32_t bid = blockIdx.x;
  const uint32_t tc = bid % g.tiles_c;
  bid /= g.tiles_c;
  const uint32_t tr = bid % g.tiles_r, split = bid / g.tiles_r;
  const int64_t row0 = (int64_t)tr * BT, col0 = (int64_t)tc * BT;
  const int64_t r_begin = (int64_t)split * g.red_per_split;
  const int64_t r_end = r_begin + g.red_per_split < g.red ? r_begin + g.red_per_split : g.red;

  MlpLoader<BT, LA, typename std::conditional<kPoolA, PT, float>::type> la;
  MlpLoader<BT, LB, typename std::conditional<kPoolB, PT, float>::type> lb;
  la.init(g.a, row0, g.rows, t);
  lb.init(g.b, col0, g.cols, t);

  f32x16 acc[TW][TW];
#pragma unroll
  for (int i = 0; i < TW; ++i)
#pragma unroll
    for (int j = 0; j < TW; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  float dbacc = 0.f;
  const bool do_db = DW && g.db != nullptr && tc == 0;

  la.load(g.a, r_begin, r_end, t);
  lb.load(g.b, r_begin, r_end, t);
  const int kh = 16 * (lane >> 5), l31 = lane & 31;
  for (int64_t r0 = r_begin; r0 < r_end; r0 += kBK) {
    __syncthreads();                                 // the previous chunk's reads are done
    la.store(sA, t);
    lb.store(sB, t);
    __syncthreads();
    if (r0 + kBK < r_end) {
      la.load(g.a, r0 + kBK, r_end, t);
      lb.load(g.b, r0 + kBK, r_end, t);
    }
    if (DW) {
      if (do_db && t < BT) {
#pragma unroll 8
        for (int r = 0; r < kBK; ++r) dbacc += sA[r * LDT + t];
      }
    }
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {                // MFMA step kk sums reduce rows kk and kk + 16 of the chunk
      float a[TW], b[TW];
#pragma unroll
      for (int i = 0; i < TW; ++i) a[i] = sA[(kk + kh) * LDT + wm * (BT / 2) + i * 32 + l31];
#pragma unroll
      for (int j = 0; j < TW; ++j) b[j] = sB[(kk + kh) * LDT + wn * (BT / 2) + j * 32 + l31];
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TW; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // write-out: lane holds column (lane & 31), rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of each 32 x 32 tile
  const bool to_scratch = DW && g.splits > 1;
  float *outp = to_scratch ? g.scratch + (int64_t)split * (g.rows * g.cols + g.rows) : g.out;
#pragma unroll
  for (int j = 0; j < TW; ++j) {
    const int64_t col = col0 + wn * (BT / 2) + j * 32 + l31;
    if (col >= g.cols) continue;
    int64_t co = col;
    float bias = 0.f;
    uint32_t wrem = 0;
    if (OW) {
      co = mlp_win_col(g.o_win, (uint32_t)col, wrem);
      wrem /= g.o_win.R;                             // the column's w inside the window
    } else if (!DW) {
      if (g.bias) bias = g.bias[col];
      if (g.o_pz) {
        const uint32_t c = (uint32_t)col / g.o_pz, z = (uint32_t)col - c * g.o_pz;
        co = (int64_t)c * g.o_hwpz + z;
      }
    } else if (!to_scratch && g.perm_hw) {
      const uint32_t s = (uint32_t)col / g.perm_R, r = (uint32_t)col - s * g.perm_R;
      co = (int64_t)r * g.perm_hw + s;
    }
#pragma unroll
    for (int i = 0; i < TW; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = row0 + wm * (BT / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= g.rows) continue;
        float x = acc[i][j][r];
        int64_t ro;
        if (OW) {
          uint32_t w0;
          ro = mlp_win_row(g.o_win, (uint32_t)row, w0);
          const uint32_t w = w0 + wrem;
          if (w == g.o_acc_w[0] || w == g.o_acc_w[1]) x += outp[ro + co];
        } else if (!DW) {
          x += bias;
          if (g.relu) x = x > 0.f ? x : 0.f;
          if (g.o_pz) {
            const uint32_t n = (uint32_t)row / g.o_hw, s = (uint32_t)row - n * g.o_hw;
            ro = (int64_t)n * g.o_nstride + (int64_t)s * g.o_pz;
          } else {
            ro = row * g.ldo;
          }
        } else {
          ro = row * (to_scratch ? g.cols : g.ldo);
        }
        if (kOutPT) ((PT *)outp)[ro + co] = (PT)x;   // the pooled input gradient in bf16: one rounding of x
        else outp[ro + co] = x;
      }
    }
  }
  if (DW) {
    if (do_db && t < BT && row0 + t < g.rows) {
      if (to_scratch) outp[g.rows * g.cols + row0 + t] = dbacc;
      else g.db[row0 + t] = dbacc;
    }
  }
}

// second stage of a split weight gradient: the partials added in split order
__global__ __launch_bounds__(256) void k_mlp_dw_reduce(const float *__restrict__ scratch, int splits, int64_t rows,
                                                       int64_t cols, uint32_t perm_R, uint32_t perm_hw, int64_t ldo,
                                                       float *__restrict__ dW, float *__restrict__ db) {
  const int64_t per = rows * cols + rows;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per || (i >= rows * cols && db == nullptr)) return;
  float s = scratch[i];
  for (int p = 1; p < splits; ++p) s += scratch[(int64_t)p * per + i];
  if (i >= rows * cols) {
    db[i - rows * cols] = s;
    return;
  }
  const int64_t row = i / cols;
  int64_t col = i - row * cols;
  if (perm_hw) {
    const int64_t sp = col / perm_R, r = col - sp * perm_R;
    col = r * perm_hw + sp;
  }
  dW[row * ldo + col] = s;
}

// fc6's weight [N, R hw] (column r hw + s, the reference's x.view(N, -1) order) -> packed [N, hw R] (column s R + r, the
// order of the stored convolution rows): reads coalesced along the packed column's r ... writes coalesced
__global__ __launch_bounds__(256) void k_mlp_pack_fc6(const float *__restrict__ W, int64_t total, int64_t R, int64_t hw,
                                                      float *__restrict__ Wp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t K = R * hw, o = i / K, kp = i - o * K, s = kp / R, r = kp - s * R;
  Wp[i] = W[o * K + r * hw + s];
}

constexpr int64_t kMlpMaxDim = 2147483647LL - 256;   // 32-bit row / column arithmetic in the kernels, padded tiles included
constexpr int kMlpDwRowsPerSplit = 256, kMlpDwMaxSplits = 64;

static int64_t mlp_tiles(int64_t rows, int64_t cols, int bt) { return ceil_div(rows, bt) * ceil_div(cols, bt); }

template <int LA, int LB, bool DW, bool OW = false, typename PT = float>
static void mlp_launch(int bt, const MlpArgs &g, hipStream_t st) {
  const unsigned grid = g.tiles_c * g.tiles_r * g.splits;
  if (bt == 128) hipLaunchKernelGGL((k_mlp_gemm<128, LA, LB, DW, OW, PT>), dim3(grid), dim3(256), 0, st, g);
  else hipLaunchKernelGGL((k_mlp_gemm<64, LA, LB, DW, OW, PT>), dim3(grid), dim3(256), 0, st, g);
}

static bool mlp_set_grid(MlpArgs &g, int bt, int64_t splits) {
  const int64_t tr = ceil_div(g.rows, bt), tc = ceil_div(g.cols, bt);
  if (tr * tc * splits >= (1LL << 31)) return false;
  g.tiles_r = (uint32_t)tr, g.tiles_c = (uint32_t)tc, g.splits = (uint32_t)splits;
  return true;
}

static void mlp_pooled(MlpOperand &q, int64_t K, int64_t hw, int pz) {
  q.hw = (uint32_t)hw, q.pz = (uint32_t)pz;
  q.hwpz = hw * pz, q.nstride = K * hw;     // C hw pz with C = K / pz
}

// the window description of the C ABI -> MlpWindow, M and K; false: a shape the kernels do not take
static bool mlp_window(const AabrMlpWindow *v, MlpWindow &w, int64_t &M, int64_t &K) {
  if (!v || v->n_rois < 0 || v->ph < 1 || v->pw < 1 || v->R < 1 || v->wlen < 1 || (v->blocks != 1 && v->blocks != 2))
    return false;
  for (int b = 0; b < v->blocks; ++b)
    if (v->w0[b] < 0 || (int64_t)v->w0[b] + v->wlen > v->pw) return false;     // every window inside the pw axis
  if ((int64_t)v->ph * v->pw * v->R > kMlpMaxDim || v->n_rois > kMlpMaxDim / 2) return false;
  w.R = (uint32_t)v->R, w.wR = (uint32_t)((int64_t)v->wlen * v->R);
  w.nsplit = (uint32_t)v->n_rois;
  w.w0a = (uint32_t)v->w0[0], w.w0b = (uint32_t)v->w0[v->blocks - 1];
  w.pwR = (int64_t)v->pw * v->R, w.nstride = (int64_t)v->ph * w.pwR;
  M = v->blocks * v->n_rois, K = (int64_t)v->ph * v->wlen * v->R;
  return true;
}

} // namespace aabr

using namespace aabr;

// the _AS forms: the same checks inside a helper, reported under the entry point's name `fn` (AABR_CHECK_ARG_AS)
#define MLP_CHECK_SHAPE_AS(fn, M, N, K)                                                                   \
  AABR_CHECK_ARG_AS(fn, (M) >= 0 && (N) >= 1 && (K) >= 4, "need M >= 0, N >= 1, K >= 4");                 \
  AABR_CHECK_ARG_AS(fn, (K) % 4 == 0, "K must be a multiple of 4");                                       \
  AABR_CHECK_ARG_AS(fn, (M) <= kMlpMaxDim && (N) <= kMlpMaxDim && (K) <= kMlpMaxDim, "M, N, K must stay below 2^31 - 256")
#define MLP_CHECK_SHAPE(M, N, K) MLP_CHECK_SHAPE_AS(__func__, M, N, K)
#define MLP_CHECK_LAYOUT_AS(fn, layout, M, K, hw, pz)                                                                    \
  AABR_CHECK_ARG_AS(fn, (layout) == AABR_MLP_ROWS || (layout) == AABR_MLP_POOLED, "a_layout must be AABR_MLP_ROWS or _POOLED"); \
  if ((layout) == AABR_MLP_POOLED) {                                                                                     \
    AABR_CHECK_ARG_AS(fn, (hw) >= 1 && (pz) >= 1 && (hw) <= kMlpMaxDim, "pooled layout: hw >= 1 and pz >= 1");           \
    AABR_CHECK_ARG_AS(fn, (K) % (pz) == 0 && (M) % (hw) == 0, "pooled layout: K = C pz and M = n hw");                   \
  }
// a bf16 operand of a _pooled_bf16 entry point: named, and 4-byte aligned, before anything else is looked at
#define MLP_CHECK_BF16(p, name) AABR_CHECK_ARG(((uintptr_t)(p) & 3) == 0, name " must be 4-byte aligned")

extern "C" int aabr_roi_mlp_tile(int64_t rows, int64_t cols) {
  if (rows < 1 || cols < 1) return 0;
  return mlp_tiles(rows, cols, 128) >= 192 ? 128 : 64;
}

extern "C" int aabr_roi_mlp_dw_splits(int64_t M, int64_t N, int64_t K) {
  if (M < 1 || N < 1 || K < 1) return 0;
  const int64_t blocks = mlp_tiles(N, K, aabr_roi_mlp_tile(N, K));
  int64_t s = 512 / blocks;
  if (s > kMlpDwMaxSplits) s = kMlpDwMaxSplits;
  const int64_t by_rows = ceil_div(M, kMlpDwRowsPerSplit);
  if (s > by_rows) s = by_rows;
  if (s < 1) s = 1;
  const int64_t per = ceil_div(ceil_div(M, s), kBK) * kBK;   // rows per split, whole chunks
  return (int)ceil_div(M, per);
}

extern "C" int64_t aabr_roi_mlp_dw_scratch_floats(int64_t M, int64_t N, int64_t K) {
  const int s = aabr_roi_mlp_dw_splits(M, N, K);
  return s > 1 ? (int64_t)s * (N * K + N) : 0;
}

// The three products; PT = the storage of the pooled tensor (A forward and weight gradient, dA input gradient): float
// for the fp32 entry points (either a_layout), __bf16 for the _pooled_bf16 ones (a_layout pooled; the pointer is passed
// as const float * and read as bf16 by the instance).  `fn`: the entry point's name for the error text.
template <typename PT>
static int mlp_forward(const char *fn, const float *A, int a_layout, int64_t hw, int pz, const float *W, const float *bias,
                       int relu, int64_t M, int64_t N, int64_t K, float *Y, void *stream_) {
  MLP_CHECK_SHAPE_AS(fn, M, N, K);
  MLP_CHECK_LAYOUT_AS(fn, a_layout, M, K, hw, pz);
  if (M == 0) return AABR_OK;
  AABR_CHECK_ARG_AS(fn, A && W && Y, "null pointer");
  MlpArgs g = {};
  g.a.p = A, g.a.ld = K;
  g.b.p = W, g.b.ld = K;
  g.rows = M, g.cols = N, g.red = K, g.red_per_split = ceil_div(K, kBK) * kBK;
  g.out = Y, g.ldo = N, g.bias = bias, g.relu = relu != 0;
  const int bt = aabr_roi_mlp_tile(M, N);
  AABR_CHECK_ARG_AS(fn, mlp_set_grid(g, bt, 1), "too many tiles");
  if (a_layout == AABR_MLP_POOLED) {
    mlp_pooled(g.a, K, hw, pz);
    mlp_launch<kPoolM, kRed, false, false, PT>(bt, g, (hipStream_t)stream_);
  } else if (std::is_same<PT, float>::value) {
    mlp_launch<kRed, kRed, false>(bt, g, (hipStream_t)stream_);
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_mlp_forward(const float *A, int a_layout, int64_t hw, int pz, const float *W, const float *bias,
                                    int relu, int64_t M, int64_t N, int64_t K, float *Y, void *stream_) {
  return mlp_forward<float>(__func__, A, a_layout, hw, pz, W, bias, relu, M, N, K, Y, stream_);
}

extern "C" int aabr_roi_mlp_forward_pooled_bf16(const void *A_bf16, int64_t hw, int pz, const float *W, const float *bias,
                                                int relu, int64_t M, int64_t N, int64_t K, float *Y, void *stream_) {
  MLP_CHECK_BF16(A_bf16, "A_bf16");
  AABR_CHECK_ARG(M <= 0 || A_bf16, "null A_bf16");
  AABR_CHECK_ARG(M <= 0 || W, "null W");
  AABR_CHECK_ARG(M <= 0 || Y, "null Y");
  return mlp_forward<__bf16>(__func__, (const float *)A_bf16, AABR_MLP_POOLED, hw, pz, W, bias, relu, M, N, K, Y, stream_);
}

template <typename PT>
static int mlp_backward_input(const char *fn, const float *dY, const float *Y, const float *W, int64_t M, int64_t N,
                              int64_t K, int a_layout, int64_t hw, int pz, float *dA, void *stream_) {
  MLP_CHECK_SHAPE_AS(fn, M, N, K);
  MLP_CHECK_LAYOUT_AS(fn, a_layout, M, K, hw, pz);
  if (M == 0) return AABR_OK;
  AABR_CHECK_ARG_AS(fn, dY && W && dA, "null pointer");
  MlpArgs g = {};
  g.a.p = dY, g.a.mask = Y, g.a.ld = N;
  g.b.p = W, g.b.ld = K;
  g.rows = M, g.cols = K, g.red = N, g.red_per_split = ceil_div(N, kBK) * kBK;
  g.out = dA, g.ldo = K;
  if (a_layout == AABR_MLP_POOLED) {
    g.o_hw = (uint32_t)hw, g.o_pz = (uint32_t)pz, g.o_hwpz = hw * pz, g.o_nstride = K * hw;
  }
  const int bt = aabr_roi_mlp_tile(M, K);
  AABR_CHECK_ARG_AS(fn, mlp_set_grid(g, bt, 1), "too many tiles");
  mlp_launch<kRed, kOut, false, false, PT>(bt, g, (hipStream_t)stream_);   // PT = __bf16: the pooled write-out in bf16
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_mlp_backward_input(const float *dY, const float *Y, const float *W, int64_t M, int64_t N,
                                           int64_t K, int a_layout, int64_t hw, int pz, float *dA, void *stream_) {
  return mlp_backward_input<float>(__func__, dY, Y, W, M, N, K, a_layout, hw, pz, dA, stream_);
}

extern "C" int aabr_roi_mlp_backward_input_pooled_bf16(const float *dY, const float *Y, const float *W, int64_t M,
                                                       int64_t N, int64_t K, int64_t hw, int pz, void *dA_bf16,
                                                       void *stream_) {
  MLP_CHECK_BF16(dA_bf16, "dA_bf16");
  AABR_CHECK_ARG(M <= 0 || dA_bf16, "null dA_bf16");
  AABR_CHECK_ARG(M <= 0 || dY, "null dY");
  AABR_CHECK_ARG(M <= 0 || W, "null W");
  return mlp_backward_input<__bf16>(__func__, dY, Y, W, M, N, K, AABR_MLP_POOLED, hw, pz, (float *)dA_bf16, stream_);
}

template <typename PT>
static int mlp_backward_weight(const char *fn, const float *dY, const float *Y, const float *A, int a_layout, int64_t hw,
                               int pz, int64_t M, int64_t N, int64_t K, int64_t perm_hw, float *dW, float *db,
                               float *scratch, void *stream_) {
  MLP_CHECK_SHAPE_AS(fn, M, N, K);
  MLP_CHECK_LAYOUT_AS(fn, a_layout, M, K, hw, pz);
  AABR_CHECK_ARG_AS(fn, perm_hw >= 0 && (perm_hw == 0 || K % perm_hw == 0), "perm_hw must be 0 or divide K");
  AABR_CHECK_ARG_AS(fn, dW, "null pointer");
  hipStream_t st = (hipStream_t)stream_;
  if (M == 0) {                                       // an empty sum: zeros, no kernel
    AABR_CHECK_HIP(hipMemsetAsync(dW, 0, sizeof(float) * N * K, st));
    if (db) AABR_CHECK_HIP(hipMemsetAsync(db, 0, sizeof(float) * N, st));
    return AABR_OK;
  }
  AABR_CHECK_ARG_AS(fn, dY && A, "null pointer");
  const int splits = aabr_roi_mlp_dw_splits(M, N, K);
  AABR_CHECK_ARG_AS(fn, splits == 1 || scratch, "null scratch");
  MlpArgs g = {};
  g.a.p = dY, g.a.mask = Y, g.a.ld = N;
  g.b.p = A, g.b.ld = K;
  g.rows = N, g.cols = K, g.red = M;
  g.red_per_split = ceil_div(ceil_div(M, splits), kBK) * kBK;
  g.out = dW, g.ldo = K, g.db = db, g.scratch = scratch;
  if (perm_hw) g.perm_hw = (uint32_t)perm_hw, g.perm_R = (uint32_t)(K / perm_hw);
  const int bt = aabr_roi_mlp_tile(N, K);
  AABR_CHECK_ARG_AS(fn, mlp_set_grid(g, bt, splits), "too many tiles");
  if (a_layout == AABR_MLP_POOLED) {
    mlp_pooled(g.b, K, hw, pz);
    mlp_launch<kOut, kPoolK, true, false, PT>(bt, g, st);
  } else if (std::is_same<PT, float>::value) {
    mlp_launch<kOut, kOut, true>(bt, g, st);
  }
  AABR_CHECK_LAUNCH();
  if (splits > 1) {
    const int64_t per = N * K + N;
    AABR_CHECK_ARG_AS(fn, ceil_div(per, 256) < (1LL << 31), "too many elements");
    hipLaunchKernelGGL(k_mlp_dw_reduce, dim3((unsigned)ceil_div(per, 256)), dim3(256), 0, st, scratch, splits, N, K,
                       g.perm_R, g.perm_hw, K, dW, db);
    AABR_CHECK_LAUNCH();
  }
  return AABR_OK;
}

extern "C" int aabr_roi_mlp_backward_weight(const float *dY, const float *Y, const float *A, int a_layout, int64_t hw,
                                            int pz, int64_t M, int64_t N, int64_t K, int64_t perm_hw, float *dW,
                                            float *db, float *scratch, void *stream_) {
  return mlp_backward_weight<float>(__func__, dY, Y, A, a_layout, hw, pz, M, N, K, perm_hw, dW, db, scratch, stream_);
}

extern "C" int aabr_roi_mlp_backward_weight_pooled_bf16(const float *dY, const float *Y, const void *A_bf16, int64_t hw,
                                                        int pz, int64_t M, int64_t N, int64_t K, int64_t perm_hw,
                                                        float *dW, float *db, float *scratch, void *stream_) {
  MLP_CHECK_BF16(A_bf16, "A_bf16");
  AABR_CHECK_ARG(M <= 0 || A_bf16, "null A_bf16");
  AABR_CHECK_ARG(M <= 0 || dY, "null dY");
  AABR_CHECK_ARG(dW, "null dW");
  return mlp_backward_weight<__bf16>(__func__, dY, Y, (const float *)A_bf16, AABR_MLP_POOLED, hw, pz, M, N, K, perm_hw, dW,
                                     db, scratch, stream_);
}

extern "C" int aabr_roi_mlp_pack_fc6(const float *W, int64_t N, int64_t R, int64_t hw, float *Wp, void *stream_) {
  AABR_CHECK_ARG(N >= 1 && R >= 1 && hw >= 1, "need N, R, hw >= 1");
  AABR_CHECK_ARG(R <= kMlpMaxDim / hw && N <= (1LL << 38) / (R * hw), "weight too large");
  AABR_CHECK_ARG(W && Wp, "null pointer");
  const int64_t total = N * R * hw;
  hipLaunchKernelGGL(k_mlp_pack_fc6, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream_, W, total,
                     R, hw, Wp);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// ---- fc6 over windows of the convolution rows (the corner form of the box head; layouts kWinM / kWinK / OW above) ----

extern "C" int aabr_roi_mlp_forward_window(const float *X, const AabrMlpWindow *win, const float *W, const float *bias,
                                           int relu, int64_t N, float *Y, void *stream_) {
  MlpWindow w;
  int64_t M, K;
  AABR_CHECK_ARG(mlp_window(win, w, M, K), "bad window (need ph, pw, R, wlen >= 1, blocks 1 or 2, 0 <= w0, w0 + wlen <= pw)");
  MLP_CHECK_SHAPE(M, N, K);
  if (M == 0) return AABR_OK;
  AABR_CHECK_ARG(X && W && Y, "null pointer");
  MlpArgs g = {};
  g.a.p = X, g.a.win = w;
  g.b.p = W, g.b.ld = K;
  g.rows = M, g.cols = N, g.red = K, g.red_per_split = ceil_div(K, kBK) * kBK;
  g.out = Y, g.ldo = N, g.bias = bias, g.relu = relu != 0;
  const int bt = aabr_roi_mlp_tile(M, N);
  AABR_CHECK_ARG(mlp_set_grid(g, bt, 1), "too many tiles");
  mlp_launch<kWinM, kRed, false>(bt, g, (hipStream_t)stream_);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_mlp_backward_input_window(const float *dY, const float *Y, const float *W,
                                                  const AabrMlpWindow *win, int64_t N, int acc_w0, int acc_w1, float *dX,
                                                  void *stream_) {
  MlpWindow w;
  int64_t M, K;
  AABR_CHECK_ARG(mlp_window(win, w, M, K), "bad window (need ph, pw, R, wlen >= 1, blocks 1 or 2, 0 <= w0, w0 + wlen <= pw)");
  MLP_CHECK_SHAPE(M, N, K);
  AABR_CHECK_ARG(acc_w0 >= -1 && acc_w1 >= -1 && acc_w0 < win->pw && acc_w1 < win->pw, "acc_w must be -1 or a w position");
  // the rows of a two-block GEMM are stored by different threads: the blocks may not overlap each other
  AABR_CHECK_ARG(win->blocks == 1 || win->w0[0] + win->wlen <= win->w0[1] || win->w0[1] + win->wlen <= win->w0[0],
                 "the two row blocks' windows overlap");
  if (M == 0) return AABR_OK;
  AABR_CHECK_ARG(dY && W && dX, "null pointer");
  MlpArgs g = {};
  g.a.p = dY, g.a.mask = Y, g.a.ld = N;
  g.b.p = W, g.b.ld = K;
  g.rows = M, g.cols = K, g.red = N, g.red_per_split = ceil_div(N, kBK) * kBK;
  g.out = dX, g.o_win = w;
  g.o_acc_w[0] = acc_w0 < 0 ? ~0u : (uint32_t)acc_w0, g.o_acc_w[1] = acc_w1 < 0 ? ~0u : (uint32_t)acc_w1;
  const int bt = aabr_roi_mlp_tile(M, K);
  AABR_CHECK_ARG(mlp_set_grid(g, bt, 1), "too many tiles");
  mlp_launch<kRed, kOut, false, true>(bt, g, (hipStream_t)stream_);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_roi_mlp_backward_weight_window(const float *dY, const float *Y, const float *X,
                                                   const AabrMlpWindow *win, int64_t N, int64_t perm_hw, float *dW,
                                                   float *db, float *scratch, void *stream_) {
  MlpWindow w;
  int64_t M, K;
  AABR_CHECK_ARG(mlp_window(win, w, M, K), "bad window (need ph, pw, R, wlen >= 1, blocks 1 or 2, 0 <= w0, w0 + wlen <= pw)");
  MLP_CHECK_SHAPE(M, N, K);
  AABR_CHECK_ARG(perm_hw >= 0 && (perm_hw == 0 || K % perm_hw == 0), "perm_hw must be 0 or divide K");
  AABR_CHECK_ARG(dW, "null pointer");
  hipStream_t st = (hipStream_t)stream_;
  if (M == 0) {                                       // an empty sum: zeros, no kernel
    AABR_CHECK_HIP(hipMemsetAsync(dW, 0, sizeof(float) * N * K, st));
    if (db) AABR_CHECK_HIP(hipMemsetAsync(db, 0, sizeof(float) * N, st));
    return AABR_OK;
  }
  AABR_CHECK_ARG(dY && X, "null pointer");
  const int splits = aabr_roi_mlp_dw_splits(M, N, K);
  AABR_CHECK_ARG(splits == 1 || scratch, "null scratch");
  MlpArgs g = {};
  g.a.p = dY, g.a.mask = Y, g.a.ld = N;
  g.b.p = X, g.b.win = w;
  g.rows = N, g.cols = K, g.red = M;
  g.red_per_split = ceil_div(ceil_div(M, splits), kBK) * kBK;
  g.out = dW, g.ldo = K, g.db = db, g.scratch = scratch;
  if (perm_hw) g.perm_hw = (uint32_t)perm_hw, g.perm_R = (uint32_t)(K / perm_hw);
  const int bt = aabr_roi_mlp_tile(N, K);
  AABR_CHECK_ARG(mlp_set_grid(g, bt, splits), "too many tiles");
  mlp_launch<kOut, kWinK, true>(bt, g, st);
  AABR_CHECK_LAUNCH();
  if (splits > 1) {
    const int64_t per = N * K + N;
    AABR_CHECK_ARG(ceil_div(per, 256) < (1LL << 31), "too many elements");
    hipLaunchKernelGGL(k_mlp_dw_reduce, dim3((unsigned)ceil_div(per, 256)), dim3(256), 0, st, scratch, splits, N, K,
                       g.perm_R, g.perm_hw, K, dW, db);
    AABR_CHECK_LAUNCH();
  }
  return AABR_OK;
}

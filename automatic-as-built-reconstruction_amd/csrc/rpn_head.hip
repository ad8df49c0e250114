// rpn_head.hip -- the RPN head (SingleConvRPNHead_Sparse3D, modeling/rpn/rpn_sparse3d.py:81-131) over the rows of every
// feature map in ONE launch, gfx950, on v_mfma_f32_32x32x2_f32 (an exact fmaf chain per element); the feature rows f and
// their gradient d_f in fp32 or bf16 storage (template parameter FT, aabr_rpn_head_*_bf16), everything else fp32:
//   t = relu(f W1^T + b1),  obj = t Wc^T + bc  [V, A],  reg = t Wr^T + br  [V, A, 7] (channel a 7 + j: the reference's
//   permute + reshape 'box_toghter', the [site, yaw] flatten order the rpn_glue consumers read).
// W1 [C, C], Wc [A, C], Wr [7 A, C] are the Conv2d weights as [out, in].  C in {32, 64, 96, 128}, 1 <= A <= 4.
// Separated-classifier groups (aabr_rpn_head_grouped_*; G = len(SEPARATE_CLASSES) + 1 RPN branches, 2 <= G <= 8,
// A G <= 16): Wc [A G, C] and Wr [7 A G, C] in the reference's row order (a G + g, a 7 G + 7 g + k), outputs GROUP-MAJOR
// ([G][V, A], [G][V, A, 7]) so a group's slice is a plain-layout tensor.
//
// The maps come as a by-value table (RpnMaps, built from the caller's AabrRpnMap records): block b serves the map m with
// first[m] <= b < first[m + 1] and the kRpnT = 64 consecutive rows (b - first[m]) 64 ... of it.  Nothing is concatenated.
//
// ONE forward and ONE backward kernel body, each instantiated per C without (kGroups = false) and with groups.  The
// switch keeps apart only what the packed [Wc; Wr] block's width decides: 8 A <= 32 columns are one MFMA tile, 8 A G <=
// 128 are NT2 = ceil(8 A G / 32) <= 4 of them, and a column's place in the outputs is the identity or rpn_col's map.
//
// Forward, k_rpn_head_fwd<C, kGroups> (256 threads = 2 x 2 waves; wave (wm, wn) owns rows wm 32 .. + 32 and the
// 32-column tiles wn, wn + 2): the f tile and W1 go through LDS in reduction chunks of 32 ([32][64 + 2] and [32][C + 2]),
// bias and ReLU are applied in registers, t is kept in LDS as [C][64 + 2] (and stored to `hidden` only when that is not
// NULL), and the second product reads it against the columns of [Wc; Wr], zero-padded to whole tiles, in the same
// order over the hidden units whatever the width: a grouped output has the plain kernel's bits on the matching weight
// row, the permutation is the write-out's.  Plain: one tile, one accumulator, the two wn = 0 waves, the chunk buffer
// [32][C + 2]; grouped: two accumulators per wave, the chunk buffer [32][128 + 2].  58.9 KB of LDS at C = 128, both.
//
// Backward, k_rpn_head_bwd<C, kGroups>: ONE fused kernel, one workgroup per CU.  Workgroup w of aabr_rpn_head_groups(
// total_tiles) serves tiles w, w + gridDim.x, ...  Per tile, with D = [d_obj | d_reg] in packed-column order, padded to
// NP = 32 NT2 columns (a NULL gradient reads as zeros):
//   d[Wc; Wr] += D^T t                     (registers; NT2 x NT tiles, wave w owning tiles w, w + 4, ...)
//   dt = (D [Wc; Wr]) . (t > 0)            -> LDS [64][C + 2]; serves as rows (reduce over the site) and, read transposed,
//                                             as columns (reduce over the hidden unit): C + 2 = 2 mod 32 keeps both
//                                             access patterns off each other's banks
//   dW1 += dt^T f                          (registers, up to 4 tiles per wave)
//   d_f = dt W1                            (W1 through LDS in chunks of 32 rows; every d_f element stored exactly once)
//   db1, [dbc; dbr]: column sums of dt and D, added in row order by one thread per column.
// Plain keeps the 32 rows of [Wc; Wr] in LDS for the whole kernel (108.5 KB of dynamic LDS at C = 128) and NP = 32 is a
// compile-time constant.  Grouped has no room for 128 rows: it stages 32 at a time in the W1 chunk buffer, dt
// accumulating over the tiles in registers, keeps up to four d[Wc; Wr] tiles per wave, and reads D through a column
// table (114.3 KiB at C = 128, A G = 16).  Each workgroup then writes ONE partial [C C + NP C + C + NP] to scratch and
// k_rpn_head_reduce adds the partials in workgroup order: deterministic, no float atomics.
//
// Storage FT of the rows (float, __bf16): the one kernel body per pass is instantiated for both.  bf16 rows are widened
// (exact) on their way into the SAME fp32 LDS images (sA in rpn_hidden_tile, sX in rpn_load_rows), a lane moving
// kRpnVec<FT> = 2 of them, 4 bytes, as it moves one float; from there on no statement knows the storage, so objectness,
// box_regression, `hidden` and the six weight gradients are the fp32 instance's bits on the widened rows.  d_f is the one
// output in FT: the fp32 value the fp32 instance stores is rounded ONCE ((__bf16)x, nearest even).  The bf16 write-out
// goes through the then idle f image sX (one more barrier per tile) so that a lane stores two values and a wave 256
// contiguous bytes; every element is still stored exactly once.  No LDS is added.
//
// Launches: forward 1; backward 2 (main, reduce) -- whatever n_maps.  No weight pack is needed.  All maps empty: no
// launch; backward then zeroes the six weight gradients with memsets.
#include "common.h"

namespace aabr {

constexpr int kRpnT = 64;          // rows per tile
constexpr int kRpnN2 = 32;         // the 8 A output columns, padded to one MFMA tile
constexpr int kRpnMaxMaps = 8;
constexpr int kRpnMaxGroups = 256; // one workgroup per CU of an MI355X; a constant, never read from the device
constexpr int kRpnLD = kRpnT + 2;  // LDS row of a [reduce][64 rows] image
constexpr int kRpnLD2 = kRpnN2 + 2;
constexpr int kRpnMaxN2 = 128;     // with groups: 8 A G <= 128 output columns, up to four MFMA tiles
constexpr int kRpnLDG = kRpnMaxN2 + 2;

struct RpnMaps {
  const void *f[kRpnMaxMaps];      // rows in the storage FT of the instance
  float *obj[kRpnMaxMaps];         // forward: outputs; backward: d_obj (read only, may be NULL)
  float *reg[kRpnMaxMaps];
  void *df[kRpnMaxMaps];           // backward: d_f, in FT
  int64_t rows[kRpnMaxMaps];
  int64_t hoff[kRpnMaxMaps];       // first row of the map in `hidden`
  uint32_t first[kRpnMaxMaps + 1]; // first tile of map m; first[n] = total tiles
  int n;
};

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// elements of row storage FT a lane moves at once: always 4 bytes
template <typename FT> constexpr int kRpnVec = sizeof(float) / sizeof(FT);

__device__ __forceinline__ void rpn_ld(const float *p, float (&x)[1]) { x[0] = *p; }
__device__ __forceinline__ void rpn_ld(const __bf16 *p, float (&x)[2]) {
  const bf16x2 v = *reinterpret_cast<const bf16x2 *>(p);
  x[0] = (float)v[0], x[1] = (float)v[1];
}

__device__ inline int rpn_map_of(const RpnMaps &g, uint32_t tile) {
  int m = 0;
  while (m + 1 < g.n && tile >= g.first[m + 1]) ++m;
  return m;
}

// element (n, k) of the packed [Wc; Wr] block, zero beyond its 8 A rows (A: the rows of Wc, A G with groups)
__device__ inline float rpn_w2(const float *__restrict__ Wc, const float *__restrict__ Wr, int A, int C, int n, int k) {
  if (n < A) return Wc[n * C + k];
  if (n < 8 * A) return Wr[(n - A) * C + k];
  return 0.f;
}

// Packed column n < 8 A G of [Wc; Wr] is row n of Wc (n < A G) or row n - A G of Wr: the reference's channel order,
// a G + g and a 7 G + 7 g + k.  Its value belongs to group g and sits at `off` of a row of that group's slice ([rows, A]
// or [rows, 7 A]); the slices of a map lie group-major behind one pointer.  Without groups: the identity, group 0.
template <bool kGroups>
__device__ inline void rpn_col(int n, int A, int G, int &g, int &off) {
  if constexpr (!kGroups) {
    g = 0, off = n < A ? n : n - A;
  } else if (n < A * G) {
    off = n / G, g = n - off * G;
  } else {
    const int r = n - A * G, a = r / (7 * G), rem = r - a * 7 * G;
    g = rem / 7;
    off = a * 7 + rem - g * 7;
  }
}

// accumulator register r of a 32 x 32 tile: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31
__device__ inline int rpn_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

template <int N>
__device__ __forceinline__ void rpn_zero(f32x16 (&acc)[N]) {
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
}

// acc += L^T R reduced over the tile's 64 sites: pl / pr point at this lane's column of row kh of L [64][ldl], R [64][ldr]
__device__ __forceinline__ void rpn_mma_sites(f32x16 &acc, const float *pl, int ldl, const float *pr, int ldr) {
#pragma unroll 4
  for (int kk = 0; kk < 16; ++kk) {
#pragma unroll
    for (int h = 0; h < kRpnT / 32; ++h) {
      const int r_ = 32 * h + kk;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pl[r_ * ldl], pr[r_ * ldr], acc, 0, 0, 0);
    }
  }
}

// 64 rows of a [.., C] array from `src` (fp32 or bf16, widened) -> sX [64][C + 2], zeros from row `left` on
template <int C, typename T>
__device__ __forceinline__ void rpn_load_rows(float *sX, const T *__restrict__ src, int64_t left) {
  constexpr int V = kRpnVec<T>;
  for (int i = threadIdx.x * V; i < kRpnT * C; i += 256 * V) {
    const int row = i / C, c = i - row * C;             // C is even: the V elements lie in one row
    float x[V] = {};
    if (row < left) rpn_ld(src + (int64_t)row * C + c, x);
#pragma unroll
    for (int v = 0; v < V; ++v) sX[row * (C + 2) + c + v] = x[v];
  }
}

// bf16 only: rows [0, left) of sX [64][C + 2] -> dst [.., C], each value rounded once, two per lane
template <int C>
__device__ __forceinline__ void rpn_store_rows(__bf16 *__restrict__ dst, const float *sX, int64_t left) {
  for (int i = threadIdx.x * 2; i < kRpnT * C; i += 512) {
    const int row = i / C, c = i - row * C;
    if (row < left)
      *reinterpret_cast<bf16x2 *>(dst + (int64_t)row * C + c) =
          (bf16x2){(__bf16)sX[row * (C + 2) + c], (__bf16)sX[row * (C + 2) + c + 1]};
  }
}

// (The other MFMA loop -- 16 steps over a 32-row reduce chunk against the column tiles wn, wn + 2 -- stays written out at
// its four sites: as a function it compiled to 40 more VGPRs in the forward kernels, occupancy 3 -> 2 at C = 96.)

// the first product of a forward tile: t = relu(f W1^T + b1) for the 64 rows from row0 of map m -> sT [hidden unit][row],
// and to `hidden` when that is not NULL.  sA [32][64 + 2], sB >= [32][C + 2].  Ends WITHOUT a barrier.
template <int C, typename FT>
__device__ __forceinline__ void rpn_hidden_tile(const RpnMaps &g, int m, int64_t row0, const float *__restrict__ W1,
                                                const float *__restrict__ b1, float *__restrict__ hidden, float *sA,
                                                float *sB, float *sT) {
  constexpr int NT = C / 32, LDB = C + 2;
  constexpr int V = kRpnVec<FT>, FK = 32 / V, FR = 256 / FK;  // f chunk: lanes per 32-column row, rows per pass
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
  const int l31 = lane & 31, kh = 16 * (lane >> 5), tk = t & 31, tr = t >> 5;
  const int fk = (t & (FK - 1)) * V, fr = t / FK;             // fp32: tk, tr
  const int64_t rows = g.rows[m];
  const FT *__restrict__ f = (const FT *)g.f[m];

  f32x16 acc[2];
  rpn_zero(acc);
  for (int k0 = 0; k0 < C; k0 += 32) {
    __syncthreads();                                  // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < kRpnT / FR; ++i) {
      const int64_t row = row0 + fr + FR * i;
      float x[V] = {};
      if (row < rows) rpn_ld(f + row * C + k0 + fk, x);
#pragma unroll
      for (int v = 0; v < V; ++v) sA[(fk + v) * kRpnLD + fr + FR * i] = x[v];
    }
#pragma unroll
    for (int i = 0; i < C / 8; ++i) sB[tk * LDB + tr + 8 * i] = W1[(tr + 8 * i) * C + k0 + tk];
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {                 // MFMA step kk sums reduce rows kk and kk + 16 of the chunk
      const float a = sA[(kk + kh) * kRpnLD + wm * 32 + l31];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = wn + 2 * jj;
        if (j < NT) acc[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sB[(kk + kh) * LDB + j * 32 + l31], acc[jj], 0, 0, 0);
      }
    }
  }
  // bias and ReLU in registers; t -> LDS [hidden unit][row], and to `hidden` for the backward pass
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int j = wn + 2 * jj;
    if (j >= NT) continue;
    const int col = j * 32 + l31;
    const float bias = b1[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wm * 32 + rpn_acc_row(r, lane);
      float x = acc[jj][r] + bias;
      x = x > 0.f ? x : 0.f;
      sT[col * kRpnLD + row] = x;
      if (hidden != nullptr && row0 + row < rows) hidden[(g.hoff[m] + row0 + row) * C + col] = x;
    }
  }
}

template <int C, bool kGroups, typename FT>
__global__ __launch_bounds__(256) void k_rpn_head_fwd(const RpnMaps g, const float *__restrict__ W1,
                                                      const float *__restrict__ b1, const float *__restrict__ Wc,
                                                      const float *__restrict__ bc, const float *__restrict__ Wr,
                                                      const float *__restrict__ br, int A, int G,
                                                      float *__restrict__ hidden) {
  constexpr int NJ = kGroups ? 2 : 1;                 // accumulators of the second product per wave
  constexpr int LD2 = kGroups ? kRpnLDG : kRpnLD2, LDB = kGroups ? kRpnLDG : C + 2;
  __shared__ float sA[32 * kRpnLD];
  __shared__ float sB[32 * LDB];
  __shared__ float sT[C * kRpnLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
  const int l31 = lane & 31, kh = 16 * (lane >> 5), tk = t & 31, tr = t >> 5;
  const int m = rpn_map_of(g, blockIdx.x);
  const int64_t rows = g.rows[m], row0 = (int64_t)(blockIdx.x - g.first[m]) * kRpnT;
  const int AG = kGroups ? A * G : A, NT2 = kGroups ? (8 * AG + 31) / 32 : 1;
  rpn_hidden_tile<C, FT>(g, m, row0, W1, b1, hidden, sA, sB, sT);

  f32x16 acc2[NJ];
  rpn_zero(acc2);
  for (int k0 = 0; k0 < C; k0 += 32) {
    __syncthreads();                                  // sT is complete; the previous chunk's reads of sB are done
    for (int i = 0; i < 4 * NT2; ++i) sB[tk * LD2 + tr + 8 * i] = rpn_w2(Wc, Wr, AG, C, tr + 8 * i, k0 + tk);
    __syncthreads();
    if (kGroups || wn == 0) {                         // plain: the one tile is the wn = 0 waves'
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        const float a = sT[(k0 + kk + kh) * kRpnLD + wm * 32 + l31];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
          const int j = wn + 2 * jj;
          if (j < NT2) acc2[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sB[(kk + kh) * LD2 + j * 32 + l31], acc2[jj], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < NJ; ++jj) {
    const int col = (wn + 2 * jj) * 32 + l31;
    if (col >= 8 * AG) continue;
    int grp, off;
    rpn_col<kGroups>(col, A, G, grp, off);
    const bool is_obj = col < AG;
    const float bias = is_obj ? bc[col] : br[col - AG];
    const int64_t ld = is_obj ? A : 7 * A;
    float *__restrict__ out = (is_obj ? g.obj[m] : g.reg[m]) + grp * rows * ld + off;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + wm * 32 + rpn_acc_row(r, lane);
      if (row < rows) out[row * ld] = acc2[jj][r] + bias;
    }
  }
}

// floats of one workgroup's partial: dW1 [C][C], d[Wc; Wr] [np][C], db1 [C], [dbc; dbr] [np]; np = the packed columns
// padded to MFMA tiles: 32 without groups
__host__ __device__ constexpr int64_t rpn_partial_floats(int C, int np = kRpnN2) { return (int64_t)C * C + np * C + C + np; }

template <int C, bool kGroups, typename FT>
__global__ __launch_bounds__(256) void k_rpn_head_bwd(const RpnMaps g, const float *__restrict__ W1,
                                                      const float *__restrict__ Wc, const float *__restrict__ Wr, int A,
                                                      int G, const float *__restrict__ hidden, uint32_t total_tiles,
                                                      float *__restrict__ scratch) {
  constexpr int NT = C / 32, LDC = C + 2;
  constexpr int NQ2 = kGroups ? 4 : 1;  // d[Wc; Wr] tiles per wave
  const int AG = kGroups ? A * G : A, NT2 = kGroups ? (8 * AG + 31) / 32 : 1, NP = 32 * NT2, LDD = NP + 2;
  extern __shared__ float smem[];
  float *sX = smem;                     // [64][C + 2]: the t tile, then the f tile
  float *sDT = sX + kRpnT * LDC;        // [64][C + 2]: dt
  float *sB = sDT + kRpnT * LDC;        // [32][C + 2]: a chunk of W1's rows; grouped: before that, 32 rows of [Wc; Wr]
  float *sW2 = sB + 32 * LDC;           // plain only, [32][C + 2]: [Wc; Wr], zero-padded, for the whole kernel
  float *sD = kGroups ? sW2 : sW2 + 32 * LDC;   // [64][NP + 2]: D = [d_obj | d_reg | 0]
  int *sCol = nullptr;                  // grouped only: group << 8 | offset of packed column n; -1 beyond the 8 A G
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave & 1, wn = wave >> 1;
  const int l31 = lane & 31, kh = 16 * (lane >> 5);

  if constexpr (kGroups) {
    __shared__ int s_col[kRpnMaxN2];
    sCol = s_col;
    if (t < kRpnMaxN2) {
      int grp, off, v = -1;
      if (t < 8 * AG) {
        rpn_col<true>(t, A, G, grp, off);
        v = grp << 8 | off;
      }
      sCol[t] = v;
    }
  } else {
    for (int i = t; i < 32 * C; i += 256) {
      const int n = i / C, c = i - n * C;
      sW2[n * LDC + c] = rpn_w2(Wc, Wr, A, C, n, c);
    }
  }

  f32x16 accW1[4], accW2[NQ2], acc[2];
  rpn_zero(accW1);
  rpn_zero(accW2);
  float dbacc = 0.f;                    // thread c < C: db1[c]; thread C + n, n < NP: [dbc; dbr][n]

  for (uint32_t tile = blockIdx.x; tile < total_tiles; tile += gridDim.x) {
    const int m = rpn_map_of(g, tile);
    const int64_t rows = g.rows[m], row0 = (int64_t)(tile - g.first[m]) * kRpnT;
    const float *__restrict__ dobj = g.obj[m];
    const float *__restrict__ dreg = g.reg[m];
    const int64_t left = rows - row0;   // >= 1

    __syncthreads();                    // the previous tile's reads are done (first tile: sW2 / sCol is complete)
    for (int i = t; i < kRpnT * NP; i += 256) {
      const int row = i / NP, n = i - row * NP;
      int64_t grp = 0;
      int off = n < AG ? n : n - AG;
      bool valid = n < 8 * AG;
      if constexpr (kGroups) {
        const int cv = sCol[n];
        valid = cv >= 0, grp = cv >> 8, off = cv & 255;
      }
      float v = 0.f;
      if (row < left && valid) {
        if (n < AG) v = dobj ? dobj[(grp * rows + row0 + row) * A + off] : 0.f;
        else v = dreg ? dreg[(grp * rows + row0 + row) * (7 * A) + off] : 0.f;
      }
      sD[row * LDD + n] = v;
    }
    rpn_load_rows<C>(sX, hidden + (g.hoff[m] + row0) * C, left);
    __syncthreads();

    // d[Wc; Wr] += D^T t: rows n (NP), columns c, reduce over the 64 sites; wave w owns tiles w, w + 4, ... of NT2 x NT
#pragma unroll
    for (int qq = 0; qq < NQ2; ++qq) {
      const int q = wave + 4 * qq;
      if (q >= NT2 * NT) continue;
      const int ni = q / NT, cj = q - ni * NT;
      rpn_mma_sites(accW2[qq], sD + kh * LDD + ni * 32 + l31, LDD, sX + kh * LDC + cj * 32 + l31, LDC);
    }
    if (t >= C && t < C + NP) {
      for (int r_ = 0; r_ < kRpnT; ++r_) dbacc += sD[r_ * LDD + t - C];
    }
    // dt = (D [Wc; Wr]) . (t > 0): rows = sites (wm), columns = hidden units (tiles wn, wn + 2), reduce over n, a
    // 32-row tile of [Wc; Wr] at a time
    rpn_zero(acc);
    for (int nt = 0; nt < NT2; ++nt) {
      const float *w2 = sW2;
      if constexpr (kGroups) {
        if (nt > 0) __syncthreads();    // the previous tile's reads of sB are done
        for (int i = t; i < 32 * C; i += 256) {
          const int n = i / C, c = i - n * C;
          sB[n * LDC + c] = rpn_w2(Wc, Wr, AG, C, nt * 32 + n, c);
        }
        __syncthreads();
        w2 = sB;
      }
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        const float a = sD[(wm * 32 + l31) * LDD + nt * 32 + kk + kh];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int j = wn + 2 * jj;
          if (j < NT) acc[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w2[(kk + kh) * LDC + j * 32 + l31], acc[jj], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = wn + 2 * jj;
      if (j >= NT) continue;
      const int col = j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 32 + rpn_acc_row(r, lane);
        sDT[row * LDC + col] = sX[row * LDC + col] > 0.f ? acc[jj][r] : 0.f;
      }
    }
    __syncthreads();                    // dt is complete; every read of the t tile and of sB is done

    rpn_load_rows<C>(sX, (const FT *)g.f[m] + row0 * C, left);
    if (t < C) {
      for (int r_ = 0; r_ < kRpnT; ++r_) dbacc += sDT[r_ * LDC + t];
    }
    __syncthreads();

    // dW1 += dt^T f: rows c, columns k, reduce over the sites; wave w owns tiles q = w, w + 4, ... of the NT x NT grid
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      const int q = wave + 4 * qq;
      if (q >= NT * NT) continue;
      const int ci = q / NT, kj = q - ci * NT;
      rpn_mma_sites(accW1[qq], sDT + kh * LDC + ci * 32 + l31, LDC, sX + kh * LDC + kj * 32 + l31, LDC);
    }

    // d_f = dt W1: rows = sites, columns k, reduce over the hidden unit c; dt read transposed
    rpn_zero(acc);
    for (int c0 = 0; c0 < C; c0 += 32) {
      __syncthreads();                  // the previous chunk's reads of sB are done
      for (int i = t; i < 32 * C; i += 256) {
        const int cc = i / C, k = i - cc * C;
        sB[cc * LDC + k] = W1[(c0 + cc) * C + k];
      }
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) {
        const float a = sDT[(wm * 32 + l31) * LDC + c0 + kk + kh];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int j = wn + 2 * jj;
          if (j < NT) acc[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sB[(kk + kh) * LDC + j * 32 + l31], acc[jj], 0, 0, 0);
        }
      }
    }
    // fp32: straight from the accumulators.  bf16: through sX -- every wave is past the chunk loop's first barrier, so
    // past its dW1 reads of the f image, and the next tile writes sX only after its opening barrier -- then two per lane
    FT *__restrict__ df = (FT *)g.df[m] + row0 * C;
    constexpr bool kStage = kRpnVec<FT> > 1;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = wn + 2 * jj;
      if (j >= NT) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 32 + rpn_acc_row(r, lane);
        if constexpr (kStage) sX[row * LDC + j * 32 + l31] = acc[jj][r];
        else if (row < left) df[(int64_t)row * C + j * 32 + l31] = acc[jj][r];
      }
    }
    if constexpr (kStage) {
      __syncthreads();
      rpn_store_rows<C>(df, sX, left);
    }
  }

  // this workgroup's partial (a workgroup without a tile writes zeros): dW1, d[Wc; Wr] [NP][C], db1, [dbc; dbr] [NP]
  float *__restrict__ part = scratch + (int64_t)blockIdx.x * rpn_partial_floats(C, NP);
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    const int q = wave + 4 * qq;
    if (q >= NT * NT) continue;
    const int ci = q / NT, kj = q - ci * NT;
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(ci * 32 + rpn_acc_row(r, lane)) * C + kj * 32 + l31] = accW1[qq][r];
  }
#pragma unroll
  for (int qq = 0; qq < NQ2; ++qq) {
    const int q = wave + 4 * qq;
    if (q >= NT2 * NT) continue;
    const int ni = q / NT, cj = q - ni * NT;
#pragma unroll
    for (int r = 0; r < 16; ++r) part[C * C + (ni * 32 + rpn_acc_row(r, lane)) * C + cj * 32 + l31] = accW2[qq][r];
  }
  if (t < C + NP) part[C * C + NP * C + t] = dbacc;
}

// the partials added in workgroup order, stored into the six gradients
// (np = padded packed columns, A = rows of Wc: the anchors, times the groups when there are any)
__global__ __launch_bounds__(256) void k_rpn_head_reduce(const float *__restrict__ scratch, int groups, int C, int A,
                                                         int np, float *__restrict__ dW1, float *__restrict__ db1,
                                                         float *__restrict__ dWc, float *__restrict__ dbc,
                                                         float *__restrict__ dWr, float *__restrict__ dbr) {
  const int64_t per = rpn_partial_floats(C, np);
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  float s = scratch[i];
  for (int p = 1; p < groups; ++p) s += scratch[(int64_t)p * per + i];
  if (i < (int64_t)C * C) {
    dW1[i] = s;
    return;
  }
  i -= (int64_t)C * C;
  if (i < np * C) {
    const int n = (int)(i / C), c = (int)(i - (int64_t)n * C);
    if (n < A) dWc[n * C + c] = s;
    else if (n < 8 * A) dWr[(n - A) * C + c] = s;
    return;
  }
  i -= np * C;
  if (i < C) {
    db1[i] = s;
    return;
  }
  i -= C;
  if (i < A) dbc[i] = s;
  else if (i < 8 * A) dbr[i - A] = s;
}

static bool rpn_c_ok(int C) { return C >= 32 && C <= 128 && C % 32 == 0; }

static bool rpn_groups_ok(int A, int G) { return A >= 1 && A <= 4 && G >= 2 && G <= 8 && A * G <= 16; }

// the packed columns padded to MFMA tiles: 32 at G = 1
static int rpn_np(int A, int G) { return 32 * ((8 * A * G + 31) / 32); }

static size_t rpn_bwd_lds_bytes(int C) { return sizeof(float) * ((size_t)(2 * kRpnT + 64) * (C + 2) + kRpnT * kRpnLD2); }

static size_t rpn_grouped_bwd_lds_bytes(int C, int np) {
  return sizeof(float) * ((size_t)(2 * kRpnT + 32) * (C + 2) + (size_t)kRpnT * (np + 2));
}

} // namespace aabr

using namespace aabr;

extern "C" int aabr_rpn_head_tile_rows(int C) { return rpn_c_ok(C) ? kRpnT : 0; }

extern "C" int aabr_rpn_head_groups(int64_t total_tiles) {
  if (total_tiles < 1) return 0;
  return total_tiles < kRpnMaxGroups ? (int)total_tiles : kRpnMaxGroups;
}

extern "C" int64_t aabr_rpn_head_scratch_floats(int64_t total_tiles, int C, int A) {
  if (total_tiles < 1 || !rpn_c_ok(C) || A < 1 || A > 4) return 0;
  return (int64_t)aabr_rpn_head_groups(total_tiles) * rpn_partial_floats(C);
}

extern "C" int64_t aabr_rpn_head_grouped_scratch_floats(int64_t total_tiles, int C, int A, int G) {
  if (total_tiles < 1 || !rpn_c_ok(C) || !rpn_groups_ok(A, G)) return 0;
  return (int64_t)aabr_rpn_head_groups(total_tiles) * rpn_partial_floats(C, rpn_np(A, G));
}

// checks the caller's records and builds the kernels' table; *total_tiles = 0 when every map is empty
static int rpn_head_table(const AabrRpnMap *maps, int n_maps, int C, int A, bool backward, RpnMaps &g, int64_t *total_tiles) {
  AABR_CHECK_ARG(n_maps >= 1 && n_maps <= kRpnMaxMaps, "n_maps must be 1..8");
  AABR_CHECK_ARG(rpn_c_ok(C), "C must be 32, 64, 96 or 128");
  AABR_CHECK_ARG(A >= 1 && A <= 4, "A must be 1..4");
  AABR_CHECK_ARG(maps, "null pointer");
  g = RpnMaps{};
  g.n = n_maps;
  int64_t tiles = 0, hoff = 0;
  for (int m = 0; m < n_maps; ++m) {
    const AabrRpnMap &q = maps[m];
    AABR_CHECK_ARG(q.rows >= 0, "negative row count");
    AABR_CHECK_ARG(q.rows <= (1LL << 40) / C, "map too large");
    if (q.rows > 0) {
      AABR_CHECK_ARG(q.features, "null features");
      if (backward) AABR_CHECK_ARG(q.d_features, "null d_features");
      else AABR_CHECK_ARG(q.objectness && q.box_regression, "null output");
      // a lane moves 4 bytes of a row whatever the storage (one float, two bf16)
      AABR_CHECK_ARG((((uintptr_t)q.features | (uintptr_t)(backward ? q.d_features : nullptr)) & 3) == 0,
                     "features / d_features must be 4-byte aligned");
    }
    g.f[m] = q.features, g.obj[m] = q.objectness, g.reg[m] = q.box_regression, g.df[m] = q.d_features;
    g.rows[m] = q.rows, g.hoff[m] = hoff;
    AABR_CHECK_ARG(tiles < (1LL << 31) - 1, "too many tiles");
    g.first[m] = (uint32_t)tiles;
    tiles += ceil_div(q.rows, kRpnT);
    hoff += q.rows;
  }
  AABR_CHECK_ARG(tiles < (1LL << 31) - 1, "too many tiles");
  for (int m = n_maps; m <= kRpnMaxMaps; ++m) g.first[m] = (uint32_t)tiles;
  *total_tiles = tiles;
  return AABR_OK;
}

// one case per C of a launcher template <int C, bool kGroups, typename FT>, plain or grouped by the run-time flag, FT the
// caller's
#define AABR_RPN_DISPATCH(rc, launcher, ...)                                                                            \
  switch (C) {                                                                                                          \
  case 32: rc = grouped ? launcher<32, true, FT>(__VA_ARGS__) : launcher<32, false, FT>(__VA_ARGS__); break;           \
  case 64: rc = grouped ? launcher<64, true, FT>(__VA_ARGS__) : launcher<64, false, FT>(__VA_ARGS__); break;           \
  case 96: rc = grouped ? launcher<96, true, FT>(__VA_ARGS__) : launcher<96, false, FT>(__VA_ARGS__); break;           \
  default: rc = grouped ? launcher<128, true, FT>(__VA_ARGS__) : launcher<128, false, FT>(__VA_ARGS__); break;         \
  }

template <int C, bool kGroups, typename FT>
static int rpn_head_fwd_launch(const RpnMaps &g, const float *W1, const float *b1, const float *Wc, const float *bc,
                               const float *Wr, const float *br, int A, int G, float *hidden, int64_t tiles,
                               hipStream_t st) {
  hipLaunchKernelGGL((k_rpn_head_fwd<C, kGroups, FT>), dim3((unsigned)tiles), dim3(256), 0, st, g, W1, b1, Wc, bc, Wr, br, A,
                     G, hidden);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

template <int C, bool kGroups, typename FT>
static int rpn_head_bwd_launch(const RpnMaps &g, const float *W1, const float *Wc, const float *Wr, int A, int G,
                               const float *hidden, int64_t tiles, int groups, float *scratch, hipStream_t st) {
  static DynLdsOnce attr;               // grouped: once, for the widest D; the launch asks for what its A G needs
  const size_t lds_max = kGroups ? rpn_grouped_bwd_lds_bytes(C, kRpnMaxN2) : rpn_bwd_lds_bytes(C);
  const size_t lds = kGroups ? rpn_grouped_bwd_lds_bytes(C, rpn_np(A, G)) : rpn_bwd_lds_bytes(C);
  AABR_CHECK_HIP(dyn_lds_once(attr, (const void *)(k_rpn_head_bwd<C, kGroups, FT>), (int)lds_max));
  hipLaunchKernelGGL((k_rpn_head_bwd<C, kGroups, FT>), dim3((unsigned)groups), dim3(256), lds, st, g, W1, Wc, Wr, A, G,
                     hidden, (uint32_t)tiles, scratch);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// the forward of both forms (G = 1, grouped = false: the plain entry) and both row storages; the entries have checked A
// and G
template <typename FT>
static int rpn_head_forward(const char *fn, const AabrRpnMap *maps_host, int n_maps, int C, int A, int G, bool grouped,
                            const float *W1, const float *b1, const float *Wc, const float *bc, const float *Wr,
                            const float *br, float *hidden, hipStream_t st) {
  RpnMaps g;
  int64_t tiles = 0;
  int rc = rpn_head_table(maps_host, n_maps, C, A, false, g, &tiles);
  if (rc != AABR_OK) return rc;
  AABR_CHECK_ARG_AS(fn, W1 && b1 && Wc && bc && Wr && br, "null pointer");
  if (tiles == 0) return AABR_OK;
  AABR_RPN_DISPATCH(rc, rpn_head_fwd_launch, g, W1, b1, Wc, bc, Wr, br, A, G, hidden, tiles, st);
  return rc;
}

template <typename FT>
static int rpn_head_backward(const char *fn, const AabrRpnMap *maps_host, int n_maps, int C, int A, int G, bool grouped,
                             const float *W1, const float *Wc, const float *Wr, const float *hidden, float *dW1,
                             float *db1, float *dWc, float *dbc, float *dWr, float *dbr, float *scratch, hipStream_t st) {
  RpnMaps g;
  int64_t tiles = 0;
  int rc = rpn_head_table(maps_host, n_maps, C, A, true, g, &tiles);
  if (rc != AABR_OK) return rc;
  AABR_CHECK_ARG_AS(fn, W1 && Wc && Wr, "null pointer");
  AABR_CHECK_ARG_AS(fn, dW1 && db1 && dWc && dbc && dWr && dbr, "null gradient pointer");
  const int AG = A * G;
  if (tiles == 0) {                                   // empty sums: zeros, no kernel
    AABR_CHECK_HIP(hipMemsetAsync(dW1, 0, sizeof(float) * C * C, st));
    AABR_CHECK_HIP(hipMemsetAsync(db1, 0, sizeof(float) * C, st));
    AABR_CHECK_HIP(hipMemsetAsync(dWc, 0, sizeof(float) * AG * C, st));
    AABR_CHECK_HIP(hipMemsetAsync(dbc, 0, sizeof(float) * AG, st));
    AABR_CHECK_HIP(hipMemsetAsync(dWr, 0, sizeof(float) * 7 * AG * C, st));
    AABR_CHECK_HIP(hipMemsetAsync(dbr, 0, sizeof(float) * 7 * AG, st));
    return AABR_OK;
  }
  AABR_CHECK_ARG_AS(fn, hidden, "null hidden");
  AABR_CHECK_ARG_AS(fn, scratch, "null scratch");
  const int groups = aabr_rpn_head_groups(tiles), np = rpn_np(A, G);
  AABR_RPN_DISPATCH(rc, rpn_head_bwd_launch, g, W1, Wc, Wr, A, G, hidden, tiles, groups, scratch, st);
  if (rc != AABR_OK) return rc;
  hipLaunchKernelGGL(k_rpn_head_reduce, dim3((unsigned)ceil_div(rpn_partial_floats(C, np), 256)), dim3(256), 0, st, scratch,
                     groups, C, AG, np, dW1, db1, dWc, dbc, dWr, dbr);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

#define AABR_RPN_CHECK_GROUPS(A, G)                                                                                     \
  AABR_CHECK_ARG((A) >= 1 && (A) <= 4, "A must be 1..4");                                                               \
  AABR_CHECK_ARG(rpn_groups_ok(A, G), "groups: 2 <= G <= 8 and A G <= 16")

// the four entry points of one row storage FT: aabr_rpn_head_{,grouped_}{forward,backward}<SUFFIX>
#define AABR_RPN_ENTRIES(SUFFIX, FT)                                                                                    \
  extern "C" int aabr_rpn_head_forward##SUFFIX(const AabrRpnMap *maps_host, int n_maps, int C, int A, const float *W1,  \
                                               const float *b1, const float *Wc, const float *bc, const float *Wr,      \
                                               const float *br, float *hidden, void *stream_) {                         \
    return rpn_head_forward<FT>(__func__, maps_host, n_maps, C, A, 1, false, W1, b1, Wc, bc, Wr, br, hidden,            \
                                (hipStream_t)stream_);                                                                  \
  }                                                                                                                     \
  extern "C" int aabr_rpn_head_backward##SUFFIX(const AabrRpnMap *maps_host, int n_maps, int C, int A, const float *W1, \
                                                const float *Wc, const float *Wr, const float *hidden, float *dW1,      \
                                                float *db1, float *dWc, float *dbc, float *dWr, float *dbr,             \
                                                float *scratch, void *stream_) {                                        \
    return rpn_head_backward<FT>(__func__, maps_host, n_maps, C, A, 1, false, W1, Wc, Wr, hidden, dW1, db1, dWc, dbc,   \
                                 dWr, dbr, scratch, (hipStream_t)stream_);                                              \
  }                                                                                                                     \
  extern "C" int aabr_rpn_head_grouped_forward##SUFFIX(const AabrRpnMap *maps_host, int n_maps, int C, int A, int G,    \
                                                       const float *W1, const float *b1, const float *Wc,               \
                                                       const float *bc, const float *Wr, const float *br,               \
                                                       float *hidden, void *stream_) {                                  \
    AABR_RPN_CHECK_GROUPS(A, G);                                                                                        \
    return rpn_head_forward<FT>(__func__, maps_host, n_maps, C, A, G, true, W1, b1, Wc, bc, Wr, br, hidden,             \
                                (hipStream_t)stream_);                                                                  \
  }                                                                                                                     \
  extern "C" int aabr_rpn_head_grouped_backward##SUFFIX(const AabrRpnMap *maps_host, int n_maps, int C, int A, int G,   \
                                                        const float *W1, const float *Wc, const float *Wr,              \
                                                        const float *hidden, float *dW1, float *db1, float *dWc,        \
                                                        float *dbc, float *dWr, float *dbr, float *scratch,             \
                                                        void *stream_) {                                                \
    AABR_RPN_CHECK_GROUPS(A, G);                                                                                        \
    return rpn_head_backward<FT>(__func__, maps_host, n_maps, C, A, G, true, W1, Wc, Wr, hidden, dW1, db1, dWc, dbc,    \
                                 dWr, dbr, scratch, (hipStream_t)stream_);                                              \
  }

AABR_RPN_ENTRIES(, float)
AABR_RPN_ENTRIES(_bf16, __bf16) // AabrRpnMap.features / .d_features point at bf16 rows

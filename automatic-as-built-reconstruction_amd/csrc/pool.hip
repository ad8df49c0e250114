// pool.hip -- MaxPooling, AveragePooling and UnPooling (SCN/CPU/MaxPooling.cpp, AveragePooling.cpp, UnPooling.cpp of the
// reference), forward and backward: six passes, each ONE gather over one of the two tables of a strided rule book
// (geometry.hip / brick.hip: table[vol][rows], the source row per destination row and filter offset, -1 where absent).
//
//   dst[r, c] = reduce over offsets o = 0 .. vol-1 in ascending order, for t[o, r] >= 0, of term(o, r, c)
//
//   MAX0     acc starts at +0.0f; x = src[t[o, r], col0 + c]; if (acc < x) acc = x      (the reference's rule over its
//            zero-filled output: the result is max(0, inputs) and a NaN input is ignored)
//   SUM      acc += x / div (one correctly rounded fp32 division per term, then an fp32 add; -ffp-contract=off), or
//            acc += x when div == 0 (UnPooling)
//   MAXGRAD  acc += dy[t[o, r], c] where y[t[o, r], c] == x[r, col0 + c] (every tied input receives the gradient,
//            +0.0 == -0.0, a NaN never matches); run over the book's input-side table
//
// Ascending offsets is the order of the reference's offset-major rule lists, in which a row appears at most once per offset:
// with fp32 storage the results are the reference's CPU results bit for bit.  bf16 storage is widened (exact), the same
// fp32 operations run, and the store rounds once to nearest even; MAXGRAD compares the stored values.
//
// Gather form: every destination element is written exactly once by one lane -- no atomics, no memset, no host read, one
// launch per pass, the same bytes run to run.  Columns of the destination outside [dst_col0, dst_col0 + planes) (the
// dropped leading planes of an input gradient) are written 0 by the same launch.
//
// Work layout: 256 threads = 4 waves.  `lpr` = 2^k lanes serve one row (lanes along the planes of the row: 16 bytes per
// lane on the vector path -- 4 fp32 / 8 bf16 planes -- when planes, column offsets and row strides are all multiples of
// the vector width and the bases are 16-byte aligned; one plane per lane otherwise), so a wave serves rpw = 64 / lpr
// consecutive rows.  The wave's table entries t[o .. o + lpr - 1, row0 .. row0 + rpw - 1] are read by ONE load instruction
// (lane = offset * rpw + row: rpw contiguous words per offset) and handed to the lanes of each row by a wave shuffle -- no
// lane reads the table per plane, and no LDS.  Rows are int64-indexed; rows * planes may exceed 2^31.
#include "common.h"

namespace aabr {
namespace {

constexpr int kPoolThreads = 256;
enum PoolMode { kPoolMax0 = 0, kPoolSum = 1 };

template <typename T> struct PoolVecWidth;                 // elements of T in 16 bytes
template <> struct PoolVecWidth<float> { static constexpr int value = 4; };
template <> struct PoolVecWidth<__bf16> { static constexpr int value = 8; };

template <typename T, int W> struct alignas(sizeof(T) * W) PoolPack { T v[W]; };

// where the lane stands in its wave, as a server of a row's planes and as a reader of the table
struct PoolLane {
  int rw, cl;          // row in the wave, lane in the row
  int lo, lr;          // table reader: offset in the chunk of lpr offsets, row in the wave
  int lpr, rpw, sh;    // lanes per row, rows per wave, log2(rpw)
  int64_t wrow0;       // first row of the wave
};
__device__ __forceinline__ PoolLane pool_lane(int lpr_log2) {
  PoolLane p;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  p.lpr = 1 << lpr_log2;
  p.sh = 6 - lpr_log2;
  p.rpw = 1 << p.sh;
  p.rw = lane >> lpr_log2;
  p.cl = lane & (p.lpr - 1);
  p.lo = lane >> p.sh;
  p.lr = lane & (p.rpw - 1);
  p.wrow0 = ((int64_t)blockIdx.x * (kPoolThreads / 64) + wave) * p.rpw;
  return p;
}
// the wave's entries of offsets o0 .. o0 + lpr - 1: one coalesced load, -1 beyond the table
__device__ __forceinline__ int32_t pool_table_chunk(const int32_t *__restrict__ table, int vol, int64_t rows, int o0,
                                                    const PoolLane &p) {
  const int o = o0 + p.lo;
  const int64_t r = p.wrow0 + p.lr;
  return (o < vol && r < rows) ? table[(int64_t)o * rows + r] : -1;
}
// entry of offset o0 + k for this lane's row (every lane of the wave calls this)
__device__ __forceinline__ int32_t pool_entry(int32_t chunk, int k, int kmax, const PoolLane &p) {
  const int32_t e = __shfl(chunk, ((k << p.sh) + p.rw) & 63);
  return k < kmax ? e : -1;
}

template <typename T, int W>
__device__ __forceinline__ void pool_store(T *dst, const float (&acc)[W]) {
  PoolPack<T, W> o;
#pragma unroll
  for (int w = 0; w < W; ++w) o.v[w] = (T)acc[w];     // bf16: the one round-to-nearest-even
  *reinterpret_cast<PoolPack<T, W> *>(dst) = o;
}

// zeros in the destination columns outside [c0, c0 + planes)
template <typename T>
__device__ __forceinline__ void pool_zero_outside(T *drow, int c0, int planes, int width, const PoolLane &p) {
  for (int c = p.cl; c < width; c += p.lpr)
    if (c < c0 || c >= c0 + planes) drow[c] = (T)0.0f;
}

template <typename T, int W, int MODE, bool DIV>
__global__ void __launch_bounds__(kPoolThreads)
k_pool_gather(const T *__restrict__ src, int64_t src_stride, int col0, int planes, const int32_t *__restrict__ table,
              int vol, int64_t rows, float div, T *__restrict__ dst, int64_t dst_stride, int dst_col0, int dst_width,
              int lpr_log2) {
  const PoolLane p = pool_lane(lpr_log2);
  const int64_t row = p.wrow0 + p.rw;
  const bool row_ok = row < rows;
  const int units = planes / W;
  for (int u0 = 0; u0 < units; u0 += p.lpr) {             // (wave-uniform bounds: the shuffles need every lane)
    const int u = u0 + p.cl;
    const bool act = row_ok && u < units;
    const T *scol = src + col0 + u * W;
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0f;
    for (int o0 = 0; o0 < vol; o0 += p.lpr) {
      const int32_t chunk = pool_table_chunk(table, vol, rows, o0, p);
      const int kmax = vol - o0 < p.lpr ? vol - o0 : p.lpr;
      for (int k0 = 0; k0 < kmax; k0 += 4) {
        int32_t e[4];
        PoolPack<T, W> x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // four gathers in flight
          e[j] = pool_entry(chunk, k0 + j, kmax, p);
          if (!act) e[j] = -1;
          if (e[j] >= 0) x[j] = *reinterpret_cast<const PoolPack<T, W> *>(scol + (int64_t)e[j] * src_stride);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {                      // reduced in ascending offset
          if (e[j] < 0) continue;
#pragma unroll
          for (int w = 0; w < W; ++w) {
            const float v = (float)x[j].v[w];
            if (MODE == kPoolMax0) {
              if (acc[w] < v) acc[w] = v;
            } else if (DIV) {
              acc[w] += v / div;
            } else {
              acc[w] += v;
            }
          }
        }
      }
    }
    if (act) pool_store<T, W>(dst + row * dst_stride + dst_col0 + u * W, acc);
  }
  if (row_ok && dst_width > planes) pool_zero_outside(dst + row * dst_stride, dst_col0, planes, dst_width, p);
}

// MaxPooling backward over the input-side table: x [rows, x_stride] read at columns [col0, col0 + planes), y and dy
// [*, planes], dx [rows, x_stride] with zeros in its first col0 columns
template <typename T, int W>
__global__ void __launch_bounds__(kPoolThreads)
k_pool_max_backward(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ dy, int64_t x_stride, int col0,
                    int planes, const int32_t *__restrict__ table, int vol, int64_t rows, T *__restrict__ dx,
                    int lpr_log2) {
  const PoolLane p = pool_lane(lpr_log2);
  const int64_t row = p.wrow0 + p.rw;
  const bool row_ok = row < rows;
  const int units = planes / W;
  for (int u0 = 0; u0 < units; u0 += p.lpr) {
    const int u = u0 + p.cl;
    const bool act = row_ok && u < units;
    PoolPack<T, W> xv;
    if (act) xv = *reinterpret_cast<const PoolPack<T, W> *>(x + row * x_stride + col0 + u * W);
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0f;
    for (int o0 = 0; o0 < vol; o0 += p.lpr) {
      const int32_t chunk = pool_table_chunk(table, vol, rows, o0, p);
      const int kmax = vol - o0 < p.lpr ? vol - o0 : p.lpr;
      for (int k0 = 0; k0 < kmax; k0 += 4) {
        int32_t e[4];
        PoolPack<T, W> yv[4], gv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          e[j] = pool_entry(chunk, k0 + j, kmax, p);
          if (!act) e[j] = -1;
          if (e[j] >= 0) {
            const int64_t at = (int64_t)e[j] * planes + u * W;
            yv[j] = *reinterpret_cast<const PoolPack<T, W> *>(y + at);
            gv[j] = *reinterpret_cast<const PoolPack<T, W> *>(dy + at);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (e[j] < 0) continue;
#pragma unroll
          for (int w = 0; w < W; ++w)
            if ((float)yv[j].v[w] == (float)xv.v[w]) acc[w] += (float)gv[j].v[w];
        }
      }
    }
    if (act) pool_store<T, W>(dx + row * x_stride + col0 + u * W, acc);
  }
  if (row_ok && col0 > 0) pool_zero_outside(dx + row * x_stride, col0, planes, (int)x_stride, p);
}

// lanes per row: the smallest power of two that covers the row's units, at most a wave
int pool_lpr_log2(int units) {
  int l = 0;
  while (l < 6 && (1 << l) < units) ++l;
  return l;
}
// blocks of a launch over `rows` rows, or 0 when the grid would not fit
int64_t pool_grid(int64_t rows, int lpr_log2) {
  const int64_t rpb = (int64_t)(kPoolThreads / 64) * (64 >> lpr_log2);
  const int64_t g = (rows + rpb - 1) / rpb;
  return g <= 0x7fffffff ? g : 0;
}
bool pool_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T, int W>
void launch_pool_gather(const void *src, int64_t src_stride, int col0, int planes, const int32_t *table, int vol,
                        int64_t rows, int mode, float div, void *dst, int64_t dst_stride, int dst_col0, int dst_width,
                        unsigned grid, int lpr_log2, hipStream_t st) {
  const T *s = static_cast<const T *>(src);
  T *d = static_cast<T *>(dst);
#define AABR_POOL_LAUNCH(MODE, DIV)                                                                                  \
  hipLaunchKernelGGL((k_pool_gather<T, W, MODE, DIV>), dim3(grid), dim3(kPoolThreads), 0, st, s, src_stride, col0,    \
                     planes, table, vol, rows, div, d, dst_stride, dst_col0, dst_width, lpr_log2)
  if (mode == kPoolMax0)
    AABR_POOL_LAUNCH(kPoolMax0, false);
  else if (div != 0.0f)
    AABR_POOL_LAUNCH(kPoolSum, true);
  else
    AABR_POOL_LAUNCH(kPoolSum, false);
#undef AABR_POOL_LAUNCH
}

} // namespace
} // namespace aabr

extern "C" int aabr_pool_gather(const void *src, int bf16, int64_t src_stride, int col0, int planes,
                                const int32_t *table, int vol, int64_t rows_dst, int mode, float div, void *dst,
                                int64_t dst_stride, int dst_col0, int dst_width, void *stream) {
  using namespace aabr;
  AABR_CHECK_ARG(planes > 0, "planes must be positive");
  AABR_CHECK_ARG(vol > 0, "vol must be positive");
  AABR_CHECK_ARG(mode == kPoolMax0 || mode == kPoolSum, "mode must be 0 (MAX0) or 1 (SUM)");
  AABR_CHECK_ARG(rows_dst >= 0, "negative row count");
  AABR_CHECK_ARG(col0 >= 0 && src_stride >= (int64_t)col0 + planes, "source columns outside the source row");
  AABR_CHECK_ARG(dst_col0 >= 0 && dst_width >= dst_col0 + planes && dst_stride >= dst_width,
                 "destination columns outside the destination row");
  AABR_CHECK_ARG(div >= 0.0f, "div must be 0 (no division) or positive");
  AABR_CHECK_ARG(rows_dst == 0 || (src && table && dst), "null pointer");
  if (rows_dst == 0) return AABR_OK;
  const int vw = bf16 ? PoolVecWidth<__bf16>::value : PoolVecWidth<float>::value;
  const bool vec = planes % vw == 0 && col0 % vw == 0 && src_stride % vw == 0 && dst_stride % vw == 0 &&
                   dst_col0 % vw == 0 && pool_aligned16(src) && pool_aligned16(dst);
  const int lpr_log2 = pool_lpr_log2(vec ? planes / vw : planes);
  const int64_t grid = pool_grid(rows_dst, lpr_log2);
  AABR_CHECK_ARG(grid > 0, "too many rows for one launch");
  hipStream_t st = (hipStream_t)stream;
#define AABR_POOL_GO(T, W)                                                                                            \
  launch_pool_gather<T, W>(src, src_stride, col0, planes, table, vol, rows_dst, mode, div, dst, dst_stride, dst_col0, \
                           dst_width, (unsigned)grid, lpr_log2, st)
  if (bf16) {
    if (vec) AABR_POOL_GO(__bf16, 8); else AABR_POOL_GO(__bf16, 1);
  } else {
    if (vec) AABR_POOL_GO(float, 4); else AABR_POOL_GO(float, 1);
  }
#undef AABR_POOL_GO
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_pool_max_backward(const void *x, const void *y, const void *dy, int bf16, int64_t x_stride, int col0,
                                      int planes, const int32_t *table_in, int vol, int64_t rows_in, void *dx,
                                      void *stream) {
  using namespace aabr;
  AABR_CHECK_ARG(planes > 0, "planes must be positive");
  AABR_CHECK_ARG(vol > 0, "vol must be positive");
  AABR_CHECK_ARG(rows_in >= 0, "negative row count");
  AABR_CHECK_ARG(col0 >= 0 && x_stride == (int64_t)col0 + planes, "x_stride must be col0 + planes");
  AABR_CHECK_ARG(rows_in == 0 || (x && y && dy && table_in && dx), "null pointer");
  if (rows_in == 0) return AABR_OK;
  const int vw = bf16 ? PoolVecWidth<__bf16>::value : PoolVecWidth<float>::value;
  const bool vec = planes % vw == 0 && col0 % vw == 0 && pool_aligned16(x) && pool_aligned16(y) && pool_aligned16(dy) &&
                   pool_aligned16(dx);
  const int lpr_log2 = pool_lpr_log2(vec ? planes / vw : planes);
  const int64_t grid = pool_grid(rows_in, lpr_log2);
  AABR_CHECK_ARG(grid > 0, "too many rows for one launch");
  hipStream_t st = (hipStream_t)stream;
#define AABR_POOL_GO(T, W)                                                                                           \
  hipLaunchKernelGGL((k_pool_max_backward<T, W>), dim3((unsigned)grid), dim3(kPoolThreads), 0, st,                    \
                     static_cast<const T *>(x), static_cast<const T *>(y), static_cast<const T *>(dy), x_stride, col0, \
                     planes, table_in, vol, rows_in, static_cast<T *>(dx), lpr_log2)
  if (bf16) {
    if (vec) AABR_POOL_GO(__bf16, 8); else AABR_POOL_GO(__bf16, 1);
  } else {
    if (vec) AABR_POOL_GO(float, 4); else AABR_POOL_GO(float, 1);
  }
#undef AABR_POOL_GO
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// conv_dw.hip -- the weight gradient of the sparse convolution (gfx950): dW[k] = sum over offset k's rules (i, o) of
// in[i]^T d_out[o], and d_bias = column sums of d_out, over the offset-major pair list conv.hip builds (offset_pairs.h).
// conv_dw_tiles.h decides which kernel runs with what grid and which reduce follows; this file holds the kernels, one
// table row per compiled instance and the entry points that carry the decision out.  Every sum has a fixed order (pairs
// ascending, waves / chunks / workgroups in index order): bit-reproducible, no atomics.
#include "common.h"
#include "conv_dw_tiles.h"  // dw_chunk, DwKnobs, conv_dw_launch: the launch decision
#include "offset_pairs.h"   // op_hdr, op_nb256, dw_chunk_range: the pair list's layout and its chunks

namespace aabr {

extern thread_local const char *g_last_variant; // conv.hip

// ----------------------------------------------------------------------------- dW
// partial[chunk][c][n] = sum over the chunk's pairs (t, o) of in[t][c] * d_out[o][n]; one workgroup
// per chunk of dw_chunk(V, vol) pairs of one offset (each wave a quarter), MFMA with the pair index as the
// reduction dimension.  Pair indices are loaded 64 at a time (coalesced) and handed to the lane
// groups by shuffles; 16 pairs are gathered per step before their MFMAs issue.  The four waves'
// accumulators are summed through LDS in wave order (deterministic).  CB x NB blocks of 16.
__device__ inline float ldf(const float *p, int64_t i) { return p[i]; }
__device__ inline float ldf(const __bf16 *p, int64_t i) { return (float)p[i]; }

// Form of the launch (bits 1 and 2 of `form`, bit 0 = direct; dw_vec_operands in conv_dw_tiles.h, fp32 storage only): an
// operand in the VECTOR form has lane (g, c16) load its CB (NB) consecutive channels CB c16 + a with one dwordx4 / dwordx2
// instead of one dword per 16-channel block -- a quarter of the load instructions through the vector L1, whole 256-byte
// row slices per instruction -- and block a then holds the channels {CB i + a}; the sums and their order are the same,
// the write-out maps the accumulators back (dw_tile_row / dw_tile_col).  Bit 3: a lane's four columns of a row are
// contiguous and 16-byte aligned in the destination, one 16-byte store.  The form is chosen once per launch, outside the
// pair loop: one copy of the loop per combination the instance can meet.
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int N> __device__ inline void ld_row(float (&d)[N], const float *p) {
  if constexpr (N == 4) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(p);
    d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
  } else if constexpr (N == 2) {
    const f32x2 v = *reinterpret_cast<const f32x2 *>(p);
    d[0] = v[0]; d[1] = v[1];
  } else d[0] = p[0];
}
template <int N> __device__ inline void ld_row(__bf16 (&)[N], const __bf16 *) {}   // (never called: bf16 keeps the scalar form)
template <bool V> struct DwForm { static constexpr bool value = V; };

template <int CB, int NB, typename T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_conv_dw_pairs(const T *__restrict__ in, int ci,
                                                       const T *__restrict__ d_out, int co, int64_t V,
                                                       const int32_t *__restrict__ words, int vol,
                                                       int chunk_pairs, float *__restrict__ partial, int form) {
  __shared__ f32x4 red[CB * NB][64];
  constexpr bool kF32 = sizeof(T) == 4;
  const int direct = form & 1;
  const bool vin = kF32 && CB > 1 && (form & (kDwVecIn << 1)), vout = kF32 && NB > 1 && (form & (kDwVecOut << 1));
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c16 = lane & 15;
  const int nnb = nnb_of(co);
  const int tiles_n = (nnb + NB - 1) / NB;
  const int tile = blockIdx.y;
  const int cb0 = (tile / tiles_n) * CB, nb0 = (tile % tiles_n) * NB;
  const int chunk = blockIdx.x;
  int k, c0, c1;                                           // the chunk's offset and pair range; each wave a quarter
  if (!dw_chunk_range(words, vol, chunk_pairs, direct, chunk, lane, k, c0, c1)) return;
  const int rk = words[k];
  const int p0 = c0 + wave * (chunk_pairs / 4);
  int p1 = p0 + chunk_pairs / 4;
  if (p1 > c1) p1 = c1;
  const int2 *pairs = reinterpret_cast<const int2 *>(words + op_hdr(vol) + (int64_t)vol * op_nb256(V)) +
                      (int64_t)k * V;
  f32x4 acc[CB][NB];
#pragma unroll
  for (int a = 0; a < CB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Software pipeline: the rows of the NEXT group of 16 pairs are in flight while the current group's
  // MFMAs issue (two register sets, static alternation: a block of 64 pairs is four groups).  All loads
  // are unconditional from clamped addresses and masked at use, so the waits stay counted.
  const int cA = ci - 1, nA = co - 1;
  int ca[CB], na[NB];
#pragma unroll
  for (int a = 0; a < CB; ++a) { int c = (cb0 + a) * 16 + c16; ca[a] = c < ci ? c : cA; }
#pragma unroll
  for (int b = 0; b < NB; ++b) { int n = (nb0 + b) * 16 + c16; na[b] = n < co ? n : nA; }
  const int cv = cb0 * 16 + CB * c16, nv = nb0 * 16 + NB * c16;   // vector form: the lane's first channel (every tile full)
  auto run = [&](auto va_, auto vb_) {
    constexpr bool VA = decltype(va_)::value, VB = decltype(vb_)::value;
    auto gather = [&](T (&av)[4][CB], T (&bv)[4][NB], int2 pr, int q0) {
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int src = q0 + st * 4 + g;
        int tq = __shfl(pr.x, src), oq = __shfl(pr.y, src);
        tq = tq < 0 ? 0 : tq; oq = oq < 0 ? 0 : oq;
        if constexpr (VA) ld_row<CB>(av[st], in + (int64_t)tq * ci + cv);
        else {
#pragma unroll
          for (int a = 0; a < CB; ++a) av[st][a] = in[(int64_t)tq * ci + ca[a]];
        }
        if constexpr (VB) ld_row<NB>(bv[st], d_out + (int64_t)oq * co + nv);
        else {
#pragma unroll
          for (int b = 0; b < NB; ++b) bv[st][b] = d_out[(int64_t)oq * co + na[b]];
        }
      }
    };
    auto mfmas = [&](T (&av)[4][CB], T (&bv)[4][NB], int qbase) {
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const bool on = qbase + st * 4 + g < p1;
        float fa[CB], fb[NB];
#pragma unroll
        for (int a = 0; a < CB; ++a) fa[a] = (on && (VA || (cb0 + a) * 16 + c16 < ci)) ? (float)av[st][a] : 0.0f;
#pragma unroll
        for (int b = 0; b < NB; ++b) fb[b] = (on && (VB || (nb0 + b) * 16 + c16 < co)) ? (float)bv[st][b] : 0.0f;
#pragma unroll
        for (int a = 0; a < CB; ++a)
#pragma unroll
          for (int b = 0; b < NB; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
    };
    T avA[4][CB], bvA[4][NB], avB[4][CB], bvB[4][NB];
    const int last = rk - 1;                                 // rk >= 1 here
    auto load_pr = [&](int q64) {
      int q = q64 + lane;
      int2 v = pairs[q < rk ? q : last];
      return (q < p1) ? v : make_int2(-1, -1);
    };
    int2 pr = load_pr(p0);
    gather(avA, bvA, pr, 0);
    for (int q64 = p0; q64 < p1; q64 += 64) {
      int2 prn = load_pr(q64 + 64);
      __builtin_amdgcn_sched_barrier(0);
      gather(avB, bvB, pr, 16);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(avA, bvA, q64);
      __builtin_amdgcn_sched_barrier(0);
      gather(avA, bvA, pr, 32);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(avB, bvB, q64 + 16);
      __builtin_amdgcn_sched_barrier(0);
      gather(avB, bvB, pr, 48);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(avA, bvA, q64 + 32);
      __builtin_amdgcn_sched_barrier(0);
      gather(avA, bvA, prn, 0);
      __builtin_amdgcn_sched_barrier(0);
      mfmas(avB, bvB, q64 + 48);
      pr = prn;
    }
  };
  if (p0 < p1) {                                             // (wave-uniform, and so is the form)
    if constexpr (kF32 && CB > 1 && NB > 1) {
      if (vin && vout) run(DwForm<true>{}, DwForm<true>{});
      else if (vin) run(DwForm<true>{}, DwForm<false>{});
      else if (vout) run(DwForm<false>{}, DwForm<true>{});
      else run(DwForm<false>{}, DwForm<false>{});
    } else if constexpr (kF32 && CB > 1) {
      if (vin) run(DwForm<true>{}, DwForm<false>{});
      else run(DwForm<false>{}, DwForm<false>{});
    } else if constexpr (kF32 && NB > 1) {
      if (vout) run(DwForm<false>{}, DwForm<true>{});
      else run(DwForm<false>{}, DwForm<false>{});
    } else run(DwForm<false>{}, DwForm<false>{});
  }
  // sum the four waves' accumulators in wave order: w0 + w1 + w2 + w3
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < CB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (w == 0) red[a * NB + b][lane] = acc[a][b];
          else {
            f32x4 t = red[a * NB + b][lane];
            t[0] += acc[a][b][0]; t[1] += acc[a][b][1]; t[2] += acc[a][b][2]; t[3] += acc[a][b][3];
            red[a * NB + b][lane] = t;
          }
        }
    }
    __syncthreads();
  }
  if (wave != 0) return;
  // D[i = 4 g + r][j = c16] of block (a, b) is row dw_tile_row, column dw_tile_col of the tile
  float *P = partial + (int64_t)(direct ? k : chunk) * ci * co;
  if constexpr (kF32 && NB == 4) {
    if (form & 8) {                                          // (vout holds: the lane's columns nv .. nv + 3, all below co)
#pragma unroll
      for (int a = 0; a < CB; ++a) {
        f32x4 t[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) t[b] = red[a * 4 + b][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = cb0 * 16 + dw_tile_row(vin, CB, g, r, a);
          if (c < ci) *reinterpret_cast<f32x4 *>(P + (int64_t)c * co + nv) = (f32x4){t[0][r], t[1][r], t[2][r], t[3][r]};
        }
      }
      return;
    }
  }
#pragma unroll
  for (int a = 0; a < CB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      f32x4 t = red[a * NB + b][lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int c = cb0 * 16 + dw_tile_row(vin, CB, g, r, a), n = nb0 * 16 + dw_tile_col(vout, NB, c16, b);
        if (c < ci && n < co) P[(int64_t)c * co + n] = t[r];
      }
    }
}

// bf16 features: the same chunked scheme on v_mfma_f32_16x16x32_bf16 with the PAIR index as K.
// The MFMA wants, per lane, 8 consecutive pairs of ONE channel -- a transpose of the row-major
// feature matrices.  Each wave stages 32 gathered rows (16-byte global loads, 16-byte LDS writes, rows
// padded by 16 B) and reads the operands back with ds_read_b64_tr_b16 (hardware 4x16 transpose: lane L
// of a 16-lane group receives column L of 4 rows): two reads per 16-channel fragment.  The next batch's
// rows are loaded into registers while the current batch's MFMAs run.  CB, NB in {2, 4}.
typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int CB, int NB>
__global__ __launch_bounds__(256) void k_conv_dw_pairs_bf16(const __bf16 *__restrict__ in, int ci,
                                                            const __bf16 *__restrict__ d_out, int co, int64_t V,
                                                            const int32_t *__restrict__ words, int vol,
                                                            int chunk_pairs, float *__restrict__ partial, int direct) {
  constexpr int SX = CB * 32 + 16, SG = NB * 32 + 16; // LDS row strides (bytes)
  constexpr int XCH = CB * 2, GCH = NB * 2;           // 16-byte chunks per row
  constexpr int XIT = (32 * XCH) / 64, GIT = (32 * GCH) / 64; // chunks per lane and batch
  __shared__ f32x4 red[CB * NB][64];
  __shared__ __attribute__((aligned(16))) unsigned char stage[4][32 * (SX + SG)];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c16 = lane & 15;
  const int nnb = nnb_of(co);
  const int tiles_n = (nnb + NB - 1) / NB;
  const int tile = blockIdx.y;
  const int cb0 = (tile / tiles_n) * CB, nb0 = (tile % tiles_n) * NB;
  const int chunk = blockIdx.x;
  int k, c0, c1;
  if (!dw_chunk_range(words, vol, chunk_pairs, direct, chunk, lane, k, c0, c1)) return;
  const int p0 = c0 + wave * (chunk_pairs / 4);
  int p1 = p0 + chunk_pairs / 4;
  if (p1 > c1) p1 = c1;
  const int2 *pairs = reinterpret_cast<const int2 *>(words + op_hdr(vol) + (int64_t)vol * op_nb256(V)) +
                      (int64_t)k * V;
  unsigned char *xs = stage[wave], *gs = stage[wave] + 32 * SX;
  f32x4 acc[CB][NB];
#pragma unroll
  for (int a = 0; a < CB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // register staging of one batch: XIT + GIT 16-byte chunks per lane (rows past the range: zeros)
  u32x4 xr[XIT], gr[GIT];
  auto load_batch = [&](int q32) {
    const int q = q32 + (lane & 31);
    const int2 pr = (q < p1) ? pairs[q] : make_int2(-1, -1);
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
      const int id = it * 64 + lane, row = id / XCH, ch = id - row * XCH;
      const int t = __shfl(pr.x, row);
      xr[it] = (u32x4){0u, 0u, 0u, 0u};
      if (t >= 0 && cb0 * 16 + ch * 8 < ci) // planes past the layer width (last tile): zeros, never read out of the row
        xr[it] = *reinterpret_cast<const u32x4 *>(in + (int64_t)t * ci + cb0 * 16 + ch * 8);
    }
#pragma unroll
    for (int it = 0; it < GIT; ++it) {
      const int id = it * 64 + lane, row = id / GCH, ch = id - row * GCH;
      const int o = __shfl(pr.y, row);
      gr[it] = (u32x4){0u, 0u, 0u, 0u};
      if (o >= 0 && nb0 * 16 + ch * 8 < co)
        gr[it] = *reinterpret_cast<const u32x4 *>(d_out + (int64_t)o * co + nb0 * 16 + ch * 8);
    }
  };
  auto store_batch = [&]() {
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
      const int id = it * 64 + lane, row = id / XCH, ch = id - row * XCH;
      *reinterpret_cast<u32x4 *>(xs + row * SX + ch * 16) = xr[it];
    }
#pragma unroll
    for (int it = 0; it < GIT; ++it) {
      const int id = it * 64 + lane, row = id / GCH, ch = id - row * GCH;
      *reinterpret_cast<u32x4 *>(gs + row * SG + ch * 16) = gr[it];
    }
  };
  // transposed operand: rows (pairs) g*8 .. g*8+7 of 16-bit column (blk*16 + c16)
  const int q4 = c16 >> 2, p4 = c16 & 3;
  auto tr_frag = [&](const unsigned char *base, int stride, int blk) {
    const unsigned char *a0 = base + (g * 8 + q4) * stride + (blk * 16 + 4 * p4) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)a0);
    const s16x4 hi =
        __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(a0 + 4 * stride));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  if (p0 < p1) { // wave-uniform: the tr reads below always run with all 64 lanes active
    load_batch(p0);
    for (int q32 = p0; q32 < p1; q32 += 32) {
      store_batch();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      if (q32 + 32 < p1) load_batch(q32 + 32);
      bf16x8 af[CB], bf[NB];
#pragma unroll
      for (int a = 0; a < CB; ++a) af[a] = tr_frag(xs, SX, a);
#pragma unroll
      for (int b = 0; b < NB; ++b) bf[b] = tr_frag(gs, SG, b);
#pragma unroll
      for (int a = 0; a < CB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bf[b], acc[a][b], 0, 0, 0);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // reads done before the next batch overwrites
    }
  }
  // sum the four waves' accumulators in wave order: w0 + w1 + w2 + w3
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int a = 0; a < CB; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          if (w == 0) red[a * NB + b][lane] = acc[a][b];
          else {
            f32x4 t = red[a * NB + b][lane];
            t[0] += acc[a][b][0]; t[1] += acc[a][b][1]; t[2] += acc[a][b][2]; t[3] += acc[a][b][3];
            red[a * NB + b][lane] = t;
          }
        }
    }
    __syncthreads();
  }
  if (wave != 0) return;
  float *P = partial + (int64_t)(direct ? k : chunk) * ci * co;
#pragma unroll
  for (int a = 0; a < CB; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      f32x4 t = red[a * NB + b][lane];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int c = (cb0 + a) * 16 + g * 4 + r, n = (nb0 + b) * 16 + c16;
        if (c < ci && n < co) P[(int64_t)c * co + n] = t[r];
      }
    }
}

// ---- full-tile weight gradient (round 5) -------------------------------------------------------------------------------
// k_conv_dw_pairs[_bf16] give a workgroup ONE 64 x 64 block of dW: a 128 x 128 layer is four workgroups per chunk and
// every gathered row (input features and output gradients) is fetched twice -- at the dominant level 800 MB (bf16) /
// 1.6 GB (fp32) of row gathers per launch, ~5.5 TB/s out of the L2s, which is what those kernels run at.  Here a
// workgroup forms a whole 128 x 128 block for its chunk: the 256 threads gather each pair's two rows ONCE (full 128-plane
// slices, 16-byte loads, whole 256- / 512-byte segments) into LDS, the four waves own one 64 x 64 quadrant each and read
// their operand fragments from there.  All waves walk all pairs of the chunk, so there is no cross-wave sum at the end;
// the summation order (pairs ascending per quadrant element, workgroups ascending in k_conv_dw_reduce_ranges) is fixed.
//
// Work split: a workgroup per 1024-pair chunk is 787 workgroups of equal weight for 768 resident slots at the dominant
// level -- a CU that receives four takes a third longer than the average of 3.07, and every workgroup here is four times as
// heavy as a 64 x 64 one.  So the pairs of ALL offsets are laid end to end (offset k owns [s_k, s_k + R_k) of R = sum R_k)
// and workgroup w takes [w per, (w + 1) per), per = ceil(R / n_wg): every workgroup the same number of pairs, whatever the
// offsets' sizes.  A workgroup whose range crosses offset boundaries writes one partial block per offset it touches, into
// slot w + (number of non-empty offsets before k): along the staircase of (w, k) cells that sum grows by one per cell, so
// slots are unique, at most n_wg + vol of them, and offset k's are contiguous: w_lo(k) + ne_k .. w_hi(k) + ne_k.
constexpr int kDwMinPer = 128;                             // pairs per workgroup at least (tiny rule books: fewer workgroups)
__device__ inline int64_t dw_range_per(int64_t rtot, int n_wg) {
  const int64_t per = (rtot + n_wg - 1) / n_wg;
  return per < kDwMinPer ? kDwMinPer : per;
}
__device__ inline int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}
__device__ inline int64_t dw_total_pairs(const int32_t *__restrict__ words, int vol, int lane) {
  int64_t rtot = 0;
  for (int k0 = 0; k0 < vol; k0 += 64) {
    const int c = k0 + lane < vol ? words[k0 + lane] : 0;
    rtot += __shfl(wave_incl_scan(c, lane), 63);
  }
  return rtot;
}
// calls seg(k, p0, p1, slot) for every offset k the range [lo, hi) of the concatenated pair list touches, k ascending;
// wave-uniform (every wave of a workgroup walks the same segments)
template <typename F>
__device__ inline void dw_for_segments(const int32_t *__restrict__ words, int vol, int lane, int64_t lo, int64_t hi, int w,
                                       F seg) {
  int64_t base = 0;
  int ne_base = 0;
  for (int k0 = 0; k0 < vol && base < hi; k0 += 64) {
    const int c = k0 + lane < vol ? words[k0 + lane] : 0;
    const int incl = wave_incl_scan(c, lane);
    const int64_t s = base + incl - c;
    const unsigned long long nz = __ballot(c > 0);
    unsigned long long m = __ballot(c > 0 && s < hi && s + c > lo);
    while (m) {
      const int j = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int64_t sk = base + __shfl(incl - c, j);
      const int ck = __shfl(c, j);
      const int ne = ne_base + (int)__popcll(nz & ((1ull << j) - 1ull));
      const int64_t a = lo > sk ? lo : sk, b = hi < sk + ck ? hi : sk + ck;
      seg(k0 + j, (int)(a - sk), (int)(b - sk), w + ne);
    }
    base += __shfl(incl, 63);
    ne_base += (int)__popcll(nz);
  }
}
// bf16 storage: batches of 64 pairs; a row slice is 256 bytes = 16 chunks of 16 bytes, stored unpadded with the chunk
// index XOR-swizzled by the row ((row & 3) | (row >> 3 & 1) << 2) << 1, so that the eight rows one half-wave of a
// ds_read_b64_tr_b16 touches land in eight different 32-byte bank groups; the pair -> LDS row assignment is free (the
// pair index is the reduction dimension) and the same for both operands.
__global__ __launch_bounds__(256) void k_conv_dw_full_bf16(const __bf16 *__restrict__ in, int ci,
                                                           const __bf16 *__restrict__ d_out, int co, int64_t V,
                                                           const int32_t *__restrict__ words, int vol,
                                                           float *__restrict__ partial) {
  constexpr int kB = 64;                                   // pairs per batch
  __shared__ __attribute__((aligned(16))) unsigned char xs[kB * 256];
  __shared__ __attribute__((aligned(16))) unsigned char gs[kB * 256];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c16 = lane & 15;
  const int tiles_n = co >> 7;
  const int tc = (int)blockIdx.y / tiles_n, tn = (int)blockIdx.y % tiles_n;
  const int wc = wave >> 1, wn = wave & 1;
  const int64_t rtot = dw_total_pairs(words, vol, lane);
  const int64_t per = dw_range_per(rtot, (int)gridDim.x);
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < rtot ? lo + per : rtot;
  if (lo >= hi) return;                                    // workgroup-uniform
  const int2 *pairs0 = reinterpret_cast<const int2 *>(words + op_hdr(vol) + (int64_t)vol * op_nb256(V));
  const __bf16 *inb = in + tc * 128, *gb = d_out + tn * 128;
  auto sw = [](int row) { return (((row & 3) | (((row >> 3) & 1) << 2)) << 1); };
  const int q4 = c16 >> 2, p4 = c16 & 3;
  dw_for_segments(words, vol, lane, lo, hi, (int)blockIdx.x, [&](int k, int p0, int p1, int slot) {
  const int2 *pairs = pairs0 + (int64_t)k * V;
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  u32x4 xr[4], gr[4];
  // the pair entries of a batch are loaded one batch ahead of its rows (a wave issues in order: waiting for them in
  // front of the row loads would stall the MFMAs behind)
  auto load_pairs = [&](int q0) {
    const int q = q0 + lane;
    return (q < p1) ? pairs[q] : make_int2(-1, -1);
  };
  auto load_batch = [&](int2 pr) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 16 + wave * 4 + g;              // this lane's chunk: (row, c16)
      const int t = __shfl(pr.x, row), o = __shfl(pr.y, row);
      xr[it] = (u32x4){0u, 0u, 0u, 0u};
      gr[it] = (u32x4){0u, 0u, 0u, 0u};
      if (t >= 0) {
        xr[it] = *reinterpret_cast<const u32x4 *>(inb + (int64_t)t * ci + c16 * 8);
        gr[it] = *reinterpret_cast<const u32x4 *>(gb + (int64_t)o * co + c16 * 8);
      }
    }
  };
  auto store_batch = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 16 + wave * 4 + g;
      const int off = row * 256 + ((c16 ^ sw(row)) << 4);
      *reinterpret_cast<u32x4 *>(xs + off) = xr[it];
      *reinterpret_cast<u32x4 *>(gs + off) = gr[it];
    }
  };
  // transposed operand of one K step (32 pairs = LDS rows r0 .. r0+31): pairs g*8 .. g*8+7 of plane blk*16 + c16
  auto tr_frag = [&](const unsigned char *base, int r0, int blk) {
    const int rl = r0 + g * 8 + q4, rh = rl + 4;
    const int ch = blk * 2 + (p4 >> 1), hb = (p4 & 1) << 3;
    const unsigned char *al = base + rl * 256 + ((ch ^ sw(rl)) << 4) + hb;
    const unsigned char *ah = base + rh * 256 + ((ch ^ sw(rh)) << 4) + hb;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)al);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)ah);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  {
    load_batch(load_pairs(p0));
    int2 prn = load_pairs(p0 + kB);
    for (int q0 = p0; q0 < p1; q0 += kB) {
      store_batch();
      __syncthreads();
      if (q0 + kB < p1) load_batch(prn);                   // in flight under this batch's MFMAs
      prn = load_pairs(q0 + 2 * kB);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 af[4], bf[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) af[a] = tr_frag(xs, ks * 32, wc * 4 + a);
#pragma unroll
        for (int b = 0; b < 4; ++b) bf[b] = tr_frag(gs, ks * 32, wn * 4 + b);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bf[b], acc[a][b], 0, 0, 0);
      }
      __syncthreads();                                     // every wave has read the batch before it is overwritten
    }
  }
  float *P = partial + (int64_t)slot * ci * co;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = tc * 128 + (wc * 4 + a) * 16 + g * 4 + r, n = tn * 128 + (wn * 4 + b) * 16 + c16;
        P[(int64_t)c * co + n] = acc[a][b][r];
      }
  });
}

// fp32: batches of 32 pairs; a row slice is 512 bytes, LDS rows padded to 144 words so that the four rows x 16 planes
// one operand read touches are 64 different banks.
__global__ __launch_bounds__(256) void k_conv_dw_full_f32(const float *__restrict__ in, int ci,
                                                          const float *__restrict__ d_out, int co, int64_t V,
                                                          const int32_t *__restrict__ words, int vol,
                                                          float *__restrict__ partial) {
  constexpr int kB = 32, kS = 144;                         // pairs per batch, LDS row stride in words
  __shared__ __attribute__((aligned(16))) float xs[kB * kS];
  __shared__ __attribute__((aligned(16))) float gs[kB * kS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, c16 = lane & 15;
  const int tiles_n = co >> 7;
  const int tc = (int)blockIdx.y / tiles_n, tn = (int)blockIdx.y % tiles_n;
  const int wc = wave >> 1, wn = wave & 1;
  const int64_t rtot = dw_total_pairs(words, vol, lane);
  const int64_t per = dw_range_per(rtot, (int)gridDim.x);
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < rtot ? lo + per : rtot;
  if (lo >= hi) return;                                    // workgroup-uniform
  const int2 *pairs0 = reinterpret_cast<const int2 *>(words + op_hdr(vol) + (int64_t)vol * op_nb256(V));
  const float *inb = in + tc * 128, *gb = d_out + tn * 128;
  const int h = lane >> 5, c32 = lane & 31;                // this lane's chunks: rows it*8 + wave*2 + h, 16-byte chunk c32
  dw_for_segments(words, vol, lane, lo, hi, (int)blockIdx.x, [&](int k, int p0, int p1, int slot) {
  const int2 *pairs = pairs0 + (int64_t)k * V;
  f32x4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 xr[4], gr[4];
  auto load_pairs = [&](int q0) {
    const int q = q0 + c32;
    return (q < p1) ? pairs[q] : make_int2(-1, -1);
  };
  auto load_batch = [&](int2 pr) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + wave * 2 + h;
      const int t = __shfl(pr.x, row), o = __shfl(pr.y, row);
      xr[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
      gr[it] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (t >= 0) {
        xr[it] = *reinterpret_cast<const f32x4 *>(inb + (int64_t)t * ci + c32 * 4);
        gr[it] = *reinterpret_cast<const f32x4 *>(gb + (int64_t)o * co + c32 * 4);
      }
    }
  };
  auto store_batch = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + wave * 2 + h;
      *reinterpret_cast<f32x4 *>(xs + row * kS + c32 * 4) = xr[it];
      *reinterpret_cast<f32x4 *>(gs + row * kS + c32 * 4) = gr[it];
    }
  };
  {
    load_batch(load_pairs(p0));
    int2 prn = load_pairs(p0 + kB);
    for (int q0 = p0; q0 < p1; q0 += kB) {
      store_batch();
      __syncthreads();
      if (q0 + kB < p1) load_batch(prn);
      prn = load_pairs(q0 + 2 * kB);
      const float *xa = xs + g * kS + wc * 64 + c16, *ga = gs + g * kS + wn * 64 + c16;
#pragma unroll
      for (int st = 0; st < 8; ++st) {                     // four pairs per MFMA step: A[i = plane][k = pair g]
        float fa[4], fb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) fa[a] = xa[st * 4 * kS + a * 16];
#pragma unroll
        for (int b = 0; b < 4; ++b) fb[b] = ga[st * 4 * kS + b * 16];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  float *P = partial + (int64_t)slot * ci * co;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = tc * 128 + (wc * 4 + a) * 16 + g * 4 + r, n = tn * 128 + (wn * 4 + b) * 16 + c16;
        P[(int64_t)c * co + n] = acc[a][b][r];
      }
  });
}

// dW[k][i] = sum over the workgroups w_lo(k) .. w_hi(k) of the full-tile launch of their partial block for offset k, in
// workgroup order (four slices as below, combined in slice order): deterministic.  Offsets without rules: zeros.
__global__ __launch_bounds__(256) void k_conv_dw_reduce_ranges(const float *__restrict__ partial,
                                                               const int32_t *__restrict__ words, int vol, int n_wg,
                                                               int64_t cico, float *__restrict__ dW) {
  __shared__ float red[4][64];
  const int k = blockIdx.y, col = threadIdx.x & 63, sl = threadIdx.x >> 6, lane = col;
  const int64_t i = (int64_t)blockIdx.x * 64 + col;
  // s_k, R_k, ne_k of this block's offset and the total (every wave the same values)
  int64_t base = 0, sk = 0;
  int ne = 0, ck = 0;
  for (int k0 = 0; k0 < vol; k0 += 64) {
    const int c = k0 + lane < vol ? words[k0 + lane] : 0;
    const int incl = wave_incl_scan(c, lane);
    const unsigned long long nz = __ballot(c > 0);
    if (k >= k0 && k < k0 + 64) {
      const int j = k - k0;
      sk = base + __shfl(incl - c, j);
      ck = __shfl(c, j);
      ne += (int)__popcll(nz & ((1ull << j) - 1ull));
    } else if (k >= k0 + 64) ne += (int)__popcll(nz);
    base += __shfl(incl, 63);
  }
  float s = 0.0f;
  if (ck > 0 && i < cico) {
    const int64_t per = dw_range_per(base, n_wg);
    const int64_t w0 = sk / per, w1 = (sk + ck - 1) / per;
#pragma unroll 4
    for (int64_t w = w0 + sl; w <= w1; w += 4) s += partial[(w + ne) * cico + i];
  }
  red[sl][col] = s;
  __syncthreads();
  if (sl == 0 && i < cico) dW[(int64_t)k * cico + i] = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
}

// dW[k][i] = sum of the partials of offset k's chunks (fixed order => deterministic): a block takes 64
// consecutive elements i and deals the chunks to 4 slices (chunk c0+s, c0+s+4, ...), several loads in
// flight per thread; the slices are combined in slice order through LDS
__global__ __launch_bounds__(256) void k_conv_dw_reduce(const float *__restrict__ partial,
                                                        const int32_t *__restrict__ words, int vol,
                                                        int chunk_pairs, int64_t cico, float *__restrict__ dW) {
  __shared__ float red[4][64];
  const int k = blockIdx.y, col = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + col;
  const int32_t *cstart = words + vol + (chunk_pairs == 256 ? vol + 1 : 0);
  const int c0 = cstart[k], c1 = cstart[k + 1];
  float s = 0.0f;
  if (i < cico) {
#pragma unroll 8
    for (int c = c0 + sl; c < c1; c += 4) s += partial[(int64_t)c * cico + i];
  }
  red[sl][col] = s;
  __syncthreads();
  if (sl == 0 && i < cico) dW[(int64_t)k * cico + i] = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
}

// d_bias[n] = sum_rows d_out[row][n] (at::sum_out, CPU/Convolution.cpp:100-101), two fixed-order stages:
// S row slices x 64-column blocks of partial sums (rows s, s+S, ... per slice; 4 sub-slices per block
// combined through LDS), then one thread per column adds the S partials in slice order => deterministic.
template <typename T>
__global__ __launch_bounds__(256) void k_col_sum_partial(const T *__restrict__ x, int64_t rows, int co, int S,
                                                         float *__restrict__ part) {
  __shared__ float red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6, sl = blockIdx.y;
  float s = 0.0f;
  if (col < co)
    for (int64_t r = (int64_t)sl * 4 + sub; r < rows; r += (int64_t)S * 4) s += ldf(x, r * co + col);
  red[sub][threadIdx.x & 63] = s;
  __syncthreads();
  if (sub == 0 && col < co)
    part[(int64_t)sl * co + col] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

__global__ __launch_bounds__(256) void k_col_sum_final(const float *__restrict__ part, int co, int S,
                                                       float *__restrict__ out) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= co) return;
  float s = 0.0f;
  for (int i = 0; i < S; ++i) s += part[(int64_t)i * co + col];
  out[col] = s;
}

// scratch: the dW partial buffer, free again once the chunk reduction has been enqueued
template <typename T>
static void launch_col_sum(const T *d_out, int64_t rows, int co, float *d_bias, float *scratch, int64_t scratch_floats,
                           hipStream_t st) {
  int64_t S = scratch_floats / co;
  if (S > 128) S = 128;
  if (S > ceil_div(rows, 4)) S = ceil_div(rows, 4);
  if (S < 1) S = 1;
  hipLaunchKernelGGL((k_col_sum_partial<T>), dim3((unsigned)ceil_div(co, 64), (unsigned)S), dim3(256), 0, st, d_out,
                     rows, co, (int)S, scratch);
  hipLaunchKernelGGL(k_col_sum_final, dim3((unsigned)ceil_div(co, 256)), dim3(256), 0, st, scratch, co, (int)S, d_bias);
}

} // namespace aabr

using namespace aabr;

// ---- conv_dw_tiles.h decides, these tables carry the decision out ---------------------------------------------------
// One row per kernel instance the decision can return, with the name aabr_conv_last_variant reports for it; no other
// instance of these kernels is compiled (tests/test_conv_dw_host.py checks both against the decision).
template <typename Fn> struct DwInst { DwKernel k; const char *name; Fn fn; };
template <typename T> using DwPairsFn = decltype(&k_conv_dw_pairs<1, 1, T>);   // (k_conv_dw_pairs_bf16: the same)
template <typename T> using DwFullFn = void (*)(const T *, int, const T *, int, int64_t, const int32_t *, int, float *);
template <typename T> struct DwTables;
#define AABR_DW_F32(CB, NB) \
  {{kDwPairs, false, CB, NB}, "k_conv_dw_pairs<" #CB "," #NB ",float>", k_conv_dw_pairs<CB, NB, float>}
#define AABR_DW_BF16(CB, NB) \
  {{kDwPairs, true, CB, NB}, "k_conv_dw_pairs<" #CB "," #NB ",bf16>", k_conv_dw_pairs<CB, NB, __bf16>}
#define AABR_DW_MFMA(CB, NB) \
  {{kDwPairsMfma, true, CB, NB}, "k_conv_dw_pairs_bf16<" #CB "," #NB ">", k_conv_dw_pairs_bf16<CB, NB>}
#define AABR_DW_FULL(S, BF) {{kDwFull, BF, 0, 0}, "k_conv_dw_full_" #S, k_conv_dw_full_##S}
template <> struct DwTables<float> {
  static constexpr DwInst<DwPairsFn<float>> pairs[] = {
      AABR_DW_F32(1, 1), AABR_DW_F32(1, 2), AABR_DW_F32(1, 4), AABR_DW_F32(2, 1), AABR_DW_F32(2, 2), AABR_DW_F32(2, 4),
      AABR_DW_F32(4, 1), AABR_DW_F32(4, 2), AABR_DW_F32(4, 4)};
  static constexpr DwInst<DwFullFn<float>> full[] = {AABR_DW_FULL(f32, false)};
};
template <> struct DwTables<__bf16> {
  static constexpr DwInst<DwPairsFn<__bf16>> pairs[] = {
      AABR_DW_BF16(1, 1), AABR_DW_BF16(1, 2), AABR_DW_BF16(1, 4), AABR_DW_BF16(2, 1), AABR_DW_BF16(2, 2),
      AABR_DW_BF16(2, 4), AABR_DW_BF16(4, 1), AABR_DW_BF16(4, 2), AABR_DW_BF16(4, 4),
      AABR_DW_MFMA(2, 2), AABR_DW_MFMA(2, 4), AABR_DW_MFMA(4, 2), AABR_DW_MFMA(4, 4)};
  static constexpr DwInst<DwFullFn<__bf16>> full[] = {AABR_DW_FULL(bf16, true)};
};
template <typename Fn, size_t N>
static const DwInst<Fn> *dw_inst(const DwInst<Fn> (&tab)[N], const DwKernel &k) {
  for (const DwInst<Fn> &e : tab)
    if (e.k == k) return &e;
  return nullptr;
}

// the `form` argument of k_conv_dw_pairs: bit 0 direct, bits 1-2 the vector-loaded operands (fp32 instances of that
// kernel only), bit 3 16-byte stores (four column blocks in the vector form, destination aligned)
static int dw_pairs_form(const DwLaunch &d, int n_in, int n_out, const void *in_feats, const void *d_out, const float *dst) {
  const int vec = d.k.kind == kDwPairs ? dw_vec_operands(d.k.bf16, n_in, n_out, d.k.cb, d.k.nb, (uintptr_t)in_feats,
                                                          (uintptr_t)d_out, knob(K_DW_VEC)) : 0;
  const int st16 = (vec & kDwVecOut) && d.k.nb == 4 && ((uintptr_t)dst & 15) == 0;
  return d.direct | vec << 1 | st16 << 3;
}

extern "C" int aabr_conv_dw_vec_operands(int bf16, const void *in_feats, int n_in, const void *d_out, int n_out,
                                         int64_t V_out, int vol, int64_t max_chunks) {
  if (n_in <= 0 || n_out <= 0 || vol <= 0 || V_out <= 0 || max_chunks <= 0) return 0;
  const bool bf = bf16 != 0, aligned16 = ((uintptr_t)in_feats & 15) == 0 && ((uintptr_t)d_out & 15) == 0;
  const DwLaunch d = conv_dw_launch(bf, n_in, n_out, V_out, vol, max_chunks, aligned16,
                                    DwKnobs{knob(K_DW_FULL), knob(K_DW_FULL_MIN), knob(K_DW_FULL_WGS)});
  return d.k.kind == kDwPairs ? dw_vec_operands(bf, n_in, n_out, d.k.cb, d.k.nb, (uintptr_t)in_feats, (uintptr_t)d_out,
                                                knob(K_DW_VEC)) : 0;
}

extern "C" int64_t aabr_conv_dw_scratch_floats(int64_t max_chunks, int n_in, int n_out) {
  return max_chunks * n_in * n_out;
}

extern "C" int aabr_conv_dw_chunk_pairs(int64_t V_out, int vol, int n_in, int n_out) {
  return dw_chunk(V_out, vol, n_in, n_out);
}

template <typename T>
static int conv_backward_weight_t(const T *in_feats, int n_in, const T *d_out, int n_out, int64_t V_out,
                                  const int32_t *pairs, int vol, int64_t max_chunks, float *dW, float *d_bias,
                                  float *scratch, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  AABR_CHECK_ARG(n_in > 0 && n_out > 0 && vol > 0 && V_out >= 0 && vol <= 65535, "bad sizes");
  AABR_CHECK_ARG(dW, "null dW");
  int64_t cico = (int64_t)n_in * n_out;
  if (V_out == 0 || max_chunks == 0) {
    hipMemsetAsync(dW, 0, vol * cico * sizeof(float), st);
    if (d_bias) hipMemsetAsync(d_bias, 0, n_out * sizeof(float), st);
    return AABR_OK;
  }
  const bool bf = sizeof(T) == 2, aligned16 = ((uintptr_t)in_feats & 15) == 0 && ((uintptr_t)d_out & 15) == 0;
  AABR_CHECK_ARG(!dw_mfma16(bf, n_in, n_out, aligned16) || (n_in <= 4096 && n_out <= 4096), "bad sizes");
  AABR_CHECK_ARG(in_feats && d_out && pairs && scratch && max_chunks > 0, "null pointer");
  const DwLaunch d = conv_dw_launch(bf, n_in, n_out, V_out, vol, max_chunks, aligned16,
                                    DwKnobs{knob(K_DW_FULL), knob(K_DW_FULL_MIN), knob(K_DW_FULL_WGS)});
  AABR_CHECK_ARG(d.tiles <= 65535, "too many tiles");
  const dim3 grid((unsigned)d.grid_x, (unsigned)d.grid_y);
  float *dst = d.to_scratch ? scratch : dW;
  if (d.k.kind == kDwFull) {
    const auto *e = dw_inst(DwTables<T>::full, d.k);
    AABR_CHECK_ARG(e, "no kernel instance for this launch");
    g_last_variant = e->name;
    hipLaunchKernelGGL(e->fn, grid, dim3(256), 0, st, in_feats, n_in, d_out, n_out, V_out, pairs, vol, dst);
  } else {
    const auto *e = dw_inst(DwTables<T>::pairs, d.k);
    AABR_CHECK_ARG(e, "no kernel instance for this launch");
    g_last_variant = e->name;
    hipLaunchKernelGGL(e->fn, grid, dim3(256), 0, st, in_feats, n_in, d_out, n_out, V_out, pairs, vol, d.chunk_pairs, dst,
                       dw_pairs_form(d, n_in, n_out, in_feats, d_out, dst));
  }
  const dim3 rgrid((unsigned)ceil_div(cico, 64), (unsigned)vol);
  if (d.reduce == kDwReduceRanges)
    hipLaunchKernelGGL(k_conv_dw_reduce_ranges, rgrid, dim3(256), 0, st, scratch, pairs, vol, d.n_wg, cico, dW);
  else if (d.reduce == kDwReduceChunks)
    hipLaunchKernelGGL(k_conv_dw_reduce, rgrid, dim3(256), 0, st, scratch, pairs, vol, d.chunk_pairs, cico, dW);
  if (d_bias) launch_col_sum<T>(d_out, V_out, n_out, d_bias, scratch, max_chunks * cico, st);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_conv_backward_weight(const float *in_feats, int n_in, const float *d_out, int n_out,
                                         int64_t V_out, const int32_t *pairs, int vol, int64_t max_chunks,
                                         float *dW, float *d_bias, float *scratch, void *stream_) {
  return conv_backward_weight_t<float>(in_feats, n_in, d_out, n_out, V_out, pairs, vol, max_chunks, dW, d_bias,
                                       scratch, stream_);
}

extern "C" int aabr_conv_backward_weight_bf16(const uint16_t *in_feats, int n_in, const uint16_t *d_out,
                                              int n_out, int64_t V_out, const int32_t *pairs, int vol,
                                              int64_t max_chunks, float *dW, float *d_bias, float *scratch,
                                              void *stream_) {
  return conv_backward_weight_t<__bf16>(reinterpret_cast<const __bf16 *>(in_feats), n_in,
                                        reinterpret_cast<const __bf16 *>(d_out), n_out, V_out, pairs, vol,
                                        max_chunks, dW, d_bias, scratch, stream_);
}

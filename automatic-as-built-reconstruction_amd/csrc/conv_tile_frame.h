// conv_tile_frame.h -- what the 64-row-tile kernels of conv.hip share (device code only).
//
// Every k_conv_blocks_mfma* kernel is one frame around its own inner pipeline: a wave sets up its tile context
// (TileLanes; TileCtx adds the buffer descriptors), streams pairs of 16-pair blocks (pair_count, pair_blocks,
// load_block_pair), gathers their rows (gather_rows), runs the interleaved MFMA chains (AABR_MFMA16), adds both
// accumulators into its private LDS tile (accumulate_pair) and the workgroup writes the tile once (tile_epilogue).
// All of it is `inline` and compiles back into the kernels: the instances keep their registers and occupancy
// (profiles/conv_tiles_fold_resources.txt).
#pragma once
#include "common.h"

namespace aabr {

// tile-major block lists (k_build_tile_blocks):
//   words:  [ntiles] nblk | [ntiles][MAXB] offset k of each block | [ntiles][MAXB][16] entries;  MAXB = 4 * vol
__host__ __device__ inline int64_t tb_ntiles(int64_t V) { return (V + 63) / 64; }
__host__ __device__ inline int tb_maxb(int vol) { return 4 * vol; }

// block entries (eA, eB) and filter offsets (kA, kB) of the two blocks a step works on
struct PairEnt { int eA, eB, kA, kB; };
// gathered rows of one 32-channel chunk of the two blocks: 2 x 16 B per lane and block
struct GStep { u32x4 a0, a1, b0, b1; };

__device__ inline float bcf(unsigned int v) { return __builtin_bit_cast(float, v); }
__device__ inline float bcf(float v) { return v; }

// ---- tile context -----------------------------------------------------------------------------------------------
// the part that needs no descriptor (all the generic kernel uses: it addresses with flat 64-bit pointers)
template <int NBW>
struct TileLanes {
  static constexpr int WS = NBW * 16;   // C-tile row stride (floats)
  static constexpr int TILE = 64 * WS;  // floats per wave
  int wave, lane, g, c16;
  float *Ct;                            // this wave's LDS tile (zero_tile clears it)
  int nkc, nnb, nb0, nvalid;            // channel chunks, column blocks, first block of the slab, blocks in it
};

// `tiles`: LDS tile of wave 0; nkc is the caller's (ci >> 5 where the kernel requires ci % 32 == 0)
template <int NBW, typename C = TileLanes<NBW>>
__device__ inline C tile_lanes(float *tiles, int nkc, int co) {
  C c;
  c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  c.lane = threadIdx.x & 63;
  c.g = c.lane >> 4;
  c.c16 = c.lane & 15;
  c.Ct = tiles + (size_t)c.wave * C::TILE;
  c.nkc = nkc;
  c.nnb = nnb_of(co);
  c.nb0 = blockIdx.y * NBW;
  c.nvalid = (c.nnb - c.nb0) < NBW ? (c.nnb - c.nb0) : NBW;
  return c;
}

// the wave clears its own tile (tile_ctx does it last, after the tile's first loads have gone out)
template <typename C>
__device__ inline void zero_tile(const C &c) {
  for (int i = c.lane; i < C::TILE; i += 64) c.Ct[i] = 0.0f;
}

// the buffer-descriptor kernels: every load takes a 32-bit offset (wave-uniform parts in SGPRs, hardware range
// check).  ES = bytes per feature / packed-weight element (4, or 2 for bf16); a packed fragment is 512 elements.
template <int NBW, int ES>
struct TileCtx : TileLanes<NBW> {
  __amdgpu_buffer_rsrc_t rin, rw, rwords;
  int nblk;                             // blocks of this tile
  unsigned kbase, ebase;                // byte offsets of the tile's blk_k and ent in `words`
  unsigned rowbytes, gofs, laneofs;     // bytes per input row, of a lane's 8 channels in a chunk, of a lane's fragment part
  unsigned wk_bytes, kc_bytes;          // packed bytes per filter offset, per channel chunk
  unsigned c16x4;
};

template <int NBW, int ES, typename T>
__device__ inline TileCtx<NBW, ES> tile_ctx(float *tiles, int64_t tile, const T *in, int ci, int64_t in_bytes, int nkc, int co,
                                            int64_t V_out, const int32_t *words, int64_t words_bytes, int vol, const T *Wp,
                                            int64_t wp_bytes) {
  TileCtx<NBW, ES> c = tile_lanes<NBW, TileCtx<NBW, ES>>(tiles, nkc, co);
  const int maxb = tb_maxb(vol);
  const int64_t ntiles = tb_ntiles(V_out);
  c.rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(in), 0, (int)in_bytes, 0x00020000);
  c.rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(Wp), 0, (int)wp_bytes, 0x00020000);
  c.rwords = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(words), 0, (int)words_bytes, 0x00020000);
  c.nblk = words[tile];
  c.kbase = (unsigned)((ntiles + tile * maxb) * 4);
  c.ebase = (unsigned)((ntiles + ntiles * maxb + tile * maxb * 16) * 4);
  c.rowbytes = (unsigned)ci * (unsigned)ES;
  c.gofs = (unsigned)c.g * (8u * ES);
  c.laneofs = (unsigned)c.lane * (8u * ES);
  c.wk_bytes = (unsigned)nkc * (unsigned)c.nnb * (512u * ES);
  c.kc_bytes = (unsigned)c.nnb * (512u * ES);
  c.c16x4 = (unsigned)c.c16 * 4u;
  zero_tile(c);
  return c;
}

// ---- block pairs --------------------------------------------------------------------------------------------------
// ADJ (throughput-bound launches): pairs of adjacent blocks (2j, 2j + 1) dealt to the waves round-robin, same-offset
// pairs share their weight fragments; else blocks dealt round-robin and a wave pairs its own consecutive ones
template <bool ADJ, int WPB>
__device__ inline int pair_count(int wave, int nblk) {
  const int nmine = wave < nblk ? (nblk - wave + WPB - 1) / WPB : 0;
  const int tpairs = (nblk + 1) >> 1;
  return ADJ ? (wave < tpairs ? (tpairs - wave + WPB - 1) / WPB : 0) : ((nmine + 1) >> 1);
}

// blocks of the wave's pr-th pair; bB may lie past the end (load_block_pair handles it)
template <bool ADJ, int WPB>
__device__ inline void pair_blocks(int wave, int pr, int nblk, int &bA, int &bB) {
  bA = ADJ ? 2 * (wave + pr * WPB) : wave + (2 * pr) * WPB;
  if (bA >= nblk) bA = nblk > 0 ? (ADJ ? ((nblk - 1) & ~1) : nblk - 1) : 0; // past the end: harmless re-read
  bB = bA + (ADJ ? 1 : WPB);
}

// entries and offsets of blocks bA (< nblk, or 0) and bB; a missing B repeats A with the discard bit set
template <typename Ctx>
__device__ inline PairEnt load_block_pair(const Ctx &c, int bA, int bB) {
  PairEnt p;
  const bool hasB = bB < c.nblk;
  if (!hasB) bB = bA;
  p.eA = (int)__builtin_amdgcn_raw_buffer_load_b32(c.rwords, c.c16x4, c.ebase + (unsigned)bA * 64u, 0);
  p.eB = (int)__builtin_amdgcn_raw_buffer_load_b32(c.rwords, c.c16x4, c.ebase + (unsigned)bB * 64u, 0);
  if (!hasB) p.eB |= (int)0x80000000;
  p.kA = (int)__builtin_amdgcn_raw_buffer_load_b32(c.rwords, 0u, c.kbase + (unsigned)bA * 4u, 0);
  p.kB = (int)__builtin_amdgcn_raw_buffer_load_b32(c.rwords, 0u, c.kbase + (unsigned)bB * 4u, 0);
  return p;
}

// ---- row gather (fp32) --------------------------------------------------------------------------------------------
// chunk kc of the pair's two partner rows; padding entries are gathered like real ones (the result is dropped).
// !ALIGNED: any plane count (the 9-plane first layer): element loads, planes past ci read as zero (their packed
// weights are zero too); rows are ci * 4 bytes apart, not 16-byte aligned
template <bool ALIGNED, typename Ctx>
__device__ inline void gather_rows(const Ctx &c, int ci, const PairEnt &p, int kc, u32x4 &a0, u32x4 &a1, u32x4 &b0, u32x4 &b1) {
  const unsigned va = (((unsigned)p.eA & 0x7fffffffu) >> 6) * c.rowbytes + c.gofs;
  const unsigned vb = (((unsigned)p.eB & 0x7fffffffu) >> 6) * c.rowbytes + c.gofs;
  const unsigned so = (unsigned)kc * 128u;
  if (ALIGNED) {
    a0 = __builtin_amdgcn_raw_buffer_load_b128(c.rin, va, so, 0);
    a1 = __builtin_amdgcn_raw_buffer_load_b128(c.rin, va + 16u, so, 0);
    b0 = __builtin_amdgcn_raw_buffer_load_b128(c.rin, vb, so, 0);
    b1 = __builtin_amdgcn_raw_buffer_load_b128(c.rin, vb + 16u, so, 0);
  } else {
    const int c0 = kc * kKC + c.g * 8;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const bool ok0 = c0 + t < ci, ok1 = c0 + 4 + t < ci;
      a0[t] = ok0 ? __builtin_amdgcn_raw_buffer_load_b32(c.rin, va + 4u * t, so, 0) : 0u;
      a1[t] = ok1 ? __builtin_amdgcn_raw_buffer_load_b32(c.rin, va + 16u + 4u * t, so, 0) : 0u;
      b0[t] = ok0 ? __builtin_amdgcn_raw_buffer_load_b32(c.rin, vb + 4u * t, so, 0) : 0u;
      b1[t] = ok1 ? __builtin_amdgcn_raw_buffer_load_b32(c.rin, vb + 16u + 4u * t, so, 0) : 0u;
    }
  }
}

// ---- MFMA chains --------------------------------------------------------------------------------------------------
// the 32-channel step of one column block: eight v_mfma_f32_16x16x4_f32 per block, operands W0/X0 (k-slots 0..3) and
// W1/X1 (4..7).  AABR_MFMA16 interleaves the chains of blocks A and B: two independent accumulators keep the
// dependent latency of the instruction off the critical path
#define AABR_MFMA1(ACC, W, X, I) ACC = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf(W[I]), bcf(X[I]), ACC, 0, 0, 0)
#define AABR_MFMA8(ACC, W0, W1, X0, X1)                                                                              \
  AABR_MFMA1(ACC, W0, X0, 0); AABR_MFMA1(ACC, W0, X0, 1); AABR_MFMA1(ACC, W0, X0, 2); AABR_MFMA1(ACC, W0, X0, 3); \
  AABR_MFMA1(ACC, W1, X1, 0); AABR_MFMA1(ACC, W1, X1, 1); AABR_MFMA1(ACC, W1, X1, 2); AABR_MFMA1(ACC, W1, X1, 3)
#define AABR_MFMA16(CA, CB, WA0, WA1, WB0, WB1, XA0, XA1, XB0, XB1)  \
  AABR_MFMA1(CA, WA0, XA0, 0); AABR_MFMA1(CB, WB0, XB0, 0);         \
  AABR_MFMA1(CA, WA0, XA0, 1); AABR_MFMA1(CB, WB0, XB0, 1);         \
  AABR_MFMA1(CA, WA0, XA0, 2); AABR_MFMA1(CB, WB0, XB0, 2);         \
  AABR_MFMA1(CA, WA0, XA0, 3); AABR_MFMA1(CB, WB0, XB0, 3);         \
  AABR_MFMA1(CA, WA1, XA1, 0); AABR_MFMA1(CB, WB1, XB1, 0);         \
  AABR_MFMA1(CA, WA1, XA1, 1); AABR_MFMA1(CB, WB1, XB1, 1);         \
  AABR_MFMA1(CA, WA1, XA1, 2); AABR_MFMA1(CB, WB1, XB1, 2);         \
  AABR_MFMA1(CA, WA1, XA1, 3); AABR_MFMA1(CB, WB1, XB1, 3)

// ---- accumulate ---------------------------------------------------------------------------------------------------
// lane holds D^T[out col = j*16 + g*4 + r][pair c16]: 4 consecutive columns of the pair's row
template <int NBW>
__device__ inline void conv_block_accumulate(float *Ct, int e, int g, const f32x4 (&acc)[NBW]) {
  if (e >= 0) {
    const int orow = e & 63;
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      float4 *dst = reinterpret_cast<float4 *>(Ct + orow * (NBW * 16) + j * 16 + g * 4);
      float4 cur = *dst;
      cur.x += acc[j][0]; cur.y += acc[j][1]; cur.z += acc[j][2]; cur.w += acc[j][3];
      *dst = cur;
    }
  }
}

template <int NBW>
__device__ inline void accumulate_pair(float *Ct, int eA, int eB, int g, const f32x4 (&accA)[NBW], const f32x4 (&accB)[NBW]) {
  conv_block_accumulate<NBW>(Ct, eA, g, accA);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // A and B may hit the same row
  conv_block_accumulate<NBW>(Ct, eB, g, accB);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// ---- epilogue -----------------------------------------------------------------------------------------------------
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
__device__ inline void tile_store(float *dst, float v) { *dst = v; }
__device__ inline void tile_store(__bf16 *dst, float v) { *dst = (__bf16)v; }
__device__ inline void tile_store4(float *dst, float4 v) { *reinterpret_cast<float4 *>(dst) = v; }
__device__ inline void tile_store4(__bf16 *dst, float4 v) {
  *reinterpret_cast<bf16x4 *>(dst) = (bf16x4){(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
}

// sum NT per-wave tiles (tile 0 first, then 1 .. NT-1: the order is part of the result's bits), add the bias
// (CPU/Convolution.cpp:59-62), round once to TO and write the slab's rows.  `tid` of NTHR threads share the work;
// VEC: rows go out as 16-byte (bf16: 8-byte) vectors when co % 4 == 0
template <int NBW, int NT, int NTHR, bool VEC, typename TO>
__device__ inline void tile_epilogue(const float *tiles, int tid, TO *__restrict__ out, int co, int64_t V_out, int64_t row0,
                                     int nb0, const float *__restrict__ bias) {
  constexpr int WS = NBW * 16, TILE = 64 * WS;
  const int nrows = (int)((V_out - row0) < 64 ? (V_out - row0) : 64);
  const int wcols = (co - nb0 * 16) < NBW * 16 ? (co - nb0 * 16) : NBW * 16;
  if (VEC && (co & 3) == 0) {
    const int q = wcols >> 2; // float4 per row
    for (int i = tid; i < nrows * q; i += NTHR) {
      const int r = i / q, cq = i % q;
      float4 v = *reinterpret_cast<const float4 *>(tiles + r * WS + cq * 4);
#pragma unroll
      for (int w = 1; w < NT; ++w) {
        float4 u = *reinterpret_cast<const float4 *>(tiles + (size_t)w * TILE + r * WS + cq * 4);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
      }
      if (bias) {
        const float *bb = bias + nb0 * 16 + cq * 4;
        v.x += bb[0]; v.y += bb[1]; v.z += bb[2]; v.w += bb[3];
      }
      tile_store4(out + (row0 + r) * co + nb0 * 16 + cq * 4, v);
    }
  } else {
    for (int i = tid; i < nrows * wcols; i += NTHR) {
      const int r = i / wcols, cc = i % wcols;
      float v = tiles[r * WS + cc];
#pragma unroll
      for (int w = 1; w < NT; ++w) v += tiles[(size_t)w * TILE + r * WS + cc];
      if (bias) v += bias[nb0 * 16 + cc];
      tile_store(out + (row0 + r) * co + nb0 * 16 + cc, v);
    }
  }
}

} // namespace aabr

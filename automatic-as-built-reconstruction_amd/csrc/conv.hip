// conv.hip -- sparse 3-D convolution on gather tables, fp32 MFMA (gfx950).
//
// One formulation serves SubmanifoldConvolution, Convolution and Deconvolution, forward and
// input-gradient (reference: SCN/CPU/Convolution.cpp:45-185, SCN/CPU/Deconvolution.cpp:7-77,
// SCN/CUDA/Convolution.cu:57-667):
//
//     out[o] = bias + sum_k  in[ table[k][o] ] @ Wl[k]          (table entry -1 -> no term)
//
// It is OUTPUT-STATIONARY: a workgroup owns 64 consecutive output rows and a slab of output
// columns, keeps that tile in LDS for the whole sweep over the filter offsets and writes it to
// HBM exactly once -- no read-modify-write of `out` per offset and no atomics (the reference's
// GPU path re-reads and re-writes `out` 27 times and its rule book crosses PCIe per offset).
// The gather table is compiled once per rule book into per-tile blocks of 16 (partner row,
// local row) pairs sharing one offset; each block is one v_mfma_f32_16x16x4_f32 chain:
//     D^T[out col][pair] += Wl^T[out col][c] * in[partner(pair)][c]
// so each lane ends up with 4 consecutive output columns of one pair (one 16-byte LDS
// read-add-write).  Accumulation order is fixed (offset order, then channel order inside the
// MFMA chain) => results are bit-reproducible run to run.
//
// fp32 MFMA == k-ordered fmaf chain (exact fp32); peak 157 TFLOP/s.
#include "common.h"
#include "conv_tile_frame.h" // the frame the k_conv_blocks_mfma* kernels share: context, pair loads, gathers, epilogue
#include "offset_pairs.h"   // op_hdr, op_nb256: the pair list's layout
#include <stdlib.h>

namespace aabr {

// Wp[k][kc][nb][lane][s] = Wl[k][kc*32 + (lane>>4)*8 + s][nb*16 + (lane&15)]   (0 outside)
// Wl[k][c][n] = W[wk][c][n] (plain) or W[wk][n][c] (transpose), wk = flip ? vol-1-k : k.
__global__ __launch_bounds__(256) void k_pack_weights(const float *__restrict__ W, int vol, int ci, int co,
                                                      int transpose, int flip, float *__restrict__ Wp) {
  const int nkc = nkc_of(ci), nnb = nnb_of(co);
  int64_t total = (int64_t)vol * nkc * nnb * 512;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int s = idx & 7;
  int lane = (idx >> 3) & 63;
  int64_t r = idx >> 9;
  int nb = (int)(r % nnb); r /= nnb;
  int kc = (int)(r % nkc); r /= nkc;
  int k = (int)r;
  int c = kc * kKC + (lane >> 4) * 8 + s;
  int n = nb * 16 + (lane & 15);
  float v = 0.0f;
  if (c < ci && n < co) {
    int wk = flip ? vol - 1 - k : k;
    v = transpose ? W[((int64_t)wk * co + n) * ci + c] : W[((int64_t)wk * ci + c) * co + n];
  }
  Wp[idx] = v;
}

// both orientations in one launch: the forward layout (Wl = W[k]) into Wf and the input-gradient
// layout (Wl = W[k]^T, plane counts swapped) into Wt -- a training step needs each exactly once per
// weight version, so the backward pass can run with the "prepacked" flag and no pack launch of its own
template <typename TO>
__device__ inline TO pack_cvt(float v);
template <> __device__ inline float pack_cvt<float>(float v) { return v; }
template <> __device__ inline __bf16 pack_cvt<__bf16>(float v) { return (__bf16)v; }

template <typename TO>
__global__ __launch_bounds__(256) void k_pack_weights2(const float *__restrict__ W, int vol, int n_in, int n_out,
                                                       TO *__restrict__ Wf, TO *__restrict__ Wt) {
  const int64_t total_f = (int64_t)vol * nkc_of(n_in) * nnb_of(n_out) * 512;
  const int64_t total_t = (int64_t)vol * nkc_of(n_out) * nnb_of(n_in) * 512;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool tr = idx >= total_f;
  if (tr) idx -= total_f;
  if (idx >= (tr ? total_t : total_f)) return;
  const int ci = tr ? n_out : n_in, co = tr ? n_in : n_out;
  const int nkc = nkc_of(ci), nnb = nnb_of(co);
  int s = idx & 7;
  int lane = (idx >> 3) & 63;
  int64_t r = idx >> 9;
  int nb = (int)(r % nnb); r /= nnb;
  int kc = (int)(r % nkc); r /= nkc;
  int k = (int)r;
  int c = kc * kKC + (lane >> 4) * 8 + s;
  int n = nb * 16 + (lane & 15);
  float v = 0.0f;
  if (c < ci && n < co) v = tr ? W[((int64_t)k * co + n) * ci + c] : W[((int64_t)k * ci + c) * co + n];
  (tr ? Wt : Wf)[idx] = pack_cvt<TO>(v);
}

// every convolution of a network in ONE launch (a training step packs each weight once per version; 40-odd
// launches of a few microseconds each otherwise).  jobs (device, 48 bytes each):
//   { W, Wf, Wt : pointers; vol, n_in, n_out, bf16 : int32; first_block : int64 } -- job j owns the
// thread blocks [first_block[j], first_block[j+1]) of the grid; a block never straddles two jobs.
struct PackJob {
  const float *W;
  void *Wf, *Wt;
  int32_t vol, n_in, n_out, bf16;
  int64_t first_block;
};
static_assert(sizeof(PackJob) == 48, "PackJob layout is part of the C ABI");

// Round 4: a workgroup owns one 64 x 64 tile of one W[k]: the tile is read ONCE with coalesced 256-byte rows into LDS
// and both orientations' fragments (8 of 2 KiB each way) are written from there with coalesced stores.  Round 3's kernel
// read W element-wise in fragment order (32-byte segments) once per orientation: 167 us for the 21 M parameters of
// FPN_Net at the head of every training step, on the critical path.
constexpr int kPT = 64;                          // tile edge: 2 channel chunks x 4 column blocks
__device__ inline void pack_store(void *dst, int64_t idx, float v, int mode, int64_t plane) {
  (void)plane;
  if (mode) reinterpret_cast<__bf16 *>(dst)[idx] = (__bf16)v;
  else reinterpret_cast<float *>(dst)[idx] = v;
}

__global__ __launch_bounds__(256) void k_pack_weights_jobs(const PackJob *__restrict__ jobs, int n_jobs) {
  __shared__ int sj;
  __shared__ float tile[kPT][kPT + 1];
  if (threadIdx.x == 0) {
    int lo = 0, hi = n_jobs - 1; // last job whose first_block <= blockIdx.x
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (jobs[mid].first_block <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    sj = lo;
  }
  __syncthreads();
  const PackJob jb = jobs[sj];
  const int vol = jb.vol, n_in = jb.n_in, n_out = jb.n_out;
  const int tc = (n_in + kPT - 1) / kPT, tn = (n_out + kPT - 1) / kPT;
  int64_t b = (int64_t)blockIdx.x - jb.first_block;
  const int tj = (int)(b % tn); b /= tn;
  const int ti = (int)(b % tc); b /= tc;
  const int k = (int)b;
  if (k >= vol) return;
  const int c0 = ti * kPT, n0 = tj * kPT;
  // W[k][c0 + r][n0 + q]: 16 threads per row (4 floats each), 16 rows per sweep
  {
    const int q4 = (threadIdx.x & 15) * 4, r0 = threadIdx.x >> 4;
    const float *Wk = jb.W + (int64_t)k * n_in * n_out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = r0 + 16 * j, c = c0 + r;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + q4 + e;
        tile[r][q4 + e] = (c < n_in && n < n_out) ? Wk[(int64_t)c * n_out + n] : 0.0f;
      }
    }
  }
  __syncthreads();
  // forward layout: Wl[c][n] = W[k][c][n], fragments (kc, nb) of 32 channels x 16 columns
  {
    const int nkc = nkc_of(n_in), nnb = nnb_of(n_out);
    const int64_t plane = (int64_t)vol * nkc * nnb * 512;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int e = i * 256 + threadIdx.x, fr = e >> 9, r = e & 511;
      const int lane = r >> 3, sidx = r & 7;
      const int kc = (c0 >> 5) + (fr >> 2), nb = (n0 >> 4) + (fr & 3);
      if (kc >= nkc || nb >= nnb) continue;
      const float v = tile[(fr >> 2) * 32 + (lane >> 4) * 8 + sidx][(fr & 3) * 16 + (lane & 15)];
      pack_store(jb.Wf, (((int64_t)k * nkc + kc) * nnb + nb) * 512 + r, v, jb.bf16, plane);
    }
  }
  // input-gradient layout: Wl[c'][n'] = W[k][n'][c'] (plane counts swapped): c' runs over this tile's columns
  {
    const int nkc = nkc_of(n_out), nnb = nnb_of(n_in);
    const int64_t plane = (int64_t)vol * nkc * nnb * 512;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int e = i * 256 + threadIdx.x, fr = e >> 9, r = e & 511;
      const int lane = r >> 3, sidx = r & 7;
      const int kc = (n0 >> 5) + (fr >> 2), nb = (c0 >> 4) + (fr & 3);
      if (kc >= nkc || nb >= nnb) continue;
      const float v = tile[(fr & 3) * 16 + (lane & 15)][(fr >> 2) * 32 + (lane >> 4) * 8 + sidx];
      pack_store(jb.Wt, (((int64_t)k * nkc + kc) * nnb + nb) * 512 + r, v, jb.bf16, plane);
    }
  }
}

// ------------------------------------------------------------------ compiled rule book, part 1
// Tile-major MFMA block lists.  For every tile of 64 consecutive output rows the gather table
// is compiled ONCE per rule book into blocks of 16 (partner row, local row) pairs that share a
// filter offset; every convolution that uses the rule book (forward of each layer at that scale,
// and the input-gradient passes) then streams these blocks with no ballots and no table reads.
//   words:  [ntiles] nblk | [ntiles][MAXB] offset k of each block | [ntiles][MAXB][16] entries
//   entry = (partner_row << 6) | local_row; padding entries repeat the block's first pair with
//   bit 31 set (gather is valid, result is discarded);  MAXB = 4 * vol  (tb_ntiles, tb_maxb: conv_tile_frame.h).

__global__ __launch_bounds__(256) void k_build_tile_blocks(const StreamJobs js) {      // common.h: one launch, many books
  const int job = stream_job_of(js, blockIdx.x);
  const int32_t *__restrict__ table = js.j[job].table;
  int32_t *__restrict__ words = js.j[job].words;
  const int64_t V = js.j[job].V;
  const int vol = js.j[job].vol;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t ntiles = tb_ntiles(V), tile = (int64_t)(blockIdx.x - js.first[job]) * 4 + wave;
  if (tile >= ntiles) return;
  const int maxb = tb_maxb(vol);
  int32_t *nblk = words;
  int32_t *blk_k = words + ntiles + tile * maxb;
  int32_t *ent = words + ntiles + ntiles * maxb + tile * maxb * 16;
  const int64_t row = tile * 64 + lane;
  const bool valid = row < V;
  int b0 = 0;
  constexpr int B = 9; // table rows fetched per batch: nine independent loads in flight, then nine ballots
  for (int k0 = 0; k0 < vol; k0 += B) {
    int tv[B];
#pragma unroll
    for (int j = 0; j < B; ++j) tv[j] = (valid && k0 + j < vol) ? table[(int64_t)(k0 + j) * V + row] : -1;
#pragma unroll
    for (int j = 0; j < B; ++j) {
    const int k = k0 + j;
    const int t = tv[j];
    const unsigned long long m = __ballot(t >= 0);
    if (m == 0) continue;
    const int cnt = __popcll(m);
    const int pos = __popcll(m & ((1ull << lane) - 1ull));
    const int nmb = (cnt + 15) >> 4;
    const int e = (t << 6) | lane;
    if (t >= 0) ent[b0 * 16 + pos] = e;
    // padding: a copy of the first pair with the discard bit (31) set, so the MFMA kernel can gather
    // unconditionally (no zero-fill selects) and simply drops the result
    const int e_first = __shfl(e, __ffsll((long long)m) - 1);
    if (lane < nmb * 16 - cnt) ent[b0 * 16 + cnt + lane] = e_first | (int)0x80000000;
    if (lane < nmb) blk_k[b0 + lane] = k;
    b0 += nmb;
    }
  }
  if (lane == 0) nblk[tile] = b0;
}

// gather 8 consecutive channels of the block entry's partner row (zeros for padding entries)
template <bool ALIGNED>
__device__ inline void conv_block_load(const float *__restrict__ in, int ci, int e, int g, int kc,
                                       float (&b8)[8]) {
  const int inrow = e >> 6;
  if (ALIGNED) {
    if (e >= 0) {
      const float4 *src = reinterpret_cast<const float4 *>(in + (int64_t)inrow * ci + kc * kKC + g * 8);
      float4 v0 = src[0], v1 = src[1];
      b8[0] = v0.x; b8[1] = v0.y; b8[2] = v0.z; b8[3] = v0.w;
      b8[4] = v1.x; b8[5] = v1.y; b8[6] = v1.z; b8[7] = v1.w;
    } else {
#pragma unroll
      for (int s = 0; s < 8; ++s) b8[s] = 0.0f;
    }
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      int c = kc * kKC + g * 8 + s;
      b8[s] = (e >= 0 && c < ci) ? in[(int64_t)inrow * ci + c] : 0.0f;
    }
  }
}

// gathered operands of one pipeline step: the same 32-channel chunk of two blocks (A, B)
struct ConvStep {
  float a8[8], b8[8];
  int eA, eB;
};

// weights stream from L2 (packed, lane-linear, 2 KiB per block and chunk) right before their MFMAs;
// the two blocks' chains are interleaved: two independent accumulators keep the 40-cycle
// dependent latency of v_mfma_f32_16x16x4_f32 off the critical path
template <int NBW>
__device__ inline void conv_step_mfma(const ConvStep &st, const float *__restrict__ WkA,
                                      const float *__restrict__ WkB, int kc, int nnb, int nb0, int lane,
                                      f32x4 (&accA)[NBW], f32x4 (&accB)[NBW]) {
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    if (nb0 + j < nnb) {
      const int64_t off = (((int64_t)kc * nnb + nb0 + j) * 64 + lane) * 8;
      const float4 *wa = reinterpret_cast<const float4 *>(WkA + off);
      const float4 *wb = reinterpret_cast<const float4 *>(WkB + off);
      const float4 w0 = wa[0], w1 = wa[1], u0 = wb[0], u1 = wb[1];
      accA[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, st.a8[0], accA[j], 0, 0, 0);
      accB[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u0.x, st.b8[0], accB[j], 0, 0, 0);
      accA[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, st.a8[1], accA[j], 0, 0, 0);
      accB[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u0.y, st.b8[1], accB[j], 0, 0, 0);
      accA[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, st.a8[2], accA[j], 0, 0, 0);
      accB[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u0.z, st.b8[2], accB[j], 0, 0, 0);
      accA[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, st.a8[3], accA[j], 0, 0, 0);
      accB[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u0.w, st.b8[3], accB[j], 0, 0, 0);
      accA[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, st.a8[4], accA[j], 0, 0, 0);
      accB[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u1.x, st.b8[4], accB[j], 0, 0, 0);
      accA[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, st.a8[5], accA[j], 0, 0, 0);
      accB[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u1.y, st.b8[5], accB[j], 0, 0, 0);
      accA[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, st.a8[6], accA[j], 0, 0, 0);
      accB[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u1.z, st.b8[6], accB[j], 0, 0, 0);
      accA[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, st.a8[7], accA[j], 0, 0, 0);
      accB[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(u1.w, st.b8[7], accB[j], 0, 0, 0);
    }
  }
}

// One workgroup owns a tile of 64 output rows x (NBW*16) output columns.  Its WPB waves take
// the tile's blocks round-robin, two blocks per step, and software-pipeline three stages in
// registers: block entries two pairs ahead, weights + gathered rows one step ahead, MFMAs now.
// Each wave accumulates into a private LDS tile; the tiles are summed in wave order at the end,
// so the result is bit-reproducible.  ALIGNED: ci % 32 == 0 (float4 gathers, no bounds checks).
// Flat 64-bit addressing (buffers of 2 GiB and more): of the shared frame it takes the descriptor-free TileLanes.
template <int NBW, int WPB, bool ALIGNED>
__global__ __launch_bounds__(WPB * 64, (NBW <= 2 ? 3 : 2)) void k_conv_blocks_mfma(const float *__restrict__ in, int ci,
                                                              float *__restrict__ out, int co,
                                                              int64_t V_out, const int32_t *__restrict__ words,
                                                              int vol, int wflip, const float *__restrict__ Wp,
                                                              const float *__restrict__ bias) {
  extern __shared__ __align__(16) float smem[];
  const TileLanes<NBW> c = tile_lanes<NBW>(smem, nkc_of(ci), co);
  const int wave = c.wave, lane = c.lane, g = c.g, c16 = c.c16, nkc = c.nkc, nnb = c.nnb, nb0 = c.nb0;
  const int maxb = tb_maxb(vol);
  const int64_t tile = blockIdx.x, row0 = tile * 64;
  const int64_t ntiles = tb_ntiles(V_out);
  const int nblk = words[tile];
  const int32_t *blk_k = words + ntiles + tile * maxb;
  const int32_t *ent = words + ntiles + ntiles * maxb + tile * maxb * 16;
  const int64_t wk_stride = (int64_t)nkc * nnb * 512;
  zero_tile(c);
  const int dbg = wflip >> 8; // timing experiments only (tools_conv_bench.py): 1 = no MFMAs, 2 = no gathers
  wflip &= 1;

  // this wave's blocks: wave, wave + WPB, ...; consumed two per pair
  const int nmine = (wave < nblk && !(dbg & 4)) ? (nblk - wave + WPB - 1) / WPB : 0; // dbg 4: skip the main loop
  const int npairs = (nmine + 1) >> 1;
  auto load_pair = [&](int pr) {
    PairEnt p;
    const int bA = wave + (2 * pr) * WPB, bB = bA + WPB;
    if (pr < npairs) {
      const bool hasB = bB < nblk;
      p.eA = ent[bA * 16 + c16];
      p.eB = hasB ? ent[bB * 16 + c16] : -1;
      p.kA = blk_k[bA];
      p.kB = hasB ? blk_k[bB] : p.kA;
    } else {
      p.eA = p.eB = -1; p.kA = p.kB = 0;
    }
    return p;
  };
  auto fetch = [&](ConvStep &st, const PairEnt &p, int kc) {
    st.eA = p.eA; st.eB = p.eB;
    conv_block_load<ALIGNED>(in, ci, st.eA, g, kc, st.a8);
    conv_block_load<ALIGNED>(in, ci, st.eB, g, kc, st.b8);
  };
  PairEnt p0 = load_pair(0), p1 = load_pair(1), p2 = load_pair(2);
  ConvStep cur, nxt;
  if (npairs > 0) fetch(cur, p0, 0);
  f32x4 accA[NBW], accB[NBW];
  for (int pr = 0; pr < npairs; ++pr) {
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      accA[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      accB[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int kA = __builtin_amdgcn_readfirstlane(p0.kA), kB = __builtin_amdgcn_readfirstlane(p0.kB);
    if (wflip) { kA = vol - 1 - kA; kB = vol - 1 - kB; }
    const float *WkA = Wp + kA * wk_stride, *WkB = Wp + kB * wk_stride;
    for (int kc = 0; kc < nkc; ++kc) {
      // the gathers of the following step go in flight before this step's MFMAs issue
      if (!(dbg & 2)) {
        if (kc + 1 < nkc) fetch(nxt, p0, kc + 1);
        else if (pr + 1 < npairs) fetch(nxt, p1, 0);
      }
      if (!(dbg & 1)) conv_step_mfma<NBW>(cur, WkA, WkB, kc, nnb, nb0, lane, accA, accB);
      cur = nxt;
    }
    accumulate_pair<NBW>(c.Ct, p0.eA, p0.eB, g, accA, accB);
    p0 = p1; p1 = p2; p2 = load_pair(pr + 3);
  }
  __syncthreads();
  tile_epilogue<NBW, WPB, WPB * 64, true>(smem, threadIdx.x, out, co, V_out, row0, nb0, bias);
}

// Lean variant for ci % 32 == 0 and tensors < 2 GiB: every load goes through a buffer descriptor
// (32-bit per-lane offsets, wave-uniform parts in SGPRs, hardware range check), padding entries are
// gathered like real ones, the step registers ping-pong (no copies) and the first MFMA of a chain
// takes a literal zero accumulator.  fp32 MFMA shares the vector datapath with the VALU on gfx950
// (ablation: kernel time = MFMA time + everything-else time), so every VALU instruction removed
// from the loop is time given back to the matrix pipe.
template <int NBW, bool ADJ>
__device__ inline void conv_step_mfma_buf(const GStep &q, __amdgpu_buffer_rsrc_t rw, unsigned lane32,
                                          unsigned soA, unsigned soB, int nvalid, f32x4 (&accA)[NBW],
                                          f32x4 (&accB)[NBW]) {
  const bool same = ADJ && soA == soB; // adjacent blocks of one offset: one set of weight fragments (wave-uniform)
  // all of the step's weight loads go out before its first MFMA: the L2 latency is paid once per
  // step, not once per column block (the last column slab may hold fewer than NBW blocks)
  u32x4 w0[NBW], w1[NBW], u0[NBW], u1[NBW];
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    if (j < nvalid) {
      w0[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32, soA + j * 2048, 0);
      w1[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32 + 16, soA + j * 2048, 0);
      if (!same) {
        u0[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32, soB + j * 2048, 0);
        u1[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32 + 16, soB + j * 2048, 0);
      }
    }
  }
  if (same) {
#pragma unroll
    for (int j = 0; j < NBW; ++j)
      if (j < nvalid) { u0[j] = w0[j]; u1[j] = w1[j]; }
  }
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    if (j < nvalid) {
      f32x4 ca = accA[j], cb = accB[j];
      AABR_MFMA16(ca, cb, w0[j], w1[j], u0[j], u1[j], q.a0, q.a1, q.b0, q.b1);
      accA[j] = ca; accB[j] = cb;
    }
  }
}

template <int NBW, int WPB, bool ADJ, bool ALIGNED>
__global__ __launch_bounds__(WPB * 64, (NBW <= 2 ? 3 : 2)) void k_conv_blocks_mfma_buf(
    const float *__restrict__ in, int ci, int64_t in_bytes, float *__restrict__ out, int co, int64_t V_out,
    const int32_t *__restrict__ words, int64_t words_bytes, int vol, int wflip, const float *__restrict__ Wp,
    int64_t wp_bytes, const float *__restrict__ bias) {
  extern __shared__ __align__(16) float smem[];
  const int64_t tile = blockIdx.x;
  const TileCtx<NBW, 4> c = tile_ctx<NBW, 4>(smem, tile, in, ci, in_bytes, ALIGNED ? (ci >> 5) : nkc_of(ci), co, V_out, words,
                                             words_bytes, vol, Wp, wp_bytes);
  const int nkc = c.nkc;
  const int npairs = pair_count<ADJ, WPB>(c.wave, c.nblk);
  auto load_pair = [&](int pr) {
    int bA, bB;
    pair_blocks<ADJ, WPB>(c.wave, pr, c.nblk, bA, bB);
    return load_block_pair(c, bA, bB);
  };
  auto gather = [&](GStep &q, const PairEnt &p, int kc) { gather_rows<ALIGNED>(c, ci, p, kc, q.a0, q.a1, q.b0, q.b1); };
  PairEnt p0 = load_pair(0), p1 = load_pair(1), p2 = load_pair(2);
  GStep s0, s1;
  if (npairs > 0) gather(s0, p0, 0);
  f32x4 accA[NBW], accB[NBW];
  int step = 0; // parity selects the ping-pong register set
  for (int pr = 0; pr < npairs; ++pr) {
    int kA = __builtin_amdgcn_readfirstlane(p0.kA), kB = __builtin_amdgcn_readfirstlane(p0.kB);
    if (wflip) { kA = vol - 1 - kA; kB = vol - 1 - kB; }
    const unsigned soA0 = (unsigned)kA * c.wk_bytes + (unsigned)c.nb0 * 2048u;
    const unsigned soB0 = (unsigned)kB * c.wk_bytes + (unsigned)c.nb0 * 2048u;
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      accA[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      accB[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    for (int kc = 0; kc < nkc; ++kc, ++step) {
      const bool more = (kc + 1 < nkc) || (pr + 1 < npairs);
      const PairEnt &pn = (kc + 1 < nkc) ? p0 : p1;
      const int kcn = (kc + 1 < nkc) ? kc + 1 : 0;
      const unsigned so = (unsigned)kc * c.kc_bytes;
      if (step & 1) {
        if (more) gather(s0, pn, kcn);
        conv_step_mfma_buf<NBW, ADJ>(s1, c.rw, c.laneofs, soA0 + so, soB0 + so, c.nvalid, accA, accB);
      } else {
        if (more) gather(s1, pn, kcn);
        conv_step_mfma_buf<NBW, ADJ>(s0, c.rw, c.laneofs, soA0 + so, soB0 + so, c.nvalid, accA, accB);
      }
    }
    accumulate_pair<NBW>(c.Ct, p0.eA, p0.eB, c.g, accA, accB);
    p0 = p1; p1 = p2; p2 = load_pair(pr + 3);
  }
  __syncthreads();
  tile_epilogue<NBW, WPB, WPB * 64, true>(smem, threadIdx.x, out, co, V_out, tile * 64, c.nb0, bias);
}

// packed weights of JG column blocks for the two blocks (A, B) of a step: JG x 4 x 16 B per lane
template <int JG> struct WSet { u32x4 a0[JG], a1[JG], b0[JG], b1[JG]; };

template <int JG>
__device__ inline void conv_load_w(WSet<JG> &w, __amdgpu_buffer_rsrc_t rw, unsigned lane32, unsigned soA,
                                   unsigned soB, int nvalid) {
#pragma unroll
  for (int j = 0; j < JG; ++j) {
    if (j < nvalid) { // last column slab may hold fewer blocks (wave-uniform)
      w.a0[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32, soA + j * 2048, 0);
      w.a1[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32 + 16, soA + j * 2048, 0);
      w.b0[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32, soB + j * 2048, 0);
      w.b1[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32 + 16, soB + j * 2048, 0);
    }
  }
}

template <int JG>
__device__ inline void conv_step_mfma_w(const GStep &q, const WSet<JG> &w, int nvalid, f32x4 *accA, f32x4 *accB) {
#pragma unroll
  for (int j = 0; j < JG; ++j) {
    if (j < nvalid) {
      f32x4 ca = accA[j], cb = accB[j];
      AABR_MFMA16(ca, cb, w.a0[j], w.a1[j], w.b0[j], w.b1[j], q.a0, q.a1, q.b0, q.b1);
      accA[j] = ca; accB[j] = cb;
    }
  }
}

// the two blocks of a pair are ADJACENT in the tile's (offset-sorted) list in the weight-prefetching
// kernel, so they often share the filter offset (the centre offset alone fills four blocks of a 64-row
// tile): then one set of weight fragments feeds both MFMA chains and the second fetch is skipped
template <int JG>
__device__ inline void conv_load_w_shared(WSet<JG> &w, __amdgpu_buffer_rsrc_t rw, unsigned lane32, unsigned soA,
                                          unsigned soB, int nvalid) {
#pragma unroll
  for (int j = 0; j < JG; ++j) {
    if (j < nvalid) {
      w.a0[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32, soA + j * 2048, 0);
      w.a1[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32 + 16, soA + j * 2048, 0);
      if (soA != soB) { // wave-uniform
        w.b0[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32, soB + j * 2048, 0);
        w.b1[j] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32 + 16, soB + j * 2048, 0);
      }
    }
  }
}

template <int JG, bool ADJ>
__device__ inline void conv_load_w_sel(WSet<JG> &w, __amdgpu_buffer_rsrc_t rw, unsigned lane32, unsigned soA,
                                       unsigned soB, int nvalid) {
  if (ADJ) conv_load_w_shared<JG>(w, rw, lane32, soA, soB, nvalid);
  else conv_load_w<JG>(w, rw, lane32, soA, soB, nvalid);
}

template <int JG>
__device__ inline void conv_step_mfma_w_shared(const GStep &q, const WSet<JG> &w, bool same, int nvalid, f32x4 *accA,
                                               f32x4 *accB) {
  if (!same) {
    conv_step_mfma_w<JG>(q, w, nvalid, accA, accB);
    return;
  }
#pragma unroll
  for (int j = 0; j < JG; ++j) {
    if (j < nvalid) {
      f32x4 ca = accA[j], cb = accB[j];
      // same weights for both blocks: the two chains stay interleaved through the scheduler
      AABR_MFMA8(ca, w.a0[j], w.a1[j], q.a0, q.a1);
      AABR_MFMA8(cb, w.a0[j], w.a1[j], q.b0, q.b1);
      accA[j] = ca; accB[j] = cb;
    }
  }
}

// weights streamed right before their MFMAs, one column block at a time (16 VGPRs live)
template <int NBW>
__device__ inline void conv_step_mfma_stream(const GStep &q, __amdgpu_buffer_rsrc_t rw, unsigned lane32,
                                             unsigned soA, unsigned soB, int nvalid, f32x4 *accA, f32x4 *accB) {
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    if (j >= nvalid) break; // last column slab may hold fewer than NBW blocks (wave-uniform)
    WSet<1> w;
    conv_load_w<1>(w, rw, lane32, soA + j * 2048, soB + j * 2048, 1);
    conv_step_mfma_w<1>(q, w, 1, accA + j, accB + j);
  }
}

// Three register-resident prefetch streams per wave: block entries two pairs ahead, gathered rows one
// step ahead, packed weights one micro-step (JG column blocks) ahead -- no load is waited on in the
// step that issues it.
// WPIPE: prefetch the packed weights one micro-step ahead (pays for wide slabs, NBW = 4; with narrow
// slabs the extra 32-64 VGPRs cost a wave of occupancy and the step is too short to need it).
// ADJ: pairs are ADJACENT blocks of the tile's list and share their weight fragments when they share the
// offset (less L2->CU traffic: pays when the launch is throughput-bound, i.e. thousands of workgroups;
// on small launches the longer loop body costs more than it saves)
template <int NBW, int WPB, bool WPIPE, bool ADJ>
__global__ __launch_bounds__(WPB * 64, 2) void k_conv_blocks_mfma_wpipe(
    const float *__restrict__ in, int ci, int64_t in_bytes, float *__restrict__ out, int co, int64_t V_out,
    const int32_t *__restrict__ words, int64_t words_bytes, int vol, int wflip, const float *__restrict__ Wp,
    int64_t wp_bytes, const float *__restrict__ bias) {
  constexpr int JG = NBW >= 2 ? 2 : 1;      // column blocks per weight set
  constexpr int NJG = NBW / JG;             // weight sets (micro-steps) per step
  extern __shared__ __align__(16) float smem[];
  const int64_t tile = blockIdx.x;
  const TileCtx<NBW, 4> c = tile_ctx<NBW, 4>(smem, tile, in, ci, in_bytes, ci >> 5, co, V_out, words, words_bytes, vol, Wp,
                                             wp_bytes);
  const int npairs = pair_count<ADJ, WPB>(c.wave, c.nblk);
  auto load_pair = [&](int pr) {
    int bA, bB;
    pair_blocks<ADJ, WPB>(c.wave, pr, c.nblk, bA, bB);
    return load_block_pair(c, bA, bB);
  };
  auto gather = [&](GStep &q, const PairEnt &p, int kc) { gather_rows<true>(c, ci, p, kc, q.a0, q.a1, q.b0, q.b1); };
  // byte offsets (wave-uniform) of a pair's packed weights for this column slab
  auto w_base = [&](int k) {
    if (wflip) k = vol - 1 - k;
    return (unsigned)k * c.wk_bytes + (unsigned)c.nb0 * 2048u;
  };
  // block entries run three pairs ahead: a pair's offsets (wave-uniform, needed one step early for the
  // weight prefetch) have been in flight for two pairs when they are first read, so waiting for them
  // does not drain the younger gathers behind them in the in-order VMEM queue
  PairEnt p0 = load_pair(0), p1 = load_pair(1), p2 = load_pair(2), p3 = load_pair(3);
  GStep s0, s1;
  WSet<JG> w0, w1;
  f32x4 accA[NBW], accB[NBW];
  unsigned soA = w_base(__builtin_amdgcn_readfirstlane(p0.kA)), soB = w_base(__builtin_amdgcn_readfirstlane(p0.kB));
  unsigned soA1 = 0, soB1 = 0;
  if (WPIPE) {
    soA1 = w_base(__builtin_amdgcn_readfirstlane(p1.kA));
    soB1 = w_base(__builtin_amdgcn_readfirstlane(p1.kB));
  }
  if (npairs > 0) {
    gather(s0, p0, 0);
    if (WPIPE) conv_load_w_sel<JG, ADJ>(w0, c.rw, c.laneofs, soA, soB, c.nvalid);
  }
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    accA[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    accB[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  int pr = 0, kc = 0;
  // one step = one 32-channel chunk of one pair of blocks; the register sets a step reads and the
  // ones it prefetches into are fixed by the call site (the loop below is unrolled by two), so the
  // ping-pong costs no register moves
  auto do_step = [&](const GStep &xc, GStep &xn, WSet<JG> &wc, WSet<JG> &wo) {
    // loop state is wave-uniform; say so (keeps the buffer soffsets in SGPRs, no waterfall loops)
    kc = __builtin_amdgcn_readfirstlane(kc); pr = __builtin_amdgcn_readfirstlane(pr);
    soA = __builtin_amdgcn_readfirstlane(soA); soB = __builtin_amdgcn_readfirstlane(soB);
    const bool last_kc = kc + 1 == c.nkc;
    const bool more = !last_kc || (pr + 1 < npairs);
    const PairEnt &pn = last_kc ? p1 : p0;
    const int kcn = last_kc ? 0 : kc + 1;
    if (more) gather(xn, pn, kcn);
    const unsigned cA = soA + (unsigned)kc * c.kc_bytes, cB = soB + (unsigned)kc * c.kc_bytes;
    if (!WPIPE) {
      // weights stream from L2 right before their MFMAs (other waves cover the latency)
      conv_step_mfma_stream<NBW>(xc, c.rw, c.laneofs, cA, cB, c.nvalid, accA, accB);
    } else {
      soA1 = __builtin_amdgcn_readfirstlane(soA1); soB1 = __builtin_amdgcn_readfirstlane(soB1);
      const unsigned nA = last_kc ? soA1 : cA + c.kc_bytes; // first weight set of the next step
      const unsigned nB = last_kc ? soB1 : cB + c.kc_bytes;
      const bool same = ADJ && soA == soB; // both blocks of the pair use the same filter offset (wave-uniform)
      if (NJG == 1) {
        if (more) conv_load_w_sel<JG, ADJ>(wo, c.rw, c.laneofs, nA, nB, c.nvalid);
        conv_step_mfma_w_shared<JG>(xc, wc, same, c.nvalid, accA, accB);
      } else {
        conv_load_w_sel<JG, ADJ>(wo, c.rw, c.laneofs, cA + JG * 2048u, cB + JG * 2048u, c.nvalid - JG);
        conv_step_mfma_w_shared<JG>(xc, wc, same, c.nvalid, accA, accB);
        if (more) conv_load_w_sel<JG, ADJ>(wc, c.rw, c.laneofs, nA, nB, c.nvalid);
        conv_step_mfma_w_shared<JG>(xc, wo, same, c.nvalid - JG, accA + JG, accB + JG);
      }
    }
    if (last_kc) {
      accumulate_pair<NBW>(c.Ct, p0.eA, p0.eB, c.g, accA, accB);
#pragma unroll
      for (int j = 0; j < NBW; ++j) {
        accA[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        accB[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      p0 = p1; p1 = p2; p2 = p3; p3 = load_pair(pr + 4);
      if (WPIPE) {
        soA = soA1; soB = soB1;
        soA1 = w_base(__builtin_amdgcn_readfirstlane(p1.kA));
        soB1 = w_base(__builtin_amdgcn_readfirstlane(p1.kB));
      } else {
        soA = w_base(__builtin_amdgcn_readfirstlane(p0.kA));
        soB = w_base(__builtin_amdgcn_readfirstlane(p0.kB));
      }
      kc = 0; ++pr;
    } else {
      ++kc;
    }
  };
  while (pr < npairs) {
    if (NJG == 1) {
      do_step(s0, s1, w0, w1);
      if (pr >= npairs) break;
      do_step(s1, s0, w1, w0);
    } else {
      do_step(s0, s1, w0, w1);
      if (pr >= npairs) break;
      do_step(s1, s0, w0, w1);
    }
  }
  __syncthreads();
  tile_epilogue<NBW, WPB, WPB * 64, true>(smem, threadIdx.x, out, co, V_out, tile * 64, c.nb0, bias);
}

// ------------------------------------------------------------------ tiny rule books
// The coarse FPN scales have 1-50 tiles and 128-256 planes: a launch of the kernels above is a handful of
// workgroups walking 30-40 dependent (pair, channel-chunk) steps each (60 us for ~50 M MACs).  This variant
// cuts the work finer: 16 output columns per workgroup, 8 waves, and the unit dealt to a wave is one
// 32-channel chunk of one block pair, so a tile's ~15 pairs x 4-8 chunks spread over 8 waves x (co/16)
// workgroups.  Every item ends with its own LDS accumulate (private tile per wave, summed in wave order:
// still deterministic).  Gathers and weights are prefetched one item ahead (fixed register sets).
template <int WPB>
__global__ __launch_bounds__(WPB * 64, 1) void k_conv_blocks_mfma_small(
    const float *__restrict__ in, int ci, int64_t in_bytes, float *__restrict__ out, int co, int64_t V_out,
    const int32_t *__restrict__ words, int64_t words_bytes, int vol, int wflip, const float *__restrict__ Wp,
    int64_t wp_bytes, const float *__restrict__ bias) {
  extern __shared__ __align__(16) float smem[];
  const int64_t tile = blockIdx.x;
  const TileCtx<1, 4> c = tile_ctx<1, 4>(smem, tile, in, ci, in_bytes, ci >> 5, co, V_out, words, words_bytes, vol, Wp, wp_bytes);
  const int wave = c.wave, nkc = c.nkc, nblk = c.nblk;

  const int nitems = ((nblk + 1) >> 1) * nkc;               // (block pair, channel chunk)
  const int nmine = wave < nitems ? (nitems - wave + WPB - 1) / WPB : 0;
  auto load_item = [&](int j) {                             // this wave's j-th item
    int it = wave + j * WPB;
    if (it >= nitems) it = nitems > 0 ? nitems - 1 : 0;     // past the end: harmless re-read, never consumed
    int bA = 2 * (it / nkc);
    if (bA >= nblk) bA = 0;
    return load_block_pair(c, bA, bA + 1);
  };
  auto kc_of = [&](int j) {
    int it = wave + j * WPB;
    if (it >= nitems) it = nitems > 0 ? nitems - 1 : 0;
    return it % nkc;
  };
  auto fetch = [&](GStep &q, WSet<1> &w, const PairEnt &p, int kc) {
    gather_rows<true>(c, ci, p, kc, q.a0, q.a1, q.b0, q.b1);
    int kA = __builtin_amdgcn_readfirstlane(p.kA), kB = __builtin_amdgcn_readfirstlane(p.kB);
    if (wflip) { kA = vol - 1 - kA; kB = vol - 1 - kB; }
    const unsigned off = (unsigned)kc * c.kc_bytes + (unsigned)c.nb0 * 2048u;
    conv_load_w<1>(w, c.rw, c.laneofs, (unsigned)kA * c.wk_bytes + off, (unsigned)kB * c.wk_bytes + off, 1);
  };
  auto compute = [&](const GStep &q, const WSet<1> &w, const PairEnt &p) {
    f32x4 accA[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}}, accB[1] = {(f32x4){0.f, 0.f, 0.f, 0.f}};
    conv_step_mfma_w<1>(q, w, 1, accA, accB);
    accumulate_pair<1>(c.Ct, p.eA, p.eB, c.g, accA, accB);
  };
  PairEnt e0 = load_item(0), e1 = load_item(1), e2 = load_item(2);
  GStep s0, s1;
  WSet<1> w0, w1;
  if (nmine > 0) fetch(s0, w0, e0, kc_of(0));
  for (int j = 0; j < nmine; j += 2) {
    if (j + 1 < nmine) fetch(s1, w1, e1, kc_of(j + 1));
    compute(s0, w0, e0);
    PairEnt e3 = load_item(j + 3);
    if (j + 1 < nmine) {
      if (j + 2 < nmine) fetch(s0, w0, e2, kc_of(j + 2));
      compute(s1, w1, e1);
    }
    PairEnt e4 = load_item(j + 4);
    e0 = e2; e1 = e3; e2 = e4;
  }
  __syncthreads();
  // the scalar path only (VEC = false): this kernel never had the vector one, and its speed is tuned as it is
  tile_epilogue<1, WPB, WPB * 64, false>(smem, threadIdx.x, out, co, V_out, tile * 64, c.nb0, bias);
}

// ------------------------------------------------------------------ LDS-resident weights
// For layers whose whole packed filter bank fits in LDS next to the output tiles
// (vol * ceil(ci/32) * ceil(co/16) * 2 KiB <= ~110 KiB: 3x3x3 at <=32->32 planes, the 2x2x2 strided
// layers at 32<->64) the weights are copied to LDS once per workgroup and every MFMA A-operand is a
// conflict-free ds_read_b128.  The lean kernel above streams 2 KiB of weights through the vector
// memory path per 16-pair block and chunk -- twice the bytes of the gathered rows -- and the L2->CU
// path (~70 GB/s per CU measured, MI355X_MICROARCH.md "Indexed rows") is what bounds it; here that
// path carries only the gathered rows.  One wave owns one 64-row tile end to end (all its blocks,
// all output columns): no cross-wave summation, no barrier after the weight copy, and the grid is
// persistent (waves loop over tiles).  Same block order per tile => same bits as the other kernels.
//   LDS image:  Wl[k][kc][nb][half][lane][4]   (half h holds k-slots 4h..4h+3 of the 8 per lane)
template <int NBW>
__device__ inline void conv_step_mfma_lds(const GStep &q, const float *__restrict__ WA,
                                          const float *__restrict__ WB, int lane, f32x4 (&accA)[NBW],
                                          f32x4 (&accB)[NBW]) {
#pragma unroll
  for (int j = 0; j < NBW; ++j) {
    const f32x4 w0 = *reinterpret_cast<const f32x4 *>(WA + j * 512 + lane * 4);
    const f32x4 w1 = *reinterpret_cast<const f32x4 *>(WA + j * 512 + 256 + lane * 4);
    const f32x4 u0 = *reinterpret_cast<const f32x4 *>(WB + j * 512 + lane * 4);
    const f32x4 u1 = *reinterpret_cast<const f32x4 *>(WB + j * 512 + 256 + lane * 4);
    f32x4 ca = accA[j], cb = accB[j];
    AABR_MFMA16(ca, cb, w0, w1, u0, u1, q.a0, q.a1, q.b0, q.b1);
    accA[j] = ca; accB[j] = cb;
  }
}

// NBW = column blocks per workgroup slab (blockIdx.y selects the slab), NKC = ceil(ci/32); the
// number of waves per workgroup is the launch's block size / 64.  Gathers run RING-1 pairs ahead of
// the MFMAs and block entries 2*RING-1 pairs ahead (registers, static ring indices through an
// unrolled loop): with one or two waves per SIMD the latency has to be hidden inside the wave.
template <int NKC> struct WStage { u32x4 a0[NKC], a1[NKC], b0[NKC], b1[NKC]; };

template <int NBW, int NKC, bool ALIGNED>
__global__ __launch_bounds__(512, 1) void k_conv_blocks_mfma_wlds(
    const float *__restrict__ in, int ci, int64_t in_bytes, float *__restrict__ out, int co, int64_t V_out,
    const int32_t *__restrict__ words, int64_t words_bytes, int vol, int wflip, const float *__restrict__ Wp,
    const float *__restrict__ bias) {
  constexpr int RING = 4;
  extern __shared__ __align__(16) float smem[];
  const int NW = blockDim.x >> 6;
  const int wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nnb = nnb_of(co);
  const int nb0 = blockIdx.y * NBW;
  const int nvalid = (nnb - nb0) < NBW ? (nnb - nb0) : NBW;
  const int wfloats = vol * NKC * NBW * 512;
  float *Wl = smem;
  // ---- weight copy: global [k][kc][nb][lane][8] -> LDS [k][kc][j = nb - nb0][half][lane][4]
  for (int i = threadIdx.x; i < vol * NKC * NBW * 128; i += blockDim.x) {
    const int f = i >> 7, r = i & 127, ln = r >> 1, h = r & 1;
    const int kk = f / NBW, j = f - kk * NBW; // kk = k*NKC + kc
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < nvalid) v = *reinterpret_cast<const float4 *>(Wp + ((size_t)(kk * nnb + nb0 + j) * 128 + r) * 4);
    *reinterpret_cast<float4 *>(Wl + ((kk * NBW + j) * 2 + h) * 256 + ln * 4) = v;
  }
  __syncthreads();
  const int64_t ntiles = tb_ntiles(V_out);
  constexpr int kstride = NKC * NBW * 512; // floats per offset in the LDS image

  for (int64_t tile = (int64_t)blockIdx.x * NW + wave0; tile < ntiles; tile += (int64_t)gridDim.x * NW) {
    // the context of this tile (the weights are in LDS: no descriptor for them); the wave's C tile follows the image
    TileCtx<NBW, 4> c = tile_ctx<NBW, 4>(smem + wfloats, tile, in, ci, in_bytes, NKC, co, V_out, words, words_bytes, vol,
                                         (const float *)nullptr, 0);
    c.nblk = __builtin_amdgcn_readfirstlane(c.nblk);
    const int npairs = (c.nblk + 1) >> 1;
    auto load_pair = [&](int pr) {
      int bA = 2 * pr;
      if (bA >= c.nblk) bA = c.nblk > 0 ? c.nblk - 1 : 0; // past the end: harmless re-read, never consumed
      return load_block_pair(c, bA, bA + 1);
    };
    auto gather = [&](WStage<NKC> &q, const PairEnt &p) {
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) gather_rows<ALIGNED>(c, ci, p, kc, q.a0[kc], q.a1[kc], q.b0[kc], q.b1[kc]);
    };
    auto compute = [&](const WStage<NKC> &q, const PairEnt &p) {
      int kA = __builtin_amdgcn_readfirstlane(p.kA), kB = __builtin_amdgcn_readfirstlane(p.kB);
      if (wflip) { kA = vol - 1 - kA; kB = vol - 1 - kB; }
      const float *WA0 = Wl + kA * kstride, *WB0 = Wl + kB * kstride;
      f32x4 accA[NBW], accB[NBW];
#pragma unroll
      for (int j = 0; j < NBW; ++j) {
        accA[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        accB[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        GStep t;
        t.a0 = q.a0[kc]; t.a1 = q.a1[kc]; t.b0 = q.b0[kc]; t.b1 = q.b1[kc];
        conv_step_mfma_lds<NBW>(t, WA0 + kc * NBW * 512, WB0 + kc * NBW * 512, c.lane, accA, accB);
      }
      accumulate_pair<NBW>(c.Ct, p.eA, p.eB, c.g, accA, accB);
    };
    PairEnt p[2 * RING];
    WStage<NKC> st[RING];
#pragma unroll
    for (int u = 0; u < 2 * RING - 1; ++u) p[u] = load_pair(u);
#pragma unroll
    for (int u = 0; u < RING - 1; ++u)
      if (u < npairs) gather(st[u], p[u]);
    for (int pr0 = 0; pr0 < npairs; pr0 += 2 * RING) {
#pragma unroll
      for (int u = 0; u < 2 * RING; ++u) {
        const int pr = pr0 + u;
        if (pr < npairs) {
          p[(u + 2 * RING - 1) % (2 * RING)] = load_pair(pr + 2 * RING - 1);
          if (pr + RING - 1 < npairs) gather(st[(u + RING - 1) % RING], p[(u + RING - 1) % (2 * RING)]);
          compute(st[u % RING], p[u]);
        }
      }
    }
    // the wave's own tile goes out once: one tile, 64 lanes
    tile_epilogue<NBW, 1, 64, true>(c.Ct, c.lane, out, co, V_out, tile * 64, c.nb0, bias);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // tile reads done before the next tile's zero fill
  }
}

// ------------------------------------------------------------------ bf16 features (extension)
// The reference is fp32-only (sparseconvnet_cuda.cpp instantiates <float>); BASELINE configs 3-5 ask
// for bf16.  Features are stored bf16, weights stay fp32 master parameters and are packed to bf16
// per call, accumulation is fp32 (v_mfma_f32_16x16x32_bf16: one instruction covers the 32-channel
// chunk that takes eight fp32 MFMAs), the LDS output tile is fp32 and is rounded to bf16 once at
// the final store.  Same tile-block streams, same determinism.  Requires ci % 32 == 0.

__device__ inline float bf2f(__bf16 v) { return (float)v; }

// Wp16[k][kc][nb][lane][j] = bf16(Wl[k][kc*32 + (lane>>4)*8 + j][nb*16 + (lane&15)])
__global__ __launch_bounds__(256) void k_pack_weights_bf16(const float *__restrict__ W, int vol, int ci, int co,
                                                           int transpose, __bf16 *__restrict__ Wp) {
  const int nkc = nkc_of(ci), nnb = nnb_of(co);
  int64_t total = (int64_t)vol * nkc * nnb * 512;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int s = idx & 7;
  int lane = (idx >> 3) & 63;
  int64_t r = idx >> 9;
  int nb = (int)(r % nnb); r /= nnb;
  int kc = (int)(r % nkc); r /= nkc;
  int k = (int)r;
  int c = kc * kKC + (lane >> 4) * 8 + s;
  int n = nb * 16 + (lane & 15);
  float v = 0.0f;
  if (c < ci && n < co) v = transpose ? W[((int64_t)k * co + n) * ci + c] : W[((int64_t)k * ci + c) * co + n];
  Wp[idx] = (__bf16)v;
}

// KG = channel chunks (of 32) gathered per work item; an item is (pair of blocks, chunk group).
template <int NBW, int WPB, int KG, bool ADJ>
__global__ __launch_bounds__(WPB * 64, 2) void k_conv_blocks_mfma_bf16(
    const __bf16 *__restrict__ in, int ci, int64_t in_bytes, __bf16 *__restrict__ out, int co, int64_t V_out,
    const int32_t *__restrict__ words, int64_t words_bytes, int vol, int wflip, const __bf16 *__restrict__ Wp,
    int64_t wp_bytes, const float *__restrict__ bias) {
  extern __shared__ __align__(16) float smem[];
  const int64_t tile = blockIdx.x;
  const TileCtx<NBW, 2> c = tile_ctx<NBW, 2>(smem, tile, in, ci, in_bytes, ci / kKC, co, V_out, words, words_bytes, vol, Wp,
                                             wp_bytes);
  const int nkc = c.nkc;
  const int ngrp = (nkc + KG - 1) / KG;
  const int nitems = pair_count<ADJ, WPB>(c.wave, c.nblk) * ngrp;
  struct Item : PairEnt { int kc0; };
  auto load_item = [&](int it) {
    Item p;
    const int pr = it / ngrp;
    int bA, bB;
    pair_blocks<ADJ, WPB>(c.wave, pr, c.nblk, bA, bB);
    static_cast<PairEnt &>(p) = load_block_pair(c, bA, bB);
    p.kc0 = (it - pr * ngrp) * KG;
    return p;
  };
  // the KG channel chunks of an item are gathered together (KG x 2 x 16 B per lane in flight)
  struct G16 { u32x4 a[KG], b[KG]; };
  auto gather = [&](G16 &q, const Item &p) {
    const unsigned va = (((unsigned)p.eA & 0x7fffffffu) >> 6) * c.rowbytes + c.gofs;
    const unsigned vb = (((unsigned)p.eB & 0x7fffffffu) >> 6) * c.rowbytes + c.gofs;
#pragma unroll
    for (int t = 0; t < KG; ++t) {
      if (p.kc0 + t < nkc) {
        q.a[t] = __builtin_amdgcn_raw_buffer_load_b128(c.rin, va, (unsigned)(p.kc0 + t) * 64u, 0);
        q.b[t] = __builtin_amdgcn_raw_buffer_load_b128(c.rin, vb, (unsigned)(p.kc0 + t) * 64u, 0);
      }
    }
  };
  auto compute = [&](const G16 &q, const Item &p) {
    int kA = __builtin_amdgcn_readfirstlane(p.kA), kB = __builtin_amdgcn_readfirstlane(p.kB);
    if (wflip) { kA = vol - 1 - kA; kB = vol - 1 - kB; }
    const unsigned soA0 = (unsigned)kA * c.wk_bytes + (unsigned)c.nb0 * 1024u;
    const unsigned soB0 = (unsigned)kB * c.wk_bytes + (unsigned)c.nb0 * 1024u;
    f32x4 accA[NBW], accB[NBW];
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      accA[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      accB[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // weight fragments of chunk t+1 are in flight while chunk t's MFMAs issue (two register sets, picked by
    // the unrolled index); a pair of adjacent same-offset blocks fetches one set for both chains
    const bool same = ADJ && kA == kB; // wave-uniform
    u32x4 wA[2][NBW], wB[2][NBW];
    auto loadw = [&](int set, int t) {
      const unsigned so = (unsigned)(p.kc0 + t) * c.kc_bytes;
#pragma unroll
      for (int j = 0; j < NBW; ++j) {
        if (j < c.nvalid) {
          wA[set][j] = __builtin_amdgcn_raw_buffer_load_b128(c.rw, c.laneofs, soA0 + so + j * 1024, 0);
          if (!same) wB[set][j] = __builtin_amdgcn_raw_buffer_load_b128(c.rw, c.laneofs, soB0 + so + j * 1024, 0);
        }
      }
    };
    if (p.kc0 < nkc) loadw(0, 0);
#pragma unroll
    for (int t = 0; t < KG; ++t) {
      if (p.kc0 + t < nkc) {
        if (t + 1 < KG && p.kc0 + t + 1 < nkc) loadw((t + 1) & 1, t + 1);
        if (same) {
#pragma unroll
          for (int j = 0; j < NBW; ++j) {
            if (j < c.nvalid) {
              accA[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wA[t & 1][j]),
                                                                __builtin_bit_cast(bf16x8, q.a[t]), accA[j], 0, 0, 0);
              accB[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wA[t & 1][j]),
                                                                __builtin_bit_cast(bf16x8, q.b[t]), accB[j], 0, 0, 0);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < NBW; ++j) {
            if (j < c.nvalid) {
              accA[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wA[t & 1][j]),
                                                                __builtin_bit_cast(bf16x8, q.a[t]), accA[j], 0, 0, 0);
              accB[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wB[t & 1][j]),
                                                                __builtin_bit_cast(bf16x8, q.b[t]), accB[j], 0, 0, 0);
            }
          }
        }
      }
    }
    accumulate_pair<NBW>(c.Ct, p.eA, p.eB, c.g, accA, accB);
  };
  Item p0 = load_item(0), p1 = load_item(1), p2 = load_item(2);
  G16 s0, s1;
  if (nitems > 0) gather(s0, p0);
  for (int it = 0; it < nitems; it += 2) {
    if (it + 1 < nitems) gather(s1, p1);
    compute(s0, p0);
    Item p3 = load_item(it + 3);
    if (it + 1 < nitems) {
      if (it + 2 < nitems) gather(s0, p2);
      compute(s1, p1);
    }
    Item p4 = load_item(it + 4);
    p0 = p2; p1 = p3; p2 = p4;
  }
  __syncthreads();
  // values are rounded to bf16 once, at the store
  tile_epilogue<NBW, WPB, WPB * 64, true>(smem, threadIdx.x, out, co, V_out, tile * 64, c.nb0, bias);
}

// ------------------------------------------------------------------ compiled rule book, part 2
// Offset-major compacted pairs (the reference's RuleBook layout: for offset k the (in, out)
// pairs in ascending out order, Metadata.h:34) for the weight-gradient pass (conv_dw.hip), whose reduction
// runs over the pairs of ONE offset.
//   words: [vol] R_k | [vol+1] first 1024-pair chunk of offset k | [vol+1] first 256-pair chunk |
//          [vol][nb256] block bases | [vol][V][2] pairs
// one block per offset: exclusive scan of the per-256-row hit counts
__global__ __launch_bounds__(256) void k_offset_bases(const StreamJobs js) {            // common.h: one launch, many books
  __shared__ int ws[4];
  __shared__ int carry_s;
  const int job = stream_job_of(js, blockIdx.x);
  const int32_t *__restrict__ counts = js.j[job].counts;
  int32_t *__restrict__ words = js.j[job].words;
  const int64_t nb = op_nb256(js.j[job].V);
  const int vol = js.j[job].vol;
  const int k = blockIdx.x - js.first[job], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t *bases = words + op_hdr(vol) + (int64_t)k * nb;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < nb; base += 256) {
    int64_t i = base + threadIdx.x;
    int v = (i < nb) ? counts[(int64_t)k * nb + i] : 0, inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      int u = __shfl_up(inc, d);
      if (lane >= d) inc += u;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int pre = carry_s;
    for (int j = 0; j < wave; ++j) pre += ws[j];
    if (i < nb) bases[i] = pre + inc - v;
    __syncthreads();
    if (threadIdx.x == 255) carry_s = pre + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) words[k] = carry_s; // R_k
}


__global__ __launch_bounds__(256) void k_fill_offset_pairs(const StreamJobs js) {       // common.h: one launch, many books
  __shared__ int ws[4];
  const int job = stream_job_of(js, blockIdx.x);
  const int32_t *__restrict__ table = js.j[job].table;
  int32_t *__restrict__ words = js.j[job].words;
  const int64_t V = js.j[job].V;
  const int vol = js.j[job].vol;
  const int64_t nb = op_nb256(V);
  const unsigned lb = blockIdx.x - js.first[job];            // block of this book: (row block, offset), offset-major
  const unsigned bx = (unsigned)(lb % (unsigned)nb);
  const int k = (int)(lb / (unsigned)nb), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)bx * 256 + threadIdx.x;
  // chunk layouts (one thread of the grid): offset k owns chunks [cstart[k], cstart[k+1]) of 1024 resp. 256
  // pairs each; the R_k were written by k_offset_bases, the previous launch on this stream
  if (lb == 0 && threadIdx.x == 0) {
    int c = 0, c4 = 0;
    for (int kk = 0; kk < vol; ++kk) {
      words[vol + kk] = c;
      words[vol + (vol + 1) + kk] = c4;
      c += (words[kk] + 1023) / 1024;
      c4 += (words[kk] + 255) / 256;
    }
    words[vol + vol] = c;
    words[vol + (vol + 1) + vol] = c4;
  }
  const int t = (row < V) ? table[(int64_t)k * V + row] : -1;
  const unsigned long long m = __ballot(t >= 0);
  if (lane == 0) ws[wave] = (int)__popcll(m);
  __syncthreads();
  int pre = words[op_hdr(vol) + (int64_t)k * nb + bx];
  for (int j = 0; j < wave; ++j) pre += ws[j];
  if (t >= 0) {
    int pos = pre + (int)__popcll(m & ((1ull << lane) - 1ull));
    int2 *pairs = reinterpret_cast<int2 *>(words + op_hdr(vol) + (int64_t)vol * nb) + (int64_t)k * V;
    pairs[pos] = make_int2(t, (int)row);
  }
}

} // namespace aabr

using namespace aabr;

// name of the kernel instance the last conv / dW entry point dispatched on this thread (bench provenance:
// `roofline.kernel` is what actually ran, not a string typed into the bench)
namespace aabr { thread_local const char *g_last_variant = ""; }
extern "C" const char *aabr_conv_last_variant(void) { return aabr::g_last_variant; }

extern "C" int64_t aabr_conv_wpack_floats(int vol, int n_in, int n_out) {
  // sized for either orientation (forward uses ci=n_in, the transposed pass ci=n_out)
  int64_t a = (int64_t)vol * nkc_of(n_in) * nnb_of(n_out) * 512;
  int64_t b = (int64_t)vol * nkc_of(n_out) * nnb_of(n_in) * 512;
  return a > b ? a : b;
}

extern "C" int64_t aabr_tile_blocks_words(int64_t V, int vol) {
  int64_t nt = tb_ntiles(V);
  return nt + nt * tb_maxb(vol) + nt * tb_maxb(vol) * 16;
}

extern "C" int aabr_build_tile_blocks(const int32_t *table, int64_t V, int vol, int32_t *blocks, void *stream_) {
  AABR_CHECK_ARG(V >= 0 && vol > 0 && vol <= 4096, "bad sizes");
  AABR_CHECK_ARG(V < (1ll << 25), "more than 2^25 sites per grid are not supported");
  if (V == 0) return AABR_OK;
  AABR_CHECK_ARG(table && blocks, "null pointer");
  const StreamJob job{table, nullptr, blocks, V, vol, 0};
  return launch_tile_blocks_jobs(&job, 1, (hipStream_t)stream_);
}

// job lists: the grid of a launch = the blocks of all its books back to back (StreamJobs::first)
template <typename F>
static int launch_stream_jobs(const StreamJob *jobs, int n, F blocks_of, void (*kernel)(const StreamJobs), hipStream_t st) {
  for (int j0 = 0; j0 < n;) {
    StreamJobs js;
    uint64_t blocks = 0;
    int m = 0;
    while (j0 + m < n && m < kStreamJobsMax) {
      const uint64_t b = (uint64_t)blocks_of(jobs[j0 + m]);
      if (m && blocks + b >= (1ull << 31)) break;
      js.j[m] = jobs[j0 + m];
      js.first[m] = (uint32_t)blocks;
      blocks += b;
      ++m;
    }
    js.n = m;
    js.first[m] = (uint32_t)blocks;
    AABR_CHECK_ARG(blocks < (1ull << 31), "too many blocks in one job list");
    if (blocks) hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, js);
    j0 += m;
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

int aabr::launch_tile_blocks_jobs(const StreamJob *jobs, int n, hipStream_t st) {
  return launch_stream_jobs(jobs, n, [](const StreamJob &j) { return ceil_div(tb_ntiles(j.V), 4); }, k_build_tile_blocks, st);
}

// the pair lists of n books: ONE scan launch (a block per book and offset), then ONE fill launch (the fill reads the
// R_k the scan wrote: stream order)
int aabr::launch_offset_pairs_jobs(const StreamJob *jobs, int n, hipStream_t st) {
  int rc = launch_stream_jobs(jobs, n, [](const StreamJob &j) { return (int64_t)j.vol; }, k_offset_bases, st);
  if (rc != AABR_OK) return rc;
  return launch_stream_jobs(jobs, n, [](const StreamJob &j) { return op_nb256(j.V) * j.vol; }, k_fill_offset_pairs, st);
}

extern "C" int64_t aabr_offset_pairs_words(int64_t V, int vol) {
  return op_hdr(vol) + (int64_t)vol * op_nb256(V) + 2 * (int64_t)vol * V;
}

extern "C" int aabr_build_offset_pairs(const int32_t *table, const int32_t *block_counts, int64_t V, int vol,
                                       int32_t *pairs, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  AABR_CHECK_ARG(V >= 0 && vol > 0 && vol <= 65535 && pairs, "bad arguments");
  if (V == 0) {
    hipMemsetAsync(pairs, 0, (size_t)op_hdr(vol) * sizeof(int32_t), st);
    return AABR_OK;
  }
  AABR_CHECK_ARG(table && block_counts, "null pointer");
  const StreamJob job{table, block_counts, pairs, V, vol, 0};
  return launch_offset_pairs_jobs(&job, 1, st);
}

// ---- the 64-row-tile launches: conv_tiles.h decides, these tables carry the decision out ---------------------------
// One row per kernel instance the decision can return, with the name aabr_conv_last_variant reports for it; no other
// instance of these kernels is compiled (tests/test_conv_tiles_host.py checks both against the decision).
template <typename Fn> struct TileInst { TileKernel k; const char *name; Fn fn; };
typedef decltype(&k_conv_blocks_mfma_wlds<1, 1, true>) WldsFn;
typedef decltype(&k_conv_blocks_mfma_buf<1, 2, true, true>) StreamFn;   // (small, wpipe, buf)
typedef decltype(&k_conv_blocks_mfma<1, 2, true>) GenericFn;
typedef decltype(&k_conv_blocks_mfma_bf16<2, 2, 1, true>) Bf16Fn;
#define AABR_WLDS(NBW, NKC, AL)                                                                                 \
  {{kTileWlds, NBW, 0, NKC, 0, AL, false}, "k_conv_blocks_mfma_wlds<" #NBW "," #NKC "," #AL ">",                 \
   k_conv_blocks_mfma_wlds<NBW, NKC, AL>}
#define AABR_SMALL(WPB)                                                                                         \
  {{kTileSmall, 0, WPB, 0, 0, false, false}, "k_conv_blocks_mfma_small<" #WPB ">", k_conv_blocks_mfma_small<WPB>}
#define AABR_WPIPE(WPB)                                                                                         \
  {{kTileWpipe, 4, WPB, 0, 0, false, false}, "k_conv_blocks_mfma_wpipe<4," #WPB ",true,false>",                  \
   k_conv_blocks_mfma_wpipe<4, WPB, true, false>}
#define AABR_BUF(NBW, WPB, AL)                                                                                  \
  {{kTileBuf, NBW, WPB, 0, 0, AL, true}, "k_conv_blocks_mfma_buf<" #NBW "," #WPB ",true," #AL ">",               \
   k_conv_blocks_mfma_buf<NBW, WPB, true, AL>}
#define AABR_GENERIC(NBW, WPB, AL)                                                                              \
  {{kTileGeneric, NBW, WPB, 0, 0, AL, false}, "k_conv_blocks_mfma<" #NBW "," #WPB "," #AL ">",                   \
   k_conv_blocks_mfma<NBW, WPB, AL>}
#define AABR_BF16(NBW, WPB, KG)                                                                                 \
  {{kTileBf16, NBW, WPB, 0, KG, false, true}, "k_conv_blocks_mfma_bf16<" #NBW "," #WPB "," #KG ",true>",         \
   k_conv_blocks_mfma_bf16<NBW, WPB, KG, true>}
static const TileInst<WldsFn> kWlds[] = {
    AABR_WLDS(1, 1, true), AABR_WLDS(1, 1, false), AABR_WLDS(1, 2, true), AABR_WLDS(1, 2, false),
    AABR_WLDS(2, 1, true), AABR_WLDS(2, 1, false), AABR_WLDS(2, 2, true), AABR_WLDS(2, 2, false),
    AABR_WLDS(4, 1, true), AABR_WLDS(4, 1, false), AABR_WLDS(4, 2, true), AABR_WLDS(4, 2, false)};
static const TileInst<StreamFn> kStream[] = {
    AABR_SMALL(8), AABR_SMALL(16), AABR_WPIPE(2), AABR_WPIPE(3),
    AABR_BUF(1, 2, true), AABR_BUF(1, 3, true), AABR_BUF(1, 4, true), AABR_BUF(2, 2, true), AABR_BUF(2, 3, true),
    AABR_BUF(2, 4, true), AABR_BUF(1, 2, false), AABR_BUF(1, 3, false), AABR_BUF(1, 4, false), AABR_BUF(2, 2, false),
    AABR_BUF(2, 3, false), AABR_BUF(2, 4, false), AABR_BUF(4, 2, false), AABR_BUF(4, 3, false)};
static const TileInst<GenericFn> kGeneric[] = {
    AABR_GENERIC(1, 2, true), AABR_GENERIC(1, 3, true), AABR_GENERIC(1, 4, true), AABR_GENERIC(2, 2, true),
    AABR_GENERIC(2, 3, true), AABR_GENERIC(2, 4, true), AABR_GENERIC(4, 2, true), AABR_GENERIC(4, 3, true),
    AABR_GENERIC(1, 2, false), AABR_GENERIC(1, 3, false), AABR_GENERIC(1, 4, false), AABR_GENERIC(2, 2, false),
    AABR_GENERIC(2, 3, false), AABR_GENERIC(2, 4, false), AABR_GENERIC(4, 2, false), AABR_GENERIC(4, 3, false)};
static const TileInst<Bf16Fn> kBf16[] = {
    AABR_BF16(2, 2, 1), AABR_BF16(2, 2, 2), AABR_BF16(2, 2, 4), AABR_BF16(2, 3, 1), AABR_BF16(2, 3, 2),
    AABR_BF16(2, 3, 4), AABR_BF16(2, 4, 1), AABR_BF16(2, 4, 2), AABR_BF16(2, 4, 4), AABR_BF16(4, 2, 1),
    AABR_BF16(4, 2, 2), AABR_BF16(4, 2, 4), AABR_BF16(4, 3, 1), AABR_BF16(4, 3, 2), AABR_BF16(4, 3, 4)};

template <typename Fn, size_t N>
static const TileInst<Fn> *tile_inst(const TileInst<Fn> (&tab)[N], const TileLaunch &t) {
  for (const TileInst<Fn> &e : tab)
    if (e.k == t.k) return &e;
  return nullptr;
}

template <typename Fn, typename... A>
static void launch_tile(const TileInst<Fn> &e, const TileLaunch &t, hipStream_t st, A... args) {
  g_last_variant = e.name;
  hipLaunchKernelGGL(e.fn, dim3((unsigned)t.grid_x, (unsigned)t.grid_y), dim3(t.block), (size_t)t.lds, st, args...);
}

static TileKnobs tile_knobs() {
  return {knob(K_CONV_WLDS), knob(K_CONV_SMALL), knob(K_SMALL_WPB), knob(K_SMALL_MAX), knob(K_CONV_NBW), knob(K_CONV_WPB)};
}

extern "C" int aabr_conv_forward(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                                 int64_t V_out, const int32_t *blocks, int vol, const float *W, const float *bias,
                                 int flags, float *wpack, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  AABR_CHECK_ARG(n_in > 0 && n_out > 0 && vol > 0 && V_out >= 0 && rows_in >= 0, "bad sizes");
  AABR_CHECK_ARG(n_in <= 4096 && n_out <= 4096, "plane count too large");
  if (V_out == 0) return AABR_OK;
  AABR_CHECK_ARG(in_feats && out_feats && blocks && W && wpack && rows_in > 0, "null pointer / empty input");
  AABR_CHECK_ARG(((uintptr_t)in_feats & 15) == 0 && ((uintptr_t)out_feats & 15) == 0 &&
                     ((uintptr_t)wpack & 15) == 0,
                 "feature / scratch pointers must be 16-byte aligned");
  const int transpose = flags & 1, flip = ((flags >> 1) & 1) | ((flags >> 8) << 8);
  const int64_t total = (int64_t)vol * nkc_of(n_in) * nnb_of(n_out) * 512;
  if (!(flags & 4)) // bit2: wpack already holds the packed weights of this (W, flags & 1) pair
    hipLaunchKernelGGL(k_pack_weights, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, W, vol, n_in,
                       n_out, transpose, 0, wpack);
  const int64_t in_bytes = rows_in * n_in * 4, wp_bytes = total * 4,
                words_bytes = aabr_tile_blocks_words(V_out, vol) * 4;
  const TileLaunch t = conv_tile_launch(n_in, n_out, V_out, vol, flags, in_bytes, wp_bytes, words_bytes, tile_knobs());
  if (const TileInst<WldsFn> *e = tile_inst(kWlds, t)) {
    static DynLdsOnce attr_set[sizeof(kWlds) / sizeof(kWlds[0])];
    AABR_CHECK_HIP(dyn_lds_once(attr_set[e - kWlds], (const void *)e->fn, 160 * 1024));
    launch_tile(*e, t, st, in_feats, n_in, in_bytes, out_feats, n_out, V_out, blocks, words_bytes, vol, flip & 1, wpack,
                bias);
  } else if (const TileInst<StreamFn> *e = tile_inst(kStream, t)) {
    launch_tile(*e, t, st, in_feats, n_in, in_bytes, out_feats, n_out, V_out, blocks, words_bytes, vol, flip & 1, wpack,
                wp_bytes, bias);
  } else if (const TileInst<GenericFn> *e = tile_inst(kGeneric, t)) {
    launch_tile(*e, t, st, in_feats, n_in, out_feats, n_out, V_out, blocks, vol, flip, wpack, bias);
  } else {
    AABR_CHECK_ARG(false, "no kernel instance for this launch");
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int64_t aabr_conv_wpack_bf16_elems(int vol, int n_in, int n_out) {
  return aabr_conv_wpack_floats(vol, n_in, n_out);
}

extern "C" int aabr_conv_forward_bf16(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats,
                                      int n_out, int64_t V_out, const int32_t *blocks, int vol, const float *W,
                                      const float *bias, int flags, uint16_t *wpack, void *stream_) {
  hipStream_t st = (hipStream_t)stream_;
  AABR_CHECK_ARG(n_in > 0 && n_out > 0 && vol > 0 && V_out >= 0 && rows_in >= 0, "bad sizes");
  AABR_CHECK_ARG(n_in <= 4096 && n_out <= 4096, "plane count too large");
  AABR_CHECK_ARG(n_in % kKC == 0 && n_out % kKC == 0, "bf16 features need plane counts divisible by 32");
  if (V_out == 0) return AABR_OK;
  AABR_CHECK_ARG(in_feats && out_feats && blocks && W && wpack && rows_in > 0, "null pointer / empty input");
  AABR_CHECK_ARG(((uintptr_t)in_feats & 15) == 0 && ((uintptr_t)out_feats & 15) == 0 &&
                     ((uintptr_t)wpack & 15) == 0,
                 "feature / scratch pointers must be 16-byte aligned");
  const int transpose = flags & 1, flip = (flags >> 1) & 1;
  const int64_t total = (int64_t)vol * nkc_of(n_in) * nnb_of(n_out) * 512;
  const int64_t in_bytes = rows_in * n_in * 2, wp_bytes = total * 2,
                words_bytes = aabr_tile_blocks_words(V_out, vol) * 4;
  AABR_CHECK_ARG(in_bytes < (1ll << 31) && wp_bytes < (1ll << 31) && words_bytes < (1ll << 31),
                 "bf16 convolution addresses its buffers with 32-bit offsets (each must be < 2 GiB)");
  __bf16 *wp = reinterpret_cast<__bf16 *>(wpack);
  if (!(flags & 4))
    hipLaunchKernelGGL(k_pack_weights_bf16, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, W, vol, n_in,
                       n_out, transpose, wp);
  const TileLaunch t = conv_tile_launch_bf16(n_in, n_out, V_out, vol, flags, in_bytes, wp_bytes, words_bytes, tile_knobs());
  const TileInst<Bf16Fn> *e = tile_inst(kBf16, t);
  AABR_CHECK_ARG(e, "no kernel instance for this launch");
  launch_tile(*e, t, st, reinterpret_cast<const __bf16 *>(in_feats), n_in, in_bytes, reinterpret_cast<__bf16 *>(out_feats),
              n_out, V_out, blocks, words_bytes, vol, flip, (const __bf16 *)wp, wp_bytes, bias);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// ---- weight packing as its own entry point (training: pack both orientations once per step) --------
template <typename TO>
static int conv_pack_weights2_t(const float *W, int vol, int n_in, int n_out, TO *wpack_fwd, TO *wpack_t,
                                void *stream_) {
  AABR_CHECK_ARG(n_in > 0 && n_out > 0 && vol > 0 && n_in <= 4096 && n_out <= 4096, "bad sizes");
  AABR_CHECK_ARG(W && wpack_fwd && wpack_t, "null pointer");
  AABR_CHECK_ARG(((uintptr_t)wpack_fwd & 15) == 0 && ((uintptr_t)wpack_t & 15) == 0, "packs must be 16-byte aligned");
  const int64_t total = (int64_t)vol * 512 *
                        ((int64_t)nkc_of(n_in) * nnb_of(n_out) + (int64_t)nkc_of(n_out) * nnb_of(n_in));
  hipLaunchKernelGGL((k_pack_weights2<TO>), dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream_,
                     W, vol, n_in, n_out, wpack_fwd, wpack_t);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// single orientation (inference / stand-alone launches of the 256-row-tile kernel)
extern "C" int aabr_conv_pack_weights(const float *W, int vol, int n_in, int n_out, int transpose, float *wpack,
                                      void *stream_) {
  AABR_CHECK_ARG(n_in > 0 && n_out > 0 && vol > 0 && n_in <= 4096 && n_out <= 4096, "bad sizes");
  AABR_CHECK_ARG(W && wpack && ((uintptr_t)wpack & 15) == 0, "null / misaligned pointer");
  const int64_t total = (int64_t)vol * nkc_of(n_in) * nnb_of(n_out) * 512;
  hipLaunchKernelGGL(k_pack_weights, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream_, W, vol,
                     n_in, n_out, transpose, 0, wpack);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

extern "C" int aabr_conv_pack_weights2(const float *W, int vol, int n_in, int n_out, float *wpack_fwd,
                                       float *wpack_t, void *stream_) {
  return conv_pack_weights2_t<float>(W, vol, n_in, n_out, wpack_fwd, wpack_t, stream_);
}

extern "C" int aabr_conv_pack_weights2_bf16(const float *W, int vol, int n_in, int n_out, uint16_t *wpack_fwd,
                                            uint16_t *wpack_t, void *stream_) {
  return conv_pack_weights2_t<__bf16>(W, vol, n_in, n_out, reinterpret_cast<__bf16 *>(wpack_fwd),
                                      reinterpret_cast<__bf16 *>(wpack_t), stream_);
}

// thread blocks of one job of aabr_conv_pack_weights_jobs (both orientations)
extern "C" int64_t aabr_conv_pack_job_blocks(int vol, int n_in, int n_out) {
  return (int64_t)vol * ceil_div(n_in, kPT) * ceil_div(n_out, kPT);   // one workgroup per 64 x 64 tile of every W[k]
}

extern "C" int aabr_conv_pack_weights_jobs(const void *jobs_dev, int n_jobs, int64_t total_blocks, void *stream_) {
  AABR_CHECK_ARG(n_jobs >= 0 && total_blocks >= 0 && total_blocks < (1ll << 31), "bad sizes");
  if (n_jobs == 0 || total_blocks == 0) return AABR_OK;
  AABR_CHECK_ARG(jobs_dev && ((uintptr_t)jobs_dev & 7) == 0, "null / misaligned job table");
  hipLaunchKernelGGL(k_pack_weights_jobs, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream_,
                     reinterpret_cast<const PackJob *>(jobs_dev), n_jobs);
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

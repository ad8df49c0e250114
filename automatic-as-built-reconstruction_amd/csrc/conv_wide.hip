// conv_wide.hip -- the wide-layer form of the sparse convolution (gfx950): 128-row output tiles, output columns
// split across the waves of a workgroup, gathered rows shared through LDS, weights held in registers per offset.
//
// Why: in the 64-row-tile kernels of conv.hip every 16-pair block streams its own 2 KiB x NBW of packed weights
// per 32-channel chunk through the vector-memory path; on the layers that dominate the FPN_Net step (64..256
// planes, 3x3x3) that is ~5x the bytes of the gathered rows, and the L2->CU feed, not the MFMA pipe, bounds the
// kernel (34 % of the fp32 MFMA peak at 128->128).  Two other forms were built and measured on the way
// (profiles/r02_conv_wide_ab.txt): weights staged through LDS per (offset, chunk) with the
// waves in lockstep (slower: a barrier per ~1.5 blocks of work and 75 % balance), and columns split across waves
// with every wave gathering every row itself (slower: 4x the gather traffic misses the vector L1).  What is kept:
//
//   k_conv_cs  -- a workgroup (4 waves) owns 128 consecutive output rows x 64 output columns in LDS (32 KiB, XOR-
//   swizzled 16-byte granules so the read-add-write of a block's 16 rows is bank-conflict free); wave w owns column
//   block w.  Per filter offset a wave loads its 16-column weight slice ONCE into registers (8 KiB per 128 input
//   channels = 32 VGPRs) and reuses it for every block of that offset in the tile; per pair of 16-pair blocks the
//   workgroup gathers the 32 rows once into a double-buffered LDS stage (each wave a quarter; loads in flight
//   during the previous pair's MFMAs) and every wave reads its MFMA B-operands from there.  Waves never touch each
//   other's tile columns, every wave issues the same MFMAs (perfect balance), accumulation order is fixed (offset,
//   block) => bit-reproducible, no atomics.  One barrier per block pair; 64 KiB LDS => two workgroups per CU.
//
// Same contraction as conv.hip (reference: SCN/CPU/Convolution.cpp:45-185, SCN/CPU/Deconvolution.cpp:7-77):
//     out[o] = bias + sum_k in[table[k][o]] @ Wl[k]
// Requires n_in % 32 == 0 (above 128: % 128), n_out % 64 == 0, vol <= 63, rows_in < 2^23, buffers < 2 GiB.
#include "common.h"
#include "conv_wide_tiles.h"   // kWS, kMaxVol, kMaxTileRows, wide_words and the launch decision
#include <stdlib.h>
#include <type_traits>

namespace aabr {


extern thread_local const char *g_last_variant; // conv.hip

constexpr int kNB = 4;     // 16-column blocks per slab

// ------------------------------------------------------------------ compiled rule book, big-tile form
//   words: [ntiles][vol+1] block prefix per offset | [ntiles][(T/16)*vol][16] entries   (T rows per tile)
//   entry = (partner_row << 8) | local_row; padding entries repeat the block's first pair with bit 31 set.
// Pairs of one offset are in ascending local-row order (deterministic).
// T = rows per tile (a multiple of 16, <= 128); the workgroup has ceil(T/64) waves
// (one launch serves the books of a job list that need the same number of waves per tile, common.h StreamJobs)
__global__ __launch_bounds__(256) void k_build_tileT(const StreamJobs js) {
  const int job = stream_job_of(js, blockIdx.x);
  const int32_t *__restrict__ table = js.j[job].table;
  int32_t *__restrict__ words = js.j[job].words;
  const int64_t V = js.j[job].V;
  const int vol = js.j[job].vol, T = js.j[job].T;
  const int kT = T;
  const int NWV = (T + 63) / 64;
  __shared__ int s_cnt[4][kMaxVol];
  __shared__ int s_base[kMaxVol + 1];
  __shared__ int s_tot[kMaxVol];
  __shared__ int s_first[kMaxVol];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t ntiles = (V + T - 1) / T, tile = blockIdx.x - js.first[job];
  const int maxb = (T / 16) * vol;
  int32_t *pre = words + tile * (vol + 1);
  int32_t *ent = words + ntiles * (vol + 1) + tile * (int64_t)maxb * 16;
  const int64_t row = tile * kT + threadIdx.x;
  const bool valid = (int)threadIdx.x < T && row < V;
  for (int k = 0; k < vol; ++k) {
    const int t = valid ? table[(int64_t)k * V + row] : -1;
    const unsigned long long m = __ballot(t >= 0);
    if (lane == 0) s_cnt[wave][k] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int b = 0;
    for (int k = 0; k < vol; ++k) {
      int tot = 0;
      for (int w = 0; w < NWV; ++w) tot += s_cnt[w][k];
      s_tot[k] = tot;
      s_base[k] = b;
      b += (tot + 15) >> 4;
    }
    s_base[vol] = b;
  }
  __syncthreads();
  if ((int)threadIdx.x <= vol) pre[threadIdx.x] = s_base[threadIdx.x];
  for (int k = 0; k < vol; ++k) {
    const int t = valid ? table[(int64_t)k * V + row] : -1;
    const unsigned long long m = __ballot(t >= 0);
    if (t >= 0) {
      int rank = __popcll(m & ((1ull << lane) - 1ull));
      for (int w = 0; w < wave; ++w) rank += s_cnt[w][k];
      const int e = (t << 8) | (int)threadIdx.x;
      ent[s_base[k] * 16 + rank] = e;
      if (rank == 0) s_first[k] = e;
    }
  }
  __syncthreads();
  for (int k = 0; k < vol; ++k) {
    const int tot = s_tot[k];
    if (tot == 0) continue;
    const int pad = ((tot + 15) & ~15) - tot;
    if ((int)threadIdx.x < pad) ent[s_base[k] * 16 + tot + threadIdx.x] = s_first[k] | (int)0x80000000;
  }
}

__device__ inline float bcf_(unsigned int v) { return __builtin_bit_cast(float, v); }

// ------------------------------------------------------------------ the kernel
// Per pair of blocks the workgroup gathers the 32 rows once (each wave a quarter, 4 x 16-byte loads per lane, in
// flight during the previous pair's MFMAs), stores them in a double-buffered, granule-swizzled stage (2 x 16 KiB)
// and every wave reads its MFMA B-operands from there with conflict-free ds_read_b128.  So per 16-pair block the
// vector-memory path carries the 8 KiB of gathered rows ONCE (64-row-tile kernels: 8 KiB + 32 KiB of weights), the
// weights cost 8 KiB per wave per OFFSET (registers), and every wave issues the same MFMAs.
// One barrier per block pair (~2 x 1024 MFMA cycles per wave) with the double-buffered stage (NBUF = 2), two with a
// single stage buffer (NBUF = 1: 49 KiB of LDS at 128-channel groups => three workgroups per CU instead of two).

// NBUF = LDS stage buffers: 2 (one barrier per pair, 2 workgroups per CU) or 1 (two barriers per pair, 3 per CU)
// BF: bf16 feature storage (extension): rows, stage and weight packs hold bf16, one v_mfma_f32_16x16x32_bf16 per 32
// channels; KG then counts 128-BYTE row chunks (64 channels), so the gather / stage code is the same byte for byte
typedef __bf16 bf16x8w __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4w __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// NCB = 16-column blocks per wave: 1 = 64-column slabs; 2 (bf16 storage) = 128-column slabs -- the kernel is bound by
// the rate at which a CU gathers random rows (~20 GB/s per CU measured in both this and the row-stationary kernel,
// profiles/r03_conv_rs_ab.txt), and a 128-column layer gathered every row once per 64-column slab, i.e. twice
// `stats` in the input-gradient form: the launch writes d_out of the BatchNorm(+leaky ReLU) whose OUTPUT the convolution
// consumed in the forward pass; with `x` set the write-out forms that BatchNorm's BACKWARD statistics instead of the
// forward ones -- per tile [2][co] fp64 sums of d and (x - mean) * d, d = d_out masked by the sign of the forward
// activation recomputed from x exactly as k_bn_partials<1> does (same floats, same operations)
// bf16 storage: the sign comes from the STORED (rounded) activation `out` as in k_bn_partials<1, .., bf16> (x, out bf16)
struct BnBwdStats {
  const float *x, *mean, *invstd, *weight, *bias;   // x == nullptr: forward statistics (or none)
  float leak;
  const float *out;                                 // bf16 storage only
};

// Forms that were built, measured slower and removed in round 5 (their A/B tables are the record): fp32 on the bf16 pipe by
// a three-term split (profiles/r03_conv_x3_ab.txt), a fourth resident workgroup through a two-slot operand ring
// (r04_conv_occ4_ab.txt), the tile rows as the MFMA chains' starting accumulators (r04_conv_bf16_defer_ab.txt), eight-wave
// workgroups on 128-column slabs (r04_conv_bf16_w8_ab.txt), the row-stationary kernel (r03_conv_rs_ab.txt).
// XO (fp32, KG <= 2, plain launches; WIDE_XOFF knob): a step takes the tile's blocks (b, b + 1) whatever their offsets --
// see the step loop below and DESIGN.md section 3.  The compiled stream, the tile, the grid and the LDS are the same.
template <int KG, int DBG, int NBUF, bool BF = false, int NCB = 1, int NSET = 2, bool XO = false>
__global__ __launch_bounds__(256, XO ? 4 : NBUF == 2 ? 2 : 3) void k_conv_cs(const float *__restrict__ in, int ci, int64_t in_bytes,
                                                    float *__restrict__ out, int co, int64_t V_out,
                                                    const int32_t *__restrict__ words, int64_t words_bytes, int vol,
                                                    int wflip, const float *__restrict__ Wp, int64_t wp_bytes,
                                                    const float *__restrict__ bias, int kT2,
                                                    const float *__restrict__ res, double *__restrict__ stats,
                                                    BnBwdStats bn) {
  constexpr int NW = 4;                   // waves per workgroup
  constexpr int NT = 64 * NW;              // threads
  constexpr int LPR = NT / 32;             // lanes per gathered pair row (8 or 16)
  constexpr int RG = KG * 8;               // 16-byte granules per staged row
  constexpr int RF = KG * 32;              // floats per staged row
  constexpr int SWZ = (RG >= 16 && (RG & 15) == 0) ? 15 : 7; // XOR must stay inside the row's granules
  constexpr int STAGE = 2 * 16 * RF;       // floats per stage buffer (two blocks)
  constexpr bool BFM = BF;                 // bf16 operands in the stage and the weight pack
  constexpr int NP = 1;                    // operand planes
  constexpr int NGL = KG * 8 / LPR;        // 16-byte gather loads per lane and pair
  extern __shared__ __align__(16) float smem[];
  float *Ct = smem;                        // [kT2 + 1][64] floats, granule-swizzled; the last row swallows padding entries
  constexpr int WS = 16 * NW * NCB;        // tile row stride in floats = slab width
  float *St = smem + (kT2 + 1) * WS;       // [2][2][16][RF]
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int g = lane >> 4, c16 = lane & 15;
  const int pr = wave * (64 / LPR) + lane / LPR, seg = lane % LPR; // gather role: pair row 0..31, 16-byte segment
  const int nkc = BFM ? ci >> 6 : ci >> 5, nnb = co >> 4;  // chunks per row (64 channels with bf16 operands, else 32)
  // Workgroups are dealt round-robin over the 8 XCDs (linear id % 8), each with its own 4 MiB L2.  Give every XCD a
  // CONTIGUOUS range of (tile, slab) work items instead of every eighth one: the slabs of a tile and the tiles next to
  // it gather the same input rows (consecutive sites lie on the same surface), so they hit that XCD's L2 instead of
  // all eight L2s fetching the whole input (round 2: 580 MB of fetches per launch for 91 MB of operands).  Speed
  // only -- which workgroup computes a tile does not change a bit of it.
  // Offset split (coarse maps: too few (tile, slab) items to fill the chip): grid.y = slabs x P, part p of a (tile, slab)
  // sweeps the filter offsets [p vol / P, (p + 1) vol / P) only and writes its fp32 partial tile to out + p V_out co;
  // k_split_reduce adds the parts in part order (bias, residual and the storage rounding happen there).
  const int nparts = (wflip >> 8) & 0xff;
  int64_t tile;
  int nb0, part = 0;
  {
    const unsigned ny = gridDim.y, total = gridDim.x * ny;
    const unsigned lin = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned per = total >> 3, rem = total & 7u, x = lin & 7u;
    const unsigned wi = x * per + (x < rem ? x : rem) + (lin >> 3);
    tile = wi / ny;
    unsigned sp = wi % ny;
    if (nparts > 1) { part = (int)(sp % (unsigned)nparts); sp /= (unsigned)nparts; }
    nb0 = (int)sp * (NW * NCB);
  }
  const int k_lo = nparts > 1 ? part * vol / nparts : 0;
  const int kend = nparts > 1 ? (part + 1) * vol / nparts : vol;   // offsets >= kend are past the end for this part
  const int64_t row0 = tile * kT2;
  const int64_t ntiles = (V_out + kT2 - 1) / kT2;
  const int maxb = (kT2 / 16) * vol;
  const int vpre = lane <= vol ? words[tile * (vol + 1) + lane] : 0;
  {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 *c4 = reinterpret_cast<f32x4 *>(Ct);
    for (int i = threadIdx.x; i < (kT2 + 1) * WS / 4; i += NT) c4[i] = z;
  }
  const __amdgpu_buffer_rsrc_t rin =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(in), 0, (int)in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rwords =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(words), 0, (int)words_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Wp), 0, (int)wp_bytes, 0x00020000);
  const unsigned ebase = (unsigned)((ntiles * (vol + 1) + tile * (int64_t)maxb * 16) * 4);
  const unsigned rowbytes = (unsigned)ci * (BF ? 2u : 4u);
  const unsigned lane32 = (unsigned)lane * 32u;
  auto pre_of = [&](int k) { return __builtin_amdgcn_readlane(vpre, k); };
  auto next_offset = [&](int k) {
    ++k;
    while (k < kend && pre_of(k + 1) == pre_of(k)) ++k;
    return k;
  };
  struct WReg { u32x4 w0[NP][NCB][KG], w1[NP][NCB][KG]; };
  struct GReg { u32x4 v[NGL]; };
  struct Ent { int eg, ea, eb, hb; };      // gather-role entry of this lane's pair row; compute-role entries (A, B);
                                           // hb (wave-uniform): the pair has a second block
  const int ngroups = (nkc + KG - 1) / KG;
  const int nblk_all = pre_of(vol);
  auto load_w = [&](WReg &w, int k, int kg) {
    const int kW = (wflip & 1) ? vol - 1 - k : k;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int c = 0; c < KG; ++c) { // nkc % KG == 0 (dispatch): every load is unconditional, so the compiler's
        const int kc = kg * KG + c;  // vmcnt bookkeeping stays exact and nothing waits for a prefetch it does not use
        if (BFM) { // two 32-channel MFMA chunks per 64-channel row chunk, 1 KiB of packed weights each
          const unsigned so = (unsigned)((((int64_t)kW * (2 * nkc) + 2 * kc) * nnb + nb0 + wave * NCB + cb) * 1024);
#pragma unroll
          for (int pl = 0; pl < NP; ++pl) {
            const unsigned po = so + (unsigned)pl * (unsigned)(wp_bytes / NP);
            w.w0[pl][cb][c] = __builtin_amdgcn_raw_buffer_load_b128(rw, (unsigned)lane * 16u, po, 0);
            w.w1[pl][cb][c] = __builtin_amdgcn_raw_buffer_load_b128(rw, (unsigned)lane * 16u, po + (unsigned)nnb * 1024u, 0);
          }
        } else {
          const unsigned so = (unsigned)((((int64_t)kW * nkc + kc) * nnb + nb0 + wave * NCB + cb) * 2048);
          w.w0[0][cb][c] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32, so, 0);
          w.w1[0][cb][c] = __builtin_amdgcn_raw_buffer_load_b128(rw, lane32 + 16u, so, 0);
        }
      }
  };
  // entries of the pair (bb, bb+1) of offset kk; the second block only if it belongs to the same offset,
  // otherwise block A again with the discard bit
  auto load_ent = [&](int bb, int kk) {
    Ent e;
    const bool hasB = bb + 1 < pre_of(kk + 1);
    const unsigned bA = (unsigned)bb * 64u, bB = (unsigned)(hasB ? bb + 1 : bb) * 64u;
    e.ea = (int)__builtin_amdgcn_raw_buffer_load_b32(rwords, (unsigned)c16 * 4u, ebase + bA, 0);
    e.eb = (int)__builtin_amdgcn_raw_buffer_load_b32(rwords, (unsigned)c16 * 4u, ebase + bB, 0);
    e.eg = (int)__builtin_amdgcn_raw_buffer_load_b32(rwords, (unsigned)(pr & 15) * 4u, ebase + (pr < 16 ? bA : bB), 0);
    if (!hasB) e.eb |= (int)0x80000000;
    e.hb = hasB ? 1 : 0;
    return e;
  };
  auto gather = [&](GReg &q, int eg, int kg) {
    const unsigned va = (((unsigned)eg & 0x7fffffffu) >> 8) * rowbytes + (unsigned)seg * 16u;
#pragma unroll
    for (int i = 0; i < NGL; ++i) { // granule seg + 8 i of the row's current channel group
      const unsigned so = (unsigned)(kg * NGL + i) * (unsigned)(LPR * 16);
      if (DBG & 2) q.v[i] = (u32x4){(unsigned)eg, 0u, 0u, 0u}; // timing experiments: no global gathers
      else q.v[i] = __builtin_amdgcn_raw_buffer_load_b128(rin, va, so, 0);
    }
  };
  auto stage_store = [&](const GReg &q, int buf) {
    float *rowp = St + (NBUF == 2 ? buf : 0) * (NP * STAGE) + pr * RF;
#pragma unroll
    for (int i = 0; i < NGL; ++i)
      *reinterpret_cast<u32x4 *>(rowp + (((seg + LPR * i) ^ (pr & SWZ)) << 2)) = q.v[i];
  };
  // branch-free: a padding entry (bit 31) lands in the dummy row; the two blocks of a pair never share a real row,
  // so both reads go out before either write
  auto accumulate2 = [&](int ea, const f32x4 (&accA)[NCB], int eb, const f32x4 (&accB)[NCB]) {
    const int ra = ea >= 0 ? (ea & 255) : kT2, rb = eb >= 0 ? (eb & 255) : kT2;
    // (LDS float adds without return, ds_add_f32, instead of this read-add-write: measured 10x slower -- 1147 us
    // instead of 100 us on the dominant bf16 instance, profiles/r03_conv_bf16_ab.txt)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      f32x4 *da = reinterpret_cast<f32x4 *>(Ct + ra * WS + ((((wave * NCB + cb) * 4 + g) ^ (ra & 15)) << 2));
      f32x4 *db = reinterpret_cast<f32x4 *>(Ct + rb * WS + ((((wave * NCB + cb) * 4 + g) ^ (rb & 15)) << 2));
      const f32x4 va = *da, vb = *db;
      *da = va + accA[cb];
      *db = vb + accB[cb];
    }
  };
  // Software pipeline over the tile's block pairs (pairs never straddle an offset):
  //   entries two pairs ahead (registers), gathered rows one pair ahead (registers -> LDS stage after this pair's
  //   MFMAs), weights one offset ahead.  A gather never waits for an entry load issued in the same iteration.
  struct Pos { int b, k; };                // k >= kend: past the end
  auto adv = [&](Pos q) {
    if (q.k >= kend) return q;
    const int kend = pre_of(q.k + 1);
    q.b += 2;
    if (q.b >= kend) { q.b = kend; q.k = next_offset(q.k); }
    return q;
  };
  auto wg_barrier = [&]() {                // LDS traffic of this wave retired, then the workgroup barrier; unlike
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // __syncthreads() it does not drain the prefetches
  };
  int par = 0;
  long long dbg_t[5] = {0, 0, 0, 0, 0};
  // XO: steps over the tile's block list.  On the 64-plane levels a 112-row tile holds ~8 pairs per non-centre offset: one
  // half-full block each, and a step per offset pays the whole skeleton (entry loads, gather, stage store, read-add-write,
  // barrier) for 16 MFMAs per wave.  Here step s takes blocks (2s, 2s + 1) of the stream as k_build_tileT wrote it; block
  // b's offset is the k with pre[k] <= b < pre[k + 1], so empty offsets vanish and only the tile's last block can lack a
  // partner (block A again with the discard bit, as above).  One channel group (KG = nkc), one part.
  //   weights: two register sets with fixed roles, block A's offset and block B's.  Each is refilled with the NEXT step's
  //   offset right after its last MFMA of this step, unconditionally (where the offset stays, the same bytes again from
  //   L2): A's refill has B's MFMAs, the step's tail and the next step's start to arrive, B's the next A's MFMAs on top.
  //   One step body per gather set, every load unconditional and into named registers: exact vmcnt waits.  (A ring of
  //   three sets with the body copied per set and kind of step was built first: the compiler joined the 24 copies in one
  //   latch and moved every just-loaded set behind s_waitcnt vmcnt(0); profiles/conv_wide_instances.txt.)
  //   accumulate: two blocks of different offsets can name the same output row (a submanifold book: usually do), so A's
  //   read-add-write goes before B's; LDS operations of a wave retire in order.  Per output element the sum order is
  //   still offset ascending, each term one MFMA chain from zero: the same bits as the loop below.
  //   entries: the step's 32 words are 128 contiguous bytes: one load (word lane & 31), three cross-lane reads.
  if constexpr (XO) {
    static_assert(!BF && NCB == 1 && NSET == 2 && DBG == 0 && KG <= 2, "the cross-offset step exists for fp32, KG <= 2");
    const int nblk = nblk_all;
    struct XPos { int b, ka, kb; };        // blocks (b, b + 1) and their offsets; b >= nblk: past the end
    auto off_from = [&](int k, int b) { while (pre_of(k + 1) <= b) ++k; return k; };   // b < nblk
    auto xadv = [&](XPos q) {
      if (q.b >= nblk) return q;
      q.b += 2;
      if (q.b >= nblk) { q.b = nblk; return q; }
      q.ka = off_from(q.kb, q.b);
      q.kb = q.b + 1 < nblk ? off_from(q.ka, q.b + 1) : q.ka;
      return q;
    };
    struct XEnt { int w, hb; };            // word (lane & 31) of the step's 32 entries; hb (wave-uniform): block B exists
    XPos pp[NSET + 2];
    XEnt ee[NSET + 2];
    auto xent_of = [&](const XPos &q) {
      const int b = q.b < nblk ? q.b : pp[0].b;
      XEnt e;
      e.w = (int)__builtin_amdgcn_raw_buffer_load_b32(rwords, (unsigned)(lane & 31) * 4u, ebase + (unsigned)b * 64u, 0);
      e.hb = b + 1 < nblk ? 1 : 0;
      return e;
    };
    // an unpaired block: the upper 16 rows of the pair are block A's again
    auto eg_of = [&](const XEnt &e) { return __builtin_amdgcn_ds_bpermute((e.hb ? pr : (pr & 15)) << 2, e.w); };
    auto accumulate1 = [&](int e, const f32x4 &acc) {
      const int r = e >= 0 ? (e & 255) : kT2;
      f32x4 *d = reinterpret_cast<f32x4 *>(Ct + r * WS + (((wave * 4 + g) ^ (r & 15)) << 2));
      *d = *d + acc;
    };
    if (nblk > 0) {
      pp[0].b = 0;
      pp[0].ka = off_from(0, 0);
      pp[0].kb = 1 < nblk ? off_from(pp[0].ka, 1) : pp[0].ka;
#pragma unroll
      for (int i = 1; i < NSET + 2; ++i) pp[i] = xadv(pp[i - 1]);
#pragma unroll
      for (int i = 0; i <= NSET; ++i) ee[i] = xent_of(pp[i]);
      ee[NSET + 1] = ee[0];
      GReg gq[NSET];
      gather(gq[0], eg_of(ee[0]), 0);
      __syncthreads();                     // zero fill done
      stage_store(gq[0], 0);
      gather(gq[1], eg_of(ee[1]), 0);
      __syncthreads();
      // weights of the next step's two blocks; past the tile's last step the current ones again (loaded, never used)
      auto kA_next = [&]() { return pp[1].b < nblk ? pp[1].ka : pp[0].ka; };
      auto kB_next = [&]() { return pp[1].b < nblk ? pp[1].kb : pp[0].kb; };
      WReg WA, WB;
      load_w(WA, pp[0].ka, 0);
      load_w(WB, pp[0].kb, 0);
      auto step = [&](GReg &g_issue, GReg &g_store) __attribute__((always_inline)) {
        gather(g_issue, eg_of(ee[NSET]), 0);                   // pair i + NSET; its entries were loaded an iteration ago
        ee[NSET + 1] = xent_of(pp[NSET + 1]);
        const XEnt e0 = ee[0];
        const int ea = __builtin_amdgcn_ds_bpermute(c16 << 2, e0.w);
        const int eb = __builtin_amdgcn_ds_bpermute((e0.hb ? 16 + c16 : c16) << 2, e0.w) | (e0.hb ? 0 : (int)0x80000000);
        __builtin_amdgcn_sched_barrier(0);                     // the prefetches are issued HERE, ahead of the MFMAs
        const float *sa_ = St + (NBUF == 2 ? par : 0) * STAGE + c16 * RF;
        const float *sb_ = sa_ + 16 * RF;
        f32x4 accA = {0.f, 0.f, 0.f, 0.f}, accB = accA;
        if (wflip & 2) __builtin_amdgcn_s_setprio(3);
        {
          u32x4 a0[KG], a1[KG], b0[KG], b1[KG];
#pragma unroll
          for (int c = 0; c < KG; ++c) {
            const int q0 = ((c * 8 + g * 2) ^ (c16 & SWZ)) << 2, q1 = ((c * 8 + g * 2 + 1) ^ (c16 & SWZ)) << 2;
            a0[c] = *reinterpret_cast<const u32x4 *>(sa_ + q0);
            b0[c] = *reinterpret_cast<const u32x4 *>(sb_ + q0);
            a1[c] = *reinterpret_cast<const u32x4 *>(sa_ + q1);
            b1[c] = *reinterpret_cast<const u32x4 *>(sb_ + q1);
          }
#pragma unroll
          for (int c = 0; c < KG; ++c) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
              accA = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf_(WA.w0[0][0][c][t]), bcf_(a0[c][t]), accA, 0, 0, 0);
#pragma unroll
            for (int t = 0; t < 4; ++t)
              accA = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf_(WA.w1[0][0][c][t]), bcf_(a1[c][t]), accA, 0, 0, 0);
          }
          // (scheduling barriers: a refill hoisted above the MFMAs that read the set would need registers of its own)
          __builtin_amdgcn_sched_barrier(0);
          load_w(WA, kA_next(), 0);
          __builtin_amdgcn_sched_barrier(0);
          if (e0.hb) {                                         // wave-uniform, around MFMAs only
#pragma unroll
            for (int c = 0; c < KG; ++c) {
#pragma unroll
              for (int t = 0; t < 4; ++t)
                accB = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf_(WB.w0[0][0][c][t]), bcf_(b0[c][t]), accB, 0, 0, 0);
#pragma unroll
              for (int t = 0; t < 4; ++t)
                accB = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf_(WB.w1[0][0][c][t]), bcf_(b1[c][t]), accB, 0, 0, 0);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
          load_w(WB, kB_next(), 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (wflip & 2) __builtin_amdgcn_s_setprio(0);
        if (pp[0].kb != pp[0].ka) {                            // wave-uniform, around LDS traffic only
          accumulate1(ea, accA);
          accumulate1(eb, accB);
        } else {
          const f32x4 aA[1] = {accA}, aB[1] = {accB};
          accumulate2(ea, aA, eb, aB);
        }
        if (NBUF == 1) wg_barrier();                           // single stage: every wave is done reading it
        if (pp[1].b < nblk) stage_store(g_store, par ^ 1);     // the next pair, gathered a step ago
        wg_barrier();
        par ^= 1;
#pragma unroll
        for (int i = 0; i < NSET + 1; ++i) { pp[i] = pp[i + 1]; ee[i] = ee[i + 1]; }
        pp[NSET + 1] = xadv(pp[NSET + 1]);
      };
      for (;;) {                                               // the gather sets alternate: two steps per turn
        step(gq[0], gq[1]);
        if (pp[0].b >= nblk) break;
        step(gq[1], gq[0]);
        if (pp[0].b >= nblk) break;
      }
    }
  }
  if constexpr (!XO)
  for (int kg = 0; kg < ngroups; ++kg) {
    // NSET register sets of gathered rows: the rows of pair i + NSET are requested while pair i is multiplied (fp32:
    // NSET = 2 -- a pair's MFMAs take ~1 us, a random-row gather ~2 us; bf16 storage: the MFMAs of a pair take 0.1 us,
    // so the workgroup's pace would be NSET pairs per gather latency -- but NSET = 4 measured SLOWER there, 111-114 us
    // against 100-104 us with two sets, profiles/r03_conv_bf16_ab.txt, and no instance uses four).  Entries run
    // one pair further ahead.  Pair i lives in set i % NSET; the step body exists once per set (static registers).
    Pos pp[NSET + 2];
    pp[0].k = next_offset(k_lo - 1);
    if (pp[0].k >= kend) break;
    pp[0].b = pre_of(pp[0].k);
#pragma unroll
    for (int i = 1; i < NSET + 2; ++i) pp[i] = adv(pp[i - 1]);
    auto ent_of = [&](const Pos &q) { const bool v = q.k < kend; return load_ent(v ? q.b : pp[0].b, v ? q.k : pp[0].k); };
    Ent ee[NSET + 2];
#pragma unroll
    for (int i = 0; i <= NSET; ++i) ee[i] = ent_of(pp[i]);
    ee[NSET + 1] = ee[0];
    GReg gq[NSET];
    gather(gq[0], ee[0].eg, kg);
    __syncthreads();                       // zero fill done / previous group's stage reads done
    par = 0;
    int gs = 0;                            // register set of the current pair
    stage_store(gq[0], par);
#pragma unroll
    for (int i = 1; i < NSET; ++i) gather(gq[i], ee[i].eg, kg);   // pairs 1 .. NSET-1: stored one step before their turn
    __syncthreads();
    // one pipeline step: pair pp[0] with the weight registers `w` (passed by reference: the two weight sets are
    // used from fixed registers by separate copies of this body -- no register shuffling at an offset change)
    auto step = [&](const WReg &w, GReg &g_issue, GReg &g_store) __attribute__((always_inline)) {
      long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
      if (DBG & 4) t0 = __builtin_amdgcn_s_memtime();
      // unconditional: past the tile's last pair the loads repeat a valid pair and their results are dropped
      gather(g_issue, ee[NSET].eg, kg);                      // pair i + NSET; its entry was loaded an iteration ago
      ee[NSET + 1] = ent_of(pp[NSET + 1]);
      const Ent e0 = ee[0];
      __builtin_amdgcn_sched_barrier(0);                     // the prefetches are issued HERE, ahead of the MFMAs
      if (DBG & 4) { t1 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }

      {
        const float *sa = St + (NBUF == 2 ? par : 0) * STAGE + c16 * RF;
        const float *sb = sa + 16 * RF;
        f32x4 accA[NCB], accB[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) { accA[cb] = (f32x4){0.f, 0.f, 0.f, 0.f}; accB[cb] = accA[cb]; }
        if (wflip & 2) __builtin_amdgcn_s_setprio(3);          // experiment (WIDE_PRIO knob): matrix phase at raised priority
        {
        // all of the pair's B operands leave LDS before the first MFMA (counted lgkmcnt waits follow)
        u32x4 a0[KG], a1[KG], b0[KG], b1[KG];
#pragma unroll
        for (int c = 0; c < KG; ++c) {
          // fp32: the lane's 8 consecutive channels of a 32-channel chunk = granules 2g, 2g+1; bf16: its 8 channels
          // of each of the chunk's two 32-channel halves = granules g and 4+g
          const int q0 = ((c * 8 + (BF ? g : g * 2)) ^ (c16 & SWZ)) << 2,
                    q1 = ((c * 8 + (BF ? 4 + g : g * 2 + 1)) ^ (c16 & SWZ)) << 2;
          a0[c] = *reinterpret_cast<const u32x4 *>(sa + q0);
          b0[c] = *reinterpret_cast<const u32x4 *>(sb + q0);
          a1[c] = *reinterpret_cast<const u32x4 *>(sa + q1);
          b1[c] = *reinterpret_cast<const u32x4 *>(sb + q1);
        }
        if (DBG & 1) { // timing experiments: operands consumed, no MFMAs
#pragma unroll
          for (int c = 0; c < KG; ++c) {
            accA[0][0] += bcf_(a0[c][0]) + bcf_(a1[c][0]) + bcf_(w.w0[0][0][c][0]) + bcf_(w.w1[0][0][c][0]);
            accB[0][0] += bcf_(b0[c][0]) + bcf_(b1[c][0]);
          }
        } else if (BF) {
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int c = 0; c < KG; ++c) {
              accA[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8w, w.w0[0][cb][c]),
                                                                 __builtin_bit_cast(bf16x8w, a0[c]), accA[cb], 0, 0, 0);
              accA[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8w, w.w1[0][cb][c]),
                                                                 __builtin_bit_cast(bf16x8w, a1[c]), accA[cb], 0, 0, 0);
            }
          if (e0.hb) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
              for (int c = 0; c < KG; ++c) {
                accB[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8w, w.w0[0][cb][c]),
                                                                   __builtin_bit_cast(bf16x8w, b0[c]), accB[cb], 0, 0, 0);
                accB[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8w, w.w1[0][cb][c]),
                                                                   __builtin_bit_cast(bf16x8w, b1[c]), accB[cb], 0, 0, 0);
              }
          }
        } else {
          // block A, then block B only if the pair has one (sparse rule books: most offsets of a tile hold a single
          // block; the branch is wave-uniform and covers nothing but MFMAs, so no load waits move)
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int c = 0; c < KG; ++c) {
#pragma unroll
              for (int t = 0; t < 4; ++t)
                accA[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf_(w.w0[0][cb][c][t]), bcf_(a0[c][t]), accA[cb], 0, 0, 0);
#pragma unroll
              for (int t = 0; t < 4; ++t)
                accA[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf_(w.w1[0][cb][c][t]), bcf_(a1[c][t]), accA[cb], 0, 0, 0);
            }
          if (e0.hb) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
              for (int c = 0; c < KG; ++c) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                  accB[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf_(w.w0[0][cb][c][t]), bcf_(b0[c][t]), accB[cb], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                  accB[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bcf_(w.w1[0][cb][c][t]), bcf_(b1[c][t]), accB[cb], 0, 0, 0);
              }
          }
        }
        }
        if (DBG & 4) { __builtin_amdgcn_sched_barrier(0); asm volatile("s_nop 0" ::"v"(accA[0]), "v"(accB[0])); t2 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); }
        if (wflip & 2) __builtin_amdgcn_s_setprio(0);
        {
          accumulate2(e0.ea, accA, e0.eb, accB);
        }
      }
      {
        if (NBUF == 1) wg_barrier();                         // single stage: every wave is done reading it
        if (pp[1].k < kend) stage_store(g_store, par ^ 1);   // the next pair, gathered NSET - 1 steps ago
      }
      if (DBG & 4) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); t3 = __builtin_amdgcn_s_memtime(); }
      wg_barrier();
      if (DBG & 4) {
        t4 = __builtin_amdgcn_s_memtime();
        dbg_t[0] += t1 - t0; dbg_t[1] += t2 - t1; dbg_t[2] += t3 - t2; dbg_t[3] += t4 - t3; dbg_t[4] += 1;
      }
      par ^= 1;
#pragma unroll
      for (int i = 0; i < NSET + 1; ++i) { pp[i] = pp[i + 1]; ee[i] = ee[i + 1]; }
      pp[NSET + 1] = adv(pp[NSET + 1]);
    };
    // the current pair's set takes the new request, the next pair's set is stored
    auto step2 = [&](const WReg &w) __attribute__((always_inline)) {
      if (NSET == 2) {
        if (gs == 0) step(w, gq[0], gq[1]);
        else step(w, gq[1], gq[0]);
      } else {
        if (gs == 0) step(w, gq[0], gq[1 % NSET]);
        else if (gs == 1) step(w, gq[1 % NSET], gq[2 % NSET]);
        else if (gs == 2) step(w, gq[2 % NSET], gq[3 % NSET]);
        else step(w, gq[3 % NSET], gq[0]);
      }
      gs = gs + 1 == NSET ? 0 : gs + 1;
    };
    WReg wA;
    int k = pp[0].k;
    load_w(wA, k, kg);
    WReg wB;
    for (;;) {
      int kn = next_offset(k);
      if (kn < kend) load_w(wB, kn, kg);                     // next offset's weights in flight during this offset
      while (pp[0].k == k) step2(wA);
      if (kn >= kend) break;
      k = kn;
      kn = next_offset(k);
      if (kn < kend) load_w(wA, kn, kg);
      while (pp[0].k == k) step2(wB);
      if (kn >= kend) break;
      k = kn;
    }
  }
  if (DBG & 4) { // timing experiments: per-wave phase clocks -> the buffer passed as `bias` (which is then not added)
    if (lane == 0) {
      long long *d = reinterpret_cast<long long *>(const_cast<float *>(bias)) +
                     (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * 5;
      for (int q = 0; q < 5; ++q) d[q] = dbg_t[q];
    }
    bias = nullptr;
  }
  __syncthreads();
  const int nrows = (int)((V_out - row0) < kT2 ? (V_out - row0) : kT2);
  // `stats`: the following BatchNorm's statistics from the values this tile writes (exactly the stored values: after
  // bias / residual, after the bf16 rounding) -- per tile one [2][co] pair of fp64 column sums (x, x^2), combined by the
  // BatchNorm's finalize in tile order, so the result does not depend on which workgroup ran when
  constexpr int QW = 4 * NW * NCB;         // 16-byte columns of the slab; NT % QW == 0: a thread keeps its column
  if (nparts > 1) {                        // this part's fp32 partial tile (an empty offset range writes zeros)
    float *po = out + (int64_t)part * V_out * co;
    for (int i = threadIdx.x; i < nrows * QW; i += NT) {
      const int r = i / QW, q = i % QW;
      *reinterpret_cast<f32x4 *>(po + (row0 + r) * co + nb0 * 16 + q * 4) =
          *reinterpret_cast<const f32x4 *>(Ct + r * WS + ((q ^ (r & 15)) << 2));
    }
    return;
  }
  double sa[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
  float bmu[4] = {0.f, 0.f, 0.f, 0.f}, bwc[4] = {0.f, 0.f, 0.f, 0.f}, bbc[4] = {0.f, 0.f, 0.f, 0.f};
  if (stats && bn.x) {                     // this thread's four columns of the BatchNorm's forward coefficients
    const int p0 = nb0 * 16 + (threadIdx.x % QW) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bmu[j] = bn.mean[p0 + j];
      if (!BF) {
        bwc[j] = bn.invstd[p0 + j] * (bn.weight ? bn.weight[p0 + j] : 1.0f);
        bbc[j] = -bmu[j] * bwc[j] + (bn.bias ? bn.bias[p0 + j] : 0.0f);
      }
    }
  }
#pragma unroll 4
  for (int i = threadIdx.x; i < nrows * QW; i += NT) {
    const int r = i / QW, q = i % QW;
    f32x4 v = *reinterpret_cast<const f32x4 *>(Ct + r * WS + ((q ^ (r & 15)) << 2));
    if (bias) {
      const float *bb = bias + nb0 * 16 + q * 4;
      v[0] += bb[0]; v[1] += bb[1]; v[2] += bb[2]; v[3] += bb[3];
    }
    if (res) { // out = conv + res: the residual / lateral add of the consumer folded into the write-out
      if (BF) {
        // bf16 storage: the separate add would read the convolution's STORED value -- round it first, add the stored
        // residual in fp32, round once more below: bit for bit what k_add2<bf16> / torch's bf16 add give
        const bf16x4w rr = *reinterpret_cast<const bf16x4w *>(reinterpret_cast<const __bf16 *>(res) + (row0 + r) * co +
                                                              nb0 * 16 + q * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)(__bf16)v[j] + (float)rr[j];
      } else {
        const f32x4 rr = *reinterpret_cast<const f32x4 *>(res + (row0 + r) * co + nb0 * 16 + q * 4);
        v[0] += rr[0]; v[1] += rr[1]; v[2] += rr[2]; v[3] += rr[3];
      }
    }
    if (BF) {
      bf16x4w o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
      *reinterpret_cast<bf16x4w *>(reinterpret_cast<__bf16 *>(out) + (row0 + r) * co + nb0 * 16 + q * 4) = o;
      if (stats) { v[0] = (float)o[0]; v[1] = (float)o[1]; v[2] = (float)o[2]; v[3] = (float)o[3]; }
    } else {
      *reinterpret_cast<f32x4 *>(out + (row0 + r) * co + nb0 * 16 + q * 4) = v;
    }
    if (stats) {
      if (BF && bn.x) {                    // (v holds the rounded, stored d_out here)
        const int64_t at = (row0 + r) * co + nb0 * 16 + q * 4;
        const bf16x4w xv = *reinterpret_cast<const bf16x4w *>(reinterpret_cast<const __bf16 *>(bn.x) + at);
        const bf16x4w ov = *reinterpret_cast<const bf16x4w *>(reinterpret_cast<const __bf16 *>(bn.out) + at);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = ((float)ov[j] > 0.0f) ? v[j] : v[j] * bn.leak;
          sa[j] += (double)d;
          sb[j] += (double)((float)xv[j] - bmu[j]) * (double)d;
        }
      } else if (bn.x) {                   // backward statistics of the BatchNorm whose d_out this tile is
        const f32x4 xv = *reinterpret_cast<const f32x4 *>(bn.x + (row0 + r) * co + nb0 * 16 + q * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float o = xv[j] * bwc[j] + bbc[j];
          const float d = (o > 0.0f) ? v[j] : v[j] * bn.leak;
          sa[j] += (double)d;
          sb[j] += (double)(xv[j] - bmu[j]) * (double)d;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { sa[j] += (double)v[j]; sb[j] += (double)v[j] * (double)v[j]; }
      }
    }
  }
  if (stats) {
    __syncthreads();                       // every read of the tile is done: its LDS holds the partial sums now
    double *red = reinterpret_cast<double *>(smem); // [NT][8] = 16 / 32 KiB <= (kT2 + 1) * WS * 4 for kT2 >= 64
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[threadIdx.x * 8 + j] = sa[j]; red[threadIdx.x * 8 + 4 + j] = sb[j]; }
    __syncthreads();
    if (threadIdx.x < 16 * NW * NCB) {
      const int q = threadIdx.x >> 2, j = threadIdx.x & 3;
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int t = 0; t < NT / QW; ++t) { a += red[(t * QW + q) * 8 + j]; b += red[(t * QW + q) * 8 + 4 + j]; }
      stats[(tile * 2 + 0) * co + nb0 * 16 + threadIdx.x] = a;
      stats[(tile * 2 + 1) * co + nb0 * 16 + threadIdx.x] = b;
    }
  }
}

} // namespace aabr
using namespace aabr;

extern "C" int64_t aabr_wide_blocks_words(int64_t V, int vol, int tile_rows) { return wide_words(V, vol, tile_rows); }

extern "C" int aabr_build_wide_blocks(const int32_t *table, int64_t V, int vol, int tile_rows, int32_t *blocks,
                                      void *stream_) {
  AABR_CHECK_ARG(V >= 0 && vol > 0 && vol <= kMaxVol, "bad sizes (vol <= 63)");
  AABR_CHECK_ARG(tile_rows >= 16 && tile_rows <= kMaxTileRows && (tile_rows & 15) == 0, "tile_rows: multiple of 16, <= 240");
  if (V == 0) return AABR_OK;
  AABR_CHECK_ARG(table && blocks, "null pointer");
  const StreamJob job{table, nullptr, blocks, V, vol, tile_rows};
  return launch_wide_blocks_jobs(&job, 1, (hipStream_t)stream_);
}

int aabr::launch_wide_blocks_jobs(const StreamJob *jobs, int n, hipStream_t st) {
  // one launch per workgroup size: a tile of T rows needs ceil(T / 64) waves, and waves beyond that would walk the whole
  // offset loop for nothing (T = 64 and T = 96..128 are what the dispatch rules produce: two launches per list)
  for (int nwv = 1; nwv <= 4; ++nwv) {
    StreamJobs js;
    js.n = 0;
    uint64_t blocks = 0;
    auto flush = [&]() -> int {
      if (js.n == 0 || blocks == 0) { js.n = 0; blocks = 0; return AABR_OK; }
      js.first[js.n] = (uint32_t)blocks;
      hipLaunchKernelGGL(k_build_tileT, dim3((unsigned)blocks), dim3(64 * nwv), 0, st, js);
      js.n = 0;
      blocks = 0;
      return AABR_OK;
    };
    for (int j = 0; j < n; ++j) {
      if ((jobs[j].T + 63) / 64 != nwv) continue;
      const uint64_t b = (uint64_t)((jobs[j].V + jobs[j].T - 1) / jobs[j].T);
      if (js.n == kStreamJobsMax || blocks + b >= (1ull << 31)) flush();
      AABR_CHECK_ARG(b < (1ull << 31), "too many tiles in one rule book");
      js.j[js.n] = jobs[j];
      js.first[js.n] = (uint32_t)blocks;
      blocks += b;
      ++js.n;
    }
    flush();
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// ---- the dispatch queries: conv_wide_tiles.h decides, with the knobs as they stand --------------------------------------
static WideKnobs wide_knobs() {
  return {knob(K_WIDE_ROWS), knob(K_CONV_WIDE), knob(K_CONV_WIDE_BF16), knob(K_WIDE_SPLIT), knob(K_SPLIT_ROWS),
          knob(K_SPLIT_MIN_ITEMS), knob(K_SPLIT_TARGET), knob(K_WIDE_NBUF), knob(K_SPLIT_NBUF), knob(K_WIDE_NCB),
          knob(K_WIDE_PRIO)};
}

// 0: use the 64-row-tile kernels of conv.hip; otherwise rows per tile of the block stream aabr_conv_forward_wide wants
extern "C" int aabr_conv_wide_tile_rows(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol) {
  return wide_tile_rows(kWideF32, n_in, n_out, rows_in, V_out, vol, wide_knobs());
}
// 0: use aabr_conv_forward_bf16 (64-row tiles); otherwise rows per tile for aabr_conv_forward_wide_bf16
extern "C" int aabr_conv_wide_tile_rows_bf16(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol) {
  return wide_tile_rows(kWideBf16, n_in, n_out, rows_in, V_out, vol, wide_knobs());
}
// (P << 16) | tile_rows when this launch should go to aabr_conv_forward_wide_split, else 0.  Asked after
// aabr_conv_wide_tile_rows declined (fewer than 320 (tile, slab) items).
extern "C" int aabr_conv_wide_split(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol) {
  return wide_split(kWideF32, n_in, n_out, rows_in, V_out, vol, wide_knobs());
}
extern "C" int aabr_conv_wide_split_bf16(int n_in, int n_out, int64_t rows_in, int64_t V_out, int vol) {
  return wide_split(kWideBf16, n_in, n_out, rows_in, V_out, vol, wide_knobs());
}

extern "C" int64_t aabr_conv_wide_stats_doubles(int64_t V_out, int tile_rows, int n_out) {
  if (V_out <= 0 || tile_rows <= 0 || n_out <= 0) return 0;
  return ((V_out + tile_rows - 1) / tile_rows) * 2 * n_out;
}

extern "C" int64_t aabr_conv_wide_split_scratch_floats(int64_t V_out, int n_out, int parts) {
  return V_out > 0 && n_out > 0 && parts > 0 ? (int64_t)parts * V_out * n_out : 0;
}

// ---- offset split for coarse maps ---------------------------------------------------------------------------------------
// The coarse FPN scales (49 .. 5,565 rows x 128-256 planes) give the wide kernel 4 .. 180 (tile, slab) items -- a fraction
// of the chip -- and the 64-row-tile kernels that ran them instead re-fetch every block's weights (8-10 TB/s of L2->CU
// traffic for 28-35 TFLOP/s).  Split: P parts per (tile, slab), each sweeping vol / P filter offsets with the wide
// kernel's economy (weights per offset in registers, gathered rows shared through LDS) into its own fp32 partial tile;
// k_split_reduce sums the parts in part order -- fixed order, bit-reproducible -- and applies bias / residual / the
// bf16 rounding.  Scratch: P x V_out x n_out floats.  Measured on the bench's coarse rule books (profiles/r04_conv_split_ab.txt):
// 128->128 at 5,565 rows 62 -> 53 us, 256->256 at 1,382 rows 83 -> 62 us, at 332 rows 47 -> 28 us; single stage buffer (three
// workgroups per CU) over the double one: -10 %; below 8 (tile, slab) items the 16-column item kernel stays ahead.
// bf16 storage (round 4: 50 launches of k_conv_blocks_mfma_bf16 per step, 8 % of the bf16 step's kernel time): the same cut
// over the filter offsets; the parts are fp32 (the kernel's LDS tile is), the reduce kernel rounds once to bf16 -- the same
// single rounding per stored value as the unsplit kernels.
namespace aabr {
template <bool BF>
__global__ __launch_bounds__(256) void k_split_reduce(const float *__restrict__ parts, int nparts, int64_t n4, int co4,
                                                      const float *__restrict__ bias, const float *__restrict__ res,
                                                      void *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 v = reinterpret_cast<const f32x4 *>(parts)[i];
  for (int p = 1; p < nparts; ++p) {
    const f32x4 w = reinterpret_cast<const f32x4 *>(parts)[(int64_t)p * n4 + i];
    v[0] += w[0]; v[1] += w[1]; v[2] += w[2]; v[3] += w[3];
  }
  if (bias) {
    const float *bb = bias + (i % co4) * 4;
    v[0] += bb[0]; v[1] += bb[1]; v[2] += bb[2]; v[3] += bb[3];
  }
  if (res) {
    if (BF) {      // the sum of two stored bf16 values (see k_conv_cs' write-out)
      const bf16x4w rr = reinterpret_cast<const bf16x4w *>(res)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (float)(__bf16)v[j] + (float)rr[j];
    } else {
      const f32x4 rr = reinterpret_cast<const f32x4 *>(res)[i];
      v[0] += rr[0]; v[1] += rr[1]; v[2] += rr[2]; v[3] += rr[3];
    }
  }
  if (BF) {
    bf16x4w o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    reinterpret_cast<bf16x4w *>(out)[i] = o;
  } else {
    reinterpret_cast<f32x4 *>(out)[i] = v;
  }
}
} // namespace aabr

// ---- the launch: one table of the compiled instances, one function that carries conv_wide_tiles.h's decision out -------
typedef decltype(&k_conv_cs<1, 0, 1>) WideFn;   // every instantiation has this type
struct WideInst {
  WideKernel k;                    // (split = false: a split launch runs the same instance)
  const char *name, *split_name;   // what aabr_conv_last_variant reports; split_name == nullptr: no split launch uses it
  WideFn fn;
  WideFn fn_xoff = nullptr;        // the same instance with steps across filter offsets (plain launches, WIDE_XOFF != 0)
};
static const WideInst kWide[] = {
    // fp32 storage: channel groups of 32 .. 128, one or two stage buffers
    {{1, 0, 1, false, 1, false}, "k_conv_cs<1,0,1>", nullptr, k_conv_cs<1, 0, 1>,
     k_conv_cs<1, 0, 1, false, 1, 2, true>},
    {{1, 0, 2, false, 1, false}, "k_conv_cs<1,0,2>", nullptr, k_conv_cs<1, 0, 2>,
     k_conv_cs<1, 0, 2, false, 1, 2, true>},
    {{2, 0, 1, false, 1, false}, "k_conv_cs<2,0,1>", "k_conv_cs<2,0,1,split>", k_conv_cs<2, 0, 1>,
     k_conv_cs<2, 0, 1, false, 1, 2, true>},
    {{2, 0, 2, false, 1, false}, "k_conv_cs<2,0,2>", "k_conv_cs<2,0,2,split>", k_conv_cs<2, 0, 2>,
     k_conv_cs<2, 0, 2, false, 1, 2, true>},
    {{3, 0, 1, false, 1, false}, "k_conv_cs<3,0,1>", "k_conv_cs<3,0,1,split>", k_conv_cs<3, 0, 1>},
    {{3, 0, 2, false, 1, false}, "k_conv_cs<3,0,2>", "k_conv_cs<3,0,2,split>", k_conv_cs<3, 0, 2>},
    {{4, 0, 1, false, 1, false}, "k_conv_cs<4,0,1>", "k_conv_cs<4,0,1,split>", k_conv_cs<4, 0, 1>},
    {{4, 0, 2, false, 1, false}, "k_conv_cs<4,0,2>", "k_conv_cs<4,0,2,split>", k_conv_cs<4, 0, 2>},
    // bf16 storage: channel groups of 64 .. 256; 128-column slabs up to 128 input channels (two gather register sets:
    // four measured slower, 100 -> 112 us)
    {{1, 0, 1, true, 1, false}, "k_conv_cs<1,0,1,bf16>", "k_conv_cs<1,0,1,bf16,split>", k_conv_cs<1, 0, 1, true, 1>},
    {{1, 0, 2, true, 1, false}, "k_conv_cs<1,0,2,bf16>", nullptr, k_conv_cs<1, 0, 2, true, 1>},
    {{1, 0, 1, true, 2, false}, "k_conv_cs<1,0,1,bf16,x128>", nullptr, k_conv_cs<1, 0, 1, true, 2>},
    {{1, 0, 2, true, 2, false}, "k_conv_cs<1,0,2,bf16,x128>", nullptr, k_conv_cs<1, 0, 2, true, 2>},
    {{2, 0, 1, true, 1, false}, "k_conv_cs<2,0,1,bf16>", "k_conv_cs<2,0,1,bf16,split>", k_conv_cs<2, 0, 1, true, 1>},
    {{2, 0, 2, true, 1, false}, "k_conv_cs<2,0,2,bf16>", nullptr, k_conv_cs<2, 0, 2, true, 1>},
    {{2, 0, 1, true, 2, false}, "k_conv_cs<2,0,1,bf16,x128>", nullptr, k_conv_cs<2, 0, 1, true, 2>},
    {{2, 0, 2, true, 2, false}, "k_conv_cs<2,0,2,bf16,x128>", nullptr, k_conv_cs<2, 0, 2, true, 2>},
    {{3, 0, 1, true, 1, false}, "k_conv_cs<3,0,1,bf16>", "k_conv_cs<3,0,1,bf16,split>", k_conv_cs<3, 0, 1, true, 1>},
    {{3, 0, 2, true, 1, false}, "k_conv_cs<3,0,2,bf16>", nullptr, k_conv_cs<3, 0, 2, true, 1>},
    {{4, 0, 1, true, 1, false}, "k_conv_cs<4,0,1,bf16>", "k_conv_cs<4,0,1,bf16,split>", k_conv_cs<4, 0, 1, true, 1>},
    {{4, 0, 2, true, 1, false}, "k_conv_cs<4,0,2,bf16>", nullptr, k_conv_cs<4, 0, 2, true, 1>},
#ifdef AABR_DEV
    // timing experiments (tools/): the 128-channel instances with debug bits.  The fp32 ones always run with two stage
    // buffers (wide_launch); their single-buffer rows are compiled but never launched.
    {{4, 1, 1, false, 1, false}, "k_conv_cs<4,1,1>", nullptr, k_conv_cs<4, 1, 1>},
    {{4, 1, 2, false, 1, false}, "k_conv_cs<4,1,2>", nullptr, k_conv_cs<4, 1, 2>},
    {{4, 2, 1, false, 1, false}, "k_conv_cs<4,2,1>", nullptr, k_conv_cs<4, 2, 1>},
    {{4, 2, 2, false, 1, false}, "k_conv_cs<4,2,2>", nullptr, k_conv_cs<4, 2, 2>},
    {{4, 3, 1, false, 1, false}, "k_conv_cs<4,3,1>", nullptr, k_conv_cs<4, 3, 1>},
    {{4, 3, 2, false, 1, false}, "k_conv_cs<4,3,2>", nullptr, k_conv_cs<4, 3, 2>},
    {{4, 4, 1, false, 1, false}, "k_conv_cs<4,4,1>", nullptr, k_conv_cs<4, 4, 1>},
    {{4, 4, 2, false, 1, false}, "k_conv_cs<4,4,2>", nullptr, k_conv_cs<4, 4, 2>},
    {{2, 4, 1, true, 1, false}, "k_conv_cs<2,4,1,bf16>", nullptr, k_conv_cs<2, 4, 1, true, 1>},
    {{2, 4, 1, true, 2, false}, "k_conv_cs<2,4,1,bf16,x128>", nullptr, k_conv_cs<2, 4, 1, true, 2>},
#endif
};
constexpr int kWideCount = sizeof(kWide) / sizeof(kWide[0]);
static DynLdsOnce kWideLds[kWideCount], kWideLdsX[kWideCount];

// One launch as an entry point hands it over.  Feature pointers are typed as the kernel types them (fp32); with bf16
// storage they point at bf16 rows.  parts != 0: the offset split through `scratch`.
struct WideArgs {
  const char *fn;   // the entry point, for its error text
  int storage;
  const void *in;
  int n_in;
  int64_t rows_in;
  void *out;
  int n_out;
  int64_t V_out;
  const int32_t *blocks;
  int tile_rows, vol;
  const float *bias;
  int flags;
  const void *wpack, *residual;
  double *stats;
  BnBwdStats bn;
  bool split;
  int parts;
  float *scratch;
  void *stream;
};

static int wide_run(const WideArgs &a) {
  hipStream_t st = (hipStream_t)a.stream;
  const WideStorageDesc &s = wide_storage(a.storage);
  const bool bf16 = a.storage == kWideBf16;
  AABR_CHECK_ARG_AS(a.fn, !a.split || (a.parts != 0 && a.scratch && ((uintptr_t)a.scratch & 15) == 0),
                    "2 <= parts <= min(32, vol) and a 16-byte aligned scratch of parts x V_out x n_out floats");
  AABR_CHECK_ARG_AS(a.fn, ((uintptr_t)a.residual & (s.res_align - 1)) == 0,
                    bf16 ? "residual must be 8-byte aligned" : "residual must be 16-byte aligned");
  AABR_CHECK_ARG_AS(a.fn, ((uintptr_t)a.stats & 7) == 0, "statistics need tiles of >= 64 rows");
  WideLaunch t;
  const char *refused = wide_launch(a.storage, a.split ? a.parts : 0, a.n_in, a.n_out, a.rows_in, a.V_out, a.tile_rows,
                                    a.vol, a.flags, a.stats != nullptr, wide_knobs(), t);
  AABR_CHECK_ARG_AS(a.fn, !refused, refused);
  if (a.V_out == 0) return AABR_OK;
  AABR_CHECK_ARG_AS(a.fn, a.in && a.out && a.blocks && a.wpack, "null pointer / empty input");
  AABR_CHECK_ARG_AS(a.fn, (((uintptr_t)a.in | (uintptr_t)a.out | (uintptr_t)a.wpack) & 15) == 0,
                    "feature / weight pointers must be 16-byte aligned");
  WideKernel k = t.k;
  k.split = false;   // a split runs the plain launch's instance: one row serves both, its split_name says whether it may
  const WideInst *e = nullptr;
  for (int i = 0; i < kWideCount && !e; ++i)
    if (kWide[i].k == k) e = &kWide[i];
  AABR_CHECK_ARG_AS(a.fn, e && (!a.split || e->split_name), "no kernel instance for this launch");
  // WIDE_XOFF: 0 = the per-offset step loop; otherwise (the default) the fp32 instances of up to 64 input channels step
  // over the tile's block list.  Same instance key, same reported name, same bits.
  const bool xoff = !a.split && e->fn_xoff && knob(K_WIDE_XOFF) != 0;
  const WideFn fn = xoff ? e->fn_xoff : e->fn;
  AABR_CHECK_HIP(dyn_lds_once(xoff ? kWideLdsX[e - kWide] : kWideLds[e - kWide], (const void *)fn, 80 * 1024));
  g_last_variant = a.split ? e->split_name : e->name;
  const dim3 grid((unsigned)t.grid_x, (unsigned)t.grid_y);
  const float *in = static_cast<const float *>(a.in), *wp = static_cast<const float *>(a.wpack);
  if (a.split) {   // fp32 partial tiles into the scratch; bias, residual and the storage rounding happen in the reduce
    hipLaunchKernelGGL(e->fn, grid, dim3(256), (size_t)t.lds_bytes, st, in, a.n_in, t.in_bytes, a.scratch, a.n_out, a.V_out,
                       a.blocks, t.words_bytes, a.vol, t.wflip, wp, t.wp_bytes, (const float *)nullptr, a.tile_rows,
                       (const float *)nullptr, (double *)nullptr, BnBwdStats{});
    const int64_t n4 = a.V_out * a.n_out / 4;
    const dim3 rgrid((unsigned)((n4 + 255) / 256));
    const float *res = static_cast<const float *>(a.residual);
    if (bf16)
      hipLaunchKernelGGL((k_split_reduce<true>), rgrid, dim3(256), 0, st, a.scratch, a.parts, n4, a.n_out / 4, a.bias, res, a.out);
    else
      hipLaunchKernelGGL((k_split_reduce<false>), rgrid, dim3(256), 0, st, a.scratch, a.parts, n4, a.n_out / 4, a.bias, res, a.out);
  } else {
    hipLaunchKernelGGL(fn, grid, dim3(256), (size_t)t.lds_bytes, st, in, a.n_in, t.in_bytes, static_cast<float *>(a.out),
                       a.n_out, a.V_out, a.blocks, t.words_bytes, a.vol, t.wflip, wp, t.wp_bytes, a.bias, a.tile_rows,
                       static_cast<const float *>(a.residual), a.stats, a.bn);
  }
  AABR_CHECK_LAUNCH();
  return AABR_OK;
}

// ---- fp32 storage -------------------------------------------------------------------------------------------------------
extern "C" int aabr_conv_forward_wide_stats(const float *in_feats, int n_in, int64_t rows_in, float *out_feats,
                                            int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                            const float *bias, int flags, const float *wpack, const float *residual,
                                            double *stats, void *stream_) {
  return wide_run({__func__, kWideF32, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, residual, stats, BnBwdStats{}, false, 0, nullptr, stream_});
}

extern "C" int aabr_conv_forward_wide_res(const float *in_feats, int n_in, int64_t rows_in, float *out_feats,
                                          int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                          const float *bias, int flags, const float *wpack, const float *residual,
                                          void *stream_) {
  return wide_run({__func__, kWideF32, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, residual, nullptr, BnBwdStats{}, false, 0, nullptr, stream_});
}

extern "C" int aabr_conv_forward_wide(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                                      int64_t V_out, const int32_t *blocks, int tile_rows, int vol, const float *bias,
                                      int flags, const float *wpack, void *stream_) {
  return wide_run({__func__, kWideF32, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, nullptr, nullptr, BnBwdStats{}, false, 0, nullptr, stream_});
}

extern "C" int aabr_conv_forward_wide_bwd_stats(const float *in_feats, int n_in, int64_t rows_in, float *out_feats,
                                                int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                                const float *bias, int flags, const float *wpack, const float *residual,
                                                double *stats, const float *bn_in, const float *save_mean,
                                                const float *save_invstd, const float *bn_weight, const float *bn_bias,
                                                float leakiness, void *stream_) {
  AABR_CHECK_ARG(stats && bn_in && save_mean && save_invstd, "null pointer");
  AABR_CHECK_ARG(leakiness >= 0.0f, "the activation sign is recomputed from the BatchNorm input: leakiness >= 0");
  AABR_CHECK_ARG(((uintptr_t)bn_in & 15) == 0, "the BatchNorm input must be 16-byte aligned");
  return wide_run({__func__, kWideF32, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, residual, stats, BnBwdStats{bn_in, save_mean, save_invstd, bn_weight, bn_bias, leakiness}, false, 0,
                   nullptr, stream_});
}

// n_in >= 64: the split compiles no 32-channel instance, and n_in = 32 is AABR_EINVAL before any launch.  (It used to
// pass every check and run the 128-channel instance on 32-channel rows; the library's own route never asks for it,
// aabr_conv_wide_split requires n_in >= 64.)
extern "C" int aabr_conv_forward_wide_split(const float *in_feats, int n_in, int64_t rows_in, float *out_feats, int n_out,
                                            int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                            const float *bias, int flags, const float *wpack, const float *residual,
                                            int parts, float *scratch, void *stream_) {
  return wide_run({__func__, kWideF32, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, residual, nullptr, BnBwdStats{}, true, parts, scratch, stream_});
}

// ---- bf16 feature storage (extension): the same kernel on 128-byte row chunks of 64 bf16 channels ------------------
// the statistics forms read the STORED activations: bn_in / bn_out are bf16 rows
static BnBwdStats bf16_bwd_stats(const uint16_t *bn_in, const uint16_t *bn_out, const float *save_mean, float leakiness) {
  return BnBwdStats{reinterpret_cast<const float *>(bn_in), save_mean, nullptr, nullptr, nullptr, leakiness,
                    reinterpret_cast<const float *>(bn_out)};
}

extern "C" int aabr_conv_forward_wide_bf16_stats(const uint16_t *in_feats, int n_in, int64_t rows_in,
                                                 uint16_t *out_feats, int n_out, int64_t V_out, const int32_t *blocks,
                                                 int tile_rows, int vol, const float *bias, int flags,
                                                 const uint16_t *wpack, double *stats, void *stream_) {
  return wide_run({__func__, kWideBf16, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, nullptr, stats, BnBwdStats{}, false, 0, nullptr, stream_});
}

extern "C" int aabr_conv_forward_wide_bf16(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats,
                                           int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                           const float *bias, int flags, const uint16_t *wpack, void *stream_) {
  return wide_run({__func__, kWideBf16, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, nullptr, nullptr, BnBwdStats{}, false, 0, nullptr, stream_});
}

// the general bf16-storage form behind the compiled pass: optional residual (out = conv + residual, both rounded as
// stored: see the write-out), optional statistics of the following BatchNorm (bn_in NULL) or backward statistics of the
// BatchNorm whose d_out this launch writes (bn_in, bn_out, save_mean, leakiness as aabr_conv_forward_wide_bf16_bwd_stats)
extern "C" int aabr_conv_forward_wide_bf16_res(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats,
                                               int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                               const float *bias, int flags, const uint16_t *wpack,
                                               const uint16_t *residual, double *stats, const uint16_t *bn_in,
                                               const uint16_t *bn_out, const float *save_mean, float leakiness,
                                               void *stream_) {
  if (bn_in) {
    AABR_CHECK_ARG(stats && bn_out && save_mean, "null pointer");
    AABR_CHECK_ARG((((uintptr_t)bn_in | (uintptr_t)bn_out) & 7) == 0, "the BatchNorm's input / output must be 8-byte aligned");
  }
  return wide_run({__func__, kWideBf16, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, residual, stats, bn_in ? bf16_bwd_stats(bn_in, bn_out, save_mean, leakiness) : BnBwdStats{}, false,
                   0, nullptr, stream_});
}

extern "C" int aabr_conv_forward_wide_bf16_bwd_stats(const uint16_t *in_feats, int n_in, int64_t rows_in,
                                                     uint16_t *out_feats, int n_out, int64_t V_out,
                                                     const int32_t *blocks, int tile_rows, int vol, const float *bias,
                                                     int flags, const uint16_t *wpack, double *stats,
                                                     const uint16_t *bn_in, const uint16_t *bn_out,
                                                     const float *save_mean, float leakiness, void *stream_) {
  AABR_CHECK_ARG(stats && bn_in && bn_out && save_mean, "null pointer");
  AABR_CHECK_ARG((((uintptr_t)bn_in | (uintptr_t)bn_out) & 7) == 0, "the BatchNorm's input / output must be 8-byte aligned");
  return wide_run({__func__, kWideBf16, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, nullptr, stats, bf16_bwd_stats(bn_in, bn_out, save_mean, leakiness), false, 0, nullptr, stream_});
}

extern "C" int aabr_conv_forward_wide_split_bf16_res(const uint16_t *in_feats, int n_in, int64_t rows_in,
                                                     uint16_t *out_feats, int n_out, int64_t V_out, const int32_t *blocks,
                                                     int tile_rows, int vol, const float *bias, int flags,
                                                     const uint16_t *wpack, int parts, float *scratch,
                                                     const uint16_t *residual, void *stream_) {
  return wide_run({__func__, kWideBf16, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, residual, nullptr, BnBwdStats{}, true, parts, scratch, stream_});
}

extern "C" int aabr_conv_forward_wide_split_bf16(const uint16_t *in_feats, int n_in, int64_t rows_in, uint16_t *out_feats,
                                                 int n_out, int64_t V_out, const int32_t *blocks, int tile_rows, int vol,
                                                 const float *bias, int flags, const uint16_t *wpack, int parts,
                                                 float *scratch, void *stream_) {
  return wide_run({__func__, kWideBf16, in_feats, n_in, rows_in, out_feats, n_out, V_out, blocks, tile_rows, vol, bias, flags,
                   wpack, nullptr, nullptr, BnBwdStats{}, true, parts, scratch, stream_});
}

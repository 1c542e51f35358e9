// KMeans assign (gfx950).  Replaces the per-partition closest-centre search that Spark's
// KMeans runs per iteration (reached through the Clustering widget -> fit,
// orangecontrib/spark/widgets/ml/spark_ml_clustering.py:14): the split-bf16 assign kernel,
// the fp16 screen kernel and its pre-split kernel (cluster sums, bounds and cost:
// kmeans_update.hip; seeding: kmeans_init.hip).  The assign and screen kernels are
// register-tuned (asm pins, __restrict__ stage bodies, load order; their look-alike
// prologues, stagers and sweeps differ by design): device code changes are checked with
// tools/isa_diff.py.  The presplit kernel is a plain loop, the host dispatch free to change.
//
// ---------------------------------------------------------------------------------
// kmeans_assign: argmin_c ||x - c||^2 = argmin_c (||c||^2 - 2 x.c) as an MFMA GEMM
// with a fused arg-min epilogue -- the N x K distance matrix is never materialised.
//
//  * D' = C . X^T with v_mfma_f32_32x32x16_bf16: A = a 32-centroid chunk (from LDS),
//    B = X^T of a 32-row tile (registers).  In this orientation each lane's 16
//    accumulators belong to ONE data row (its column) and 16 centroids, so the running
//    (min, argmin) is lane-local: no cross-lane work until one final half-wave merge.
//  * split precision: x = xh + xl, c = ch + cl (bf16 hi/lo); x.c ~ xh.ch + xl.ch + xh.cl
//    (3 bf16 MFMAs, ~2^-16 relative error, i.e. fp32-level distance accuracy at the
//    bf16 MFMA rate; a 1-pass bf16 product would mis-assign near ties).  The -2 factor
//    is folded into the centre split on the host.
//  * each wave owns one 32-row tile (X fragments hi/lo: 64 VGPRs at D=128, held for the
//    whole centroid sweep); 8 waves share each centroid chunk through LDS, staged by
//    LDS-DMA (global_load_lds_dwordx4) double-buffered so chunk j+1 lands under chunk
//    j's MFMAs; the 16-B slot XOR-swizzle (slot ^= row & 15, applied to the DMA SOURCE
//    address since the DMA image is lane-linear) makes the 32-row ds_read_b128
//    fragment reads bank-conflict free (CDNA guide §5.5 T2, §5.4 rule 21).
#include "common.h"

using namespace o3s;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kAssignWaves = 8;   // 8 waves x one 32-row tile share each centroid chunk
constexpr int kAssignThreads = kAssignWaves * kWave;

__device__ __forceinline__ void split_bf16(float v, short& hi, short& lo) {
  const uint16_t h = f32_to_bf16(v);
  hi = (short)h;
  lo = (short)f32_to_bf16(v - bf16_to_f32(h));
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// XOR-swizzle mask of a row of `slots` 16-B slots: slot ^ (row & mask) must stay inside the
// row, so the mask covers only the row's power-of-two factor (12 slots: 3, 24 slots: 7 --
// slots - 1 would send slot 8 of row 16 into the next row), at most `cap`.
constexpr int swz_mask(int slots, int cap) { return ((slots & -slots) - 1) & cap; }

// x * scale split into two fp16 halves (hi + lo carries ~22 significant bits); the caller
// picks the power-of-two scale so |x * scale| <= 2^15 (no fp16 overflow)
__device__ __forceinline__ void split_f16(float v, float scale, short& hi, short& lo) {
  const float sv = v * scale;
  const _Float16 h = (_Float16)sv;
  hi = __builtin_bit_cast(short, h);
  lo = __builtin_bit_cast(short, (_Float16)(sv - (float)h));
}

// as split_f16, also returning the scaled rounding error of the hi half (exact in fp32:
// the hi half is the fp16 rounding of sv, so sv - hi is representable)
__device__ __forceinline__ float split_f16e(float v, float scale, short& hi, short& lo) {
  const float sv = v * scale;
  const _Float16 h = (_Float16)sv;
  const float d = sv - (float)h;
  hi = __builtin_bit_cast(short, h);
  lo = __builtin_bit_cast(short, (_Float16)d);
  return d;
}

__device__ __forceinline__ float f16_bits_to_f32(uint32_t bits16) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}

// The 16 ||c||^2 values of one lane's accumulators (c: float[16] or f32x16): accumulator i
// belongs to centroid p + (i & 3) + 8 * (i >> 2), so four float4 at stride 8.
template <class V>
__device__ __forceinline__ void load_cn16(const float* p, V& c) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 c4 = *reinterpret_cast<const float4*>(p + 8 * q);
    c[4 * q + 0] = c4.x; c[4 * q + 1] = c4.y; c[4 * q + 2] = c4.z; c[4 * q + 3] = c4.w;
  }
}

// Lane (r, h)'s A fragment of k-step ks from the chunk image L ([32][D] 16-bit elements, 16-B
// slots XOR-swizzled by row as the DMA stagers wrote them): one ds_read_b128.
template <int D>
__device__ __forceinline__ bf16x8 centre_frag(const uint16_t* L, int ks, int r, int h) {
  const int sw = (ks * 2 + h) ^ (r & swz_mask(D / 8, 15));
  return *reinterpret_cast<const bf16x8*>(L + r * D + sw * 8);
}

// KS = D / 16 k-steps, TT = 32-row tiles per wave.  Cpad: centroids padded to 32
// (padding rows carry cn = +inf).  CNL: ||c||^2 staged in LDS (when Cpad floats fit beside
// the chunk buffers) and folded into the accumulator init; else read per chunk.  The
// epilogue keeps explicit indices (exact ties resolve to the lowest index: the screen's
// slot-coded keys would order exact ties of negative partial distances backwards), which
// costs little here: three MFMAs per k-step leave the VALU mostly idle.
template <int KS, int TT, bool CNL>
__global__ __launch_bounds__(kAssignThreads, 2) void kmeans_assign_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const uint16_t* __restrict__ Chi,
    const uint16_t* __restrict__ Clo, const float* __restrict__ cn, int Cpad,
    int32_t* __restrict__ assign, float* __restrict__ mind, int Dx, const int32_t* __restrict__ rowlist) {
  constexpr int D = KS * 16;
  constexpr int SLOTS = D / 8;                 // 16-B slots per centroid row
  constexpr int CH_ELEMS = 32 * D;             // bf16 per chunk (hi or lo)
  constexpr int PIECES = 2 * 32 * SLOTS;       // 16-B pieces per chunk (hi + lo)
  // G centroid chunks per LDS stage (one barrier per G chunks), double-buffered
  constexpr int G = D <= 128 ? 4 : 2;
  constexpr int PER_THREAD = (G * PIECES + kAssignThreads - 1) / kAssignThreads;
  static_assert(PIECES % kWave == 0, "whole waves per DMA instruction");
  constexpr int ROWS_PER_WAVE = 32 * TT;
  constexpr int ROWS_PER_BLOCK = kAssignWaves * ROWS_PER_WAVE;
  // ONE __shared__ array (guide §5 item 4a): [buf][hi|lo][32][D] bf16, slot-swizzled rows,
  // then (CNL) Cpad floats of ||c||^2
  constexpr int STAGE_ELEMS = 2 * G * 2 * CH_ELEMS;
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  float* const scn = reinterpret_cast<float*>(lds + STAGE_ELEMS);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t row_base = (int64_t)blockIdx.x * ROWS_PER_BLOCK + wid * ROWS_PER_WAVE;

  // ---- X^T fragments (B operand) for the wave's rows, split hi/lo, + ||x||^2.
  // The fragment layout wants 32 rows per load instruction (lane r <- row r), which
  // touches 32 rows x 32 B per wave-instruction; instead the wave streams its 32-row
  // tile row-contiguously (1 KiB per instruction) into its slice of the (not yet used)
  // centroid LDS buffer and reads the fragments back transposed.  16-B slots are
  // XOR-swizzled by row so the 32-row column reads are conflict free.
  // (D > 128: the tile does not fit the stage buffer; load the fragments directly.)
  constexpr int XS = D / 4;                    // 16-B slots per staged row
  constexpr bool kStageX = kAssignWaves * ROWS_PER_WAVE * D * 4 <= STAGE_ELEMS * 2;
  if constexpr (CNL) {
    for (int i = threadIdx.x; i < Cpad; i += kAssignThreads) scn[i] = cn[i];
  }
  float* xt = reinterpret_cast<float*>(lds) + wid * ROWS_PER_WAVE * D;
  bf16x8 bh[TT][KS], bl[TT][KS];
  float xn[TT];
  if constexpr (kStageX) {
    constexpr int PIECES_X = ROWS_PER_WAVE * XS;
#pragma unroll 4
    for (int P = lane; P < PIECES_X; P += kWave) {
      const int rr = P / XS, sl = P % XS;
      const int64_t row = row_base + rr;
      int64_t rowc = row < n ? row : n - 1;
      if (rowlist) rowc = rowlist[rowc];        // recheck pass: rows gathered by index
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 v = 4 * sl < Dx ? *reinterpret_cast<const float4*>(X + rowc * ldx + 4 * sl) : z;
      *reinterpret_cast<float4*>(xt + rr * D + 4 * (sl ^ (rr & swz_mask(XS, 31)))) = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave reads back only its own slice
  }
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const int rr = t * 32 + r;
    float s = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float4 a, b;
      if constexpr (kStageX) {
        const int s0 = (ks * 16 + 8 * h) / 4;
        const int sw = rr & swz_mask(XS, 31);
        a = *reinterpret_cast<const float4*>(xt + rr * D + 4 * (s0 ^ sw));
        b = *reinterpret_cast<const float4*>(xt + rr * D + 4 * ((s0 + 1) ^ sw));
      } else {
        const int64_t row = row_base + rr;
        int64_t rowc = row < n ? row : n - 1;
        if (rowlist) rowc = rowlist[rowc];
        const float* xp = X + rowc * ldx;
        const int c0 = ks * 16 + 8 * h;        // Dx % 4 == 0: whole float4s are in or out
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        a = c0 < Dx ? *reinterpret_cast<const float4*>(xp + c0) : z;
        b = c0 + 4 < Dx ? *reinterpret_cast<const float4*>(xp + c0 + 4) : z;
      }
      const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      // pack pairs into dwords explicitly and pin the packed registers: left as 16 separate
      // shorts, hipcc keeps one bf16 per VGPR and re-packs every fragment (4 v_perm) for
      // every chunk of the centroid sweep
      uint32_t ph[4], pl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        short h0, l0, h1, l1;
        split_bf16(v[2 * j], h0, l0);
        split_bf16(v[2 * j + 1], h1, l1);
        ph[j] = (uint32_t)(uint16_t)h0 | ((uint32_t)(uint16_t)h1 << 16);
        pl[j] = (uint32_t)(uint16_t)l0 | ((uint32_t)(uint16_t)l1 << 16);
        s = fmaf(v[2 * j], v[2 * j], s);
        s = fmaf(v[2 * j + 1], v[2 * j + 1], s);
      }
      bh[t][ks] = __builtin_bit_cast(bf16x8, ph);
      bl[t][ks] = __builtin_bit_cast(bf16x8, pl);
      asm volatile("" : "+v"(bh[t][ks]), "+v"(bl[t][ks]));
    }
    xn[t] = s + __shfl_xor(s, 32, 64);
  }
  __syncthreads();                             // every wave done with the staging area

  // ---- chunk staging by LDS-DMA (global_load_lds_dwordx4): the LDS image is lane-linear,
  // so the XOR swizzle is applied to the SOURCE slot (guide §5.4 rule 21).
  const int nchunks = Cpad / 32;
  auto stage = [&](int stg, uint16_t* __restrict__ dbuf) {
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
      const int P = threadIdx.x + k * kAssignThreads;      // linear 16-B piece index in the stage
      const int g = P / PIECES;                            // wave-uniform (PIECES % 64 == 0)
      const int chunk = stg * G + g;
      if (P >= G * PIECES || chunk >= nchunks) continue;  // the DMA image stays lane-linear
      const int Q = P % PIECES;
      const int which = Q / (32 * SLOTS);
      const int rem = Q % (32 * SLOTS);
      const int cr = rem / SLOTS, sw = rem % SLOTS;
      const int sl = sw ^ (cr & swz_mask(SLOTS, 15));
      const uint16_t* src = (which ? Clo : Chi) + ((int64_t)(chunk * 32 + cr)) * D + sl * 8;
      __builtin_amdgcn_global_load_lds(src, dbuf + (wid * kWave + k * kAssignThreads) * 8, 16, 0, 0);   // wave-uniform
    }
  };

  float bestv[TT], xnv[TT];
  int besti[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) { bestv[t] = INFINITY; besti[t] = 0; xnv[t] = xn[t]; }
  stage(0, lds);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // Software pipeline: the MFMAs of chunk ch are issued, then the arg-min epilogue of
  // chunk ch-1 (independent VALU work) fills the MFMA issue gaps instead of running in
  // a separate phase after every barrier.
  f32x16 accp[TT];
  auto epilogue = [&](const f32x16 (&a)[TT], int chp) {
    const int cbase = chp * 32 + 4 * h;      // acc reg i -> centroid cbase + (i&3) + 8*(i>>2)
    float cv[16];
    if constexpr (!CNL) load_cn16(cn + cbase, cv);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int idx = cbase + (i & 3) + 8 * (i >> 2);
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const float dv = CNL ? a[t][i] : a[t][i] + cv[i];
        const bool better = dv < bestv[t];
        bestv[t] = better ? dv : bestv[t];
        besti[t] = better ? idx : besti[t];
      }
    }
  };
  const int nstages = (nchunks + G - 1) / G;
  // One stage's body with its LDS regions as __restrict__ pointers: the scoped no-alias
  // info keeps hipcc from draining the next stage's in-flight DMA (vmcnt(0)) before the
  // first LDS read of every chunk.
  auto run_stage = [&](int stg, const uint16_t* __restrict__ cur, uint16_t* __restrict__ nxt,
                       const float* __restrict__ sc) {
    if (stg + 1 < nstages) stage(stg + 1, nxt);         // DMA in flight under the MFMAs
    for (int g = 0; g < G; ++g) {
      const int ch = stg * G + g;
      if (ch >= nchunks) break;
      const uint16_t* Lh = cur + g * 2 * CH_ELEMS;
      const uint16_t* Ll = Lh + CH_ELEMS;
      f32x16 acc[TT];
      if constexpr (CNL) {                             // accumulators start at ||c||^2
        f32x16 c0;
        load_cn16(sc + ch * 32 + 4 * h, c0);
#pragma unroll
        for (int t = 0; t < TT; ++t) acc[t] = c0;
      } else {
#pragma unroll
        for (int t = 0; t < TT; ++t)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
      }
      // A fragments are read one k-step ahead of the MFMAs that consume them, so the LDS
      // latency hides under the previous step's three MFMAs
      bf16x8 nh = centre_frag<D>(Lh, 0, r, h), nl = centre_frag<D>(Ll, 0, r, h);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 ah = nh, al = nl;
        if (ks + 1 < KS) { nh = centre_frag<D>(Lh, ks + 1, r, h); nl = centre_frag<D>(Ll, ks + 1, r, h); }
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[t][ks], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[t][ks], acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[t][ks], acc[t], 0, 0, 0);
        }
      }
      if (ch > 0) epilogue(accp, ch - 1);
#pragma unroll
      for (int t = 0; t < TT; ++t) accp[t] = acc[t];
    }
  };
  for (int stg = 0; stg < nstages; ++stg) {
    const int buf = stg & 1;
    run_stage(stg, lds + buf * G * 2 * CH_ELEMS, lds + (buf ^ 1) * G * 2 * CH_ELEMS, scn);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // next stage landed
    __syncthreads();                                    // ... for every wave; buf free again
  }
  if (nchunks > 0) epilogue(accp, nchunks - 1);
  // merge the two half-waves (different centroid subsets of the same row)
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    const float ov = __shfl_xor(bestv[t], 32, 64);
    const int oi = __shfl_xor(besti[t], 32, 64);
    if (ov < bestv[t] || (ov == bestv[t] && oi < besti[t])) { bestv[t] = ov; besti[t] = oi; }
    const int64_t row = row_base + t * 32 + r;
    if (h == 0 && row < n) {
      const int64_t orow = rowlist ? (int64_t)rowlist[row] : row;
      assign[orow] = besti[t];
      if (mind) mind[orow] = fmaxf(bestv[t] + xnv[t], 0.f);
    }
  }
}

// ---------------------------------------------------------------------------------
// kmeans_screen: ONE fp16 MFMA per k-step plus a rigorous error bound.
//
// x and m = -2c are scaled by powers of two (xs, ms: |x xs|, |m ms| <= 2^15, chosen on the
// host) and rounded to fp16 (11 significant bits, 8x finer than bf16), so the screened
// distance S d~_c = S ||c||^2 + (m ms)~.(x xs)~ with S = xs ms differs from S (||c||^2 -
// 2 x.c) by at most S E, where (derivation in ops/kmeans.py::screen_bound)
//   E = eps_x ||x|| + eps_e' ||dx|| + eps0,   dx = fp16(x xs)/xs - x: the row's ACTUAL
//   rounding error (its norm comes with ||x||^2 from the prologue / the pre-split rows),
//   eps_x = max_c ||fp16(m_c ms)/ms - m_c|| (+ fp32 accumulation), eps_e' ~ max||m||
// -- Cauchy-Schwarz on the actual rounding errors instead of 2^-11 per element: ~5x
// tighter on data with full mantissas (profiles/kernel_experiments_r6.json)
// Each lane tracks best, index and SECOND best (one v_med3: the new
// second is med3(old best, v, old second)); a row whose margin (second - best) exceeds
// 2E has provably the same arg-min as the exact product and is finished here: its
// squared distance is recomputed exactly in fp32 from the register-resident split x
// (fp16 hi + lo, ~22 bits) and the fp32 centre row.  Other rows (near-ties) are appended
// to a compacted list (one atomic per wave) and re-solved by the split-precision kernel
// above.  This is 1/3 of the MFMAs of the split kernel; the S ||c||^2 bias is folded
// into the accumulator init (read from LDS).  The epilogue is 2.5 VALU per distance and
// touches no VCC: the candidate's slot in its chunk (0..15) replaces the low 4 mantissa
// bits of the distance (v_and_or: a perturbation below 2^-19 of its magnitude, added to
// the bound), so best = v_min and second = v_med3 carry the index with them; the chunk
// of the best is recorded once per chunk.  On structureless data (uniform in a cube) the
// fp16 bound leaves ~10% of the rows as near ties where the bf16 one flagged nearly all.
// All LDS (staging + ||c||^2) is ONE dynamic __shared__ array, and each stage's body sees
// its three regions as __restrict__ pointers (see run_stage).
//
// 4 waves (one per SIMD) x TT 32-row tiles per block, 2 blocks per CU: one block's X
// staging and DMA prologue overlaps the other's MFMA sweep.
constexpr int kScrWaves = 4;
constexpr int kScrThreads = kScrWaves * kWave;

template <int KS>
struct ScrLds {
  static constexpr int D = KS * 16;
  static constexpr int G = D <= 128 ? 4 : 2;                    // centroid chunks per stage
  static constexpr int CHUNK_BYTES = 2 * 32 * D;                // hi only
  static constexpr int STAGE_BYTES = 2 * G * CHUNK_BYTES;       // double buffered
  static constexpr int X_BYTES = kScrWaves * 32 * D * 4;        // one 32-row tile per wave
  static constexpr int BYTES = STAGE_BYTES > X_BYTES ? STAGE_BYTES : X_BYTES;
};

// NOD (plain screen, mind == nullptr: the Lloyd iterations, whose cost comes from the
// cluster sums -- models/kmeans.py): no per-row distance, so neither the lo half of x (the
// pre-split rows' second 16 B: half the prologue's HBM bytes) nor the chosen centre's fp32
// row (an L2 gather of D floats per row) is read.
// (a lean build -- 2-chunk stages, 3 blocks per CU at 168 VGPRs -- measured slower: 44.4 vs
// 39.2 ms per iteration, profiles/kernel_experiments_r4.json)
template <int KS, int TT, bool PAIR, bool PS = false, bool NOD = false>
__global__ __launch_bounds__(kScrThreads, 2) void kmeans_screen_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const uint16_t* __restrict__ Chi,
    const float* __restrict__ cn, const float* __restrict__ C32, int ldc, int Cpad, float eps_x, float eps0,
    float eps_e, float xscale, float sscale, int32_t* __restrict__ assign, float* __restrict__ mind,
    int32_t* __restrict__ flag_cnt, int32_t* __restrict__ flag_rows, int Dx,
    const uint4* __restrict__ XP = nullptr, const float2* __restrict__ XN = nullptr,
    const int32_t* __restrict__ rowlist = nullptr, float2* __restrict__ bnd = nullptr) {
  using L = ScrLds<KS>;
  constexpr int D = L::D;
  constexpr int G = L::G;
  constexpr int SLOTS = D / 8;
  constexpr int CH_ELEMS = 32 * D;
  constexpr int PIECES = 32 * SLOTS;
  constexpr int PER_THREAD = (G * PIECES + kScrThreads - 1) / kScrThreads;
  static_assert(PIECES % kWave == 0, "whole waves per DMA instruction");
  static_assert(G % 2 == 0, "chunks are processed in ping-pong pairs");
  constexpr int XS = D / 4;
  constexpr int XL = 32 * XS / kWave;          // float4 loads per lane per 32-row tile
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];   // [L::BYTES staging | Cpad floats]
  float* const scn = reinterpret_cast<float*>(lds + L::BYTES / 2);  // S ||c||^2 (padding: 2^125)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t row_base = (int64_t)blockIdx.x * (kScrWaves * 32 * TT) + (int64_t)wid * 32 * TT;

  // padded centres (+inf) become 2^125: finite, so a slot code in the low bits never
  // turns a key into a NaN, and still farther than any real centre
  for (int i = threadIdx.x; i < Cpad; i += kScrThreads) scn[i] = fminf(cn[i] * sscale, 0x1p125f);
  // ---- X tiles -> split fp16 fragments (hi: B operand) + ||x||^2.  All XL loads of a tile
  // are issued before any is consumed (one HBM round trip per tile), then staged
  // row-contiguously through this wave's LDS slice (slot XOR swizzle: conflict-free
  // transposed reads).
  float* xt = reinterpret_cast<float*>(lds) + wid * 32 * D;
  bf16x8 bh[TT][KS], bl[TT][KS];
  float xn[TT], xe[TT];                    // ||x||^2 and ||x xs - fp16(x xs)||^2 per row
  if constexpr (PS) {
    // pre-split rows (kmeans_presplit_kernel, once per data version): per row and
    // (k-step, half) group 16 B of scaled fp16 hi then 16 B of lo, loaded straight into the
    // MFMA B fragments -- no fp32 staging, no conversion VALU in the prologue
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      const int64_t row = row_base + t * 32 + r;
      const int64_t rowc = rowlist ? (int64_t)rowlist[row < n ? row : n - 1] : (row < n ? row : n - 1);
      const uint4* src = XP + rowc * (D / 4);
      uint4 hv[KS], lv[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        hv[ks] = src[(ks * 2 + h) * 2];
        if constexpr (!NOD) lv[ks] = src[(ks * 2 + h) * 2 + 1];
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        bh[t][ks] = __builtin_bit_cast(bf16x8, hv[ks]);
        if constexpr (!NOD) bl[t][ks] = __builtin_bit_cast(bf16x8, lv[ks]);
      }
      const float2 ne = XN[rowc];
      xn[t] = ne.x;
      xe[t] = ne.y;
    }
  } else {
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      float4 xv[XL];
#pragma unroll
      for (int q = 0; q < XL; ++q) {
        const int P = lane + q * kWave;
        const int rr = P / XS, sl = P % XS;
        const int64_t row = row_base + t * 32 + rr;
        const int64_t rowc = rowlist ? (int64_t)rowlist[row < n ? row : n - 1] : (row < n ? row : n - 1);
        const int slc = 4 * sl < Dx ? sl : 0;
        xv[q] = *reinterpret_cast<const float4*>(X + rowc * ldx + 4 * slc);
        if (4 * sl >= Dx) xv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int q = 0; q < XL; ++q) {
        const int P = lane + q * kWave;
        const int rr = P / XS, sl = P % XS;
        *reinterpret_cast<float4*>(xt + rr * D + 4 * (sl ^ (rr & swz_mask(XS, 31)))) = xv[q];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      float s = 0.f, e = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int s0 = (ks * 16 + 8 * h) / 4;
        const int sw = r & swz_mask(XS, 31);
        const float4 a = *reinterpret_cast<const float4*>(xt + r * D + 4 * (s0 ^ sw));
        const float4 b = *reinterpret_cast<const float4*>(xt + r * D + 4 * ((s0 + 1) ^ sw));
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t ph[4], pl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          short h0, l0, h1, l1;
          const float d0 = split_f16e(v[2 * j], xscale, h0, l0);
          const float d1 = split_f16e(v[2 * j + 1], xscale, h1, l1);
          ph[j] = (uint32_t)(uint16_t)h0 | ((uint32_t)(uint16_t)h1 << 16);
          pl[j] = (uint32_t)(uint16_t)l0 | ((uint32_t)(uint16_t)l1 << 16);
          s = fmaf(v[2 * j], v[2 * j], s);
          s = fmaf(v[2 * j + 1], v[2 * j + 1], s);
          e = fmaf(d0, d0, e);
          e = fmaf(d1, d1, e);
        }
        bh[t][ks] = __builtin_bit_cast(bf16x8, ph);
        bl[t][ks] = __builtin_bit_cast(bf16x8, pl);
        if constexpr (NOD) asm volatile("" : "+v"(bh[t][ks]));
        else asm volatile("" : "+v"(bh[t][ks]), "+v"(bl[t][ks]));
      }
      xn[t] = s + __shfl_xor(s, 32, 64);
      xe[t] = e + __shfl_xor(e, 32, 64);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // slice reads done before the next tile
    }
  }
  __syncthreads();                                         // staging area free; scn visible

  const int nchunks = Cpad / 32;
  // one stage = G centroid chunks, DMA'd into dbuf (per-thread offsets from a uniform stage base)
  auto stage = [&](int stg, uint16_t* __restrict__ dbuf) __attribute__((always_inline)) {
    const uint16_t* sbase = Chi + (int64_t)stg * G * CH_ELEMS;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
      const int P = threadIdx.x + k * kScrThreads;
      const int g = P / PIECES;
      if (P >= G * PIECES || stg * G + g >= nchunks) continue;
      const int Q = P % PIECES;
      const int cr = Q / SLOTS, sw = Q % SLOTS;
      const int sl = sw ^ (cr & swz_mask(SLOTS, 15));
      __builtin_amdgcn_global_load_lds(sbase + ((g * 32 + cr) * D + sl * 8),
                                       dbuf + (wid * kWave + k * kScrThreads) * 8, 16, 0, 0);   // wave-uniform dst
    }
  };
  // Running (best, second) per row.  PAIR keeps explicit indices RELATIVE to the current
  // chunk base (ch*32 + 4h): candidates are the inline constants (i&3) + 8*(i>>2) and a new
  // chunk costs one subtract; it also keeps the second's index and the THIRD value
  // (v_med3 again): a row whose third is clear of the best by the bound has its arg-min
  // among {best, second} and is settled by two exact distances instead of the split
  // re-solve (8 VALU per distance).  The plain screen carries the slot in the key's low
  // mantissa bits (3 VALU per distance, epi_step) and the chunk of the best in bch.
  float best[TT], second[TT], third[TT];
  int bidx[TT], sidx[TT], bch[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    best[t] = INFINITY; second[t] = INFINITY; third[t] = INFINITY; bidx[t] = 0; sidx[t] = 0; bch[t] = 0;
  }
  auto epilogue = [&](const f32x16 (&a)[TT], int ch) __attribute__((always_inline)) {
    if constexpr (PAIR) {
#pragma unroll
      for (int t = 0; t < TT; ++t) {                     // re-base onto this chunk
        bidx[t] -= 32;
        sidx[t] -= 32;
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = (i & 3) + 8 * (i >> 2);
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          const float dv = a[t][i];
          const bool better = dv < best[t];
          const bool better2 = dv < second[t];
          third[t] = __builtin_amdgcn_fmed3f(second[t], dv, third[t]);
          sidx[t] = better ? bidx[t] : (better2 ? k : sidx[t]);
          second[t] = __builtin_amdgcn_fmed3f(best[t], dv, second[t]);
          bidx[t] = better ? k : bidx[t];
          best[t] = better ? dv : best[t];
        }
      }
    }
  };
  // plain screen: two distances of the previous chunk (pair e of E = 8 TT, tiles
  // interleaved) folded into the running (best, second) keys.  With best <= second, the
  // second smallest of {best, second, ka, kb} is min(second, med3(best, ka, kb)): 3 VALU
  // per PAIR (med3, min3, min) plus the two slot codes -- 2.5 VALU per distance where one
  // distance at a time took 3 (med3, min, slot), which left the SIMD's issue port, not
  // the matrix core, setting the pace (103 VALU per 16 MFMAs of a chunk).
  auto epi_step = [&](const f32x16 (&a)[TT], int e) __attribute__((always_inline)) {
    const int t = e % TT, i = 2 * (e / TT);
    const float ka = __uint_as_float((__float_as_uint(a[t][i]) & 0xfffffff0u) | (uint32_t)i);
    const float kb = __uint_as_float((__float_as_uint(a[t][i + 1]) & 0xfffffff0u) | (uint32_t)(i + 1));
    float m3, b3, s2;
    // the instructions themselves: fminf / fmed3 would canonicalise the (bit-built) keys
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(m3) : "v"(best[t]), "v"(ka), "v"(kb));
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(b3) : "v"(best[t]), "v"(ka), "v"(kb));
    asm("v_min_f32 %0, %1, %2" : "=v"(s2) : "v"(second[t]), "v"(m3));
    best[t] = b3;
    second[t] = s2;
  };
  // One chunk's MFMAs (accumulators start at S ||c||^2, the bias folded into the first
  // MFMA's C).  EPI: the previous chunk's epilogue (accumulator old, chunk ch_old) is
  // spread over the k-steps, E/KS distance pairs after each step's MFMAs, so the wave issues
  // that VALU work while its own MFMAs occupy the matrix pipe.
  auto sweep = [&](auto epi_tag, const uint16_t* Lh, const float* sc, int ch, f32x16 (&acc)[TT],
                   const f32x16 (&old)[TT], int ch_old) __attribute__((always_inline)) {
    constexpr bool EPI = decltype(epi_tag)::value;
    constexpr int E = 8 * TT;                                     // distance pairs
    f32x16 c0;
    load_cn16(sc + ch * 32 + 4 * h, c0);
    float b0[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) b0[t] = best[t];
    bf16x8 nh = centre_frag<D>(Lh, 0, r, h);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const bf16x8 ah = nh;
      if (ks + 1 < KS) nh = centre_frag<D>(Lh, ks + 1, r, h);
#pragma unroll
      for (int t = 0; t < TT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, ah),
                                                         __builtin_bit_cast(f16x8, bh[t][ks]),
                                                         ks == 0 ? c0 : acc[t], 0, 0, 0);
      if constexpr (EPI) {
#pragma unroll
        for (int e = ks * E / KS; e < (ks + 1) * E / KS; ++e) epi_step(old, e);
      }
    }
    if constexpr (EPI) {
#pragma unroll
      for (int t = 0; t < TT; ++t) bch[t] = best[t] != b0[t] ? ch_old : bch[t];
    }
  };
  // The plain screen's chunk sweep with its centre fragments loaded one chunk AHEAD (all KS
  // of them, double-buffered in registers): the next chunk's LDS reads are issued at the
  // top of this chunk's sweep, so no MFMA waits on a fragment read (the one-step-ahead
  // read of the loop above left a lgkmcnt wait every other k-step).
  auto load_frags = [&](const uint16_t* Lh, bf16x8 (&F)[KS]) __attribute__((always_inline)) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) F[ks] = centre_frag<D>(Lh, ks, r, h);
  };
  auto sweep_f = [&](const bf16x8 (&F)[KS], const uint16_t* Lnext, bf16x8 (&Fn)[KS], const float* sc, int ch,
                     f32x16 (&acc)[TT], const f32x16 (&old)[TT], int ch_old) __attribute__((always_inline)) {
    constexpr int E = 8 * TT;
    f32x16 c0;
    load_cn16(sc + ch * 32 + 4 * h, c0);
    if (Lnext) load_frags(Lnext, Fn);
    float b0[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) b0[t] = best[t];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int t = 0; t < TT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, F[ks]),
                                                         __builtin_bit_cast(f16x8, bh[t][ks]),
                                                         ks == 0 ? c0 : acc[t], 0, 0, 0);
#pragma unroll
      for (int e = ks * E / KS; e < (ks + 1) * E / KS; ++e) epi_step(old, e);
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) bch[t] = best[t] != b0[t] ? ch_old : bch[t];
  };
  stage(0, lds);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // ping-pong accumulators: the epilogue of one chunk runs beside the next chunk's MFMAs
  f32x16 accA[TT], accB[TT];
  const int nstages = (nchunks + G - 1) / G;
  using Yes = std::integral_constant<bool, true>;
  using No = std::integral_constant<bool, false>;
  if constexpr (!PAIR) {
    // sentinel 2^126: the first chunk's "previous" epilogue cannot beat a real distance
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
      for (int j = 0; j < 16; ++j) accB[t][j] = 0x1p126f;
  }
  bool pendA = false, pendB = false;
  bf16x8 FA[KS], FB[KS];
  // One stage's body with its three LDS regions as __restrict__ pointers: the scoped
  // no-alias info lets hipcc's wait insertion see that the chunk / ||c||^2 reads do not
  // touch the next stage's in-flight DMA (otherwise it drains that DMA, vmcnt(0), before
  // the first read of every chunk).  G is even, so chunk pairs never straddle stages.
  auto run_stage = [&](int stg, const uint16_t* __restrict__ cur, uint16_t* __restrict__ nxt,
                       const float* __restrict__ sc) __attribute__((always_inline)) {
    if (stg + 1 < nstages) stage(stg + 1, nxt);
#pragma unroll
    for (int g = 0; g < G; g += 2) {
      const int ch = stg * G + g;
      if constexpr (PAIR) {
        if (ch < nchunks) {
          sweep(No{}, cur + g * CH_ELEMS, sc, ch, accA, accB, 0);
          if (pendB) epilogue(accB, ch - 1);
          pendA = true; pendB = false;
        }
        if (ch + 1 < nchunks) {
          sweep(No{}, cur + (g + 1) * CH_ELEMS, sc, ch + 1, accB, accA, 0);
          if (pendA) epilogue(accA, ch);
          pendB = true; pendA = false;
        }
      } else if constexpr (!NOD) {                      // (with lo halves held: too many registers)
        if (ch < nchunks) sweep(Yes{}, cur + g * CH_ELEMS, sc, ch, accA, accB, ch - 1);
        if (ch + 1 < nchunks) sweep(Yes{}, cur + (g + 1) * CH_ELEMS, sc, ch + 1, accB, accA, ch);
      } else {
        // fragments of chunk g in FA (g even) / FB (g odd); the stage's first chunk loads
        // its own after the stage barrier, every later one was loaded by its predecessor
        // (a chunk index past nchunks reads stale LDS that no MFMA uses)
        if (g == 0) load_frags(cur, FA);
        if (ch < nchunks) sweep_f(FA, cur + (g + 1) * CH_ELEMS, FB, sc, ch, accA, accB, ch - 1);
        if (ch + 1 < nchunks)
          sweep_f(FB, g + 2 < G ? cur + (g + 2) * CH_ELEMS : nullptr, FA, sc, ch + 1, accB, accA, ch);
      }
    }
  };
  for (int stg = 0; stg < nstages; ++stg) {
    const int buf = stg & 1;
    run_stage(stg, lds + buf * G * CH_ELEMS, lds + (buf ^ 1) * G * CH_ELEMS, scn);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  // the last chunk's epilogue (chunk c sits in accA when c is even)
  if constexpr (PAIR) {
    if (pendA) epilogue(accA, nchunks - 1);
    if (pendB) epilogue(accB, nchunks - 1);
  } else {
    const bool lastA = ((nchunks - 1) & 1) == 0;
    float b0[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) b0[t] = best[t];
    if (lastA) {
#pragma unroll
      for (int e = 0; e < 8 * TT; ++e) epi_step(accA, e);
    } else {
#pragma unroll
      for (int e = 0; e < 8 * TT; ++e) epi_step(accB, e);
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) bch[t] = best[t] != b0[t] ? nchunks - 1 : bch[t];
  }
  const int last_base = (nchunks - 1) * 32 + 4 * h;

#pragma unroll
  for (int t = 0; t < TT; ++t) {
    // absolute indices, then merge the half-waves (disjoint centroid subsets of one row):
    // the k-th smallest of two sorted triples is min over i + j = k of max(a_i, b_j)
    int myi;
    if constexpr (PAIR) {
      myi = bidx[t] + last_base;
    } else {
      const uint32_t slot = __float_as_uint(best[t]) & 15u;
      myi = bch[t] * 32 + 4 * h + (int)((slot & 3u) + 8u * (slot >> 2));
    }
    const int mys = sidx[t] + last_base;
    const float ob = __shfl_xor(best[t], 32, 64), os = __shfl_xor(second[t], 32, 64);
    const int oi = __shfl_xor(myi, 32, 64);
    const float sec = fminf(fmaxf(best[t], ob), fminf(second[t], os));
    const bool take = ob < best[t] || (ob == best[t] && oi < myi);
    const int idx = take ? oi : myi;
    const float bv = fminf(best[t], ob);
    // a row whose distances never compared (all NaN / inf) keeps an out-of-range index:
    // clamp it for the loads below; the NaN margin flags the row for the exact re-solve.
    // A NaN key can also carry the slot of a padding centre (||c||^2 = 2^125): not a
    // centre either, so the pick a caller without the re-solve keeps stays below K.
    const bool idx_in = idx >= 0 && idx < Cpad;
    const bool idx_ok = idx_in && scn[idx_in ? idx : 0] < 0x1p125f;
    int idx2 = idx;
    float thr = INFINITY;
    if (PAIR) {
      const float ot = __shfl_xor(third[t], 32, 64);
      const int osi = __shfl_xor(mys, 32, 64);
      thr = fminf(fminf(third[t], ot), fminf(fmaxf(second[t], ob), fmaxf(best[t], os)));
      // the runner-up: the other list's head against the winner list's second
      idx2 = take ? ((best[t] < os || (best[t] == os && myi < osi)) ? myi : osi)
                  : ((ob < second[t] || (ob == second[t] && oi < mys)) ? oi : mys);
    }
    // exact fp32 squared distances from x = (xh + xl) / xs (branch-free: padded columns
    // hold x = 0 and read c = 0) -- to the chosen centre, and (PAIR) to the runner-up
    const float ixs = 1.f / xscale;
    const int idc = idx_ok ? idx : 0;
    const int idc2 = idx2 >= 0 && idx2 < Cpad ? idx2 : idc;
    float s = 0.f, s2 = 0.f;
    if constexpr (!NOD) {
      const float* cp = C32 + (int64_t)idc * ldc;
      const float* cq = C32 + (int64_t)idc2 * ldc;
      // every centre-row load in flight before the first use (one L2 round trip, not KS)
      float4 cu[KS], cwv[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int c0 = ks * 16 + 8 * h;
        cu[ks] = *reinterpret_cast<const float4*>(cp + (c0 < Dx ? c0 : 0));
        cwv[ks] = *reinterpret_cast<const float4*>(cp + (c0 + 4 < Dx ? c0 + 4 : 0));
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int c0 = ks * 16 + 8 * h;
        const bool v0 = c0 < Dx, v1 = c0 + 4 < Dx;
        float4 u = cu[ks];
        float4 w = cwv[ks];
        if (!v0) u = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!v1) w = make_float4(0.f, 0.f, 0.f, 0.f);
        const float cv[8] = {u.x, u.y, u.z, u.w, w.x, w.y, w.z, w.w};
        float cw[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (PAIR) {
          float4 u2 = *reinterpret_cast<const float4*>(cq + (v0 ? c0 : 0));
          float4 w2 = *reinterpret_cast<const float4*>(cq + (v1 ? c0 + 4 : 0));
          if (!v0) u2 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (!v1) w2 = make_float4(0.f, 0.f, 0.f, 0.f);
          cw[0] = u2.x; cw[1] = u2.y; cw[2] = u2.z; cw[3] = u2.w;
          cw[4] = w2.x; cw[5] = w2.y; cw[6] = w2.z; cw[7] = w2.w;
        }
        const uint32_t* ph = reinterpret_cast<const uint32_t*>(&bh[t][ks]);
        const uint32_t* pl = reinterpret_cast<const uint32_t*>(&bl[t][ks]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t hw = ph[j >> 1], lw = pl[j >> 1];
          const float xh = f16_bits_to_f32((j & 1) ? (hw >> 16) : (hw & 0xffffu));
          const float xl = f16_bits_to_f32((j & 1) ? (lw >> 16) : (lw & 0xffffu));
          const float xv = (xh + xl) * ixs;
          const float df = xv - cv[j];
          s = fmaf(df, df, s);
          if (PAIR) {
            const float dg = xv - cw[j];
            s2 = fmaf(dg, dg, s2);
          }
        }
      }
      s += __shfl_xor(s, 32, 64);
      if (PAIR) s2 += __shfl_xor(s2, 32, 64);
    }
    const int64_t row_l = row_base + t * 32 + r;                  // position in this launch
    const bool ok = row_l < n && h == 0;
    const int64_t row = rowlist ? (int64_t)rowlist[ok ? row_l : 0] : row_l;   // the data row
    // in the scaled units of bv, sec; the plain screen's slot codes move each key by less
    // than 2^-19 of its magnitude (twice that allowed for)
    float bound = 2.f * (sscale * (eps_x * sqrtf(xn[t]) + eps0) + eps_e * sqrtf(xe[t]));
    if constexpr (!PAIR) bound += 0x1p-18f * (fabsf(bv) + fabsf(sec));
    bool fl = ok && (!(sec - bv > bound) || !idx_ok);      // near-tie (or NaN): exact re-solve
    int pick = idc;
    float pd = s;
    if (PAIR && fl && idx_ok && idc2 == idx2 && thr - bv > bound) {
      // every other centre is provably farther than both: the exact pair decides
      fl = false;
      const bool second_wins = s2 < s || (s2 == s && idx2 < idx);
      pick = second_wins ? idx2 : idc;
      pd = second_wins ? s2 : s;
    }
    if (ok) {
      assign[row] = pick;
      if (!NOD && mind) mind[row] = pd;
      if (bnd) {
        // Hamerly bounds for the next Lloyd iteration (unscaled distances, not squared):
        // ub >= ||x - c_pick||, lb <= ||x - c|| for every other centre.  Screened partial
        // distances (||c||^2 - 2 x.c) are within bound / (2 S) of the exact ones (the whole
        // bound is used), plus fp32 rounding of ||x||^2 + partial.  Near ties: (inf, 0) --
        // rechecked next time.
        float2 o = make_float2(INFINITY, 0.f);
        if (!fl && !PAIR) {
          const float inv = 1.f / sscale;
          const float pb = bv * inv, psec = sec * inv, mg = bound * inv;
          const float slack = 0x1p-20f * (xn[t] + fabsf(pb) + fabsf(psec));
          o.x = sqrtf(fmaxf(xn[t] + pb + mg + slack, 0.f)) * (1.f + 0x1p-20f);
          o.y = sqrtf(fmaxf(xn[t] + psec - mg - slack, 0.f)) * (1.f - 0x1p-20f);
        }
        bnd[row] = o;
      }
    }
    const uint64_t m = __ballot(fl);
    if (m) {
      const int leader = __ffsll((unsigned long long)m) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(flag_cnt, (int)__popcll(m));
      base = __shfl(base, leader, 64);
      if (fl) flag_rows[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)row;
    }
  }
}

// Host dispatch of the padded width D = 16 KS to a template argument: f gets KS as a
// std::integral_constant (the even values MAXKS, MAXKS - 2, ..., 2 are tried: D is a multiple
// of 32) and returns the entry point's return code; -2 when D is none of them.
template <int MAXKS, class F>
int with_ksteps(int D, F&& f) {
  if constexpr (MAXKS < 2) return -2;
  else return D == 16 * MAXKS ? f(std::integral_constant<int, MAXKS>{}) : with_ksteps<MAXKS - 2>(D, f);
}

}  // namespace

// D must be a multiple of 16 (<= 256), X rows 16-B aligned (ldx % 4 == 0); Cpad % 32 == 0.
// Dx: true feature count (% 4 == 0); Chi/Clo are [Cpad][Dp] with Dp = roundup(Dx, 32).
// rowlist (optional): process rows rowlist[0..n) of X (the screen pass's near-ties).
O3S_API int o3s_kmeans_assign(const float* X, int64_t n, int64_t ldx, int Dx, const void* Chi,
                              const void* Clo, const float* cn, int Cpad, int32_t* assign, float* mind,
                              const int32_t* rowlist, hipStream_t st) {
  if (n <= 0) return 0;
  const int D = (Dx + 31) / 32 * 32;
  if (Dx % 4 != 0 || D > 256 || ldx % 4 != 0 || Cpad % 32 != 0) return -1;
  const int rows_per_block = kAssignWaves * 32;
  const int grid = (int)((n + rows_per_block - 1) / rows_per_block);
  // chunk buffers: 2 buffers x G chunks x (hi + lo) x 32 x D bf16 = 128 KB at every D
  const size_t stage_bytes = 2 * (D <= 128 ? 4 : 2) * 2 * 32 * (size_t)D * 2;
  const bool cnl = stage_bytes + sizeof(float) * (size_t)Cpad <= 160 * 1024;
  const size_t lds = stage_bytes + (cnl ? sizeof(float) * (size_t)Cpad : 0);
  return with_ksteps<16>(D, [&](auto KS) {
    return with_bool(cnl, [&](auto CNL) {
      hipLaunchKernelGGL((kmeans_assign_kernel<KS, 1, CNL>), dim3(grid), dim3(kAssignThreads), lds, st, X, n, ldx,
                         (const uint16_t*)Chi, (const uint16_t*)Clo, cn, Cpad, assign, mind, Dx, rowlist);
      O3S_CHECK_LAUNCH();
      return 0;
    });
  });
}

namespace {
// X (fp32 [n][ldx], Dx valid columns) -> the screen kernel's pre-split rows: per row D/8
// groups (group g = 2 ks + h: dims 8 g .. 8 g + 7) of 16 B scaled-fp16 hi + 16 B lo (the
// split_f16 of the kernel's prologue, zero past Dx), and ||x||^2 in fp32.  One lane per
// group; the row norm is a shuffle reduction over the row's lanes.
template <int D>
__global__ __launch_bounds__(256) void kmeans_presplit_kernel(const float* __restrict__ X, int64_t n, int64_t ldx,
                                                              int Dx, float xscale, uint4* __restrict__ XP,
                                                              float2* __restrict__ XN) {
  constexpr int G = D / 8;                     // groups per row
  // a row takes GP lanes, G rounded up to a power of two (D = 96: 12 groups on 16 lanes,
  // four of them idle), so rows never straddle the butterfly below or a wave
  constexpr int GP = G <= 4 ? 4 : G <= 8 ? 8 : 16;
  static_assert(G <= GP, "at most 16 groups per row");
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = tid / GP;
  const int g = (int)(tid % GP);
  float s = 0.f, e = 0.f;
  if (row < n && g < G) {
    uint32_t ph[4], pl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c0 = 8 * g + 2 * j;
      const float v0 = c0 < Dx ? X[row * ldx + c0] : 0.f;
      const float v1 = c0 + 1 < Dx ? X[row * ldx + c0 + 1] : 0.f;
      short h0, l0, h1, l1;
      const float d0 = split_f16e(v0, xscale, h0, l0);
      const float d1 = split_f16e(v1, xscale, h1, l1);
      ph[j] = (uint32_t)(uint16_t)h0 | ((uint32_t)(uint16_t)h1 << 16);
      pl[j] = (uint32_t)(uint16_t)l0 | ((uint32_t)(uint16_t)l1 << 16);
      s = fmaf(v0, v0, s);
      s = fmaf(v1, v1, s);
      e = fmaf(d0, d0, e);
      e = fmaf(d1, d1, e);
    }
    XP[(row * G + g) * 2] = make_uint4(ph[0], ph[1], ph[2], ph[3]);
    XP[(row * G + g) * 2 + 1] = make_uint4(pl[0], pl[1], pl[2], pl[3]);
  }
#pragma unroll
  for (int o = 1; o < GP; o <<= 1) {
    s += __shfl_xor(s, o, 64);
    e += __shfl_xor(e, o, 64);
  }
  if (row < n && g == 0) XN[row] = make_float2(s, e);
}
}  // namespace

// Pre-split rows for the screen kernel (see kmeans_presplit_kernel): XP [n][D / 8][2] x 16 B,
// XN [n] fp32; D = Dx rounded up to 32 (<= 128).
O3S_API int o3s_kmeans_presplit(const float* X, int64_t n, int64_t ldx, int Dx, float xscale, void* XP, float* XN2,
                                hipStream_t st) {
  if (n <= 0) return 0;
  const int D = (Dx + 31) / 32 * 32;
  if (Dx % 4 != 0 || D > 128) return -1;
  const int64_t threads = n * (D == 96 ? 16 : D / 8);      // lanes per row: see the kernel's GP
  const dim3 grid((unsigned)((threads + 255) / 256));
  return with_ksteps<8>(D, [&](auto KS) {
    hipLaunchKernelGGL((kmeans_presplit_kernel<16 * KS>), grid, dim3(256), 0, st, X, n, ldx, Dx, xscale, (uint4*)XP,
                       reinterpret_cast<float2*>(XN2));
    O3S_CHECK_LAUNCH();
    return 0;
  });
}

namespace {
// The arguments of o3s_kmeans_screen2 as the kernel takes them.
struct ScreenArgs {
  const float* X;
  int64_t n, ldx;
  int Dx, ldc, Cpad;
  const uint16_t* Chi;
  const float *cn, *C32;
  float eps_x, eps0, eps_e, xscale, sscale;
  int32_t *assign, *flag_cnt, *flag_rows;
  float* mind;
  const uint4* XP;
  const float2* XN;
  const int32_t* rowlist;
  float2* bnd;
  hipStream_t st;
};

template <int KS, int TT, bool PAIR, bool PS, bool NOD>
int launch_screen(const ScreenArgs& a) {
  constexpr int rows_per_block = kScrWaves * 32 * TT;
  const int64_t grid = (a.n + rows_per_block - 1) / rows_per_block;
  const size_t dyn = ScrLds<KS>::BYTES + sizeof(float) * (size_t)a.Cpad;
  if (dyn > 160 * 1024) return -3;
  hipLaunchKernelGGL((kmeans_screen_kernel<KS, TT, PAIR, PS, NOD>), dim3((unsigned)grid), dim3(kScrThreads), dyn, a.st,
                     a.X, a.n, a.ldx, a.Chi, a.cn, a.C32, a.ldc, a.Cpad, a.eps_x, a.eps0, a.eps_e, a.xscale, a.sscale,
                     a.assign, a.mind, a.flag_cnt, a.flag_rows, a.Dx, PS ? a.XP : nullptr, PS ? a.XN : nullptr,
                     a.rowlist, a.bnd);
  O3S_CHECK_LAUNCH();
  return 0;
}
}  // namespace

// Screen pass (see kmeans_screen_kernel).  Ch16: fp16 bits of -2 C ms [Cpad][D]; C32: fp32
// centres [K][ldc] (ldc % 4 == 0); bound S E = S (eps_x ||x|| + eps0) + eps_e ||dx xs||
// (eps_e = eps_e' ms: the error norm is kept in the scaled units); xscale = xs, sscale = xs ms;
// flag_cnt (zeroed by the caller) / flag_rows [n]: near-tie rows for
// o3s_kmeans_assign(rowlist).  tt: 32-row tiles per wave (1 or 2; D = 160 has the 1-tile build
// only).  pair: one tile per wave (registers), never the pre-split rows (PS) or the
// distance-free build (NOD) -- the PAIR builds with PS / NOD set are compiled, not launched.
O3S_API int o3s_kmeans_screen2(const float* X, int64_t n, int64_t ldx, int Dx, const void* Chi, const float* cn,
                               const float* C32, int ldc, int Cpad, float eps_x, float eps0, float eps_e,
                               float xscale, float sscale, int32_t* assign, float* mind, int32_t* flag_cnt,
                               int32_t* flag_rows, int tt, int pair, const void* XP, const float* XN2,
                               const int32_t* rowlist, float* bnd2, hipStream_t st) {
  if (n <= 0) return 0;
  const int D = (Dx + 31) / 32 * 32;
  if (Dx % 4 != 0 || D > 160 || ldx % 4 != 0 || ldc % 4 != 0 || Cpad % 32 != 0 || n > 0x7fffffffll) return -1;
  if (tt != 1 && tt != 2) return -1;
  const ScreenArgs a{X, n, ldx, Dx, ldc, Cpad, (const uint16_t*)Chi, cn, C32, eps_x, eps0, eps_e, xscale, sscale,
                     assign, flag_cnt, flag_rows, mind, (const uint4*)XP, reinterpret_cast<const float2*>(XN2),
                     rowlist, reinterpret_cast<float2*>(bnd2), st};
  return with_ksteps<10>(D, [&](auto KS) {
    return with_bool(pair != 0, [&](auto PAIR) {
      return with_bool(XP != nullptr && !PAIR, [&](auto PS) {
        return with_bool(mind == nullptr && !PAIR, [&](auto NOD) {
          constexpr int TT2 = KS < 10 && !PAIR ? 2 : 1;          // the two-tile build, where there is one
          return tt == 2 ? launch_screen<KS, TT2, PAIR, PS, NOD>(a) : launch_screen<KS, 1, PAIR, PS, NOD>(a);
        });
      });
    });
  });
}

// Dynamic LDS of the screen kernel for Dx features and Cpad centres; -3 (as o3s_kmeans_screen2)
// when it exceeds the 160 KB of a workgroup: the caller takes the split kernel, which reads
// ||c||^2 from global memory when it does not fit.
O3S_API int o3s_kmeans_screen_lds(int Dx, int Cpad, int* lds_bytes) {
  size_t b = 0;
  const int rc = with_ksteps<10>((Dx + 31) / 32 * 32, [&](auto KS) {
    b = ScrLds<KS>::BYTES + sizeof(float) * (size_t)(Cpad > 0 ? Cpad : 0);
    return b > 160 * 1024 ? -3 : 0;
  });
  *lds_bytes = rc != 0 ? -1 : (int)b;
  return rc;
}

O3S_PRELOAD(kmeans_assign)

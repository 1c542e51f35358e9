// The 32-row MFMA tile that glm_softmax.hip, linear_predict.hip, fm.hip and mlp.hip are built
// on (gfx950), once.
//
// Lanes.  v_mfma_f32_32x32x16_bf16 with lane (r = lane & 31, h = lane >> 5):
//   forward  A = parameters (class / output / unit r, dims 8h..+8 of a 16-dim step) from LDS,
//            B = X (row r, the same 8 dims: exactly the lane's 16-B (bf16) or 32-B (fp32) global
//            load of the row) -> acc[v] = row r, class 4h + mt_cv(v);
//   backward A = residuals (class r, rows 8h..+8 of a 16-row step) from LDS, B = X^T (rows
//            8h..+8, dim r of a 32-dim block, read transposed from the wave's LDS copy of the
//            tile) -> G[nb][v] = class 4h + mt_cv(v), dim 32 nb + r.
// Rows past n are loaded clamped (the caller gives them weight 0 or never stores them), 16-column
// chunks at or past ldx are zero-filled, and the next tile is loaded into a second register copy
// while this one computes.
//
// Terms.  bf16 rows are exact.  Parameters come as three bf16 terms hi + mid + lo, each the
// rounding of the fp32 remainder so far (ops/_terms.py; on the device split_bf16x3 of
// glm_rows.h): results at fp32 level.  fp32 rows are split the same way as they are consumed,
// and two three-term operands meet in the six products of total order <= 2 only, smallest
// first (mt_mfma6).  Residual-like operands go through LDS as two terms hi + lo (split_bf16x2,
// 2^-17 relative) and meet another two-term operand in all four products (mt_mfma4), since
// lo x lo is as large as what a two-term split leaves behind.
//
// Sums over rows leave a kernel as one fp32 slab row per wave (or group of waves), summed in
// fp64 in a fixed order by glm_finish_kernel (glm_launch.h): no float atomics.
//
// The kernels are register-tuned around these helpers as they stand (by-value vector
// arguments, h and r passed in): a change here is checked with tools/isa_diff.py against the
// build before it (doc/performance.md).
#pragma once
#include <type_traits>

#include "glm_rows.h"

namespace {

typedef float mt_f32x16 __attribute__((ext_vector_type(16)));
typedef short mt_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t mt_u32x4 __attribute__((ext_vector_type(4)));

// register v of a lane's accumulator tile is class 4 h + mt_cv(v)
__device__ __forceinline__ constexpr int mt_cv(int v) { return 8 * (v >> 2) + (v & 3); }

// LDS row pitches (bf16 elements) for NB blocks of 32 dims.
template <int NB>
struct MtPitch {
  static constexpr int D = 32 * NB;
  static constexpr int WLD = D + 8;     // +16 B per row: conflict-free 16-B A-fragment reads
  static constexpr int XLD = D + 8;     // the same for the 16-B tile writes
  static constexpr int RLD = 40;        // 80-B rows: the 16-B R fragment reads hit distinct banks
};

__device__ __forceinline__ void mt_wave_sync() {   // this wave's LDS traffic done and visible to its lanes
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Parameter terms [ROWS][D] (ROWS = 3 x 32 x blocks: hi, mid, lo) -> LDS rows of pitch WLD.
template <int ROWS, int NB, int THREADS>
__device__ __forceinline__ void mt_stage_w(uint16_t* Ws, const uint16_t* __restrict__ Wsp) {
  constexpr int D = MtPitch<NB>::D, WLD = MtPitch<NB>::WLD;
  for (int p = threadIdx.x; p < ROWS * (D / 8); p += THREADS) {
    const int row = p / (D / 8), k8 = p % (D / 8);
    *reinterpret_cast<mt_bf16x8*>(Ws + row * WLD + k8 * 8) =
        *reinterpret_cast<const mt_bf16x8*>(Wsp + (int64_t)row * D + k8 * 8);
  }
}

// Row sources: the registers of one 16-dim step of a lane (dims 8h..+8 of row r).  NT: a
// non-temporal load (linear_predict, whose rows are read once and whose outputs are larger).
struct MtBf16 {
  using elem = uint16_t;
  using chunk = mt_bf16x8;
  template <bool NT>
  __device__ static __forceinline__ void load(const elem* p, chunk& c) {
    if constexpr (NT) c = __builtin_nontemporal_load(reinterpret_cast<const chunk*>(p));
    else c = *reinterpret_cast<const chunk*>(p);
  }
  __device__ static __forceinline__ void zero(chunk& c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = 0;
  }
};
struct MtF32 {
  using elem = float;
  struct chunk { float4_ a, b; };
  template <bool NT>
  __device__ static __forceinline__ void load(const elem* p, chunk& c) {
    if constexpr (NT) {
      c.a = __builtin_nontemporal_load(reinterpret_cast<const float4_*>(p));
      c.b = __builtin_nontemporal_load(reinterpret_cast<const float4_*>(p) + 1);
    } else {
      c.a = *reinterpret_cast<const float4_*>(p);
      c.b = *reinterpret_cast<const float4_*>(p + 4);
    }
  }
  __device__ static __forceinline__ void zero(chunk& c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c.a[j] = c.b[j] = 0.f;
  }
};

// This lane's share of tile `tile`: row 32 tile + r (clamped to n - 1), chunks 16 ks + 8 h.
template <class SRC, int KS, bool NT = false>
__device__ __forceinline__ void mt_load_tile(const typename SRC::elem* __restrict__ X, int64_t n, int64_t ldx,
                                             int64_t tile, int r, int h, typename SRC::chunk (&dst)[KS]) {
  int64_t row = tile * 32 + r;
  row = row < n ? row : n - 1;
  const typename SRC::elem* src = X + row * ldx;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int col = ks * 16 + 8 * h;
    if (col < ldx) {
      SRC::template load<NT>(src + col, dst[ks]);
    } else {
      SRC::zero(dst[ks]);
    }
  }
}

// 8 fp32 -> bf16 terms hi + mid + lo (split_bf16x3, pair by pair).
__device__ __forceinline__ void mt_split8(const float4_ a, const float4_ b, mt_bf16x8& hi, mt_bf16x8& mid,
                                          mt_bf16x8& lo) {
  mt_u32x4 ph, pm, pl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x0 = j < 2 ? a[2 * j] : b[2 * j - 4], x1 = j < 2 ? a[2 * j + 1] : b[2 * j - 3];
    uint32_t h, m, l;
    split_bf16x3(x0, x1, h, m, l);
    ph[j] = h;
    pm[j] = m;
    pl[j] = l;
  }
  hi = __builtin_bit_cast(mt_bf16x8, ph);
  mid = __builtin_bit_cast(mt_bf16x8, pm);
  lo = __builtin_bit_cast(mt_bf16x8, pl);
}

// acc += W x for one k-step of exact (bf16) rows: the three W terms in the order given.
__device__ __forceinline__ mt_f32x16 mt_mfma3(mt_f32x16 acc, const mt_bf16x8 wa, const mt_bf16x8 wb,
                                              const mt_bf16x8 wc, const mt_bf16x8 x) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa, x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wb, x, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(wc, x, acc, 0, 0, 0);
}
// W and x as hi + mid + lo terms (0, 1, 2): the six products of order <= 2, small ones first.
__device__ __forceinline__ mt_f32x16 mt_mfma6(mt_f32x16 acc, const mt_bf16x8 w0, const mt_bf16x8 w1,
                                              const mt_bf16x8 w2, const mt_bf16x8 x0, const mt_bf16x8 x1,
                                              const mt_bf16x8 x2) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, x0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x0, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, x0, acc, 0, 0, 0);
}
// The backward 2 x 2: residual terms r0 + r1 with row terms x0 + x1, small ones first.
__device__ __forceinline__ mt_f32x16 mt_mfma4(mt_f32x16 acc, const mt_bf16x8 r0, const mt_bf16x8 r1,
                                              const mt_bf16x8 x0, const mt_bf16x8 x1) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(r1, x1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(r0, x1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(r1, x0, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(r0, x0, acc, 0, 0, 0);
}

// Registers v, v + 1 (v even) of a residual tile -> LDS, class major [hi, lo][32][RLD], as two
// bf16 terms.  Rw = buffer + 4 h RLD + r.
__device__ __forceinline__ void mt_store_r_pair(uint16_t* Rw, int v, float rv0, float rv1, int RLD) {
  uint32_t ph, pl;
  split_bf16x2(rv0, rv1, ph, pl);
  Rw[mt_cv(v) * RLD] = (uint16_t)ph;
  Rw[mt_cv(v + 1) * RLD] = (uint16_t)(ph >> 16);
  Rw[(32 + mt_cv(v)) * RLD] = (uint16_t)pl;
  Rw[(32 + mt_cv(v + 1)) * RLD] = (uint16_t)(pl >> 16);
}

// The transposed B fragment: rows row0..+8 of column col of a tile in LDS.
__device__ __forceinline__ mt_bf16x8 mt_read_xt(const uint16_t* Xs, int row0, int col, int XLD) {
  mt_bf16x8 b;
#pragma unroll
  for (int q = 0; q < 8; ++q) b[q] = (short)Xs[(row0 + q) * XLD + col];
  return b;
}

// G (class major, 32 x D) -> the head of a slab row.
template <int NB>
__device__ __forceinline__ void mt_write_slab_g(const mt_f32x16 (&G)[NB], float* out, int r, int h) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) out[(4 * h + mt_cv(v)) * (32 * NB) + b * 32 + r] = G[b][v];
}

// ---- host side ----
// f(std::integral_constant<int, nb>) for 1 <= nb <= 8 blocks of 32 dims, else -1.
template <class F>
int mt_dispatch_nb(int nb, F&& f) {
  switch (nb) {
#define O3S_NB(V) case V: return f(std::integral_constant<int, V>{});
    O3S_NB(1) O3S_NB(2) O3S_NB(3) O3S_NB(4) O3S_NB(5) O3S_NB(6) O3S_NB(7) O3S_NB(8)
#undef O3S_NB
    default: return -1;
  }
}
// Launches of `grid` blocks, each `per_block` slab rows (or tile walks), until every one of the
// `walks` has had its waves: launch(blocks, first walk).
template <class F>
int mt_walk_slabs(int64_t walks, int grid, int per_block, F&& launch) {
  for (int64_t w0 = 0; w0 < walks; w0 += (int64_t)grid * per_block) {
    const int64_t left = (walks - w0 + per_block - 1) / per_block;
    launch((int)(grid < left ? grid : left), (int)w0);
    O3S_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

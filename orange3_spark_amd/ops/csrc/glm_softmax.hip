// Multinomial (softmax) logistic regression (gfx950), one fused pass over bf16 rows
// (glm_softmax_kernel) or over fp32 rows (glm_softmax_f32_kernel, further down):
//   margins M = X W^T + b (MFMA), row log-sum-exp, residual R = w (softmax(M) - onehot(y)),
//   gradient G = R^T X (MFMA), sum(R) per class and the weighted cross-entropy.
// Reference: Spark's MultinomialLogisticRegression aggregator reached from the
// Classification widget (orangecontrib/spark/widgets/ml/spark_ml_classification.py:15,
// SURVEY §2.8 "Multinomial: X.W with C classes uses MFMA").
//
// Layout (v_mfma_f32_32x32x16_bf16; lane (r = lane&31, h = lane>>5)):
//   forward  A = W split (32 classes x 16 dims, class r, dims 8h..+8), B = X (row r, the
//            same 8 dims -- exactly the 16-B global load of the row) -> acc[v] = margin of
//            row r, class 8(v>>2) + 4h + (v&3);
//   backward A = R split (class r, rows 8h..+8 of a 16-row step), B = X^T (rows 8h..+8,
//            dim r of a 32-dim block, read transposed from this wave's LDS copy of the
//            tile) -> G[nb][v] = dG of class 8(v>>2) + 4h + (v&3), dim 32 nb + r.
// X is exact in bf16; W is split into three bf16 terms (hi + mid + lo: margins and loss
// at fp32 level), the residuals R (|R| <= w) into two (hi + lo: ~2^-17 relative per term
// of the gradient sums).  The MFMA
// work is a few % of the HBM time of a tile: the kernel streams X once per pass (the
// next tile's rows are loaded while this tile computes).  One wave per SIMD (the
// 128-register gradient accumulators); per-wave slab rows, summed in fp64 by
// glm_finish_kernel (glm_launch.h) in a fixed order (no float atomics).
// The two kernels share nothing with the binary GLM passes but that finish kernel and the
// bf16 packing of glm_rows.h (pk_bf16, split_bf16x3).  Their differences from each other are
// deliberate (see the budget note at the fp32 kernel); both sit at one wave per SIMD with no
// scratch, which tools/isa_diff.py checks against the build before a change.
#include "glm_launch.h"

namespace {

typedef float sm_f32x16 __attribute__((ext_vector_type(16)));
typedef short sm_bf16x8 __attribute__((ext_vector_type(8)));
constexpr int kSmWaves = 4;
constexpr int kSmThreads = kSmWaves * kWave;

template <int NB>
struct SmLds {
  static constexpr int D = 32 * NB;
  static constexpr int WLD = D + 8;     // +16 B per row: conflict-free 16-B fragment reads
  static constexpr int XLD = D + 8;
  static constexpr int RLD = 40;        // 80-B rows: the 16-B R fragment reads hit distinct banks
  static constexpr int W_ELEMS = 3 * 32 * WLD;
  static constexpr int WAVE_ELEMS = 32 * XLD + 2 * 32 * RLD;
  static constexpr int ELEMS = W_ELEMS + kSmWaves * WAVE_ELEMS;
};

template <int NB>
__global__ __launch_bounds__(kSmThreads, 1) void glm_softmax_kernel(
    const uint16_t* __restrict__ X, int64_t n, int64_t ldx, const int32_t* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ bias, int K,
    float* __restrict__ partial, int pstride) {
  using L = SmLds<NB>;
  constexpr int D = L::D, KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;
  uint16_t* Rs = Xs + 32 * XLD;

  // W splits [3][32][D] -> LDS (padded rows)
  for (int p = threadIdx.x; p < 3 * 32 * (D / 8); p += kSmThreads) {
    const int row = p / (D / 8), k8 = p % (D / 8);
    *reinterpret_cast<sm_bf16x8*>(Ws + row * WLD + k8 * 8) =
        *reinterpret_cast<const sm_bf16x8*>(Wsp + (int64_t)row * D + k8 * 8);
  }
  float bl[16];
  int cls[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    cls[v] = 8 * (v >> 2) + 4 * h + (v & 3);
    bl[v] = cls[v] < K ? bias[cls[v]] : -INFINITY;
  }
  __syncthreads();

  sm_f32x16 G[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) G[b][v] = 0.f;
  float gb[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) gb[v] = 0.f;
  float lossacc = 0.f;

  const int64_t ntiles = (n + 31) / 32;
  const int64_t step = (int64_t)gridDim.x * kSmWaves;
  int64_t tile = (int64_t)blockIdx.x * kSmWaves + wid;
  sm_bf16x8 xb[KS], xn[KS];
  auto load = [&](int64_t t, sm_bf16x8 (&dst)[KS]) {
    int64_t row = t * 32 + r;
    row = row < n ? row : n - 1;
    const uint16_t* src = X + row * ldx;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int col = ks * 16 + 8 * h;
      if (col < ldx) {
        dst[ks] = *reinterpret_cast<const sm_bf16x8*>(src + col);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[ks][j] = 0;
      }
    }
  };
  if (tile < ntiles) load(tile, xb);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) load(tile + step, xn);
    const int64_t row = tile * 32 + r;
    const bool valid = row < n;
    const int yl = valid ? y[row] : -1;
    const float wr = valid ? (sw ? sw[row] : 1.f) : 0.f;
    // ---- forward: margins of row r, 16 classes per lane
    sm_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = bl[v];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const sm_bf16x8 a = *reinterpret_cast<const sm_bf16x8*>(Ws + (s * 32 + r) * WLD + ks * 16 + 8 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[ks], acc, 0, 0, 0);
      }
      *reinterpret_cast<sm_bf16x8*>(Xs + r * XLD + ks * 16 + 8 * h) = xb[ks];   // for the X^T reads
    }
    // ---- row softmax (the two half-waves hold disjoint class subsets of row r)
    float mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) mx = fmaxf(mx, acc[v]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float se = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) se += __expf(acc[v] - mx);
    se += __shfl_xor(se, 32, 64);
    const float lse = mx + __logf(se);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const bool hit = cls[v] == yl;
      const float p = __expf(acc[v] - lse);
      const float rv = wr * (p - (hit ? 1.f : 0.f));
      gb[v] += rv;
      if (hit) lossacc += wr * (lse - acc[v]);
      const uint16_t a0 = f32_to_bf16(rv);
      Rs[(0 * 32 + cls[v]) * RLD + r] = a0;
      Rs[(1 * 32 + cls[v]) * RLD + r] = f32_to_bf16(rv - bf16_to_f32(a0));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // ---- backward: G[class][dim] += sum over the tile's rows of R[row][class] X[row][dim]
    sm_bf16x8 ar[2][2];
#pragma unroll
    for (int rs = 0; rs < 2; ++rs)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        ar[rs][s] = *reinterpret_cast<const sm_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        sm_bf16x8 bx;
#pragma unroll
        for (int q = 0; q < 8; ++q) bx[q] = (short)Xs[(rs * 16 + 8 * h + q) * XLD + b * 32 + r];
#pragma unroll
        for (int s = 0; s < 2; ++s) G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][s], bx, G[b], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // tile's LDS reads done before it is overwritten
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xb[ks] = xn[ks];
  }
  // ---- this wave's slab row: [G class-major 32 x D | sum R (32) | loss]
  float* out = partial + ((int64_t)blockIdx.x * kSmWaves + wid) * pstride;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) out[cls[v] * D + b * 32 + r] = G[b][v];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float s = gb[v];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);   // over the 32 rows (same h)
    if (r == 0) out[32 * D + cls[v]] = s;
  }
  const float lt = wave_sum(lossacc);
  if (lane == 0) out[32 * D + 32] = lt;
}

}  // namespace

// ---------------------------------------------------------------------------------
// Multinomial pass over fp32 rows: the contract, MFMA layouts, slab rows and finish of
// glm_softmax_kernel above, for X = float [n, ldx].
//
// gfx950 has no xf32 and its f32-input MFMA runs at 1/16 of the bf16 rate, so a row is
// split into bf16 terms as it is consumed (v_cvt_pk_bf16_f32 of the running remainder,
// every subtraction exact): hi + mid + lo forward, where the margins and the loss have to
// be at fp32 level, hi + mid backward (2^-17 relative, below the two-term split of R).
// Forward products of total order <= 2 only (X hi with the three W terms, X mid with W hi
// and mid, X lo with W hi: 6 MFMAs per 16 dims where the bf16 kernel issues 3); backward
// all four of (R hi, R lo) x (X hi, X mid).
//
// Budget.  An fp32 tile is twice the bytes of a bf16 one, so neither of the bf16 kernel's
// two tile copies carries over: four 32-row hi + mid tiles and the W splits exceed the
// 160 KB of LDS, and two fp32 register copies are 256 VGPRs.  Chosen here, to keep four
// waves per CU (one per SIMD) and a whole tile of loads in flight per wave:
//   * the forward takes its X operand straight from the registers the row was loaded into
//     (row r, dims 8h..+8 is one lane's 32-B load) and leaves the packed hi and mid terms
//     in them -- the same 8 registers per 16 dims;
//   * only the backward operand goes through LDS, 16 rows (one MFMA k-step) at a time: the
//     half-wave that holds those rows writes hi and mid, all lanes read them transposed.
//     [2][16][XLD] is exactly the bf16 kernel's 32-row tile area, so SmLds serves both;
//   * the next tile is prefetched by plain vector loads into a second fp32 register copy
//     (no LDS-DMA).  With the 128 accumulator registers that is 384 of the 512 registers
//     a lone wave per SIMD has; the bias lives in LDS and the class of an accumulator
//     register is recomputed from the lane id so that the NB = 8 instantiation stays out
//     of scratch (doc/performance.md has the table).
// Chunks at or past ldx are zero-filled, rows past n are clamped and carry weight 0.
namespace {

typedef uint32_t sm_u32x4 __attribute__((ext_vector_type(4)));

// 8 fp32 -> bf16 terms hi + mid + lo (split_bf16x3 of glm_rows.h, pair by pair).
__device__ __forceinline__ void split8(const float4_ a, const float4_ b, sm_bf16x8& hi, sm_bf16x8& mid,
                                       sm_bf16x8& lo) {
  sm_u32x4 ph, pm, pl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x0 = j < 2 ? a[2 * j] : b[2 * j - 4], x1 = j < 2 ? a[2 * j + 1] : b[2 * j - 3];
    uint32_t h, m, l;
    split_bf16x3(x0, x1, h, m, l);
    ph[j] = h;
    pm[j] = m;
    pl[j] = l;
  }
  hi = __builtin_bit_cast(sm_bf16x8, ph);
  mid = __builtin_bit_cast(sm_bf16x8, pm);
  lo = __builtin_bit_cast(sm_bf16x8, pl);
}

template <int NB>
__global__ __launch_bounds__(kSmThreads, 1) void glm_softmax_f32_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const int32_t* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ bias, int K,
    float* __restrict__ partial, int pstride) {
  using L = SmLds<NB>;
  constexpr int D = L::D, KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  __shared__ __attribute__((aligned(16))) float bs[32];   // bias, -inf for the classes past K
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;   // [hi, mid][16 rows][XLD]
  uint16_t* Rs = Xs + 32 * XLD;

  for (int p = threadIdx.x; p < 3 * 32 * (D / 8); p += kSmThreads) {
    const int row = p / (D / 8), k8 = p % (D / 8);
    *reinterpret_cast<sm_bf16x8*>(Ws + row * WLD + k8 * 8) =
        *reinterpret_cast<const sm_bf16x8*>(Wsp + (int64_t)row * D + k8 * 8);
  }
  // register v of a lane's accumulator tile is class 4 h + cv(v)
  auto cv = [](int v) { return 8 * (v >> 2) + (v & 3); };
  if (threadIdx.x < 32) bs[threadIdx.x] = (int)threadIdx.x < K ? bias[threadIdx.x] : -INFINITY;
  uint16_t* Rw = Rs + 4 * h * RLD + r;
  __syncthreads();

  sm_f32x16 G[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) G[b][v] = 0.f;
  float gb[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) gb[v] = 0.f;
  float lossacc = 0.f;

  const int64_t ntiles = (n + 31) / 32;
  const int64_t step = (int64_t)gridDim.x * kSmWaves;
  int64_t tile = (int64_t)blockIdx.x * kSmWaves + wid;
  float4_ xf[KS][2], xn[KS][2];
  auto load = [&](int64_t t, float4_ (*dst)[2]) {
    int64_t row = t * 32 + r;
    row = row < n ? row : n - 1;
    const float* src = X + row * ldx;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int col = ks * 16 + 8 * h;
      if (col < ldx) {
        dst[ks][0] = *reinterpret_cast<const float4_*>(src + col);
        dst[ks][1] = *reinterpret_cast<const float4_*>(src + col + 4);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[ks][0][j] = dst[ks][1][j] = 0.f;
      }
    }
  };
  if (tile < ntiles) load(tile, xf);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) load(tile + step, xn);
    const int64_t row = tile * 32 + r;
    const bool valid = row < n;
    const int ylh = (valid ? y[row] : -1) - 4 * h;   // label relative to this half-wave's classes
    const float wr = valid ? (sw ? sw[row] : 1.f) : 0.f;
    // ---- forward: margins of row r, 16 classes per lane; the hi and mid terms of the row
    // stay in the registers the fp32 values came in, for the backward staging below
    sm_f32x16 acc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4_ b4 = *reinterpret_cast<const float4_*>(bs + 8 * j + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[4 * j + u] = b4[u];
    }
    sm_bf16x8 xh[KS], xm[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      sm_bf16x8 xl;
      split8(xf[ks][0], xf[ks][1], xh[ks], xm[ks], xl);
      const uint16_t* wp = Ws + r * WLD + ks * 16 + 8 * h;
      const sm_bf16x8 a0 = *reinterpret_cast<const sm_bf16x8*>(wp);
      const sm_bf16x8 a1 = *reinterpret_cast<const sm_bf16x8*>(wp + 32 * WLD);
      const sm_bf16x8 a2 = *reinterpret_cast<const sm_bf16x8*>(wp + 64 * WLD);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, xh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xm[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xm[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xh[ks], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- row softmax (the two half-waves hold disjoint class subsets of row r)
    float mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) mx = fmaxf(mx, acc[v]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float se = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) se += __expf(acc[v] - mx);
    se += __shfl_xor(se, 32, 64);
    const float lse = mx + __logf(se);
#pragma unroll
    for (int v = 0; v < 16; v += 2) {
      float rv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bool hit = cv(v + u) == ylh;
        rv[u] = wr * (__expf(acc[v + u] - lse) - (hit ? 1.f : 0.f));
        gb[v + u] += rv[u];
        if (hit) lossacc += wr * (lse - acc[v + u]);
      }
      const uint32_t ph = pk_bf16(rv[0], rv[1]);
      const uint32_t pl = pk_bf16(rv[0] - __uint_as_float(ph << 16), rv[1] - __uint_as_float(ph & 0xffff0000u));
      Rw[cv(v) * RLD] = (uint16_t)ph;
      Rw[cv(v + 1) * RLD] = (uint16_t)(ph >> 16);
      Rw[(32 + cv(v)) * RLD] = (uint16_t)pl;
      Rw[(32 + cv(v + 1)) * RLD] = (uint16_t)(pl >> 16);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // ---- backward: G[class][dim] += sum over the tile's rows of R[row][class] X[row][dim],
    // 16 rows (one MFMA k-step) at a time through this wave's staging area
    sm_bf16x8 ar[2][2];
#pragma unroll
    for (int rs = 0; rs < 2; ++rs)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        ar[rs][s] = *reinterpret_cast<const sm_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) {
      if ((r >> 4) == rs) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          *reinterpret_cast<sm_bf16x8*>(Xs + (r & 15) * XLD + ks * 16 + 8 * h) = xh[ks];
          *reinterpret_cast<sm_bf16x8*>(Xs + (16 + (r & 15)) * XLD + ks * 16 + 8 * h) = xm[ks];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        sm_bf16x8 bh, bm;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          bh[q] = (short)Xs[(8 * h + q) * XLD + b * 32 + r];
          bm[q] = (short)Xs[(16 + 8 * h + q) * XLD + b * 32 + r];
        }
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][1], bm, G[b], 0, 0, 0);
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][0], bm, G[b], 0, 0, 0);
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][1], bh, G[b], 0, 0, 0);
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][0], bh, G[b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // staged reads done before the area is overwritten
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      xf[ks][0] = xn[ks][0];
      xf[ks][1] = xn[ks][1];
    }
  }
  // ---- this wave's slab row: [G class-major 32 x D | sum R (32) | loss]
  float* out = partial + ((int64_t)blockIdx.x * kSmWaves + wid) * pstride;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) out[(4 * h + cv(v)) * D + b * 32 + r] = G[b][v];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float s = gb[v];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (r == 0) out[32 * D + 4 * h + cv(v)] = s;
  }
  const float lt = wave_sum(lossacc);
  if (lane == 0) out[32 * D + 32] = lt;
}

// The two kernel families, as the host pass below takes them: the rows' element type and the
// kernel for NB blocks of 32 dims.
struct SoftmaxBf16 {
  using elem = uint16_t;
  template <int NB> static auto kernel() { return glm_softmax_kernel<NB>; }
};
struct SoftmaxF32 {
  using elem = float;
  template <int NB> static auto kernel() { return glm_softmax_f32_kernel<NB>; }
};

// What the two entry points share: the argument check, the launch of the family's kernel for
// nb = ceil(d / 32) (an empty pass zeroes the slab instead) and the fp64 finish over the
// per-wave slab rows.
template <class FAM>
int softmax_pass(const void* X, int64_t n, int64_t ldx, int d, const int32_t* y, const float* sw, const void* Wsp,
                 const float* bias, int K, float* partial, int grid, double* out, hipStream_t st) {
  const int nb = (d + 31) / 32;
  if (ldx % 8 != 0 || nb < 1 || nb > 8 || K < 1 || K > 32 || grid <= 0) return -1;
  const int D = 32 * nb, pstride = 32 * D + 33;
  const auto* Xe = (const typename FAM::elem*)X;
  const uint16_t* Wh = (const uint16_t*)Wsp;
  if (n > 0) {
    switch (nb) {
#define O3S_SM(NBV) \
  case NBV: hipLaunchKernelGGL(FAM::template kernel<NBV>(), dim3(grid), dim3(kSmThreads), 0, st, Xe, n, ldx, y, sw, \
                               Wh, bias, K, partial, pstride); break;
      O3S_SM(1) O3S_SM(2) O3S_SM(3) O3S_SM(4) O3S_SM(5) O3S_SM(6) O3S_SM(7) O3S_SM(8)
#undef O3S_SM
      default: return -1;
    }
  } else {
    hipMemsetAsync(partial, 0, sizeof(float) * pstride * (size_t)grid * kSmWaves, st);
  }
  return launch_finish(partial, grid * kSmWaves, pstride, pstride, out, 0, st);
}

}  // namespace

// One multinomial pass: out (fp64, [32 * D | 32 | 1]) = (gradient class-major over
// D = 32 * ceil(d / 32) dims, per-class residual sums, weighted cross-entropy) over the n
// rows of X (bf16, row stride ldx, ldx % 8 == 0).  y: int32 labels in [0, K); sw: fp32
// weights or null; Wsp: bf16 [3][32][D] (hi, mid, lo splits of the class-major
// coefficients, zero-padded); bias: fp32 [32].  partial: fp32 [grid * 4][32 D + 33].
O3S_API int o3s_glm_softmax(const void* X, int64_t n, int64_t ldx, int d, const int32_t* y, const float* sw,
                            const void* Wsp, const float* bias, int K, float* partial, int grid, double* out,
                            hipStream_t st) {
  return softmax_pass<SoftmaxBf16>(X, n, ldx, d, y, sw, Wsp, bias, K, partial, grid, out, st);
}

// One multinomial pass over fp32 rows: the arguments, the out / partial layout and the
// return codes of o3s_glm_softmax with X = float [n, ldx] (ldx % 8 == 0).
O3S_API int o3s_glm_softmax_f32(const void* X, int64_t n, int64_t ldx, int d, const int32_t* y, const float* sw,
                                const void* Wsp, const float* bias, int K, float* partial, int grid, double* out,
                                hipStream_t st) {
  return softmax_pass<SoftmaxF32>(X, n, ldx, d, y, sw, Wsp, bias, K, partial, grid, out, st);
}

O3S_PRELOAD(glm_softmax)

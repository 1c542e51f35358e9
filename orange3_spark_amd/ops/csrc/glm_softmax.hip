// Multinomial (softmax) logistic regression (gfx950), one fused pass over bf16 rows
// (glm_softmax_kernel) or over fp32 rows (glm_softmax_f32_kernel, further down):
//   margins M = X W^T + b (MFMA), row log-sum-exp, residual R = w (softmax(M) - onehot(y)),
//   gradient G = R^T X (MFMA), sum(R) per class and the weighted cross-entropy.
// Reference: Spark's MultinomialLogisticRegression aggregator reached from the
// Classification widget (orangecontrib/spark/widgets/ml/spark_ml_classification.py:15,
// SURVEY §2.8 "Multinomial: X.W with C classes uses MFMA").
//
// The tile, its lane layout and the term splitting are those of mfma_tile.h: W as three terms,
// the residuals R (|R| <= w) as two.  The MFMA work is a few % of the HBM time of a tile: the
// kernel streams X once per pass.  One wave per SIMD (the 128-register gradient accumulators);
// per-wave slab rows [G class-major 32 x D | sum R (32) | loss].
// The two kernels' differences from each other are deliberate (see the budget note at the fp32
// kernel); both sit at one wave per SIMD with no scratch, which tools/isa_diff.py checks
// against the build before a change.
#include "glm_launch.h"
#include "mfma_tile.h"

namespace {

constexpr int kSmWaves = 4;
constexpr int kSmThreads = kSmWaves * kWave;

template <int NB>
struct SmLds : MtPitch<NB> {
  using P = MtPitch<NB>;
  static constexpr int W_ELEMS = 3 * 32 * P::WLD;
  static constexpr int WAVE_ELEMS = 32 * P::XLD + 2 * 32 * P::RLD;
  static constexpr int ELEMS = W_ELEMS + kSmWaves * WAVE_ELEMS;
};

// Label and weight of row `row` (-1 and 0 past n).
__device__ __forceinline__ void sm_row(int64_t row, int64_t n, const int32_t* __restrict__ y,
                                       const float* __restrict__ sw, int& yl, float& wr) {
  const bool valid = row < n;
  yl = valid ? y[row] : -1;
  wr = valid ? (sw ? sw[row] : 1.f) : 0.f;
}
// Row log-sum-exp (the two half-waves hold disjoint class subsets of row r).
__device__ __forceinline__ float sm_lse(const mt_f32x16 acc) {
  float mx = -INFINITY;
#pragma unroll
  for (int v = 0; v < 16; ++v) mx = fmaxf(mx, acc[v]);
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  float se = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) se += __expf(acc[v] - mx);
  se += __shfl_xor(se, 32, 64);
  return mx + __logf(se);
}
// This wave's slab row: [G class-major 32 x D | sum R (32) | loss]
template <int NB>
__device__ __forceinline__ void sm_write_slab(const mt_f32x16 (&G)[NB], const float (&gb)[16], float lossacc,
                                              float* out, int r, int h, int lane) {
  constexpr int D = 32 * NB;
  mt_write_slab_g<NB>(G, out, r, h);
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float s = gb[v];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);   // over the 32 rows (same h)
    if (r == 0) out[32 * D + 4 * h + mt_cv(v)] = s;
  }
  const float lt = wave_sum(lossacc);
  if (lane == 0) out[32 * D + 32] = lt;
}

template <int NB>
__global__ __launch_bounds__(kSmThreads, 1) void glm_softmax_kernel(
    const uint16_t* __restrict__ X, int64_t n, int64_t ldx, const int32_t* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ bias, int K,
    float* __restrict__ partial, int pstride) {
  using L = SmLds<NB>;
  constexpr int KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;
  uint16_t* Rs = Xs + 32 * XLD;

  mt_stage_w<3 * 32, NB, kSmThreads>(Ws, Wsp);
  float bl[16];
  int cls[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    cls[v] = 4 * h + mt_cv(v);
    bl[v] = cls[v] < K ? bias[cls[v]] : -INFINITY;
  }
  __syncthreads();

  mt_f32x16 G[NB];
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
  mt_bf16x8 xb[KS], xn[KS];
  if (tile < ntiles) mt_load_tile<MtBf16, KS>(X, n, ldx, tile, r, h, xb);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) mt_load_tile<MtBf16, KS>(X, n, ldx, tile + step, r, h, xn);
    int yl;
    float wr;
    sm_row(tile * 32 + r, n, y, sw, yl, wr);
    // ---- forward: margins of row r, 16 classes per lane
    mt_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = bl[v];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint16_t* wp = Ws + r * WLD + ks * 16 + 8 * h;
      acc = mt_mfma3(acc, *reinterpret_cast<const mt_bf16x8*>(wp), *reinterpret_cast<const mt_bf16x8*>(wp + 32 * WLD),
                     *reinterpret_cast<const mt_bf16x8*>(wp + 64 * WLD), xb[ks]);
      *reinterpret_cast<mt_bf16x8*>(Xs + r * XLD + ks * 16 + 8 * h) = xb[ks];   // for the X^T reads
    }
    const float lse = sm_lse(acc);
    // (the residual terms by integer rounding here, by v_cvt_pk_bf16_f32 in the fp32 kernel)
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
    mt_wave_sync();
    // ---- backward: G[class][dim] += sum over the tile's rows of R[row][class] X[row][dim]
    mt_bf16x8 ar[2][2];
#pragma unroll
    for (int rs = 0; rs < 2; ++rs)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        ar[rs][s] = *reinterpret_cast<const mt_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        const mt_bf16x8 bx = mt_read_xt(Xs, rs * 16 + 8 * h, b * 32 + r, XLD);
#pragma unroll
        for (int s = 0; s < 2; ++s) G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][s], bx, G[b], 0, 0, 0);
      }
    }
    mt_wave_sync();    // tile's LDS reads done before it is overwritten
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xb[ks] = xn[ks];
  }
  sm_write_slab<NB>(G, gb, lossacc, partial + ((int64_t)blockIdx.x * kSmWaves + wid) * pstride, r, h, lane);
}

// ---------------------------------------------------------------------------------
// Multinomial pass over fp32 rows: the contract, MFMA layouts, slab rows and finish of
// glm_softmax_kernel above, for X = float [n, ldx].
//
// gfx950 has no xf32 and its f32-input MFMA runs at 1/16 of the bf16 rate, so a row is
// split into bf16 terms as it is consumed (v_cvt_pk_bf16_f32 of the running remainder,
// every subtraction exact): hi + mid + lo forward, where the margins and the loss have to
// be at fp32 level, hi + mid backward (2^-17 relative, below the two-term split of R).
// Forward products of total order <= 2 only (6 MFMAs per 16 dims where the bf16 kernel issues
// 3); backward all four of (R hi, R lo) x (X hi, X mid).
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
template <int NB>
__global__ __launch_bounds__(kSmThreads, 1) void glm_softmax_f32_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const int32_t* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ bias, int K,
    float* __restrict__ partial, int pstride) {
  using L = SmLds<NB>;
  constexpr int KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  __shared__ __attribute__((aligned(16))) float bs[32];   // bias, -inf for the classes past K
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;   // [hi, mid][16 rows][XLD]
  uint16_t* Rs = Xs + 32 * XLD;

  mt_stage_w<3 * 32, NB, kSmThreads>(Ws, Wsp);
  if (threadIdx.x < 32) bs[threadIdx.x] = (int)threadIdx.x < K ? bias[threadIdx.x] : -INFINITY;
  uint16_t* Rw = Rs + 4 * h * RLD + r;
  __syncthreads();

  mt_f32x16 G[NB];
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
  MtF32::chunk xf[KS], xn[KS];
  if (tile < ntiles) mt_load_tile<MtF32, KS>(X, n, ldx, tile, r, h, xf);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) mt_load_tile<MtF32, KS>(X, n, ldx, tile + step, r, h, xn);
    int yl;
    float wr;
    sm_row(tile * 32 + r, n, y, sw, yl, wr);
    const int ylh = yl - 4 * h;   // label relative to this half-wave's classes
    // ---- forward: margins of row r, 16 classes per lane; the hi and mid terms of the row
    // stay in the registers the fp32 values came in, for the backward staging below
    mt_f32x16 acc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4_ b4 = *reinterpret_cast<const float4_*>(bs + 8 * j + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[4 * j + u] = b4[u];
    }
    mt_bf16x8 xh[KS], xm[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      mt_bf16x8 xl;
      mt_split8(xf[ks].a, xf[ks].b, xh[ks], xm[ks], xl);
      const uint16_t* wp = Ws + r * WLD + ks * 16 + 8 * h;
      acc = mt_mfma6(acc, *reinterpret_cast<const mt_bf16x8*>(wp), *reinterpret_cast<const mt_bf16x8*>(wp + 32 * WLD),
                     *reinterpret_cast<const mt_bf16x8*>(wp + 64 * WLD), xh[ks], xm[ks], xl);
      __builtin_amdgcn_sched_barrier(0);
    }
    const float lse = sm_lse(acc);
#pragma unroll
    for (int v = 0; v < 16; v += 2) {
      float rv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bool hit = mt_cv(v + u) == ylh;
        rv[u] = wr * (__expf(acc[v + u] - lse) - (hit ? 1.f : 0.f));
        gb[v + u] += rv[u];
        if (hit) lossacc += wr * (lse - acc[v + u]);
      }
      mt_store_r_pair(Rw, v, rv[0], rv[1], RLD);
    }
    mt_wave_sync();
    // ---- backward: G[class][dim] += sum over the tile's rows of R[row][class] X[row][dim],
    // 16 rows (one MFMA k-step) at a time through this wave's staging area
    mt_bf16x8 ar[2][2];
#pragma unroll
    for (int rs = 0; rs < 2; ++rs)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        ar[rs][s] = *reinterpret_cast<const mt_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) {
      if ((r >> 4) == rs) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          *reinterpret_cast<mt_bf16x8*>(Xs + (r & 15) * XLD + ks * 16 + 8 * h) = xh[ks];
          *reinterpret_cast<mt_bf16x8*>(Xs + (16 + (r & 15)) * XLD + ks * 16 + 8 * h) = xm[ks];
        }
      }
      mt_wave_sync();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const mt_bf16x8 bh = mt_read_xt(Xs, 8 * h, b * 32 + r, XLD), bm = mt_read_xt(Xs, 16 + 8 * h, b * 32 + r, XLD);
        G[b] = mt_mfma4(G[b], ar[rs][0], ar[rs][1], bh, bm);
        __builtin_amdgcn_sched_barrier(0);
      }
      mt_wave_sync();    // staged reads done before the area is overwritten
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xf[ks] = xn[ks];
  }
  sm_write_slab<NB>(G, gb, lossacc, partial + ((int64_t)blockIdx.x * kSmWaves + wid) * pstride, r, h, lane);
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
    mt_dispatch_nb(nb, [&](auto NB) {
      hipLaunchKernelGGL(FAM::template kernel<NB>(), dim3(grid), dim3(kSmThreads), 0, st, Xe, n, ldx, y, sw, Wh, bias,
                         K, partial, pstride);
      return 0;
    });
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

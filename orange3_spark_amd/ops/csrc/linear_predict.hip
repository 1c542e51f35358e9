// Scoring of the multi-output linear models (gfx950): Y = X W^T + b for 1 <= K <= 32 outputs
// over bf16 or fp32 rows, with the row softmax / argmax epilogue of a classifier, written as
// the frame's fp64 columns in the same pass.  Serves multinomial LogisticRegressionModel,
// NaiveBayesModel (multinomial, bernoulli, complement) and PCAModel.transform
// (ops/linear_predict.py).  Reference: the `transform` of the fitted Spark models that the
// Classification / PCA widgets apply (orangecontrib/spark/base/spark_ml_estimator.py).
//
// The tile is the forward half of mfma_tile.h: 3 MFMAs per 16 dims on bf16 rows, 6 on fp32
// rows, outputs at fp32 level.  The bias comes as hi + lo floats: the
// accumulators start from hi, lo is added after the products (a bernoulli NaiveBayes bias
// reaches hundreds; one float would shift a whole class by its rounding).
//
// Epilogue, each output optional (null pointer), all fp64:
//   raw  [n, ldo]  margins, or margins - row log-sum-exp (LP_LOG_SOFTMAX_RAW);
//   prob [n, ldo]  exp(m - max) / sum of those very values (rows sum to 1 within K 2^-24);
//   pred [n]       index of the largest margin, the lowest index on equal margins.
// The outputs past K start from a -inf bias, so they drop out of max, sum and argmax.  The
// row reductions are in-lane plus one exchange with lane ^ 32.
//
// No cross-row reduction, no atomics, no slabs: a row's outputs depend on the row and the
// operands alone, so any grid gives the same bits.  Rows past n are clamped on load and never
// stored; 16-B chunks at or past ldx are zero-filled; columns in [d, ldx) meet zero columns
// of W (finite padding assumed, as in glm_softmax_kernel).
//
// Stores.  With ldo == K a tile's 32 rows x K outputs are one contiguous range: the wave
// stages the fp32 values in its 4 KB of LDS in output order and stores them as 16-B pairs of
// doubles, 1 KB contiguous per instruction.  With ldo != K (column blocks of a wider output)
// or LP_DIRECT_STORE each lane stores its 32-B fragments itself.
//
// The rows are loaded non-temporally.  Without gradient accumulators the kernel holds two waves per SIMD; only
// fp32 rows wider than 128 dims, whose two register copies alone are 256 VGPRs, stay at one
// (doc/performance.md has the table; no instantiation uses scratch).
#include "mfma_tile.h"

namespace {

typedef double lp_f64x2 __attribute__((ext_vector_type(2)));
constexpr int kLpWaves = 4;
constexpr int kLpThreads = kLpWaves * kWave;
constexpr int kLpStage = 32 * 32;        // floats of one wave's staged output tile
constexpr int kLpMaxLds = 160 * 1024;
enum { LP_LOG_SOFTMAX_RAW = 1, LP_DIRECT_STORE = 2 };

template <int NB>
struct LpLds : MtPitch<NB> {
  static constexpr int W_ELEMS = 3 * 32 * MtPitch<NB>::WLD;
  static constexpr int BYTES = 2 * W_ELEMS + 4 * kLpWaves * kLpStage + 4 * 64;
};

// The row sources of mfma_tile.h and how a chunk meets the three W terms a0 (hi), a1 (mid),
// a2 (lo), smallest terms first.
struct LpBf16 : MtBf16 {
  __device__ static __forceinline__ void mma(const mt_bf16x8 a0, const mt_bf16x8 a1, const mt_bf16x8 a2,
                                             const chunk& c, mt_f32x16& acc) {
    acc = mt_mfma3(acc, a2, a1, a0, c);
  }
};
struct LpF32 : MtF32 {
  __device__ static __forceinline__ void mma(const mt_bf16x8 a0, const mt_bf16x8 a1, const mt_bf16x8 a2,
                                             const chunk& c, mt_f32x16& acc) {
    mt_bf16x8 xh, xm, xl;
    mt_split8(c.a, c.b, xh, xm, xl);
    acc = mt_mfma6(acc, a0, a1, a2, xh, xm, xl);
  }
};

// Waves per SIMD the kernel is compiled for (the register budget of __launch_bounds__).
template <class SRC, int NB>
constexpr int lp_min_blocks() {
  return (sizeof(typename SRC::elem) == 4 && NB > 4) ? 1 : 2;
}

template <class SRC, int NB>
__global__ __launch_bounds__(kLpThreads, (lp_min_blocks<SRC, NB>())) void linear_predict_kernel(
    const typename SRC::elem* __restrict__ X, int64_t n, int64_t ldx, const uint16_t* __restrict__ Wsp,
    const float* __restrict__ bias_hi, const float* __restrict__ bias_lo, int K, int flags,
    double* __restrict__ raw, double* __restrict__ prob, double* __restrict__ pred, int64_t ldo) {
  using L = LpLds<NB>;
  using chunk = typename SRC::chunk;
  constexpr int KS = 2 * NB, WLD = L::WLD;
  __shared__ __attribute__((aligned(16))) uint16_t Ws[L::W_ELEMS];
  __shared__ __attribute__((aligned(16))) float stage[kLpWaves * kLpStage];
  __shared__ __attribute__((aligned(16))) float bs[64];   // bias hi (-inf past K) | bias lo
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  float* St = stage + wid * kLpStage;

  mt_stage_w<3 * 32, NB, kLpThreads>(Ws, Wsp);
  if (threadIdx.x < 32) {
    const bool in = (int)threadIdx.x < K;
    bs[threadIdx.x] = in ? bias_hi[threadIdx.x] : -INFINITY;
    bs[32 + threadIdx.x] = in ? bias_lo[threadIdx.x] : 0.f;
  }
  __syncthreads();

  const bool staged = ldo == K && !(flags & LP_DIRECT_STORE);
  const bool lsm = (flags & LP_LOG_SOFTMAX_RAW) != 0;
  const bool need_exp = prob != nullptr || (lsm && raw != nullptr);

  const int64_t ntiles = (n + 31) / 32;
  const int64_t step = (int64_t)gridDim.x * kLpWaves;
  int64_t tile = (int64_t)blockIdx.x * kLpWaves + wid;
  chunk xb[KS], xn[KS];
  if (tile < ntiles) mt_load_tile<SRC, KS, true>(X, n, ldx, tile, r, h, xb);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) mt_load_tile<SRC, KS, true>(X, n, ldx, tile + step, r, h, xn);
    const int64_t row0 = tile * 32, row = row0 + r;
    const bool valid = row < n;
    const int nrows = n - row0 < 32 ? (int)(n - row0) : 32;

    // ---- outputs of row r, 16 per lane
    mt_f32x16 acc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4_ b4 = *reinterpret_cast<const float4_*>(bs + 8 * j + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[4 * j + u] = b4[u];
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint16_t* wp = Ws + r * WLD + ks * 16 + 8 * h;
      const mt_bf16x8 a0 = *reinterpret_cast<const mt_bf16x8*>(wp);
      const mt_bf16x8 a1 = *reinterpret_cast<const mt_bf16x8*>(wp + 32 * WLD);
      const mt_bf16x8 a2 = *reinterpret_cast<const mt_bf16x8*>(wp + 64 * WLD);
      SRC::mma(a0, a1, a2, xb[ks], acc);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4_ b4 = *reinterpret_cast<const float4_*>(bs + 32 + 8 * j + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[4 * j + u] += b4[u];
    }

    // ---- one output matrix: vals[v] is output 4 h + mt_cv(v) of row r
    auto emit = [&](double* __restrict__ out, const mt_f32x16& vals) {
      if (staged) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int c = 4 * h + mt_cv(v);
          if (c < K) St[r * K + c] = vals[v];
        }
        mt_wave_sync();
        const int E = nrows * K;
        double* base = out + row0 * K;
        for (int i = 2 * lane; i < E; i += 2 * kWave) {
          if (i + 1 < E) {
            const float2_ f = *reinterpret_cast<const float2_*>(St + i);
            lp_f64x2 dv;
            dv[0] = (double)f[0];
            dv[1] = (double)f[1];
            *reinterpret_cast<lp_f64x2*>(base + i) = dv;
          } else {
            base[i] = (double)St[i];
          }
        }
        mt_wave_sync();   // staged reads done before the next overwrite
      } else if (valid) {
        double* o = out + row * ldo + 4 * h;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          if (4 * h + mt_cv(v) < K) o[mt_cv(v)] = (double)vals[v];
        }
      }
    };

    if (pred != nullptr) {      // lowest index among equal margins: strict > in index order
      float best = acc[0];
      int bi = 4 * h;
#pragma unroll
      for (int v = 1; v < 16; ++v) {
        const bool up = acc[v] > best;
        best = up ? acc[v] : best;
        bi = up ? 4 * h + mt_cv(v) : bi;
      }
      const float ob = __shfl_xor(best, 32, 64);
      const int oi = __shfl_xor(bi, 32, 64);
      if (ob > best || (ob == best && oi < bi)) bi = oi;
      if (valid && h == 0) pred[row] = (double)bi;
    }
    if (need_exp) {
      float mx = -INFINITY;
#pragma unroll
      for (int v = 0; v < 16; ++v) mx = fmaxf(mx, acc[v]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      mt_f32x16 e;
      float se = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        e[v] = expf(acc[v] - mx);
        se += e[v];
      }
      se += __shfl_xor(se, 32, 64);
      if (raw != nullptr) {
        if (lsm) {
          const float ls = logf(se);
          mt_f32x16 t;
#pragma unroll
          for (int v = 0; v < 16; ++v) t[v] = (acc[v] - mx) - ls;
          emit(raw, t);
        } else {
          emit(raw, acc);
        }
      }
      if (prob != nullptr) {
#pragma unroll
        for (int v = 0; v < 16; ++v) e[v] = e[v] / se;
        emit(prob, e);
      }
    } else if (raw != nullptr) {
      emit(raw, acc);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xb[ks] = xn[ks];
  }
}

template <class SRC>
int lp_launch(const void* X, int64_t n, int64_t ldx, int nb, const void* Wsp, const float* bias_hi,
              const float* bias_lo, int K, int flags, double* raw, double* prob, double* pred, int64_t ldo,
              int grid, hipStream_t st) {
  const auto* Xe = (const typename SRC::elem*)X;
  const uint16_t* Wh = (const uint16_t*)Wsp;
  return mt_dispatch_nb(nb, [&](auto NB) {
    hipLaunchKernelGGL((linear_predict_kernel<SRC, NB>), dim3(grid), dim3(kLpThreads), 0, st, Xe, n, ldx, Wh, bias_hi,
                       bias_lo, K, flags, raw, prob, pred, ldo);
    O3S_CHECK_LAUNCH();
    return 0;
  });
}

constexpr int lp_lds_bytes(int nb) { return 2 * 3 * 32 * (32 * nb + 8) + 4 * kLpWaves * kLpStage + 4 * 64; }
static_assert(lp_lds_bytes(1) == LpLds<1>::BYTES && lp_lds_bytes(8) == LpLds<8>::BYTES, "LDS size");

}  // namespace

// LDS bytes of one block and the blocks a CU holds (the persistent grid's size per CU) for
// rows of d logical columns: what the LDS admits, capped by the waves per SIMD the
// instantiation is compiled for.  -1: d outside [1, 256].
O3S_API int o3s_linear_predict_layout(int is_f32, int d, int* lds_bytes, int* blocks_per_cu) {
  const int nb = (d + 31) / 32;
  if (d < 1 || nb > 8) return -1;
  // waves per SIMD by registers, from the compiler's resource report (doc/performance.md);
  // a block is one wave per SIMD.  Only the grid's size depends on it.
  static const int kByRegs[2][8] = {{4, 4, 4, 3, 3, 3, 2, 2}, {4, 3, 2, 2, 2, 1, 1, 1}};
  const int lds = lp_lds_bytes(nb);
  const int by_lds = kLpMaxLds / lds, by_regs = kByRegs[is_f32 ? 1 : 0][nb - 1];
  *lds_bytes = lds;
  *blocks_per_cu = by_lds < by_regs ? by_lds : by_regs;
  return 0;
}

// Y = X W^T + b over the n rows of X (bf16, or fp32 with is_f32; row stride ldx, ldx % 8 == 0;
// d logical columns, 1 <= d <= 256).  Wsp: bf16 [3][32][D], D = 32 ceil(d / 32) (hi, mid, lo
// splits of the output-major coefficients, zero-padded); bias_hi + bias_lo: fp32 [32] each;
// 1 <= K <= 32.  raw, prob: fp64 [n, ldo] (ldo >= K; a pointer into a wider matrix selects a
// column block), pred: fp64 [n]; null skips an output.  flags: LP_LOG_SOFTMAX_RAW (1),
// LP_DIRECT_STORE (2).  Returns 0, -1 for a bad argument, or the hipError of the launch.
O3S_API int o3s_linear_predict(const void* X, int is_f32, int64_t n, int64_t ldx, int d, const void* Wsp,
                               const float* bias_hi, const float* bias_lo, int K, int flags, double* raw,
                               double* prob, double* pred, int64_t ldo, int grid, hipStream_t st) {
  const int nb = (d + 31) / 32;
  if (n < 0 || ldx < 8 || ldx % 8 != 0 || d < 1 || nb > 8 || K < 1 || K > 32 || grid <= 0) return -1;
  if (!X || !Wsp || !bias_hi || !bias_lo || (flags & ~3)) return -1;
  if ((raw || prob) && ldo < K) return -1;
  if (n == 0 || (!raw && !prob && !pred)) return 0;
  // the staged store writes 16-B pairs from the matrix's first element
  if ((((uintptr_t)raw | (uintptr_t)prob) & 15) != 0) flags |= LP_DIRECT_STORE;
  return is_f32 ? lp_launch<LpF32>(X, n, ldx, nb, Wsp, bias_hi, bias_lo, K, flags, raw, prob, pred, ldo, grid, st)
                : lp_launch<LpBf16>(X, n, ldx, nb, Wsp, bias_hi, bias_lo, K, flags, raw, prob, pred, ldo, grid, st);
}

O3S_PRELOAD(linear_predict)

// Factorization machines (gfx950): one fused loss / gradient pass over bf16 rows
// (fm_pass_kernel) or over fp32 rows (fm_pass_f32_kernel), and the forward half alone
// (MARGIN = true) that writes the margin of every row.
//   q_f = sum_i v_if x_i,  s_i = sum_f v_if^2
//   m   = w0 + sum_i w_i x_i + 1/2 (sum_f q_f^2 - sum_i s_i x_i^2)
//   r, l = residual and loss of m (logistic or squared, loss_terms of glm_rows.h)
//   dV_if = sum_rows r q_f x_i - v_if t_i,  t_i = sum_rows r x_i^2
//   dw_i  = sum_rows r x_i,  dw0 = sum_rows r
// Reference: Spark's FMClassifier / FMRegressor gradient (BaseFactorizationMachinesGradient),
// reached from the classification and regression widgets.
//
// An FM pass is the multinomial pass of glm_softmax.hip with another epilogue, and the
// kernels keep that file's structure: 256 threads = 4 independent waves, 32-row tiles,
// v_mfma_f32_32x32x16_bf16 with lane (r = lane&31, h = lane>>5), the row's own global loads
// as the forward B operand, the next tile prefetched into a second register copy, per-wave
// slab rows summed in fp64 by glm_finish_kernel in a fixed order.  No float atomics, and the
// same bits for any grid: slab row v sums the tiles v, v + nslab, ..., one wave per slab row, and
// a grid with fewer waves than slab rows is launched as often as it takes (fm_launch).
//   forward  A = the hi + mid + lo bf16 split of the "classes" [V columns (F) | w], zero
//            padded to 32 -> acc[v] = q_f (class < F) or the linear term (class F) of row
//            r, class 8(v>>2) + 4h + (v&3).  sum_i s_i x_i^2 is an in-lane fp32 FMA over
//            the lane's 8 columns per k-step (s as floats in LDS), sum_f q_f^2 an in-lane
//            sum over the lane's accumulator registers; one __shfl_xor(.., 32) combines
//            the two halves of a row.
//   backward A = the residual matrix, two bf16 terms (hi + lo) through LDS: class f < F is
//            r q_f, class F is r, every other class 0.  B = X^T read transposed from LDS
//            -> G[class][dim].  t lands in row F + 1 of the same accumulators: a second A
//            fragment that is zero except in lane r == F + 1, where it holds r, multiplies
//            x^2, formed from the transposed fragment and split into two bf16 terms
//            (exact for bf16 rows: the square of 8 significant bits has 16).  Row F + 1 of
//            the plain residual matrix is zero, so X itself never reaches that row.
// A slab row: [G class-major 32 x D | sum r | 31 zeros | loss], pstride = 32 D + 33.
// Hence F <= 30.  No scratch in any instantiation at the one wave per SIMD the wide ones run
// at (the table is in doc/performance.md).
#include "glm_launch.h"

namespace {

typedef float fm_f32x16 __attribute__((ext_vector_type(16)));
typedef short fm_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t fm_u32x4 __attribute__((ext_vector_type(4)));
constexpr int kFmWaves = 4;
constexpr int kFmThreads = kFmWaves * kWave;

template <int NB, bool MARGIN>
struct FmLds {
  static constexpr int D = 32 * NB;
  static constexpr int WLD = D + 8;     // +16 B per row: conflict-free 16-B fragment reads
  static constexpr int XLD = D + 8;
  static constexpr int RLD = 40;        // 80-B rows: the 16-B R fragment reads hit distinct banks
  static constexpr int W_ELEMS = 3 * 32 * WLD;
  // per wave: the tile for the X^T reads, R hi + lo [2][32][RLD], and r hi + lo [2][RLD]
  static constexpr int WAVE_ELEMS = MARGIN ? 0 : 32 * XLD + 2 * 32 * RLD + 2 * RLD;
  static constexpr int ELEMS = W_ELEMS + kFmWaves * WAVE_ELEMS;
};

// register v of a lane's accumulator tile is class 4 h + fm_cv(v)
__device__ __forceinline__ constexpr int fm_cv(int v) { return 8 * (v >> 2) + (v & 3); }

// The margin of row r from its accumulators (q_f, linear term), sx = this lane's share of
// sum_i s_i x_i^2, and w0 = w0h + w0l.  Both halves of the row return the same bits.
__device__ __forceinline__ float fm_margin_of(const fm_f32x16& acc, float sx, int F, int h, float w0h, float w0l) {
  float qq = 0.f, lin = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int c = 4 * h + fm_cv(v);
    qq = c < F ? fmaf(acc[v], acc[v], qq) : qq;
    lin = c == F ? acc[v] : lin;
  }
  const float part = fmaf(0.5f, qq - sx, lin);
  return (part + __shfl_xor(part, 32, 64) + w0h) + w0l;
}

// The residual matrix of the tile -> LDS: class f < F is rr q_f, class F is rr, the rest 0,
// as hi + lo bf16 (Rw = Rs + 4 h RLD + r); rr itself as hi + lo for the x^2 product (Rq).
__device__ __forceinline__ void fm_store_r(const fm_f32x16& acc, float rr, int F, int h, int r, uint16_t* Rw,
                                           uint16_t* Rq, int RLD) {
#pragma unroll
  for (int v = 0; v < 16; v += 2) {
    float rv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = 4 * h + fm_cv(v + u);
      rv[u] = c < F ? rr * acc[v + u] : (c == F ? rr : 0.f);
    }
    const uint32_t ph = pk_bf16(rv[0], rv[1]);
    const uint32_t pl = pk_bf16(rv[0] - __uint_as_float(ph << 16), rv[1] - __uint_as_float(ph & 0xffff0000u));
    Rw[fm_cv(v) * RLD] = (uint16_t)ph;
    Rw[fm_cv(v + 1) * RLD] = (uint16_t)(ph >> 16);
    Rw[(32 + fm_cv(v)) * RLD] = (uint16_t)pl;
    Rw[(32 + fm_cv(v + 1)) * RLD] = (uint16_t)(pl >> 16);
  }
  if (h == 0) {
    const uint32_t ph = pk_bf16(rr, 0.f);
    const uint32_t pl = pk_bf16(rr - __uint_as_float(ph << 16), 0.f);
    Rq[r] = (uint16_t)ph;
    Rq[RLD + r] = (uint16_t)pl;
  }
}

// 8 squares -> two bf16 terms each (hi + lo of the fp32 product).
__device__ __forceinline__ void fm_square8(const float (&x)[8], fm_bf16x8& hi, fm_bf16x8& lo) {
  fm_u32x4 ph, pl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = x[2 * j] * x[2 * j], b = x[2 * j + 1] * x[2 * j + 1];
    ph[j] = pk_bf16(a, b);
    pl[j] = pk_bf16(a - __uint_as_float(ph[j] << 16), b - __uint_as_float(ph[j] & 0xffff0000u));
  }
  hi = __builtin_bit_cast(fm_bf16x8, ph);
  lo = __builtin_bit_cast(fm_bf16x8, pl);
}

// This wave's slab row: [G class-major 32 x D | sum r | 31 zeros | loss].
template <int NB>
__device__ __forceinline__ void fm_write_slab(const fm_f32x16 (&G)[NB], float racc, float lossacc, int r, int h,
                                              int lane, float* out) {
  constexpr int D = 32 * NB;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) out[(4 * h + fm_cv(v)) * D + b * 32 + r] = G[b][v];
  const float rt = wave_sum(racc), lt = wave_sum(lossacc);
  if (lane < 32) out[32 * D + lane] = lane == 0 ? rt : 0.f;
  if (lane == 0) out[32 * D + 32] = lt;
}

template <int NB, int LOSS, bool MARGIN = false>
__global__ __launch_bounds__(kFmThreads, 1) void fm_pass_kernel(
    const uint16_t* __restrict__ X, int64_t n, int64_t ldx, const float* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ sv,
    const float* __restrict__ w0p, int F, float* __restrict__ partial, int pstride, int nslab,
    int slab0, float* __restrict__ margin) {
  using L = FmLds<NB, MARGIN>;
  constexpr int D = L::D, KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  __shared__ __attribute__((aligned(16))) float ss[D];   // s_i, zero past d
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;
  uint16_t* Rs = Xs + 32 * XLD;
  uint16_t* Rq = Rs + 2 * 32 * RLD;

  // class splits [3][32][D] -> LDS (padded rows)
  for (int p = threadIdx.x; p < 3 * 32 * (D / 8); p += kFmThreads) {
    const int row = p / (D / 8), k8 = p % (D / 8);
    *reinterpret_cast<fm_bf16x8*>(Ws + row * WLD + k8 * 8) =
        *reinterpret_cast<const fm_bf16x8*>(Wsp + (int64_t)row * D + k8 * 8);
  }
  for (int p = threadIdx.x; p < D; p += kFmThreads) ss[p] = sv[p];
  const float w0h = w0p[0], w0l = w0p[1];
  __syncthreads();

  // Slab row v sums the tiles v, v + nslab, ... (nslab <= the number of tiles), and this wave
  // holds slab row slab0 + its index in the grid: how many blocks a launch has decides which
  // wave sums a slab row, not what the row holds.
  const int64_t ntiles = (n + 31) / 32;
  const int64_t step = nslab;
  const int slab = slab0 + blockIdx.x * kFmWaves + wid;
  if (slab >= nslab) return;   // the waves are independent from here on
  fm_f32x16 G[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) G[b][v] = 0.f;
  float racc = 0.f, lossacc = 0.f;
  int64_t tile = slab;
  fm_bf16x8 xb[KS], xn[KS];
  auto load = [&](int64_t t, fm_bf16x8 (&dst)[KS]) {
    int64_t row = t * 32 + r;
    row = row < n ? row : n - 1;
    const uint16_t* src = X + row * ldx;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int col = ks * 16 + 8 * h;
      if (col < ldx) {
        dst[ks] = *reinterpret_cast<const fm_bf16x8*>(src + col);
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
    // ---- forward: q_f and the linear term of row r, 16 classes per lane
    fm_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    float sx = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const fm_bf16x8 a = *reinterpret_cast<const fm_bf16x8*>(Ws + (s * 32 + r) * WLD + ks * 16 + 8 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[ks], acc, 0, 0, 0);
      }
      if (!MARGIN) *reinterpret_cast<fm_bf16x8*>(Xs + r * XLD + ks * 16 + 8 * h) = xb[ks];   // for the X^T reads
      const float4_ s0 = *reinterpret_cast<const float4_*>(ss + ks * 16 + 8 * h);
      const float4_ s1 = *reinterpret_cast<const float4_*>(ss + ks * 16 + 8 * h + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xv = bf16_to_f32((uint16_t)xb[ks][j]);
        sx = fmaf((j < 4 ? s0[j] : s1[j - 4]) * xv, xv, sx);
      }
    }
    const float m = fm_margin_of(acc, sx, F, h, w0h, w0l);
    if (MARGIN) {
      if (h == 0 && valid) margin[row] = m;
    } else {
      const float yv = valid ? y[row] : 0.f;
      const float wr = valid ? (sw ? sw[row] : 1.f) : 0.f;
      float rr, ll;
      loss_terms<LOSS>(m, yv, wr, rr, ll);
      if (h == 0) {
        racc += rr;
        lossacc += ll;
      }
      fm_store_r(acc, rr, F, h, r, Rs + 4 * h * RLD + r, Rq, RLD);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      // ---- backward: G[class][dim] += sum over the tile's rows of R[row][class] X[row][dim],
      // and row F + 1 += r x^2
      fm_bf16x8 ar[2][2], aq[2][2];
#pragma unroll
      for (int rs = 0; rs < 2; ++rs)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          ar[rs][s] = *reinterpret_cast<const fm_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
          const fm_bf16x8 t = *reinterpret_cast<const fm_bf16x8*>(Rq + s * RLD + rs * 16 + 8 * h);
          const fm_bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
          aq[rs][s] = r == F + 1 ? t : z;
        }
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int rs = 0; rs < 2; ++rs) {
          fm_bf16x8 bx, qh, ql;
          float xv[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            bx[q] = (short)Xs[(rs * 16 + 8 * h + q) * XLD + b * 32 + r];
            xv[q] = bf16_to_f32((uint16_t)bx[q]);
          }
          fm_square8(xv, qh, ql);
#pragma unroll
          for (int s = 0; s < 2; ++s) G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][s], bx, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[rs][1], ql, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[rs][0], ql, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[rs][1], qh, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[rs][0], qh, G[b], 0, 0, 0);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // tile's LDS reads done before it is overwritten
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xb[ks] = xn[ks];
  }
  if (!MARGIN) fm_write_slab<NB>(G, racc, lossacc, r, h, lane, partial + (int64_t)slab * pstride);
}

// ---------------------------------------------------------------------------------
// The pass over fp32 rows: the contract, layouts and slab rows of fm_pass_kernel for
// X = float [n, ldx].  As in glm_softmax_f32_kernel a row is split into bf16 terms as it is
// consumed: hi + mid + lo forward with the six products of order <= 2 (margins and loss at
// fp32 level), hi + mid backward, staged through LDS 16 rows (one MFMA k-step) at a time.
// sum_i s_i x_i^2 takes the fp32 values before the split.  x^2 for t is the fp32 square of
// hi + mid read back transposed, split into two bf16 terms.  The class of an accumulator
// register is recomputed from the lane id and the R fragments are read per 16-row step, to
// keep the NB = 8 instantiation out of scratch.
// 8 fp32 -> bf16 terms hi + mid + lo (split_bf16x3 of glm_rows.h, pair by pair).
__device__ __forceinline__ void fm_split8(const float4_ a, const float4_ b, fm_bf16x8& hi, fm_bf16x8& mid,
                                          fm_bf16x8& lo) {
  fm_u32x4 ph, pm, pl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x0 = j < 2 ? a[2 * j] : b[2 * j - 4], x1 = j < 2 ? a[2 * j + 1] : b[2 * j - 3];
    uint32_t h, m, l;
    split_bf16x3(x0, x1, h, m, l);
    ph[j] = h;
    pm[j] = m;
    pl[j] = l;
  }
  hi = __builtin_bit_cast(fm_bf16x8, ph);
  mid = __builtin_bit_cast(fm_bf16x8, pm);
  lo = __builtin_bit_cast(fm_bf16x8, pl);
}

template <int NB, int LOSS, bool MARGIN = false>
__global__ __launch_bounds__(kFmThreads, 1) void fm_pass_f32_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const float* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ sv,
    const float* __restrict__ w0p, int F, float* __restrict__ partial, int pstride, int nslab,
    int slab0, float* __restrict__ margin) {
  using L = FmLds<NB, MARGIN>;
  constexpr int D = L::D, KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  __shared__ __attribute__((aligned(16))) float ss[D];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;   // [hi, mid][16 rows][XLD]
  uint16_t* Rs = Xs + 32 * XLD;
  uint16_t* Rq = Rs + 2 * 32 * RLD;

  for (int p = threadIdx.x; p < 3 * 32 * (D / 8); p += kFmThreads) {
    const int row = p / (D / 8), k8 = p % (D / 8);
    *reinterpret_cast<fm_bf16x8*>(Ws + row * WLD + k8 * 8) =
        *reinterpret_cast<const fm_bf16x8*>(Wsp + (int64_t)row * D + k8 * 8);
  }
  for (int p = threadIdx.x; p < D; p += kFmThreads) ss[p] = sv[p];
  const float w0h = w0p[0], w0l = w0p[1];
  __syncthreads();

  // Slab row v sums the tiles v, v + nslab, ... (nslab <= the number of tiles), and this wave
  // holds slab row slab0 + its index in the grid: how many blocks a launch has decides which
  // wave sums a slab row, not what the row holds.
  const int64_t ntiles = (n + 31) / 32;
  const int64_t step = nslab;
  const int slab = slab0 + blockIdx.x * kFmWaves + wid;
  if (slab >= nslab) return;   // the waves are independent from here on
  fm_f32x16 G[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) G[b][v] = 0.f;
  float racc = 0.f, lossacc = 0.f;
  int64_t tile = slab;
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
    // ---- forward; the hi and mid terms of the row stay in the registers the fp32 values
    // came in, for the backward staging below
    fm_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    float sx = 0.f;
    fm_bf16x8 xh[KS], xm[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float4_ s0 = *reinterpret_cast<const float4_*>(ss + ks * 16 + 8 * h);
      const float4_ s1 = *reinterpret_cast<const float4_*>(ss + ks * 16 + 8 * h + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sx = fmaf(s0[j] * xf[ks][0][j], xf[ks][0][j], sx);
        sx = fmaf(s1[j] * xf[ks][1][j], xf[ks][1][j], sx);
      }
      fm_bf16x8 xl;
      fm_split8(xf[ks][0], xf[ks][1], xh[ks], xm[ks], xl);
      const uint16_t* wp = Ws + r * WLD + ks * 16 + 8 * h;
      const fm_bf16x8 a0 = *reinterpret_cast<const fm_bf16x8*>(wp);
      const fm_bf16x8 a1 = *reinterpret_cast<const fm_bf16x8*>(wp + 32 * WLD);
      const fm_bf16x8 a2 = *reinterpret_cast<const fm_bf16x8*>(wp + 64 * WLD);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, xh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xm[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xm[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xh[ks], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    const float m = fm_margin_of(acc, sx, F, h, w0h, w0l);
    if (MARGIN) {
      if (h == 0 && valid) margin[row] = m;
    } else {
      const float yv = valid ? y[row] : 0.f;
      const float wr = valid ? (sw ? sw[row] : 1.f) : 0.f;
      float rr, ll;
      loss_terms<LOSS>(m, yv, wr, rr, ll);
      if (h == 0) {
        racc += rr;
        lossacc += ll;
      }
      fm_store_r(acc, rr, F, h, r, Rs + 4 * h * RLD + r, Rq, RLD);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      // ---- backward, 16 rows (one MFMA k-step) at a time through this wave's staging area
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        if ((r >> 4) == rs) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            *reinterpret_cast<fm_bf16x8*>(Xs + (r & 15) * XLD + ks * 16 + 8 * h) = xh[ks];
            *reinterpret_cast<fm_bf16x8*>(Xs + (16 + (r & 15)) * XLD + ks * 16 + 8 * h) = xm[ks];
          }
        }
        fm_bf16x8 ar[2], aq[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          ar[s] = *reinterpret_cast<const fm_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
          const fm_bf16x8 t = *reinterpret_cast<const fm_bf16x8*>(Rq + s * RLD + rs * 16 + 8 * h);
          const fm_bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
          aq[s] = r == F + 1 ? t : z;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          fm_bf16x8 bh, bm, qh, ql;
          float xv[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            bh[q] = (short)Xs[(8 * h + q) * XLD + b * 32 + r];
            bm[q] = (short)Xs[(16 + 8 * h + q) * XLD + b * 32 + r];
            xv[q] = bf16_to_f32((uint16_t)bh[q]) + bf16_to_f32((uint16_t)bm[q]);
          }
          fm_square8(xv, qh, ql);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[1], bm, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[0], bm, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[1], bh, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[0], bh, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[1], ql, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[0], ql, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[1], qh, G[b], 0, 0, 0);
          G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[0], qh, G[b], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // staged reads done before the area is overwritten
        __builtin_amdgcn_wave_barrier();
      }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      xf[ks][0] = xn[ks][0];
      xf[ks][1] = xn[ks][1];
    }
  }
  if (!MARGIN) fm_write_slab<NB>(G, racc, lossacc, r, h, lane, partial + (int64_t)slab * pstride);
}

// The two kernel families, as the host pass below takes them: the rows' element type and the
// kernel for NB blocks of 32 dims.
struct FmBf16 {
  using elem = uint16_t;
  template <int NB, int LOSS, bool MARGIN> static auto kernel() { return fm_pass_kernel<NB, LOSS, MARGIN>; }
};
struct FmF32 {
  using elem = float;
  template <int NB, int LOSS, bool MARGIN> static auto kernel() { return fm_pass_f32_kernel<NB, LOSS, MARGIN>; }
};

bool fm_args_ok(int64_t n, int64_t ldx, int d, int F, int grid) {
  const int nb = (d + 31) / 32;
  return n >= 0 && ldx > 0 && ldx % 8 == 0 && d >= 1 && nb >= 1 && nb <= 8 && F >= 1 && F <= 30 && grid > 0;
}

template <class FAM, int LOSS, bool MARGIN>
int fm_launch(int nb, int grid, hipStream_t st, const typename FAM::elem* X, int64_t n, int64_t ldx, const float* y,
              const float* sw, const uint16_t* Wsp, const float* sv, const float* w0p, int F, float* partial,
              int pstride, int nslab, float* margin) {
  // launches of `grid` blocks until every slab row has had its wave
  for (int slab0 = 0; slab0 < nslab; slab0 += grid * kFmWaves) {
    const int left = (nslab - slab0 + kFmWaves - 1) / kFmWaves, g = grid < left ? grid : left;
    switch (nb) {
#define O3S_FM(NBV) \
  case NBV: hipLaunchKernelGGL((FAM::template kernel<NBV, LOSS, MARGIN>()), dim3(g), dim3(kFmThreads), 0, st, X, n, \
                               ldx, y, sw, Wsp, sv, w0p, F, partial, pstride, nslab, slab0, margin); break;
      O3S_FM(1) O3S_FM(2) O3S_FM(3) O3S_FM(4) O3S_FM(5) O3S_FM(6) O3S_FM(7) O3S_FM(8)
#undef O3S_FM
      default: return -1;
    }
    O3S_CHECK_LAUNCH();
  }
  return 0;
}

// What the two pass entry points share: the argument check, the launch of the family's kernel
// for nb = ceil(d / 32) (an empty pass zeroes the slab instead) and the fp64 finish over the
// slab rows.
template <class FAM>
int fm_pass(const void* X, int64_t n, int64_t ldx, int d, const float* y, const float* sw, const void* Wsp,
            const float* sv, const float* w0p, int F, int loss, float* partial, int slabs, int grid, double* out,
            hipStream_t st) {
  if (!fm_args_ok(n, ldx, d, F, grid) || slabs <= 0 || (loss != LOSS_LOGISTIC && loss != LOSS_SQUARED)) return -1;
  const int nb = (d + 31) / 32, D = 32 * nb, pstride = 32 * D + 33;
  const auto* Xe = (const typename FAM::elem*)X;
  const uint16_t* Wh = (const uint16_t*)Wsp;
  // every slab row holds a tile; an empty pass sums one zeroed row
  const int64_t ntiles = (n + 31) / 32;
  const int used = n > 0 ? (int)(ntiles < slabs ? ntiles : slabs) : 1;
  if (n > 0) {
    const int rc = loss == LOSS_LOGISTIC
        ? fm_launch<FAM, LOSS_LOGISTIC, false>(nb, grid, st, Xe, n, ldx, y, sw, Wh, sv, w0p, F, partial, pstride,
                                               used, nullptr)
        : fm_launch<FAM, LOSS_SQUARED, false>(nb, grid, st, Xe, n, ldx, y, sw, Wh, sv, w0p, F, partial, pstride,
                                              used, nullptr);
    if (rc != 0) return rc;
  } else {
    hipMemsetAsync(partial, 0, sizeof(float) * pstride, st);
  }
  return launch_finish(partial, used, pstride, pstride, out, 0, st);
}

template <class FAM>
int fm_margin(const void* X, int64_t n, int64_t ldx, int d, const void* Wsp, const float* sv, const float* w0p,
              int F, float* margin, int grid, hipStream_t st) {
  if (!fm_args_ok(n, ldx, d, F, grid)) return -1;
  if (n == 0) return 0;
  const int64_t ntiles = (n + 31) / 32;
  if (grid > (ntiles + kFmWaves - 1) / kFmWaves) grid = (int)((ntiles + kFmWaves - 1) / kFmWaves);
  const int walks = (int)(ntiles < (int64_t)grid * kFmWaves ? ntiles : (int64_t)grid * kFmWaves);
  return fm_launch<FAM, LOSS_SQUARED, true>((d + 31) / 32, grid, st, (const typename FAM::elem*)X, n, ldx, nullptr,
                                            nullptr, (const uint16_t*)Wsp, sv, w0p, F, nullptr, 0, walks, margin);
}

}  // namespace

// One FM pass: out (fp64, [32 * D | 32 | 1]) = (G class-major over D = 32 * ceil(d / 32) dims:
// rows f < F hold sum r q_f x, row F sum r x, row F + 1 sum r x^2; sum r in slot 32 D; the
// loss sum in slot 32 D + 32) over the n rows of X (bf16, row stride ldx, ldx % 8 == 0).
// y: fp32 labels; sw: fp32 weights or null; Wsp: bf16 [3][32][D] (hi, mid, lo splits of the
// class-major [V^T | w], zero-padded); sv: fp32 [D] (s_i = sum_f v_if^2, zero-padded); w0p:
// fp32 [2] (w0 as hi + lo); loss: 0 logistic, 2 squared.  partial: fp32 [slabs][32 D + 33]:
// with S = min(slabs, tiles), slab row v < S sums the tiles v, v + S, ..., so the result
// depends on slabs and not on the grid: a wave sums one slab row, and fewer than S / 4 blocks
// mean several launches.
O3S_API int o3s_fm_pass(const void* X, int64_t n, int64_t ldx, int d, const float* y, const float* sw,
                        const void* Wsp, const float* sv, const float* w0p, int F, int loss, float* partial,
                        int slabs, int grid, double* out, hipStream_t st) {
  return fm_pass<FmBf16>(X, n, ldx, d, y, sw, Wsp, sv, w0p, F, loss, partial, slabs, grid, out, st);
}

// o3s_fm_pass over fp32 rows: X = float [n, ldx] (ldx % 8 == 0).
O3S_API int o3s_fm_pass_f32(const void* X, int64_t n, int64_t ldx, int d, const float* y, const float* sw,
                            const void* Wsp, const float* sv, const float* w0p, int F, int loss, float* partial,
                            int slabs, int grid, double* out, hipStream_t st) {
  return fm_pass<FmF32>(X, n, ldx, d, y, sw, Wsp, sv, w0p, F, loss, partial, slabs, grid, out, st);
}

// The forward half alone: margin (fp32 [n]) of every row of X (bf16), operands as above.
O3S_API int o3s_fm_margin(const void* X, int64_t n, int64_t ldx, int d, const void* Wsp, const float* sv,
                          const float* w0p, int F, float* margin, int grid, hipStream_t st) {
  return fm_margin<FmBf16>(X, n, ldx, d, Wsp, sv, w0p, F, margin, grid, st);
}

// o3s_fm_margin over fp32 rows.
O3S_API int o3s_fm_margin_f32(const void* X, int64_t n, int64_t ldx, int d, const void* Wsp, const float* sv,
                              const float* w0p, int F, float* margin, int grid, hipStream_t st) {
  return fm_margin<FmF32>(X, n, ldx, d, Wsp, sv, w0p, F, margin, grid, st);
}

O3S_PRELOAD(fm)

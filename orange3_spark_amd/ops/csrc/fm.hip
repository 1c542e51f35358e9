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
// An FM pass is the multinomial pass of glm_softmax.hip with another epilogue, on the tile of
// mfma_tile.h: 256 threads = 4 independent waves, per-wave slab rows.  The same bits for any
// grid: slab row v sums the tiles v, v + nslab, ..., one wave per slab row, and a grid with fewer
// waves than slab rows is launched as often as it takes (fm_launch).
//   forward  A = the hi + mid + lo bf16 split of the "classes" [V columns (F) | w], zero
//            padded to 32 -> acc[v] = q_f (class < F) or the linear term (class F) of row
//            r, class 4h + mt_cv(v).  sum_i s_i x_i^2 is an in-lane fp32 FMA over
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
#include "mfma_tile.h"

namespace {

constexpr int kFmWaves = 4;
constexpr int kFmThreads = kFmWaves * kWave;

template <int NB, bool MARGIN>
struct FmLds : MtPitch<NB> {
  using P = MtPitch<NB>;
  static constexpr int W_ELEMS = 3 * 32 * P::WLD;
  // per wave: the tile for the X^T reads, R hi + lo [2][32][RLD], and r hi + lo [2][RLD]
  static constexpr int WAVE_ELEMS = MARGIN ? 0 : 32 * P::XLD + 2 * 32 * P::RLD + 2 * P::RLD;
  static constexpr int ELEMS = W_ELEMS + kFmWaves * WAVE_ELEMS;
};

// The margin of row r from its accumulators (q_f, linear term), sx = this lane's share of
// sum_i s_i x_i^2, and w0 = w0h + w0l.  Both halves of the row return the same bits.
__device__ __forceinline__ float fm_margin_of(const mt_f32x16& acc, float sx, int F, int h, float w0h, float w0l) {
  float qq = 0.f, lin = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int c = 4 * h + mt_cv(v);
    qq = c < F ? fmaf(acc[v], acc[v], qq) : qq;
    lin = c == F ? acc[v] : lin;
  }
  const float part = fmaf(0.5f, qq - sx, lin);
  return (part + __shfl_xor(part, 32, 64) + w0h) + w0l;
}

// The residual matrix of the tile -> LDS: class f < F is rr q_f, class F is rr, the rest 0,
// as hi + lo bf16 (Rw = Rs + 4 h RLD + r); rr itself as hi + lo for the x^2 product (Rq).
__device__ __forceinline__ void fm_store_r(const mt_f32x16& acc, float rr, int F, int h, int r, uint16_t* Rw,
                                           uint16_t* Rq, int RLD) {
#pragma unroll
  for (int v = 0; v < 16; v += 2) {
    float rv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = 4 * h + mt_cv(v + u);
      rv[u] = c < F ? rr * acc[v + u] : (c == F ? rr : 0.f);
    }
    mt_store_r_pair(Rw, v, rv[0], rv[1], RLD);
  }
  if (h == 0) {
    uint32_t ph, pl;
    split_bf16x2(rr, 0.f, ph, pl);
    Rq[r] = (uint16_t)ph;
    Rq[RLD + r] = (uint16_t)pl;
  }
}

// 8 squares -> two bf16 terms each (hi + lo of the fp32 product).
__device__ __forceinline__ void fm_square8(const float (&x)[8], mt_bf16x8& hi, mt_bf16x8& lo) {
  mt_u32x4 ph, pl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t h, l;
    split_bf16x2(x[2 * j] * x[2 * j], x[2 * j + 1] * x[2 * j + 1], h, l);
    ph[j] = h;
    pl[j] = l;
  }
  hi = __builtin_bit_cast(mt_bf16x8, ph);
  lo = __builtin_bit_cast(mt_bf16x8, pl);
}

// The R and r fragments of 16-row step rs: ar = R hi, lo; aq = r hi, lo in lane F + 1, else 0.
__device__ __forceinline__ void fm_read_r(const uint16_t* Rs, const uint16_t* Rq, int rs, int F, int r, int h, int RLD,
                                          mt_bf16x8 (&ar)[2], mt_bf16x8 (&aq)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    ar[s] = *reinterpret_cast<const mt_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
    const mt_bf16x8 t = *reinterpret_cast<const mt_bf16x8*>(Rq + s * RLD + rs * 16 + 8 * h);
    const mt_bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    aq[s] = r == F + 1 ? t : z;
  }
}

// The two tile steps.  forward: acc += [V^T | w] x and sx += sum_i s_i x_i^2 over the lane's
// columns of row r; backward: G += R^T X and row F + 1 += r x^2 over the tile's rows.
// bf16 rows: the tile goes to LDS as it is, once, and is read back transposed.
struct FmRowsBf16 : MtBf16 {
  template <int KS> struct terms {};
  template <int KS, bool MARGIN>
  __device__ static __forceinline__ void forward(const chunk (&xb)[KS], terms<KS>&, const uint16_t* Ws, const float* ss,
                                                 uint16_t* Xs, int r, int h, mt_f32x16& acc, float& sx) {
    constexpr int WLD = MtPitch<KS / 2>::WLD, XLD = MtPitch<KS / 2>::XLD;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint16_t* wp = Ws + r * WLD + ks * 16 + 8 * h;
      acc = mt_mfma3(acc, *reinterpret_cast<const mt_bf16x8*>(wp), *reinterpret_cast<const mt_bf16x8*>(wp + 32 * WLD),
                     *reinterpret_cast<const mt_bf16x8*>(wp + 64 * WLD), xb[ks]);
      if (!MARGIN) *reinterpret_cast<mt_bf16x8*>(Xs + r * XLD + ks * 16 + 8 * h) = xb[ks];   // for the X^T reads
      const float4_ s0 = *reinterpret_cast<const float4_*>(ss + ks * 16 + 8 * h);
      const float4_ s1 = *reinterpret_cast<const float4_*>(ss + ks * 16 + 8 * h + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xv = bf16_to_f32((uint16_t)xb[ks][j]);
        sx = fmaf((j < 4 ? s0[j] : s1[j - 4]) * xv, xv, sx);
      }
    }
  }
  template <int NB>
  __device__ static __forceinline__ void backward(const terms<2 * NB>&, uint16_t* Xs, const uint16_t* Rs,
                                                  const uint16_t* Rq, int F, int r, int h, mt_f32x16 (&G)[NB]) {
    constexpr int XLD = MtPitch<NB>::XLD, RLD = MtPitch<NB>::RLD;
    mt_bf16x8 ar[2][2], aq[2][2];
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) fm_read_r(Rs, Rq, rs, F, r, h, RLD, ar[rs], aq[rs]);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        const mt_bf16x8 bx = mt_read_xt(Xs, rs * 16 + 8 * h, b * 32 + r, XLD);
        mt_bf16x8 qh, ql;
        float xv[8];
        unpack8(bx, xv);
        fm_square8(xv, qh, ql);
#pragma unroll
        for (int s = 0; s < 2; ++s) G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][s], bx, G[b], 0, 0, 0);
        G[b] = mt_mfma4(G[b], aq[rs][0], aq[rs][1], qh, ql);
      }
    }
    mt_wave_sync();    // tile's LDS reads done before it is overwritten
  }
};
// fp32 rows.  As in glm_softmax_f32_kernel a row is split into bf16 terms as it is consumed:
// hi + mid + lo forward with the six products of order <= 2 (margins and loss at fp32 level),
// hi + mid backward, staged through LDS 16 rows (one MFMA k-step) at a time (Xs is
// [hi, mid][16 rows][XLD]).  sum_i s_i x_i^2 takes the fp32 values before the split.  x^2 for t
// is the fp32 square of hi + mid read back transposed, split into two bf16 terms.  The class of
// an accumulator register is recomputed from the lane id and the R fragments are read per 16-row
// step, to keep the NB = 8 instantiation out of scratch.
struct FmRowsF32 : MtF32 {
  template <int KS> struct terms { mt_bf16x8 xh[KS], xm[KS]; };   // stay in the registers the fp32 values came in
  template <int KS, bool MARGIN>
  __device__ static __forceinline__ void forward(const chunk (&xf)[KS], terms<KS>& t, const uint16_t* Ws,
                                                 const float* ss, uint16_t*, int r, int h, mt_f32x16& acc, float& sx) {
    constexpr int WLD = MtPitch<KS / 2>::WLD;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float4_ s0 = *reinterpret_cast<const float4_*>(ss + ks * 16 + 8 * h);
      const float4_ s1 = *reinterpret_cast<const float4_*>(ss + ks * 16 + 8 * h + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sx = fmaf(s0[j] * xf[ks].a[j], xf[ks].a[j], sx);
        sx = fmaf(s1[j] * xf[ks].b[j], xf[ks].b[j], sx);
      }
      mt_bf16x8 xl;
      mt_split8(xf[ks].a, xf[ks].b, t.xh[ks], t.xm[ks], xl);
      const uint16_t* wp = Ws + r * WLD + ks * 16 + 8 * h;
      acc = mt_mfma6(acc, *reinterpret_cast<const mt_bf16x8*>(wp), *reinterpret_cast<const mt_bf16x8*>(wp + 32 * WLD),
                     *reinterpret_cast<const mt_bf16x8*>(wp + 64 * WLD), t.xh[ks], t.xm[ks], xl);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  template <int NB>
  __device__ static __forceinline__ void backward(const terms<2 * NB>& t, uint16_t* Xs, const uint16_t* Rs,
                                                  const uint16_t* Rq, int F, int r, int h, mt_f32x16 (&G)[NB]) {
    constexpr int KS = 2 * NB, XLD = MtPitch<NB>::XLD, RLD = MtPitch<NB>::RLD;
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) {
      if ((r >> 4) == rs) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          *reinterpret_cast<mt_bf16x8*>(Xs + (r & 15) * XLD + ks * 16 + 8 * h) = t.xh[ks];
          *reinterpret_cast<mt_bf16x8*>(Xs + (16 + (r & 15)) * XLD + ks * 16 + 8 * h) = t.xm[ks];
        }
      }
      mt_bf16x8 ar[2], aq[2];
      fm_read_r(Rs, Rq, rs, F, r, h, RLD, ar, aq);
      mt_wave_sync();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        // (mt_read_xt of hi and mid, and their sum, element by element in one loop: read apart, hipcc
        // forms the sums with scalar adds in place of packed ones)
        mt_bf16x8 bh, bm, qh, ql;
        float xv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          bh[q] = (short)Xs[(8 * h + q) * XLD + b * 32 + r];
          bm[q] = (short)Xs[(16 + 8 * h + q) * XLD + b * 32 + r];
          xv[q] = bf16_to_f32((uint16_t)bh[q]) + bf16_to_f32((uint16_t)bm[q]);
        }
        fm_square8(xv, qh, ql);
        G[b] = mt_mfma4(G[b], ar[0], ar[1], bh, bm);
        G[b] = mt_mfma4(G[b], aq[0], aq[1], qh, ql);
        __builtin_amdgcn_sched_barrier(0);
      }
      mt_wave_sync();    // staged reads done before the area is overwritten
    }
  }
};

// What the two passes share: the prologue, the slab walk, the prefetch, everything between the
// forward and the backward products of a tile, and the slab row.
template <class SRC, int NB, int LOSS, bool MARGIN>
__device__ __forceinline__ void fm_body(const typename SRC::elem* __restrict__ X, int64_t n, int64_t ldx,
                                        const float* __restrict__ y, const float* __restrict__ sw,
                                        const uint16_t* __restrict__ Wsp, const float* __restrict__ sv,
                                        const float* __restrict__ w0p, int F, float* __restrict__ partial, int pstride,
                                        int nslab, int slab0, float* __restrict__ margin) {
  using L = FmLds<NB, MARGIN>;
  constexpr int D = L::D, KS = 2 * NB, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  __shared__ __attribute__((aligned(16))) float ss[D];   // s_i, zero past d
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;
  uint16_t* Rs = Xs + 32 * XLD;
  uint16_t* Rq = Rs + 2 * 32 * RLD;

  mt_stage_w<3 * 32, NB, kFmThreads>(Ws, Wsp);
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
  mt_f32x16 G[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) G[b][v] = 0.f;
  float racc = 0.f, lossacc = 0.f;
  int64_t tile = slab;
  typename SRC::chunk xc[KS], xn[KS];
  if (tile < ntiles) mt_load_tile<SRC, KS>(X, n, ldx, tile, r, h, xc);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) mt_load_tile<SRC, KS>(X, n, ldx, tile + step, r, h, xn);
    const int64_t row = tile * 32 + r;
    const bool valid = row < n;
    // ---- forward: q_f and the linear term of row r, 16 classes per lane
    mt_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    float sx = 0.f;
    typename SRC::template terms<KS> xt;
    SRC::template forward<KS, MARGIN>(xc, xt, Ws, ss, Xs, r, h, acc, sx);
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
      mt_wave_sync();
      SRC::template backward<NB>(xt, Xs, Rs, Rq, F, r, h, G);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xc[ks] = xn[ks];
  }
  if (!MARGIN) {
    // ---- this wave's slab row: [G class-major 32 x D | sum r | 31 zeros | loss]
    float* out = partial + (int64_t)slab * pstride;
    mt_write_slab_g<NB>(G, out, r, h);
    const float rt = wave_sum(racc), lt = wave_sum(lossacc);
    if (lane < 32) out[32 * D + lane] = lane == 0 ? rt : 0.f;
    if (lane == 0) out[32 * D + 32] = lt;
  }
}

template <int NB, int LOSS, bool MARGIN = false>
__global__ __launch_bounds__(kFmThreads, 1) void fm_pass_kernel(
    const uint16_t* __restrict__ X, int64_t n, int64_t ldx, const float* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ sv,
    const float* __restrict__ w0p, int F, float* __restrict__ partial, int pstride, int nslab,
    int slab0, float* __restrict__ margin) {
  fm_body<FmRowsBf16, NB, LOSS, MARGIN>(X, n, ldx, y, sw, Wsp, sv, w0p, F, partial, pstride, nslab, slab0, margin);
}

template <int NB, int LOSS, bool MARGIN = false>
__global__ __launch_bounds__(kFmThreads, 1) void fm_pass_f32_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const float* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ sv,
    const float* __restrict__ w0p, int F, float* __restrict__ partial, int pstride, int nslab,
    int slab0, float* __restrict__ margin) {
  fm_body<FmRowsF32, NB, LOSS, MARGIN>(X, n, ldx, y, sw, Wsp, sv, w0p, F, partial, pstride, nslab, slab0, margin);
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
  return mt_dispatch_nb(nb, [&](auto NB) {
    return mt_walk_slabs(nslab, grid, kFmWaves, [&](int g, int slab0) {
      hipLaunchKernelGGL((FAM::template kernel<NB, LOSS, MARGIN>()), dim3(g), dim3(kFmThreads), 0, st, X, n, ldx, y,
                         sw, Wsp, sv, w0p, F, partial, pstride, nslab, slab0, margin);
    });
  });
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

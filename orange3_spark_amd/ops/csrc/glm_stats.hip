// The GLM passes beside the gradient (gfx950), over bf16, lineage and fp32 rows: the summarizer
// pass fused with the first gradient (glm_stats_mixed_kernel, glm_stats_f32_kernel), margins
// for transform / predict, weighted column moments, and the kernel that materialises synthetic
// rows.  The row layout and the row sources are in glm_rows.h, the layout dispatch and the
// fp64 finish in glm_launch.h.
// stats_tile and the two stats kernels are register-tuned (see the note in
// glm_stats_mixed_kernel); the margin, column-moment and synth kernels are plain streaming
// loops.  Device code changes are checked with tools/isa_diff.py.
#include "glm_launch.h"

namespace {

// ---------------------------------------------------------------------------
// Summarizer pass of a gradient-descent fit, fused with its first gradient: per column
// s1 = sum w x, s2 = sum w x^2 and syx = sum w y x, per row sum w, sum w y, sum w y^2,
// over the resident rows of X and n_lin lineage rows in ONE interleaved launch (same
// tile schedule as glm_grad_mixed_kernel, glm_mixed.hip).  At the initial iterate every coefficient is
// zero, so each row's margin is the intercept b0 and the step-1 gradient of every loss
// is a combination of s1 and syx (logistic: sigmoid(b0) s1 - syx) -- the fit's first
// step needs no pass of its own (models/glm.py: DeviceSGD.first_step_from_stats).
// One tile of G * U rows from source SRC.  Lineage rows keep only the row's feature key
// and regenerate each chunk where it is used.
// UNW: a full tile (every row < n) of an unweighted fit -- w = 1 is folded away, which
// drops the w*x product from every element (the pass is VALU-bound on lineage tiles).
// FULL: every row of the tile is < n and every chunk of the layout is < nch: no clamps, no
// masks; a weighted FULL tile (UNW false) has a weight column (sw is not null).
template <class SRC, int LPR, int CPL, int U, bool UNW, bool FULL = false>
__device__ __forceinline__ void stats_tile(int64_t base, int64_t n, const typename SRC::elem* __restrict__ X,
                                           int64_t ld, int nch, const float* __restrict__ y,
                                           const float* __restrict__ sw, uint32_t seed, int64_t row0, int g, int c,
                                           float2_ (&s1)[CPL][4], float2_ (&s2)[CPL][4], float2_ (&syx)[CPL][4],
                                           float (&rsum)[3]) {
  constexpr int G = kWave / LPR;
  typename SRC::chunk xv[U][CPL];
  uint32_t fk[U];
  float yv[U], wv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t row = base + u * G + g;
    const bool ok = row < n;
    const int64_t rowc = FULL ? row : (ok ? row : n - 1);
    yv[u] = y[rowc];
    if (UNW) {
      wv[u] = 1.f;
    } else if constexpr (FULL) {
      wv[u] = sw[row];
    } else {
      const float w0 = sw ? sw[rowc] : 1.f;
      wv[u] = ok ? w0 : 0.f;
    }
    if constexpr (SRC::kLineage) {
      fk[u] = feat_key(seed, row0 + rowc);
    } else {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int ch = c + k * LPR;
        if constexpr (FULL) {
          SRC::load(X, ld, row, ch, xv[u][k]);
        } else {
          SRC::load(X, ld, rowc, ch < nch ? ch : nch - 1, xv[u][k]);
          SRC::mask(xv[u][k], ch < nch);
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float2_ w2 = {wv[u], wv[u]};
    const float wy = wv[u] * yv[u];
    const float2_ wy2 = {wy, wy};
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      float x[8];
      if constexpr (SRC::kLineage) {
        SRC::load(fk[u], c + k * LPR, xv[u][k]);
        SRC::values(xv[u][k], x);
      } else {
        SRC::unpack(xv[u][k], x);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float2_ xx = {x[2 * j], x[2 * j + 1]};
        const float2_ wx = UNW ? xx : w2 * xx;
        s1[k][j] += wx;
        s2[k][j] = __builtin_elementwise_fma(wx, xx, s2[k][j]);
        syx[k][j] = __builtin_elementwise_fma(wy2, xx, syx[k][j]);
      }
    }
    if (c == 0) {
      rsum[0] += wv[u];
      rsum[1] += wy;
      rsum[2] = fmaf(wy, yv[u], rsum[2]);
    }
  }
}
// Block epilogue of the stats passes: fold the G row groups of the wave, then the waves
// through LDS in a fixed order, into the slab row [s1 | s2 | syx (DP each) | row sums (3)].
template <int LPR, int CPL>
__device__ __forceinline__ void stats_epilogue(const float2_ (&s1)[CPL][4], const float2_ (&s2)[CPL][4],
                                               const float2_ (&syx)[CPL][4], const float (&rsum)[3],
                                               float* __restrict__ partial, int pstride, int lane, int wid, int c) {
  constexpr int DP = LPR * CPL * 8;
  __shared__ float red[kWavesPerBlock][3 * DP + 4];
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float a = s1[k][j][h], b = s2[k][j][h], e = syx[k][j][h];
#pragma unroll
        for (int off = LPR; off < kWave; off <<= 1) {
          a += __shfl_xor(a, off, kWave);
          b += __shfl_xor(b, off, kWave);
          e += __shfl_xor(e, off, kWave);
        }
        const int col = 8 * (c + k * LPR) + 2 * j + h;
        if (lane < LPR) {
          red[wid][col] = a;
          red[wid][DP + col] = b;
          red[wid][2 * DP + col] = e;
        }
      }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float v = wave_sum(rsum[q]);
    if (lane == 0) red[wid][3 * DP + q] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * DP + 3; i += kBlock) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < kWavesPerBlock; ++q) s += red[q][i];
    partial[(int64_t)blockIdx.x * pstride + i] = s;
  }
}

// FULL: 0 = any row counts (four tile bodies in the loop); 1 / 2 = n_res and n_lin are
// multiples of RT and ld is the layout's full width, an unweighted (1) or a weighted (2) pass:
// the loop holds that one pair of mask-free bodies.  y_lin / sw_lin: the lineage rows' labels.
template <int LPR, int CPL, int MW, int FULL = 0>
__global__ __launch_bounds__(kBlock, MW) void glm_stats_mixed_kernel(
    const uint16_t* __restrict__ X, int64_t ld, int64_t n_res, const float* __restrict__ y,
    const float* __restrict__ sw, const float* __restrict__ y_lin, const float* __restrict__ sw_lin, uint32_t seed,
    int64_t row0, int64_t n_lin, float* __restrict__ partial, int pstride) {
  constexpr int G = kWave / LPR;
  constexpr int U = CPL >= 8 ? 1 : 8 / CPL;
  constexpr int RT = G * U;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int g = lane / LPR, c = lane % LPR;
  const int nch = (int)(ld / 8);
  float2_ s1[CPL][4], s2[CPL][4], syx[CPL][4];
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) s1[k][j] = s2[k][j] = syx[k][j] = float2_{0.f, 0.f};
  float rsum[3] = {0.f, 0.f, 0.f};
  const int64_t Tr = (n_res + RT - 1) / RT, Tl = (n_lin + RT - 1) / RT, S = Tr + Tl;
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wid;
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  if (gw < S) {
    int64_t L = gw * Tl / S, rem = gw * Tl - L * S;
    const int64_t q0 = nw * Tl / S, r0 = nw * Tl - q0 * S;
    for (int64_t s = gw; s < S; s += nw) {
      // full tiles of an unweighted pass take the UNW body (chosen here and in
      // glm_stats_f32_kernel, and s1 / s2 / syx zeroed by a plain loop in both: either one in a
      // helper took glm_stats_mixed_kernel<8,4,2> from 184 to 256 VGPRs)
      if constexpr (FULL != 0) {
        if (rem + Tl >= S)
          stats_tile<RowsLineage, LPR, CPL, U, FULL == 1, true>(L * RT, n_lin, X, ld, nch, y_lin, sw_lin, seed, row0, g, c,
                                                               s1, s2, syx, rsum);
        else
          stats_tile<RowsBf16, LPR, CPL, U, FULL == 1, true>((s - L) * RT, n_res, X, ld, nch, y, sw, seed, row0, g, c, s1,
                                                            s2, syx, rsum);
      } else if (rem + Tl >= S) {
        const int64_t base = L * RT;
        if (sw == nullptr && base + RT <= n_lin)
          stats_tile<RowsLineage, LPR, CPL, U, true>(base, n_lin, X, ld, nch, y_lin, sw_lin, seed, row0, g, c, s1,
                                                     s2, syx, rsum);
        else
          stats_tile<RowsLineage, LPR, CPL, U, false>(base, n_lin, X, ld, nch, y_lin, sw_lin, seed, row0, g, c, s1,
                                                      s2, syx, rsum);
      } else {
        const int64_t base = (s - L) * RT;
        if (sw == nullptr && base + RT <= n_res)
          stats_tile<RowsBf16, LPR, CPL, U, true>(base, n_res, X, ld, nch, y, sw, seed, row0, g, c, s1, s2, syx, rsum);
        else
          stats_tile<RowsBf16, LPR, CPL, U, false>(base, n_res, X, ld, nch, y, sw, seed, row0, g, c, s1, s2, syx, rsum);
      }
      rem += r0;
      L += q0;
      if (rem >= S) { rem -= S; ++L; }
    }
  }
  stats_epilogue<LPR, CPL>(s1, s2, syx, rsum, partial, pstride, lane, wid, c);
}

// Materialise synthetic rows [row0, row0+n) into X (bf16) and labels y.
template <int LPR, int CPL>
__global__ __launch_bounds__(kBlock) void synth_glm_kernel(
    uint16_t* __restrict__ X, int64_t ld, int64_t n, float* __restrict__ y, uint32_t seed,
    int64_t row0, const float* __restrict__ wtrue, float btrue) {
  constexpr int G = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, c = lane % LPR;
  float wt[CPL][8];
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = 8 * (c + k * LPR) + j;
      wt[k][j] = col < ld ? wtrue[col] : 0.f;
    }
  const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t ntiles = (n + G - 1) / G;
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t row = t * G + g;
    const bool ok = row < n;
    const uint32_t rk = row_key(seed, row0 + row), fk = feat_key(seed, row0 + row);
    float dt = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int ch = c + k * LPR;
      if (8 * ch < ld) {
        short8 v = synth_chunk(fk, ch);
        float x[8];
        unpack8(v, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) dt = fmaf(x[j], wt[k][j], dt);
        if (ok) *reinterpret_cast<short8*>(X + row * ld + 8 * ch) = v;
      }
    }
    dt = group_sum<LPR>(dt);
    if (ok && c == 0) y[row] = synth_label(rk, dt + btrue);
  }
}

// margins[i] = x_i . coef + intercept (model.transform / predict path), U rows in flight
// per lane.
template <class SRC, int LPR, int CPL, int U>
__device__ __forceinline__ void margin_body(const typename SRC::elem* __restrict__ X, int64_t ld, int64_t n,
                                            const float* __restrict__ coef, float intercept,
                                            float* __restrict__ out) {
  constexpr int G = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, c = lane % LPR;
  const int nch = (int)(ld / 8);
  float w[CPL][8];
  load_coef<LPR, CPL>(coef, ld, c, w);
  const int64_t gw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) / kWave;
  const int64_t RT = (int64_t)G * U;
  const int64_t ntiles = (n + RT - 1) / RT;
  for (int64_t t = gw; t < ntiles; t += nw) {
    typename SRC::chunk xv[U][CPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = t * RT + u * G + g;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int ch = c + k * LPR;
        SRC::load_if(X, ld, row, ch, row < n && ch < nch, xv[u][k]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = t * RT + u * G + g;
      float d = 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        float x[8];
        SRC::unpack(xv[u][k], x);
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf(x[j], w[k][j], d);
      }
      d = group_sum<LPR>(d);
      if (row < n && c == 0) out[row] = d + intercept;
    }
  }
}
template <int LPR, int CPL>
__global__ __launch_bounds__(kBlock) void glm_margin_kernel(
    const uint16_t* __restrict__ X, int64_t ld, int64_t n, const float* __restrict__ coef,
    float intercept, float* __restrict__ out) {
  margin_body<RowsBf16, LPR, CPL, (CPL >= 8 ? 1 : 8 / CPL)>(X, ld, n, coef, intercept, out);
}

// Weighted column moments (Spark's MultivariateOnlineSummarizer subset used by the
// GLM solvers for standardization): per column sum(w*x), sum(w*x^2), plus sum(w).
// Same lane layout as the gradient pass; one slab row per block, fp64 finish.  Lineage
// rows go through their bf16 chunk (synth_chunk), as the materialised rows would.
template <class SRC, int LPR, int CPL>
__device__ __forceinline__ void colstats_body(const typename SRC::elem* __restrict__ X, int64_t ld, int64_t n,
                                              const float* __restrict__ sw, uint32_t seed, int64_t row0,
                                              float* __restrict__ partial, int pstride) {
  constexpr int G = kWave / LPR;
  constexpr int UNROLL = CPL >= 4 ? 1 : 4 / CPL;
  constexpr int DP = LPR * CPL * 8;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int g = lane / LPR, c = lane % LPR;
  const int nch = (int)(ld / 8);
  float s1[CPL][8], s2[CPL][8];
  zero(s1);
  zero(s2);
  float sw_acc = 0.f;
  const int64_t RT = (int64_t)G * UNROLL;
  const int64_t ntiles = (n + RT - 1) / RT;
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wid;
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t t = gw; t < ntiles; t += nw) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t row = t * RT + u * G + g;
      const bool ok = row < n;
      const int64_t rowc = ok ? row : n - 1;
      const float wv = sw ? sw[rowc] : 1.f;
      const float w = ok ? wv : 0.f;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int ch = c + k * LPR;
        const int chc = ch < nch ? ch : nch - 1;
        const float wk = ch < nch ? w : 0.f;        // the mask is on the weight, not on the chunk
        float x[8];
        if constexpr (SRC::kLineage) {
          unpack8(synth_chunk(feat_key(seed, row0 + rowc), chc), x);
        } else {
          typename SRC::chunk v;
          SRC::load(X, ld, rowc, chc, v);
          SRC::unpack(v, x);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float wx = wk * x[j];
          s1[k][j] += wx;
          s2[k][j] = fmaf(wx, x[j], s2[k][j]);
        }
      }
      if (c == 0) sw_acc += w;
    }
  }
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = s1[k][j], b = s2[k][j];
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1) {
        a += __shfl_xor(a, off, kWave);
        b += __shfl_xor(b, off, kWave);
      }
      s1[k][j] = a;
      s2[k][j] = b;
    }
  sw_acc = wave_sum(sw_acc);
  // waves add into one LDS row in turn (fixed order -> deterministic)
  __shared__ float red[2 * DP + 2];
  for (int q = 0; q < kWavesPerBlock; ++q) {
    if (wid == q) {
      if (lane < LPR) {
#pragma unroll
        for (int k = 0; k < CPL; ++k)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int i1 = 8 * (c + k * LPR) + j;
            red[i1] = (q == 0 ? 0.f : red[i1]) + s1[k][j];
            red[DP + i1] = (q == 0 ? 0.f : red[DP + i1]) + s2[k][j];
          }
      }
      if (lane == 0) red[2 * DP] = (q == 0 ? 0.f : red[2 * DP]) + sw_acc;
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < 2 * DP + 1; i += kBlock) partial[(int64_t)blockIdx.x * pstride + i] = red[i];
}
template <int LPR, int CPL, int SRC>
__global__ __launch_bounds__(kBlock) void glm_colstats_kernel(
    const uint16_t* __restrict__ X, int64_t ld, int64_t n, const float* __restrict__ sw,
    uint32_t seed, int64_t row0, float* __restrict__ partial, int pstride) {
  colstats_body<std::conditional_t<SRC == 0, RowsBf16, RowsLineage>, LPR, CPL>(X, ld, n, sw, seed, row0, partial,
                                                                               pstride);
}

// Summarizer + first-gradient pass (glm_stats_mixed_kernel, resident role), U rows per lane.
template <int LPR, int CPL, int U, int MW>
__global__ __launch_bounds__(kBlock, MW) void glm_stats_f32_kernel(
    const float* __restrict__ X, int64_t ld, int64_t n, const float* __restrict__ y, const float* __restrict__ sw,
    float* __restrict__ partial, int pstride) {
  constexpr int RT = kWave / LPR * U;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int g = lane / LPR, c = lane % LPR;
  const int nch = (int)(ld / 8);
  float2_ s1[CPL][4], s2[CPL][4], syx[CPL][4];
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) s1[k][j] = s2[k][j] = syx[k][j] = float2_{0.f, 0.f};
  float rsum[3] = {0.f, 0.f, 0.f};
  const int64_t ntiles = (n + RT - 1) / RT;
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wid;
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t base = t * RT;
    if (sw == nullptr && base + RT <= n)
      stats_tile<RowsF32, LPR, CPL, U, true>(base, n, X, ld, nch, y, sw, 0u, 0, g, c, s1, s2, syx, rsum);
    else
      stats_tile<RowsF32, LPR, CPL, U, false>(base, n, X, ld, nch, y, sw, 0u, 0, g, c, s1, s2, syx, rsum);
  }
  stats_epilogue<LPR, CPL>(s1, s2, syx, rsum, partial, pstride, lane, wid, c);
}

template <int LPR, int CPL>
__global__ __launch_bounds__(kBlock) void glm_margin_f32_kernel(
    const float* __restrict__ X, int64_t ld, int64_t n, const float* __restrict__ coef, float intercept,
    float* __restrict__ out) {
  margin_body<RowsF32, LPR, CPL, (CPL >= 4 ? 1 : 4 / CPL)>(X, ld, n, coef, intercept, out);
}

template <int LPR, int CPL>
__global__ __launch_bounds__(kBlock) void glm_colstats_f32_kernel(
    const float* __restrict__ X, int64_t ld, int64_t n, const float* __restrict__ sw, float* __restrict__ partial,
    int pstride) {
  colstats_body<RowsF32, LPR, CPL>(X, ld, n, sw, 0u, 0, partial, pstride);
}

}  // namespace

O3S_API int o3s_synth_glm(void* X, int64_t ld, int64_t n, float* y, uint32_t seed, int64_t row0,
                          const float* wtrue, float btrue, int grid, hipStream_t st) {
  Layout l;
  if (!resolve_layout(ld, &l)) return -1;
  if (n <= 0) return 0;
  return with_natural_layout(l, [&](auto L, auto C) {
    launch(synth_glm_kernel<L, C>, grid, st, (uint16_t*)X, ld, n, y, seed, row0,
           wtrue, btrue);
    O3S_CHECK_LAUNCH();
    return 0;
  });
}

O3S_API int o3s_glm_margin(const void* X, int64_t ld, int64_t n, const float* coef,
                           float intercept, float* out, int grid, hipStream_t st) {
  Layout l;
  if (!resolve_layout(ld, &l)) return -1;
  if (n <= 0) return 0;
  return with_natural_layout(l, [&](auto L, auto C) {
    launch(glm_margin_kernel<L, C>, grid, st, (const uint16_t*)X, ld, n, coef,
           intercept, out);
    O3S_CHECK_LAUNCH();
    return 0;
  });
}

// Column moments: out (fp64, 2*dpad+1) = [sum w x | sum w x^2 | sum w].  partial must hold
// grid * (2*dpad+2) floats.
O3S_API int o3s_glm_colstats(int src, const void* X, int64_t ld, int64_t n, const float* sw,
                             uint32_t seed, int64_t row0, float* partial, int grid, double* out,
                             hipStream_t st) {
  Layout l;
  if (!resolve_layout(ld, &l) || grid <= 0) return -1;
  const int pstride = 2 * l.dpad + 2;
  const uint16_t* Xh = (const uint16_t*)X;
  if (n > 0) {
    const int rc = with_natural_layout(l, [&](auto L, auto C) {
      if (src == 0) launch(glm_colstats_kernel<L, C, 0>, grid, st, Xh, ld, n, sw, seed, row0, partial, pstride);
      else launch(glm_colstats_kernel<L, C, 1>, grid, st, Xh, ld, n, sw, seed, row0, partial, pstride);
      return 0;
    });
    if (rc != 0) return rc;
  } else {
    hipMemsetAsync(partial, 0, sizeof(float) * pstride * (size_t)grid, st);
  }
  return launch_finish(partial, grid, pstride, 2 * l.dpad + 1, out, 0, st);
}

// Fused summarizer + first-gradient pass (glm_stats_mixed_kernel): out (fp64, 3*dpad+3) =
// [s1 | s2 | syx | sum w | sum w y | sum w y^2]; partial holds (grid + 1) * (3*dpad+4) floats.
// Returns -2 when the row layout has no stats instantiation (ld > 2048): the caller then
// uses o3s_glm_colstats plus a regular first pass.
// full_tiles: as in o3s_glm_grad_mixed (glm_mixed.hip) -- the whole tiles of both roles run through the
// mask-free kernel of the unweighted or of the weighted pass (sw == nullptr decides), the
// fewer than RT rows left of each role through one block of the masked kernel, which writes
// slab row `grid`; the finish then sums grid + 1 rows.
O3S_API int o3s_glm_stats_mixed(const void* X, int64_t ld, int64_t n_res, const float* y, const float* sw,
                                uint32_t seed, int64_t row0, int64_t n_lin, float* partial, int grid, double* out,
                                int waves, int full_tiles, hipStream_t st) {
  Layout l;
  if (!resolve_layout(ld, &l) || grid <= 0 || n_res < 0 || n_lin < 0) return -1;
  const int pstride = 3 * l.dpad + 4;
  const uint16_t* Xh = (const uint16_t*)X;
  int slab_rows = grid;
  const int rc = with_remapped_layout(l, [&](auto L, auto C) {
    if constexpr (C > 4) {
      return -2;
    } else {
      constexpr int64_t RT = (kWave / L) * (8 / C);
      // rows [r_lo, r_lo + r_n) of X and lineage rows [l_lo, l_lo + l_n), g blocks, into `slab`
      auto pass = [&](auto FULL, int g, float* slab, int64_t r_lo, int64_t r_n, int64_t l_lo, int64_t l_n) {
        // the mask-free kernels read whole tiles (and the weighted one sw) unguarded
        if (FULL != 0 && (r_n % RT != 0 || l_n % RT != 0 || ld != 8 * L * C || (FULL == 2) != (sw != nullptr)))
          return -1;
        auto go = [&](auto MW) {
          launch(glm_stats_mixed_kernel<L, C, MW, FULL>, g, st, Xh + r_lo * ld, ld, r_n, y + r_lo,
                 sw ? sw + r_lo : nullptr, y + n_res + l_lo, sw ? sw + n_res + l_lo : nullptr, seed, row0 + l_lo, l_n,
                 slab, pstride);
        };
        // (a mask-free kernel fits 3 waves/SIMD without a spill under either bound)
        if constexpr (FULL == 0) {
          if (waves == 3) go(IC<3>{});
          else go(IC<2>{});
        } else {
          go(IC<2>{});
        }
        return 0;
      };
      // (64x4: one wave/SIMD either way, and the weighted mask-free kernel needs more registers)
      if constexpr (L < 64) {
        const int64_t r_full = n_res / RT * RT, l_full = n_lin / RT * RT;
        if (full_tiles && ld == 8 * L * C && r_full + l_full > 0) {
          const int rc = sw ? pass(IC<2>{}, grid, partial, 0, r_full, 0, l_full)
                            : pass(IC<1>{}, grid, partial, 0, r_full, 0, l_full);
          if (rc != 0 || (r_full == n_res && l_full == n_lin)) return rc;
          O3S_CHECK_LAUNCH();
          slab_rows = grid + 1;
          return pass(IC<0>{}, 1, partial + (size_t)grid * pstride, r_full, n_res - r_full, l_full, n_lin - l_full);
        }
      }
      return pass(IC<0>{}, grid, partial, 0, n_res, 0, n_lin);
    }
  });
  if (rc != 0) return rc;
  return launch_finish(partial, slab_rows, pstride, 3 * l.dpad + 3, out, 0, st);
}

// Fused summarizer + first-gradient pass over fp32 rows: the out / partial contract of
// o3s_glm_stats_mixed, -2 for the layouts that one has no instantiation for (ld > 2048).
O3S_API int o3s_glm_stats_f32(const void* X, int64_t ld, int64_t n, const float* y, const float* sw, int64_t n_lin,
                              float* partial, int grid, double* out, hipStream_t st) {
  Layout l;
  if (ld <= 0 || !resolve_layout(ld, &l) || grid <= 0 || n < 0 || n_lin != 0) return -1;
  const int pstride = 3 * l.dpad + 4;
  const int rc = with_remapped_layout(l, [&](auto L, auto C) {
    if constexpr (C > 4) {
      return -2;
    } else {
      launch(glm_stats_f32_kernel<L, C, (C >= 4 ? 1 : 4 / C), 2>, grid, st, (const float*)X, ld, n, y, sw, partial,
             pstride);
      return 0;
    }
  });
  if (rc != 0) return rc;
  return launch_finish(partial, grid, pstride, 3 * l.dpad + 3, out, 0, st);
}

O3S_API int o3s_glm_margin_f32(const void* X, int64_t ld, int64_t n, const float* coef, float intercept, float* out,
                               int grid, hipStream_t st) {
  Layout l;
  if (ld <= 0 || !resolve_layout(ld, &l) || grid <= 0) return -1;
  if (n <= 0) return 0;
  return with_remapped_layout(l, [&](auto L, auto C) {
    launch(glm_margin_f32_kernel<L, C>, grid, st, (const float*)X, ld, n, coef,
           intercept, out);
    O3S_CHECK_LAUNCH();
    return 0;
  });
}

// Column moments over fp32 rows: the out / partial contract of o3s_glm_colstats.
O3S_API int o3s_glm_colstats_f32(const void* X, int64_t ld, int64_t n, const float* sw, float* partial, int grid,
                                 double* out, hipStream_t st) {
  Layout l;
  if (ld <= 0 || !resolve_layout(ld, &l) || grid <= 0 || n < 0) return -1;
  const int pstride = 2 * l.dpad + 2;
  if (n > 0) {
    const int rc = with_remapped_layout(l, [&](auto L, auto C) {
      launch(glm_colstats_f32_kernel<L, C>, grid, st, (const float*)X, ld, n, sw,
             partial, pstride);
      return 0;
    });
    if (rc != 0) return rc;
  } else {
    hipMemsetAsync(partial, 0, sizeof(float) * pstride * (size_t)grid, st);
  }
  return launch_finish(partial, grid, pstride, 2 * l.dpad + 1, out, 0, st);
}

O3S_PRELOAD(glm_stats)

// The legacy GLM gradient pass with one row source per launch (gfx950; glm_grad_kernel, bf16 or
// lineage rows) and the two device-side SGD update kernels.  The row layout, the row sources
// and the block epilogue are in glm_rows.h, the layout dispatch and the fp64 finish in
// glm_launch.h; the mixed resident + lineage pass and the fp32-row pass are in glm_mixed.hip.
// glm_grad_kernel is register-tuned: move statements in it only with tools/isa_diff.py at
// hand.  The update kernels and the entry points are plain code.
#include "glm_launch.h"

namespace {

// The legacy gradient pass (L-BFGS and the two-stream overlap path): one source per launch,
// SRC == 1 draws the lineage rows' labels in-kernel from the ground truth wtrue / btrue.
template <int LPR, int CPL, int UNROLL, int LOSS, int SRC>
__global__ __launch_bounds__(kBlock) void glm_grad_kernel(
    const uint16_t* __restrict__ X, int64_t ld, int64_t n, const float* __restrict__ y,
    const float* __restrict__ sw, const float* __restrict__ coef, const float* __restrict__ bptr,
    uint32_t seed, int64_t row0, const float* __restrict__ wtrue, float btrue,
    float* __restrict__ partial, int pstride) {
  constexpr int G = kWave / LPR;             // rows per wave-instruction
  constexpr int RT = G * UNROLL;             // rows per wave tile
  using RR = RowReduce<LPR, UNROLL>;
  constexpr int NF = RR::NF;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int g = lane / LPR, c = lane % LPR;
  const int nch = (int)(ld / 8);
  const int ubase = RR::base(c);
  const bool rep = RR::representative(c);
  // read from device memory so a device-side optimizer step never syncs the host
  const float intercept = *bptr;

  // SRC == 1 works on raw bytes b (x = b*kSynthScale + kSynthShift): the weights are
  // pre-scaled by kSynthScale and each lane's dot products start from the shift term
  // kSynthShift * sum(w over its columns); X^T r accumulates r*b/128 plus a per-lane
  // residual sum rs, corrected once at the end.
  // (its own coefficient loop, not load_coef: it scales w and loads wtrue alongside)
  float w[CPL][8], wt[CPL][8], acc[CPL][8];
  float wshift = 0.f, wtshift = 0.f, rs = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = 8 * (c + k * LPR) + j;
      const float wv = col < ld ? coef[col] : 0.f;
      const float wtv = (SRC == 1 && col < ld) ? wtrue[col] : 0.f;
      w[k][j] = SRC == 1 ? wv * kSynthScale : wv;
      wt[k][j] = wtv * kSynthScale;
      wshift += wv;
      wtshift += wtv;
      acc[k][j] = 0.f;
    }
  wshift *= kSynthShift;
  wtshift *= kSynthShift;
  float acc_r = 0.f, acc_loss = 0.f, acc_w = 0.f;

  const int64_t ntiles = (n + RT - 1) / RT;
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wid;
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t base = t * RT;
    // Loads are issued unconditionally from clamped addresses and masked in
    // registers afterwards: a per-load `ok ? load : 0` makes hipcc branch around
    // every load and serialise them (CDNA guide §5, "three .s-level traps" (c)).
    // SRC == 1: rows past n are harmless (their residual is masked to 0) and columns
    // past ld meet zero weights and are never written out, so no masking is needed.
    short8 xv[UNROLL][CPL];
    float xf[UNROLL][CPL][8];          // SRC == 1: decoded once, reused by dot and X^T r
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t row = base + u * G + g;
      const bool ok = row < n;
      const int64_t rowc = ok ? row : n - 1;
      const uint32_t rk = SRC == 1 ? feat_key(seed, row0 + row) : 0u;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int ch = c + k * LPR;
        if (SRC == 0) {
          const bool okc = ok && ch < nch;
          const int chc = ch < nch ? ch : nch - 1;
          short8 v = __builtin_nontemporal_load(reinterpret_cast<const short8*>(X + rowc * ld + 8 * chc));
          xv[u][k] = okc ? v : short8{0, 0, 0, 0, 0, 0, 0, 0};
        } else {
          const uint32_t h0 = synth_word(rk, 2 * ch), h1 = synth_word(rk, 2 * ch + 1);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            xf[u][k][j] = synth_byte(h0, j);
            xf[u][k][4 + j] = synth_byte(h1, j);
          }
        }
      }
    }
    // labels / weights of the rows this lane finishes
    float yy[NF], ww[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int64_t row = base + (ubase + j) * G + g;
      const bool ok = row < n;
      const int64_t rowc = ok ? row : n - 1;
      if (SRC == 0) {
        const float yv = y[rowc];
        const float wv = sw ? sw[rowc] : 1.f;
        yy[j] = ok ? yv : 0.f;
        ww[j] = ok ? wv : 0.f;
      } else {
        ww[j] = ok ? 1.f : 0.f;
      }
    }
    float dot[UNROLL], dtrue[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float d = SRC == 1 ? wshift : 0.f, dt = wtshift;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        float x[8];
        if (SRC == 0) {
          unpack8(xv[u][k], x);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = xf[u][k][j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          d = fmaf(x[j], w[k][j], d);
          if (SRC == 1) dt = fmaf(x[j], wt[k][j], dt);
        }
      }
      dot[u] = d;
      dtrue[u] = dt;
    }
    RR::run(dot, c);
    if (SRC == 1) {
      RR::run(dtrue, c);
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        const int64_t row = base + (ubase + j) * G + g;
        yy[j] = synth_label(row_key(seed, row0 + row), dtrue[j] + btrue);
      }
    }
    float res[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      float r, l;
      loss_terms<LOSS>(dot[j] + intercept, yy[j], ww[j], r, l);
      res[j] = r;
      if (rep) { acc_r += r; acc_loss += l; acc_w += ww[j]; }
    }
    // Re-unpack from the packed registers for X^T r instead of keeping 8*UNROLL*CPL
    // unpacked floats live across the reduction (halves the VGPR footprint).
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        if (SRC == 0) asm volatile("" : "+v"(xv[u][k]));
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(xf[u][k][j]));
        }
      }
    // broadcast each row's residual back to its LPR lanes, accumulate X^T r
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float r = __shfl(res[u % NF], g * LPR + RR::owner(u), kWave);
      if (SRC == 1) { rs += r; r *= kSynthScale; }
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        float x[8];
        if (SRC == 0) {
          unpack8(xv[u][k], x);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = xf[u][k][j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(r, x[j], acc[k][j]);
      }
    }
  }

  if (SRC == 1) {
#pragma unroll
    for (int k = 0; k < CPL; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(rs, kSynthShift, acc[k][j]);
  }
  grad_epilogue<LPR, CPL>(acc, acc_r, acc_loss, acc_w, partial, pstride, 0, lane, wid, c);
}

// One device-side gradient-descent step on the all-reduced pass result `out`
// (DeviceSGD): standardised coefficients bt <- bt - eta*(g/W + l2*bt), intercept
// b <- b - eta * sum(r)/W, then refresh the fp32 kernel operand coef_eff (dpad
// coefficients + intercept) and record the loss -- no host round trip per step.
__global__ __launch_bounds__(256) void glm_sgd_update_kernel(
    const double* __restrict__ out, int dpad, double* __restrict__ bt, double* __restrict__ b,
    const double* __restrict__ inv_std, const double* __restrict__ l2v, double l2, double eta,
    int fit_intercept, float* __restrict__ coef_eff, double* __restrict__ loss_slot) {
  const double W = out[dpad + 2];
  const double invW = W > 0.0 ? 1.0 / W : 0.0;
  for (int i = threadIdx.x; i < dpad; i += blockDim.x) {
    const double inv = inv_std[i];
    const double reg = l2v ? l2v[i] : l2;
    const double v = bt[i] - eta * (out[i] * inv * invW + reg * bt[i]);
    bt[i] = v;
    coef_eff[i] = (float)(v * inv);
  }
  if (threadIdx.x == 0) {
    double bv = b[0];
    if (fit_intercept) bv -= eta * out[dpad] * invW;
    b[0] = bv;
    coef_eff[dpad] = (float)bv;
    if (loss_slot) loss_slot[0] = out[dpad + 1] * invW;
  }
}

// Graph-capturable variant: the step counter lives on the device (t <- t + 1, eta =
// step_size / sqrt(t), loss recorded at loss_hist[t - 1] while t <= cap), so a captured
// step has no per-step host arguments and can be replayed from a HIP graph.  An L1 term
// (elastic net / mllib L1Updater) is applied as the proximal soft-threshold
// bt <- sign(bt) max(|bt| - eta * l1, 0) after the gradient step.
__global__ __launch_bounds__(256) void glm_sgd_update_dev_kernel(
    const double* __restrict__ out, int dpad, double* __restrict__ bt, double* __restrict__ b,
    const double* __restrict__ inv_std, const double* __restrict__ l2v, double l2, const double* __restrict__ l1v,
    double l1, double step_size, int fit_intercept, float* __restrict__ coef_eff, double* __restrict__ loss_hist,
    int64_t cap, int64_t* __restrict__ t_dev) {
  const int64_t t = t_dev[0] + 1;
  const double eta = step_size / sqrt((double)t);
  const double W = out[dpad + 2];
  const double invW = W > 0.0 ? 1.0 / W : 0.0;
  const bool prox = l1v != nullptr || l1 > 0.0;
  for (int i = threadIdx.x; i < dpad; i += blockDim.x) {
    const double inv = inv_std[i];
    const double reg = l2v ? l2v[i] : l2;
    double v = bt[i] - eta * (out[i] * inv * invW + reg * bt[i]);
    if (prox) {
      const double sh = eta * (l1v ? l1v[i] : l1);
      v = v > sh ? v - sh : (v < -sh ? v + sh : 0.0);
    }
    bt[i] = v;
    coef_eff[i] = (float)(v * inv);
  }
  __syncthreads();                       // every lane has read t_dev before it moves
  if (threadIdx.x == 0) {
    double bv = b[0];
    if (fit_intercept) bv -= eta * out[dpad] * invW;
    b[0] = bv;
    coef_eff[dpad] = (float)bv;
    if (t <= cap) loss_hist[t - 1] = out[dpad + 1] * invW;
    t_dev[0] = t;
  }
}

}  // namespace

// Number of fp32 slots per partial-slab row and the padded width for `ld`.
O3S_API int o3s_glm_layout(int64_t ld, int* dpad, int* pstride) {
  Layout l;
  if (!resolve_layout(ld, &l)) return -1;
  *dpad = l.dpad;
  *pstride = l.dpad + 4;
  return 0;
}

// Gradient/loss pass.  out (fp64, dpad+3): [grad (dpad) | sum r | loss | weight sum],
// overwritten (accumulate == 0) or added to.  coef holds dpad+1 floats: the padded
// coefficients followed by the intercept.  partial must hold grid * pstride floats.
// src: 0 = X in memory, 1 = synthetic lineage.
O3S_API int o3s_glm_grad(int loss, int src, const void* X, int64_t ld, int64_t n, const float* y,
                         const float* sw, const float* coef, uint32_t seed,
                         int64_t row0, const float* wtrue, float btrue, float* partial,
                         int grid, double* out, int accumulate, hipStream_t st) {
  Layout l;
  if (!resolve_layout(ld, &l) || grid <= 0) return -1;
  const int pstride = l.dpad + 4;
  const uint16_t* Xh = (const uint16_t*)X;
  if (n > 0) {
    const int rc = with_loss(loss, [&](auto LOSS) {
      // rows in flight per lane: 8 loads for the streaming pass; the lineage pass keeps
      // fewer chunks live (its hash work, not memory latency, is the limiter)
      if (src == 0)
        return with_natural_layout(l, [&](auto L, auto C) {
          constexpr int U = C == 1 ? 8 : (C == 2 ? 2 : 1);
          launch(glm_grad_kernel<L, C, U, LOSS, 0>, grid, st, Xh, ld, n, y, sw, coef, coef + l.dpad, seed, row0,
                 wtrue, btrue, partial, pstride);
          return 0;
        });
      return with_remapped_layout(l, [&](auto L, auto C) {
        constexpr int U = C >= 8 ? 1 : 8 / C;
        launch(glm_grad_kernel<L, C, U, LOSS, 1>, grid, st, Xh, ld, n, y, sw, coef, coef + l.dpad, seed, row0,
               wtrue, btrue, partial, pstride);
        return 0;
      });
    });
    if (rc != 0) return rc;
  } else {
    if (accumulate) return 0;
    hipMemsetAsync(partial, 0, sizeof(float) * pstride * (size_t)grid, st);
  }
  return launch_finish(partial, grid, pstride, l.dpad + 3, out, accumulate, st);
}

O3S_API int o3s_glm_sgd_update(const double* out, int dpad, double* bt, double* b, const double* inv_std,
                               const double* l2v, double l2, double eta, int fit_intercept, float* coef_eff,
                               double* loss_slot, hipStream_t st) {
  hipLaunchKernelGGL(glm_sgd_update_kernel, dim3(1), dim3(256), 0, st, out, dpad, bt, b, inv_std, l2v, l2,
                     eta, fit_intercept, coef_eff, loss_slot);
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_API int o3s_glm_sgd_update_dev(const double* out, int dpad, double* bt, double* b, const double* inv_std,
                                   const double* l2v, double l2, const double* l1v, double l1, double step_size,
                                   int fit_intercept, float* coef_eff, double* loss_hist, int64_t cap,
                                   int64_t* t_dev, hipStream_t st) {
  hipLaunchKernelGGL(glm_sgd_update_dev_kernel, dim3(1), dim3(256), 0, st, out, dpad, bt, b, inv_std, l2v, l2,
                     l1v, l1, step_size, fit_intercept, coef_eff, loss_hist, cap, t_dev);
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_PRELOAD(glm_grad)

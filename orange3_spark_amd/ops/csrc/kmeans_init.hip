// k-means|| seeding, step 2 (Spark LocalKMeans.kMeansPlusPlus on the weighted candidates):
// greedy k-means++ -- per step, `trials` weighted draws from w * d2 (inverse CDF over a
// prefix sum), each draw's potential sum_i w_i min(d2_i, |p_i - c|^2), the best one kept.
// Distances by the |p|^2 + |c|^2 - 2 p.c form of the torch reference
// (models/kmeans._local_kmeanspp) over fp32-rounded coordinates, products and sums in fp64;
// draws from the same counter-hash uniforms U [k][trials + 1].
//
// Two launches per step, spread over the GPU: kpp_dist_kernel (one row per thread, every
// candidate row of the chip at once: the trials' distances cd [trials][m] and per-block
// partial potentials) and kpp_pick_kernel (one block: the potentials summed over the blocks
// in a fixed order, the pick, d2 = min(d2, cd[best]), the prefix sum of w * d2 in LDS and
// the next step's draws).  The host loop in o3s_kmeanspp enqueues all 2k launches.  (A
// single workgroup running all k steps spent 0.17 s of a 0.33 s k-means|| init at k = 1024,
// m = 4097 -- 94% of it in the fp64 distance sums one CU can issue:
// profiles/kmeans_init_phases_r5.json.)
// Plain fp64 code, nothing register-tuned; the Lloyd kernels are in kmeans_assign.hip and
// kmeans_update.hip.
#include "common.h"

using namespace o3s;

namespace {
constexpr int kPPThreads = 512;             // kpp_pick_kernel
constexpr int kPDThreads = 256;             // kpp_dist_kernel
constexpr int kPPMaxT = 16;

__device__ double pp_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  return t;
}

// first index i with cs[i] > u * tot (searchsorted right), clamped; tot <= 0: uniform
__device__ int pp_draw(const double* cs, int m, double tot, double u) {
  if (!(tot > 0.0)) {
    const long long r = (long long)(u * m);
    return (int)(r < m - 1 ? r : m - 1);
  }
  const double x = u * tot;
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cs[mid] > x) hi = mid; else lo = mid + 1;
  }
  return lo < m - 1 ? lo : m - 1;
}

// mode 0: d2[i] = |p_i - p_cand[0]|^2 (the first centre); mode 1: cd[j][i] = distance of
// row i to trial candidate j and partial[block][j] = sum over the block's rows of
// w_i min(d2_i, cd[j][i]).  PT: fp32 [D][m]; pn: |p|^2 of the rounded rows (fp64).
__device__ void kpp_dist(const float* __restrict__ PT, const double* __restrict__ w, const double* __restrict__ pn,
                         int m, int D, int trials, const int* __restrict__ cand, int mode, double* __restrict__ d2,
                         double* __restrict__ cd, double* __restrict__ partial, int blk, double* sc, double* red) {
  // sc: [trials][D] candidate coordinates (LDS); red: [kPDThreads / 64]
  const int nt = mode == 0 ? 1 : trials;
  for (int e = threadIdx.x; e < nt * D; e += kPDThreads) {
    const int j = e / D, d = e - j * D;
    sc[e] = (double)PT[(int64_t)d * m + cand[j]];
  }
  __syncthreads();
  const int i = blk * kPDThreads + threadIdx.x;
  const bool ok = i < m;
  const int ic = ok ? i : m - 1;
  // 8 coordinates per round, loaded before use (one L2 round trip per 8 instead of per 1)
  constexpr int UD = 8;
  if (mode == 0) {
    double s = 0.0;
    for (int d0 = 0; d0 < D; d0 += UD) {
      float x[UD];
#pragma unroll
      for (int u = 0; u < UD; ++u) x[u] = d0 + u < D ? PT[(int64_t)(d0 + u) * m + ic] : 0.f;
#pragma unroll
      for (int u = 0; u < UD; ++u)
        if (d0 + u < D) {
          const double t = (double)x[u] - sc[d0 + u];
          s = fma(t, t, s);
        }
    }
    if (ok) d2[i] = s;
    return;
  }
  double dot[kPPMaxT];
#pragma unroll
  for (int j = 0; j < kPPMaxT; ++j) dot[j] = 0.0;
  for (int d0 = 0; d0 < D; d0 += UD) {
    float x[UD];
#pragma unroll
    for (int u = 0; u < UD; ++u) x[u] = d0 + u < D ? PT[(int64_t)(d0 + u) * m + ic] : 0.f;
#pragma unroll
    for (int u = 0; u < UD; ++u) {
      if (d0 + u < D) {
        const double xv = (double)x[u];
#pragma unroll
        for (int j = 0; j < kPPMaxT; ++j)
          if (j < nt) dot[j] = fma(xv, sc[j * D + d0 + u], dot[j]);
      }
    }
  }
  const double wi = ok ? w[i] : 0.0, di = ok ? d2[i] : 0.0, pi = pn[ic];
#pragma unroll
  for (int j = 0; j < kPPMaxT; ++j) {
    if (j < nt) {
      const double c = fmax(pi + pn[cand[j]] - 2.0 * dot[j], 0.0);
      if (ok) cd[(int64_t)j * m + i] = c;
      const double s = pp_block_sum(wi * fmin(di, c), red);
      if (threadIdx.x == 0) partial[(int64_t)blk * kPPMaxT + j] = s;
    }
  }
}

__global__ __launch_bounds__(kPDThreads) void kpp_dist_kernel(const float* __restrict__ PT,
                                                               const double* __restrict__ w,
                                                               const double* __restrict__ pn, int m, int D,
                                                               int trials, const int* __restrict__ cand, int mode,
                                                               double* __restrict__ d2, double* __restrict__ cd,
                                                               double* __restrict__ partial) {
  extern __shared__ double sc[];
  __shared__ double red[kPDThreads / 64];
  if (mode == 0 || gridDim.y == 1) {
    kpp_dist(PT, w, pn, m, D, trials, cand, mode, d2, cd, partial, blockIdx.x, sc, red);
    return;
  }
  // mode 1 on a (row block, trial) grid: one trial per block -- the same FMA sequence per
  // (row, trial) as the all-trials loop, spread over trials x more blocks (the one-block-
  // per-256-rows grid kept ~16 CUs busy for ~80 us per greedy step)
  const int j = blockIdx.y;
  const int cj = cand[j];
  for (int d = threadIdx.x; d < D; d += kPDThreads) sc[d] = (double)PT[(int64_t)d * m + cj];
  __syncthreads();
  const int blk = blockIdx.x;
  const int i = blk * kPDThreads + threadIdx.x;
  const bool ok = i < m;
  const int ic = ok ? i : m - 1;
  constexpr int UD = 8;
  double dot = 0.0;
  for (int d0 = 0; d0 < D; d0 += UD) {
    float x[UD];
#pragma unroll
    for (int u = 0; u < UD; ++u) x[u] = d0 + u < D ? PT[(int64_t)(d0 + u) * m + ic] : 0.f;
#pragma unroll
    for (int u = 0; u < UD; ++u)
      if (d0 + u < D) dot = fma((double)x[u], sc[d0 + u], dot);
  }
  const double wi = ok ? w[i] : 0.0, di = ok ? d2[i] : 0.0, pi = pn[ic];
  const double c = fmax(pi + pn[cj] - 2.0 * dot, 0.0);
  if (ok) cd[(int64_t)j * m + i] = c;
  const double sj = pp_block_sum(wi * fmin(di, c), red);
  if (threadIdx.x == 0) partial[(int64_t)blk * kPPMaxT + j] = sj;
}

// One block.  mode 0 (t = 1): prefix sum of w * d2, the step-1 draws.  mode 1 (step t):
// pick = argmin of the trials' potentials (block partials summed in order), picks[t],
// d2 = min(d2, cd[best]), then (t + 1 < k) the prefix sum and step t+1's draws.  mode 2
// (t = 0): prefix sum of w alone and the first draw.  LDS: cs [m] (m <= kPPLdsRows) else
// the global cs.
constexpr int kPPLdsRows = 16384;
template <int NTH>
__device__ void kpp_pick(const double* __restrict__ w, int m, int k, int trials, const double* __restrict__ U, int t,
                         int mode, int nblocks, const double* __restrict__ partial, const double* __restrict__ cd,
                         double* __restrict__ d2, double* __restrict__ csg, int* __restrict__ cand,
                         int* __restrict__ picks, double* lcs, double* part, int& s_best) {
  double* const cs = lcs != nullptr ? lcs : csg;
  const int tid = threadIdx.x;
  const int nt = trials + 1;
  if (mode == 1) {
    // trial j's potential = its block partials summed in block order: the partials are
    // loaded by all threads at once (part[] as staging), then summed per trial from LDS
    double pj = 0.0;
    for (int b0 = 0; b0 < nblocks; b0 += NTH / kPPMaxT) {
      const int bb = b0 + tid / kPPMaxT, jj = tid % kPPMaxT;
      __syncthreads();
      part[tid] = (bb < nblocks && jj < trials) ? partial[(int64_t)bb * kPPMaxT + jj] : 0.0;
      __syncthreads();
      if (tid < trials) {
        const int nb = min(NTH / kPPMaxT, nblocks - b0);
        for (int q = 0; q < nb; ++q) pj += part[q * kPPMaxT + tid];
      }
    }
    __syncthreads();
    if (tid < trials) part[tid] = pj;
    __syncthreads();
    if (tid == 0) {
      int best = 0;
      for (int j = 1; j < trials; ++j)
        if (part[j] < part[best]) best = j;
      s_best = best;
      picks[t] = cand[best];
    }
    __syncthreads();
    if (t + 1 >= k) return;                  // last step: d2 is not needed any more
  }
  const int best = mode == 1 ? s_best : 0;
  // p_i = w_i * d2_i (d2 updated with the pick first): coalesced pass into cs, then each
  // thread scans its contiguous chunk of cs
  for (int i = tid; i < m; i += NTH) {
    double pi = w[i];
    if (mode != 2) {
      double di = d2[i];
      if (mode == 1) {
        di = fmin(di, cd[(int64_t)best * m + i]);
        d2[i] = di;
      }
      pi *= di;
    }
    cs[i] = pi;
  }
  __syncthreads();
  const int per = (m + NTH - 1) / NTH;
  const int a = tid * per, e = min(m, a + per);
  double s = 0.0;
  for (int i = a; i < e; ++i) {
    s += cs[i];
    cs[i] = s;                               // local running sum, offset below
  }
  part[tid] = s;
  __syncthreads();
  for (int off = 1; off < NTH; off <<= 1) {   // Hillis-Steele, fixed order
    const double add = tid >= off ? part[tid - off] : 0.0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  const double base = tid ? part[tid - 1] : 0.0;
  for (int i = a; i < e; ++i) cs[i] += base;
  __syncthreads();
  const double tot = part[NTH - 1];
  if (mode == 2) {
    if (tid == 0) {
      const int first = pp_draw(cs, m, tot, U[0]);
      cand[0] = first;
      picks[0] = first;
    }
  } else {
    const int tn = mode == 0 ? 1 : t + 1;    // the step the draws are for
    if (tid < trials) cand[tid] = pp_draw(cs, m, tot, U[(int64_t)tn * nt + tid]);
  }
}

__global__ __launch_bounds__(kPPThreads) void kpp_pick_kernel(const double* __restrict__ w, int m, int k, int trials,
                                                               const double* __restrict__ U, int t, int mode,
                                                               int nblocks, const double* __restrict__ partial,
                                                               const double* __restrict__ cd, double* __restrict__ d2,
                                                               double* __restrict__ csg, int* __restrict__ cand,
                                                               int* __restrict__ picks) {
  extern __shared__ double lcs[];
  __shared__ double part[kPPThreads];
  __shared__ int s_best;
  kpp_pick<kPPThreads>(w, m, k, trials, U, t, mode, nblocks, partial, cd, d2, csg, cand, picks,
                       m <= kPPLdsRows ? lcs : nullptr, part, s_best);
}

}  // namespace

// PT = fp32(P)^T [D][m], w [m] weights, pn [m] = |fp32(p)|^2 (fp64 sums), U [k][trials + 1]
// uniforms; ws: d2 [m], cs [m], cd [trials][m] fp64, partial [ceil(m / 256)][16] fp64,
// cand [16] int32 scratch; picks [k] int32 out.  trials <= 16.  (One cooperative launch with
// grid barriers between the phases measured no faster than the 2k launches: 0.104 vs 0.096 s
// at k = 1024, m = 4097 -- each grid barrier writes back and invalidates the L2.)
O3S_API int o3s_kmeanspp(const float* PT, const double* w, const double* pn, int m, int D, int k, int trials,
                         const double* U, double* d2, double* cs, double* cd, double* partial, int* cand,
                         int* picks, hipStream_t st) {
  if (m <= 0 || k <= 0 || D <= 0 || trials < 1 || trials > kPPMaxT) return -1;
  const size_t dl = sizeof(double) * (size_t)trials * D;
  if (dl > 64 * 1024) return -2;
  const int nb = (m + kPDThreads - 1) / kPDThreads;
  const size_t pl = m <= kPPLdsRows ? sizeof(double) * (size_t)m : 0;
  hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(kPPThreads), pl, st, w, m, k, trials, U, 0, 2, nb, partial, cd, d2,
                     cs, cand, picks);
  if (k > 1) {
    hipLaunchKernelGGL(kpp_dist_kernel, dim3(nb), dim3(kPDThreads), sizeof(double) * D, st, PT, w, pn, m, D, trials,
                       cand, 0, d2, cd, partial);
    hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(kPPThreads), pl, st, w, m, k, trials, U, 1, 0, nb, partial, cd,
                       d2, cs, cand, picks);
  }
  for (int t = 1; t < k; ++t) {
    hipLaunchKernelGGL(kpp_dist_kernel, dim3(nb, trials), dim3(kPDThreads), sizeof(double) * D, st, PT, w, pn, m, D,
                       trials, cand, 1, d2, cd, partial);
    hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(kPPThreads), pl, st, w, m, k, trials, U, t, 1, nb, partial, cd,
                       d2, cs, cand, picks);
  }
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_PRELOAD(kmeans_init)

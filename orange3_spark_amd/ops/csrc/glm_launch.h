// Host side of the GLM passes (glm_grad.hip, glm_mixed.hip, glm_stats.hip, glm_softmax.hip):
// the row layout for a row stride, the run-time -> compile-time dispatchers, the launch
// helpers, and the two finish kernels that sum a pass's slab rows.
//
// The finish kernels are no templates, so every unit that includes this header compiles its
// own copy of the two (anonymous namespace: no duplicate symbol); they are tiny.  The rest is
// host code and free to change: it does not reach the device code of any kernel.
#pragma once
#include <type_traits>

#include "glm_rows.h"

namespace {

// out[i] = sum_b partial[b][i] in fp64, fixed order (deterministic).  Block = 32
// columns x 32 strided partial-row groups; each thread sums nblocks/32 rows, then the
// 32 group sums of a column are combined in LDS in a fixed order.
__global__ __launch_bounds__(1024) void glm_finish_kernel(const float* __restrict__ partial, int nblocks,
                                                          int pstride, int ncols, double* __restrict__ out,
                                                          int accumulate) {
  __shared__ double red[32][33];
  const int cx = threadIdx.x & 31, gy = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + cx;
  double s = 0.0;
  if (i < ncols)
    for (int b = gy; b < nblocks; b += 32) s += (double)partial[(int64_t)b * pstride + i];
  red[gy][cx] = s;
  __syncthreads();
  if (gy == 0 && i < ncols) {
    double t = 0.0;
#pragma unroll 8
    for (int q = 0; q < 32; ++q) t += red[q][cx];
    out[i] = accumulate ? out[i] + t : t;
  }
}

// glm_finish_kernel over fp64 rows (level 2 of the item slab's sum: the mid rows of
// glm_item_sum_kernel, glm_mixed.hip), same order.
__global__ __launch_bounds__(1024) void glm_finish_f64_kernel(const double* __restrict__ mid, int nrows, int pstride,
                                                              int ncols, double* __restrict__ out) {
  __shared__ double red[32][33];
  const int cx = threadIdx.x & 31, gy = threadIdx.x >> 5;
  const int i = blockIdx.x * 32 + cx;
  double s = 0.0;
  if (i < ncols)
    for (int b = gy; b < nrows; b += 32) s += mid[(int64_t)b * pstride + i];
  red[gy][cx] = s;
  __syncthreads();
  if (gy == 0 && i < ncols) {
    double t = 0.0;
#pragma unroll 8
    for (int q = 0; q < 32; ++q) t += red[q][cx];
    out[i] = t;
  }
}

int pick_lpr(int nch) {
  int l = 4;
  while (l < nch && l < 64) l <<= 1;
  return l;
}
int pick_cpl(int nch) {
  if (nch <= 64) return 1;
  const int need = (nch + 63) / 64;
  int c = 2;
  while (c < need) c <<= 1;
  return c;  // 2,4,8,16 (caller checks <= 16)
}

// Row layout for row stride ld: (lpr, cpl) is the natural split of pick_lpr / pick_cpl.
// The lineage pass is VALU bound and its per-row work (row key, cross-lane dot reduction,
// residual broadcast) is replicated on every lane of a row, so the mixed, stats and fp32
// passes use (lpr_s, cpl_s): 4x fewer lanes per row with 4x more columns each where the
// natural split has spare lanes (same padded width dpad).
struct Layout { int lpr, cpl, lpr_s, cpl_s, dpad; };
bool resolve_layout(int64_t ld, Layout* l) {
  const int nch = (int)(ld / 8);
  const int lpr = pick_lpr(nch), cpl = pick_cpl(nch);
  if (ld % 8 != 0 || cpl > 16) return false;
  int lpr_s = lpr, cpl_s = cpl;
  if (cpl == 1 && lpr >= 16) { lpr_s = lpr / 4; cpl_s = 4; }
  else if (cpl == 2) { lpr_s = 32; cpl_s = 4; }
  *l = Layout{lpr, cpl, lpr_s, cpl_s, lpr * cpl * 8};
  return true;
}

// Every (lpr, cpl) and every (lpr_s, cpl_s) resolve_layout can return.
#define O3S_NATURAL_LAYOUTS(M) M(4, 1) M(8, 1) M(16, 1) M(32, 1) M(64, 1) M(64, 2) M(64, 4) M(64, 8) M(64, 16)
#define O3S_REMAPPED_LAYOUTS(M) M(4, 1) M(8, 1) M(4, 4) M(8, 4) M(16, 4) M(32, 4) M(64, 4) M(64, 8) M(64, 16)

// Run-time -> compile-time dispatch: f gets each value as a std::integral_constant object,
// which converts to its int in constant expressions (template arguments included), and
// returns the entry point's return code.
template <int V> using IC = std::integral_constant<int, V>;
#define O3S_LAYOUT_CASE(L, C) \
  if (lpr == L && cpl == C) return f(IC<L>{}, IC<C>{});
template <class F>
int with_natural_layout(const Layout& l, F&& f) {
  const int lpr = l.lpr, cpl = l.cpl;
  O3S_NATURAL_LAYOUTS(O3S_LAYOUT_CASE)
  return -1;
}
template <class F>
int with_remapped_layout(const Layout& l, F&& f) {
  const int lpr = l.lpr_s, cpl = l.cpl_s;
  O3S_REMAPPED_LAYOUTS(O3S_LAYOUT_CASE)
  return -1;
}
#undef O3S_LAYOUT_CASE
#undef O3S_NATURAL_LAYOUTS
#undef O3S_REMAPPED_LAYOUTS
template <class F>
int with_loss(int loss, F&& f) {
  if (loss == LOSS_LOGISTIC) return f(IC<LOSS_LOGISTIC>{});
  if (loss == LOSS_HINGE) return f(IC<LOSS_HINGE>{});
  return f(IC<LOSS_SQUARED>{});
}
template <class F>
int with_remapped_layout_and_loss(const Layout& l, int loss, F&& f) {
  return with_remapped_layout(l, [&](auto L, auto C) {
    return with_loss(loss, [&](auto LOSS) { return f(L, C, LOSS); });
  });
}

template <class... P, class... A>
void launch(void (*kernel)(P...), int grid, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, static_cast<P>(args)...);
}
// out[0..ncols) = (accumulate ? out : 0) + the column sums of the grid slab rows.
int launch_finish(const float* partial, int grid, int pstride, int ncols, double* out, int accumulate,
                  hipStream_t st) {
  O3S_CHECK_LAUNCH();
  hipLaunchKernelGGL(glm_finish_kernel, dim3((ncols + 31) / 32), dim3(1024), 0, st, partial, grid, pstride, ncols,
                     out, accumulate);
  O3S_CHECK_LAUNCH();
  return 0;
}

// A gradient pass runs as `splits` launches over consecutive 1/splits slices of the
// resident and of the lineage rows; later slices add their block sums into the first
// slice's slabs (pacc; slice order fixed: as deterministic as one launch).  A grid-stride
// tile walk drifts over a long launch -- waves that started together end up gigabytes
// apart, so the resident stream touches a wider address window; restarting the walk every
// 1/splits of a 255 GB table measured 44.2 -> 43.7 ms even with a finish per slice
// (tools/bench_glm_split_ab.py).  slice(r_lo, r_n, l_lo, l_n, pacc) launches one slice.
// unit: every slice boundary, the last included, is rounded down to a multiple of it, so
// the slices cover the whole tiles of each role and leave fewer than `unit` rows of each.
template <class F>
int for_row_slices(int splits, int64_t n_res, int64_t n_lin, F&& slice, int64_t unit = 1) {
  const int K = splits < 1 ? 1 : splits;
  const auto cut = [&](int64_t n, int k) { return n * k / K / unit * unit; };
  for (int k = 0; k < K; ++k) {
    const int64_t r_lo = cut(n_res, k), l_lo = cut(n_lin, k);
    const int rc = slice(r_lo, cut(n_res, k + 1) - r_lo, l_lo, cut(n_lin, k + 1) - l_lo, k > 0);
    if (rc != 0) return rc;
    O3S_CHECK_LAUNCH();
  }
  return 0;
}

}  // namespace

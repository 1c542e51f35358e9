// Fused tree-ensemble scoring (DecisionTree / RandomForest / GBT transform) for gfx950.
//
// Packed ensemble (built and validated on the host, ops/tree_predict.py):
//   node   8 bytes = two dwords {w0, w1}
//            internal: w0 = fp32 threshold bits (the fp64 threshold rounded toward -inf, so
//                      float(x) <= w0 equals double(x) <= t for every fp32 / bf16 x),
//                      w1 = feature (bits 0..15, < 0xffff) | left child (bits 16..31); the
//                      right child is left + 1; child indices count from the first node of
//                      the launch's tree group and are larger than their parent's
//            leaf:     w1 bits 0..15 = 0xffff, w0 = the leaf's preorder index in its tree
//   tree_root[t]   index of tree t's root in the group's node image
//   tree_base[t]   row of tree t's leaf 0 in the value table: a leaf's row is base + w0
//   values         fp64 [total leaves][V], leaf value * tree weight (multiplied on the host:
//                  the kernel only adds, there is nothing for -ffp-contract to fuse)
//
// One launch scores one tree group over all rows; one lane owns one row, a wave owns 64
// consecutive rows, the grid is persistent (grid-stride over 64-row chunks).  The group's
// nodes are copied into LDS once per block.  SUM mode: out[row][0..V) += values[leaf] tree
// by tree in ensemble order (the accumulators start from out, which the host zeroes before
// the first group): a fixed sequence of fp64 adds per row, the same bits for any grid, LDS
// budget or grouping; no atomics.  LEAF mode: out[row][col0 + t] = preorder leaf index.
//
// Two trees are walked at a time: a step is two dependent LDS reads (node, feature), and a
// second independent chain per lane hides half of that latency without more LDS per wave.
// A tree's leaf values are gathered after its walk and added after the next pair's walk, in
// tree order, so the gather's latency is covered by that walk (two pending sets used in
// turn, so no register is copied while its load is in flight).
//
// V is a template width VT in {1, 4, 16} (accumulators in registers, V <= VT at run time):
// a run-time loop over V would index the accumulators dynamically (scratch) or accumulate
// in memory per tree; three widths keep V = 1 (GBT, regressors) at two VGPRs per
// accumulator set and cover binary / few-class / up to 16-class forests.
//
// STAGE: rows whose stride in bytes is a multiple of 16 from a 16-B aligned base are staged
// per wave into LDS with coalesced 16-B loads (the wave's 64 rows are one contiguous run)
// at a padded pitch (pitch / 4 odd: the lanes' rows start on distinct banks); padding
// columns land in the tile and are never read as a feature (features < d <= ld).
// Otherwise every split feature is read from global memory.
#include "common.h"

using namespace o3s;

namespace {

constexpr int kTpThreads = 256;
constexpr int kTpWaves = kTpThreads / kWave;
constexpr uint32_t kTpLeaf = 0xffffu;
constexpr size_t kTpMaxLds = 160 * 1024;
constexpr int kTpInFlight = 8;            // 16-B row loads a lane keeps in flight while staging

template <bool BF16, bool STAGE>
__device__ __forceinline__ float tp_feature(const uint8_t* srow, const void* grow, uint32_t f) {
  if constexpr (BF16) {
    const uint16_t* p = reinterpret_cast<const uint16_t*>(STAGE ? (const void*)srow : grow);
    return bf16_to_f32(p[f]);
  } else {
    const float* p = reinterpret_cast<const float*>(STAGE ? (const void*)srow : grow);
    return p[f];
  }
}

template <bool BF16, bool STAGE, int VT, bool LEAF>
__global__ __launch_bounds__(kTpThreads) void tree_predict_kernel(
    const uint8_t* __restrict__ X, int64_t n, int64_t ldb, int pitch, const uint2* __restrict__ nodes, int n_nodes,
    const int32_t* __restrict__ tree_root, const int32_t* __restrict__ tree_base, int n_trees, int max_depth,
    const double* __restrict__ values, int V, double* __restrict__ out, int64_t out_ld, int col0) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  uint2* img = reinterpret_cast<uint2*>(lds);                              // [n_nodes]
  uint8_t* stage = lds + 8 * (size_t)((n_nodes + 1) & ~1);                 // [waves][64][pitch]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < n_nodes; i += kTpThreads) img[i] = nodes[i];
  __syncthreads();
  uint8_t* my_stage = stage + (size_t)wid * 64 * pitch;
  const uint8_t* srow = my_stage + lane * pitch;
  const int64_t nchunks = (n + 63) / 64;
  const int64_t wstride = (int64_t)gridDim.x * kTpWaves;
  for (int64_t c = (int64_t)blockIdx.x * kTpWaves + wid; c < nchunks; c += wstride) {
    const int64_t r0 = c * 64;
    const int rows = n - r0 < 64 ? (int)(n - r0) : 64;
    const bool ok = lane < rows;
    const int64_t i = r0 + (ok ? lane : rows - 1);
    const uint8_t* grow = X + i * ldb;
    if constexpr (STAGE) {
      const int qpr = (int)(ldb >> 4), qtot = rows * qpr;
      const uint4* src = reinterpret_cast<const uint4*>(X + r0 * ldb);
      // kTpInFlight loads per lane are issued before the first is written to LDS (one load
      // at a time left the whole stage at one HBM latency per 1 KB of the wave's rows)
      for (int e0 = lane; e0 < qtot; e0 += 64 * kTpInFlight) {
        uint4 v[kTpInFlight];
#pragma unroll
        for (int k = 0; k < kTpInFlight; ++k)
          if (e0 + 64 * k < qtot) v[k] = src[e0 + 64 * k];
#pragma unroll
        for (int k = 0; k < kTpInFlight; ++k) {
          const int e = e0 + 64 * k;
          if (e < qtot) {
            const int rr = e / qpr, q = e - rr * qpr;
            uint32_t* d = reinterpret_cast<uint32_t*>(my_stage + rr * pitch + 16 * q);
            d[0] = v[k].x; d[1] = v[k].y; d[2] = v[k].z; d[3] = v[k].w;
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // pend[0..1]: the gathered values of the pair walked first in an iteration, pend[2..3] of
    // the pair walked second; each is added, in tree order, after the walk that follows its
    // gather.  VT = 16 adds at once (four pending sets would not fit the register file).
    constexpr bool DEFER = VT <= 4;
    double acc[VT], pend[4][VT];
#pragma unroll
    for (int v = 0; v < VT; ++v) {
      acc[v] = (!LEAF && v < V) ? out[i * out_ld + v] : 0.0;
      pend[0][v] = pend[1][v] = pend[2][v] = pend[3][v] = 0.0;
    }
    // trees t and t + 1 (t alone where it is the last): their leaves' preorder indices
    auto walk = [&](int t, uint32_t& ka, uint32_t& kb) {
      const bool two = t + 1 < n_trees;
      int ia = tree_root[t], ib = tree_root[two ? t + 1 : t];
      uint2 na = img[ia], nb = img[ib];
      for (int s = 0; s < max_depth; ++s) {
        const uint32_t fa = na.y & 0xffffu, fb = nb.y & 0xffffu;
        const bool la = fa == kTpLeaf, lb = fb == kTpLeaf;
        if (la && lb) break;                                               // both at a leaf (lane-divergent)
        const float xa = tp_feature<BF16, STAGE>(srow, grow, la ? 0u : fa);
        const float xb = tp_feature<BF16, STAGE>(srow, grow, lb ? 0u : fb);
        // !(x <= t): NaN goes right
        ia = la ? ia : (int)(na.y >> 16) + (xa <= __uint_as_float(na.x) ? 0 : 1);
        ib = lb ? ib : (int)(nb.y >> 16) + (xb <= __uint_as_float(nb.x) ? 0 : 1);
        na = img[ia];
        nb = img[ib];
      }
      // the host validated every tree's depth <= max_depth: both nodes are leaves here
      ka = (na.y & 0xffffu) == kTpLeaf ? na.x : 0u;
      kb = (nb.y & 0xffffu) == kTpLeaf ? nb.x : 0u;
      if constexpr (LEAF) {
        if (ok) {
          out[i * out_ld + col0 + t] = (double)ka;
          if (two) out[i * out_ld + col0 + t + 1] = (double)kb;
        }
      }
    };
    auto gather = [&](int t, uint32_t ka, uint32_t kb, double (&pa)[VT], double (&pb)[VT]) {
      const bool two = t + 1 < n_trees;
      const double* va = values + ((int64_t)tree_base[t] + ka) * V;
      const double* vb = values + ((int64_t)tree_base[two ? t + 1 : t] + kb) * V;
#pragma unroll
      for (int v = 0; v < VT; ++v) {
        pa[v] = v < V ? va[v] : 0.0;
        pb[v] = (two && v < V) ? vb[v] : 0.0;
      }
    };
    auto add = [&](const double (&pa)[VT], const double (&pb)[VT]) {
#pragma unroll
      for (int v = 0; v < VT; ++v) { acc[v] += pa[v]; acc[v] += pb[v]; }
    };
    for (int t = 0; t < n_trees; t += 4) {
      uint32_t ka, kb;
      walk(t, ka, kb);
      if constexpr (!LEAF) {
        if constexpr (DEFER) add(pend[2], pend[3]);
        gather(t, ka, kb, pend[0], pend[1]);
        if constexpr (!DEFER) add(pend[0], pend[1]);
      }
      if (t + 2 < n_trees) {
        walk(t + 2, ka, kb);
        if constexpr (!LEAF) {
          if constexpr (DEFER) add(pend[0], pend[1]);
          gather(t + 2, ka, kb, pend[2], pend[3]);
          if constexpr (!DEFER) add(pend[2], pend[3]);
        }
      } else if constexpr (!LEAF && DEFER) {
        add(pend[0], pend[1]);
#pragma unroll
        for (int v = 0; v < VT; ++v) pend[2][v] = pend[3][v] = 0.0;
      }
    }
    if constexpr (!LEAF) {
      if constexpr (DEFER) add(pend[2], pend[3]);
#pragma unroll
      for (int v = 0; v < VT; ++v)
        if (ok && v < V) out[i * out_ld + v] = acc[v];
    }
    if constexpr (STAGE) __builtin_amdgcn_wave_barrier();                  // the stage is rewritten next chunk
  }
}

// pitch of a staged row of ldb bytes (0: this layout is not staged)
int tp_pitch(int64_t ldb) {
  if (ldb <= 0 || ldb % 16 != 0 || ldb > (1 << 20)) return 0;
  return (int)((ldb / 4) % 2 == 0 ? ldb + 4 : ldb);
}

}  // namespace

// LDS of a launch: the node image, and the row stage if `aligned` rows of ldb bytes fit beside
// it within lds_budget.  *pitch: the staged row pitch (0 = split features come from global
// memory), *lds: bytes.  Returns -2 where the node image alone exceeds the budget.
O3S_API int o3s_tree_predict_layout(int64_t ldb, int aligned, int n_nodes, int lds_budget, int* pitch, int* lds) {
  if (n_nodes < 1 || n_nodes > 65536 || lds_budget <= 0 || !pitch || !lds) return -1;
  const size_t img = 8 * (size_t)((n_nodes + 1) & ~1);
  const size_t cap = (size_t)lds_budget < kTpMaxLds ? (size_t)lds_budget : kTpMaxLds;
  *pitch = 0;
  *lds = 0;
  if (img > cap) return -2;
  const int p = aligned ? tp_pitch(ldb) : 0;
  const size_t st = (size_t)kTpWaves * 64 * (size_t)p;
  *pitch = (p && img + st <= cap) ? p : 0;
  *lds = (int)(img + (*pitch ? st : 0));
  return 0;
}

// X: [n] rows of d features (bf16 if bf16 else fp32), row stride ld elements (>= d);
// nodes / tree_root / tree_base / values: one tree group of the packed ensemble (above);
// leaf_mode 0: out[row * out_ld + v] += ... for v < V (out_ld >= V), 1: out[row * out_ld +
// col0 + t] = leaf index.  pitch: from o3s_tree_predict_layout (0 = unstaged).
O3S_API int o3s_tree_predict(const void* X, int bf16, int64_t n, int64_t ld, int d, const void* nodes, int n_nodes,
                             const int32_t* tree_root, const int32_t* tree_base, int n_trees, int max_depth,
                             const double* values, int V, int leaf_mode, double* out, int64_t out_ld, int col0,
                             int pitch, int lds_budget, int grid, hipStream_t st) {
  if (!X || !nodes || !tree_root || !tree_base || !out || (!leaf_mode && !values)) return -1;
  if (d < 1 || d > 65534 || ld < d || n_trees < 1 || max_depth < 0 || grid < 1 || col0 < 0) return -1;
  if (n_nodes < 1 || n_nodes > 65536) return -1;
  if (!leaf_mode && (V < 1 || V > 16 || out_ld < V)) return -1;
  if (leaf_mode && out_ld < (int64_t)col0 + n_trees) return -1;
  const int64_t ldb = ld * (bf16 ? 2 : 4);
  if (pitch != 0 && (pitch != tp_pitch(ldb) || ((uintptr_t)X & 15) != 0)) return -3;
  const size_t lds = 8 * (size_t)((n_nodes + 1) & ~1) + (size_t)kTpWaves * 64 * (size_t)pitch;
  if (lds_budget <= 0 || lds > (size_t)lds_budget || lds > kTpMaxLds) return -2;
  if (n <= 0) return 0;
#define O3S_TP4(B, S, VT, L)                                                                               \
  do {                                                                                                     \
    auto kern = tree_predict_kernel<B, S, VT, L>;                                                          \
    if (lds > 64 * 1024) {                                                                                 \
      hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),                             \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);           \
      if (e_ != hipSuccess) return (int)e_;                                                                \
    }                                                                                                      \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kTpThreads), lds, st, (const uint8_t*)X, n, ldb, pitch,      \
                       (const uint2*)nodes, n_nodes, tree_root, tree_base, n_trees, max_depth, values, V,  \
                       out, out_ld, col0);                                                                 \
  } while (0)
#define O3S_TP2(B, S)                                                                                      \
  do {                                                                                                     \
    if (leaf_mode) O3S_TP4(B, S, 1, true);                                                                 \
    else if (V == 1) O3S_TP4(B, S, 1, false);                                                              \
    else if (V <= 4) O3S_TP4(B, S, 4, false);                                                              \
    else O3S_TP4(B, S, 16, false);                                                                         \
  } while (0)
  if (bf16 && pitch) O3S_TP2(true, true);
  else if (bf16) O3S_TP2(true, false);
  else if (pitch) O3S_TP2(false, true);
  else O3S_TP2(false, false);
#undef O3S_TP2
#undef O3S_TP4
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_PRELOAD(tree_predict)

// KMeans beside the assign pass of kmeans_assign.hip (gfx950): the per-cluster sums that
// Spark's KMeans runs per iteration, the Hamerly bound update, the centring moments and the
// training cost.  Nothing here is register-tuned (kmeans_update_kernel's order of operations
// makes its sums bitwise deterministic; the rest are plain streaming loops); device code
// changes are still checked with tools/isa_diff.py.
//
// kmeans_update: per-cluster sums without float atomics.  Each block takes chunks of
// R rows, counting-sorts their indices by cluster in LDS, then each wave owns a contiguous
// cluster range and streams its rows (coalesced 512-B row reads) accumulating in
// registers; a cluster's sum is flushed once per chunk into the block's private slab.
// (The bucket order is row order, produced by a stable ballot-ranked scatter.)
// Slabs are summed by kmeans_reduce in a fixed order (bitwise deterministic).
#include "common.h"

using namespace o3s;

namespace {

constexpr int kUpdThreads = 512;
constexpr int kUpdWaves = kUpdThreads / kWave;

// Rows per chunk R (host-chosen, <= 65536 so sorted indices fit uint16): the largest of
// 16384..1024 whose LDS image fits.  Bigger chunks amortise the per-chunk slab
// read-modify-write (Kp x D floats) over more X bytes.
__host__ __device__ inline int upd_lds_bytes(int Kp, int R) {
  // start[Kp+1] int + per-(wave, cluster) uint16 counts + sorted[R] uint16
  return (int)(sizeof(int) * (Kp + 1) + sizeof(uint16_t) * (kUpdWaves * Kp + R));
}
inline int upd_rows(int Kp) {
  for (int R = 16384; R >= 8192; R >>= 1)              // 2 blocks per CU
    if (upd_lds_bytes(Kp, R) <= 80 * 1024) return R;
  for (int R = 16384; R >= 256; R >>= 1)               // 1 block per CU
    if (upd_lds_bytes(Kp, R) <= 160 * 1024) return R;
  return 0;
}

// One block: chunks of R rows; slab (block-private) = [Kp][D] sums + [Kp] counts.
// Counting sort by cluster that is STABLE without any sort pass: wave w owns rows
// [w R/8, (w+1) R/8) of the chunk; per-(wave, cluster) counts give each wave its base
// inside every bucket, and inside a wave the 64-row groups are scattered in row order
// with ballot ranking (peel one key per step: rank = popcount of same-key lanes below).
// Bucket order is therefore row order -> bitwise-deterministic sums for any k (the old
// in-bucket insertion sort was O(bucket^2) per thread, i.e. quadratic at small k).
// DV: floats per lane per row (scalar path, D <= 64 * DV); LPR > 0: vector path, LPR
// lanes x float4 per row (D <= 4 * LPR, D % 4 == 0, 16-B rows), 64 / LPR rows per load.
template <int DV, int LPR>
__global__ __launch_bounds__(kUpdThreads) void kmeans_update_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, int D, const int32_t* __restrict__ assign,
    int Kp, int R, float* __restrict__ slab, float* __restrict__ cnt_slab) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  int* start = smem;                                    // [Kp+1] bucket starts
  // [waves][Kp] uint16 counts -> per-wave bases (seg <= 2048 rows per wave fits 16 bits).
  // Counted as 32-bit LDS atomics on the word shared by waves 2j / 2j+1 (halves never carry).
  uint16_t* cntw = reinterpret_cast<uint16_t*>(start + Kp + 1);
  uint32_t* cnt32 = reinterpret_cast<uint32_t*>(cntw);  // [waves/2][Kp] words
  uint16_t* sorted = cntw + kUpdWaves * Kp;             // [R]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int seg = R / kUpdWaves;                        // rows per wave segment (a multiple of 64, or 32 at R = 256)
  uint16_t* mycw = cntw + (wid >> 1) * 2 * Kp;          // element (key) at mycw[2*key + (wid&1)]
  const int half = wid & 1;
  float* myslab = slab + (int64_t)blockIdx.x * Kp * D;
  float* mycnt = cnt_slab + (int64_t)blockIdx.x * Kp;
  const int64_t nch = (n + R - 1) / R;
  for (int64_t cidx = blockIdx.x; cidx < nch; cidx += gridDim.x) {
    const int64_t r0 = cidx * R;
    const int rows = (int)min((int64_t)R, n - r0);
    for (int i = threadIdx.x; i < kUpdWaves / 2 * Kp; i += kUpdThreads) cnt32[i] = 0u;
    __syncthreads();
    const int s0 = wid * seg, s1 = min(rows, s0 + seg);
    for (int i = s0 + lane; i < s1; i += kWave)
      atomicAdd(&cnt32[(wid >> 1) * Kp + assign[r0 + i]], 1u << (16 * half));
    __syncthreads();
    // per cluster: exclusive prefix over waves (in place), total -> start[]
    for (int c = threadIdx.x; c < Kp; c += kUpdThreads) {
      int run = 0;
#pragma unroll
      for (int j = 0; j < kUpdWaves / 2; ++j) {
        const uint32_t v = cnt32[j * Kp + c];
        const int lo = (int)(v & 0xffffu), hi = (int)(v >> 16);
        cnt32[j * Kp + c] = (uint32_t)run | ((uint32_t)(run + lo) << 16);
        run += lo + hi;
      }
      start[c] = run;
    }
    __syncthreads();
    if (wid == 0) {   // exclusive scan of bucket sizes by one wave
      int carry = 0;
      for (int b = 0; b < Kp; b += 64) {
        const int v = (b + lane < Kp) ? start[b + lane] : 0;
        int x = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int y = __shfl_up(x, off, 64);
          if (lane >= off) x += y;
        }
        if (b + lane < Kp) start[b + lane] = carry + x - v;
        carry += __shfl(x, 63, 64);
      }
      if (lane == 0) start[Kp] = carry;
    }
    __syncthreads();
    // stable scatter: this wave's groups in row order; mycw[k] is the running base
    for (int g = s0; g < s1; g += kWave) {
      const int i = g + lane;
      const int key = i < s1 ? assign[r0 + i] : -1;
      if (Kp <= 32) {
        // few clusters: peel one key per step (<= 32 steps, usually a handful)
        uint64_t todo = __ballot(i < s1);
        while (todo) {
          const int leader = __ffsll((unsigned long long)todo) - 1;
          const int k = __shfl(key, leader, 64);
          const uint64_t m = __ballot(key == k);
          if (key == k) {
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            sorted[start[k] + mycw[2 * k + half] + rank] = (uint16_t)i;
          }
          if (lane == leader) mycw[2 * k + half] = (uint16_t)(mycw[2 * k + half] + __popcll(m));
          todo &= ~m;
        }
      } else {
        // many clusters (up to 64 distinct keys per group): bitonic-sort the 64
        // (key, lane) pairs in registers (21 compare-exchange steps), then every lane's
        // rank inside its key run comes from one ballot of the run heads -- the same
        // stable order as the peeling loop at a fraction of its ~64 iterations
        uint32_t v = ((uint32_t)(key < 0 ? 0xFFFF : key) << 6) | (uint32_t)lane;
#pragma unroll
        for (int kk = 2; kk <= 64; kk <<= 1) {
#pragma unroll
          for (int j = kk >> 1; j > 0; j >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)v, j, 64);
            const bool keep_min = ((lane & kk) == 0) == ((lane & j) == 0);
            v = keep_min ? (v < o ? v : o) : (v > o ? v : o);
          }
        }
        const int k = (int)(v >> 6);
        const bool valid = k != 0xFFFF;
        const int prev = __shfl_up((int)v, 1, 64) >> 6;
        const int next = __shfl_down((int)v, 1, 64) >> 6;
        const uint64_t heads = __ballot(valid && (lane == 0 || prev != k));
        const uint64_t upto = ~0ull >> (63 - lane);                  // bits 0..lane
        const int run0 = 63 - __clzll((long long)(heads & upto));
        const int rank = lane - run0;
        if (valid) {
          sorted[start[k] + mycw[2 * k + half] + rank] = (uint16_t)(g + (int)(v & 63u));
          if (lane == 63 || next != k) mycw[2 * k + half] = (uint16_t)(mycw[2 * k + half] + rank + 1);
        }
      }
    }
    __syncthreads();
    // wave w owns clusters [c0, c1): its rows are the contiguous sorted range
    const int c0 = (int)((int64_t)Kp * wid / kUpdWaves), c1 = (int)((int64_t)Kp * (wid + 1) / kUpdWaves);
    if constexpr (LPR > 0) {
      // Streaming form: the wave's sorted range is cut at cluster boundaries into RPI
      // contiguous pieces, one per row slot (LPR lanes x float4 = one row); each slot
      // streams its rows with U loads in flight and flushes its register sum to the
      // block slab whenever the cluster changes.  No cluster spans two slots (cut points
      // are bucket starts), so every cluster is summed by one slot in row order
      // (deterministic) and loads stay in flight across cluster boundaries -- the old
      // per-cluster loop waited one HBM round trip per (small) cluster.
      constexpr int RPI = kWave / LPR;
      constexpr int U = 8;
      const int slot = lane / LPR, col = 4 * (lane % LPR);
      const bool cok = col < D;
      const int b0 = start[c0], b1 = start[c1];
      auto cut = [&](int sl) {                    // first cluster of piece sl
        if (sl <= 0) return c0;
        if (sl >= RPI) return c1;
        const int t = b0 + (int)((int64_t)(b1 - b0) * sl / RPI);
        int lo = c0, hi = c1;                     // smallest c in [c0, c1] with start[c] >= t
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (start[mid] >= t) hi = mid; else lo = mid + 1;
        }
        return lo;
      };
      int c = cut(slot);
      const int pe = start[cut(slot + 1)];
      const int pb = start[c];
      int cend = c < c1 ? start[c + 1] : pb;      // (empty piece at the last cluster: no rows)
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      auto flush = [&](int cc) {
        if (!cok) return;
        float4* dst = reinterpret_cast<float4*>(myslab + (int64_t)cc * D + col);
        float4 d4 = *dst;
        d4.x += acc.x; d4.y += acc.y; d4.z += acc.z; d4.w += acc.w;
        *dst = d4;
      };
      for (int t = pb; __ballot(t < pe) != 0ull; t += U) {
        float4 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int pos = t + u;
          x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (cok && pos < pe) x[u] = *reinterpret_cast<const float4*>(X + (r0 + sorted[pos]) * ldx + col);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int pos = t + u;
          if (pos < pe) {
            while (pos >= cend) {                 // leave cluster c (flush it if it had rows)
              if (cend > start[c]) flush(c);
              acc = make_float4(0.f, 0.f, 0.f, 0.f);
              ++c;
              cend = start[c + 1];
            }
            acc.x += x[u].x; acc.y += x[u].y; acc.z += x[u].z; acc.w += x[u].w;
          }
        }
      }
      if (pe > pb) flush(c);
      for (int cc = c0 + lane; cc < c1; cc += kWave) {
        const int sz = start[cc + 1] - start[cc];
        if (sz) mycnt[cc] += (float)sz;
      }
    } else {
    for (int c = c0; c < c1; ++c) {
      const int b0 = start[c], b1 = start[c + 1];
      if (b0 == b1) continue;
      float acc[DV];
#pragma unroll
      for (int v = 0; v < DV; ++v) acc[v] = 0.f;
      int i = b0;
      for (; i + 4 <= b1; i += 4) {       // 4 rows in flight
        float x[4][DV];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float* xp = X + (r0 + sorted[i + u]) * ldx;
#pragma unroll
          for (int v = 0; v < DV; ++v) {
            const int col = lane + 64 * v;
            x[u][v] = col < D ? xp[col] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < DV; ++v) acc[v] += x[u][v];
      }
      for (; i < b1; ++i) {
        const float* xp = X + (r0 + sorted[i]) * ldx;
#pragma unroll
        for (int v = 0; v < DV; ++v) {
          const int col = lane + 64 * v;
          acc[v] += col < D ? xp[col] : 0.f;
        }
      }
      float* dst = myslab + (int64_t)c * D;
#pragma unroll
      for (int v = 0; v < DV; ++v) {
        const int col = lane + 64 * v;
        if (col < D) dst[col] += acc[v];
      }
      if (lane == 0) mycnt[c] += (float)(b1 - b0);
    }
    }
    __syncthreads();
  }
}

// sums[k][d] = sum_g slab[g][k][d] (fixed order), counts likewise.
__global__ void kmeans_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ cnt_slab,
                                     int G, int64_t KD, int Kp, double* __restrict__ sums,
                                     double* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < KD) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)slab[(int64_t)g * KD + i];
    sums[i] = s;
  }
  if (i < Kp) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)cnt_slab[(int64_t)g * Kp + i];
    counts[i] = s;
  }
}

}  // namespace

O3S_API int o3s_kmeans_update_ws(int Kp, int D, int grid, int64_t* slab_floats, int64_t* cnt_floats,
                                 int* lds_bytes) {
  const int R = upd_rows(Kp);
  *slab_floats = (int64_t)grid * Kp * D;
  *cnt_floats = (int64_t)grid * Kp;
  *lds_bytes = R ? upd_lds_bytes(Kp, R) : -1;   // -1: Kp too large for the LDS sort
  return R ? 0 : -3;
}

// slab/cnt_slab must be zeroed by the caller (hipMemsetAsync) before each call.
O3S_API int o3s_kmeans_update(const float* X, int64_t n, int64_t ldx, int D, const int32_t* assign, int Kp,
                              float* slab, float* cnt_slab, int grid, double* sums, double* counts,
                              hipStream_t st) {
  if (D > 256 || n < 0) return -1;
  const int R = upd_rows(Kp);
  if (!R) return -3;
  const int lds = upd_lds_bytes(Kp, R);
  if (n > 0) {
    // every build has the same signature: pick one (template arguments: see the kernel)
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)X & 15) == 0;
    const auto kernel =
        vec ? (D <= 32    ? kmeans_update_kernel<1, 8>
               : D <= 64  ? kmeans_update_kernel<1, 16>
               : D <= 128 ? kmeans_update_kernel<2, 32>
                          : kmeans_update_kernel<4, 64>)
            : (D <= 64    ? kmeans_update_kernel<1, 0>
               : D <= 128 ? kmeans_update_kernel<2, 0>
               : D <= 192 ? kmeans_update_kernel<3, 0>
                          : kmeans_update_kernel<4, 0>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kUpdThreads), lds, st, X, n, ldx, D, assign, Kp, R, slab, cnt_slab);
    O3S_CHECK_LAUNCH();
  }
  const int64_t KD = (int64_t)Kp * D;
  const int64_t work = KD > Kp ? KD : Kp;
  hipLaunchKernelGGL(kmeans_reduce_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, slab, cnt_slab,
                     grid, KD, Kp, sums, counts);
  O3S_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------
// Hamerly bound update of a Lloyd iteration (models/kmeans.py): per row, the upper bound
// on the distance to its centre grows by that centre's shift and the lower bound on every
// other centre shrinks by the largest shift; a row whose bounds no longer certify its
// centre (ub >= lb, or NaN) must be screened again.  Two passes, no atomics, rows in
// ascending order: block b owns the contiguous rows [b R, (b + 1) R); pass 0 updates the
// bounds and counts the block's rows to recheck; pass 1 (only when the caller wants the
// list) writes them at the block's prefix offset, ranked by ballots in row order.
constexpr int kBndThreads = 256;

__device__ __forceinline__ bool bnd_recheck(float2 b) { return !(b.x < b.y); }

__global__ __launch_bounds__(kBndThreads) void kmeans_bounds_kernel(
    const int32_t* __restrict__ a, float2* __restrict__ bnd, int64_t n, int64_t per_block,
    const float* __restrict__ delta, float dmax, int pass, int32_t* __restrict__ cnt,
    const int64_t* __restrict__ offs, int32_t* __restrict__ rows) {
  __shared__ int wtot[kBndThreads / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * per_block;
  const int64_t r1 = r0 + per_block < n ? r0 + per_block : n;
  int64_t out = pass ? offs[blockIdx.x] : 0;
  int total = 0;
  for (int64_t base = r0; base < r1; base += kBndThreads) {
    const int64_t i = base + threadIdx.x;
    bool need = false;
    if (i < r1) {
      float2 bv = bnd[i];
      if (pass == 0) {
        bv.x += delta[a[i]];
        bv.y -= dmax;
        bnd[i] = bv;
      }
      need = bnd_recheck(bv);
    }
    const uint64_t m = __ballot(need);
    if (pass == 0) {
      total += __popcll(m);                                  // wave-uniform
      continue;
    }
    if (lane == 0) wtot[wid] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < kBndThreads / 64; ++q) {
      before += q < wid ? wtot[q] : 0;
      all += wtot[q];
    }
    if (need) rows[out + before + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
    out += all;
    __syncthreads();                                       // wtot reused next chunk
  }
  if (pass == 0) {
    if (lane == 0) wtot[wid] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int q = 0; q < kBndThreads / 64; ++q) t += wtot[q];
      cnt[blockIdx.x] = t;
    }
  }
}

// pass 0: a int32 [n] centres, bnd fp32 [n][2] (ub, lb) moved in place by delta (fp32 [K],
// rounded up) / dmax; cnt int32 [grid] = rows to recheck per block.  pass 1: offs int64
// [grid] (exclusive prefix of cnt) -> rows int32 (ascending).  Rows per block: ceil(n / grid).
O3S_API int o3s_kmeans_bounds(const int32_t* a, float* bnd, int64_t n, const float* delta, float dmax, int pass,
                              int32_t* cnt, const int64_t* offs, int32_t* rows, int grid, hipStream_t st) {
  if (n <= 0) return 0;
  if (n > 0x7fffffffll || grid <= 0 || (pass == 1 && (!offs || !rows))) return -1;
  const int64_t per_block = (n + grid - 1) / grid;
  hipLaunchKernelGGL(kmeans_bounds_kernel, dim3(grid), dim3(kBndThreads), 0, st, a, reinterpret_cast<float2*>(bnd),
                     n, per_block, delta, dmax, pass, cnt, offs, rows);
  O3S_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------
// Shifted moments of the rows in ONE pass (the Lloyd cost identity's centring): per block
// of consecutive rows, fp64 sums of (x - s) per column and of ||x - s||^2, with s a shift
// near the data (models/kmeans.py: a row of rank 0) so the later centring about the exact
// mean cancels nothing.  Thread t owns the float4 column group t % G (G = D / 4) of rows
// t / G, t / G + 256 / G, ...; the block's partial row [D + 1] is written in a fixed order.
namespace {
constexpr int kMomThreads = 256;
__global__ __launch_bounds__(kMomThreads) void kmeans_moments_kernel(const float* __restrict__ X, int64_t n,
                                                                     int64_t ldx, int D, const float* __restrict__ sh,
                                                                     int64_t rows_per_block, double* __restrict__ part) {
  __shared__ double red[kMomThreads][5];
  const int G = D / 4;
  const int per = kMomThreads / G;                       // rows per sweep of the block
  const int t = threadIdx.x;
  const int cg = t % G, r0 = t / G;
  const bool active = r0 < per;
  const int64_t b0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t b1 = b0 + rows_per_block < n ? b0 + rows_per_block : n;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, q = 0.0;
  const float4 c = active ? *reinterpret_cast<const float4*>(sh + 4 * cg) : make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) {
    for (int64_t r = b0 + r0; r < b1; r += per) {
      const float4 v = *reinterpret_cast<const float4*>(X + r * ldx + 4 * cg);
      const double d0 = (double)v.x - c.x, d1 = (double)v.y - c.y, d2 = (double)v.z - c.z, d3 = (double)v.w - c.w;
      s0 += d0; s1 += d1; s2 += d2; s3 += d3;
      q = fma(d0, d0, fma(d1, d1, fma(d2, d2, fma(d3, d3, q))));
    }
  }
  red[t][0] = s0; red[t][1] = s1; red[t][2] = s2; red[t][3] = s3; red[t][4] = q;
  __syncthreads();
  double* out = part + (int64_t)blockIdx.x * (D + 1);
  if (t < G) {                                           // column group t: its threads t, t + G, ...
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int k = t; k < per * G; k += G) { a0 += red[k][0]; a1 += red[k][1]; a2 += red[k][2]; a3 += red[k][3]; }
    out[4 * t] = a0; out[4 * t + 1] = a1; out[4 * t + 2] = a2; out[4 * t + 3] = a3;
  }
  if (t == 0) {
    double a = 0.0;
    for (int k = 0; k < per * G; ++k) a += red[k][4];
    out[D] = a;
  }
}
}  // namespace

// part: fp64 [grid][D + 1] (column sums of x - sh, then the sum of ||x - sh||^2), rows split
// into grid contiguous ranges; D % 4 == 0, D <= 1024, 16-B aligned rows and shift.
O3S_API int o3s_kmeans_moments(const float* X, int64_t n, int64_t ldx, int D, const float* sh, int grid,
                               double* part, hipStream_t st) {
  if (D % 4 != 0 || D <= 0 || D > 4 * kMomThreads || ldx % 4 != 0 || grid <= 0) return -1;
  if (n <= 0) return 0;
  const int64_t rpb = (n + grid - 1) / grid;
  hipLaunchKernelGGL(kmeans_moments_kernel, dim3(grid), dim3(kMomThreads), 0, st, X, n, ldx, D, sh, rpb, part);
  O3S_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------
// Training cost of an assignment: sum over rows of ||x - c_a(x)||^2, directly from the rows
// (one streaming pass; the centre rows are L2-resident gathers).  Thread t owns float4
// column group t % G of rows t / G, t / G + 256 / G, ... of its block's contiguous range;
// a row's four squared differences are summed in fp32 (fma), everything above in fp64,
// the block partial in a fixed order.
namespace {
__global__ __launch_bounds__(kMomThreads) void kmeans_cost_kernel(const float* __restrict__ X, int64_t n, int64_t ldx,
                                                                  int D, const int32_t* __restrict__ a,
                                                                  const float* __restrict__ C, int ldc,
                                                                  int64_t rows_per_block, double* __restrict__ part) {
  __shared__ double red[kMomThreads];
  const int G = D / 4;
  const int per = kMomThreads / G;
  const int t = threadIdx.x;
  const int cg = t % G, r0 = t / G;
  const int64_t b0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t b1 = b0 + rows_per_block < n ? b0 + rows_per_block : n;
  double acc = 0.0;
  if (r0 < per) {
    for (int64_t r = b0 + r0; r < b1; r += per) {
      const float4 x = *reinterpret_cast<const float4*>(X + r * ldx + 4 * cg);
      const float4 c = *reinterpret_cast<const float4*>(C + (int64_t)a[r] * ldc + 4 * cg);
      const float d0 = x.x - c.x, d1 = x.y - c.y, d2 = x.z - c.z, d3 = x.w - c.w;
      acc += (double)fmaf(d0, d0, fmaf(d1, d1, fmaf(d2, d2, d3 * d3)));
    }
  }
  red[t] = acc;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < kMomThreads; ++k) s += red[k];
    part[blockIdx.x] = s;
  }
}
}  // namespace

// part: fp64 [grid] partial costs (rows split into grid contiguous ranges); C: fp32 centre
// rows [.][ldc] indexed by a; D % 4 == 0, 16-B aligned rows.
O3S_API int o3s_kmeans_cost(const float* X, int64_t n, int64_t ldx, int D, const int32_t* a, const float* C, int ldc,
                            int grid, double* part, hipStream_t st) {
  if (D % 4 != 0 || D <= 0 || D > 4 * kMomThreads || ldx % 4 != 0 || ldc % 4 != 0 || grid <= 0) return -1;
  if (n <= 0) return 0;
  const int64_t rpb = (n + grid - 1) / grid;
  hipLaunchKernelGGL(kmeans_cost_kernel, dim3(grid), dim3(kMomThreads), 0, st, X, n, ldx, D, a, C, ldc, rpb, part);
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_PRELOAD(kmeans_update)

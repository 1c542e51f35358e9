// Weighted Gram statistics of resident feature rows in one streaming pass:
//   G = sum_r w_r x_r x_r^T, sx = sum w x, xty = sum w y x, sw = sum w, sy = sum w y,
//   syy = sum w y^2
// for LinearRegression (normal equations), PCA, Correlation and the IRLS step of
// GeneralizedLinearRegression (ops/gram.py::weighted_gram).  Rows are the GLM layout: bf16
// [n, ld] or fp32 [n, ld], ld % 8 == 0, logical width d <= 256.
//
// A Gram matrix is the backward half of the multinomial pass (glm_softmax.hip, R^T X) with R := X:
// every row is shifted and scaled to z = sqrt(w) (x - shift), and the augmented row
// [z | 0 .. | sqrt(w) y | sqrt(w)] of DA = 32 NBA columns (NBA = ceil((d + 2) / 32) <= 9; the
// y and ones columns are the last two) is multiplied with itself, so those columns deliver
// xty and sx (and sy, sw, syy, which the op replaces by fp64 sums over w and y alone: the error
// of an fp32 chain of positive terms would be multiplied by the squared shift) as entries of
// the same product.  The host undoes the shift in fp64.
//
// Tile.  A block of four waves takes 64 rows at a time.  All 256 threads load them (thread
// -> row tid / 4, the 32-B / 16-B chunk tid % 4 of column block k: four lanes read 128
// contiguous bytes of a row), shift and scale in fp32, split every value into bf16 hi + mid
// + lo (each the rounding of the exact remainder) and write the three terms TRANSPOSED into
// LDS, Zt[term][column][row].  The fragment of v_mfma_f32_32x32x16_bf16 for column block b
// (lane (r, h): column 32 b + r, rows 8 h .. + 8 of a 16-row step) is then one 16-B LDS
// read, and it is the A operand and the B operand alike.  Products of total order <= 2
// (hh, hm, mh, hl, lh, mm): the dropped ones are below 2^-25 of |z_i| |z_j|.  bf16 rows go
// the same way -- after the shift and the weight they are no bf16 numbers any more.
//
// The NBA (NBA + 1) / 2 upper tiles of the block triangle are dealt to the four waves in
// contiguous runs of the row-major order (consecutive tiles share their A fragment); X is
// read from HBM once at every NBA.  An fp32 accumulator takes at most kFlushRows rows, then
// it is added into the wave's own fp64 slab (global memory, L2 resident); slabs are summed
// over the blocks in a fixed order by gram_finish_kernel, which also mirrors the lower
// triangle.  No float atomics: the result is a function of (n, d, grid) only.
#include <type_traits>

#include "common.h"

using namespace o3s;

namespace {

typedef float gr_f32x16 __attribute__((ext_vector_type(16)));
typedef short gr_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gr_bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t gr_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kGrWaves = 4;
constexpr int kGrThreads = kGrWaves * kWave;
constexpr int kGrRows = 64;                  // rows per block tile (four MFMA k-steps)
constexpr int kGrTLD = kGrRows + 8;          // 144-B LDS rows: the 16-B fragment reads hit distinct banks
constexpr int kGrFlushTiles = 32;
constexpr int kGrFlushRows = kGrRows * kGrFlushTiles;
constexpr int kGrMaxNBA = 9;

__host__ __device__ constexpr int gr_tiles(int nba) { return nba * (nba + 1) / 2; }
__host__ __device__ constexpr int gr_wave_start(int tiles, int w) { return tiles * w / kGrWaves; }
__host__ __device__ constexpr int gr_wave_tiles(int nba) { return (gr_tiles(nba) + kGrWaves - 1) / kGrWaves; }
// tile t of the row-major upper block triangle -> block row i (in the high half) and block column j
__host__ __device__ constexpr int gr_tile_ij(int nba, int t) {
  int i = 0;
  while (t >= nba - i) {
    t -= nba - i;
    ++i;
  }
  return (i << 8) | (i + t);
}

struct GramBf16 {
  using T = uint16_t;
  using Raw = short8;
  static __device__ __forceinline__ Raw load(const T* p) { return *reinterpret_cast<const short8*>(p); }
  static __device__ __forceinline__ Raw zero() { return Raw{0, 0, 0, 0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ void unpack(const Raw& v, float (&x)[8]) { unpack8(v, x); }
};

struct GramF32 {
  using T = float;
  struct Raw { float4_ a, b; };
  static __device__ __forceinline__ Raw load(const T* p) {
    return Raw{*reinterpret_cast<const float4_*>(p), *reinterpret_cast<const float4_*>(p + 4)};
  }
  static __device__ __forceinline__ Raw zero() { return Raw{float4_{0.f, 0.f, 0.f, 0.f}, float4_{0.f, 0.f, 0.f, 0.f}}; }
  static __device__ __forceinline__ void unpack(const Raw& v, float (&x)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = v.a[j];
      x[4 + j] = v.b[j];
    }
  }
};

// Two fp32 -> one dword of two bf16 (round to nearest even: v_cvt_pk_bf16_f32), a in the low half.
__device__ __forceinline__ uint32_t gr_pk_bf16(float a, float b) {
  float2_ v;
  v[0] = a;
  v[1] = b;
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, gr_bf16x2));
}

// The hi, mid and lo fragments of one column block for one 16-row step.
struct GramFrag {
  gr_bf16x8 h, m, l;
};

// f points at this lane's fragment of column block 0, term hi.
template <int NBA>
__device__ __forceinline__ GramFrag gram_frag(const uint16_t* f, int b) {
  constexpr int DA = 32 * NBA;
  const uint16_t* p = f + 32 * b * kGrTLD;
  return GramFrag{*reinterpret_cast<const gr_bf16x8*>(p), *reinterpret_cast<const gr_bf16x8*>(p + DA * kGrTLD),
                  *reinterpret_cast<const gr_bf16x8*>(p + 2 * DA * kGrTLD)};
}

// Local tile L of a wave whose run starts at tile T0, one 16-row step: acc[L] += Z_i^T Z_j over
// the six products of order <= 2, smallest terms first.  a, b are this tile's fragments; the
// next tile's are read before the MFMAs issue (a row of the triangle keeps its A fragment, a
// diagonal tile's B fragment is its A fragment).
template <int NBA, int T0, int CNT, int L>
__device__ __forceinline__ void gram_tile_steps(const uint16_t* f, gr_f32x16* acc, const GramFrag& a,
                                                const GramFrag& b) {
  constexpr int ij = gr_tile_ij(NBA, T0 + L), ib = ij >> 8;
  GramFrag an = a, bn = b;
  if constexpr (L + 1 < CNT) {
    constexpr int ijn = gr_tile_ij(NBA, T0 + L + 1), ibn = ijn >> 8, jbn = ijn & 255;
    if constexpr (ibn != ib) an = gram_frag<NBA>(f, ibn);
    if constexpr (jbn == ibn) bn = an; else bn = gram_frag<NBA>(f, jbn);
  }
  gr_f32x16 c = acc[L];
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.m, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.h, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.m, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, c, 0, 0, 0);
  acc[L] = c;
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (L + 1 < CNT) gram_tile_steps<NBA, T0, CNT, L + 1>(f, acc, an, bn);
}

// The tiles of wave W over the staged 64 rows.
template <int NBA, int W>
__device__ __forceinline__ void gram_wave_tiles(const uint16_t* Zt, gr_f32x16* acc, int r, int h) {
  constexpr int T = gr_tiles(NBA), T0 = gr_wave_start(T, W), CNT = gr_wave_start(T, W + 1) - T0;
  if constexpr (CNT > 0) {
    constexpr int ij = gr_tile_ij(NBA, T0), ib = ij >> 8, jb = ij & 255;
#pragma unroll 1
    for (int ks = 0; ks < kGrRows / 16; ++ks) {
      const uint16_t* f = Zt + r * kGrTLD + ks * 16 + 8 * h;
      const GramFrag a = gram_frag<NBA>(f, ib);
      const GramFrag b = jb == ib ? a : gram_frag<NBA>(f, jb);
      gram_tile_steps<NBA, T0, CNT, 0>(f, acc, a, b);
    }
  }
}

template <class SRC, int NBA>
__global__ __launch_bounds__(kGrThreads, NBA >= 6 ? 1 : 2) void gram_kernel(
    const typename SRC::T* __restrict__ X, int64_t n, int64_t ld, int d, const float* __restrict__ w,
    const float* __restrict__ y, const float* __restrict__ shift, double* __restrict__ slab) {
  constexpr int DA = 32 * NBA, TW = gr_wave_tiles(NBA);
  __shared__ __attribute__((aligned(16))) uint16_t Zt[3 * DA * kGrTLD];   // [hi, mid, lo][column][row]
  __shared__ __attribute__((aligned(16))) float cs[DA];                    // shift, 0 past d
  __shared__ __attribute__((aligned(16))) uint32_t live[DA];               // all ones below d, else 0
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: the tile switch is a scalar branch
  const int r = lane & 31, h = lane >> 5;
  const int q = threadIdx.x & 3, rho = threadIdx.x >> 2;    // this thread's chunk of a column block, its row of the tile
  for (int c = threadIdx.x; c < DA; c += kGrThreads) {
    cs[c] = c < d ? shift[c] : 0.f;
    live[c] = c < d ? 0xffffffffu : 0u;
  }
  __syncthreads();

  const int64_t ntiles = (n + kGrRows - 1) / kGrRows;
  typename SRC::Raw raw[NBA];
  float wr = 0.f, yr = 0.f;
  auto load = [&](int64_t tile) __attribute__((always_inline)) {
    int64_t row = tile * kGrRows + rho;
    const bool valid = row < n;
    row = valid ? row : n - 1;                      // clamped rows carry weight 0
    wr = valid ? (w ? w[row] : 1.f) : 0.f;
    yr = y ? y[row] : 0.f;
    const typename SRC::T* src = X + row * ld;
#pragma unroll
    for (int k = 0; k < NBA; ++k) {
      const int col0 = 32 * k + 8 * q;              // col0 < d <= ld, both multiples of 8: the chunk is inside the row
      raw[k] = col0 < d ? SRC::load(src + col0) : SRC::zero();
    }
  };
  // where this thread stores column 8 q of block 0, row rho, per term
  uint16_t* const zh = Zt + 8 * q * kGrTLD + rho;
  uint16_t* const zm = zh + DA * kGrTLD;
  uint16_t* const zl = zm + DA * kGrTLD;
  // shift, scale, split and store this thread's chunks transposed
  auto stage = [&]() __attribute__((always_inline)) {
    const float s = sqrtf(wr), sy = s * yr;
#pragma unroll
    for (int k = 0; k < NBA; ++k) {
      const int col0 = 32 * k + 8 * q;
      float x[8], z[8];
      SRC::unpack(raw[k], x);
      const float4_ c0 = *reinterpret_cast<const float4_*>(cs + col0);
      const float4_ c1 = *reinterpret_cast<const float4_*>(cs + col0 + 4);
      const gr_u32x4 m0 = *reinterpret_cast<const gr_u32x4*>(live + col0);
      const gr_u32x4 m1 = *reinterpret_cast<const gr_u32x4*>(live + col0 + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // columns past d read as 0 whatever the storage holds there (their shift is 0)
        const float xl = __uint_as_float(__float_as_uint(x[j]) & (j < 4 ? m0[j] : m1[j - 4]));
        z[j] = (xl - (j < 4 ? c0[j] : c1[j - 4])) * s;
      }
      if (k == NBA - 1 && q == 3) {     // the y and ones columns: DA - 2, DA - 1 (d <= DA - 2)
        z[6] = sy;
        z[7] = s;
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float x0 = z[2 * p], x1 = z[2 * p + 1];
        const uint32_t ph = gr_pk_bf16(x0, x1);
        const float r0 = x0 - __uint_as_float(ph << 16), r1 = x1 - __uint_as_float(ph & 0xffff0000u);
        const uint32_t pm = gr_pk_bf16(r0, r1);
        const uint32_t pl = gr_pk_bf16(r0 - __uint_as_float(pm << 16), r1 - __uint_as_float(pm & 0xffff0000u));
        const int e = (32 * k + 2 * p) * kGrTLD;     // below 64 KB: an immediate offset of the store
        zh[e] = (uint16_t)ph;
        zh[e + kGrTLD] = (uint16_t)(ph >> 16);
        zm[e] = (uint16_t)pm;
        zm[e + kGrTLD] = (uint16_t)(pm >> 16);
        zl[e] = (uint16_t)pl;
        zl[e + kGrTLD] = (uint16_t)(pl >> 16);
      }
      __builtin_amdgcn_sched_barrier(0);   // one chunk's temporaries at a time
    }
  };
  // this wave's slab: [64][TW][16] doubles, a lane's registers contiguous (every slab access is this
  // pointer plus an immediate offset); the finish kernel skips the local tiles a wave does not have
  double* mine = slab + ((int64_t)blockIdx.x * kGrWaves + wid) * (TW * 1024) + lane * (TW * 16);
  // The whole walk of wave W.  Each wave runs its own copy of the loop (the branch on the wave
  // id is scalar and taken once), so its accumulators are the loop-carried values of one plain
  // loop nest; the four copies execute the same barriers the same number of times.
  auto walk = [&](auto wc) __attribute__((always_inline)) {
    constexpr int W = decltype(wc)::value, T = gr_tiles(NBA);
    constexpr int CNT = gr_wave_start(T, W + 1) - gr_wave_start(T, W);
    gr_f32x16 acc[CNT > 0 ? CNT : 1];
    bool first = true;
    int64_t tile = blockIdx.x;
    if (tile < ntiles) load(tile);
    do {                                                      // a block without rows still writes its zeros
#pragma unroll
      for (int l = 0; l < CNT; ++l)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[l][v] = 0.f;
#pragma unroll 1
      for (int c = 0; c < kGrFlushTiles && tile < ntiles; ++c) {
        stage();
        tile += gridDim.x;
        if (tile < ntiles) load(tile);                        // in flight under the MFMAs
        __syncthreads();
        gram_wave_tiles<NBA, W>(Zt, acc, r, h);
        __syncthreads();                                      // fragment reads done before the tile is overwritten
      }
      // one local tile at a time, so that the 16 slab values of a tile are all that is in flight
#pragma unroll
      for (int l = 0; l < CNT; ++l) {
        double* p = mine + l * 16;
        if (first) {
#pragma unroll
          for (int v = 0; v < 16; ++v) p[v] = (double)acc[l][v];
        } else {
#pragma unroll
          for (int v = 0; v < 16; ++v) p[v] += (double)acc[l][v];
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      first = false;
    } while (tile < ntiles);
  };
  switch (wid) {
    case 0: walk(std::integral_constant<int, 0>{}); break;
    case 1: walk(std::integral_constant<int, 1>{}); break;
    case 2: walk(std::integral_constant<int, 2>{}); break;
    default: walk(std::integral_constant<int, 3>{}); break;
  }
}

// GA[i][j] (fp64 [DA, DA], both triangles) = sum over the blocks of their slabs, fixed order.
// Block = 32 slab elements x 32 strided block groups, as glm_finish_kernel.
__global__ __launch_bounds__(1024) void gram_finish_kernel(const double* __restrict__ slab, int nblocks, int nba,
                                                           double* __restrict__ GA) {
  __shared__ double red[32][33];
  const int cx = threadIdx.x & 31, gy = threadIdx.x >> 5;
  const int tw = gr_wave_tiles(nba), tiles = gr_tiles(nba), da = 32 * nba;
  const int64_t per_block = (int64_t)kGrWaves * tw * 1024;
  const int e = blockIdx.x * 32 + cx;                     // < per_block (a multiple of 32)
  double s = 0.0;
  for (int b = gy; b < nblocks; b += 32) s += slab[b * per_block + e];
  red[gy][cx] = s;
  __syncthreads();
  if (gy != 0) return;
  double t = 0.0;
#pragma unroll 8
  for (int g = 0; g < 32; ++g) t += red[g][cx];
  const int wid = e / (tw * 1024), lane = e % (tw * 1024) / (tw * 16), l = (e >> 4) % tw, v = e & 15;
  const int t0 = gr_wave_start(tiles, wid);
  if (l >= gr_wave_start(tiles, wid + 1) - t0) return;    // a wave with fewer tiles than tw
  const int ij = gr_tile_ij(nba, t0 + l), ib = ij >> 8, jb = ij & 255;
  const int i = 32 * ib + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3), j = 32 * jb + (lane & 31);
  if (i > j) return;                                      // a diagonal tile holds both (i, j) and (j, i): keep one,
  GA[(int64_t)i * da + j] = t;                            // so that the result is symmetric to the bit
  GA[(int64_t)j * da + i] = t;
}

template <class SRC>
int launch_gram(int nba, int grid, hipStream_t st, const void* X, int64_t n, int64_t ld, int d, const float* w,
                const float* y, const float* shift, double* slab) {
  const typename SRC::T* Xp = (const typename SRC::T*)X;
  switch (nba) {
#define O3S_GR(NBV) \
  case NBV: hipLaunchKernelGGL((gram_kernel<SRC, NBV>), dim3(grid), dim3(kGrThreads), 0, st, Xp, n, ld, d, w, y, \
                               shift, slab); break;
    O3S_GR(1) O3S_GR(2) O3S_GR(3) O3S_GR(4) O3S_GR(5) O3S_GR(6) O3S_GR(7) O3S_GR(8) O3S_GR(9)
#undef O3S_GR
    default: return -1;
  }
  return 0;
}

}  // namespace

// Sizes for logical width d: da[0] = DA (the fp64 result is [DA, DA]), slab_per_block[0] =
// doubles of slab per block, flush_rows[0] = the most rows an fp32 accumulator takes.
O3S_API int o3s_gram_layout(int d, int* da, int* slab_per_block, int* flush_rows) {
  const int nba = (d + 2 + 31) / 32;
  if (d < 1 || nba > kGrMaxNBA) return -1;
  *da = 32 * nba;
  *slab_per_block = kGrWaves * gr_wave_tiles(nba) * 1024;
  *flush_rows = kGrFlushRows;
  return 0;
}

// One pass: GA (fp64 [DA, DA], DA = 32 ceil((d + 2) / 32)) = Z^T Z of the augmented rows
// Z = [sqrt(w) (x - shift) | 0 .. | sqrt(w) y | sqrt(w)] (DA columns) over the n rows of X (f32 ? float : bf16,
// [n, ld], ld % 8 == 0, ld >= d).  w (fp32 >= 0), y (fp32): null for all ones / all zeros;
// shift: fp32 [d].  slab: fp64 [grid][slab_per_block] (o3s_gram_layout).
O3S_API int o3s_gram(const void* X, int f32, int64_t n, int64_t ld, int d, const float* w, const float* y,
                     const float* shift, double* slab, int grid, double* GA, hipStream_t st) {
  const int nba = (d + 2 + 31) / 32;
  if (d < 1 || d > 256 || ld < d || ld % 8 != 0 || n < 0 || grid <= 0) return -1;
  if (n == 0) {
    if (hipMemsetAsync(GA, 0, sizeof(double) * 32 * nba * 32 * nba, st) != hipSuccess) return (int)hipGetLastError();
    return 0;
  }
  const int rc = f32 ? launch_gram<GramF32>(nba, grid, st, X, n, ld, d, w, y, shift, slab)
                     : launch_gram<GramBf16>(nba, grid, st, X, n, ld, d, w, y, shift, slab);
  if (rc) return rc;
  O3S_CHECK_LAUNCH();
  hipLaunchKernelGGL(gram_finish_kernel, dim3(kGrWaves * gr_wave_tiles(nba) * 32), dim3(1024), 0, st, slab, grid, nba,
                     GA);
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_PRELOAD(gram)

// Squared-Euclidean silhouette coefficient of every stored row in one streaming pass
// (ops/silhouette.py::silhouette_rows).  Rows are the GLM layout: bf16 [n, ld] or fp32 [n, ld],
// ld % 8 == 0, logical width d <= 256.  With the k <= 1024 clusters given by their shifted
// means mu'_j = Y_j / N_j - c, const_j = Psi'_j / N_j (the mean of |x - c|^2 over the cluster,
// +inf for an empty one) and f_j = N_j / (N_j - 1) (0 for N_j <= 1), a row x of cluster ci
// computes, with x' = x - c,
//   dist_j = |x'|^2 + const_j - 2 x' . mu'_j     (the mean squared distance to cluster j)
//   a = dist_ci f_ci,  b = min_{j != ci} dist_j,  s = (b - a) / max(a, b)
// and s = 0 when f_ci = 0 or max(a, b) <= 0.  Every output is a function of its own row only:
// no LDS, no barriers, no atomics, the same bits for any grid.
//
// The product is the one of gmm.hip with the cluster means in place of the whitened
// coordinates: v_mfma_f32_32x32x16_bf16 with A = a block of 32 means (lane (r, h): mean
// 32 cb + r, dims 16 s + 8 h .. + 8) and B = the rows (lane (r, h): row r, the same dims), so a
// lane's 16 accumulators are 16 distances of ONE data row; the own distance is picked and the
// minimum over the others is taken in-lane over the blocks, then exchanged once between the
// lane halves.
//
// Rows.  A wave takes 32 RB rows at a time (RB = 2 up to d = 64, else 1).  Lane (r, h) loads
// the 8-column chunks 16 s + 8 h of its rows, shifts them in fp32, zeroes the columns past d
// and splits every value into bf16 hi + mid + lo; the fragments of all NS = ceil(d / 16) steps
// stay in registers for the whole walk over the means (12 RB NS VGPRs).  bf16 rows go the same
// way: after the shift they are no bf16 numbers any more.
//
// Means.  The host splits mu' (fp64 -> fp32) into the same three bf16 terms and stores them in
// fragment order, Mp[cb][s][term][lane][8], zero-padded to 32 ceil(k / 32) means: a fragment is
// one coalesced 1-KB load; the whole table is at most 1.5 MB and stays in L2.  Products of
// total order <= 2 are kept (hh, hm, mh, hl, lh, mm); the dropped ones are below 2^-25 of
// |mu'| |x'|.  Padding means have const = +inf and never win the minimum.
#include "common.h"

using namespace o3s;

namespace {

typedef float sil_f32x16 __attribute__((ext_vector_type(16)));
typedef short sil_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sil_bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kSilWaves = 4;
constexpr int kSilThreads = kSilWaves * kWave;
constexpr int kSilMaxNS = 16;                 // d <= 256
constexpr int kSilMaxK = 1024;
constexpr int kSilFrag = 3 * 64 * 8;          // bf16 elements of one split fragment (hi, mid, lo)

__host__ __device__ constexpr int sil_rb(int ns) { return ns <= 4 ? 2 : 1; }

struct SilBf16 {
  using T = uint16_t;
  static __device__ __forceinline__ void load(const T* p, float (&x)[8]) {
    unpack8(*reinterpret_cast<const short8*>(p), x);
  }
};

struct SilF32 {
  using T = float;
  static __device__ __forceinline__ void load(const T* p, float (&x)[8]) {
    const float4_ a = *reinterpret_cast<const float4_*>(p), b = *reinterpret_cast<const float4_*>(p + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = a[j];
      x[4 + j] = b[j];
    }
  }
};

// Two fp32 -> one dword of two bf16 (round to nearest even: v_cvt_pk_bf16_f32), a in the low half.
__device__ __forceinline__ uint32_t sil_pk_bf16(float a, float b) {
  float2_ v;
  v[0] = a;
  v[1] = b;
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, sil_bf16x2));
}

struct SilFrag {
  sil_bf16x8 h, m, l;
};

// z[8] -> its hi, mid and lo fragments (each the rounding of the exact remainder)
__device__ __forceinline__ SilFrag sil_split(const float (&z)[8]) {
  uint32_t ph[4], pm[4], pl[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = z[2 * p], x1 = z[2 * p + 1];
    ph[p] = sil_pk_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(ph[p] << 16), r1 = x1 - __uint_as_float(ph[p] & 0xffff0000u);
    pm[p] = sil_pk_bf16(r0, r1);
    pl[p] = sil_pk_bf16(r0 - __uint_as_float(pm[p] << 16), r1 - __uint_as_float(pm[p] & 0xffff0000u));
  }
  SilFrag f;
  __builtin_memcpy(&f.h, ph, 16);
  __builtin_memcpy(&f.m, pm, 16);
  __builtin_memcpy(&f.l, pl, 16);
  return f;
}

template <class SRC, int NS>
__global__ __launch_bounds__(kSilThreads, NS <= 8 ? 2 : 1) void silhouette_kernel(
    const typename SRC::T* __restrict__ X, int64_t n, int64_t ld, int d, int kb, const int* __restrict__ cid,
    const float* __restrict__ shift, const uint16_t* __restrict__ Mp, const float* __restrict__ cst,
    const float* __restrict__ fj, float* __restrict__ out) {
  constexpr int RB = sil_rb(NS), TR = 32 * RB;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int64_t ntiles = (n + TR - 1) / TR;
  const int64_t nwaves = (int64_t)gridDim.x * kSilWaves;
  const float inf = __builtin_inff();
  for (int64_t tile = (int64_t)blockIdx.x * kSilWaves + wid; tile < ntiles; tile += nwaves) {
    // ---- this lane's chunks of its RB rows: shift, mask, split; |x'|^2 of the row
    SilFrag xf[RB][NS];
    int64_t row[RB];
    bool valid[RB];
    int ci[RB];
    float xx[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      row[rb] = tile * TR + 32 * rb + r;
      valid[rb] = row[rb] < n;
      const int64_t rr = valid[rb] ? row[rb] : n - 1;                    // clamped rows are not stored
      const typename SRC::T* src = X + rr * ld;
      ci[rb] = cid[rr];
      float q = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int col0 = 16 * s + 8 * h;      // col0 < d <= ld, both multiples of 8: the chunk is inside the row
        float x[8], z[8];
        if (col0 < d) {
          SRC::load(src + col0, x);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = 0.f;
        }
        const float4_ c0 = *reinterpret_cast<const float4_*>(shift + col0);   // shift: 16 NS floats, 0 past d
        const float4_ c1 = *reinterpret_cast<const float4_*>(shift + col0 + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) {  // columns past d read as 0 whatever the storage holds there
          z[j] = col0 + j < d ? x[j] - (j < 4 ? c0[j] : c1[j - 4]) : 0.f;
          q = fmaf(z[j], z[j], q);
        }
        xf[rb][s] = sil_split(z);
      }
      xx[rb] = q + __shfl_xor(q, 32, 64);     // the other half of every 16-column step
    }
    // ---- the walk over the blocks of 32 means
    float own[RB], bmin[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) own[rb] = bmin[rb] = inf;
    const uint16_t* mk = Mp + lane * 8;
    const float* ck = cst + 4 * h;
#pragma unroll 1
    for (int cb = 0; cb < kb; ++cb, mk += NS * kSilFrag, ck += 32) {
      // register v of the accumulator is mean 32 cb + 8 (v >> 2) + 4 h + (v & 3)
      sil_f32x16 acc[RB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[rb][v] = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const uint16_t* p = mk + s * kSilFrag;
        const sil_bf16x8 wh = *reinterpret_cast<const sil_bf16x8*>(p);
        const sil_bf16x8 wm = *reinterpret_cast<const sil_bf16x8*>(p + 512);
        const sil_bf16x8 wl = *reinterpret_cast<const sil_bf16x8*>(p + 1024);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          sil_f32x16 c = acc[rb];
          const SilFrag& x = xf[rb][s];
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, x.m, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, x.h, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, x.l, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, x.h, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, x.m, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, x.h, c, 0, 0, 0);
          acc[rb] = c;
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4_ c4 = *reinterpret_cast<const float4_*>(ck + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int mean = 32 * cb + 8 * g + 4 * h + j;
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            const float dist = fmaf(-2.f, acc[rb][4 * g + j], xx[rb] + c4[j]);
            if (mean == ci[rb]) own[rb] = dist;
            else bmin[rb] = fminf(bmin[rb], dist);
          }
        }
      }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      // the own distance sits in one lane half (the other holds +inf), the minimum in both
      const float o = fminf(own[rb], __shfl_xor(own[rb], 32, 64));
      const float b = fminf(bmin[rb], __shfl_xor(bmin[rb], 32, 64));
      const bool known = ci[rb] >= 0 && ci[rb] < 32 * kb;      // an id outside the table reads nothing
      const float f = known ? fj[ci[rb]] : 0.f;
      const float a = o * f;
      const float m = fmaxf(a, b);
      const float sv = (f != 0.f && m > 0.f) ? (b - a) / m : 0.f;
      if (valid[rb] && h == 0) out[row[rb]] = sv;
    }
  }
}

template <class SRC>
int launch_sil(int ns, int grid, hipStream_t st, const void* X, int64_t n, int64_t ld, int d, int kb, const int* cid,
               const float* shift, const uint16_t* Mp, const float* cst, const float* fj, float* out) {
  const typename SRC::T* Xp = (const typename SRC::T*)X;
  switch (ns) {
#define O3S_SIL(NSV) \
  case NSV: hipLaunchKernelGGL((silhouette_kernel<SRC, NSV>), dim3(grid), dim3(kSilThreads), 0, st, Xp, n, ld, d, kb, \
                               cid, shift, Mp, cst, fj, out); break;
    O3S_SIL(1) O3S_SIL(2) O3S_SIL(3) O3S_SIL(4) O3S_SIL(5) O3S_SIL(6) O3S_SIL(7) O3S_SIL(8)
    O3S_SIL(9) O3S_SIL(10) O3S_SIL(11) O3S_SIL(12) O3S_SIL(13) O3S_SIL(14) O3S_SIL(15) O3S_SIL(16)
#undef O3S_SIL
    default: return -1;
  }
  return 0;
}

}  // namespace

// Sizes for logical width d and k clusters: ns[0] = 16-column steps (the shift is 16 ns floats,
// zero past d), kp[0] = 32 ceil(k / 32) padded means (const and f are kp floats), m_elems[0] =
// bf16 elements of the split means Mp[kp / 32][ns][3][64][8], tile_rows[0] = rows one wave takes
// at a time.  -1: a width or a cluster count the kernel does not take.
O3S_API int o3s_silhouette_layout(int d, int k, int* ns, int* kp, int64_t* m_elems, int* tile_rows) {
  const int s = (d + 15) / 16;
  if (d < 1 || s > kSilMaxNS || k < 2 || k > kSilMaxK) return -1;
  const int kb = (k + 31) / 32;
  *ns = s;
  *kp = 32 * kb;
  *m_elems = (int64_t)kb * s * kSilFrag;
  *tile_rows = 32 * sil_rb(s);
  return 0;
}

// One pass over the n rows of X (f32 ? float : bf16, [n, ld], ld % 8 == 0, ld >= d): out (fp32
// [n]) = the silhouette coefficient of every row, for cluster ids cid (int32 [n], in [0, k)),
// the shift (fp32 [16 ns], zero past d), the split shifted means Mp, const and f (fp32 [kp];
// o3s_silhouette_layout).  grid blocks of four waves.
O3S_API int o3s_silhouette(const void* X, int f32, int64_t n, int64_t ld, int d, int k, const int* cid,
                           const float* shift, const void* Mp, const float* cst, const float* fj, float* out,
                           int grid, hipStream_t st) {
  const int ns = (d + 15) / 16;
  if (d < 1 || ns > kSilMaxNS || k < 2 || k > kSilMaxK || ld < d || ld % 8 != 0 || n < 0 || grid <= 0) return -1;
  if (n == 0) return 0;
  const int kb = (k + 31) / 32;
  const int rc = f32 ? launch_sil<SilF32>(ns, grid, st, X, n, ld, d, kb, cid, shift, (const uint16_t*)Mp, cst, fj, out)
                     : launch_sil<SilBf16>(ns, grid, st, X, n, ld, d, kb, cid, shift, (const uint16_t*)Mp, cst, fj, out);
  if (rc) return rc;
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_PRELOAD(silhouette)

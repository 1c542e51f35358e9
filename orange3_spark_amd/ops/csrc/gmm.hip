// E-step of a Gaussian mixture over resident feature rows in one streaming pass
// (ops/gmm.py::estep).  Rows are the GLM layout: bf16 [n, ld] or fp32 [n, ld], ld % 8 == 0,
// logical width d <= 256.  For K <= 64 components given as whitening matrices W_k = L_k^-1
// (lower triangular), offsets b_k = W_k (mu_k - c) and constants a_k, every row x computes
//   z_k = W_k (x - c) - b_k,  lp_k = a_k - |z_k|^2 / 2,  lse = logsumexp_k lp_k,
//   resp[k] = exp(lp_k - lse) (times the row weight, if given)
// and writes resp component-major [K, n] (resp[k] is the weight vector of the Gram pass of
// component k) and lse [n].  Every output is a function of its own row only: no slabs, no
// atomics, the same bits for any grid.
//
// The product is the forward half of the multinomial pass (glm_softmax.hip) with the K d whitened
// coordinates as classes, on v_mfma_f32_32x32x16_bf16 with A = a block of W (lane (r, h):
// coordinate 32 cb + r, dims 16 s + 8 h .. + 8) and B = the rows (lane (r, h): row r, the same
// dims), so a lane's 16 accumulators are 16 coordinates of ONE data row and |z|^2 is an
// in-lane sum plus one exchange between the lane halves.
//
// Rows.  A wave takes 32 RB rows at a time (RB = 2 up to d = 64, else 1) and nothing is
// shared between waves: no LDS, no barriers.  Lane (r, h) loads the 8-column chunks 16 s + 8 h
// of its rows, shifts them in fp32 (c: the op's per-column shift), zeroes the columns past d
// and splits every value into bf16 hi + mid + lo (each the rounding of the exact remainder);
// the three fragments of all NS = ceil(d / 16) steps stay in registers for the whole walk over
// the components (12 RB NS VGPRs).  bf16 rows go the same way: after the shift they are no
// bf16 numbers any more.
//
// Coefficients.  The host splits W (fp64) into the same three bf16 terms and stores them in
// fragment order, Wp[k][cb][s][term][lane][8]: a fragment is one coalesced 1-KB load, its
// address the component's base plus a compile-time offset.  Coordinate block cb only needs
// the dims below 32 (cb + 1) -- W is lower triangular -- so its steps s >= 2 cb + 2 are never
// read.  Products of total order <= 2 are kept (hh, hm, mh, hl, lh, mm), as in gram.hip: the
// dropped ones are below 2^-25 of |w| |x - c|.  The accumulator starts at -b.
//
// Log-sum-exp.  lp_k goes into resp[k] while a running maximum is kept per row; two more
// sweeps over the K values of the tile (the lane reads back its own stores, L2-hot) turn them
// into exp(lp_k - max) and their sum, then into responsibilities.
#include "common.h"

using namespace o3s;

namespace {

typedef float gm_f32x16 __attribute__((ext_vector_type(16)));
typedef short gm_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gm_bf16x2 __attribute__((ext_vector_type(2)));

constexpr int kGmWaves = 4;
constexpr int kGmThreads = kGmWaves * kWave;
constexpr int kGmMaxNS = 16;                 // d <= 256
constexpr int kGmMaxK = 64;
constexpr int kGmFrag = 3 * 64 * 8;          // bf16 elements of one split fragment (hi, mid, lo)

__host__ __device__ constexpr int gm_ncb(int ns) { return (ns + 1) / 2; }
// 16-dim steps coordinate block cb needs: the dims below 32 (cb + 1)
__host__ __device__ constexpr int gm_steps(int ns, int cb) { return 2 * cb + 2 < ns ? 2 * cb + 2 : ns; }
__host__ __device__ constexpr int gm_rb(int ns) { return ns <= 4 ? 2 : 1; }

struct GmmBf16 {
  using T = uint16_t;
  static __device__ __forceinline__ void load(const T* p, float (&x)[8]) {
    unpack8(*reinterpret_cast<const short8*>(p), x);
  }
};

struct GmmF32 {
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
__device__ __forceinline__ uint32_t gm_pk_bf16(float a, float b) {
  float2_ v;
  v[0] = a;
  v[1] = b;
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, gm_bf16x2));
}

struct GmmFrag {
  gm_bf16x8 h, m, l;
};

// z[8] -> its hi, mid and lo fragments
__device__ __forceinline__ GmmFrag gm_split(const float (&z)[8]) {
  uint32_t ph[4], pm[4], pl[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = z[2 * p], x1 = z[2 * p + 1];
    ph[p] = gm_pk_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(ph[p] << 16), r1 = x1 - __uint_as_float(ph[p] & 0xffff0000u);
    pm[p] = gm_pk_bf16(r0, r1);
    pl[p] = gm_pk_bf16(r0 - __uint_as_float(pm[p] << 16), r1 - __uint_as_float(pm[p] & 0xffff0000u));
  }
  GmmFrag f;
  __builtin_memcpy(&f.h, ph, 16);
  __builtin_memcpy(&f.m, pm, 16);
  __builtin_memcpy(&f.l, pl, 16);
  return f;
}

template <class SRC, int NS>
__global__ __launch_bounds__(kGmThreads, NS <= 8 ? 2 : 1) void gmm_estep_kernel(
    const typename SRC::T* __restrict__ X, int64_t n, int64_t ld, int d, int K, const uint16_t* __restrict__ Wp,
    const float* __restrict__ bp, const float* __restrict__ ak, const float* __restrict__ shift,
    const float* __restrict__ w, float* resp, float* __restrict__ lse) {
  constexpr int NCB = gm_ncb(NS), RB = gm_rb(NS), TR = 32 * RB;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wid = threadIdx.x >> 6;
  const int64_t ntiles = (n + TR - 1) / TR;
  const int64_t nwaves = (int64_t)gridDim.x * kGmWaves;
  for (int64_t tile = (int64_t)blockIdx.x * kGmWaves + wid; tile < ntiles; tile += nwaves) {
    // ---- this lane's chunks of its RB rows: shift, mask, split
    GmmFrag xf[RB][NS];
    int64_t row[RB];
    bool valid[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      row[rb] = tile * TR + 32 * rb + r;
      valid[rb] = row[rb] < n;
      const typename SRC::T* src = X + (valid[rb] ? row[rb] : n - 1) * ld;    // clamped rows are not stored
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
        for (int j = 0; j < 8; ++j)    // columns past d read as 0 whatever the storage holds there
          z[j] = col0 + j < d ? x[j] - (j < 4 ? c0[j] : c1[j - 4]) : 0.f;
        xf[rb][s] = gm_split(z);
      }
    }
    // ---- the walk over the components
    float mx[RB];
    const uint16_t* wk = Wp + lane * 8;
    const float* bk = bp + 4 * h;
#pragma unroll 1
    for (int k = 0; k < K; ++k, wk += NCB * NS * kGmFrag, bk += 32 * NCB) {
      float sq[RB];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) sq[rb] = 0.f;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        // register v of the accumulator is coordinate 32 cb + 8 (v >> 2) + 4 h + (v & 3)
        gm_f32x16 acc[RB];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4_ b4 = *reinterpret_cast<const float4_*>(bk + 32 * cb + 8 * g);
#pragma unroll
          for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[rb][4 * g + j] = -b4[j];
        }
#pragma unroll
        for (int s = 0; s < gm_steps(NS, cb); ++s) {
          const uint16_t* p = wk + (cb * NS + s) * kGmFrag;
          const gm_bf16x8 wh = *reinterpret_cast<const gm_bf16x8*>(p);
          const gm_bf16x8 wm = *reinterpret_cast<const gm_bf16x8*>(p + 512);
          const gm_bf16x8 wl = *reinterpret_cast<const gm_bf16x8*>(p + 1024);
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            gm_f32x16 c = acc[rb];
            const GmmFrag& x = xf[rb][s];
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
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
          for (int v = 0; v < 16; ++v) sq[rb] = fmaf(acc[rb][v], acc[rb][v], sq[rb]);
      }
      // a_k = hi + lo: rounded to one float it would shift every row of the component the same
      // way, an error that adds up over the rows in the log-likelihood instead of averaging out
      const float ahi = ak[2 * k], alo = ak[2 * k + 1];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const float q = sq[rb] + __shfl_xor(sq[rb], 32, 64);     // the other 16 coordinates of every block
        const float lp = ahi + fmaf(-0.5f, q, alo);
        mx[rb] = k == 0 ? lp : fmaxf(mx[rb], lp);
        if (valid[rb] && h == 0) resp[(int64_t)k * n + row[rb]] = lp;
      }
    }
    // ---- lp -> responsibilities: p_k = exp(lp_k - max), their sum s in the order of k, then
    // p_k / s -- dividing by the very sum of the stored p_k keeps a row's sum within K 2^-24 of 1,
    // which exp(lp_k - lse) does not (lse rounds at 2^-24 |lse|)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      if (!(valid[rb] && h == 0)) continue;
      float* const p0 = resp + row[rb];
      float s = 0.f;
      float* p = p0;
      for (int k = 0; k < K; ++k, p += n) {
        const float e = expf(*p - mx[rb]);
        *p = e;
        s += e;
      }
      lse[row[rb]] = mx[rb] + logf(s);
      const float wr = w ? w[row[rb]] : 1.f;
      p = p0;
      for (int k = 0; k < K; ++k, p += n) *p = *p / s * wr;
    }
  }
}

template <class SRC>
int launch_gmm(int ns, int grid, hipStream_t st, const void* X, int64_t n, int64_t ld, int d, int K,
               const uint16_t* Wp, const float* bp, const float* ak, const float* shift, const float* w, float* resp,
               float* lse) {
  const typename SRC::T* Xp = (const typename SRC::T*)X;
  switch (ns) {
#define O3S_GM(NSV) \
  case NSV: hipLaunchKernelGGL((gmm_estep_kernel<SRC, NSV>), dim3(grid), dim3(kGmThreads), 0, st, Xp, n, ld, d, K, Wp, \
                               bp, ak, shift, w, resp, lse); break;
    O3S_GM(1) O3S_GM(2) O3S_GM(3) O3S_GM(4) O3S_GM(5) O3S_GM(6) O3S_GM(7) O3S_GM(8)
    O3S_GM(9) O3S_GM(10) O3S_GM(11) O3S_GM(12) O3S_GM(13) O3S_GM(14) O3S_GM(15) O3S_GM(16)
#undef O3S_GM
    default: return -1;
  }
  return 0;
}

}  // namespace

// Sizes for logical width d and k components: ns[0] = 16-column steps (the shift is 16 ns
// floats, zero past d), dp[0] = padded coordinates per component (b is [k, dp] floats, zero
// past d), w_elems[0] = bf16 elements of the split coefficients Wp[k][dp / 32][ns][3][64][8],
// tile_rows[0] = rows one wave takes at a time.
O3S_API int o3s_gmm_layout(int d, int k, int* ns, int* dp, int64_t* w_elems, int* tile_rows) {
  const int s = (d + 15) / 16;
  if (d < 1 || s > kGmMaxNS || k < 1 || k > kGmMaxK) return -1;
  *ns = s;
  *dp = 32 * gm_ncb(s);
  *w_elems = (int64_t)k * gm_ncb(s) * s * kGmFrag;
  *tile_rows = 32 * gm_rb(s);
  return 0;
}

// One pass over the n rows of X (f32 ? float : bf16, [n, ld], ld % 8 == 0, ld >= d): resp (fp32
// [K, n]) and lse (fp32 [n]) of the mixture given by Wp, bp (o3s_gmm_layout), ak (fp32 [K, 2]:
// a_k as hi + lo) and the shift (fp32 [16 ns], zero past d).  w (fp32 [n], >= 0): null for all ones.  grid blocks of four waves.
O3S_API int o3s_gmm_estep(const void* X, int f32, int64_t n, int64_t ld, int d, int K, const void* Wp,
                          const float* bp, const float* ak, const float* shift, const float* w, float* resp,
                          float* lse, int grid, hipStream_t st) {
  const int ns = (d + 15) / 16;
  if (d < 1 || ns > kGmMaxNS || K < 1 || K > kGmMaxK || ld < d || ld % 8 != 0 || n < 0 || grid <= 0) return -1;
  if (n == 0) return 0;
  const int rc = f32 ? launch_gmm<GmmF32>(ns, grid, st, X, n, ld, d, K, (const uint16_t*)Wp, bp, ak, shift, w, resp, lse)
                     : launch_gmm<GmmBf16>(ns, grid, st, X, n, ld, d, K, (const uint16_t*)Wp, bp, ak, shift, w, resp, lse);
  if (rc) return rc;
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_PRELOAD(gmm)

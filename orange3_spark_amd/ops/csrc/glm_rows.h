// Device building blocks of the generalised-linear-model streaming kernels (gfx950): what
// every pass of glm_grad.hip, glm_mixed.hip, glm_stats.hip and glm_softmax.hip shares.
//
// The kernels replace the per-partition gradient closure that Spark MLlib runs inside
// `treeAggregate` for LogisticRegression / LinearSVC / LinearRegression (reached in
// the reference through OWSparkEstimator.apply -> `fit`,
// orangecontrib/spark/base/spark_ml_estimator.py:19-25).
//
// Layout: X is a row-major bf16 matrix [n, ld] (ld % 8 == 0, zero padded).  A row
// is split over LPR lanes ("row group"); lane c of a group owns the 16-B chunks
// c, c+LPR, ... (CPL chunks).  A wave therefore streams 64/LPR consecutive rows per
// `global_load_dwordx4` -- for D = 256 that is two rows per wave-instruction, 1 KiB
// contiguous -- and the gradient  X^T r  is lane-local (each lane always touches
// the same 8*CPL columns), so only the per-row dot product needs a cross-lane sum.
//
// Cross-block reduction: one fp32 slab row per block + `glm_finish` (glm_launch.h; fp64, fixed
// order) -> bitwise deterministic results, no float atomics (Guideline 12).
//
// SRC == 1 ("synthetic lineage"): instead of loading a chunk, the lane regenerates
// it from the counter hash used by `synth_glm_kernel` (glm_stats.hip), so rows that did not fit
// in HBM are recomputed from lineage on every pass -- the MI355X equivalent of Spark's
// MEMORY_ONLY caching, where evicted partitions are recomputed.  Regenerated and
// materialised rows are bit-identical.
//
// Everything here sits in an anonymous namespace: each unit that includes the header holds
// its own copy, and only the O3S_API entry points are exported.
// The tile bodies of the .hip files are register-tuned around these helpers as they stand (see
// the notes at grad_epilogue, RowsLineage and in the kernels): a change here is checked with
// tools/isa_diff.py against the build before it.
#pragma once
#include "common.h"

using namespace o3s;

namespace {

enum { LOSS_LOGISTIC = 0, LOSS_HINGE = 1, LOSS_SQUARED = 2 };

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;

// Synthetic features: word i = mix24(fk + i * 0x9E3779) of the row's feature key fk
// supplies the four features 4i..4i+3, one per byte b: x = (2b - 255) / 256, i.e. 256
// symmetric levels in (-1, 1) (mean 0, var ~1/3), every one EXACT in bf16 (<= 8
// significant bits).  Exactness lets the lineage pass skip the bf16 round trip: it
// decodes a byte with one v_cvt_f32_ubyteN and folds the affine map into the weights
// (see glm_grad_kernel, glm_grad.hip), two hashes per 16-B chunk.
//
// mix24 is a bijective 32-bit mixer built from full-rate VALU ops only: two
// v_mad_u32_u24 steps h <- (h mod 2^24) * C + h (a bijection for even C: the low 24 bits
// are multiplied by the odd C + 1, the top byte is recovered from the carry) between
// xorshifts -- 5 issue cycles per word, vs 13 for murmur's fmix32 whose two
// v_mul_lo_u32 are quarter rate.  On byte-uniformity (chi^2), cross-column correlation
// and word-uniqueness tests it matches fmix32 (see ops/glm.py::_mix24, the torch twin).
__host__ __device__ __forceinline__ uint32_t umad24(uint32_t a, uint32_t c, uint32_t add) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(a, c) + add;
#else
  return (a & 0xFFFFFFu) * c + add;
#endif
}
__host__ __device__ __forceinline__ uint32_t mix24(uint32_t h) {
  h ^= h >> 16;
  h = umad24(h, 0xED5AD4u, h);
  h ^= h >> 15;
  return umad24(h, 0x2C1B3Cu, h);
}
// Feature key of global row `row` (labels use the murmur row_key of common.h).
__device__ __forceinline__ uint32_t feat_key(uint32_t seed, int64_t row) {
  const uint32_t lo = (uint32_t)(row & 0xffffffffll);
  const uint32_t hi = (uint32_t)((uint64_t)row >> 32);
  return mix24(mix24(lo + seed * 0x9E3779B1u) ^ umad24(hi, 0x7FEB35u, 0x165667u));
}
__device__ __forceinline__ uint32_t synth_word(uint32_t fk, int i) {
  return mix24(umad24((uint32_t)i, 0x9E3779u, fk));
}
__device__ __forceinline__ float synth_byte(uint32_t h, int q) {
  return (float)((h >> (8 * q)) & 0xffu);     // -> v_cvt_f32_ubyte{q}
}
constexpr float kSynthScale = 1.0f / 128.0f, kSynthShift = -255.0f / 256.0f;
// One 16-B chunk (8 features) of synthetic row `rk` at chunk index ch, as bf16.
__device__ __forceinline__ short8 synth_chunk(uint32_t fk, int ch) {
  short8 v;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint32_t h = synth_word(fk, 2 * ch + p);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      v[4 * p + q] = (short)f32_to_bf16(fmaf(synth_byte(h, q), kSynthScale, kSynthShift));
  }
  return v;
}
// Label draw for a synthetic row: y ~ Bernoulli(sigmoid(margin_true)).
__device__ __forceinline__ float synth_label(uint32_t rk, float margin_true) {
  const float u = (float)(fmix32(rk ^ 0xA511E9B3u) >> 8) * (1.0f / 16777216.0f);
  return u < sigmoidf(margin_true) ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------------------
// "Transpose" reduction of U per-row partial sums over the LPR lanes of a row group.
// A butterfly would cost U*log2(LPR) cross-lane ops; recursive halving costs
// U/2 + U/4 + ... + (remaining butterfly) -- for LPR=32, U=8: 9 instead of 40 -- and
// leaves every lane with the COMPLETE sums of NF = U >> H consecutive rows
// (H = min(log2 U, log2 LPR)), so the per-row epilogue (sigmoid, loss) runs once per
// row instead of once per lane-row.
constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x / 2); }

template <int LPR, int U>
struct RowReduce {
  static constexpr int LL = ilog2(LPR), LU = ilog2(U);
  static constexpr int H = LL < LU ? LL : LU;   // halving steps
  static constexpr int NF = U >> H;             // rows finished per lane
  // first row index owned by group-lane c
  __device__ static __forceinline__ int base(int c) {
    int b = 0;
#pragma unroll
    for (int s = 0; s < H; ++s) b += ((c >> (LL - 1 - s)) & 1) * (U >> (s + 1));
    return b;
  }
  // group-lane holding row u (lower, butterflied bits zero)
  __host__ __device__ static constexpr int owner(int u) {
    int c = 0;
    for (int s = 0; s < H; ++s) c += (((u - u % NF) >> (LU - 1 - s)) & 1) << (LL - 1 - s);
    return c;
  }
  // true for exactly one lane per finished row
  __device__ static __forceinline__ bool representative(int c) {
    return (c & ((1 << (LL - H)) - 1)) == 0;
  }
  __device__ static __forceinline__ void run(float (&v)[U], int c) {
    int n = U;
#pragma unroll
    for (int s = 0; s < LL; ++s) {
      const int off = LPR >> (s + 1);
      if (s < H) {
        const bool up = (c & off) != 0;
        n >>= 1;
#pragma unroll
        for (int j = 0; j < U / 2; ++j) {
          if (j < n) {
            const float keep = up ? v[j + n] : v[j];
            const float send = up ? v[j] : v[j + n];
            v[j] = keep + __shfl_xor(send, off, kWave);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < NF; ++j) v[j] += __shfl_xor(v[j], off, kWave);
      }
    }
  }
};

// ---------------------------------------------------------------------------
// Row sources.  Every tile body (grad_tile in glm_mixed.hip; stats_tile, margin_body and
// colstats_body in glm_stats.hip) is written once and instantiated per source; a
// source owns the registers of one 8-column chunk (`chunk`), how they are filled (`load`)
// and how they become eight floats (`unpack`).
//   * The memory sources take CLAMPED row / chunk indices and load unconditionally; the
//     caller masks in registers (`mask`).  A per-load `ok ? load : 0` makes hipcc branch
//     around every load and serialise them (CDNA guide §5, "three .s-level traps" (c)).
//   * `pin` keeps the packed registers live across the row reduction, so that X^T r unpacks
//     them again instead of holding 8 floats per chunk (halves the VGPR footprint).  fp32
//     rows are held unpacked, once: nothing to pin.
//   * Lineage rows are the raw bytes b of the hash (x = b*kSynthScale + kSynthShift): the
//     affine map is folded into the dot product (`dot`, with wshift = kSynthShift * sum w
//     over the lane's columns) and into X^T r (`resid`: r*b/128 plus a per-lane residual
//     sum rs, corrected once at the end).  Rows past n are harmless (their weight is 0) and
//     columns past ld meet zero weights and are never written out: no masking.
struct MemoryRows {
  static constexpr bool kLineage = false;
  __device__ static __forceinline__ float dot(float d, float) { return d; }
  __device__ static __forceinline__ float resid(float r, float&) { return r; }
};
struct RowsBf16 : MemoryRows {          // bf16 [n, ld] in memory, 16-B chunks
  using elem = uint16_t;
  using chunk = short8;
  __device__ static __forceinline__ void load(const elem* __restrict__ X, int64_t ld, int64_t rowc, int chc,
                                              chunk& v) {
    v = __builtin_nontemporal_load(reinterpret_cast<const short8*>(X + rowc * ld + 8 * chc));
  }
  __device__ static __forceinline__ void mask(chunk& v, bool keep) {
    v = keep ? v : short8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  // the predict path's form: a plain load under its own guard
  __device__ static __forceinline__ void load_if(const elem* __restrict__ X, int64_t ld, int64_t row, int ch,
                                                 bool ok, chunk& v) {
    v = ok ? *reinterpret_cast<const short8*>(X + row * ld + 8 * ch) : short8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  __device__ static __forceinline__ void unpack(const chunk& v, float (&x)[8]) { unpack8(v, x); }
  __device__ static __forceinline__ void pin(chunk& v) { asm volatile("" : "+v"(v)); }
};
struct RowsF32 : MemoryRows {           // float [n, ld] in memory, 32-B chunks (two 16-B loads)
  using elem = float;
  struct chunk { float4_ lo, hi; };
  __device__ static __forceinline__ void load(const elem* __restrict__ X, int64_t ld, int64_t rowc, int chc,
                                              chunk& v) {
    const float4_* p = reinterpret_cast<const float4_*>(X + rowc * ld + 8 * chc);
    v.lo = __builtin_nontemporal_load(p);
    v.hi = __builtin_nontemporal_load(p + 1);
  }
  __device__ static __forceinline__ void mask(chunk& v, bool keep) {
    v.lo = keep ? v.lo : float4_{0.f, 0.f, 0.f, 0.f};
    v.hi = keep ? v.hi : float4_{0.f, 0.f, 0.f, 0.f};
  }
  __device__ static __forceinline__ void load_if(const elem* __restrict__ X, int64_t ld, int64_t row, int ch,
                                                 bool ok, chunk& v) {
    const float4_* p = reinterpret_cast<const float4_*>(X + row * ld + 8 * ch);
    v.lo = ok ? p[0] : float4_{0.f, 0.f, 0.f, 0.f};
    v.hi = ok ? p[1] : float4_{0.f, 0.f, 0.f, 0.f};
  }
  __device__ static __forceinline__ void unpack(const chunk& v, float (&x)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = v.lo[j];
      x[4 + j] = v.hi[j];
    }
  }
  __device__ static __forceinline__ void pin(chunk&) {}
};
// (Two ways in: stats_tile (glm_stats.hip) regenerates a chunk where it is used, load(fk, ch);
// grad_tile (glm_mixed.hip) forms the two hash words itself and calls decode -- with the chunk
// index passed through
// load, hipcc simplifies 2*ch and 2*ch+1 inside it first and the lineage hash of the mixed
// kernel comes out with different adds and registers.)
struct RowsLineage {                    // regenerated from the row's feature key
  using elem = uint16_t;                // (of the X argument the tile bodies share; never read)
  static constexpr bool kLineage = true;
  struct chunk { float b[8]; };
  __device__ static __forceinline__ void load(uint32_t fk, int ch, chunk& v) {
    decode(synth_word(fk, 2 * ch), synth_word(fk, 2 * ch + 1), v);
  }
  __device__ static __forceinline__ void decode(uint32_t h0, uint32_t h1, chunk& v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v.b[j] = synth_byte(h0, j);
      v.b[4 + j] = synth_byte(h1, j);
    }
  }
  __device__ static __forceinline__ void unpack(const chunk& v, float (&x)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = v.b[j];
  }
  // the feature values themselves (exact: no bf16 round trip)
  __device__ static __forceinline__ void values(const chunk& v, float (&x)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = fmaf(v.b[j], kSynthScale, kSynthShift);
  }
  __device__ static __forceinline__ void pin(chunk& v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(v.b[j]));
  }
  __device__ static __forceinline__ float dot(float d, float wshift) { return fmaf(d, kSynthScale, wshift); }
  __device__ static __forceinline__ float resid(float r, float& rs) {
    rs += r;
    return r * kSynthScale;
  }
};

template <int LOSS>
__device__ __forceinline__ void loss_terms(float m, float yv, float wv, float& r, float& l) {
  if (LOSS == LOSS_LOGISTIC) {
    const float e = __expf(-fabsf(m));
    const float inv = __builtin_amdgcn_rcpf(1.0f + e);
    const float p = m >= 0.f ? inv : e * inv;   // sigmoid(m)
    r = (p - yv) * wv;
    l = wv * (fmaxf(m, 0.f) + __logf(1.0f + e) - yv * m);
  } else if (LOSS == LOSS_HINGE) {
    const float s = 2.f * yv - 1.f;
    const float mg = 1.f - s * m;
    r = mg > 0.f ? -s * wv : 0.f;
    l = mg > 0.f ? wv * mg : 0.f;
  } else {
    const float e = m - yv;
    r = e * wv;
    l = 0.5f * wv * e * e;
  }
}

// Coefficients of the columns lane c owns (chunks c, c + LPR, ...), zero past ld.
template <int LPR, int CPL>
__device__ __forceinline__ void load_coef(const float* __restrict__ coef, int64_t ld, int c, float (&w)[CPL][8]) {
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = 8 * (c + k * LPR) + j;
      w[k][j] = col < ld ? coef[col] : 0.f;
    }
}
template <class T, int A, int B>
__device__ __forceinline__ void zero(T (&a)[A][B]) {
#pragma unroll
  for (int k = 0; k < A; ++k)
#pragma unroll
    for (int j = 0; j < B; ++j) a[k][j] = T{};
}

// Block epilogue of the gradient passes: sum the G row groups of the wave (lanes c,
// c + LPR, ...), then the 4 waves via LDS in a fixed order, into the block's slab row
// [X^T r (DP) | sum r | loss | weight sum].  pacc: later slices of a split pass add in.
// (The block helpers take lane / wid / c from the kernel: recomputing them from threadIdx
// reorders the kernel's first instructions and, with them, its register allocation.)
template <int LPR, int CPL>
__device__ __forceinline__ void grad_epilogue(float (&acc)[CPL][8], float acc_r, float acc_loss, float acc_w,
                                              float* __restrict__ partial, int pstride, int pacc, int lane, int wid,
                                              int c) {
  constexpr int DP = LPR * CPL * 8;
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = acc[k][j];
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
      acc[k][j] = v;
    }
  acc_r = wave_sum(acc_r);
  acc_loss = wave_sum(acc_loss);
  acc_w = wave_sum(acc_w);
  __shared__ float red[kWavesPerBlock][DP + 4];
  if (lane < LPR) {
#pragma unroll
    for (int k = 0; k < CPL; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) red[wid][8 * (c + k * LPR) + j] = acc[k][j];
  }
  if (lane == 0) {
    red[wid][DP] = acc_r;
    red[wid][DP + 1] = acc_loss;
    red[wid][DP + 2] = acc_w;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DP + 3; i += kBlock) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < kWavesPerBlock; ++q) s += red[q][i];
    float* const pp = partial + (int64_t)blockIdx.x * pstride + i;
    *pp = pacc ? *pp + s : s;
  }
}

// Cross-lane sums for the LPR = 8, two-rows-per-lane layout without LDS traffic: the
// quad butterflies use quad_perm DPP, the cross-quad halving row_half_mirror (lane i <->
// 7 - i: after the quad sums every lane of a quad holds the same value, so the mirror
// partner serves as lane i ^ 4).  Leaves lanes c < 4 with row 0's sum and lanes c >= 4
// with row 1's -- the RowReduce<8, 2> layout (base(c) = c >> 2) -- in v[0].  Replaces
// three ds_bpermute round trips (and their lgkmcnt waits) per tile by five DPP adds.
// (Every caller is in glm_mixed.hip, on purpose: what hipcc makes of the lane test below
// depends on the callers it sees in the unit -- see the note at glm_grad_f32_kernel.)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF,
                                                               false));
}
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141;
__device__ __forceinline__ void row_reduce_8x2(float (&v)[2], int c) {
  v[0] += dpp_f<kDppXor1>(v[0]);
  v[1] += dpp_f<kDppXor1>(v[1]);
  v[0] += dpp_f<kDppXor2>(v[0]);
  v[1] += dpp_f<kDppXor2>(v[1]);
  const bool up = (c & 4) != 0;
  const float keep = up ? v[1] : v[0], send = up ? v[0] : v[1];
  v[0] = keep + dpp_f<kDppHalfMirror>(send);
}

// Mini-batch sampling (miniBatchFraction < 1, mllib GradientDescent's per-iteration
// `data.sample(false, fraction, seed + i)`): row r of iteration t is kept iff
// row_key(sample_key(seed, t), global r) >> 8 < fraction * 2^24.  The mask only zeroes a
// row's weight (its residual, loss and weight-sum terms), so it costs one hash per row,
// needs no compaction pass, and the kept set is independent of the sharding.
struct RowSampler {
  uint32_t key, thr;   // thr >= 2^24: every row kept (sampling off)
  int64_t grow0;       // global index of the role's row 0
  __device__ __forceinline__ bool on() const { return thr < (1u << 24); }
  __device__ __forceinline__ bool keep(int64_t row) const { return (row_key(key, grow0 + row) >> 8) < thr; }
};
__host__ __device__ __forceinline__ uint32_t sample_key(uint32_t seed, uint32_t iter) {
  return fmix32(seed ^ fmix32(iter * 0x9E3779B1u + 0x7F4A7C15u));
}

typedef __bf16 sm_bf16x2 __attribute__((ext_vector_type(2)));
// Two fp32 -> one dword of two bf16 (round to nearest even: v_cvt_pk_bf16_f32), a in the low half.
__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
  float2_ v;
  v[0] = a;
  v[1] = b;
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, sm_bf16x2));
}
// Two fp32 -> two such dwords hi + lo: x - (hi + lo) is below 2^-17 |x|.
__device__ __forceinline__ void split_bf16x2(float x0, float x1, uint32_t& ph, uint32_t& pl) {
  ph = pk_bf16(x0, x1);
  pl = pk_bf16(x0 - __uint_as_float(ph << 16), x1 - __uint_as_float(ph & 0xffff0000u));
}
// Two fp32 -> three such dwords hi + mid + lo, each the rounding of the exact remainder so
// far: x - (hi + mid + lo) is below 2^-25 |x|, x - (hi + mid) below 2^-17 |x|.
__device__ __forceinline__ void split_bf16x3(float x0, float x1, uint32_t& ph, uint32_t& pm, uint32_t& pl) {
  ph = pk_bf16(x0, x1);
  const float r0 = x0 - __uint_as_float(ph << 16), r1 = x1 - __uint_as_float(ph & 0xffff0000u);
  pm = pk_bf16(r0, r1);
  pl = pk_bf16(r0 - __uint_as_float(pm << 16), r1 - __uint_as_float(pm & 0xffff0000u));
}

}  // namespace

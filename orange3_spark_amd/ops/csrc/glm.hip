// Generalised-linear-model streaming kernels (gfx950).
//
// Replaces the per-partition gradient closure that Spark MLlib runs inside
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
// The op is a GEMV (512 B/row at D=256): a pass over resident rows alone runs at the HBM
// streaming rate (12.9 G rows/s, about 6.6 TB/s; doc/performance.md), and the budget there is
// bytes.  The mixed pass of a table larger than HBM is not bytes alone: its lineage rows are
// VALU work (two hashes and eight byte decodes per chunk).  What it is held to is the time of
// its resident rows alone.  glm_grad_staged_kernel keeps each wave's next resident tile in
// flight through an LDS slot, which took the waves' s_waitcnt share from a third of their
// cycles to a tenth and left the pass VALU-issue bound (VALU issued in 94 - 96 % of its cycles);
// since then the resident tiles' dot products run on the matrix cores, which were idle, and
// the VALU keeps the lineage tiles and X^T r (doc/performance.md has the counters of each step).
// A pass large enough runs that kernel's tiles as ONE launch of persistent waves that claim row
// items from a ticket (glm_grad_persist_kernel, glm_items.h), which fills the wave slots that
// the blocks of 14 sliced launches left empty between their prologues and epilogues.
//
// Cross-block reduction: one fp32 slab row per block + `glm_finish` (fp64, fixed
// order) -> bitwise deterministic results, no float atomics (Guideline 12).
//
// SRC == 1 ("synthetic lineage"): instead of loading a chunk, the lane regenerates
// it from the counter hash used by `synth_glm_kernel`, so rows that did not fit in
// HBM are recomputed from lineage on every pass -- the MI355X equivalent of Spark's
// MEMORY_ONLY caching, where evicted partitions are recomputed.  Regenerated and
// materialised rows are bit-identical.
#include <type_traits>

#include "common.h"
#include "glm_items.h"

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
// (see glm_grad_kernel), two hashes per 16-B chunk.
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
// Row sources.  Every tile body below is written once and instantiated per source; a
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
// (Two ways in: stats_tile regenerates a chunk where it is used, load(fk, ch); grad_tile
// forms the two hash words itself and calls decode -- with the chunk index passed through
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

// ---------------------------------------------------------------------------
// Mixed pass: resident rows (HBM stream, memory bound) and lineage rows (regenerated
// in-kernel, VALU bound) in ONE launch.  Two back-to-back or two-stream launches leave
// one resource idle (the first grid fills every CU slot, so the second kernel only
// starts as the first drains: profiles/glm_overlap.json, 63.8 ms vs 41 + 25 ms alone).
// Here every wave walks one interleaved sequence of S = Tr + Tl row tiles in which
// lineage tiles are spread evenly (Bresenham: tile s is lineage iff
// floor((s+1) Tl / S) > floor(s Tl / S)), so at any moment each CU holds a mix of
// load-bound and ALU-bound waves and both roles finish together.  Both roles use the
// same lane->column mapping (the lineage one), so they share w / acc registers.

// Cross-lane sums for the LPR = 8, two-rows-per-lane layout without LDS traffic: the
// quad butterflies use quad_perm DPP, the cross-quad halving row_half_mirror (lane i <->
// 7 - i: after the quad sums every lane of a quad holds the same value, so the mirror
// partner serves as lane i ^ 4).  Leaves lanes c < 4 with row 0's sum and lanes c >= 4
// with row 1's -- the RowReduce<8, 2> layout (base(c) = c >> 2) -- in v[0].  Replaces
// three ds_bpermute round trips (and their lgkmcnt waits) per tile by five DPP adds.
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

// The wave-private LDS slot of glm_grad_staged_kernel (the schedule and its wait discipline
// are described there) and what the wave has in flight into it.  The slot holds the next
// resident tile (16 rows x 32 chunks of 16 B) as its 8 DMA images of 1 KB, then the 64 labels
// of that tile (lane l holds tile row l & 15's) and the 64 labels of the next lineage tile
// (lane l's label at l * 4).
// Placement: image u * CPL + k holds chunks 8k .. 8k + 7 of the rows 8u .. 8u + 7, row 8u + g
// in the 128 B at g * 128, its chunk 8k + p at position p ^ t(g), t(g) = g >> 1 (lane (g, c')
// of the DMA fetches chunk 8k + (c' ^ t(g)): every 8 lanes still cover one whole 128-B line).
// The tile is read out twice with ds_read_b128:
//   * for X^T r, lane (g, c) takes chunk c + 8k of the rows g and 8 + g, as grad_tile's loads
//     return them: every read covers 1 KB contiguously, permuted inside 64-B quarters of a
//     line, which no 16-lane group of ds_read_b128 straddles: conflict-free;
//   * as the B operand of v_mfma_f32_16x16x32_bf16, lane l takes chunk 8 (l >> 4) + s of tile
//     row l & 15 in step s.  Unswizzled, the 8 lanes of a 16-lane group that share l >> 4 sit
//     on 2 of the 16 slots of the 256-B bank row (4-way); with t the 16 rows of a group spread
//     over 8 slots, rows R and R + 8 together: 2-way.  (s ^ t) = (s & 4) | ((s & 3) ^ t), so
//     four per-lane bases and the immediate offsets 0 / 64 address the eight steps.
// Every wait and every LDS read of the slot is inline asm: hipcc then sees no LDS load that
// could alias a DMA target and adds no vmcnt(0) of its own, and the waits count the DMAs
// exactly.  The only vector-memory operations of the tile loop are the DMAs issued here, in
// batches of kTileOps (label, then 8 images) and single lineage labels.
// Beside the slots the block keeps one image of the coefficients as the A operand of the same
// MFMA (kStgFragBytes, filled once in the kernel's prologue; see TileStage::dot).
constexpr int kStgTileBytes = 8 * 1024, kStgLabelBytes = kWave * 4;
constexpr int kStgWaveBytes = kStgTileBytes + 2 * kStgLabelBytes;
constexpr int kStgFragBytes = 8 * 1024;   // 8 k-steps x 64 lanes x 16 B
constexpr int kStgLd = 256;            // row width of the one layout that is staged: (8, 4, 2)
constexpr unsigned kAuxNt = 2;         // cache policy bit "nt", as __builtin_nontemporal_load sets
struct TileStage {
  static constexpr int LPR = 8, CPL = 4, UNROLL = 2, G = kWave / LPR, kTileOps = 1 + UNROLL * CPL;
  // Wave-uniform state only (SGPRs).  What a lane adds -- its byte offset in a tile's rows,
  // its label's, its LDS addresses -- is recomputed from the lane id where it is used: held in
  // registers across the loop, those values are what makes the lineage tile spill.
  unsigned char* slot;
  uint32_t sbase;              // the slot's LDS byte address (a multiple of 256)
  uint32_t fbase;              // the coefficient fragments' LDS byte address
  const unsigned char* xs;     // row 0 of the next resident tile to issue
  const float* yrs;            // label 0 of the next resident / lineage tile to issue
  const float* yls;
  int64_t tstep;               // rows from one tile of this wave to its next
  uint32_t r_ahead, l_ahead;   // tiles of each role not issued yet
  // a lineage label is in flight and was issued after the last batch: a wait for that batch
  // may leave it (vmcnt(1)), and a wait for it drains the batch with it (vmcnt(0))
  bool lab_younger;
  // glm_grad_persist_kernel only (PERSIST in take_tile / take_label; zero and unused elsewhere):
  // the bases of the pass's three arrays, the next item's first tiles and counts (nx_nr / nx_nl
  // are zero until that item is known and again once the stager has moved on to it), and
  // whether the first batch / label of the next item is already in flight.
  const unsigned char* x0;
  const float* yr0;
  const float* yl0;
  uint32_t nx_r0, nx_nr, nx_l0, nx_nl;
  bool r_pre, l_pre;

  // (an empty asm per use: otherwise the offsets are hoisted out of the loop as invariants)
  __device__ static __forceinline__ uint32_t fresh(int v) {
    asm volatile("" : "+v"(v));
    return (uint32_t)v;
  }
  // the tile row whose label lane (g, c) takes: RowReduce<8, 2>::base(c) * G + g
  __device__ static __forceinline__ uint32_t label_off(uint32_t g, uint32_t c) { return ((c >> 2) * G + g) * 4; }

  __device__ __forceinline__ void issue_tile(int lane) {
    const uint32_t ln = fresh(lane);
    // (a resident tile's rows are finished in the lanes 0 .. 15, row = lane: TileStage::dot)
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const unsigned char*>(yrs) + (ln & 15) * 4,
                                     slot + kStgTileBytes, 4, 0, 0);
    // lane (g, c') = (ln >> 3, ln & 7) fetches chunk c' ^ t(g) of row g (+ 8u, + 8k chunks)
    const uint32_t xoff = (ln >> 3) * (kStgLd * 2) + ((ln ^ (ln >> 4)) & 7) * 16;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int k = 0; k < CPL; ++k)
        __builtin_amdgcn_global_load_lds(xs + (u * G * kStgLd * 2 + k * LPR * 16) + xoff, slot + (u * CPL + k) * 1024,
                                         16, 0, kAuxNt);
    xs += tstep * (kStgLd * 2);
    yrs += tstep;
    --r_ahead;
    lab_younger = false;
  }
  __device__ __forceinline__ void issue_label(int g, int c) {
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const unsigned char*>(yls) + label_off(fresh(g), fresh(c)),
                                     slot + kStgTileBytes + kStgLabelBytes, 4, 0, 0);
    yls += tstep;
    --l_ahead;
    lab_younger = true;
  }
  // Resident tile: one wait for its batch, the slot read out (lgkmcnt(0): it is rewritten
  // only after its reads have returned), then the wave's next resident tile issued -- none
  // after the last, so nothing past the wave's own tiles is ever read.
  // xb[s]: the B operand of k-step s (chunk 8 (lane >> 4) + s of tile row lane & 15); xv: the
  // X^T r layout; yv: the label of tile row lane & 15; fa: the coefficient fragments (A
  // operand, see dot) of the k-steps 0 - 2.
  // PERSIST: after the last tile of the item the stager moves on to the next item's first.
  template <bool PERSIST = false>
  __device__ __forceinline__ void take_tile(int lane, short8 (&xb)[8], short8 (&xv)[UNROLL][CPL], float& yv,
                                            short8 (&fa)[3]) {
    if (lab_younger) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t ln = fresh(lane);
    // operand read: image (R >> 3) * 4 + q, row R & 7, position s ^ t(R), t(R) = (R >> 1) & 3;
    // sbase is a multiple of 128, so the xor acts on the position bits alone
    const uint32_t b0 = sbase + ((ln & 8) << 9) + ((ln >> 4) << 10) + ((ln & 7) << 7) + (((ln >> 1) & 3) << 4);
    asm volatile(
        "ds_read_b128 %17, %26\n\t"
        "ds_read_b128 %18, %26 offset:1024\n\t"
        "ds_read_b128 %19, %26 offset:2048\n\t"
        "ds_read_b128 %0, %20\n\t"
        "ds_read_b128 %1, %21\n\t"
        "ds_read_b128 %2, %22\n\t"
        "ds_read_b128 %3, %23\n\t"
        "ds_read_b128 %4, %20 offset:64\n\t"
        "ds_read_b128 %5, %21 offset:64\n\t"
        "ds_read_b128 %6, %22 offset:64\n\t"
        "ds_read_b128 %7, %23 offset:64\n\t"
        "ds_read_b128 %8, %24\n\t"
        "ds_read_b128 %9, %24 offset:1024\n\t"
        "ds_read_b128 %10, %24 offset:2048\n\t"
        "ds_read_b128 %11, %24 offset:3072\n\t"
        "ds_read_b128 %12, %24 offset:4096\n\t"
        "ds_read_b128 %13, %24 offset:5120\n\t"
        "ds_read_b128 %14, %24 offset:6144\n\t"
        "ds_read_b128 %15, %24 offset:7168\n\t"
        "ds_read_b32 %16, %25 offset:8192\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(xb[0]), "=&v"(xb[1]), "=&v"(xb[2]), "=&v"(xb[3]), "=&v"(xb[4]), "=&v"(xb[5]), "=&v"(xb[6]),
          "=&v"(xb[7]), "=&v"(xv[0][0]), "=&v"(xv[0][1]), "=&v"(xv[0][2]), "=&v"(xv[0][3]), "=&v"(xv[1][0]),
          "=&v"(xv[1][1]), "=&v"(xv[1][2]), "=&v"(xv[1][3]), "=&v"(yv), "=&v"(fa[0]), "=&v"(fa[1]), "=&v"(fa[2])
        : "v"(b0), "v"(b0 ^ 16u), "v"(b0 ^ 32u), "v"(b0 ^ 48u), "v"(sbase + ((ln ^ (ln >> 4)) << 4)),
          "v"(sbase + ln * 4), "v"(fbase + ln * 16)
        : "memory");
    if constexpr (PERSIST) {
      if (r_ahead == 0 && nx_nr > 0) {
        xs = x0 + (uint64_t)nx_r0 * (UNROLL * G * kStgLd * 2);
        yrs = yr0 + (uint64_t)nx_r0 * (UNROLL * G);
        r_ahead = nx_nr;
        nx_nr = 0;
        r_pre = true;
      }
    }
    if (r_ahead > 0) issue_tile(lane);
    __builtin_amdgcn_sched_barrier(0);   // the DMAs go out ahead of the tile's math
  }
  // The 16 rows' dot products with the coefficients on the matrix cores: D (16 x 16) = A x B
  // over eight k-steps of 32 columns.  B is the tile (take_tile's xb); A comes from the block's
  // fragment image, one ds_read_b128 per step at fbase + s * 1024 + lane * 16: row 0 holds the
  // coefficients' bf16 hi terms, row 1 the mid and row 2 the lo terms (w = hi + mid + lo
  // exactly), rows 3 .. 15 zeros.  D has col = lane & 15, row = 4 (lane >> 4) + reg, so the
  // lanes 0 .. 15 end with their own tile row's three partial dots in d[0], d[1], d[2].
  // The fragments of the steps 0 - 2 come with the tile reads (take_tile's fa: their latency
  // hides behind the tile's 16 reads); the steps 3 - 7 are read here, behind the next tile's
  // DMAs, two steps ahead of their MFMA, each into the buffer of the MFMA issued a step before
  // (at least 9 wait states earlier).  They are not in the slot and do not gate its reuse.
  // Nothing inside an asm statement gets hazard padding from the compiler: each dependent MFMA
  // is at least 9 wait states behind the one before, and the D registers are read by VALU 12
  // wait states after the last one.
  __device__ __forceinline__ float4_ dot(int lane, const short8 (&xb)[8], short8 (&fa)[3]) {
    float4_ d;
    asm volatile(
        "v_mfma_f32_16x16x32_bf16 %0, %1, %5, 0\n\t"
        "s_nop 7\n\t"
        "ds_read_b128 %1, %4 offset:3072\n\t"
        "v_mfma_f32_16x16x32_bf16 %0, %2, %6, %0\n\t"
        "s_nop 7\n\t"
        "ds_read_b128 %2, %4 offset:4096\n\t"
        "v_mfma_f32_16x16x32_bf16 %0, %3, %7, %0\n\t"
        "s_nop 7\n\t"
        "ds_read_b128 %3, %4 offset:5120\n\t"
        "s_waitcnt lgkmcnt(2)\n\t"
        "v_mfma_f32_16x16x32_bf16 %0, %1, %8, %0\n\t"
        "s_nop 7\n\t"
        "ds_read_b128 %1, %4 offset:6144\n\t"
        "s_waitcnt lgkmcnt(2)\n\t"
        "v_mfma_f32_16x16x32_bf16 %0, %2, %9, %0\n\t"
        "s_nop 7\n\t"
        "ds_read_b128 %2, %4 offset:7168\n\t"
        "s_waitcnt lgkmcnt(2)\n\t"
        "v_mfma_f32_16x16x32_bf16 %0, %3, %10, %0\n\t"
        "s_nop 7\n\t"
        "s_waitcnt lgkmcnt(1)\n\t"
        "v_mfma_f32_16x16x32_bf16 %0, %1, %11, %0\n\t"
        "s_nop 7\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_mfma_f32_16x16x32_bf16 %0, %2, %12, %0\n\t"
        "s_nop 7\n\t"
        "s_nop 3"
        : "=&v"(d), "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2])
        : "v"(fbase + fresh(lane) * 16), "v"(xb[0]), "v"(xb[1]), "v"(xb[2]), "v"(xb[3]), "v"(xb[4]), "v"(xb[5]),
          "v"(xb[6]), "v"(xb[7])
        : "memory");
    return d;
  }
  // Lineage tile: its label was issued a lineage tile earlier.  With a batch issued since
  // (lab_younger false) the wait leaves that batch in flight; otherwise the label is the
  // youngest operation and the in-order counter leaves no choice but vmcnt(0).
  template <bool PERSIST = false>
  __device__ __forceinline__ void take_label(int g, int c, float& yv) {
    if (lab_younger) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kTileOps) : "memory");
    const uint32_t a4 = sbase + (fresh(g) * LPR + fresh(c)) * 4;
    asm volatile("ds_read_b32 %0, %1 offset:8448\n\ts_waitcnt lgkmcnt(0)" : "=v"(yv) : "v"(a4) : "memory");
    lab_younger = false;
    if constexpr (PERSIST) {
      if (l_ahead == 0 && nx_nl > 0) {
        yls = yl0 + (uint64_t)nx_l0 * (UNROLL * G);
        l_ahead = nx_nl;
        nx_nl = 0;
        l_pre = true;
      }
    }
    if (l_ahead > 0) issue_label(g, c);
  }
};
static_assert(kStgTileBytes == 8192 && kStgLabelBytes == 256, "the asm offsets in TileStage");

// One gradient tile of RT = G * UNROLL rows from source SRC.  Labels / weights come from
// the materialised label column (y, sw already offset to the role's first row).
// FULL: every row of the tile is < n and every chunk of the layout is < nch (the caller
// guarantees both), so rows, chunks and labels are read unclamped and nothing is masked.
// STAGED (with FULL, unweighted, lineage rows): the labels come out of the wave's LDS slot
// (stg); y and sw are not read here.  (The staged resident tile is staged_resident_tile.)
template <class SRC, int LPR, int CPL, int UNROLL, int LOSS, bool SMP, bool FULL = false, bool STAGED = false,
          bool PERSIST = false>
__device__ __forceinline__ void grad_tile(
    int64_t base, int64_t n, const typename SRC::elem* __restrict__ X, int64_t ld, int nch,
    const float* __restrict__ y, const float* __restrict__ sw, uint32_t seed, int64_t row0, const float (&w)[CPL][8],
    float wshift, float intercept, int g, int c, const RowSampler smp, float (&acc)[CPL][8], float& rs, float& acc_r,
    float& acc_loss, float& acc_w, TileStage* stg = nullptr) {
  constexpr int G = kWave / LPR;
  using RR = RowReduce<LPR, UNROLL>;
  constexpr int NF = RR::NF;
  static_assert(!STAGED || (SRC::kLineage && FULL && NF == 1 && LPR == TileStage::LPR && CPL == TileStage::CPL &&
                            UNROLL == TileStage::UNROLL),
                "the staged slot holds the labels of one (8, 4, 2) lineage tile");
  const int ubase = RR::base(c);
  const bool rep = RR::representative(c);
  typename SRC::chunk xv[UNROLL][CPL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    // (STAGED: the lane's row group made opaque per tile, or hipcc keeps row0 + g, 64 bits per
    // lane, across the loop of the staged kernel, which has no register left for it)
    const int64_t row = base + u * G + (STAGED ? (int)TileStage::fresh(g) : g);
    const bool ok = row < n;
    const int64_t rowc = ok ? row : n - 1;
    const uint32_t fk = SRC::kLineage ? feat_key(seed, row0 + row) : 0u;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int ch = c + k * LPR;
      if constexpr (SRC::kLineage) {
        SRC::decode(synth_word(fk, 2 * ch), synth_word(fk, 2 * ch + 1), xv[u][k]);
      } else if constexpr (FULL) {
        SRC::load(X, ld, row, ch, xv[u][k]);
      } else {
        const int chc = ch < nch ? ch : nch - 1;
        SRC::load(X, ld, rowc, chc, xv[u][k]);
        SRC::mask(xv[u][k], ok && ch < nch);
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
    if constexpr (STAGED) {
      ww[j] = 1.f;   // (the label: take_label below)
    } else if constexpr (FULL) {
      yy[j] = y[row];
      ww[j] = sw ? sw[row] : 1.f;
    } else {
      const float yv = y[rowc];
      const float wv = sw ? sw[rowc] : 1.f;
      yy[j] = ok ? yv : 0.f;
      ww[j] = ok ? wv : 0.f;
    }
    if constexpr (SMP && !STAGED) {
      if (!smp.keep(row)) ww[j] = 0.f;
    }
  }
  float dot[UNROLL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    // two interleaved partial sums -> v_pk_fma_f32 (one issue per two features)
    float2_ d2 = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      float x[8];
      SRC::unpack(xv[u][k], x);
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const float2_ xx = {x[j], x[j + 1]}, ww2 = {w[k][j], w[k][j + 1]};
        d2 = __builtin_elementwise_fma(xx, ww2, d2);
      }
    }
    dot[u] = SRC::dot(d2.x + d2.y, wshift);
  }
  constexpr bool kDpp = LPR == 8 && UNROLL == 2;
  if constexpr (kDpp) row_reduce_8x2(dot, c);
  else RR::run(dot, c);
  if constexpr (STAGED && SRC::kLineage) stg->template take_label<PERSIST>(g, c, yy[0]);   // as late as the label is needed
  if constexpr (STAGED && SMP) {   // (and the sampler's hash: a register less across the dot products)
    // (the lane's row in the tile made opaque: hipcc otherwise keeps grow0 + it, 64 bits per
    // role, in registers across the loop, which spills)
    if (!smp.keep(base + (int64_t)TileStage::fresh(ubase * G + g))) ww[0] = 0.f;
  }
  float res[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    float r, l;
    loss_terms<LOSS>(dot[j] + intercept, yy[j], ww[j], r, l);
    res[j] = r;
    if (rep) { acc_r += r; acc_loss += l; acc_w += ww[j]; }
  }
#pragma unroll
  for (int u = 0; u < UNROLL; ++u)
#pragma unroll
    for (int k = 0; k < CPL; ++k) SRC::pin(xv[u][k]);
  // broadcast each row's residual back to its LPR lanes, accumulate X^T r
  float other = 0.f;
  if constexpr (kDpp) other = dpp_f<kDppHalfMirror>(res[0]);   // the other row's residual
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    float r;
    if constexpr (kDpp) r = ((c & 4) != 0) == (u == 0) ? other : res[0];
    else r = __shfl(res[u % NF], g * LPR + RR::owner(u), kWave);
    r = SRC::resid(r, rs);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      float x[8];
      SRC::unpack(xv[u][k], x);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(r, x[j], acc[k][j]);
    }
  }
}

// The resident tile of glm_grad_staged_kernel: 16 rows out of the wave's LDS slot, their dot
// products on the matrix cores (TileStage::dot), X^T r as in grad_tile.  The rows are finished
// in the lanes 0 .. 15 (tile row = lane; the other lanes compute on D rows that are zero and
// add nowhere): margin = (lo + mid) + hi partial dots, one loss_terms for the 16 rows, no
// cross-lane reduction.  Lane (g, c) then fetches the residuals of its rows g and 8 + g from
// the lanes g and 8 + g.  base: the tile's first row within the role (the sampler's row index).
template <int LOSS, bool SMP, bool PERSIST = false>
__device__ __forceinline__ void staged_resident_tile(int64_t base, float intercept, int lane, const RowSampler smp,
                                                     float (&acc)[TileStage::CPL][8], float& acc_r, float& acc_loss,
                                                     float& acc_w, TileStage* stg) {
  constexpr int CPL = TileStage::CPL, UNROLL = TileStage::UNROLL;
  short8 xb[8], xv[UNROLL][CPL];
  float yv;
  short8 fa[3];
  stg->template take_tile<PERSIST>(lane, xb, xv, yv, fa);
  const float4_ d = stg->dot(lane, xb, fa);
  float wv = 1.f;
  if constexpr (SMP) {
    // (the lane's row in the tile made opaque: hipcc otherwise keeps grow0 + it, 64 bits, in
    // registers across the loop, which spills)
    if (!smp.keep(base + (int64_t)(TileStage::fresh(lane) & 15u))) wv = 0.f;
  }
  float r, l;
  loss_terms<LOSS>(((d[2] + d[1]) + d[0]) + intercept, yv, wv, r, l);
  if (lane < 16) { acc_r += r; acc_loss += l; acc_w += wv; }
#pragma unroll
  for (int u = 0; u < UNROLL; ++u)
#pragma unroll
    for (int k = 0; k < CPL; ++k) RowsBf16::pin(xv[u][k]);
  // row g's residual sits in lane g, row 8 + g's in lane 8 + g (byte address = 4 * lane)
  const int src = (int)(TileStage::fresh(lane) >> 3) * 4;
  const float rr[UNROLL] = {
      __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, r))),
      __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src + 32, __builtin_bit_cast(int, r)))};
#pragma unroll
  for (int u = 0; u < UNROLL; ++u)
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      float x[8];
      unpack8(xv[u][k], x);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(rr[u], x[j], acc[k][j]);
    }
}

// y / sw hold n_res + n_lin entries: the resident rows' labels, then the lineage rows'.
// MW: minimum waves per SIMD the register allocator must allow (at D = 256, masked: 2 =
// 170-175 VGPRs and two waves, 3 = 168 VGPRs with up to 28 B of scratch; mask-free: 163-168
// VGPRs, no scratch and three waves either way -- the table in doc/performance.md).
// Every wave walks the interleaved tile sequence (both roles per wave; fixed-role layouts
// -- some waves regenerating, the others streaming -- measured slower and were removed).
// A resident tile's loads are issued at its top and waited for a few instructions later, so
// only the other waves of the SIMD cover their latency; glm_grad_staged_kernel below is the
// same pass with each wave's next resident tile kept in flight through an LDS slot.
// FULL: n_res and n_lin are multiples of RT and ld is the layout's full width, so both tile
// bodies drop their clamps and masks (grad_tile); the host launches the ragged rest apart
// (o3s_glm_grad_mixed).  The loop holds two tile bodies either way: a third one spills.
template <int LPR, int CPL, int UNROLL, int LOSS, int MW, bool SMP, bool FULL = false>
__global__ __launch_bounds__(kBlock, MW) void glm_grad_mixed_kernel(
    const uint16_t* __restrict__ X, int64_t ld, int64_t n_res, const float* __restrict__ y,
    const float* __restrict__ sw, const float* __restrict__ y_lin, const float* __restrict__ sw_lin,
    const float* __restrict__ coef, const float* __restrict__ bptr, uint32_t seed, int64_t row0, int64_t n_lin,
    float* __restrict__ partial, int pstride, int64_t res_row0, const int64_t* __restrict__ t_dev, uint32_t sseed,
    uint32_t sthr, int pacc) {
  constexpr int G = kWave / LPR;
  constexpr int RT = G * UNROLL;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int g = lane / LPR, c = lane % LPR;
  const int nch = (int)(ld / 8);
  // read from device memory so a device-side optimizer step never syncs the host
  const float intercept = *bptr;
  // iteration t of a device-side SGD loop = t_dev + 1 (the update kernel advances it)
  // (SMP = false: the sampler is compiled out -- no hash, no extra registers)
  const uint32_t skey = SMP ? sample_key(sseed, (uint32_t)((t_dev ? t_dev[0] : 0) + 1)) : 0u;
  const RowSampler smp_res{skey, sthr, res_row0}, smp_lin{skey, sthr, row0};

  // (the coefficient loop is written out, not load_coef: it also sums wshift, and even as a
  // helper with this very loop it cost 16 B of scratch in <8,4,2,0,3,false>)
  float w[CPL][8], acc[CPL][8];
  float wshift = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = 8 * (c + k * LPR) + j;
      w[k][j] = col < ld ? coef[col] : 0.f;
      wshift += w[k][j];
      acc[k][j] = 0.f;
    }
  wshift *= kSynthShift;
  float rs = 0.f;
  float acc_r = 0.f, acc_loss = 0.f, acc_w = 0.f;

  const int64_t Tr = (n_res + RT - 1) / RT, Tl = (n_lin + RT - 1) / RT, S = Tr + Tl;
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wid;
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  if (gw < S) {
    // lineage tiles before unit s: L = floor(s Tl / S), rem = s Tl mod S (s Tl < 2^62)
    int64_t L = gw * Tl / S, rem = gw * Tl - L * S;
    const int64_t q0 = nw * Tl / S, r0 = nw * Tl - q0 * S;
    for (int64_t s = gw; s < S; s += nw) {
      if (rem + Tl >= S)
        grad_tile<RowsLineage, LPR, CPL, UNROLL, LOSS, SMP, FULL>(L * RT, n_lin, X, ld, nch, y_lin, sw_lin, seed, row0, w,
                                                                  wshift, intercept, g, c, smp_lin, acc, rs, acc_r, acc_loss,
                                                                  acc_w);
      else
        grad_tile<RowsBf16, LPR, CPL, UNROLL, LOSS, SMP, FULL>((s - L) * RT, n_res, X, ld, nch, y, sw, seed, row0, w, wshift,
                                                               intercept, g, c, smp_res, acc, rs, acc_r, acc_loss, acc_w);
      rem += r0;
      L += q0;
      if (rem >= S) { rem -= S; ++L; }
    }
  }
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(rs, kSynthShift, acc[k][j]);
  grad_epilogue<LPR, CPL>(acc, acc_r, acc_loss, acc_w, partial, pstride, pacc, lane, wid, c);
}

// The coefficients as the A operand of the resident tiles' MFMAs (TileStage::dot): entry
// (step s, lane l) of the image is A[row l & 15][k = 8 (l >> 4) + j] = the bf16 term l & 15
// (0 hi, 1 mid, 2 lo, as split8 forms them; zero from 3 on) of the coefficients of chunk
// 8 (l >> 4) + s, the chunk that lane l's B operand holds in step s.
// Written by the whole block; the caller's __syncthreads() stands between it and the first read.
__device__ __forceinline__ void build_coef_frags(unsigned char* __restrict__ frags, const float* __restrict__ coef) {
  for (int e = threadIdx.x; e < kStgFragBytes / 16; e += kBlock) {
    const int s = e >> 6, term = e & 15, q = (e & 63) >> 4;
    uint32_t p[4] = {0u, 0u, 0u, 0u};
    if (term < 3) {
      const float* cw = coef + 8 * (8 * q + s);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = cw[2 * j], x1 = cw[2 * j + 1];
        const uint32_t ph = pk_bf16(x0, x1);
        const float r0 = x0 - __uint_as_float(ph << 16), r1 = x1 - __uint_as_float(ph & 0xffff0000u);
        const uint32_t pm = pk_bf16(r0, r1);
        const uint32_t pl = pk_bf16(r0 - __uint_as_float(pm << 16), r1 - __uint_as_float(pm & 0xffff0000u));
        p[j] = term == 0 ? ph : term == 1 ? pm : pl;
      }
    }
    uint32_t* const dst = reinterpret_cast<uint32_t*>(frags + e * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = p[j];
  }
}

// The mixed pass with the resident tiles staged through LDS: the (8, 4, 2) layout on whole
// tiles of 256-column bf16 rows, unweighted (contract of glm_grad_mixed_kernel<8, 4, 2, LOSS,
// 3, SMP, true> with sw == nullptr; n_res / 16 and n_lin / 16 are below 2^31).
// Why: a resident tile of glm_grad_mixed_kernel issues its 8 loads at its top and waits for
// them a few instructions later, and during its lineage tiles a wave has nothing in flight,
// so the bytes in flight per CU stay well under what three waves per SIMD could hold.  Here a
// wave issues its NEXT resident tile (label + 8 LDS-DMA images, TileStage) while it takes the
// current one out of its slot, so those loads stay in flight across the tile's math and the
// lineage tiles that follow.  A second register copy of a tile does not fit three waves per
// SIMD; the 8.5 KB slot per wave does.
// The resident tile's 16 dot products are eight v_mfma_f32_16x16x32_bf16 (TileStage::dot,
// staged_resident_tile): the tile as it lies in the slot is the B operand, the coefficients
// split into three bf16 terms are the A operand, read from an 8 KB image the block builds
// once (the products are exact in fp32; only the accumulation order differs from the fp32
// chain of the unstaged kernels).  The lineage tile's dot and both tiles' X^T r stay on the
// VALU, on the fp32 w.  LDS per block: 4 slots, the image and the epilogue's array, 47 168 B
// (three blocks per CU: 141.5 of 160 KB).
// Order: a wave owns the resident tiles gw, gw + nw, ... and the lineage tiles gw, gw + nw,
// ... (gw its global index, nw the waves of the grid) and interleaves its own two counts by
// Bresenham, so "next resident tile" is a pointer bump and the mix stays even per wave.  The
// order is fixed, so the pass is as deterministic as the unstaged one; which wave sums which
// row differs from it (fp32 block-sum order).
// Waits (vmcnt completes in order, and the DMAs are the loop's only vector-memory ops):
//   resident tile: vmcnt(0), or vmcnt(1) when a lineage label was issued after its batch;
//   lineage tile:  vmcnt(9) for its label when a batch (9 ops) was issued after it, so the
//                  batch stays in flight; vmcnt(0) when the label is the youngest op -- the
//                  second of two consecutive lineage tiles, or no resident tile left.
// wid comes from readfirstlane: the role switch, the guards and the waits are scalar branches.
// The coefficient image and the epilogue's array are __shared__ objects of their own: the
// image is written before the first DMA is issued (one __syncthreads()) and read by inline
// asm only; the epilogue's array is touched only after the loop, when every DMA has been
// waited for, so a drain in front of it costs nothing.
template <int LOSS, bool SMP>
__global__ __launch_bounds__(kBlock, 3) void glm_grad_staged_kernel(
    const uint16_t* __restrict__ X, int64_t n_res, const float* __restrict__ y, const float* __restrict__ y_lin,
    const float* __restrict__ coef, const float* __restrict__ bptr, uint32_t seed, int64_t row0, int64_t n_lin,
    float* __restrict__ partial, int pstride, int64_t res_row0, const int64_t* __restrict__ t_dev, uint32_t sseed,
    uint32_t sthr, int pacc) {
  constexpr int LPR = TileStage::LPR, CPL = TileStage::CPL, UNROLL = TileStage::UNROLL, G = TileStage::G;
  constexpr int RT = G * UNROLL;
  constexpr int64_t ld = kStgLd;
  __shared__ __attribute__((aligned(256))) unsigned char slots[kWavesPerBlock * kStgWaveBytes];
  __shared__ __attribute__((aligned(256))) unsigned char frags[kStgFragBytes];
  static_assert(kStgWaveBytes % 256 == 0, "TileStage: a slot starts on a bank row");
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int g = lane / LPR, c = lane % LPR;
  const float intercept = *bptr;
  const uint32_t skey = SMP ? sample_key(sseed, (uint32_t)((t_dev ? t_dev[0] : 0) + 1)) : 0u;
  const RowSampler smp_res{skey, sthr, res_row0}, smp_lin{skey, sthr, row0};

  float w[CPL][8], acc[CPL][8];
  float wshift = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      w[k][j] = coef[8 * (c + k * LPR) + j];
      wshift += w[k][j];
      acc[k][j] = 0.f;
    }
  wshift *= kSynthShift;
  float rs = 0.f;
  float acc_r = 0.f, acc_loss = 0.f, acc_w = 0.f;

  const uint32_t Tr = (uint32_t)(n_res / RT), Tl = (uint32_t)(n_lin / RT);
  const uint32_t gw = blockIdx.x * kWavesPerBlock + wid, nw = gridDim.x * kWavesPerBlock;
  const uint32_t nr = gw < Tr ? (Tr - gw + nw - 1) / nw : 0u;     // this wave's tiles of each role
  const uint32_t nl = gw < Tl ? (Tl - gw + nw - 1) / nw : 0u;
  const uint32_t S = nr + nl;
  int64_t br = (int64_t)gw * RT, bl = br;                         // first row of the wave's current tile
  using lds_byte = __attribute__((address_space(3))) unsigned char;
  build_coef_frags(frags, coef);
  __syncthreads();   // (ahead of the first DMA: a barrier drains vmcnt)
  TileStage st{slots + wid * kStgWaveBytes,
               (uint32_t)(uintptr_t)(lds_byte*)slots + wid * kStgWaveBytes,
               (uint32_t)(uintptr_t)(lds_byte*)frags,
               reinterpret_cast<const unsigned char*>(X + br * ld),
               y + br,
               y_lin + bl,
               (int64_t)nw * RT,
               nr,
               nl,
               false};
  static_assert(RowReduce<LPR, UNROLL>::NF == 1, "TileStage::label_off: one label per lane");
  if (nl > 0) st.issue_label(g, c);
  if (nr > 0) st.issue_tile(lane);
  uint32_t rem = 0;
  for (uint32_t s = 0; s < S; ++s) {
    // tile s of the wave is a lineage tile iff floor((s + 1) nl / S) > floor(s nl / S)
    rem += nl;
    if (rem >= S) {
      rem -= S;
      grad_tile<RowsLineage, LPR, CPL, UNROLL, LOSS, SMP, true, true>(bl, n_lin, X, ld, CPL * LPR, y_lin, nullptr, seed, row0,
                                                                      w, wshift, intercept, g, c, smp_lin, acc, rs, acc_r,
                                                                      acc_loss, acc_w, &st);
      bl += st.tstep;
    } else {
      staged_resident_tile<LOSS, SMP>(br, intercept, lane, smp_res, acc, acc_r, acc_loss, acc_w, &st);
      br += st.tstep;
    }
  }
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(rs, kSynthShift, acc[k][j]);
  grad_epilogue<LPR, CPL>(acc, acc_r, acc_loss, acc_w, partial, pstride, pacc, lane, wid, c);
}

// One lane takes the next ticket (a vector atomic with return); every lane gets its value.
__device__ __forceinline__ uint32_t claim_item(uint32_t* __restrict__ ticket, int lane) {
  uint32_t t = 0;
  if (lane == 0) t = atomicAdd(ticket, 1u);
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
}
// Item i of the pass, wave-uniform (SGPRs).
__device__ __forceinline__ GlmItem uniform_item(uint32_t i, uint32_t Tr, uint32_t Tl, uint32_t items, double inv) {
  const GlmItem it = glm_item(i, Tr, Tl, items, inv);
  return GlmItem{(uint32_t)__builtin_amdgcn_readfirstlane((int)it.r0), (uint32_t)__builtin_amdgcn_readfirstlane((int)it.nr),
                 (uint32_t)__builtin_amdgcn_readfirstlane((int)it.l0), (uint32_t)__builtin_amdgcn_readfirstlane((int)it.nl)};
}
// End of an item: the wave's sums over its 8 row groups, written in full to the item's slab
// row [X^T r (DP) | sum r | loss | weight sum]; the accumulators start the next item at zero.
// The 32 column sums of a lane are reduced by recursive halving over the three group bits of
// the lane id (lane ^ 32, ^ 16, ^ 8): at each step a lane keeps one half of its values, sends
// the other half to its partner and adds what the partner sends -- 16 + 8 + 4 exchanges
// instead of the 96 of a butterfly over all 32 -- and ends with the complete sums of four
// consecutive columns, chunk c + 8 k, k = (g >> 1) & 3, floats 4 (g & 1) .. + 3: one 16-B
// store per lane covers the 256 columns.  The order is fixed (a function of the lane id).
template <int LPR, int CPL>
__device__ __forceinline__ void item_flush(float (&acc)[CPL][8], float& rs, float& acc_r, float& acc_loss,
                                           float& acc_w, float* __restrict__ dst, int lane) {
  static_assert(LPR == 8 && CPL == 4, "the halving below is written for the (8, 4) layout");
  constexpr int DP = LPR * CPL * 8;
  float a[16], b[8];
  float4_ q;
  // (the lane id made opaque here: what is derived from it -- the three selects, the store's
  // offset -- would otherwise be computed ahead of the item's tile loop and spill across it)
  const uint32_t ln = TileStage::fresh(lane);
  const bool h2 = (ln & 32) != 0, h1 = (ln & 16) != 0, h0 = (ln & 8) != 0;
  // (ds_bpermute on byte addresses formed from ln: __shfl_xor takes the lane id anew, hoisted too)
  const auto xch = [&](float v, uint32_t bit) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)((ln ^ bit) << 2), __builtin_bit_cast(int, v)));
  };
#pragma unroll
  for (int t = 0; t < 16; ++t) {   // lane ^ 32: k = 0, 1 stay in the lower half, k = 2, 3 in the upper
    const float lo = fmaf(rs, kSynthShift, acc[t >> 3][t & 7]), hi = fmaf(rs, kSynthShift, acc[2 + (t >> 3)][t & 7]);
    a[t] = (h2 ? hi : lo) + xch(h2 ? lo : hi, 32u);
  }
#pragma unroll
  for (int t = 0; t < 8; ++t)      // lane ^ 16: the chunk of the pair
    b[t] = (h1 ? a[8 + t] : a[t]) + xch(h1 ? a[t] : a[8 + t], 16u);
#pragma unroll
  for (int t = 0; t < 4; ++t)      // lane ^ 8: the half of the chunk
    q[t] = (h0 ? b[4 + t] : b[t]) + xch(h0 ? b[t] : b[4 + t], 8u);
  const float sr = wave_sum_dpp(acc_r), sl = wave_sum_dpp(acc_loss), sw = wave_sum_dpp(acc_w);
  {
    const uint32_t g = ln >> 3, cc = ln & (LPR - 1);
    *reinterpret_cast<float4_*>(dst + (8 * (cc + ((g >> 1) & 3) * LPR) + 4 * (g & 1))) = q;
  }
  if (ln == 0) {
    dst[DP] = sr;
    dst[DP + 1] = sl;
    dst[DP + 2] = sw;
  }
  zero(acc);
  rs = acc_r = acc_loss = acc_w = 0.f;
}

// The staged pass (glm_grad_staged_kernel: same tiles, slots, MFMA dot and waits) with
// persistent waves: ONE launch covers every whole tile of the pass, cut into `items` row
// items (glm_items.h), and each wave claims item after item from a ticket until none is left.
// What the sliced launches pay per block -- 32 coefficient loads, the fragment image, a
// first DMA batch with nothing to cover it, the LDS reduction, a slab read-modify-write, and
// the wait of a block's fast waves for its slowest -- is paid once per wave and pass, and the
// balancing that the 32-blocks-per-CU grid bought from the dispatcher comes from the ticket.
// Items, not blocks, are claimed, and the loop has no block barrier (the one __syncthreads()
// stands behind the fragment image): a wave that finds no item exits alone.
// Inside an item the wave interleaves its nr resident and nl lineage tiles by Bresenham as
// the staged kernel does; the tiles of a role are consecutive, so "next tile" is one tile on.
// Result: the wave ends an item by writing the item's sums to slab row i (item_flush) and
// zeroing its accumulators.  Every slab row is written once, in full, by whichever wave took
// the item, from that item's rows alone in a fixed order, so the pass's result is a function
// of (n_res, n_lin, items) only: not of the grid, nor of which wave ran what or when.
// Next item: the wave claims it just before it takes the item's LAST resident tile (an item
// of lineage tiles alone: after its last tile), so it holds no unstarted item for longer than
// one tile pair and the tail of the pass is at most one item per wave.  take_tile then
// issues the next item's first batch in place of "none after the last", and the item's last
// take_label the next item's first label: in steady state the stager never drains.  Only an
// item that follows one without tiles of that role starts its batch / label cold.
// Waits: the claim's value is used at once, so the compiler puts a vmcnt(0) behind the
// atomic.  It stands directly in front of take_tile's own wait for the batch in flight, which
// it drains a little early together with at most one label: one vmcnt(0) per item where the
// wave waits for its batch anyway, plus the atomic's round trip while the other waves of the
// SIMD issue.  The hand-counted waits of TileStage stay sufficient.  vmcnt(k) returns once at
// most k vector-memory operations are outstanding, and the loads (DMAs included) retire in
// order among themselves.  The claim is retired where it is issued.  The flush's stores are
// the only operations a TileStage wait does not know of: one that is older than the batch or
// label waited for does not change which loads may remain, and one that is still outstanding
// takes one of the k places, so fewer loads may remain than the count allows -- the wait
// retires more than it must, never less.
template <int LOSS, bool SMP>
__global__ __launch_bounds__(kBlock, 3) void glm_grad_persist_kernel(
    const uint16_t* __restrict__ X, int64_t n_res, const float* __restrict__ y, const float* __restrict__ y_lin,
    const float* __restrict__ coef, const float* __restrict__ bptr, uint32_t seed, int64_t row0, int64_t n_lin,
    float* __restrict__ islab, int pstride, int64_t res_row0, const int64_t* __restrict__ t_dev, uint32_t sseed,
    uint32_t sthr, uint32_t* __restrict__ ticket, uint32_t items, double inv_items) {
  constexpr int LPR = TileStage::LPR, CPL = TileStage::CPL, UNROLL = TileStage::UNROLL, G = TileStage::G;
  constexpr int RT = G * UNROLL;
  constexpr int64_t ld = kStgLd;
  __shared__ __attribute__((aligned(256))) unsigned char slots[kWavesPerBlock * kStgWaveBytes];
  __shared__ __attribute__((aligned(256))) unsigned char frags[kStgFragBytes];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int g = lane / LPR, c = lane % LPR;
  const float intercept = *bptr;
  const uint32_t skey = SMP ? sample_key(sseed, (uint32_t)((t_dev ? t_dev[0] : 0) + 1)) : 0u;
  const RowSampler smp_res{skey, sthr, res_row0}, smp_lin{skey, sthr, row0};

  float w[CPL][8], acc[CPL][8];
  float wshift = 0.f;
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      w[k][j] = coef[8 * (c + k * LPR) + j];
      wshift += w[k][j];
      acc[k][j] = 0.f;
    }
  wshift *= kSynthShift;
  float rs = 0.f;
  float acc_r = 0.f, acc_loss = 0.f, acc_w = 0.f;

  const uint32_t Tr = (uint32_t)(n_res / RT), Tl = (uint32_t)(n_lin / RT);
  using lds_byte = __attribute__((address_space(3))) unsigned char;
  build_coef_frags(frags, coef);
  __syncthreads();   // (ahead of the first DMA: a barrier drains vmcnt; the only barrier of the kernel)
  TileStage st{slots + wid * kStgWaveBytes,
               (uint32_t)(uintptr_t)(lds_byte*)slots + wid * kStgWaveBytes,
               (uint32_t)(uintptr_t)(lds_byte*)frags,
               nullptr,
               nullptr,
               nullptr,
               (int64_t)RT,
               0u,
               0u,
               false,
               reinterpret_cast<const unsigned char*>(X),
               y,
               y_lin,
               0u,
               0u,
               0u,
               0u,
               false,
               false};
  uint32_t cur = claim_item(ticket, lane);
  if (cur >= items) return;
  GlmItem it = uniform_item(cur, Tr, Tl, items, inv_items);
  for (;;) {
    const uint32_t nr = it.nr, nl = it.nl, S = nr + nl;
    int64_t br = (int64_t)it.r0 * RT, bl = (int64_t)it.l0 * RT;   // first row of the current tile of each role
    // the item's first label and batch, unless the item before has sent them ahead
    if (nl > 0 && !st.l_pre) {
      st.yls = y_lin + bl;
      st.l_ahead = nl;
      st.issue_label(g, c);
    }
    if (nr > 0 && !st.r_pre) {
      st.xs = st.x0 + br * (ld * 2);
      st.yrs = y + br;
      st.r_ahead = nr;
      st.issue_tile(lane);
    }
    st.r_pre = st.l_pre = false;
    st.nx_nr = st.nx_nl = 0u;
    uint32_t nxt = items;
    GlmItem nx{0u, 0u, 0u, 0u};
    bool claimed = false;
    const auto claim_next = [&]() {
      claimed = true;
      nxt = claim_item(ticket, lane);
      if (nxt < items) {
        nx = uniform_item(nxt, Tr, Tl, items, inv_items);
        st.nx_r0 = nx.r0;
        st.nx_nr = nx.nr;
        st.nx_l0 = nx.l0;
        st.nx_nl = nx.nl;
      }
    };
    uint32_t rem = 0, r_left = nr;
    for (uint32_t s = 0; s < S; ++s) {
      // tile s of the item is a lineage tile iff floor((s + 1) nl / S) > floor(s nl / S)
      rem += nl;
      if (rem >= S) {
        rem -= S;
        grad_tile<RowsLineage, LPR, CPL, UNROLL, LOSS, SMP, true, true, true>(bl, n_lin, X, ld, CPL * LPR, y_lin, nullptr,
                                                                              seed, row0, w, wshift, intercept, g, c,
                                                                              smp_lin, acc, rs, acc_r, acc_loss, acc_w, &st);
        bl += RT;
      } else {
        if (r_left == 1) claim_next();
        --r_left;
        staged_resident_tile<LOSS, SMP, true>(br, intercept, lane, smp_res, acc, acc_r, acc_loss, acc_w, &st);
        br += RT;
      }
    }
    if (!claimed) claim_next();
    item_flush<LPR, CPL>(acc, rs, acc_r, acc_loss, acc_w, islab + (int64_t)cur * pstride, lane);
    if (nxt >= items) break;
    cur = nxt;
    it = nx;
  }
}

// Sum of the item slab, level 1: block b adds the slab rows [b kItemChunk, (b + 1) kItemChunk)
// column by column in fp64, in row order, into mid row b.  Level 2 (glm_finish_f64_kernel)
// adds the mid rows in a fixed order.  The chunk is a constant: the sum's order depends on the
// number of slab rows alone.
constexpr int kItemChunk = 256, kItemSumBlock = 320;
__global__ __launch_bounds__(kItemSumBlock) void glm_item_sum_kernel(const float* __restrict__ slab, int64_t nrows,
                                                                    int pstride, int ncols,
                                                                    double* __restrict__ mid) {
  const int64_t lo = (int64_t)blockIdx.x * kItemChunk;
  const int64_t hi = lo + kItemChunk < nrows ? lo + kItemChunk : nrows;
  for (int i = threadIdx.x; i < ncols; i += kItemSumBlock) {
    double s = 0.0;
#pragma unroll 8
    for (int64_t r = lo; r < hi; ++r) s += (double)__builtin_nontemporal_load(slab + r * pstride + i);
    mid[(int64_t)blockIdx.x * pstride + i] = s;
  }
}

// ---------------------------------------------------------------------------
// Summarizer pass of a gradient-descent fit, fused with its first gradient: per column
// s1 = sum w x, s2 = sum w x^2 and syx = sum w y x, per row sum w, sum w y, sum w y^2,
// over the resident rows of X and n_lin lineage rows in ONE interleaved launch (same
// tile schedule as glm_grad_mixed_kernel).  At the initial iterate every coefficient is
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
// glm_item_sum_kernel), same order.
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

// The persistent staged pass (glm_grad_persist_kernel): whether a pass takes it, and the item
// slab it then needs.  persist: 0 = never; 1 = a staged-eligible pass (full_tiles, 256-column
// bf16 rows, unweighted, `staged` as in o3s_glm_grad_mixed, taken over the whole tiles of the
// pass) that holds both roles and has at least 64 items per resident wave -- a smaller pass
// keeps its sliced launches, whose grid is already cut to its size; 2 = every staged-eligible
// pass (tests).  items == 0: not taken.
struct PersistPlan { int64_t items, slab_floats, mid_doubles; };
// What __launch_bounds__(kBlock, 3) and 43 KB of LDS allow.  The threshold of persist == 1 is
// formed from this constant, not from the occupancy the launch queries per instantiation, so
// that whether a pass takes the kernel (o3s_glm_persist_plan) does not depend on loss or sampler.
constexpr int kPersistBlocksPerCu = 3;
constexpr int kMaxDevices = 64;
int current_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kMaxDevices ? dev : -1;
}
int device_cus() {
  static int cus[kMaxDevices] = {};
  const int dev = current_device();
  if (dev < 0) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}
PersistPlan persist_plan(int64_t ld, int64_t n_res, int64_t n_lin, bool weighted, int full_tiles, int staged,
                         int persist, int item_tiles, int pstride) {
  constexpr int64_t RT = TileStage::G * TileStage::UNROLL;
  const PersistPlan none{0, 0, 0};
  if (persist <= 0 || item_tiles <= 0 || !full_tiles || ld != kStgLd || weighted || n_res < 0 || n_lin < 0) return none;
  const uint64_t Tr = (uint64_t)(n_res / RT), Tl = (uint64_t)(n_lin / RT);
  if (Tr + Tl == 0 || Tr >= kGlmItemMaxTiles || Tl >= kGlmItemMaxTiles) return none;
  if (!(staged >= 2 || (staged == 1 && Tr > 0 && Tl > 0))) return none;
  const uint64_t items = glm_item_count(Tr, Tl, (uint64_t)item_tiles);
  if (items > kGlmItemMaxTiles) return none;
  if (persist == 1) {
    const uint64_t waves = (uint64_t)kPersistBlocksPerCu * device_cus() * kWavesPerBlock;
    if (Tr == 0 || Tl == 0 || items < 64 * waves) return none;
  }
  const int64_t rows = (int64_t)items + 1;   // the last row is the ragged rows' launch's
  return PersistPlan{(int64_t)items, rows * pstride, (rows + kItemChunk - 1) / kItemChunk * pstride};
}
template <int LOSS, bool SMP>
int persist_blocks_per_cu() {   // cached per device and instantiation
  static int occ[kMaxDevices] = {};
  const int dev = current_device();
  if (dev < 0) return 1;
  if (occ[dev] == 0) {
    int o = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, glm_grad_persist_kernel<LOSS, SMP>, kBlock, 0) != hipSuccess ||
        o < 1)
      o = 1;
    occ[dev] = o;
  }
  return occ[dev];
}
// out[0..ncols) = the column sums of slab rows 0 .. nrows - 1, in fp64, in an order that
// depends on nrows alone (two levels: glm_item_sum_kernel, glm_finish_f64_kernel).
int launch_item_finish(const float* islab, int64_t nrows, int pstride, int ncols, double* imid, double* out,
                       hipStream_t st) {
  const int chunks = (int)((nrows + kItemChunk - 1) / kItemChunk);
  hipLaunchKernelGGL(glm_item_sum_kernel, dim3(chunks), dim3(kItemSumBlock), 0, st, islab, nrows, pstride, ncols, imid);
  O3S_CHECK_LAUNCH();
  hipLaunchKernelGGL(glm_finish_f64_kernel, dim3((ncols + 31) / 32), dim3(1024), 0, st, imid, chunks, pstride, ncols,
                     out);
  O3S_CHECK_LAUNCH();
  return 0;
}

}  // namespace

// What o3s_glm_grad_mixed with the same arguments needs for the persistent staged pass: the
// number of items (0: the pass does not take it) and the sizes of the item slab (floats) and
// of its fp64 mid rows.
O3S_API int o3s_glm_persist_plan(int64_t ld, int64_t n_res, int64_t n_lin, int weighted, int full_tiles, int staged,
                                 int persist, int item_tiles, int64_t* items, int64_t* slab_floats,
                                 int64_t* mid_doubles) {
  Layout l;
  if (!resolve_layout(ld, &l)) return -1;
  const PersistPlan p = persist_plan(ld, n_res, n_lin, weighted != 0, full_tiles, staged, persist, item_tiles, l.dpad + 4);
  *items = p.items;
  *slab_floats = p.slab_floats;
  *mid_doubles = p.mid_doubles;
  return 0;
}

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

// Mixed resident + lineage pass in one launch (see glm_grad_mixed_kernel): n_res rows
// of X plus n_lin synthetic rows starting at global row row0; y / sw cover all
// n_res + n_lin rows.  Same out / coef / partial
// contract as o3s_glm_grad (out is overwritten).  waves: 3 asks the register allocator
// for 3 waves/SIMD (see glm_grad_mixed_kernel), anything else 2.  Mini-batch sampling: res_row0 is the global
// index of resident row 0, t_dev (may be null = iteration 1) the device step counter,
// sthr = fraction * 2^24 (>= 2^24: no sampling), sseed the sampling seed.  splits: see
// for_row_slices.
// full_tiles: where ld is the layout's full width, the slices are cut at whole tiles and
// run through the mask-free kernel, and the fewer than RT rows that remain of each role go
// through the masked kernel in one more launch of one block, which adds into slab row 0
// (pacc; every other slab row stays as the slices left it).  0: masked kernel throughout.
// staged: 1 = the whole-tile slices of an unweighted pass over the 8x4 layout
// (256-column rows) that hold rows of both roles run through glm_grad_staged_kernel; 2 = those
// of one role alone too; every other case, and 0, takes the kernels above.
// persist / item_tiles: see persist_plan.  A pass that takes the persistent kernel runs all its
// whole tiles in ONE launch of min(blocks that fit the card, items / 4) blocks -- `grid` and
// `splits` do not shape it -- whose waves claim items from *ticket (zeroed here, on st); item i
// goes to row i of islab, the ragged rows' launch to row `items`, and the two-level finish
// sums those rows through imid into out.  Such a pass neither reads nor writes `partial`.
// persist_blocks > 0 caps that launch's blocks (tests: one block takes its four waves through
// every item; the result does not depend on it).
// Returns -2, and launches nothing, when islab / imid are smaller than o3s_glm_persist_plan
// says or the ticket is missing.
O3S_API int o3s_glm_grad_mixed(int loss, const void* X, int64_t ld, int64_t n_res, const float* y,
                               const float* sw, const float* coef, uint32_t seed, int64_t row0,
                               int64_t n_lin, float* partial, int grid, double* out, int waves,
                               int64_t res_row0, const int64_t* t_dev, uint32_t sseed,
                               uint32_t sthr, int splits, int full_tiles, int staged, int persist, int item_tiles,
                               float* islab, int64_t islab_floats, double* imid, int64_t imid_doubles,
                               uint32_t* ticket, int persist_blocks, hipStream_t st) {
  Layout l;
  if (!resolve_layout(ld, &l) || grid <= 0 || n_res < 0 || n_lin < 0) return -1;
  const int pstride = l.dpad + 4;
  const PersistPlan plan = persist_plan(ld, n_res, n_lin, sw != nullptr, full_tiles, staged, persist, item_tiles, pstride);
  if (plan.items > 0 && (!islab || !imid || !ticket || islab_floats < plan.slab_floats ||
                         imid_doubles < plan.mid_doubles))
    return -2;
  bool persisted = false;
  const uint16_t* Xh = (const uint16_t*)X;
  const bool smp = sthr < (1u << 24);
  const int rc = with_remapped_layout_and_loss(l, loss, [&](auto L, auto C, auto LOSS) {
    constexpr int U = C >= 8 ? 1 : 8 / C;
    constexpr int64_t RT = (kWave / L) * U;
    // rows [r_lo, r_lo + r_n) of X and lineage rows [l_lo, l_lo + l_n) in one launch
    auto slice = [&](auto FULL, int g, int64_t r_lo, int64_t r_n, int64_t l_lo, int64_t l_n, int pacc,
                     float* partial) {
      // the mask-free kernel reads whole tiles unguarded: never launch it on anything else
      if (FULL && (r_n % RT != 0 || l_n % RT != 0 || ld != 8 * L * C)) return -1;
      const float* y_lin = y + n_res + l_lo;
      const float* sw_lin = sw ? sw + n_res + l_lo : nullptr;
      if constexpr (decltype(FULL)::value && L == TileStage::LPR && C == TileStage::CPL) {
        static_assert(U == TileStage::UNROLL, "the staged kernel's tile");
        // whole tiles of the bench layout, unweighted: resident tiles staged through LDS (one
        // build, 3 waves/SIMD, whatever `waves` says; its tile counters are 32-bit)
        // (1: slices that hold both roles -- a single role alone measured 3-5 % slower staged
        // than unstaged, it has no lineage tile to cover; 2: every eligible slice, for tests)
        const bool wanted = staged >= 2 || (staged == 1 && r_n > 0 && l_n > 0);
        if (wanted && !sw && r_n / RT < (int64_t(1) << 31) && l_n / RT < (int64_t(1) << 31)) {
          auto go_staged = [&](auto SMP) {
            launch(glm_grad_staged_kernel<LOSS, SMP>, g, st, Xh + r_lo * ld, r_n, y + r_lo, y_lin, coef, coef + l.dpad,
                   seed, row0 + l_lo, l_n, partial, pstride, res_row0 + r_lo, t_dev, sseed, sthr, pacc);
          };
          if (smp) go_staged(std::true_type{});
          else go_staged(std::false_type{});
          return 0;
        }
      }
      auto go = [&](auto MW, auto SMP) {
        launch(glm_grad_mixed_kernel<L, C, U, LOSS, MW, SMP, FULL>, g, st, Xh + r_lo * ld, ld, r_n, y + r_lo,
               sw ? sw + r_lo : nullptr, y_lin, sw_lin, coef, coef + l.dpad, seed, row0 + l_lo, l_n, partial, pstride,
               res_row0 + r_lo, t_dev, sseed, sthr, pacc);
      };
      if (waves == 3 && smp) go(IC<3>{}, std::true_type{});
      else if (waves == 3) go(IC<3>{}, std::false_type{});
      else if (smp) go(IC<2>{}, std::true_type{});
      else go(IC<2>{}, std::false_type{});
      return 0;
    };
    // (the 32x4 and 64x4 layouts have no mask-free kernel: built for 3 waves/SIMD it spills
    // where its masked twin does not)
    constexpr bool kHasFull = !(L >= 32 && C == 4);
    const int64_t r_full = n_res / RT * RT, l_full = n_lin / RT * RT;
    if constexpr (L == TileStage::LPR && C == TileStage::CPL) {
      if (plan.items > 0) {
        // every whole tile of the pass in one launch of persistent waves
        persisted = true;
        if (hipMemsetAsync(ticket, 0, sizeof(uint32_t), st) != hipSuccess) return -3;
        auto go_persist = [&](auto SMP) {
          int64_t fit = (int64_t)persist_blocks_per_cu<LOSS, SMP>() * device_cus();
          if (persist_blocks > 0 && persist_blocks < fit) fit = persist_blocks;
          const int64_t need = (plan.items + kWavesPerBlock - 1) / kWavesPerBlock;
          launch(glm_grad_persist_kernel<LOSS, SMP>, (int)(fit < need ? fit : need), st, Xh, r_full, y, y + n_res, coef,
                 coef + l.dpad, seed, row0, l_full, islab, pstride, res_row0, t_dev, sseed, sthr, ticket,
                 (uint32_t)plan.items, glm_item_inv((uint64_t)plan.items));
        };
        if (smp) go_persist(std::true_type{});
        else go_persist(std::false_type{});
        O3S_CHECK_LAUNCH();
        int64_t rows = plan.items;
        if (r_full != n_res || l_full != n_lin) {
          // the ragged rows: one block of the masked kernel, which writes slab row `items` in full
          const int rc2 = slice(std::false_type{}, 1, r_full, n_res - r_full, l_full, n_lin - l_full, 0,
                                islab + plan.items * pstride);
          O3S_CHECK_LAUNCH();
          if (rc2 != 0) return rc2;
          ++rows;
        }
        return launch_item_finish(islab, rows, pstride, l.dpad + 3, imid, out, st);
      }
    }
    if constexpr (kHasFull) {
      if (full_tiles && ld == 8 * L * C && r_full + l_full > 0) {
        const int rc = for_row_slices(
            splits, n_res, n_lin,
            [&](int64_t r_lo, int64_t r_n, int64_t l_lo, int64_t l_n, int pacc) {
              return slice(std::true_type{}, grid, r_lo, r_n, l_lo, l_n, pacc, partial);
            },
            RT);
        if (rc != 0 || (r_full == n_res && l_full == n_lin)) return rc;
        const int rc2 = slice(std::false_type{}, 1, r_full, n_res - r_full, l_full, n_lin - l_full, 1, partial);
        O3S_CHECK_LAUNCH();
        return rc2;
      }
    }
    return for_row_slices(splits, n_res, n_lin, [&](int64_t r_lo, int64_t r_n, int64_t l_lo, int64_t l_n, int pacc) {
      return slice(std::false_type{}, grid, r_lo, r_n, l_lo, l_n, pacc, partial);
    });
  });
  if (rc != 0 || persisted) return rc;
  return launch_finish(partial, grid, pstride, l.dpad + 3, out, 0, st);
}

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

// Fused summarizer + first-gradient pass (glm_stats_mixed_kernel): out (fp64, 3*dpad+3) =
// [s1 | s2 | syx | sum w | sum w y | sum w y^2]; partial holds (grid + 1) * (3*dpad+4) floats.
// Returns -2 when the row layout has no stats instantiation (ld > 2048): the caller then
// uses o3s_glm_colstats plus a regular first pass.
// full_tiles: as in o3s_glm_grad_mixed -- the whole tiles of both roles run through the
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

// ---------------------------------------------------------------------------------
// Multinomial (softmax) logistic regression, one fused pass over bf16 rows:
//   margins M = X W^T + b (MFMA), row log-sum-exp, residual R = w (softmax(M) - onehot(y)),
//   gradient G = R^T X (MFMA), sum(R) per class and the weighted cross-entropy.
// Reference: Spark's MultinomialLogisticRegression aggregator reached from the
// Classification widget (orangecontrib/spark/widgets/ml/spark_ml_classification.py:15,
// SURVEY §2.8 "Multinomial: X.W with C classes uses MFMA").
//
// Layout (v_mfma_f32_32x32x16_bf16; lane (r = lane&31, h = lane>>5)):
//   forward  A = W split (32 classes x 16 dims, class r, dims 8h..+8), B = X (row r, the
//            same 8 dims -- exactly the 16-B global load of the row) -> acc[v] = margin of
//            row r, class 8(v>>2) + 4h + (v&3);
//   backward A = R split (class r, rows 8h..+8 of a 16-row step), B = X^T (rows 8h..+8,
//            dim r of a 32-dim block, read transposed from this wave's LDS copy of the
//            tile) -> G[nb][v] = dG of class 8(v>>2) + 4h + (v&3), dim 32 nb + r.
// X is exact in bf16; W is split into three bf16 terms (hi + mid + lo: margins and loss
// at fp32 level), the residuals R (|R| <= w) into two (hi + lo: ~2^-17 relative per term
// of the gradient sums).  The MFMA
// work is a few % of the HBM time of a tile: the kernel streams X once per pass (the
// next tile's rows are loaded while this tile computes).  One wave per SIMD (the
// 128-register gradient accumulators); per-wave slab rows, summed in fp64 by
// glm_finish_kernel in a fixed order (no float atomics).
namespace {

typedef float sm_f32x16 __attribute__((ext_vector_type(16)));
typedef short sm_bf16x8 __attribute__((ext_vector_type(8)));
constexpr int kSmWaves = 4;
constexpr int kSmThreads = kSmWaves * kWave;

template <int NB>
struct SmLds {
  static constexpr int D = 32 * NB;
  static constexpr int WLD = D + 8;     // +16 B per row: conflict-free 16-B fragment reads
  static constexpr int XLD = D + 8;
  static constexpr int RLD = 40;        // 80-B rows: the 16-B R fragment reads hit distinct banks
  static constexpr int W_ELEMS = 3 * 32 * WLD;
  static constexpr int WAVE_ELEMS = 32 * XLD + 2 * 32 * RLD;
  static constexpr int ELEMS = W_ELEMS + kSmWaves * WAVE_ELEMS;
};

template <int NB>
__global__ __launch_bounds__(kSmThreads, 1) void glm_softmax_kernel(
    const uint16_t* __restrict__ X, int64_t n, int64_t ldx, const int32_t* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ bias, int K,
    float* __restrict__ partial, int pstride) {
  using L = SmLds<NB>;
  constexpr int D = L::D, KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;
  uint16_t* Rs = Xs + 32 * XLD;

  // W splits [3][32][D] -> LDS (padded rows)
  for (int p = threadIdx.x; p < 3 * 32 * (D / 8); p += kSmThreads) {
    const int row = p / (D / 8), k8 = p % (D / 8);
    *reinterpret_cast<sm_bf16x8*>(Ws + row * WLD + k8 * 8) =
        *reinterpret_cast<const sm_bf16x8*>(Wsp + (int64_t)row * D + k8 * 8);
  }
  float bl[16];
  int cls[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    cls[v] = 8 * (v >> 2) + 4 * h + (v & 3);
    bl[v] = cls[v] < K ? bias[cls[v]] : -INFINITY;
  }
  __syncthreads();

  sm_f32x16 G[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) G[b][v] = 0.f;
  float gb[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) gb[v] = 0.f;
  float lossacc = 0.f;

  const int64_t ntiles = (n + 31) / 32;
  const int64_t step = (int64_t)gridDim.x * kSmWaves;
  int64_t tile = (int64_t)blockIdx.x * kSmWaves + wid;
  sm_bf16x8 xb[KS], xn[KS];
  auto load = [&](int64_t t, sm_bf16x8 (&dst)[KS]) {
    int64_t row = t * 32 + r;
    row = row < n ? row : n - 1;
    const uint16_t* src = X + row * ldx;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int col = ks * 16 + 8 * h;
      if (col < ldx) {
        dst[ks] = *reinterpret_cast<const sm_bf16x8*>(src + col);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[ks][j] = 0;
      }
    }
  };
  if (tile < ntiles) load(tile, xb);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) load(tile + step, xn);
    const int64_t row = tile * 32 + r;
    const bool valid = row < n;
    const int yl = valid ? y[row] : -1;
    const float wr = valid ? (sw ? sw[row] : 1.f) : 0.f;
    // ---- forward: margins of row r, 16 classes per lane
    sm_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = bl[v];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const sm_bf16x8 a = *reinterpret_cast<const sm_bf16x8*>(Ws + (s * 32 + r) * WLD + ks * 16 + 8 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, xb[ks], acc, 0, 0, 0);
      }
      *reinterpret_cast<sm_bf16x8*>(Xs + r * XLD + ks * 16 + 8 * h) = xb[ks];   // for the X^T reads
    }
    // ---- row softmax (the two half-waves hold disjoint class subsets of row r)
    float mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) mx = fmaxf(mx, acc[v]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float se = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) se += __expf(acc[v] - mx);
    se += __shfl_xor(se, 32, 64);
    const float lse = mx + __logf(se);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const bool hit = cls[v] == yl;
      const float p = __expf(acc[v] - lse);
      const float rv = wr * (p - (hit ? 1.f : 0.f));
      gb[v] += rv;
      if (hit) lossacc += wr * (lse - acc[v]);
      const uint16_t a0 = f32_to_bf16(rv);
      Rs[(0 * 32 + cls[v]) * RLD + r] = a0;
      Rs[(1 * 32 + cls[v]) * RLD + r] = f32_to_bf16(rv - bf16_to_f32(a0));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // ---- backward: G[class][dim] += sum over the tile's rows of R[row][class] X[row][dim]
    sm_bf16x8 ar[2][2];
#pragma unroll
    for (int rs = 0; rs < 2; ++rs)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        ar[rs][s] = *reinterpret_cast<const sm_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        sm_bf16x8 bx;
#pragma unroll
        for (int q = 0; q < 8; ++q) bx[q] = (short)Xs[(rs * 16 + 8 * h + q) * XLD + b * 32 + r];
#pragma unroll
        for (int s = 0; s < 2; ++s) G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][s], bx, G[b], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // tile's LDS reads done before it is overwritten
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xb[ks] = xn[ks];
  }
  // ---- this wave's slab row: [G class-major 32 x D | sum R (32) | loss]
  float* out = partial + ((int64_t)blockIdx.x * kSmWaves + wid) * pstride;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) out[cls[v] * D + b * 32 + r] = G[b][v];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float s = gb[v];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);   // over the 32 rows (same h)
    if (r == 0) out[32 * D + cls[v]] = s;
  }
  const float lt = wave_sum(lossacc);
  if (lane == 0) out[32 * D + 32] = lt;
}

}  // namespace

// One multinomial pass: out (fp64, [32 * D | 32 | 1]) = (gradient class-major over
// D = 32 * ceil(d / 32) dims, per-class residual sums, weighted cross-entropy) over the n
// rows of X (bf16, row stride ldx, ldx % 8 == 0).  y: int32 labels in [0, K); sw: fp32
// weights or null; Wsp: bf16 [3][32][D] (hi, mid, lo splits of the class-major
// coefficients, zero-padded); bias: fp32 [32].  partial: fp32 [grid * 4][32 D + 33].
O3S_API int o3s_glm_softmax(const void* X, int64_t n, int64_t ldx, int d, const int32_t* y, const float* sw,
                            const void* Wsp, const float* bias, int K, float* partial, int grid, double* out,
                            hipStream_t st) {
  const int nb = (d + 31) / 32;
  if (ldx % 8 != 0 || nb < 1 || nb > 8 || K < 1 || K > 32 || grid <= 0) return -1;
  const int D = 32 * nb, pstride = 32 * D + 33;
  const uint16_t* Xh = (const uint16_t*)X;
  const uint16_t* Wh = (const uint16_t*)Wsp;
  if (n > 0) {
    switch (nb) {
#define O3S_SM(NBV) \
  case NBV: hipLaunchKernelGGL((glm_softmax_kernel<NBV>), dim3(grid), dim3(kSmThreads), 0, st, Xh, n, ldx, y, sw, \
                               Wh, bias, K, partial, pstride); break;
      O3S_SM(1) O3S_SM(2) O3S_SM(3) O3S_SM(4) O3S_SM(5) O3S_SM(6) O3S_SM(7) O3S_SM(8)
#undef O3S_SM
      default: return -1;
    }
  } else {
    hipMemsetAsync(partial, 0, sizeof(float) * pstride * (size_t)grid * kSmWaves, st);
  }
  O3S_CHECK_LAUNCH();
  hipLaunchKernelGGL(glm_finish_kernel, dim3((pstride + 31) / 32), dim3(1024), 0, st, partial, grid * kSmWaves,
                     pstride, pstride, out, 0);
  O3S_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------
// fp32 feature rows (o3s.vector.dtype=float32): the passes above over X = float [n, ld]
// (ld % 8 == 0, zero padded), with the RowsF32 source.  What that source changes: an
// 8-column chunk is 32 B, two 16-B loads per lane, and the row is held once, unpacked as
// loaded, for the dot product and for X^T r -- twice the row registers of the bf16 kernels,
// so the rows in flight and the register budget are chosen per layout (F32Cfg) to stay out
// of scratch.  fp32 rows never have lineage rows (lineage storage is bf16): one plain
// streaming tile walk per kernel, no lineage code in any instantiation.  The stats, margin
// and column-moment kernels instantiate the shared bodies; the gradient kernel keeps its own
// tile (below).  The lane -> column
// mapping (the remapped layouts), the slab layout and the fp64 finish are those of the mixed
// pass, so o3s_glm_layout, the workspace, the SGD update kernels and a captured DeviceSGD
// step serve both dtypes.
namespace {

// Gradient pass (contract of glm_grad_mixed_kernel's resident role).  It shares the row
// source's load / mask, loss_terms, the row reduction and grad_epilogue with the other
// gradient kernels, but NOT grad_tile: instantiated as grad_tile<RowsF32> the same statements
// cost 2-6 VGPRs in every layout -- 3 -> 2 waves/SIMD in <4,4,2,*,true>, dot[] spilled to LDS
// in <4,1,8> -- and hipcc contracts the weighted loss line differently (last-bit changes in
// sum r / loss).  Written here, in the kernel, the tile keeps its registers and its bits.
template <int LPR, int CPL, int UNROLL, int LOSS, int MW, bool SMP>
__global__ __launch_bounds__(kBlock, MW) void glm_grad_f32_kernel(
    const float* __restrict__ X, int64_t ld, int64_t n, const float* __restrict__ y, const float* __restrict__ sw,
    const float* __restrict__ coef, const float* __restrict__ bptr, float* __restrict__ partial, int pstride,
    int64_t res_row0, const int64_t* __restrict__ t_dev, uint32_t sseed, uint32_t sthr, int pacc) {
  constexpr int G = kWave / LPR;
  constexpr int RT = G * UNROLL;
  using RR = RowReduce<LPR, UNROLL>;
  constexpr int NF = RR::NF;
  constexpr bool kDpp = LPR == 8 && UNROLL == 2;
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
  const int g = lane / LPR, c = lane % LPR;
  const int nch = (int)(ld / 8);
  const int ubase = RR::base(c);
  const bool rep = RR::representative(c);
  const float intercept = *bptr;
  const uint32_t skey = SMP ? sample_key(sseed, (uint32_t)((t_dev ? t_dev[0] : 0) + 1)) : 0u;
  const RowSampler smp{skey, sthr, res_row0};

  // (written out, not load_coef: the helper cost 4 VGPRs in every layout of this kernel)
  float w[CPL][8], acc[CPL][8];
#pragma unroll
  for (int k = 0; k < CPL; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = 8 * (c + k * LPR) + j;
      w[k][j] = col < ld ? coef[col] : 0.f;
      acc[k][j] = 0.f;
    }
  float acc_r = 0.f, acc_loss = 0.f, acc_w = 0.f;

  const int64_t ntiles = (n + RT - 1) / RT;
  const int64_t gw = (int64_t)blockIdx.x * kWavesPerBlock + wid;
  const int64_t nw = (int64_t)gridDim.x * kWavesPerBlock;
  for (int64_t t = gw; t < ntiles; t += nw) {
    const int64_t base = t * RT;
    float4_ xv[UNROLL][CPL][2];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t row = base + u * G + g;
      const bool ok = row < n;
      const int64_t rowc = ok ? row : n - 1;
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int ch = c + k * LPR;
        const int chc = ch < nch ? ch : nch - 1;
        RowsF32::chunk v;
        RowsF32::load(X, ld, rowc, chc, v);
        RowsF32::mask(v, ok && ch < nch);
        xv[u][k][0] = v.lo;
        xv[u][k][1] = v.hi;
      }
    }
    float yy[NF], ww[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      const int64_t row = base + (ubase + j) * G + g;
      const bool ok = row < n;
      const int64_t rowc = ok ? row : n - 1;
      const float yv = y[rowc];
      const float wv = sw ? sw[rowc] : 1.f;
      yy[j] = ok ? yv : 0.f;
      ww[j] = ok ? wv : 0.f;
      if constexpr (SMP) {
        if (!smp.keep(row)) ww[j] = 0.f;
      }
    }
    float dot[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      // two interleaved partial sums -> v_pk_fma_f32 (one issue per two features)
      float2_ d2 = {0.f, 0.f};
#pragma unroll
      for (int k = 0; k < CPL; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int j = 0; j < 4; j += 2) {
            const float2_ xx = {xv[u][k][h][j], xv[u][k][h][j + 1]};
            const float2_ ww2 = {w[k][4 * h + j], w[k][4 * h + j + 1]};
            d2 = __builtin_elementwise_fma(xx, ww2, d2);
          }
      dot[u] = d2.x + d2.y;
    }
    if constexpr (kDpp) row_reduce_8x2(dot, c);
    else RR::run(dot, c);
    float res[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) {
      float r, l;
      loss_terms<LOSS>(dot[j] + intercept, yy[j], ww[j], r, l);
      res[j] = r;
      if (rep) { acc_r += r; acc_loss += l; acc_w += ww[j]; }
    }
    float other = 0.f;
    if constexpr (kDpp) other = dpp_f<kDppHalfMirror>(res[0]);   // the other row's residual
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      float r;
      if constexpr (kDpp) r = ((c & 4) != 0) == (u == 0) ? other : res[0];
      else r = __shfl(res[u % NF], g * LPR + RR::owner(u), kWave);
#pragma unroll
      for (int k = 0; k < CPL; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[k][4 * h + j] = fmaf(r, xv[u][k][h][j], acc[k][4 * h + j]);
    }
  }

  grad_epilogue<LPR, CPL>(acc, acc_r, acc_loss, acc_w, partial, pstride, pacc, lane, wid, c);
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

// Rows in flight per lane (U) and waves per SIMD asked of the register allocator (MW) of
// the fp32 gradient pass, per chunks-per-lane: the widest layouts keep one row at a time
// and one wave per SIMD so that w + acc + the row stay in registers.
template <int C> struct F32Cfg { static constexpr int U = C >= 8 ? 1 : 8 / C, MW = C >= 8 ? 1 : 2; };

}  // namespace

// Gradient/loss pass over fp32 rows: the out / coef / partial contract of o3s_glm_grad
// (accumulate adds into out) with the mini-batch sampler and the splits loop of
// o3s_glm_grad_mixed.  n_lin must be 0: fp32 rows have no lineage rows.
O3S_API int o3s_glm_grad_f32(int loss, const void* X, int64_t ld, int64_t n, const float* y, const float* sw,
                             const float* coef, int64_t n_lin, float* partial, int grid, double* out,
                             int accumulate, int64_t res_row0, const int64_t* t_dev, uint32_t sseed, uint32_t sthr,
                             int splits, hipStream_t st) {
  Layout l;
  if (ld <= 0 || !resolve_layout(ld, &l) || grid <= 0 || n < 0 || n_lin != 0) return -1;
  const int pstride = l.dpad + 4;
  const float* Xf = (const float*)X;
  const bool smp = sthr < (1u << 24);
  const int rc = for_row_slices(splits, n, 0, [&](int64_t r_lo, int64_t r_n, int64_t, int64_t, int pacc) {
    return with_remapped_layout_and_loss(l, loss, [&](auto L, auto C, auto LOSS) {
      constexpr int U = F32Cfg<C>::U, MW = F32Cfg<C>::MW;
      auto go = [&](auto SMP) {
        launch(glm_grad_f32_kernel<L, C, U, LOSS, MW, SMP>, grid, st, Xf + r_lo * ld, ld, r_n, y + r_lo,
               sw ? sw + r_lo : nullptr, coef, coef + l.dpad, partial, pstride, res_row0 + r_lo, t_dev, sseed, sthr,
               pacc);
      };
      if (smp) go(std::true_type{});
      else go(std::false_type{});
      return 0;
    });
  });
  if (rc != 0) return rc;
  return launch_finish(partial, grid, pstride, l.dpad + 3, out, accumulate, st);
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

// ---------------------------------------------------------------------------------
// Multinomial pass over fp32 rows: the contract, MFMA layouts, slab rows and finish of
// glm_softmax_kernel above, for X = float [n, ldx].
//
// gfx950 has no xf32 and its f32-input MFMA runs at 1/16 of the bf16 rate, so a row is
// split into bf16 terms as it is consumed (v_cvt_pk_bf16_f32 of the running remainder,
// every subtraction exact): hi + mid + lo forward, where the margins and the loss have to
// be at fp32 level, hi + mid backward (2^-17 relative, below the two-term split of R).
// Forward products of total order <= 2 only (X hi with the three W terms, X mid with W hi
// and mid, X lo with W hi: 6 MFMAs per 16 dims where the bf16 kernel issues 3); backward
// all four of (R hi, R lo) x (X hi, X mid).
//
// Budget.  An fp32 tile is twice the bytes of a bf16 one, so neither of the bf16 kernel's
// two tile copies carries over: four 32-row hi + mid tiles and the W splits exceed the
// 160 KB of LDS, and two fp32 register copies are 256 VGPRs.  Chosen here, to keep four
// waves per CU (one per SIMD) and a whole tile of loads in flight per wave:
//   * the forward takes its X operand straight from the registers the row was loaded into
//     (row r, dims 8h..+8 is one lane's 32-B load) and leaves the packed hi and mid terms
//     in them -- the same 8 registers per 16 dims;
//   * only the backward operand goes through LDS, 16 rows (one MFMA k-step) at a time: the
//     half-wave that holds those rows writes hi and mid, all lanes read them transposed.
//     [2][16][XLD] is exactly the bf16 kernel's 32-row tile area, so SmLds serves both;
//   * the next tile is prefetched by plain vector loads into a second fp32 register copy
//     (no LDS-DMA).  With the 128 accumulator registers that is 384 of the 512 registers
//     a lone wave per SIMD has; the bias lives in LDS and the class of an accumulator
//     register is recomputed from the lane id so that the NB = 8 instantiation stays out
//     of scratch (doc/performance.md has the table).
// Chunks at or past ldx are zero-filled, rows past n are clamped and carry weight 0.
namespace {

typedef uint32_t sm_u32x4 __attribute__((ext_vector_type(4)));

// 8 fp32 -> bf16 terms hi + mid + lo (each the rounding of the exact remainder so far):
// x - (hi + mid + lo) is below 2^-25 |x|, x - (hi + mid) below 2^-17 |x|.
__device__ __forceinline__ void split8(const float4_ a, const float4_ b, sm_bf16x8& hi, sm_bf16x8& mid,
                                       sm_bf16x8& lo) {
  sm_u32x4 ph, pm, pl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float x0 = j < 2 ? a[2 * j] : b[2 * j - 4], x1 = j < 2 ? a[2 * j + 1] : b[2 * j - 3];
    ph[j] = pk_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(ph[j] << 16), r1 = x1 - __uint_as_float(ph[j] & 0xffff0000u);
    pm[j] = pk_bf16(r0, r1);
    pl[j] = pk_bf16(r0 - __uint_as_float(pm[j] << 16), r1 - __uint_as_float(pm[j] & 0xffff0000u));
  }
  hi = __builtin_bit_cast(sm_bf16x8, ph);
  mid = __builtin_bit_cast(sm_bf16x8, pm);
  lo = __builtin_bit_cast(sm_bf16x8, pl);
}

template <int NB>
__global__ __launch_bounds__(kSmThreads, 1) void glm_softmax_f32_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const int32_t* __restrict__ y,
    const float* __restrict__ sw, const uint16_t* __restrict__ Wsp, const float* __restrict__ bias, int K,
    float* __restrict__ partial, int pstride) {
  using L = SmLds<NB>;
  constexpr int D = L::D, KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS];
  __shared__ __attribute__((aligned(16))) float bs[32];   // bias, -inf for the classes past K
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* Xs = smem + L::W_ELEMS + wid * L::WAVE_ELEMS;   // [hi, mid][16 rows][XLD]
  uint16_t* Rs = Xs + 32 * XLD;

  for (int p = threadIdx.x; p < 3 * 32 * (D / 8); p += kSmThreads) {
    const int row = p / (D / 8), k8 = p % (D / 8);
    *reinterpret_cast<sm_bf16x8*>(Ws + row * WLD + k8 * 8) =
        *reinterpret_cast<const sm_bf16x8*>(Wsp + (int64_t)row * D + k8 * 8);
  }
  // register v of a lane's accumulator tile is class 4 h + cv(v)
  auto cv = [](int v) { return 8 * (v >> 2) + (v & 3); };
  if (threadIdx.x < 32) bs[threadIdx.x] = (int)threadIdx.x < K ? bias[threadIdx.x] : -INFINITY;
  uint16_t* Rw = Rs + 4 * h * RLD + r;
  __syncthreads();

  sm_f32x16 G[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) G[b][v] = 0.f;
  float gb[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) gb[v] = 0.f;
  float lossacc = 0.f;

  const int64_t ntiles = (n + 31) / 32;
  const int64_t step = (int64_t)gridDim.x * kSmWaves;
  int64_t tile = (int64_t)blockIdx.x * kSmWaves + wid;
  float4_ xf[KS][2], xn[KS][2];
  auto load = [&](int64_t t, float4_ (*dst)[2]) {
    int64_t row = t * 32 + r;
    row = row < n ? row : n - 1;
    const float* src = X + row * ldx;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int col = ks * 16 + 8 * h;
      if (col < ldx) {
        dst[ks][0] = *reinterpret_cast<const float4_*>(src + col);
        dst[ks][1] = *reinterpret_cast<const float4_*>(src + col + 4);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[ks][0][j] = dst[ks][1][j] = 0.f;
      }
    }
  };
  if (tile < ntiles) load(tile, xf);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) load(tile + step, xn);
    const int64_t row = tile * 32 + r;
    const bool valid = row < n;
    const int ylh = (valid ? y[row] : -1) - 4 * h;   // label relative to this half-wave's classes
    const float wr = valid ? (sw ? sw[row] : 1.f) : 0.f;
    // ---- forward: margins of row r, 16 classes per lane; the hi and mid terms of the row
    // stay in the registers the fp32 values came in, for the backward staging below
    sm_f32x16 acc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float4_ b4 = *reinterpret_cast<const float4_*>(bs + 8 * j + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[4 * j + u] = b4[u];
    }
    sm_bf16x8 xh[KS], xm[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      sm_bf16x8 xl;
      split8(xf[ks][0], xf[ks][1], xh[ks], xm[ks], xl);
      const uint16_t* wp = Ws + r * WLD + ks * 16 + 8 * h;
      const sm_bf16x8 a0 = *reinterpret_cast<const sm_bf16x8*>(wp);
      const sm_bf16x8 a1 = *reinterpret_cast<const sm_bf16x8*>(wp + 32 * WLD);
      const sm_bf16x8 a2 = *reinterpret_cast<const sm_bf16x8*>(wp + 64 * WLD);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, xh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xm[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xm[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, xh[ks], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, xh[ks], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- row softmax (the two half-waves hold disjoint class subsets of row r)
    float mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < 16; ++v) mx = fmaxf(mx, acc[v]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float se = 0.f;
#pragma unroll
    for (int v = 0; v < 16; ++v) se += __expf(acc[v] - mx);
    se += __shfl_xor(se, 32, 64);
    const float lse = mx + __logf(se);
#pragma unroll
    for (int v = 0; v < 16; v += 2) {
      float rv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bool hit = cv(v + u) == ylh;
        rv[u] = wr * (__expf(acc[v + u] - lse) - (hit ? 1.f : 0.f));
        gb[v + u] += rv[u];
        if (hit) lossacc += wr * (lse - acc[v + u]);
      }
      const uint32_t ph = pk_bf16(rv[0], rv[1]);
      const uint32_t pl = pk_bf16(rv[0] - __uint_as_float(ph << 16), rv[1] - __uint_as_float(ph & 0xffff0000u));
      Rw[cv(v) * RLD] = (uint16_t)ph;
      Rw[cv(v + 1) * RLD] = (uint16_t)(ph >> 16);
      Rw[(32 + cv(v)) * RLD] = (uint16_t)pl;
      Rw[(32 + cv(v + 1)) * RLD] = (uint16_t)(pl >> 16);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    // ---- backward: G[class][dim] += sum over the tile's rows of R[row][class] X[row][dim],
    // 16 rows (one MFMA k-step) at a time through this wave's staging area
    sm_bf16x8 ar[2][2];
#pragma unroll
    for (int rs = 0; rs < 2; ++rs)
#pragma unroll
      for (int s = 0; s < 2; ++s)
        ar[rs][s] = *reinterpret_cast<const sm_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
#pragma unroll
    for (int rs = 0; rs < 2; ++rs) {
      if ((r >> 4) == rs) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          *reinterpret_cast<sm_bf16x8*>(Xs + (r & 15) * XLD + ks * 16 + 8 * h) = xh[ks];
          *reinterpret_cast<sm_bf16x8*>(Xs + (16 + (r & 15)) * XLD + ks * 16 + 8 * h) = xm[ks];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        sm_bf16x8 bh, bm;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          bh[q] = (short)Xs[(8 * h + q) * XLD + b * 32 + r];
          bm[q] = (short)Xs[(16 + 8 * h + q) * XLD + b * 32 + r];
        }
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][1], bm, G[b], 0, 0, 0);
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][0], bm, G[b], 0, 0, 0);
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][1], bh, G[b], 0, 0, 0);
        G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[rs][0], bh, G[b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // staged reads done before the area is overwritten
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      xf[ks][0] = xn[ks][0];
      xf[ks][1] = xn[ks][1];
    }
  }
  // ---- this wave's slab row: [G class-major 32 x D | sum R (32) | loss]
  float* out = partial + ((int64_t)blockIdx.x * kSmWaves + wid) * pstride;
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) out[(4 * h + cv(v)) * D + b * 32 + r] = G[b][v];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    float s = gb[v];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (r == 0) out[32 * D + 4 * h + cv(v)] = s;
  }
  const float lt = wave_sum(lossacc);
  if (lane == 0) out[32 * D + 32] = lt;
}

}  // namespace

// One multinomial pass over fp32 rows: the arguments, the out / partial layout and the
// return codes of o3s_glm_softmax with X = float [n, ldx] (ldx % 8 == 0).
O3S_API int o3s_glm_softmax_f32(const void* X, int64_t n, int64_t ldx, int d, const int32_t* y, const float* sw,
                                const void* Wsp, const float* bias, int K, float* partial, int grid, double* out,
                                hipStream_t st) {
  const int nb = (d + 31) / 32;
  if (ldx % 8 != 0 || nb < 1 || nb > 8 || K < 1 || K > 32 || grid <= 0) return -1;
  const int D = 32 * nb, pstride = 32 * D + 33;
  const float* Xf = (const float*)X;
  const uint16_t* Wh = (const uint16_t*)Wsp;
  if (n > 0) {
    switch (nb) {
#define O3S_SM(NBV) \
  case NBV: hipLaunchKernelGGL((glm_softmax_f32_kernel<NBV>), dim3(grid), dim3(kSmThreads), 0, st, Xf, n, ldx, y, \
                               sw, Wh, bias, K, partial, pstride); break;
      O3S_SM(1) O3S_SM(2) O3S_SM(3) O3S_SM(4) O3S_SM(5) O3S_SM(6) O3S_SM(7) O3S_SM(8)
#undef O3S_SM
      default: return -1;
    }
  } else {
    hipMemsetAsync(partial, 0, sizeof(float) * pstride * (size_t)grid * kSmWaves, st);
  }
  O3S_CHECK_LAUNCH();
  hipLaunchKernelGGL(glm_finish_kernel, dim3((pstride + 31) / 32), dim3(1024), 0, st, partial, grid * kSmWaves,
                     pstride, pstride, out, 0);
  O3S_CHECK_LAUNCH();
  return 0;
}

O3S_PRELOAD(glm)

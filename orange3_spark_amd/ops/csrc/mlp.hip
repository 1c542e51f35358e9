// One-hidden-layer perceptron (gfx950): one fused loss / gradient pass over bf16 rows
// (mlp_pass_kernel) or over fp32 rows (mlp_pass_f32_kernel), and the forward half alone
// (LOGITS = true) that writes the output layer's logits of every row.
//   Z = X W1 + b1,  A = sigmoid(Z),  L = A W2 + b2,  P = softmax(L)
//   loss = sum_rows (logsumexp(L) - L[y]),  R = P - onehot(y)
//   gW2 = A^T R,  gb2 = sum R,  dZ = (R W2^T) . A . (1 - A),  gW1 = X^T dZ,  gb1 = sum dZ
// Reference: Spark's MultilayerPerceptronClassifier with layers [d, H, K] (sigmoid hidden
// layer, softmax output with cross-entropy), reached from the classification widget.
//
// The pass is the multinomial pass of glm_softmax.hip with one more small MFMA layer in the
// middle, on the tile and the term rules of mfma_tile.h; the same bits for any grid.  A and R
// stay in registers between the layers and enter the next MFMA as three terms too (one more MFMA
// per k-step than two terms, and the two-term remainder of R would reach gW1 through dH).  The
// four products of the backward GEMMs are issued A term by A term here, not in mt_mfma4's order.
//
// Hidden blocks across the waves of a block.  H units are NH = ceil(H / 32) blocks of 32; the
// gradient of W1 is H x D accumulators, one block of which fills a wave's registers at D = 256.
// A thread block is NH waves (1..4) that share one 32-row tile; wave j owns units 32j..32j+31:
// its Z block, A_j, its partial logits W2[block j]^T A_j, dZ_j, its 32 x D slice of gW1 and its
// K x 32 slice of gW2.  The partial logits (32 classes x 32 rows, fp32) are exchanged through
// LDS; every wave sums the NH partials in the same order and computes the softmax and R
// redundantly.  gb2 and the loss are written by wave 0.  With NH = 1 there is nothing to
// exchange and no block barrier: a block is up to four independent waves (as many as LDS
// holds), each on a tile and a slab row of its own, that share the W1 / W2 terms.
//
// No LDS trip between the layers.  Register v of a lane's accumulator tile is unit
// 8(v>>2) + 4h + (v&3) of row r, so registers 8s..8s+7 of lane (r, h) are a legal B fragment
// (8 consecutive k of column r) of k-step s of the next MFMA once the k index of its A operand
// is permuted to match: unit 16s + 8(e>>2) + 4h + (e&3) sits at k = 8h + e.  The host packs W2
// that way for the logits, and W2^T likewise for dH = W2 R, whose B operand is R in the logits'
// accumulator layout; dH lands in the layout of A and dZ = dH A (1 - A) is in-lane.
//
// Backward.  gW2_j += R A_j (A operand R: class r, rows 8h..+8 of a 16-row step; B operand A_j:
// unit r, the same rows) and gW1_j += dZ_j^T X (A operand dZ_j, B operand X^T read transposed
// from the X tile in LDS that the block writes once per tile: bf16 rows as they are, fp32 rows
// as hi + mid).  R, A_j and then dZ_j go through this wave's own LDS buffers as hi + lo (the
// first two of the three terms for R and A_j).
//
// Barriers.  The tile loop's trip count depends on blockIdx, the slab count and n only, rows
// past n are loaded clamped and carry R = 0, so all NH waves reach both __syncthreads() of a
// tile: one after the partial logits are written, one after they are read.  The shared X tile
// is written between the two (every wave has arrived in this tile, nobody reads X before the
// second), and a wave's exchange slot aliases its own R buffer, which only that wave touches
// outside the two barriers.
//
// A slab row (one per group of NH waves): [gW1 32 NH x D | gW2 32 x 32 NH | gb1 32 NH | gb2 32 | loss].
#include "glm_launch.h"
#include "mfma_tile.h"

namespace {

constexpr int kMlpMaxNh = 4, kMlpMaxNb = 8;
// (NH, NB) the kernels are built for: up to NH NB = 16; on fp32 rows (twice the registers per row
// copy and twice the X tile) past one hidden block only up to NB = 6: (2, 7) and (2, 8) would
// spill.
constexpr bool mlp_taken(bool f32, int nh, int nb) {
  return nh >= 1 && nh <= kMlpMaxNh && nb >= 1 && nb <= kMlpMaxNb && nh * nb <= 16 && (!f32 || nh == 1 || nb <= 6);
}

template <int NH, int NB, bool F32, bool LOGITS>
struct MlpLds : MtPitch<NB> {
  using MtPitch<NB>::D;
  using MtPitch<NB>::WLD;
  using MtPitch<NB>::XLD;
  using MtPitch<NB>::RLD;
  static constexpr int FRAG = 64 * 8;   // one A fragment of a wave: 64 lanes x 16 B
  static constexpr int W1_ELEMS = 3 * 32 * NH * WLD;
  static constexpr int X_ELEMS = LOGITS ? 0 : (F32 ? 2 : 1) * 32 * XLD;
  // per wave: R (then dZ) hi + lo [2][32][RLD] and A hi + lo [2][32][RLD]; the first 4 KB are
  // the wave's exchange slot (16 x 64 floats), all the LOGITS kernels need
  static constexpr int WAVE_ELEMS = LOGITS ? (NH > 1 ? 2048 : 0) : 2 * 2 * 32 * RLD;
  static constexpr int BIAS = 2 * 32 * NH + 64;   // floats: b1 hi | b1 lo | b2 hi | b2 lo
  // the widest fp32 pass keeps its gb1 / gb2 sums in lane-private LDS slots, not in registers:
  // two fp32 row copies and the gW1 accumulators are 384 registers at NB = 8
  static constexpr bool GB_IN_LDS = !LOGITS && F32 && NB == 8;
  static constexpr int GB_WAVE = GB_IN_LDS ? 32 * 64 : 0;   // floats: [gb2 16 | gb1 16][lane]
  static constexpr int W2_FRAGS = (LOGITS ? 1 : 2) * NH * 6 * FRAG;
  // bytes with `groups` tiles in flight (an X tile each) on `waves` waves, W2 fragments in LDS or not
  static constexpr int bytes(int groups, int waves, bool w2) {
    return 2 * (W1_ELEMS + (w2 ? W2_FRAGS : 0) + groups * X_ELEMS + waves * WAVE_ELEMS) + 4 * (BIAS + waves * GB_WAVE);
  }
  static constexpr int groups1() {   // NH = 1: as many of four waves as fit
    int g = 4;
    while (g > 1 && bytes(g, g, true) > 160 * 1024) --g;
    return g;
  }
  // With one hidden block the waves of a block are independent, each on a tile and a slab row
  // of its own (GROUPS of them, sharing the W1 / W2 terms in LDS); with more, the block is one
  // group of NH waves on one tile.
  static constexpr int GROUPS = NH == 1 ? groups1() : 1;
  static constexpr int WAVES = NH == 1 ? GROUPS : NH;
  static constexpr int GB = WAVES * GB_WAVE;
  // the W2 / W2^T fragments sit in LDS up to NH = 2 where they fit (all but NB = 8 at NH = 2)
  // and in the wave's registers otherwise
  static constexpr bool W2_IN_LDS = NH <= 2 && bytes(GROUPS, WAVES, true) <= 160 * 1024;
  static constexpr int W2_ELEMS = W2_IN_LDS ? W2_FRAGS : 0;
  static constexpr int ELEMS = W1_ELEMS + W2_ELEMS + GROUPS * X_ELEMS + WAVES * WAVE_ELEMS;
  // the biases are read from LDS unless that is what does not fit (fp32 rows at NH = NB = 4)
  static constexpr bool BIAS_IN_LDS = 2 * ELEMS + 4 * (BIAS + GB) <= 160 * 1024;
  static constexpr int BYTES = 2 * ELEMS + 4 * ((BIAS_IN_LDS ? BIAS : 0) + GB);
  static_assert(BYTES <= 160 * 1024, "exceeds the LDS of a CU");
};

// 16 accumulator registers -> the B fragments of two k-steps (element e of k-step s is
// register 8 s + e) as bf16 terms hi + mid (+ lo), each the rounding of the remainder so far.
__device__ __forceinline__ void mlp_split16(const float (&x)[16], mt_bf16x8 (&hi)[2], mt_bf16x8 (&mid)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    mt_u32x4 ph, pm;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t h, m;
      split_bf16x2(x[8 * s + 2 * j], x[8 * s + 2 * j + 1], h, m);
      ph[j] = h;
      pm[j] = m;
    }
    hi[s] = __builtin_bit_cast(mt_bf16x8, ph);
    mid[s] = __builtin_bit_cast(mt_bf16x8, pm);
  }
}
__device__ __forceinline__ void mlp_split16(const float (&x)[16], mt_bf16x8 (&hi)[2], mt_bf16x8 (&mid)[2],
                                            mt_bf16x8 (&lo)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    mt_u32x4 ph, pm, pl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t h, m, l;
      split_bf16x3(x[8 * s + 2 * j], x[8 * s + 2 * j + 1], h, m, l);
      ph[j] = h;
      pm[j] = m;
      pl[j] = l;
    }
    hi[s] = __builtin_bit_cast(mt_bf16x8, ph);
    mid[s] = __builtin_bit_cast(mt_bf16x8, pm);
    lo[s] = __builtin_bit_cast(mt_bf16x8, pl);
  }
}

// The same two-term fragments -> LDS, class / unit major ([2][32][RLD], Bw = buffer + 4 h RLD + r),
// for the A-operand (16 B along the rows) and transposed B-operand reads of the backward.
__device__ __forceinline__ void mlp_store_t(const mt_bf16x8 (&hi)[2], const mt_bf16x8 (&lo)[2], uint16_t* Bw,
                                            int RLD) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      Bw[mt_cv(8 * s + e) * RLD] = (uint16_t)hi[s][e];
      Bw[(32 + mt_cv(8 * s + e)) * RLD] = (uint16_t)lo[s][e];
    }
}

template <int NH, int NB, bool F32, bool LOGITS>
__device__ __forceinline__ void mlp_body(const void* __restrict__ Xv, int64_t n, int64_t ldx,
                                         const int32_t* __restrict__ y, const uint16_t* __restrict__ W1sp,
                                         const uint16_t* __restrict__ W2p, const float* __restrict__ bias, int K,
                                         float* __restrict__ partial, int pstride, int nslab, int slab0,
                                         float* __restrict__ logits) {
  using L = MlpLds<NH, NB, F32, LOGITS>;
  using SRC = std::conditional_t<F32, MtF32, MtBf16>;
  using elem = typename SRC::elem;
  constexpr int D = L::D, KS = 2 * NB, WLD = L::WLD, XLD = L::XLD, RLD = L::RLD, T = 64 * L::WAVES;
  __shared__ __attribute__((aligned(16))) uint16_t smem[L::ELEMS > 0 ? L::ELEMS : 8];
  __shared__ __attribute__((aligned(16))) float bs[L::BIAS_IN_LDS ? L::BIAS : 4];
  __shared__ float gbs[L::GB > 0 ? L::GB : 1];
  const elem* __restrict__ X = static_cast<const elem*>(Xv);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wid = NH > 1 ? wv : 0;   // this wave's hidden block
  const int grp = NH > 1 ? 0 : wv;   // and its tile group
  const int r = lane & 31, h = lane >> 5;
  uint16_t* Ws = smem;
  uint16_t* W2s = Ws + L::W1_ELEMS;
  uint16_t* Xs = W2s + L::W2_ELEMS;
  uint16_t* Wv = Xs + L::GROUPS * L::X_ELEMS;      // the waves' buffers, wave q at q * WAVE_ELEMS
  uint16_t* Rs = Wv + wv * L::WAVE_ELEMS;
  Xs += grp * L::X_ELEMS;                          // this group's X tile
  uint16_t* As = Rs + 2 * 32 * RLD;

  // W1 splits [3][32 NH][D] -> LDS (padded rows), the W2 fragments, the biases
  mt_stage_w<3 * 32 * NH, NB, T>(Ws, W1sp);
  if constexpr (L::W2_IN_LDS) {
    for (int p = threadIdx.x; p < L::W2_ELEMS / 8; p += T)
      *reinterpret_cast<mt_bf16x8*>(W2s + p * 8) = *reinterpret_cast<const mt_bf16x8*>(W2p + p * 8);
  }
  if constexpr (L::BIAS_IN_LDS) {
    for (int p = threadIdx.x; p < L::BIAS; p += T) bs[p] = bias[p];
  }
  auto bias4 = [&](int off) -> float4_ {   // four consecutive bias floats, off % 4 == 0
    if constexpr (L::BIAS_IN_LDS) {
      return *reinterpret_cast<const float4_*>(bs + off);
    } else {
      return *reinterpret_cast<const float4_*>(bias + off);
    }
  };
  // fragment t (hi, mid, lo) of k-step s of W2 (which = 0) or W2^T (which = 1) for this wave's block
  mt_bf16x8 w2r[L::W2_IN_LDS ? 1 : (LOGITS ? 6 : 12)];
  if constexpr (!L::W2_IN_LDS) {
#pragma unroll
    for (int i = 0; i < (LOGITS ? 6 : 12); ++i)
      w2r[i] = *reinterpret_cast<const mt_bf16x8*>(W2p + ((((i / 6) * NH + wid) * 6 + i % 6) * 64 + lane) * 8);
  }
  auto w2frag = [&](int which, int s, int t) -> mt_bf16x8 {
    if constexpr (L::W2_IN_LDS) {
      return *reinterpret_cast<const mt_bf16x8*>(W2s + (((which * NH + wid) * 6 + s * 3 + t) * 64 + lane) * 8);
    } else {
      return w2r[which * 6 + s * 3 + t];
    }
  };
  __syncthreads();

  // A pass: group g of the block holds slab row slab0 + blockIdx.x GROUPS + g, which sums the tiles slab, slab + nslab,
  // ... (nslab <= the number of tiles).  Logits: a grid-stride walk.  Either way one trip count
  // for the whole block.
  const int64_t ntiles = (n + 31) / 32;
  const int slab = slab0 + blockIdx.x * L::GROUPS + grp;
  const int64_t step = LOGITS ? (int64_t)gridDim.x * L::GROUPS : (int64_t)nslab;
  int64_t tile = LOGITS ? (int64_t)blockIdx.x * L::GROUPS + grp : (int64_t)slab;
  if (!LOGITS && slab >= nslab) return;   // the whole group: with NH > 1 the block, else an independent wave

  mt_f32x16 G[NB], G2;
  float gb1[16], gb2[16], lossacc = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
#pragma unroll
    for (int b = 0; b < NB; ++b) G[b][v] = 0.f;
    G2[v] = 0.f;
    gb1[v] = gb2[v] = 0.f;
  }
  float* gbl = gbs + (L::GB_IN_LDS ? wv * 32 * 64 + lane : 0);   // this lane's slots, stride 64
  if constexpr (L::GB_IN_LDS) {
#pragma unroll
    for (int v = 0; v < 32; ++v) gbl[v * 64] = 0.f;
  }

  typename SRC::chunk xc[KS], xn[KS];
  if (tile < ntiles) mt_load_tile<SRC, KS>(X, n, ldx, tile, r, h, xc);
  for (; tile < ntiles; tile += step) {
    if (tile + step < ntiles) mt_load_tile<SRC, KS>(X, n, ldx, tile + step, r, h, xn);
    const int64_t row = tile * 32 + r;
    const bool valid = row < n;
    // ---- hidden layer: Z of row r, 16 units of this wave's block per lane.  On fp32 rows the
    // hi and mid terms stay in registers for the shared tile
    mt_f32x16 z;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4_ b4 = bias4(32 * wid + 8 * q + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u) z[4 * q + u] = b4[u];
    }
    mt_bf16x8 xh[KS], xm[F32 ? KS : 1];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint16_t* wp = Ws + (32 * wid + r) * WLD + ks * 16 + 8 * h;
      const mt_bf16x8 a0 = *reinterpret_cast<const mt_bf16x8*>(wp);
      const mt_bf16x8 a1 = *reinterpret_cast<const mt_bf16x8*>(wp + 32 * NH * WLD);
      const mt_bf16x8 a2 = *reinterpret_cast<const mt_bf16x8*>(wp + 64 * NH * WLD);
      if constexpr (F32) {
        mt_bf16x8 xl;
        mt_split8(xc[ks].a, xc[ks].b, xh[ks], xm[ks], xl);
        z = mt_mfma6(z, a0, a1, a2, xh[ks], xm[ks], xl);
        __builtin_amdgcn_sched_barrier(0);
      } else {
        xh[ks] = xc[ks];
        z = mt_mfma3(z, a2, a1, a0, xh[ks]);
      }
    }
    float a[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4_ b4 = bias4(32 * NH + 32 * wid + 8 * q + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u) a[4 * q + u] = 1.f / (1.f + __expf(-(z[4 * q + u] + b4[u])));
    }
    mt_bf16x8 ah[2], am[2], al[2];
    mlp_split16(a, ah, am, al);
    // ---- output layer: this block's share of the logits of row r, 16 classes per lane
    mt_f32x16 lg;
#pragma unroll
    for (int v = 0; v < 16; ++v) lg[v] = 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      lg = mt_mfma6(lg, w2frag(0, s, 0), w2frag(0, s, 1), w2frag(0, s, 2), ah[s], am[s], al[s]);
    }
    auto share_x = [&]() {   // this wave's k-steps of the tile -> the block's X tile
      if constexpr (!LOGITS) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          if (NH == 1 || ks % NH == wid) {
            *reinterpret_cast<mt_bf16x8*>(Xs + r * XLD + ks * 16 + 8 * h) = xh[ks];
            if constexpr (F32) *reinterpret_cast<mt_bf16x8*>(Xs + (32 + r) * XLD + ks * 16 + 8 * h) = xm[ks];
          }
        }
      }
    };
    if constexpr (NH > 1) {
      float* mine = reinterpret_cast<float*>(Rs);
#pragma unroll
      for (int v = 0; v < 16; ++v) mine[v * 64 + lane] = lg[v];
      __syncthreads();
      share_x();
#pragma unroll
      for (int v = 0; v < 16; ++v) lg[v] = 0.f;
#pragma unroll
      for (int q = 0; q < NH; ++q) {
        const float* slot = reinterpret_cast<const float*>(Wv + q * L::WAVE_ELEMS);
#pragma unroll
        for (int v = 0; v < 16; ++v) lg[v] += slot[v * 64 + lane];
      }
      __syncthreads();
    } else {
      share_x();
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4_ bh = bias4(64 * NH + 8 * q + 4 * h);
      const float4_ bl = bias4(64 * NH + 32 + 8 * q + 4 * h);
#pragma unroll
      for (int u = 0; u < 4; ++u) lg[4 * q + u] = (lg[4 * q + u] + bh[u]) + bl[u];   // -inf past K
    }
    if constexpr (LOGITS) {
      // registers 4q..4q+3 are the classes 8q + 4h .. +3 of row r: one 16-B store where K allows
      if (valid) {
        float* dst = logits + row * K;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c0 = 8 * q + 4 * h;
          if ((NH == 1 || q % NH == wid) && c0 < K) {
            if ((K & 3) == 0) {
              float4_ o;
#pragma unroll
              for (int u = 0; u < 4; ++u) o[u] = lg[4 * q + u];
              *reinterpret_cast<float4_*>(dst + c0) = o;
            } else {
#pragma unroll
              for (int u = 0; u < 4; ++u)
                if (c0 + u < K) dst[c0 + u] = lg[4 * q + u];
            }
          }
        }
      }
    } else {
      // ---- row softmax (the two half-waves hold disjoint class subsets of row r) and R
      const int ylh = (valid ? y[row] : -1) - 4 * h;   // label relative to this half-wave's classes
      float mx = -INFINITY;
#pragma unroll
      for (int v = 0; v < 16; ++v) mx = fmaxf(mx, lg[v]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float se = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) se += __expf(lg[v] - mx);
      se += __shfl_xor(se, 32, 64);
      const float lse = mx + __logf(se);
      float rv[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const bool hit = mt_cv(v) == ylh;
        rv[v] = valid ? __expf(lg[v] - lse) - (hit ? 1.f : 0.f) : 0.f;
        if constexpr (L::GB_IN_LDS) gbl[v * 64] += rv[v]; else gb2[v] += rv[v];
        if (hit) lossacc += lse - lg[v];
      }
      mt_bf16x8 rh[2], rm[2], rl[2];
      mlp_split16(rv, rh, rm, rl);
      mlp_store_t(rh, rm, Rs + 4 * h * RLD + r, RLD);
      mlp_store_t(ah, am, As + 4 * h * RLD + r, RLD);
      // ---- dH = W2 R in the layout of A, dZ in-lane.  Classes 16..31 are k-step 1
      mt_f32x16 dh;
#pragma unroll
      for (int v = 0; v < 16; ++v) dh[v] = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s == 0 || K > 16)
          dh = mt_mfma6(dh, w2frag(1, s, 0), w2frag(1, s, 1), w2frag(1, s, 2), rh[s], rm[s], rl[s]);
      }
      float dz[16];
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        dz[v] = dh[v] * (a[v] * (1.f - a[v]));
        if constexpr (L::GB_IN_LDS) gbl[(16 + v) * 64] += dz[v]; else gb1[v] += dz[v];
      }
      mt_wave_sync();
      // ---- gW2[class][unit] += sum over the tile's rows of R[row][class] A[row][unit]
#pragma unroll
      for (int rs = 0; rs < 2; ++rs) {
        const int o = r * RLD + rs * 16 + 8 * h;
        const mt_bf16x8 ar0 = *reinterpret_cast<const mt_bf16x8*>(Rs + o);
        const mt_bf16x8 ar1 = *reinterpret_cast<const mt_bf16x8*>(Rs + 32 * RLD + o);
        const mt_bf16x8 ba0 = *reinterpret_cast<const mt_bf16x8*>(As + o);
        const mt_bf16x8 ba1 = *reinterpret_cast<const mt_bf16x8*>(As + 32 * RLD + o);
        G2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar1, ba1, G2, 0, 0, 0);
        G2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar1, ba0, G2, 0, 0, 0);
        G2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar0, ba1, G2, 0, 0, 0);
        G2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar0, ba0, G2, 0, 0, 0);
      }
      mt_wave_sync();    // R has been read: dZ takes its buffer
      mt_bf16x8 dzh[2], dzl[2];
      mlp_split16(dz, dzh, dzl);
      mlp_store_t(dzh, dzl, Rs + 4 * h * RLD + r, RLD);
      mt_wave_sync();
      // ---- gW1[unit][dim] += sum over the tile's rows of dZ[row][unit] X[row][dim]
      mt_bf16x8 ad[2][2];
#pragma unroll
      for (int rs = 0; rs < 2; ++rs)
#pragma unroll
        for (int s = 0; s < 2; ++s)
          ad[rs][s] = *reinterpret_cast<const mt_bf16x8*>(Rs + (s * 32 + r) * RLD + rs * 16 + 8 * h);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int rs = 0; rs < 2; ++rs) {
          const mt_bf16x8 bx = mt_read_xt(Xs, rs * 16 + 8 * h, b * 32 + r, XLD);
          if constexpr (F32) {
            const mt_bf16x8 bm = mt_read_xt(Xs, 32 + rs * 16 + 8 * h, b * 32 + r, XLD);
            G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad[rs][1], bm, G[b], 0, 0, 0);
            G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad[rs][1], bx, G[b], 0, 0, 0);
            G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad[rs][0], bm, G[b], 0, 0, 0);
            G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad[rs][0], bx, G[b], 0, 0, 0);
          } else {
            G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad[rs][1], bx, G[b], 0, 0, 0);
            G[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ad[rs][0], bx, G[b], 0, 0, 0);
          }
        }
      }
      mt_wave_sync();    // this tile's LDS reads are done before the wave writes the next one's
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xc[ks] = xn[ks];
  }
  if constexpr (!LOGITS) {
    // ---- the block's slab row: [gW1 32 NH x D | gW2 32 x 32 NH | gb1 32 NH | gb2 32 | loss]
    float* out = partial + (int64_t)slab * pstride;
    float* o2 = out + 32 * NH * D;
    float* o3 = o2 + 32 * 32 * NH;
    float* o4 = o3 + 32 * NH;
    mt_write_slab_g<NB>(G, out + 32 * wid * D, r, h);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int c = 4 * h + mt_cv(v);
      o2[c * 32 * NH + 32 * wid + r] = G2[v];
      float s1 = gb1[v], s2 = gb2[v];
      if constexpr (L::GB_IN_LDS) {
        s1 = gbl[(16 + v) * 64];
        s2 = gbl[v * 64];
      }
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {   // over the 32 rows (same h)
        s1 += __shfl_xor(s1, off, 64);
        s2 += __shfl_xor(s2, off, 64);
      }
      if (r == 0) {
        o3[32 * wid + c] = s1;
        if (wid == 0) o4[c] = s2;
      }
    }
    const float lt = wave_sum(lossacc);
    if (wid == 0 && lane == 0) o4[32] = lt;
  }
}

template <int NH, int NB, bool LOGITS>
__global__ __launch_bounds__((64 * MlpLds<NH, NB, false, LOGITS>::WAVES), 1) void mlp_pass_kernel(
    const uint16_t* __restrict__ X, int64_t n, int64_t ldx, const int32_t* __restrict__ y,
    const uint16_t* __restrict__ W1sp, const uint16_t* __restrict__ W2p, const float* __restrict__ bias, int K,
    float* __restrict__ partial, int pstride, int nslab, int slab0, float* __restrict__ logits) {
  mlp_body<NH, NB, false, LOGITS>(X, n, ldx, y, W1sp, W2p, bias, K, partial, pstride, nslab, slab0, logits);
}

// The pass over fp32 rows: a row is split into bf16 terms as it is consumed (hi + mid + lo with
// the six products of order <= 2 forward, hi + mid in the shared tile for gW1).
template <int NH, int NB, bool LOGITS>
__global__ __launch_bounds__((64 * MlpLds<NH, NB, true, LOGITS>::WAVES), 1) void mlp_pass_f32_kernel(
    const float* __restrict__ X, int64_t n, int64_t ldx, const int32_t* __restrict__ y,
    const uint16_t* __restrict__ W1sp, const uint16_t* __restrict__ W2p, const float* __restrict__ bias, int K,
    float* __restrict__ partial, int pstride, int nslab, int slab0, float* __restrict__ logits) {
  mlp_body<NH, NB, true, LOGITS>(X, n, ldx, y, W1sp, W2p, bias, K, partial, pstride, nslab, slab0, logits);
}

template <bool F32> struct MlpFam {
  using elem = uint16_t;
  template <int NH, int NB, bool LOGITS> static auto kernel() { return mlp_pass_kernel<NH, NB, LOGITS>; }
};
template <> struct MlpFam<true> {
  using elem = float;
  template <int NH, int NB, bool LOGITS> static auto kernel() { return mlp_pass_f32_kernel<NH, NB, LOGITS>; }
};

bool mlp_args_ok(bool f32, int64_t n, int64_t ldx, int d, int H, int K, int grid) {
  return n >= 0 && ldx > 0 && ldx % 8 == 0 && d >= 1 && H >= 1 && K >= 2 && K <= 32 && grid > 0 &&
         mlp_taken(f32, (H + 31) / 32, (d + 31) / 32);
}

// The launches of one instantiation: `grid` blocks at a time, each block GROUPS slab rows (a
// pass: until every one of the nslab slab rows has had its group) or GROUPS tile walks (logits:
// one launch).
template <int NH, int NB, bool F32, bool LOGITS>
int mlp_launch_inst(int grid, hipStream_t st, const typename MlpFam<F32>::elem* X, int64_t n, int64_t ldx,
                    const int32_t* y, const uint16_t* W1sp, const uint16_t* W2p, const float* bias, int K,
                    float* partial, int pstride, int nslab, float* logits) {
  using L = MlpLds<NH, NB, F32, LOGITS>;
  const auto kernel = MlpFam<F32>::template kernel<NH, NB, LOGITS>();
  // logits: a grid-stride walk covers every tile in one launch of at most `grid` blocks
  const int64_t ntiles = (n + 31) / 32, reach = (int64_t)grid * L::GROUPS;
  const int64_t walks = LOGITS ? (ntiles < reach ? ntiles : reach) : (int64_t)nslab;
  return mt_walk_slabs(walks, grid, L::GROUPS, [&](int g, int w0) {
    hipLaunchKernelGGL(kernel, dim3(g), dim3(64 * L::WAVES), 0, st, X, n, ldx, y, W1sp, W2p, bias, K, partial,
                       pstride, nslab, w0, logits);
  });
}

template <bool F32, bool LOGITS>
int mlp_launch(int nh, int nb, int grid, hipStream_t st, const typename MlpFam<F32>::elem* X, int64_t n, int64_t ldx,
               const int32_t* y, const uint16_t* W1sp, const uint16_t* W2p, const float* bias, int K, float* partial,
               int pstride, int nslab, float* logits) {
  const auto leg = [&](auto NH) {
    return mt_dispatch_nb(nb, [&](auto NB) {
      if constexpr (mlp_taken(F32, NH, NB))
        return mlp_launch_inst<NH, NB, F32, LOGITS>(grid, st, X, n, ldx, y, W1sp, W2p, bias, K, partial, pstride,
                                                    nslab, logits);
      return -1;
    });
  };
  switch (nh) {
    case 1: return leg(IC<1>{});
    case 2: return leg(IC<2>{});
    case 3: return leg(IC<3>{});
    case 4: return leg(IC<4>{});
    default: return -1;
  }
}

// What the two pass entry points share: the argument check, the launches (an empty pass zeroes
// one slab row instead) and the fp64 finish over the slab rows.
template <bool F32>
int mlp_pass(const void* X, int64_t n, int64_t ldx, int d, int H, int K, const int32_t* y, const void* W1sp,
             const void* W2p, const float* bias, float* partial, int slabs, int grid, double* out, hipStream_t st) {
  if (!mlp_args_ok(F32, n, ldx, d, H, K, grid) || slabs <= 0) return -1;
  const int nh = (H + 31) / 32, nb = (d + 31) / 32, D = 32 * nb;
  const int pstride = 32 * nh * D + 32 * 32 * nh + 32 * nh + 33;
  const int64_t ntiles = (n + 31) / 32;
  const int used = n > 0 ? (int)(ntiles < slabs ? ntiles : slabs) : 1;
  if (n > 0) {
    const int rc = mlp_launch<F32, false>(nh, nb, grid, st, (const typename MlpFam<F32>::elem*)X, n, ldx, y,
                                          (const uint16_t*)W1sp, (const uint16_t*)W2p, bias, K, partial, pstride,
                                          used, nullptr);
    if (rc != 0) return rc;
  } else {
    (void)hipMemsetAsync(partial, 0, sizeof(float) * pstride, st);
  }
  return launch_finish(partial, used, pstride, pstride, out, 0, st);
}

template <bool F32>
int mlp_logits(const void* X, int64_t n, int64_t ldx, int d, int H, int K, const void* W1sp, const void* W2p,
               const float* bias, float* logits, int grid, hipStream_t st) {
  if (!mlp_args_ok(F32, n, ldx, d, H, K, grid)) return -1;
  if (n == 0) return 0;
  return mlp_launch<F32, true>((H + 31) / 32, (d + 31) / 32, grid, st, (const typename MlpFam<F32>::elem*)X, n, ldx,
                               nullptr, (const uint16_t*)W1sp, (const uint16_t*)W2p, bias, K, nullptr, 0, 0, logits);
}

}  // namespace

// One MLP pass over the n rows of X (bf16, row stride ldx, ldx % 8 == 0) for layers [d, H, K]
// with NH = ceil(H / 32), D = 32 ceil(d / 32), NH D / 32 <= 16: out (fp64) =
// [gW1 unit-major 32 NH x D | gW2 class-major 32 x 32 NH | gb1 32 NH | gb2 32 | loss sum].
// y: int32 labels in [0, K).  W1sp: bf16 [3][32 NH][D], the hi, mid, lo splits of the unit-major
// W1^T, zero-padded.  W2p: bf16 [2][NH][2][3][64][8]: for W2 (0) and W2^T (1), hidden block j,
// k-step s and term t the A fragment of lane 32 h + r, whose element e is
// W2[32 j + 16 s + 8 (e >> 2) + 4 h + (e & 3)][r] resp. W2[32 j + r][16 s + 8 (e >> 2) + 4 h + (e & 3)],
// zero past H and K.  bias: fp32 [b1 hi 32 NH | b1 lo 32 NH | b2 hi 32 | b2 lo 32], b2 hi = -inf
// past K.  partial: fp32 [slabs][pstride]: with S = min(slabs, tiles), slab row v < S sums the
// tiles v, v + S, ..., so the result depends on slabs and not on the grid: a group of NH waves sums
// one slab row, and fewer blocks than it takes mean several launches.
O3S_API int o3s_mlp_pass(const void* X, int64_t n, int64_t ldx, int d, int H, int K, const int32_t* y,
                         const void* W1sp, const void* W2p, const float* bias, float* partial, int slabs, int grid,
                         double* out, hipStream_t st) {
  return mlp_pass<false>(X, n, ldx, d, H, K, y, W1sp, W2p, bias, partial, slabs, grid, out, st);
}

// o3s_mlp_pass over fp32 rows: X = float [n, ldx] (ldx % 8 == 0); NH = 1 or D <= 192.
O3S_API int o3s_mlp_pass_f32(const void* X, int64_t n, int64_t ldx, int d, int H, int K, const int32_t* y,
                             const void* W1sp, const void* W2p, const float* bias, float* partial, int slabs,
                             int grid, double* out, hipStream_t st) {
  return mlp_pass<true>(X, n, ldx, d, H, K, y, W1sp, W2p, bias, partial, slabs, grid, out, st);
}

// The forward half alone: logits (fp32 [n, K], row-major) of every row of X (bf16); operands as
// above (the W2^T half of W2p is not read).
O3S_API int o3s_mlp_logits(const void* X, int64_t n, int64_t ldx, int d, int H, int K, const void* W1sp,
                           const void* W2p, const float* bias, float* logits, int grid, hipStream_t st) {
  return mlp_logits<false>(X, n, ldx, d, H, K, W1sp, W2p, bias, logits, grid, st);
}

// o3s_mlp_logits over fp32 rows.
O3S_API int o3s_mlp_logits_f32(const void* X, int64_t n, int64_t ldx, int d, int H, int K, const void* W1sp,
                               const void* W2p, const float* bias, float* logits, int grid, hipStream_t st) {
  return mlp_logits<true>(X, n, ldx, d, H, K, W1sp, W2p, bias, logits, grid, st);
}

O3S_PRELOAD(mlp)

// The mixed gradient pass of the GLM solvers (gfx950): resident and lineage rows in one launch,
// as the masked / mask-free kernel (glm_grad_mixed_kernel), with the resident tiles staged
// through LDS (glm_grad_staged_kernel), and as one launch of persistent waves
// (glm_grad_persist_kernel); at the end, the gradient pass over fp32 rows
// (glm_grad_f32_kernel), which has to be compiled with them.  The row layout, the row sources and the block epilogue are in
// glm_rows.h, the layout dispatch and the finish kernels in glm_launch.h.
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
// That launch reads the 0/1 labels of a logistic or hinge pass from two bit planes packed once
// per fit (o3s_glm_pack_labels, glm_grad_persist_kernel<.., YB = true>): 125 MB instead of the
// 4 GB float column per pass at 1B rows, fetched with scalar loads instead of label DMAs.
//
// Every kernel of this file is register-tuned to the instruction: the notes in them record
// what moving a statement into a helper cost in scratch or occupancy.  Device code here
// changes only with tools/isa_diff.py at hand; the host dispatch (the persist plan and
// o3s_glm_grad_mixed, at the end) is plain code.
#include "glm_launch.h"
#include "glm_items.h"

namespace {

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
  // glm_grad_persist_kernel<.., YB = true> only (zero and unused elsewhere): the labels as bits.
  // br0 / bl0: the two bit planes read as dwords (tile t of a role: bits 16 (t & 1) .. + 15 of
  // dword t >> 1); rt / lt: the next tile of each role whose word is to be loaded; rw / lw: the
  // dword that holds the labels of the role's next tile to be TAKEN, and rsh / lsh = 16 (t & 1)
  // of that tile (the shift is applied where the word is used, never where it is loaded: a use
  // makes the compiler wait for the load).  All wave-uniform: the loads are scalar loads.
  const uint32_t* br0;
  const uint32_t* bl0;
  uint32_t rt, lt, rw, lw, rsh, lsh;

  // (an empty asm per use: otherwise the offsets are hoisted out of the loop as invariants)
  __device__ static __forceinline__ uint32_t fresh(int v) {
    asm volatile("" : "+v"(v));
    return (uint32_t)v;
  }
  // the tile row whose label lane (g, c) takes: RowReduce<8, 2>::base(c) * G + g
  __device__ static __forceinline__ uint32_t label_off(uint32_t g, uint32_t c) { return ((c >> 2) * G + g) * 4; }

  // YB: no label DMA (a batch is 8 operations); the tile's label word is a scalar load.
  template <bool YB = false>
  __device__ __forceinline__ void issue_tile(int lane) {
    const uint32_t ln = fresh(lane);
    // (a resident tile's rows are finished in the lanes 0 .. 15, row = lane: TileStage::dot)
    if constexpr (!YB)
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
    if constexpr (YB) {
      rw = br0[rt >> 1];
      rsh = (rt & 1u) << 4;
      ++rt;
    } else {
      yrs += tstep;
    }
    --r_ahead;
    lab_younger = false;
  }
  // YB: the label word of the next lineage tile (lt) of the item; l_ahead counts the item's
  // lineage tiles whose word is not loaded yet.
  __device__ __forceinline__ void issue_bits() {
    lw = bl0[lt >> 1];
    lsh = (lt & 1u) << 4;
    ++lt;
    --l_ahead;
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
  // YB: the batch is the only thing in flight (vmcnt(0)); the slot holds no label, yv comes
  // from the tile's label word (rw), which was loaded with the batch and is valid behind the
  // closing lgkmcnt(0) of the reads (the compiler, which knows of the scalar load, puts its own
  // wait in front of the use as well); only then is the next tile's word loaded over it.
  template <bool PERSIST = false, bool YB = false>
  __device__ __forceinline__ void take_tile(int lane, short8 (&xb)[8], short8 (&xv)[UNROLL][CPL], float& yv,
                                            short8 (&fa)[3]) {
    if constexpr (YB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (lab_younger) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t ln = fresh(lane);
    // operand read: image (R >> 3) * 4 + q, row R & 7, position s ^ t(R), t(R) = (R >> 1) & 3;
    // sbase is a multiple of 128, so the xor acts on the position bits alone
    const uint32_t b0 = sbase + ((ln & 8) << 9) + ((ln >> 4) << 10) + ((ln & 7) << 7) + (((ln >> 1) & 3) << 4);
    if constexpr (YB) {
      asm volatile(
          "ds_read_b128 %16, %24\n\t"
          "ds_read_b128 %17, %24 offset:1024\n\t"
          "ds_read_b128 %18, %24 offset:2048\n\t"
          "ds_read_b128 %0, %19\n\t"
          "ds_read_b128 %1, %20\n\t"
          "ds_read_b128 %2, %21\n\t"
          "ds_read_b128 %3, %22\n\t"
          "ds_read_b128 %4, %19 offset:64\n\t"
          "ds_read_b128 %5, %20 offset:64\n\t"
          "ds_read_b128 %6, %21 offset:64\n\t"
          "ds_read_b128 %7, %22 offset:64\n\t"
          "ds_read_b128 %8, %23\n\t"
          "ds_read_b128 %9, %23 offset:1024\n\t"
          "ds_read_b128 %10, %23 offset:2048\n\t"
          "ds_read_b128 %11, %23 offset:3072\n\t"
          "ds_read_b128 %12, %23 offset:4096\n\t"
          "ds_read_b128 %13, %23 offset:5120\n\t"
          "ds_read_b128 %14, %23 offset:6144\n\t"
          "ds_read_b128 %15, %23 offset:7168\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(xb[0]), "=&v"(xb[1]), "=&v"(xb[2]), "=&v"(xb[3]), "=&v"(xb[4]), "=&v"(xb[5]), "=&v"(xb[6]),
            "=&v"(xb[7]), "=&v"(xv[0][0]), "=&v"(xv[0][1]), "=&v"(xv[0][2]), "=&v"(xv[0][3]), "=&v"(xv[1][0]),
            "=&v"(xv[1][1]), "=&v"(xv[1][2]), "=&v"(xv[1][3]), "=&v"(fa[0]), "=&v"(fa[1]), "=&v"(fa[2])
          : "v"(b0), "v"(b0 ^ 16u), "v"(b0 ^ 32u), "v"(b0 ^ 48u), "v"(sbase + ((ln ^ (ln >> 4)) << 4)),
            "v"(fbase + ln * 16)
          : "memory");
      yv = (float)(((rw >> rsh) >> (ln & 15u)) & 1u);
    } else
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
        if constexpr (YB) rt = nx_r0;
        else yrs = yr0 + (uint64_t)nx_r0 * (UNROLL * G);
        r_ahead = nx_nr;
        nx_nr = 0;
        r_pre = true;
      }
    }
    if (r_ahead > 0) issue_tile<YB>(lane);
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
  // YB: the lineage tile's label out of its word (lw, loaded a lineage tile earlier or, for an
  // item's first, at the end of the item before: glm_grad_persist_kernel): no vector-memory
  // wait and no LDS read.  Then the word of the item's next lineage tile, if it has one.
  __device__ __forceinline__ void take_bits(int g, int c, float& yv) {
    yv = (float)(((lw >> lsh) >> (label_off(fresh(g), fresh(c)) >> 2)) & 1u);
    if (l_ahead > 0) issue_bits();
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
          bool PERSIST = false, bool YB = false>
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
  if constexpr (STAGED && SRC::kLineage && YB) stg->take_bits(g, c, yy[0]);
  else if constexpr (STAGED && SRC::kLineage) stg->template take_label<PERSIST>(g, c, yy[0]);   // as late as the label is needed
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
template <int LOSS, bool SMP, bool PERSIST = false, bool YB = false>
__device__ __forceinline__ void staged_resident_tile(int64_t base, float intercept, int lane, const RowSampler smp,
                                                     float (&acc)[TileStage::CPL][8], float& acc_r, float& acc_loss,
                                                     float& acc_w, TileStage* stg) {
  constexpr int CPL = TileStage::CPL, UNROLL = TileStage::UNROLL;
  short8 xb[8], xv[UNROLL][CPL];
  float yv;
  short8 fa[3];
  stg->template take_tile<PERSIST, YB>(lane, xb, xv, yv, fa);
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
// (0 hi, 1 mid, 2 lo, as split_bf16x3 forms them; zero from 3 on) of the coefficients of chunk
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
        uint32_t ph, pm, pl;
        split_bf16x3(cw[2 * j], cw[2 * j + 1], ph, pm, pl);
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

// The float label column of a persistent pass, or none when its labels are bit planes (YB).
template <bool YB, class T>
__device__ __forceinline__ const float* label_col(const T* p) {
  if constexpr (YB) return nullptr;
  else return p;
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
// YB (labels from bit planes; YB = false is the kernel as it was, instruction for instruction):
// y / y_lin are the two planes of o3s_glm_pack_labels read as dwords, and a tile's 16 labels are
// one wave-uniform word, fetched by a scalar load (TileStage::issue_tile<true>, issue_bits): no
// label DMA, no label ds_read_b32, no lab_younger.  A batch is 8 operations, at most one batch
// is in flight, take_tile waits vmcnt(0) and the lineage tile has no vmcnt wait at all; the
// claim's atomic and the flush's stores remain the only other vector-memory operations, and the
// argument above carries over.  A resident tile's word is loaded with its batch (so across an
// item boundary too), a lineage tile's one lineage tile ahead, and the first lineage word of
// the next item at the end of the item, once that item is known, ahead of the flush.  Only
// loads are scalar: nothing scalar is ever written to memory.
// lgkmcnt with a scalar load outstanding: scalar loads count in lgkmcnt and may return out of
// order relative to LDS operations, so (1) a scalar result is valid only behind lgkmcnt(0), and
// (2) a counted wait sees one more operation.  (1): the words are plain C++ loads, so the
// compiler, which knows of them, puts its own lgkmcnt(0) in front of each first use, and the
// resident tile's use also stands behind take_tile's closing lgkmcnt(0); no use is moved in
// front of either.  (2): the counted waits of TileStage::dot (lgkmcnt(2), (1)) stay sufficient
// for the LDS reads: LDS operations retire in order among themselves, and an outstanding scalar
// load only takes a place in the count, so fewer LDS reads may remain than the count allows.
// The slot keeps its two 256-B label areas (43 008 B per block): TileStage's offsets are shared
// with glm_grad_staged_kernel.  loss_terms gets the same expression on the same values, so the
// outputs are bit-equal to YB = false (tests/test_glm_label_bits.py).
template <int LOSS, bool SMP, bool YB = false>
__global__ __launch_bounds__(kBlock, 3) void glm_grad_persist_kernel(
    const uint16_t* __restrict__ X, int64_t n_res, const std::conditional_t<YB, uint32_t, float>* __restrict__ y,
    const std::conditional_t<YB, uint32_t, float>* __restrict__ y_lin,
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
               label_col<YB>(y),
               label_col<YB>(y_lin),
               0u,
               0u,
               0u,
               0u,
               false,
               false};
  if constexpr (YB) {
    st.br0 = y;
    st.bl0 = y_lin;
  }
  uint32_t cur = claim_item(ticket, lane);
  if (cur >= items) return;
  GlmItem it = uniform_item(cur, Tr, Tl, items, inv_items);
  if constexpr (YB) {
    // the label word of the wave's very first lineage tile; every later item's comes at the end
    // of the item before it
    if (it.nl > 0) {
      st.lt = it.l0;
      st.l_ahead = it.nl;
      st.issue_bits();
    }
  }
  for (;;) {
    const uint32_t nr = it.nr, nl = it.nl, S = nr + nl;
    int64_t br = (int64_t)it.r0 * RT, bl = (int64_t)it.l0 * RT;   // first row of the current tile of each role
    // the item's first label and batch, unless the item before has sent them ahead
    if constexpr (!YB) {
      if (nl > 0 && !st.l_pre) {
        st.yls = y_lin + bl;
        st.l_ahead = nl;
        st.issue_label(g, c);
      }
    }
    if (nr > 0 && !st.r_pre) {
      st.xs = st.x0 + br * (ld * 2);
      if constexpr (YB) st.rt = it.r0;
      else st.yrs = y + br;
      st.r_ahead = nr;
      st.template issue_tile<YB>(lane);
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
        grad_tile<RowsLineage, LPR, CPL, UNROLL, LOSS, SMP, true, true, true, YB>(bl, n_lin, X, ld, CPL * LPR, label_col<YB>(y_lin),
                                                                                  nullptr, seed, row0, w, wshift, intercept, g, c,
                                                                                  smp_lin, acc, rs, acc_r, acc_loss, acc_w, &st);
        bl += RT;
      } else {
        if (r_left == 1) claim_next();
        --r_left;
        staged_resident_tile<LOSS, SMP, true, YB>(br, intercept, lane, smp_res, acc, acc_r, acc_loss, acc_w, &st);
        br += RT;
      }
    }
    if (!claimed) claim_next();
    if constexpr (YB) {
      // the next item is known and this item's lineage tiles are all taken: its first lineage
      // word goes out now, ahead of the flush
      if (nxt < items && nx.nl > 0) {
        st.lt = nx.l0;
        st.l_ahead = nx.nl;
        st.issue_bits();
      }
    }
    item_flush<LPR, CPL>(acc, rs, acc_r, acc_loss, acc_w, islab + (int64_t)cur * pstride, lane);
    if (nxt >= items) break;
    cur = nxt;
    it = nx;
  }
}

// Sum of the item slab, level 1: block b adds the slab rows [b kItemChunk, (b + 1) kItemChunk)
// column by column in fp64, in row order, into mid row b.  Level 2 (glm_finish_f64_kernel,
// glm_launch.h) adds the mid rows in a fixed order.  The chunk is a constant: the sum's order depends on the
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
template <int LOSS, bool SMP, bool YB = false>
int persist_blocks_per_cu() {   // cached per device and instantiation
  static int occ[kMaxDevices] = {};
  const int dev = current_device();
  if (dev < 0) return 1;
  if (occ[dev] == 0) {
    int o = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, glm_grad_persist_kernel<LOSS, SMP, YB>, kBlock, 0) != hipSuccess ||
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

// The 0/1 labels of a role as a bit plane: word t (16 bits) holds the rows 16 t .. 16 t + 15,
// bit j is row 16 t + j.  One lane per row, the wave's 64 bits by ballot, the lanes 0, 16, 32
// and 48 store one word each; n16 is a multiple of 16, so a wave holds whole words only.
// *flag is set when a label is neither 0.0f nor 1.0f by its bit pattern (NaN, -0.0, 0.5 ...).
constexpr int kPackBlock = 256;
__global__ __launch_bounds__(kPackBlock) void glm_pack_labels_kernel(const float* __restrict__ y, int64_t n16,
                                                                    uint16_t* __restrict__ bits, int* __restrict__ flag) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t step = (int64_t)gridDim.x * kPackBlock;
  // (n16 rounded up to whole waves: every lane of a wave takes part in each ballot)
  const int64_t end = (n16 + kWave - 1) / kWave * kWave;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * kPackBlock + threadIdx.x; i < end; i += step) {
    const bool in = i < n16;
    const uint32_t u = in ? __float_as_uint(y[i]) : 0u;
    bad |= u != 0u && u != 0x3f800000u;
    const unsigned long long m = __ballot(u == 0x3f800000u);
    if ((lane & 15) == 0 && in) bits[i >> 4] = (uint16_t)(m >> lane);
  }
  if (__ballot(bad) != 0ull && lane == 0) atomicOr(flag, 1);
}

}  // namespace

// bits[t] (t < n / 16) = the labels y[16 t .. 16 t + 15] as one bit each (bit j: row 16 t + j);
// only the n / 16 whole tiles are packed.  *flag (a device int the caller has zeroed) is set
// non-zero when one of those labels is neither 0.0f nor 1.0f, compared as bit patterns.
O3S_API int o3s_glm_pack_labels(const float* y, int64_t n, uint16_t* bits, int* flag, hipStream_t st) {
  if (n < 0 || !flag || (n >= 16 && (!y || !bits))) return -1;
  const int64_t n16 = n / 16 * 16;
  if (n16 == 0) return 0;
  const int64_t need = (n16 + kPackBlock - 1) / kPackBlock;
  const int64_t cap = (int64_t)device_cus() * 32;
  hipLaunchKernelGGL(glm_pack_labels_kernel, dim3((unsigned)(need < cap ? need : cap)), dim3(kPackBlock), 0, st, y, n16,
                     bits, flag);
  O3S_CHECK_LAUNCH();
  return 0;
}

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

// Mixed resident + lineage pass in one launch (see glm_grad_mixed_kernel): n_res rows
// of X plus n_lin synthetic rows starting at global row row0; y / sw cover all
// n_res + n_lin rows.  Same out / coef / partial
// contract as o3s_glm_grad (glm_grad.hip; out is overwritten).  waves: 3 asks the register allocator
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
// bits_res / bits_lin: the 0/1 labels of the resident and of the lineage rows as bit planes
// (o3s_glm_pack_labels over y, n_res and over y + n_res, n_lin; each 4-byte aligned with at
// least one dword behind its last word), or null.  With both given, a logistic or hinge pass
// that takes the persistent kernel reads its whole tiles' labels from them
// (glm_grad_persist_kernel<.., YB = true>); the ragged rows' launch and every other pass read y.
// Returns -2, and launches nothing, when islab / imid are smaller than o3s_glm_persist_plan
// says or the ticket is missing.
O3S_API int o3s_glm_grad_mixed(int loss, const void* X, int64_t ld, int64_t n_res, const float* y,
                               const float* sw, const float* coef, uint32_t seed, int64_t row0,
                               int64_t n_lin, float* partial, int grid, double* out, int waves,
                               int64_t res_row0, const int64_t* t_dev, uint32_t sseed,
                               uint32_t sthr, int splits, int full_tiles, int staged, int persist, int item_tiles,
                               float* islab, int64_t islab_floats, double* imid, int64_t imid_doubles,
                               uint32_t* ticket, int persist_blocks, const uint32_t* bits_res,
                               const uint32_t* bits_lin, hipStream_t st) {
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
          return with_bool(smp, [&](auto SMP) {
            launch(glm_grad_staged_kernel<LOSS, SMP>, g, st, Xh + r_lo * ld, r_n, y + r_lo, y_lin, coef, coef + l.dpad,
                   seed, row0 + l_lo, l_n, partial, pstride, res_row0 + r_lo, t_dev, sseed, sthr, pacc);
            return 0;
          });
        }
      }
      return with_bool(waves == 3, [&](auto W3) {
        return with_bool(smp, [&](auto SMP) {
          launch(glm_grad_mixed_kernel<L, C, U, LOSS, (W3 ? 3 : 2), SMP, FULL>, g, st, Xh + r_lo * ld, ld, r_n, y + r_lo,
                 sw ? sw + r_lo : nullptr, y_lin, sw_lin, coef, coef + l.dpad, seed, row0 + l_lo, l_n, partial, pstride,
                 res_row0 + r_lo, t_dev, sseed, sthr, pacc);
          return 0;
        });
      });
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
        with_bool(smp, [&](auto SMP) {
          const int64_t need = (plan.items + kWavesPerBlock - 1) / kWavesPerBlock;
          if constexpr (decltype(LOSS)::value != LOSS_SQUARED) {
            if (bits_res && bits_lin) {
              int64_t fit = (int64_t)persist_blocks_per_cu<LOSS, SMP, true>() * device_cus();
              if (persist_blocks > 0 && persist_blocks < fit) fit = persist_blocks;
              launch(glm_grad_persist_kernel<LOSS, SMP, true>, (int)(fit < need ? fit : need), st, Xh, r_full, bits_res,
                     bits_lin, coef, coef + l.dpad, seed, row0, l_full, islab, pstride, res_row0, t_dev, sseed, sthr,
                     ticket, (uint32_t)plan.items, glm_item_inv((uint64_t)plan.items));
              return 0;
            }
          }
          int64_t fit = (int64_t)persist_blocks_per_cu<LOSS, SMP>() * device_cus();
          if (persist_blocks > 0 && persist_blocks < fit) fit = persist_blocks;
          launch(glm_grad_persist_kernel<LOSS, SMP>, (int)(fit < need ? fit : need), st, Xh, r_full, y, y + n_res, coef,
                 coef + l.dpad, seed, row0, l_full, islab, pstride, res_row0, t_dev, sseed, sthr, ticket,
                 (uint32_t)plan.items, glm_item_inv((uint64_t)plan.items));
          return 0;
        });
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

namespace {

// ---------------------------------------------------------------------------------
// fp32 feature rows (o3s.vector.dtype=float32): the bf16 passes (the gradient pass above, the
// stats, margin and column-moment passes of glm_stats.hip) over X = float
// [n, ld] (ld % 8 == 0, zero padded), with the RowsF32 source.  What that source changes: an
// 8-column chunk is 32 B, two 16-B loads per lane, and the row is held once, unpacked as
// loaded, for the dot product and for X^T r -- twice the row registers of the bf16 kernels,
// so the rows in flight and the register budget are chosen per layout (F32Cfg) to stay out
// of scratch.  fp32 rows never have lineage rows (lineage storage is bf16): one plain
// streaming tile walk per kernel, no lineage code in any instantiation.  The stats, margin
// and column-moment kernels (glm_stats.hip) instantiate the shared bodies; the gradient kernel
// keeps its own tile (below).  The lane -> column
// mapping (the remapped layouts), the slab layout and the fp64 finish are those of the mixed
// pass, so o3s_glm_layout, the workspace, the SGD update kernels and a captured DeviceSGD
// step serve both dtypes.
// (The kernel is in this unit, with grad_tile, not beside glm_grad_kernel in glm_grad.hip:
// compiled without the mixed kernels, which share row_reduce_8x2 with it, its six <8,4,2>
// instantiations come out with other instructions -- hipcc then folds the lane test of
// row_reduce_8x2 before it is inlined.)

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

// Rows in flight per lane (U) and waves per SIMD asked of the register allocator (MW) of
// the fp32 gradient pass, per chunks-per-lane: the widest layouts keep one row at a time
// and one wave per SIMD so that w + acc + the row stay in registers.
template <int C> struct F32Cfg { static constexpr int U = C >= 8 ? 1 : 8 / C, MW = C >= 8 ? 1 : 2; };

}  // namespace

// Gradient/loss pass over fp32 rows: the out / coef / partial contract of o3s_glm_grad (glm_grad.hip)
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
      return with_bool(smp, [&](auto SMP) {
        launch(glm_grad_f32_kernel<L, C, U, LOSS, MW, SMP>, grid, st, Xf + r_lo * ld, ld, r_n, y + r_lo,
               sw ? sw + r_lo : nullptr, coef, coef + l.dpad, partial, pstride, res_row0 + r_lo, t_dev, sseed, sthr,
               pacc);
        return 0;
      });
    });
  });
  if (rc != 0) return rc;
  return launch_finish(partial, grid, pstride, l.dpad + 3, out, accumulate, st);
}

O3S_PRELOAD(glm_mixed)

// Row items of the persistent staged GLM pass (glm_grad_persist_kernel in glm_mixed.hip).
//
// A pass over Tr resident and Tl lineage whole tiles is cut into I = ceil((Tr + Tl) / T)
// items.  Item i holds the resident tiles [floor(i Tr / I), floor((i + 1) Tr / I)) and the
// lineage tiles [floor(i Tl / I), floor((i + 1) Tl / I)): contiguous in each role, evenly
// mixed, at most T tiles of a role (Tr / I <= T), possibly none of one role, and a pure
// function of (Tr, Tl, T).  The waves of the kernel claim item indices from a ticket and the
// entry point sizes the item slab from the same functions, so this header is plain C++: no
// HIP type, usable from a host-only program (tests/test_glm_items_host.py compiles it alone).
//
// Arithmetic: Tr, Tl < 2^31 and I <= 2^31 (the entry point refuses anything else), so every
// product below is at most 2^62.  floor(x / I) is taken as a double-precision estimate
// (x * inv, inv = 1 / I; off by at most one for quotients below 2^31) corrected exactly in
// integers -- a 64-bit integer division is some hundred VALU instructions on the device, and
// a wave cuts four times per item.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define O3S_HD __host__ __device__
#else
#define O3S_HD
#endif

namespace o3s {

struct GlmItem {
  uint32_t r0, nr;   // first resident tile, resident tiles
  uint32_t l0, nl;   // first lineage tile, lineage tiles
};

constexpr uint64_t kGlmItemMaxTiles = uint64_t(1) << 31;   // bound on Tr, Tl (exclusive) and I

// I: the number of items (0 for an empty pass or T == 0).
O3S_HD inline uint64_t glm_item_count(uint64_t Tr, uint64_t Tl, uint64_t T) {
  return T == 0 ? 0 : (Tr + Tl + T - 1) / T;
}
O3S_HD inline double glm_item_inv(uint64_t I) { return 1.0 / (double)I; }

// floor(i n / I) for i <= I, n < 2^31, I <= 2^31; inv = glm_item_inv(I).
O3S_HD inline uint64_t glm_item_cut(uint64_t i, uint64_t n, uint64_t I, double inv) {
  const uint64_t x = i * n;
  uint64_t q = (uint64_t)((double)x * inv);
  while (q * I > x) --q;
  while (x - q * I >= I) ++q;
  return q;
}

O3S_HD inline GlmItem glm_item(uint64_t i, uint64_t Tr, uint64_t Tl, uint64_t I, double inv) {
  const uint64_t r0 = glm_item_cut(i, Tr, I, inv), r1 = glm_item_cut(i + 1, Tr, I, inv);
  const uint64_t l0 = glm_item_cut(i, Tl, I, inv), l1 = glm_item_cut(i + 1, Tl, I, inv);
  return GlmItem{(uint32_t)r0, (uint32_t)(r1 - r0), (uint32_t)l0, (uint32_t)(l1 - l0)};
}

}  // namespace o3s

"""The row items of the persistent staged GLM pass (csrc/glm_items.h), checked on the host: the
header is compiled alone into a small program under UBSan + ASan and run over a grid of (Tr, Tl,
T) and over the tile counts of the 1B-row benchmark, where a 32-bit product would wrap.  An item
out of range would make the kernel read past the table, so the partition is proven here first.
Against exact 128-bit arithmetic: every cut is floor(i n / I); the items of each role are in
order, start at tile 0, end at the last tile and leave no gap (every tile exactly once); no item
holds more than T + 1 tiles of a role; no product the header forms reaches 2^63."""
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "orange3_spark_amd" / "ops" / "csrc"

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "glm_items.h"
using namespace o3s;
typedef unsigned __int128 u128;
static int check(uint64_t Tr, uint64_t Tl, uint64_t T) {
  const uint64_t I = glm_item_count(Tr, Tl, T);
  if (I != (uint64_t)(((u128)Tr + Tl + T - 1) / T)) { std::printf("count %llu\n", (unsigned long long)I); return 1; }
  if (I == 0) return Tr + Tl == 0 ? 0 : 1;
  const double inv = glm_item_inv(I);
  const u128 lim = (u128)1 << 63;
  const uint64_t m = Tr > Tl ? Tr : Tl;
  // the largest products of glm_item_cut: i n with i <= I, and (q + 1) I with q <= n
  if ((u128)I * m >= lim || ((u128)m + 2) * I >= lim) { std::printf("intermediate past 2^63\n"); return 1; }
  uint64_t r = 0, l = 0;
  for (uint64_t i = 0; i < I; ++i) {
    const GlmItem it = glm_item(i, Tr, Tl, I, inv);
    const uint64_t er0 = (uint64_t)((u128)i * Tr / I), er1 = (uint64_t)((u128)(i + 1) * Tr / I);
    const uint64_t el0 = (uint64_t)((u128)i * Tl / I), el1 = (uint64_t)((u128)(i + 1) * Tl / I);
    if (it.r0 != er0 || it.nr != er1 - er0 || it.l0 != el0 || it.nl != el1 - el0) {
      std::printf("item %llu is not the exact cut\n", (unsigned long long)i);
      return 1;
    }
    if (it.r0 != r || it.l0 != l) { std::printf("item %llu leaves a gap or overlaps\n", (unsigned long long)i); return 1; }
    if (it.nr > T + 1 || it.nl > T + 1) { std::printf("item %llu too large\n", (unsigned long long)i); return 1; }
    r += it.nr;
    l += it.nl;
  }
  if (r != Tr || l != Tl) { std::printf("tiles left over\n"); return 1; }
  return 0;
}
int main() {
  const uint64_t ns[] = {0, 1, 2, 7, 255, 256, 257}, ts[] = {1, 2, 8, 128};
  int cases = 0;
  for (uint64_t Tr : ns)
    for (uint64_t Tl : ns)
      for (uint64_t T : ts) {
        if (check(Tr, Tl, T)) { std::printf("FAILED Tr=%llu Tl=%llu T=%llu\n", (unsigned long long)Tr, (unsigned long long)Tl, (unsigned long long)T); return 1; }
        ++cases;
      }
  const uint64_t bench_ts[] = {128, 256};
  for (uint64_t T : bench_ts) {
    if (check(31112243ull, 31387756ull, T)) { std::printf("FAILED bench T=%llu\n", (unsigned long long)T); return 1; }
    ++cases;
  }
  // the header's own bound: tile counts just below 2^31
  if (check((1ull << 31) - 1, (1ull << 31) - 1, 4096)) { std::printf("FAILED bound\n"); return 1; }
  ++cases;
  std::printf("OK %d cases\n", cases);
  return 0;
}
"""


def test_glm_items_partition_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    src = tmp_path / "items_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "items_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                    "-I", str(CSRC), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == f"OK {7 * 7 * 4 + 2 + 1} cases"

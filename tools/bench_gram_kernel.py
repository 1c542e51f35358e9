"""Fused weighted Gram pass (ops.gram.weighted_gram, csrc/gram.hip) against the path it replaces.

Per shape and row dtype (fp32, bf16), weighted with y, in ONE process, alternating, device
events, after a warm-up:
  * kernel:  ``weighted_gram(X, d, w, y)`` on the stored rows;
  * parent:  what ``_normal_equations`` did before -- ``X.to(float64)``, ``Xw = Xd * w``, two
             ``rows_t_matmul`` calls and the sums;
  * colstats: ``glm_colstats`` over the same rows, the achieved-bandwidth yardstick.
Also the peak memory either path adds to the table, and the larger of the byte bound (8 TB/s
HBM peak) and the MFMA bound (computed from the kernel's tile split: tiles of the busiest wave x
6 products x 4 k-steps x 32 cycles per 64-row tile and CU, at 2.4 GHz) per shape.

    python tools/bench_gram_kernel.py [--out profiles/gram_pass.json] [--runs 10] [--shapes 4000000x64,...]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orange3_spark_amd.ops import glm as G  # noqa: E402
from orange3_spark_amd.ops import gram as GR  # noqa: E402

HBM_PEAK = 8.0e12
CLOCK = 2.4e9


def _parent(X, d, w, y):
    Xd = X[:, :d].to(torch.float64)
    yd = y.to(torch.float64)
    wd = w.to(torch.float64)
    Xw = Xd * wd[:, None]
    return torch.cat([GR.rows_t_matmul(Xw, Xd).reshape(-1), GR.rows_t_matmul(Xw, yd), Xw.sum(0),
                      (wd * yd).sum().reshape(1), wd.sum().reshape(1), (wd * yd * yd).sum().reshape(1)])


def _kernel(X, d, w, y):
    return GR.weighted_gram(X, d, w, y).G


def _timed(fns, runs):
    """Alternate the callables; ms per run each (device events)."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [sorted(m)[len(m) // 2] for m in ms], [min(m) for m in ms]


def _peak(f):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _mfma_bound_s(n, d, cus):
    nba = (d + 2 + 31) // 32
    tw = (nba * (nba + 1) // 2 + 3) // 4
    tiles = (n + 63) // 64
    return -(-tiles // cus) * tw * 6 * 4 * 32 / CLOCK


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/gram_pass.json")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--shapes", default="4000000x64,20000000x128,20000000x256")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    res = {"device": torch.cuda.get_device_name(dev), "cus": cus, "runs": a.runs, "flush_rows": GR.FLUSH_ROWS,
           "shapes": {}}
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        w = torch.rand(n, device=dev, generator=g) + 0.5
        y = torch.randn(n, device=dev, generator=g)
        off = torch.tensor([50.0, -50.0, 50.0, -50.0, 10.0, 0.0, 50.0, -50.0], device=dev).repeat(d // 8)
        for dtype in (torch.float32, torch.bfloat16):
            X = torch.empty((n, d), dtype=dtype, device=dev)
            step = 1 << 22
            for s in range(0, n, step):
                X[s:s + step] = (torch.randn((min(step, n - s), d), device=dev, generator=g) + off).to(dtype)
            nbytes = X.numel() * X.element_size()
            fns = [lambda: _kernel(X, d, w, y), lambda: _parent(X, d, w, y), lambda: G.glm_colstats(X, w)]
            med, best = _timed(fns, a.runs)
            bound = max(nbytes / HBM_PEAK, _mfma_bound_s(n, d, cus))
            r = {"table_bytes": nbytes,
                 "kernel_ms": round(med[0], 3), "kernel_min_ms": round(best[0], 3),
                 "parent_ms": round(med[1], 3), "parent_min_ms": round(best[1], 3),
                 "colstats_ms": round(med[2], 3),
                 "kernel_bytes_per_s": round(nbytes / (med[0] * 1e-3), 0),
                 "colstats_bytes_per_s": round(nbytes / (med[2] * 1e-3), 0),
                 "byte_bound_ms": round(nbytes / HBM_PEAK * 1e3, 3),
                 "mfma_bound_ms": round(_mfma_bound_s(n, d, cus) * 1e3, 3),
                 "bound_ms": round(bound * 1e3, 3),
                 "kernel_peak_bytes": _peak(fns[0]), "parent_peak_bytes": _peak(fns[1])}
            res["shapes"][f"{n}x{d}_{'f32' if dtype == torch.float32 else 'bf16'}"] = r
            print(json.dumps({shape: r}), flush=True)
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
            del X
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""Micro-benchmark of the fp32-row GLM gradient pass on one GPU, against the bf16 pass and the
chunked fp64 torch pass (what fp32 rows took before the fp32 kernels), plus the assembler
writing fp32 and bf16 rows.

All three gradient passes run over the same number of rows in one process; the two kernel
passes are timed in alternating rounds (device-synchronised host clock around ``iters``
launches) and the median round is reported.  Bytes are what the pass has to read: the rows
plus the fp32 label column.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orange3_spark_amd.frame import column as C  # noqa: E402
from orange3_spark_amd.models.glm import GlmData  # noqa: E402
from orange3_spark_amd.ops import _native as N  # noqa: E402
from orange3_spark_amd.ops import assemble as A  # noqa: E402
from orange3_spark_amd.ops import glm as G  # noqa: E402
from orange3_spark_amd.parallel.comm import LocalComm  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def rate(rows, row_bytes, secs):
    return {"ms": secs * 1e3, "rows_per_s": rows / secs, "bytes_per_s": rows * row_bytes / secs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--asm-rows", type=int, default=16_000_000)
    ap.add_argument("--asm-cols", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "glm_f32_pass.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_glm_f32 needs a GPU")
    dev = torch.device("cuda", 0)
    n, d = a.rows, a.d
    ld = G.padded_width(d)
    Xb, y = G.synth_glm(n, d, seed=1, device=dev)
    # fp32 rows that are not representable in bf16
    X32 = Xb.float() * 3.0 + torch.rand((n, ld), device=dev) * 1e-3
    coef = torch.full((ld,), 0.01, device=dev)
    tiles = -(-n // 16)
    grid = max(1, min(N.num_cus(dev) * 32, -(-tiles // 4)))        # GlmData's mixed-pass grid
    ws = G.GlmWorkspace(dev, ld, grid=grid)
    f32 = lambda: G.glm_grad_mixed(X32, y, None, 0, d, 0, 0, coef, 0.0, 0, ws)      # noqa: E731
    bf16 = lambda: G.glm_grad_mixed(Xb, y, None, 0, d, 1, 0, coef, 0.0, 0, ws)      # noqa: E731
    for fn in (f32, bf16):
        timed(fn, 10)                                              # warm-up: code objects, clocks
    t32, tbf = [], []
    for _ in range(a.rounds):
        t32.append(timed(f32, a.iters))
        tbf.append(timed(bf16, a.iters))
    res = {"rows": n, "d": d, "grid": grid, "iters": a.iters, "rounds": a.rounds,
           "grad_f32": rate(n, ld * 4 + 4, statistics.median(t32)),
           "grad_bf16_mixed": rate(n, ld * 2 + 4, statistics.median(tbf)),
           "grad_f32_rounds_ms": [t * 1e3 for t in t32], "grad_bf16_rounds_ms": [t * 1e3 for t in tbf]}
    res["f32_over_bf16_byte_rate"] = res["grad_f32"]["bytes_per_s"] / res["grad_bf16_mixed"]["bytes_per_s"]

    # what fp32 rows took before: chunked fp64 torch math (GlmData.pass_torch)
    data = GlmData(LocalComm(dev), C.VectorColumn(X32, d), y)
    cf = coef.double().cpu()
    timed(lambda: data.pass_torch(cf, 0.0, 0), 1)
    res["grad_f32_pass_torch"] = rate(n, ld * 4 + 4, timed(lambda: data.pass_torch(cf, 0.0, 0), 3))
    res["kernel_over_pass_torch"] = res["grad_f32_pass_torch"]["ms"] / res["grad_f32"]["ms"]
    ref = data.pass_torch(cf, 0.0, 0)
    out = f32().clone()
    res["grad_f32_vs_fp64_max_rel"] = float(((out[:ld] - ref[:ld]).abs().max() / ref[:ld].abs().max()).item())
    del data, X32, Xb, ref

    # assembler: fp64 columns -> fp32 / bf16 rows
    m, k = a.asm_rows, a.asm_cols
    cols = [torch.randn(m, dtype=torch.float64, device=dev) for _ in range(k)]
    srcs = [(c, None, 1) for c in cols]
    ta = {torch.float32: [], torch.bfloat16: []}
    for dt in ta:
        timed(lambda: A.assemble(srcs, m, dev, dt), 3)
    for _ in range(a.rounds):
        for dt in ta:
            ta[dt].append(timed(lambda: A.assemble(srcs, m, dev, dt), 10))
    kp = G.padded_width(k)
    res["assemble_rows"], res["assemble_cols"] = m, k
    res["assemble_f64_to_f32"] = rate(m, k * 8 + kp * 4, statistics.median(ta[torch.float32]))
    res["assemble_f64_to_bf16"] = rate(m, k * 8 + kp * 2, statistics.median(ta[torch.bfloat16]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Multinomial LogisticRegression: seconds per objective/gradient pass and per fit.

Synthetic n x d features (bf16 vector column, as VectorAssembler / synthetic produce) with
K classes; prints one JSON line.

``--dtype float32`` keeps the same rows as a padded fp32 vector column (what a session with
``o3s.vector.dtype=float32`` assembles) and records, per pass, seconds and bytes/s of the
fused pass on them, of the bf16 kernel on the bf16 rows in the same run, and of the chunked
path (``O3S_SOFTMAX_KERNEL=0``) on the same fp32 rows."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orange3_spark_amd import Session  # noqa: E402


def _f32_column(X: torch.Tensor) -> torch.Tensor:
    """The [:, :d] view of a zero-padded fp32 copy of X, scaled off the bf16 grid."""
    from orange3_spark_amd.ops import glm as G
    n, d = X.shape
    base = torch.zeros((n, G.padded_width(d)), dtype=torch.float32, device=X.device)
    for a in range(0, n, 1 << 21):
        base[a:a + (1 << 21), :d] = X[a:a + (1 << 21)].float() * 1.0001
    return base[:, :d]


def _time_pass(X, y32, W, b, reps):
    """Device seconds of one fused pass (operand split + kernel + finish), mean of ``reps``
    passes queued back to back between two events."""
    from orange3_spark_amd.ops import glm as G
    G.softmax_pass(X, y32, None, W, b)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        G.softmax_pass(X, y32, None, W, b)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps


def _time_fit(s, X, y, classes, iters, sync):
    """(fit seconds, optimizer result, seconds of every objective/gradient evaluation)."""
    from orange3_spark_amd.models import glm as GLM
    from orange3_spark_amd.models import optim
    evals = []
    real = optim.lbfgs

    def timed_lbfgs(fg, x0, **kw):
        def tfg(x):
            sync()
            t = time.perf_counter()
            out = fg(x)
            sync()
            evals.append(time.perf_counter() - t)
            return out
        return real(tfg, x0, **kw)
    optim.lbfgs = timed_lbfgs
    try:
        sync()
        t = time.perf_counter()
        B, b, r = GLM.fit_multinomial(s.comm, X, y, None, classes, max_iter=iters, tol=0.0)
        sync()
        return time.perf_counter() - t, r, evals
    finally:
        optim.lbfgs = real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--features", type=int, default=256)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dtype", choices=["bfloat16", "float32"], default="bfloat16")
    ap.add_argument("--reps", type=int, default=10, help="timed repeats of a single pass")
    a = ap.parse_args()
    s = Session.getOrCreate()
    from orange3_spark_amd.ml import common as U
    from orange3_spark_amd.ops import glm as G
    df = s.synthetic.classification(a.rows, a.features, seed=3)
    Xb = U.dense_features(df, "features")
    # K ordered classes from two features (learnable)
    z = (Xb[:, 0].float() + 0.5 * Xb[:, 1].float() + 1.5) / 3.0
    y = (z * a.classes).floor().clamp(0, a.classes - 1).to(torch.float64)
    sync = torch.cuda.synchronize if Xb.is_cuda else (lambda: None)
    X = _f32_column(Xb) if a.dtype == "float32" else Xb
    dt, r, evals = _time_fit(s, X, y, a.classes, a.iters, sync)
    out = {"metric": "multinomial LR fit", "rows": a.rows, "features": a.features, "classes": a.classes,
           "x_dtype": str(X.dtype), "fit_s": dt, "iters": r.iterations, "s_per_iter": dt / max(r.iterations, 1),
           "x_shape": list(X.shape), "x_contiguous": X.is_contiguous(),
           "eval_s": statistics.median(evals), "evals": len(evals)}
    if a.dtype == "float32" and X.is_cuda:
        y32 = y.to(torch.int32)
        g = torch.Generator().manual_seed(1)
        W = (torch.randn((a.classes, a.features), generator=g) * 0.3).to(X.device)
        b = (torch.randn(a.classes, generator=g) * 0.5).to(X.device)

        def rec(sec, nbytes):
            return {"s": sec, "bytes_per_s": nbytes / sec}
        f32_bytes = X.shape[0] * X.stride(0) * 4
        bf_bytes = Xb.shape[0] * Xb.stride(0) * 2
        out["fused_kernel"] = G.softmax_kernel_ok(X, a.classes)
        out["pass_float32"] = rec(_time_pass(X, y32, W, b, a.reps), f32_bytes)
        out["pass_bfloat16"] = rec(_time_pass(Xb, y32, W, b, a.reps), bf_bytes)
        out["eval_float32"] = rec(out["eval_s"], f32_bytes)
        os.environ["O3S_SOFTMAX_KERNEL"] = "0"
        try:
            dtc, rc, evc = _time_fit(s, X, y, a.classes, min(a.iters, 3), sync)
        finally:
            del os.environ["O3S_SOFTMAX_KERNEL"]
        out["eval_float32_chunked"] = rec(statistics.median(evc), f32_bytes)
        out["chunked_over_fused"] = out["eval_float32_chunked"]["s"] / out["eval_float32"]["s"]
        out["f32_over_bf16_bytes_per_s"] = out["pass_float32"]["bytes_per_s"] / out["pass_bfloat16"]["bytes_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()

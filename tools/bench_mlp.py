"""MultilayerPerceptronClassifier: the fused MLP passes against the torch program
(``O3S_MLP_KERNEL=0``).

One process; per shape and row dtype, on the same GPU frame and with the two paths
alternating (warm-up, then ``--runs`` runs each, device events around back-to-back calls):

* seconds per objective / gradient evaluation (``Objective.local`` of the fit);
* seconds per ``transform`` of the fitted classifier;
* peak memory a 10-iteration fit adds to what was allocated before it;
* seconds and bytes/s of ``glm_softmax`` with K = 10 on the same rows, the byte-rate yardstick.

A shape the gate gives back to the torch program on a row type is reported as ``"gated": true``
with the torch program's figures only.  Prints one JSON line per (shape, dtype) and, with
``--out``, writes the list to a file."""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orange3_spark_amd import Session, SessionConf  # noqa: E402

SWITCH = "O3S_MLP_KERNEL"


def _events(fn, reps):
    """Device seconds per call of ``fn``: ``reps`` calls queued back to back between two events."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps


def _frame(s, n, d, H, K, dtype):
    """n x d rows of ``dtype`` and labels drawn from a planted [d, H, K] network."""
    from orange3_spark_amd.frame import column as C
    from orange3_spark_amd.frame.dataframe import DataFrame
    from orange3_spark_amd.ops import mlp as MLP
    dev = s.device
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.empty((n, d), dtype=dtype, device=dev)
    y = torch.empty(n, dtype=torch.float64, device=dev)
    W1 = torch.randn((d, H), generator=g, device=dev) / d ** 0.5
    W2 = torch.randn((H, K), generator=g, device=dev) * 2.0 / H ** 0.5
    b1, b2 = torch.zeros(H, device=dev), torch.zeros(K, device=dev)
    for a in range(0, n, 1 << 20):
        b = min(n, a + (1 << 20))
        X[a:b] = torch.randn((b - a, d), generator=g, device=dev)
        P = torch.softmax(MLP.mlp_logits_torch(X[a:b].float(), W1, b1, W2, b2).float(), dim=1)
        y[a:b] = torch.multinomial(P, 1, generator=g).reshape(-1).double()
    return DataFrame(s, OrderedDict(features=C.VectorColumn(X), label=C.NumericColumn(y)), n), X


def _objective(est, df):
    """The objective ``fit`` would minimise and its start, without running the solver."""
    from orange3_spark_amd.models import dist_opt
    real, got = dist_opt.lbfgs, {}

    def capture(obj, x0, *a, **k):
        got["obj"], got["x0"] = obj, x0
        return real(obj, x0, 1, *a[1:], **k)
    dist_opt.lbfgs = capture
    try:
        est.fit(df)
    finally:
        dist_opt.lbfgs = real
    obj = got["obj"]
    theta = torch.from_numpy(got["x0"]).to(obj.device, obj.dtype)
    return obj, theta


def _with_switch(on, fn):
    if on:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = "0"
    try:
        return fn()
    finally:
        os.environ.pop(SWITCH, None)


def _fit_peak(est, df, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    est.fit(df)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - before


def measure(s, n, d, H, K, dtype, runs, reps):
    from orange3_spark_amd.ml import _mlp
    from orange3_spark_amd.ml import classification as CL
    from orange3_spark_amd.ops import glm as G
    df, X = _frame(s, n, d, H, K, dtype)
    dev = X.device
    table = X.element_size() * X.numel()
    est = CL.MultilayerPerceptronClassifier(layers=[d, H, K], maxIter=10, tol=0.0, seed=1)
    fused_obj, theta = _with_switch(True, lambda: _objective(est, df))
    torch_obj, _ = _with_switch(False, lambda: _objective(est, df))
    gated = not isinstance(fused_obj, _mlp._FusedMLPObjective)
    assert not isinstance(torch_obj, _mlp._FusedMLPObjective)
    model = _with_switch(True, lambda: est.fit(df))
    paths = ((False, torch_obj),) if gated else ((True, fused_obj), (False, torch_obj))
    ev = {True: [], False: []}
    tr = {True: [], False: []}
    for on, obj in paths:               # warm-up
        _with_switch(on, lambda: (obj.local(theta), model.transform(df)))
    for _ in range(runs):
        for on, obj in paths:
            k = reps if on else max(1, reps // 4)
            ev[on].append(_with_switch(on, lambda: _events(lambda: obj.local(theta), k)))
            tr[on].append(_with_switch(on, lambda: _events(lambda: model.transform(df), k)))
    peak = {on: _with_switch(on, lambda: _fit_peak(est, df, dev)) for on, _ in paths}
    # the byte-rate yardstick: glm_softmax with K = 10 on the same rows
    g = torch.Generator().manual_seed(1)
    W = (torch.randn((10, d), generator=g) * 0.3).to(dev)
    b = (torch.randn(10, generator=g) * 0.5).to(dev)
    y10 = torch.randint(0, 10, (n,), generator=g).to(dev, torch.int32)
    G.softmax_pass(X, y10, None, W, b)
    sm = [_events(lambda: G.softmax_pass(X, y10, None, W, b), reps) for _ in range(runs)]
    med = statistics.median
    out = {"metric": "MLP fused pass vs torch program", "rows": n, "features": d, "hidden": H, "classes": K,
           "x_dtype": str(dtype), "table_bytes": table, "runs": runs, "gated": gated,
           "eval_torch_s": ev[False], "transform_torch_s": tr[False], "fit10_peak_added_torch_bytes": peak[False],
           "softmax_k10_s": sm, "softmax_k10_bytes_per_s": table / med(sm)}
    if not gated:
        out.update({"eval_fused_s": ev[True], "eval_ratio": med(ev[False]) / med(ev[True]),
                    "eval_ratio_min": min(ev[False]) / max(ev[True]), "eval_ratio_max": max(ev[False]) / min(ev[True]),
                    "eval_fused_bytes_per_s": table / med(ev[True]),
                    "transform_fused_s": tr[True], "transform_ratio": med(tr[False]) / med(tr[True]),
                    "transform_ratio_min": min(tr[False]) / max(tr[True]),
                    "transform_ratio_max": max(tr[False]) / min(tr[True]),
                    "fit10_peak_added_fused_bytes": peak[True],
                    "mlp_over_softmax_time": med(ev[True]) / med(sm)})
    del df, X, model, fused_obj, torch_obj
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4000000x256x64x10,20000000x64x128x10",
                    help="comma-separated rows x features x hidden x classes")
    ap.add_argument("--dtypes", default="bfloat16,float32")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8, help="back-to-back calls of the fused path per run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp needs a GPU: the torch program on a CPU says nothing about either path")
    s = Session(SessionConf().set("o3s.device", "cuda"))
    results = []
    for shape in a.shapes.split(","):
        n, d, H, K = (int(v) for v in shape.split("x"))
        for name in a.dtypes.split(","):
            r = measure(s, n, d, H, K, getattr(torch, name), a.runs, a.reps)
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

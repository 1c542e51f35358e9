"""Multinomial LogisticRegression, NaiveBayes and PCA ``transform`` on the linear scoring
kernel (ops/linear_predict.py, csrc/linear_predict.hip) against the torch paths it replaces
(``O3S_LINEAR_PREDICT_FUSED=0``: the same model then runs the old code).

Models are built directly from random parameters (no fit); rows are random on the device.  Per
shape, in ONE process, the two paths alternate, three runs each after a warm-up, host clock
around a device synchronise:
  * transform: ``model.transform(df)`` (every output column of the model);
  * kernel:    ``ops.linear_predict.linear_predict`` alone with the same outputs, device events,
               with the staged store and with the direct store;
  * softmax:   for the LogisticRegression shapes one ``ops.glm.softmax_pass`` (the fit's
               forward + backward pass over the same rows), device events;
  * the peak memory each transform adds to the table; an out-of-memory of the old path is
    recorded as such instead of a time.
The kernel's byte bound is (row bytes + output bytes) / 8.0 TB/s.

    python tools/bench_linear_predict.py [--out profiles/linear_predict.json] [--runs 3] [--rows 20000000]
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orange3_spark_amd import Session, SessionConf  # noqa: E402
from orange3_spark_amd.frame import column as C  # noqa: E402
from orange3_spark_amd.frame.dataframe import DataFrame  # noqa: E402
from orange3_spark_amd.ml import classification as CLS  # noqa: E402
from orange3_spark_amd.ml import feature as FT  # noqa: E402
from orange3_spark_amd.ops import glm as G  # noqa: E402
from orange3_spark_amd.ops import linear_predict as LP  # noqa: E402

HBM_PEAK = 8.0e12
SWITCH = "O3S_LINEAR_PREDICT_FUSED"

# name: (model, features, outputs, row dtype)
SHAPES = OrderedDict([
    ("lr_256x10_bf16", ("lr", 256, 10, torch.bfloat16)),
    ("lr_256x10_f32", ("lr", 256, 10, torch.float32)),
    ("nb_64x4_bf16", ("nb", 64, 4, torch.bfloat16)),
    ("pca_256x8_bf16", ("pca", 256, 8, torch.bfloat16)),
])


def make_model(kind, d, K, seed=0):
    """(model, packed operands, the outputs its transform writes)."""
    rng = np.random.default_rng(seed)
    if kind == "lr":
        m = CLS.LogisticRegressionModel._from(rng.normal(size=(K, d)) / np.sqrt(d), rng.normal(size=K), True, K)
        return m, LP.pack(m._B, m._b), dict(raw=True, prob=True, pred=True)
    if kind == "nb":
        theta = torch.log_softmax(torch.from_numpy(rng.normal(size=(K, d))), 1).numpy()
        pi = torch.log_softmax(torch.from_numpy(rng.normal(size=K)), 0).numpy()
        m = CLS.NaiveBayesModel._from(pi, theta, np.zeros((0, 0)), "multinomial")
        return m, LP.pack(theta, pi), dict(raw=True, prob=True, pred=True)
    m = FT.PCAModel()
    m._pc = np.linalg.qr(rng.normal(size=(d, K)))[0]
    m._set(inputCol="features", outputCol="pca")
    return m, LP.pack(m._pc.T), dict(raw=True)


def make_rows(kind, n, d, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.empty((n, d), dtype=dtype, device=dev)
    for s in range(0, n, 1 << 22):
        m = min(1 << 22, n - s)
        if kind == "nb":                                   # term counts
            X[s:s + m] = torch.poisson(torch.full((m, d), 3.0, device=dev), generator=g).to(dtype)
        else:
            X[s:s + m] = torch.randn((m, d), device=dev, generator=g).to(dtype)
    return X


def _wall(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def _events(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _peak(f):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _guarded(f):
    """f(), or the allocation failure as text (the old path's converted copy may not fit)."""
    try:
        return f()
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return f"out of memory: {str(e).splitlines()[0]}"


def _stats(v):
    nums = [x for x in v if not isinstance(x, str)]
    if len(nums) != len(v):
        return {"runs": v}
    return {"runs": [round(x, 3) for x in v], "mean": round(sum(v) / len(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3)}


def _transform(model, df, fused):
    if fused:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = "0"
    try:
        out = model.transform(df)
        return [out.column_data(c) for c in out.columns]
    finally:
        os.environ.pop(SWITCH, None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/linear_predict.json")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sess = Session(SessionConf().set("o3s.device", "cuda"))
    res = {"device": torch.cuda.get_device_name(dev), "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
           "runs": a.runs, "rows": a.rows, "shapes": {}}
    n = a.rows
    for name in a.shapes.split(","):
        kind, d, K, dtype = SHAPES[name]
        X = make_rows(kind, n, d, dtype, dev)
        df = DataFrame(sess, OrderedDict(features=C.VectorColumn(X, d)), n)
        model, packed, outs = make_model(kind, d, K)
        assert LP.column_rows(df.column_data("features"), d) is not None, "the gate refused a benchmark shape"
        nbytes = X.numel() * X.element_size()
        _transform(model, df, True)                                       # warm-up of both paths
        _guarded(lambda: _transform(model, df, False))
        LP.linear_predict(X, d, packed, direct_store=True, **outs)
        t = {"transform": [], "transform_old": [], "kernel": [], "kernel_direct_store": []}
        if kind == "lr":
            y = torch.randint(0, K, (n,), device=dev, dtype=torch.int32)
            W, b = torch.from_numpy(model._B).float().to(dev), torch.from_numpy(model._b).float().to(dev)
            G.softmax_pass(X, y, None, W, b)
            t["softmax_pass"] = []
        for _ in range(a.runs):
            t["transform"].append(_wall(lambda: _transform(model, df, True)))
            t["transform_old"].append(_guarded(lambda: _wall(lambda: _transform(model, df, False))))
            t["kernel"].append(_events(lambda: LP.linear_predict(X, d, packed, **outs)))
            t["kernel_direct_store"].append(_events(lambda: LP.linear_predict(X, d, packed, direct_store=True, **outs)))
            if kind == "lr":
                t["softmax_pass"].append(_events(lambda: G.softmax_pass(X, y, None, W, b)))
        out_bytes = 8 * n * (K * (int(outs.get("raw", False)) + int(outs.get("prob", False)))
                             + int(outs.get("pred", False)))
        r = {"table_bytes": nbytes, "output_bytes": out_bytes, "d": d, "K": K, "grid": LP.launch_grid(X, d)}
        r.update({k + "_ms": _stats(v) for k, v in t.items()})
        r["byte_bound_ms"] = round((nbytes + out_bytes) / HBM_PEAK * 1e3, 3)
        r["kernel_over_byte_bound"] = round(r["kernel_ms"]["mean"] / r["byte_bound_ms"], 2)
        new, was = r["transform_ms"], r["transform_old_ms"]
        r["old_over_new"] = round(was["mean"] / new["mean"], 2) if "mean" in was else None
        r["faster"] = bool(new["max"] < was["min"]) if "mean" in was else None
        r["transform_peak_bytes"] = _peak(lambda: _transform(model, df, True))
        r["transform_old_peak_bytes"] = _guarded(lambda: _peak(lambda: _transform(model, df, False)))
        res["shapes"][name] = r
        print(json.dumps({name: r}), flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        X = df = model = packed = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

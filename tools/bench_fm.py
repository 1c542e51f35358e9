"""Factorization machines: the fused FM passes against the torch program (``O3S_FM_KERNEL=0``).

One process; per shape and row dtype, on the same GPU frame and with the two paths
alternating (warm-up, then ``--runs`` runs each, device events around back-to-back calls):

* seconds per objective / gradient evaluation (``Objective.local`` of the fit);
* seconds per ``transform`` of the fitted classifier;
* peak memory a 10-iteration fit adds to what was allocated before it;
* seconds and bytes/s of ``glm_softmax`` with K = 10 on the same rows, the structural twin of
  the FM pass, for the distance from the stream rate.

Prints one JSON line per (shape, dtype) and, with ``--out``, writes the list to a file."""
import argparse
import json
import os
import statistics
import sys
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orange3_spark_amd import Session, SessionConf  # noqa: E402

SWITCH = "O3S_FM_KERNEL"


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


def _frame(s, n, d, F, dtype):
    """n x d rows of ``dtype`` and 0/1 labels drawn from a planted FM model."""
    from orange3_spark_amd.frame import column as C
    from orange3_spark_amd.frame.dataframe import DataFrame
    from orange3_spark_amd.ops import fm as FM
    dev = s.device
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.empty((n, d), dtype=dtype, device=dev)
    for a in range(0, n, 1 << 21):
        b = min(n, a + (1 << 21))
        X[a:b] = torch.randn((b - a, d), generator=g, device=dev)
    V = torch.randn((d, F), generator=g, device=dev) * 0.5 / d ** 0.5
    w = torch.randn(d, generator=g, device=dev) * 0.3 / d ** 0.5
    m = FM.fm_margin(X, V, w, 0.0)
    y = (torch.rand(n, generator=g, device=dev) < torch.sigmoid(m)).to(torch.float64)
    return DataFrame(s, OrderedDict(features=C.VectorColumn(X), label=C.NumericColumn(y)), n), X


def _objective(est, df):
    """The objective ``fit`` would minimise and its start, without running the solver."""
    from orange3_spark_amd.ml import _fm
    from orange3_spark_amd.models import dist_opt
    real, got = dist_opt.gradient_descent, {}

    def capture(obj, x0, *a, **k):
        got["obj"], got["x0"] = obj, x0
        return real(obj, x0, 1, *a[1:], **k)
    dist_opt.gradient_descent = capture
    try:
        _fm._fit_fm(est, df, True)
    finally:
        dist_opt.gradient_descent = real
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


def measure(s, n, d, F, dtype, runs, reps):
    from orange3_spark_amd.ml import _fm
    from orange3_spark_amd.ml import classification as CL
    from orange3_spark_amd.ops import glm as G
    df, X = _frame(s, n, d, F, dtype)
    dev = X.device
    table = X.element_size() * X.numel()
    est = CL.FMClassifier(factorSize=F, maxIter=10, stepSize=0.05, tol=0.0, seed=1)
    fused_obj, theta = _with_switch(True, lambda: _objective(est, df))
    torch_obj, _ = _with_switch(False, lambda: _objective(est, df))
    assert isinstance(fused_obj, _fm._FusedFMObjective) and not isinstance(torch_obj, _fm._FusedFMObjective)
    model = _with_switch(True, lambda: est.fit(df))
    ev = {True: [], False: []}
    tr = {True: [], False: []}
    for on, obj in ((True, fused_obj), (False, torch_obj)):               # warm-up
        _with_switch(on, lambda: (obj.local(theta), model.transform(df)))
    for _ in range(runs):
        for on, obj in ((True, fused_obj), (False, torch_obj)):
            k = reps if on else max(1, reps // 4)
            ev[on].append(_with_switch(on, lambda: _events(lambda: obj.local(theta), k)))
            tr[on].append(_with_switch(on, lambda: _events(lambda: model.transform(df), k)))
    peak = {on: _with_switch(on, lambda: _fit_peak(est, df, dev)) for on in (True, False)}
    # the structural twin: glm_softmax with K = 10 on the same rows
    g = torch.Generator().manual_seed(1)
    W = (torch.randn((10, d), generator=g) * 0.3).to(dev)
    b = (torch.randn(10, generator=g) * 0.5).to(dev)
    y10 = torch.randint(0, 10, (n,), generator=g).to(dev, torch.int32)
    G.softmax_pass(X, y10, None, W, b)
    sm = [_events(lambda: G.softmax_pass(X, y10, None, W, b), reps) for _ in range(runs)]
    med = statistics.median
    out = {"metric": "FM fused pass vs torch program", "rows": n, "features": d, "factors": F,
           "x_dtype": str(dtype), "table_bytes": table, "runs": runs,
           "eval_fused_s": ev[True], "eval_torch_s": ev[False],
           "eval_ratio": med(ev[False]) / med(ev[True]),
           "eval_fused_bytes_per_s": table / med(ev[True]),
           "transform_fused_s": tr[True], "transform_torch_s": tr[False],
           "transform_ratio": med(tr[False]) / med(tr[True]),
           "fit10_peak_added_fused_bytes": peak[True], "fit10_peak_added_torch_bytes": peak[False],
           "softmax_k10_s": sm, "softmax_k10_bytes_per_s": table / med(sm),
           "fm_over_softmax_time": med(ev[True]) / med(sm)}
    del df, X, model, fused_obj, torch_obj
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4000000x256,20000000x64", help="comma-separated rows x features")
    ap.add_argument("--factors", type=int, default=8)
    ap.add_argument("--dtypes", default="bfloat16,float32")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8, help="back-to-back calls of the fused path per run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fm needs a GPU: the torch program on a CPU says nothing about either path")
    s = Session(SessionConf().set("o3s.device", "cuda"))
    results = []
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        for name in a.dtypes.split(","):
            r = measure(s, n, d, a.factors, getattr(torch, name), a.runs, a.reps)
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

"""Tree-model ``transform`` on the fused scoring kernel (ops/tree_predict.py,
csrc/tree_predict.hip) against the per-tree torch walk it replaces
(``O3S_TREE_PREDICT_FUSED=0``: the same tree then runs the old code).

Trees are random ``Tree`` objects built directly (full trees, seeded, no fit); rows are random
on the device.  Per shape, in ONE process, the two paths alternate, three runs each after a
warm-up, host clock around a device synchronise:
  * transform: ``model.transform(df)`` (every output column of the model);
  * kernel:    ``ops.tree_predict.ensemble_predict`` alone (SUM mode), device events;
  * the peak memory each transform adds to the table; an out-of-memory of the old path is
    recorded as such instead of a time.
The kernel's two lower bounds come from the shapes: bytes = (row bytes x groups + 2 x output
bytes x groups) / 8.0 TB/s (every group reads the rows and reads and writes the fp64 sums), and
walk = rows / 64 x trees x depth wave-steps x INSTR_PER_STEP instructions, one instruction per
cycle and SIMD, four SIMDs per CU, at 2.4 GHz.  INSTR_PER_STEP = 18: the staged bf16 loop body
is 36 instructions for the two trees a lane walks at a time (counted in the kernel's assembly).

    python tools/bench_tree_predict.py [--out profiles/tree_predict.json] [--runs 3] [--rows 20000000]
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
from orange3_spark_amd.ml import regression as REG  # noqa: E402
from orange3_spark_amd.models.trees import Ensemble, Tree  # noqa: E402
from orange3_spark_amd.ops import tree_predict as TP  # noqa: E402

CLOCK = 2.4e9
HBM_PEAK = 8.0e12
INSTR_PER_STEP = 18

# name: (model kind, trees, depth, classes, features, row dtype)
SHAPES = OrderedDict([
    ("gbt_100x8_d64_bf16", ("gbt", 100, 8, 2, 64, torch.bfloat16)),
    ("gbt_100x8_d64_f32", ("gbt", 100, 8, 2, 64, torch.float32)),
    ("rf_20x10_c2_d64_bf16", ("rf", 20, 10, 2, 64, torch.bfloat16)),
    ("dt_1x5_d256_bf16", ("dtr", 1, 5, 0, 256, torch.bfloat16)),
])


def full_tree(d, depth, V, rng):
    size = 2 ** (depth + 1)
    feat = -np.ones(size, dtype=np.int64)
    feat[1:2 ** depth] = rng.integers(0, d, 2 ** depth - 1)
    thr = rng.normal(size=size)
    val = rng.random((size, V)) if V > 1 else rng.normal(size=(size, 1))
    if V > 1:
        val /= val.sum(1, keepdims=True)
    cnt = np.ones(size)
    cnt[0] = 0
    return Tree(feat, thr, np.zeros(size, dtype=np.int64), val, np.zeros(size), np.zeros(size), cnt, d)


def make_model(kind, T, depth, classes, d, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "gbt":
        m = CLS.GBTClassificationModel()
        m._ens = Ensemble([full_tree(d, depth, 1, rng) for _ in range(T)], [1.0] + [0.1] * (T - 1), "gbt", 2)
        m.numClasses = 2
    elif kind == "rf":
        m = CLS.RandomForestClassificationModel()
        m._ens = Ensemble([full_tree(d, depth, classes, rng) for _ in range(T)], [1.0] * T, "rf", classes)
        m.numClasses = classes
    else:
        m = REG.DecisionTreeRegressionModel._of_tree(full_tree(d, depth, 1, rng))
    m.numFeatures = d
    return m


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
    """f(), or the allocation failure as text (the old path's fp32 copy may not fit)."""
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
        os.environ.pop("O3S_TREE_PREDICT_FUSED", None)
    else:
        os.environ["O3S_TREE_PREDICT_FUSED"] = "0"
    try:
        out = model.transform(df)
        return [out.column_data(c) for c in out.columns]
    finally:
        os.environ.pop("O3S_TREE_PREDICT_FUSED", None)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/tree_predict.json")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", type=int, default=20_000_000)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--no-old", action="store_true", help="skip the torch walk (LDS budget A/B runs)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sess = Session(SessionConf().set("o3s.device", "cuda"))
    res = {"device": torch.cuda.get_device_name(dev), "cus": cus, "runs": a.runs, "rows": a.rows,
           "lds_budget": TP.PREDICT_LDS_BUDGET, "blocks_per_cu": TP.PREDICT_BLOCKS_PER_CU,
           "instr_per_step": INSTR_PER_STEP, "shapes": {}}
    n = a.rows
    for name in a.shapes.split(","):
        kind, T, depth, classes, d, dtype = SHAPES[name]
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.empty((n, d), dtype=dtype, device=dev)
        for s in range(0, n, 1 << 22):
            X[s:s + (1 << 22)] = torch.randn((min(1 << 22, n - s), d), device=dev, generator=g).to(dtype)
        df = DataFrame(sess, OrderedDict(features=C.VectorColumn(X, d)), n)
        model = make_model(kind, T, depth, classes, d)
        packed = model._packed_for(model._rows(df))
        assert packed is not None, "the gate refused a benchmark shape"
        nbytes = X.numel() * X.element_size()
        _transform(model, df, True)                                       # warm-up of both paths
        old = (lambda f: "skipped") if a.no_old else _guarded
        old(lambda: _transform(model, df, False))
        t = {"transform": [], "transform_old": [], "kernel": []}
        for _ in range(a.runs):
            t["transform"].append(_wall(lambda: _transform(model, df, True)))
            t["transform_old"].append(old(lambda: _wall(lambda: _transform(model, df, False))))
            t["kernel"].append(_events(lambda: TP.ensemble_predict(X, d, packed, TP.SUM)))
        groups = len(packed.groups)
        out_bytes = 8 * n * packed.V
        r = {"table_bytes": nbytes, "trees": T, "depth": depth, "V": packed.V, "groups": groups,
             "node_budget": packed.budget, "staged": TP.staged(X, d, packed)[0]}
        r.update({k + "_ms": _stats(v) for k, v in t.items()})
        r["byte_bound_ms"] = round((nbytes * groups + 2 * out_bytes * groups) / HBM_PEAK * 1e3, 3)
        r["walk_bound_ms"] = round(-(-n // 64) * T * depth * INSTR_PER_STEP / (4 * cus) / CLOCK * 1e3, 3)
        new, was = r["transform_ms"], r["transform_old_ms"]
        r["old_over_new"] = round(was["mean"] / new["mean"], 2) if "mean" in was else None
        r["no_slower"] = bool(new["max"] <= was["min"]) if "mean" in was else None
        r["transform_peak_bytes"] = _peak(lambda: _transform(model, df, True))
        r["transform_old_peak_bytes"] = old(lambda: _peak(lambda: _transform(model, df, False)))
        res["shapes"][name] = r
        print(json.dumps({name: r}), flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        X = df = model = packed = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

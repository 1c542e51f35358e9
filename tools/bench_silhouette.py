"""ClusteringEvaluator on the fused silhouette pass (ops/silhouette.py, csrc/silhouette.hip)
against the fp64 torch path it replaces (``O3S_SILHOUETTE_KERNEL=0``: the same tree then runs
the old code).

Per shape (n x d, k clusters) and row dtype (fp32, bf16), in ONE process, the two paths
alternating, ``--runs`` runs each after a warm-up, all timed with device events:
  * evaluate:  ``ClusteringEvaluator().evaluate`` on a DataFrame of the rows and ids, fused and
               with the switch off.  The torch path is skipped, and the skip recorded, where its
               fp64 copy of the table and its fp64 [n, k] matrices (n (d + 3 k) 8 bytes) do not
               fit the free device memory; an allocation failure is recorded as text;
  * moments:   ``cluster_moments`` (``bin_sums`` on the stored rows) alone;
  * kernel:    ``silhouette_rows`` alone (host packing + the kernel);
  * colstats:  ``ops.glm.glm_colstats`` over the same rows, the streaming pass the byte rate of
               the kernel is compared with (both read the table once);
  * the peak memory either evaluation adds to the table, and the values of both paths.
The kernel's MFMA bound is computed from its step count: per 32 rows and block of 32 means
ns steps x 6 products x 32 cycles, four SIMDs per CU, at 2.4 GHz.

    python tools/bench_silhouette.py [--out profiles/silhouette_pass.json] [--runs 3] [--shapes 4000000x64x8,...]
"""
import argparse
import json
import os
import sys
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orange3_spark_amd import Session, SessionConf  # noqa: E402
from orange3_spark_amd.frame import column as C  # noqa: E402
from orange3_spark_amd.frame.dataframe import DataFrame  # noqa: E402
from orange3_spark_amd.ml.evaluation import ClusteringEvaluator  # noqa: E402
from orange3_spark_amd.ops import glm as GLM  # noqa: E402
from orange3_spark_amd.ops import silhouette as SIL  # noqa: E402

CLOCK = 2.4e9
HBM_PEAK = 8.0e12


def _rows(n, d, k, dtype, dev):
    """(rows, ids): 2 centre + N(0, 1) + 50 per column, ids the generating centre."""
    g = torch.Generator(device=dev).manual_seed(0)
    centres = 2 * torch.randn((k, d), device=dev, generator=g) + 50
    X = torch.empty((n, d), dtype=dtype, device=dev)
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    step = 1 << 22
    for s in range(0, n, step):
        m = min(step, n - s)
        lab = torch.randint(0, k, (m,), device=dev, generator=g)
        X[s:s + m] = (centres[lab] + torch.randn((m, d), device=dev, generator=g)).to(dtype)
        ids[s:s + m] = lab.int()
    return X, ids


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
    """f(), or the allocation failure as text."""
    try:
        return f()
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return f"out of memory: {str(e).splitlines()[0]}"


def _stats(v):
    nums = [x for x in v if not isinstance(x, str)]
    if not v or len(nums) != len(v):
        return {"runs": v}
    return {"runs": [round(x, 3) for x in v], "mean": round(sum(v) / len(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3)}


def _faster(new, old):
    """The rule of doc/performance.md: the new path's slowest run beats the old path's fastest and
    the means differ by at least three times the old path's spread."""
    if "mean" not in new or "mean" not in old:
        return None
    return bool(new["max"] < old["min"] and old["mean"] - new["mean"] >= 3 * (old["max"] - old["min"]))


def _mfma_bound_ms(n, d, k, cus):
    ns = (d + 15) // 16
    tiles = (n + 31) // 32
    return -(-tiles // (4 * cus)) * ((k + 31) // 32) * ns * 6 * 32 / CLOCK * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/silhouette_pass.json")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--shapes", default="4000000x64x8,20000000x64x16,20000000x128x256,20000000x128x1024")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_silhouette needs a GPU: a time taken elsewhere says nothing about it")
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sess = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    res = {"device": torch.cuda.get_device_name(dev), "cus": cus, "runs": a.runs, "shapes": {}}
    ev = ClusteringEvaluator()
    for shape in a.shapes.split(","):
        n, d, k = (int(v) for v in shape.split("x"))
        for dtype in (torch.float32, torch.bfloat16):
            X, ids = _rows(n, d, k, dtype, dev)
            df = DataFrame(sess, OrderedDict(features=C.VectorColumn(X, d), prediction=C.NumericColumn(ids)), n)
            nbytes = X.numel() * X.element_size()
            r = {"table_bytes": nbytes, "k": k}

            def evaluate(fused):
                os.environ["O3S_SILHOUETTE_KERNEL"] = "1" if fused else "0"
                try:
                    return ev.evaluate(df)
                finally:
                    os.environ.pop("O3S_SILHOUETTE_KERNEL", None)

            need = n * (d + 3 * k) * 8
            free = torch.cuda.mem_get_info(dev)[0]
            old = need < free
            if not old:
                r["evaluate_old_skipped"] = (f"the torch path needs about {need / 1e9:.0f} GB for its fp64 copy and "
                                             f"[n, k] matrices, {free / 1e9:.0f} GB are free")
            r["value"] = evaluate(True)                                   # also the warm-ups
            if old:
                r["value_old"] = _guarded(lambda: evaluate(False))
            Y, N, Psi = SIL.cluster_moments(X, ids, k, None, d)
            SIL.silhouette_rows(X, d, ids, Y, N, Psi)
            GLM.glm_colstats(X)
            t = {key: [] for key in ("evaluate", "evaluate_old", "moments", "kernel", "colstats")}
            for _ in range(a.runs):
                t["evaluate"].append(_events(lambda: evaluate(True)))
                if old:
                    t["evaluate_old"].append(_guarded(lambda: _events(lambda: evaluate(False))))
                t["moments"].append(_events(lambda: SIL.cluster_moments(X, ids, k, None, d)))
                t["kernel"].append(_events(lambda: SIL.silhouette_rows(X, d, ids, Y, N, Psi)))
                t["colstats"].append(_events(lambda: GLM.glm_colstats(X)))
            r.update({key + "_ms": _stats(v) for key, v in t.items()})
            r["kernel_mfma_bound_ms"] = round(_mfma_bound_ms(n, d, k, cus), 3)
            r["kernel_byte_bound_ms"] = round((nbytes + 8 * n) / HBM_PEAK * 1e3, 3)
            r["kernel_table_GBps"] = round(nbytes / r["kernel_ms"]["mean"] / 1e6, 1)
            r["colstats_table_GBps"] = round(nbytes / r["colstats_ms"]["mean"] / 1e6, 1)
            r["evaluate_faster"] = _faster(r["evaluate_ms"], r["evaluate_old_ms"])
            r["evaluate_peak_bytes"] = _peak(lambda: evaluate(True))
            if old:
                r["evaluate_old_peak_bytes"] = _guarded(lambda: _peak(lambda: evaluate(False)))
            res["shapes"][f"{n}x{d}_k{k}_{'f32' if dtype == torch.float32 else 'bf16'}"] = r
            print(json.dumps({shape: r}), flush=True)
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
            X = ids = df = Y = N = Psi = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

"""GaussianMixture on the fused E-step and Gram passes (ops/gmm.py, csrc/gmm.hip) against the
chunked fp64 path it replaces (``O3S_GMM_FUSED=0``: the same tree then runs the old code).

Per shape (n x d, K components) and row dtype (fp32, bf16), in ONE process, the two paths
alternating, three runs each after a warm-up:
  * estep:  ``ops.gmm.estep`` on the stored rows (host preparation + kernel, device events),
            and the old path's E-step (``gmm_log_prob`` + softmax over 262 144-row chunks of an
            fp64 copy made beforehand);
  * iter:   one EM iteration (E + M) = (fit with maxIter 5 - fit with maxIter 1) / 4 of
            ``models.clustering_extra.fit_gmm``, host clock around a device synchronise;
  * fit:    ``GaussianMixture(k, maxIter=10, tol=0).fit`` on a DataFrame of the rows;
  * the peak memory either fit adds to the table.
Where the old path cannot allocate its fp64 copy the error is recorded instead of a time.  The
E-step's MFMA bound is computed from the kernel's step count: per 32 rows and component
sum_cb min(2 cb + 2, ns) steps x 6 products x 32 cycles, four SIMDs per CU, at 2.4 GHz.

    python tools/bench_gmm.py [--out profiles/gmm_pass.json] [--runs 3] [--shapes 4000000x64x8,...]
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from orange3_spark_amd import Session, SessionConf  # noqa: E402
from orange3_spark_amd.frame import column as C  # noqa: E402
from orange3_spark_amd.frame.dataframe import DataFrame  # noqa: E402
from orange3_spark_amd.ml import clustering as CL  # noqa: E402
from orange3_spark_amd.models import clustering_extra as CE  # noqa: E402
from orange3_spark_amd.ops import gmm as GM  # noqa: E402
from orange3_spark_amd.parallel.comm import LocalComm  # noqa: E402

CLOCK = 2.4e9
HBM_PEAK = 8.0e12


def _rows(n, d, k, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    scales = torch.rand(d, device=dev, generator=g) * 19.5 + 0.5
    offsets = torch.rand(d, device=dev, generator=g) * 100 - 50
    centres = 0.45 * torch.randn((k, d), device=dev, generator=g)
    X = torch.empty((n, d), dtype=dtype, device=dev)
    step = 1 << 22
    for s in range(0, n, step):
        m = min(step, n - s)
        lab = torch.randint(0, k, (m,), device=dev, generator=g)
        X[s:s + m] = ((centres[lab] + torch.randn((m, d), device=dev, generator=g)) * scales + offsets).to(dtype)
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
    """f(), or the allocation failure as text (the old path's fp64 copy may not fit)."""
    try:
        return f()
    except torch.cuda.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return f"out of memory: {str(e).splitlines()[0]}"


def _old_estep(Xd, weights, means, covs, chunk=1 << 18):
    logw = torch.log(weights)
    for a in range(0, Xd.shape[0], chunk):
        lp = CE.gmm_log_prob(Xd[a:a + chunk], means, covs, logw)
        torch.exp(lp - torch.logsumexp(lp, dim=1)[:, None])


def _mfma_bound_ms(n, d, k, cus):
    ns = (d + 15) // 16
    steps = sum(min(2 * cb + 2, ns) for cb in range((ns + 1) // 2))
    tiles = (n + 31) // 32
    return -(-tiles // (4 * cus)) * k * steps * 6 * 32 / CLOCK * 1e3


def _stats(v):
    nums = [x for x in v if not isinstance(x, str)]
    if len(nums) != len(v):
        return {"runs": v}
    return {"runs": [round(x, 3) for x in v], "mean": round(sum(v) / len(v), 3), "min": round(min(v), 3),
            "max": round(max(v), 3)}


def _faster(new, old):
    """The rule of doc/performance.md: the new path's slowest run beats the old path's fastest and
    the means differ by at least three times the old path's spread."""
    if "mean" not in new or "mean" not in old:
        return None
    return bool(new["max"] < old["min"] and old["mean"] - new["mean"] >= 3 * (old["max"] - old["min"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/gmm_pass.json")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--shapes", default="4000000x64x8,20000000x64x8,4000000x128x4")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    sess = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    comm = LocalComm(dev)
    res = {"device": torch.cuda.get_device_name(dev), "cus": cus, "runs": a.runs, "shapes": {}}
    for shape in a.shapes.split(","):
        n, d, k = (int(v) for v in shape.split("x"))
        for dtype in (torch.float32, torch.bfloat16):
            X = _rows(n, d, k, dtype, dev)
            df = DataFrame(sess, OrderedDict(features=C.VectorColumn(X, d)), n)
            nbytes = X.numel() * X.element_size()

            def engine(iters, fused):
                if fused:
                    return CE.fit_gmm(comm, X, k, iters, 0.0, 1, d=d)
                return CE.fit_gmm(comm, X, k, iters, 0.0, 1)

            def fit(fused):
                GM.FUSED = int(fused)
                try:
                    return CL.GaussianMixture(k=k, maxIter=10, tol=0.0, seed=1).fit(df)
                finally:
                    GM.FUSED = 1

            model = engine(3, True)                                   # also the warm-up of the fused passes
            wts, mu, cov = (torch.from_numpy(v).to(dev) for v in (model.weights, model.means, model.covs))
            _guarded(lambda: engine(1, False))
            t = {key: [] for key in ("estep", "estep_old", "iter", "iter_old", "fit", "fit_old")}
            for _ in range(a.runs):
                t["estep"].append(_events(lambda: GM.estep(X, d, wts, mu, cov)))

                def old_estep():
                    Xd = X.to(torch.float64)
                    return _events(lambda: _old_estep(Xd, wts, mu, cov))
                t["estep_old"].append(_guarded(old_estep))
                t["iter"].append((_wall(lambda: engine(5, True)) - _wall(lambda: engine(1, True))) / 4)
                t["iter_old"].append(_guarded(
                    lambda: (_wall(lambda: engine(5, False)) - _wall(lambda: engine(1, False))) / 4))
                t["fit"].append(_wall(lambda: fit(True)))
                t["fit_old"].append(_guarded(lambda: _wall(lambda: fit(False))))
            r = {"table_bytes": nbytes, "k": k}
            r.update({key + "_ms": _stats(v) for key, v in t.items()})
            r["estep_mfma_bound_ms"] = round(_mfma_bound_ms(n, d, k, cus), 3)
            r["estep_byte_bound_ms"] = round((nbytes + 4 * n * (k + 1)) / HBM_PEAK * 1e3, 3)
            for key in ("estep", "iter", "fit"):
                r[key + "_faster"] = _faster(r[key + "_ms"], r[key + "_old_ms"])
            r["fit_peak_bytes"] = _peak(lambda: fit(True))
            r["fit_old_peak_bytes"] = _guarded(lambda: _peak(lambda: fit(False)))
            res["shapes"][f"{n}x{d}_k{k}_{'f32' if dtype == torch.float32 else 'bf16'}"] = r
            print(json.dumps({shape: r}), flush=True)
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
            X = df = None
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

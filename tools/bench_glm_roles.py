"""The mixed GLM gradient pass by role on one GPU: the resident rows alone, the lineage rows
alone and both in one launch (``ops.glm.glm_grad_mixed``), each timed over ``--iters`` passes
after a warm-up pass.  ``--staged 0/1/2`` selects ``ops.glm.MIX_STAGED`` (resident tiles staged
through a per-wave LDS slot; 2 stages a single role too); ``--only`` runs one of the three, for
a profiler or counter run.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orange3_spark_amd.ops import glm as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=125_000_000)
    ap.add_argument("--lin", type=int, default=125_000_000)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--staged", type=int, default=None)
    ap.add_argument("--only", choices=["resident", "lineage", "mixed"], default=None)
    a = ap.parse_args()
    if a.staged is not None:
        G.MIX_STAGED = a.staged
    dev = torch.device("cuda", 0)
    X, yr = G.synth_glm(a.res, a.d, seed=1, device=dev)
    ld = X.shape[1]
    yl = (torch.rand(a.lin, device=dev) < 0.5).float()
    y = torch.cat([yr, yl])
    ws = G.GlmWorkspace(dev, ld)
    coef = torch.full((ld,), 0.01, device=dev)
    roles = {
        "resident": lambda: G.glm_grad_mixed(X, yr, None, 0, a.d, 1, a.res, coef, 0.0, 0, ws),
        "lineage": lambda: G.glm_grad_mixed(X[:0], yl, None, a.lin, a.d, 1, a.res, coef, 0.0, 0, ws),
        "mixed": lambda: G.glm_grad_mixed(X, y, None, a.lin, a.d, 1, a.res, coef, 0.0, 0, ws),
    }
    out = {"res": a.res, "lin": a.lin, "d": a.d, "iters": a.iters, "staged": getattr(G, "MIX_STAGED", None),
           "splits": G.mix_splits(a.res + a.lin)}
    for name, fn in roles.items():
        if a.only and name != a.only:
            continue
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        out[name + "_ms"] = (time.perf_counter() - t) / a.iters * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()

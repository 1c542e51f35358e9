"""The mixed GLM gradient pass by role on one GPU: the resident rows alone, the lineage rows
alone and both in one launch (``ops.glm.glm_grad_mixed``), each timed over ``--iters`` passes
after a warm-up pass.  ``--staged 0/1/2`` selects ``ops.glm.MIX_STAGED`` (resident tiles staged
through a per-wave LDS slot; 2 stages a single role too); ``--persist 0/1/2`` selects
``ops.glm.MIX_PERSIST`` (the ticket-scheduled persistent form of the staged pass); ``--only``
runs one of the three, for a profiler or counter run.
``--label-bits 0/1`` selects ``ops.glm.MIX_LABEL_BITS`` (the persistent pass reads its 0/1 labels
from bit planes).
``--grid G [G ...]`` and ``--item-tiles T [T ...]`` time the mixed pass once per value on the
same table (a static-grid sweep of the sliced launches, an item-size sweep of the persistent
one); the per-value times are reported under ``sweep``.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from orange3_spark_amd.ops import glm as G  # noqa: E402


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=125_000_000)
    ap.add_argument("--lin", type=int, default=125_000_000)
    ap.add_argument("--d", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--staged", type=int, default=None)
    ap.add_argument("--persist", type=int, default=None)
    ap.add_argument("--grid", type=int, nargs="*", default=None)
    ap.add_argument("--item-tiles", type=int, nargs="*", default=None)
    ap.add_argument("--label-bits", type=int, choices=[0, 1], default=None)
    ap.add_argument("--only", choices=["resident", "lineage", "mixed"], default=None)
    a = ap.parse_args()
    if a.staged is not None:
        G.MIX_STAGED = a.staged
    if a.persist is not None:
        G.MIX_PERSIST = a.persist
    if a.label_bits is not None:
        G.MIX_LABEL_BITS = a.label_bits
    dev = torch.device("cuda", 0)
    X, yr = G.synth_glm(a.res, a.d, seed=1, device=dev)
    ld = X.shape[1]
    yl = (torch.rand(a.lin, device=dev) < 0.5).float()
    y = torch.cat([yr, yl])
    grids = a.grid or [None]
    ws = G.GlmWorkspace(dev, ld, grid=grids[0])
    coef = torch.full((ld,), 0.01, device=dev)
    if G.MIX_LABEL_BITS:
        ws.pack_labels(y, a.res, a.lin)     # the mixed pass's label column, as a fit packs it
    roles = {
        "resident": lambda: G.glm_grad_mixed(X, yr, None, 0, a.d, 1, a.res, coef, 0.0, 0, ws),
        "lineage": lambda: G.glm_grad_mixed(X[:0], yl, None, a.lin, a.d, 1, a.res, coef, 0.0, 0, ws),
        "mixed": lambda: G.glm_grad_mixed(X, y, None, a.lin, a.d, 1, a.res, coef, 0.0, 0, ws),
    }
    out = {"res": a.res, "lin": a.lin, "d": a.d, "iters": a.iters, "staged": getattr(G, "MIX_STAGED", None),
           "persist": getattr(G, "MIX_PERSIST", None), "label_bits": G.MIX_LABEL_BITS, "grid": ws.grid,
           "splits": G.mix_splits(a.res + a.lin)}
    for name, fn in roles.items():
        if a.only and name != a.only:
            continue
        out[name + "_ms"] = _time(fn, a.iters)
        if name == "mixed":
            out["mixed_used_label_bits"] = ws.used_label_bits
    if len(grids) > 1 or a.item_tiles:
        sweep = []
        for grid in grids:
            w = G.GlmWorkspace(dev, ld, grid=grid)
            for tiles in a.item_tiles or [None]:
                if tiles is not None:
                    G.MIX_ITEM_TILES = tiles
                ms = _time(lambda: G.glm_grad_mixed(X, y, None, a.lin, a.d, 1, a.res, coef, 0.0, 0, w), a.iters)
                sweep.append({"grid": w.grid, "item_tiles": tiles, "mixed_ms": ms})
        out["sweep"] = sweep
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""The packed tree ensemble of ``ops/tree_predict.py`` on the host: the threshold rounding
rule, ``pack_ensemble`` + ``ensemble_walk_torch`` against the per-tree ``Tree`` walk, the
kernel gate, validation, and that the per-model cache never travels in a pickle.

The ensembles built here are shared with ``test_tree_predict_kernel.py``."""
import functools
import pickle

import numpy as np
import pytest
import torch

from orange3_spark_amd.models.trees import Ensemble, Tree
from orange3_spark_amd.ops import tree_predict as TP

TINY_BUDGET = 8 * 2047 + 64           # one full depth-10 tree and little else: 40 trees split into many groups


# ----------------------------------------------------------------------------- trees
def make_tree(d, depth, V, rng, shape="random", thresholds=None):
    """Heap-ordered ``Tree`` over ``d`` features.  shape: "random" (early leaves with
    probability 0.3 below the root), "full", "chain" (a left chain of ``depth`` splits), "root"
    (a single leaf), "corners" (depth 2: the root splits on feature d - 1, node 2 on feature 0).
    ``thresholds``: the values split thresholds are drawn from."""
    size = 2 ** (depth + 1)
    feat = -np.ones(size, dtype=np.int64)
    thr = np.zeros(size)
    cnt = np.zeros(size)
    val = rng.random((size, V)) if V > 1 else rng.normal(size=(size, 1))
    if V > 1:
        val /= val.sum(1, keepdims=True)
    pick = (lambda: rng.choice(thresholds)) if thresholds is not None else (lambda: rng.normal())

    def split(nid):
        feat[nid] = rng.integers(0, d)
        thr[nid] = pick()
        cnt[2 * nid] = cnt[2 * nid + 1] = 1

    cnt[1] = 1
    if shape == "chain":
        nid = 1
        for _ in range(depth):
            split(nid)
            nid *= 2
    elif shape == "corners":
        split(1), split(2)
        feat[1], feat[2] = d - 1, 0
    elif shape != "root":
        for nid in range(1, 2 ** depth):
            if cnt[nid] and (shape == "full" or nid == 1 or rng.random() > 0.3):
                split(nid)
    return Tree(feat, thr, np.zeros(size, dtype=np.int64), val, np.zeros(size), np.zeros(size), cnt, d)


THRESHOLDS = np.array([-1.5, -0.25, 0.0, 0.5, 1.0, 3.0])         # exact in bf16
# the rows' values: every threshold (ties go left), values between them, and the specials
ROW_VALUES = np.concatenate([THRESHOLDS, [-2.0, -0.5, 0.25, 0.75, 2.0, 4.0, -0.0, np.nan, np.inf, -np.inf]])


@functools.lru_cache(maxsize=None)
def ensemble(name: str, d: int, V: int):
    """(trees, weights, kind, num_classes) of the named ensemble over ``d`` features:
    "one" (a root-only tree), "three" (depth 1, a depth-14 left chain, the corners tree),
    "forty" (40 trees: a full depth-10 tree, random trees of depth 1 - 9 with early leaves)."""
    rng = np.random.default_rng({"one": 1, "three": 3, "forty": 40}[name] + 1000 * d + V)
    mk = functools.partial(make_tree, d, V=V, rng=rng, thresholds=THRESHOLDS)
    if name == "one":
        trees = [mk(0, shape="root")]
    elif name == "three":
        trees = [mk(1, shape="full"), mk(14, shape="chain"), mk(2, shape="corners")]
    else:
        trees = [mk(1 + i % 9) for i in range(38)]
        trees[1:1] = [mk(2, shape="corners")]
        trees[20:20] = [mk(10, shape="full")]              # fills a group of TINY_BUDGET almost alone
    weights = [1.0] + [float(w) for w in rng.uniform(0.05, 0.5, len(trees) - 1)]
    return trees, weights, ("gbt" if V == 1 else "rf"), (0 if V == 1 else V)


def rows(n: int, d: int, seed: int = 0) -> torch.Tensor:
    """fp32 [n, d] rows drawn from ROW_VALUES (all exact in bf16); column 0 cycles through
    NaN, +inf, -inf and -0.0 among ordinary values."""
    rng = np.random.default_rng(seed)
    X = ROW_VALUES[:12][rng.integers(0, 12, (n, d))]
    X[:, 0] = ROW_VALUES[rng.integers(0, len(ROW_VALUES), n)]
    return torch.from_numpy(X.astype(np.float32))


def sequential_sum(trees, weights, kind, k, X64):
    """zeros, then one fp64 add per tree in order (what SUM mode must equal bit for bit)."""
    V = k if (kind != "gbt" and k) else 1
    out = torch.zeros((X64.shape[0], V), dtype=torch.float64)
    for t, w in zip(trees, weights):
        out += (1.0 if V > 1 else w) * t.predict_value(X64)[:, :V]
    return out


# ----------------------------------------------------------------------------- rounding
def _adversarial_pairs():
    rng = np.random.default_rng(7)
    mag = 10.0 ** rng.uniform(-40, 38, 1500)
    x = (mag * rng.choice([-1.0, 1.0], 1500)).astype(np.float32)
    x = np.concatenate([x, np.float32([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4028235e38,
                                       -3.4028235e38, 1.17549435e-38, 1.0, -1.0])])
    x64 = x.astype(np.float64)
    fin = x64[np.isfinite(x64)]
    nb = np.concatenate([np.nextafter(fin, np.inf), np.nextafter(fin, -np.inf), fin])
    with np.errstate(over="ignore"):
        up = np.nextafter(fin.astype(np.float32), np.float32(np.inf)).astype(np.float64)
    mid = (fin[np.isfinite(up)] + up[np.isfinite(up)]) / 2             # fp32 midpoints: ties of round-to-nearest
    t = np.concatenate([nb, mid, rng.normal(size=2000) * 10.0 ** rng.uniform(-40, 38, 2000),
                        [1e300, -1e300, 3.5e38, -3.5e38, 1e-320, -1e-320, 0.0, -0.0, np.inf, -np.inf, np.nan]])
    return x, t


def test_threshold_rounding_rule_matches_fp64_compare():
    x, t = _adversarial_pairs()
    assert len(x) >= 1500 and len(t) >= 6000
    t32 = TP.round_down_f32(t)
    with np.errstate(invalid="ignore"):
        got = x[:, None] <= t32[None, :]
        want = x.astype(np.float64)[:, None] <= t[None, :]
    assert np.array_equal(got, want)
    fin = np.isfinite(t) & (np.abs(t) <= 3.4028234663852886e38)
    assert np.all(t32[fin].astype(np.float64) <= t[fin])              # toward -inf, never above
    assert TP.round_down_f32(1e300) == np.float32(3.4028235e38) and TP.round_down_f32(-1e300) == -np.inf
    assert np.isnan(TP.round_down_f32(np.nan)) and TP.round_down_f32(np.inf) == np.inf
    # round-to-nearest would be wrong: 0.1 rounds up in fp32
    assert float(np.float32(0.1)) > 0.1 and float(TP.round_down_f32(0.1)) < 0.1


# ----------------------------------------------------------------------------- pack + walk
@pytest.mark.parametrize("V", [1, 2, 3, 16])
@pytest.mark.parametrize("name", ["one", "three", "forty"])
def test_packed_walk_matches_tree_walk(name, V):
    d = 7
    trees, weights, kind, k = ensemble(name, d, V)
    budget = TINY_BUDGET if name == "forty" else None
    p = TP.pack_ensemble(trees, weights, kind, k, budget=budget, num_features=d)
    if name == "forty":
        assert len(p.groups) >= 3
    assert p.V == V and p.num_trees == len(trees) and p.nodes.dtype == np.uint32 and p.nodes.shape[1] == 2
    assert p.max_depth == max(t.depth for t in trees)
    X = rows(777, d)
    X64 = X.double()
    got = TP.ensemble_walk_torch(p, X64, TP.SUM)
    assert torch.equal(got, sequential_sum(trees, weights, kind, k, X64))
    leaves = TP.ensemble_walk_torch(p, X, TP.LEAF)
    assert torch.equal(leaves, torch.stack([t.leaf_index(X64) for t in trees], 1).double())
    # the same bits under any grouping
    one_group = TP.pack_ensemble(trees, weights, kind, k, budget=160 * 1024, num_features=d)
    assert torch.equal(TP.ensemble_walk_torch(one_group, X64, TP.SUM), got)


def test_packed_table_is_compact_for_deep_unbalanced_trees():
    trees, weights, kind, k = ensemble("three", 7, 1)
    p = TP.pack_ensemble(trees, weights, kind, k, num_features=7)
    assert len(p.nodes) == 3 + (2 * 14 + 1) + 5                        # not 2^15 for the chain
    feat, left = p.nodes[:, 1] & 0xFFFF, p.nodes[:, 1] >> 16
    inner = feat != TP.LEAF_CODE
    assert np.all(left[inner] > np.nonzero(inner)[0])                  # children after their parent


# ----------------------------------------------------------------------------- gate, validation
def test_gate_refusals(monkeypatch):
    ok = dict(is_cuda=True, dtype=torch.bfloat16, col_stride=1, d=64, V=2, max_tree_bytes=4096)
    assert TP.gate_reason(**ok) is None
    assert TP.gate_reason(**{**ok, "dtype": torch.float32}) is None
    assert TP.gate_reason(**{**ok, "V": 16, "d": 65534}) is None
    assert TP.gate_reason(**{**ok, "V": 17}) is not None
    assert TP.gate_reason(**{**ok, "d": 65535}) is not None
    assert TP.gate_reason(**{**ok, "max_tree_bytes": TP.PREDICT_LDS_BUDGET + 8}) is not None
    assert TP.gate_reason(**{**ok, "is_cuda": False}) is not None
    assert TP.gate_reason(**{**ok, "dtype": torch.float64}) is not None
    assert TP.gate_reason(**{**ok, "col_stride": 2}) is not None
    assert not TP.predict_kernel_ok(torch.zeros(4, 64), 64, 2, 4096)   # a host tensor
    monkeypatch.setenv("O3S_TREE_PREDICT_FUSED", "0")
    assert TP.gate_reason(**ok) == "O3S_TREE_PREDICT_FUSED=0"


def test_pack_rejects_tree_larger_than_budget_and_missing_child():
    rng = np.random.default_rng(0)
    full = make_tree(4, 10, 1, rng, shape="full")
    with pytest.raises(TP.PackError):
        TP.pack_ensemble([full], [1.0], "gbt", 0, budget=8 * 2046, num_features=4)
    t = make_tree(4, 3, 1, rng, shape="full")
    t.count[2 * 2 + 1] = 0                                             # node 2 keeps only its left child
    with pytest.raises(TP.PackError):
        TP.pack_ensemble([t], [1.0], "gbt", 0, num_features=4)
    bad = make_tree(4, 2, 1, rng, shape="full")
    bad.feature[1] = 4                                                 # feature == number of features
    with pytest.raises(TP.PackError):
        TP.pack_ensemble([bad], [1.0], "gbt", 0, num_features=4)


def test_validate_packed_rejects_corrupt_tables():
    trees, weights, kind, k = ensemble("three", 7, 1)
    p = TP.pack_ensemble(trees, weights, kind, k, num_features=7)
    TP.validate_packed(p)
    q = pickle.loads(pickle.dumps(p))
    q.nodes[0, 1] = (q.nodes[0, 1] & 0xFFFF)                           # the root's left child = itself
    with pytest.raises(TP.PackError):
        TP.validate_packed(q)
    q = pickle.loads(pickle.dumps(p))
    leaf = np.nonzero((q.nodes[:, 1] & 0xFFFF) == TP.LEAF_CODE)[0][0]
    q.nodes[leaf, 0] = 10 ** 6                                         # a leaf row outside the value table
    with pytest.raises(TP.PackError):
        TP.validate_packed(q)


def test_non_unit_column_stride_is_refused_on_the_host_too():
    trees, weights, kind, k = ensemble("three", 7, 1)
    p = TP.pack_ensemble(trees, weights, kind, k, num_features=7)
    X = rows(10, 14)
    with pytest.raises(ValueError):
        TP.ensemble_predict(X[:, ::2], 7, p, TP.SUM)
    assert torch.equal(TP.ensemble_predict(X[:, :7], 7, p, TP.SUM), TP.ensemble_walk_torch(p, X[:, :7], TP.SUM))


# ----------------------------------------------------------------------------- model cache
def test_model_cache_is_not_pickled_or_copied():
    from orange3_spark_amd.ml.classification import GBTClassificationModel
    trees, weights, kind, _ = ensemble("three", 7, 1)
    m = GBTClassificationModel()
    m._ens, m.numFeatures = Ensemble(trees, weights, "gbt", 2), 7
    p = TP.pack_ensemble(trees, weights, "gbt", 2, num_features=7)
    m.__dict__["_tp_cache"] = (m._ens, len(trees), {"tree_bytes": 8, TP.PREDICT_LDS_BUDGET: p})
    blob = pickle.dumps(m)
    assert b"_tp_cache" not in blob and b"PackedEnsemble" not in blob
    m2 = pickle.loads(blob)
    assert "_tp_cache" not in m2.__dict__ and m2.getNumTrees == 3
    assert "_tp_cache" not in m.copy().__dict__
    # a packed table itself drops its device copies
    p._dev["cuda:0"] = ("device tensors",)
    assert pickle.loads(pickle.dumps(p))._dev == {}

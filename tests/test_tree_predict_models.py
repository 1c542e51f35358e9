"""Tree models' ``transform`` on the fused scoring kernel against the per-tree torch walk
(``O3S_TREE_PREDICT_FUSED=0``): the same columns, bit for bit where the walk's own sum order is
fixed; the memory the fused path adds; and the CPU, which keeps the torch walk."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.frame import column as C
from orange3_spark_amd.frame.dataframe import DataFrame
from orange3_spark_amd.ml import classification as CLS
from orange3_spark_amd.ml import regression as REG
from orange3_spark_amd.models.trees import Ensemble
from orange3_spark_amd.ops import tree_predict as TP
from test_tree_predict_host import make_tree

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "spark_models")


def _estimators(classes):
    kw = dict(seed=3, leafCol="leaf")
    est = [CLS.DecisionTreeClassifier(**kw), CLS.RandomForestClassifier(numTrees=5, **kw),
           REG.DecisionTreeRegressor(**kw), REG.RandomForestRegressor(numTrees=5, **kw),
           REG.GBTRegressor(maxIter=5, **kw)]
    if classes == 2:                                       # GBTClassifier is binary
        est.append(CLS.GBTClassifier(maxIter=5, **kw))
    return est


def _three_class(df):
    """The synthetic frame with a third class: label + [feature 0 > 0.3]."""
    X = df.column_data("features").dense().float()
    y = df.column_data("label").data.float() + (X[:, 0] > 0.3).float()
    return df.withColumnData("label", C.NumericColumn(y))


def _columns(out, names):
    return {k: out.column_data(k).data for k in names if k in out.columns}


def _compare(model, df, monkeypatch):
    """transform with the kernel and with the switch off; the comparison the models owe."""
    names = ("prediction", "rawPrediction", "probability", "leaf")
    monkeypatch.delenv("O3S_TREE_PREDICT_FUSED", raising=False)
    fused = _columns(model.transform(df), names)
    monkeypatch.setenv("O3S_TREE_PREDICT_FUSED", "0")
    walk = _columns(model.transform(df), names)
    monkeypatch.delenv("O3S_TREE_PREDICT_FUSED", raising=False)
    assert set(fused) == set(walk) and "prediction" in fused and "leaf" in fused
    ens = model._ens
    exact = ens.kind == "gbt" or not ens.num_classes       # GBT and every regressor: a fixed sum order
    T = len(ens.trees)
    for k in fused:
        a, b = fused[k].double(), walk[k].double()
        assert a.shape == b.shape, k
        if exact or k in ("prediction", "leaf"):
            assert torch.equal(a, b), k
        elif k == "rawPrediction":
            # torch.stack(...).sum(0) promises no order: T distributions in [0, 1], both sums
            # within T * 2^-53 * T of the exact one
            assert float((a - b).abs().max()) <= T * T * 2.0 ** -52, k
        else:
            # probability = raw / s, s = the row sum = T up to V * eps, eps the bound above:
            # |a/sa - b/sb| <= eps / T + V * eps / T = (1 + V) * T * 2^-52, plus the division's rounding
            assert float((a - b).abs().max()) <= (2 + ens.num_classes) * T * 2.0 ** -52, k
    return fused


def _check_session(s, monkeypatch, fused_expected):
    df2 = s.synthetic.trees(20_000, 16)
    for classes, df in ((2, df2), (3, _three_class(df2))):
        for est in _estimators(classes):
            m = est.fit(df)
            _compare(m, df, monkeypatch)
            X = m._rows(df)
            assert (m._packed_for(X) is not None) == fused_expected, type(m).__name__


@pytest.mark.gpu
def test_fused_transform_equals_torch_walk_bf16(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    assert s.synthetic.trees(64, 16).column_data("features").data.dtype == torch.bfloat16
    _check_session(s, monkeypatch, True)


@pytest.mark.gpu
def test_fused_transform_equals_torch_walk_fp32(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    df = s.synthetic.trees(20_000, 16)
    assert df.column_data("features").data.dtype == torch.float32
    for est in (CLS.GBTClassifier(maxIter=5, seed=3, leafCol="leaf"),
                CLS.RandomForestClassifier(numTrees=5, seed=3, leafCol="leaf"),
                REG.RandomForestRegressor(numTrees=5, seed=3, leafCol="leaf")):
        m = est.fit(df)
        _compare(m, df, monkeypatch)
        assert m._packed_for(m._rows(df)) is not None


@pytest.mark.gpu
def test_fused_transform_of_a_loaded_spark_model(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    m = CLS.GBTClassificationModel.load(os.path.join(FIX, "gbt_classifier")).copy()
    m._set(leafCol="leaf")
    g = torch.Generator().manual_seed(0)
    X = torch.rand((5000, 2), generator=g) * torch.tensor([1.0, 3.0])
    X[:4] = torch.tensor([[0.5, 1.0], [0.2, 0.0], [0.9, 3.0], [0.7, 0.5]])          # the thresholds themselves
    for dtype in (torch.bfloat16, torch.float32):
        df = DataFrame(s, OrderedDict(features=C.VectorColumn(X.to(dtype).to(s.device))), len(X))
        out = _compare(m, df, monkeypatch)
        raw = out["rawPrediction"][:4, 1].cpu().numpy()
        np.testing.assert_allclose(raw, [-0.6 + 0.02, -0.6 + 0.02, 0.8 - 0.03, 0.8 + 0.02], rtol=0, atol=1e-12)
        assert m._packed_for(m._rows(df)) is not None


@pytest.mark.gpu
def test_fused_transform_makes_no_fp32_copy_of_the_table(gpu):
    """500 000 x 256 bf16 rows (256 MB) scored by a 5-tree depth-4 GBT: the transform's peak
    allocation above the level before the call stays under the table's own bytes (outputs and
    epilogue temporaries are ~50 MB; the torch walk's ``X.float()`` alone adds 512 MB)."""
    s = Session(SessionConf().set("o3s.device", "cuda"))
    n, d = 500_000, 256
    rng = np.random.default_rng(0)
    trees = [make_tree(d, 4, 1, rng) for _ in range(5)]
    m = REG.GBTRegressionModel()
    m._ens, m.numFeatures = Ensemble(trees, [1.0, 0.1, 0.1, 0.1, 0.1], "gbt", 0), d
    X = torch.randn((n, d), device=s.device).to(torch.bfloat16)
    df = DataFrame(s, OrderedDict(features=C.VectorColumn(X)), n)
    table = X.element_size() * X.numel()
    m.transform(DataFrame(s, OrderedDict(features=C.VectorColumn(X[:64])), 64))      # tables packed and uploaded
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(s.device)
    before = torch.cuda.memory_allocated(s.device)
    out = m.transform(df)
    torch.cuda.synchronize()
    added = torch.cuda.max_memory_allocated(s.device) - before
    print(f"table {table / 2**20:.0f} MB, transform peak above baseline {added / 2**20:.1f} MB")
    assert added < table
    pred = out.column_data("prediction").data
    want = TP.ensemble_walk_torch(TP.pack_ensemble(trees, m._ens.weights, "gbt", 0, num_features=d),
                                  X[:4096].cpu().double())[:, 0]
    assert torch.equal(pred[:4096].cpu().double(), want)


def test_cpu_transform_is_unchanged_by_the_switch(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cpu"))
    df2 = s.synthetic.trees(3000, 8)
    for classes, df in ((2, df2), (3, _three_class(df2))):
        for est in _estimators(classes):
            m = est.fit(df)
            assert m._packed_for(m._rows(df)) is None                  # the gate keeps host rows on the torch walk
            _compare(m, df, monkeypatch)

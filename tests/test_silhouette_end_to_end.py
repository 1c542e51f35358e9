"""``ClusteringEvaluator`` on the fused silhouette pass (``ops/silhouette.py``) against the fp64
torch path of the same GPU session (``O3S_SILHOUETTE_KERNEL=0``).

The value is a weighted mean of per-row coefficients, so the two paths may differ by at most the
kernel tests' per-row bar, ``4 E32 + 2^-23`` with ``E32`` the max row error of the float32 torch
evaluation of the kernel's formula on the stored rows.  The memory test is the one the torch path
cannot pass: it makes an fp64 copy of the table and an fp64 [n, k] distance matrix.
"""
from collections import OrderedDict

import numpy as np
import pandas as pd
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.ml import clustering as CL
from orange3_spark_amd.ml import feature as F
from orange3_spark_amd.ml.evaluation import ClusteringEvaluator
from orange3_spark_amd.ops import silhouette as SIL

pytestmark = pytest.mark.gpu

N, D, K = 20000, 24, 8


def _data():
    rng = np.random.default_rng(0)
    centres = rng.normal(size=(K, D))
    lab = rng.integers(0, K, N)
    X = 2 * centres[lab] + rng.normal(size=(N, D)) + 50
    return X, rng.uniform(0.5, 1.5, N)


def _frame(session, X, **cols):
    names = [f"f{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    for k, v in cols.items():
        pdf[k] = v
    return F.VectorAssembler(inputCols=names, outputCol="features").transform(session.createDataFrame(pdf))


def _clustered(dtype):
    X, wt = _data()
    df = _frame(Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", dtype)), X, wt=wt)
    return CL.KMeans(k=K, seed=1, maxIter=10).fit(df).transform(df)


def _count_launches(monkeypatch):
    calls, real = [], SIL.silhouette_rows
    monkeypatch.setattr(SIL, "silhouette_rows", lambda *a, **k: (calls.append(a[0].dtype), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_agrees_with_the_torch_path(dtype, weighted, monkeypatch):
    out = _clustered(dtype)
    col = out.column_data("features")
    assert col.data.dtype == getattr(torch, dtype)
    ev = ClusteringEvaluator(weightCol="wt") if weighted else ClusteringEvaluator()
    monkeypatch.delenv("O3S_SILHOUETTE_KERNEL", raising=False)
    calls = _count_launches(monkeypatch)
    fused = ev.evaluate(out)
    assert calls == [col.data.dtype], "the evaluator did not take the fused pass"
    monkeypatch.setenv("O3S_SILHOUETTE_KERNEL", "0")
    parent = ev.evaluate(out)
    assert len(calls) == 1
    # the bar, from the stored rows alone
    c = out.column_data("prediction").data.long().cpu()
    w = torch.from_numpy(_data()[1]) if weighted else None
    X = col.dense().cpu()
    Y, Nn, Psi = SIL.cluster_moments(X.double(), c, K, w)
    s64 = SIL.silhouette_torch(X.double(), c, K, w, Y, Nn, Psi)
    E32 = float((SIL.silhouette_formula(X.float(), c, Y, Nn, Psi, torch.float32).double() - s64).abs().max())
    bar = 4 * E32 + 2.0 ** -23
    print(f"{dtype} weighted={weighted}: fused {fused:.9f} torch path {parent:.9f} difference "
          f"{abs(fused - parent):.3e} bar {bar:.3e}")
    assert 0.1 < parent < 1
    assert abs(fused - parent) <= bar


def test_cosine_is_unchanged(monkeypatch):
    out = _clustered("float32")
    ev = ClusteringEvaluator(distanceMeasure="cosine")
    monkeypatch.setattr(SIL, "silhouette_rows", lambda *a, **k: pytest.fail("fused pass on cosine distance"))
    monkeypatch.delenv("O3S_SILHOUETTE_KERNEL", raising=False)
    on = ev.evaluate(out)
    monkeypatch.setenv("O3S_SILHOUETTE_KERNEL", "0")
    assert ev.evaluate(out) == on and -1 < on < 1


def test_a_single_cluster_keeps_the_nan(monkeypatch):
    """One non-empty cluster: both switches give the formula's NaN, and no kernel is launched."""
    out = _clustered("float32")
    monkeypatch.setattr(SIL, "silhouette_rows", lambda *a, **k: pytest.fail("fused pass on a single cluster"))
    from orange3_spark_amd.frame import column as C
    from orange3_spark_amd.frame.dataframe import DataFrame
    col = out.column_data("features")
    pred = C.NumericColumn(torch.full((N,), 3, dtype=torch.int32, device=col.data.device))
    one = DataFrame(out.session, OrderedDict(features=col, prediction=pred), N)
    monkeypatch.delenv("O3S_SILHOUETTE_KERNEL", raising=False)
    assert np.isnan(ClusteringEvaluator().evaluate(one))
    monkeypatch.setenv("O3S_SILHOUETTE_KERNEL", "0")
    assert np.isnan(ClusteringEvaluator().evaluate(one))


def test_evaluation_makes_no_copy_of_the_table(monkeypatch):
    """400 000 x 64 fp32 rows (102 MB), k = 64: the evaluation raises the peak by less than
    n d 2 bytes, a quarter of an fp64 copy of the table -- ids, s and the products with the
    weights are a few words per row, the moment partials are constant.  The torch path adds at
    least n (d + k) 8 bytes."""
    from orange3_spark_amd.frame import column as C
    from orange3_spark_amd.frame.dataframe import DataFrame
    monkeypatch.delenv("O3S_SILHOUETTE_KERNEL", raising=False)
    n, d, k = 400_000, 64, 64
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(0, k, (n,), device=dev, generator=g, dtype=torch.int32)
    cen = torch.randn((k, d), device=dev, generator=g) * 2 + 50
    X = torch.randn((n, d), device=dev, generator=g) + cen[ids.long()]
    df = DataFrame(sg, OrderedDict(features=C.VectorColumn(X, d), prediction=C.NumericColumn(ids)), n)
    del cen
    calls = _count_launches(monkeypatch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    val = ClusteringEvaluator().evaluate(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"silhouette {val:.6f}, peak rise {rise / 1e6:.1f} MB, n d 2 = {n * d * 2 / 1e6:.1f} MB")
    assert calls == [torch.float32] and 0.1 < val < 1
    assert rise < n * d * 2

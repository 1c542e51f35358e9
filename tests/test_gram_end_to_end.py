"""Estimators on the fused weighted Gram pass (``ops/gram.py::weighted_gram``): GPU session with
``o3s.vector.dtype=float32`` against the CPU fp64 session.

Data and yardstick are those of test_f32_end_to_end.py (per-column scales 0.5 - 20, offsets
+-50, 20 000 x 24): the reference is the CPU fp64 fit, the yardstick the CPU fp64 fit on the
same rows rounded through bf16; the GPU result must be at least 4x closer to the reference
than that.  The memory test is the one that the ``rows_t_matmul`` path cannot pass: it makes
fp64 copies of the table.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.ml import feature as F
from orange3_spark_amd.ml import regression as RG
from orange3_spark_amd.ml.stat import Correlation
from orange3_spark_amd.ops import gram as GR

N, D = 20000, 24


def _data():
    rng = np.random.default_rng(0)
    scales = rng.uniform(0.5, 20, D)
    offsets = rng.uniform(-50, 50, D)
    Z = rng.normal(size=(N, D))
    X = Z * scales + offsets
    w = rng.normal(size=D)
    margin = Z @ w / np.sqrt(D)
    y_reg = margin + 0.5 * rng.normal(size=N)
    y_cnt = rng.poisson(np.exp(0.3 * margin)).astype(float)
    wt = rng.uniform(0.5, 1.5, N)
    return X, y_reg, y_cnt, wt


def _frame(session, X, **cols):
    names = [f"f{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    for k, v in cols.items():
        pdf[k] = v
    return F.VectorAssembler(inputCols=names, outputCol="features").transform(session.createDataFrame(pdf))


def _coefs(m):
    return np.concatenate([m.coefficients.toArray(), [m.intercept]])


def _linreg(df):
    return _coefs(RG.LinearRegression(regParam=0.01, labelCol="target").fit(df))


def _linreg_w(df):
    return _coefs(RG.LinearRegression(regParam=0.01, labelCol="target", weightCol="wt").fit(df))


def _pca(df):
    m = F.PCA(k=5, inputCol="features", outputCol="p").fit(df)
    return np.concatenate([np.asarray(m.explainedVariance.toArray()), np.abs(m.pc.toArray()).reshape(-1)])


def _corr(df):
    out = Correlation.corr(df, "features")
    return out.column_data(out.columns[0]).to_pylist()[0].toArray().reshape(-1)


def _glr(df):
    return _coefs(RG.GeneralizedLinearRegression(family="poisson", labelCol="count", maxIter=50, tol=1e-10).fit(df))


FITS = {"linreg": _linreg, "linreg_weighted": _linreg_w, "pca": _pca, "corr": _corr, "glr_poisson": _glr}


@pytest.fixture(scope="module")
def cpu_results():
    """name -> (CPU fp64 result on the exact rows, on the rows rounded through bf16)."""
    X, y_reg, y_cnt, wt = _data()
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    Xbf = torch.from_numpy(X).to(torch.bfloat16).double().numpy()
    c64 = _frame(sc, X, target=y_reg, count=y_cnt, wt=wt)
    cbf = _frame(sc, Xbf, target=y_reg, count=y_cnt, wt=wt)
    return {k: (f(c64), f(cbf)) for k, f in FITS.items()}


@pytest.fixture(scope="module")
def gpu_frame():
    X, y_reg, y_cnt, wt = _data()
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    return _frame(sg, X, target=y_reg, count=y_cnt, wt=wt)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FITS))
def test_gpu_f32_session_matches_cpu_fp64(cpu_results, gpu_frame, name, monkeypatch):
    feat = gpu_frame.column_data("features")
    assert feat.data.dtype == torch.float32 and GR.column_rows(feat) is not None
    calls = []
    real = GR.weighted_gram
    monkeypatch.setattr(GR, "weighted_gram", lambda *a, **k: (calls.append(a[0].dtype), real(*a, **k))[1])
    import orange3_spark_amd.models.irls as irls
    monkeypatch.setattr(irls, "weighted_gram", GR.weighted_gram)
    c64, cbf = cpu_results[name]
    got = FITS[name](gpu_frame)
    assert calls and set(calls) == {torch.float32}, "the estimator did not take the fused pass"
    e32, ebf = np.abs(got - c64).max(), np.abs(cbf - c64).max()
    print(f"{name}: max|GPU float32 - C64| {e32:.3e}  CPU on bf16-rounded rows {ebf:.3e}  ratio {ebf / e32:.1f}")
    assert e32 <= ebf / 4


@pytest.mark.gpu
def test_default_linear_regression_makes_no_copy_of_the_table():
    """400 000 x 64 fp32 features (102 MB): the default LinearRegression().fit raises the peak by
    less than half the feature matrix (the rows_t_matmul path allocates four times the matrix)."""
    from orange3_spark_amd.frame import column as C
    from orange3_spark_amd.frame.dataframe import DataFrame
    n, d = 400_000, 64
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn((n, d), device=dev, generator=g) * 3 + 20
    beta = torch.linspace(-1, 1, d, device=dev)
    y = (X - 20) @ beta + 0.1 * torch.randn(n, device=dev, generator=g)
    from collections import OrderedDict
    df = DataFrame(sg, OrderedDict(features=C.VectorColumn(X, d), label=C.NumericColumn(y)), n)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = RG.LinearRegression().fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    table = X.numel() * X.element_size()
    print(f"peak rise {rise / 1e6:.1f} MB, table {table / 1e6:.1f} MB")
    assert np.abs(m.coefficients.toArray() - beta.cpu().numpy()).max() < 1e-3
    assert rise < table / 2


@pytest.mark.gpu
def test_lineage_and_wide_columns_keep_the_old_path(monkeypatch):
    """A lineage column and a d = 300 column are not the kernel's: they fit through
    rows_t_matmul as before and match the CPU fit."""
    from orange3_spark_amd.synthetic import LineageVectorColumn
    monkeypatch.setattr(GR, "weighted_gram", lambda *a, **k: pytest.fail("fused pass on a column it must not take"))
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    rng = np.random.default_rng(3)
    X = rng.normal(size=(2000, 300)) + 5
    y = X[:, :10] @ np.arange(1, 11) + 0.1 * rng.normal(size=2000)
    cg = _coefs(RG.LinearRegression(regParam=0.01, labelCol="target").fit(_frame(sg, X, target=y)))
    cc = _coefs(RG.LinearRegression(regParam=0.01, labelCol="target").fit(_frame(sc, X, target=y)))
    assert np.abs(cg - cc).max() < 1e-3 * np.abs(cc).max()
    lg = sg.synthetic.classification(20000, 16, seed=5, resident_fraction=1e-12)   # no resident rows
    lc = sc.synthetic.classification(20000, 16, seed=5)
    assert isinstance(lg.column_data("features"), LineageVectorColumn)
    assert GR.column_rows(lg.column_data("features")) is None
    mg, mc = RG.LinearRegression(regParam=0.01).fit(lg), RG.LinearRegression(regParam=0.01).fit(lc)
    assert np.abs(_coefs(mg) - _coefs(mc)).max() < 1e-3

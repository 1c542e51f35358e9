"""``o3s.vector.dtype=float32`` end to end: GPU session with fp32 feature rows vs the CPU fp64
session, from ``createDataFrame`` -> ``VectorAssembler`` to the fitted model and its
predictions.

The data (per-column scales 0.5 - 20, offsets +-50) loses most of its information when the
rows are rounded to bf16.  The reference is the CPU fp64 fit; the yardstick is the CPU fp64
fit on the same rows rounded through bf16 on the host: the fp32 GPU fit must be at least 4x
closer to the reference than that.  (On the CPU, rows rounded to fp32 land three to five
orders of magnitude closer than rows rounded to bf16 -- test_cpu_fp32_rounded_rows_pass_the_bar
prints both -- so the factor leaves room for fp32 accumulation and line-search noise; a path
that silently rounds to bf16 lands at a ratio of about 1.)
"""
import numpy as np
import pandas as pd
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.ml import classification as CL
from orange3_spark_amd.ml import clustering as CU
from orange3_spark_amd.ml import feature as F
from orange3_spark_amd.ml import regression as RG

N, D = 20000, 24


def _data():
    rng = np.random.default_rng(0)
    scales = rng.uniform(0.5, 20, D)
    offsets = rng.uniform(-50, 50, D)
    Z = rng.normal(size=(N, D))
    X = Z * scales + offsets
    w = rng.normal(size=D)
    margin = Z @ w / np.sqrt(D)
    y_cls = (margin * 2 + rng.logistic(size=N) > 0).astype(float)
    y_reg = margin + 0.5 * rng.normal(size=N)
    return X, y_cls, y_reg


def _frame(session, X, **cols):
    names = [f"f{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    for k, v in cols.items():
        pdf[k] = v
    return F.VectorAssembler(inputCols=names, outputCol="features").transform(session.createDataFrame(pdf))


def _col(df, name):
    v = df.select(name).toPandas()[name]
    if len(v) and hasattr(v.iloc[0], "toArray"):
        return np.stack([x.toArray() for x in v])
    return np.asarray(v.tolist(), dtype=np.float64)


def _lr():
    return CL.LogisticRegression(maxIter=200, tol=1e-12, regParam=0.01)


def _linreg():
    return RG.LinearRegression(solver="l-bfgs", maxIter=200, tol=1e-12, regParam=0.01, labelCol="target")


def _coefs(m):
    return np.concatenate([m.coefficients.toArray(), [m.intercept]])


@pytest.fixture(scope="module")
def cpu_fits():
    """CPU fp64 fits on the exact rows (C64) and on the rows rounded through bf16 (Cbf)."""
    X, y_cls, y_reg = _data()
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    Xbf = torch.from_numpy(X).to(torch.bfloat16).double().numpy()
    c64 = _frame(sc, X, label=y_cls, target=y_reg)
    cbf = _frame(sc, Xbf, label=y_cls, target=y_reg)
    out = {}
    for name, make in (("lr", _lr), ("linreg", _linreg)):
        m64, mbf = make().fit(c64), make().fit(cbf)
        out[name] = (_coefs(m64), _coefs(mbf), _col(m64.transform(c64), "prediction"))
    return out


def test_cpu_fp32_rounded_rows_pass_the_bar(cpu_fits):
    """The bar is reachable and meaningful: CPU fits on rows rounded to fp32 are far inside
    it and predict like the fp64 fits, while the bf16-rounded fits define it."""
    X, y_cls, y_reg = _data()
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    c32 = _frame(sc, X.astype(np.float32).astype(np.float64), label=y_cls, target=y_reg)
    for name, make in (("lr", _lr), ("linreg", _linreg)):
        c64, cbf, p64 = cpu_fits[name]
        m = make().fit(c32)
        e32, ebf = np.abs(_coefs(m) - c64).max(), np.abs(cbf - c64).max()
        print(f"{name}: max|coef - C64|  fp32-rounded rows {e32:.3e}  bf16-rounded rows {ebf:.3e}")
        assert e32 <= ebf / 400
        p = _col(m.transform(c32), "prediction")
        if name == "lr":
            assert (p == p64).mean() >= 0.995
        else:                 # the GPU-vs-CPU regression bound of test_gpu_estimators.py
            assert np.sqrt(np.mean((p - p64) ** 2)) < 0.05 * np.std(p64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lr", "linreg"])
def test_gpu_f32_session_fit_matches_cpu_fp64(cpu_fits, name):
    from orange3_spark_amd.models.glm import GlmData
    X, y_cls, y_reg = _data()
    make = _lr if name == "lr" else _linreg
    c64, cbf, p64 = cpu_fits[name]
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    g32 = _frame(sg, X, label=y_cls, target=y_reg)
    feat = g32.column_data("features")
    assert feat.data.dtype == torch.float32 and feat.ld == 24 and feat.size == 24
    data = GlmData(g32.comm, feat, g32.column_data("label").data)
    assert data.kernel and data.X.dtype == torch.float32
    m = make().fit(g32)
    e32, ebf = np.abs(_coefs(m) - c64).max(), np.abs(cbf - c64).max()
    # for contrast: the default (bf16) GPU session on the same table
    sb = Session(SessionConf().set("o3s.device", "cuda"))
    eauto = np.abs(_coefs(make().fit(_frame(sb, X, label=y_cls, target=y_reg))) - c64).max()
    print(f"{name}: max|coef - C64|  GPU float32 {e32:.3e}  GPU auto (bf16) {eauto:.3e}  "
          f"CPU on bf16-rounded rows {ebf:.3e}")
    assert e32 <= ebf / 4
    p = _col(m.transform(g32), "prediction")
    if name == "lr":
        assert (p == p64).mean() >= 0.995
    else:                     # the GPU-vs-CPU regression bound of test_gpu_estimators.py
        assert np.sqrt(np.mean((p - p64) ** 2)) < 0.05 * np.std(p64)


@pytest.mark.gpu
def test_gpu_f32_svc_predicts_through_margin_kernel(monkeypatch):
    """LinearSVC on padded fp32 rows (d = 6 -> 8): fit through the fp32 kernels, predictions
    through glm_margin on the stored rows (no fp64 copy), agreeing with the CPU session."""
    from orange3_spark_amd.ops import glm as G
    rng = np.random.default_rng(0)
    X = rng.normal(size=(4000, 6)) * 3 + 10
    y = ((X[:, 0] + 0.5 * X[:, 1] - 0.25 * X[:, 2] - 12.5 + 0.3 * rng.normal(size=4000)) > 0).astype(float)
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    g, c = _frame(sg, X, label=y), _frame(sc, X, label=y)
    seen = []
    real = G.glm_margin

    def counted(Xr, coef, b):
        seen.append((Xr.dtype, tuple(Xr.shape)))
        return real(Xr, coef, b)
    monkeypatch.setattr(G, "glm_margin", counted)
    pg = _col(CL.LinearSVC(maxIter=50).fit(g).transform(g), "prediction")
    assert (torch.float32, (4000, 8)) in seen
    pc = _col(CL.LinearSVC(maxIter=50).fit(c).transform(c), "prediction")
    assert (pg == pc).mean() > 0.97 and (pg == y).mean() > 0.8


@pytest.mark.gpu
def test_gpu_f32_padding_leaves_other_estimators_alone():
    """KMeans, DecisionTreeClassifier and StandardScaler on padded fp32 rows (d = 6 -> 8) vs
    the CPU session: data and thresholds of test_gpu_estimators.py."""
    from sklearn.metrics import adjusted_rand_score
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    rng = np.random.default_rng(0)
    X = np.round(rng.normal(size=(4000, 6)) * 8) / 8
    y = ((X[:, 0] + 0.5 * X[:, 1] - 0.25 * X[:, 2] + 0.3 * rng.normal(size=4000)) > 0).astype(float)
    g, c = _frame(sg, X, label=y), _frame(sc, X, label=y)
    feat = g.column_data("features")
    assert feat.data.dtype == torch.float32 and feat.ld == 8 and feat.size == 6
    make = lambda: CL.DecisionTreeClassifier(maxDepth=4, seed=1)       # noqa: E731
    pg, pc = _col(make().fit(g).transform(g), "prediction"), _col(make().fit(c).transform(c), "prediction")
    assert (pg == pc).mean() > 0.97 and (pg == y).mean() > 0.8
    # scaler: fp32 storage of the output, so within fp32 rounding of the fp64 result
    mk = lambda: F.StandardScaler(inputCol="features", outputCol="scaled", withMean=True, withStd=True)   # noqa: E731
    og, oc = mk().fit(g).transform(g), mk().fit(c).transform(c)
    sgc = og.column_data("scaled")
    assert sgc.size == 6
    a, b = _col(og, "scaled"), _col(oc, "scaled")
    assert a.shape == b.shape == (4000, 6)
    assert np.allclose(a, b, rtol=1e-6, atol=np.finfo(np.float32).eps * np.abs(b).max())
    # clusters
    cent = np.array([[0, 0, 0, 0, 0, 0], [6, 0, 0, 0, 3, 0], [0, 6, 0, 3, 0, 0], [0, 0, 6, 0, 0, 3]], dtype=float)
    rng = np.random.default_rng(2)
    Xk = np.round(np.concatenate([ci + rng.normal(0, 0.5, (500, 6)) for ci in cent]) * 8) / 8
    gk, ck = _frame(sg, Xk), _frame(sc, Xk)
    mg, mc = CU.KMeans(k=4, seed=1).fit(gk), CU.KMeans(k=4, seed=1).fit(ck)
    assert adjusted_rand_score(_col(mg.transform(gk), "prediction"), _col(mc.transform(ck), "prediction")) > 0.99

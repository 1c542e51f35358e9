"""Multinomial LogisticRegression with ``o3s.vector.dtype=float32`` end to end: a GPU session
with fp32 feature rows vs the CPU fp64 session, from ``createDataFrame`` -> ``VectorAssembler``
to the fitted coefficient matrix and the predictions (the pattern of test_f32_end_to_end.py).

The reference is the CPU fp64 fit; the yardstick is the CPU fp64 fit on the same rows rounded
through bf16 on the host: the fp32 GPU fit must be at least 4x closer to the reference than
that, and has to get there through the fused pass (``glm_softmax_f32_kernel``), not the
chunked one.  The columns have scales 0.5 - 4 and offsets within +-1: with larger offsets
Spark's uncentred standardisation leaves the multinomial L-BFGS unconverged, and two CPU fp64
fits then disagree by more than the bar.
"""
import numpy as np
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.ml import classification as CL
from test_f32_end_to_end import _col, _frame

N, D, K = 20000, 24, 4


def _data(n=N, d=D, k=K, seed=0):
    rng = np.random.default_rng(seed)
    scales = rng.uniform(0.5, 4, d)
    offsets = rng.uniform(-1, 1, d)
    Z = rng.normal(size=(n, d))
    X = Z * scales + offsets
    Wt = rng.normal(size=(k, d))
    y = np.argmax(Z @ Wt.T / np.sqrt(d) * 2 + rng.gumbel(size=(n, k)), axis=1).astype(float)
    return X, y


def _lr():
    return CL.LogisticRegression(maxIter=300, tol=1e-12, regParam=0.01)


def _coefs(m):
    return np.concatenate([m.coefficientMatrix.toArray().ravel(), m.interceptVector.toArray()])


@pytest.fixture(scope="module")
def cpu_fits():
    """CPU fp64 fits on the exact rows and on the rows rounded through bf16: (coefficients,
    coefficients, predictions of the exact fit)."""
    X, y = _data()
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    Xbf = torch.from_numpy(X).to(torch.bfloat16).double().numpy()
    c64, cbf = _frame(sc, X, label=y), _frame(sc, Xbf, label=y)
    m64, mbf = _lr().fit(c64), _lr().fit(cbf)
    return _coefs(m64), _coefs(mbf), _col(m64.transform(c64), "prediction")


def test_cpu_fp32_rounded_rows_pass_the_bar(cpu_fits):
    """The bar is reachable and meaningful: the CPU fit on rows rounded to fp32 is at least
    400x closer to the exact fit than the fit on bf16-rounded rows."""
    X, y = _data()
    c64, cbf, p64 = cpu_fits
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    c32 = _frame(sc, X.astype(np.float32).astype(np.float64), label=y)
    m = _lr().fit(c32)
    assert m.numClasses == K
    e32, ebf = np.abs(_coefs(m) - c64).max(), np.abs(cbf - c64).max()
    print(f"multinomial: max|coef - C64|  fp32-rounded rows {e32:.3e}  bf16-rounded rows {ebf:.3e}  "
          f"({m.summary.totalIterations} iterations)")
    assert e32 <= ebf / 400
    assert (_col(m.transform(c32), "prediction") == p64).mean() >= 0.995


def _count_passes(monkeypatch):
    """Count fused passes (by row dtype) and chunked evaluations (they alone call
    torch.logsumexp during a fit)."""
    from orange3_spark_amd.ops import glm as G
    fused, chunked = [], []
    real_pass, real_lse = G.softmax_pass, torch.logsumexp

    def counted_pass(Xr, *a):
        fused.append((Xr.dtype, Xr.stride(0)))
        return real_pass(Xr, *a)

    def counted_lse(*a, **kw):
        chunked.append(1)
        return real_lse(*a, **kw)
    monkeypatch.setattr(G, "softmax_pass", counted_pass)
    monkeypatch.setattr(torch, "logsumexp", counted_lse)
    return fused, chunked


@pytest.mark.gpu
def test_gpu_f32_session_multinomial_fit_matches_cpu_fp64(cpu_fits, monkeypatch):
    X, y = _data()
    c64, cbf, p64 = cpu_fits
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    g32 = _frame(sg, X, label=y)
    feat = g32.column_data("features")
    assert feat.data.dtype == torch.float32 and feat.ld == 24 and feat.size == 24
    with monkeypatch.context() as mp:
        fused, chunked = _count_passes(mp)
        m = _lr().fit(g32)
    assert fused and set(fused) == {(torch.float32, 24)} and not chunked
    e32, ebf = np.abs(_coefs(m) - c64).max(), np.abs(cbf - c64).max()
    print(f"multinomial: max|coef - C64|  GPU float32 {e32:.3e}  CPU on bf16-rounded rows {ebf:.3e}  "
          f"({m.summary.totalIterations} iterations, {len(fused)} fused passes)")
    assert e32 <= ebf / 4
    assert (_col(m.transform(g32), "prediction") == p64).mean() >= 0.995


@pytest.mark.gpu
def test_gpu_f32_session_multinomial_fit_on_padded_rows(monkeypatch):
    """d = 6 -> ld 8, K = 3: the fused pass takes the [:, :6] view of the padded fp32 column."""
    X, y = _data(4000, 6, 3, seed=1)
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    g, c = _frame(sg, X, label=y), _frame(sc, X, label=y)
    feat = g.column_data("features")
    assert feat.data.dtype == torch.float32 and feat.ld == 8 and feat.size == 6
    with monkeypatch.context() as mp:
        fused, chunked = _count_passes(mp)
        mg = CL.LogisticRegression(maxIter=100, regParam=0.01).fit(g)
    assert fused and set(fused) == {(torch.float32, 8)} and not chunked
    pg = _col(mg.transform(g), "prediction")
    pc = _col(CL.LogisticRegression(maxIter=100, regParam=0.01).fit(c).transform(c), "prediction")
    assert (pg == pc).mean() >= 0.97

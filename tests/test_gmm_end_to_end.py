"""GaussianMixture on the fused E-step and Gram passes (``ops/gmm.py``): GPU sessions against
the CPU fp64 session.

Data: 20 000 x 24, four overlapping components (centres 0.45 N(0, 1) per coordinate before
scaling), per-column scales 0.5 - 20, offsets +-50.  The reference is the CPU fp64 fit, the
yardstick the CPU fp64 fit on the same rows rounded through bf16; a GPU fit must be at least 4x
closer to its reference than that, for weights, means and covariances (each relative to its
largest entry, components sorted by their first mean coordinate).  The memory test is the one
the chunked fp64 path cannot pass: it makes an fp64 copy of the table.
"""
from collections import OrderedDict

import numpy as np
import pandas as pd
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.ml import clustering as CL
from orange3_spark_amd.ml import feature as F
from orange3_spark_amd.ops import gmm as GM

N, D, K = 20000, 24, 4


def _data():
    rng = np.random.default_rng(0)
    scales = rng.uniform(0.5, 20, D)
    offsets = rng.uniform(-50, 50, D)
    centres = 0.45 * rng.normal(size=(K, D))
    lab = rng.integers(0, K, N)
    X = (centres[lab] + rng.normal(size=(N, D))) * scales + offsets
    return X, rng.uniform(0.5, 1.5, N)


def _frame(session, X, **cols):
    names = [f"f{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X, columns=names)
    for k, v in cols.items():
        pdf[k] = v
    return F.VectorAssembler(inputCols=names, outputCol="features").transform(session.createDataFrame(pdf))


def _fit(df, weighted=False, **kw):
    return CL.GaussianMixture(k=K, seed=3, maxIter=100, tol=1e-3, weightCol="wt" if weighted else None, **kw).fit(df)


def _params(m):
    """(weights, means, covs) with the components sorted by their first mean coordinate."""
    mu = np.stack([g.mean.toArray() for g in m.gaussians])
    o = np.argsort(mu[:, 0])
    return np.asarray(m.weights)[o], mu[o], np.stack([g.cov.toArray() for g in m.gaussians])[o]


def _rel(a, b):
    return [np.abs(x - y).max() / np.abs(y).max() for x, y in zip(a, b)]


def _bf16(X):
    return torch.from_numpy(X).to(torch.bfloat16).double().numpy()


@pytest.fixture(scope="module")
def cpu_fits():
    """weighted? -> (CPU fp64 fit on the exact rows, on the rows rounded through bf16)."""
    X, wt = _data()
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    c64, cbf = _frame(sc, X, wt=wt), _frame(sc, _bf16(X), wt=wt)
    return {wd: (_params(_fit(c64, wd)), _params(_fit(cbf, wd))) for wd in (False, True)}


def _gpu_frame(dtype):
    X, wt = _data()
    return _frame(Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", dtype)), X, wt=wt)


def _count_esteps(monkeypatch):
    calls, real = [], GM.estep
    monkeypatch.setattr(GM, "estep", lambda *a, **k: (calls.append(a[0].dtype), real(*a, **k))[1])
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_gpu_f32_session_matches_cpu_fp64(cpu_fits, weighted, monkeypatch):
    df = _gpu_frame("float32")
    assert df.column_data("features").data.dtype == torch.float32
    calls = _count_esteps(monkeypatch)
    m = _fit(df, weighted)
    assert calls and set(calls) == {torch.float32}, "the estimator did not take the fused E-step"
    c64, cbf = cpu_fits[weighted]
    got, yard = _rel(_params(m), c64), _rel(cbf, c64)
    for name, e, y in zip(("weights", "means", "covs"), got, yard):
        print(f"{name}: GPU float32 vs C64 {e:.3e}  CPU on bf16-rounded rows {y:.3e}  ratio {y / e:.1f}")
    print(f"iterations {m.summary.numIter}, log-likelihood {m.summary.logLikelihood:.6f}")
    assert all(e <= y / 4 for e, y in zip(got, yard))
    assert sum(m.summary.clusterSizes) == N


@pytest.mark.gpu
def test_gpu_bf16_session_matches_cpu_fp64_on_the_rounded_rows(cpu_fits, monkeypatch):
    df = _gpu_frame("bfloat16")
    assert df.column_data("features").data.dtype == torch.bfloat16
    calls = _count_esteps(monkeypatch)
    m = _fit(df)
    assert calls and set(calls) == {torch.bfloat16}
    c64, cbf = cpu_fits[False]
    got, yard = _rel(_params(m), cbf), _rel(cbf, c64)
    for name, e, y in zip(("weights", "means", "covs"), got, yard):
        print(f"{name}: GPU bf16 vs CPU on the same rows {e:.3e}  yardstick {y:.3e}  ratio {y / e:.1f}")
    assert all(e <= y / 4 for e, y in zip(got, yard))


@pytest.mark.gpu
def test_default_tolerance_terminates():
    """The per-row log density is fp32 on the fused path; Spark's default tol = 0.01 is above the
    noise that leaves in the log-likelihood, so the stop rule is met.  (The CPU fp64 fit of this
    data meets it after 215 iterations, hence the maxIter.)"""
    m = CL.GaussianMixture(k=K, seed=3, maxIter=400).fit(_gpu_frame("float32"))
    h = m.summary.objectiveHistory
    print(f"default tol: {m.summary.numIter} iterations, last steps {np.diff(h)[-3:]}")
    assert m.summary.numIter < 400 and abs(h[-1] - h[-2]) < 0.01


@pytest.mark.gpu
def test_transform_probabilities(monkeypatch):
    """probability: fp64, rows sum to 1 within 1e-12, prediction its argmax, and within the kernel
    test's bar (4x the float32 evaluation's error, floor 2^-24) of the CPU model's on the same rows."""
    X, wt = _data()
    X = torch.from_numpy(X).float().double().numpy()            # the rows both sessions hold exactly
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    dg, dc = _frame(sg, X), _frame(sc, X)
    m = _fit(dg)
    calls = _count_esteps(monkeypatch)
    out = m.transform(dg)
    assert calls == [torch.float32]
    pc = out.column_data("probability")
    assert pc.data.dtype == torch.float64 and pc.size == K
    P = pc.dense().cpu()
    assert float((P.sum(1) - 1).abs().max()) <= 1e-12
    pred = out.column_data("prediction").data.cpu().long()
    assert torch.equal(pred, P.argmax(1))
    Pc = m.transform(dc).column_data("probability").dense()
    w, mu, cov = (torch.from_numpy(a) for a in (m._w, m._mu, m._cov))
    yard = GM.estep_torch(torch.from_numpy(X), D, w, mu, cov, dtype=torch.float32)[0].T.double()
    bar = 4 * max(float((yard - Pc).abs().max()), 2.0 ** -24)
    err = float((P - Pc).abs().max())
    print(f"transform: max |P gpu - P cpu| {err:.3e}, bar {bar:.3e}")
    assert err <= bar


@pytest.mark.gpu
def test_fit_makes_no_copy_of_the_table():
    """400 000 x 64 fp32 features (102 MB), K = 4: the fit raises the peak by less than half the
    table -- resp is K / d = 1/16 of it, lse and the weight copies 1/64 each, the Gram slabs are
    constant; the chunked path's fp64 copy alone is twice the table."""
    from orange3_spark_amd.frame import column as C
    from orange3_spark_amd.frame.dataframe import DataFrame
    n, d = 400_000, 64
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn((n, d), device=dev, generator=g) * 3 + 20
    X[: n // 2, :8] += 6
    df = DataFrame(sg, OrderedDict(features=C.VectorColumn(X, d)), n)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = CL.GaussianMixture(k=4, maxIter=3, seed=1).fit(df)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    table = X.numel() * X.element_size()
    print(f"peak rise {rise / 1e6:.1f} MB, table {table / 1e6:.1f} MB")
    assert sum(m.summary.clusterSizes) == n and m.summary.numIter == 3
    assert rise < table / 2


@pytest.mark.gpu
def test_other_columns_and_the_switch_keep_the_old_path(monkeypatch):
    """A lineage column, a d = 300 column, K = 65 and FUSED = 0 are not the kernel's: they fit
    through the chunked fp64 path as before and match the CPU fit."""
    from sklearn.metrics import adjusted_rand_score
    from orange3_spark_amd.synthetic import LineageVectorColumn
    monkeypatch.setattr(GM, "estep", lambda *a, **k: pytest.fail("fused E-step on a fit it must not take"))
    sg = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    sc = Session(SessionConf().set("o3s.device", "cpu"))

    def same_partition(make, g, c, floor=0.99):
        pg = make().fit(g).transform(g).column_data("prediction").data.cpu().numpy()
        pc = make().fit(c).transform(c).column_data("prediction").data.cpu().numpy()
        assert adjusted_rand_score(pg, pc) > floor

    rng = np.random.default_rng(2)
    cent = np.array([[0, 0, 0], [6, 0, 0], [0, 6, 0], [0, 0, 6]], dtype=float)
    X3 = np.round(np.concatenate([c + rng.normal(0, 0.5, (500, 3)) for c in cent]) * 8) / 8
    with monkeypatch.context() as mp:                                        # the switch
        mp.setattr(GM, "FUSED", 0)
        same_partition(lambda: CL.GaussianMixture(k=4, seed=1), _frame(sg, X3), _frame(sc, X3))
    # wider than the kernel: two blobs 8 apart in the first three of 300 columns
    Xw = np.round(rng.normal(0, 0.5, (1500, 300)) * 8) / 8
    Xw[:750, :3] += 8
    same_partition(lambda: CL.GaussianMixture(k=2, seed=1, maxIter=10), _frame(sg, Xw), _frame(sc, Xw))
    # more components than the kernel takes: the gate alone
    col = _frame(sg, X3).column_data("features")
    assert GM.estep_ok(col.data, col.size, 64) and not GM.estep_ok(col.data, col.size, 65)
    g65 = CL.GaussianMixture(k=65, seed=1, maxIter=2).fit(_frame(sg, X3))
    c65 = CL.GaussianMixture(k=65, seed=1, maxIter=2).fit(_frame(sc, X3))
    assert g65.summary.logLikelihood == pytest.approx(c65.summary.logLikelihood, rel=1e-6)
    # lineage rows
    lg = sg.synthetic.classification(20000, 16, seed=5, resident_fraction=1e-12)   # no resident rows
    lc = sc.synthetic.classification(20000, 16, seed=5)
    assert isinstance(lg.column_data("features"), LineageVectorColumn)
    mg = CL.GaussianMixture(k=2, seed=1, maxIter=5).fit(lg)
    mc = CL.GaussianMixture(k=2, seed=1, maxIter=5).fit(lc)
    assert mg.summary.logLikelihood == pytest.approx(mc.summary.logLikelihood, rel=1e-3)

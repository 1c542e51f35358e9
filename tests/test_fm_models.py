"""FMClassifier / FMRegressor on the fused FM passes against their torch program
(``O3S_FM_KERNEL=0``) on GPU frames: the fit takes the kernel and never ``dense_features``,
the fitted parameters and the transform columns agree, mini-batches use the kernel, the inputs
that keep the torch program do so without error, and a saved model scores the same."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.frame import column as C
from orange3_spark_amd.frame.dataframe import DataFrame
from orange3_spark_amd.ml import _fm
from orange3_spark_amd.ml import classification as CL
from orange3_spark_amd.ml import common as U
from orange3_spark_amd.ml import feature as FT
from orange3_spark_amd.ml import regression as RG
from orange3_spark_amd.ops import fm as FM

N, D = 20_000, 24
SWITCH = "O3S_FM_KERNEL"
KW = dict(maxIter=30, stepSize=0.05, seed=1)


def _frames(s):
    rng = np.random.default_rng(5)
    X = rng.normal(size=(N, D))
    score = X[:, 0] * X[:, 1] - X[:, 2] * X[:, 3] + 0.5 * X[:, 4] + 0.3 * rng.normal(size=N)
    Xt = torch.from_numpy(X)

    def frame(y):
        return DataFrame(s, OrderedDict(features=FT.to_vector_column(s, Xt.to(s.device)),
                                        label=C.NumericColumn(torch.from_numpy(y).to(s.device))), N)

    return frame((score > 0).astype(np.float64)), frame(score)


def _watch(monkeypatch):
    """Count fm_pass / fm_margin calls and the dense_features calls of the FM module."""
    calls = dict(fm_pass=0, fm_margin=0, dense=0)
    real_pass, real_margin, real_dense = FM.fm_pass, FM.fm_margin, U.dense_features

    def count(key, fn):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(FM, "fm_pass", count("fm_pass", real_pass))
    monkeypatch.setattr(FM, "fm_margin", count("fm_margin", real_margin))
    monkeypatch.setattr(U, "dense_features", count("dense", real_dense))
    return calls


def _params(m):
    return m.factors.toArray(), m.linear.toArray(), np.array([m.intercept])


def _fit_both(est, df, monkeypatch, what):
    calls = _watch(monkeypatch)
    monkeypatch.delenv(SWITCH, raising=False)
    on = est.fit(df)
    assert calls["fm_pass"] >= 30 and calls["dense"] == 0, (what, calls)
    taken = calls["fm_pass"]
    monkeypatch.setenv(SWITCH, "0")
    off = est.fit(df)
    assert calls["fm_pass"] == taken and calls["dense"] >= 1, (what, calls)
    monkeypatch.delenv(SWITCH, raising=False)
    for name, a, b in zip(("factors", "linear", "intercept"), _params(on), _params(off)):
        top = max(np.abs(np.concatenate([p.reshape(-1) for p in _params(off)])).max(), 1e-30)
        diff = np.abs(a - b).max()
        print(f"{what}: {name} kernel vs torch program {diff:.2e} (largest entry {top:.2e}, bar {1e-3 * top:.2e})")
        assert diff <= 1e-3 * top, (what, name)
    return on, off, calls


def _transform_both(model, df, monkeypatch, calls, what):
    monkeypatch.delenv(SWITCH, raising=False)
    before = dict(calls)
    on = model.transform(df)
    assert calls["fm_margin"] == before["fm_margin"] + 1 and calls["dense"] == before["dense"], (what, calls)
    monkeypatch.setenv(SWITCH, "0")
    off = model.transform(df)
    assert calls["fm_margin"] == before["fm_margin"] + 1 and calls["dense"] == before["dense"] + 1, (what, calls)
    monkeypatch.delenv(SWITCH, raising=False)
    assert on.columns == off.columns
    g = lambda out, k: out.column_data(k).data      # noqa: E731
    if "probability" in on.columns:
        m = g(off, "rawPrediction")[:, 1]
        dp = float((g(on, "probability") - g(off, "probability")).abs().max())
        dm = float((g(on, "rawPrediction") - g(off, "rawPrediction")).abs().max())
        clear = m.abs() >= 1e-5
        print(f"{what}: transform probability {dp:.2e} (bar 1e-05), rawPrediction {dm:.2e}, "
              f"{int((~clear).sum())} rows with |m| < 1e-5")
        assert g(on, "probability").dtype == torch.float64 and g(on, "rawPrediction").shape == (N, 2)
        assert dp <= 1e-5
        assert torch.equal(g(on, "prediction")[clear], g(off, "prediction")[clear])
    else:
        m = g(off, "prediction")
        dm = float((g(on, "prediction") - m).abs().max())
        bar = 1e-5 * max(1.0, float(m.abs().max()))
        print(f"{what}: transform prediction {dm:.2e} (bar {bar:.2e})")
        assert dm <= bar
    return on


def _check_session(s, monkeypatch, tmp_path, dtype):
    cls_df, reg_df = _frames(s)
    assert cls_df.column_data("features").data.dtype == dtype
    for est, df, what in ((CL.FMClassifier(**KW), cls_df, f"FMClassifier {dtype}"),
                          (RG.FMRegressor(**KW), reg_df, f"FMRegressor {dtype}")):
        on, off, calls = _fit_both(est, df, monkeypatch, what)
        out = _transform_both(on, df, monkeypatch, calls, what)
        # save -> load -> transform
        path = str(tmp_path / what.replace(" ", "_").replace(".", "_"))
        on.save(path)
        back = type(on).load(path)
        again = back.transform(df)
        for k in ("prediction", "probability"):
            if k in out.columns:
                assert torch.equal(again.column_data(k).data, out.column_data(k).data), (what, k)
        # single vectors stay on torch
        x = df.column_data("features").dense()[0].double().cpu().numpy()
        before = calls["fm_margin"]
        assert np.isfinite(on.predict(x)) and calls["fm_margin"] == before
    return cls_df, reg_df


@pytest.mark.gpu
def test_fit_and_transform_take_the_kernel_bf16(monkeypatch, tmp_path):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    _check_session(s, monkeypatch, tmp_path, torch.bfloat16)


@pytest.mark.gpu
def test_fit_and_transform_take_the_kernel_fp32(monkeypatch, tmp_path):
    s = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    _check_session(s, monkeypatch, tmp_path, torch.float32)


@pytest.mark.gpu
def test_mini_batch_fit_takes_the_kernel(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    cls_df, _ = _frames(s)
    est = CL.FMClassifier(miniBatchFraction=0.5, **KW)
    on, off, calls = _fit_both(est, cls_df, monkeypatch, "FMClassifier miniBatchFraction=0.5")
    assert calls["fm_pass"] > 30          # 2500-row chunks: several launches per step


@pytest.mark.gpu
def test_masks_and_weights_on_the_kernel(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    _, reg_df = _frames(s)
    w = torch.rand(N, dtype=torch.float64, generator=torch.Generator().manual_seed(2)) + 0.5
    df = reg_df.withColumnData("weight", C.NumericColumn(w.to(s.device)))
    est = RG.FMRegressor(fitLinear=False, fitIntercept=False, regParam=0.01, **KW)
    est._set(weightCol="weight")
    on, off, _ = _fit_both(est, df, monkeypatch, "FMRegressor weighted, no linear term, no intercept")
    assert not on.linear.toArray().any() and on.intercept == 0.0


@pytest.mark.gpu
def test_sparse_lineage_wide_and_cpu_inputs_keep_the_torch_program(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    cls_df, _ = _frames(s)
    model = CL.FMClassifier(maxIter=3, stepSize=0.05, seed=1).fit(cls_df)
    called = []
    monkeypatch.setattr(FM, "fm_pass", lambda *a, **k: called.append("pass"))
    monkeypatch.setattr(FM, "fm_margin", lambda *a, **k: called.append("margin"))
    kw = dict(maxIter=3, stepSize=0.05, seed=1)
    # lineage rows: nothing resident, every row regenerated
    lin = s.synthetic.classification(3000, D, resident_fraction=0.0)
    assert type(lin.column_data("features")).__name__ == "LineageVectorColumn"
    assert _fm._kernel_rows(lin, "features", 8) is None
    CL.FMClassifier(**kw).fit(lin).transform(lin)
    assert "probability" in model.transform(lin).columns
    # sparse rows
    dense = cls_df.column_data("features").dense()[:2000].float().cpu().numpy()
    dense[np.abs(dense) < 1.0] = 0.0
    rows, cols = np.nonzero(dense)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=2000))])
    sp = C.SparseVectorColumn(torch.from_numpy(indptr.astype(np.int64)).to(s.device),
                              torch.from_numpy(cols.astype(np.int32)).to(s.device),
                              torch.from_numpy(dense[rows, cols]).to(s.device), D)
    sdf = DataFrame(s, OrderedDict(features=sp, label=C.NumericColumn(cls_df.column_data("label").data[:2000])), 2000)
    assert _fm._kernel_rows(sdf, "features", 8) is None
    CL.FMClassifier(**kw).fit(sdf).transform(sdf)
    assert "probability" in model.transform(sdf).columns
    # more factors than the kernel takes
    assert _fm._kernel_rows(cls_df, "features", 31) is None and _fm._kernel_rows(cls_df, "features", 30) is not None
    CL.FMClassifier(factorSize=31, **kw).fit(cls_df).transform(cls_df)
    assert not called
    # a CPU session
    c = Session(SessionConf().set("o3s.device", "cpu"))
    cpu_df, _ = _frames(c)
    CL.FMClassifier(**kw).fit(cpu_df).transform(cpu_df)
    assert not called

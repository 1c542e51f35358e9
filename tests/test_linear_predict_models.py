"""Multinomial LogisticRegression, NaiveBayes and PCA ``transform`` on the linear scoring
kernel against their torch paths (``O3S_LINEAR_PREDICT_FUSED=0``): the same columns, values
within the kernel test's bar of the fp64 oracle on the stored rows, equal predictions outside
the near-tie rows; thresholds, unnamed columns, the inputs that keep the torch path, and the
memory the fused path adds."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.frame import column as C
from orange3_spark_amd.frame.dataframe import DataFrame
from orange3_spark_amd.ml import classification as CLS
from orange3_spark_amd.ml import feature as FT
from orange3_spark_amd.ops import linear_predict as LP

U = 2.0 ** -24
N, D = 20_000, 24
SWITCH = "O3S_LINEAR_PREDICT_FUSED"
NAMES = ("rawPrediction", "probability", "prediction", "pca")


def _frame(s, X, y=None):
    cols = OrderedDict(features=FT.to_vector_column(s, X.to(s.device)))
    if y is not None:
        cols["label"] = C.NumericColumn(y.to(s.device))
    return DataFrame(s, cols, X.shape[0])


def _data(s):
    """(real-valued frame with a 3-class label, counts, 0/1 bits, 48-column frame, 2-class)."""
    rng = np.random.default_rng(21)
    Xr = rng.normal(size=(N, D)) * rng.uniform(0.5, 4, D) + rng.uniform(-3, 3, D)
    score = Xr[:, :3] @ rng.normal(size=(3, 3)) + rng.normal(size=(N, 3))
    y3 = torch.from_numpy(score.argmax(1).astype(np.float64))
    lam = np.where(y3.numpy()[:, None] == np.arange(D)[None, :] % 3, 5.0, 2.0)
    counts = rng.poisson(lam).astype(np.float64)
    wide = rng.normal(size=(N, 48)) * rng.uniform(0.5, 4, 48)
    t = torch.from_numpy
    return (_frame(s, t(Xr), y3), _frame(s, t(counts), y3), _frame(s, t((counts > 2).astype(np.float64)), y3),
            _frame(s, t(wide)), _frame(s, t(Xr), (y3 > 0).double()))


def _columns(out):
    return {k: out.column_data(k).data for k in NAMES if k in out.columns}


def _both(model, df, monkeypatch):
    """transform with the kernel (which must be taken) and with the switch off (never)."""
    calls = []
    real = LP.linear_predict
    monkeypatch.setattr(LP, "linear_predict", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    monkeypatch.delenv(SWITCH, raising=False)
    on = model.transform(df)
    assert len(calls) == 1, type(model).__name__
    monkeypatch.setenv(SWITCH, "0")
    off = model.transform(df)
    assert len(calls) == 1
    monkeypatch.delenv(SWITCH, raising=False)
    monkeypatch.setattr(LP, "linear_predict", real)
    assert on.columns == off.columns
    return _columns(on), _columns(off), calls[0]


def _oracle(model, df):
    """fp64 (raw, prob) on the stored rows and their bars (see test_linear_predict_kernel)."""
    col = df.column_data("features")
    S, d = col.data.cpu(), col.size
    if isinstance(model, FT.PCAModel):
        W, b, lsm = model._pc.T, None, False
    else:
        (_, make, lsm) = model._linear_spec()
        W, b = make()
    p = LP.pack(W, b)
    margins = LP.linear_predict_torch(S, d, p)[0]
    M = S[:, :d].float() @ torch.from_numpy(p.W).float().T + torch.from_numpy(p.b).float()
    if isinstance(model, FT.PCAModel):
        oracle, yard = (margins,), (M,)
    else:
        oracle = LP.linear_predict_torch(S, d, p, raw=True, prob=True, log_softmax_raw=lsm)[:2]
        yard = (M - torch.logsumexp(M, 1, keepdim=True) if lsm else M, torch.softmax(M, 1))
    bars = tuple(4 * max(float((q.double() - o).abs().max()), U * float(o.abs().max())) for o, q in zip(oracle, yard))
    return oracle[0], oracle[-1], margins, (bars[0], bars[-1])


def _compare(model, df, monkeypatch):
    on, off, kw = _both(model, df, monkeypatch)
    assert set(on) == set(off) and on
    o_raw, o_prob, margins, (bar_raw, bar_prob) = _oracle(model, df)
    for k in on:
        assert on[k].shape == off[k].shape and on[k].dtype == off[k].dtype == torch.float64, k
    name = type(model).__name__
    if "pca" in on:
        err, err_off = (float((t.cpu() - o_raw).abs().max()) for t in (on["pca"], off["pca"]))
        print(f"{name} k={o_raw.shape[1]}: error / bar {err / bar_raw:.3f} (torch path {err_off / bar_raw:.3f})")
        assert err <= bar_raw
        return on
    e_raw = float((on["rawPrediction"].cpu() - o_raw).abs().max())
    e_prob = float((on["probability"].cpu() - o_prob).abs().max())
    top = margins.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 2 * bar_raw
    left_out = 1.0 - float(clear.double().mean())
    print(f"{name}: error / bar raw {e_raw / bar_raw:.3f}, prob {e_prob / bar_prob:.3f} (torch path raw "
          f"{float((off['rawPrediction'].cpu() - o_raw).abs().max()) / bar_raw:.3f}); pred rows left out "
          f"{100 * left_out:.2f} %")
    assert e_raw <= bar_raw and e_prob <= bar_prob
    assert left_out <= 0.01
    a, b = on["prediction"].cpu(), off["prediction"].cpu()
    assert torch.equal(a[clear], b[clear]) and torch.equal(a[clear], margins.argmax(1).double()[clear])
    return on


def _check_session(s, monkeypatch):
    real, counts, bits, wide, binary = _data(s)
    lr = CLS.LogisticRegression(family="multinomial", maxIter=8).fit(real)
    assert lr._multinomial and lr.numClasses == 3
    _compare(lr, real, monkeypatch)
    for mt, df in (("multinomial", counts), ("complement", counts), ("bernoulli", bits)):
        _compare(CLS.NaiveBayes(modelType=mt).fit(df), df, monkeypatch)
    out = _compare(FT.PCA(k=5, inputCol="features", outputCol="pca").fit(real), real, monkeypatch)
    assert out["pca"].shape == (N, 5)
    out = _compare(FT.PCA(k=40, inputCol="features", outputCol="pca").fit(wide), wide, monkeypatch)
    assert out["pca"].shape == (N, 40)
    # a two-class multinomial model: its threshold is applied to the kernel's probabilities
    lr2 = CLS.LogisticRegression(family="multinomial", maxIter=5).fit(binary)
    assert lr2._multinomial and lr2.numClasses == 2
    on, off, kw = _both(lr2, binary, monkeypatch)
    assert kw["prob"] and not kw["pred"]
    assert torch.equal(on["prediction"], (on["probability"][:, 1] > 0.5).double())
    assert float((on["prediction"] != off["prediction"]).double().mean()) <= 0.01
    return lr, real, counts


@pytest.mark.gpu
def test_fused_transform_matches_the_torch_path_bf16(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    lr, real, counts = _check_session(s, monkeypatch)
    assert real.column_data("features").data.dtype == torch.bfloat16


@pytest.mark.gpu
def test_fused_transform_matches_the_torch_path_fp32(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda").set("o3s.vector.dtype", "float32"))
    lr, real, counts = _check_session(s, monkeypatch)
    assert real.column_data("features").data.dtype == torch.float32


@pytest.mark.gpu
def test_thresholds_and_unnamed_columns(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    real, counts = _data(s)[:2]
    for m, df in ((CLS.LogisticRegression(family="multinomial", maxIter=5).fit(real), real),
                  (CLS.NaiveBayes().fit(counts), counts)):
        m._set(thresholds=[0.1, 0.8, 0.3])
        on, off, kw = _both(m, df, monkeypatch)
        assert kw["prob"] and not kw["pred"] and kw["raw"]
        assert torch.equal(on["prediction"], m._prob2pred(on["probability"]))
        assert float((on["prediction"] != off["prediction"]).double().mean()) <= 0.01
        assert not torch.equal(on["prediction"], on["probability"].argmax(1).double())      # the thresholds matter
        m.clear(m.thresholds)
        m._set(rawPredictionCol="", probabilityCol="")
        on, off, kw = _both(m, df, monkeypatch)
        assert set(on) == set(off) == {"prediction"}
        assert not kw["raw"] and not kw["prob"] and kw["pred"]
        assert float((on["prediction"] != off["prediction"]).double().mean()) <= 0.01
        m._set(predictionCol="")
        assert m.transform(df).columns == df.columns


@pytest.mark.gpu
def test_gaussian_lineage_and_sparse_inputs_keep_the_torch_path(monkeypatch):
    s = Session(SessionConf().set("o3s.device", "cuda"))
    real, counts, _, _, binary = _data(s)
    called = []
    monkeypatch.setattr(LP, "linear_predict", lambda *a, **k: called.append(1))

    def same(model, df):
        monkeypatch.delenv(SWITCH, raising=False)
        on = _columns(model.transform(df))
        monkeypatch.setenv(SWITCH, "0")
        off = _columns(model.transform(df))
        monkeypatch.delenv(SWITCH, raising=False)
        assert set(on) == set(off) and on
        for k in on:
            assert torch.equal(on[k], off[k]), (type(model).__name__, k)

    same(CLS.NaiveBayes(modelType="gaussian").fit(real), real)
    # lineage rows: nothing resident, every row regenerated
    lin = s.synthetic.classification(3000, D, resident_fraction=0.0)
    assert type(lin.column_data("features")).__name__ == "LineageVectorColumn"
    same(CLS.LogisticRegression(family="multinomial", maxIter=3).fit(binary), lin)
    same(FT.PCA(k=3, inputCol="features", outputCol="pca").fit(real), lin)
    # sparse counts
    dense = counts.column_data("features").dense()[:2000].float().cpu().numpy()
    rows, cols = np.nonzero(dense)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=2000))])
    sp = C.SparseVectorColumn(torch.from_numpy(indptr.astype(np.int64)).to(s.device),
                              torch.from_numpy(cols.astype(np.int32)).to(s.device),
                              torch.from_numpy(dense[rows, cols]).to(s.device), D)
    sdf = DataFrame(s, OrderedDict(features=sp), 2000)
    same(CLS.NaiveBayes().fit(counts), sdf)
    assert not called


@pytest.mark.gpu
def test_fused_transform_makes_no_converted_copy_of_the_table(gpu):
    """400 000 x 256 bf16 rows (205 MB): the transform of a 4-class multinomial model (72 B of
    outputs per row) and of PCA(k=8) (64 B per row) raises the peak allocation by less than
    half the table's bytes; the torch paths add an fp32 (2x) and an fp64 (4x) copy."""
    s = Session(SessionConf().set("o3s.device", "cuda"))
    n, d = 400_000, 256
    rng = np.random.default_rng(0)
    X = torch.randn((n, d), device=s.device).to(torch.bfloat16)
    table = X.element_size() * X.numel()
    lr = CLS.LogisticRegressionModel._from(rng.normal(size=(4, d)) / 16, rng.normal(size=4), True, 4)
    pca = FT.PCAModel()
    pca._pc = np.linalg.qr(rng.normal(size=(d, 8)))[0]
    pca._set(inputCol="features", outputCol="pca")
    df = DataFrame(s, OrderedDict(features=C.VectorColumn(X)), n)
    small = DataFrame(s, OrderedDict(features=C.VectorColumn(X[:64])), 64)
    for m, names in ((lr, ("rawPrediction", "probability", "prediction")), (pca, ("pca",))):
        m.transform(small)                                   # operands packed and uploaded
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(s.device)
        before = torch.cuda.memory_allocated(s.device)
        out = m.transform(df)
        torch.cuda.synchronize()
        added = torch.cuda.max_memory_allocated(s.device) - before
        print(f"{type(m).__name__}: table {table / 2**20:.0f} MB, transform peak above baseline "
              f"{added / 2**20:.1f} MB")
        assert added < table / 2
        assert all(k in out.columns for k in names)
        got = out.column_data(names[0]).data[:4096].cpu()
        W, b = (lr._B, lr._b) if m is lr else (pca._pc.T, np.zeros(8))
        Xs = X[:4096].cpu()
        want = LP.linear_predict_torch(Xs, d, LP.pack(W, b))[0]
        # 3 MFMAs x 16 steps and the bias: 50 fp32 roundings of partial sums below sum |x w| + |b|
        size = float((Xs.double().abs() @ torch.from_numpy(np.abs(W)).T + torch.from_numpy(np.abs(b))).max())
        assert float((got - want).abs().max()) <= 50 * U * size
        del out

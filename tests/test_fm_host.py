"""The host side of the fused factorization-machine path on the CPU: the fp64 references of
``ops/fm.py`` against autograd of the torch program, the fused objective against the autograd
objective through ``gradient_descent``, and the gate of the kernels."""
import numpy as np
import pandas as pd
import pytest
import torch

from orange3_spark_amd import Session, SessionConf
from orange3_spark_amd.ml import _fm
from orange3_spark_amd.ml import classification as CL
from orange3_spark_amd.ml import regression as RG
from orange3_spark_amd.ml.feature import VectorAssembler
from orange3_spark_amd.ops import fm as FM
from orange3_spark_amd.ops.glm import LOSS_LOGISTIC, LOSS_SQUARED


@pytest.fixture(scope="module")
def session():
    return Session(SessionConf().set("o3s.device", "cpu"))


def _problem(n=300, d=7, F=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((n, d), generator=g, dtype=torch.float64)
    theta = torch.randn(d * F + d + 1, generator=g, dtype=torch.float64) * 0.4
    yb = (torch.rand(n, generator=g, dtype=torch.float64) < 0.4).double()
    yr = torch.randn(n, generator=g, dtype=torch.float64)
    sw = torch.rand(n, generator=g, dtype=torch.float64) + 0.5
    return X, theta, yb, yr, sw


def _autograd(X, y, sw, theta, mask, d, F, loss):
    th = theta.clone().requires_grad_(True)
    m = _fm.fm_forward(th * mask, X, d, F)                      # local_loss of _fit_fm
    l = torch.nn.functional.softplus(m) - y * m if loss == LOSS_LOGISTIC else 0.5 * (m - y) ** 2
    total = (l if sw is None else l * sw).sum()
    g, = torch.autograd.grad(total, th)
    return total.detach(), g


@pytest.mark.parametrize("loss", [LOSS_LOGISTIC, LOSS_SQUARED])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fit_linear,fit_intercept", [(True, True), (False, True), (True, False), (False, False)])
def test_pass_reference_equals_autograd(loss, weighted, fit_linear, fit_intercept):
    d, F = 7, 3
    X, theta, yb, yr, sw = _problem(d=d, F=F)
    y = yb if loss == LOSS_LOGISTIC else yr
    sw = sw if weighted else None
    mask = torch.ones_like(theta)
    if not fit_linear:
        mask[d * F: d * F + d] = 0
    if not fit_intercept:
        mask[-1] = 0
    want_l, want_g = _autograd(X, y, sw, theta, mask, d, F, loss)
    th = theta * mask
    gV, gw, gw0, l = FM.fm_pass_torch(X, y, sw, th[: d * F].reshape(d, F), th[d * F: d * F + d], th[-1], loss)
    got_g = torch.cat([gV.reshape(-1), gw, gw0.reshape(1)]) * mask
    assert gV.shape == (d, F) and gw.shape == (d,) and gw0.shape == () and l.shape == ()
    assert float((got_g - want_g).abs().max()) <= 1e-10 * float(want_g.abs().max())
    assert abs(float(l - want_l)) <= 1e-10 * abs(float(want_l))
    if not fit_linear:
        assert float(got_g[d * F: d * F + d].abs().max()) == 0.0
    if not fit_intercept:
        assert float(got_g[-1]) == 0.0


def test_margin_reference_equals_fm_forward():
    d, F = 7, 3
    X, theta, *_ = _problem(d=d, F=F)
    want = _fm.fm_forward(theta, X, d, F)
    got = FM.fm_margin_torch(X, theta[: d * F].reshape(d, F), theta[d * F: d * F + d], float(theta[-1]))
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # a 0-d tensor for w0, and bf16 rows
    Xb = X.to(torch.bfloat16)
    got = FM.fm_margin_torch(Xb, theta[: d * F].reshape(d, F), theta[d * F: d * F + d], theta[-1])
    assert float((got - _fm.fm_forward(theta, Xb.double(), d, F)).abs().max()) <= 1e-12 * float(want.abs().max())


def _frame(session, X, **cols):
    pdf = pd.DataFrame(X, columns=[f"f{i}" for i in range(X.shape[1])])
    for k, v in cols.items():
        pdf[k] = v
    return VectorAssembler(inputCols=[f"f{i}" for i in range(X.shape[1])], outputCol="features").transform(
        session.createDataFrame(pdf))


def _frames(session, n):
    rng = np.random.default_rng(1)
    X = rng.normal(0, 1, (n, 4))
    yb = ((X[:, 0] * X[:, 1] + 0.5 * X[:, 2]) > 0).astype(float)
    yr = X[:, 0] * X[:, 1] + 0.3 * X[:, 3]
    sw = rng.uniform(0.5, 1.5, n)
    return _frame(session, X, label=yb, weight=sw), _frame(session, X, label=yr, weight=sw)


@pytest.fixture(scope="module")
def frames(session):
    """The data of test_fm_classifier_and_regressor: 800 x 4, a pairwise label."""
    return _frames(session, 800)


@pytest.fixture(scope="module")
def frames5k(session):
    """The same recipe with 5000 rows: five 1024-row chunks for a mini-batch to choose from
    (the 800 rows are one chunk, which every mini-batch then takes whole)."""
    return _frames(session, 5000)


@pytest.mark.parametrize("kind,n,kw", [
    ("classifier", 800, {}),
    ("regressor", 800, {}),
    ("classifier", 800, {"miniBatchFraction": 0.5}),
    ("classifier", 5000, {"miniBatchFraction": 0.5}),
    ("regressor", 5000, {"miniBatchFraction": 0.5, "solver": "gd", "regParam": 0.01, "weightCol": "weight"}),
    ("classifier", 800, {"fitLinear": False, "regParam": 0.05}),
    ("regressor", 800, {"fitIntercept": False, "weightCol": "weight"}),
])
def test_fused_objective_reproduces_the_autograd_fit(frames, frames5k, kind, n, kw):
    """gradient_descent over the fused objective (fm_pass_torch in place of the kernel) and
    over the autograd objective: the same parts, the same seed, history and theta to 1e-9."""
    cls = kind == "classifier"
    kw = dict(kw)
    df = (frames if n == 800 else frames5k)[0 if cls else 1]
    weight = kw.pop("weightCol", None)
    est = (CL.FMClassifier if cls else RG.FMRegressor)(stepSize=0.05, maxIter=60, seed=3, factorSize=4, **kw)
    if weight:
        est._set(weightCol=weight)
    calls = []

    def counted(*a):
        calls.append(a[0].shape[0])
        return FM.fm_pass_torch(*a)

    V0, w0, b0, r0 = _fm._fit_fm(est, df, cls)
    V1, w1, b1, r1 = _fm._fit_fm(est, df, cls, pass_fn=counted)
    assert r0.iterations == r1.iterations == len(r1.history) > 5
    np.testing.assert_allclose(r1.history, r0.history, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(r1.x, r0.x, rtol=0, atol=1e-9 * np.abs(r0.x).max())
    np.testing.assert_allclose(V1, V0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(w1, w0, rtol=0, atol=1e-9)
    assert abs(b1 - b0) <= 1e-9
    if n > 800:
        assert len(calls) > r1.iterations and max(calls) == 1024     # one pass per selected chunk
    else:
        assert calls == [800] * r1.iterations                        # the full batch, or its one chunk: one pass
    if kw.get("fitLinear") is False:
        assert not w1.any()
    if kw.get("fitIntercept") is False:
        assert b1 == 0.0


def test_cpu_session_keeps_the_torch_program(frames, monkeypatch):
    called = []
    monkeypatch.setattr(FM, "fm_pass", lambda *a, **k: called.append(1))
    monkeypatch.setattr(FM, "fm_margin", lambda *a, **k: called.append(1))
    m = CL.FMClassifier(stepSize=0.05, maxIter=5, seed=3, factorSize=4).fit(frames[0])
    out = m.transform(frames[0])
    assert "probability" in out.columns and not called
    assert _fm._kernel_rows(frames[0], "features", 4) is None


def test_gate():
    ok = dict(is_cuda=True, dtype=torch.bfloat16, row_stride=256, col_stride=1, d=256, F=8)
    assert FM.gate_reason(**ok) is None
    assert FM.gate_reason(**{**ok, "dtype": torch.float32, "row_stride": 24, "d": 20, "F": 30}) is None
    assert FM.gate_reason(**{**ok, "F": 1, "d": 1, "row_stride": 8}) is None
    for bad in ({"d": 257, "row_stride": 264}, {"F": 31}, {"F": 0}, {"row_stride": 12, "d": 12}, {"is_cuda": False},
                {"dtype": torch.float64}, {"col_stride": 2}, {"d": 0}):
        assert FM.gate_reason(**{**ok, **bad}) is not None, bad
    # the tensors themselves: CPU rows and fp64 rows are refused whatever their shape
    assert not FM.fm_kernel_ok(torch.zeros((4, 256), dtype=torch.bfloat16), 8)
    assert not FM.fm_kernel_ok(torch.zeros((4, 256), dtype=torch.float64), 8)
    assert not FM.fm_kernel_ok(torch.zeros((4, 257)), 8)
    assert not FM.fm_kernel_ok(torch.zeros((4, 12)), 8)
    assert not FM.fm_kernel_ok(torch.zeros((4, 16)), 31)
    assert not FM.fm_kernel_ok(torch.zeros((4, 16)), 0)
    assert not FM.fm_kernel_ok(torch.zeros(16), 8)
    with pytest.raises(ValueError):
        FM.fm_pass(torch.zeros((4, 16)), torch.zeros(4), None, torch.zeros((16, 2)), torch.zeros(16), 0.0, LOSS_LOGISTIC)
    with pytest.raises(ValueError):
        FM.fm_pass_torch(torch.zeros((4, 16)), torch.zeros(4), None, torch.zeros((16, 2)), torch.zeros(16), 0.0, 1)


def test_switch_is_read_per_call(monkeypatch):
    monkeypatch.setenv("O3S_FM_KERNEL", "0")
    assert not FM.fm_enabled()
    monkeypatch.setenv("O3S_FM_KERNEL", "1")
    assert FM.fm_enabled()

"""fp32 feature rows through the fused GLM kernels (csrc/glm_mixed.hip and csrc/glm_stats.hip, the ``*_f32`` kernels) vs
fp64 PyTorch references.

The inputs are deliberately NOT representable in bf16 (normal values around 10), and the
storage checks assert that a path which rounded the rows to bf16 on the way would fail.
Tolerances are those of the bf16 tests in test_glm_kernels.py named in each test: the
accumulation arithmetic is the same fp32.
"""
import functools

import numpy as np
import pytest
import torch

from orange3_spark_amd.ops import glm as G

N = 30001


@functools.lru_cache(maxsize=None)
def _rows(n, d, seed=0):
    """(X fp32 [n, padded_width(d)] with zero pad columns, y in {0, 1}, weights), host."""
    g = torch.Generator().manual_seed(1000 * seed + d + n)
    ld = G.padded_width(d)
    X = torch.zeros((n, ld), dtype=torch.float32)
    X[:, :d] = torch.randn((n, d), generator=g) * 3 + 10
    y = (torch.rand(n, generator=g) < 0.5).float()
    sw = torch.rand(n, generator=g) + 0.25
    return X, y, sw


def _coef(ld, seed=1, scale=0.05):
    return torch.randn(ld, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _storage_case():
    """d = 256 squared-loss pass near its optimum (labels = the model's own margins + unit
    noise): the gradient is small, so what bf16 rounding of the rows does to it stands well
    above the tolerance of the gradient assertions.  (X, y, coef, fp64 reference over the
    exact rows, fp64 reference over the bf16-rounded rows.)"""
    X, _, _ = _rows(N, 256)
    coef = _coef(256)
    g = torch.Generator().manual_seed(77)
    y = (X.double() @ coef.double() - 0.2 + torch.randn(N, generator=g).double()).float()
    ref = G.glm_grad_torch(X, y, None, coef.double(), -0.2, 2)
    refb = G.glm_grad_torch(X.bfloat16(), y, None, coef.double(), -0.2, 2)
    return X, y, coef, ref, refb


def _assert_grad(out, ref, ld, n):
    """The assertions of test_glm_kernels.test_gpu_grad_matches_fp64."""
    dpad, _ = G.layout(ld)
    scale = ref[:ld].abs().max().item() + 1.0
    assert (out[:ld] - ref[:ld]).abs().max().item() < 2e-4 * scale * (n ** 0.5) / 50
    assert abs(out[dpad] - ref[ld]) < 1e-3 * (abs(ref[ld].item()) + 10)
    assert abs(out[dpad + 1] - ref[ld + 1]) < 1e-4 * abs(ref[ld + 1].item()) + 1e-2
    assert abs(out[dpad + 2] - ref[ld + 2]) < 1e-3


# ------------------------------------------------------------------------------ CPU
def test_cpu_paths_accept_fp32_as_before():
    X, y, sw = _rows(300, 20)
    ld = X.shape[1]
    coef = _coef(ld)
    dpad, _ = G.layout(ld)
    for loss in (0, 1, 2):
        out = G.glm_grad(X, y, sw, coef, 0.3, loss)
        ref = G.glm_grad_torch(X, y, sw, coef.double(), 0.3, loss)
        assert torch.allclose(out[:ld], ref[:ld]) and torch.allclose(out[dpad:], ref[ld:])
    ws = G.GlmWorkspace("cpu", ld)
    mixed = G.glm_grad_mixed(X, y, sw, 0, 20, 0, 0, coef, 0.3, 0, ws)
    assert torch.allclose(mixed, G.glm_grad(X, y, sw, coef, 0.3, 0))
    m = G.glm_margin(X, coef, 0.5)
    assert m.dtype == torch.float32 and torch.allclose(m.double(), X.double() @ coef.double() + 0.5, atol=1e-5)
    cs = G.glm_colstats(X, sw)
    assert torch.allclose(cs[:ld], sw.double() @ X.double())
    st = G.glm_stats_mixed(X, y, sw, 0, 20, 0, 0)
    assert torch.equal(st, G.glm_stats_torch(X, y, sw))
    assert not G.f32_rows(X) and not G.kernel_rows(X)        # CPU rows never go to the kernels


def test_cpu_storage_check_is_meaningful():
    """The two fp64 references of the d = 256 storage check (exact rows, bf16-rounded rows)
    differ by far more than the gradient tolerance, and bf16-rounded rows break the margin
    bound: a kernel path that rounded to bf16 could not pass either GPU test."""
    X, y, coef, ref, refb = _storage_case()
    ld = X.shape[1]
    tol = 2e-4 * (ref[:ld].abs().max().item() + 1.0) * (N ** 0.5) / 50
    assert (refb[:ld] - ref[:ld]).abs().max().item() > 20 * tol
    Xm, _, _ = _rows(10007, 256)
    cm = torch.randn(256, generator=torch.Generator().manual_seed(3))
    exact = Xm.double() @ cm.double() + 0.5
    rounded = Xm.bfloat16().double() @ cm.double() + 0.5
    assert not torch.allclose(rounded, exact, atol=1e-3, rtol=1e-4)
    assert ((rounded - exact).abs() > 1e-3 + 1e-4 * exact.abs()).float().mean().item() > 0.9


# ------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("d", [8, 20, 256, 520, 1024, 2056, 4104])
@pytest.mark.parametrize("loss", [0, 1, 2])
def test_gpu_grad_f32_matches_fp64(gpu, d, loss):
    """(d = 2056 / 4104: the 8 and 16 chunks-per-lane layouts, fewer rows.)"""
    n = N if d <= 1024 else 3001
    X, y, sw = _rows(n, d)
    ld = X.shape[1]
    coef = _coef(ld, scale=0.05 if d <= 1024 else 0.01)
    sw = sw if loss == 0 else None
    out = G.glm_grad(X.to(gpu), y.to(gpu), None if sw is None else sw.to(gpu), coef.to(gpu), -0.2, loss).cpu()
    ref = G.glm_grad_torch(X, y, sw, coef.double(), -0.2, loss)
    assert out.shape[0] == G.layout(ld)[0] + 3
    _assert_grad(out, ref, ld, n)
    assert torch.equal(out[d:G.layout(ld)[0]], torch.zeros(G.layout(ld)[0] - d, dtype=torch.float64))


@pytest.mark.gpu
def test_gpu_grad_f32_keeps_fp32_storage(gpu):
    """d = 256, squared loss: the kernel result is more than 10x closer to the fp64 pass over
    the exact rows than to the fp64 pass over the rows rounded to bf16."""
    X, y, coef, ref, refb = _storage_case()
    ld = X.shape[1]
    out = G.glm_grad(X.to(gpu), y.to(gpu), None, coef.to(gpu), -0.2, 2).cpu()
    _assert_grad(out, ref, ld, N)
    near = (out[:ld] - ref[:ld]).abs().max().item()
    far = (out[:ld] - refb[:ld]).abs().max().item()
    assert far > 10 * near, (near, far)


@pytest.mark.gpu
@pytest.mark.parametrize("d,loss", [(256, 0), (256, 1), (256, 2), (20, 0), (100, 0), (600, 0)])
def test_gpu_grad_mixed_f32_matches_fp64(gpu, d, loss):
    """glm_grad_mixed with fp32 rows and no lineage rows, checked as
    test_gpu_grad_mixed_matches_fp64."""
    X, y, sw = _rows(30011, d)
    ld = X.shape[1]
    coef = _coef(ld, seed=4).to(gpu)
    ws = G.GlmWorkspace(gpu, ld, grid=96)
    Xg, yg, swg = X.to(gpu), y.to(gpu), sw.to(gpu)
    out = G.glm_grad_mixed(Xg, yg, swg, 0, d, 0, 0, coef, 0.1, loss, ws).clone().cpu()
    ref = G.glm_grad_torch(X, y, sw, coef.double().cpu(), 0.1, loss)
    dpad = ws.dpad
    assert torch.allclose(out[:ld], ref[:ld], rtol=1e-3, atol=0.05), (out[:ld] - ref[:ld]).abs().max()
    assert torch.allclose(out[dpad:], ref[ld:], rtol=1e-3, atol=0.5)
    again = G.glm_grad_mixed(Xg, yg, swg, 0, d, 0, 0, coef, 0.1, loss, ws).clone().cpu()
    assert torch.equal(out, again)                      # deterministic slab reduction


@pytest.mark.gpu
@pytest.mark.parametrize("slice_rows", [7000, 30000])
@pytest.mark.parametrize("frac", [1.0, 0.3])
def test_gpu_grad_mixed_f32_split_launches_agree(gpu, slice_rows, frac, monkeypatch):
    """Checked as test_gpu_grad_mixed_split_launches_agree."""
    n, d = 70020, 256
    X, y, _ = _rows(n, d)
    Xg, yg = X.to(gpu), y.to(gpu)
    coef = _coef(d, seed=2).to(gpu)
    ws = G.GlmWorkspace(gpu, d, grid=512)
    kw = dict(res_row0=123, sample_seed=9, fraction=frac)
    monkeypatch.setattr(G, "MIX_SLICE_ROWS", 1 << 40)
    ref = G.glm_grad_mixed(Xg, yg, None, 0, d, 0, 0, coef, -0.2, 0, ws, **kw).clone()
    monkeypatch.setattr(G, "MIX_SLICE_ROWS", slice_rows)
    assert G.mix_splits(n) > 1
    out = G.glm_grad_mixed(Xg, yg, None, 0, d, 0, 0, coef, -0.2, 0, ws, **kw).clone()
    again = G.glm_grad_mixed(Xg, yg, None, 0, d, 0, 0, coef, -0.2, 0, ws, **kw).clone()
    assert torch.equal(out, again)
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("frac", [0.3, 0.05])
def test_gpu_grad_mixed_f32_minibatch_matches_cpu_mask(gpu, frac):
    """Checked as test_gpu_grad_mixed_minibatch_matches_cpu_mask."""
    n, d = 60020, 256
    X, y, _ = _rows(n, d)
    coef = _coef(d, seed=2)
    ws = G.GlmWorkspace(gpu, d, grid=512)
    t_dev = torch.tensor([4], dtype=torch.int64, device=gpu)          # iteration 5
    out = G.glm_grad_mixed(X.to(gpu), y.to(gpu), None, 0, d, 0, 0, coef.to(gpu), 0.1, 0, ws,
                           res_row0=5_000_000, t_dev=t_dev, sample_seed=99, fraction=frac).clone().cpu()
    keep = G.sample_mask(99, 5, torch.arange(5_000_000, 5_000_000 + n), frac).double()
    ref = G.glm_grad_torch(X, y, keep, coef.double(), 0.1, 0)
    assert abs(out[d + 2].item() - keep.sum().item()) < 0.5           # identical kept set
    assert torch.allclose(out[:d], ref[:d], rtol=1e-3, atol=0.05)
    assert torch.allclose(out[d:], ref[d:], rtol=1e-3, atol=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("d,weighted", [(256, False), (256, True), (20, False), (20, True), (100, False),
                                        (100, True), (600, False), (600, True), (2048, False), (2048, True)])
def test_gpu_stats_f32_matches_fp64(gpu, d, weighted):
    """Checked as test_gpu_stats_mixed_matches_fp64."""
    X, y, sw = _rows(30011 if d < 2048 else 8009, d)
    ld = X.shape[1]
    sw = sw if weighted else None
    Xg, yg, swg = X.to(gpu), y.to(gpu), None if sw is None else sw.to(gpu)
    out = G.glm_stats_mixed(Xg, yg, swg, 0, d, 0, 0)
    assert out is not None
    out = out.cpu()
    ref = G.glm_stats_torch(X, y, sw)
    dpad, _ = G.layout(ld)
    for k in range(3):
        a, b = out[k * dpad:k * dpad + ld], ref[k * dpad:k * dpad + ld]
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5 * (1 + b.abs().max().item())), (k, (a - b).abs().max())
    assert torch.allclose(out[3 * dpad:], ref[3 * dpad:], rtol=1e-6)
    assert torch.equal(out, G.glm_stats_mixed(Xg, yg, swg, 0, d, 0, 0).cpu())


@pytest.mark.gpu
def test_gpu_stats_f32_wide_rows_have_no_fused_pass(gpu):
    """ld > 2048 keeps the "no instantiation" answer of the bf16 entry point."""
    X = torch.ones((33, 2056), dtype=torch.float32, device=gpu)
    assert G.glm_stats_mixed(X, torch.ones(33, device=gpu), None, 0, 2056, 0, 0) is None


@pytest.mark.gpu
@pytest.mark.parametrize("d,weighted", [(20, True), (256, False), (600, True), (2056, False), (4104, True)])
def test_gpu_colstats_f32_matches_fp64(gpu, d, weighted):
    X, _, sw = _rows(N if d <= 1024 else 3001, d)
    ld = X.shape[1]
    sw = sw if weighted else None
    out = G.glm_colstats(X.to(gpu), None if sw is None else sw.to(gpu)).cpu()
    w = torch.ones(X.shape[0], dtype=torch.float64) if sw is None else sw.double()
    Xd = X.double()
    ref = torch.cat([w @ Xd, w @ (Xd * Xd), w.sum().reshape(1)])
    assert out.shape == ref.shape
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("n,d", [(10007, 256), (1001, 20), (1001, 600), (301, 2056), (301, 4104)])
def test_gpu_margin_f32(gpu, n, d):
    """The bound of test_gpu_margin (which bf16-rounded rows miss:
    test_cpu_storage_check_is_meaningful)."""
    X, _, _ = _rows(n, d)
    ld = X.shape[1]
    coef = torch.randn(d, generator=torch.Generator().manual_seed(3)) * (1.0 if d <= 256 else 0.1)
    m = G.glm_margin(X.to(gpu), coef.to(gpu), 0.5)
    assert m.dtype == torch.float32 and m.shape == (n,)
    ref = X.double()[:, :d] @ coef.double() + 0.5
    assert torch.allclose(m.double().cpu(), ref, atol=1e-3, rtol=1e-4)
    assert ld == G.padded_width(d)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [8, 256])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17])
def test_gpu_f32_edges(gpu, n, d):
    X, y, sw = (t[:n] for t in _rows(64, d))
    coef = _coef(d)
    Xg, yg, swg = X.to(gpu), y.to(gpu), sw.to(gpu)
    ws = G.GlmWorkspace(gpu, d, grid=8)
    ref = G.glm_grad_torch(X, y, sw, coef.double(), 0.1, 0)
    for out in (G.glm_grad(Xg, yg, swg, coef.to(gpu), 0.1, 0).cpu(),
                G.glm_grad_mixed(Xg, yg, swg, 0, d, 0, 0, coef.to(gpu), 0.1, 0, ws).clone().cpu()):
        dpad = G.layout(d)[0]
        if n == 0:
            assert torch.equal(out, torch.zeros_like(out))
        else:
            assert torch.allclose(out[:d], ref[:d], rtol=1e-5, atol=1e-3)
            assert torch.allclose(out[dpad:], ref[d:], rtol=1e-5, atol=1e-3)
    st = G.glm_stats_mixed(Xg, yg, swg, 0, d, 0, 0).cpu()
    assert torch.allclose(st, G.glm_stats_torch(X, y, sw), rtol=1e-5, atol=1e-4)
    cs = G.glm_colstats(Xg, swg).cpu()
    assert torch.allclose(cs[:d], sw.double() @ X.double(), rtol=1e-5, atol=1e-4)
    m = G.glm_margin(Xg, coef.to(gpu), 0.5).cpu()
    assert m.shape == (n,)
    assert torch.allclose(m.double(), X.double() @ coef.double() + 0.5, atol=1e-3, rtol=1e-4)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_f32_rejections(gpu):
    X = torch.randn((100, 20), device=gpu)                   # row stride not a multiple of 8
    y = torch.zeros(100, device=gpu)
    coef = torch.zeros(20, device=gpu)
    with pytest.raises(TypeError):
        G.glm_grad(X, y, None, coef, 0.0, 0)
    with pytest.raises(TypeError):
        G.glm_grad(torch.randn((100, 48), device=gpu)[:, :24], y, None, coef, 0.0, 0)      # not contiguous
    ws = G.GlmWorkspace(gpu, 24)
    with pytest.raises(TypeError):
        G.glm_grad_mixed(X, y, None, 0, 20, 0, 0, coef, 0.0, 0, ws)
    X24 = torch.randn((100, 24), device=gpu)
    with pytest.raises(ValueError):
        G.glm_grad_mixed(X24, torch.zeros(150, device=gpu), None, 50, 24, 0, 100, coef, 0.0, 0, ws)
    # the torch fall-backs of the other two ops stay
    ref = X.double() @ coef.double() + 1.0
    assert torch.allclose(G.glm_margin(X, coef, 1.0).double(), ref)
    assert G.glm_colstats(X).shape == (41,)


# ------------------------------------------------------------------------------ device SGD
@pytest.mark.gpu
def test_gpu_sgd_fit_f32_matches_cpu(gpu):
    """test_gpu_sgd_fit_matches_cpu on fp32 rows: fused stats pass, graph-replayed steps and
    the in-kernel mini-batch mask over the fp32 kernels == the CPU fp64 path."""
    from collections import OrderedDict

    from orange3_spark_amd import Session, SessionConf
    from orange3_spark_amd.frame import column as Cc
    from orange3_spark_amd.frame.dataframe import DataFrame
    from orange3_spark_amd.ml.classification import LogisticRegression
    from orange3_spark_amd.models.glm import GlmData
    g = torch.Generator().manual_seed(31)
    X = torch.randn((60_000, 64), generator=g) * 0.5
    w = torch.randn(64, generator=torch.Generator().manual_seed(32)) * 0.5
    y = (X @ w + 0.1 > 0).float()                            # labels from a fixed hyperplane
    sg = Session(SessionConf().setAppName("g").set("o3s.vector.dtype", "float32"), device=gpu)
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    dg = DataFrame(sg, OrderedDict(features=Cc.VectorColumn(X.to(gpu), 64), label=Cc.NumericColumn(y.to(gpu))),
                   X.shape[0])
    dc = DataFrame(sc, OrderedDict(features=Cc.VectorColumn(X.double(), 64), label=Cc.NumericColumn(y.double())),
                   X.shape[0])
    data = GlmData(dg.comm, dg.column_data("features"), y.to(gpu))
    assert data.kernel and data.mixed and data.X.dtype == torch.float32
    for frac in (1.0, 0.2):
        kw = dict(solver="sgd", maxIter=12, tol=0.0, miniBatchFraction=frac, seed=5, regParam=0.01)
        a = LogisticRegression(**kw).fit(dg)
        b = LogisticRegression(**kw).fit(dc)
        assert np.allclose(a.coefficients.toArray(), b.coefficients.toArray(), rtol=2e-3, atol=2e-4)
        assert abs(a.intercept - b.intercept) < 2e-4
        assert a.summary.totalIterations == 12

"""The mixed GLM pass split on the host into whole tiles (mask-free kernel) and the ragged
rest (one launch of the masked kernel that adds into slab row 0): csrc/glm_mixed.hip
``o3s_glm_grad_mixed`` with ``full_tiles``, switched by ``ops.glm.MIX_FULL_TILES``.

Shapes: d = 256 is the 8x4 layout (tile = 16 rows); d = 32 the 4x1 layout (tile = 128 rows).
d = 24 and d = 100 have rows narrower than their layout (24 < 32, 104 < 128 columns) and
must stay on the masked kernel."""
from collections import OrderedDict

import pytest
import torch

from orange3_spark_amd.ops import glm as G

pytestmark = pytest.mark.gpu

SEED = 13
# bound for a pure change of fp32 block-sum order (test_gpu_grad_mixed_split_launches_agree)
ORDER = dict(rtol=1e-5, atol=1e-3)


def _rows(gpu, d, n_res, n_lin, row0=None):
    """Resident rows, the materialised twin of the lineage rows, and labels of both."""
    ld = G.padded_width(d)
    row0 = n_res if row0 is None else row0
    wt, bt = G.synth_truth(SEED, d, ld)
    Xr, yr = G.synth_glm(n_res, d, SEED + 1, device=gpu, ld=ld)
    Xl, yl = G.synth_glm(n_lin, d, SEED, row0=row0, device=gpu, ld=ld, wtrue=wt, btrue=bt)
    coef = torch.randn(ld, generator=torch.Generator().manual_seed(4)).to(gpu) * 0.05
    return ld, Xr, Xl, torch.cat([yr, 1.0 - yl]), coef


def _check_fp64(out, ref, ld, dpad):
    # the tolerances of test_gpu_grad_mixed_matches_fp64
    print("max |grad - fp64|", (out[:ld] - ref[:ld]).abs().max().item(), "tail", (out[dpad:] - ref[ld:]).abs().tolist())
    assert torch.allclose(out[:ld], ref[:ld], rtol=1e-3, atol=0.05), (out[:ld] - ref[:ld]).abs().max()
    assert torch.allclose(out[dpad:], ref[ld:], rtol=1e-3, atol=0.5)


@pytest.mark.parametrize("d,n_res,n_lin", [
    (256, 4096, 2048),      # whole tiles only: no leftover launch
    (256, 4097, 2063),      # 1 and 15 leftover rows
    (256, 5, 7),            # leftover rows only: the masked path as it was
    (256, 0, 2051),
    (256, 4099, 0),
    (32, 1000, 700),        # 4x1 layout, 128-row tiles
    (24, 1000, 700),        # 24 columns in a 32-column layout: masked path
    (100, 3001, 2007),      # 104 columns in a 128-column layout: masked path
])
def test_gpu_grad_mixed_full_tiles_match_fp64_and_masked(gpu, d, n_res, n_lin, monkeypatch):
    ld, Xr, Xl, yall, coef = _rows(gpu, d, n_res, n_lin)
    ws = G.GlmWorkspace(gpu, ld, grid=96)
    assert G.MIX_FULL_TILES == 1

    def run():
        return G.glm_grad_mixed(Xr, yall, None, n_lin, d, SEED, n_res, coef, 0.1, 0, ws).clone()
    out = run()
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, 0)
    _check_fp64(out, ref, ld, ws.dpad)
    assert torch.equal(out, run())                       # deterministic
    monkeypatch.setattr(G, "MIX_FULL_TILES", 0)
    masked = run()
    print("max |full - masked|", (out - masked).abs().max().item())
    assert torch.allclose(out, masked, **ORDER)


@pytest.mark.parametrize("loss", [1, 2])
def test_gpu_grad_mixed_full_tiles_other_losses(gpu, loss, monkeypatch):
    ld, Xr, Xl, yall, coef = _rows(gpu, 256, 4097, 2063)
    ws = G.GlmWorkspace(gpu, ld, grid=96)
    out = G.glm_grad_mixed(Xr, yall, None, 2063, 256, SEED, 4097, coef, 0.1, loss, ws).clone()
    _check_fp64(out, G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, loss), ld, ws.dpad)
    monkeypatch.setattr(G, "MIX_FULL_TILES", 0)
    assert torch.allclose(out, G.glm_grad_mixed(Xr, yall, None, 2063, 256, SEED, 4097, coef, 0.1, loss, ws), **ORDER)


@pytest.mark.parametrize("waves", [2, 3])
@pytest.mark.parametrize("mode", ["weights", "minibatch"])
def test_gpu_grad_mixed_full_tiles_sliced(gpu, mode, waves, monkeypatch):
    """Several slices whose boundaries are rounded to tiles, then the leftover launch: a
    wrong row0 / res_row0 / label offset in any of them moves the kept set or the labels."""
    n_res, n_lin, d, res_row0 = 4097, 2063, 256, 123
    ld, Xr, Xl, yall, coef = _rows(gpu, d, n_res, n_lin, row0=res_row0 + n_res)
    ws = G.GlmWorkspace(gpu, ld, grid=96)
    monkeypatch.setattr(G, "MIX_WAVES", waves)
    monkeypatch.setattr(G, "MIX_SLICE_ROWS", 1000)
    assert G.mix_splits(n_res + n_lin) == 6
    if mode == "weights":
        sw = (torch.rand(n_res + n_lin, generator=torch.Generator().manual_seed(3)) + 0.5).to(gpu)
        kw, w64 = dict(res_row0=res_row0), sw.double()
    else:
        sw = None
        kw = dict(res_row0=res_row0, t_dev=torch.tensor([4], dtype=torch.int64, device=gpu), sample_seed=99,
                  fraction=0.3)
        grows = torch.arange(res_row0, res_row0 + n_res + n_lin)
        w64 = G.sample_mask(99, 5, grows, 0.3).double().to(gpu)

    def run():
        return G.glm_grad_mixed(Xr, yall, sw, n_lin, d, SEED, res_row0 + n_res, coef, 0.1, 0, ws, **kw).clone()
    out = run()
    assert torch.equal(out, run())
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, w64, coef.double(), 0.1, 0)
    # as test_gpu_grad_mixed_minibatch_matches_cpu_mask
    print("weight sum", out[d + 2].item(), "fp64", w64.sum().item())
    if mode == "minibatch":
        assert abs(out[d + 2].item() - w64.sum().item()) < 0.5           # identical kept set
    assert torch.allclose(out[:d], ref[:d], rtol=1e-3, atol=0.05)
    assert torch.allclose(out[d:], ref[d:], rtol=1e-3, atol=0.5)
    monkeypatch.setattr(G, "MIX_FULL_TILES", 0)
    masked = run()
    print("max |full - masked|", (out - masked).abs().max().item())
    assert torch.allclose(out, masked, **ORDER)


@pytest.mark.parametrize("n_res,n_lin", [(4097, 2063), (5, 7), (4096, 2048)])
@pytest.mark.parametrize("weighted", [False, True])
def test_gpu_stats_mixed_ragged_shapes_match_fp64(gpu, n_res, n_lin, weighted, monkeypatch):
    """The summarizer pass with the same host-side split (its ragged rows write a slab row of
    their own), against fp64 and against the masked kernel alone."""
    d = 256
    ld, Xr, Xl, yall, _ = _rows(gpu, d, n_res, n_lin)
    sw = (torch.rand(n_res + n_lin, generator=torch.Generator().manual_seed(3)) + 0.5).to(gpu) if weighted else None
    out = G.glm_stats_mixed(Xr, yall, sw, n_lin, d, SEED, n_res, grid=96).cpu()
    ref = G.glm_stats_torch(torch.cat([Xr, Xl]).cpu(), yall.cpu(), None if sw is None else sw.cpu())
    dpad, _ = G.layout(ld)
    # the tolerances of test_gpu_stats_mixed_matches_fp64
    for k in range(3):
        a, b = out[k * dpad:k * dpad + ld], ref[k * dpad:k * dpad + ld]
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5 * (1 + b.abs().max().item())), (k, (a - b).abs().max())
    assert torch.allclose(out[3 * dpad:], ref[3 * dpad:], rtol=1e-6)
    assert torch.equal(out, G.glm_stats_mixed(Xr, yall, sw, n_lin, d, SEED, n_res, grid=96).cpu())
    monkeypatch.setattr(G, "MIX_FULL_TILES", 0)
    masked = G.glm_stats_mixed(Xr, yall, sw, n_lin, d, SEED, n_res, grid=96).cpu()
    print("max |full - masked|", (out - masked).abs().max().item())
    for k in range(3):
        a, b = out[k * dpad:k * dpad + ld], masked[k * dpad:k * dpad + ld]
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5 * (1 + b.abs().max().item()))
    assert torch.allclose(out[3 * dpad:], masked[3 * dpad:], rtol=1e-6)


def test_gpu_captured_sgd_fit_same_with_and_without_full_tiles(gpu, monkeypatch):
    """A graph-captured SGD fit over resident + lineage rows (3001 + 1999, both ragged): the
    captured step holds the leftover launch, and the objective history is what the masked
    kernel gives."""
    from orange3_spark_amd import Session, SessionConf
    from orange3_spark_amd.frame import column as Cc
    from orange3_spark_amd.frame.dataframe import DataFrame
    from orange3_spark_amd.ml.classification import LogisticRegression
    from orange3_spark_amd.synthetic import GlmSpec, LineageVectorColumn
    n, n_res, d, seed = 5000, 3001, 256, 7
    wt, bt = G.synth_truth(seed, d, d)
    X, y = G.synth_glm(n, d, seed, device=gpu, ld=d, wtrue=wt, btrue=bt)
    s = Session(SessionConf().setAppName("full-tiles"), device=gpu)
    feat = LineageVectorColumn(GlmSpec(seed, d, d, wt, bt), n, 0, X[:n_res].contiguous())
    assert feat.lineage_rows == n - n_res
    df = DataFrame(s, OrderedDict(features=feat, label=Cc.NumericColumn(y)), n)
    monkeypatch.setenv("O3S_SGD_GRAPH", "force")

    def fit(full):
        monkeypatch.setattr(G, "MIX_FULL_TILES", full)
        m = LogisticRegression(solver="sgd", maxIter=6, tol=0.0).fit(df)
        return torch.tensor(m.summary.objectiveHistory, dtype=torch.float64)
    on, off = fit(1), fit(0)
    print("objective", on.tolist(), "max diff", (on - off).abs().max().item())
    assert len(on) == 6 and on[-1] < on[0]
    assert torch.allclose(on, off, **ORDER)

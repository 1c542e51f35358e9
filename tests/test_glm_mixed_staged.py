"""The mixed GLM gradient pass with the resident tiles staged through a per-wave LDS slot
(csrc/glm_mixed.hip ``glm_grad_staged_kernel``, switched by ``ops.glm.MIX_STAGED``): whole tiles of
unweighted passes over d = 256 rows (the 8x4 layout, tile = 16 rows, block = 4
waves).  Every case checks the staged pass against fp64, against the unstaged mask-free pass
(another fp32 block-sum order, nothing more) and against itself: a slot overwritten before it
was read, or read before it landed, shows up as two runs that differ."""
import pytest
import torch

from orange3_spark_amd.ops import glm as G

pytestmark = pytest.mark.gpu

SEED, D = 13, 256
# bound for a pure change of fp32 block-sum order (test_glm_mixed_full_tiles.ORDER)
ORDER = dict(rtol=1e-5, atol=1e-3)


def _rows(gpu, n_res, n_lin, row0=None):
    """Resident rows, the materialised twin of the lineage rows, and labels of both."""
    row0 = n_res if row0 is None else row0
    wt, bt = G.synth_truth(SEED, D, D)
    Xr, yr = G.synth_glm(n_res, D, SEED + 1, device=gpu, ld=D)
    Xl, yl = G.synth_glm(n_lin, D, SEED, row0=row0, device=gpu, ld=D, wtrue=wt, btrue=bt)
    coef = torch.randn(D, generator=torch.Generator().manual_seed(4)).to(gpu) * 0.05
    return Xr, Xl, torch.cat([yr, 1.0 - yl]), coef


def _check_fp64(out, ref):
    # the tolerances of test_glm_mixed_full_tiles
    print("max |grad - fp64|", (out[:D] - ref[:D]).abs().max().item(), "tail", (out[D:] - ref[D:]).abs().tolist())
    assert torch.allclose(out[:D], ref[:D], rtol=1e-3, atol=0.05), (out[:D] - ref[:D]).abs().max()
    assert torch.allclose(out[D:], ref[D:], rtol=1e-3, atol=0.5)


def _three_checks(run, ref, monkeypatch):
    assert G.MIX_FULL_TILES == 1
    monkeypatch.setattr(G, "MIX_STAGED", 2)                  # 2: also a pass over one role alone
    out = run()
    _check_fp64(out, ref)
    assert torch.equal(out, run())
    monkeypatch.setattr(G, "MIX_STAGED", 0)
    plain = run()
    print("max |staged - unstaged|", (out - plain).abs().max().item())
    assert torch.allclose(out, plain, **ORDER)


@pytest.mark.parametrize("grid,n_res,n_lin", [
    (96, 4096, 2048),    # fewer tiles than waves: waves with no resident tile, no lineage tile, or neither
    (1, 64, 0),          # one tile per wave: nothing is issued after the last tile
    (1, 0, 64),
    (1, 336, 336),       # wave 0 gets one tile more than the others
    (1, 1600, 1600),     # 25 tile pairs per wave: the slot in steady state
    (2, 4800, 1600),     # 3:1, consecutive resident tiles
    (2, 1600, 4800),     # 1:3, consecutive lineage tiles: two labels with no tile batch between them
    (2, 4097, 2063),     # the leftover launch adds into slab row 0 after the staged slices
])
def test_gpu_grad_mixed_staged_matches_fp64_and_unstaged(gpu, grid, n_res, n_lin, monkeypatch):
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    ws = G.GlmWorkspace(gpu, D, grid=grid)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, 0)
    _three_checks(lambda: G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws).clone(), ref,
                  monkeypatch)


@pytest.mark.parametrize("loss", [1, 2])
def test_gpu_grad_mixed_staged_other_losses(gpu, loss, monkeypatch):
    n_res, n_lin = 4097, 2063
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    ws = G.GlmWorkspace(gpu, D, grid=2)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, loss)
    _three_checks(lambda: G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, loss, ws).clone(), ref,
                  monkeypatch)


@pytest.mark.parametrize("waves", [2, 3])
@pytest.mark.parametrize("mode", ["all_rows", "minibatch"])
def test_gpu_grad_mixed_staged_sliced(gpu, mode, waves, monkeypatch):
    """Six slices cut at tiles, then the leftover launch: a wrong row0 / res_row0 / label offset
    in any staged slice moves the lineage rows, the labels or the sampler's kept set."""
    n_res, n_lin, res_row0 = 4097, 2063, 123
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin, row0=res_row0 + n_res)
    ws = G.GlmWorkspace(gpu, D, grid=96)
    monkeypatch.setattr(G, "MIX_WAVES", waves)
    monkeypatch.setattr(G, "MIX_SLICE_ROWS", 1000)
    assert G.mix_splits(n_res + n_lin) == 6
    if mode == "all_rows":
        kw, w64 = dict(res_row0=res_row0), None
    else:
        kw = dict(res_row0=res_row0, t_dev=torch.tensor([4], dtype=torch.int64, device=gpu), sample_seed=99,
                  fraction=0.3)
        grows = torch.arange(res_row0, res_row0 + n_res + n_lin)
        w64 = G.sample_mask(99, 5, grows, 0.3).double().to(gpu)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, w64, coef.double(), 0.1, 0)

    def run():
        return G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, res_row0 + n_res, coef, 0.1, 0, ws, **kw).clone()
    _three_checks(run, ref, monkeypatch)
    if mode == "minibatch":
        monkeypatch.setattr(G, "MIX_STAGED", 2)
        out = run()
        print("weight sum", out[D + 2].item(), "fp64", w64.sum().item())
        assert abs(out[D + 2].item() - w64.sum().item()) < 0.5           # identical kept set


def test_gpu_grad_mixed_staged_leaves_weighted_passes_alone(gpu, monkeypatch):
    """A weight column keeps a pass on the unstaged kernels: the switch changes no bit."""
    n_res, n_lin, res_row0 = 4097, 2063, 123
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin, row0=res_row0 + n_res)
    ws = G.GlmWorkspace(gpu, D, grid=96)
    monkeypatch.setattr(G, "MIX_SLICE_ROWS", 1000)
    sw = (torch.rand(n_res + n_lin, generator=torch.Generator().manual_seed(3)) + 0.5).to(gpu)

    def run(staged):
        monkeypatch.setattr(G, "MIX_STAGED", staged)
        return G.glm_grad_mixed(Xr, yall, sw, n_lin, D, SEED, res_row0 + n_res, coef, 0.1, 0, ws,
                                res_row0=res_row0).clone()
    out = run(2)
    assert torch.equal(out, run(0))
    _check_fp64(out, G.glm_grad_torch(torch.cat([Xr, Xl]), yall, sw.double(), coef.double(), 0.1, 0))


@pytest.mark.parametrize("n_res,n_lin", [(1600, 0), (0, 1600)])
def test_gpu_grad_mixed_staged_default_leaves_single_role_passes_alone(gpu, n_res, n_lin, monkeypatch):
    """MIX_STAGED = 1 stages only passes that hold both roles (one role alone is slower staged)."""
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    ws = G.GlmWorkspace(gpu, D, grid=1)

    def run(staged):
        monkeypatch.setattr(G, "MIX_STAGED", staged)
        return G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws).clone()
    assert torch.equal(run(1), run(0))

"""The resident tile of ``glm_grad_staged_kernel`` (csrc/glm_mixed.hip) takes its 16 dot products on
the matrix cores: the tile out of the wave's LDS slot is the B operand of
``v_mfma_f32_16x16x32_bf16``, the coefficients, split into bf16 hi + mid + lo terms, are rows
0 - 2 of the A operand, and the lanes 0 - 15 finish the 16 rows.  What can go wrong there and
nowhere else: a k-step of the coefficient image that does not match the chunk the tile read
supplies, a dropped or misplaced term of the split, a row finished in the wrong lane (its
label, its sampler draw, its residual handed to the wrong X^T r lanes), a row counted twice or
not at all.  d = 256, ``MIX_STAGED = 2`` (single-role slices staged too), tiles of 16 rows.

Measured on one MI355X (printed by the tests; see doc/performance.md): see the docstring of
``test_gpu_staged_mfma_one_live_row_margin``."""
import math

import pytest
import torch

from orange3_spark_amd.ops import glm as G

pytestmark = pytest.mark.gpu

SEED, D, RT = 13, 256, 16
# bound for a pure change of fp32 block-sum order (test_glm_mixed_full_tiles.ORDER)
ORDER = dict(rtol=1e-5, atol=1e-3)


def _check_fp64(out, ref):
    # the tolerances of test_glm_mixed_staged._check_fp64
    print("max |grad - fp64|", (out[:D] - ref[:D]).abs().max().item(), "tail", (out[D:] - ref[D:]).abs().tolist())
    assert torch.allclose(out[:D], ref[:D], rtol=1e-3, atol=0.05), (out[:D] - ref[:D]).abs().max()
    assert torch.allclose(out[D:], ref[D:], rtol=1e-3, atol=0.5)


def _coef(scale, seed):
    """randn * scale * exp(U(-6, 0)): mixed signs, six decades with the three scales."""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(D, generator=gen) * scale * torch.exp(-6.0 * torch.rand(D, generator=gen))).float()


def _one_live_row(pos, seed):
    """A 16-row tile whose rows are zero but row ``pos``, which holds random bf16 values."""
    X = torch.zeros(RT, D, dtype=torch.bfloat16)
    X[pos] = torch.randn(D, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)
    return X


@pytest.mark.parametrize("scale", [0.05, 1.0, 30.0])
def test_gpu_staged_mfma_one_live_row_margin(gpu, scale, monkeypatch):
    """One live row at each of the 16 tile positions, squared loss, one block: the dead rows'
    residual is 0 (x = 0, y = intercept), the live row's label is 0, so out[D] is its margin.
    Bar: |margin - fp64| <= 4 x max(error of the unstaged fp32 chain on the same 16 inputs,
    2^-23 sum |x_j w_j|).

    Measured (max over the 16 positions of staged error / max(unstaged error, floor)):
    see doc/performance.md, "Mixed GLM passes: the resident tiles' dot product on MFMA"."""
    b0 = 0.25
    coef = _coef(scale, 7)
    up = (coef.to(torch.bfloat16).float() - coef) * torch.sign(coef) > 0
    assert up.any() and (~up).any()          # bf16 roundings up (negative mid term) and down
    ws = G.GlmWorkspace(gpu, D, grid=1)
    cg = coef.to(gpu)
    y = torch.full((RT,), b0)
    worst = 0.0
    for pos in range(RT):
        X = _one_live_row(pos, 100 + pos)
        yy = y.clone()
        yy[pos] = 0.0
        Xg, yg = X.to(gpu), yy.to(gpu)
        x64 = X[pos].double()
        m64 = (x64 @ coef.double()).item() + b0
        floor = 2.0 ** -23 * (x64.abs() @ coef.double().abs()).item()

        def run(staged):
            monkeypatch.setattr(G, "MIX_STAGED", staged)
            return G.glm_grad_mixed(Xg, yg, None, 0, D, SEED, RT, cg, b0, 2, ws).clone().cpu()
        out, plain = run(2), run(0)
        err, err0 = abs(out[D].item() - m64), abs(plain[D].item() - m64)
        ratio = err / max(err0, floor)
        worst = max(worst, ratio)
        print(f"scale {scale} pos {pos}: staged err {err:.3e} unstaged err {err0:.3e} floor {floor:.3e} "
              f"ratio {ratio:.2f}")
        assert out[D + 2].item() == RT
        assert err <= 4.0 * max(err0, floor), (pos, err, err0, floor)
        # X^T r of the one live row: x times the residual the kernel formed, rounded to fp32 once
        g64 = x64 * out[D].item()
        assert torch.allclose(out[:D], g64, rtol=2.0 ** -23, atol=0.0), (pos, (out[:D] - g64).abs().max())
    print(f"scale {scale}: worst ratio {worst:.2f}")


def test_gpu_staged_mfma_one_live_row_beside_lineage_tile(gpu, monkeypatch):
    """The same 16 positions with a lineage tile alongside, logistic loss: the two roles finish
    their rows in different lanes; a row counted twice or not at all shows in the weight sum."""
    monkeypatch.setattr(G, "MIX_STAGED", 2)
    wt, bt = G.synth_truth(SEED, D, D)
    Xl, yl = G.synth_glm(RT, D, SEED, row0=RT, device=gpu, ld=D, wtrue=wt, btrue=bt)
    coef = (torch.randn(D, generator=torch.Generator().manual_seed(4)) * 0.05).to(gpu)
    yr = (torch.rand(RT, generator=torch.Generator().manual_seed(5)) < 0.5).float().to(gpu)
    yall = torch.cat([yr, 1.0 - yl])
    ws = G.GlmWorkspace(gpu, D, grid=1)
    for pos in range(RT):
        Xr = _one_live_row(pos, 200 + pos).to(gpu)
        ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, 0)
        out = G.glm_grad_mixed(Xr, yall, None, RT, D, SEED, RT, coef, 0.1, 0, ws).clone()
        _check_fp64(out, ref)
        assert out[D + 2].item() == 2 * RT, pos


def test_gpu_staged_mfma_sampler(gpu, monkeypatch):
    """Mini-batch sampler on, six slices cut at tiles and the leftover launch: a resident row's
    draw is taken in the lane that finishes it, so the kept set must be sample_mask's."""
    n_res, n_lin, res_row0 = 4097, 2063, 123
    wt, bt = G.synth_truth(SEED, D, D)
    Xr, yr = G.synth_glm(n_res, D, SEED + 1, device=gpu, ld=D)
    Xl, yl = G.synth_glm(n_lin, D, SEED, row0=res_row0 + n_res, device=gpu, ld=D, wtrue=wt, btrue=bt)
    yall = torch.cat([yr, 1.0 - yl])
    coef = torch.randn(D, generator=torch.Generator().manual_seed(4)).to(gpu) * 0.05
    ws = G.GlmWorkspace(gpu, D, grid=96)
    monkeypatch.setattr(G, "MIX_SLICE_ROWS", 1000)
    assert G.mix_splits(n_res + n_lin) == 6
    kw = dict(res_row0=res_row0, t_dev=torch.tensor([4], dtype=torch.int64, device=gpu), sample_seed=99,
              fraction=0.3)
    grows = torch.arange(res_row0, res_row0 + n_res + n_lin)
    w64 = G.sample_mask(99, 5, grows, 0.3).double().to(gpu)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, w64, coef.double(), 0.1, 0)

    def run(staged):
        monkeypatch.setattr(G, "MIX_STAGED", staged)
        return G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, res_row0 + n_res, coef, 0.1, 0, ws, **kw).clone()
    out = run(2)
    _check_fp64(out, ref)
    print("weight sum", out[D + 2].item(), "sample_mask", w64.sum().item())
    assert abs(out[D + 2].item() - w64.sum().item()) < 0.5
    assert torch.equal(out, run(2))
    assert torch.allclose(out, run(0), **ORDER)


@pytest.mark.parametrize("case", ["zeros", "plus_3e38", "minus_3e38"])
def test_gpu_staged_mfma_zero_and_huge_coefficients(gpu, case, monkeypatch):
    """All-zero coefficient fragments, and one +-3e38 coefficient against a column of zeros
    (resident rows only: no lineage value is 0): finite, and the unstaged pass within ORDER.
    No NaN may come out of 0 x the rows 3 - 15 of the coefficient operand either."""
    n_res = 336
    n_lin = 336 if case == "zeros" else 0
    Xr, yr = G.synth_glm(n_res, D, SEED + 1, device=gpu, ld=D)
    yl = (torch.rand(n_lin, generator=torch.Generator().manual_seed(6)) < 0.5).float().to(gpu)
    yall = torch.cat([yr, yl])
    if case == "zeros":
        coef = torch.zeros(D)
    else:
        coef = torch.randn(D, generator=torch.Generator().manual_seed(4)) * 0.05
        coef[77] = 3e38 if case == "plus_3e38" else -3e38
        Xr = Xr.clone()
        Xr[:, 77] = 0
    coef = coef.to(gpu)
    ws = G.GlmWorkspace(gpu, D, grid=1)

    def run(staged):
        monkeypatch.setattr(G, "MIX_STAGED", staged)
        return G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws).clone()
    out, plain = run(2), run(0)
    assert torch.isfinite(out).all()
    print("max |staged - unstaged|", (out - plain).abs().max().item())
    assert torch.allclose(out, plain, **ORDER)
    assert math.isclose(out[D + 2].item(), n_res + n_lin)

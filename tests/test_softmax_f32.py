"""Fused multinomial pass over fp32 feature rows (``glm_softmax_f32_kernel``) vs the fp64 torch
pass, and ``fit_multinomial`` through it.

The inputs sit near an optimum (labels drawn from the model's own softmax, features with a
mean of 10 and a matching intercept), where the gradient is a small difference of large sums:
there, rows rounded to bf16 move it by more than a hundred times the tolerance
(test_bf16_rounded_rows_miss_the_gradient_tolerance), so a path that rounded the rows could
not pass the GPU test.
"""
import functools
import math

import pytest
import torch

from orange3_spark_amd.ops import glm as G

GRAD_TOL = 2e-5      # of max|G_ref|, as for the bf16 kernel (test_glm_kernels.py)


@functools.lru_cache(maxsize=2)
def _case(n, d, K, weighted, pad):
    """(Xfull fp32 [n, d + pad] with zero padding, y int64, sw or None, W [K, d], b [K]) on the CPU."""
    g = torch.Generator().manual_seed(1000 * d + 10 * K + pad)
    X = torch.randn((n, d), generator=g) * 3 + 10
    W = torch.randn((K, d), generator=g) * (0.3 / math.sqrt(d))
    b = torch.randn(K, generator=g) * 0.5 - 10 * W.sum(1)
    P = torch.softmax(X.double() @ W.double().T + b.double(), 1)
    y = torch.multinomial(P, 1, generator=g).squeeze(1)
    sw = torch.rand(n, generator=g) + 0.5 if weighted else None
    Xfull = torch.zeros((n, d + pad))
    Xfull[:, :d] = X
    return Xfull, y, sw, W, b


SHAPES = [(40_003, 256, 10, False, 0),     # NB = 8
          (40_003, 20, 3, True, 4),        # padded view; d not a multiple of 8
          (40_003, 100, 32, True, 4),      # K at its limit; NB = 4 with a ragged last block
          (40_003, 64, 2, False, 0),       # K = 2
          (40_003, 200, 7, False, 56),     # stride 256 != d
          (40_003, 8, 1, False, 0),        # one chunk; a single class
          (40_003, 33, 32, True, 7),       # NB = 2, only one live column in the second block
          (17, 40, 5, True, 0),            # fewer rows than a tile
          (100_003, 256, 10, False, 0),    # several tiles per wave: prefetch steady state and tail
          (67, 96, 10, False, 0),          # NB = 3, 5 and 6: two full tiles and a 3-row tail
          (67, 160, 3, True, 0),
          (67, 192, 32, True, 8)]


@pytest.mark.parametrize("d,K", [(256, 10), (20, 3), (100, 32), (8, 5)])
def test_bf16_rounded_rows_miss_the_gradient_tolerance(d, K):
    """The storage check is meaningful: the fp64 pass on rows rounded through bf16 leaves the
    fp64 pass on the exact rows by more than 20x the gradient tolerance."""
    Xfull, y, _, W, b = _case(40_003, d, K, False, 0)
    Gr, _, _ = G.softmax_pass_torch(Xfull, y, None, W, b)
    Gb, _, _ = G.softmax_pass_torch(Xfull.to(torch.bfloat16), y, None, W, b)
    ratio = (Gb - Gr).abs().max().item() / (GRAD_TOL * Gr.abs().max().item())
    print(f"d={d} K={K}: bf16-rounded rows are {ratio:.0f}x the gradient tolerance away")
    assert ratio > 20


def _to_gpu(case, d, gpu):
    Xfull, y, sw, W, b = case
    return Xfull.to(gpu)[:, :d], y.to(gpu), None if sw is None else sw.to(gpu), W.to(gpu), b.to(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,K,weighted,pad", SHAPES)
def test_gpu_softmax_f32_pass_matches_fp64(gpu, n, d, K, weighted, pad):
    X, y, sw, W, b = _to_gpu(_case(n, d, K, weighted, pad), d, gpu)
    assert X.dtype == torch.float32 and X.stride(0) == d + pad
    assert G.softmax_kernel_ok(X, K)
    Gk, gb, loss = G.softmax_pass(X, y, sw, W, b)
    Gr, gbr, lr = G.softmax_pass_torch(X, y, sw, W, b)
    scale = Gr.abs().max().item()
    print(f"n={n} d={d} K={K}: |G - Gref| / max|Gref| = {(Gk - Gr).abs().max().item() / max(scale, 1e-300):.3e}, "
          f"|gb - gbref| = {(gb - gbr).abs().max().item():.3e}, "
          f"loss rel = {abs(loss.item() - lr.item()) / max(abs(lr.item()), 1e-300):.3e}")
    assert Gk.shape == (K, d) and gb.shape == (K,)
    assert (Gk - Gr).abs().max().item() <= GRAD_TOL * scale
    assert torch.allclose(gb, gbr, rtol=1e-5, atol=1e-6 * n)
    assert abs(loss.item() - lr.item()) <= 1e-5 * abs(lr.item())


@pytest.mark.gpu
def test_gpu_softmax_f32_dispatch_conditions(gpu):
    X = torch.zeros((64, 264), device=gpu)
    assert G.softmax_kernel_ok(X[:, :256], 32)
    assert not G.softmax_kernel_ok(X[:, :257], 10)                                # d = 257
    assert not G.softmax_kernel_ok(X[:, :256], 33)                                # K = 33
    assert not G.softmax_kernel_ok(torch.zeros((64, 12), device=gpu)[:, :5], 3)   # row stride 12
    assert not G.softmax_kernel_ok(torch.zeros((64, 16)), 3)                      # CPU rows
    assert not G.softmax_kernel_ok(torch.zeros((64, 16), dtype=torch.bfloat16), 3)


@pytest.mark.gpu
def test_gpu_softmax_f32_pass_is_repeatable_and_handles_no_rows(gpu):
    X, y, sw, W, b = _to_gpu(_case(40_003, 100, 32, True, 4), 100, gpu)
    one = [t.clone() for t in G.softmax_pass(X, y, sw, W, b)]
    two = G.softmax_pass(X, y, sw, W, b)
    for a, c in zip(one, two):
        assert torch.equal(a, c)
    Gk, gb, loss = G.softmax_pass(X[:0], y[:0], None, W, b)
    assert Gk.shape == (32, 100) and not Gk.any() and not gb.any() and loss.item() == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_gpu_multinomial_fit_f32_kernel_matches_chunked(gpu, monkeypatch, alpha):
    """Data recipe and bounds of test_glm_kernels.test_gpu_multinomial_fit_kernel_matches_chunked,
    with the rows kept fp32 and not bf16-exact; alpha > 0 goes through OWL-QN."""
    from orange3_spark_amd.models import glm as GLM
    from orange3_spark_amd.parallel.comm import LocalComm
    g = torch.Generator().manual_seed(5)
    n, d, K = 50_000, 24, 4
    X = (torch.rand((n, d), generator=g) * 2 - 1).to(gpu)
    assert not torch.equal(X, X.to(torch.bfloat16).float())
    z = X[:, 0] + 0.5 * X[:, 1]
    y = ((z + 1.5) / 3 * K).floor().clamp(0, K - 1).double()
    comm = LocalComm(gpu)
    seen = []
    real = G.softmax_pass

    def counted(Xr, *a):
        seen.append(Xr.dtype)
        return real(Xr, *a)
    monkeypatch.setattr(G, "softmax_pass", counted)
    B1, b1, r1 = GLM.fit_multinomial(comm, X, y, None, K, reg=0.01, alpha=alpha, max_iter=50)
    assert seen and set(seen) == {torch.float32}
    calls = len(seen)
    monkeypatch.setenv("O3S_SOFTMAX_KERNEL", "0")
    B0, b0, r0 = GLM.fit_multinomial(comm, X, y, None, K, reg=0.01, alpha=alpha, max_iter=50)
    assert len(seen) == calls                      # the switch still forces the chunked path
    print(f"alpha={alpha}: f kernel {r1.f:.9f} ({r1.iterations} it, {r1.reason})  chunked {r0.f:.9f} "
          f"({r0.iterations} it, {r0.reason})  |dB| {abs(B1 - B0).max():.2e}  |db| {abs(b1 - b0).max():.2e}")
    assert abs(r1.f - r0.f) <= 1e-6 * abs(r0.f)
    assert abs(B1 - B0).max() < 1e-3 and abs(b1 - b0).max() < 1e-3

"""The fused one-hidden-layer perceptron kernels (csrc/mlp.hip) against the fp64 references
``ops.mlp.mlp_pass_torch`` / ``mlp_logits_torch`` on the same rows.

The inputs sit near an optimum, so the gradient is a small difference of large sums: the labels
are drawn from the model's own softmax (``case`` of test_mlp_host.py).  bf16 rows are exact in
the kernel; fp32 rows are split into bf16 terms on the fly, and
``test_mlp_host.py::test_bf16_rounded_rows_miss_the_gradient_ceiling`` shows on the CPU that a
path which merely rounded them to bf16 would miss the gradient bound by more than 10x its
ceiling."""
import pytest
import torch

from orange3_spark_amd.ops import mlp as MLP
from test_mlp_host import N, TOL, case

#        d    H    K  pad mean n
SHAPES = [
    (256, 64, 10, 0, 0.0, N),          # NH 2, widest rows
    (128, 128, 32, 0, 0.0, N),         # NH 4, full classes, tightest LDS
    (64, 128, 3, 0, 0.0, N),           # NH 4 on both dtypes
    (20, 5, 3, 4, 0.0, N),             # padded d, H, K
    (8, 33, 2, 0, 2.0, N),             # one unit into the second block, shifted columns
    (100, 100, 4, 4, 0.0, N),          # NH 4 ragged
    (33, 32, 32, 7, 0.0, N),           # NH 1 exactly full
    (40, 7, 3, 0, 0.0, 17),            # one partial tile, most slab rows empty
    (256, 32, 10, 0, 0.0, 100_003),    # several tiles per slab row
    (96, 64, 10, 0, 0.0, 67),          # 3, 5 and 6 column blocks of 32 (as far as the gate takes
    (160, 32, 5, 0, 0.0, 67),          # them on both row types): two full tiles and a 3-row tail
    (192, 33, 3, 8, 0.0, 67),
]
IDS = [f"d{d}-H{H}-K{K}-pad{p}{'-mean2' if m else ''}-n{n}" for d, H, K, p, m, n in SHAPES]
DTYPES = [torch.bfloat16, torch.float32]


def _gated_out(shape, dtype):
    """A shape the gate gives back to the torch program on this row type (fp32 rows wider than
    192 columns past one hidden block): there is no kernel to compare."""
    d, H, K, pad, mean, n = shape
    return MLP.gate_reason(True, dtype, d + pad, 1, d, H, K) is not None


def _cases():
    return [pytest.param(s, t, id=f"{i}-{'bf16' if t == torch.bfloat16 else 'fp32'}")
            for s, i in zip(SHAPES, IDS) for t in DTYPES if not _gated_out(s, t)]


def _errors(got, ref, n):
    gW1, gb1, gW2, gb2, l = (t.double().cpu() for t in got)
    rW1, rb1, rW2, rb2, rl = (t.double().cpu() for t in ref)
    rel = lambda a, b: float((a - b).abs().max()) / float(b.abs().max())      # noqa: E731
    return dict(gW1=rel(gW1, rW1), gW2=rel(gW2, rW2),
                gb1=float((gb1 - rb1).abs().max()), gb1_bar=1e-5 * float(rb1.abs().max()) + 1e-6 * n,
                gb2=float((gb2 - rb2).abs().max()), gb2_bar=1e-5 * float(rb2.abs().max()) + 1e-6 * n,
                loss=abs(float(l - rl)), loss_bar=1e-5 * abs(float(rl)))


def test_the_gate_takes_every_shape_on_bf16_rows_and_all_but_one_on_fp32():
    assert not any(_gated_out(s, torch.bfloat16) for s in SHAPES)
    assert [s[:3] for s in SHAPES if _gated_out(s, torch.float32)] == [(256, 64, 10)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", _cases())
def test_pass_matches_the_fp64_reference(shape, dtype):
    d, H, K, pad, mean, n = shape
    c = case(n, d, H, K, pad, mean, dtype, "cuda")
    assert MLP.mlp_kernel_ok(c["X"], H, K) and c["X"].stride(0) == d + pad and c["X"].dtype == dtype
    got = MLP.mlp_pass(c["X"], c["y"], *c["par"])
    assert [tuple(t.shape) for t in got] == [(d, H), (H,), (H, K), (K,), ()]
    assert all(t.dtype == torch.float64 and t.is_cuda for t in got)
    e = _errors(got, c["ref"], n)
    print(f"mlp_pass {shape} {dtype}: gW1 {e['gW1']:.2e} gW2 {e['gW2']:.2e} (of max|ref|, bar {TOL:.0e}); "
          f"gb1 {e['gb1']:.2e} (bar {e['gb1_bar']:.2e}); gb2 {e['gb2']:.2e} (bar {e['gb2_bar']:.2e}); "
          f"loss {e['loss']:.2e} (bar {e['loss_bar']:.2e})")
    assert e["gW1"] <= TOL and e["gW2"] <= TOL
    assert e["gb1"] <= e["gb1_bar"] and e["gb2"] <= e["gb2_bar"] and e["loss"] <= e["loss_bar"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype", _cases())
def test_logits_match_the_fp64_reference(shape, dtype):
    d, H, K, pad, mean, n = shape
    c = case(n, d, H, K, pad, mean, dtype, "cuda")
    L = MLP.mlp_logits(c["X"], *c["par"])
    assert L.shape == (n, K) and L.dtype == torch.float32
    err = float((L.double() - c["L"]).abs().max())
    bar = 1e-5 * max(1.0, float(c["L"].abs().max()))
    print(f"mlp_logits {shape} {dtype}: {err:.2e} (bar {bar:.2e})")
    assert err <= bar
    assert torch.equal(L, MLP.mlp_logits(c["X"], *c["par"], grid=3))      # any grid, the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_repeatable_and_grid_independent(dtype):
    d, H, K, pad, mean, n = SHAPES[5]
    c = case(n, d, H, K, pad, mean, dtype, "cuda")
    args = (c["X"], c["y"], *c["par"])
    a, b = MLP.mlp_pass(*args), MLP.mlp_pass(*args)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the tiles are dealt to a fixed set of slab rows, summed in fp64 in a fixed order: how many
    # blocks walk them does not reach the result
    for grid in (1, 7):
        assert all(torch.equal(x, y) for x, y in zip(a, MLP.mlp_pass(*args, grid=grid))), grid
    # two row ranges are consistent: they add up to the whole
    k = 20_000
    pre = MLP.mlp_pass(c["X"][:k], c["y"][:k], *c["par"])
    post = MLP.mlp_pass(c["X"][k:], c["y"][k:], *c["par"])
    e = _errors(tuple(x + y for x, y in zip(pre, post)), c["ref"], n)
    assert e["gW1"] <= 2 * TOL and e["gW2"] <= 2 * TOL
    e = _errors(pre, MLP.mlp_pass_torch(c["X"][:k], c["y"][:k], *c["par"]), k)
    assert e["gW1"] <= TOL and e["gW2"] <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_empty_pass_returns_zeros(dtype):
    d, H, K = 24, 5, 3
    X = torch.zeros((0, d), dtype=dtype, device="cuda")
    par = (torch.ones((d, H), device="cuda"), torch.ones(H, device="cuda"), torch.ones((H, K), device="cuda"),
           torch.ones(K, device="cuda"))
    got = MLP.mlp_pass(X, torch.zeros(0, dtype=torch.int32, device="cuda"), *par)
    assert [tuple(t.shape) for t in got] == [(d, H), (H,), (H, K), (K,), ()]
    assert all(t.dtype == torch.float64 and not t.any() for t in got)
    assert MLP.mlp_logits(X, *par).shape == (0, K)


@pytest.mark.gpu
def test_dispatch():
    dev = "cuda"
    pad = torch.zeros((64, 24), dtype=torch.bfloat16, device=dev)
    assert MLP.mlp_kernel_ok(pad[:, :20], 8, 3) and not pad[:, :20].is_contiguous()    # the view of a padded column
    assert MLP.mlp_kernel_ok(torch.zeros((64, 256), device=dev), 32, 32)
    assert MLP.mlp_kernel_ok(torch.zeros((64, 256), dtype=torch.bfloat16, device=dev), 64, 10)
    assert not MLP.mlp_kernel_ok(torch.zeros((64, 256), device=dev), 64, 10)            # fp32: 2 x 8 blocks
    assert MLP.mlp_kernel_ok(torch.zeros((64, 128), device=dev), 128, 32)               # fp32: 4 x 4
    assert not MLP.mlp_kernel_ok(torch.zeros((64, 160), dtype=torch.bfloat16, device=dev), 128, 10)    # 4 x 5
    assert not MLP.mlp_kernel_ok(torch.zeros((64, 264), device=dev)[:, :257], 8, 3)
    assert not MLP.mlp_kernel_ok(pad, 129, 3) and not MLP.mlp_kernel_ok(pad, 0, 3)
    assert not MLP.mlp_kernel_ok(pad, 8, 1) and not MLP.mlp_kernel_ok(pad, 8, 33)
    assert not MLP.mlp_kernel_ok(torch.zeros((64, 12), device=dev), 8, 3)               # row stride 12
    assert not MLP.mlp_kernel_ok(pad[:, 8:], 8, 3)          # a view that would be read past its parent's row
    assert not MLP.mlp_kernel_ok(pad.cpu(), 8, 3)
    assert not MLP.mlp_kernel_ok(torch.zeros((64, 24), dtype=torch.float64, device=dev), 8, 3)
    assert not MLP.mlp_kernel_ok(pad.t(), 8, 3)
    z = lambda *s: torch.zeros(s, device=dev)      # noqa: E731
    with pytest.raises(ValueError):
        MLP.mlp_pass(z(64, 12), torch.zeros(64, dtype=torch.int32, device=dev), z(12, 8), z(8), z(8, 3), z(3))
    with pytest.raises(ValueError):
        MLP.mlp_logits(pad, z(24, 8), z(8), z(8, 33), z(33))
    with pytest.raises(ValueError):
        MLP.mlp_logits(pad, z(20, 8), z(8), z(8, 3), z(3))      # the rows' width is not the network's

"""Fused weighted Gram pass (``ops/gram.py::weighted_gram``, ``csrc/gram.hip``) against its fp64
reference on the same stored values.

Data: columns offset by (50, -50, 50, -50, 10, 0, 50, -50) (tiled across the width) plus
N(0, 1), weights U(0.5, 1.5).  Offsets that large against unit variance are what an fp32
Gram accumulation gets wrong unless the rows are shifted first, and what bf16 storage cannot
hold: test_storage_check_is_meaningful shows that rows rounded through bf16 miss the bound
used below by far more than 20x, so a path that rounds the rows cannot pass.

Bound per entry (u = 2^-24, z = x - shift, K = flush_rows, both reported by the op):

    T_ij = (K + 8) u sum_r w_r |z_ri| |z_rj| + u (|c_i| sum w |z_j| + |c_j| sum w |z_i|)

an fp32 accumulator takes at most K rows before it is added into fp64 (the first term; the
+ 8 covers the sqrt(w) scaling, the subtraction and the dropped split terms), and the shift
is undone in fp64 from the fp32 shift values (the second).  The y and ones columns are two
more columns of z with shift 0.
"""
import numpy as np
import pytest
import torch

from orange3_spark_amd.ops import gram as GR

OFFSETS = np.array([50.0, -50.0, 50.0, -50.0, 10.0, 0.0, 50.0, -50.0])
U = 2.0 ** -24


def _data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)) + np.resize(OFFSETS, d)
    w = rng.uniform(0.5, 1.5, n)
    y = rng.normal(size=n) + 0.1 * (X[:, 0] - OFFSETS[0]) if n else np.zeros(0)
    return X, w, y


def _bound(X64, d, w64, y64, shift, K):
    """T for the augmented matrix [x | y | 1], as [d + 2, d + 2] (fp64 torch tensors in and out)."""
    n = X64.shape[0]
    Za = torch.cat([X64[:, :d] - shift, y64[:, None], torch.ones(n, 1, dtype=torch.float64)], 1).abs()
    ca = torch.cat([shift.abs(), torch.zeros(2, dtype=torch.float64)])
    A = (Za * w64[:, None]).T @ Za
    s1 = w64 @ Za
    return (K + 8) * U * A + U * (torch.outer(ca, s1) + torch.outer(s1, ca))


def _augmented(st, d):
    """GramStats -> the [d + 2, d + 2] matrix of [x | y | 1]."""
    M = torch.zeros(d + 2, d + 2, dtype=torch.float64)
    M[:d, :d] = st.G.cpu()
    M[:d, d] = M[d, :d] = st.xty.cpu()
    M[:d, d + 1] = M[d + 1, :d] = st.sx.cpu()
    M[d, d] = st.syy.cpu()
    M[d, d + 1] = M[d + 1, d] = st.sy.cpu()
    M[d + 1, d + 1] = st.sw.cpu()
    return M


# --------------------------------------------------------------------------- CPU
def test_reference_equals_einsum():
    X, w, y = _data(501, 13, seed=3)
    Xt, wt, yt = torch.from_numpy(X), torch.from_numpy(w), torch.from_numpy(y)
    st = GR.weighted_gram_torch(Xt, 13, wt, yt)
    np.testing.assert_allclose(st.G.numpy(), np.einsum("r,ri,rj->ij", w, X, X), rtol=1e-12)
    np.testing.assert_allclose(st.sx.numpy(), np.einsum("r,ri->i", w, X), rtol=1e-12)
    np.testing.assert_allclose(st.xty.numpy(), np.einsum("r,r,ri->i", w, y, X), rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose([float(st.sw), float(st.sy), float(st.syy)], [w.sum(), (w * y).sum(), (w * y * y).sum()],
                               rtol=1e-12)
    un = GR.weighted_gram_torch(Xt, 13)
    np.testing.assert_allclose(un.G.numpy(), X.T @ X, rtol=1e-12)
    assert float(un.sw) == 501 and float(un.sy) == 0 and float(un.xty.abs().max()) == 0
    # CPU tensors take the reference
    assert torch.equal(GR.weighted_gram(Xt, 13, wt, yt).G, st.G)


def test_shift_algebra_round_trips():
    X, w, y = _data(2000, 8, seed=4)
    Xt, wt, yt = torch.from_numpy(X), torch.from_numpy(w), torch.from_numpy(y)
    c = Xt[:1024].mean(0)
    z = GR.weighted_gram_torch(Xt - c, 8, wt, yt)
    G, sx, xty = GR.unshift(z.G, z.sx, z.xty, z.sw, z.sy, c)
    ref = GR.weighted_gram_torch(Xt, 8, wt, yt)
    np.testing.assert_allclose(G.numpy(), ref.G.numpy(), rtol=1e-12)
    np.testing.assert_allclose(sx.numpy(), ref.sx.numpy(), rtol=1e-12)
    np.testing.assert_allclose(xty.numpy(), ref.xty.numpy(), rtol=1e-10, atol=1e-9)


def test_storage_check_is_meaningful():
    n, d = 40003, 8
    X, w, y = _data(n, d)
    Xt, wt, yt = torch.from_numpy(X), torch.from_numpy(w), torch.from_numpy(y)
    X32 = Xt.float().double()                       # the values an fp32 column stores
    shift = X32[:1024].float().mean(0).double()
    T = _bound(X32, d, wt, yt, shift, GR.FLUSH_ROWS)[:d, :d]
    ref = GR.weighted_gram_torch(X32, d, wt, yt).G
    rounded = GR.weighted_gram_torch(X32.to(torch.bfloat16).double(), d, wt, yt).G
    miss = float(((rounded - ref).abs() / T).max())
    print(f"bf16-rounded rows: {miss:.1f} x the bound")
    assert miss > 20


# --------------------------------------------------------------------------- GPU
# (n, d, stride, weighted, with y, nwaves)
CASES = [
    (17, 40, None, False, False, None),
    (40003, 8, None, False, False, None),
    (40003, 20, 24, False, False, None),
    (40003, 33, None, False, False, None),
    (40003, 64, None, False, False, None),
    (40003, 100, None, True, False, None),
    (40003, 200, 256, False, False, None),
    (40003, 256, None, True, True, None),
    (100003, 256, None, False, False, 4),
    (100003, 64, None, False, False, 4),
]
_CACHE = {}


def _case(case, dtype, gpu):
    """(stored rows on the GPU, the same values fp64 on the host, w, y, fp64 reference), computed once."""
    key = (case, dtype)
    if key not in _CACHE:
        n, d, stride, weighted, with_y, _ = case
        X, w, y = _data(n, d)
        ld = stride or (d + 7) // 8 * 8
        S = torch.from_numpy(np.random.default_rng(9).uniform(-1e3, 1e3, (n, ld))).to(dtype)   # dead columns: garbage
        S[:, :d] = torch.from_numpy(X).to(dtype)
        wt = torch.from_numpy(w).float() if weighted else None
        yt = torch.from_numpy(y).float() if with_y else None
        ref = GR.weighted_gram_torch(S.double(), d, None if wt is None else wt.double(),
                                     None if yt is None else yt.double())
        _CACHE[key] = (S, wt, yt, ref)
    S, wt, yt, ref = _CACHE[key]
    return S.to(gpu), S, wt, yt, ref


def _run(case, dtype, gpu):
    Xg, S, wt, yt, ref = _case(case, dtype, gpu)
    st = GR.weighted_gram(Xg, case[1], None if wt is None else wt.to(gpu), None if yt is None else yt.to(gpu),
                          nwaves=case[5])
    return st, S, wt, yt, ref


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"n{c[0]}-d{c[1]}" + (f"-ld{c[2]}" if c[2] else "")
                         + ("-w" if c[3] else "") + ("-y" if c[4] else "") + (f"-nw{c[5]}" if c[5] else ""))
def test_matches_reference(case, dtype, gpu):
    n, d = case[0], case[1]
    st, S, wt, yt, ref = _run(case, dtype, gpu)
    assert st.flush_rows == GR.FLUSH_ROWS <= 4096
    w64 = torch.ones(n, dtype=torch.float64) if wt is None else wt.double()
    y64 = torch.zeros(n, dtype=torch.float64) if yt is None else yt.double()
    T = _bound(S.double(), d, w64, y64, st.shift.cpu(), st.flush_rows)
    err = (_augmented(st, d) - _augmented(ref, d)).abs()
    worst = float((err / T.clamp_min(1e-300)).max())
    print(f"n={n} d={d} {dtype}: max err / bound = {worst:.4f}, max err = {float(err.max()):.3e}")
    assert torch.isfinite(err).all()
    assert bool((err <= T).all()), f"worst entry at {worst:.2f} x the bound"
    assert torch.equal(st.G, st.G.T)
    # two calls are bitwise equal
    again = _run(case, dtype, gpu)[0]
    for f in ("G", "sx", "xty", "sw", "sy", "syy"):
        assert torch.equal(getattr(st, f), getattr(again, f)), f


def _emulation_error(S, d, w64, y64, shift, K, ref_aug):
    """Max error over the entries of a float32 sequential accumulation (one rank-1 update per row)
    in chunks of K rows, fp64 across chunks, of the shifted, scaled, augmented rows; the shift is
    undone in fp64 as the op does."""
    n = S.shape[0]
    s = w64.float().sqrt()
    Za = torch.cat([(S[:, :d].float() - shift.float()) * s[:, None], (s * y64.float())[:, None], s[:, None]], 1)
    da = d + 2
    Gz = torch.zeros(da, da, dtype=torch.float64)
    for a in range(0, n, K):
        acc = torch.zeros(da, da, dtype=torch.float32)
        for z in Za[a:a + K]:
            acc.addr_(z, z)
        Gz += acc.double()
    # the sums over w and y alone in fp64, as the op takes them
    sw, sy, syy = w64.sum(), (w64 * y64).sum(), (w64 * y64 * y64).sum()
    G, sx, xty = GR.unshift(Gz[:d, :d], Gz[:d, d + 1], Gz[:d, d], sw, sy, shift)
    emu = GR.GramStats(G, sx, xty, sw, sy, syy, shift, K)
    return float((_augmented(emu, d) - ref_aug).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[4], CASES[7]], ids=["d64", "d256"])
def test_error_is_that_of_an_fp32_chain(case, gpu):
    """The bound above is worst case; measured, the kernel's error is within 4x of a float32
    sequential chain over flush_rows rows on the same input (the MFMA's and the waves' order of
    summation is another draw from the same error distribution)."""
    n, d = case[0], case[1]
    st, S, wt, yt, ref = _run(case, torch.float32, gpu)
    w64 = torch.ones(n, dtype=torch.float64) if wt is None else wt.double()
    y64 = torch.zeros(n, dtype=torch.float64) if yt is None else yt.double()
    ref_aug = _augmented(ref, d)
    kern = float((_augmented(st, d) - ref_aug).abs().max())
    emu = _emulation_error(S, d, w64, y64, st.shift.cpu(), st.flush_rows, ref_aug)
    print(f"d={d}: kernel max err {kern:.3e}, fp32 chain max err {emu:.3e}, ratio {kern / emu:.3f}")
    assert kern <= 4 * emu


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_empty_table(dtype, gpu):
    st = GR.weighted_gram(torch.zeros((0, 16), dtype=dtype, device=gpu), 10,
                          torch.zeros(0, device=gpu), torch.zeros(0, device=gpu))
    assert st.G.shape == (10, 10)
    for f in ("G", "sx", "xty", "sw", "sy", "syy"):
        assert float(getattr(st, f).abs().max()) == 0.0, f


@pytest.mark.gpu
def test_kernel_ok(gpu):
    X = torch.zeros((64, 24), device=gpu)
    assert GR.gram_kernel_ok(X, 20) and GR.gram_kernel_ok(X.bfloat16(), 24, torch.ones(64, device=gpu))
    assert not GR.gram_kernel_ok(X, 25)
    assert not GR.gram_kernel_ok(X, 0)
    assert not GR.gram_kernel_ok(X.double(), 20)
    assert not GR.gram_kernel_ok(X[:, :20], 20)
    assert not GR.gram_kernel_ok(X, 20, -torch.ones(64, device=gpu))
    assert not GR.gram_kernel_ok(torch.zeros((8, 264), device=gpu), 257)
    assert not GR.gram_kernel_ok(X.cpu(), 20)
    with pytest.raises(TypeError):
        GR.weighted_gram(X.double(), 20)

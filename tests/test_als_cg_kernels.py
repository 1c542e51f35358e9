"""The ALS conjugate-gradient path (csrc/als.hip: als_pass_kernel, als_cg_kernel,
als_init_kernel) at every lanes-per-dim instantiation RV = ceil(R / 64) = 1..8.

The inputs are small integers, so every product and every partial sum of the kernels is an
exactly representable fp32 number whatever the order of summation, the FMA contraction or
the shape of the wave reduction: the kernel output must equal the fp64 reference bitwise.
The condition for that (every sum of absolute values below 2^24) is asserted on the
reference inputs by unmarked tests, for every parametrisation the GPU tests use."""
import functools

import pytest
import torch

from orange3_spark_amd.models import als as AE
from orange3_spark_amd.ops import als as A

F32_EXACT = 1 << 24            # integers below this are exact in fp32

# 13 rows (not a multiple of the 4 waves of a block); empty rows first, inner and near the
# end; every remainder of the 4-ratings-in-flight unroll, and a long row
LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 40, 0, 13, 6]
N_ROWS = len(LENS)
N_OTHER = 50
VIEW = (3, 11)                 # the row-range view indptr[3:11] (absolute offsets)
RANKS = [1, 63, 64, 65, 128, 192, 256, 257, 320, 384, 385, 448, 449, 512]   # RV 1..8: 64 RV and one past
RV_RANKS = [37, 100, 190, 250, 300, 383, 440, 509]                           # one odd rank per RV
INIT_RANKS = [1, 64, 65, 192, 256, 257, 320, 384, 448, 449, 512]            # RV 1, 1, 2, 3, 4, 5, 5, 6, 7, 8, 8
MODES = ["matvec", "rhs", "both"]


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def _pass_case(R, integer=True):
    """(indptr, cols, coef, coef2, F, V) on the CPU; shared, never modified."""
    g = torch.Generator().manual_seed(1000 + R)
    indptr = torch.zeros(N_ROWS + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.tensor(LENS), 0)
    nnz = int(indptr[-1])
    cols = torch.randint(0, N_OTHER, (nnz,), generator=g, dtype=torch.int32)
    if integer:
        coef, coef2 = _ints(g, -4, 4, (nnz,)), _ints(g, -4, 4, (nnz,))
        F, V = _ints(g, -3, 3, (N_OTHER, R)), _ints(g, -3, 3, (N_ROWS, R))
    else:
        coef, coef2 = torch.rand(nnz, generator=g), torch.rand(nnz, generator=g)
        F, V = torch.randn(N_OTHER, R, generator=g), torch.randn(N_ROWS, R, generator=g)
    return indptr, cols, coef, coef2, F, V


@functools.lru_cache(maxsize=None)
def _pass_ref(R, integer=True):
    """fp64 references cast to fp32: (matvec with coef, rhs with coef, rhs with coef2)."""
    indptr, cols, coef, coef2, F, V = _pass_case(R, integer)
    return (A.pass_torch(0, indptr, cols, coef, F, V), A.pass_torch(1, indptr, cols, coef, F, None),
            A.pass_torch(1, indptr, cols, coef2, F, None))


def pass_abs_bound(indptr, cols, coef, coef2, F, V):
    """Largest value any partial sum of als_pass_kernel can take on these inputs, every
    term replaced by its absolute value (fp64): the per-rating dot product, its product
    with the coefficient, and the matvec / rhs accumulators."""
    Fa, Va = F.double().abs(), V.double().abs()
    rows = torch.repeat_interleave(torch.arange(indptr.numel() - 1), indptr[1:] - indptr[:-1])
    Fg = Fa[cols.long()]
    dot = (Fg * Va[rows]).sum(1)
    s = coef.double().abs() * dot
    top = [dot.max(), s.max()]
    for c in (s, coef.double().abs(), coef2.double().abs()):
        top.append(torch.zeros((indptr.numel() - 1, F.shape[1]), dtype=torch.float64)
                   .index_add_(0, rows, Fg * c[:, None]).max())
    return float(torch.stack(top).max())


@pytest.mark.parametrize("R", RANKS)
def test_pass_inputs_are_exact_in_fp32(R):
    indptr, cols, coef, coef2, F, V = _pass_case(R)
    for t in (coef, coef2, F, V):
        assert torch.equal(t, t.round())
    assert (indptr[1:] - indptr[:-1]).tolist() == LENS and N_ROWS % 4 != 0
    bound = pass_abs_bound(indptr, cols, coef, coef2, F, V)
    assert 0 < bound < F32_EXACT, bound


def test_pass_torch_row_range_view_is_rows_of_full_result():
    """The reference itself: a view of indptr with absolute offsets gives those rows."""
    indptr, cols, coef, coef2, F, V = _pass_case(65)
    a, e = VIEW
    assert int(indptr[a]) > 0 and int(indptr[e]) < cols.numel()
    assert torch.equal(A.pass_torch(0, indptr[a:e + 1], cols, coef, F, V[a:e]), _pass_ref(65)[0][a:e])
    assert torch.equal(A.pass_torch(1, indptr[a:e + 1], cols, coef2, F, None), _pass_ref(65)[2][a:e])


def _run_pass(mode, dev, indptr, cols, coef, coef2, F, V):
    """The kernel's outputs for ``mode`` and the matching slots of _pass_ref."""
    d = lambda t: t.to(dev)
    if mode == "matvec":
        return [A.pass_(0, d(indptr), d(cols), d(coef), d(F), d(V))], [0]
    if mode == "rhs":
        return [A.pass_(1, d(indptr), d(cols), d(coef), d(F), None)], [1]
    return list(A.pass_both(d(indptr), d(cols), d(coef), d(F), d(V), d(coef2))), [0, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", RANKS)
def test_gpu_als_pass_bitwise(gpu, R, mode):
    """als_pass_kernel<RV, 0 | 1 | 2> == the fp64 reference bitwise on integer inputs: rows
    of 0..9 ratings (every tail of the 4-rating unroll), 13 rows, dims d >= R masked."""
    case = _pass_case(R)
    got, slots = _run_pass(mode, gpu, *case)
    for o, s in zip(got, slots):
        assert o.dtype == torch.float32 and o.shape == (N_ROWS, R)
        assert torch.equal(o.cpu(), _pass_ref(R)[s])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", RANKS)
def test_gpu_als_pass_row_range_view_bitwise(gpu, R, mode):
    """The chunked path of solve_side: indptr[a:e+1] keeps its absolute offsets into
    cols / coef, V and the output hold the rows of the range only."""
    indptr, cols, coef, coef2, F, V = _pass_case(R)
    a, e = VIEW
    dptr = indptr.to(gpu)                                   # the view is taken on the device tensor
    d = lambda t: t.to(gpu)
    if mode == "matvec":
        got, slots = [A.pass_(0, dptr[a:e + 1], d(cols), d(coef), d(F), d(V[a:e]))], [0]
    elif mode == "rhs":
        got, slots = [A.pass_(1, dptr[a:e + 1], d(cols), d(coef), d(F), None)], [1]
    else:
        got, slots = list(A.pass_both(dptr[a:e + 1], d(cols), d(coef), d(F), d(V[a:e]), d(coef2))), [0, 2]
    for o, s in zip(got, slots):
        assert o.shape == (e - a, R)
        assert torch.equal(o.cpu(), _pass_ref(R)[s][a:e])


@pytest.mark.gpu
@pytest.mark.parametrize("R", RV_RANKS)
def test_gpu_als_pass_random_floats(gpu, R):
    """Random floats (rounding now matters) at the tolerance of tests/test_als.py."""
    case = _pass_case(R, False)
    ref = _pass_ref(R, False)
    for mode in MODES:
        got, slots = _run_pass(mode, gpu, *case)
        for o, s in zip(got, slots):
            assert torch.allclose(o.cpu(), ref[s], rtol=1e-4, atol=1e-3)


# ----------------------------------------------------------------------------- als_cg_kernel

CG_ROWS = 13
ROW_P0, ROW_NEG, ROW_RS0 = 2, 7, 12          # den == 0, den < 0, rs0 == 0 (the last: a partial block)


@functools.lru_cache(maxsize=None)
def _cg_init_case(R, with_pf):
    g = torch.Generator().manual_seed(2000 + R + with_pf)
    x, ax, rhs = (_ints(g, -3, 3, (CG_ROWS, R)) for _ in range(3))
    pf = _ints(g, -3, 3, (CG_ROWS, R)) if with_pf else None
    lam = (torch.arange(CG_ROWS) % 3).float()                # 0, 1, 2
    return x, ax, pf, rhs, lam


def cg_init_ref(x, ax, pf, rhs, lam):
    """fp64 (r, rs) of the documented init, and the absolute-value bound of rs."""
    x, ax, rhs, lam = x.double(), ax.double(), rhs.double(), lam.double()
    pfd = torch.zeros_like(x) if pf is None else pf.double()
    r = rhs - (ax + pfd + lam[:, None] * x)
    ra = rhs.abs() + ax.abs() + pfd.abs() + lam[:, None] * x.abs()
    return r, (r * r).sum(1), float((ra * ra).sum(1).max())


@functools.lru_cache(maxsize=None)
def _cg_step_case(R, with_pf):
    """(x, r, p, ap, pf, lam, rs) with den = p.q a positive integer, rs = den * a for
    a in {0.5, 1}, and the three guard rows."""
    g = torch.Generator().manual_seed(3000 + R + with_pf)
    x, r, p = (_ints(g, -3, 3, (CG_ROWS, R)) for _ in range(3))
    p[p.abs().sum(1) == 0, 0] = 1.0                        # den > 0 needs p != 0
    pf = _ints(g, -1, 1, (CG_ROWS, R)) if with_pf else None
    lam = (torch.arange(CG_ROWS) % 3).float()
    p[ROW_P0] = 0.0
    ap = _ints(g, -1, 1, (CG_ROWS, R)) + 5.0 * p           # p.q >= 5 |p|^2 - 2 |p|_1 > 0
    ap[ROW_NEG] = -3.0 * p[ROW_NEG]
    lam[ROW_NEG] = 0.0
    if pf is not None:
        pf[ROW_NEG] = 0.0
    pfd = torch.zeros_like(p) if pf is None else pf
    q = ap + pfd + lam[:, None] * p
    den = (p.double() * q.double()).sum(1)
    a = torch.where(torch.arange(CG_ROWS) % 2 == 0, 0.5, 1.0).double()
    rs = (den * a).float()
    rs[ROW_P0] = 6.0
    rs[ROW_NEG] = 6.0
    rs[ROW_RS0] = 0.0
    return x, r, p, ap, pf, lam, rs


def cg_step_ref(x, r, p, ap, pf, lam, rs):
    """fp64 result of the documented step with its two guards, and the bounds (in units of
    the smallest spacing: 1 for den, 1/2 for x and r, 1/4 for rs') of the exact parts."""
    x, r, p, ap, lam, rs0 = (t.double() for t in (x, r, p, ap, lam, rs))
    pfd = torch.zeros_like(p) if pf is None else pf.double()
    q = ap + pfd + lam[:, None] * p
    den = (p * q).sum(1)
    a = torch.where(den > 0, rs0 / den.clamp_min(1e-30), torch.zeros_like(den))
    x1 = x + a[:, None] * p
    r1 = r - a[:, None] * q
    rs1 = (r1 * r1).sum(1)
    beta = torch.where(rs0 > 0, rs1 / rs0.clamp_min(1e-30), torch.zeros_like(rs0))
    p1 = r1 + beta[:, None] * p
    qa = ap.abs() + pfd.abs() + lam[:, None] * p.abs()
    ra = r.abs() + a[:, None] * qa
    bounds = {"den": float((p.abs() * qa).sum(1).max()),
              "x": float(2 * (x.abs() + a[:, None] * p.abs()).max()),
              "r": float(2 * ra.max()),
              "rs": float(4 * (ra * ra).sum(1).max())}
    return dict(x=x1, r=r1, rs=rs1, p=p1, a=a, beta=beta, den=den, ptol=2.0 ** -22 * (r1.abs() + beta[:, None].abs() * p.abs())), bounds


@pytest.mark.parametrize("with_pf", [False, True], ids=["nopf", "pf"])
@pytest.mark.parametrize("R", RANKS)
def test_cg_inputs_are_exact_in_fp32(R, with_pf):
    x, ax, pf, rhs, lam = _cg_init_case(R, with_pf)
    assert sorted(set(lam.tolist())) == [0.0, 1.0, 2.0]
    assert 0 < cg_init_ref(x, ax, pf, rhs, lam)[2] < F32_EXACT
    case = _cg_step_case(R, with_pf)
    ref, bounds = cg_step_ref(*case)
    for k, b in bounds.items():
        assert 0 < b < F32_EXACT, (k, b)
    normal = torch.ones(CG_ROWS, dtype=torch.bool)
    normal[[ROW_P0, ROW_NEG, ROW_RS0]] = False
    assert bool((ref["den"][normal] >= 1).all()) and ref["den"][ROW_RS0] >= 1
    assert ref["den"][ROW_P0] == 0 and ref["den"][ROW_NEG] < 0 and case[6][ROW_RS0] == 0
    assert set(ref["a"][normal].tolist()) == {0.5, 1.0}      # rs0 / den is exact
    assert not ref["a"][[ROW_P0, ROW_NEG, ROW_RS0]].any() and ref["beta"][ROW_RS0] == 0
    assert torch.equal(case[6].double(), torch.where(normal, ref["den"] * ref["a"], case[6].double()))


@pytest.mark.gpu
@pytest.mark.parametrize("with_pf", [False, True], ids=["nopf", "pf"])
@pytest.mark.parametrize("R", RANKS)
def test_gpu_als_cg_init_bitwise(gpu, R, with_pf):
    """als_cg_kernel<RV, 0>: r = rhs - (ax + pf + lam x), p = r, rs = r.r bitwise; the
    inputs are left untouched."""
    x, ax, pf, rhs, lam = _cg_init_case(R, with_pf)
    dx, dax, drhs, dlam = (t.to(gpu) for t in (x, ax, rhs, lam))
    dpf = None if pf is None else pf.to(gpu)
    r, p, rs = A.cg_init(dx, dax, dpf, drhs, dlam)
    rr, rrs, _ = cg_init_ref(x, ax, pf, rhs, lam)
    assert torch.equal(r.cpu(), rr.float()) and torch.equal(p.cpu(), rr.float())
    assert torch.equal(rs.cpu(), rrs.float())
    assert torch.equal(dx.cpu(), x) and torch.equal(dax.cpu(), ax) and torch.equal(drhs.cpu(), rhs)


@pytest.mark.gpu
@pytest.mark.parametrize("with_pf", [False, True], ids=["nopf", "pf"])
@pytest.mark.parametrize("R", RANKS)
def test_gpu_als_cg_step_bitwise(gpu, R, with_pf):
    """als_cg_kernel<RV, 1>: with q = ap + pf + lam p, a = rs / p.q (0 unless p.q > 0),
    x += a p, r -= a q, rs' = r.r, p = r + (rs' / rs) p (beta = 0 unless rs > 0).

    x, r and rs' are exact on these inputs (integers, a in {0.5, 1}) and must be bitwise.
    p takes two roundings: beta~ = fl(rs' / rs) = beta (1 + e1) and the fused
    p~ = fl(r' + beta~ p) = (r' + beta~ p)(1 + e2), |e1|, |e2| <= 2^-24, hence
    |p~ - p| <= 2^-24 |beta p| + 2^-24 (|r'| + |beta~ p|) <= 2^-23 (|r'| + |beta| |p|) to
    first order; the test allows twice that, 2^-22 (|r'| + |beta| |p_old|) per element.

    Guard rows of the same launch: p = 0 (den == 0) and ap = -3 p (den < 0) leave x and r
    bitwise unchanged; rs == 0 gives beta = 0, so p = r'."""
    x, r, p, ap, pf, lam, rs = _cg_step_case(R, with_pf)
    dx, dr, dp, dap, dlam, drs = (t.to(gpu) for t in (x, r, p, ap, lam, rs))
    dpf = None if pf is None else pf.to(gpu)
    A.cg_step(dx, dr, dp, dap, dpf, dlam, drs)
    ref, _ = cg_step_ref(x, r, p, ap, pf, lam, rs)
    gx, gr, gp, grs = dx.cpu(), dr.cpu(), dp.cpu(), drs.cpu()
    assert torch.equal(gx, ref["x"].float()) and torch.equal(gr, ref["r"].float())
    assert torch.equal(grs, ref["rs"].float())
    assert bool(((gp.double() - ref["p"]).abs() <= ref["ptol"]).all())
    for u in (ROW_P0, ROW_NEG):
        assert torch.equal(gx[u], x[u]) and torch.equal(gr[u], r[u])
    assert torch.equal(gx[ROW_RS0], x[ROW_RS0]) and torch.equal(gp[ROW_RS0], gr[ROW_RS0])
    assert torch.equal(dap.cpu(), ap) and (pf is None or torch.equal(dpf.cpu(), pf))


# --------------------------------------------------------------------------- als_init_kernel

# |norm - 1|: the wave's sum of squares takes at most RV FMAs and 6 reduction levels per
# term (all terms positive: relative error <= 14 * 2^-24, halved by the square root), then
# sqrt, reciprocal, the scaling product and the test's own fp32 input each round once
NORM_TOL = 18 * 2.0 ** -24


@pytest.mark.gpu
@pytest.mark.parametrize("nonneg", [False, True], ids=["signed", "nonneg"])
@pytest.mark.parametrize("row0", [0, 2 ** 32 + 5], ids=["row0", "row2p32"])
@pytest.mark.parametrize("R", INIT_RANKS)
def test_gpu_als_init_kernel(gpu, R, row0, nonneg):
    """als_init_kernel<RV> == the torch draws of init_factors (the tolerance of
    tests/test_als.py), unit row norms, a 64-bit global row index."""
    ref = AE.init_factors(row0, 7, R, 777, torch.device("cpu"), nonneg)
    got = AE.init_factors(row0, 7, R, 777, gpu, nonneg).cpu()
    assert got.shape == (7, R)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)
    assert float((got.double().norm(dim=1) - 1).abs().max()) <= NORM_TOL
    assert not nonneg or bool((got >= 0).all())
    assert nonneg or R == 1 or bool((got < 0).any())


@pytest.mark.gpu
@pytest.mark.parametrize("R", [65, 449])
def test_gpu_als_init_rows_keyed_on_global_index(gpu, R):
    a = AE.init_factors(1000, 7, R, 31, gpu, False)
    b = AE.init_factors(998, 9, R, 31, gpu, False)
    assert torch.equal(a, b[2:])


# ----------------------------------------------------------------------- end to end, R = 192

# Largest per-row relative error against exact_solve_torch (fp64) of the unfused torch CG
# (models/als.py FUSED_CG = False, the project's reference path) on _solve_case(), measured
# on an MI355X; the fused kernels are the same fp32 CG up to rounding: 4x that is allowed.
UNFUSED_CG_ERR = 2.536e-07


@functools.lru_cache(maxsize=None)
def _solve_case():
    R, n, n_other = 192, 60, 300
    g = torch.Generator().manual_seed(192)
    lens = torch.randint(20, 41, (n,), generator=g)
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(lens, 0)
    nnz = int(indptr[-1])
    cols = torch.randint(0, n_other, (nnz,), generator=g, dtype=torch.int32)
    vals = torch.randn(nnz, generator=g) * 2
    F = torch.randn(n_other, R, generator=g) / R ** 0.5
    X0 = torch.randn(n, R, generator=g) / R ** 0.5
    return indptr, cols, vals, F, X0


def _solve_errors(dev, fused):
    """Per-row relative error of solve_side(exact=False, cg_iters=R) against the fp64 solve."""
    indptr, cols, vals, F, X0 = (t.to(dev) for t in _solve_case())
    n, R = X0.shape
    csr = AE.Csr(indptr, cols, vals, 0, n)
    old = AE.FUSED_CG
    AE.FUSED_CG = fused
    try:
        got = AE.solve_side(csr, F, X0, 0.5, False, 1.0, None, R, False, exact=False)
    finally:
        AE.FUSED_CG = old
    w, b, lam = next(iter(csr.cache.values()))
    ref = torch.empty((n, R), dtype=torch.float64, device=dev)
    A.exact_solve_torch(indptr, cols, w, b, F, None, lam, ref)
    return ((got.double() - ref).norm(dim=1) / ref.norm(dim=1)).cpu()


def test_solve_side_cg_reference_path_converges_on_cpu():
    """The case itself is well conditioned (lam_u = 0.5 n_u >= 10 against unit-norm factor
    rows): the fp32 torch CG on the CPU reaches the fp64 solve; the bound is one fp32
    rounding (2^-24) per CG step, 192 steps, accumulating linearly."""
    err = _solve_errors("cpu", False)
    assert float(err.max()) < 192 * 2.0 ** -24, float(err.max())


@pytest.mark.gpu
def test_gpu_solve_side_rank192_cg_matches_exact(gpu):
    """solve_side above rank 128 (no exact kernel there): als_pass_kernel<3, *> and
    als_cg_kernel<3, *> through 192 CG steps, far past convergence, so the den <= 0 and
    rs == 0 guards run too.  Measured largest per-row relative error against the fp64 solve
    on an MI355X: unfused torch CG 2.536e-07 (UNFUSED_CG_ERR), fused kernels 1.983e-07; the
    bound is 4 x the unfused figure, 1.014e-06."""
    fused = _solve_errors(gpu, True)
    assert torch.isfinite(fused).all()
    assert float(fused.max()) <= 4 * UNFUSED_CG_ERR, (float(fused.max()), UNFUSED_CG_ERR)

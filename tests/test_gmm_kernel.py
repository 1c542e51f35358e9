"""Fused GaussianMixture E-step (``ops/gmm.py::estep``, ``csrc/gmm.hip``) against its fp64
reference on the same stored values, and the M-step on its responsibilities.

Data: per-column scales 0.5 - 20 and offsets up to +-50 (what an unshifted fp32 evaluation gets
wrong and what bf16 storage cannot hold).  Model: means drawn from the rows, random SPD
covariances with condition numbers up to 1e3, one component of weight 1e-12.

Accuracy bar (no absolute tolerance): the oracle is ``estep_torch`` in fp64 on the upcast stored
rows, the yardstick the same formula evaluated in float32 by torch on the CPU; the kernel's
max error over ``lse`` and over ``resp`` must be at most

    4 x max(yardstick's max error, 2^-24 max |oracle|)

4x is what the Gram pass is held to against its fp32 chain; the floor is the rounding of an
fp32 result.  On fp32 rows the oracle on rows rounded through bf16 is shown to be at least 10x
that bar away, so a kernel that rounds the rows to bf16 cannot pass.
"""
import numpy as np
import pytest
import torch

from orange3_spark_amd.ops import gmm as GM
from orange3_spark_amd.ops import gram as GR

U = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16

# (n, d, K, row dtype, row stride or None = d rounded up to 8, weighted)
CASES = [
    (1, 3, 1, F32, None, False),
    (31, 8, 2, BF16, None, False),
    (33, 24, 5, F32, None, True),
    (64, 33, 32, BF16, None, False),
    (4099, 3, 32, F32, None, False),
    (4099, 8, 64, F32, None, False),
    (4099, 24, 5, F32, 40, False),          # stride d + 16, padding 7.0
    (4099, 24, 5, BF16, None, True),
    (4099, 33, 2, F32, None, True),
    (4099, 64, 33, F32, None, False),
    (4099, 64, 1, BF16, None, False),
    (64, 64, 64, F32, None, False),
    (4099, 100, 64, BF16, None, False),
    (33, 100, 1, F32, None, False),
    (4099, 128, 5, F32, None, False),
    (31, 128, 33, BF16, None, True),
    (1, 128, 64, BF16, None, False),
    (4099, 136, 2, F32, None, False),       # the first width past 128: nine 16-column steps
    (4099, 200, 5, BF16, None, False),
    (64, 256, 2, F32, None, False),
    (4099, 256, 5, F32, None, True),        # the widest width built
]


def _id(c):
    return (f"n{c[0]}-d{c[1]}-k{c[2]}-{'f32' if c[3] is F32 else 'bf16'}" + (f"-ld{c[4]}" if c[4] else "")
            + ("-w" if c[5] else ""))


def _spd(rng, d, scales):
    """Random SPD matrix in the data's units: condition number of the correlation part up to 1e3."""
    Q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    lam = 10.0 ** rng.uniform(-1.5, 1.5, d)
    return (Q * lam) @ Q.T * np.outer(scales, scales)


def _problem(case):
    n, d, K, dtype, stride, weighted = case
    rng = np.random.default_rng(1000 * d + K)
    scales, offsets = rng.uniform(0.5, 20, d), rng.uniform(-50, 50, d)
    X = rng.normal(size=(n, d)) * scales + offsets
    ld = stride or (d + 7) // 8 * 8
    S = torch.full((n, ld), 7.0, dtype=dtype)
    S[:, :d] = torch.from_numpy(X).to(dtype)
    means = S[rng.integers(0, n, K), :d].double()
    covs = torch.from_numpy(np.stack([_spd(rng, d, scales) for _ in range(K)]))
    wts = rng.uniform(0.5, 1.5, K)
    if K > 1:
        wts[K // 2] = 1e-12 * wts.sum()
    weights = torch.from_numpy(wts / wts.sum())
    w = torch.from_numpy(rng.uniform(0.5, 1.5, n)).float() if weighted else None
    return S, d, weights, means, covs, w


_CACHE = {}


def _reference(case):
    """(problem, fp64 oracle, float32 yardstick) of a case, computed once and left unchanged."""
    if case not in _CACHE:
        S, d, weights, means, covs, w = p = _problem(case)
        _CACHE[case] = (p, GM.estep_torch(S, d, weights, means, covs, w),
                        GM.estep_torch(S, d, weights, means, covs, w, dtype=torch.float32))
    return _CACHE[case]


def _bars(oracle, yard):
    """The bar for resp and for lse."""
    return tuple(4 * max(float((y.double() - o).abs().max()), U * float(o.abs().max())) for o, y in zip(oracle, yard))


def _kernel(case, gpu, nwaves=None):
    (S, d, weights, means, covs, w), _, _ = _reference(case)
    resp, lse = GM.estep(S.to(gpu), d, weights, means, covs, None if w is None else w.to(gpu), nwaves=nwaves)
    assert resp.dtype == lse.dtype == torch.float32 and resp.shape == (case[2], case[0]) and lse.shape == (case[0],)
    assert resp.is_contiguous()
    return resp.cpu(), lse.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_matches_reference(case, gpu):
    n, d, K = case[:3]
    (S, _, weights, means, covs, w), oracle, yard = _reference(case)
    resp, lse = _kernel(case, gpu)
    assert torch.isfinite(resp).all() and torch.isfinite(lse).all()
    bar_r, bar_l = _bars(oracle, yard)
    err_r, err_l = float((resp.double() - oracle[0]).abs().max()), float((lse.double() - oracle[1]).abs().max())
    print(f"{_id(case)}: resp err {err_r:.3e} = {4 * err_r / bar_r:.3f} x bar/4, lse err {err_l:.3e} = "
          f"{4 * err_l / bar_l:.3f} x bar/4 (yardstick errs {float((yard[0].double() - oracle[0]).abs().max()):.3e}, "
          f"{float((yard[1].double() - oracle[1]).abs().max()):.3e})")
    assert err_r <= bar_r and err_l <= bar_l
    # every row of resp sums to 1 (to its row weight) within K 2^-23
    sums = resp.double().sum(0)
    want = torch.ones(n, dtype=torch.float64) if w is None else w.double()
    assert float(((sums - want).abs() / want).max()) <= K * 2.0 ** -23
    assert (resp >= 0).all()
    # two calls are bitwise equal, and so are launches of other sizes
    for nwaves in (None, 4, 20):
        r2, l2 = _kernel(case, gpu, nwaves)
        assert torch.equal(r2, resp) and torch.equal(l2, lse), f"nwaves={nwaves}"


@pytest.mark.parametrize("case", [c for c in CASES if c[3] is F32 and c[0] >= 31], ids=_id)
def test_bar_catches_rows_rounded_to_bf16(case):
    """The oracle on the fp32 rows rounded through bf16 is at least 10x the bar away from the
    oracle on the rows themselves (CPU only: it is a statement about the bar)."""
    (S, d, weights, means, covs, w), oracle, yard = _reference(case)
    _, bar_l = _bars(oracle, yard)
    _, lse_bf = GM.estep_torch(S.to(BF16), d, weights, means, covs, w)
    miss = float((lse_bf - oracle[1]).abs().max())
    print(f"{_id(case)}: bf16-rounded rows miss lse by {miss:.3e} = {miss / bar_l:.1f} x the bar")
    assert miss >= 10 * bar_l


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_outliers_stay_finite(dtype, gpu):
    """Rows 1e4 standard deviations from every mean: finite lse, finite resp, rows still sum to 1."""
    case = (4099, 24, 5, dtype, None, False)
    (S, d, weights, means, covs, _), _, _ = _reference(case)
    S = S.clone()
    sd = S[:, :d].double().std(0)
    far = torch.tensor([0, 31, 32, 63, 64, 1000, 4098])
    S[far, :d] = (S[far, :d].double() + 1e4 * sd * torch.tensor([1.0, -1.0]).repeat(d // 2)).to(dtype)
    resp, lse = GM.estep(S.to(gpu), d, weights, means, covs)
    resp, lse = resp.cpu(), lse.cpu()
    assert torch.isfinite(resp).all() and torch.isfinite(lse).all()
    assert float(lse[far].max()) < -1e6
    assert float((resp.double().sum(0) - 1).abs().max()) <= 5 * 2.0 ** -23
    oracle = GM.estep_torch(S, d, weights, means, covs)
    assert torch.equal(resp[:, far].argmax(0), oracle[0][:, far].argmax(0))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[7], CASES[9], CASES[20]], ids=_id)
def test_mstep_on_the_kernels_responsibilities(case, gpu):
    """``mstep`` on the kernel's resp against the fp64 sums over the same resp, within the bound
    of the weighted Gram pass (u = 2^-24, z = x - shift, F = the rows an fp32 accumulator takes):

        T_ij = (F + 8) u sum_r w_r |z_ri| |z_rj| + u (|c_i| sum w |z_j| + |c_j| sum w |z_i|)

    with the ones column (z = 1, shift 0) for the first moments."""
    n, d, K = case[:3]
    (S, _, weights, means, covs, w), _, _ = _reference(case)
    Xg = S.to(gpu)
    resp, _ = GM.estep(Xg, d, weights, means, covs, None if w is None else w.to(gpu))
    Nk, Sk, Qk = GM.mstep(Xg, d, resp)
    assert Nk.dtype == Sk.dtype == Qk.dtype == torch.float64 and Qk.shape == (K, d, d)
    shift = Xg[: min(n, 1024), :d].to(torch.float32).mean(0).double().cpu()
    X64, r64 = S[:, :d].double(), resp.double().cpu()
    Za = torch.cat([X64 - shift, torch.ones(n, 1, dtype=torch.float64)], 1).abs()
    ca = torch.cat([shift.abs(), torch.zeros(1, dtype=torch.float64)])
    worst = 0.0
    for k in range(K):
        s1 = r64[k] @ Za
        T = (GR.FLUSH_ROWS + 8) * U * ((Za * r64[k][:, None]).T @ Za) + U * (torch.outer(ca, s1) + torch.outer(s1, ca))
        Xw = X64 * r64[k][:, None]
        eq, es = (Qk[k].cpu() - Xw.T @ X64).abs(), (Sk[k].cpu() - Xw.sum(0)).abs()
        worst = max(worst, float((eq / T[:d, :d].clamp_min(1e-300)).max()), float((es / T[:d, d].clamp_min(1e-300)).max()))
        assert abs(float(Nk[k]) - float(r64[k].sum())) <= 1e-12 * max(1.0, float(r64[k].sum()))
    print(f"{_id(case)}: mstep max err / bound = {worst:.4f}")
    assert worst <= 1.0

"""EM passes of a Gaussian mixture over the stored rows.

``estep(X, d, weights, means, covs, w)`` is one streaming pass over bf16 or fp32 rows in the GLM
layout (``csrc/gmm.hip``): per row the K log densities on the matrix cores, their log-sum-exp
and the responsibilities, written component-major ``[K, n]`` in fp32 with no fp64 copy of the
table.  ``mstep(X, d, resp)`` is K passes of :func:`ops.gram.weighted_gram` with ``resp[k]`` as
the row weights.  CPU tensors take the fp64 references, which are also the tests' oracle.

The model enters the kernel as whitening matrices: with Sigma_k = L_k L_k^T (fp64 Cholesky),
W_k = L_k^-1, a per-column shift c (the mean of the first min(n, 1024) rows, as the Gram pass
takes it), b_k = W_k (mu_k - c) and a_k = log w_k - (log det Sigma_k + d log 2 pi) / 2,

    z_k = W_k (x - c) - b_k,   lp_k = a_k - |z_k|^2 / 2.

All of it is prepared here in fp64 (K tiny d x d factorizations); W is split into three bf16
terms and stored in the kernel's fragment order.

``FUSED`` (env ``O3S_GMM_FUSED``, default 1): 0 keeps GaussianMixture on the chunked fp64 path
(``models/clustering_extra.py``), which is what ``tools/bench_gmm.py`` compares against.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import torch

from . import _native as N
from . import glm as _glm
from . import gram as _gram

FUSED = int(os.environ.get("O3S_GMM_FUSED", "1"))
MAX_D = 256          # csrc/gmm.hip kGmMaxNS * 16
MAX_K = 64           # csrc/gmm.hip kGmMaxK


def estep_ok(X: torch.Tensor, d: int, k: int) -> bool:
    """Rows and model sizes the fused E-step takes: the GLM kernels' layout (bf16 or fp32, row
    stride a multiple of 8), 1 <= d <= 256 logical columns, 1 <= k <= 64 components."""
    return (_glm.kernel_rows(X) and X.dim() == 2 and X.shape[1] % 8 == 0 and X.shape[1] >= d
            and 1 <= d <= MAX_D and 1 <= k <= MAX_K)


def _layout(d: int, k: int) -> tuple[int, int, int, int]:
    """(16-column steps, padded coordinates per component, bf16 elements of the split
    coefficients, rows per wave tile) of the kernel for d columns and k components."""
    ns, dp, tr, we = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    N.check(N.kernels().o3s_gmm_layout(d, k, C.byref(ns), C.byref(dp), C.byref(we), C.byref(tr)), "gmm_layout")
    return ns.value, dp.value, we.value, tr.value


def whiten(weights: torch.Tensor, means: torch.Tensor, covs: torch.Tensor, c: torch.Tensor):
    """fp64 (W [K, d, d] = L^-1, b [K, d] = W (mu - c), a [K]) of a mixture and a shift c."""
    d = means.shape[1]
    L = torch.linalg.cholesky(covs)
    eye = torch.eye(d, dtype=covs.dtype, device=covs.device).expand_as(L)
    W = torch.linalg.solve_triangular(L, eye, upper=False)
    b = (W @ (means - c)[:, :, None])[:, :, 0]
    logdet = 2 * torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)
    a = torch.log(weights.clamp_min(1e-300)) - 0.5 * (logdet + d * math.log(2 * math.pi))
    return W, b, a


def estep_torch(X: torch.Tensor, d: int, weights: torch.Tensor, means: torch.Tensor, covs: torch.Tensor,
                w: torch.Tensor | None = None, dtype: torch.dtype = torch.float64):
    """Reference of :func:`estep`: ``gmm_log_prob`` on X[:, :d], its log-sum-exp and softmax, in
    ``dtype`` (fp64: the oracle; fp32: the tests' yardstick).  Returns (resp [K, n], lse [n])."""
    from ..models.clustering_extra import gmm_log_prob
    Xd = X[:, :d].to(dtype)
    dev = Xd.device
    lp = gmm_log_prob(Xd, means.to(dev, dtype), covs.to(dev, dtype),
                      torch.log(weights.to(dev, torch.float64).clamp_min(1e-300)).to(dtype))
    lse = torch.logsumexp(lp, dim=1)
    resp = torch.exp(lp - lse[:, None]).T
    if w is not None:
        resp = resp * w.to(dev, dtype)[None, :]
    return resp.contiguous(), lse


def _pack(W: torch.Tensor, ns: int, dp: int) -> torch.Tensor:
    """fp64 W [K, d, d] -> bf16 [K, dp / 32, ns, 3 (hi, mid, lo), 64 lanes, 8]: lane (r, h) of
    fragment (cb, s) holds W[32 cb + r, 16 s + 8 h .. + 8]."""
    K, d, _ = W.shape
    Wp = torch.zeros((K, dp, 16 * ns), dtype=torch.float64, device=W.device)
    Wp[:, :d, :d] = W
    t = Wp.reshape(K, dp // 32, 32, ns, 2, 8).permute(0, 1, 3, 4, 2, 5)
    hi = t.to(torch.bfloat16)
    r1 = t - hi.to(torch.float64)
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.to(torch.float64)).to(torch.bfloat16)
    return torch.stack([hi, mid, lo], dim=3).reshape(K, dp // 32, ns, 3, 64, 8).contiguous()


def estep(X: torch.Tensor, d: int, weights: torch.Tensor, means: torch.Tensor, covs: torch.Tensor,
          w: torch.Tensor | None = None, nwaves: int | None = None):
    """(resp [K, n] fp32, lse [n] fp32) of the rows X[:, :d] under the mixture (weights [K], means
    [K, d], covs [K, d, d]; any float dtype, taken in fp64): resp[k, r] is the responsibility of
    component k for row r, times w[r] if row weights are given; lse the unweighted log density.
    CUDA rows go to ``csrc/gmm.hip``; CPU tensors take :func:`estep_torch` (fp64 results).

    ``nwaves`` fixes the launch to that many waves (four per block) instead of filling the
    device; the result does not depend on it."""
    if not X.is_cuda:
        return estep_torch(X, d, weights, means, covs, w)
    K = int(weights.shape[0])
    if not estep_ok(X, d, K):
        raise TypeError("estep expects contiguous bf16 or fp32 rows whose stride is a multiple of 8, "
                        f"1 <= d <= {MAX_D} and 1 <= k <= {MAX_K}")
    n, ld = X.shape
    dev = X.device
    ns, dp, w_elems, tile_rows = _layout(d, K)
    wf = None if w is None else w.to(device=dev, dtype=torch.float32).contiguous()
    if wf is not None and wf.shape[0] != n:
        raise ValueError("weights must have one entry per row")
    shift = torch.zeros(16 * ns, dtype=torch.float32, device=dev)
    if n:
        shift[:d] = X[: min(n, 1024), :d].to(torch.float32).mean(0)
    f64 = dict(device=dev, dtype=torch.float64)
    Wk, b, a = whiten(weights.to(**f64), means.to(**f64), covs.to(**f64), shift[:d].to(torch.float64))
    Wp = _pack(Wk, ns, dp)
    if Wp.numel() != w_elems:
        raise N.NativeError(f"kernel library expects {w_elems} coefficient elements, the op packed {Wp.numel()}")
    bp = torch.zeros((K, dp), dtype=torch.float32, device=dev)
    bp[:, :d] = b.to(torch.float32)
    ahi = a.to(torch.float32)
    ak = torch.stack([ahi, (a - ahi.to(torch.float64)).to(torch.float32)], dim=1).contiguous()     # a_k = hi + lo
    resp = torch.empty((K, n), dtype=torch.float32, device=dev)
    lse = torch.empty(n, dtype=torch.float32, device=dev)
    if nwaves is None:
        tiles = (n + tile_rows - 1) // tile_rows
        grid = N.grid_for(dev, tiles, 4, blocks_per_cu=4)
    else:
        grid = max(1, int(nwaves) // 4)
    N.check(N.kernels().o3s_gmm_estep(X.data_ptr(), int(X.dtype == torch.float32), n, ld, d, K, Wp.data_ptr(),
                                      bp.data_ptr(), ak.data_ptr(), shift.data_ptr(), N.ptr(wf), resp.data_ptr(),
                                      lse.data_ptr(), grid, N.stream_of(X)), "gmm_estep")
    return resp, lse


def mstep(X: torch.Tensor, d: int, resp: torch.Tensor):
    """fp64 (Nk [K], Sk [K, d], Qk [K, d, d]) = sums of resp[k], resp[k] x and resp[k] x x^T over
    the rows X[:, :d]: one :func:`ops.gram.weighted_gram` pass per component."""
    st = [_gram.weighted_gram(X, d, w=resp[k]) for k in range(resp.shape[0])]
    return (torch.stack([s.sw for s in st]).to(torch.float64), torch.stack([s.sx for s in st]),
            torch.stack([s.G for s in st]))

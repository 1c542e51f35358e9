"""Squared-Euclidean silhouette over the stored rows (``csrc/silhouette.hip``).

Spark's O(n k) formulation: with per-cluster moments ``Y_j = sum w x``, ``N_j = sum w`` and
``Psi_j = sum w |x|^2`` the mean squared distance of a row to cluster j is

    dist_j = |x|^2 + Psi_j / N_j - 2 x . Y_j / N_j,

``a = dist_own N_own / (N_own - 1)``, ``b = min_{j != own} dist_j`` over the non-empty clusters and
``s = (b - a) / max(a, b)`` (0 for a cluster of weight <= 1).

``cluster_moments`` takes the moments from the stored bf16 / fp32 rows (``ops.binsum``), ``pack``
turns them into the kernel's operands in fp64 -- every quantity about the weighted global mean
``c`` (squared-Euclidean silhouette is translation invariant, and the kernel's fp32 products are
only as good as the coordinates are small) -- and ``silhouette_rows`` is one streaming pass that
writes ``s`` per row in fp32: no fp64 copy of the table and no ``[n, k]`` distance matrix.
``silhouette_torch`` is the fp64 formula: the reference of the tests, the CPU path and the path
of everything the kernel does not take.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as _nat
from . import glm as _glm
from ._terms import split3
from .binsum import bin_sums

MAX_D = 256          # csrc/silhouette.hip kSilMaxNS * 16
MAX_K = 1024         # csrc/silhouette.hip kSilMaxK


def enabled() -> bool:
    """O3S_SILHOUETTE_KERNEL=0: ClusteringEvaluator keeps its torch path (read per call)."""
    return os.environ.get("O3S_SILHOUETTE_KERNEL", "1") != "0"


def gate_reason(is_cuda: bool, dtype, contiguous: bool, ld: int, d: int, k: int) -> str | None:
    """Why rows of this layout and a model of this size do not go to the kernel (None: they do)."""
    if not is_cuda:
        return "rows are not on a GPU"
    if dtype not in (torch.bfloat16, torch.float32):
        return f"row dtype {dtype}"
    if not contiguous or ld % 8 != 0 or ld < d:
        return "rows need to be contiguous with a row stride that is a multiple of 8"
    if not 1 <= d <= MAX_D:
        return f"{d} columns"
    if not 2 <= k <= MAX_K:
        return f"{k} clusters"
    return None


def kernel_ok(X: torch.Tensor, d: int, k: int) -> bool:
    """Rows and sizes the fused pass takes: what ``ops.glm.kernel_rows`` accepts (CUDA bf16 or
    fp32, contiguous, row stride a multiple of 8), 1 <= d <= 256 logical columns, 2 <= k <= 1024."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        return False
    return (gate_reason(X.is_cuda, X.dtype, X.is_contiguous(), X.shape[1], int(d), int(k)) is None
            and _glm.kernel_rows(X))


def column_rows(col, k: int) -> torch.Tensor | None:
    """The stored rows of a vector column if the kernel takes them for k clusters -- a plain
    resident VectorColumn (not lineage, not spilled, not sparse) that :func:`kernel_ok` accepts
    -- else None (the caller keeps its torch path)."""
    from ..frame import column as Cc
    from ..frame.spill import SpilledVectorColumn
    from ..synthetic import LineageVectorColumn
    if isinstance(col, Cc.VectorColumn) and not isinstance(col, (LineageVectorColumn, SpilledVectorColumn)) \
            and kernel_ok(col.data, col.size, k):
        return col.data
    return None


def layout(d: int, k: int) -> tuple[int, int, int, int]:
    """(16-column steps, padded means, bf16 elements of the split means, rows per wave tile) of
    the kernel for d columns and k clusters (``o3s_silhouette_layout``)."""
    ns, kp, tr, me = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    _nat.check(_nat.kernels().o3s_silhouette_layout(d, k, C.byref(ns), C.byref(kp), C.byref(me), C.byref(tr)),
               "silhouette_layout")
    return ns.value, kp.value, me.value, tr.value


def cluster_moments(X: torch.Tensor, c: torch.Tensor, k: int, w: torch.Tensor | None, d: int | None = None):
    """fp64 (Y [k, d], N [k], Psi [k]) = per-cluster sums of w x, w and w |x|^2 over the rows
    X[:, :d] as stored (bf16 / fp32 rows with a row stride go to ``bin_sums_kernel``)."""
    d = X.shape[1] if d is None else d
    st = bin_sums(X if d == X.shape[1] else X[:, :d], c, k, w)
    return st[:, :d].contiguous(), st[:, d].contiguous(), st[:, d + 1].contiguous()


def silhouette_torch(X: torch.Tensor, c: torch.Tensor, k: int, w: torch.Tensor, Y: torch.Tensor, N: torch.Tensor,
                     Psi: torch.Tensor, cosine: bool = False) -> torch.Tensor:
    """fp64 silhouette coefficient of every row of X (fp64 [n, d]; unit rows for ``cosine``), ids
    c (int64 [n]) and the all-reduced moments.  Builds the [n, k] distance matrix."""
    if cosine:
        dist = 1 - (X @ Y.T) / N.clamp_min(1e-300)[None, :]
    else:
        sq = (X * X).sum(1)
        dist = (sq[:, None] * N[None, :] + Psi[None, :] - 2 * X @ Y.T) / N.clamp_min(1e-300)[None, :]
    own = dist.gather(1, c[:, None]).squeeze(1)
    nown = N[c]
    a = torch.where(nown > 1, own * nown / (nown - 1).clamp_min(1e-300), torch.zeros_like(own))
    dist.scatter_(1, c[:, None], float("inf"))
    dist[:, N == 0] = float("inf")
    b = dist.min(1).values
    return torch.where(nown > 1, (b - a) / torch.maximum(a, b).clamp_min(1e-300), torch.zeros_like(a))


def operands(Y: torch.Tensor, N: torch.Tensor, Psi: torch.Tensor):
    """fp64 (c [d], mu' [k, d], const [k], f [k]) of the kernel's formula: c the weighted global
    mean rounded to fp32 (the kernel subtracts it in fp32), mu'_j = Y_j / N_j - c,
    const_j = (Psi_j - 2 c . Y_j + N_j |c|^2) / N_j (+inf for an empty cluster) and
    f_j = N_j / (N_j - 1) (0 for N_j <= 1)."""
    Y, N, Psi = Y.double(), N.double(), Psi.double()
    c = (Y.sum(0) / N.sum().clamp_min(1e-300)).float().double()
    full = N > 0
    Ns = torch.where(full, N, torch.ones_like(N))
    mu = torch.where(full[:, None], Y / Ns[:, None] - c, torch.zeros_like(Y))
    psi = Psi - 2 * (Y @ c) + N * (c @ c)
    const = torch.where(full, psi / Ns, torch.full_like(N, float("inf")))
    f = torch.where(N > 1, N / (N - 1).clamp_min(1e-300), torch.zeros_like(N))
    return c, mu, const, f


def silhouette_formula(X: torch.Tensor, c: torch.Tensor, Y: torch.Tensor, N: torch.Tensor, Psi: torch.Tensor,
                       dtype: torch.dtype = torch.float32, shift: bool = True) -> torch.Tensor:
    """The kernel's formula evaluated by torch in ``dtype`` on X [n, d] (any float dtype): operands
    finished in fp64 (:func:`operands`) and rounded to ``dtype``, then x' = x - c,
    dist_j = |x'|^2 + const_j - 2 x' . mu'_j, a, b and s in ``dtype``.  In float32 it is the tests'
    yardstick for the kernel; ``shift=False`` is the same evaluation about the origin (what a
    kernel that skips the shift would compute)."""
    cc, mu, const, f = operands(Y, N, Psi)
    if not shift:
        Nd = N.double()
        Ns = torch.where(Nd > 0, Nd, torch.ones_like(Nd))
        cc = torch.zeros_like(cc)
        mu = torch.where((Nd > 0)[:, None], Y.double() / Ns[:, None], torch.zeros_like(mu))
        const = torch.where(Nd > 0, Psi.double() / Ns, torch.full_like(Nd, float("inf")))
    xs = X.to(dtype) - cc.to(dtype)
    dist = (xs * xs).sum(1)[:, None] + const.to(dtype)[None, :] - 2 * (xs @ mu.to(dtype).T)
    ci = c.long()
    own = dist.gather(1, ci[:, None]).squeeze(1)
    fo = f.to(dtype)[ci]
    a = own * fo
    b = dist.scatter(1, ci[:, None], float("inf")).min(1).values
    m = torch.maximum(a, b)
    return torch.where((fo != 0) & (m > 0), (b - a) / m, torch.zeros_like(a))


def pack(Y: torch.Tensor, N: torch.Tensor, Psi: torch.Tensor):
    """The kernel's operands from the all-reduced moments, finished in fp64 on their device:
    (shift fp32 [16 ns], zero past d; Mp bf16 [kp / 32, ns, 3 (hi, mid, lo), 64 lanes, 8]: lane
    (r, h) = 32 h + r of fragment (cb, s) holds mu'[32 cb + r, 16 s + 8 h .. + 8]; const fp32
    [kp], +inf for empty and padding clusters; f fp32 [kp]), kp = 32 ceil(k / 32)."""
    k, d = Y.shape
    ns, kp = (d + 15) // 16, 32 * ((k + 31) // 32)
    dev = Y.device
    c, mu, const, f = operands(Y, N, Psi)
    shift = torch.zeros(16 * ns, dtype=torch.float32, device=dev)
    shift[:d] = c.float()
    M = torch.zeros((kp, 16 * ns), dtype=torch.float32, device=dev)
    M[:k, :d] = mu.float()
    t = split3(M.reshape(kp // 32, 32, ns, 2, 8).permute(0, 2, 3, 1, 4))         # [3, cb, s, h, r, 8]
    Mp = t.permute(1, 2, 0, 3, 4, 5).reshape(kp // 32, ns, 3, 64, 8).contiguous()
    cst = torch.full((kp,), float("inf"), dtype=torch.float32, device=dev)
    cst[:k] = const.float()
    fj = torch.zeros(kp, dtype=torch.float32, device=dev)
    fj[:k] = f.float()
    return shift, Mp, cst, fj


def unpack_means(Mp: torch.Tensor, k: int, d: int) -> torch.Tensor:
    """fp64 [k, d]: the sum of the three terms of ``Mp``, back in row-major order."""
    kb, ns = Mp.shape[:2]
    t = Mp.double().sum(2).reshape(kb, ns, 2, 32, 8)                              # [cb, s, h, r, 8]
    return t.permute(0, 3, 1, 2, 4).reshape(32 * kb, 16 * ns)[:k, :d]


def silhouette_rows(X: torch.Tensor, d: int, c: torch.Tensor, Y: torch.Tensor, N: torch.Tensor, Psi: torch.Tensor,
                    grid: int | None = None) -> torch.Tensor:
    """fp32 [n]: the silhouette coefficient of every stored row X[:, :d] (CUDA bf16 or fp32 rows
    in the GLM layout) with cluster ids c in [0, k) and the all-reduced fp64 moments Y [k, d],
    N [k], Psi [k].  At least two clusters must be non-empty.

    ``grid`` fixes the launch to that many blocks of four waves instead of filling the device;
    the result does not depend on it."""
    k = int(Y.shape[0])
    if not kernel_ok(X, d, k):
        raise TypeError("silhouette_rows expects contiguous CUDA bf16 or fp32 rows whose stride is a multiple of "
                        f"8, 1 <= d <= {MAX_D} and 2 <= k <= {MAX_K}")
    n, ld = X.shape
    dev = X.device
    if c.shape[0] != n:
        raise ValueError("one cluster id per row")
    ns, kp, m_elems, tile_rows = layout(d, k)
    shift, Mp, cst, fj = pack(Y.to(dev), N.to(dev), Psi.to(dev))
    if Mp.numel() != m_elems or cst.numel() != kp or shift.numel() != 16 * ns:
        raise _nat.NativeError(f"kernel library expects {m_elems} mean elements, the op packed {Mp.numel()}")
    ci = c.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if grid is None:
        grid = _nat.grid_for(dev, (n + tile_rows - 1) // tile_rows, 4, blocks_per_cu=4)
    _nat.check(_nat.kernels().o3s_silhouette(X.data_ptr(), int(X.dtype == torch.float32), n, ld, d, k, ci.data_ptr(),
                                       shift.data_ptr(), Mp.data_ptr(), cst.data_ptr(), fj.data_ptr(),
                                       out.data_ptr(), max(1, int(grid)), _nat.stream_of(X)), "silhouette")
    return out

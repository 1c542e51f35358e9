"""Reductions over the rows as block-batched GEMMs: ``rows_t_matmul(A, B) = A^T B``.

A plain ``A.T @ B`` with A, B of millions of rows and a small output (Gram matrices,
X^T r gradients, per-cluster sums) maps to a GEMM whose output is one or two tiles and
whose K is the row count: hipBLASLt/rocBLAS then run it on one or two workgroups.  fp64 on
one MI355X (tools/bench_gram.py): 4M x 64 X^T X 426 ms -> 0.69 ms as 1024-row batched
GEMMs summed over the batch; X^T v 92 ms -> 0.4 ms; 20M x 256 X^T X 2.1 s -> 41 ms (the
fp64 matrix peak).  Host tensors take the plain product.

``weighted_gram(X, d, w, y)`` is the fused alternative for the stored rows themselves
(``csrc/gram.hip``): one streaming pass over bf16 or fp32 rows in the GLM layout, d <= 256,
delivers G = X^T W X, sx, xty, sw, sy and syy in fp64 with no fp64 copy of the table.  On it
(for a plain resident vector column of a CUDA session that :func:`gram_kernel_ok` accepts):
LinearRegression's normal equations, PCA, Correlation.corr (pearson), the IRLS step of
GeneralizedLinearRegression, the coefficient-inference summary and the GaussianMixture M-step
(``ops/gmm.py::mstep``: one pass per component, its responsibilities as the weights).  Still on
``rows_t_matmul``: NaiveBayes, lineage and spilled columns, d > 256, CPU sessions, and
spearman correlation (its operand is a rank matrix, not the stored rows).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _native as N
from . import glm as _glm

_BATCH_BYTES = 256 << 20          # bound on the [batches, p, q] partial products
FLUSH_ROWS = 2048                 # most rows one fp32 accumulator of the fused pass takes (csrc/gram.hip kGrFlushRows)


def rows_t_matmul(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """A^T B for A [n, p] and B [n, q] (or [n]: returns [p]) of one dtype."""
    vec = B.dim() == 1
    if vec:
        B = B[:, None]
    if not A.is_cuda or A.shape[0] < 8192:
        out = A.T @ B
        return out[:, 0] if vec else out
    n, p = A.shape
    q = B.shape[1]
    bs = 1024 if max(p, q) <= 64 else 4096
    while (n // bs) * p * q * A.element_size() > _BATCH_BYTES:
        bs *= 2
    nb = n // bs
    head = nb * bs
    out = torch.bmm(A[:head].reshape(nb, bs, p).transpose(1, 2), B[:head].reshape(nb, bs, q)).sum(0)
    if head < n:
        out = out + A[head:].T @ B[head:]
    return out[:, 0] if vec else out


# --------------------------------------------------------------------------- fused pass
@dataclass
class GramStats:
    """fp64 statistics of one pass: G [d, d], sx [d], xty [d], scalars sw, sy, syy (0-dim), the
    ``shift`` [d] the kernel worked with and the most rows one fp32 accumulator took."""
    G: torch.Tensor
    sx: torch.Tensor
    xty: torch.Tensor
    sw: torch.Tensor
    sy: torch.Tensor
    syy: torch.Tensor
    shift: torch.Tensor
    flush_rows: int


def _layout(d: int) -> tuple[int, int, int]:
    """(DA, slab doubles per block, flush_rows) of the kernel for logical width d."""
    da, per_block, flush = C.c_int(), C.c_int(), C.c_int()
    N.check(N.kernels().o3s_gram_layout(d, C.byref(da), C.byref(per_block), C.byref(flush)), "gram_layout")
    return da.value, per_block.value, flush.value


def gram_kernel_ok(X: torch.Tensor, d: int, w: torch.Tensor | None = None) -> bool:
    """Rows the fused pass takes: the GLM kernels' layout (bf16 or fp32, row stride a multiple
    of 8), 1 <= d <= 256 logical columns, weights absent or non-negative."""
    return (_glm.kernel_rows(X) and X.dim() == 2 and X.shape[1] % 8 == 0 and X.shape[1] >= d and 1 <= d <= 256
            and (w is None or w.numel() == 0 or bool((w >= 0).all())))


def unshift(Gz, sz, zty, sw, sy, c):
    """Statistics of x from those of z = x - c (all fp64): G, sx, xty."""
    cs = torch.outer(c, sz)
    G = Gz + (cs + cs.T) + sw * torch.outer(c, c)       # symmetric to the bit when Gz is
    return G, sz + sw * c, zty + sy * c


def weighted_gram_torch(X: torch.Tensor, d: int, w: torch.Tensor | None = None,
                        y: torch.Tensor | None = None) -> GramStats:
    """fp64 reference of :func:`weighted_gram` (CPU tensors; the tests' oracle)."""
    Xd = X[:, :d].to(torch.float64)
    n = Xd.shape[0]
    wd = torch.ones(n, dtype=torch.float64, device=X.device) if w is None else w.to(torch.float64)
    yd = torch.zeros(n, dtype=torch.float64, device=X.device) if y is None else y.to(torch.float64)
    Xw = Xd * wd[:, None]
    return GramStats(Xw.T @ Xd, Xw.sum(0), Xw.T @ yd, wd.sum(), (wd * yd).sum(), (wd * yd * yd).sum(),
                     torch.zeros(d, dtype=torch.float64, device=X.device), 0)


def weighted_gram(X: torch.Tensor, d: int, w: torch.Tensor | None = None, y: torch.Tensor | None = None,
                  nwaves: int | None = None) -> GramStats:
    """G = sum w x x^T, sx = sum w x, xty = sum w y x, sw, sy, syy over the rows of X[:, :d] in
    one pass over the stored rows (``csrc/gram.hip``); CPU tensors take the fp64 reference.

    The kernel works on z = x - shift, shift = the mean of the first min(n, 1024) rows, and the
    shift is undone here in fp64, so callers see plain statistics.  ``nwaves`` fixes the launch
    to that many waves (four per block) instead of filling the device; results are bitwise
    reproducible for a given (n, d, launch)."""
    if not X.is_cuda:
        return weighted_gram_torch(X, d, w, y)
    if not gram_kernel_ok(X, d, None):
        raise TypeError("weighted_gram expects contiguous bf16 or fp32 rows whose stride is a multiple of 8, "
                        "and 1 <= d <= 256")
    n, ld = X.shape
    dev = X.device
    da, per_block, flush = _layout(d)
    if flush != FLUSH_ROWS:
        raise N.NativeError(f"kernel library flushes every {flush} rows, the op expects {FLUSH_ROWS}")
    wf = None if w is None else w.to(device=dev, dtype=torch.float32).contiguous()
    yf = None if y is None else y.to(device=dev, dtype=torch.float32).contiguous()
    if (wf is not None and wf.shape[0] != n) or (yf is not None and yf.shape[0] != n):
        raise ValueError("weights / labels must have one entry per row")
    shift = (X[: min(n, 1024), :d].to(torch.float32).mean(0) if n else torch.zeros(d, device=dev)).contiguous()
    if nwaves is None:
        tiles = (n + 63) // 64
        grid = max(1, min(N.num_cus(dev) * (2 if da <= 160 else 1), (tiles + 15) // 16))
    else:
        grid = max(1, int(nwaves) // 4)
    slab = torch.empty(grid * per_block, dtype=torch.float64, device=dev)
    GA = torch.empty((da, da), dtype=torch.float64, device=dev)
    N.check(N.kernels().o3s_gram(X.data_ptr(), int(X.dtype == torch.float32), n, ld, d, N.ptr(wf), N.ptr(yf),
                                 shift.data_ptr(), slab.data_ptr(), grid, GA.data_ptr(), N.stream_of(X)), "gram")
    c = shift.to(torch.float64)
    # The sums over w and y alone (4 B per row, not the table) are taken in fp64 here instead of
    # from GA's corner: sum w is a chain of positive fp32 terms, its error would be multiplied
    # by c_i c_j when the shift is undone.
    wd = None if wf is None else wf.to(torch.float64)
    sw = torch.tensor(float(n), dtype=torch.float64, device=dev) if wd is None else wd.sum()
    if yf is None:
        sy = syy = torch.zeros((), dtype=torch.float64, device=dev)
    else:
        yd = yf.to(torch.float64)
        wy = yd if wd is None else wd * yd
        sy, syy = wy.sum(), torch.dot(wy, yd)
    G, sx, xty = unshift(GA[:d, :d], GA[:d, da - 1], GA[:d, da - 2], sw, sy, c)
    return GramStats(G, sx, xty, sw, sy, syy, c, flush)


def column_rows(col, w: torch.Tensor | None = None) -> torch.Tensor | None:
    """The stored rows of a vector column if the fused pass takes them -- a plain resident
    VectorColumn (not lineage, not spilled) on a CUDA device that :func:`gram_kernel_ok`
    accepts with weights ``w`` -- else None (the caller keeps its ``rows_t_matmul`` path)."""
    from ..frame import column as Cc
    from ..frame.spill import SpilledVectorColumn
    from ..synthetic import LineageVectorColumn
    if isinstance(col, Cc.VectorColumn) and not isinstance(col, (LineageVectorColumn, SpilledVectorColumn)) \
            and col.data.is_cuda and gram_kernel_ok(col.data, col.size, w):
        return col.data
    return None

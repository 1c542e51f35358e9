"""Factorization-machine ops: the fused loss / gradient pass and the margin pass over the
stored rows (csrc/fm.hip), and their fp64 PyTorch references.

    q_f = sum_i v_if x_i,  s_i = sum_f v_if^2
    m   = w0 + sum_i w_i x_i + 1/2 (sum_f q_f^2 - sum_i s_i x_i^2)
    logistic: l = sw (softplus(m) - y m),  r = sw (sigmoid(m) - y)
    squared:  l = 1/2 sw (m - y)^2,        r = sw (m - y)
    dV_if = sum_rows r q_f x_i - v_if t_i,  t_i = sum_rows r x_i^2
    dw_i  = sum_rows r x_i,  dw0 = sum_rows r

GPU rows that :func:`fm_kernel_ok` accepts go to the HIP kernels; the ``*_torch`` functions
are the references the tests compare against and run on any device.  Loss ids are those of
``ops.glm``: 0 logistic (y in {0, 1}), 2 squared.
"""
from __future__ import annotations

import os

import torch

from . import _native as N
from ._terms import hi_lo, pad_rows, split3
from .glm import LOSS_LOGISTIC, LOSS_SQUARED

MAX_D = 256      # columns of a row the kernels take
MAX_F = 30       # factors: F + 2 of the 32 class rows of a tile (V columns, w, t)


def fm_enabled() -> bool:
    """O3S_FM_KERNEL=0: fit and transform keep their torch paths (read per call)."""
    return os.environ.get("O3S_FM_KERNEL", "1") != "0"


def gate_reason(is_cuda: bool, dtype, row_stride: int, col_stride: int, d: int, F: int) -> str | None:
    """Why rows of this layout do not go to the FM kernels (None: they do)."""
    if not is_cuda:
        return "rows are not on a GPU"
    if dtype not in (torch.bfloat16, torch.float32):
        return f"row dtype {dtype}"
    if col_stride != 1 or row_stride % 8 != 0:
        return "rows need a unit column stride and a row stride that is a multiple of 8"
    if not 1 <= d <= MAX_D:
        return f"{d} columns"
    if not 1 <= F <= MAX_F:
        return f"{F} factors"
    return None


def fm_kernel_ok(X: torch.Tensor, F: int) -> bool:
    """Rows the fused FM passes take: CUDA bf16 or fp32, unit column stride and a row stride
    that is a multiple of 8 (so also the ``[:, :d]`` view of a padded vector column), at most
    256 columns, and ``1 <= F <= 30`` factors."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        return False
    return gate_reason(X.is_cuda, X.dtype, X.stride(0), X.stride(1), X.shape[1], int(F)) is None


def _check_loss(loss: int) -> int:
    if loss not in (LOSS_LOGISTIC, LOSS_SQUARED):
        raise ValueError(f"FM loss must be {LOSS_LOGISTIC} (logistic) or {LOSS_SQUARED} (squared), got {loss}")
    return int(loss)


def _operands(X: torch.Tensor, V: torch.Tensor, w: torch.Tensor, w0):
    """The checked sizes ``(d, F)`` and the :func:`_pack` of the model on the rows' device."""
    d = X.shape[1]
    F = V.shape[1]
    if V.shape[0] != d or w.shape[0] != d:
        raise ValueError(f"V must be [{d}, F] and w [{d}], got {tuple(V.shape)} and {tuple(w.shape)}")
    if not fm_kernel_ok(X, F):
        raise ValueError("FM kernel rows must be CUDA bf16 / fp32 with unit column stride, a row stride that is "
                         f"a multiple of 8, at most {MAX_D} columns, and 1 <= F <= {MAX_F}")
    return (d, F) + _pack(V, w, w0, X.device)


def _pack(V: torch.Tensor, w: torch.Tensor, w0, dev):
    """The kernel operands ``(D, Wsp, sv, w0p, V64)``, built on the device (no host sync): the
    hi + mid + lo bf16 split of the class-major ``[V^T | w]`` padded to [32, D], ``s`` as fp32
    [D], ``w0`` as hi + lo floats, and the fp64 ``V`` the gradient is assembled with.  ``V`` and
    ``w`` enter at fp32."""
    d = V.shape[0]
    D = 32 * (-(-d // 32))
    V32 = V.to(dev, torch.float32)
    Wsp = split3(pad_rows(torch.cat([V32.T, w.to(dev, torch.float32)[None]]), 32, D)).contiguous()
    V64 = V32.double()
    sv = torch.zeros(D, dtype=torch.float32, device=dev)
    sv[:d] = (V64 * V64).sum(1).float()
    w0p = torch.stack(hi_lo(_w0_f64(w0, dev))).contiguous()
    return D, Wsp, sv, w0p, V64


def fm_pass(X: torch.Tensor, y: torch.Tensor, sw: torch.Tensor | None, V: torch.Tensor, w: torch.Tensor, w0,
            loss: int, grid: int | None = None):
    """One fused FM pass over the rows of X (``fm_pass_kernel`` for bf16 rows,
    ``fm_pass_f32_kernel`` for fp32 rows, csrc/fm.hip).

    X bf16 or fp32 [n, d] (:func:`fm_kernel_ok`), y labels and sw weights (or None) of the n
    rows, V [d, F], w [d], w0 a float or a 0-d tensor, ``loss`` 0 (logistic) or 2 (squared).
    Returns fp64 device tensors ``(gV [d, F], gw [d], gw0, loss_sum)``: the gradient of the
    loss sum in V, w, w0 and the loss sum itself.  The tiles of 32 rows are dealt round-robin
    to ``4 * CUs`` slab rows, which the finish sums in fp64 in a fixed order; ``grid`` fixes
    the number of blocks that walk them (default: one slab row per wave), and any grid gives
    the same bits."""
    loss = _check_loss(loss)
    d, F, D, Wsp, sv, w0p, V64 = _operands(X, V, w, w0)
    n = X.shape[0]
    dev = X.device
    slabs = 4 * N.num_cus(dev)
    grid = slabs // 4 if grid is None else int(grid)
    pstride = 32 * D + 33
    partial = torch.empty(slabs * pstride, dtype=torch.float32, device=dev)
    out = torch.empty(pstride, dtype=torch.float64, device=dev)
    y32 = y.to(dev, torch.float32).contiguous()
    sw32 = None if sw is None else sw.to(dev, torch.float32).contiguous()
    if y32.shape[0] != n or (sw32 is not None and sw32.shape[0] != n):
        raise ValueError("labels and weights must have one entry per row")
    lib = N.kernels()
    fn = lib.o3s_fm_pass_f32 if X.dtype == torch.float32 else lib.o3s_fm_pass
    N.check(fn(X.data_ptr(), n, X.stride(0), d, y32.data_ptr(), N.ptr(sw32), Wsp.data_ptr(), sv.data_ptr(),
               w0p.data_ptr(), F, loss, partial.data_ptr(), slabs, grid, out.data_ptr(), N.stream_of(X)), "fm_pass")
    G = out[: 32 * D].view(32, D)
    gV = G[:F, :d].T - V64 * G[F + 1, :d][:, None]
    return gV, G[F, :d], out[32 * D], out[32 * D + 32]


def fm_margin(X: torch.Tensor, V: torch.Tensor, w: torch.Tensor, w0, grid: int | None = None) -> torch.Tensor:
    """Margins of the rows of X (:func:`fm_kernel_ok`) as fp32 [n]: the forward half of
    :func:`fm_pass` alone (``MARGIN`` instantiations of the pass kernels)."""
    d, F, D, Wsp, sv, w0p, _ = _operands(X, V, w, w0)
    n = X.shape[0]
    out = torch.empty(n, dtype=torch.float32, device=X.device)
    if n == 0:
        return out
    if grid is None:
        grid = max(1, min(2 * N.num_cus(X.device), (n + 127) // 128))
    lib = N.kernels()
    fn = lib.o3s_fm_margin_f32 if X.dtype == torch.float32 else lib.o3s_fm_margin
    N.check(fn(X.data_ptr(), n, X.stride(0), d, Wsp.data_ptr(), sv.data_ptr(), w0p.data_ptr(), F, out.data_ptr(),
               int(grid), N.stream_of(X)), "fm_margin")
    return out


def _w0_f64(w0, dev) -> torch.Tensor:
    return torch.as_tensor(w0, dtype=torch.float64).to(dev).reshape(())


def fm_margin_torch(X: torch.Tensor, V: torch.Tensor, w: torch.Tensor, w0) -> torch.Tensor:
    """fp64 reference of :func:`fm_margin` (returns fp64 [n])."""
    Xd = X.to(torch.float64)
    Vd = V.to(Xd.device, torch.float64)
    Q = Xd @ Vd
    s = (Vd * Vd).sum(1)
    return _w0_f64(w0, Xd.device) + Xd @ w.to(Xd.device, torch.float64) + 0.5 * ((Q * Q).sum(1) - (Xd * Xd) @ s)


def fm_pass_torch(X, y, sw, V, w, w0, loss: int):
    """fp64 reference of :func:`fm_pass`, from the formulas in the module docstring (no
    autograd)."""
    loss = _check_loss(loss)
    Xd = X.to(torch.float64)
    dev = Xd.device
    Vd = V.to(dev, torch.float64)
    Q = Xd @ Vd
    s = (Vd * Vd).sum(1)
    X2 = Xd * Xd
    m = _w0_f64(w0, dev) + Xd @ w.to(dev, torch.float64) + 0.5 * ((Q * Q).sum(1) - X2 @ s)
    yd = y.to(dev, torch.float64)
    wd = torch.ones_like(yd) if sw is None else sw.to(dev, torch.float64)
    if loss == LOSS_LOGISTIC:
        r = wd * (torch.sigmoid(m) - yd)
        l = wd * (torch.nn.functional.softplus(m) - yd * m)
    else:
        e = m - yd
        r = wd * e
        l = 0.5 * wd * e * e
    t = X2.T @ r
    gV = Xd.T @ (Q * r[:, None]) - Vd * t[:, None]
    return gV, Xd.T @ r, r.sum(), l.sum()

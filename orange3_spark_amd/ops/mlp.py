"""One-hidden-layer perceptron ops: the fused loss / gradient pass and the logits pass over the
stored rows (csrc/mlp.hip), and their fp64 PyTorch references.

    Z = X W1 + b1,  A = sigmoid(Z),  L = A W2 + b2,  P = softmax(L)
    loss = sum_rows (logsumexp(L) - L[y]),  R = P - onehot(y)
    gW2 = A^T R,  gb2 = sum R,  dZ = (R W2^T) . A . (1 - A),  gW1 = X^T dZ,  gb1 = sum dZ

for ``layers = [d, H, K]``, unweighted rows: exactly ``ml._mlp.forward`` with the summed
cross-entropy.  GPU rows that :func:`mlp_kernel_ok` accepts go to the HIP kernels; the
``*_torch`` functions are the references the tests compare against and run on any device.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch

from . import _native as N
from ._terms import hi_lo, pad_rows, split3

MAX_D = 256      # columns of a row the kernels take
MAX_H = 128      # hidden units: up to four blocks of 32, one wave each
MAX_K = 32       # classes: one block of 32
# hidden blocks x column blocks (ceil(H / 32) * ceil(d / 32)) the kernels are built for; fp32
# rows past one hidden block only up to F32_WIDE_NB column blocks (the wider ones would spill)
MAX_BLOCKS = 16
F32_WIDE_NB = 6


def mlp_enabled() -> bool:
    """O3S_MLP_KERNEL=0: fit and transform keep their torch paths (read per call)."""
    return os.environ.get("O3S_MLP_KERNEL", "1") != "0"


def _blocks_taken(dtype, d: int, H: int) -> bool:
    nh, nb = -(-H // 32), -(-d // 32)
    return nh * nb <= MAX_BLOCKS and (dtype != torch.float32 or nh == 1 or nb <= F32_WIDE_NB)


def gate_reason(is_cuda: bool, dtype, row_stride: int, col_stride: int, d: int, H: int, K: int) -> str | None:
    """Why rows of this layout and a network of this size do not go to the MLP kernels (None:
    they do)."""
    if not is_cuda:
        return "rows are not on a GPU"
    if dtype not in (torch.bfloat16, torch.float32):
        return f"row dtype {dtype}"
    if col_stride != 1 or row_stride % 8 != 0:
        return "rows need a unit column stride and a row stride that is a multiple of 8"
    if not 1 <= d <= MAX_D:
        return f"{d} columns"
    if not 1 <= H <= MAX_H:
        return f"{H} hidden units"
    if not 2 <= K <= MAX_K:
        return f"{K} classes"
    if not _blocks_taken(dtype, d, H):
        return f"{-(-H // 32)} hidden blocks x {-(-d // 32)} column blocks on {dtype} rows"
    return None


def mlp_kernel_ok(X: torch.Tensor, H: int, K: int) -> bool:
    """Rows and sizes the fused MLP passes take: CUDA bf16 or fp32, unit column stride and a row
    stride that is a multiple of 8 (so also the ``[:, :d]`` view of a padded vector column), at
    most 256 columns, 128 hidden units and 32 classes, and ``ceil(H / 32) * ceil(d / 32)`` at most
    16 (on fp32 rows with more than 32 hidden units also at most 192 columns).  The kernels load
    whole 16-B chunks of a row up to its stride, so a view has to start 16-B aligned and early
    enough in its parent's row."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        return False
    d = X.shape[1]
    if gate_reason(X.is_cuda, X.dtype, X.stride(0), X.stride(1), d, int(H), int(K)) is not None:
        return False
    ld = X.stride(0)
    return X.data_ptr() % 16 == 0 and X.storage_offset() % ld + min(32 * (-(-d // 32)), ld) <= ld


def k_index() -> torch.Tensor:
    """int64 [2, 2, 8]: the hidden unit (resp. class) of its block of 32 that element ``e`` of
    lane half ``h`` holds in k-step ``s`` of the permuted W2 (resp. W2^T) operand,
    ``16 s + 8 (e >> 2) + 4 h + (e & 3)``: where the previous MFMA's accumulator registers
    ``8 s .. 8 s + 7`` of that lane half put it."""
    s = torch.arange(2).view(2, 1, 1)
    h = torch.arange(2).view(1, 2, 1)
    e = torch.arange(8).view(1, 1, 8)
    return 16 * s + 8 * (e >> 2) + 4 * h + (e & 3)


@dataclass
class PackedMLP:
    """The operands as the kernels read them.

    ``W1sp`` bf16 [3, 32 NH, D]: hi, mid, lo terms of fp32(W1)^T, zero-padded to NH = ceil(H / 32)
    blocks of units and D = 32 ceil(d / 32) columns.  ``W2p`` bf16 [2, NH, 2, 3, 64, 8]: for W2
    (0) and W2^T (1), hidden block j, k-step s and term t, the MFMA A fragment of lane 32 h + r:
    element e is ``W2[32 j + k_index()[s, h, e], r]`` resp. ``W2[32 j + r, k_index()[s, h, e]]``,
    zero past H and K.  ``bias`` fp32 [b1 hi 32 NH | b1 lo 32 NH | b2 hi 32 | b2 lo 32], b2 hi
    -inf past K: a padded class has probability 0; a padded unit has A = 1/2 but zero W2 rows."""
    d: int
    H: int
    K: int
    W1sp: torch.Tensor
    W2p: torch.Tensor
    bias: torch.Tensor


def pack(W1: torch.Tensor, b1: torch.Tensor, W2: torch.Tensor, b2: torch.Tensor, device=None) -> PackedMLP:
    """The device operands of a network (W1 [d, H], b1 [H], W2 [H, K], b2 [K]), built on
    ``device`` (default: where W1 is) with no host sync.  The weights enter at fp32, the biases
    as two floats each."""
    d, H = W1.shape
    K = W2.shape[1]
    if W2.shape[0] != H or b1.shape != (H,) or b2.shape != (K,):
        raise ValueError(f"MLP operands must be W1 [d, H], b1 [H], W2 [H, K], b2 [K]; got {tuple(W1.shape)}, "
                         f"{tuple(b1.shape)}, {tuple(W2.shape)}, {tuple(b2.shape)}")
    if not (1 <= d <= MAX_D and 1 <= H <= MAX_H and 2 <= K <= MAX_K):
        raise ValueError(f"MLP kernels take d <= {MAX_D}, H <= {MAX_H}, 2 <= K <= {MAX_K}; got {d}, {H}, {K}")
    dev = torch.device(device) if device is not None else W1.device
    NH, D = -(-H // 32), 32 * (-(-d // 32))
    W1p = pad_rows(W1.to(dev, torch.float32).T, 32 * NH, D)
    idx = k_index().to(dev)
    t3 = split3(pad_rows(W2.to(dev, torch.float32), 32 * NH, 32)).view(3, NH, 32, 32)   # [t, j, unit, class]
    fwd = t3[:, :, idx, :].permute(1, 2, 0, 3, 5, 4)               # [t, j, s, h, e, c] -> [j, s, t, h, c, e]
    bwd = t3[:, :, :, idx].permute(1, 3, 0, 4, 2, 5)               # [t, j, u, s, h, e] -> [j, s, t, h, u, e]
    W2p = torch.stack([fwd, bwd]).reshape(2, NH, 2, 3, 64, 8).contiguous()
    bias = torch.zeros(64 * NH + 64, dtype=torch.float32, device=dev)
    b1h, b1l = hi_lo(b1.to(dev, torch.float64))
    b2h, b2l = hi_lo(b2.to(dev, torch.float64))
    bias[:H], bias[32 * NH: 32 * NH + H] = b1h, b1l
    bias[64 * NH + K: 64 * NH + 32] = float("-inf")
    bias[64 * NH: 64 * NH + K], bias[64 * NH + 32: 64 * NH + 32 + K] = b2h, b2l
    return PackedMLP(d, H, K, split3(W1p).contiguous(), W2p, bias)


def _packed_for(X: torch.Tensor, W1, b1, W2, b2, packed: PackedMLP | None) -> PackedMLP:
    H, K = (packed.H, packed.K) if packed is not None else (W1.shape[1], W2.shape[1])
    dp = packed.d if packed is not None else W1.shape[0]
    if X.dim() != 2 or X.shape[1] != dp:
        raise ValueError(f"rows must be [n, {dp}], got {tuple(X.shape)}")
    if not mlp_kernel_ok(X, H, K):
        raise ValueError("MLP kernel rows must be CUDA bf16 / fp32 with unit column stride and a row stride that "
                         f"is a multiple of 8, with d <= {MAX_D}, H <= {MAX_H}, 2 <= K <= {MAX_K} and "
                         "ceil(H / 32) * ceil(d / 32) <= 16 (fp32 rows past H = 32: d <= 192)")
    if packed is None:
        packed = pack(W1, b1, W2, b2, device=X.device)
    return packed


def mlp_pass(X: torch.Tensor, y: torch.Tensor, W1, b1, W2, b2, grid: int | None = None,
             packed: PackedMLP | None = None):
    """One fused pass over the rows of X (``mlp_pass_kernel`` for bf16 rows,
    ``mlp_pass_f32_kernel`` for fp32 rows, csrc/mlp.hip).

    X bf16 or fp32 [n, d] (:func:`mlp_kernel_ok`), y the labels of the n rows in [0, K), W1
    [d, H], b1 [H], W2 [H, K], b2 [K] (or ``packed``, their :func:`pack`).  Returns fp64 device
    tensors ``(gW1 [d, H], gb1 [H], gW2 [H, K], gb2 [K], loss_sum)``.  The tiles of 32 rows are
    dealt round-robin to ``4 * CUs`` slab rows, which the finish sums in fp64 in a fixed order;
    ``grid`` fixes the number of blocks that walk them (default: one per slab row), and any grid
    gives the same bits."""
    p = _packed_for(X, W1, b1, W2, b2, packed)
    d, H, K = p.d, p.H, p.K
    n = X.shape[0]
    dev = X.device
    if y.shape[0] != n:
        raise ValueError("labels must have one entry per row")
    if n == 0:
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)      # noqa: E731
        return z(d, H), z(H), z(H, K), z(K), z()
    NH, D = -(-H // 32), 32 * (-(-d // 32))
    slabs = 4 * N.num_cus(dev)
    grid = slabs if grid is None else int(grid)
    pstride = 32 * NH * D + 1024 * NH + 32 * NH + 33
    partial = torch.empty(slabs * pstride, dtype=torch.float32, device=dev)
    out = torch.empty(pstride, dtype=torch.float64, device=dev)
    y32 = y.to(dev, torch.int32).contiguous()
    lib = N.kernels()
    fn = lib.o3s_mlp_pass_f32 if X.dtype == torch.float32 else lib.o3s_mlp_pass
    N.check(fn(X.data_ptr(), n, X.stride(0), d, H, K, y32.data_ptr(), p.W1sp.data_ptr(), p.W2p.data_ptr(),
               p.bias.data_ptr(), partial.data_ptr(), slabs, grid, out.data_ptr(), N.stream_of(X)), "mlp_pass")
    o2 = 32 * NH * D
    o3 = o2 + 1024 * NH
    o4 = o3 + 32 * NH
    gW1 = out[:o2].view(32 * NH, D)[:H, :d].T
    gW2 = out[o2:o3].view(32, 32 * NH)[:K, :H].T
    return gW1, out[o3:o3 + H], gW2, out[o4:o4 + K], out[o4 + 32]


def mlp_logits(X: torch.Tensor, W1, b1, W2, b2, grid: int | None = None,
               packed: PackedMLP | None = None) -> torch.Tensor:
    """Logits of the rows of X (:func:`mlp_kernel_ok`) as fp32 [n, K]: the forward half of
    :func:`mlp_pass` alone (``LOGITS`` instantiations of the pass kernels)."""
    p = _packed_for(X, W1, b1, W2, b2, packed)
    n = X.shape[0]
    out = torch.empty((n, p.K), dtype=torch.float32, device=X.device)
    if n == 0:
        return out
    if grid is None:
        grid = max(1, min(8 * N.num_cus(X.device), (n + 31) // 32))
    lib = N.kernels()
    fn = lib.o3s_mlp_logits_f32 if X.dtype == torch.float32 else lib.o3s_mlp_logits
    N.check(fn(X.data_ptr(), n, X.stride(0), p.d, p.H, p.K, p.W1sp.data_ptr(), p.W2p.data_ptr(), p.bias.data_ptr(),
               out.data_ptr(), int(grid), N.stream_of(X)), "mlp_logits")
    return out


def _f64(X, W1, b1, W2, b2):
    Xd = X.to(torch.float64)
    return (Xd,) + tuple(t.to(Xd.device, torch.float64) for t in (W1, b1, W2, b2))


def mlp_logits_torch(X, W1, b1, W2, b2) -> torch.Tensor:
    """fp64 reference of :func:`mlp_logits` (returns fp64 [n, K])."""
    Xd, W1d, b1d, W2d, b2d = _f64(X, W1, b1, W2, b2)
    return torch.sigmoid(Xd @ W1d + b1d) @ W2d + b2d


def mlp_pass_torch(X, y, W1, b1, W2, b2):
    """fp64 reference of :func:`mlp_pass`, from the formulas in the module docstring (no
    autograd)."""
    Xd, W1d, b1d, W2d, b2d = _f64(X, W1, b1, W2, b2)
    A = torch.sigmoid(Xd @ W1d + b1d)
    Lg = A @ W2d + b2d
    lse = torch.logsumexp(Lg, dim=1)
    yl = y.to(Xd.device).long()
    rows = torch.arange(Xd.shape[0], device=Xd.device)
    loss = (lse - Lg[rows, yl]).sum()
    R = torch.exp(Lg - lse[:, None])
    R[rows, yl] -= 1.0
    dZ = (R @ W2d.T) * A * (1.0 - A)
    return Xd.T @ dZ, dZ.sum(0), A.T @ R, R.sum(0), loss

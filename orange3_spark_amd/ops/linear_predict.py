"""Multi-output linear scoring op: ``Y = X W^T + b`` with the classifier epilogue (softmax,
argmax) on the stored rows -- the packed operands, the gfx950 kernel
(csrc/linear_predict.hip) and the fp64 PyTorch reference of the same outputs."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as N
from . import glm as G
from ._terms import hi_lo, pad_rows, split3

MAX_D = 256                          # logical columns of a row the kernel takes
MAX_K = 32                           # outputs of one launch
LOG_SOFTMAX_RAW, DIRECT_STORE = 1, 2  # kernel flags


def fused_enabled() -> bool:
    """O3S_LINEAR_PREDICT_FUSED=0: every model keeps its torch path (read per call)."""
    return os.environ.get("O3S_LINEAR_PREDICT_FUSED", "1") != "0"


def gate_reason(is_cuda: bool, dtype, contiguous: bool, width: int, row_stride: int, d: int, K: int) -> str | None:
    """Why rows of this layout do not go to the kernel (None: they do)."""
    if not is_cuda:
        return "rows are not on a GPU"
    if dtype not in (torch.bfloat16, torch.float32):
        return f"row dtype {dtype}"
    if not contiguous or width < 1 or row_stride % 8 != 0:
        return "rows are not contiguous with a row stride that is a multiple of 8"
    if not 1 <= d <= MAX_D or d > width:
        return f"{d} logical columns"
    if K < 1:
        return f"{K} outputs"
    return None


def linear_predict_ok(X: torch.Tensor, d: int, K: int = 1) -> bool:
    """Rows the kernel takes: contiguous CUDA bf16, or fp32 that passes ``ops.glm.f32_rows``,
    with a row stride that is a multiple of 8, ``1 <= d <= 256`` logical columns that the rows
    hold, and at least one output."""
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        return False
    if X.dtype == torch.float32 and not G.f32_rows(X):
        return False
    return gate_reason(X.is_cuda, X.dtype, X.is_contiguous(), X.shape[1], X.stride(0), d, K) is None


def column_rows(col, d: int) -> torch.Tensor | None:
    """The stored rows of a vector column if the kernel takes them -- a plain resident
    VectorColumn (not lineage, not spilled, not sparse) on a CUDA device that
    :func:`linear_predict_ok` accepts for ``d`` columns -- else None (the caller keeps its
    torch path)."""
    from ..frame import column as Cc
    from ..frame.spill import SpilledVectorColumn
    from ..synthetic import LineageVectorColumn
    if isinstance(col, Cc.VectorColumn) and not isinstance(col, (LineageVectorColumn, SpilledVectorColumn)) \
            and d == col.size and linear_predict_ok(col.data, d):
        return col.data
    return None


@dataclass
class PackedLinear:
    """The operands as the kernel reads them, one entry per block of 32 outputs.

    ``wsp`` int16 (bf16 bits) [blocks, 3, 32, D]: hi, mid, lo terms of fp32(W), zero-padded to
    32 outputs and D = 32 ceil(d / 32) columns; ``bias_hi`` + ``bias_lo`` fp32 [blocks, 32]:
    the fp64 bias as two floats; ``W`` fp64 [K, d] and ``b`` fp64 [K] as they came."""
    W: np.ndarray
    b: np.ndarray
    wsp: np.ndarray
    bias_hi: np.ndarray
    bias_lo: np.ndarray
    _dev: dict = field(default_factory=dict, repr=False, compare=False)

    @property
    def K(self) -> int:
        return int(self.W.shape[0])

    @property
    def d(self) -> int:
        return int(self.W.shape[1])

    @property
    def D(self) -> int:
        return int(self.wsp.shape[3])

    def on(self, device) -> tuple:
        """(wsp, bias_hi, bias_lo) on ``device``, uploaded once."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(N.upload_many(device, self.wsp, self.bias_hi, self.bias_lo))
        return self._dev[key]

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev"] = {}
        return st


def pack(W, b=None) -> PackedLinear:
    """fp64 ``W [K, d]`` and ``b [K]`` (None: no bias) -> :class:`PackedLinear`.

    fp32(W) is split into hi + mid + lo by successive bf16 rounding of the fp32 remainder
    (exact: three 8-bit significands hold the 24 bits), the bias into hi = fp32(b) and
    lo = fp32(b - hi), which leaves 2^-48 |b|."""
    W = np.ascontiguousarray(np.asarray(W, dtype=np.float64))
    if W.ndim != 2 or W.shape[0] < 1 or not 1 <= W.shape[1] <= MAX_D:
        raise ValueError(f"W must be [K >= 1, 1 <= d <= {MAX_D}], got {W.shape}")
    K, d = W.shape
    b = np.zeros(K) if b is None else np.ascontiguousarray(np.asarray(b, dtype=np.float64)).reshape(-1)
    if b.shape[0] != K:
        raise ValueError(f"bias has {b.shape[0]} entries for {K} outputs")
    nblk, D = -(-K // MAX_K), 32 * (-(-d // 32))
    terms = split3(pad_rows(torch.from_numpy(W).to(torch.float32), nblk * MAX_K, D))
    wsp = terms.view(3, nblk, MAX_K, D).transpose(0, 1).contiguous()
    bp = torch.zeros(nblk * MAX_K, dtype=torch.float64)
    bp[:K] = torch.from_numpy(b)
    bh, bl = (t.view(nblk, MAX_K).numpy() for t in hi_lo(bp))
    return PackedLinear(W, b, wsp.view(torch.int16).numpy(), bh, bl)


def model_pack(owner, arrays: tuple, make) -> PackedLinear:
    """The packed operands of a fitted model, built by ``pack(*make())`` at the first use and
    kept on ``owner`` for as long as its parameter ``arrays`` are the same objects (strings
    among them compare by value).  Models drop the cache from their pickles."""
    cache = owner.__dict__.get("_lp_cache")
    if cache is None or len(cache[0]) != len(arrays) or not all(
            (a == b) if isinstance(a, str) else (a is b) for a, b in zip(cache[0], arrays)):
        cache = owner.__dict__["_lp_cache"] = (tuple(arrays), pack(*make()))
    return cache[1]


def _outputs(M: torch.Tensor, raw: bool, prob: bool, pred: bool, log_softmax_raw: bool):
    r = p = y = None
    if raw:
        r = M - torch.logsumexp(M, dim=1, keepdim=True) if log_softmax_raw else M
    if prob:
        p = torch.softmax(M, dim=1)
    if pred:
        y = M.argmax(1).to(torch.float64)        # the first of equal maxima
    return r, p, y


def linear_predict_torch(X: torch.Tensor, d: int, packed: PackedLinear, *, raw: bool = True, prob: bool = False,
                         pred: bool = False, log_softmax_raw: bool = False):
    """fp64 reference of :func:`linear_predict` on any device: ``(raw, prob, pred)``, None for
    an output that was not asked for."""
    _check(X, d, packed, raw, prob, pred)
    Xd = X[:, :d].to(torch.float64)
    M = Xd @ torch.from_numpy(packed.W).to(X.device).T + torch.from_numpy(packed.b).to(X.device)
    return _outputs(M, raw, prob, pred, log_softmax_raw)


def _check(X, d, packed, raw, prob, pred):
    if X.dim() != 2 or X.shape[1] < d or d != packed.d:
        raise ValueError(f"rows must be a [n, >= {packed.d}] matrix of {packed.d} logical columns")
    if packed.K > MAX_K and (prob or pred or not raw):
        raise ValueError(f"{packed.K} outputs: more than {MAX_K} only with raw alone")


def launch_grid(X: torch.Tensor, d: int) -> int:
    """Blocks of the default launch: every tile of 32 rows its own wave, up to the blocks the
    CUs hold at once (``o3s_linear_predict_layout``)."""
    lds, bpc = C.c_int(0), C.c_int(0)
    N.check(N.kernels().o3s_linear_predict_layout(int(X.dtype == torch.float32), d, C.byref(lds), C.byref(bpc)),
            "linear_predict_layout")
    tiles = (X.shape[0] + 31) // 32
    return int(max(1, min(N.num_cus(X.device) * bpc.value, (tiles + 3) // 4)))


def linear_predict(X: torch.Tensor, d: int, packed: PackedLinear, *, raw: bool = True, prob: bool = False,
                   pred: bool = False, log_softmax_raw: bool = False, grid: int | None = None,
                   direct_store: bool = False):
    """Score the stored rows ``X`` ([n, ld], bf16 / fp32, :func:`linear_predict_ok`) with the
    packed operands: ``(raw, prob, pred)`` as fp64 tensors ([n, K], [n, K], [n]), None for an
    output that was not asked for.

    ``raw`` holds the margins, with ``log_softmax_raw`` the margins minus their row
    log-sum-exp; ``prob`` the softmax over the K outputs; ``pred`` the index of the largest
    margin (the lowest on equal margins).  More than 32 outputs run as column blocks of 32 and
    only with ``raw`` alone.  ``grid`` fixes the number of blocks (any grid gives the same
    bits); ``direct_store`` takes the kernel's per-lane store instead of the staged one (A/B).
    GPU: one ``linear_predict_kernel`` launch per column block; CPU tensors:
    :func:`linear_predict_torch`."""
    _check(X, d, packed, raw, prob, pred)
    if not X.is_cuda:
        return linear_predict_torch(X, d, packed, raw=raw, prob=prob, pred=pred, log_softmax_raw=log_softmax_raw)
    if not linear_predict_ok(X, d, packed.K):
        raise ValueError("rows must be contiguous bf16 or padded fp32 with a row stride that is a multiple of 8")
    dev, n, K = X.device, X.shape[0], packed.K
    r = torch.empty((n, K), dtype=torch.float64, device=dev) if raw else None
    p = torch.empty((n, K), dtype=torch.float64, device=dev) if prob else None
    y = torch.empty(n, dtype=torch.float64, device=dev) if pred else None
    if n == 0 or not (raw or prob or pred):
        return r, p, y
    wsp, bh, bl = packed.on(dev)
    g = launch_grid(X, d) if grid is None else int(grid)
    flags = (LOG_SOFTMAX_RAW if log_softmax_raw else 0) | (DIRECT_STORE if direct_store else 0)
    lib, st = N.kernels(), N.stream_of(X)
    for blk in range(wsp.shape[0]):
        c0 = blk * MAX_K
        kb = min(MAX_K, K - c0)
        N.check(lib.o3s_linear_predict(X.data_ptr(), int(X.dtype == torch.float32), n, X.stride(0), d,
                                       wsp[blk].data_ptr(), bh[blk].data_ptr(), bl[blk].data_ptr(), kb, flags,
                                       None if r is None else r.data_ptr() + 8 * c0, N.ptr(p), N.ptr(y), K, g, st),
                "linear_predict")
    return r, p, y

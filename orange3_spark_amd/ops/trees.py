"""Tree histogram op: gfx950 kernel (csrc/trees.hip) with a PyTorch reference."""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _native as N
from . import sampling


def _host(x, dtype=np.int64):
    """numpy copy (int64: indices) of a small array given as numpy or a (device) tensor."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def _dev(x, dev):
    return x.to(dev) if isinstance(x, torch.Tensor) else N.upload(_host(x), dev)


def _plan_items(lo, hi, chunk: int):
    """Segments [lo, hi) (host int64) cut into work items of <= ``chunk`` rows: per item its
    segment and bounds (seg_of, it_lo, it_hi), per segment its first item and item count
    (first, n_it).  The ONE plan: these bounds fix the fp32 partials and the fp64 sum order."""
    n_it = (np.maximum(hi - lo, 0) + chunk - 1) // chunk
    first = np.cumsum(n_it) - n_it
    seg_of = np.repeat(np.arange(len(lo)), n_it)
    it_lo = lo[seg_of] + (np.arange(len(seg_of)) - first[seg_of]) * chunk
    it_hi = np.minimum(it_lo + chunk, hi[seg_of])
    return seg_of, it_lo, it_hi, first, n_it


def _range_sums(src: torch.Tensor, C: int, r_lo: torch.Tensor, r_cnt: torch.Tensor, out: torch.Tensor, st) -> None:
    """out[i] = fp64 sum, in row order, of the rows [r_lo[i], r_lo[i] + r_cnt[i]) of ``src``
    ([rows, C], fp32 or fp64): ``slab_range_sum_kernel``, <= 65535 ranges per launch."""
    n = out.shape[0]
    for a in range(0, n, 65535):
        b = min(a + 65535, n)
        N.check(N.kernels().o3s_slab_range_sum(src.data_ptr(), int(src.dtype == torch.float64), C, r_lo[a:].data_ptr(),
                                               r_cnt[a:].data_ptr(), b - a, out[a:].data_ptr(), st), "slab_range_sum")


def _bins_src(bins, bins_t):     # (matrix, row stride, column stride) of the per-row feature reads
    return (bins_t, 1, bins.shape[0]) if bins_t is not None else (bins, bins.shape[1], 1)


def _check_target(target: torch.Tensor | None, n: int) -> None:
    if target is not None and (target.dtype != torch.float32 or target.numel() != n or not target.is_contiguous()):
        raise ValueError("target must be a contiguous fp32 [n] tensor")


def hist_kernel_ok(bins: torch.Tensor, B: int, S: int, cls: bool) -> bool:
    if not bins.is_cuda or bins.dtype != torch.uint8:
        return False
    F = bins.shape[1]
    fp = 4
    while fp < F and fp < 64:
        fp <<= 1
    return N.kernels().o3s_tree_hist_lds(fp, B, S, int(cls)) > 0


def bin_block(X: torch.Tensor, tht, Tp, out: torch.Tensor, out_t: torch.Tensor | None, ldt: int) -> None:
    """``bin_features_kernel`` on a row block X (fp32 / bf16; thresholds ``tht`` [F, Tp]): bins
    into ``out`` and, with ``out_t`` (row length ``ldt``), feature-major in the same pass."""
    n, F = X.shape
    N.check(N.kernels().o3s_bin_features2(X.data_ptr(), int(X.dtype == torch.bfloat16), n, X.stride(0), F,
                                          tht.data_ptr(), Tp, out.data_ptr(), N.ptr(out_t), ldt, N.stream_of(X)),
            "bin_features")


def forest_weights(rows: torch.Tensor, seeds, rate: float, bootstrap: bool, w: torch.Tensor | None) -> torch.Tensor:
    """fp32 [len(seeds), n]: ``w`` times every tree's bootstrap / subsample weights in ONE
    launch (``forest_weights_kernel``): ``models.trees.subsample_weights``' draws per seed."""
    dev = rows.device
    seeds = np.asarray(seeds, dtype=np.uint32)
    table = sampling.poisson_table(rate, dev) if bootstrap else None
    wf = None if w is None else w.to(dev, torch.float32).contiguous()
    out = torch.empty((len(seeds), rows.shape[0]), dtype=torch.float32, device=dev)
    r64 = rows.to(torch.int64).contiguous()
    N.check(N.kernels().o3s_forest_weights(r64.data_ptr(), r64.shape[0], N.upload(seeds.view(np.int32), dev).data_ptr(),
                                           len(seeds), N.ptr(table), 0 if table is None else table.numel(),
                                           float(rate), N.ptr(wf), out.data_ptr(), N.stream_of(out)),
            "forest_weights")
    return out


# row-major bins -> the feature-major copy written in the same pass by the binning kernel
# (models/trees.bin_features), so feature_major() needs no second pass over the matrix.
# Kept as an attribute of the bins tensor itself: it lives exactly as long as the bins (a
# WeakKeyDictionary keyed by tensors compares keys with Tensor.__eq__ on hash collisions).
def remember_feature_major(bins: torch.Tensor, bins_t: torch.Tensor) -> None:
    bins._o3s_feature_major = bins_t


def feature_major(bins: torch.Tensor) -> torch.Tensor | None:
    """[F, n] copy of the binned matrix for the partition's per-row feature reads (GPU;
    the binning kernel's own feature-major output when it wrote one, else the LDS-tiled
    ``u8_transpose_kernel``, F % 4 == 0, or torch's strided copy)."""
    if not bins.is_cuda:
        return None
    fm = getattr(bins, "_o3s_feature_major", None)
    if fm is not None:
        return fm
    n, F = bins.shape
    if F % 4 != 0 or not bins.is_contiguous():
        return bins.t().contiguous()
    out = torch.empty((F, n), dtype=torch.uint8, device=bins.device)
    N.check(N.kernels().o3s_u8_transpose(bins.data_ptr(), n, F, out.data_ptr(), N.stream_of(bins)), "u8_transpose")
    return out


PART_CHUNK = int(os.environ.get("O3S_PART_CHUNK", str(1 << 14)))   # rows per partition work item


def partition(bins: torch.Tensor, order: torch.Tensor, s_lo: torch.Tensor, s_hi: torch.Tensor,
              s_feat: torch.Tensor, s_bin: torch.Tensor, chunk: int | None = None, bins_t: torch.Tensor | None = None,
              out: torch.Tensor | None = None, payload=(), payload_out=()):
    """Stable split of every segment [s_lo, s_hi) of ``order`` into rows with
    bins[row, feat] <= bin (first) and the rest.  Returns (new_order, nleft per segment).

    ``out`` (GPU): write the split segments into this buffer and leave every other
    position of it untouched (ping-pong buffers of a caller that no longer needs the
    rows outside the split segments); default: a full copy of ``order`` first.

    ``payload`` (<= 2 fp32 arrays in POSITION order, e.g. y and w): moved with the rows
    into the matching ``payload_out`` buffers (same rule as ``out``: positions outside
    the split segments are not written).

    GPU: two passes of ``tree_part_*_kernel`` over work items (count, then scatter to
    destinations from ``tree_part_dest_kernel``); CPU: the PyTorch reference."""
    payload, payload_out = tuple(payload), tuple(payload_out)
    chunk = chunk or PART_CHUNK
    if len(payload) != len(payload_out) or len(payload) > 2:
        raise ValueError("payload / payload_out mismatch")
    if not (bins.is_cuda and order.dtype == torch.int32):
        dv = bins.device
        return partition_torch(bins, order, _dev(s_lo, dv), _dev(s_hi, dv), _dev(s_feat, dv), _dev(s_bin, dv),
                               out=out, payload=payload, payload_out=payload_out)
    dev = bins.device
    # work items planned on the host (segment bounds are tiny) and uploaded in one copy
    lo, hi = _host(s_lo), _host(s_hi)
    nseg = len(lo)
    seg_of, it_lo_h, it_hi_h, first, _ = _plan_items(lo, hi, chunk)
    n_items = len(seg_of)
    new_order = order.clone() if out is None else out
    if n_items == 0:
        return new_order, torch.zeros(nseg, dtype=torch.int64, device=dev)
    seg_first = np.append(first, n_items)
    fb = np.concatenate([_host(s_feat).astype(np.int32)[seg_of], _host(s_bin).astype(np.int32)[seg_of]])
    i64, i32 = N.upload_many(dev, np.concatenate([it_lo_h, it_hi_h, seg_first, lo]).astype(np.int64), fb)
    it_lo, it_hi = i64[:n_items], i64[n_items:2 * n_items]
    seg_first_d, seg_lo_d = i64[2 * n_items:2 * n_items + nseg + 1], i64[2 * n_items + nseg + 1:]
    it_feat, it_bin = i32[:n_items], i32[n_items:]
    work = torch.empty(3 * n_items + nseg, dtype=torch.int64, device=dev)
    it_left, dst_left, dst_right = work[:n_items], work[n_items:2 * n_items], work[2 * n_items:3 * n_items]
    nleft = work[3 * n_items:]
    flags = torch.empty(order.shape[0], dtype=torch.uint8, device=dev)
    lib = N.kernels()
    st = N.stream_of(bins)
    src, rs, cs = _bins_src(bins, bins_t)
    N.check(lib.o3s_tree_partition(src.data_ptr(), rs, cs, order.data_ptr(), None, it_lo.data_ptr(), it_hi.data_ptr(),
                                   it_feat.data_ptr(), it_bin.data_ptr(), it_left.data_ptr(), None, None,
                                   flags.data_ptr(), n_items, 0, None, None, None, None, st), "tree_part_count")
    N.check(lib.o3s_tree_part_dest(it_lo.data_ptr(), it_hi.data_ptr(), it_left.data_ptr(), seg_first_d.data_ptr(),
                                   seg_lo_d.data_ptr(), nseg, dst_left.data_ptr(), dst_right.data_ptr(),
                                   nleft.data_ptr(), st), "tree_part_dest")
    pl = [None] * 4
    for q, (a, b) in enumerate(zip(payload, payload_out)):
        if a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != order.numel() \
                or b.numel() != order.numel() or not (a.is_contiguous() and b.is_contiguous()):
            raise ValueError("payloads must be contiguous fp32 arrays of the order's length")
        pl[2 * q], pl[2 * q + 1] = a.data_ptr(), b.data_ptr()
    N.check(lib.o3s_tree_partition(src.data_ptr(), rs, cs, order.data_ptr(), new_order.data_ptr(), it_lo.data_ptr(),
                                   it_hi.data_ptr(), it_feat.data_ptr(), it_bin.data_ptr(), None,
                                   dst_left.data_ptr(), dst_right.data_ptr(), flags.data_ptr(), n_items, 1, *pl, st),
            "tree_part_scatter")
    return new_order, nleft


def final_level(bins: torch.Tensor, order: torch.Tensor, s_lo, s_hi, s_feat, s_bin, vl, vr, y: torch.Tensor,
                w: torch.Tensor | None, acc: torch.Tensor | None, need_y2: bool,
                bins_t: torch.Tensor | None = None, chunk: int = 1 << 14):
    """Last split level of a tree: rows of every splitting segment are routed by its
    split; ``acc`` (fp64 [n], boosting) gets the left / right child's leaf value per row
    (``vl`` / ``vr`` per segment) and, with ``need_y2``, the children's sums of w*y^2
    (fp64 [nseg, 2]: left, right; y / w in position order) are returned, else None.

    GPU: ``tree_final_level_kernel`` + ordered fp64 range sums; CPU: ``final_level_torch``."""
    if not (bins.is_cuda and order.dtype == torch.int32):
        return final_level_torch(bins, order, s_lo, s_hi, s_feat, s_bin, vl, vr, y, w, acc, need_y2)
    lo, hi = _host(s_lo), _host(s_hi)
    nseg = len(lo)
    dev = bins.device
    vl, vr = np.asarray(vl, dtype=np.float64), np.asarray(vr, dtype=np.float64)
    seg_of, it_lo, it_hi, first, n_it = _plan_items(lo, hi, chunk)
    n_items = len(seg_of)
    if n_items == 0:
        return torch.zeros((nseg, 2), dtype=torch.float64, device=dev) if need_y2 else None
    fb = np.concatenate([_host(s_feat).astype(np.int32)[seg_of], _host(s_bin).astype(np.int32)[seg_of]])
    i64, i32, f64 = N.upload_many(dev, np.concatenate([it_lo, it_hi, first, n_it]).astype(np.int64), fb,
                                  np.concatenate([vl[seg_of], vr[seg_of]]))
    part = torch.empty((n_items, 2), dtype=torch.float32, device=dev) if need_y2 else None
    yf = y.to(torch.float32).contiguous() if need_y2 else None
    wf = None if (w is None or not need_y2) else w.to(torch.float32).contiguous()
    src, rs, cs = _bins_src(bins, bins_t)
    st = N.stream_of(bins)
    N.check(N.kernels().o3s_tree_final_level(src.data_ptr(), rs, cs, order.data_ptr(), i64[:n_items].data_ptr(),
                                             i64[n_items:2 * n_items].data_ptr(), i32[:n_items].data_ptr(),
                                             i32[n_items:].data_ptr(), f64[:n_items].data_ptr(),
                                             f64[n_items:].data_ptr(), N.ptr(yf), N.ptr(wf), N.ptr(acc), N.ptr(part),
                                             n_items, st), "tree_final_level")
    if not need_y2:
        return None
    out = torch.empty((nseg, 2), dtype=torch.float64, device=dev)
    # item partials summed per segment, in order
    _range_sums(part, 2, i64[2 * n_items:2 * n_items + nseg], i64[2 * n_items + nseg:], out, st)
    return out


def final_level_torch(bins, order, s_lo, s_hi, s_feat, s_bin, vl, vr, y, w, acc, need_y2):
    """Reference of ``final_level``: fp64 gathers and scatter-adds over the segments' rows."""
    lo, hi = _host(s_lo), _host(s_hi)
    nseg = len(lo)
    dev = bins.device
    vl, vr = np.asarray(vl, dtype=np.float64), np.asarray(vr, dtype=np.float64)
    F = bins.shape[1]
    lens = np.maximum(hi - lo, 0)
    sid = np.repeat(np.arange(nseg), lens)
    pos = torch.from_numpy(np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]) if lens.sum()
                           else np.zeros(0, dtype=np.int64)).to(dev)
    rows = order[pos].long()
    fe = torch.from_numpy(_host(s_feat)[sid]).to(dev)
    bb = torch.from_numpy(_host(s_bin)[sid]).to(dev)
    left = bins.view(-1)[rows * F + fe].to(torch.int64) <= bb
    sid_t = torch.from_numpy(sid).to(dev)
    if acc is not None:
        v = torch.where(left, torch.from_numpy(vl[sid]).to(dev), torch.from_numpy(vr[sid]).to(dev))
        acc.index_add_(0, rows.to(acc.device), v.to(acc.dtype))
    if not need_y2:
        return None
    yy = y[pos].to(torch.float64)
    ww = torch.ones_like(yy) if w is None else w[pos].to(torch.float64)
    out = torch.zeros((nseg, 2), dtype=torch.float64, device=dev)
    out.view(-1).index_add_(0, sid_t * 2 + (~left).long(), ww * yy * yy)
    return out


def leaf_apply(order: torch.Tensor, seg_lo: torch.Tensor, seg_hi: torch.Tensor, seg_val: torch.Tensor,
               acc: torch.Tensor, chunk: int = 1 << 14) -> None:
    """acc[order[p]] += seg_val[s] for every position p of segment s (fp64 acc).

    GPU: ``tree_leaf_apply_kernel`` over <= chunk-row items planned on the host; CPU: ``leaf_apply_torch``."""
    if not (acc.is_cuda and order.dtype == torch.int32 and acc.dtype == torch.float64):
        return leaf_apply_torch(order, seg_lo, seg_hi, seg_val, acc)
    seg_of, it_lo, it_hi, _, _ = _plan_items(_host(seg_lo), _host(seg_hi), chunk)
    n_items = len(seg_of)
    if n_items == 0:
        return
    i64, fv = N.upload_many(acc.device, np.concatenate([it_lo, it_hi]).astype(np.int64),
                            np.ascontiguousarray(_host(seg_val, np.float64)[seg_of], dtype=np.float64))
    N.check(N.kernels().o3s_tree_leaf_apply(order.data_ptr(), i64[:n_items].data_ptr(), i64[n_items:].data_ptr(),
                                            fv.data_ptr(), n_items, acc.data_ptr(), N.stream_of(acc)),
            "tree_leaf_apply")


def leaf_apply_torch(order, seg_lo, seg_hi, seg_val, acc) -> None:
    lo, hi = _host(seg_lo), _host(seg_hi)
    lens = np.maximum(hi - lo, 0)
    if lens.sum() == 0:
        return
    pos = torch.from_numpy(np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)])).to(order.device)
    v = torch.from_numpy(np.repeat(_host(seg_val, np.float64), lens)).to(acc.device, acc.dtype)
    acc.index_add_(0, order[pos].long().to(acc.device), v)


_KINDS = {"variance": 0, "gini": 1, "entropy": 2}
_GBT_LOSS = {"logistic": 0, "squared": 1, "absolute": 2}


def gbt_point_loss(loss: str, yy: torch.Tensor, Fm: torch.Tensor) -> torch.Tensor:
    """Spark GBT per-row loss (logistic: 2*log(1 + e^{-2yF}), evaluated stably)."""
    if loss == "logistic":
        z = -2.0 * yy * Fm
        return 2.0 * torch.where(z > 0, z + torch.log1p(torch.exp(-z)), torch.log1p(torch.exp(z)))
    if loss == "squared":
        return (yy - Fm) ** 2
    return (yy - Fm).abs()


def gbt_residual(loss: str, yy: torch.Tensor, Fm: torch.Tensor) -> torch.Tensor:
    """Pseudo-residuals (negative loss gradients) the next tree is fit to."""
    if loss == "logistic":
        return 4.0 * yy / (1.0 + torch.exp(2.0 * yy * Fm))
    if loss == "squared":
        return 2.0 * (yy - Fm)
    return torch.sign(yy - Fm)


def gbt_grad_loss(loss: str, yy: torch.Tensor, Fm: torch.Tensor, w: torch.Tensor | None, w_val: torch.Tensor | None,
                  target: torch.Tensor | None = None) -> torch.Tensor:
    """One boosting epilogue pass: returns fp64 [sum loss*w, sum w, sum loss*w_val,
    sum w_val] over the local rows and (``target`` given, fp32) writes the residuals of
    the next tree into it.  GPU: ``gbt_grad_loss_kernel`` (one fused pass, fixed-grid
    partial sums); CPU: ``gbt_grad_loss_torch``."""
    n = yy.shape[0]
    if not (yy.is_cuda and n > 0):
        return gbt_grad_loss_torch(loss, yy, Fm, w, w_val, target)
    f64 = [None if t is None else t.to(torch.float64).contiguous() for t in (yy, Fm, w, w_val)]
    nb = int(min(2048, max(1, (n + 255) // 256)))
    part = torch.empty((nb, 4), dtype=torch.float64, device=yy.device)
    _check_target(target, n)
    N.check(N.kernels().o3s_gbt_grad_loss(*(N.ptr(t) for t in f64), n, _GBT_LOSS[loss], N.ptr(target),
                                          part.data_ptr(), nb, N.stream_of(yy)), "gbt_grad_loss")
    return part.sum(0)


def gbt_grad_loss_torch(loss, yy, Fm, w, w_val, target=None):
    """Reference of ``gbt_grad_loss`` (fp64 torch reductions)."""
    dev = yy.device
    pl = gbt_point_loss(loss, yy.double(), Fm.double())
    wt = torch.ones_like(pl) if w is None else w.double()
    out = [(pl * wt).sum(), wt.sum()]
    if w_val is not None:
        out += [(pl * w_val.double()).sum(), w_val.double().sum()]
    else:
        out += [torch.zeros((), dtype=torch.float64, device=dev)] * 2
    if target is not None:
        target.copy_(gbt_residual(loss, yy.double(), Fm.double()))
    return torch.stack(out)


LEAF_PASS_MAX_DEPTH = 10            # 2^D per-leaf y^2 columns per wave fit the kernel's LDS


def tree_node_arrays(feature: np.ndarray, split_bin: np.ndarray, value: np.ndarray, scale: float):
    """Heap-ordered tree -> (node_fb int32 [nodes]: feature | bin << 16 for internal
    nodes, -1 for leaves / absent; node_val fp64 [nodes]: leaf value * scale)."""
    fe = np.asarray(feature, dtype=np.int64)
    fb = np.where(fe >= 0, fe | (np.asarray(split_bin, dtype=np.int64) << 16), -1).astype(np.int32)
    return fb, np.asarray(value, dtype=np.float64).reshape(len(fe), -1)[:, 0] * float(scale)


LEAF_BLOCKS_PER_CU = int(os.environ.get("O3S_LEAF_BLOCKS", "4"))     # gbt_leaf_pass_kernel grid (A/B 4 / 8 / 16: 12.2 / 12.6 / 13.5 ms per tree)


def gbt_leaf_pass(bins: torch.Tensor, feature, split_bin, value, scale: float, depth: int, loss: str,
                  yy: torch.Tensor, Fm: torch.Tensor, wt: torch.Tensor | None, wd: torch.Tensor | None,
                  wv: torch.Tensor | None, first: bool, target: torch.Tensor | None, need_y2: bool):
    """The GBT tree epilogue in ONE pass over the rows in row order (``gbt_leaf_pass_kernel``):
    every row walks the finished tree on its bins, ``Fm += scale * value(leaf)``, the loss
    partials of the updated ensemble [sum l*wd, sum wd, sum l*wv, sum wv] (fp64 [4]) are
    returned, ``target`` (fp32, optional) receives the next tree's residuals, and with
    ``need_y2`` the sums of wt*y^2 of the leaves at depth ``depth`` (fp64 [2^depth], y =
    the residual this tree was fit to: yy for the first tree, else the loss gradient at
    the pre-update Fm) -- the last level's children impurities.  CPU: ``gbt_leaf_pass_torch``."""
    n, F = bins.shape
    dev = bins.device
    if not bins.is_contiguous():                     # the kernel reads row i at bins + i * F
        raise ValueError("bins must be a contiguous [n, F] matrix")
    if not (bins.is_cuda and n > 0):
        return gbt_leaf_pass_torch(bins, feature, split_bin, value, scale, depth, loss, yy, Fm, wt, wd, wv, first,
                                   target, need_y2)
    fb, val = tree_node_arrays(feature, split_bin, value, scale)
    L = 1 << depth
    f64 = [None if t is None else t.to(torch.float64).contiguous() for t in (wd, wv)]
    wt32 = None if wt is None else wt.to(torch.float32).contiguous()
    _check_target(target, n)
    if not (yy.dtype == torch.float64 and Fm.dtype == torch.float64 and yy.is_contiguous() and Fm.is_contiguous()):
        raise ValueError("yy / Fm must be contiguous fp64")
    grid = int(max(1, min(N.num_cus(dev) * LEAF_BLOCKS_PER_CU, (n + 255) // 256)))
    part = torch.empty((grid, 4), dtype=torch.float64, device=dev)
    slab = torch.empty((grid * 4, L), dtype=torch.float32, device=dev) if need_y2 else None   # a row per wave
    fb_d, val_d = N.upload_many(dev, fb, val)
    st = N.stream_of(Fm)
    N.check(N.kernels().o3s_gbt_leaf_pass(bins.data_ptr(), n, F, fb_d.data_ptr(), len(fb), val_d.data_ptr(), depth,
                                          yy.data_ptr(), Fm.data_ptr(), N.ptr(wt32), N.ptr(f64[0]), N.ptr(f64[1]),
                                          _GBT_LOSS[loss], int(first), N.ptr(target), part.data_ptr(), N.ptr(slab),
                                          grid, st), "gbt_leaf_pass")
    y2 = None
    if need_y2:
        y2 = torch.empty((1, L), dtype=torch.float64, device=dev)
        lo, cnt = N.upload_many(dev, np.zeros(1, np.int64), np.full(1, grid * 4, np.int64))
        _range_sums(slab, L, lo, cnt, y2, st)
        y2 = y2[0]
    return part.sum(0), y2


def gbt_leaf_pass_torch(bins, feature, split_bin, value, scale, depth, loss, yy, Fm, wt, wd, wv, first, target,
                        need_y2):
    """Reference of ``gbt_leaf_pass``: walk the tree, update, loss / residual, per-leaf y^2."""
    n = bins.shape[0]
    dev = bins.device
    fb, val = tree_node_arrays(feature, split_bin, value, scale)
    L = 1 << depth
    fb_t = torch.from_numpy(fb.astype(np.int64)).to(dev)
    node = torch.ones(n, dtype=torch.int64, device=dev)
    for _ in range(depth):
        code = fb_t[node]
        inner = code >= 0
        if not bool(inner.any()):
            break
        f = torch.where(inner, code & 0xFFFF, torch.zeros_like(code))
        sb = (code >> 16) & 0x7FFF
        b = bins.gather(1, f[:, None]).squeeze(1).to(torch.int64)
        node = torch.where(inner, 2 * node + (b > sb).to(torch.int64), node)
    Fo = Fm.clone()
    Fm += torch.from_numpy(val).to(dev)[node]
    out = gbt_grad_loss_torch(loss, yy, Fm, wd, wv, target)
    y2 = None
    if need_y2:
        yo = yy.to(torch.float32) if first else gbt_residual(loss, yy.double(), Fo.double()).to(torch.float32)
        ww = torch.ones_like(yo) if wt is None else wt.to(torch.float32)
        v = (ww * yo * yo).to(torch.float64)
        at = node >= L
        y2 = torch.zeros(L, dtype=torch.float64, device=dev)
        y2.index_add_(0, (node[at] - L), v[at])
    return out, y2


def best_splits(H: torch.Tensor, nb: torch.Tensor, fmask, kind: str, min_inst: float, min_w: float,
                min_wfrac: float, min_w_node=None) -> torch.Tensor:
    """Per-node best split of histograms H [k, F, B, S] (fp64, GPU) in ONE launch of
    ``tree_split_kernel``.  Returns the fp64 bundle [idx | gain | impurity | weight |
    wL | wR | values (k x V)] (V = S for classification, 1 for variance).

    ``fmask`` (numpy bool [k, F] or None): features each node may split on (forests);
    ``min_wfrac`` > 0: the minimum child weight is that fraction of the node's weight
    (the root level), else ``min_w``; ``min_w_node`` (numpy [k]) overrides both per node.
    CPU: ``best_splits_torch``."""
    if not H.is_cuda:
        return best_splits_torch(H, nb, fmask, kind, min_inst, min_w, min_wfrac, min_w_node)
    k, F, B, S = H.shape
    dev = H.device
    Hc = H.to(torch.float64).contiguous()
    nb32 = nb.to(dev, torch.int32).contiguous()
    fm = None if fmask is None else N.upload(np.asarray(fmask, dtype=np.uint8), dev)
    V = 1 if kind == "variance" else S
    mwn = None if min_w_node is None else N.upload(np.asarray(min_w_node, dtype=np.float64), dev)
    out = torch.empty(6 * k + k * V, dtype=torch.float64, device=dev)
    N.check(N.kernels().o3s_tree_split(Hc.data_ptr(), k, F, B, S, _KINDS[kind], nb32.data_ptr(), N.ptr(fm),
                                       float(min_inst), float(min_w), float(min_wfrac), N.ptr(mwn), out.data_ptr(),
                                       N.stream_of(Hc)), "tree_split")
    return out


def _impurity(stats: torch.Tensor, kind: str) -> tuple[torch.Tensor, torch.Tensor]:
    """stats [..., S] -> (impurity, weight)."""
    if kind == "variance":
        w = stats[..., 0]
        mean = stats[..., 1] / w.clamp_min(1e-300)
        imp = (stats[..., 2] / w.clamp_min(1e-300) - mean * mean).clamp_min(0.0)
        return torch.where(w > 0, imp, torch.zeros_like(imp)), w
    w = stats.sum(-1)
    p = stats / w.clamp_min(1e-300)[..., None]
    if kind == "gini":
        imp = 1.0 - (p * p).sum(-1)
    elif kind == "entropy":
        imp = -(torch.where(p > 0, p * torch.log2(p.clamp_min(1e-300)), torch.zeros_like(p))).sum(-1)
    else:
        raise ValueError(kind)
    return torch.where(w > 0, imp, torch.zeros_like(imp)), w


def best_splits_torch(H, nb, fm, kind, min_inst, min_w, min_wfrac, min_w_node=None):
    """Reference of ``tree_split_kernel``: the per-node decision bundle (fp64
    [idx | gain | impurity | weight | wL | wR | values]) from histograms [k, F, B, S]."""
    k = H.shape[0]
    dev = H.device
    cls, nb, bin_ids = kind != "variance", nb.to(dev), torch.arange(H.shape[2] - 1, device=dev)
    tot = H[:, 0].sum(1)                                   # [k, S] node stats (feature 0 bins)
    imp_p, w_p = _impurity(tot, kind)
    vals = (tot / w_p.clamp_min(1e-300)[:, None]) if cls else (tot[:, 1] / w_p.clamp_min(1e-300))[:, None]
    # split search: cumulative stats over bins (left = bins <= j)
    cum = H.cumsum(2)                                      # [k, F, B, S]
    left = cum[:, :, :-1]
    right = tot[:, None, None, :] - left
    W = w_p[:, None, None].clamp_min(1e-300)
    if cls:
        iL, wL = _impurity(left, kind)
        iR, wR = _impurity(right, kind)
        g = imp_p[:, None, None] - (wL / W) * iL - (wR / W) * iR
    else:
        # variance gain from (w, w*y) only: (SyL^2/wL + SyR^2/wR - Sy^2/W) / W
        wL, wR = left[..., 0], right[..., 0]
        sL, sR = left[..., 1], right[..., 1]
        sP = tot[:, 1][:, None, None]
        g = (sL * sL / wL.clamp_min(1e-300) + sR * sR / wR.clamp_min(1e-300) - sP * sP / W) / W
    ok = (wL >= min_inst) & (wR >= min_inst)
    if min_w_node is not None:
        mw = torch.as_tensor(np.asarray(min_w_node, dtype=np.float64), device=dev)[:, None, None]
    else:
        mw = (min_wfrac * w_p)[:, None, None] if min_wfrac > 0.0 else torch.full_like(W, min_w)
    ok &= (mw <= 0.0) | ((wL >= mw) & (wR >= mw))
    ok &= bin_ids[None, None, :] < nb[None, :, None]
    if fm is not None:
        ok &= torch.from_numpy(fm).to(dev)[:, :, None]
    g = torch.where(ok, g, torch.full_like(g, -math.inf))
    best = g.reshape(k, -1).max(1)
    # global child weights at the chosen split decide which child the next level scans
    wl_best = wL.reshape(k, -1).gather(1, best.indices[:, None])[:, 0]
    wr_best = wR.reshape(k, -1).gather(1, best.indices[:, None])[:, 0]
    return torch.cat([best.indices.to(torch.float64), best.values, imp_p, w_p, wl_best, wr_best, vals.reshape(-1)])


def partition_torch(bins, order, s_lo, s_hi, s_feat, s_bin, out=None, payload=(), payload_out=()):
    dev = bins.device
    F = bins.shape[1]
    lens = s_hi - s_lo
    total = int(lens.sum())
    sid = torch.repeat_interleave(torch.arange(s_lo.numel(), device=dev), lens)
    first = torch.cumsum(lens, 0) - lens
    pos = s_lo[sid] + (torch.arange(total, device=dev) - first[sid])
    rows = order[pos].long()
    bvals = bins.view(-1)[rows * F + s_feat[sid]]
    go_left = bvals.to(torch.int64) <= s_bin[sid]
    gl = go_left.to(torch.int64)
    cl = torch.cumsum(gl, 0)
    nleft = torch.zeros(s_lo.numel(), dtype=torch.int64, device=dev).index_add_(0, sid, gl)
    new_order = order.clone() if out is None else out
    if total == 0:
        return new_order, nleft
    cl_before = cl[first.clamp_max(total - 1)] - gl[first.clamp_max(total - 1)]
    lrank = cl - cl_before[sid]                            # inclusive rank among lefts
    rel = torch.arange(total, device=dev) - first[sid]
    rrank = rel + 1 - lrank
    newpos = torch.where(go_left, s_lo[sid] + lrank - 1, s_lo[sid] + nleft[sid] + rrank - 1)
    new_order[newpos] = order[pos]
    for a, b in zip(payload, payload_out):
        b[newpos] = a[pos]
    return new_order, nleft


def node_hist(bins: torch.Tensor, order: torch.Tensor, y: torch.Tensor, w: torch.Tensor | None,
              seg_lo: torch.Tensor, seg_hi: torch.Tensor, seg_node: torch.Tensor, n_nodes: int, B: int, S: int,
              cls: bool, chunk: int | None = None, ypos: bool = False) -> torch.Tensor:
    """Histograms [n_nodes, F, B, S] (fp64) of rows order[lo:hi] for each segment -> node.

    ``ypos``: y / w are in position order (y[p] is the label of row order[p], kept so
    by moving them through ``partition(payload=...)``): they stream contiguously.

    Classification: per-bin weighted class counts.  Regression (S = 3): per-bin sums of
    w and w*y; the node's sum of w*y^2 sits in (feature 0, bin 0, stat 2) -- variance
    split gains need only the first two, the node impurity the third.

    Segments are split into work items of <= ``chunk`` rows; the kernel writes one fp32
    slab row per item (exact for integer weights: <= 8192 rows per item) and the slab rows
    of each segment are summed in fp64, in item order, by ``slab_range_sum_kernel``
    (two fixed-shape stages), so the result is bitwise reproducible and bins past 2^24
    weight keep full precision -- which histogram subtraction (sibling = parent - child)
    relies on."""
    F = bins.shape[1]
    dev = bins.device
    chunk = chunk or HIST_CHUNK
    if len(seg_lo) == 0:
        return torch.zeros((n_nodes, F, B, S), dtype=torch.float64, device=dev)
    if not hist_kernel_ok(bins, B, S, cls):
        # reference path (CPU / oversize bins): direct scatter-add per segment
        return hist_torch(bins, order, y, w, _dev(seg_lo, dev), _dev(seg_hi, dev), _dev(seg_node, dev), n_nodes,
                          B, S, cls, ypos=ypos)
    plan = _HistPlan(seg_lo, seg_hi, seg_node, chunk, dev)
    if plan.n_items == 0:
        return torch.zeros((n_nodes, F, B, S), dtype=torch.float64, device=dev)
    C = F * B * S
    slab = torch.empty((plan.n_items, C), dtype=torch.float32, device=dev)
    yf = y.to(torch.float32).contiguous()
    wf = None if w is None else w.to(torch.float32).contiguous()
    st = N.stream_of(bins)
    N.check(N.kernels().o3s_tree_hist(bins.data_ptr(), bins.shape[0], F, B, S, int(cls), order.data_ptr(),
                                      yf.data_ptr(), N.ptr(wf), plan.it_lo.data_ptr(), plan.it_hi.data_ptr(),
                                      plan.n_items, slab.data_ptr(), int(bool(ypos)), st), "tree_hist")
    # ordered fp64 sums: runs of <= 64 item rows, then each segment's runs in order
    runs = torch.empty((plan.n_runs, C), dtype=torch.float64, device=dev)
    _range_sums(slab, C, plan.r_lo, plan.r_cnt, runs, st)
    nseg = plan.nseg
    seg_sum = torch.empty((nseg, C), dtype=torch.float64, device=dev)
    _range_sums(runs, C, plan.s_run0, plan.s_nrun, seg_sum, st)
    if plan.identity and nseg == n_nodes:                 # the engine: segment i is node i
        return seg_sum.view(n_nodes, F, B, S)
    out = torch.zeros((n_nodes, C), dtype=torch.float64, device=dev)
    out.index_add_(0, plan.seg_node, seg_sum)
    return out.view(n_nodes, F, B, S)


def sibling_hists(Hs: torch.Tensor, parent: torch.Tensor, small_right, cls: bool) -> torch.Tensor:
    """Level histograms [2P, F, B, S] from the scanned smaller children Hs [P] and the
    parents [P]: node 2p + small_right[p] is Hs[p], its sibling parent[p] - Hs[p] with
    the rounding residue of fractional weights cleaned (class counts / weights clamped
    at 0, REG w*y zeroed where w <= 0, the node's w*y^2 clamped at 0).

    GPU: ``tree_sibling_kernel`` (one pass); CPU: ``sibling_torch`` + torch indexing."""
    P = Hs.shape[0]
    sr = np.asarray(small_right, dtype=np.uint8)
    H = torch.empty((2 * P,) + tuple(Hs.shape[1:]), dtype=torch.float64, device=Hs.device)
    if Hs.is_cuda and P > 0:
        Hs_c, par = Hs.contiguous(), parent.contiguous()
        srd = N.upload(sr, Hs.device)
        _, F, B, S = Hs.shape
        N.check(N.kernels().o3s_tree_sibling(Hs_c.data_ptr(), par.data_ptr(), srd.data_ptr(), P, F * B, S, int(cls),
                                             H.data_ptr(), N.stream_of(Hs)), "tree_sibling")
        return H
    pick = torch.from_numpy(2 * np.arange(P) + sr.astype(np.int64)).to(Hs.device)
    H[pick] = Hs
    H[pick ^ 1] = sibling_torch(parent, Hs, cls)
    return H


def sibling_torch(parent: torch.Tensor, child: torch.Tensor, cls: bool) -> torch.Tensor:
    """Histogram of the scanned child's sibling, parent - child ([P, F, B, S] fp64).

    Both operands are exact ordered fp64 sums, but with fractional weights the
    difference can still leave rounding residue in bins the sibling does not populate;
    it is cleaned so such a bin reads as empty: weights / class counts are clamped at 0
    and REG bins whose weight is not positive get zero w*y.  The REG node total of w*y^2
    (feature 0, bin 0, stat 2) is only clamped at 0."""
    sib = parent - child
    if cls:
        return sib.clamp_min_(0.0)
    y2 = sib[:, 0, 0, 2].clamp_min(0.0)
    empty = sib[..., 0] <= 0.0
    sib[..., :2] = torch.where(empty[..., None], torch.zeros_like(sib[..., :2]), sib[..., :2])
    sib[:, 0, 0, 2] = y2
    return sib


_RUN = 64      # slab rows per first-stage partial
# rows per histogram work item: with the LDS-DMA row stage 16384 is best on the 500M x 64
# depth-8 config (s/tree 0.1253 / 0.1195 / 0.1169 / 0.1173 at 4096 / 8192 / 16384 / 32768,
# profiles/kernel_experiments_r6.json); O3S_HIST_CHUNK overrides for A/B runs
HIST_CHUNK = int(os.environ.get("O3S_HIST_CHUNK", str(1 << 14)))


class _HistPlan:
    """Work items (<= chunk rows of one segment) and their fixed-order reduction runs,
    planned on the host from the (small) segment bounds and uploaded in ONE copy --
    instead of a dozen tiny device ops and syncs per tree level."""

    def __init__(self, seg_lo, seg_hi, seg_node, chunk: int, dev):
        lo, hi, nd = _host(seg_lo), _host(seg_hi), _host(seg_node)
        seg_of, it_lo, it_hi, first, n_it = _plan_items(lo, hi, chunk)
        self.nseg = len(lo)
        self.n_items = len(seg_of)
        n_run = (n_it + _RUN - 1) // _RUN
        run0 = np.cumsum(n_run) - n_run
        self.n_runs = int(n_run.sum())
        rseg = np.repeat(np.arange(self.nseg), n_run)
        kr = np.arange(self.n_runs) - run0[rseg]
        r_lo = first[rseg] + kr * _RUN
        r_cnt = np.minimum(_RUN, first[rseg] + n_it[rseg] - r_lo)
        parts = [it_lo, it_hi, r_lo, r_cnt, run0, n_run, nd]
        buf = N.upload(np.concatenate(parts).astype(np.int64), dev)
        self.it_lo, self.it_hi, self.r_lo, self.r_cnt, self.s_run0, self.s_nrun, self.seg_node = buf.split(
            [len(p) for p in parts])
        self.identity = bool(np.array_equal(nd, np.arange(self.nseg)))


def hist_torch(bins, order, y, w, seg_lo, seg_hi, seg_node, n_nodes, B, S, cls, ypos=False):
    F = bins.shape[1]
    dev = bins.device
    out = torch.zeros(n_nodes * F * B * S, dtype=torch.float64, device=dev)
    lens = (seg_hi - seg_lo).clamp_min(0)
    if int(lens.sum()) == 0:
        return out.view(n_nodes, F, B, S)
    pos = torch.cat([torch.arange(int(a), int(b), device=dev) for a, b in zip(seg_lo.tolist(), seg_hi.tolist())])
    node = torch.repeat_interleave(seg_node.to(dev), lens)
    rows = order[pos].long()
    bb = bins[rows].long()                                  # [m, F]
    at = pos if ypos else rows
    yy = y[at].to(torch.float64)
    ww = torch.ones_like(yy) if w is None else w[at].to(torch.float64)
    fidx = torch.arange(F, device=dev)[None, :]
    base = ((node[:, None] * F + fidx) * B + bb) * S        # [m, F]
    if cls:
        idx = base + yy.long()[:, None]
        out.index_add_(0, idx.reshape(-1), ww[:, None].expand(-1, F).reshape(-1))
    else:
        for s, v in enumerate((ww, ww * yy)):
            out.index_add_(0, (base + s).reshape(-1), v[:, None].expand(-1, F).reshape(-1))
        # sum of w*y^2 is a node total (the split gain needs only w and w*y per bin),
        # stored in (feature 0, bin 0) like the kernel does; rows are grouped by segment,
        # so per-segment totals come from one prefix sum (no contended atomics)
        cs = torch.cumsum(ww * yy * yy, 0)
        ends = torch.cumsum(lens, 0)
        seg_tot = cs[(ends - 1).clamp_min(0)] - torch.where(ends - lens > 0, cs[(ends - lens - 1).clamp_min(0)],
                                                             torch.zeros_like(ends, dtype=cs.dtype))
        seg_tot = torch.where(lens > 0, seg_tot, torch.zeros_like(seg_tot))
        out.index_add_(0, seg_node.to(dev).long() * F * B * S + 2, seg_tot)
    return out.view(n_nodes, F, B, S)

"""Tree-ensemble scoring op: the packed ensemble, its gfx950 kernel (csrc/tree_predict.hip)
and a PyTorch reference walker over the same packed table."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as N

LEAF_CODE = 0xFFFF                   # feature code of a leaf node
MAX_FEATURES = 65534                 # features are 16-bit, 0xffff is the leaf code
MAX_V = 16                           # widest value row the kernel accumulates in registers
MAX_GROUP_NODES = 65536              # child indices inside a group are 16-bit
SUM, LEAF = "sum", "leaf"

# LDS of one block: the group's node image plus, where the rows are staged, 4 waves x 64 rows
# of the padded row pitch.  80 KB = two blocks (8 waves) per CU; doc/performance.md has the
# A/B.  O3S_TREE_PREDICT_LDS overrides (bytes, <= 160 KB).
PREDICT_LDS_BUDGET = int(os.environ.get("O3S_TREE_PREDICT_LDS", str(80 * 1024)))
PREDICT_BLOCKS_PER_CU = max(1, (160 * 1024) // PREDICT_LDS_BUDGET)   # persistent grid: the blocks a CU's LDS holds
_MIN_STAGED_NODE_BYTES = 8 * 1024    # a stage that leaves the nodes less than this is not taken


class PackError(ValueError):
    """The ensemble cannot be packed (malformed tree, too many features, ...)."""


def fused_enabled() -> bool:
    """O3S_TREE_PREDICT_FUSED=0: the per-tree torch walk instead of the kernel (read per call)."""
    return os.environ.get("O3S_TREE_PREDICT_FUSED", "1") != "0"


def round_down_f32(t) -> np.ndarray:
    """fp64 thresholds -> the largest fp32 <= t.  A finite t above FLT_MAX gives FLT_MAX, one
    below -FLT_MAX gives -inf, +-inf and NaN map to themselves.  Then ``float(x) <= t32``
    equals ``double(x) <= t`` for every fp32 (or bf16) x, NaN included (false both ways)."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t32 = t.astype(np.float32)                       # round to nearest
        above = t32.astype(np.float64) > t               # rounded up (or overflowed to +inf)
        return np.where(above, np.nextafter(t32, np.float32(-np.inf)), t32).astype(np.float32)


@dataclass
class PackedEnsemble:
    """The ensemble as the kernel reads it (layout: csrc/tree_predict.hip).

    ``nodes`` uint32 [N, 2]; ``values`` fp64 [leaves, V] (times the tree weight);
    ``tree_root`` int32 [T]: the root's index inside its group's node image; ``tree_base``
    int32 [T]: value row of the tree's leaf 0; ``groups``: (node_lo, node_hi, tree_lo,
    tree_hi) per launch, in tree order; ``max_depth``: the deepest leaf of any tree."""
    nodes: np.ndarray
    values: np.ndarray
    tree_root: np.ndarray
    tree_base: np.ndarray
    tree_leaves: np.ndarray
    tree_nodes: np.ndarray
    groups: list
    max_depth: int
    num_features: int
    V: int
    budget: int
    _dev: dict = field(default_factory=dict, repr=False, compare=False)

    @property
    def num_trees(self) -> int:
        return len(self.tree_root)

    def max_tree_bytes(self) -> int:
        return 8 * int(self.tree_nodes.max())

    def on(self, device) -> tuple:
        """(nodes, values, tree_root, tree_base) on ``device``, uploaded once."""
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(N.upload_many(device, self.nodes.view(np.int32), self.values, self.tree_root,
                                                 self.tree_base))
        return self._dev[key]

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev"] = {}
        return st


def tree_node_count(tree) -> int:
    """Nodes of ``tree`` reachable from the root (what its packed image holds)."""
    n, stack = 0, [1]
    while stack:
        nid = stack.pop()
        n += 1
        if not tree.is_leaf(nid):
            stack += [2 * nid, 2 * nid + 1]
    return n


def _pack_tree(tree, V: int, weight: float, d: int):
    """One heap-ordered ``Tree`` -> (w0 uint32 [m], w1 uint32 [m], values fp64 [leaves, V],
    depth).  Nodes are laid out breadth first, siblings adjacent (right = left + 1), every
    child after its parent; leaves are numbered in preorder (``Tree.leaf_index_map``)."""
    feature, count, nheap = tree.feature, tree.count, len(tree.feature)
    value = np.asarray(tree.value, dtype=np.float64).reshape(nheap, -1)
    if value.shape[1] < V:
        raise PackError(f"tree values have {value.shape[1]} columns, the ensemble needs {V}")
    if nheap < 2:
        raise PackError("tree without a root")
    # preorder leaf numbers (left subtree first)
    leaf_no, stack = {}, [1]
    while stack:
        nid = stack.pop()
        if tree.is_leaf(nid):
            leaf_no[nid] = len(leaf_no)
        else:
            for ch in (2 * nid, 2 * nid + 1):
                if ch >= nheap or not count[ch] > 0:
                    raise PackError(f"internal node {nid} has no child {ch}")
            stack += [2 * nid + 1, 2 * nid]
    heap, depth_of, left, q = [1], [0], [], 0
    while q < len(heap):                                  # breadth first: children after parents
        nid = heap[q]
        if nid in leaf_no:
            left.append(0)
        else:
            left.append(len(heap))
            heap += [2 * nid, 2 * nid + 1]
            depth_of += [depth_of[q] + 1] * 2
        q += 1
    heap = np.asarray(heap, dtype=np.int64)
    is_leaf = np.asarray([h in leaf_no for h in heap.tolist()])
    feat = np.where(is_leaf, LEAF_CODE, feature[heap]).astype(np.int64)
    if np.any((feat < 0) | ((feat >= d) & ~is_leaf)):
        raise PackError(f"split feature outside [0, {d})")
    thr = round_down_f32(np.asarray(tree.threshold, dtype=np.float64)[heap]).view(np.uint32)
    payload = np.asarray([leaf_no.get(h, 0) for h in heap.tolist()], dtype=np.uint32)
    w0 = np.where(is_leaf, payload, thr).astype(np.uint32)
    left = np.asarray(left, dtype=np.int64)
    vals = np.zeros((len(leaf_no), V))
    vals[payload[is_leaf]] = float(weight) * value[heap[is_leaf], :V]
    return w0, feat, left, vals, max(depth_of)


def pack_ensemble(trees, weights, kind: str, num_classes: int, budget: int | None = None,
                  num_features: int | None = None) -> PackedEnsemble:
    """Heap-ordered ``Tree`` objects -> one compact node table and one leaf-value table, cut in
    tree order into groups of at most ``budget`` bytes of nodes (one kernel launch each).

    GBT and regressors: V = 1, the leaf mean times the tree weight.  DT / RF classifiers:
    V = ``num_classes``, the leaf's class distribution (unweighted: the classifier vote sums
    the distributions as they are).  Raises :class:`PackError` for an ensemble the kernel
    must not see; the caller then keeps the per-tree torch walk."""
    budget = PREDICT_LDS_BUDGET if budget is None else int(budget)
    if not trees:
        raise PackError("empty ensemble")
    classifier = kind != "gbt" and num_classes > 0
    V = int(num_classes) if classifier else 1
    d = int(num_features if num_features is not None else max(t.num_features for t in trees))
    if d < 1:
        d = int(max(int(np.max(t.feature)) for t in trees)) + 1
        d = max(d, 1)
    if d > MAX_FEATURES:
        raise PackError(f"{d} features exceed {MAX_FEATURES}")
    cap = min(budget // 8, MAX_GROUP_NODES)
    w0s, w1s, vals, roots, bases, leaves, groups = [], [], [], [], [], [], []
    g_nodes = g_tree0 = n_nodes = n_leaves = depth = 0
    for ti, (t, w) in enumerate(zip(trees, weights)):
        w0, feat, left, v, dep = _pack_tree(t, V, 1.0 if classifier else float(w), d)
        m = len(w0)
        if m > cap:
            raise PackError(f"tree {ti} has {m} nodes, a group holds {cap}")
        if g_nodes + m > cap:                             # close the group
            groups.append((n_nodes - g_nodes, n_nodes, g_tree0, ti))
            g_nodes, g_tree0 = 0, ti
        roots.append(g_nodes)
        w1s.append((feat | (np.where(feat == LEAF_CODE, 0, left + g_nodes) << 16)).astype(np.uint32))
        w0s.append(w0)
        vals.append(v)
        bases.append(n_leaves)
        leaves.append(len(v))
        g_nodes, n_nodes, n_leaves, depth = g_nodes + m, n_nodes + m, n_leaves + len(v), max(depth, dep)
    groups.append((n_nodes - g_nodes, n_nodes, g_tree0, len(trees)))
    if n_leaves >= 2 ** 31:
        raise PackError("too many leaves")
    p = PackedEnsemble(np.ascontiguousarray(np.stack([np.concatenate(w0s), np.concatenate(w1s)], 1)),
                       np.ascontiguousarray(np.concatenate(vals)), np.asarray(roots, dtype=np.int32),
                       np.asarray(bases, dtype=np.int32), np.asarray(leaves, dtype=np.int32),
                       np.asarray([len(w) for w in w0s], dtype=np.int64), groups, int(depth), d, V, budget)
    validate_packed(p)
    return p


def validate_packed(p: PackedEnsemble) -> None:
    """Host check of the table the kernel will trust: children in range and after their
    parent, features < d, leaf rows inside the value table, every walk at most ``max_depth``
    steps.  Raises :class:`PackError`."""
    w0, w1 = p.nodes[:, 0].astype(np.int64), p.nodes[:, 1].astype(np.int64)
    feat, left = w1 & 0xFFFF, w1 >> 16
    leaf = feat == LEAF_CODE
    if len(p.values) != int(p.tree_leaves.sum()) or p.values.shape[1] != p.V or not 1 <= p.V:
        raise PackError("value table does not match the trees")
    for lo, hi, t0, t1 in p.groups:
        m = hi - lo
        if not 0 < m <= MAX_GROUP_NODES or 8 * m > p.budget:
            raise PackError("group larger than the LDS budget")
        idx = np.arange(m)
        f, l, lf = feat[lo:hi], left[lo:hi], leaf[lo:hi]
        if np.any(~lf & ((l <= idx) | (l + 1 >= m) | (f >= p.num_features))):
            raise PackError("node table: child index or feature out of range")
        # depth of every node, parents before children
        dep = np.zeros(m, dtype=np.int64)
        for i in np.nonzero(~lf)[0]:
            dep[l[i]] = dep[l[i] + 1] = dep[i] + 1
        if dep.max(initial=0) > p.max_depth:
            raise PackError("node table: a walk is longer than max_depth")
        roots = p.tree_root[t0:t1].astype(np.int64)
        ends = np.append(roots[1:], m)
        if roots[0] != 0 or np.any(ends <= roots):
            raise PackError("tree roots out of order")
        for t, a, b in zip(range(t0, t1), roots, ends):
            if np.any(lf[a:b] & (w0[lo + a:lo + b] >= p.tree_leaves[t])):
                raise PackError("leaf index outside its tree")
            if np.any(~lf[a:b] & ((l[a:b] < a) | (l[a:b] + 1 >= b))):
                raise PackError("child outside its tree")


def gate_reason(is_cuda: bool, dtype, col_stride: int, d: int, V: int, max_tree_bytes: int,
                budget: int | None = None) -> str | None:
    """Why these rows / this ensemble do not go to the kernel (None: they do)."""
    budget = PREDICT_LDS_BUDGET if budget is None else budget
    if not fused_enabled():
        return "O3S_TREE_PREDICT_FUSED=0"
    if not is_cuda:
        return "rows are not on a GPU"
    if dtype not in (torch.bfloat16, torch.float32):
        return f"row dtype {dtype}"
    if col_stride != 1:
        return "column stride is not 1"
    if not 1 <= d <= MAX_FEATURES:
        return f"{d} features"
    if not 1 <= V <= MAX_V:
        return f"{V} values per leaf"
    if max_tree_bytes > min(budget, 8 * MAX_GROUP_NODES):
        return "a tree exceeds the LDS budget"
    return None


def predict_kernel_ok(X: torch.Tensor, d: int, V: int, max_tree_bytes: int, budget: int | None = None) -> bool:
    """Kernel or the per-tree torch walk: CUDA rows, bf16 / fp32, unit column stride,
    d <= 65534, V <= 16, every single tree within the LDS budget, switch not off."""
    cs = X.stride(1) if X.dim() == 2 and X.shape[1] > 1 else 1
    return X.dim() == 2 and gate_reason(X.is_cuda, X.dtype, cs, d, V, max_tree_bytes, budget) is None


def _row_layout(X: torch.Tensor, d: int):
    """(ld in elements, stageable): the rows may be staged where the wave's run of rows is
    16-B aligned whole rows that lie inside the tensor's storage."""
    n = X.shape[0]
    ld = int(X.stride(0)) if n > 1 else max(int(X.stride(0)), d)
    if ld < d:
        raise ValueError("rows overlap: row stride below the number of features")
    es = X.element_size()
    inside = (X.storage_offset() + n * ld) * es <= X.untyped_storage().nbytes()
    return ld, bool(inside and (ld * es) % 16 == 0 and X.data_ptr() % 16 == 0)


def node_budget(X: torch.Tensor, d: int, max_tree_bytes: int, budget: int | None = None) -> int:
    """Bytes of nodes per group for these rows: what the row stage leaves of the block's LDS
    where the rows can be staged and that still holds the largest tree (and at least 8 KB),
    else the whole budget (split features then come from global memory)."""
    budget = PREDICT_LDS_BUDGET if budget is None else budget
    if X.is_cuda and X.dim() == 2 and X.dtype in (torch.bfloat16, torch.float32):
        ld, ok = _row_layout(X, d)
        if ok:
            ldb = ld * X.element_size()
            pitch = ldb + 4 if (ldb // 4) % 2 == 0 else ldb
            rest = budget - 4 * 64 * pitch
            if rest >= max(max_tree_bytes, _MIN_STAGED_NODE_BYTES):
                return rest
    return budget


def _check_rows(X: torch.Tensor, d: int) -> None:
    if X.dim() != 2 or X.shape[1] < d:
        raise ValueError(f"rows must be a [n, >= {d}] matrix")
    if X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError("rows must have unit column stride")


def ensemble_walk_torch(packed: PackedEnsemble, X: torch.Tensor, mode: str = SUM) -> torch.Tensor:
    """Reference walk over the packed table on any device: fp64 [n, V] sums (``SUM``: zeros,
    then one add per tree in ensemble order) or fp64 [n, T] preorder leaf indices (``LEAF``).
    Rows are compared in fp64 against the fp32 thresholds: for fp32- or bf16-valued rows that
    is the kernel's fp32 compare and the fp64 compare against the original thresholds."""
    dev, n = X.device, X.shape[0]
    w0 = torch.from_numpy(p_i64(packed.nodes[:, 0])).to(dev)
    thr = torch.from_numpy(packed.nodes[:, 0].copy().view(np.float32).astype(np.float64)).to(dev)
    w1 = torch.from_numpy(p_i64(packed.nodes[:, 1])).to(dev)
    values = torch.from_numpy(packed.values).to(dev)
    out = torch.zeros((n, packed.V if mode == SUM else packed.num_trees), dtype=torch.float64, device=dev)
    Xd = X.to(torch.float64)
    for lo, _, t0, t1 in packed.groups:
        for t in range(t0, t1):
            idx = torch.full((n,), lo + int(packed.tree_root[t]), dtype=torch.int64, device=dev)
            for _ in range(packed.max_depth):
                feat, left = w1[idx] & 0xFFFF, (w1[idx] >> 16) + lo
                leaf = feat == LEAF_CODE
                x = Xd.gather(1, torch.where(leaf, torch.zeros_like(feat), feat)[:, None]).squeeze(1)
                idx = torch.where(leaf, idx, left + (~(x <= thr[idx])).to(torch.int64))   # NaN goes right
            k = w0[idx]
            if mode == SUM:
                out += values[int(packed.tree_base[t]) + k]
            else:
                out[:, t] = k.to(torch.float64)
    return out


def p_i64(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).astype(np.int64)


def ensemble_predict(X: torch.Tensor, d: int, packed: PackedEnsemble, mode: str = SUM) -> torch.Tensor:
    """Score the stored rows ``X`` ([n, >= d], bf16 / fp32, any row stride, unit column
    stride) with the packed ensemble: fp64 [n, V] (``SUM``) or [n, T] (``LEAF``).  GPU: one
    ``tree_predict_kernel`` launch per tree group, accumulating in place; other devices:
    :func:`ensemble_walk_torch`."""
    if mode not in (SUM, LEAF):
        raise ValueError(f"mode {mode!r}")
    _check_rows(X, d)
    if d > packed.num_features and packed.num_features > 0:
        d = packed.num_features
    if d < packed.num_features:
        raise ValueError(f"rows have {d} features, the ensemble splits on {packed.num_features}")
    n, T = X.shape[0], packed.num_trees
    if not X.is_cuda:
        return ensemble_walk_torch(packed, X[:, :d], mode)
    if X.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"rows must be bf16 or fp32, got {X.dtype}")
    dev = X.device
    width = packed.V if mode == SUM else T
    out = torch.zeros((n, width), dtype=torch.float64, device=dev)
    if n == 0:
        return out
    ld, stageable = _row_layout(X, d)
    nodes_d, values_d, root_d, base_d = packed.on(dev)
    lib = N.kernels()
    st = N.stream_of(X)
    grid = int(max(1, min(N.num_cus(dev) * PREDICT_BLOCKS_PER_CU, (n + 255) // 256)))
    budget = max(packed.budget, PREDICT_LDS_BUDGET)
    pitch, lds = C.c_int(0), C.c_int(0)
    for lo, hi, t0, t1 in packed.groups:
        N.check(lib.o3s_tree_predict_layout(ld * X.element_size(), int(stageable), hi - lo, budget, C.byref(pitch),
                                            C.byref(lds)), "tree_predict_layout")
        N.check(lib.o3s_tree_predict(X.data_ptr(), int(X.dtype == torch.bfloat16), n, ld, d, nodes_d[lo:].data_ptr(),
                                     hi - lo, root_d[t0:].data_ptr(), base_d[t0:].data_ptr(), t1 - t0,
                                     packed.max_depth, values_d.data_ptr(), packed.V, int(mode == LEAF),
                                     out.data_ptr(), width, t0 if mode == LEAF else 0, pitch.value, budget, grid, st),
                "tree_predict")
    return out


def staged(X: torch.Tensor, d: int, packed: PackedEnsemble) -> list:
    """Per group: does the kernel stage these rows in LDS (tests, benchmark)."""
    ld, stageable = _row_layout(X, d)
    pitch, lds = C.c_int(0), C.c_int(0)
    out = []
    for lo, hi, _, _ in packed.groups:
        N.check(N.kernels().o3s_tree_predict_layout(ld * X.element_size(), int(stageable), hi - lo,
                                                    max(packed.budget, PREDICT_LDS_BUDGET), C.byref(pitch),
                                                    C.byref(lds)), "tree_predict_layout")
        out.append(pitch.value != 0)
    return out

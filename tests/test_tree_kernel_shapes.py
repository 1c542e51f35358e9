"""Tree kernels (ops/csrc/trees.hip) at every shape their host entry points dispatch on:
the fused GBT leaf pass (staged / unstaged rows, grid stride, argument variants), the
histogram kernel (every feature-group width, LDS images above 64 KB, work items of 1 to
129 rows, exact on integer data) and the split kernel (several features per thread, the
tie rule, constant / masked features, the class-count template boundary) -- each against
its fp64 torch reference."""
import functools

import numpy as np
import pytest
import torch

from orange3_spark_amd.ops import _native as N
from orange3_spark_amd.ops import trees as T


# ----------------------------------------------------------------------------- leaf pass
def _random_tree(F, D, seed=3):
    """Heap-ordered depth-D tree, full except a few early leaves; the root splits on the
    row's last byte (F - 1), node 2 on feature 0, the rest at random."""
    nodes = 1 << (D + 1)
    rng = np.random.default_rng(seed)
    feature = -np.ones(nodes, dtype=np.int64)
    split_bin = np.zeros(nodes, dtype=np.int64)
    for nid in range(1, 1 << D):
        if nid in (5, 12):
            continue
        if nid > 1 and feature[nid // 2] < 0:
            continue
        feature[nid] = F - 1 if nid == 1 else 0 if nid == 2 else rng.integers(0, F)
        split_bin[nid] = rng.integers(0, 31)
    return feature, split_bin, rng.normal(size=(nodes, 1))


def _check_leaf_pass(gpu, n, F, D, loss="logistic", first=False, *, weighted=True, val_weights=False, need_y2=True,
                     with_target=True, misaligned=False):
    """T.gbt_leaf_pass on the GPU (twice) against gbt_leaf_pass_torch on the CPU, with the
    assertions and tolerances of test_trees.test_gpu_gbt_leaf_pass_matches_torch_and_is_deterministic."""
    g = torch.Generator().manual_seed(5)
    bins = torch.randint(0, 32, (n, F), generator=g, dtype=torch.uint8)
    feature, split_bin, value = _random_tree(F, D)
    yy = (torch.randint(0, 2, (n,), generator=g).double() * 2 - 1) if loss == "logistic" else \
        torch.randn(n, generator=g, dtype=torch.float64)
    Fm0 = torch.randn(n, generator=g, dtype=torch.float64) * 0.3
    wt = torch.rand(n, generator=g) if weighted else None
    wd = wv = None
    if val_weights:                                  # fp64 training / validation weights, wv mostly zero
        wd = torch.rand(n, generator=g, dtype=torch.float64) + 0.5
        wv = torch.where(torch.rand(n, generator=g) < 0.1, torch.rand(n, generator=g, dtype=torch.float64) + 0.5,
                         torch.zeros(n, dtype=torch.float64))
    if misaligned:                                   # a contiguous [n, F] view one byte into a larger buffer
        buf = torch.zeros(n * F + 16, dtype=torch.uint8, device=gpu)
        bins_gpu = buf[1:1 + n * F].view(n, F)
        bins_gpu.copy_(bins)
        assert bins_gpu.is_contiguous() and bins_gpu.data_ptr() % 16 != 0
    else:
        bins_gpu = bins.to(gpu)
        assert bins_gpu.data_ptr() % 16 == 0
    out = []
    for dev in ("cpu", gpu, gpu):
        mv = lambda t: None if t is None else t.to(dev)
        Fm = Fm0.clone().to(dev)
        tgt = torch.full((n,), 7.0, dtype=torch.float32, device=dev) if with_target else None
        part, y2 = T.gbt_leaf_pass(bins if dev == "cpu" else bins_gpu, feature, split_bin, value, 0.5, D, loss,
                                   yy.to(dev), Fm, mv(wt), mv(wd), mv(wv), first, tgt, need_y2)
        assert (y2 is not None) == need_y2
        out.append((Fm.cpu(), part.cpu(), None if y2 is None else y2.cpu(), None if tgt is None else tgt.cpu()))
    ref, a, b = out
    torch.testing.assert_close(a[0], ref[0], rtol=0, atol=0)
    torch.testing.assert_close(a[1], ref[1], rtol=1e-12, atol=1e-9)
    if need_y2:
        torch.testing.assert_close(a[2], ref[2], rtol=1e-5, atol=1e-6)
    if with_target:
        torch.testing.assert_close(a[3], ref[3], rtol=1e-6, atol=1e-7)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


# F % 16 == 0, F <= 256, aligned: rows staged in LDS where the stage fits in 64 KB beside
# the tree and the leaf sums -- (192, 9) and (240, 3) are the largest that do; (192, 10),
# (208, 9), (240, 10) and F = 256 do not and run unstaged like F % 16 != 0 and F > 256
@pytest.mark.gpu
@pytest.mark.parametrize("F,D", [(16, 1), (64, 10), (192, 10), (208, 9), (256, 3), (256, 10), (240, 10),
                                 (192, 9), (240, 3), (12, 6), (7, 1), (272, 6)])
def test_gpu_gbt_leaf_pass_widths_and_depths(gpu, F, D):
    _check_leaf_pass(gpu, 4099, F, D, "squared", False)


@pytest.mark.gpu
def test_gpu_gbt_leaf_pass_misaligned_bins(gpu):
    _check_leaf_pass(gpu, 4099, 64, 6, "logistic", False, misaligned=True)


# fewer rows than a wave, and a last chunk of one row (lanes past the rows clamp to the last)
@pytest.mark.gpu
@pytest.mark.parametrize("F", [64, 12])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_gpu_gbt_leaf_pass_tiny_row_counts(gpu, n, F):
    _check_leaf_pass(gpu, n, F, 6, "logistic", False)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [16, 12])
def test_gpu_gbt_leaf_pass_grid_stride(gpu, F, monkeypatch):
    """One block per CU and 3 * 256 rows per block (+ a tail): every wave walks at least
    three 64-row chunks, so the staged kernel rewrites its LDS rows between chunks."""
    monkeypatch.setattr(T, "LEAF_BLOCKS_PER_CU", 1)
    _check_leaf_pass(gpu, 3 * 256 * N.num_cus(gpu) + 37, F, 6, "logistic", False)


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["logistic", "squared", "absolute"])
@pytest.mark.parametrize("variant", ["weights", "no_wt", "no_y2", "no_target"])
def test_gpu_gbt_leaf_pass_argument_variants(gpu, loss, variant):
    kw = {"weights": dict(val_weights=True), "no_wt": dict(weighted=False), "no_y2": dict(need_y2=False),
          "no_target": dict(with_target=False)}[variant]
    _check_leaf_pass(gpu, 4099, 64, 6, loss, variant == "no_wt", **kw)


def test_gbt_leaf_pass_rejects_non_contiguous_bins():
    """The kernel addresses row i at bins + i * F: a column slice or a transposed view is
    refused (on every device) instead of being read with the wrong stride."""
    n, F, D = 40, 8, 2
    feature, split_bin, value = _random_tree(F, D)
    wide = torch.zeros((n, 2 * F), dtype=torch.uint8)
    yy, Fm = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for bad in (wide[:, :F], torch.zeros((F, n), dtype=torch.uint8).t()):
        assert bad.shape == (n, F) and not bad.is_contiguous()
        with pytest.raises(ValueError, match="contiguous"):
            T.gbt_leaf_pass(bad, feature, split_bin, value, 1.0, D, "squared", yy, Fm, None, None, None, True, None,
                            False)
    assert torch.equal(Fm, torch.zeros(n, dtype=torch.float64))          # nothing was applied
    T.gbt_leaf_pass(wide[:, :F].contiguous(), feature, split_bin, value, 1.0, D, "squared", yy, Fm, None, None, None,
                    True, None, False)
    assert bool((Fm != 0).any())


# ----------------------------------------------------------------------------- histogram
_HN = 20_000
_SEG_LENS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)


@functools.lru_cache(maxsize=None)
def _hist_segments():
    """(order, seg_lo, seg_hi, node maps): a random order cut into segments of 0 .. 129
    rows and the remainder; the identity map and one where two segments share a node."""
    g = torch.Generator().manual_seed(11)
    order = torch.randperm(_HN, generator=g).to(torch.int32)
    cuts = np.concatenate([[0], np.cumsum(_SEG_LENS), [_HN]]).astype(np.int64)
    lo, hi = torch.from_numpy(cuts[:-1].copy()), torch.from_numpy(cuts[1:].copy())
    nseg = len(lo)
    shared = torch.tensor([5, 0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 5])       # first and last -> node 5
    assert len(shared) == nseg
    return order, lo, hi, ((torch.arange(nseg), nseg), (shared, nseg - 1))


def _hist_inputs(F, B, S, cls, seed):
    """Integer-valued data: every fp32 partial of an item of <= 8192 rows is an integer
    below 3 * 16 * 8192 < 2^24, so the sums are exact in any order."""
    g = torch.Generator().manual_seed(seed)
    bins = torch.randint(0, B, (_HN, F), generator=g, dtype=torch.uint8)
    bins[0] = B - 1                                                       # the last bin occurs
    if cls:
        y = torch.randint(0, S, (_HN,), generator=g).float()
        y[1] = S - 1                                                      # and the last class
    else:
        y = torch.randint(-4, 5, (_HN,), generator=g).float()
    w = torch.randint(0, 4, (_HN,), generator=g).float()
    w[:2] = 1.0
    return bins, y, w


def _check_hist_exact(gpu, F, B, S, cls, expect_kernel=True):
    order, lo, hi, maps = _hist_segments()
    bins, y, w = _hist_inputs(F, B, S, cls, 1000 * F + B + S)
    ol = order.long()
    bins_g, order_g = bins.to(gpu), order.to(gpu)
    assert T.hist_kernel_ok(bins_g, B, S, cls) == expect_kernel
    for ww in (w, None):
        for nd, n_nodes in maps:
            ref = T.hist_torch(bins, order, y, ww, lo, hi, nd, n_nodes, B, S, cls)
            assert ref[..., B - 1, :].abs().sum() > 0 and (not cls or ref[..., S - 1].sum() > 0)
            for ypos in (False, True):
                yg = (y[ol] if ypos else y).contiguous().to(gpu)
                wg = None if ww is None else (ww[ol] if ypos else ww).contiguous().to(gpu)
                for chunk in (64, 8192):
                    got = T.node_hist(bins_g, order_g, yg, wg, lo, hi, nd, n_nodes, B, S, cls, chunk=chunk, ypos=ypos)
                    assert got.dtype == torch.float64
                    assert torch.equal(got.cpu(), ref), (ypos, chunk, ww is None, n_nodes)


def test_hist_reference_is_integer_valued_on_integer_data():
    """The exact comparison below rests on this: on the integer inputs the fp64 reference
    holds integers only (and the largest is far below 2^24)."""
    order, lo, hi, maps = _hist_segments()
    for F, B, S, cls in ((5, 16, 3, False), (5, 16, 3, True)):
        bins, y, w = _hist_inputs(F, B, S, cls, 1)
        for ww in (w, None):
            for nd, n_nodes in maps:
                ref = T.hist_torch(bins, order, y, ww, lo, hi, nd, n_nodes, B, S, cls)
                assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 3 * 16 * _HN
                # the position-ordered variant is the same histogram
                ol = order.long()
                rp = T.hist_torch(bins, order, y[ol], None if ww is None else ww[ol], lo, hi, nd, n_nodes, B, S, cls,
                                  ypos=True)
                assert torch.equal(ref, rp)


# F -> feature-group width 4, 4, 4, 8, 8, 16, 32, 32, 64: every instantiation, several
# row-slots per wave (F <= 32) and one (F = 33), partial groups
@pytest.mark.gpu
@pytest.mark.parametrize("cls,S", [(False, 3), (True, 3)])
@pytest.mark.parametrize("F", [1, 3, 4, 5, 8, 16, 17, 32, 33])
def test_gpu_hist_exact_on_integer_data(gpu, F, cls, S):
    _check_hist_exact(gpu, F, 16, S, cls)


# LDS images above 64 KB (with and without room for the DMA row stage), two feature groups
# under the DMA stage with a short second group, and a bin count the kernel does not take
@pytest.mark.gpu
@pytest.mark.parametrize("F,B,S,cls,kernel", [(64, 128, 3, False, True), (64, 160, 3, False, True),
                                              (64, 64, 3, True, True), (48, 32, 5, True, True),
                                              (128, 32, 3, False, True), (80, 32, 2, True, True),
                                              (64, 161, 3, False, False)])
def test_gpu_hist_exact_on_integer_data_large_images(gpu, F, B, S, cls, kernel):
    _check_hist_exact(gpu, F, B, S, cls, expect_kernel=kernel)


# ----------------------------------------------------------------------------- split kernel
def _split_hists(k, F, B, S, kind, seed):
    """Node histograms [k, F, B, S] of 40 * B random weighted rows per node, binned
    independently per feature: every feature sees the node's rows, and no two candidate
    splits cut the rows alike (permuted copies of one feature's bins would: a first bin
    against the rest is another copy's rest against its last bin -- a tie up to rounding)."""
    g = torch.Generator().manual_seed(seed)
    m = 40 * B
    bins = torch.randint(0, B, (k, m, F), generator=g)
    w = torch.rand((k, m), generator=g, dtype=torch.float64) * 2 + 0.5
    cell = (torch.arange(k)[:, None, None] * F + torch.arange(F)[None, None, :]) * B + bins     # [k, m, F]
    H = torch.zeros(k * F * B * S, dtype=torch.float64)
    if kind == "variance":
        y = torch.randn((k, m), generator=g, dtype=torch.float64)
        for s, v in enumerate((w, w * y)):
            H.index_add_(0, (cell * S + s).reshape(-1), v[:, :, None].expand(-1, -1, F).reshape(-1))
        H = H.view(k, F, B, S)
        H[:, 0, 0, 2] = (w * y * y).sum(1)
    else:
        c = torch.randint(0, S, (k, m), generator=g)
        H.index_add_(0, (cell * S + c[:, :, None]).reshape(-1), w[:, :, None].expand(-1, -1, F).reshape(-1))
        H = H.view(k, F, B, S)
    return H, g


def _check_split(gpu, H, nb, fmask, kind, mi, mw, mwf):
    """best_splits (GPU) against best_splits_torch with the per-field assertions of
    test_trees.test_gpu_split_kernel_matches_torch; returns (ref, got)."""
    k = H.shape[0]
    ref = T.best_splits_torch(H, nb, fmask, kind, mi, mw, mwf)
    got = T.best_splits(H.to(gpu), nb.to(gpu), fmask, kind, mi, mw, mwf).cpu()
    fin = torch.isfinite(ref[k:2 * k])
    assert torch.equal(fin, torch.isfinite(got[k:2 * k]))
    assert torch.equal(ref[:k][fin], got[:k][fin])
    torch.testing.assert_close(got[k:2 * k][fin], ref[k:2 * k][fin], rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(got[2 * k:4 * k], ref[2 * k:4 * k], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got[4 * k:6 * k][fin.repeat(2)], ref[4 * k:6 * k][fin.repeat(2)])
    torch.testing.assert_close(got[6 * k:], ref[6 * k:], rtol=1e-12, atol=1e-12)
    # a node without a valid split: gain -inf and index 0
    assert bool((got[k:2 * k][~fin] == -np.inf).all()) and bool((got[:k][~fin] == 0).all())
    return ref, got


_SPLIT_ARGS = ((False, 1.0, 0.0, 0.0), (True, 30.0, 0.0, 0.0), (True, 1.0, 0.0, 0.2), (False, 1.0, 90.0, 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,S,k,F,B", [("variance", 3, 5, 300, 16), ("gini", 3, 5, 300, 16),     # features per thread > 1
                                          ("variance", 3, 6, 20, 2), ("gini", 2, 6, 20, 2),          # one threshold
                                          ("variance", 3, 1, 20, 16), ("entropy", 4, 1, 20, 16),     # one node
                                          ("entropy", 8, 7, 20, 16), ("entropy", 9, 7, 20, 16),      # template boundary
                                          ("entropy", 64, 7, 20, 16)])
def test_gpu_split_kernel_shapes(gpu, kind, S, k, F, B):
    H, g = _split_hists(k, F, B, S, kind, 100 * S + F + B)
    if k > 3:
        H[3] = 0.0                                                        # an empty node
    nb = torch.randint(1, B, (F,), generator=g)
    fm = (torch.rand((k, F), generator=g) < 0.5).numpy()
    for masked, mi, mw, mwf in _SPLIT_ARGS:
        _check_split(gpu, H, nb, fm if masked else None, kind, mi, mw, mwf)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,S", [("variance", 3), ("gini", 3), ("entropy", 9)])
def test_gpu_split_kernel_constant_and_masked_features(gpu, kind, S):
    """Features without thresholds (nb == 0; feature 0 still supplies the node total), a node
    whose feature mask is empty and a node whose rows all sit in one bin of every feature."""
    k, F, B = 6, 20, 16
    H, g = _split_hists(k, F, B, S, kind, 7 * S)
    one_bin = 4                                       # node 4: all weight in bin f % B of feature f
    stats = H[one_bin, 0].sum(0)
    H[one_bin] = 0.0
    for f in range(F):
        H[one_bin, f, f % B] = stats
    if kind == "variance":
        H[one_bin, :, :, 2] = 0.0
        H[one_bin, 0, 0, 2] = 1e4
    fm = (torch.rand((k, F), generator=g) < 0.6).numpy()
    fm[2] = False                                     # node 2: no feature allowed
    fm[one_bin] = True
    for zeros in ((0, 5, 7), (2, 4, 19)):
        nb = torch.randint(1, B, (F,), generator=g)
        nb[list(zeros)] = 0
        for fmask in (fm, None):
            ref, got = _check_split(gpu, H, nb, fmask, kind, 1.0, 0.0, 0.0)
            none = [one_bin] + ([2] if fmask is not None else [])
            for node in none:
                assert got[k + node] == -np.inf and got[node] == 0 and ref[k + node] == -np.inf
            assert int(torch.isfinite(got[k:2 * k]).sum()) == k - len(none)
            # no chosen split lies on a feature without thresholds
            fin = torch.isfinite(got[k:2 * k])
            assert not np.isin((got[:k][fin].long() // (B - 1)).numpy(), zeros).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,S", [("variance", 3), ("gini", 3)])
def test_gpu_split_kernel_ties_take_the_lowest_candidate(gpu, kind, S):
    """Duplicate columns tie exactly; the rule is the lowest f * (B - 1) + b.  Each node's best
    column is copied over columns 3, 100 and 259: 3 and 259 belong to one thread (its own
    scan keeps the first), 100 to another (the block reduction's tie branch)."""
    k, F, B = 5, 300, 16
    H, _ = _split_hists(k, F, B, S, kind, 31 + S)
    nb = torch.full((F,), B - 1)
    ref0 = T.best_splits_torch(H, nb, None, kind, 1.0, 0.0, 0.0)
    assert bool(torch.isfinite(ref0[k:2 * k]).all())
    fbest, bbest = ref0[:k].long() // (B - 1), ref0[:k].long() % (B - 1)
    ns = 2 if kind == "variance" else S               # w*y^2 lives in (feature 0, bin 0) only
    for node in range(k):
        for c in (3, 100, 259):
            H[node, c, :, :ns] = H[node, fbest[node], :, :ns]
    ref, got = _check_split(gpu, H, nb, None, kind, 1.0, 0.0, 0.0)
    want = (torch.minimum(fbest, torch.tensor(3)) * (B - 1) + bbest).double()
    assert torch.equal(got[:k], want)
    assert torch.equal(ref[:k], want)

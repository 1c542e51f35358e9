"""The CSR GLM kernels (csrc/sparse.hip: csr_glm_kernel, csc_piece_kernel,
csc_combine_kernel) on hand-built layouts laid on their edges: 8-lane row groups, 32 rows
per block, column pieces of 256 entries, 32 pieces per block of the piece kernel.

Values and coefficients are small integers, the intercept and the weights dyadic fractions,
so every product and partial sum is exact in fp32 (the margin, the residual / loss terms,
the block slab, the piece sums) and in fp64 (the combine): margins, column sums and the
whole hinge / squared loss_grad must equal an fp64 reference computed straight from the raw
CSR arrays bitwise.  The condition is asserted on the reference by an unmarked test."""
import functools

import pytest
import torch

from orange3_spark_amd.ops.sparse import SparseRows

F32_EXACT = 1 << 24
NS = [0, 1, 31, 32, 33, 300]
DS = [1, 256, 257]
ROW_LENS = [0, 1, 7, 8, 9, 17, 0, 2, 16, 3, 24, 5]      # the first rows: around the 8-lane group
COL_COUNTS = [0, 1, 8, 9, 255, 256, 257, 513]           # columns 0..7: around the 256-entry piece
TRAILING_EMPTY = 3
INTERCEPT = -1.5
LOSS_LOGISTIC, LOSS_HINGE, LOSS_SQUARED = 0, 1, 2


def _nfree(d):
    """Distinct other columns the first rows use: 22 or 23, which with the 10 pieces of
    COL_COUNTS makes 32 pieces (one block of the piece kernel) or 33."""
    return 23 if d == 257 else 22


@functools.lru_cache(maxsize=None)
def _layout(n, d):
    """(indptr, idx, val) on the CPU.  Rows 0..11 have ROW_LENS entries, in the last
    _nfree(d) columns (column d - 1 included); the following rows share out COL_COUNTS
    entries of columns 0..7 (a row may hold a column twice: 513 > n); the last three rows
    are empty.  d = 1 puts everything in column 0; n = 1 is one row of 9 entries."""
    g = torch.Generator().manual_seed(17 * n + d)
    rows, cols = [], []
    if n == 1:
        rows, cols = [0] * 9, [(d - 1 - i) % d for i in range(9)]
    elif n > 1:
        k = 0
        for r, ln in enumerate(ROW_LENS):
            for _ in range(ln):
                rows.append(r)
                cols.append(max(0, d - 1 - k % _nfree(d)))
                k += 1
        first, last = len(ROW_LENS), n - TRAILING_EMPTY
        counts = COL_COUNTS if d >= 8 else [2 * (last - first) - 1]
        k = 0
        for c, cnt in enumerate(counts):
            for _ in range(cnt):
                rows.append(first + k % (last - first))
                cols.append(c)
                k += 1
    rows, cols = torch.tensor(rows, dtype=torch.int64), torch.tensor(cols, dtype=torch.int32)
    order = torch.argsort(rows, stable=True)
    indptr = torch.zeros(n + 1, dtype=torch.int64)
    if n:
        indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    val = torch.randint(-2, 3, (rows.numel(),), generator=g).float()
    return indptr, cols[order].contiguous(), val


@functools.lru_cache(maxsize=None)
def _operands(n, d):
    """(coef, y, w): integer coefficients in [-2, 2], 0/1 labels, weights k/4."""
    g = torch.Generator().manual_seed(31 * n + d)
    return (torch.randint(-2, 3, (d,), generator=g).float(), torch.randint(0, 2, (n,), generator=g).float(),
            torch.randint(0, 9, (n,), generator=g).float() / 4)


def _rows(n, d, dev="cpu"):
    indptr, idx, val = _layout(n, d)
    return SparseRows(indptr.to(dev), idx.to(dev), val.to(dev), d)


def _residual(n):
    """Integer residuals in [-2, 2] for colsum(r)."""
    return (torch.arange(n) % 5 - 2).float()


class _Ref:
    """fp64 reference straight from the CSR arrays of _layout (index_add_ over the raw
    entries): it shares nothing with SparseRows, neither its CSC copy nor its loss terms."""

    def __init__(self, n, d):
        self.n, self.d = n, d
        indptr, idx, val = _layout(n, d)
        self.row = torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1])
        self.col, self.val = idx.long(), val.double()

    def margins64(self, coef, intercept):
        m = torch.zeros(self.n, dtype=torch.float64)
        return m.index_add_(0, self.row, self.val * coef.double()[self.col]) + float(intercept)

    def margins(self, coef, intercept):
        return self.margins64(coef, intercept).float()

    def colsum(self, r, square=False):
        v = self.val * self.val if square else self.val
        if r is not None:
            v = v * r.double()[self.row]
        return torch.zeros(self.d, dtype=torch.float64).index_add_(0, self.col, v)

    def loss_terms(self, coef, intercept, loss, y, w):
        m, y = self.margins64(coef, intercept), y.double()
        w = torch.ones_like(y) if w is None else w.double()
        if loss == LOSS_LOGISTIC:
            return (torch.sigmoid(m) - y) * w, w * (torch.log1p(torch.exp(-m.abs())) + m.clamp_min(0) - y * m), w
        if loss == LOSS_HINGE:
            s = 2 * y - 1
            act = (1 - s * m > 0).double()
            return -s * w * act, w * (1 - s * m) * act, w
        return (m - y) * w, 0.5 * w * (m - y) ** 2, w

    def loss_grad(self, coef, intercept, loss, y, w):
        r, l, w = self.loss_terms(coef, intercept, loss, y, w)
        return torch.cat([self.colsum(r), torch.stack([r.sum(), l.sum(), w.sum()])])


def _piece_count(n, d):
    _, idx, _ = _layout(n, d)
    cnt = torch.bincount(idx.long(), minlength=d)
    return int(((cnt + 255) // 256).sum()), cnt


def sparse_abs_bounds(n, d, loss, w):
    """Every fp32 quantity of the margin / loss_grad / colsum kernels with each term
    replaced by its absolute value, in units of its smallest spacing."""
    coef, y, _ = _operands(n, d)
    ref = _Ref(n, d)
    absref = _Ref(n, d)
    absref.val = ref.val.abs()
    wd = torch.ones(n, dtype=torch.float64) if w is None else w.double()
    top = lambda t: t.max() if t.numel() else torch.zeros(())
    out = {"margin /2": 2 * top(absref.margins64(coef.abs(), abs(INTERCEPT))),
           "colsum": top(absref.colsum(None)),
           "colsum r": top(absref.colsum(_residual(n).abs())),
           "colsum sq": top(absref.colsum(None, square=True)),
           "colsum sq w /4": 4 * top(absref.colsum(wd, square=True))}
    if loss is not None:
        r, l, _ = ref.loss_terms(coef, INTERCEPT, loss, y, w)
        out["sum r /8"] = 8 * r.abs().sum()                 # over all rows: bounds every block's partial
        out["sum loss /64"] = 64 * l.abs().sum()
        out["sum w /4"] = 4 * wd.sum()
        out["grad /8"] = 8 * top(absref.colsum(r.abs()))
    return {k: float(v) for k, v in out.items()}


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_sparse_inputs_are_exact_in_fp32(n, d):
    _, _, w = _operands(n, d)
    for loss in (None, LOSS_HINGE, LOSS_SQUARED):
        for ww in (None, w):
            for k, b in sparse_abs_bounds(n, d, loss, ww).items():
                assert b < F32_EXACT, (k, b)
    assert torch.equal(w * 4, (w * 4).round()) and INTERCEPT * 2 == round(INTERCEPT * 2)


def test_sparse_layouts_sit_on_the_kernel_edges():
    lens, counts, pieces = set(), set(), {}
    for n in NS:
        for d in DS:
            indptr, idx, _ = _layout(n, d)
            assert indptr.numel() == n + 1 and int(indptr[-1]) == idx.numel()
            assert idx.numel() == 0 or (0 <= int(idx.min()) and int(idx.max()) == d - 1)
            ln = (indptr[1:] - indptr[:-1])
            lens |= set(ln.tolist())
            if n > 1:
                assert not ln[-TRAILING_EMPTY:].any() and ln[-TRAILING_EMPTY - 1] > 0
            pieces[(n, d)], cnt = _piece_count(n, d)
            counts |= set(cnt.tolist())
    assert {0, 1, 7, 8, 9, 17} <= lens
    assert set(COL_COUNTS) <= counts
    assert 32 in pieces.values() and 33 in pieces.values(), pieces
    assert pieces[(300, 1)] >= 2                            # d = 1: one column over several pieces


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_cpu_sparse_rows_match_the_raw_csr_reference(n, d):
    """The CPU path of SparseRows (its CSC copy included) == sums over the raw CSR entries."""
    coef, y, w = _operands(n, d)
    ref, S = _Ref(n, d), _rows(n, d)
    assert torch.equal(S.margins(coef, INTERCEPT), ref.margins(coef, INTERCEPT))
    for rr, sq in ((None, False), (_residual(n), False), (None, True), (w, True)):
        assert torch.equal(S.colsum(rr, square=sq), ref.colsum(rr, square=sq))
    for loss in (LOSS_HINGE, LOSS_SQUARED):
        assert torch.equal(S.loss_grad(coef, INTERCEPT, loss, y, w), ref.loss_grad(coef, INTERCEPT, loss, y, w))
    # logistic: two fp64 evaluations (sigmoid / softplus written differently), each term
    # within a few ulps (< 1e-14 relative), at most ~1e3 entries of magnitude < 1e2 per sum;
    # torch's softplus returns m beyond its threshold of 20: up to e^-20 = 2.1e-9 per row,
    # times a weight of at most 2
    assert torch.allclose(S.loss_grad(coef, INTERCEPT, LOSS_LOGISTIC, y, w),
                          ref.loss_grad(coef, INTERCEPT, LOSS_LOGISTIC, y, w), rtol=0, atol=1e-9 + 4.2e-9 * n)


def test_cpu_sparse_empty_shard():
    S = _rows(0, 257)
    coef, y, _ = _operands(0, 257)
    assert S.margins(coef, INTERCEPT).shape == (0,)
    assert torch.equal(S.loss_grad(coef, INTERCEPT, LOSS_SQUARED, y, None), torch.zeros(260, dtype=torch.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_gpu_sparse_margins_and_colsums_bitwise(gpu, n, d):
    coef, y, w = _operands(n, d)
    ref, S = _Ref(n, d), _rows(n, d, gpu)
    m = S.margins(coef.to(gpu), INTERCEPT)
    assert m.dtype == torch.float32 and torch.equal(m.cpu(), ref.margins(coef, INTERCEPT))
    r = _residual(n)
    for rr, sq in ((None, False), (r, False), (None, True), (w, True)):
        got = S.colsum(None if rr is None else rr.to(gpu), square=sq)
        assert got.dtype == torch.float64 and got.shape == (d,)
        assert torch.equal(got.cpu(), ref.colsum(rr, square=sq)), (sq, rr is None)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "w"])
@pytest.mark.parametrize("loss", [LOSS_HINGE, LOSS_SQUARED], ids=["hinge", "squared"])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_gpu_sparse_loss_grad_bitwise(gpu, n, d, loss, weighted):
    """[gradient (d) | sum r | loss | weight sum] of the hinge and squared losses."""
    coef, y, w = _operands(n, d)
    w = w if weighted else None
    ref, S = _Ref(n, d), _rows(n, d, gpu)
    want = ref.loss_grad(coef, INTERCEPT, loss, y, w)
    got = S.loss_grad(coef.to(gpu), INTERCEPT, loss, y.to(gpu), None if w is None else w.to(gpu))
    assert got.dtype == torch.float64 and got.shape == (d + 3,)
    assert torch.equal(got.cpu(), want)
    if n == 0:
        assert not got.any()
    assert torch.equal(S.loss_grad(coef.to(gpu), INTERCEPT, loss, y.to(gpu), None if w is None else w.to(gpu)), got)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_gpu_sparse_logistic_close_and_deterministic(gpu, n, d):
    """The logistic loss rounds (expf, log1pf): the project's tolerance for this kernel."""
    coef, y, w = _operands(n, d)
    ref, S = _Ref(n, d), _rows(n, d, gpu)
    for ww in (None, w):
        want = ref.loss_grad(coef, INTERCEPT, LOSS_LOGISTIC, y, ww)
        args = (coef.to(gpu), INTERCEPT, LOSS_LOGISTIC, y.to(gpu), None if ww is None else ww.to(gpu))
        got = S.loss_grad(*args)
        assert torch.allclose(got.cpu(), want, rtol=2e-4, atol=2e-3)
        assert torch.equal(S.loss_grad(*args), got)
        assert torch.equal(got[-1].cpu(), want[-1])         # the weight sum is exact
    if n == 0:
        assert torch.equal(got.cpu(), torch.zeros(d + 3, dtype=torch.float64))

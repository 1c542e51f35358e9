"""bin_sums_kernel (csrc/binsum.hip) vs the fp64 index_add_ reference."""
import pytest
import torch

from orange3_spark_amd.ops import binsum as BS


def test_cpu_bin_sums_layout():
    X = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    b = torch.tensor([1, -1, 1])
    out = BS.bin_sums(X, b, 2)
    assert out.shape == (2, 4)
    assert out[1].tolist() == [6.0, 8.0, 2.0, 1 + 4 + 25 + 36]
    assert out[0].tolist() == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,D,nbins,weighted", [(torch.float32, 64, 16, False), (torch.bfloat16, 130, 5, True),
                                                    (torch.float64, 3, 300, True), (torch.float32, 256, 9, False)])
def test_gpu_bin_sums_matches_index_add(gpu, dtype, D, nbins, weighted):
    g = torch.Generator().manual_seed(D + nbins)
    n = 300_001
    X = (torch.randn((n, D), generator=g)).to(dtype).to(gpu)
    b = torch.randint(-2, nbins + 2, (n,), generator=g).to(gpu)      # out-of-range rows are ignored
    w = (torch.rand(n, generator=g) + 0.5).to(gpu) if weighted else None
    got = BS.bin_sums(X, b, nbins, w)
    ref = BS.bin_sums_torch(X, b, nbins, None if w is None else w.float())
    assert torch.allclose(got, ref, rtol=1e-9, atol=1e-7 * n)
    again = BS.bin_sums(X, b, nbins, w)
    assert torch.equal(got, again)                                   # deterministic


# ------------------------------------------------------------------------------------------
# Exact-arithmetic edge tests.  X holds integers in [-8, 8] (exact in bf16 too) and the
# weights are k/8, so every term and every partial sum of the kernel's fp64 accumulators is
# an exact multiple of 1/8 far below 2^53: the kernel must equal the fp64 index_add_
# reference bitwise, whatever the order its waves and blocks are folded in.  The condition
# is asserted on the inputs by an unmarked test for every parametrisation used below.

F64_EXACT = 1 << 53
BS_DTYPES = [torch.float32, torch.bfloat16, torch.float64]
CPL_DS = [1, 64, 65, 128, 129, 192, 193, 256]        # 1..4 columns per lane: 64 CPL and one past
ROW_NS = [0, 1, 5, 1023]                             # 5: fewer rows than the waves of one block
ROW_DS = [3, 64, 129]
GROUPS = [(62, 32), (254, 8)]                        # (D, bins per launch): D + 2 divides 2048
PAD = 5                                              # row stride = D + PAD
_ID = lambda d: str(d).replace("torch.", "")
CASES = ([(1023, D, 6) for D in CPL_DS + [257]] + [(n, D, 6) for n in ROW_NS for D in ROW_DS]
         + [(1023, D, g + 1) for D, g in GROUPS])


def _bs_case(n, D, nbins):
    """(table [n, D + PAD], bins, w) on the CPU in fp64 / int64 / fp32.  Bins run over
    [-2, nbins + 1] (rows outside [0, nbins) are ignored) and bin 1 has no rows."""
    g = torch.Generator().manual_seed(7 * n + 13 * D + nbins)
    base = torch.randint(-8, 9, (n, D + PAD), generator=g).double()
    b = torch.randint(-2, nbins + 2, (n,), generator=g)
    b[b == 1] = nbins - 1
    w = (torch.randint(0, 17, (n,), generator=g).double() / 8).float()
    return base, b, w


def bs_abs_bound(X, w):
    """Upper bound of any bin's sums with every term replaced by its absolute value, in
    units of 1/8: all rows in one bin."""
    Xa = X.double().abs()
    ww = torch.ones(X.shape[0], dtype=torch.float64) if w is None else w.double().abs()
    return 8.0 * float(max((ww[:, None] * Xa).sum(0).max() if X.shape[0] else 0.0, ww.sum(),
                           (ww * (Xa * Xa).sum(1)).sum()))


@pytest.mark.parametrize("n,D,nbins", CASES)
def test_bin_sums_inputs_are_exact(n, D, nbins):
    base, b, w = _bs_case(n, D, nbins)
    X = base[:, :D]
    assert torch.equal(X.to(torch.bfloat16).double(), X) and torch.equal(w * 8, (w * 8).round())
    assert bs_abs_bound(X, w) < F64_EXACT and bs_abs_bound(X, None) < F64_EXACT
    if n >= 1023:
        assert int(b.min()) < 0 and int(b.max()) >= nbins and not bool((b == 1).any())
        assert all(bool((b == k).any()) for k in range(nbins) if k != 1)


@pytest.mark.parametrize("n", [0, 5])
def test_cpu_bin_sums_row_stride_and_empty_input(n):
    """The reference path: a row stride wider than D, no rows, ignored rows, an empty bin."""
    base, b, w = _bs_case(n, 3, 6)
    out = BS.bin_sums(base[:, :3], b, 6, w)
    assert out.shape == (6, 5) and not out[1].any()
    ok = (b >= 0) & (b < 6)
    assert float(out[:, 3].sum()) == float(w[ok].double().sum())
    assert torch.equal(out[:, :3].sum(0), (base[:, :3] * w.double()[:, None])[ok].sum(0))


def _check_bitwise(gpu, n, D, nbins, dtype, kernel=True):
    base, b, w = _bs_case(n, D, nbins)
    X = base.to(dtype).to(gpu)[:, :D]
    assert X.stride(0) == D + PAD and BS.kernel_ok(X) == kernel
    for ww in (None, w):
        got = BS.bin_sums(X, b.to(gpu), nbins, None if ww is None else ww.to(gpu))
        ref = BS.bin_sums_torch(base[:, :D], b, nbins, ww)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (nbins, D + 2)
        assert torch.equal(got.cpu(), ref)
        assert not got[1].any()                                      # a bin without rows stays zero
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("D", CPL_DS)
@pytest.mark.parametrize("dtype", BS_DTYPES, ids=_ID)
def test_gpu_bin_sums_columns_per_lane_bitwise(gpu, dtype, D):
    """bin_sums_kernel<T, CPL> for every dtype and CPL = 1..4, rows read through a stride
    wider than D (X = base[:, :D] of an [n, D + 5] table)."""
    _check_bitwise(gpu, 1023, D, 6, dtype)


@pytest.mark.gpu
def test_gpu_bin_sums_wider_than_kernel_uses_torch(gpu):
    _check_bitwise(gpu, 1023, 257, 6, torch.float32, kernel=False)


@pytest.mark.gpu
@pytest.mark.parametrize("D", ROW_DS)
@pytest.mark.parametrize("n", ROW_NS)
def test_gpu_bin_sums_row_counts_bitwise(gpu, n, D):
    """No rows (all zeros), one row, fewer rows than waves in a block, an odd count."""
    for dtype in BS_DTYPES:
        got = _check_bitwise(gpu, n, D, 6, dtype)
        if n == 0:
            assert not got.any()


@pytest.mark.gpu
@pytest.mark.parametrize("D,group", GROUPS)
def test_gpu_bin_sums_full_lds_bin_group_bitwise(gpu, D, group):
    """(D + 2) divides 2048: a launch of ``group`` bins fills the 64 KB of LDS exactly
    (4 waves x group x (D + 2) fp64); nbins = group + 1 adds a second launch at bin0 > 0."""
    assert 2048 // (D + 2) == group and 4 * group * (D + 2) * 8 == 64 * 1024
    for dtype in BS_DTYPES:
        _check_bitwise(gpu, 1023, D, group + 1, dtype)

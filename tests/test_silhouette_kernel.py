"""``silhouette_kernel`` (``csrc/silhouette.hip``, ``ops/silhouette.py::silhouette_rows``) against
the fp64 formula on the same stored values.

Cases and data: ``test_silhouette_host.py`` (``CASES``: column offsets +50, an emptied id, a
singleton, a wrong-id row, NaN in the padding columns of the storage); each on bf16 and fp32 rows.

Bar, per row and for the weighted mean: ``|s_kernel - s_fp64| <= 4 E32 + 2^-23`` where ``E32`` is
the max row error of the float32 torch evaluation of the kernel's formula on that case (never
taken from the kernel).  4x is for the MFMA's summation order and the dropped products of
order > 2; ``test_silhouette_host.py::test_yardstick`` shows that the same evaluation without
the shift is more than 100x E32 away.
"""
import ctypes as C

import pytest
import torch

from orange3_spark_amd.ops import _native as N
from orange3_spark_amd.ops import silhouette as SIL
from test_silhouette_host import BF16, CASES, F32, SINGLE, case_id, reference

pytestmark = pytest.mark.gpu

PARAMS = [(c, t) for c in CASES for t in (F32, BF16)]


def _pid(p):
    return case_id(p[0]) + ("-f32" if p[1] is F32 else "-bf16")


def _kernel(ref, d, gpu, grid=None):
    s = SIL.silhouette_rows(ref["S"].to(gpu), d, ref["c"].to(gpu), ref["Y"], ref["N"], ref["Psi"], grid=grid)
    assert s.dtype == torch.float32 and s.shape == (ref["S"].shape[0],)
    return s.cpu()


@pytest.mark.parametrize("param", PARAMS, ids=_pid)
def test_matches_fp64(param, gpu):
    case, dtype = param
    n, d, pad, k = case
    ref = reference(case, dtype)
    s = _kernel(ref, d, gpu)
    assert bool(torch.isfinite(s).all())
    bar = 4 * ref["E32"] + 2.0 ** -23
    err = float((s.double() - ref["s64"]).abs().max())
    w = ref["w"]
    mean, want = float((s.double() * w).sum() / w.sum()), float((ref["s64"] * w).sum() / w.sum())
    print(f"{_pid(param)}: max row error {err:.3e} = {err / ref['E32']:.3f} x E32 ({ref['E32']:.3e}), "
          f"weighted mean {mean:.9f} vs {want:.9f} (error {abs(mean - want):.3e})")
    assert err <= bar
    assert abs(mean - want) <= bar
    # the singleton's row is exactly 0, the row under a wrong id is negative
    assert bool((s[ref["c"] == SINGLE] == 0).all()) and int((ref["c"] == SINGLE).sum()) == 1
    assert float(s[ref["wrong"]]) < 0
    # the same bits for one block and for a grid that fills the device, and for the default
    one = _kernel(ref, d, gpu, grid=1)
    many = _kernel(ref, d, gpu, grid=N.num_cus(gpu) * 4)
    assert torch.equal(one, many) and torch.equal(one, s)


def test_moments_from_the_stored_rows(gpu):
    """``cluster_moments`` on strided bf16 / fp32 storage is the fp64 sum over the stored values."""
    for dtype in (F32, BF16):
        case = CASES[4]
        n, d, pad, k = case
        ref = reference(case, dtype)
        Y, Nn, Psi = SIL.cluster_moments(ref["S"].to(gpu), ref["c"].to(gpu), k, None, d)
        assert Y.dtype == torch.float64 and Y.shape == (k, d)
        assert torch.equal(Nn.cpu(), ref["N"])
        assert torch.allclose(Y.cpu(), ref["Y"], rtol=1e-12, atol=1e-9)
        assert torch.allclose(Psi.cpu(), ref["Psi"], rtol=1e-12, atol=1e-9)


def _entry(X, d, k, gpu):
    """Return code of the C entry point for these rows (nothing is launched when it refuses)."""
    n, ld = X.shape
    z = torch.zeros(32 * 33 * 16 * 16 * 3 * 2, dtype=torch.int32, device=gpu)          # room for any operand
    return N.kernels().o3s_silhouette(X.data_ptr(), int(X.dtype == F32), n, ld, d, k, z.data_ptr(), z.data_ptr(),
                                      z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, N.stream_of(X))


def test_gate(gpu):
    X = torch.zeros((64, 264), dtype=F32, device=gpu)
    ok = torch.zeros((64, 64), dtype=F32, device=gpu)
    assert SIL.kernel_ok(ok, 64, 1024) and SIL.kernel_ok(X, 256, 2) and SIL.kernel_ok(ok.to(BF16), 60, 8)
    ns, kp, tr, me = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    lay = N.kernels().o3s_silhouette_layout
    for rows, d, k, word in [(ok, 64, 1025, "clusters"), (X, 257, 8, "columns"), (ok, 64, 1, "clusters")]:
        reason = SIL.gate_reason(True, rows.dtype, True, rows.shape[1], d, k)
        assert reason is not None and word in reason and not SIL.kernel_ok(rows, d, k)
        assert lay(d, k, C.byref(ns), C.byref(kp), C.byref(me), C.byref(tr)) == -1
        assert _entry(rows, d, k, gpu) == -1
    assert lay(256, 1024, C.byref(ns), C.byref(kp), C.byref(me), C.byref(tr)) == 0
    assert (ns.value, kp.value, tr.value, me.value) == (16, 1024, 32, 32 * 16 * 1536)
    assert SIL.layout(64, 33) == (4, 64, 2 * 4 * 1536, 64)
    # fp64 rows, rows on the host and a stride that is no multiple of 8 have a reason too
    x64 = torch.zeros((64, 64), dtype=torch.float64, device=gpu)
    assert "dtype" in SIL.gate_reason(True, x64.dtype, True, 64, 64, 8) and not SIL.kernel_ok(x64, 64, 8)
    assert not SIL.kernel_ok(ok.cpu(), 64, 8)
    assert not SIL.kernel_ok(torch.zeros((64, 20), dtype=F32, device=gpu), 20, 8)
    with pytest.raises(TypeError):
        SIL.silhouette_rows(x64, 64, torch.zeros(64, dtype=torch.long, device=gpu), torch.zeros(8, 64),
                            torch.ones(8), torch.ones(8))
    torch.cuda.synchronize()

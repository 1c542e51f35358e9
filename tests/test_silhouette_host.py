"""Host side of the fused silhouette pass (``ops/silhouette.py``): the fp64 formula against a
brute-force O(n^2) silhouette, the packing of the kernel's operands, the fp32 yardstick the
kernel tests hold the kernel to, and the evaluator on two gloo ranks.

The kernel cases (``CASES``, shared with ``test_silhouette_kernel.py``): per column
``2 centre + N(0, 1) + 50``, so points are distinct and ``max(a, b) > 0`` on every row; one id is
emptied (several in the last block of the k = 1024 case; none for k = 2, where it would leave a
single cluster and no silhouette), one cluster is a singleton, one row sits next to another
cluster's centre under a wrong id, and the storage has NaN in its padding columns.
"""
import os

import numpy as np
import pytest
import torch

from orange3_spark_amd.ops import silhouette as SIL
from orange3_spark_amd.ops.binsum import bin_sums_torch

F32, BF16 = torch.float32, torch.bfloat16

# (n, d, pad, k)
CASES = [
    (67, 8, 0, 2),             # NS = 1; two full tiles and a 3-row tail at RB = 2
    (33, 20, 4, 31),           # ragged 16-column step; one block not full
    (1000, 64, 0, 32),         # RB = 2 boundary; exactly one full block
    (1000, 72, 0, 33),         # RB = 1; one mean into the second block
    (2000, 128, 8, 65),        # three blocks; padded stride
    (1000, 256, 0, 33),        # widest rows; NS = 16
    (20011, 128, 0, 1024),     # MAX_K; empty ids in the last block
]
SINGLE, OWN, OTHER = 1, 0, 1   # the singleton id; the wrong-id row has id OWN and sits at centre OTHER (2 if k > 2)


def case_id(c):
    return f"n{c[0]}-d{c[1]}-pad{c[2]}-k{c[3]}"


def brute_force(X, c, w):
    """O(n^2) weighted silhouette coefficients of fp64 rows X with ids c: a = the weighted sum of
    squared distances to the own cluster over (N_own - 1), b = the least weighted mean squared
    distance to another non-empty cluster, s = (b - a) / max(a, b), 0 for N_own <= 1."""
    n = X.shape[0]
    D2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(2)
    ids = [int(j) for j in torch.unique(c)]
    Nj = {j: float(w[c == j].sum()) for j in ids}
    s = torch.zeros(n, dtype=torch.float64)
    for i in range(n):
        own = int(c[i])
        if Nj[own] <= 1:
            continue
        tot = {j: float((D2[i, c == j] * w[c == j]).sum()) for j in ids}
        a = tot[own] / (Nj[own] - 1)
        b = min(tot[j] / Nj[j] for j in ids if j != own)
        s[i] = (b - a) / max(a, b)
    return s


def moments(X64, c, k, w=None):
    st = bin_sums_torch(X64, c, k, w)
    d = X64.shape[1]
    return st[:, :d].contiguous(), st[:, d].contiguous(), st[:, d + 1].contiguous()


def _small(kind):
    rng = np.random.default_rng({"plain": 1, "weighted": 2, "gaps": 3}[kind])
    n, d, k = 60, 5, 3
    if kind == "gaps":
        k = 5
    cen = rng.normal(size=(k, d))
    c = rng.integers(0, k, n)
    X = 2 * cen[c] + rng.normal(size=(n, d))
    w = rng.uniform(0.5, 1.5, n) if kind == "weighted" else np.ones(n)
    if kind == "gaps":
        c[c == 2] = 3                                        # an empty id in the middle
        c[c == 1] = 0
        c[7] = 1                                             # a singleton
    return torch.from_numpy(X), torch.from_numpy(c), k, torch.from_numpy(w)


@pytest.mark.parametrize("kind", ["plain", "weighted", "gaps"])
def test_fp64_formula_and_evaluator_match_brute_force(kind):
    import pandas as pd
    from orange3_spark_amd import Session, SessionConf
    from orange3_spark_amd.ml import feature as F
    from orange3_spark_amd.ml.evaluation import ClusteringEvaluator
    X, c, k, w = _small(kind)
    want = brute_force(X, c, w)
    Y, N, Psi = moments(X, c, k, w)
    got = SIL.silhouette_torch(X, c, k, w, Y, N, Psi)
    assert got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12
    if kind == "gaps":
        assert float(N[2]) == 0 and float(N[1]) == 1 and float(got[7]) == 0 and float(want[7]) == 0
    names = [f"f{i}" for i in range(X.shape[1])]
    pdf = pd.DataFrame(X.numpy(), columns=names)
    pdf["prediction"], pdf["wt"] = c.numpy(), w.numpy()
    sc = Session(SessionConf().set("o3s.device", "cpu"))
    df = F.VectorAssembler(inputCols=names, outputCol="features").transform(sc.createDataFrame(pdf))
    ev = ClusteringEvaluator(weightCol="wt") if kind == "weighted" else ClusteringEvaluator()
    assert abs(ev.evaluate(df) - float((want * w).sum() / w.sum())) <= 1e-12


def test_pack():
    rng = np.random.default_rng(5)
    k, d = 37, 20
    Y = torch.from_numpy(rng.normal(size=(k, d)) * 30 + 50)
    N = torch.from_numpy(rng.integers(2, 9, k).astype(np.float64))
    N[3], N[11], N[12] = 0, 1, 0.5
    Y = Y * N[:, None]
    Y[3] = 0
    Psi = (Y * Y).sum(1) / N.clamp_min(1) + N
    shift, Mp, cst, fj = SIL.pack(Y, N, Psi)
    c, mu, const, f = SIL.operands(Y, N, Psi)
    assert shift.dtype == cst.dtype == fj.dtype == F32 and Mp.dtype == BF16
    assert shift.shape == (32,) and Mp.shape == (2, 2, 3, 64, 8) and cst.shape == fj.shape == (64,)
    assert Mp.is_contiguous()
    assert torch.equal(shift[:d].double(), c) and not shift[d:].any()
    # un-splitting and unscrambling gives back mu' [k, d] within the rounding of an fp32 number
    back = SIL.unpack_means(Mp, k, d)
    assert back.shape == (k, d)
    assert bool(((back - mu).abs() <= 2.0 ** -24 * mu.abs()).all())
    # lane (r, h) of fragment (cb, s) holds mean 32 cb + r, dims 16 s + 8 h .. + 8
    for cb, s, r, h in [(0, 0, 0, 0), (0, 1, 5, 0), (1, 0, 4, 1), (0, 0, 31, 1)]:
        j, lo = 32 * cb + r, 16 * s + 8 * h
        want = torch.zeros(8, dtype=torch.float64)
        if j < k and lo < d:
            m = min(8, d - lo)
            want[:m] = mu[j, lo:lo + m].float().double()
        assert torch.equal(Mp[cb, s, :, 32 * h + r].double().sum(0), want)
    # padding means and padding columns are zero
    full = Mp.double().sum(2).reshape(2, 2, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(64, 32)
    assert not full[k:].any() and not full[:, d:].any()
    # const: +inf for empty and padding clusters, the mean of |x - c|^2 elsewhere; f = 0 for N <= 1
    assert bool(torch.isinf(cst[k:]).all()) and bool((cst[k:] > 0).all())
    assert float(cst[3]) == float("inf") and float(cst[12]) < float("inf")
    assert bool(torch.isfinite(cst[:k][N > 0]).all())
    assert float(fj[3]) == 0 and float(fj[11]) == 0 and float(fj[12]) == 0 and not fj[k:].any()
    big = N > 1
    assert torch.equal(fj[:k][big], (N / (N - 1))[big].float())
    assert not mu[3].any()
    assert torch.allclose(const[N > 0], ((Psi - 2 * Y @ c + N * (c @ c)) / N)[N > 0], rtol=1e-14, atol=0)


def test_gate_reasons_without_a_gpu():
    assert SIL.gate_reason(True, F32, True, 64, 64, 8) is None
    assert SIL.gate_reason(True, BF16, True, 24, 20, 1024) is None
    assert "clusters" in SIL.gate_reason(True, F32, True, 64, 64, 1025)
    assert "clusters" in SIL.gate_reason(True, F32, True, 64, 64, 1)
    assert "columns" in SIL.gate_reason(True, F32, True, 264, 257, 8)
    assert "dtype" in SIL.gate_reason(True, torch.float64, True, 64, 64, 8)
    assert SIL.gate_reason(False, F32, True, 64, 64, 8) is not None
    assert SIL.gate_reason(True, F32, True, 20, 20, 8) is not None
    assert not SIL.kernel_ok(torch.zeros(4, 8), 8, 2)
    os.environ.pop("O3S_SILHOUETTE_KERNEL", None)
    assert SIL.enabled()


_CACHE = {}


def problem(case, dtype):
    """(storage [n, d + pad] in ``dtype`` with NaN padding, ids int64 [n], weights fp64 [n],
    wrong-id row) of a kernel case."""
    n, d, pad, k = case
    rng = np.random.default_rng(100 * d + k)
    cen = rng.normal(size=(k, d))
    c = rng.integers(0, k, n)
    other = 2 if k > 2 else OTHER
    empty = [] if k < 4 else [k // 2] + ([1001, 1010, 1023] if k == 1024 else [])
    for e in empty:
        c[c == e] = OWN
    c[c == SINGLE] = OWN
    c[1] = SINGLE
    wrong = 2
    c[wrong] = OWN
    if other != SINGLE:
        c[3] = other                                         # the other cluster is not empty
    X = 2 * cen[c] + rng.normal(size=(n, d)) + 50
    X[wrong] = 2 * cen[other] + 0.1 * rng.normal(size=d) + 50
    S = torch.full((n, d + pad), float("nan"), dtype=dtype)
    S[:, :d] = torch.from_numpy(X).to(dtype)
    return S, torch.from_numpy(c), torch.from_numpy(rng.uniform(0.5, 1.5, n)), wrong


def reference(case, dtype):
    """A kernel case once, left unchanged: dict of the problem, the fp64 moments of the stored
    values, the fp64 coefficients ``s64``, the fp32 yardstick's ``s32`` and ``E32`` = its max row
    error against fp64."""
    key = (case, dtype)
    if key not in _CACHE:
        S, c, w, wrong = problem(case, dtype)
        n, d, pad, k = case
        X64 = S[:, :d].double()
        Y, N, Psi = moments(X64, c, k)
        s64 = SIL.silhouette_torch(X64, c, k, None, Y, N, Psi)
        s32 = SIL.silhouette_formula(S[:, :d].float(), c, Y, N, Psi, torch.float32).double()
        _CACHE[key] = dict(S=S, c=c, w=w, wrong=wrong, Y=Y, N=N, Psi=Psi, s64=s64, s32=s32,
                           E32=float((s32 - s64).abs().max()))
    return _CACHE[key]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_yardstick(case, dtype):
    """The fp32 evaluation of the kernel's formula is a yardstick that a kernel without the
    shift cannot meet: the same evaluation about the origin is more than 100x further from fp64."""
    n, d, pad, k = case
    ref = reference(case, dtype)
    assert bool(torch.isfinite(ref["s64"]).all())
    assert float(ref["N"][SINGLE]) == 1 and bool((ref["s64"][ref["c"] == SINGLE] == 0).all())
    assert float(ref["s64"][ref["wrong"]]) < 0
    if k >= 4:
        assert float(ref["N"][k // 2]) == 0
    # the fp64 evaluation of the kernel's formula is the reference itself
    f64 = SIL.silhouette_formula(ref["S"][:, :d].double(), ref["c"], ref["Y"], ref["N"], ref["Psi"], torch.float64)
    assert float((f64 - ref["s64"]).abs().max()) <= 1e-9
    raw = SIL.silhouette_formula(ref["S"][:, :d].float(), ref["c"], ref["Y"], ref["N"], ref["Psi"], torch.float32,
                                 shift=False).double()
    e_raw = float((raw - ref["s64"]).abs().max())
    print(f"{case_id(case)}: E32 {ref['E32']:.3e}, without the shift {e_raw:.3e} = {e_raw / ref['E32']:.0f} x")
    assert ref["E32"] > 0 and e_raw > 100 * ref["E32"]


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_work(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import pandas as pd
    from orange3_spark_amd import Session, SessionConf
    from orange3_spark_amd.ml import feature as F
    from orange3_spark_amd.ml.evaluation import ClusteringEvaluator
    s = Session(SessionConf().set("o3s.device", "cpu").set("spark.master", "spmd" if world > 1 else "local"))
    rng = np.random.default_rng(11)
    n, d, k = 501, 6, 4
    c = rng.integers(0, k, n)
    X = 2 * rng.normal(size=(k, d))[c] + rng.normal(size=(n, d)) + 50
    names = [f"f{i}" for i in range(d)]
    pdf = pd.DataFrame(X, columns=names)
    pdf["prediction"], pdf["wt"] = c, rng.uniform(0.5, 1.5, n)
    df = F.VectorAssembler(inputCols=names, outputCol="features").transform(s.createDataFrame(pdf))
    res = [ClusteringEvaluator().evaluate(df), ClusteringEvaluator(weightCol="wt").evaluate(df),
           ClusteringEvaluator(distanceMeasure="cosine").evaluate(df), df.count()]
    if rank == 0:
        torch.save(res, os.path.join(out_dir, f"w{world}.pt"))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_give_the_single_process_value(tmp_path):
    import torch.multiprocessing as mp
    _rank_work(0, 1, _free_port(), str(tmp_path))
    port = _free_port()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_work, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    a = torch.load(tmp_path / "w1.pt", weights_only=False)
    b = torch.load(tmp_path / "w2.pt", weights_only=False)
    assert a[3] == b[3] == 501
    for x, y in zip(a[:3], b[:3]):
        assert -1 < x < 1 and abs(x - y) <= 1e-9

"""fp32 feature rows out of the assembler (csrc/assemble.hip, the fp32 output branch of both
kernels) and through VectorAssembler on a session with ``o3s.vector.dtype=float32``: the rows
are bitwise the host ``astype(float32)`` of the inputs, whole padded rows with zero pad
columns, and invalid rows are flagged as on the bf16 path."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from orange3_spark_amd.ops import glm as G

DS = [1, 7, 8, 65, 130]
NS = [1, 255, 257, 1031]


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check(out, bad, nbad, D, want: np.ndarray):
    """``want``: host float32 [n, D] with NaN for null / NaN values."""
    n = want.shape[0]
    ld = G.padded_width(D)
    assert out.dtype == torch.float32 and tuple(out.shape) == (n, ld) and out.is_contiguous()
    got = out.cpu().numpy()
    assert not got[:, D:].any()                                    # pad columns are zero
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got[:, :D]), nan)
    assert np.array_equal(_bits(got[:, :D])[~nan], _bits(want)[~nan])      # bitwise
    rb = nan.any(1)
    assert np.array_equal(bad.cpu().numpy().astype(bool), rb)
    assert int(nbad) == int(rb.sum())


def test_cpu_assemble_rejects_cpu_tensors_and_other_dtypes():
    from orange3_spark_amd.ops import assemble as A
    with pytest.raises(TypeError):
        A.assemble([(torch.zeros(4), None, 1)], 4, "cpu", torch.float32)
    with pytest.raises(TypeError):
        A.assemble_bf16([(torch.zeros(4), None, 1)], 4, "cpu")
    with pytest.raises(TypeError):
        A.assemble([(torch.zeros(4), None, 1)], 4, "cpu", torch.float64)


def test_cpu_session_keeps_fp32_rows_unpadded():
    from orange3_spark_amd import Session, SessionConf
    from orange3_spark_amd.ml.feature import to_vector_column
    s = Session(SessionConf().set("o3s.device", "cpu").set("o3s.vector.dtype", "float32"))
    col = to_vector_column(s, torch.randn(5, 6, dtype=torch.float64))
    assert col.data.dtype == torch.float32 and tuple(col.data.shape) == (5, 6) and col.size == 6
    s64 = Session(SessionConf().set("o3s.device", "cpu"))
    col = to_vector_column(s64, torch.randn(5, 6, dtype=torch.float64))
    assert col.data.dtype == torch.float64 and tuple(col.data.shape) == (5, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("src", ["float64", "float32"])
@pytest.mark.parametrize("D", DS)
def test_gpu_assemble_f32_cols_path(gpu, D, src):
    from orange3_spark_amd.ops import assemble as A
    rng = np.random.default_rng(D)
    for n in NS:
        cols = [(rng.normal(size=n) * 1e3 + np.pi).astype(src) for _ in range(D)]
        cols[D // 2][n // 3] = np.nan
        valid = np.ones(n, dtype=bool)
        valid[::97] = False
        srcs = [(torch.from_numpy(c).to(gpu), torch.from_numpy(valid).to(gpu) if j == D - 1 else None, 1)
                for j, c in enumerate(cols)]
        out, bad, nbad, d = A.assemble(srcs, n, gpu, torch.float32, path="cols")
        want = np.stack([c.astype(np.float32) for c in cols], 1)
        want[~valid, D - 1] = np.nan
        assert d == D
        _check(out, bad, nbad, D, want)
        gen, gbad, gnbad, _ = A.assemble(srcs, n, gpu, torch.float32, path="generic")
        _check(gen, gbad, gnbad, D, want)


def _mixed_sources(n, width, rng):
    """Sources whose widths sum to ``width`` (>= 1): numeric columns of several dtypes, one
    with a null mask, and (from 7 columns up) a strided fp32 vector column."""
    makers = [lambda: (rng.normal(size=n) * 1e3 + np.e).astype(np.float64),
              lambda: rng.integers(-10**9, 10**9, n).astype(np.int64),
              lambda: rng.normal(size=n).astype(np.float32),
              lambda: rng.random(n) > 0.5,
              lambda: rng.integers(-1000, 1000, n).astype(np.int32),
              lambda: rng.integers(0, 255, n).astype(np.uint8)]
    host, want = [], []
    left = width
    if width >= 7:
        w = min(5, width - 2)
        vec = np.zeros((n, w + 3), dtype=np.float32)               # row stride > width
        vec[:, :w] = rng.normal(size=(n, w)) * 7
        host.append((vec, None, w))
        want.append(vec[:, :w])
        left -= w
    for j in range(left):
        a = makers[j % len(makers)]()
        valid = None
        col = a.astype(np.float32)[:, None].copy()
        if j == 0:
            a[n // 2] = np.nan
            col[n // 2] = np.nan
        if j == 1 or left == 1:
            valid = np.ones(n, dtype=bool)
            valid[::53] = False
            col[~valid] = np.nan
        host.append((a, valid, 1))
        want.append(col)
    return host, np.concatenate(want, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_gpu_assemble_f32_generic_path(gpu, D):
    from orange3_spark_amd.ops import assemble as A
    rng = np.random.default_rng(100 + D)
    for n in NS:
        host, want = _mixed_sources(n, D, rng)
        srcs = [(torch.from_numpy(a).to(gpu), None if v is None else torch.from_numpy(v).to(gpu), w)
                for a, v, w in host]
        out, bad, nbad, d = A.assemble(srcs, n, gpu, torch.float32)
        assert d == D
        _check(out, bad, nbad, D, want)


@pytest.fixture(scope="module")
def f32_session():
    from orange3_spark_amd import Session, SessionConf
    return Session(SessionConf().setAppName("asm32").set("o3s.vector.dtype", "float32"),
                   device=torch.device("cuda", 0))


def _frame(session, host, n):
    from orange3_spark_amd.frame import column as C
    from orange3_spark_amd.frame.dataframe import DataFrame
    dev = session.device
    cols = OrderedDict()
    for i, (a, v, w) in enumerate(host):
        t = torch.from_numpy(a).to(dev)
        cols[f"c{i}"] = C.VectorColumn(t, w) if a.ndim == 2 else \
            C.NumericColumn(t, None if v is None else torch.from_numpy(v).to(dev))
    cols["row"] = C.NumericColumn(torch.arange(n, dtype=torch.float64).to(dev))
    return DataFrame(session, cols, n), [f"c{i}" for i in range(len(host))]


@pytest.mark.gpu
@pytest.mark.parametrize("handle", ["keep", "skip", "error"])
@pytest.mark.parametrize("D,n", [(1, 257), (7, 1031), (8, 255), (65, 1), (130, 1031)])
def test_gpu_vector_assembler_f32_session(f32_session, monkeypatch, D, n, handle):
    """VectorAssembler on a float32 session takes the fused kernel (counted) and stores padded
    fp32 rows of logical width D; handleInvalid behaves as on the bf16 path."""
    from orange3_spark_amd.ml.feature import VectorAssembler
    from orange3_spark_amd.ops import assemble as A
    host, want = _mixed_sources(n, D, np.random.default_rng(7 * D + n))
    df, names = _frame(f32_session, host, n)
    calls = []
    real = A.assemble

    def counted(sources, rows, device, dtype=torch.bfloat16, path="auto"):
        calls.append(dtype)
        return real(sources, rows, device, dtype, path)
    monkeypatch.setattr(A, "assemble", counted)
    va = VectorAssembler(inputCols=names, outputCol="f", handleInvalid=handle)
    rb = np.isnan(want).any(1)
    if handle == "error" and rb.any():
        with pytest.raises(ValueError, match="handleInvalid"):
            va.transform(df)
        assert calls == [torch.float32]
        return
    out = va.transform(df)
    assert calls == [torch.float32]                               # the kernel path was taken
    col = out.column_data("f")
    keep = ~rb if handle == "skip" else np.ones(n, dtype=bool)
    w = want[keep]
    assert col.size == D and col.ld == G.padded_width(D) and col.data.dtype == torch.float32
    got = col.data.cpu().numpy()
    assert got.shape == (int(keep.sum()), G.padded_width(D)) and not got[:, D:].any()
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(got[:, :D]), nan)
    assert np.array_equal(_bits(got[:, :D])[~nan], _bits(w)[~nan])
    assert np.array_equal(out.column_data("row").data.cpu().numpy(), np.nonzero(keep)[0].astype(np.float64))
    if len(w):
        vecs = out.select("f").toPandas()["f"]
        assert len(vecs) == len(w) and all(len(v.toArray()) == D for v in vecs[:5])
        assert np.array_equal(np.isnan(vecs.iloc[0].toArray()), nan[0])
        assert np.array_equal(vecs.iloc[0].toArray()[~nan[0]], w[0].astype(np.float64)[~nan[0]])


@pytest.mark.gpu
def test_gpu_vector_assembler_f32_plain_float_columns(f32_session, monkeypatch):
    """createDataFrame -> VectorAssembler over plain float64 columns (the column-window
    kernel) == host astype(float32), D = 6 padded to 8."""
    import pandas as pd

    from orange3_spark_amd.ml.feature import VectorAssembler
    from orange3_spark_amd.ops import assemble as A
    rng = np.random.default_rng(5)
    X = rng.normal(size=(1031, 6)) * 20 + 3
    pdf = pd.DataFrame(X, columns=[f"f{i}" for i in range(6)])
    calls = []
    real = A.assemble

    def counted(sources, rows, device, dtype=torch.bfloat16, path="auto"):
        calls.append((dtype, A._cols_ok(sources)))
        return real(sources, rows, device, dtype, path)
    monkeypatch.setattr(A, "assemble", counted)
    out = VectorAssembler(inputCols=list(pdf.columns), outputCol="features").transform(f32_session.createDataFrame(pdf))
    assert calls == [(torch.float32, True)]
    col = out.column_data("features")
    assert col.size == 6 and col.ld == 8 and col.data.dtype == torch.float32
    got = col.data.cpu().numpy()
    assert np.array_equal(_bits(got[:, :6]), _bits(X.astype(np.float32))) and not got[:, 6:].any()

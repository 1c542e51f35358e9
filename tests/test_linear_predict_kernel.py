"""``linear_predict_kernel`` (``ops/linear_predict.py``, ``csrc/linear_predict.hip``) against
the fp64 oracle on the stored rows.

Shapes: the smallest at which the 32-row tile, the prefetch of the next tile and the padding
can go wrong -- n in {1, 31, 32, 33, 4099} (4099 also with ``grid=1``: one block, 33 tiles per
wave), d in {3, 8, 40, 256} in rows whose stride is the next multiple of 8 (padding 7.0, which
meets zero columns of W), K in {1, 2, 3, 10, 32} and raw-only K = 40 (two column blocks), both
row types, every subset of the outputs, ``log_softmax_raw``.

Data: "scaled" -- per-column scales 0.5 - 20 and offsets up to +-50 (as the GMM kernel test),
W ~ N(0, 1) / (10 sqrt d), b ~ N(0, 1); "counts" -- Poisson counts with theta =
log_softmax(N(0, 1)) and pi, the NaiveBayes case (|raw| up to ~3000).

Accuracy bar for raw and prob (no absolute tolerance; ``tests/test_gmm_kernel.py``): the oracle
is ``linear_predict_torch`` in fp64 on the upcast stored rows, the yardstick the same formula in
float32 torch on the CPU; the kernel's max error must be at most

    4 x max(yardstick's max error, 2^-24 max |oracle|).

Predictions are compared on the rows whose two largest oracle margins differ by more than
2 x the bar of raw; the rows left out may be at most 1 % of a shape's rows.
"""
import numpy as np
import pytest
import torch

from orange3_spark_amd.ops import linear_predict as LP

U = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16
SCALED, COUNTS = "scaled", "counts"

# (n, d, K, row dtype, recipe)
CASES = [
    (1, 3, 1, BF16, SCALED),
    (1, 256, 32, F32, SCALED),
    (31, 8, 2, F32, SCALED),
    (31, 40, 10, BF16, SCALED),
    (32, 40, 3, F32, SCALED),
    (32, 8, 32, BF16, SCALED),
    (33, 3, 2, F32, SCALED),
    (33, 256, 10, BF16, SCALED),
    (33, 256, 10, F32, SCALED),
    (33, 8, 2, F32, COUNTS),
    (67, 96, 10, BF16, SCALED),       # 3, 5 and 6 column blocks of 32: two full tiles and a 3-row tail
    (67, 96, 10, F32, SCALED),
    (67, 160, 3, BF16, SCALED),
    (67, 160, 3, F32, SCALED),
    (67, 192, 32, BF16, SCALED),
    (67, 192, 32, F32, SCALED),
    (4099, 3, 1, F32, SCALED),
    (4099, 8, 2, BF16, SCALED),
    (4099, 40, 3, BF16, SCALED),
    (4099, 40, 3, F32, SCALED),
    (4099, 40, 10, F32, SCALED),
    (4099, 256, 10, BF16, SCALED),
    (4099, 256, 10, F32, SCALED),
    (4099, 256, 32, BF16, SCALED),
    (4099, 256, 32, F32, SCALED),
    (4099, 40, 3, BF16, COUNTS),
    (4099, 40, 3, F32, COUNTS),
    (4099, 256, 10, BF16, COUNTS),
]
GRID_CASES = [c for c in CASES if c[0] == 4099 and c[1:3] in ((256, 10), (40, 3), (8, 2))]


def _id(c):
    return f"n{c[0]}-d{c[1]}-k{c[2]}-{'f32' if c[3] is F32 else 'bf16'}-{c[4]}"


def _problem(case):
    """Stored rows [n, ld] (padding 7.0), fp64 W [K, d], b [K]."""
    n, d, K, dtype, recipe = case
    rng = np.random.default_rng(1000 * d + K + (7 if recipe == COUNTS else 0))
    if recipe == SCALED:
        X = rng.normal(size=(n, d)) * rng.uniform(0.5, 20, d) + rng.uniform(-50, 50, d)
        W, b = rng.normal(size=(K, d)) / (10 * np.sqrt(d)), rng.normal(size=K)
    else:
        X = rng.poisson(3.0, size=(n, d)).astype(np.float64)
        W = torch.log_softmax(torch.from_numpy(rng.normal(size=(K, d))), 1).numpy()
        b = torch.log_softmax(torch.from_numpy(rng.normal(size=K)), 0).numpy()
    ld = (d + 7) // 8 * 8
    S = torch.full((n, ld), 7.0, dtype=dtype)
    S[:, :d] = torch.from_numpy(X).to(dtype)
    return S, W, b


def _formula(X, W, b):
    """(raw, prob, log-softmax raw) in the dtype of the operands."""
    M = X @ W.T + b
    return M, torch.softmax(M, 1), M - torch.logsumexp(M, 1, keepdim=True)


_CACHE = {}


def _reference(case):
    """(rows, packed operands, fp64 oracle, bars) of a case, computed once and left unchanged."""
    if case not in _CACHE:
        S, W, b = _problem(case)
        d = case[1]
        p = LP.pack(W, b)
        r, pr, y = LP.linear_predict_torch(S, d, p, raw=True, prob=True, pred=True)
        ls = LP.linear_predict_torch(S, d, p, raw=True, log_softmax_raw=True)[0]
        oracle = (r, pr, ls)
        yard = _formula(S[:, :d].float(), torch.from_numpy(W).float(), torch.from_numpy(b).float())
        bars = tuple(4 * max(float((q.double() - o).abs().max()), U * float(o.abs().max()))
                     for o, q in zip(oracle, yard))
        _CACHE[case] = (S, p, oracle, y, bars)
    return _CACHE[case]


def _run(case, gpu, **kw):
    S, p = _reference(case)[:2]
    out = LP.linear_predict(S.to(gpu), case[1], p, **kw)
    for t in out:
        assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.shape[0] == case[0])
    return tuple(None if t is None else t.cpu() for t in out)


def _ratio(err, bar):
    return err / bar if bar else (0.0 if err == 0 else float("inf"))


def _check_pred(case, pred, raw_oracle, bar_raw):
    n, K = case[0], case[2]
    if K == 1:
        assert not pred.any()
        return 0.0
    top = raw_oracle.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 2 * bar_raw
    left_out = 1.0 - float(clear.double().mean())
    assert left_out <= 0.01, f"{left_out:.4f} of the rows are near ties"
    assert torch.equal(pred[clear], raw_oracle.argmax(1).double()[clear])
    assert bool(((pred >= 0) & (pred < K) & (pred == pred.round())).all())
    return left_out


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_matches_reference(case, gpu):
    n, d, K = case[:3]
    S, p, (o_raw, o_prob, o_ls), o_pred, (bar_raw, bar_prob, bar_ls) = _reference(case)
    raw, prob, pred = _run(case, gpu, raw=True, prob=True, pred=True)
    ls, prob2, pred2 = _run(case, gpu, raw=True, prob=True, pred=True, log_softmax_raw=True)
    assert raw.shape == prob.shape == ls.shape == (n, K) and pred.shape == (n,)
    for t in (raw, prob, pred, ls):
        assert torch.isfinite(t).all()
    assert torch.equal(prob, prob2) and torch.equal(pred, pred2)
    e_raw, e_prob, e_ls = (float((a - o).abs().max()) for a, o in ((raw, o_raw), (prob, o_prob), (ls, o_ls)))
    rowsum = float((prob.sum(1) - 1).abs().max())
    left_out = _check_pred(case, pred, o_raw, bar_raw)
    print(f"{_id(case)}: error / bar raw {_ratio(e_raw, bar_raw):.3f}, prob {_ratio(e_prob, bar_prob):.3f}, log-softmax raw "
          f"{_ratio(e_ls, bar_ls):.3f}; |row sum - 1| {rowsum / U:.2f} x 2^-24 (K = {K}); pred rows left out "
          f"{100 * left_out:.2f} %")
    assert e_raw <= bar_raw and e_prob <= bar_prob and e_ls <= bar_ls
    assert rowsum <= K * U


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRID_CASES, ids=_id)
def test_any_grid_and_either_store_give_the_same_bits(case, gpu):
    """grid=1: one block whose waves loop over 33 tiles each (prefetch on every step but the
    last); the default grid gives every tile its own wave.  The staged and the direct store
    write the same values."""
    kw = dict(raw=True, prob=True, pred=True)
    base = _run(case, gpu, **kw)
    for other in (_run(case, gpu, grid=1, **kw), _run(case, gpu, grid=3, **kw), _run(case, gpu, direct_store=True, **kw),
                  _run(case, gpu, grid=1, direct_store=True, **kw)):
        assert all(torch.equal(a, b) for a, b in zip(base, other))
    bars = _reference(case)[4]
    o_raw = _reference(case)[2][0]
    assert float((base[0] - o_raw).abs().max()) <= bars[0]
    ls = _run(case, gpu, raw=True, log_softmax_raw=True)[0]
    assert torch.equal(ls, _run(case, gpu, raw=True, log_softmax_raw=True, grid=1)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(4099, 40, 10, BF16, SCALED), (33, 256, 10, F32, SCALED)], ids=_id)
def test_every_output_subset(case, gpu):
    full = _run(case, gpu, raw=True, prob=True, pred=True)
    for mask in range(8):
        want = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
        got = _run(case, gpu, raw=want[0], prob=want[1], pred=want[2])
        for w, g, f in zip(want, got, full):
            assert (g is None) == (not w)
            assert g is None or torch.equal(g, f)
    ls = _run(case, gpu, raw=True, prob=False, pred=False, log_softmax_raw=True)[0]
    assert float((ls - _reference(case)[2][2]).abs().max()) <= _reference(case)[4][2]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,dtype", [(4099, 40, BF16), (33, 256, F32), (4099, 8, F32)])
def test_raw_only_column_blocks(n, d, dtype, gpu):
    """K = 40: two launches, each filling its own column block of the [n, 40] output."""
    case = (n, d, 40, dtype, SCALED)
    S, p, (o_raw, _, _), _, (bar_raw, _, _) = _reference_wide(case)
    raw = LP.linear_predict(S.to(gpu), d, p)[0].cpu()
    assert raw.shape == (n, 40) and torch.isfinite(raw).all()
    err = float((raw - o_raw).abs().max())
    print(f"{_id(case)}: error / bar raw {err / bar_raw:.3f}")
    assert err <= bar_raw
    assert torch.equal(raw, LP.linear_predict(S.to(gpu), d, p, grid=1)[0].cpu())
    for kw in (dict(prob=True), dict(pred=True)):
        with pytest.raises(ValueError):
            LP.linear_predict(S.to(gpu), d, p, **kw)


def _reference_wide(case):
    if case not in _CACHE:
        S, W, b = _problem(case)
        p = LP.pack(W, b)
        o = LP.linear_predict_torch(S, case[1], p)[0]
        y = S[:, :case[1]].float() @ torch.from_numpy(W).float().T + torch.from_numpy(b).float()
        bar = 4 * max(float((y.double() - o).abs().max()), U * float(o.abs().max()))
        _CACHE[case] = (S, p, (o, None, None), None, (bar, None, None))
    return _CACHE[case]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_equal_margins_give_the_lowest_index(dtype, gpu):
    """Identical rows of W have equal margins bit for bit: outputs 3 and 20 sit in the two
    half-waves of a row (the exchange with lane ^ 32), 9 and 11 in one lane."""
    rng = np.random.default_rng(3)
    n, d, K = 200, 40, 32
    X = torch.from_numpy(rng.normal(size=(n, d))).to(dtype)
    W = rng.normal(size=(K, d)) * 0.01
    b = np.zeros(K)
    for lo, hi in ((3, 20), (9, 11)):
        W2, b2 = W.copy(), b.copy()
        W2[hi] = W2[lo]
        b2[lo] = b2[hi] = 100.0                   # the pair is every row's maximum
        raw, _, pred = LP.linear_predict(X.to(gpu), d, LP.pack(W2, b2), raw=True, pred=True)
        assert torch.equal(raw[:, lo], raw[:, hi])
        assert bool((pred == float(lo)).all())


@pytest.mark.gpu
def test_bias_pair_and_rejected_rows(gpu):
    """A bias of hundreds keeps its low float; rows the gate rejects raise instead of falling
    back."""
    d, K = 8, 3
    X = torch.zeros((40, d), dtype=BF16)
    X[:, 0] = 1.0
    W = np.zeros((K, d))
    W[0, 0] = -300.0                              # cancels the high float of b[0] exactly
    b = np.array([300.0 + 2.0 ** -20, -517.123456789, 0.1])
    raw = LP.linear_predict(X.to(gpu), d, LP.pack(W, b))[0].cpu()
    want = np.array([2.0 ** -20, np.float32(b[1]), np.float32(b[2])], dtype=np.float64)
    assert torch.equal(raw, torch.from_numpy(want).expand(40, K))
    assert LP.linear_predict_ok(X.to(gpu), d, K) and not LP.linear_predict_ok(X.to(gpu)[:, :4], 4, K)
    with pytest.raises(ValueError):
        LP.linear_predict(X.to(gpu)[:, :4], 4, LP.pack(np.zeros((K, 4))))
    with pytest.raises(ValueError):
        LP.linear_predict(X.to(gpu).double(), d, LP.pack(np.zeros((K, d))))
    empty = LP.linear_predict(X.to(gpu)[:0], d, LP.pack(np.zeros((K, d))), raw=True, prob=True, pred=True)
    assert [tuple(t.shape) for t in empty] == [(0, K), (0, K), (0,)]

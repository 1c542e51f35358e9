"""Every row layout of the fused GLM kernels (csrc/glm_*.hip), in both element types.

A row of ld = 8 * nch columns is split over LPR lanes with CPL 16-B (bf16) / 32-B (fp32)
chunks each.  The mixed, stats and fp32 passes use the nine "remapped" (LPR, CPL) layouts,
the legacy gradient pass, column moments and margins of bf16 rows the nine "natural" ones;
WIDTHS has one feature count per layout.  Few rows and an 8-block grid: every wave walks
several tiles, the last tile of each role is partial, and some waves get no lineage tile.

Tolerances are those of the tests named in each docstring (test_glm_kernels.py,
test_glm_f32.py): same arithmetic, fewer rows.
"""
import functools

import pytest
import torch

from orange3_spark_amd.ops import glm as G

# d -> 16-B chunks per bf16 row; remapped layout / natural layout
WIDTHS = {20: 3,       # (4,1)   / (4,1)
          40: 5,       # (8,1)   / (8,1)
          100: 13,     # (4,4)   / (16,1)
          256: 32,     # (8,4)   / (32,1)
          300: 38,     # (16,4)  / (64,1)
          600: 75,     # (32,4)  / (64,2)
          1100: 138,   # (64,4)  / (64,4)
          2056: 257,   # (64,8)  / (64,8)
          4104: 513}   # (64,16) / (64,16)
THREE = [40, 300, 1100]       # the layouts the older modules' sampling / fp32 / stats tests miss
SEED, GROW0, GRID = 13, 5_000_000, 8


def _ld(d):
    ld = G.padded_width(d)
    assert ld // 8 == WIDTHS[d]          # a new padding rule must not move a case to another layout
    return ld


def _rows_of(d):
    return (3001, 2003) if d <= 600 else (301, 203)


def _coef(ld, seed=4, scale=0.05):
    return torch.randn(ld, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _bf16_case(d):
    """Host tensors: resident rows, lineage rows (global rows GROW0 + n_res ..) as the kernel
    regenerates them, labels and weights of both, and the lineage ground truth."""
    ld = _ld(d)
    n_res, n_lin = _rows_of(d)
    wt, bt = G.synth_truth(SEED, d, ld)
    Xr, yr = G.synth_glm(n_res, d, SEED + 1, ld=ld)
    Xl, yl = G.synth_glm(n_lin, d, SEED, row0=GROW0 + n_res, ld=ld, wtrue=wt, btrue=bt)
    yall = torch.cat([yr, 1.0 - yl])     # lineage labels come from the label column
    sw = torch.rand(n_res + n_lin, generator=torch.Generator().manual_seed(3)) + 0.5
    return Xr, Xl, yall, sw, wt, bt


@functools.lru_cache(maxsize=None)
def _f32_case(d):
    """Host fp32 rows that bf16 cannot hold (test_glm_f32._rows), labels, weights."""
    ld = _ld(d)
    n = _rows_of(d)[0]
    g = torch.Generator().manual_seed(d + n)
    X = torch.zeros((n, ld), dtype=torch.float32)
    X[:, :d] = torch.randn((n, d), generator=g) * 3 + 10
    y = (torch.rand(n, generator=g) < 0.5).float()
    sw = torch.rand(n, generator=g) + 0.25
    return X, y, sw


@functools.lru_cache(maxsize=None)
def _bf16_grad_ref(d, loss, weighted):
    Xr, Xl, yall, sw, _, _ = _bf16_case(d)
    return G.glm_grad_torch(torch.cat([Xr, Xl]), yall, sw if weighted else None, _coef(_ld(d)).double(), 0.1, loss)


def _assert_mixed(out, ref, ld, dpad):
    """The assertions of test_gpu_grad_mixed_matches_fp64."""
    assert torch.allclose(out[:ld], ref[:ld], rtol=1e-3, atol=0.05), (out[:ld] - ref[:ld]).abs().max()
    assert torch.allclose(out[dpad:], ref[ld:], rtol=1e-3, atol=0.5)


def _assert_stats(out, ref, ld):
    """The assertions of test_gpu_stats_mixed_matches_fp64."""
    dpad, _ = G.layout(ld)
    for k in range(3):
        a, b = out[k * dpad:k * dpad + ld], ref[k * dpad:k * dpad + ld]
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-5 * (1 + b.abs().max().item())), (k, (a - b).abs().max())
    assert torch.allclose(out[3 * dpad:], ref[3 * dpad:], rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("d,loss", [(d, 0) for d in WIDTHS] + [(d, loss) for d in (40, 300) for loss in (1, 2)])
def test_gpu_grad_mixed_every_layout(gpu, d, loss):
    """bf16 resident + lineage pass, checked as test_gpu_grad_mixed_matches_fp64."""
    Xr, _, yall, _, _, _ = _bf16_case(d)
    ld = _ld(d)
    n_res, n_lin = _rows_of(d)
    ws = G.GlmWorkspace(gpu, ld, grid=GRID)
    args = (Xr.to(gpu), yall.to(gpu), None, n_lin, d, SEED, GROW0 + n_res, _coef(ld).to(gpu), 0.1, loss, ws)
    out = G.glm_grad_mixed(*args).clone()
    _assert_mixed(out.cpu(), _bf16_grad_ref(d, loss, False), ld, ws.dpad)
    assert torch.equal(out, G.glm_grad_mixed(*args))        # deterministic slab reduction


@pytest.mark.gpu
@pytest.mark.parametrize("d", THREE)
def test_gpu_grad_mixed_minibatch_every_layout(gpu, d):
    """fraction = 0.3, checked as test_gpu_grad_mixed_minibatch_matches_cpu_mask."""
    Xr, Xl, yall, _, _, _ = _bf16_case(d)
    ld = _ld(d)
    n_res, n_lin = _rows_of(d)
    ws = G.GlmWorkspace(gpu, ld, grid=GRID)
    t_dev = torch.tensor([4], dtype=torch.int64, device=gpu)          # iteration 5
    out = G.glm_grad_mixed(Xr.to(gpu), yall.to(gpu), None, n_lin, d, SEED, GROW0 + n_res, _coef(ld).to(gpu), 0.1,
                           0, ws, res_row0=GROW0, t_dev=t_dev, sample_seed=99, fraction=0.3).clone().cpu()
    keep = G.sample_mask(99, 5, torch.arange(GROW0, GROW0 + n_res + n_lin), 0.3).double()
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, keep, _coef(ld).double(), 0.1, 0)
    dpad = ws.dpad
    assert abs(out[dpad + 2].item() - keep.sum().item()) < 0.5        # identical kept set
    assert torch.allclose(out[:ld], ref[:ld], rtol=1e-3, atol=0.05)
    assert torch.allclose(out[dpad:], ref[ld:], rtol=1e-3, atol=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", THREE)
def test_gpu_grad_mixed_f32_every_layout(gpu, d, weighted):
    """fp32 rows through glm_grad_mixed (no lineage rows), checked as
    test_gpu_grad_mixed_f32_matches_fp64."""
    X, y, sw = _f32_case(d)
    ld = _ld(d)
    sw = sw if weighted else None
    coef = _coef(ld, scale=0.05 if d <= 600 else 0.01)
    ws = G.GlmWorkspace(gpu, ld, grid=GRID)
    args = (X.to(gpu), y.to(gpu), None if sw is None else sw.to(gpu), 0, d, 0, 0, coef.to(gpu), 0.1, 0, ws)
    out = G.glm_grad_mixed(*args).clone()
    _assert_mixed(out.cpu(), G.glm_grad_torch(X, y, sw, coef.double(), 0.1, 0), ld, ws.dpad)
    assert torch.equal(out, G.glm_grad_mixed(*args))


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", THREE)
def test_gpu_stats_mixed_every_layout(gpu, d, weighted):
    """bf16 fused summarizer pass with lineage rows, checked as test_gpu_stats_mixed_matches_fp64."""
    Xr, Xl, yall, sw, _, _ = _bf16_case(d)
    n_res, n_lin = _rows_of(d)
    sw = sw if weighted else None
    args = (Xr.to(gpu), yall.to(gpu), None if sw is None else sw.to(gpu), n_lin, d, SEED, GROW0 + n_res)
    out = G.glm_stats_mixed(*args, grid=GRID)
    assert out is not None
    _assert_stats(out.cpu(), G.glm_stats_torch(torch.cat([Xr, Xl]), yall, sw), _ld(d))
    assert torch.equal(out, G.glm_stats_mixed(*args, grid=GRID))


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", THREE)
def test_gpu_stats_f32_every_layout(gpu, d, weighted):
    """Checked as test_gpu_stats_f32_matches_fp64."""
    X, y, sw = _f32_case(d)
    sw = sw if weighted else None
    args = (X.to(gpu), y.to(gpu), None if sw is None else sw.to(gpu), 0, d, 0, 0)
    out = G.glm_stats_mixed(*args, grid=GRID)
    assert out is not None
    _assert_stats(out.cpu(), G.glm_stats_torch(X, y, sw), _ld(d))
    assert torch.equal(out, G.glm_stats_mixed(*args, grid=GRID))


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("d", THREE)
def test_gpu_colstats_every_layout(gpu, d, f32):
    """Weighted column moments of both element types, the bound of
    test_gpu_colstats_f32_matches_fp64."""
    X, _, sw = _f32_case(d)
    if not f32:
        X = X.bfloat16()                 # same magnitudes as the fp32 rows, so the same bound holds
    out = G.glm_colstats(X.to(gpu), sw.to(gpu)).cpu()
    Xd, w = X.double(), sw.double()
    ref = torch.cat([w @ Xd, w @ (Xd * Xd), w.sum().reshape(1)])
    assert out.shape == ref.shape
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("d", THREE)
def test_gpu_margin_every_layout(gpu, d, f32):
    """Margins of both element types, the bound of test_gpu_margin / test_gpu_margin_f32."""
    X = _f32_case(d)[0] if f32 else _bf16_case(d)[0]
    coef = torch.randn(d, generator=torch.Generator().manual_seed(3)) * (1.0 if d <= 256 else 0.1)
    m = G.glm_margin(X.to(gpu), coef.to(gpu), 0.5)
    assert m.dtype == torch.float32 and m.shape == (X.shape[0],)
    ref = X.double()[:, :d] @ coef.double() + 0.5
    assert torch.allclose(m.double().cpu(), ref, atol=1e-3, rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [40, 1100, 2056, 4104])
def test_gpu_grad_legacy_every_layout(gpu, d):
    """glm_grad over bf16 rows at the natural layouts (8,1), (64,4), (64,8), (64,16), the
    assertions of test_gpu_grad_matches_fp64 (weighted logistic)."""
    Xr, Xl, yall, sw, _, _ = _bf16_case(d)
    ld = _ld(d)
    X = torch.cat([Xr, Xl])
    n = X.shape[0]
    ws = G.GlmWorkspace(gpu, ld, grid=GRID)
    out = G.glm_grad(X.to(gpu), yall.to(gpu), sw.to(gpu), _coef(ld).to(gpu), 0.1, 0, ws).cpu()
    ref = _bf16_grad_ref(d, 0, True)
    dpad = ws.dpad
    scale = ref[:ld].abs().max().item() + 1.0
    assert (out[:ld] - ref[:ld]).abs().max().item() < 2e-4 * scale * (n ** 0.5) / 50
    assert abs(out[dpad] - ref[ld]) < 1e-3 * (abs(ref[ld].item()) + 10)
    assert abs(out[dpad + 1] - ref[ld + 1]) < 1e-4 * abs(ref[ld + 1].item()) + 1e-2
    assert abs(out[dpad + 2] - ref[ld + 2]) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("d", [40, 1100])
def test_gpu_grad_synth_every_layout(gpu, d):
    """Lineage-only legacy pass (labels drawn in-kernel) == the pass over the materialised
    rows, as test_gpu_grad_synth_lineage_equals_materialised."""
    ld = _ld(d)
    n_res, n_lin = _rows_of(d)
    wt, bt = G.synth_truth(SEED, d, ld)
    Xl, yl = G.synth_glm(n_lin, d, SEED, row0=GROW0 + n_res, device=gpu, ld=ld, wtrue=wt, btrue=bt)
    coef = _coef(ld, scale=0.02).to(gpu)
    ws = G.GlmWorkspace(gpu, ld, grid=GRID)
    a = G.glm_grad(Xl, yl, None, coef, 0.1, 0, ws).clone()
    b = G.glm_grad_synth(n_lin, ld, d, SEED, GROW0 + n_res, wt, bt, coef, 0.1, 0, ws).clone()
    # identical rows; labels may flip on ~1e-6 of rows due to sum order -> tiny tolerance
    # (the lineage pass regenerates all dpad columns: the slots past ld are not part of the result)
    assert torch.allclose(a[:ld], b[:ld], rtol=1e-4, atol=1e-2)
    assert torch.allclose(a[ws.dpad:], b[ws.dpad:], rtol=1e-4, atol=1e-2)

"""The persistent GLM pass with its 0/1 labels read from bit planes (csrc/glm_mixed.hip
``o3s_glm_pack_labels``, ``glm_grad_persist_kernel<.., YB = true>``; ``ops.glm.MIX_LABEL_BITS``,
``GlmWorkspace.pack_labels``).

The pack kernel is held to its torch twin word for word.  The gradient kernel is held to the
float-label kernel bit for bit (``torch.equal`` on the whole output): the loss arithmetic is the
same expression on the same values, only where the label comes from differs.  The shapes are
those of tests/test_glm_staged_persistent.py, the smallest that cross item boundaries, forced
onto the path with ``MIX_PERSIST = 2`` and run with one block (four waves take every item), so
the word prefetch crosses item boundaries, starts cold after items without a role, and the
lineage plane starts at a float offset that is no multiple of 16.  The labels are the synthetic
random ones: a wrong bit order, half-word or plane offset changes the result."""
import pytest
import torch

from orange3_spark_amd.ops import _native as N
from orange3_spark_amd.ops import glm as G

pytestmark = pytest.mark.gpu

SEED, D = 13, 256


def _rows(gpu, n_res, n_lin, row0=None):
    row0 = n_res if row0 is None else row0
    wt, bt = G.synth_truth(SEED, D, D)
    Xr, yr = G.synth_glm(n_res, D, SEED + 1, device=gpu, ld=D)
    Xl, yl = G.synth_glm(n_lin, D, SEED, row0=row0, device=gpu, ld=D, wtrue=wt, btrue=bt)
    coef = torch.randn(D, generator=torch.Generator().manual_seed(4)).to(gpu) * 0.05
    return Xr, Xl, torch.cat([yr, 1.0 - yl]), coef


def _words(plane, n):
    """The n // 16 packed words of a plane as int32 values 0 .. 65535, and its padding dwords."""
    w = plane.view(torch.int16)[: n // 16].to(torch.int32) & 0xFFFF
    return w.cpu(), plane[(n // 16 + 1) // 2:].cpu()


# --------------------------------------------------------------------------- pack kernel
@pytest.mark.parametrize("n_res,n_lin", [(16, 16), (4096 + 16, 16), (4097, 2063), (1607, 4096 + 16), (0, 48)])
def test_gpu_pack_matches_the_twin(gpu, n_res, n_lin):
    y = (torch.rand(n_res + n_lin, generator=torch.Generator().manual_seed(n_res)) < 0.5).float().to(gpu)
    ws = G.GlmWorkspace(gpu, D, grid=1)
    assert ws.pack_labels(y, n_res, n_lin)
    for plane, off, n in ((ws.label_bits[0], 0, n_res), (ws.label_bits[1], n_res, n_lin)):
        assert plane.data_ptr() % 4 == 0
        words, pad = _words(plane, n)
        ref, bad = G.pack_labels_torch(y[off:off + n])
        assert not bad
        assert torch.equal(words, ref)
        assert pad.numel() >= 1 and bool((pad[-1:] == 0).all()), "the padding dword was written"
        if (n // 16) % 2 == 1:     # the upper half of the last word's dword stays zero too
            assert int(plane[n // 32].item()) >> 16 == 0


@pytest.mark.parametrize("where", ["resident", "lineage"])
def test_gpu_pack_flags_a_label_that_is_not_0_or_1(gpu, where):
    n_res, n_lin = 1607, 4096 + 16
    y = (torch.rand(n_res + n_lin, generator=torch.Generator().manual_seed(3)) < 0.5).float().to(gpu)
    flag = torch.zeros(1, dtype=torch.int32, device=gpu)
    plane = torch.zeros(n_lin // 32 + 2, dtype=torch.int32, device=gpu)
    N.check(N.kernels().o3s_glm_pack_labels(y.data_ptr() + 4 * n_res, n_lin, plane.data_ptr(), flag.data_ptr(),
                                            N.stream_of(y)), "pack")
    assert int(flag.item()) == 0
    y[5 if where == "resident" else n_res + 4100] = 0.5
    ws = G.GlmWorkspace(gpu, D, grid=1)
    assert not ws.pack_labels(y, n_res, n_lin) and ws.label_bits is None
    # a label outside the whole tiles is not packed and does not count
    y2 = (torch.rand(40, generator=torch.Generator().manual_seed(5)) < 0.5).float().to(gpu)
    y2[39] = 0.5
    assert ws.pack_labels(y2, 40, 0)


# --------------------------------------------------------------------------- gradient kernel
def _on_off(gpu, monkeypatch, tiles, Xr, yall, n_lin, row0, coef, loss, blocks=1, expect_bits=True, **kw):
    """The pass with the planes handed in and with the switch off, same workspace settings."""
    monkeypatch.setattr(G, "MIX_ITEM_TILES", tiles)
    monkeypatch.setattr(G, "MIX_PERSIST", 2)
    monkeypatch.setattr(G, "MIX_PERSIST_BLOCKS", blocks)
    outs = []
    for bits in (1, 0):
        monkeypatch.setattr(G, "MIX_LABEL_BITS", bits)
        ws = G.GlmWorkspace(gpu, D, grid=2)
        packed = ws.pack_labels(yall, Xr.shape[0], n_lin)
        out = G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, row0, coef, 0.1, loss, ws, **kw).clone()
        assert ws.islab is not None, "the pass did not take the persistent kernel"
        assert ws.used_label_bits == (bits == 1 and expect_bits), (bits, packed, ws.used_label_bits)
        if bits:
            # two consecutive runs are bit-equal, the slab NaN-filled in between
            ws.islab.fill_(float("nan"))
            ws.imid.fill_(float("nan"))
            again = G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, row0, coef, 0.1, loss, ws, **kw)
            assert torch.equal(out, again), "two consecutive runs differ"
        outs.append(out)
    return outs


@pytest.mark.parametrize("loss", [0, 1])
@pytest.mark.parametrize("tiles,n_res,n_lin", [
    (4, 1600, 1600),
    (4, 4800, 1600),
    (4, 1600, 4800),
    (4, 64, 6400),         # items that hold no resident tile: a cold start of the word prefetch
    (4, 6400, 64),
    (1000, 336, 336),      # a single item
    (256, 40000, 40000),
])
def test_gpu_label_bits_equal_float_labels(gpu, loss, tiles, n_res, n_lin, monkeypatch):
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    on, off = _on_off(gpu, monkeypatch, tiles, Xr, yall, n_lin, n_res, coef, loss)
    print("max |on - off|", (on - off).abs().max().item())
    assert torch.equal(on, off)


@pytest.mark.parametrize("loss", [0, 1])
@pytest.mark.parametrize("mode", ["all_rows", "minibatch"])
def test_gpu_label_bits_ragged_rows_and_offsets(gpu, loss, mode, monkeypatch):
    """4097 + 2063 rows: the lineage plane starts at float 4097 of the column, the ragged rows
    read the float column, the table does not start at row 0."""
    n_res, n_lin, res_row0 = 4097, 2063, 123
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin, row0=res_row0 + n_res)
    kw = dict(res_row0=res_row0)
    if mode == "minibatch":
        kw.update(t_dev=torch.tensor([4], dtype=torch.int64, device=gpu), sample_seed=99, fraction=0.3)
    on, off = _on_off(gpu, monkeypatch, 4, Xr, yall, n_lin, res_row0 + n_res, coef, loss, **kw)
    assert torch.equal(on, off)


def test_gpu_label_bits_against_fp64(gpu, monkeypatch):
    n_res, n_lin = 4800, 1600
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, 0)
    on, _ = _on_off(gpu, monkeypatch, 4, Xr, yall, n_lin, n_res, coef, 0)
    # the tolerances of tests/test_glm_staged_persistent.py::_check_fp64
    print("max |grad - fp64|", (on[:D] - ref[:D]).abs().max().item(), "tail", (on[D:] - ref[D:]).abs().tolist())
    assert torch.allclose(on[:D], ref[:D], rtol=1e-3, atol=0.05)
    assert torch.allclose(on[D:], ref[D:], rtol=1e-3, atol=0.5)


def test_gpu_label_bits_do_not_depend_on_the_launch(gpu, monkeypatch):
    """Block caps 1, 3 and 0 (uncapped) hand the items to the waves differently: bit-equal."""
    n_res, n_lin = 4800, 1600
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    outs = [_on_off(gpu, monkeypatch, 4, Xr, yall, n_lin, n_res, coef, 0, blocks=b)[0] for b in (1, 3, 0)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# --------------------------------------------------------------------------- eligibility
def test_gpu_a_label_of_one_half_keeps_the_float_path(gpu, monkeypatch):
    n_res, n_lin = 1600, 1600
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    yall[n_res + 37] = 0.5
    on, off = _on_off(gpu, monkeypatch, 4, Xr, yall, n_lin, n_res, coef, 0, expect_bits=False)
    assert torch.equal(on, off)


def test_gpu_squared_loss_keeps_the_float_path(gpu, monkeypatch):
    n_res, n_lin = 1600, 1600
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    # real-valued labels: not packable
    yreal = yall + torch.randn(yall.shape[0], generator=torch.Generator().manual_seed(8)).to(gpu)
    on, off = _on_off(gpu, monkeypatch, 4, Xr, yreal, n_lin, n_res, coef, 2, expect_bits=False)
    assert torch.equal(on, off)
    # 0/1 labels under squared loss: packable, but the pass has no bit-plane kernel
    on, off = _on_off(gpu, monkeypatch, 4, Xr, yall, n_lin, n_res, coef, 2, expect_bits=False)
    assert torch.equal(on, off)


def test_gpu_planes_of_another_column_are_not_used(gpu, monkeypatch):
    n_res, n_lin = 1600, 1600
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    monkeypatch.setattr(G, "MIX_ITEM_TILES", 4)
    monkeypatch.setattr(G, "MIX_PERSIST", 2)
    ws = G.GlmWorkspace(gpu, D, grid=2)
    assert ws.pack_labels(yall, n_res, n_lin)
    other = (1.0 - yall).contiguous()
    out = G.glm_grad_mixed(Xr, other, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws).clone()
    assert not ws.used_label_bits
    monkeypatch.setattr(G, "MIX_LABEL_BITS", 0)
    assert torch.equal(out, G.glm_grad_mixed(Xr, other, None, n_lin, D, SEED, n_res, coef, 0.1, 0,
                                             G.GlmWorkspace(gpu, D, grid=2)))

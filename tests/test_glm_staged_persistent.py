"""The staged GLM pass as one launch of persistent waves that claim row items from a ticket
(csrc/glm_mixed.hip ``glm_grad_persist_kernel``, csrc/glm_items.h; ``ops.glm.MIX_PERSIST`` /
``MIX_ITEM_TILES``).  Every case forces the path (``MIX_PERSIST = 2``) on d = 256 rows and checks
it against fp64 (the tolerances of tests/test_glm_mixed_staged.py), against the sliced launches
(``MIX_PERSIST = 0``: another fp32 summation order, nothing more), against itself (two
consecutive runs are bit-equal: a ticket that was not reset, or a slot reused too early, breaks
that) and across three launches that hand the items to the waves differently (bit-equal: the
result depends on the rows and the item size alone).

The workspace's ``grid`` does not size the persistent launch, so workspaces of grid 1, 2 and 96
alone would run the same launch three times.  What varies the assignment is
``MIX_PERSIST_BLOCKS``: the launch has min(blocks that fit the card, items / 4) blocks, which for
these small tables is one wave per item -- every wave would take one item and find the ticket
exhausted.  Capped to ONE block, four waves take every item of the pass between them, 5 to 25
items per wave: the claim of a next item, the prefetch of its first batch and label across
the boundary (and their cold starts after an item that lacks a role), the hand-over, the flush
with that batch in flight and the zeroed accumulators are all run, in every case but the
single-item one.  Three blocks (12 waves) and the uncapped launch give two more assignments."""
import pytest
import torch

from orange3_spark_amd.ops import glm as G

pytestmark = pytest.mark.gpu

SEED, D = 13, 256
ORDER = dict(rtol=1e-5, atol=1e-3)   # tests/test_glm_mixed_staged.py


def _rows(gpu, n_res, n_lin, row0=None):
    row0 = n_res if row0 is None else row0
    wt, bt = G.synth_truth(SEED, D, D)
    Xr, yr = G.synth_glm(n_res, D, SEED + 1, device=gpu, ld=D)
    Xl, yl = G.synth_glm(n_lin, D, SEED, row0=row0, device=gpu, ld=D, wtrue=wt, btrue=bt)
    coef = torch.randn(D, generator=torch.Generator().manual_seed(4)).to(gpu) * 0.05
    return Xr, Xl, torch.cat([yr, 1.0 - yl]), coef


def _check_fp64(out, ref):
    print("max |grad - fp64|", (out[:D] - ref[:D]).abs().max().item(), "tail", (out[D:] - ref[D:]).abs().tolist())
    assert torch.allclose(out[:D], ref[:D], rtol=1e-3, atol=0.05), (out[:D] - ref[:D]).abs().max()
    assert torch.allclose(out[D:], ref[D:], rtol=1e-3, atol=0.5)


def _checks(gpu, make_run, ref, tiles, monkeypatch, sliced_grid=2):
    """make_run(ws) -> a function that runs the pass on workspace ws and returns a copy of its result."""
    assert G.MIX_FULL_TILES == 1 and G.MIX_STAGED >= 1
    monkeypatch.setattr(G, "MIX_ITEM_TILES", tiles)
    monkeypatch.setattr(G, "MIX_PERSIST", 2)
    outs = []
    for grid, blocks in ((1, 1), (2, 3), (96, 0)):
        monkeypatch.setattr(G, "MIX_PERSIST_BLOCKS", blocks)
        ws = G.GlmWorkspace(gpu, D, grid=grid)
        run = make_run(ws)
        out = run()
        assert ws.islab is not None, "the pass did not take the persistent kernel"
        # every pass writes every slab row it sums, in full: what the first run left must not
        # be what makes the second one equal to it
        ws.islab.fill_(float("nan"))
        ws.imid.fill_(float("nan"))
        assert torch.equal(out, run()), f"two consecutive runs differ (grid {grid}, {blocks} blocks)"
        outs.append(out)
    _check_fp64(outs[0], ref)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), \
        "the result depends on which wave took which item"
    monkeypatch.setattr(G, "MIX_PERSIST", 0)
    ws = G.GlmWorkspace(gpu, D, grid=sliced_grid)
    sliced = make_run(ws)()
    assert ws.islab is None
    print("max |persistent - sliced|", (outs[0] - sliced).abs().max().item())
    assert torch.allclose(outs[0], sliced, **ORDER)
    return outs[0]


@pytest.mark.parametrize("tiles,n_res,n_lin", [
    # (items; with one block, items per wave)
    (4, 1600, 1600),       # 50; 12-13: steady state across item boundaries, 1:1
    (4, 4800, 1600),       # 100; 25: 3:1
    (4, 1600, 4800),       # 100; 25: 1:3
    (4, 64, 6400),         # 101; 25: 97 items with no resident tile, 4 with one -- cold batches
    (4, 6400, 64),         # 101; 25: items with no lineage tile -- cold labels
    (1000, 336, 336),      # 1: fewer items than waves; a wave that claims nothing writes nothing
    (128, 40000, 40000),   # 40; 10: a large item size, 62 or 63 tile pairs per item
    (256, 40000, 40000),   # 20; 5: the default item size
])
def test_gpu_persistent_matches_fp64_sliced_and_itself(gpu, tiles, n_res, n_lin, monkeypatch):
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, 0)
    _checks(gpu, lambda ws: lambda: G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws).clone(),
            ref, tiles, monkeypatch)


def test_gpu_persistent_several_items_per_wave_on_a_full_card(gpu, monkeypatch):
    """15 625 items of four tile pairs: the uncapped launch fills the card (768 blocks on 256
    CUs) and still takes each of its waves through five items on average, claimed in an order
    that differs from run to run.  The sliced launches it is compared with get one block per 16
    tile pairs, so that their fp32 partial sums are as short as in the small cases whose
    tolerance is used."""
    n_res = n_lin = 500_000
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, 0)
    del Xl
    _checks(gpu, lambda ws: lambda: G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws).clone(),
            ref, 4, monkeypatch, sliced_grid=(n_res + n_lin) // 16 // 16)


@pytest.mark.parametrize("mode", ["all_rows", "minibatch"])
def test_gpu_persistent_ragged_rows_and_offsets(gpu, mode, monkeypatch):
    """Ragged rows of both roles (their launch has a slab row of its own) and a table that does
    not start at row 0: a wrong row0 / res_row0 / label offset moves the lineage rows, the
    labels or the sampler's kept set."""
    n_res, n_lin, res_row0 = 4097, 2063, 123
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin, row0=res_row0 + n_res)
    if mode == "all_rows":
        kw, w64 = dict(res_row0=res_row0), None
    else:
        kw = dict(res_row0=res_row0, t_dev=torch.tensor([4], dtype=torch.int64, device=gpu), sample_seed=99,
                  fraction=0.3)
        grows = torch.arange(res_row0, res_row0 + n_res + n_lin)
        w64 = G.sample_mask(99, 5, grows, 0.3).double().to(gpu)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, w64, coef.double(), 0.1, 0)
    out = _checks(gpu, lambda ws: lambda: G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, res_row0 + n_res, coef, 0.1,
                                                           0, ws, **kw).clone(), ref, 4, monkeypatch)
    if mode == "minibatch":
        print("weight sum", out[D + 2].item(), "fp64", w64.sum().item())
        assert abs(out[D + 2].item() - w64.sum().item()) < 0.5           # identical kept set


@pytest.mark.parametrize("loss", [1, 2])
def test_gpu_persistent_other_losses(gpu, loss, monkeypatch):
    n_res, n_lin = 4097, 2063
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    ref = G.glm_grad_torch(torch.cat([Xr, Xl]), yall, None, coef.double(), 0.1, loss)
    _checks(gpu, lambda ws: lambda: G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, loss, ws).clone(),
            ref, 4, monkeypatch)


def test_gpu_persistent_refuses_a_short_slab(gpu, monkeypatch):
    """The entry point returns an error, and launches nothing, when the item slab it is given is
    smaller than the pass needs."""
    from orange3_spark_amd.ops import _native as N
    n_res = n_lin = 1600
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    monkeypatch.setattr(G, "MIX_ITEM_TILES", 4)
    monkeypatch.setattr(G, "MIX_PERSIST", 2)
    ws = G.GlmWorkspace(gpu, D, grid=2)
    monkeypatch.setattr(ws, "item_slab", lambda slab, mid: G.GlmWorkspace.item_slab(ws, slab - 1, mid))
    ws.out.fill_(-7.0)
    with pytest.raises(N.NativeError):
        G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws)
    torch.cuda.synchronize()
    assert bool((ws.out == -7.0).all())


def test_gpu_persistent_falls_back_when_the_slab_does_not_fit(gpu, monkeypatch):
    """A slab that cannot be allocated leaves the workspace on the sliced launches, bit for bit,
    for this and every later pass."""
    n_res = n_lin = 1600
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    monkeypatch.setattr(G, "MIX_ITEM_TILES", 4)
    monkeypatch.setattr(G, "MIX_PERSIST", 2)
    ws = G.GlmWorkspace(gpu, D, grid=2)

    def no_memory(slab, mid):
        raise torch.cuda.OutOfMemoryError("no room for the item slab")
    monkeypatch.setattr(ws, "item_slab", no_memory)
    out = G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws).clone()
    assert ws.persist_failed and ws.islab is None
    assert torch.equal(out, G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws))   # still sliced
    monkeypatch.setattr(G, "MIX_PERSIST", 0)
    assert torch.equal(out, G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0,
                                             G.GlmWorkspace(gpu, D, grid=2)))


def test_gpu_persistent_default_leaves_small_passes_alone(gpu, monkeypatch):
    """MIX_PERSIST = 1 keeps a pass with fewer than 64 items per resident wave on the sliced
    launches: the switch changes no bit of it."""
    n_res, n_lin = 4097, 2063
    Xr, Xl, yall, coef = _rows(gpu, n_res, n_lin)
    ws = G.GlmWorkspace(gpu, D, grid=2)

    def run(persist):
        monkeypatch.setattr(G, "MIX_PERSIST", persist)
        return G.glm_grad_mixed(Xr, yall, None, n_lin, D, SEED, n_res, coef, 0.1, 0, ws).clone()
    assert torch.equal(run(1), run(0))
    assert ws.islab is None

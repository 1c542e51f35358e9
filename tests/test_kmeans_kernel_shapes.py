"""K-means kernels (ops/csrc/kmeans_assign.hip, kmeans_update.hip) at every shape their host entry points dispatch on,
each against an fp64 torch reference.  The test that owns each variant:

  kmeans_assign_kernel<KS,1,true>   KS 2..10       test_gpu_split_assign_every_width
  kmeans_assign_kernel<KS,1,false>  KS 2, 8        test_gpu_split_assign_centre_norms_outside_lds
                                    KS 8, 10       test_gpu_assign_beyond_the_screen_lds_limit
  kmeans_assign_kernel, rowlist                    test_gpu_guard_words_and_rowlist (and every screen re-solve)
  kmeans_screen_kernel<KS,TT,false,PS,NOD>         test_gpu_plain_screen_every_variant
      KS 2..8 x TT 1, 2 x PS x NOD; KS 10 x TT 1 x NOD (no presplit above D = 128)
  kmeans_screen_kernel<KS,1,true>   KS 2..10       test_gpu_pair_screen_every_width
  kmeans_screen_kernel, rowlist + bnd              test_gpu_hamerly_bounds_are_certificates,
                                                   test_gpu_guard_words_and_rowlist
  kmeans_presplit_kernel<32|64|96|128>             test_gpu_plain_screen_every_variant (PRESPLIT on)
  kmeans_bounds_kernel                             test_gpu_bounds_recheck_small_sizes
  kmeans_update_kernel, R 8192..256                test_gpu_update_every_chunk_size
  kmeans_update_kernel, peeling / bitonic          test_gpu_update_key_count_boundary
  kmeans_update_kernel<1,8> <1,16> <2,32> <4,64>
                       <1,0> <2,0> <3,0> <4,0>     test_gpu_update_every_lane_layout
  screen LDS limit (o3s_kmeans_screen_lds)         test_screen_lds_query, test_gpu_assign_beyond_the_screen_lds_limit,
                                                   test_gpu_fit_without_the_screen
  16-byte base gate (kernel_ok)                    test_gpu_misaligned_base_takes_the_torch_path

Row count 1031 unless a test is about the count: more than one 256-row block of either
kernel, with a 7-row ragged tile."""
import ctypes as Ct
import functools

import pytest
import torch

from orange3_spark_amd.ops import _native as N
from orange3_spark_amd.ops import kmeans as K

N_ROWS = 1031
WIDTHS = [32, 36, 64, 68, 96, 100, 128, 132, 160]     # every padded D, full and with a padded tail
KINDS = ["blobs", "uniform"]
MAX_UNDECIDED = {"blobs": 0.0, "uniform": 0.05}


# ------------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def _data(kind, n, D, Kc):
    """(X [n, D], C [Kc, D]) on the CPU: the two generators of
    test_kmeans.test_gpu_screen_assign_matches_split_and_fp64."""
    g = torch.Generator(device="cpu").manual_seed(D * 7 + Kc)
    if kind == "blobs":
        C = torch.rand(Kc, D, generator=g) * 20 - 10
        X = C[torch.randint(0, Kc, (n,), generator=g)] + torch.randn(n, D, generator=g)
        C = C + 0.3 * torch.randn(Kc, D, generator=g)
    else:
        X = torch.rand(n, D, generator=g)
        C = torch.rand(Kc, D, generator=g)
    return X, C


def _sqdist(X, C):
    """fp64 squared distances [n, K] by differences (no ||x||^2 + ||c||^2 - 2 x.c cancellation)."""
    return torch.cdist(X.double(), C.double(), compute_mode="donot_use_mm_for_euclid_dist") ** 2


def _reference(X, C):
    """fp64: (d [n, K], min, argmin with the lowest index on exact ties, runner-up gap, tau)."""
    d = _sqdist(X, C)
    mn = d.min(1).values
    am = (d == mn[:, None]).to(torch.int8).argmax(1)             # the first of equal minima
    rest = d.clone()
    rest[torch.arange(d.shape[0], device=d.device), am] = float("inf")
    gap = rest.min(1).values - mn                                # inf with one centre
    cmax = C.double().norm(dim=1).max()
    tau = 2.0 ** -12 * X.double().norm(dim=1) * cmax + 2.0 ** -20 * cmax * cmax
    return d, mn, am, gap, tau


def _oracle(X, C, a, mind=None, kind=None, keep=None):
    """Judge an assignment of EVERY row of X (or of the rows ``keep``) against fp64.

    tau(x) = 2^-12 ||x|| max||c|| + 2^-20 max||c||^2 is the largest difference of two
    squared distances the kernels may get wrong.  From the kernel file's header: the split
    product x.c ~ xh.ch + xl.ch + xh.cl is off by about 2^-16 ||x|| ||c||; the folded factor
    -2 doubles that (2^-15), and a comparison involves two competing centres (2^-14).  The
    fp32 accumulation of D <= 160 terms adds about 2^-16.7 of the same scale per centre,
    2^-15.7 for two: 2^-14 + 2^-15.7 = 2^-13.6, and a 2.5x margin gives 2^-12.3 <= 2^-12.
    The second term covers the fp32 ||c||^2 (2^-24 max||c||^2 per centre) with the same kind
    of margin.  It comes from the header, not from what the kernels return.

    Asserted for all rows, with no share-of-rows escape:
      * decided rows (runner-up gap > tau): ``a`` is the fp64 argmin exactly;
      * every other row: 0 <= a < K and d64(x, C[a]) <= min + tau;
      * ``mind`` when given: |mind - d64(x, C[a])| <= tau + 2^-18 d64;
      * from the reference alone (``kind``): no undecided row on blobs, at most 5% on
        uniform data -- "near tie" cannot excuse a wrong kernel.
    Exact ties (duplicated centres) are asserted by calling this with the centres WITHOUT
    their duplicates: the lower index is then the only index below K."""
    Kc = C.shape[0]
    d, mn, am, gap, tau = _reference(X, C)
    a = a.long()
    if keep is None:
        keep = torch.ones(X.shape[0], dtype=torch.bool, device=X.device)
    assert bool(((a >= 0) & (a < Kc)).all()), "index outside [0, K)"
    decided = gap > tau
    if kind is not None:
        share = float((~decided[keep]).double().mean())
        print(f"undecided share {kind} n={X.shape[0]} D={X.shape[1]} K={Kc}: {share:.4f}")
        assert share <= MAX_UNDECIDED[kind], share
    wrong = keep & decided & (a != am)
    assert not bool(wrong.any()), (int(wrong.sum()), wrong.nonzero()[:8].flatten().tolist())
    da = d.gather(1, a[:, None])[:, 0]
    far = keep & ~(da <= mn + tau)
    assert not bool(far.any()), (int(far.sum()), float((da - mn)[far].max()))
    if mind is not None:
        err = (mind.double() - da).abs()
        bad = keep & ~(err <= tau + 2.0 ** -18 * da)
        assert not bool(bad.any()), (int(bad.sum()), float(err[bad].max()))


def _gpu_data(gpu, kind, n, D, Kc):
    X, C = _data(kind, n, D, Kc)
    return X.to(gpu), C.to(gpu)


# ------------------------------------------------------------------ assign / screen / pair
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Kc", [1, 7, 32, 33, 100])
@pytest.mark.parametrize("D", WIDTHS)
def test_gpu_split_assign_every_width(gpu, D, Kc, kind):
    X, C = _gpu_data(gpu, kind, N_ROWS, D, Kc)
    a, d = K.assign(X, C, mode="split")
    _oracle(X, C, a, d, kind)


def _assign_stage_bytes(D):
    Dp = (D + 31) // 32 * 32
    return 2 * (4 if Dp <= 128 else 2) * 2 * 32 * Dp * 2


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,Kc,n", [(128, 8224, N_ROWS), (32, 32800, 257)])
def test_gpu_split_assign_centre_norms_outside_lds(gpu, D, Kc, n, kind):
    """kmeans_assign_kernel<KS,1,false>: stage bytes + 4 Cpad > 160 KB, so ||c||^2 is read
    from global memory per chunk and added in the epilogue."""
    Cpad = (Kc + 31) // 32 * 32                  # the first padded count past the limit
    assert _assign_stage_bytes(D) + 4 * Cpad > 160 * 1024 >= _assign_stage_bytes(D) + 4 * (Cpad - 32)
    assert n * Kc <= 10_000_000
    X, C = _gpu_data(gpu, kind, n, D, Kc)
    a, d = K.assign(X, C, mode="split")
    _oracle(X, C, a, d, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,tt", [(D, tt) for D in WIDTHS for tt in (1, 2) if D <= 128 or tt == 1])
def test_gpu_plain_screen_every_variant(gpu, D, tt, kind, monkeypatch):
    """mode='screen' with one and two tiles per wave (one above D = 128), rows converted in
    the prologue or pre-split (D <= 128), with and without the exact distance: each passes
    the oracle and all four give the same assignment."""
    monkeypatch.setattr(K, "SCREEN_TT", tt)
    X, C = _gpu_data(gpu, kind, N_ROWS, D, 100)
    P = K.prepare_centers(C)
    first = None
    for ps in ([False, True] if D <= 128 else [False]):
        monkeypatch.setattr(K, "PRESPLIT", ps)
        K.clear_presplit()
        for need_dist in (True, False):
            st = {}
            a, d = K.assign(X, C, P, mode="screen", stats=st, need_dist=need_dist)
            assert st["mode"] == "screen" and (d is None) == (not need_dist)
            assert (K.presplit(X, K.x_scale(X)) is not None) == ps
            _oracle(X, C, a, d, kind)
            if kind == "blobs":
                assert st["flagged"] == 0            # gaps of hundreds against a bound below one
            first = a if first is None else first
            assert torch.equal(a, first), (ps, need_dist)
    K.clear_presplit()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", WIDTHS)
def test_gpu_pair_screen_every_width(gpu, D, kind):
    X, C = _gpu_data(gpu, kind, N_ROWS, D, 100)
    st = {}
    a, d = K.assign(X, C, mode="pair", stats=st)
    assert st["mode"] == "pair"
    _oracle(X, C, a, d, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "screen", "pair", "auto"])
@pytest.mark.parametrize("D", [64, 96, 160])
def test_gpu_exact_ties_go_to_the_lower_index(gpu, D, mode):
    """Centres 0..4 repeated at the end (K = 33 + 5: the copies sit in another chunk and
    in the other half-wave's slots): every row picks an index below 33, the fp64 argmin."""
    X, C = _gpu_data(gpu, "blobs", N_ROWS, D, 33)
    C2 = torch.cat([C, C[:5]])
    a, d = K.assign(X, C2, mode=mode)
    _oracle(X, C, a, d, "blobs")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_approx_assign_keeps_its_rule(gpu, kind):
    """mode='approx' (test_kmeans.test_gpu_approx_assign_is_within_the_screen_bound): the
    distance is exact for the picked centre, the pick within twice the screen bound of the
    minimum."""
    X, C = _gpu_data(gpu, kind, N_ROWS, 96, 100)
    a, d = K.assign(X, C, mode="approx")
    d64, mn, _, _, tau = _reference(X, C)
    assert bool(((a >= 0) & (a < 100)).all())
    da = d64.gather(1, a.long()[:, None])[:, 0]
    assert bool(((d.double() - da).abs() <= tau + 2.0 ** -18 * da).all())
    # the screened keys order the pick before the minimum: each is within E of its exact
    # partial distance, and its slot code moves it by less than 2^-19 of |p| <= d + ||x||^2
    xn = (X.double() ** 2).sum(1)
    bound = 2 * K.row_bound(X, K.prepare_centers(C), K.x_scale(X)) + 2.0 ** -18 * (da + mn + 2 * xn)
    assert bool((da <= mn + bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "screen"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257])
def test_gpu_assign_row_counts(gpu, n, mode):
    X, C = _gpu_data(gpu, "blobs", n, 64, 33)
    a, d = K.assign(X, C, mode=mode)
    _oracle(X, C, a, d, "blobs")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "screen", "pair"])
@pytest.mark.parametrize("D,wide", [(128, 160), (36, 64)])
def test_gpu_assign_strided_rows(gpu, D, wide, mode, monkeypatch):
    """X = big[:, :D] of a wider tensor: aligned base, row stride != D."""
    Xc, C = _data("uniform", N_ROWS, D, 33)
    big = torch.full((N_ROWS, wide), 7.0, device=gpu)
    big[:, :D] = Xc.to(gpu)
    X = big[:, :D]
    assert X.stride(0) == wide and X.data_ptr() % 16 == 0 and K.kernel_ok(X)
    C = C.to(gpu)
    for ps in (False, True):                     # (the presplit kernel reads the strided rows too)
        monkeypatch.setattr(K, "PRESPLIT", ps)
        K.clear_presplit()
        a, d = K.assign(X, C, mode=mode)
        _oracle(X, C, a, d, "uniform")
    K.clear_presplit()


def _raw_screen(X, n, P, a, d, cnt, flag, tt=2, pair=0, rows=None, bnd=None):
    xs = K.x_scale(X)
    eps_x, eps0, eps_e = K.screen_bound(P, xs, X.shape[1])
    f = Ct.c_float
    N.check(N.kernels().o3s_kmeans_screen2(
        X.data_ptr(), n, X.stride(0), X.shape[1], P.h16.data_ptr(), P.cn.data_ptr(), P.c32.data_ptr(),
        P.c32.stride(0), P.hi.shape[0], f(eps_x), f(eps0), f(eps_e * P.ms), f(xs), f(xs * P.ms), a.data_ptr(),
        N.ptr(d), cnt.data_ptr(), flag.data_ptr(), tt, pair, None, None, N.ptr(rows), N.ptr(bnd),
        N.stream_of(X)), "kmeans_screen")


def _raw_split(X, n, P, a, d, rows=None):
    N.check(N.kernels().o3s_kmeans_assign(X.data_ptr(), n, X.stride(0), X.shape[1], P.hi.data_ptr(),
                                          P.lo.data_ptr(), P.cn.data_ptr(), P.hi.shape[0], a.data_ptr(),
                                          N.ptr(d), N.ptr(rows), N.stream_of(X)), "kmeans_assign")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N_ROWS, 33])
def test_gpu_guard_words_and_rowlist(gpu, n):
    """The raw entry points write rows [0, n) of their outputs (with a row list: the listed
    rows) and nothing else: 64 sentinel entries behind each output stay as they were."""
    X, C = _gpu_data(gpu, "uniform", n, 68, 33)
    P = K.prepare_centers(C)
    A, F = -77, -123.0

    def outputs():
        return (torch.full((n + 64,), A, dtype=torch.int32, device=gpu),
                torch.full((n + 64,), F, dtype=torch.float32, device=gpu),
                torch.full((n + 64,), A, dtype=torch.int32, device=gpu),
                torch.full((n + 64, 2), F, dtype=torch.float32, device=gpu))
    g = torch.Generator().manual_seed(n)
    rows = torch.sort(torch.randperm(n, generator=g)[: max(1, n // 3)]).values.to(torch.int32).to(gpu)
    out = torch.zeros(n, dtype=torch.bool, device=gpu)
    out[rows.long()] = True
    ref = K.assign(X, C, mode="split")
    _oracle(X, C, *ref, "uniform")

    a, d, _, _ = outputs()                                     # split kernel, every row
    _raw_split(X, n, P, a, d)
    assert torch.equal(a[:n], ref[0]) and torch.equal(d[:n], ref[1])
    assert bool((a[n:] == A).all()) and bool((d[n:] == F).all())
    a, d, _, _ = outputs()                                     # split kernel, listed rows
    _raw_split(X, rows.numel(), P, a, d, rows)
    assert torch.equal(a[:n][out], ref[0][out]) and torch.equal(d[:n][out], ref[1][out])
    assert bool((a[:n][~out] == A).all()) and bool((d[:n][~out] == F).all())
    assert bool((a[n:] == A).all()) and bool((d[n:] == F).all())

    for pair in (0, 1):
        for rl in (None, rows):
            m = n if rl is None else int(rl.numel())
            a, d, flag, bnd = outputs()
            cnt = torch.zeros(1, dtype=torch.int32, device=gpu)
            _raw_screen(X, m, P, a, d, cnt, flag, pair=pair, rows=rl, bnd=bnd)
            c = int(cnt)
            written = out if rl is not None else torch.ones_like(out)
            assert 0 <= c <= m
            fl = flag[:c].long()
            assert bool((flag[c:] == A).all())
            assert bool(written[fl].all()) and fl.unique().numel() == c      # listed rows, each once
            assert bool((a[:n][~written] == A).all()) and bool((d[:n][~written] == F).all())
            assert bool((bnd[:n][~written] == F).all())
            assert bool((a[n:] == A).all()) and bool((d[n:] == F).all()) and bool((bnd[n:] == F).all())
            # the screen's own rows are final; its flagged rows go to the split kernel
            if c:
                _raw_split(X, c, P, a, d, flag)
            if not pair:                         # (the pair screen settles some ties itself, in fp32)
                assert torch.equal(a[:n][written], ref[0][written])
            _oracle(X, C, torch.where(written, a[:n], ref[0]), torch.where(written, d[:n], ref[1]), "uniform")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "screen", "pair", "auto", "approx"])
@pytest.mark.parametrize("D,Kc", [(64, 33), (96, 100), (160, 7)])
def test_gpu_non_finite_rows_keep_indices_in_range(gpu, D, Kc, mode):
    """One all-NaN row and one row holding an inf: their index still lies in [0, K) (the
    update kernel indexes LDS with it) and every other row passes the oracle."""
    Xc, C = _data("blobs", N_ROWS, D, Kc)
    X = Xc.clone()
    X[5] = float("nan")
    X[700, D // 2] = float("inf")
    X, C = X.to(gpu), C.to(gpu)
    keep = torch.ones(N_ROWS, dtype=torch.bool, device=gpu)
    keep[5] = keep[700] = False
    for need_dist in (True, False):
        a, d = K.assign(X, C, mode=mode, need_dist=need_dist)
        assert bool(((a >= 0) & (a < Kc)).all()), a[[5, 700]].tolist()
        Xf = torch.where(keep[:, None], X, torch.zeros_like(X))      # a finite reference for the others
        if mode == "approx":
            d64 = _sqdist(Xf, C)
            da = d64.gather(1, a.long()[:, None])[:, 0]
            mn = d64.min(1).values
            # (test_gpu_approx_assign_keeps_its_rule; a non-finite max |x| scales the rows by 1)
            bound = 2 * K.row_bound(Xf, K.prepare_centers(C), 1.0) \
                + 2.0 ** -18 * (da + mn + 2 * (Xf.double() ** 2).sum(1))
            assert bool((da <= mn + bound)[keep].all())
        else:
            _oracle(Xf, C, a, d, None, keep)


# ----------------------------------------------------------------------------- Hamerly bounds
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Kc", [7, 100])
@pytest.mark.parametrize("D", [32, 68, 128, 160])
def test_gpu_hamerly_bounds_are_certificates(gpu, D, Kc, kind, monkeypatch):
    """assign_bounded's bnd[row] = (ub, lb) against fp64 distances.

    Soundness, no tolerance: ub >= ||x - c_a|| and lb <= ||x - c|| for every c != a.
    Tightness: with E = K.row_bound, a row whose fp64 runner-up gap exceeds 8 E is certified
    (finite ub, lb > 0) with ub^2 <= d_a + 4 E + s and lb^2 >= d_2 - 4 E - s, where
    s = 2^-16 (||x||^2 + |p_a| + |p_2|) over the partial distances p = ||c||^2 - 2 x.c.  The
    kernel's epilogue: a screened partial distance is within E of the exact one, and the
    margin it adds is mg = bound / S with bound = 2 S E (+ 2^-18 of the keys for the slot
    codes), so ub^2 and lb^2 sit within 3 E of the exact squares: 4 E holds with one E to
    spare, and s covers the slot codes, the 2^-20 slack and the two (1 +- 2^-20) factors.
    A screened gap is at least the true gap less 2 E, so 8 E leaves 6 E against the 2 E the
    kernel asks for.  From the reference alone: such rows are all of the blobs and at least
    half of the uniform rows."""
    X, C = _gpu_data(gpu, kind, N_ROWS, D, Kc)
    n = N_ROWS
    P = K.prepare_centers(C)
    d64, mn, am, gap, tau = _reference(X, C)
    Xd, Cd = X.double(), C.double()
    p64 = (Cd * Cd).sum(1)[None, :] - 2 * Xd @ Cd.T
    E = K.row_bound(X, P, K.x_scale(X))
    g = torch.Generator().manual_seed(D + Kc)
    third = torch.sort(torch.randperm(n, generator=g)[: n // 3]).values.to(torch.int32).to(gpu)
    first = None
    for ps in ([False, True] if D <= 128 else [False]):
        monkeypatch.setattr(K, "PRESPLIT", ps)
        K.clear_presplit()
        for rows in (None, third):
            a = torch.full((n,), -77, dtype=torch.int32, device=gpu)
            bnd = torch.full((n, 2), -123.0, device=gpu)
            K.assign_bounded(X, P, a, bnd, rows)
            w = torch.ones(n, dtype=torch.bool, device=gpu)
            if rows is not None:
                w = torch.zeros(n, dtype=torch.bool, device=gpu)
                w[rows.long()] = True
                assert bool((a[~w] == -77).all()) and bool((bnd[~w] == -123.0).all())    # bit for bit
            al = torch.where(w, a, am.to(torch.int32)).long()
            _oracle(X, C, al, None, kind)
            ub, lb = bnd[:, 0].double(), bnd[:, 1].double()
            da = d64.gather(1, al[:, None])[:, 0]
            pa = p64.gather(1, al[:, None])[:, 0]
            rest = d64.clone()
            rest[torch.arange(n, device=gpu), al] = float("inf")
            d2, i2 = rest.min(1)
            p2 = p64.gather(1, i2[:, None])[:, 0]
            # soundness
            assert bool((ub >= da.sqrt())[w].all()), float((da.sqrt() - ub)[w].max())
            assert bool((lb <= d2.sqrt())[w].all()), float((lb - d2.sqrt())[w].max())
            # tightness
            clear = (d2 - da) > 8 * E
            share = float(clear.double().mean())
            print(f"rows clear of 8E {kind} D={D} K={Kc}: {share:.4f}")
            assert share == 1.0 if kind == "blobs" else share >= 0.5
            cw = clear & w
            assert bool(torch.isfinite(ub[cw]).all()) and bool((lb[cw] > 0).all())
            s = 2.0 ** -16 * ((Xd * Xd).sum(1) + pa.abs() + p2.abs())
            assert bool((ub * ub <= da + 4 * E + s)[cw].all())
            assert bool((lb * lb >= d2 - 4 * E - s)[cw].all())
            if rows is None:
                first = (a, bnd) if first is None else first
                assert torch.equal(a, first[0])                      # presplit rows: the same pick
    K.clear_presplit()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_gpu_bounds_recheck_small_sizes(gpu, n):
    g = torch.Generator().manual_seed(n)
    Kc = 9
    a = torch.randint(0, Kc, (n,), generator=g, dtype=torch.int32)
    ub = torch.rand(n, generator=g) * 2
    lb = ub + torch.randn(n, generator=g) * 0.3
    lb[n // 2] = float("nan")
    bnd = torch.stack([ub, lb], 1).contiguous()
    delta = torch.rand(Kc, generator=g) * 0.05
    dmax = float(delta.max())
    b_ref = bnd.clone()
    m_ref, r_ref = K.bounds_recheck(a, b_ref, delta, dmax)
    assert m_ref >= 1 and n // 2 in r_ref.tolist()               # the NaN bound is rechecked
    b_gpu = bnd.to(gpu)
    m, r = K.bounds_recheck(a.to(gpu), b_gpu, delta.to(gpu), dmax)
    assert m == m_ref and torch.equal(r.cpu(), r_ref)
    torch.testing.assert_close(b_gpu.cpu(), b_ref, rtol=0, atol=0, equal_nan=True)
    for max_rows in (m_ref - 1, m_ref):
        b2 = bnd.to(gpu)
        m2, r2 = K.bounds_recheck(a.to(gpu), b2, delta.to(gpu), dmax, max_rows=max_rows)
        assert m2 == m_ref
        assert r2 is None if max_rows < m_ref else torch.equal(r2.cpu(), r_ref)
        torch.testing.assert_close(b2.cpu(), b_ref, rtol=0, atol=0, equal_nan=True)


# ------------------------------------------------------------------------------ update kernel
def _update_ws(gpu, Kp, D):
    """(workspace with three blocks, LDS bytes, rows per chunk R) as the library reports them."""
    ws = K.UpdateWorkspace(gpu, Kp, D, grid=3)
    sf, cf, lds = Ct.c_int64(), Ct.c_int64(), Ct.c_int()
    rc = N.kernels().o3s_kmeans_update_ws(Kp, D, 3, Ct.byref(sf), Ct.byref(cf), Ct.byref(lds))
    assert (rc == 0) == ws.ok
    R = (lds.value - 4 * (Kp + 1) - 16 * Kp) // 2 if ws.ok else 0
    return ws, lds.value, R


def _labels(n, Kp, g):
    """Uniform labels in [0, Kp) with one large bucket and (Kp >= 3) an empty cluster."""
    a = torch.randint(0, Kp, (n,), generator=g, dtype=torch.int32)
    if Kp >= 3:
        a[a == Kp - 2] = 0
    a[: n // 5] = 0
    return a


def _check_update(gpu, X, a, Kp, ws):
    """K.update against update_torch in fp64: equal counts, sums within 2^-20 sum|x| per
    cluster entry (fp32 accumulation in row order; sum|x| from the reference), and a second
    call bitwise equal."""
    assert bool(((a >= 0) & (a < Kp)).all())
    s, c = (t.clone() for t in K.update(X, a, Kp, ws))
    rs, rc = K.update_torch(X, a, Kp)
    rabs, _ = K.update_torch(X.abs(), a, Kp)
    assert torch.equal(c, rc)
    err = (s - rs).abs()
    assert bool((err <= 2.0 ** -20 * rabs).all()), float((err - 2.0 ** -20 * rabs).max())
    s2, c2 = K.update(X, a, Kp, ws)
    assert torch.equal(s, s2) and torch.equal(c, c2)


@pytest.mark.gpu
@pytest.mark.parametrize("Kp,R_want,lds_tier", [(3000, 8192, 80), (7000, 8192, 160), (7600, 4096, 160),
                                                (7900, 2048, 160), (8050, 1024, 160), (8120, 512, 160),
                                                (8160, 256, 160)])
def test_gpu_update_every_chunk_size(gpu, Kp, R_want, lds_tier):
    """upd_rows(Kp) from 8192 rows per chunk (both LDS tiers) down to 256, three blocks
    walking four chunks."""
    ws, lds, R = _update_ws(gpu, Kp, 8)
    assert ws.ok and R == R_want and lds <= lds_tier * 1024 and (lds_tier == 80 or lds > 80 * 1024)
    n = 3 * R + 100
    g = torch.Generator().manual_seed(Kp)
    X = torch.randn(n, 8, generator=g).to(gpu)
    _check_update(gpu, X, _labels(n, Kp, g).to(gpu), Kp, ws)


@pytest.mark.gpu
def test_gpu_update_too_many_clusters_takes_the_torch_path(gpu):
    ws, lds, _ = _update_ws(gpu, 8167, 8)
    assert not ws.ok and lds == -1
    assert _update_ws(gpu, 8166, 8)[0].ok
    g = torch.Generator().manual_seed(1)
    X = torch.randn(1000, 8, generator=g).to(gpu)
    a = _labels(1000, 8167, g).to(gpu)
    s, c = K.update(X, a, 8167, ws)
    rs, rc = K.update_torch(X, a, 8167)
    assert torch.equal(s, rs) and torch.equal(c, rc)


@pytest.mark.gpu
@pytest.mark.parametrize("Kp", [1, 2, 32, 33, 64, 65])
def test_gpu_update_key_count_boundary(gpu, Kp):
    """Kp <= 32 peels one key per step, Kp > 32 sorts the 64 keys of a group."""
    ws, _, R = _update_ws(gpu, Kp, 64)
    assert R == 16384
    n = 3 * R + 100
    g = torch.Generator().manual_seed(Kp)
    X = torch.randn(n, 64, generator=g).to(gpu)
    _check_update(gpu, X, _labels(n, Kp, g).to(gpu), Kp, ws)


@pytest.mark.gpu
@pytest.mark.parametrize("D,ld", [(32, 32), (64, 64), (128, 128), (256, 256), (30, 30), (70, 70), (130, 130),
                                  (250, 250), (64, 66)])
def test_gpu_update_every_lane_layout(gpu, D, ld):
    """Vector rows <1,8> <1,16> <2,32> <4,64> (D % 4 == 0, 16-byte rows), scalar rows <1,0>
    <2,0> <3,0> <4,0> (any other D), and D = 64 at a row stride of 66 floats: scalar too."""
    Kp = 8050                                   # 1024 rows per chunk: a few thousand rows do
    ws, _, R = _update_ws(gpu, Kp, D)
    assert R == 1024
    n = 3 * R + 100
    g = torch.Generator().manual_seed(D + ld)
    big = torch.randn(n, ld, generator=g).to(gpu)
    X = big[:, :D]
    assert X.data_ptr() % 16 == 0 and X.stride(0) == ld
    a = _labels(n, Kp, g)
    a[n // 5:] %= 40                            # buckets of ~60 rows: the four-row loop and its tail
    _check_update(gpu, X, a.to(gpu), Kp, ws)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 16385])
def test_gpu_update_row_counts(gpu, n):
    ws, _, R = _update_ws(gpu, 33, 64)
    assert R == 16384                           # 16385 = R + 1: a second chunk of one row
    g = torch.Generator().manual_seed(n)
    X = torch.randn(n, 64, generator=g).to(gpu)
    _check_update(gpu, X, _labels(n, 33, g).to(gpu), 33, ws)


# ----------------------------------------------------------------- screen LDS limit, alignment
def test_screen_lds_query():
    """The screen kernel holds ||c||^2 of every padded centre in LDS beside its staging
    buffers: at most 24576 centres at a padded D of 128, 20480 at 160."""
    assert K.screen_fits(128, 24576) and not K.screen_fits(128, 24608)
    assert K.screen_fits(100, 24576) and not K.screen_fits(100, 24608)
    assert K.screen_fits(160, 20480) and not K.screen_fits(160, 20512)
    assert K.screen_fits(32, 32800) and K.screen_fits(4, 32)
    lds = Ct.c_int()
    assert N.kernels().o3s_kmeans_screen_lds(128, 1024, Ct.byref(lds)) == 0 and lds.value == 65536 + 4096
    assert N.kernels().o3s_kmeans_screen_lds(164, 32, Ct.byref(lds)) == -2


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["auto", "screen", "pair", "approx", "bounded"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D,Kc", [(128, 24608), (160, 20512)])
def test_gpu_assign_beyond_the_screen_lds_limit(gpu, D, Kc, kind, mode):
    """More centres than the screen kernel's LDS holds: every screen mode (the candidate
    passes of k-means|| run 'approx') answers through the split kernel instead of raising."""
    n = 257
    assert not K.screen_fits(D, Kc) and K.screen_fits(D, Kc - 32)
    X, C = _gpu_data(gpu, kind, n, D, Kc)
    P = K.prepare_centers(C)
    if mode == "bounded":
        a = torch.full((n,), -77, dtype=torch.int32, device=gpu)
        bnd = torch.full((n, 2), -123.0, device=gpu)
        rows = torch.arange(0, n, 3, dtype=torch.int32, device=gpu)
        K.assign_bounded(X, P, a, bnd, rows)
        w = torch.zeros(n, dtype=torch.bool, device=gpu)
        w[rows.long()] = True
        assert bool((a[~w] == -77).all()) and bool((bnd[~w] == -123.0).all())
        assert bool((bnd[w, 0] == float("inf")).all()) and bool((bnd[w, 1] == 0).all())
        K.assign_bounded(X, P, a, bnd, None)
        assert bool((bnd[:, 0] == float("inf")).all()) and bool((bnd[:, 1] == 0).all())
        d = None
    else:
        st = {}
        a, d = K.assign(X, C, P, mode=mode, stats=st)
        assert st["mode"] == "split"
    _oracle(X, C, a, d, kind)


@pytest.mark.gpu
def test_gpu_fit_without_the_screen(gpu, monkeypatch):
    """A fit whose centre count does not fit the screen (here: the LDS query answers 'no'
    for every shape) runs Lloyd without Hamerly bounds, on the split kernel.  From the same
    random initial centres it finds the centres of the ordinary fit (the tolerance of
    test_kmeans.test_gpu_hamerly_lloyd_equals_full_screens); with k-means|| seeding, whose
    candidate passes ask for the screen, it still fits."""
    import numpy as np
    from orange3_spark_amd import Session, SessionConf
    from orange3_spark_amd.ml.clustering import KMeans
    from orange3_spark_amd.models import kmeans as KM
    s = Session(SessionConf().set("o3s.device", "cuda"))
    df = s.synthetic.blobs(2000, 128, k=64, seed=4, spread=0.5)
    m0 = KMeans(k=64, seed=1, maxIter=5, tol=0.0, initMode="random").fit(df)
    assert len(KM.LAST_HAMERLY_STATS) > 0
    called = []
    real = K.assign_bounded
    monkeypatch.setattr(K, "screen_fits", lambda D, Kp: False)
    monkeypatch.setattr(K, "assign_bounded", lambda *a, **k: (called.append(1), real(*a, **k))[1])
    m1 = KMeans(k=64, seed=1, maxIter=5, tol=0.0, initMode="random").fit(df)
    assert not called and len(KM.LAST_HAMERLY_STATS) == 0
    np.testing.assert_allclose(np.array(m1.clusterCenters()), np.array(m0.clusterCenters()), rtol=1e-5, atol=1e-6)
    assert m1.summary.trainingCost == pytest.approx(m0.summary.trainingCost, rel=1e-6)
    m2 = KMeans(k=64, seed=1, maxIter=5, tol=0.0, initSteps=3).fit(df)
    assert not called and sum(m2.summary.clusterSizes) == 2000 and np.isfinite(m2.summary.trainingCost)


@pytest.mark.gpu
def test_gpu_misaligned_base_takes_the_torch_path(gpu):
    """big[:, 1:129] of a 132-wide tensor: whole-float4 row stride, but a base 4 bytes off a
    16-byte boundary -- kernel_ok says no, and assign answers through assign_torch."""
    Xc, C = _data("blobs", N_ROWS, 128, 33)
    big = torch.zeros(N_ROWS, 132, device=gpu)
    big[:, 1:129] = Xc.to(gpu)
    X = big[:, 1:129]
    assert X.stride(0) % 4 == 0 and X.data_ptr() % 16 == 4
    assert not K.kernel_ok(X) and not K.screen_ok(X) and K.kernel_ok(big[:, :128])
    C = C.to(gpu)
    for mode in ("auto", "split", "screen", "pair", "approx"):
        st = {}
        a, d = K.assign(X, C, mode=mode, stats=st)
        assert not st                                   # no kernel mode was chosen
        _oracle(X, C, a, d, "blobs")

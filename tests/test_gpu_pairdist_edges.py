"""GPU: the forms of csrc/pairdist.hip that no other test reaches, and d == 0, each against the
plain fp64 reference of tests/pairdist_ref.py (proved against fp64 autograd on the same input sets
by tests/test_pairdist_ref_host.py).

(a) cdist backward from the LDS image of G, pairdist_tile_kernel<MODE_FULL, VEC = true>: through
    ``ops.pairwise_dist(c).backward(G)`` at N = 128, 256, 384 (diagonal tiles only; one interior
    pair; interior tiles on both sides of the diagonal) and through ``pairdist_bwd`` on a G padded
    to ``padded_ld(N)`` columns at N = 129, 300 (clamped last rows, edge tiles from the image; the pad
    holds 1e6 so a leak of it into a sum shows).
(b) the fused loss reading T from global memory, <MODE_SYM, VEC = false, KIND> for the three kinds:
    an unpadded [N, N] truth at N = 58, 129, 300, 301, and a band of it with a misaligned column
    origin; plus the band argument check.
(c) coincident points through the masked path (inv clamped to 1e30), the packed interior path and the
    support pass (d2 + 2^-100) and the forward (sqrtf(0)): a few coincident pairs at N = 300 / 256 and
    fully collapsed coordinates at N = 129, 300.
(d) more than 16 column tiles per row in pairdist_reduce_kernel (N = 2177, nb = 18), in the SYM and
    the FULL mode.

Tolerances are the suite's existing ones, none widened: D 1e-6, gradients 1e-5 of their max, mse 1e-5
relative, Pearson r 1e-5 (n >= 100), contrastive loss 1e-6 relative and its gradient 1e-5 of the max
plus 2 x scale per near-tie pair of the row (test_gpu_pairdist_occ.py); two kernel forms fed the same
numbers: moments 1e-6 relative, gradients 1e-5.  The raw moments against fp64 are held to 1e-5
relative as well: each is a sum of same-signed terms (or, for L, of squares), at most 64 of them added
in fp32 per thread (64 x 2^-24 = 4e-6 relative at worst) before the fp64 tree, and d itself is good to
2 ulp.

Pearson r of fully collapsed coordinates is not asserted: the reference's is NaN (no variance in d)
and the kernel's depends on which tiles formed d = 2^-50 instead of 0; the values are printed.
"""
import numpy as np
import pytest
import torch

import pairdist_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = R.KINDS
EINVAL_SENTINEL = -7.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hicgat  # noqa: F401  (fails loudly if libhicgat.so is missing)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _dev(a):
    return torch.tensor(a, device=DEV)


@pytest.fixture(scope="module")
def refs():
    """Per input set, computed once and left unchanged: the set and its fp64 distances."""
    cache = {}

    def get(name):
        if name not in cache:
            s = R.inputs(name)
            cache[name] = (s, R.dist(s.c))
        return cache[name]
    return get


def _fused(c, tbuf, n, kind, t0=0, t1=-1, row0=0, col0=0):
    import hicgat
    stats = torch.empty(12, dtype=torch.float64, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    dc = torch.empty_like(c)
    hicgat.kernels.default().fused_loss(c, tbuf, n, KINDS[kind], t0, t1, stats, loss, dc, row0=row0, col0=col0)
    torch.cuda.synchronize()
    return stats.cpu().numpy(), float(loss), dc.cpu().numpy()


def _fused_support(c, tr, kind):
    import hicgat
    stats = torch.empty(12, dtype=torch.float64, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    dc = torch.empty_like(c)
    hicgat.kernels.default().fused_loss_support(c, tr.support, tr.n, KINDS[kind], stats, loss, dc)
    torch.cuda.synchronize()
    return stats.cpu().numpy(), float(loss), dc.cpu().numpy()


def _dense_truth(t):
    """The padded dense truth the fused loss's LDS-image form takes (no background form)."""
    import hicgat
    tr = hicgat.Truth(_dev(t), background=None)
    assert tr.support is None and not tr.asymmetric_source and tr.ld == hicgat.graph.padded_ld(tr.n)
    return tr


def _bg_truth(tb):
    import hicgat
    from hicgat import graph
    tr = hicgat.Truth(_dev(tb))
    if tr.support is None:
        tr.support = graph.SupportForm.build(tr, R.BG, max_fraction=1.0)
    assert tr.support is not None and tr.support.background == R.BG and not tr.asymmetric_source
    return tr


def _moment_ids(kind):
    return {"mse": (0, 6), "combined": tuple(range(7)), "contrastive": (0,)}[kind]


def _contrastive_excess(g, gref, D, t, n):
    """Worst |g - gref| beyond 2 x scale per near-tie pair of the row, relative to max |gref|."""
    near = R.near_ties(D, t)
    allow = 2.0 * R.contrastive_scale(n) * near.sum(1).astype(np.float64)
    excess = np.clip(np.abs(g.astype(np.float64) - gref) - allow[:, None], 0.0, None)
    return float(excess.max()) / max(float(np.abs(gref).max()), 1e-30), int(near.sum()) // 2


def _check_whole_vs_ref(label, out, s, t, D, kind):
    """One whole fused-loss call (stats, loss, dcoords) against the fp64 reference."""
    st, loss, g = out
    n = s.n
    # (stats[8] is NaN by design outside the combined kind, and the mse kind's total with it)
    assert np.isfinite(g).all() and np.isfinite(loss) and np.isfinite(st[:8]).all() and np.isfinite(st[9])
    assert np.isfinite(st[10]) or kind == "mse"
    if kind == "contrastive":
        l_ref = R.contrastive(D, t)
        worst, ties = _contrastive_excess(g, R.grad_contrastive(s.c, t, D), D, t, n)
        print(f"{label} {kind}: loss {st[10]:.10g} fp64 {l_ref:.10g}; dcoords excess {worst:.1e} ({ties} near ties)")
        assert abs(st[10] - l_ref) <= 1e-6 * l_ref and abs(loss - l_ref) <= 1e-6 * l_ref
        assert abs(st[7] - 10 * l_ref) <= 1e-6 * 10 * l_ref and np.isnan(st[8]) and st[9] == 0.1
        assert worst <= 1e-5
        return
    m = R.moments(D, t)
    mse = R.mse(m, n)
    gerr = _rel(g, R.grad_mse(s.c, t, D))
    merr = max(abs(st[k] - m[k]) / max(abs(m[k]), 1e-30) for k in _moment_ids(kind))
    print(f"{label} {kind}: mse {st[7]:.9g} fp64 {mse:.9g}; moments rel {merr:.1e}; grad rel {gerr:.1e}")
    assert abs(st[7] - mse) <= 1e-5 * mse
    assert merr <= 1e-5
    assert gerr < 1e-5
    if kind == "mse":
        assert abs(loss - mse) <= 1e-5 * mse
        return
    assert np.isfinite(st[8])
    if n >= 100:
        r = R.pearson(D, t)
        print(f"  r {st[8]:.9g} fp64 {r:.9g}")
        assert abs(st[8] - r) <= 1e-5


def _check_forms_agree(label, a, b, kind, n, D=None, t=None):
    """Two kernel forms fed the same numbers: moments, stats[7..10] and dcoords."""
    (sa, la, ga), (sb, lb, gb) = a, b
    merr = max(abs(sa[k] - sb[k]) / max(abs(sb[k]), 1e-30) for k in _moment_ids(kind))
    if kind == "contrastive":
        gerr, _ = _contrastive_excess(ga, gb.astype(np.float64), D, t, n)
    else:
        gerr = _rel(ga, gb)
    print(f"{label} {kind}: forms agree: moments {merr:.1e} stats[7] {abs(sa[7] - sb[7]) / abs(sb[7]):.1e} "
          f"grad {gerr:.1e}")
    assert merr <= 1e-6
    assert gerr <= 1e-5
    assert abs(sa[7] - sb[7]) <= 1e-6 * abs(sb[7])
    assert abs(la - lb) <= 1e-6 * abs(lb)
    if kind == "contrastive":
        assert np.isnan(sa[8]) and np.isnan(sb[8]) and sa[9] == sb[9] == 0.1
        assert abs(sa[10] - sb[10]) <= 1e-6 * abs(sb[10])
        return
    rtol = 1e-6 if n >= 100 else 1e-5
    if kind == "combined":
        assert abs(sa[8] - sb[8]) <= rtol
    assert abs(sa[9] - sb[9]) <= 1e-6 * abs(sb[9])
    if kind == "combined":   # total = mse + alpha (1 - r)
        assert abs(sa[10] - sb[10]) <= 1e-6 * max(1.0, abs(sb[10])) + sb[9] * rtol


def _lds_image_form(G, n):
    """hicgat_pairdist_bwd's condition for the LDS-image form, on the buffer it is handed."""
    nb = (n + R.BT - 1) // R.BT
    return G.is_contiguous() and G.shape[1] % 4 == 0 and G.data_ptr() % 16 == 0 and G.shape[1] >= nb * R.BT


def _sym_lds_image_form(tbuf, n, col0):
    """hicgat_pairdist_mse_fused's condition for the LDS-image form."""
    nb = (n + R.BT - 1) // R.BT
    return (tbuf.is_contiguous() and tbuf.shape[1] % 4 == 0 and col0 % 4 == 0 and tbuf.data_ptr() % 16 == 0
            and tbuf.shape[1] >= nb * R.BT - col0)


# ------------------------------------------------------------------ (a) cdist backward, LDS-image form
def _op_fwd_bwd(s, expect_lds):
    import hicgat
    c = _dev(s.c).requires_grad_(True)
    G = _dev(s.g)
    assert _lds_image_form(G, s.n) == expect_lds
    Dm = hicgat.ops.pairwise_dist(c)
    Dm.backward(G)      # G itself reaches the kernel: contiguous fp32 already
    torch.cuda.synchronize()
    return Dm.detach().cpu().numpy(), c.grad.cpu().numpy()


@pytest.mark.parametrize("n", [128, 256, 384])
def test_cdist_backward_lds_image_through_op(refs, n):
    s, D = refs(f"lds{n}")
    Dm, g = _op_fwd_bwd(s, expect_lds=True)
    derr, gerr = _rel(Dm, D), _rel(g, R.grad_cdist(s.c, s.g, D))
    print(f"n {n}: D rel {derr:.1e} grad rel {gerr:.1e}")
    assert np.isfinite(g).all()
    assert derr < 1e-6 and np.all(np.diagonal(Dm) == 0)
    assert gerr < 1e-5


@pytest.mark.parametrize("n", [129, 300])
def test_cdist_backward_lds_image_padded_g(refs, n):
    import hicgat
    from hicgat import graph
    s, D = refs(f"lds{n}")
    K = hicgat.kernels.default()
    c, G = _dev(s.c), _dev(s.g)
    Gp = torch.full((n, graph.padded_ld(n)), 1e6, dtype=torch.float32, device=DEV)
    Gp[:, :n] = G
    assert _lds_image_form(Gp, n) and not _lds_image_form(G, n)
    g_img = K.pairdist_bwd(c, Gp).cpu().numpy()
    g_glb = K.pairdist_bwd(c, G).cpu().numpy()
    torch.cuda.synchronize()
    gref = R.grad_cdist(s.c, s.g, D)
    print(f"n {n}: grad rel fp64: image {_rel(g_img, gref):.1e} global {_rel(g_glb, gref):.1e}; "
          f"image vs global {_rel(g_img, g_glb):.1e}")
    assert np.isfinite(g_img).all()
    assert _rel(g_img, gref) < 1e-5
    assert _rel(g_img, g_glb) < 1e-5


# ------------------------------------------------------------------ (b) fused loss, global-read form
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", [58, 129, 300, 301])
def test_fused_loss_global_read_form(refs, n, kind):
    s, D = refs(f"glob{n}")
    c, t32 = _dev(s.c), _dev(s.t)
    assert t32.shape == (n, n) and not _sym_lds_image_form(t32, n, 0)
    out = _fused(c, t32, n, kind)
    _check_whole_vs_ref(f"global-read n {n}", out, s, s.t, D, kind)
    tr = _dense_truth(s.t)
    assert _sym_lds_image_form(tr.buf, n, 0)
    _check_forms_agree(f"n {n}", out, _fused(c, tr.buf, n, kind), kind, n, D, s.t)


BAND = dict(t0=3, t1=6, row0=120, col0=126)    # tile-rows 1 and 2 of N = 300


@pytest.mark.parametrize("kind", ["mse", "combined"])
def test_fused_loss_global_read_band(refs, kind):
    s, D = refs("glob300")
    n = s.n
    c, t32 = _dev(s.c), _dev(s.t)
    tbuf = t32[BAND["row0"]:n, BAND["col0"]:n].contiguous()
    assert tbuf.shape[1] == 174 and not _sym_lds_image_form(tbuf, n, BAND["col0"])
    st, _, g = _fused(c, tbuf, n, kind, **BAND)
    m, gref = R.tile_range(s.c, s.t, BAND["t0"], BAND["t1"], kind, D)
    merr = max(abs(st[k] - m[k]) / max(abs(m[k]), 1e-30) for k in _moment_ids(kind))
    print(f"band {kind}: moments rel fp64 {merr:.1e} grad rel fp64 {_rel(g, gref):.1e}")
    assert np.isfinite(g).all() and np.isfinite(st[:7]).all()
    assert merr <= 1e-5
    assert _rel(g, gref) < 1e-5
    assert np.all(g[:128] == 0)       # rows of tile-row 0 meet no tile of the range
    # the same range from the aligned band of the padded truth (the LDS-image form)
    ab = _dense_truth(s.t).buf[128:, 128:].contiguous()
    assert _sym_lds_image_form(ab, n, 128)
    sa, _, ga = _fused(c, ab, n, kind, BAND["t0"], BAND["t1"], 128, 128)
    merr2 = max(abs(st[k] - sa[k]) / max(abs(sa[k]), 1e-30) for k in _moment_ids(kind))
    print(f"  vs aligned band: moments {merr2:.1e} grad {_rel(g, ga):.1e}")
    assert merr2 <= 1e-6
    assert _rel(g, ga) <= 1e-5


def test_fused_loss_band_rejects_column_origin_past_first_tile_row():
    """col0 = 129 > I0 * 128 = 128: the band lacks a column of tile (1, 1); HICGAT_EINVAL before
    any launch (the outputs keep what they held)."""
    import hicgat
    from hicgat import _lib
    s = R.inputs("glob300")
    n = s.n
    c, t32 = _dev(s.c), _dev(s.t)
    tbuf = t32[BAND["row0"]:n, BAND["col0"]:n].contiguous()
    stats = torch.full((12,), EINVAL_SENTINEL, dtype=torch.float64, device=DEV)
    loss = torch.full((), EINVAL_SENTINEL, dtype=torch.float32, device=DEV)
    dc = torch.full_like(c, EINVAL_SENTINEL)
    with pytest.raises(_lib.HicgatError, match="hicgat_pairdist_mse_fused failed: invalid argument"):
        hicgat.kernels.default().fused_loss(c, tbuf, n, KINDS["mse"], BAND["t0"], BAND["t1"], stats, loss, dc,
                                            row0=BAND["row0"], col0=129)
    torch.cuda.synchronize()
    assert bool((stats == EINVAL_SENTINEL).all()) and float(loss) == EINVAL_SENTINEL
    assert bool((dc == EINVAL_SENTINEL).all())


# ------------------------------------------------------------------ (c) coincident points
@pytest.mark.parametrize("kind", list(KINDS))
def test_coincident_points_dense_truth(refs, kind):
    s, D = refs("coin300")
    assert s.t[5, 130] == 0.0 and s.t[5, 6] != 0.0 and D[5, 130] == 0.0 and D[5, 6] == 0.0 and D[140, 299] == 0.0
    out = _fused(_dev(s.c), _dense_truth(s.t).buf, s.n, kind)
    _check_whole_vs_ref("coincident dense", out, s, s.t, D, kind)


@pytest.mark.parametrize("kind", list(KINDS))
def test_coincident_points_background_form(refs, kind):
    s, D = refs("coin300")
    tr = _bg_truth(s.tb)
    rp, col = tr.support.rowptr.cpu().long(), tr.support.col.cpu().long()
    row5, row140 = col[rp[5]:rp[6]].tolist(), col[rp[140]:rp[141]].tolist()
    # coincident pairs: two support entries (t = 0 and t = 0.75) and a background pair
    assert 130 in row5 and 6 in row5 and 299 not in row140
    assert np.array_equal(tr.dense().cpu().numpy(), s.tb)
    _check_whole_vs_ref("coincident background", _fused_support(_dev(s.c), tr, kind), s, s.tb, D, kind)


@pytest.mark.parametrize("name", ["coin300", "coin256"])
def test_coincident_points_cdist(refs, name):
    """Forward and backward; at N = 256 the backward is the LDS-image form of (a)."""
    s, D = refs(name)
    Dm, g = _op_fwd_bwd(s, expect_lds=(s.n % 128 == 0))
    for a, b in s.coincident:
        assert Dm[a, b] == 0.0 and Dm[b, a] == 0.0
    derr, gerr = _rel(Dm, D), _rel(g, R.grad_cdist(s.c, s.g, D))
    print(f"{name}: D rel {derr:.1e} grad rel {gerr:.1e}")
    assert np.isfinite(Dm).all() and np.isfinite(g).all()
    assert derr < 1e-6 and np.all(np.diagonal(Dm) == 0)
    assert gerr < 1e-5


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("form", ["dense", "background"])
@pytest.mark.parametrize("n", [129, 300])
def test_collapsed_coordinates(refs, n, form, kind):
    """Every row of c equal: no gradient anywhere, mse = mean(T^2), contrastive = 0.1 mean |T|.  The
    combined kind runs for its mse and gradient; its Pearson r is printed, not asserted."""
    s, D = refs(f"flat{n}")
    assert not D.any()
    c = _dev(s.c)
    if form == "dense":
        t = s.t
        st, loss, g = _fused(c, _dense_truth(t).buf, n, kind)
    else:
        t = s.tb
        st, loss, g = _fused_support(c, _bg_truth(t), kind)
    t64 = t.astype(np.float64)
    assert np.isfinite(g).all() and np.all(g == 0)
    if kind == "contrastive":
        iu = np.triu_indices(n, 1)
        l_ref = 0.1 * np.abs(t64[iu]).mean()
        assert abs(l_ref - R.contrastive(D, t)) <= 1e-15
        print(f"collapsed {form} n {n}: contrastive {st[10]:.10g} fp64 {l_ref:.10g}")
        assert abs(st[10] - l_ref) <= 1e-6 * l_ref and abs(loss - l_ref) <= 1e-6 * l_ref
        return
    mse = (t64 * t64).mean()
    assert abs(mse - R.mse(R.moments(D, t), n)) <= 1e-12 * mse
    print(f"collapsed {form} n {n} {kind}: mse {st[7]:.9g} fp64 {mse:.9g}" +
          (f"; r {st[8]!r} (fp64: nan)" if kind == "combined" else ""))
    assert abs(st[7] - mse) <= 1e-5 * mse
    if kind == "mse":
        assert abs(loss - mse) <= 1e-5 * mse


# ------------------------------------------------------------------ (d) reduce beyond 16 column tiles
def test_reduce_second_column_group_fused_loss(refs):
    s, D = refs("big2177")
    assert (s.n + R.BT - 1) // R.BT == 18 and s.n % 64 == 1
    st, loss, g = _fused(_dev(s.c), _dense_truth(s.t).buf, s.n, "mse")
    mse = R.mse(R.moments(D, s.t), s.n)
    gerr = _rel(g, R.grad_mse(s.c, s.t, D))
    print(f"n {s.n}: mse {st[7]:.9g} fp64 {mse:.9g} grad rel {gerr:.1e}")
    assert np.isfinite(g).all()
    assert abs(st[7] - mse) <= 1e-5 * mse
    assert gerr < 1e-5


def test_reduce_second_column_group_cdist_backward(refs):
    s, D = refs("big2177")
    Dm, g = _op_fwd_bwd(s, expect_lds=False)
    derr, gerr = _rel(Dm, D), _rel(g, R.grad_cdist(s.c, s.g, D))
    print(f"n {s.n}: D rel {derr:.1e} grad rel {gerr:.1e}")
    assert np.isfinite(g).all()
    assert derr < 1e-6
    assert gerr < 1e-5

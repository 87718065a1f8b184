"""GPU: the background + support form of the fused loss at the sizes where the tile kernel's epilogue
(row partials through planar LDS, column partials by lane shuffles and a cross-wave LDS sum, fp64
moments) can go wrong, for the three loss kinds, through ``hicgat.ops.fused_dist_loss``.

Sizes: N = 2, 3 (less than one thread's 8 x 8 patch), 127 / 128 / 129 (a partial tile, exactly one
tile, one tile plus a one-row tile: the column partials of tile (0, 1) have one live column), 257
(three row blocks: diagonal and off-diagonal tiles with a ragged last block) and 300 with two
supports: "300e" leaves rows 100..149 and 299 empty and fills row 7 at every other column (a
symmetric support cannot have a full row beside an empty one), "300f" fills row 7 entirely.

References and tolerances are those of tests/test_gpu_support.py (an fp64 torch restatement: mse 1e-5
relative, gradients 1e-5 of their max, Pearson r 1e-5 for n >= 100; against the dense-truth kernel,
which adds the same terms in another order: moments 1e-6 relative, r 1e-6 for n >= 100 else 1e-5) and,
for the contrastive kind, of tests/test_gpu_contrastive.py (fp64 loss 1e-6 relative; gradients 1e-5
of their max plus 2 x scale per pair of the row whose sign(d - t) rounding can decide).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = {"mse": 0, "combined": 1, "contrastive": 2}
CASES = ["2", "3", "127", "128", "129", "257", "300e", "300f"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hicgat  # noqa: F401  (fails loudly if libhicgat.so is missing)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _truth_matrix(case):
    """A symmetric target at the background 1 off the diagonal except at a support; zero diagonal
    but for a few entries (the MSE's diagonal moment)."""
    n = int(case.rstrip("ef"))
    rng = np.random.default_rng(n)
    t = np.ones((n, n))
    if n <= 3:
        mask = np.ones((n, n), bool)
    else:
        mask = np.triu(rng.random((n, n)) < 0.05, 1)
    if case in ("300e", "300f"):
        mask[7, :] = True
        mask[:, 7] = True
    vals = 0.05 + 2.5 * rng.random((n, n))
    mask = np.triu(mask, 1)
    t[mask] = vals[mask]
    t = np.triu(t, 1)
    t = t + t.T
    if case == "300e":
        empty = list(range(100, 150)) + [299]
        t[empty, :] = 1.0
        t[:, empty] = 1.0
    np.fill_diagonal(t, 0.0)
    t[n // 2, n // 2] = 0.25
    return n, t


@pytest.fixture(scope="module")
def setups():
    """Per case, built once and left unchanged: the device truth (with its support form), the
    coordinates, the fp64 distances and the dense fp64 truth as the kernel stores it."""
    import hicgat
    from hicgat import graph
    cache = {}

    def get(case):
        if case not in cache:
            n, t = _truth_matrix(case)
            tr = hicgat.Truth(torch.tensor(t, device=DEV))
            if tr.support is None:   # tiny graphs are all support: force the form anyway
                tr.support = graph.SupportForm.build(tr, 1.0, max_fraction=1.0)
            assert tr.support is not None and not tr.asymmetric_source
            rp = tr.support.rowptr.cpu().long()
            deg = rp[1:n + 1] - rp[:n]
            if case == "300e":
                assert int((deg == 0).sum()) == 51 and int(deg[7]) == n - 1 - 51
            if case == "300f":
                assert int(deg[7]) == n - 1 and int(deg.min()) >= 1
            c = torch.tensor(np.random.default_rng(n + 1).standard_normal((n, 3)).astype(np.float32), device=DEV)
            cache[case] = (n, tr, c, tr.dense().double().cpu())
        return cache[case]
    return get


def _run(c, tr, kind):
    import hicgat
    cm = c.clone().requires_grad_(True)
    loss, stats = hicgat.ops.fused_dist_loss(cm, tr, kind)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), stats.cpu(), cm.grad.cpu()


def _dense_kernel(c, tr, kind_i):
    import hicgat
    K = hicgat.kernels.default()
    stats = torch.empty(12, dtype=torch.float64, device=DEV)
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    dc = torch.empty_like(c)
    K.fused_loss(c, tr.buf, tr.n, kind_i, 0, -1, stats, loss, dc)
    torch.cuda.synchronize()
    return stats.cpu().numpy(), dc.cpu().numpy()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("case", CASES)
def test_background_form_matches_fp64_and_dense_kernel(setups, case, kind):
    n, tr, c, T64 = setups(case)
    loss, stats, grad = _run(c, tr, kind)
    st, g = stats.numpy(), grad.numpy()
    cd = c.double().cpu().requires_grad_(True)
    D = torch.cdist(cd, cd, compute_mode="donot_use_mm_for_euclid_dist")
    iu = np.triu_indices(n, 1)
    iut = (torch.as_tensor(iu[0]), torch.as_tensor(iu[1]))
    M = n * (n - 1) / 2
    if kind == "contrastive":
        ref = 0.1 * (T64[iut] - D[iut]).abs().mean()
        ref.backward()
        l_ref = float(ref.detach())
        print(f"{case} {kind}: loss {st[10]:.10g} fp64 {l_ref:.10g}")
        assert abs(st[10] - l_ref) <= 1e-6 * l_ref, (st[10], l_ref)
        assert abs(st[7] - 10 * l_ref) <= 1e-6 * 10 * l_ref and np.isnan(st[8]) and st[9] == 0.1
        assert abs(float(loss) - l_ref) <= 1e-6 * l_ref
        scale = float(np.float32(0.1 / M))
        Dd = D.detach()
        near = (Dd - T64).abs() <= 1e-6 * torch.maximum(Dd, T64.abs())
        near.fill_diagonal_(False)
        allow = 2.0 * scale * near.sum(1).double()
        excess = ((grad.double() - cd.grad).abs() - allow[:, None]).clamp_min(0.0)
        worst = float(excess.max()) / max(float(cd.grad.abs().max()), 1e-30)
        print(f"  dcoords excess {worst:.1e} ({int(near.sum()) // 2} near-tie pairs)")
        assert worst <= 1e-5, worst
        return
    mse = torch.nn.functional.mse_loss(D, T64)
    mse.backward()
    m = float(mse.detach())
    sd, gd = _dense_kernel(c, tr, KINDS[kind])
    print(f"{case} {kind}: mse {st[7]:.9g} dense kernel {sd[7]:.9g} fp64 {m:.9g}; "
          f"grad rel fp64 {_rel(g, cd.grad.numpy()):.2e} dense {_rel(g, gd):.2e}")
    assert abs(st[7] - m) <= 1e-5 * m and abs(st[7] - sd[7]) <= 1e-6 * abs(sd[7])
    for k in (0, 6) if kind == "mse" else range(7):
        assert abs(st[k] - sd[k]) <= 1e-6 * max(abs(sd[k]), 1e-30) + 1e-9, (k, st[k], sd[k])
    assert _rel(g, gd) < 1e-5
    assert _rel(g, cd.grad.numpy()) < 1e-5
    if kind == "mse":
        assert abs(float(loss) - m) <= 1e-5 * m
        return
    if n > 2:   # r's cancellation amplifies the fp32 rounding of a few-pair sum
        assert abs(st[8] - sd[8]) < (1e-6 if n >= 100 else 1e-5)
    # the reference's alpha from the fp32 mse, total = mse + alpha (1 - r) as an fp32 sum
    msef = np.float32(st[7])
    alpha = min(1.0, 0.1 + 1.0 / (float(msef) + 1e-6))
    assert abs(st[9] - alpha) <= 1e-12 * alpha
    if n >= 100:
        d, t = D.detach().numpy()[iu], T64.numpy()[iu]
        r64 = float(np.corrcoef(t, d)[0, 1])
        print(f"  r {st[8]:.9g} fp64 {r64:.9g}")
        assert abs(st[8] - r64) <= 1e-5
    if n > 2:
        total = float(msef + np.float32(alpha * (1.0 - st[8])))
        assert abs(st[10] - total) <= 2e-7 * max(1.0, abs(total)) and float(loss) == np.float32(st[10])   # one fp32 ulp


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("case", CASES)
def test_background_form_is_bitwise_reproducible(setups, case, kind):
    n, tr, c, _ = setups(case)
    a, b = _run(c, tr, kind), _run(c, tr, kind)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1][:11].view(torch.int64), b[1][:11].view(torch.int64))   # NaN r compares by bits
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("wide", [False, True], ids=["own-support-launch", "support-in-tile-launch"])
def test_background_tile_ranges_sum_to_whole(setups, case, kind, wide):
    """Bulk tiles split at an arbitrary tile and support rows split at an arbitrary row add up to the
    whole call: moments to fp64 reassociation, dcoords to fp32 rounding.  fp32 dcoords take the
    separate support launch (the one-GPU form), fp64 dcoords the support blocks riding in the tile
    launch (a rank's share of the sharded step)."""
    import hicgat
    from hicgat import _lib
    n, tr, c, _ = setups(case)
    K = hicgat.kernels.default()
    tiles = _lib.load().hicgat_pairdist_num_tiles(n, 1)

    def part(t0, t1, s0, s1):
        stats = torch.zeros(12, dtype=torch.float64, device=DEV)
        loss = torch.zeros((), dtype=torch.float32, device=DEV)
        dc = torch.zeros((n, 3), dtype=torch.float64 if wide else torch.float32, device=DEV)
        K.fused_loss_support_range(c, tr.support, n, KINDS[kind], t0, t1, s0, s1, stats, loss, dc)
        torch.cuda.synchronize()
        return stats[:7].cpu(), dc.double().cpu()

    whole_s, whole_g = part(0, tiles, 0, n)
    cut_t, cut_s = tiles // 2, n // 3
    (s0, g0), (s1, g1) = part(0, cut_t, 0, cut_s), part(cut_t, tiles, cut_s, n)
    assert torch.allclose(s0 + s1, whole_s, rtol=1e-12)
    assert _rel(g0 + g1, whole_g) < 1e-6
    # and the whole range is the public op's result, bit for bit (fp64 dcoords: the fp32 values widened)
    _, st, g = _run(c, tr, kind)
    assert torch.equal(whole_g.float().view(torch.int32), g.view(torch.int32))
    if not wide:
        assert torch.equal(whole_s.view(torch.int64), st[:7].view(torch.int64))

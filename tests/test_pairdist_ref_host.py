"""tests/pairdist_ref.py on the CPU: the explicit fp64 formulas agree with torch's fp64 autograd
through ``torch.cdist(..., compute_mode="donot_use_mm_for_euclid_dist")`` to 1e-12, on every input
set tests/test_gpu_pairdist_edges.py uses -- the sets with coincident points included, where cdist's
backward gives no gradient through d == 0 -- and the contrastive inputs have no accidental near tie
|d - t| <= 1e-6 max(d, |t|): the only pairs whose sign(d - t) an fp32 rounding could decide are the
designed coincident pairs with t == 0, which keeps the contrastive gradient's allowance in the GPU
test at zero everywhere else."""
import numpy as np
import pytest
import torch

import pairdist_ref as R

TOL = 1e-12


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _torch_dist(s):
    c = torch.tensor(s.c, dtype=torch.float64, requires_grad=True)
    return c, torch.cdist(c, c, compute_mode="donot_use_mm_for_euclid_dist")


def _truths(s):
    return [(k, t) for k, t in (("t", s.t), ("tb", s.tb)) if t is not None]


@pytest.fixture(scope="module")
def dists():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = R.dist(R.inputs(name).c)
        return cache[name]
    return get


@pytest.mark.parametrize("name", R.NAMES)
def test_distance_and_coincident_pairs(dists, name):
    s, D = R.inputs(name), dists(name)
    _, Dt = _torch_dist(s)
    assert _rel(D, Dt.detach().numpy()) <= TOL
    assert np.all(np.diagonal(D) == 0.0) and np.array_equal(D, D.T)
    zero = {(int(a), int(b)) for a, b in zip(*np.nonzero(np.triu(D == 0.0, 1)))}
    assert zero == set(s.coincident)      # the designed pairs and no others


@pytest.mark.parametrize("name", [n for n in R.NAMES if R.inputs(n).g is not None])
def test_cdist_backward_matches_autograd(dists, name):
    s, D = R.inputs(name), dists(name)
    c, Dt = _torch_dist(s)
    (Dt * torch.tensor(s.g, dtype=torch.float64)).sum().backward()
    assert torch.isfinite(c.grad).all()
    assert _rel(R.grad_cdist(s.c, s.g, D), c.grad.numpy()) <= TOL


@pytest.mark.parametrize("name", [n for n in R.NAMES if _truths(R.inputs(n))])
def test_losses_and_gradients_match_autograd(dists, name):
    s, D = R.inputs(name), dists(name)
    n = s.n
    iu = np.triu_indices(n, 1)
    iut = (torch.as_tensor(iu[0]), torch.as_tensor(iu[1]))
    for key, t in _truths(s):
        assert np.array_equal(t, t.T)
        T = torch.tensor(t, dtype=torch.float64)
        m = R.moments(D, t)
        c, Dt = _torch_dist(s)
        l = torch.nn.functional.mse_loss(Dt, T)
        l.backward()
        assert torch.isfinite(c.grad).all()
        assert abs(R.mse(m, n) - l.item()) <= TOL * l.item(), key
        assert _rel(R.grad_mse(s.c, t, D), c.grad.numpy()) <= TOL, key
        d, tt = D[iu], t.astype(np.float64)[iu]
        for k, want in enumerate([((d - tt) ** 2).sum(), d.sum(), (d * d).sum(), (d * tt).sum(), tt.sum(),
                                  (tt * tt).sum(), (np.diagonal(t).astype(np.float64) ** 2).sum()]):
            assert abs(m[k] - want) <= TOL * max(abs(want), 1e-300), (key, k)
        r = R.pearson(D, t)
        if s.name.startswith("flat"):
            assert np.isnan(r)             # every d is 0: no variance
        else:
            assert abs(r - float(np.corrcoef(tt, d)[0, 1])) <= 1e-12, key
        c, Dt = _torch_dist(s)
        lc = 0.1 * (T[iut] - Dt[iut]).abs().mean()
        lc.backward()
        assert torch.isfinite(c.grad).all()
        assert abs(R.contrastive(D, t) - lc.item()) <= TOL * lc.item(), key
        assert abs(R.moments(D, t, "contrastive")[0] / (0.5 * n * (n - 1)) * 0.1 - lc.item()) <= TOL * lc.item()
        # autograd scales by the fp64 0.1 / M, the reference by its fp32 rounding (as an fp32 loss does)
        ratio = R.contrastive_scale(n) / (0.1 / (0.5 * n * (n - 1)))
        assert abs(ratio - 1.0) <= 2.0 ** -24
        assert _rel(R.grad_contrastive(s.c, t, D), ratio * c.grad.numpy()) <= TOL, key


# the sets the GPU module runs the contrastive kind on
CONTRASTIVE_SETS = ["glob58", "glob129", "glob300", "glob301", "coin300", "flat129", "flat300"]


@pytest.mark.parametrize("name", CONTRASTIVE_SETS)
def test_no_accidental_near_ties(dists, name):
    s, D = R.inputs(name), dists(name)
    for key, t in _truths(s):
        near = R.near_ties(D, t)
        assert np.array_equal(near, near.T)
        assert int(near.sum()) // 2 == R.designed_zero_ties(s, t), (key, np.argwhere(np.triu(near)))
    if name == "coin300":
        assert R.designed_zero_ties(s, s.t) == 1 and R.designed_zero_ties(s, s.tb) == 1
        assert s.t[5, 6] != 0.0 and s.tb[5, 6] not in (0.0, R.BG) and s.tb[140, 299] == R.BG
    if name.startswith("flat"):
        assert R.designed_zero_ties(s, s.t) == 0 and R.designed_zero_ties(s, s.tb) == 0


@pytest.mark.parametrize("name,t0,t1", [("glob300", 3, 6), ("glob300", 0, 2), ("glob300", 2, 6), ("glob129", 1, 3),
                                        ("coin300", 1, 5)])
@pytest.mark.parametrize("kind", ["combined", "contrastive"])
def test_tile_range_matches_masked_autograd(dists, name, t0, t1, kind):
    s, D = R.inputs(name), dists(name)
    n, nb = s.n, (s.n + R.BT - 1) // R.BT
    # the range's entries from the tile list itself: tile-row I holds tiles (I, I), (I, I + 1), ...
    tiles = [(I, J) for I in range(nb) for J in range(I, nb)]
    assert len(tiles) == R.num_tiles(n) and all(tiles[R.tri_start(I, nb)] == (I, I) for I in range(nb))
    mask = np.zeros((n, n), bool)
    for I, J in tiles[t0:t1]:
        mask[I * R.BT:(I + 1) * R.BT, J * R.BT:(J + 1) * R.BT] = True
    dsel = np.diagonal(mask).copy()
    mask = np.triu(mask, 1)
    m, g = R.tile_range(s.c, s.t, t0, t1, kind, D)
    T = torch.tensor(s.t, dtype=torch.float64)
    Mk = torch.tensor(mask)
    c, Dt = _torch_dist(s)
    if kind == "contrastive":
        part = (Dt - T).abs()[Mk].sum()
        (part * (0.1 / (0.5 * n * (n - 1)))).backward()
        ratio = R.contrastive_scale(n) / (0.1 / (0.5 * n * (n - 1)))
        assert abs(m[0] - part.item()) <= TOL * part.item() and m[6] == 0.0
        assert _rel(g, ratio * c.grad.numpy()) <= TOL
    else:
        part = ((Dt - T) ** 2)[Mk].sum()
        (2.0 * part / (n * n)).backward()
        assert abs(m[0] - part.item()) <= TOL * part.item()
        assert abs(m[6] - float((T.diagonal()[torch.tensor(dsel)] ** 2).sum())) <= TOL
        assert _rel(g, c.grad.numpy()) <= TOL
        d, tt = D[mask], s.t.astype(np.float64)[mask]
        for k, want in zip(range(1, 6), [d.sum(), (d * d).sum(), (d * tt).sum(), tt.sum(), (tt * tt).sum()]):
            assert abs(m[k] - want) <= TOL * abs(want)
    # and complementary ranges add up to the whole
    tiles_n = R.num_tiles(n)
    m0, g0 = R.tile_range(s.c, s.t, 0, t0, kind, D)
    m2, g2 = R.tile_range(s.c, s.t, t1, tiles_n, kind, D)
    whole = R.moments(D, s.t, kind)
    gw = R.grad_contrastive(s.c, s.t, D) if kind == "contrastive" else R.grad_mse(s.c, s.t, D)
    assert np.all(np.abs(m0 + m + m2 - whole) <= TOL * np.maximum(np.abs(whole), 1e-300))
    assert _rel(g0 + g + g2, gw) <= TOL

"""GPU: the fused Spearman / per-step dSCC path (spearman.hip, hicgat.metrics.DsccScorer) against
scipy.stats.spearmanr on the very float32 values the device ranks, 1e-12 absolute (the tolerance of
test_dscc_matches_scipy for the same comparison)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12


def _lib():
    from hicgat import _lib
    return _lib, _lib.lib()


def _tile():
    return _lib()[1].hicgat_rank_tile()


class _Side:
    """hicgat_avg_rank2 of a host float32 vector."""

    def __init__(self, v):
        L, lib = _lib()
        self.m = len(v)
        self.v = torch.tensor(v, device=DEV)
        self.rank2 = torch.empty(self.m, dtype=torch.int32, device=DEV)
        self.stats = torch.empty(4, dtype=torch.float64, device=DEV)
        self.ws = L.workspace(lib.hicgat_rank_workspace_bytes(self.m), DEV)
        L.check(lib.hicgat_avg_rank2(L.ptr(self.v), self.m, L.ptr(self.rank2), L.ptr(self.stats), L.ptr(self.ws),
                                     self.ws.numel(), L.stream(DEV)), "hicgat_avg_rank2")

    def ranks(self):
        return self.rank2.cpu().numpy().view(np.uint32)

    def rho(self, v):
        L, lib = _lib()
        vd = torch.tensor(v, device=DEV)
        out = torch.empty(4, dtype=torch.float64, device=DEV)
        L.check(lib.hicgat_spearman_vs_rank2(L.ptr(vd), L.ptr(self.rank2), L.ptr(self.stats), self.m, L.ptr(out),
                                             L.ptr(self.ws), self.ws.numel(), L.stream(DEV)),
                "hicgat_spearman_vs_rank2")
        return out.cpu().numpy()


def _bits(rng, m):
    """Random finite float32 bit patterns: both signs, every exponent but the top one, denormals."""
    return (rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFF7FFFFF)).view(np.float32)


def _check(truth, pred):
    """Device rho and ranks of (truth, pred) against scipy; returns the device's out[4]."""
    from scipy.stats import rankdata, spearmanr
    ref = spearmanr(truth, pred)[0]
    assert not math.isnan(ref)
    side = _Side(truth)
    assert np.array_equal(side.ranks().astype(np.float64), 2 * rankdata(truth))
    out = side.rho(pred)
    print(f"M={len(truth)} rho {out[0]!r} scipy {ref!r} diff {abs(out[0] - ref):.3e} groups {out[2]:.0f}")
    assert abs(out[0] - ref) < TOL
    assert out[2] == len(np.unique(np.where(pred == 0, np.float32(0), pred).view(np.uint32)))
    assert out[3] == 0
    return out


@pytest.mark.parametrize("where", ["2", "3", "T-1", "T", "T+1", "3T+5"])
def test_vector_random_bits(where):
    T = _tile()
    m = {"2": 2, "3": 3, "T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[where]
    rng = np.random.default_rng(m)
    truth, pred = _bits(rng, m), _bits(rng, m)
    _check(truth, pred)
    # the predicted side's own ranks as well (every digit pass matters for these keys)
    from scipy.stats import rankdata
    assert np.array_equal(_Side(pred).ranks().astype(np.float64), 2 * rankdata(pred))


def _three_values(rng, m):
    return rng.choice(np.array([-2.5, 0.75, 3.0e-41], dtype=np.float32), m)      # one of them a denormal


def _long_run(rng, m, T):
    v = rng.permutation(np.arange(m, dtype=np.float32) - m // 2)
    v[rng.choice(m, 2 * T + 7, replace=False)] = 0.5      # one group of > 2T in the middle of distinct values
    return v


def _zeros(rng, m):
    return rng.choice(np.array([-1.0, -0.0, 0.0, 1.0, 2.0], dtype=np.float32), m)


@pytest.mark.parametrize("kind", ["three_values", "long_run", "signed_zeros"])
@pytest.mark.parametrize("side", ["truth", "pred", "both"])
def test_vector_ties(kind, side):
    T = _tile()
    m = 3 * T + 5
    rng = np.random.default_rng(7)
    make = {"three_values": lambda: _three_values(rng, m), "long_run": lambda: _long_run(rng, m, T),
            "signed_zeros": lambda: _zeros(rng, m)}[kind]
    truth = make() if side in ("truth", "both") else _bits(rng, m)
    pred = make() if side in ("pred", "both") else _bits(rng, m)
    _check(truth, pred)


def test_signed_zeros_tie():
    from scipy.stats import rankdata
    v = np.array([0.0, -0.0, 1.0, -0.0, -1.0, 0.0], dtype=np.float32)
    r = _Side(v).ranks()
    assert np.array_equal(r.astype(np.float64), 2 * rankdata(v))
    assert r[0] == r[1] == r[3] == r[5]


def test_degenerate_inputs_give_nan():
    T = _tile()
    m = T + 3
    rng = np.random.default_rng(1)
    rnd, const = _bits(rng, m), np.full(m, 1.5, dtype=np.float32)
    assert math.isnan(_Side(rnd).rho(const)[0])           # constant predicted side
    assert math.isnan(_Side(const).rho(rnd)[0])           # constant truth
    bad = rnd.copy()
    bad[m // 2] = np.nan
    out = _Side(rnd).rho(bad)
    assert math.isnan(out[0]) and out[3] == 1             # one NaN in the values
    assert math.isnan(_Side(bad).rho(rnd)[0])             # ... or in the truth
    one = np.array([3.0], dtype=np.float32)
    assert math.isnan(_Side(one).rho(one)[0])             # M = 1
    assert not math.isnan(_Side(rnd).rho(rnd)[0])         # and the workspace is clean afterwards


def test_size_limit_is_refused_before_any_launch():
    """M = 2^31: refused through the size query and the argument checks (nothing of that size exists)."""
    L, lib = _lib()
    big = 2 ** 31
    assert lib.hicgat_rank_workspace_bytes(big) == 0
    assert lib.hicgat_rank_workspace_bytes(big - 1) > 0
    small = torch.zeros(64, dtype=torch.float64, device=DEV)
    p = L.ptr(small)
    assert lib.hicgat_avg_rank2(p, big, p, p, p, 512, L.stream(DEV)) == -3
    assert lib.hicgat_spearman_vs_rank2(p, p, p, big, p, p, 512, L.stream(DEV)) == -3
    assert lib.hicgat_dscc_coords(p, 65537, p, p, p, p, 512, L.stream(DEV)) == -3
    assert lib.hicgat_triu_gather(p, 65537, 65537, p, L.stream(DEV)) == -3
    assert b"unsupported" in lib.hicgat_strerror(-3)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the coordinates form

def _problem(n, lattice=False):
    rng = np.random.default_rng(n)
    if lattice:
        c = rng.integers(0, 4, (n, 3)).astype(np.float32)
    else:
        c = rng.standard_normal((n, 3)).astype(np.float32)
    t = rng.random((n, n)).astype(np.float32)
    t = np.triu(t, 1)
    t = t + t.T
    return c, t


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) < TOL


@pytest.mark.parametrize("n,lattice", [(2, False), (3, False), (58, False), (300, False), (200, True)])
def test_coords_form(n, lattice):
    import hicgat
    from scipy.stats import spearmanr
    c_h, t_h = _problem(n, lattice)
    c, t = torch.tensor(c_h, device=DEV), torch.tensor(t_h, device=DEV)
    iu = np.triu_indices(n, 1)
    d = hicgat.ops.pairwise_dist(c).cpu().numpy()
    ref = spearmanr(t_h[iu], d[iu])[0] if n > 2 else float("nan")
    assert math.isnan(ref) == (n == 2)                      # M = 1 is the only NaN case here
    if lattice:
        assert len(np.unique(d[iu])) < 40 and (d[iu] == 0).any()      # many equal distances, duplicate points
    scorer = hicgat.metrics.DsccScorer(t)
    rho = scorer.score(c)
    old = hicgat.metrics.dscc(c, t)
    print(f"N={n} rho {rho!r} scipy {ref!r} metrics.dscc {old!r}")
    assert _same(rho, ref)
    assert _same(rho, old)
    # a strided [:, :N] view of a padded buffer scores like the contiguous copy
    buf = torch.full((n, n + 37), 9.0, device=DEV)
    buf[:, :n] = t
    assert not buf[:, :n].is_contiguous() or n == 0
    rho_v = hicgat.metrics.DsccScorer(buf[:, :n]).score(c)
    assert (math.isnan(rho_v) and math.isnan(rho)) or rho_v == rho
    # reproducible: the same fp64 bits twice
    a = scorer.score_into(c).clone()
    b = scorer.score_into(c).clone()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))


def test_spearman_fused_matches_scipy():
    import hicgat
    from scipy.stats import spearmanr
    rng = np.random.default_rng(3)
    a = rng.standard_normal(5000).astype(np.float32).round(2)
    b = (a + rng.standard_normal(5000)).astype(np.float32).round(1)
    rho = hicgat.metrics.spearman_fused(torch.tensor(a, device=DEV), torch.tensor(b, device=DEV))
    assert abs(rho - spearmanr(a, b)[0]) < TOL


def test_score_into_in_a_captured_step():
    """score_into inside graphs.CapturedStep: each replay, after the coords buffer was overwritten in
    place, equals the eager result bit for bit."""
    import hicgat
    from hicgat.graphs import CapturedStep
    n = 300
    c_h, t_h = _problem(n)
    scorer = hicgat.metrics.DsccScorer(torch.tensor(t_h, device=DEV))
    eager = hicgat.metrics.DsccScorer(torch.tensor(t_h, device=DEV))
    buf = torch.tensor(c_h, device=DEV)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    step = CapturedStep(lambda: scorer.score_into(buf, out), warmup=0)
    rng = np.random.default_rng(11)
    for k in range(3):
        new = torch.tensor((rng.standard_normal((n, 3)) * (k + 1)).astype(np.float32), device=DEV)
        buf.copy_(new)
        got = step().clone()
        want = eager.score_into(new).clone()
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (k, got, want)
        assert abs(float(got[0])) <= 1


# ---------------------------------------------------------------- training with loss="mse+dscc"

MODEL = "GATNetHeadsChanged3LayersLeakyReLUv2"


def _chr19():
    import hicgat
    g = load_golden("graph_chr19_1mb.npz")
    mfx = load_golden("model_GATNetSelectiveResidualsUpdated.npz")
    y = torch.tensor(g["matrix"], device=DEV)
    y.fill_diagonal_(0)
    data = hicgat.Data(x=torch.tensor(mfx["x"], device=DEV), edge_index=hicgat.Adj.from_dense_device(y), y=y)
    return data, hicgat.Truth.from_contacts(y, 0.5)


def _run(data, tr, steps, **kw):
    import hicgat
    torch.manual_seed(0)
    model = hicgat.MODELS[MODEL]().to(DEV)
    _, hist = hicgat.train.train(model, data, tr, steps=steps, **kw)
    return model, hist


def test_train_mse_plus_dscc():
    import hicgat
    from scipy.stats import spearmanr
    data, tr = _chr19()
    K = 5
    m_mse, h_mse = _run(data, tr, K, loss="mse")
    rhos, mses = [], []
    m_cmb, h_cmb = _run(data, tr, K, loss="mse+dscc", alpha=1.0, dscc_history=rhos, mse_history=mses)
    # the gradient is the MSE's: the same parameters, bit for bit
    for (k1, p1), (k2, p2) in zip(m_mse.state_dict().items(), m_cmb.state_dict().items()):
        assert k1 == k2 and torch.equal(p1, p2), k1
    assert mses == h_mse and len(rhos) == K
    # every recorded value = that step's MSE + (1 - scipy rho of that step's coordinates)
    n = tr.n
    iu = np.triu_indices(n, 1)
    t_h = tr.scoring().cpu().numpy()
    for k in range(K):
        model, _ = _run(data, tr, k, loss="mse") if k else (_fresh(), None)
        with torch.no_grad():
            coords = model.get_model(data.x, data.edge_index)
        d = hicgat.ops.pairwise_dist(coords).cpu().numpy()
        ref = spearmanr(t_h[iu], d[iu])[0]
        assert not math.isnan(ref)
        want = h_mse[k] + (1.0 - ref)
        print(f"step {k}: recorded {h_cmb[k]!r} want {want!r} rho {rhos[k]!r} scipy {ref!r}")
        assert abs(h_cmb[k] - want) <= 1e-6 * abs(want)
    # alpha = 0: the mse run's history
    _, h_zero = _run(data, tr, K, loss="mse+dscc", alpha=0.0)
    assert h_zero == h_mse


def _fresh():
    import hicgat
    torch.manual_seed(0)
    return hicgat.MODELS[MODEL]().to(DEV).train()


def test_train_dscc_history_uses_the_scorer():
    """train(dscc_history=...) appends the fused score: equal to metrics.dscc on the first step's
    coordinates within 1e-12."""
    import hicgat
    data, tr = _chr19()
    rhos = []
    _run(data, tr, 3, loss="mse", dscc_history=rhos)
    coords = _fresh().loss(data.x, data.edge_index, tr, "mse")[2].detach()     # what train_step scores
    assert len(rhos) == 3 and abs(rhos[0] - hicgat.metrics.dscc(coords, tr.scoring())) < TOL

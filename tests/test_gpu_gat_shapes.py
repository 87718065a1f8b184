"""GPU parity of ``hicgat.GATConv`` at every (in, out, heads) the reference's models.py instantiates,
against ``oracle.gat.GATConv`` -- the generic aggregation kernels (gat_fwd.hip, gat_bwd.hip; the shape
list of gat_launch.hpp) and the routing around them (ops.gat_conv, the fused tail, the two zoo models).

Tolerances are those of tests/test_gpu_parity.py: outputs rtol 1e-5 / atol 1e-6, gradients 1e-4
relative to the tensor's max magnitude; the long-row test's atol 2e-6; the rows-pass test's 2e-5;
the model tests' 2e-4 for gradients."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (F, C, H) of the zoo, without the flagship's (512, 256, 2) that tests/test_gpu_parity.py covers
SHAPES = [(512, 256, 1), (512, 512, 1), (512, 128, 2), (256, 128, 2), (128, 128, 2), (256, 256, 2), (512, 512, 2),
          (256, 256, 4)]
GRAPHS = [(58, 1.0), (257, 0.02), (600, 0.5)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hicgat  # noqa: F401  (fails loudly if libhicgat.so is missing)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


@functools.lru_cache(maxsize=None)
def _graph(n, p):
    """Random symmetric 0/1 contacts (n = 257: node 5 isolated, its row is the self loop only) and
    their Adj; built once per (n, p) and shared, never written."""
    import hicgat
    rng = np.random.default_rng(n)
    a = (rng.random((n, n)) < p).astype(np.float64)
    a = np.triu(a, 1)
    a = a + a.T
    if n == 257:
        a[5, :] = 0
        a[:, 5] = 0
    adj = hicgat.Adj.from_dense_device(torch.tensor(a, device=DEV))
    return adj, (adj.storage.rowptr(), adj.storage.col())


def _gat_pair(seed, fin, out, heads):
    import hicgat
    from oracle import gat as og
    torch.manual_seed(seed)
    ref = og.GATConv(fin, out, heads=heads)
    torch.manual_seed(seed)
    mine = hicgat.GATConv(fin, out, heads=heads)
    for (k1, v1), (k2, v2) in zip(ref.state_dict().items(), mine.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    with torch.no_grad():
        mine.bias.copy_(torch.randn_like(mine.bias) * 0.1)
        ref.bias.copy_(mine.bias)
    return ref, mine.to(DEV)


# leaky_relu'(e) jumps at e = 0, so an edge whose logit e_ij = a_src[j] + a_dst[i] lies within the fp32
# rounding of the logits can take the other slope on the device: one such edge (|e| = 4.5e-8,
# (256, 128, 2) at n = 600) moved da_dst by 1.9e-2 -- identically in the rows pass and in the
# independent gathering pass -- while every other tensor agreed to 1e-6.  That is the conditioning of
# the problem, not of a kernel, so the gradient checks run on weights whose ORACLE logits keep every
# edge away from the kink: the first seed of a fixed sequence that does.  The margin: two fp32
# evaluations of a logit (a 128- to 512-term dot product of rows that are 128- to 512-term dot products
# themselves) differ by up to ~4e-7 of the largest logit (the bound test_gat_linear_att_matches_torch
# uses is 1e-5; 2.7e-7 .. 4.1e-7 measured), the largest logit here is ~0.3, e is the sum of two:
# 2.4e-7, and the margin is twice that.
KINK_MARGIN = 5e-7


def _min_abs_logit(ref, x, radj):
    from oracle import gat as og
    with torch.no_grad():
        rowptr, col = og.set_diag(*radj)
        h = ref.lin_l(x).view(-1, ref.heads, ref.out_channels)
        a_l, a_r = (h * ref.att_l).sum(-1), (h * ref.att_r).sum(-1)
        rows = torch.repeat_interleave(torch.arange(len(rowptr) - 1), rowptr[1:] - rowptr[:-1])
        return float((a_l[col] + a_r[rows]).abs().min())


def _conditioned_pair(seed, F, C, H, x, radj):
    for t in range(200):
        ref, mine = _gat_pair(seed + 1000 * t, F, C, H)
        if _min_abs_logit(ref, x, radj) > KINK_MARGIN:
            return ref, mine
    raise AssertionError("no seed keeps the logits away from the leaky-relu kink")


def _check_fwd_bwd(F, C, H, n, p, act):
    adj, radj = _graph(n, p)
    D = H * C
    rng = np.random.default_rng(n)
    x = torch.tensor((0.1 * rng.standard_normal((n, F))).astype(np.float32))
    g = torch.tensor(rng.standard_normal((n, D)).astype(np.float32))
    ref, mine = _conditioned_pair(n + H + C, F, C, H, x, radj)
    xr = x.clone().requires_grad_(True)
    out_r = ref(xr, radj)
    if act:
        out_r = torch.relu(out_r)
    (out_r * g).sum().backward()
    xm = x.to(DEV).requires_grad_(True)
    out_m = mine(xm, adj, act=act)
    (out_m * g.to(DEV)).sum().backward()
    np.testing.assert_allclose(out_m.detach().cpu().numpy(), out_r.detach().numpy(), rtol=1e-5, atol=1e-6)
    e = _rel(xm.grad.cpu(), xr.grad)
    assert e < 1e-4, ("x.grad", e)
    for (name, pr), (_, pm) in zip(ref.named_parameters(), mine.named_parameters()):
        e = _rel(pm.grad.cpu(), pr.grad)
        assert e < 1e-4, (name, e)
    return mine, x, adj, out_m


# ---------------------------------------------------------------- 1, 2: against the oracle
@pytest.mark.parametrize("n,p", GRAPHS)
@pytest.mark.parametrize("F,C,H", SHAPES)
def test_gatconv_shapes_forward_backward_match_oracle(F, C, H, n, p):
    """n = 58: a full row shorter than one 64-edge chunk; n = 257: a self-loop-only row; n = 600:
    ~300 neighbours per row (several chunks, a tail that is no multiple of the gather unroll) -- a graph
    that (2, 256) sends to the tiled kernels, so every other shape must be routed around them."""
    _check_fwd_bwd(F, C, H, n, p, None)


@pytest.mark.parametrize("n,p", [(257, 0.02), (600, 0.5)])
@pytest.mark.parametrize("F,C,H", [(128, 128, 4), (128, 1024, 1), (128, 384, 2), (128, 256, 3), (128, 768, 1)])
def test_gatconv_rule_shapes_outside_the_zoo_match_oracle(F, C, H, n, p):
    """The shapes the rule admits beyond the zoo's: four half-wave slices ((4, 128)), one head over four
    slices ((1, 1024)), a slice that spans two heads between slices that do not ((2, 384)), and a head
    count that is no power of two ((3, 256))."""
    _check_fwd_bwd(F, C, H, n, p, "relu" if H == 3 else None)


@pytest.mark.parametrize("n,p", [(257, 0.02), (600, 0.5)])
@pytest.mark.parametrize("F,C,H", [(512, 128, 2), (512, 512, 2)])
def test_gatconv_shapes_fused_relu_matches_oracle(F, C, H, n, p):
    mine, x, adj, out_m = _check_fwd_bwd(F, C, H, n, p, "relu")
    with torch.no_grad():                     # inference form (no out2) gives the same bits
        assert torch.equal(mine(x.to(DEV), adj, act="relu"), out_m.detach())


# ---------------------------------------------------------------- 3: softmax extremes, long rows
@pytest.mark.parametrize("F,C,H", [(512, 128, 2), (256, 256, 4)])
def test_gatconv_shapes_long_rows_and_softmax_extremes(F, C, H):
    import hicgat
    n = 200
    a = np.ones((n, n)) - np.eye(n)
    ref, mine = _gat_pair(5, F, C, H)
    with torch.no_grad():
        ref.att_l.mul_(40.0)
        mine.att_l.copy_(ref.att_l.to(DEV))
    adj = hicgat.Adj.from_dense_device(torch.tensor(a, device=DEV))
    x = torch.tensor((0.1 * np.random.default_rng(0).standard_normal((n, F))).astype(np.float32))
    out_r = ref(x, (adj.storage.rowptr(), adj.storage.col()))
    out_m = mine(x.to(DEV), adj)
    assert torch.isfinite(out_m).all()
    np.testing.assert_allclose(out_m.detach().cpu().numpy(), out_r.detach().numpy(), rtol=1e-5, atol=2e-6)


# ---------------------------------------------------------------- 4, 5: the kernels among themselves
def _kernel_inputs(H, C, n, density, seed):
    import hicgat
    from hicgat import synth
    i, j, c = synth.contact_pairs(n, density=density, seed=seed)
    A = synth.dense_contacts(n, i, j, c, device=DEV)
    adj = hicgat.Adj.from_dense_device(A, keep_host=False)
    D = H * C
    torch.manual_seed(seed)
    t = dict(h=torch.randn(n, D, device=DEV) * 0.1, a_s=torch.randn(n, H, device=DEV),
             a_d=torch.randn(n, H, device=DEV), b=torch.randn(D, device=DEV) * 0.1, g=torch.randn(n, D, device=DEV),
             al=torch.randn(1, H, C, device=DEV), ar=torch.randn(1, H, C, device=DEV))
    return adj, t


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("H,C", [(2, 128), (1, 512), (4, 256), (2, 256)])
def test_shapes_bwd_rows_equals_gather_dst(H, C, act):
    import hicgat
    K = hicgat.kernels.default()
    n, D = 300, H * C
    adj, t = _kernel_inputs(H, C, n, 0.1, 7)
    h, a_s, a_d, b, g = t["h"], t["a_s"], t["a_d"], t["b"], t["g"]
    out, out2, rs = torch.empty(n, D, device=DEV), torch.empty(n, D, device=DEV), torch.empty(n, 4 * H, device=DEV)
    K.agg_fwd_act(adj.rowptr32, adj.col32, 0, n, h, a_s, a_d, b, 0.2, act, out, out2, rs)
    out_plain, rs_plain = torch.empty_like(out), torch.empty_like(rs)
    K.agg_fwd(adj.rowptr32, adj.col32, 0, n, h, a_s, a_d, b, 0.2, out_plain, rs_plain)
    assert torch.equal(out, torch.relu(out_plain) if act else out_plain)
    assert torch.equal(rs[:, :2 * H], rs_plain[:, :2 * H])
    dout = torch.empty_like(g)
    K.agg_bwd_rows(0, n, act, g, out, b, out2, dout, rs)
    dref = torch.where(out_plain > 0, g, torch.zeros_like(g)) if act else g
    if act:
        assert torch.equal(dout, dref)
    K.agg_bwd_dst(adj.rowptr32, adj.col32, 0, n, h, a_s, a_d, dref, 0.2, rs_plain)
    for k in range(2 * H, 4 * H):                                  # delta[H], da_dst[H]
        e = _rel(rs[:, k].cpu(), rs_plain[:, k].cpu())
        assert e < 2e-5, (k, e)


@pytest.mark.parametrize("H,C", [(2, 128), (2, 512), (2, 256)])
def test_shapes_row_ranges_and_determinism(H, C):
    """[0, 100) + [100, 257) launches write the bits of one [0, 257) launch (forward and source
    pass); so does a second identical call."""
    import hicgat
    K = hicgat.kernels.default()
    n, D = 257, H * C
    adj, t = _kernel_inputs(H, C, n, 0.1, 9)
    h, a_s, a_d, b, g = t["h"], t["a_s"], t["a_d"], t["b"], t["g"]
    rp, col = adj.rowptr32, adj.col32

    def fwd(ranges):
        out, out2 = torch.full((n, D), np.nan, device=DEV), torch.full((n, D), np.nan, device=DEV)
        rs = torch.full((n, 4 * H), np.nan, device=DEV)
        for r0, r1 in ranges:
            K.agg_fwd_act(rp, col, r0, r1, h, a_s, a_d, b, 0.2, 1, out, out2, rs)
        return out, out2, rs

    whole, split, again = fwd([(0, n)]), fwd([(0, 100), (100, n)]), fwd([(0, n)])
    for a, s, w in zip(whole, split, again):
        assert not torch.isnan(a).any()
        assert torch.equal(a, s) and torch.equal(a, w)
    out, out2, rs = whole
    dout = torch.empty_like(g)
    K.agg_bwd_rows(0, n, 1, g, out, b, out2, dout, rs)

    def src(ranges):
        dh, da = torch.full((n, D), np.nan, device=DEV), torch.full((n, H), np.nan, device=DEV)
        for r0, r1 in ranges:
            K.agg_bwd_src(rp, col, r0, r1, h, a_s, a_d, rs, dout, t["al"], t["ar"], 0.2, dh, da)
        return dh, da

    whole, split, again = src([(0, n)]), src([(0, 100), (100, n)]), src([(0, n)])
    for a, s, w in zip(whole, split, again):
        assert not torch.isnan(a).any()
        assert torch.equal(a, s) and torch.equal(a, w)


# ---------------------------------------------------------------- 6: the fused-tail trap
def test_other_shape_feeding_the_fused_tail():
    """GATConv(512, 512, heads=1) -> relu -> the flagship's tail at n = FUSED_TAIL_MIN_M rows: the
    one-kernel tail runs, and its fused rows epilogue (which writes (2, 256)-layout row stats) must
    not be taken for this layer."""
    import hicgat
    from hicgat import ops
    from oracle import gat as og
    n = 1024
    assert n == ops.FUSED_TAIL_MIN_M
    adj, radj = _graph(n, 0.02)
    torch.manual_seed(4)
    ref = og.GATNetSelectiveResidualsUpdated()
    ref.conv = og.GATConv(512, 512, heads=1)
    torch.manual_seed(4)
    mine = hicgat.GATNetSelectiveResidualsUpdated()
    mine.conv = hicgat.GATConv(512, 512, heads=1)
    with torch.no_grad():
        ref.conv.bias.copy_(torch.randn_like(ref.conv.bias) * 0.1)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(DEV)
    rng = np.random.default_rng(1)
    x = torch.tensor((0.1 * rng.standard_normal((n, 512))).astype(np.float32))
    g = torch.tensor(rng.standard_normal((n, 3)).astype(np.float32))
    xd = x.to(DEV)
    assert ops.fused_tail_ok(mine, xd)
    c_ref = ref.get_model(x, radj)
    (c_ref * g).sum().backward()
    c = mine.get_model(xd, adj)
    (c * g.to(DEV)).sum().backward()
    np.testing.assert_allclose(c.detach().cpu().numpy(), c_ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    for (k, p), pr in zip(mine.named_parameters(), ref.parameters()):
        e = _rel(p.grad.cpu(), pr.grad)
        assert e < 2e-4, (k, e)


# ---------------------------------------------------------------- 7: the two models
class _RefHeadsChangedLeakyReLU(torch.nn.Module):
    """models.py:181-222 over the oracle's GATConv."""

    def __init__(self):
        from oracle import gat as og
        super().__init__()
        self.conv = og.GATConv(512, 128, heads=2, concat=True)
        self.densea = torch.nn.Linear(256, 128)
        self.dense1 = torch.nn.Linear(128, 64)
        self.dense2 = torch.nn.Linear(64, 32)
        self.dense3 = torch.nn.Linear(32, 3)
        self.leaky_relu = torch.nn.LeakyReLU()

    def get_model(self, x, adj):
        x = self.leaky_relu(self.conv(x, adj))
        x = self.leaky_relu(self.densea(x))
        x = self.leaky_relu(self.dense1(x))
        x = self.leaky_relu(self.dense2(x))
        return self.dense3(x)


class _RefReduced(torch.nn.Module):
    """models.py:1414-1459 over the oracle's GATConv (get_model: no dropout)."""

    def __init__(self):
        from oracle import gat as og
        super().__init__()
        self.conv = og.GATConv(512, 512, heads=2, concat=True)
        self.densea = torch.nn.Linear(1024, 256)
        self.dense1 = torch.nn.Linear(256, 64)
        self.dense2 = torch.nn.Linear(64, 3)
        self.dropout = torch.nn.Dropout(p=0.4)

    def get_model(self, x, adj):
        x = self.conv(x, adj).relu()
        x = self.densea(x).relu()
        x = self.dense1(x).relu()
        return self.dense2(x)


@functools.lru_cache(maxsize=None)
def _model_problem():
    """n = 130, p = 0.3 weighted contacts, features, and the oracle's graph / truth of them."""
    from oracle import graph as ogr
    n = 130
    rng = np.random.default_rng(130)
    a = (rng.random((n, n)) < 0.3) * rng.integers(1, 100, (n, n)).astype(np.float64)
    a = np.triu(a, 1)
    a = a + a.T
    x = (0.1 * rng.standard_normal((n, 512))).astype(np.float32)
    d = ogr.load_input(a.copy(), x)
    t_ref = ogr.cont2dist(d["y"], 0.5)
    return a, x, d, t_ref


def _device_problem():
    import hicgat
    a, x, _, _ = _model_problem()
    y = torch.tensor(a, device=DEV)
    return hicgat.Adj.from_dense_device(y), hicgat.Truth.from_contacts(y, 0.5), torch.tensor(x, device=DEV), y


def test_heads_changed_leaky_relu_matches_oracle():
    import hicgat
    from oracle import gat as og
    _, _, d, t_ref = _model_problem()
    adj, truth, x, _ = _device_problem()
    torch.manual_seed(2)
    ref = _RefHeadsChangedLeakyReLU()
    torch.manual_seed(2)
    model = hicgat.MODELS["GATNetHeadsChangedLeakyReLU"]().to(DEV)
    radj = (torch.tensor(d["rowptr"]), torch.tensor(d["col"]))
    assert torch.equal(truth.dense().cpu(), t_ref.float())
    og.CDIST_MODE = "donot_use_mm_for_euclid_dist"
    try:
        c_ref = ref.get_model(d["x"], radj)
        l_ref = torch.nn.functional.mse_loss(torch.cdist(c_ref, c_ref, compute_mode=og.CDIST_MODE).float(),
                                             t_ref.float())
        l_ref.backward()
    finally:
        og.CDIST_MODE = "use_mm_for_euclid_dist_if_necessary"
    coords = model.get_model(x, adj)
    np.testing.assert_allclose(coords.detach().cpu().numpy(), c_ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    loss, _, _ = model.loss(x, adj, truth, "mse")
    loss.backward()
    assert abs(loss.item() - l_ref.item()) <= 1e-5 * l_ref.item()
    gscale = max(pr.grad.abs().max().item() for pr in ref.parameters())
    for (k, p), pr in zip(model.named_parameters(), ref.parameters()):
        if pr.grad.abs().max().item() < 1e-3 * gscale:
            # zero in exact arithmetic (the last bias, by translation invariance): fp32 noise on both sides
            assert p.grad.abs().max().item() < 1e-3 * gscale, k
            continue
        e = _rel(p.grad.cpu(), pr.grad)
        assert e < 2e-4, (k, e)


def test_reduced_eval_matches_oracle():
    import hicgat
    _, _, d, _ = _model_problem()
    adj, truth, x, _ = _device_problem()
    torch.manual_seed(3)
    ref = _RefReduced().eval()
    torch.manual_seed(3)
    model = hicgat.MODELS["GATNetReduced"]().to(DEV).eval()
    radj = (torch.tensor(d["rowptr"]), torch.tensor(d["col"]))
    with torch.no_grad():
        c_ref = ref.get_model(d["x"], radj)
        coords = model.get_model(x, adj)
        dist = model(x, adj)
    np.testing.assert_allclose(coords.cpu().numpy(), c_ref.numpy(), rtol=1e-5, atol=1e-6)
    c64 = c_ref.double()
    d_exact = torch.cdist(c64, c64, compute_mode="donot_use_mm_for_euclid_dist")
    np.testing.assert_allclose(dist.cpu().numpy(), d_exact.numpy(), rtol=1e-5, atol=1e-6)
    with pytest.raises(NotImplementedError):
        model.train().loss(x, adj, truth)


def test_heads_changed_graph_replay_equals_eager_steps():
    """hicgat.train's loop with the model ``--model GATNetHeadsChangedLeakyReLU`` selects: the two eager
    warm-up steps and three replays of the captured step give the bits of five eager steps."""
    import hicgat
    adj, truth, x, y = _device_problem()
    data = hicgat.Data(x=x, edge_index=adj, y=y)
    steps = hicgat.train.GRAPH_WARMUP + 3
    res = []
    for graphed in (False, True):
        torch.manual_seed(0)
        model = hicgat.MODELS["GATNetHeadsChangedLeakyReLU"]().to(DEV)
        opt, hist = hicgat.train.train(model, data, truth, steps=steps, graph=graphed)
        res.append((hist, opt.flat.clone()))
    (he, pe), (hg, pg) = res
    assert len(he) == steps and he == hg
    assert torch.equal(pe, pg)


# ---------------------------------------------------------------- 8: outside the rule
def test_unsupported_shape_raises_before_any_launch(monkeypatch):
    import hicgat
    adj, _ = _graph(58, 1.0)
    conv = hicgat.GATConv(512, 96, heads=2).to(DEV)
    x = torch.zeros(58, 512, device=DEV)

    def no_kernels():
        raise AssertionError("a kernel interface was asked for")

    monkeypatch.setattr(hicgat.kernels, "default", no_kernels)
    with pytest.raises(NotImplementedError, match="out_channels % 128"):
        conv(x, adj)

"""GPU: feature dropout (dropout.hip) against the mask's definition (tests/philox_ref.py) and torch --
mask bits, forward and backward values bit for bit, the refusals, a training step of three of the
dropout models against the oracle, the models' mode semantics and the captured step."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import philox_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 4), (37, 64), (5, 1024), (130, 256), (257, 512)]
SEEDS = (0x1234, (1 << 32) + 5)
NONE, RELU, LEAKY = 0, 1, 2   # include/hicgat.h HICGAT_ACT_*
SLOPE = 0.01


def _ref_mask(rows, W, p, seed, step, site, row_offset=0):
    return torch.from_numpy(philox_ref.keep_mask(rows, W, p, seed, step, site, row_offset))


def _act(x, act):
    return x if act == NONE else F.relu(x) if act == RELU else F.leaky_relu(x, SLOPE)


def _ref_y(x, act, p, mask):
    """where(mask, act(x), 0) * scale in torch fp32 on the CPU."""
    return torch.where(mask, _act(x, act), torch.zeros((), dtype=x.dtype)) * torch.tensor(philox_ref.scale(p))


def _normal(M, W, seed, nonzero=False):
    x = torch.randn(M, W, generator=torch.Generator().manual_seed(seed))
    return torch.where(x == 0, torch.ones_like(x), x) if nonzero else x


# ---------------------------------------------------------------- 1: mask bits
@pytest.mark.parametrize("M,W", SHAPES)
def test_mask_bits_equal_the_definition(M, W):
    from hicgat import ops
    for seed in SEEDS:
        for step in (1, (1 << 32) + 1):
            for site in (0, 2):
                got = ops.dropout_mask(M, W, 0.4, seed, step, site).cpu()
                assert got.dtype == torch.bool
                assert torch.equal(got, _ref_mask(M, W, 0.4, seed, step, site)), (seed, step, site)
    assert torch.equal(ops.dropout_mask(M, W, 0.4, SEEDS[0], 1, 0), ops.dropout_mask(M, W, 0.4, SEEDS[0], (1 << 32) + 1, 0))
    assert ops.dropout_mask(M, W, 0.0, SEEDS[0], 1, 0).all()


@pytest.mark.parametrize("row_offset", [0, (1 << 24) - 1, (1 << 24) + 3])
def test_mask_bits_where_the_quad_index_passes_2_32(row_offset):
    """W = 1024: 256 quads per row, so the quad index g reaches 2^32 at row 2^24."""
    from hicgat import ops
    got = ops.dropout_mask(3, 1024, 0.3, SEEDS[1], 1, 0, row_offset=row_offset).cpu()
    assert torch.equal(got, _ref_mask(3, 1024, 0.3, SEEDS[1], 1, 0, row_offset))


def test_mask_of_a_row_range_is_that_range_of_the_whole_mask():
    from hicgat import ops
    whole = ops.dropout_mask(130, 256, 0.4, SEEDS[0], 1, 0)
    part = ops.dropout_mask(90, 256, 0.4, SEEDS[0], 1, 0, row_offset=40)
    assert torch.equal(whole[40:], part)
    assert torch.equal(part.cpu(), _ref_mask(130, 256, 0.4, SEEDS[0], 1, 0)[40:])


# ---------------------------------------------------------------- 2: forward values
@pytest.mark.parametrize("M,W", SHAPES)
def test_forward_values(M, W):
    from hicgat import kernels
    K = kernels.default()
    x = _normal(M, W, 7)
    x[0, :2] = 0.0
    xd = x.to(DEV)
    for act in (NONE, RELU, LEAKY):
        for p in (0.0, 0.1, 0.4):
            y = K.act_dropout_fwd(xd, act, SLOPE, p, SEEDS[1], None, 3, 1, 0, torch.empty_like(xd))
            want = _ref_y(x, act, p, _ref_mask(M, W, p, SEEDS[1], 3, 1))
            assert torch.equal(y.cpu(), want), (act, p)
            if p == 0.0:
                assert torch.equal(y.cpu(), _act(x, act))


def test_forward_strided_in_place_and_device_step():
    from hicgat import kernels
    K = kernels.default()
    wide = _normal(37, 96, 8)
    x = wide[:, 16:80]
    want = _ref_y(x, RELU, 0.4, _ref_mask(37, 64, 0.4, SEEDS[0], 7, 2, 11))
    wd = wide.to(DEV)
    xd = wd[:, 16:80]
    assert xd.stride(0) == 96
    y = K.act_dropout_fwd(xd, RELU, SLOPE, 0.4, SEEDS[0], None, 7, 2, 11, torch.empty((37, 64), device=DEV))
    assert torch.equal(y.cpu(), want)
    ctr = torch.tensor([7], dtype=torch.int64, device=DEV)
    y2 = K.act_dropout_fwd(xd, RELU, SLOPE, 0.4, SEEDS[0], ctr, 12345, 2, 11, torch.empty((37, 64), device=DEV))
    assert torch.equal(y2, y)                      # the device count wins over step_value
    K.act_dropout_fwd(xd, RELU, SLOPE, 0.4, SEEDS[0], ctr, 0, 2, 11, xd)      # in place, through the strided view
    assert torch.equal(xd.cpu(), want)
    assert torch.equal(wd[:, :16].cpu(), wide[:, :16]) and torch.equal(wd[:, 80:].cpu(), wide[:, 80:])


# ---------------------------------------------------------------- 3: backward values
@pytest.mark.parametrize("M,W", SHAPES)
@pytest.mark.parametrize("act", [RELU, LEAKY])
def test_backward_values(M, W, act):
    from hicgat import kernels
    K = kernels.default()
    p = 0.4
    x = _normal(M, W, 9, nonzero=True).requires_grad_()
    dy = _normal(M, W, 10)
    yr = _ref_y(x, act, p, _ref_mask(M, W, p, SEEDS[0], 1, 0))
    yr.backward(dy)
    y = K.act_dropout_fwd(x.detach().to(DEV), act, SLOPE, p, SEEDS[0], None, 1, 0, 0, torch.empty((M, W), device=DEV))
    assert torch.equal(y.cpu(), yr.detach())
    dyd = dy.to(DEV)
    dx = K.act_dropout_bwd(dyd, y, act, SLOPE, p, torch.empty_like(y))
    assert torch.equal(dx.cpu(), x.grad)
    if (M, W) == (130, 256):
        K.act_dropout_bwd(dyd, y, act, SLOPE, p, dyd)        # dx aliases dy
        assert torch.equal(dyd.cpu(), x.grad)


@pytest.mark.parametrize("act", ["relu", "leaky_relu"])
def test_autograd_function_saves_the_output_and_matches_torch(act):
    import hicgat
    M, W, p = 130, 256, 0.3
    st = hicgat.DropoutState(DEV, seed=SEEDS[1])
    st.advance()
    st.advance()
    assert st.step == 2
    x = _normal(M, W, 11, nonzero=True).requires_grad_()
    dy = _normal(M, W, 12)
    code = RELU if act == "relu" else LEAKY
    yr = _ref_y(x, code, p, _ref_mask(M, W, p, SEEDS[1], 2, 1, 5))
    yr.backward(dy)
    xd = x.detach().to(DEV).requires_grad_()
    y = hicgat.ops.act_dropout(xd, act, p, st, site=1, row_offset=5)
    assert [t.data_ptr() for t in y.grad_fn.saved_tensors] == [y.data_ptr()]
    y.backward(dy.to(DEV))
    assert torch.equal(y.detach().cpu(), yr.detach()) and torch.equal(xd.grad.cpu(), x.grad)


# ---------------------------------------------------------------- 4: refusals
def test_refusals_come_before_any_launch():
    from hicgat import _lib
    lib = _lib.lib()
    st = _lib.stream(torch.device(DEV))
    x = torch.randn(4, 8, device=DEV)
    y = torch.full((4, 8), 7.0, device=DEV)
    m = torch.full((4, 8), 7, dtype=torch.uint8, device=DEV)
    P = _lib.ptr
    off = ctypes.c_void_p(x.data_ptr() + 4)
    EINVAL, EUNSUPPORTED = -1, -3
    assert lib.hicgat_act_dropout_fwd(P(x), 8, 4, 6, RELU, 0.0, 0.3, 1, None, 1, 0, 0, P(y), 8, st) == EUNSUPPORTED
    assert lib.hicgat_act_dropout_fwd(P(x), 6, 4, 4, RELU, 0.0, 0.3, 1, None, 1, 0, 0, P(y), 8, st) == EUNSUPPORTED
    assert lib.hicgat_act_dropout_fwd(off, 8, 4, 4, RELU, 0.0, 0.3, 1, None, 1, 0, 0, P(y), 8, st) == EINVAL
    assert lib.hicgat_act_dropout_fwd(P(x), 8, 4, 8, RELU, 0.0, 1.0, 1, None, 1, 0, 0, P(y), 8, st) == EINVAL
    assert lib.hicgat_act_dropout_fwd(P(x), 8, 4, 8, 3, 0.0, 0.3, 1, None, 1, 0, 0, P(y), 8, st) == EINVAL
    assert lib.hicgat_act_dropout_bwd(P(x), 8, P(x), 8, 4, 8, NONE, 0.0, 0.3, P(y), 8, st) == EUNSUPPORTED
    assert lib.hicgat_act_dropout_bwd(P(x), 8, P(x), 8, 4, 6, RELU, 0.0, 0.3, P(y), 8, st) == EUNSUPPORTED
    assert lib.hicgat_act_dropout_bwd(off, 8, P(x), 8, 4, 4, RELU, 0.0, 0.3, P(y), 8, st) == EINVAL
    assert lib.hicgat_act_dropout_bwd(P(x), 8, P(x), 8, 4, 8, LEAKY, 0.0, 0.3, P(y), 8, st) == EINVAL
    assert lib.hicgat_dropout_mask(P(m), 4, 6, 0.3, 1, None, 1, 0, 0, st) == EUNSUPPORTED
    assert lib.hicgat_dropout_mask(P(m), 4, 8, -0.5, 1, None, 1, 0, 0, st) == EINVAL
    assert lib.hicgat_dropout_advance(None, st) == EINVAL
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (m == 7).all()


# ---------------------------------------------------------------- 5: a model step against the oracle
class _RefDropoutModel(torch.nn.Module):
    """A reference dropout model (models.py) over the oracle's GATConv, submodules in its order;
    ``forward_train`` is its training ``forward`` before the cdist, with the masks given."""

    def __init__(self, conv, widths, act, p, sites):
        from oracle import gat as og
        super().__init__()
        self.conv = og.GATConv(*conv[:2], heads=conv[2], concat=True)
        for k, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
            setattr(self, "densea" if k == 0 else f"dense{k}", torch.nn.Linear(a, b))
        self.dropout = torch.nn.Dropout(p=p)
        self.act_code, self.sites = act, sites

    def layers(self):
        return [m for m in self.children() if isinstance(m, torch.nn.Linear)]

    def forward_train(self, x, adj, masks, pre=None):
        """``masks[k]``: the keep mask of site k; ``pre``: a list that receives (activation input,
        elements that count) per activation."""
        scale = float(philox_ref.scale(self.dropout.p))
        h = self.conv(x, adj)
        for k, lin in enumerate(self.layers()):
            if pre is not None:
                pre.append((h.detach(), masks[k] if k < self.sites else torch.ones_like(h, dtype=torch.bool)))
            h = _act(h, self.act_code)
            if k < self.sites:
                h = h * masks[k].to(h.dtype) * scale
            h = lin(h)
        return h


REF_MODELS = {   # models.py:1461-1494, :971-1007, :60-98, :1365-1411
    "GATNetMoreReduced": dict(conv=(512, 256, 2), widths=(512, 128, 32, 3), act=RELU, p=0.4, sites=2),
    "GATNetHeadsChanged3LayersLeakyReLU": dict(conv=(512, 256, 2), widths=(512, 256, 128, 3), act=LEAKY, p=0.3, sites=2),
    "GATNet": dict(conv=(512, 512, 1), widths=(512, 256, 128, 64, 3), act=RELU, p=0.3, sites=3),
    "GATNetHeadsChanged4LayerEmbedding512Dense": dict(conv=(512, 256, 2), widths=(512, 256, 128, 64, 32, 3), act=RELU,
                                                      p=0.3, sites=2),
}


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


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _masks(cfg, n, seed, step):
    return [_ref_mask(n, cfg["widths"][k], cfg["p"], seed, step, k) for k in range(cfg["sites"])]


def _seeded_reference(name, x, radj):
    """The first model seed of 0..7 whose float64 training forward keeps every activation input that
    counts (every element of a plain activation, the kept ones of a dropout site) farther than 1e-6 of
    its layer's largest from the activation's kink at 0: there the fp32 device value and the fp32
    oracle value are on the same branch, so the gradients are comparable.  The seed is also the
    masks' seed (the model's DropoutState reads torch.initial_seed())."""
    cfg = REF_MODELS[name]
    for seed in range(8):
        torch.manual_seed(seed)
        ref = _RefDropoutModel(**cfg)
        masks = _masks(cfg, x.shape[0], seed, 1)
        pre = []
        with torch.no_grad():
            copy.deepcopy(ref).double().forward_train(x.double(), radj, masks, pre)
        if all((h[m].abs() > 1e-6 * h.abs().max()).all() for h, m in pre):
            return seed, ref, masks
    raise AssertionError(f"{name}: no seed of 0..7 keeps the activation inputs away from 0")


@pytest.mark.parametrize("name", ["GATNetMoreReduced", "GATNetHeadsChanged3LayersLeakyReLU", "GATNet"])
def test_training_step_matches_oracle(name):
    import hicgat
    from oracle import gat as og
    _, _, d, t_ref = _model_problem()
    adj, truth, x, _ = _device_problem()
    radj = (torch.tensor(d["rowptr"]), torch.tensor(d["col"]))
    seed, ref, masks = _seeded_reference(name, d["x"], radj)
    torch.manual_seed(seed)
    model = hicgat.MODELS[name]().to(DEV)
    assert model.training
    og.CDIST_MODE = "donot_use_mm_for_euclid_dist"
    try:
        c_ref = ref.forward_train(d["x"], radj, masks)
        l_ref = F.mse_loss(torch.cdist(c_ref, c_ref, compute_mode=og.CDIST_MODE).float(), t_ref.float())
        l_ref.backward()
    finally:
        og.CDIST_MODE = "use_mm_for_euclid_dist_if_necessary"
    loss, _, coords = model.loss(x, adj, truth, "mse")
    loss.backward()
    st = model.dropout_state(x.device)
    assert st.seed == seed and st.step == 1 and st.p == REF_MODELS[name]["p"]
    np.testing.assert_allclose(coords.detach().cpu().numpy(), c_ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert abs(loss.item() - l_ref.item()) <= 1e-5 * l_ref.item()
    gscale = max(pr.grad.abs().max().item() for pr in ref.parameters())
    for (k, p), pr in zip(model.named_parameters(), ref.parameters()):
        if pr.grad.abs().max().item() < 1e-3 * gscale:
            # zero in exact arithmetic (the last bias, by translation invariance): fp32 noise on both sides
            assert p.grad.abs().max().item() < 1e-3 * gscale, k
            continue
        e = _rel(p.grad.cpu(), pr.grad)
        assert e < 2e-4, (k, e)


# ---------------------------------------------------------------- 6: mode semantics
def test_mode_semantics():
    import hicgat
    adj, truth, x, _ = _device_problem()
    torch.manual_seed(4)
    model = hicgat.GATNetMoreReduced().to(DEV)
    with torch.no_grad():
        c_train_mode = model.train().get_model(x, adj)
        assert getattr(model, "_dropout_state", None) is None         # get_model never drops
        c_eval = model.eval().get_model(x, adj)
        assert torch.equal(c_train_mode, c_eval)
        l_eval, _, ce = model.loss(x, adj, truth)
        assert torch.equal(ce, c_eval)
        d_eval = model(x, adj)
        model.train()
        l1, _, c1 = model.loss(x, adj, truth)
        st = model.dropout_state(x.device)
        assert st.step == 1 and st.seed == 4
        l2, _, c2 = model.loss(x, adj, truth)
        assert st.step == 2
        assert l1.item() != l_eval.item() and not torch.equal(c1, c_eval)
        assert not torch.equal(c1, c2)
        d_train = model(x, adj)                                        # forward() drops too
        assert st.step == 3 and not torch.equal(d_train, d_eval)
        model.eval()
        model.loss(x, adj, truth)
        model(x, adj)
        assert st.step == 3                                            # eval forwards do not count
        model.train()
        st.reset(step=0)
        assert st.step == 0
        l1b, _, c1b = model.loss(x, adj, truth)
        assert torch.equal(c1b, c1) and torch.equal(l1b, l1) and st.step == 1
        st.reset(seed=5, step=0)
        assert not torch.equal(model.loss(x, adj, truth)[2], c1)


# ---------------------------------------------------------------- 7: the captured step
@pytest.mark.parametrize("name", ["GATNetHeadsChanged4LayerEmbedding512Dense", "GATNetHeadsChanged3LayersLeakyReLU"])
def test_graph_replay_equals_eager_steps(name):
    """hicgat.train's loop: the eager warm-up steps and three replays of the captured step give the
    bits of as many eager steps -- the replays advance the dropout count on the device -- and they
    are not the bits of the same model trained without dropout."""
    import hicgat
    adj, truth, x, y = _device_problem()
    data = hicgat.Data(x=x, edge_index=adj, y=y)
    steps = hicgat.train.GRAPH_WARMUP + 3
    res = []
    for graphed, p in ((False, None), (True, None), (False, 0.0)):
        torch.manual_seed(0)
        model = hicgat.MODELS[name]().to(DEV)
        st = model.dropout_state(x.device)
        if p is not None:
            st.p = p
        opt, hist = hicgat.train.train(model, data, truth, steps=steps, graph=graphed)
        assert st is model.dropout_state(x.device) and st.step == steps
        res.append((hist, opt.flat.clone()))
    (he, pe), (hg, pg), (h0, _) = res
    assert len(he) == steps and he == hg
    assert torch.equal(pe, pg)
    assert he != h0 and he[0] != h0[0]

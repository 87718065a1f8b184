"""GPU: BatchNorm1d -> act -> Dropout (batchnorm.hip) against torch's own BatchNorm1d in float64 on the
CPU composed with the mask's definition (tests/philox_ref.py) -- values, gradients and buffers, the
variance without cancellation, bitwise determinism and graph replay, the C ABI's refusals, a training
step of both BatchNorm models against the reference composite over the oracle's GATConv, their mode
semantics and the captured training loop."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn import BatchNorm1d

import philox_ref
from test_batchnorm_host import NAMES, ref_model

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(2, 64), (37, 64), (63, 128), (65, 128), (130, 256), (257, 256), (4097, 64), (300, 1024)]
CASES = [(None, 0.0), ("relu", 0.0), ("relu", 0.4), ("leaky_relu", 0.0), ("leaky_relu", 0.4)]
SEED, STEP, SITE, ROW0 = (1 << 32) + 5, 3, 1, 5
SLOPE = 0.01


def _act(x, act):
    return x if act is None else F.relu(x) if act == "relu" else F.leaky_relu(x, SLOPE)


def _rel(a, b):
    """max |a - b| over max |b| (float64)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _module(W, g):
    """A BatchNorm1d(W) with non-trivial parameters and running buffers."""
    bn = BatchNorm1d(W)
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(W, generator=g))
        bn.bias.copy_(0.3 * torch.randn(W, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(W, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(W, generator=g))
    return bn


@functools.lru_cache(maxsize=None)
def _mask(M, W, p):
    if p == 0.0:
        return torch.ones(M, W, dtype=torch.bool)
    return torch.from_numpy(philox_ref.keep_mask(M, W, p, SEED, STEP, SITE, ROW0))


def _ref(bn, y, dz, act, p, mask, training):
    """torch in float64 on the fp32 inputs: (z, dy, dgamma, dbeta, pre-activation, the module)."""
    r = copy.deepcopy(bn).double().train(training)
    y64 = y.double().requires_grad_()
    pre = r(y64)
    z = _act(pre, act) * mask.double() * float(philox_ref.scale(p))
    z.backward(dz.double())
    return z.detach(), y64.grad, r.weight.grad, r.bias.grad, pre.detach(), r


@functools.lru_cache(maxsize=None)
def _drawn(M, W, act, p, training):
    """Inputs of the first seed of 0..7 that keeps every pre-activation that counts (the kept ones)
    farther than 1e-6 of the layer's largest from the activation's kink, with the float64 reference.
    A tensor of 3e5 elements has a few that close under every seed: those inputs are moved by 0.01
    (a few rounds: in training mode that moves the statistics a little) before the seed is judged."""
    mask = _mask(M, W, p)
    for seed in range(8):
        g = torch.Generator().manual_seed(1000 * seed + M + W)
        bn = _module(W, g)
        y = torch.randn(M, W, generator=g) * 1.5 + 0.5
        dz = torch.randn(M, W, generator=g)
        for _ in range(4):
            ref = _ref(bn, y, dz, act, p, mask, training)
            pre = ref[4]
            near = mask & (pre.abs() <= 1e-6 * pre.abs().max())
            if act is None or not near.any():
                return bn, y, dz, ref
            y = torch.where(near, y + 0.01, y)
    raise AssertionError("no seed of 0..7 keeps the pre-activations away from 0")


def _state(p):
    import hicgat
    if p == 0.0:
        return None
    st = hicgat.DropoutState(DEV, seed=SEED, p=p)
    st.reset(step=STEP)
    return st


def _run(bn, y, dz, act, p, training, view=None):
    """The op on the device: (z, dy, dgamma, dbeta, the device module)."""
    import hicgat
    d = copy.deepcopy(bn).to(DEV).train(training)
    yd = (y.to(DEV) if view is None else view).requires_grad_()
    st = _state(p)
    z = hicgat.ops.bn_act_dropout(yd, d, act, st, SITE if st is not None else None, ROW0)
    z.backward(dz.to(DEV))
    return z.detach(), yd.grad, d.weight.grad, d.bias.grad, d


# ---------------------------------------------------------------- 1: values, gradients, buffers
@pytest.mark.parametrize("M,W", SHAPES)
@pytest.mark.parametrize("act,p", CASES)
def test_training_mode_against_torch(M, W, act, p):
    """(2, 64) is the hard case for dy: with two rows dy = gamma rstd h (1 - a^2), a^2 = d^2 / (d^2 + eps),
    so the three terms of g - dbeta / M - yhat dgamma / M cancel to eps / (d^2 + eps) ~ 0.02 of their
    size in the column that sets the tensor's max.  An fp32 yhat, rstd and column sums left dy at
    1.2e-5 ... 2.6e-5 there; the backward therefore forms them in fp64 (batchnorm.hip)."""
    bn, y, dz, ref = _drawn(M, W, act, p, True)
    got = _run(bn, y, dz, act, p, True)
    for name, a, b in zip(("z", "dy", "dgamma", "dbeta"), got, ref):
        e = _rel(a, b)
        print(f"({M}, {W}) {act} p={p} {name}: {e:.2e}")
        assert e <= 1e-5, (name, e)
    d, r = got[4], ref[5]
    assert _rel(d.running_mean, r.running_mean) <= 1e-6 and _rel(d.running_var, r.running_var) <= 1e-6
    assert d.num_batches_tracked.item() == 1 and d.num_batches_tracked.dtype == torch.int64


@pytest.mark.parametrize("M,W", SHAPES)
def test_buffers_after_three_forwards_with_and_without_grad(M, W):
    import hicgat
    bn, y, _, _ = _drawn(M, W, "leaky_relu", 0.0, True)
    d, r = copy.deepcopy(bn).to(DEV), copy.deepcopy(bn).double()
    ys = [y, 0.5 * y + 1.0, y.flip(0) * 2.0]
    for k, v in enumerate(ys):
        r(v.double())
        with torch.no_grad() if k == 1 else torch.enable_grad():
            hicgat.ops.bn_act_dropout(v.to(DEV), d, "leaky_relu")
    assert _rel(d.running_mean, r.running_mean) <= 1e-6 and _rel(d.running_var, r.running_var) <= 1e-6
    assert d.num_batches_tracked.item() == 3 == r.num_batches_tracked.item()


@pytest.mark.parametrize("M,W", SHAPES + [(1, 64)])
@pytest.mark.parametrize("act,p", CASES)
def test_eval_mode_against_torch_and_buffers_untouched(M, W, act, p):
    bn, y, dz, ref = _drawn(M, W, act, p, False)
    got = _run(bn, y, dz, act, p, False)
    for name, a, b in zip(("z", "dy", "dgamma", "dbeta"), got, ref):
        e = _rel(a, b)
        print(f"eval ({M}, {W}) {act} p={p} {name}: {e:.2e}")
        assert e <= 1e-5, (name, e)
    d = got[4]
    assert torch.equal(d.running_mean.cpu(), bn.running_mean) and torch.equal(d.running_var.cpu(), bn.running_var)
    assert d.num_batches_tracked.item() == 0


@pytest.mark.parametrize("training", [True, False])
def test_strided_input_gives_the_bits_of_the_contiguous_call(training):
    M, W = 65, 128
    bn, y, dz, _ = _drawn(M, W, "leaky_relu", 0.4, training)
    want = _run(bn, y, dz, "leaky_relu", 0.4, training)
    wide = torch.randn(M, W + 128, generator=torch.Generator().manual_seed(3))
    wide[:, 64:64 + W] = y
    wd = wide.to(DEV)
    view = wd[:, 64:64 + W]
    assert view.stride(0) == W + 128 and not view.is_contiguous()
    got = _run(bn, y, dz, "leaky_relu", 0.4, training, view=view.detach())
    for a, b in zip(got[:4], want[:4]):
        assert torch.equal(a, b)
    assert torch.equal(got[4].running_var, want[4].running_var)
    assert torch.equal(wd.cpu(), wide)                  # the input and its neighbouring columns are untouched


# ---------------------------------------------------------------- 2: no cancellation
def test_variance_has_no_cancellation():
    """Columns c + s N(0, 1) with |c| >> s, and a constant column.  Deviations from an fp32-rounded mean
    are exact to (ulp(c) / 2 / s)^2 ~ 1.5e-7 of the variance, so rstd holds 1e-5; an fp32
    E[y^2] - E[y]^2 is wrong by more than 100 % on the first kind."""
    import hicgat
    from hicgat import kernels
    M, W, eps = 4097, 64, 1e-5
    g = torch.Generator().manual_seed(2)
    kinds = [(100.0, 0.01), (-1000.0, 0.5), (0.0, 1e-3)]
    y = torch.empty(M, W)
    for j in range(W):
        y[:, j] = 7.25 if j % 4 == 3 else kinds[j % 4][0] + kinds[j % 4][1] * torch.randn(M, generator=g)
    want = 1.0 / torch.sqrt(y.double().var(0, unbiased=False) + eps)
    stats = torch.empty(4, W, device=DEV)
    kernels.default().bn_stats(y.to(DEV), eps, 0.1, stats, None, None, None)
    mean, lo, rstd, _ = stats.cpu().double()
    err = ((rstd - want).abs() / want)
    print("rstd relative error per kind:", [float(err[k::4].max()) for k in range(4)])
    assert (err <= 1e-5).all()
    assert ((mean + lo - y.double().mean(0)).abs() <= 1e-7 * y.double().mean(0).abs() + 1e-9).all()
    const = torch.arange(W) % 4 == 3
    assert ((rstd[const] - 1.0 / np.sqrt(eps)).abs() <= 1e-6 / np.sqrt(eps)).all()      # var = 0 exactly
    bn = BatchNorm1d(W).to(DEV)
    z = hicgat.ops.bn_act_dropout(y.to(DEV), bn, None)
    assert torch.isfinite(z).all() and (z[:, const] == 0).all()
    ref = copy.deepcopy(bn).cpu().double()(y.double())
    assert _rel(z, ref) <= 1e-5


# ---------------------------------------------------------------- 3: determinism
def _fwd_bwd(d, st, yd, dzd):
    import hicgat
    st.advance()
    yv = yd.detach().requires_grad_()
    z = hicgat.ops.bn_act_dropout(yv, d, "leaky_relu", st, 1)
    return (z,) + torch.autograd.grad(z, (yv, d.weight, d.bias), dzd)


def test_two_calls_give_equal_bits_and_a_replayed_graph_gives_eager_calls():
    import hicgat
    M, W = 4097, 64
    bn, y, dz, _ = _drawn(M, W, "leaky_relu", 0.4, True)
    a, b = _run(bn, y, dz, "leaky_relu", 0.4, True), _run(bn, y, dz, "leaky_relu", 0.4, True)
    for u, v in zip(a[:4], b[:4]):
        assert torch.equal(u, v)
    assert torch.equal(a[4].running_mean, b[4].running_mean) and torch.equal(a[4].running_var, b[4].running_var)
    yd, dzd = y.to(DEV), dz.to(DEV)
    de, dg = copy.deepcopy(bn).to(DEV), copy.deepcopy(bn).to(DEV)
    se, sg = (hicgat.DropoutState(DEV, seed=SEED, p=0.4) for _ in range(2))
    eager = [[t.clone() for t in _fwd_bwd(de, se, yd, dzd)] for _ in range(3)]
    assert not torch.equal(eager[0][0], eager[1][0])                 # the mask moves with the step count
    step = hicgat.graphs.CapturedStep(lambda: _fwd_bwd(dg, sg, yd, dzd), warmup=0)
    for k in range(3):
        out = step()
        torch.cuda.synchronize()
        for u, v in zip(out, eager[k]):
            assert torch.equal(u, v), k
    assert torch.equal(dg.running_mean, de.running_mean) and torch.equal(dg.running_var, de.running_var)
    assert dg.num_batches_tracked.item() == 3 == de.num_batches_tracked.item() and sg.step == 3


# ---------------------------------------------------------------- 4: refusals
def test_refusals_come_before_any_launch():
    from hicgat import _lib
    lib = _lib.lib()
    st = _lib.stream(torch.device(DEV))
    P = _lib.ptr
    M, W = 8, 64
    y = torch.randn(M, 2 * W, device=DEV)
    out = torch.full((M, 2 * W), 7.0, device=DEV)
    vec = torch.full((4 * W,), 7.0, device=DEV)       # stats / gamma / dgamma stand-ins
    rm, rv = torch.full((W,), 7.0, device=DEV), torch.full((W,), 7.0, device=DEV)
    nbt = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    ws = torch.full((1 << 16,), 7, dtype=torch.uint8, device=DEV)
    off = ctypes.c_void_p(y.data_ptr() + 4)
    EINVAL, EUNSUPPORTED = -1, -3

    def stats(yp=P(y), ld=2 * W, m=M, w=W, eps=1e-5, mom=0.1):
        return lib.hicgat_bn_stats(yp, ld, m, w, eps, mom, P(vec), P(rm), P(rv), P(nbt), P(ws), ws.numel(), st)

    def fwd(yp=P(y), ld=2 * W, m=M, w=W, eps=1e-5, act=1, p=0.4, sp=P(vec), ldz=2 * W):
        return lib.hicgat_bn_act_dropout_fwd(yp, ld, m, w, P(vec), P(vec), sp, P(rm), P(rv), eps, act, 0.01, p, 1, None,
                                             1, 0, 0, P(out), ldz, st)

    def bwd(dzp=P(y), ld=2 * W, m=M, w=W, eps=1e-5, act=1, p=0.4, sp=P(vec), slope=0.01):
        return lib.hicgat_bn_act_dropout_bwd(dzp, ld, P(y), 2 * W, P(y), 2 * W, m, w, P(vec), sp, P(rm), P(rv), eps,
                                             act, slope, p, P(out), 2 * W, P(vec), P(vec), 0, P(ws), ws.numel(), st)

    for f in (stats, fwd, bwd):
        for w in (32, 96, 1088):
            assert f(w=w, ld=2048) == EUNSUPPORTED, (f.__name__, w)
        assert f(off) == EINVAL and f(ld=W + 2) == EINVAL and f(ld=W - 4) == EINVAL
        assert f(eps=0.0) == EINVAL and f(eps=-1e-5) == EINVAL
    for mom in (0.0, -0.1, 1.5, float("nan")):
        assert stats(mom=mom) == EINVAL
    assert stats(m=1) == EINVAL and bwd(m=1) == EINVAL            # one row with batch statistics
    assert fwd(m=0, sp=None) == EINVAL
    assert fwd(p=1.0) == EINVAL and fwd(act=3) == EINVAL and fwd(ldz=W + 2) == EINVAL
    assert bwd(act=0) == EUNSUPPORTED and bwd(act=2, slope=0.0) == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (vec == 7.0).all() and (rm == 7.0).all() and (rv == 7.0).all()
    assert nbt.item() == 7 and (ws == 7).all()


# ---------------------------------------------------------------- 5: a model step against the reference
@functools.lru_cache(maxsize=None)
def _problem(feats):
    """test_gpu_dropout._model_problem with ``feats`` feature columns: n = 130, 30 % weighted contacts."""
    from oracle import graph as ogr
    n = 130
    rng = np.random.default_rng(130)
    a = (rng.random((n, n)) < 0.3) * rng.integers(1, 100, (n, n)).astype(np.float64)
    a = np.triu(a, 1)
    a = a + a.T
    x = (0.1 * rng.standard_normal((n, feats))).astype(np.float32)
    d = ogr.load_input(a.copy(), x)
    return a, x, d, ogr.cont2dist(d["y"], 0.5)


def _device_problem(feats):
    import hicgat
    a, x, _, _ = _problem(feats)
    y = torch.tensor(a, device=DEV)
    return hicgat.Adj.from_dense_device(y), hicgat.Truth.from_contacts(y, 0.5), torch.tensor(x, device=DEV), y


def _feats(name):
    return 256 if name.endswith("Heads4") else 512


def _ref_coords(ref, x, adj, masks=None, pre=None):
    """The reference's forward before its cdist (``masks``: the two sites' keep masks) or, without
    masks, its get_model; BatchNorm follows ``ref.training``.  ``pre`` receives (pre-activation,
    elements that count) per activation."""
    scale = float(philox_ref.scale(ref.dropout.p))
    h = ref.conv(x, adj)
    stages = [(None, None), (ref.densea, ref.bn_a), (ref.dense1, ref.bn1), (ref.dense2, ref.bn2)]
    for k, (lin, bn) in enumerate(stages):
        if lin is not None:
            h = bn(lin(h))
        m = masks[k] if masks is not None and k < 2 else None
        if pre is not None:
            pre.append((h.detach(), m if m is not None else torch.ones_like(h, dtype=torch.bool)))
        h = F.leaky_relu(h)
        if m is not None:
            h = h * m.to(h.dtype) * scale
    return ref.dense3(h)


def _seeded_reference(name, x, radj):
    """The first seed of 0..7 (the model's and the masks') whose float64 training forward keeps every
    counted pre-activation farther than 1e-6 of its layer's largest from 0."""
    n = x.shape[0]
    for seed in range(8):
        torch.manual_seed(seed)
        ref = ref_model(name)
        masks = [torch.from_numpy(philox_ref.keep_mask(n, w, 0.4, seed, 1, k))
                 for k, w in enumerate((ref.densea.in_features, 256))]
        pre = []
        with torch.no_grad():
            _ref_coords(copy.deepcopy(ref).double(), x.double(), radj, masks, pre)
        if all((h[m].abs() > 1e-6 * h.abs().max()).all() for h, m in pre):
            return seed, ref, masks
    raise AssertionError(f"{name}: no seed of 0..7 keeps the pre-activations away from 0")


@pytest.mark.parametrize("name", NAMES)
def test_training_step_matches_the_reference_composite(name):
    import hicgat
    from oracle import gat as og
    _, _, d, t_ref = _problem(_feats(name))
    adj, truth, x, _ = _device_problem(_feats(name))
    radj = (torch.tensor(d["rowptr"]), torch.tensor(d["col"]))
    seed, ref, masks = _seeded_reference(name, d["x"], radj)
    torch.manual_seed(seed)
    model = hicgat.MODELS[name]().to(DEV)
    assert model.training and ref.training
    og.CDIST_MODE = "donot_use_mm_for_euclid_dist"
    try:
        c_ref = _ref_coords(ref, d["x"], radj, masks)
        l_ref = F.mse_loss(torch.cdist(c_ref, c_ref, compute_mode=og.CDIST_MODE).float(), t_ref.float())
        l_ref.backward()
    finally:
        og.CDIST_MODE = "use_mm_for_euclid_dist_if_necessary"
    loss, _, coords = model.loss(x, adj, truth, "mse")
    loss.backward()
    st = model.dropout_state(x.device)
    assert st.seed == seed and st.step == 1 and st.p == 0.4
    np.testing.assert_allclose(coords.detach().cpu().numpy(), c_ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    assert abs(loss.item() - l_ref.item()) <= 1e-5 * l_ref.item()
    gscale = max(pr.grad.abs().max().item() for pr in ref.parameters())
    small = []
    for (k, p), pr in zip(model.named_parameters(), ref.parameters()):
        if pr.grad.abs().max().item() < 1e-3 * gscale:
            # zero in exact arithmetic: a bias in front of a training-mode BatchNorm, and the last bias
            assert p.grad.abs().max().item() < 1e-3 * gscale, k
            small.append(k)
            continue
        e = _rel(p.grad, pr.grad)
        print(f"{name} {k}: {e:.2e}")
        assert e < 2e-4, (k, e)
    assert set(small) <= {"densea.bias", "dense1.bias", "dense2.bias", "dense3.bias"}, small
    for bn in ("bn_a", "bn1", "bn2"):
        m, r = getattr(model, bn), getattr(ref, bn)
        assert _rel(m.running_mean, r.running_mean) <= 1e-5 and _rel(m.running_var, r.running_var) <= 1e-5
        assert m.num_batches_tracked.item() == 1


# ---------------------------------------------------------------- 6: mode semantics
def _buffers(model):
    return [b.clone() for b in model.buffers()]


@pytest.mark.parametrize("name", NAMES)
def test_mode_semantics(name):
    import hicgat
    from hicgat.train import cpu_state_dict
    _, _, d, _ = _problem(_feats(name))
    adj, truth, x, _ = _device_problem(_feats(name))
    torch.manual_seed(4)
    model = hicgat.MODELS[name]().to(DEV)
    norms = [getattr(model, n) for n in model.norms]
    with torch.no_grad():
        c1 = model.train().get_model(x, adj)
        c2 = model.get_model(x, adj)
        assert getattr(model, "_dropout_state", None) is None            # get_model never drops ...
        assert torch.equal(c1, c2)                                       # ... normalises by batch statistics ...
        assert all(bn.num_batches_tracked.item() == 2 for bn in norms)   # ... and moves the buffers
        _, _, ct = model.loss(x, adj, truth)
        st = model.dropout_state(x.device)
        assert st.step == 1 and not torch.equal(ct, c1)                  # the training forward drops
        assert all(bn.num_batches_tracked.item() == 3 for bn in norms)
        before = _buffers(model.eval())
        c_eval = model.get_model(x, adj)
        d_eval = model(x, adj)
        _, _, ce = model.loss(x, adj, truth)
        assert torch.equal(ce, c_eval) and d_eval.shape == (x.shape[0], x.shape[0])
        assert all(torch.equal(a, b) for a, b in zip(before, model.buffers())) and st.step == 1
        assert not torch.equal(c_eval, c1)
    ref = ref_model(name)
    ref.load_state_dict(cpu_state_dict(model), strict=True)
    radj = (torch.tensor(d["rowptr"]), torch.tensor(d["col"]))
    with torch.no_grad():
        c_ref = _ref_coords(ref.eval(), d["x"], radj)
    np.testing.assert_allclose(c_eval.cpu().numpy(), c_ref.numpy(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- 7: captured training
@pytest.mark.parametrize("name", NAMES)
def test_graph_replay_equals_eager_steps(name):
    """hicgat.train's loop: eager warm-up steps plus three replays give the bits of as many eager steps,
    the BatchNorm buffers included -- the replays run the running update on the device."""
    import hicgat
    adj, truth, x, y = _device_problem(_feats(name))
    data = hicgat.Data(x=x, edge_index=adj, y=y)
    steps = hicgat.train.GRAPH_WARMUP + 3
    res = []
    for graphed in (False, True):
        torch.manual_seed(0)
        model = hicgat.MODELS[name]().to(DEV)
        opt, hist = hicgat.train.train(model, data, truth, steps=steps, graph=graphed)
        assert all(getattr(model, n).num_batches_tracked.item() == steps for n in model.norms)
        with torch.no_grad():
            c_train = model.train().get_model(x, adj)
            c_eval = model.eval().get_model(x, adj)
        assert not torch.equal(c_train, c_eval)
        res.append((hist, opt.flat.clone(), _buffers(model), c_eval))
    (he, pe, be, ce), (hg, pg, bg, cg) = res
    assert len(he) == steps and he == hg
    assert torch.equal(pe, pg) and torch.equal(ce, cg)
    assert all(torch.equal(a, b) for a, b in zip(be, bg))
    fresh = BatchNorm1d(64)
    assert not torch.equal(bg[-3].cpu(), fresh.running_mean) and not torch.equal(bg[-2].cpu(), fresh.running_var)

"""GPU tests of the GATConv attention weights (gat_attn.hip, ops._GATConvAttnFn) against the fp64
restatement of tests/attention_ref.py.

Graphs (attention_ref.GRAPHS): n7 has an isolated row (the self loop only: alpha exactly 1); n70 is
dense (every row 70 edges: over the 64-lane chunk); n130 is a path plus a hub of degree 130 (rows of
degree 2, 3, 4 and 130, two chunks, N no multiple of 4); deg63 has rows of degree 63, 64 and 65.
Shapes (H, C): (2, 256), (2, 128), (1, 512), (4, 256) -- both lane / head classes, H = 1 and H = 4.

Tolerances are those of tests/test_gpu_gat_shapes.py: outputs (alpha, out, coordinates) rtol 1e-5 /
atol 1e-6, gradients 1e-4 of each tensor's maximum, the loss 1e-5 relative; row sums of alpha within
1e-6 of 1.  The gradient checks need every logit away from the leaky-relu kink: the inputs are the
first seed of a fixed sequence whose fp64 reference has no |z| < 1e-5, which the test asserts; no
entry is left out of a comparison."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
F_IN = 256
SHAPES = [(2, 256), (2, 128), (1, 512), (4, 256)]
NAMES = ["n7", "n70", "n130", "deg63"]
KINK = 1e-5
ENTROPY = "GATNetHeadsChanged3LayersEmbeddingDim256Entropy"


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
def _adj(name):
    """The graph's Adj, built once and never written; its device CSR is attention_ref's CSR."""
    import hicgat
    adj = hicgat.Adj.from_dense_device(torch.tensor(ar.GRAPHS[name](), device=DEV))
    rowptr, col = ar.csr_with_self_loops(name)
    assert torch.equal(adj.rowptr32.cpu().long(), rowptr) and torch.equal(adj.col32.cpu().long(), col)
    return adj


@functools.lru_cache(maxsize=None)
def _case(name, H, C):
    """Conditioned inputs and the fp64 reference of one (graph, shape), computed once: feature and
    weight scales of tests/test_gpu_gat_shapes.py (x 0.1 N(0, 1), the layer's own init, bias 0.1 N(0, 1),
    dout and G N(0, 1)); reference gradients for a loss on G alone and on G and dout together."""
    from oracle import gat as og
    rowptr, col = ar.csr_with_self_loops(name)
    n = rowptr.numel() - 1
    rng = np.random.default_rng(n + H + C)
    x = torch.tensor((0.1 * rng.standard_normal((n, F_IN))).astype(np.float32))
    g = torch.tensor(rng.standard_normal((n, H * C)).astype(np.float32))
    G = torch.tensor(rng.standard_normal((col.numel(), H)).astype(np.float32))
    for t in range(400):
        torch.manual_seed(n + H + C + 1000 * t)
        conv = og.GATConv(F_IN, C, heads=H)
        with torch.no_grad():
            conv.bias.copy_(torch.randn_like(conv.bias) * 0.1)
        p32 = {k: v.detach().clone() for k, v in conv.named_parameters()}
        P = {k: v.double().requires_grad_(True) for k, v in p32.items()}
        xd = x.double().requires_grad_(True)
        out, alpha, z = ar.gat_attention(xd, P["lin_l.weight"], P["att_l"], P["att_r"], P["bias"], rowptr, col)
        if float(z.detach().abs().min()) >= KINK:
            break
    grads = {}
    leaves = [xd] + [P[k] for k in ("lin_l.weight", "att_l", "att_r", "bias")]
    for key, loss in (("G", (alpha * G.double()).sum()),
                      ("G+dout", (alpha * G.double()).sum() + (out * g.double()).sum())):
        gr = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
        grads[key] = [torch.zeros_like(l) if t is None else t for l, t in zip(leaves, gr)]
    return dict(x=x, g=g, G=G, p32=p32, out=out.detach(), alpha=alpha.detach(), z=z.detach(), grads=grads,
                h=(x.double() @ p32["lin_l.weight"].double().t()), rowptr=rowptr, col=col)


def _layer(case, H, C):
    import hicgat
    conv = hicgat.GATConv(F_IN, C, heads=H)
    with torch.no_grad():
        for k, v in conv.named_parameters():
            v.copy_(case["p32"][k])
    return conv.to(DEV)


GRID = [(n, H, C) for n in NAMES for (H, C) in SHAPES]


# ---------------------------------------------------------------- 1: the transpose map
@pytest.mark.parametrize("name", NAMES)
def test_transpose_map_equals_numpy(name):
    adj = _adj(name)
    t = adj.transpose_map()
    assert t.dtype == torch.int32 and t is adj.tmap32          # cached on the Adj
    assert np.array_equal(t.cpu().numpy(), ar.transpose_map_np(*ar.csr_with_self_loops(name)))


def test_transpose_map_refuses_an_asymmetric_csr():
    import hicgat
    adj = hicgat.Adj.from_dense_device(torch.tensor(ar.GRAPHS["n7"](), device=DEV))
    adj.col32 = adj.col32.clone()
    rp = adj.rowptr32.cpu()
    adj.col32[int(rp[0])] = 6 if int(adj.col32[int(rp[0])]) != 6 else 5     # (0, 6) without (6, 0)
    t = hicgat.kernels.default().transpose_map(adj.rowptr32, adj.col32)
    assert int(t.min()) == -1
    with pytest.raises(ValueError, match="symmetric"):
        adj.transpose_map()


# ---------------------------------------------------------------- 2: alpha against the fp64 reference
@pytest.mark.parametrize("name,H,C", GRID)
def test_alpha_matches_reference(name, H, C):
    import hicgat
    case, adj = _case(name, H, C), _adj(name)
    conv = _layer(case, H, C)
    with torch.no_grad():
        out, attn = conv(case["x"].to(DEV), adj, return_attention_weights=True)
        plain = conv(case["x"].to(DEV), adj)
    assert isinstance(attn, hicgat.Adj) and attn.sparse_sizes() == (adj.n, adj.n)
    st = attn.storage
    assert st.rowptr().dtype == torch.int64 and st.col().dtype == torch.int64
    assert torch.equal(st.rowptr().cpu(), case["rowptr"]) and torch.equal(st.col().cpu(), case["col"])
    alpha = st.value()
    assert alpha.shape == (case["col"].numel(), H) and alpha.dtype == torch.float32
    assert torch.equal(out, plain)
    a = alpha.cpu().double()
    np.testing.assert_allclose(a.numpy(), case["alpha"].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out.cpu().numpy(), case["out"].numpy(), rtol=1e-5, atol=1e-6)
    row = ar.rows_of(case["rowptr"])
    sums = torch.zeros(adj.n, H, dtype=torch.float64).index_add(0, row, a)
    assert float((sums - 1).abs().max()) <= 1e-6
    # sum_j alpha_ij h_j + bias from the DEVICE's alpha reproduces out
    h = case["h"].view(adj.n, H, C)
    agg = torch.zeros_like(h).index_add(0, row, h[case["col"]] * a.unsqueeze(-1)).reshape(adj.n, H * C)
    np.testing.assert_allclose((agg + case["p32"]["bias"].double()).numpy(), case["out"].numpy(), rtol=1e-5,
                               atol=1e-6)
    if name == "n7":
        lo, hi = int(case["rowptr"][6]), int(case["rowptr"][7])
        assert hi - lo == 1 and torch.equal(alpha[lo:hi].cpu(), torch.ones(1, H))


# ---------------------------------------------------------------- 3: a random G, with and without dout
def _run_G(case, adj, H, C, with_dout, act=None):
    conv = _layer(case, H, C)
    x = case["x"].to(DEV).requires_grad_(True)
    out, attn = conv(x, adj, act=act, return_attention_weights=True)
    loss = (attn.storage.value() * case["G"].to(DEV)).sum()
    if with_dout:
        loss = loss + (out * case["g"].to(DEV)).sum()
    loss.backward()
    return [x.grad, conv.lin_l.weight.grad, conv.att_l.grad, conv.att_r.grad, conv.bias.grad]


@pytest.mark.parametrize("with_dout", [False, True])
@pytest.mark.parametrize("name,H,C", GRID)
def test_gradient_through_alpha_matches_reference(name, H, C, with_dout):
    case, adj = _case(name, H, C), _adj(name)
    assert float(case["z"].abs().min()) >= KINK          # a condition on the inputs, nothing is excluded
    got = _run_G(case, adj, H, C, with_dout)
    want = case["grads"]["G+dout" if with_dout else "G"]
    for k, gm, gr in zip(("x", "lin_l.weight", "att_l", "att_r", "bias"), got, want):
        e = _rel(gm.cpu(), gr)      # (the bias without a dout: zeros on both sides)
        print(f"{name} ({H}, {C}) dout={with_dout} {k}: {e:.3e}")
        assert e < 1e-4, (k, e)


# ---------------------------------------------------------------- 4: nothing depends on alpha
def _plain_vs_attn(adj, conv, x0, g, act, tail=None):
    res = []
    for attn in (False, True):
        conv.zero_grad()
        if tail is not None:
            tail.zero_grad()
        x = x0.clone().requires_grad_(True)
        out = conv(x, adj, act=act, return_attention_weights=attn)
        alpha = None
        if attn:
            out, a = out
            alpha = a.storage.value()
        loss = (out * g).sum() if tail is None else tail.post_act(out).square().sum()
        loss.backward()
        grads = [x.grad.clone()] + [p.grad.clone() for p in conv.parameters()]
        if tail is not None:
            grads += [p.grad.clone() for n_, p in tail.named_parameters() if not n_.startswith("conv.")]
        res.append((out.detach().clone(), grads, alpha))
    (o0, g0, _), (o1, g1, alpha) = res
    assert alpha is not None and alpha.requires_grad
    assert torch.equal(o0, o1)
    assert len(g0) == len(g1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("name,H,C", [("n130", 2, 256), ("n130", 2, 128), ("deg63", 4, 256), ("n70", 1, 512)])
def test_unused_alpha_is_bit_equal_to_the_plain_call(name, H, C, act):
    case, adj = _case(name, H, C), _adj(name)
    _plain_vs_attn(adj, _layer(case, H, C), case["x"].to(DEV), case["g"].to(DEV), act)


def test_unused_alpha_bit_equal_in_the_tiled_form(monkeypatch):
    """(2, 256) on the dense graph with the tile threshold lifted: 32 x 32 tiles on the matrix cores plus
    a sparse remainder (the 6 x 6 corner); also a G through the tiled source pass against the reference."""
    import hicgat
    monkeypatch.setattr(hicgat.graph, "TILE_MIN_N", 0)
    case = _case("n70", 2, 256)
    adj = hicgat.Adj.from_dense_device(torch.tensor(ar.GRAPHS["n70"](), device=DEV))
    t = adj.tiles()
    assert t is not None and 0 < t.n_dense < adj.device_nnz
    _plain_vs_attn(adj, _layer(case, 2, 256), case["x"].to(DEV), case["g"].to(DEV), "relu")
    got = _run_G(case, adj, 2, 256, True)
    for k, gm, gr in zip(("x", "lin_l.weight", "att_l", "att_r", "bias"), got, case["grads"]["G+dout"]):
        assert _rel(gm.cpu(), gr) < 1e-4, k


def test_unused_alpha_bit_equal_feeding_the_fused_tail():
    """(2, 256) into the flagship's one-kernel tail, whose backward runs this layer's rows pass
    (HICGAT_FUSE_ROWS on): the attention call must keep that link."""
    import hicgat
    from hicgat import ops
    assert ops.FUSE_ROWS and ops.FUSED_TAIL and ops.FUSED_TAIL_BWD
    n = max(1024, ops.FUSED_TAIL_MIN_M)
    rng = np.random.default_rng(4)
    a = np.triu((rng.random((n, n)) < 0.01).astype(np.float64), 1)
    adj = hicgat.Adj.from_dense_device(torch.tensor(a + a.T, device=DEV))
    torch.manual_seed(2)
    model = hicgat.GATNetSelectiveResidualsUpdated().to(DEV)
    x = torch.tensor((0.1 * rng.standard_normal((n, 512))).astype(np.float32), device=DEV)
    assert ops.fused_tail_ok(model, x)
    out, attn = model.conv(x, adj, act="relu", return_attention_weights=True)
    if hicgat.kernels.default().tail_waves() == 16:
        assert hasattr(out, "_hicgat_rows")
    _plain_vs_attn(adj, model.conv, x, None, "relu", tail=model)


# ---------------------------------------------------------------- 5: determinism and capture
@pytest.mark.parametrize("name,H,C", [("n130", 2, 128), ("n70", 4, 256)])
def test_two_runs_are_bit_equal(name, H, C):
    case, adj = _case(name, H, C), _adj(name)
    a, b = _run_G(case, adj, H, C, True, "relu"), _run_G(case, adj, H, C, True, "relu")
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@functools.lru_cache(maxsize=None)
def _entropy_problem():
    import hicgat
    a = ar.GRAPHS["n130"]()
    rng = np.random.default_rng(130)
    y = a * np.triu(rng.integers(1, 50, a.shape), 1).astype(np.float64)
    y = torch.tensor(y + y.T, device=DEV)
    adj = hicgat.Adj.from_dense_device(y)
    truth = hicgat.Truth.from_contacts(y, 0.5)
    x = torch.tensor((0.1 * rng.standard_normal((130, 256))).astype(np.float32), device=DEV)
    return adj, truth, x, y


def test_entropy_model_graph_replay_equals_eager_steps():
    import hicgat
    adj, truth, x, y = _entropy_problem()
    data = hicgat.Data(x=x, edge_index=adj, y=y)
    steps = hicgat.train.GRAPH_WARMUP + 3
    res = []
    for graphed in (False, True):
        torch.manual_seed(0)
        model = hicgat.MODELS[ENTROPY]().to(DEV)
        opt, hist = hicgat.train.train(model, data, truth, steps=steps, graph=graphed)
        res.append((hist, opt.flat.clone()))
    (he, pe), (hg, pg) = res
    assert len(he) == steps and he == hg and he[0] != he[-1]
    assert torch.equal(pe, pg)


# ---------------------------------------------------------------- 6: the Entropy model against fp64
def test_entropy_model_matches_the_fp64_restatement():
    import hicgat
    adj, truth, x, _ = _entropy_problem()
    torch.manual_seed(0)
    ref = ar.EntropyRef()
    torch.manual_seed(0)
    model = hicgat.MODELS[ENTROPY]()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"layout_{ENTROPY}.json")) as fh:
        fx = json.load(fh)
    assert list(model.state_dict()) == fx["keys"] == list(ref.state_dict())
    assert sum(p.numel() for p in model.parameters()) == fx["parameters"]
    for k, v in model.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k]), k
    ref = ref.double()
    model = model.to(DEV).train()
    csr = ar.csr_with_self_loops("n130")
    l_ref, c_ref = ref.loss(x.cpu().double(), csr, truth.dense().cpu().double())
    l_ref.backward()
    loss, _, coords = model.loss(x, adj, truth)
    loss.backward()
    np.testing.assert_allclose(coords.detach().cpu().numpy(), c_ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    e = abs(loss.item() - l_ref.item()) / abs(l_ref.item())
    print(f"loss {loss.item():.8g} ref {l_ref.item():.8g} rel {e:.2e}")
    assert e < 1e-5
    gr = dict(ref.named_parameters())
    gscale = max(float(p.grad.abs().max()) for p in gr.values())
    for k, p in model.named_parameters():
        if k == "dense2.bias":
            # zero in exact arithmetic (a translation of the coordinates changes no distance; the fp64
            # reference gives ~1e-18), so it has no maximum of its own to be relative to: fp32 rounding
            # on the device, held to 1e-4 of the model's largest gradient
            assert float(gr[k].grad.abs().max()) < 1e-12 * gscale
            print(f"{k}: {float(p.grad.abs().max()):.3e} absolute, gscale {gscale:.3e}")
            assert float(p.grad.abs().max()) < 1e-4 * gscale, k
            continue
        e = _rel(p.grad.cpu(), gr[k].grad)
        print(f"{k}: {e:.3e}")
        assert e < 1e-4, (k, e)
    # forward(): (D, attn) as the reference returns them; get_model(): the coordinates
    with torch.no_grad():
        D, attn = model(x, adj)
        assert torch.equal(model.get_model(x, adj), coords.detach())
    assert D.shape == (130, 130) and attn.storage.value().shape == (csr[1].numel(), 2)


# ---------------------------------------------------------------- 7: refusals
def test_refusals():
    import hicgat
    conv = hicgat.GATConv(64, 96, heads=2).to(DEV)
    with pytest.raises(NotImplementedError, match="out_channels % 128"):
        conv(torch.zeros(7, 64, device=DEV), _adj("n7"), return_attention_weights=True)
    K = hicgat.kernels.default()
    adj = _adj("n7")
    z = torch.zeros(7, 2, device=DEV)
    with pytest.raises(hicgat._lib.HicgatError, match="-3"):     # HICGAT_EUNSUPPORTED from the C ABI itself
        K.gat_alpha(adj.rowptr32, adj.col32, 96, z, z, torch.zeros(7, 8, device=DEV), 0.2,
                    torch.zeros(adj.device_nnz, 2, device=DEV))
    with pytest.raises(NotImplementedError, match=r"GATConv\(512, 256, heads=2\)"):
        hicgat.dist.ShardedTrainer(hicgat.MODELS[ENTROPY](), torch.zeros(8, 256), None, None)

"""GPU: attention dropout (``GATConv(dropout=p)`` in training mode) on the DROP forms of the forward
gather and the source pass.

The device mask is compared bit for bit with the numpy restatement (tests/attn_dropout_ref.py); outputs
and gradients with a float64 torch composite written here (segment softmax over the self-looped CSR,
times the restated mask and scale) under the bounds tests/test_gpu_parity.py uses for the same
quantities of the undropped layer (out: rtol 1e-5 + atol 1e-6; gradients: 1e-4 of the tensor's max --
a masked sum has no more terms than the unmasked one); everything else is bit equality.

One graph of 80 nodes: hub 0 has 69 neighbours (70 edges with its self loop: a second, partly filled
64-edge chunk), 1 .. 76 is a path (3 - 4 edges; node 76: 2, fewer than the smallest gather unroll),
77 - 78 a pair, 79 has its self loop alone.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_dropout_ref as adr

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 80
FIN = 16                 # the smallest in_channels lin_l's GEMM takes with 16-byte rows to spare
SEED, STEP, SITE = 0x5EED0123456789AB, 3, 2
SHAPES = [(1, 256), (2, 128), (2, 384), (2, 256), (4, 256)]
KINK_MARGIN = 5e-7       # tests/test_gpu_gat_shapes.py: logits this close to 0 may take either slope in fp32
EINVAL, EUNSUPPORTED = -1, -3


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
def _graph():
    import hicgat
    e = [(0, j) for j in range(1, 70)] + [(i, i + 1) for i in range(1, 76)] + [(77, 78)]
    row = [i for i, _ in e] + [j for _, j in e]
    col = [j for _, j in e] + [i for i, _ in e]
    adj = hicgat.Adj(row, col, sparse_sizes=(N, N)).to(DEV)
    rowptr, colv = adj.rowptr32.cpu().long(), adj.col32.cpu().long()
    deg = (rowptr[1:] - rowptr[:-1]).tolist()
    assert deg[0] == 70 and deg[76] == 2 and deg[79] == 1 and int(colv[rowptr[79]]) == 79
    return adj, rowptr, colv


@functools.lru_cache(maxsize=None)
def _inputs(D):
    rng = np.random.default_rng(D)
    x = torch.tensor((0.5 * rng.standard_normal((N, FIN))).astype(np.float32))
    g = torch.tensor(rng.standard_normal((N, D)).astype(np.float32))
    return x, g


def _composite(x, W, al, ar, b, rowptr, col, M, act=None, ns=0.2):
    """PyG 1.7.2 GATConv with ``alpha = alpha * M`` before the aggregation (M: keep bit x scale, [nnz, H]);
    any dtype (the tests run it in float64).  Returns (out, alpha before the dropout, logits z, out
    before the activation)."""
    n = rowptr.numel() - 1
    H, C = al.shape[-2], al.shape[-1]
    h = (x @ W.t()).view(n, H, C)
    a_l, a_r = (h * al.view(1, H, C)).sum(-1), (h * ar.view(1, H, C)).sum(-1)
    row = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    z = a_l[col] + a_r[row]
    e = F.leaky_relu(z, ns)
    idx = row.view(-1, 1).expand_as(e)
    emax = torch.full((n, H), float("-inf"), dtype=e.dtype).scatter_reduce(0, idx, e.detach(), reduce="amax")
    u = (e - emax[row]).exp()
    alpha = u / (torch.zeros((n, H), dtype=e.dtype).index_add(0, row, u)[row] + 1e-16)
    pre = torch.zeros_like(h).index_add(0, row, h[col] * (alpha * M).unsqueeze(-1)).reshape(n, H * C) + b
    return (torch.relu(pre) if act else pre), alpha, z, pre


def _factor(H, p, step=STEP, seed=SEED, site=SITE):
    _, rowptr, col = _graph()
    keep = adr.keep_mask(rowptr.numpy(), col.numpy(), H, p, seed, step, site)
    return torch.tensor(keep.astype(np.float64) * float(adr.scale(p)))


def _conv(H, C, p, M, act, fin=FIN, x=None, csr=None):
    """A seeded GATConv(fin, C, heads=H, dropout=p) on the device whose float64 logits stay away from the
    leaky-relu kink and (act) whose float64 outputs stay away from the relu's: the first seed of a
    fixed sequence that does (the reference's own arithmetic is discontinuous there)."""
    import hicgat
    if x is None:
        x = _inputs(H * C)[0]
    rowptr, col = csr if csr is not None else _graph()[1:]
    for t in range(200):
        torch.manual_seed(100 * H + C + 1000 * t)
        conv = hicgat.GATConv(fin, C, heads=H, dropout=p)
        with torch.no_grad():
            conv.bias.copy_(torch.randn_like(conv.bias) * 0.1)
            _, _, z, pre = _composite(x.double(), conv.lin_l.weight.double(), conv.att_l.double(),
                                      conv.att_r.double(), conv.bias.double(), rowptr, col, M, act)
        if float(z.abs().min()) > KINK_MARGIN and (not act or float(pre.abs().min()) > 1e-6 * float(pre.abs().max())):
            return conv.to(DEV)
    raise AssertionError("no seed keeps the logits away from the kinks")


def _state(step=STEP, seed=SEED):
    import hicgat
    st = hicgat.DropoutState(DEV, seed=seed)
    st.reset(step=step)
    return st


def _params(conv):
    return [conv.lin_l.weight, conv.att_l, conv.att_r, conv.bias]


def _run(conv, x, g, act=None, attn=False, state=None, site=SITE, ent=0.3):
    """One forward + backward of loss = <out, g> (+ ent * entropy(alpha)): (out, alpha or None, grads of
    x, W, att_l, att_r, bias), detached."""
    from hicgat import ops
    adj = _graph()[0]
    for p in conv.parameters():
        p.grad = None
    xd = x.to(DEV).requires_grad_(True)
    kw = {} if state is None else {"dropout_state": state, "site": site}
    if attn:
        out, a = conv(xd, adj, act=act, return_attention_weights=True, **kw)
        alpha = a.storage.value()
        loss = (out * g.to(DEV)).sum() + ent * ops.attention_entropy(alpha)
    else:
        out, alpha = conv(xd, adj, act=act, **kw), None
        loss = (out * g.to(DEV)).sum()
    loss.backward()
    grads = [xd.grad] + [p.grad for p in _params(conv)]
    return out.detach(), None if alpha is None else alpha.detach(), [t.detach().clone() for t in grads]


# ---------------------------------------------------------------- the mask
@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("H", [1, 2, 4])
def test_device_mask_is_the_restated_one(H, p):
    from hicgat import ops
    adj, rowptr, col = _graph()
    m = ops.attention_dropout_mask(adj, H, p, SEED, STEP, SITE)
    assert m.dtype == torch.bool and tuple(m.shape) == (col.numel(), H)
    ref = adr.keep_mask(rowptr.numpy(), col.numpy(), H, p, SEED, STEP, SITE)
    assert np.array_equal(m.cpu().numpy(), ref)
    for what, o in {"step": ops.attention_dropout_mask(adj, H, p, SEED, STEP + 1, SITE),
                    "site": ops.attention_dropout_mask(adj, H, p, SEED, STEP, SITE + 1),
                    "seed": ops.attention_dropout_mask(adj, H, p, SEED + 1, STEP, SITE)}.items():
        assert not torch.equal(m, o), what
    # mask(i, j) is not mask(j, i): compare every off-diagonal edge with its transpose
    t = adj.transpose_map().long()
    off = torch.tensor(np.repeat(np.arange(N), np.diff(rowptr.numpy())) != col.numpy(), device=DEV)
    differ = (m[t] != m)[off].float().mean().item()
    assert 0.5 * 2 * p * (1 - p) < differ < 1.5 * 2 * p * (1 - p), differ
    # the step from a device counter is the step by value; p = 0 keeps everything
    K = _kernels()
    buf = torch.empty((col.numel(), H), dtype=torch.uint8, device=DEV)
    K.attn_mask(adj.rowptr32, adj.col32, H, buf, (p, SEED, _state().counter, 0, SITE))
    assert torch.equal(buf.bool(), m)
    assert ops.attention_dropout_mask(adj, H, 0.0, SEED, STEP, SITE).all()


def _kernels():
    from hicgat import kernels
    return kernels.default()


@pytest.mark.parametrize("p", [0.5, 0.9])
def test_kept_share(p):
    """On a complete graph of 200 nodes (40 000 edges x 4 heads): within 5 sigma of 1 - p."""
    import hicgat
    from hicgat import ops
    n = 200
    adj = hicgat.Adj.from_dense_device(torch.ones((n, n), dtype=torch.float64, device=DEV) - torch.eye(
        n, dtype=torch.float64, device=DEV))
    m = ops.attention_dropout_mask(adj, 4, p, SEED, 1, 0)
    cnt = m.numel()
    assert cnt == n * n * 4
    share = m.float().mean().item()
    bound = 5 * math.sqrt(p * (1 - p) / cnt)
    print(f"p={p}: kept {share:.5f} of {cnt}, |dev| {abs(share - (1 - p)):.2e} (bound {bound:.2e})")
    assert abs(share - (1 - p)) <= bound
    assert np.array_equal(m.cpu().numpy(), adr.keep_mask(adj.rowptr32.cpu().numpy(), adj.col32.cpu().numpy(), 4, p,
                                                         SEED, 1, 0))


# ---------------------------------------------------------------- parity with the float64 composite
@pytest.mark.parametrize("attn", [False, True])
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("p", [0.5, 0.9])
@pytest.mark.parametrize("H,C", SHAPES)
def test_parity_with_float64_composite(H, C, p, act, attn):
    _, rowptr, col = _graph()
    x, g = _inputs(H * C)
    M = _factor(H, p)
    conv = _conv(H, C, p, M, act)
    assert conv.training
    out, alpha, grads = _run(conv, x, g, act, attn, _state())

    xr = x.double().requires_grad_(True)
    pr = [t.detach().cpu().double().requires_grad_(True) for t in _params(conv)]
    out_r, alpha_r, _, _ = _composite(xr, *pr, rowptr, col, M, act)
    loss = (out_r * g.double()).sum()
    if attn:
        loss = loss - 0.3 * (alpha_r * torch.log(alpha_r + 1e-12)).sum()
    loss.backward()
    np.testing.assert_allclose(out.cpu().numpy(), out_r.detach().numpy(), rtol=1e-5, atol=1e-6)
    errs = {}
    for name, a, b in zip(("x", "lin_l.weight", "att_l", "att_r", "bias"), grads, [xr] + pr):
        errs[name] = _rel(a.cpu(), b.grad)
    print(f"(H, C) = ({H}, {C}) p = {p} act = {act} attn = {attn}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for name, e in errs.items():
        assert e < 1e-4, (name, e)
    if attn:
        # the returned attention weights are the undropped softmax: the bits of the dropout = 0 layer
        conv.dropout = 0.0
        _, alpha0, _ = _run(conv, x, g, act, True)
        assert torch.equal(alpha, alpha0)


# ---------------------------------------------------------------- bit equality
@pytest.mark.parametrize("H,C", [(2, 256), (2, 128)])
@pytest.mark.parametrize("attn", [False, True])
def test_p0_training_and_eval_are_the_current_path(H, C, attn):
    x, g = _inputs(H * C)
    conv = _conv(H, C, 0.0, torch.ones(()), "relu")
    base = _run(conv, x, g, "relu", attn)

    def same(res):
        assert torch.equal(res[0], base[0])
        assert (res[1] is None and base[1] is None) or torch.equal(res[1], base[1])
        assert all(torch.equal(a, b) for a, b in zip(res[2], base[2]))

    same(_run(conv, x, g, "relu", attn, _state()))      # training, dropout = 0, a state passed
    conv.dropout = 0.6
    conv.eval()
    same(_run(conv, x, g, "relu", attn))                # eval mode, dropout = 0.6
    assert getattr(conv, "_dropout_state", None) is None   # neither made nor advanced a state
    conv.train()
    dropped = _run(conv, x, g, "relu", attn)
    assert not torch.equal(dropped[0], base[0])
    assert conv._dropout_state.step == 1                # its own state, advanced by the forward


@pytest.mark.parametrize("H,C", [(2, 256), (4, 256)])
def test_no_grad_still_drops_and_a_step_repeats(H, C):
    adj = _graph()[0]
    x, g = _inputs(H * C)
    conv = _conv(H, C, 0.5, _factor(H, 0.5), None)
    a = _run(conv, x, g, None, True, _state())
    b = _run(conv, x, g, None, True, _state())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(s, t) for s, t in zip(a[2], b[2]))
    c = _run(conv, x, g, None, True, _state(step=STEP + 1))
    assert not torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    with torch.no_grad():                               # the inference form of the DROP kernel (no out2)
        out = conv(x.to(DEV), adj, dropout_state=_state(), site=SITE)
    assert torch.equal(out, a[0])
    conv.eval()
    with torch.no_grad():
        plain = conv(x.to(DEV), adj)
    assert not torch.equal(plain, out)
    # a later advance of the state does not reach the backward of an earlier forward
    conv.train()
    st = _state()
    xd = x.to(DEV).requires_grad_(True)
    out = conv(xd, adj, dropout_state=st, site=SITE)
    st.advance()
    (out * g.to(DEV)).sum().backward()
    assert torch.equal(xd.grad, _run(conv, x, g, None, False, _state())[2][0])


@pytest.mark.parametrize("H,C", [(2, 256), (2, 384)])
def test_row_ranges_at_the_c_abi(H, C):
    """[0, 30) + [30, 57) + [57, 80) gives the bits of [0, 80) in both DROP passes, with the step by value
    or from a device counter."""
    K = _kernels()
    adj = _graph()[0]
    rp, cl = adj.rowptr32, adj.col32
    D = H * C
    x, g = _inputs(D)
    conv = _conv(H, C, 0.5, _factor(H, 0.5), None)
    W, al, ar, b = [t.detach().contiguous() for t in _params(conv)]
    h, a_src, a_dst = K.linear_att(x.to(DEV), W, al, ar)
    dout = g.to(DEV).contiguous()

    def run(ranges, drop):
        out, out2 = (torch.full((N, D), float("nan"), device=DEV) for _ in range(2))
        rs = torch.full((N, 4 * H), float("nan"), device=DEV)
        for r0, r1 in ranges:
            K.agg_fwd_act(rp, cl, r0, r1, h, a_src, a_dst, b, 0.2, 0, out, out2, rs, drop=drop)
        K.agg_bwd_rows(0, N, 0, dout, out, b, out2, None, rs)
        dh = torch.full((N, D), float("nan"), device=DEV)
        da = torch.full((N, H), float("nan"), device=DEV)
        for r0, r1 in ranges:
            K.agg_bwd_src(rp, cl, r0, r1, h, a_src, a_dst, rs, dout, al, ar, 0.2, dh, da, drop=drop)
        return out, out2, rs, dh, da

    whole = run([(0, N)], (0.5, SEED, None, STEP, SITE))
    parts = run([(0, 30), (30, 57), (57, N)], (0.5, SEED, None, STEP, SITE))
    ctr = run([(0, N)], (0.5, SEED, _state().counter, 0, SITE))
    for a, s, c in zip(whole, parts, ctr):
        assert not torch.isnan(a).any()
        assert torch.equal(a, s) and torch.equal(a, c)
    empty = run([(40, 40)], (0.5, SEED, None, STEP, SITE))
    assert torch.isnan(empty[0]).all() and torch.isnan(empty[3]).all()      # an empty range writes nothing


@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("H,C", [(2, 256), (4, 256), (2, 128)])
def test_all_dropped_row(H, C, act):
    """Node 79 has its self loop alone; at a step where every head drops it: out = bias (or relu(bias))
    and the row hands nothing to dx as a destination -- its own dx row, which nothing else feeds, is 0."""
    _, rowptr, col = _graph()
    e = int(rowptr[79])
    step = next(s for s in range(1, 400) if not adr.keep_mask(rowptr.numpy(), col.numpy(), H, 0.9, SEED, s, SITE)[e].any())
    x, g = _inputs(H * C)
    conv = _conv(H, C, 0.9, _factor(H, 0.9, step=step), act)
    out, _, grads = _run(conv, x, g, act, False, _state(step=step))
    bias = conv.bias.detach()
    assert torch.equal(out[79], torch.relu(bias) if act else bias)
    assert torch.count_nonzero(grads[0][79]) == 0
    assert torch.count_nonzero(grads[0][0]) > 0


# ---------------------------------------------------------------- (2, 256) under the fused tail
def test_flagship_step_with_the_fused_rows_epilogue():
    """One training step of the flagship at ops.FUSED_TAIL_MIN_M rows with conv.dropout = 0.5: the
    one-kernel tail runs the layer's (unchanged) rows pass in its backward's epilogue.  Against the
    float64 composite of the conv followed by the reference's tail (oracle.gat's layers in float64);
    bounds: those of tests/test_gpu_gat_shapes.py's fused-tail check of the undropped layer."""
    import hicgat
    from hicgat import ops
    from oracle import gat as og
    n = ops.FUSED_TAIL_MIN_M
    assert ops.FUSE_ROWS
    rng = np.random.default_rng(3)
    a = np.triu((rng.random((n, n)) < 0.02).astype(np.float64), 1)
    adj = hicgat.Adj.from_dense_device(torch.tensor(a + a.T, device=DEV))
    rowptr, col = adj.rowptr32.cpu().long(), adj.col32.cpu().long()
    x = torch.tensor((0.1 * rng.standard_normal((n, 512))).astype(np.float32))
    g = torch.tensor(rng.standard_normal((n, 3)).astype(np.float32))
    keep = adr.keep_mask(rowptr.numpy(), col.numpy(), 2, 0.5, SEED, 1, 0)
    M = torch.tensor(keep.astype(np.float64) * 2.0)

    def tail(m, o):
        r = m.align_densea(o)
        o = F.relu(m.norm_a(m.densea(o))) + r
        r = m.align_dense1(o)
        o = F.relu(m.norm1(m.dense1(o))) + r
        return m.dense3(F.relu(m.norm2(m.dense2(o))))

    def build(t):
        torch.manual_seed(40 + t)
        ref = og.GATNetSelectiveResidualsUpdated()
        with torch.no_grad():
            ref.conv.bias.copy_(torch.randn_like(ref.conv.bias) * 0.1)
        return ref

    # weights whose float64 logits and relu inputs keep off the kinks: two evaluations agree to ~1e-7 of
    # the layer's max (tests/kinks.py), and an element closer to 0 than that may fall on either side
    for t in range(100):
        ref = build(t).double()
        with torch.no_grad():
            c = ref.conv
            _, _, z, pre = _composite(x.double(), c.lin_l.weight, c.att_l, c.att_r, c.bias, rowptr, col, M, "relu")
            o = torch.relu(pre)
            z1 = ref.norm_a(ref.densea(o))
            o1 = F.relu(z1) + ref.align_densea(o)
            z2 = ref.norm1(ref.dense1(o1))
            o2 = F.relu(z2) + ref.align_dense1(o1)
            z3 = ref.norm2(ref.dense2(o2))
        if float(z.abs().min()) > KINK_MARGIN and all(float(v.abs().min()) > 3e-7 * float(v.abs().max())
                                                      for v in (pre, z1, z2, z3)):
            break
    else:
        raise AssertionError("no seed keeps the relu inputs off the kinks")
    mine = hicgat.GATNetSelectiveResidualsUpdated()
    mine.load_state_dict(build(t).state_dict())
    mine = mine.to(DEV).train()
    mine.conv.dropout = 0.5
    mine.conv.dropout_state(DEV).reset(seed=SEED, step=0)      # the forward advances it to step 1
    xd = x.to(DEV)
    assert ops.fused_tail_ok(mine, xd)
    coords = mine.get_model(xd, adj)
    (coords * g.to(DEV)).sum().backward()
    assert mine.conv._dropout_state.step == 1

    c = ref.conv
    o, _, _, _ = _composite(x.double(), c.lin_l.weight, c.att_l, c.att_r, c.bias, rowptr, col, M, "relu")
    c_ref = tail(ref, o)
    (c_ref * g.double()).sum().backward()
    np.testing.assert_allclose(coords.detach().cpu().numpy(), c_ref.detach().numpy(), rtol=1e-5, atol=1e-6)
    worst = {}
    for (k, p), pr in zip(mine.named_parameters(), ref.parameters()):
        worst[k] = _rel(p.grad.cpu(), pr.grad)
    print("fused tail under dropout: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, e in worst.items():
        assert e < 2e-4, (k, e)


# ---------------------------------------------------------------- the captured step
def test_captured_step_replays_as_the_next_step(monkeypatch):
    """train(attn_dropout=0.5) of a small zoo model (GATConv(512, 128, heads=2) -> four Linears): one
    eager step, then the captured step replayed three times, against four eager steps from the same
    seed -- loss and parameter bits."""
    import hicgat
    from hicgat import train as tr
    monkeypatch.setattr(tr, "GRAPH_WARMUP", 1)
    adj = _graph()[0]
    rng = np.random.default_rng(9)
    x = torch.tensor((0.1 * rng.standard_normal((N, 512))).astype(np.float32), device=DEV)
    y = torch.tensor(rng.integers(1, 50, (N, N)).astype(np.float64), device=DEV)
    y = torch.triu(y, 1)
    truth = hicgat.Truth.from_contacts(y + y.t(), 0.5)
    data = hicgat.graph.Data(x=x, edge_index=adj, y=y)

    def run(graph):
        torch.manual_seed(21)
        model = hicgat.GATNetHeadsChangedLeakyReLU().to(DEV)
        _, hist = tr.train(model, data, truth, steps=4, graph=graph, attn_dropout=0.5)
        assert model.conv.dropout == 0.5 and model.conv._dropout_state.step == 4
        assert model.conv._dropout_state.seed == 21
        return hist, [p.detach().clone() for p in model.parameters()]

    eager, replayed = run(False), run(True)
    assert eager[0] == replayed[0], (eager[0], replayed[0])
    assert len(set(eager[0])) == 4
    assert all(torch.equal(a, b) for a, b in zip(eager[1], replayed[1]))
    torch.manual_seed(21)
    model = hicgat.GATNetHeadsChangedLeakyReLU().to(DEV)
    _, plain = tr.train(model, data, truth, steps=2, graph=False)
    assert plain != eager[0][:2]                                   # dropout changed the run


# ---------------------------------------------------------------- the C ABI's refusals
def test_c_abi_refusals():
    from hicgat import _lib
    lib, P = _lib.lib(), _lib.ptr
    st = _lib.stream(torch.device(DEV))
    adj = _graph()[0]
    rp, cl = adj.rowptr32, adj.col32
    H, C = 2, 128
    D = H * C
    f = lambda *s: torch.zeros(s, device=DEV)   # noqa: E731
    h, a, b, out, rs, att = f(N, D), f(N, H), f(D), f(N, D), f(N, 4 * H), f(H, C)
    dh, da = f(N, D), f(N, H)
    ctr = torch.zeros(2, dtype=torch.int64, device=DEV)
    odd = ctypes_offset(ctr, 4)

    def graph(r0, r1):
        return _lib.GatGraph(rowptr=rp.data_ptr(), col=cl.data_ptr(), N=N, nnz=cl.numel(), row_begin=r0, row_end=r1)

    def feats(Hh, Cc):
        return _lib.GatFeats(h=h.data_ptr(), a_src=a.data_ptr(), a_dst=a.data_ptr(), H=Hh, C=Cc, neg_slope=0.2)

    def drop(p, step, site):
        return _lib.AttnDrop(p=p, seed=1, step_counter=getattr(step, "value", None), step_value=1, site=site)

    def fwd(p=0.5, site=0, Hh=H, Cc=C, r0=0, r1=N, step=None, outp=P(out)):
        return lib.hicgat_gat_agg_fwd(graph(r0, r1), feats(Hh, Cc), P(b), 0, outp, None, P(rs), drop(p, step, site),
                                      None, st)

    def src(p=0.5, site=0, Hh=H, Cc=C, r0=0, r1=N, step=None, flags=0, ld=4 * H):
        return lib.hicgat_gat_agg_bwd_src(graph(r0, r1), feats(Hh, Cc), P(rs), ld, P(out), D, P(att), P(att), P(dh),
                                          P(da), flags, drop(p, step, site), None, st)

    def mask(p=0.5, site=0, Hh=H, n=N, step=None, m=True):
        buf = torch.zeros((cl.numel(), 4), dtype=torch.uint8, device=DEV)
        return lib.hicgat_gat_attn_mask(P(rp), P(cl), n, Hh, drop(p, step, site), P(buf) if m else None, st)

    for fn in (fwd, src, mask):
        assert fn() == 0
        assert fn(p=0.0) == 0
        for p in (-0.1, 1.0, float("nan")):
            assert fn(p=p) == EINVAL, (fn.__name__, p)
        assert fn(site=(1 << 31) - 1) == 0
        assert fn(site=1 << 31) == EINVAL
        assert fn(step=odd) == EINVAL
    for fn in (fwd, src):
        assert fn(Hh=2, Cc=96) == EUNSUPPORTED
        assert fn(Hh=8, Cc=128) == EUNSUPPORTED
        assert fn(p=1.0, Hh=2, Cc=96) == EINVAL           # the probability is checked before the shape
        assert fn(r0=5, r1=5) == 0                          # empty range: nothing else is looked at
        assert fn(r0=5, r1=4) == EINVAL and fn(r1=N + 1) == EINVAL
    assert fwd(outp=None) == EINVAL
    assert src(flags=2) == EINVAL and src(ld=4 * H + 2) == EINVAL
    assert mask(Hh=5) == EUNSUPPORTED and mask(Hh=0) == EUNSUPPORTED
    assert mask(n=0, m=False) == 0 and mask(m=False) == EINVAL and mask(n=-1) == EINVAL
    torch.cuda.synchronize()


def ctypes_offset(t, nbytes):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + nbytes)

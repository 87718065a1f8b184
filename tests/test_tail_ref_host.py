"""tests/tail_ref.py on the CPU: the fp64 stage reference of the one-kernel MLP tail is right
(against fp64 autograd through the plain-torch tail), its per-stage bound is honest (a plain fp32
evaluation of every stage lies inside it, for every input set tests/test_gpu_tail_stages.py uses)
and sharp enough (each seeded fault leaves it).  The last two are the evidence, without a GPU, that
the GPU test neither fails on a correct kernel nor passes on a subtly wrong one."""
import pytest
import torch

import tail_ref as R

F32, F64 = torch.float32, torch.float64
MS = (1, 15, 16, 17, 47, 2033)
M_PERSIST = 16 * 256 + 1     # the MI355X's 256 CUs: the smallest M on the persistent forward


# ------------------------------------------------- plain torch evaluation of each stage (dtype, fault)
def f_gemm_bias(a, w, b, dt, fault=None):
    a, w, b = a.to(dt), w.to(dt), b.to(dt)
    if fault == "bias":
        b = torch.roll(b, 1)
    y = a @ w.t() + b
    if fault == "dropk":      # one k term of one output column
        k = int(a.abs().sum(0).argmax())
        y[:, 1] = y[:, 1] - a[:, k] * w[1, k]
    return y


def f_heads_fwd(xa, Wh, bh, dt, fault=None):
    return torch.cat([f_gemm_bias(xa[h], Wh[256 * h:256 * h + 256], bh[256 * h:256 * h + 256], dt, fault)
                      for h in range(2)], 1)


def f_ln_fwd(y, gamma, beta, eps, W, res, dt, fault=None):
    y, gamma, beta = y.to(dt), gamma.to(dt), beta.to(dt)
    h = y[:, :W]
    mean = h.sum(1, keepdim=True) / W
    d = h - mean
    var = (d * d).sum(1, keepdim=True) / ((W - 1) if fault == "unbiased" else W)
    rstd = 1.0 / torch.sqrt(var + (0.0 if fault == "noeps" else eps))
    z = torch.relu(d * rstd * gamma + beta)
    if res:
        z = z + y[:, W:2 * W]
    return torch.cat([mean, rstd], 1), z


def f_ln_bwd(dz_in, wt, y, st, gamma, beta, W, res, dt, fault=None):
    dz_in, wt, y, st, gamma, beta = (t.to(dt) for t in (dz_in, wt, y, st, gamma, beta))
    dz = dz_in @ wt
    if fault == "dropk":
        k = int(dz_in.abs().sum(0).argmax())
        dz[:, 1] = dz[:, 1] - dz_in[:, k] * wt[k, 1]
    rstd = st[:, 1:2]
    xh = (y[:, :W] - st[:, 0:1]) * rstd
    pre = xh * gamma + beta
    g = dz * (pre > 0).to(dt)
    dh = g * gamma
    m1 = dh.sum(1, keepdim=True) / W
    m2 = (dh * xh).sum(1, keepdim=True) / W
    dy = rstd * (dh - m1 - xh * m2)
    dY = torch.cat([dy, dz], 1) if res else dy
    M = y.shape[0]
    nt = -(-M // R.TILE)

    def tiles(v):
        return torch.cat([v, torch.zeros((nt * R.TILE - M, W), dtype=dt)]).reshape(nt, R.TILE, W).sum(1)

    p = torch.cat([tiles(g * xh), tiles(g)], 1)
    if fault == "padrow":     # a row past M takes part: it holds what some other row of the tile buffer held
        p[-1] = p[-1] + torch.cat([g[0] * xh[0], g[0]])
    return dY, p


def f_dout(dY1, W1c, y, act, dt, fault=None):
    dx = dY1.to(dt) @ W1c.to(dt)
    if fault == "dropk":
        k = int(dY1.abs().sum(0).argmax())
        dx[:, 1] = dx[:, 1] - dY1[:, k].to(dt) * W1c[k, 1].to(dt)
    if act:
        m = y > 0
        if fault == "wronghead":
            m = torch.roll(m, 256, 1)
        dx = dx * m.to(dt)
    return dx


def _dots(a, b):
    return (a * b).reshape(a.shape[0], 2, 256).sum(2)


def f_rows_stats(dout, y, bias, out2, s3, dt, fault=None):
    d, y, bias, out2, s3 = (t.to(dt) for t in (dout, y, bias, out2, s3))
    if fault == "bias":
        bias = torch.roll(bias, 1)
    if fault == "s3zero":
        s3 = torch.zeros_like(s3)
    delta = _dots(d, y - bias)
    return torch.cat([delta, _dots(d, out2) - delta * s3], 1)


def f_heads_delta(dout, Y0, bh, dt, fault=None):
    bh = bh.to(dt)
    return _dots(dout.to(dt), Y0.to(dt) - (torch.roll(bh, 1) if fault == "bias" else bh))


def f_heads_dxa(dout, Wh, dt, fault=None):
    d, Wh = dout.to(dt), Wh.to(dt)
    o = torch.cat([d[:, 256 * h:256 * h + 256] @ Wh[256 * h:256 * h + 256] for h in range(2)], 1)
    if fault == "dropk":
        k = int(d[:, :256].abs().sum(0).argmax())
        o[:, 1] = o[:, 1] - d[:, k] * Wh[k, 1]
    return o


def _outside(got, ref):
    """Elements of the fp32 ``got`` outside the stage's bound."""
    val, bnd = ref
    return int((~((got.to(F32).double() - val).abs() <= bnd)).sum())


def _inside(got, ref, what):
    val, bnd = ref
    err = (got.double() - val).abs()
    bad = ~(err <= bnd)
    assert not bad.any(), (what, int(bad.sum()), float((err / bnd.clamp_min(1e-300)).max()))
    return float((err / bnd.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------- the stage chains
FWD = (("Y1", "x", "W1c", "b1c"), ("Y2", "z1", "W2c", "b2c"), ("y3", "z2", "W3", "b3"), ("coords", "z3", "W4", "b4"))
LNF = {"Y1": ("st1", "z1", "g1", "be1", 256, True), "Y2": ("st2", "z2", "g2", "be2", 128, True),
       "y3": ("st3", "z3", "g3", "be3", 64, False)}
BWD = (("dy3", "p3", "dc", lambda P: P["W4"], "y3", "st3", "g3", "be3", 64, False),
       ("dY2", "p2", "dy3", lambda P: P["W3"], "Y2", "st2", "g2", "be2", 128, True),
       ("dY1", "p1", "dY2", lambda P: P["W2c"], "Y1", "st1", "g1", "be1", 256, True))


def forward_chain(P, x, dt, eps, heads_xa=None, faults=()):
    """Every forward stage evaluated in ``dt`` by the plain formulas, each from the ``dt`` output of
    the stage before (as the kernel chains them).  faults: {stage name: fault}."""
    faults = dict(faults)
    T = {}
    if heads_xa is not None:
        T["Y0"] = f_heads_fwd(heads_xa, P["Wh"], P["bh"], dt, faults.get("Y0"))
        T["O"] = torch.relu(T["Y0"])
        x = T["O"]
    T["x"] = x.to(dt)
    for out, a, w, b in FWD:
        T[out] = f_gemm_bias(T[a], P[w], P[b], dt, faults.get(out))
        if out in LNF:
            st, z, ga, be, W, res = LNF[out]
            T[st], T[z] = f_ln_fwd(T[out], P[ga], P[be], eps, W, res, dt, faults.get(st))
    return T


def forward_refs(P, T, eps, heads_xa=None):
    """The fp64 (value, bound) of every forward stage from the inputs in T (a chain's tensors)."""
    ref = {}
    if heads_xa is not None:
        ref["Y0"] = R.heads_fwd(heads_xa, P["Wh"], P["bh"])
        ref["O"] = (torch.relu(ref["Y0"][0]), ref["Y0"][1])
    for out, a, w, b in FWD:
        ref[out] = R.gemm_bias(T[a], P[w], P[b])
        if out in LNF:
            st, z, ga, be, W, res = LNF[out]
            ref[st], ref[z] = R.ln_fwd(T[out], P[ga], P[be], eps, W, res)
    return ref


def backward_chain(P, B, dt, act=1, faults=()):
    faults = dict(faults)
    T = {k: v for k, v in B.items()}
    for dY, p, dzin, wt, y, st, ga, be, W, res in BWD:
        T[dY], T[p] = f_ln_bwd(T[dzin], wt(P), T[y], T[st], P[ga], P[be], W, res, dt, faults.get(dY))
    T["dx"] = f_dout(T["dY1"], P["W1c"], None, 0, dt, faults.get("dx"))
    T["dout"] = f_dout(T["dY1"], P["W1c"], B["y"], act, dt, faults.get("dout"))
    T["rows_rs"] = f_rows_stats(T["dout"], B["y"], P["bh"], B["out2"], B["rs"][:, 4:6], dt, faults.get("rows_rs"))
    T["delta"] = f_heads_delta(T["dout"], B["y"], P["bh"], dt, faults.get("delta"))
    T["moved"] = B["rs"][:, 6:8] if faults.get("moved") == "notmoved" else B["rs"][:, 4:6]
    T["dxa"] = f_heads_dxa(T["dout"], P["Wh"], dt, faults.get("dxa"))
    return T


def backward_refs(P, B, T, act=1):
    ref = {}
    for dY, p, dzin, wt, y, st, ga, be, W, res in BWD:
        s = R.ln_bwd(T[dzin], wt(P), B[y], B[st], P[ga], P[be], W, res)
        ref[dY], ref[p] = s["dY"], s["p"]
    ref["dx"] = R.gemm_t(T["dY1"], P["W1c"])
    ref["dout"] = R.dout_stage(T["dY1"], P["W1c"], B["y"], act)
    ref["rows_rs"] = R.rows_stats(T["dout"], B["y"], P["bh"], B["out2"], B["rs"][:, 4:6])
    ref["delta"] = R.heads_delta(T["dout"], B["y"], P["bh"])
    ref["moved"] = R.heads_moved(B["rs"])
    ref["dxa"] = R.heads_dxa(T["dout"], P["Wh"])
    return ref


# ------------------------------------------------------------------------- the reference is right
def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def test_chained_fp64_stages_equal_fp64_autograd():
    """M = 47: the stage functions chained in fp64 (every stage fed the fp64 value of the one before)
    against fp64 autograd through cpu_kernels.torch_tail's post_act: coords, dx and every tail
    parameter's gradient rebuilt from dY1, dY2, dy3, dc and the LayerNorm partials, to 1e-12."""
    import hicgat
    from cpu_kernels import torch_tail
    M, eps = 47, 1e-5
    P, x, _ = R.forward_inputs(M)
    dc = torch.randn(M, 3, generator=torch.Generator().manual_seed(3)).double()
    cls = hicgat.GATNetSelectiveResidualsUpdated
    saved = (cls.post_act, cls.tail)
    try:
        torch_tail(hicgat)
        model = cls().double()
        with torch.no_grad():
            for lin, w, b, lo, hi in (("densea", "W1c", "b1c", 0, 256), ("align_densea", "W1c", "b1c", 256, 512),
                                      ("dense1", "W2c", "b2c", 0, 128), ("align_dense1", "W2c", "b2c", 128, 256),
                                      ("dense2", "W3", "b3", 0, 64), ("dense3", "W4", "b4", 0, 3)):
                getattr(model, lin).weight.copy_(P[w][lo:hi])
                getattr(model, lin).bias.copy_(P[b][lo:hi])
            for ln, ga, be in (("norm_a", "g1", "be1"), ("norm1", "g2", "be2"), ("norm2", "g3", "be3")):
                getattr(model, ln).weight.copy_(P[ga])
                getattr(model, ln).bias.copy_(P[be])
        xg = x.double().requires_grad_(True)
        coords = model.post_act(xg)
        (coords * dc).sum().backward()
    finally:
        cls.post_act, cls.tail = saved
    Pd = {k: v.double() for k, v in P.items()}
    T = {"x": x.double()}
    for out, a, w, b in FWD:
        T[out] = R.gemm_bias(T[a], Pd[w], Pd[b])[0]
        if out in LNF:
            st, z, ga, be, W, res = LNF[out]
            (T[st], _), (T[z], _) = R.ln_fwd(T[out], Pd[ga], Pd[be], eps, W, res)
    assert _rel(T["coords"], coords.detach()) < 1e-12
    T["dc"] = dc
    for dY, p, dzin, wt, y, st, ga, be, W, res in BWD:
        s = R.ln_bwd(T[dzin], wt(Pd), T[y], T[st], Pd[ga], Pd[be], W, res)
        T[dY], T[p] = s["dY"][0], s["p"][0]
        assert T[p].shape == (3, 2 * W)
    dx = R.gemm_t(T["dY1"], Pd["W1c"])[0]
    assert _rel(dx, xg.grad) < 1e-12
    got = {"W1c": T["dY1"].t() @ T["x"], "b1c": T["dY1"].sum(0), "W2c": T["dY2"].t() @ T["z1"],
           "b2c": T["dY2"].sum(0), "W3": T["dy3"].t() @ T["z2"], "b3": T["dy3"].sum(0),
           "W4": dc.t() @ T["z3"], "b4": dc.sum(0),
           "g1": T["p1"].sum(0)[:256], "be1": T["p1"].sum(0)[256:], "g2": T["p2"].sum(0)[:128],
           "be2": T["p2"].sum(0)[128:], "g3": T["p3"].sum(0)[:64], "be3": T["p3"].sum(0)[64:]}
    m = model
    want = {"W1c": torch.cat([m.densea.weight.grad, m.align_densea.weight.grad]),
            "b1c": torch.cat([m.densea.bias.grad, m.align_densea.bias.grad]),
            "W2c": torch.cat([m.dense1.weight.grad, m.align_dense1.weight.grad]),
            "b2c": torch.cat([m.dense1.bias.grad, m.align_dense1.bias.grad]),
            "W3": m.dense2.weight.grad, "b3": m.dense2.bias.grad, "W4": m.dense3.weight.grad,
            "b4": m.dense3.bias.grad, "g1": m.norm_a.weight.grad, "be1": m.norm_a.bias.grad,
            "g2": m.norm1.weight.grad, "be2": m.norm1.bias.grad, "g3": m.norm2.weight.grad,
            "be3": m.norm2.bias.grad}
    for k in want:
        assert _rel(got[k], want[k]) < 1e-12, k


def test_epilogue_formulas_equal_the_cpu_stand_ins():
    """The two epilogues' fp64 stages against the independent statements of the same contracts in
    cpu_kernels (agg_bwd_rows, xagg_rows_bwd), to fp32 rounding of their outputs."""
    from cpu_kernels import CpuKernels
    P, B = R.backward_inputs(47)
    K = CpuKernels()
    g = torch.randn(47, 512, generator=torch.Generator().manual_seed(9))
    for act in (0, 1):
        dout = g * (B["y"] > 0) if act else g
        rs = B["rs"].clone()
        K.agg_bwd_rows(0, 47, act, g, B["y"], P["bh"], B["out2"], torch.empty(47, 512), rs)
        assert _rel(R.rows_stats(dout, B["y"], P["bh"], B["out2"], B["rs"][:, 4:6])[0], rs[:, 4:8]) < 1e-6
        assert torch.equal(rs[:, :4], B["rs"][:, :4])
        rs = B["rs"].clone()
        K.xagg_rows_bwd(act, g, B["y"], P["bh"], torch.empty(47, 512), rs)
        assert _rel(R.heads_delta(dout, B["y"], P["bh"])[0], rs[:, 4:6]) < 1e-6
        assert torch.equal(R.heads_moved(B["rs"])[0].float(), rs[:, 6:8])


# ---------------------------------------------------------------------------- the bound is honest
@pytest.mark.parametrize("M,small", [(m, False) for m in MS + (M_PERSIST,)] + [(47, True)])
def test_fp32_forward_stages_lie_inside_the_bound(M, small):
    P, x, X4 = R.forward_inputs(M, small)
    forms = [None] if (small or M == M_PERSIST) else [None, X4[:, 0, :M]]
    for xa in forms:
        T = forward_chain(P, x, F32, R.EPS32, heads_xa=xa)
        ref = forward_refs(P, T, R.EPS32, heads_xa=xa)
        for k, r in ref.items():
            _inside(T[k], r, (M, small, xa is not None, k))


@pytest.mark.parametrize("M,zero_row", [(m, False) for m in MS] + [(47, True)])
def test_fp32_backward_stages_lie_inside_the_bound(M, zero_row):
    P, B = R.backward_inputs(M, zero_row)
    for act in (0, 1):
        T = backward_chain(P, B, F32, act)
        ref = backward_refs(P, B, T, act)
        for k, r in ref.items():
            _inside(T[k], r, (M, zero_row, act, k))


def test_backward_inputs_keep_pre_off_the_kink():
    """|pre| >= 1e-4 in fp64 everywhere, except the zero row's four exact zeros per LayerNorm, whose
    gradient is 0 (torch's relu backward at 0)."""
    for M, zero_row in [(m, False) for m in MS] + [(47, True)]:
        P, B = R.backward_inputs(M, zero_row)
        for dY, p, dzin, wt, y, st, ga, be, W, res in BWD:
            s = R.ln_bwd(torch.ones(M, wt(P).shape[0]), wt(P), B[y], B[st], P[ga], P[be], W, res)
            pre = s["pre"]
            zero = pre == 0
            assert int(zero.sum()) == (4 if zero_row else 0)
            assert float(pre[~zero].abs().min()) >= 0.99 * R.PRE_MIN
            if zero_row:
                assert zero[M - 1].sum() == 4
                row = pre[M - 1].clone().requires_grad_(True)
                torch.relu(row).sum().backward()
                assert (row.grad[zero[M - 1]] == 0).all()      # torch's relu masks at exactly 0, as [pre > 0] does


# ----------------------------------------------------------------------- the bound is sharp enough
FWD_FAULTS = ([(s, "dropk") for s in ("Y0", "Y1", "Y2", "y3", "coords")]
              + [(s, "bias") for s in ("Y0", "Y1", "Y2", "y3", "coords")]
              + [(s, "unbiased") for s in ("st1", "st2", "st3")])


@pytest.mark.parametrize("stage,fault", FWD_FAULTS)
def test_seeded_forward_fault_leaves_the_bound(stage, fault):
    M = 47
    P, x, X4 = R.forward_inputs(M)
    xa = X4[:, 0, :M]
    T = forward_chain(P, x, F64, R.EPS32, heads_xa=xa, faults={stage: fault})
    ref = forward_refs(P, T, R.EPS32, heads_xa=xa)
    hit = [stage] if stage[:2] != "st" else [stage, "z" + stage[2]]
    for k in hit:
        assert _outside(T[k], ref[k]) > 0, (stage, fault, k)
    for k in ref:       # and only the faulted stage: every later stage sees the faulted input and agrees
        if k not in hit and not (stage == "Y0" and k == "O"):
            assert _outside(T[k], ref[k]) == 0, (stage, fault, k)


def test_eps_left_out_is_caught_on_the_small_scale_inputs_only():
    """eps = 1e-5 is of the order of the first LayerNorm's row variance only when x is scaled by
    1e-3 with b1c = 0: there a kernel that leaves eps out of the square root leaves the bound (st1 and
    z1); on the unit-scale inputs eps changes rstd by less than the bound, which is why the GPU test
    has the small-scale set."""
    M = 47
    for small in (True, False):
        P, x, _ = R.forward_inputs(M, small)
        T = forward_chain(P, x, F64, R.EPS32, faults={"st1": "noeps"})
        ref = forward_refs(P, T, R.EPS32)
        var = T["Y1"][:, :256].var(1, unbiased=False)
        if small:
            assert 1e-7 < float(var.min()) and float(var.max()) < 1e-4      # eps = 1e-5 is comparable
            assert _outside(T["st1"], ref["st1"]) > 0 and _outside(T["z1"], ref["z1"]) > 0
        else:
            assert float(var.min()) > 1e3 * R.EPS32
            assert _outside(T["st1"], ref["st1"]) == 0 and _outside(T["z1"], ref["z1"]) == 0


BWD_FAULTS = ([(s, "dropk") for s in ("dy3", "dY2", "dY1", "dx", "dout", "dxa")]
              + [("dy3", "padrow"), ("dY2", "padrow"), ("dY1", "padrow"), ("moved", "notmoved"),
                 ("rows_rs", "s3zero"), ("dout", "wronghead"), ("rows_rs", "bias"), ("delta", "bias")])


@pytest.mark.parametrize("stage,fault", BWD_FAULTS)
def test_seeded_backward_fault_leaves_the_bound(stage, fault):
    P, B = R.backward_inputs(47)
    T = backward_chain(P, B, F64, 1, faults={stage: fault})
    ref = backward_refs(P, B, T, 1)
    hit = {"dy3": "p3", "dY2": "p2", "dY1": "p1"}[stage] if fault == "padrow" else stage
    assert _outside(T[hit], ref[hit]) > 0, (stage, fault)
    if fault == "padrow":       # the partial's last row, nothing else
        val, bnd = ref[hit]
        bad = ~((T[hit].to(F32).double() - val).abs() <= bnd)
        assert not bad[:-1].any()
    for k in ref:
        if k != hit and not (fault == "dropk" and k == {"dy3": "p3", "dY2": "p2", "dY1": "p1"}.get(stage)):
            assert _outside(T[k], ref[k]) == 0, (stage, fault, k)

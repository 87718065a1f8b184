"""tests/xagg_ref.py on the CPU (no GPU): the float64 restatements that tests/test_gpu_xagg_edges.py holds
the aggregate-first GATConv kernels to are chained here in the order of hicgat.dist._step_xagg and tied to
float64 torch autograd through an independently written h-first dense GATConv (1e-10 relative); every
input maker is checked for what its name promises; the tolerance table xagg_ref.TOL is measured (8 x the
sequential-fp32 rendition's error over the condition bound, floor 2^-22); and every seeded fault,
applied to the reference output, fails the GPU file's comparison at that tolerance."""
import functools

import numpy as np
import pytest
import torch

import xagg_ref as R

R0, R1 = R.DEGREES_RANGE
ROWS = R1 - R0


# ------------------------------------------------------------------------------- 1. the autograd tie
def _dense_gat(x, W, att_s, att_d, bias, mask, rows, g):
    """h-first dense GATConv (PyG 1.7.2 forward: h = x W^T, alpha = softmax over the neighbours of
    leaky_relu(a_src_j + a_dst_i) with 1e-16 in the denominator, out = sum alpha h_j + b) for the
    destination rows ``rows``; loss = <g, relu(out)>."""
    h = (x @ W.t()).view(-1, 2, 256)
    a_s, a_d = (h * att_s.view(1, 2, 256)).sum(-1), (h * att_d.view(1, 2, 256)).sum(-1)
    e = torch.nn.functional.leaky_relu(a_s[None, :, :] + a_d[rows][:, None, :], R.NS)      # [rows, N, 2]
    mk = mask[:, :, None]
    e = torch.where(mk, e, torch.zeros_like(e))
    mx = torch.where(mk, e, torch.full_like(e, -1e300)).amax(1, keepdim=True)
    mx = torch.where(mk.any(1, keepdim=True), mx, torch.zeros_like(mx)).detach()
    ex = torch.exp(torch.where(mk, e - mx, torch.zeros_like(e))) * mk
    alpha = ex / (ex.sum(1, keepdim=True) + R.EPS)
    out = torch.einsum("inh,nhc->ihc", alpha, h).reshape(len(rows), 512) + bias
    return out, (g * torch.relu(out)).sum()


@functools.lru_cache(maxsize=None)
def _chain():
    rng = np.random.default_rng(77)
    n = R.N_GATHER
    rp, col = R.shard_csr(R0, R1)
    x = R.features().astype(np.float64)
    W = rng.standard_normal((512, 512)) / np.sqrt(512)
    att_s, att_d = rng.standard_normal((2, 256)) * 0.3, rng.standard_normal((2, 256)) * 0.3
    bias, g = rng.standard_normal(512) * 0.1, rng.standard_normal((ROWS, 512))
    # the reference functions in the step's order
    v, _ = R.vec_ref(W, att_s, att_d)
    a_src, a_dst, _ = R.logits_ref(x, v)
    fw = R.fwd_ref(rp, col, R0, R1, x, a_src, a_dst)
    y0 = np.concatenate([fw["X4"][h, 0] @ W[256 * h:256 * h + 256].T for h in range(2)], 1)
    y, o = R.bias_relu_ref(y0, bias)
    dout, delta, _ = R.rows_bwd_ref(1, g, y, bias)
    dxa = np.concatenate([dout[:, 256 * h:256 * h + 256] @ W[256 * h:256 * h + 256] for h in range(2)], 1)
    ed = R.edge_ref(rp, col, R0, R1, x, a_src, a_dst, fw["m"], fw["s"], delta, dxa, S3=fw["S3"],
                    xa2=fw["X4"][:, 1])
    srp, perm = R.slab_of(rp, col, R0, R1, n)
    _, _, g_src_slab, _ = R.slab_ref(srp, perm, ed["ds"], x)
    gpart, _ = R.gpart_ref(ed["G"], ed["G_abs"], (ROWS + 1) // 2)
    g_src_acc, _ = R.colsum_ref(gpart)
    g_dst = np.concatenate([R.colsum_ref(x[R0:R1], wt=ed["da_dst"][:, h])[0] for h in range(2)], 1)
    dW0 = np.concatenate([dout[:, 256 * h:256 * h + 256].T @ fw["X4"][h, 0] for h in range(2)])
    # segmented: g_src in 3 parts that add up to it
    parts = rng.standard_normal((3, 1024))
    parts[2] = g_src_slab - parts[0] - parts[1]
    dW, _, datt_s, datt_d, _, _ = R.param_finish_ref(W, att_s, att_d, parts, np.stack([g_dst[0]] + [0 * g_dst[0]] * 2),
                                                     dW0, np.zeros(512), np.zeros(512))
    # autograd
    t = {k: torch.tensor(val, dtype=torch.float64, requires_grad=True)
         for k, val in dict(W=W, att_s=att_s, att_d=att_d, bias=bias).items()}
    mask = np.zeros((ROWS, n), bool)
    for r in range(ROWS):
        mask[r, col[rp[R0 + r]:rp[R0 + r + 1]]] = True
    out, loss = _dense_gat(torch.tensor(x), t["W"], t["att_s"], t["att_d"], t["bias"], torch.tensor(mask),
                           torch.arange(R0, R1), torch.tensor(g))
    loss.backward()
    return dict(ours=dict(out=y, o=o, dW=dW, datt_s=datt_s.reshape(2, 256), datt_d=datt_d.reshape(2, 256),
                          dbias=dout.sum(0)),
                auto=dict(out=out.detach().numpy(), o=torch.relu(out).detach().numpy(), dW=t["W"].grad.numpy(),
                          datt_s=t["att_s"].grad.numpy(), datt_d=t["att_d"].grad.numpy(), dbias=t["bias"].grad.numpy()),
                g_src=(g_src_slab, g_src_acc[0]))


@pytest.mark.parametrize("what", ["out", "o", "dW", "datt_s", "datt_d", "dbias"])
def test_chain_equals_float64_autograd(what):
    c = _chain()
    a, b = c["ours"][what], c["auto"][what]
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-10 * np.abs(b).max(), (what, np.abs(a - b).max(), np.abs(b).max())


def test_slab_route_equals_edge_acc_route():
    slab, acc = _chain()["g_src"]
    assert np.abs(slab - acc).max() <= 1e-12 * np.abs(slab).max()


# ------------------------------------------------------------------------------- 2. the input makers
def test_gather_graph_degrees_and_columns():
    rp, col = R.gather_graph()
    assert rp.dtype == np.int32 and col.dtype == np.int32 and len(rp) == R.N_GATHER + 1 and rp[-1] == len(col)
    deg = np.diff(rp)
    assert all(deg[i] == R.degree_of(i) for i in range(R.N_GATHER))
    assert set(deg.tolist()) == set(R.DEGREES)
    assert sorted(deg[R0:R1].tolist()) == sorted(R.DEGREES)
    for i in range(R.N_GATHER):
        c = col[rp[i]:rp[i + 1]]
        assert np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] >= 0 and c[-1] < R.N_GATHER))
    for name, (a, b) in R.row_ranges().items():
        srp, scol = R.shard_csr(a, b)
        assert srp.dtype == np.int32 and srp[a] == 0 and srp[b] == len(scol) and len(srp) == R.N_GATHER + 1
        assert np.array_equal(np.diff(srp)[a:b], deg[a:b]) and np.all(np.diff(srp)[:a] == 0) and np.all(np.diff(srp)[b:] == 0)
    shard_rows = sorted({b - a for k, (a, b) in R.row_ranges().items() if k not in ("whole", "degrees")})
    assert shard_rows == [1, 2, 3, 7, 8, 9, 17]
    # the shards hold rows on both sides of one 64-entry chunk, of 256 entries and rows of > 1000
    assert max(deg[R.MID:R.MID + 17]) >= 1023 and max(deg[:17]) == 1025 and deg[0] == 0


def test_boundary_entries_hold_the_row_maximum():
    rp, col = R.gather_graph()
    a_src, a_dst = R.logits("boundary")
    hot = R.hot_nodes()
    assert a_src[hot].min() - a_src[~hot].max() >= 3.0
    for i in range(R.N_GATHER):
        c = col[rp[i]:rp[i + 1]]
        want = sorted({p for p in R.BOUNDARY if p < len(c)} | ({len(c) - 1} if len(c) else set()))
        assert np.flatnonzero(hot[c]).tolist() == want, i
    fw = R.fwd_ref(*R.shard_csr(R0, R1), R0, R1, R.features(), a_src, a_dst)
    srp, scol = R.shard_csr(R0, R1)
    for r in range(ROWS):
        al = fw["alpha"][srp[R0 + r]:srp[R0 + r + 1]]
        h = hot[scol[srp[R0 + r]:srp[R0 + r + 1]]]
        if len(al) and not h.all():
            assert al[h].min() > 7 * al[~h].max()       # a_dst in (-2, 2): a hot e is >= 2, lrelu gap >= 2, e^2 > 7
    e = a_src[scol] + np.repeat(a_dst[R0:R1], np.diff(srp)[R0:R1], 0)
    assert (e > 0).any() and (e < 0).any()


def test_extreme_logits_underflow_without_nan():
    a_src, a_dst = R.logits("extreme")
    rp, col = R.shard_csr(R0, R1)
    f32 = R.fwd_ref(rp, col, R0, R1, R.features(), a_src, a_dst, dt=np.float32)
    f64 = R.fwd_ref(rp, col, R0, R1, R.features(), a_src, a_dst)
    assert np.isfinite(f32["alpha"]).all() and np.isfinite(f32["X4"]).all() and np.isfinite(f64["X4"]).all()
    assert (f32["alpha"][:, 0] == 0).any() and (f64["alpha"] > 0).all()           # fp32 expf underflow only
    deg = np.diff(rp)[R0:R1]
    big = deg >= 2
    first = f64["alpha"][rp[R0:R1][big]]
    assert np.allclose(first[:, 1], 1.0 / deg[big], rtol=1e-12)                    # all logits equal: head 1
    assert max(f64["alpha"][rp[R0 + r]:rp[R0 + r + 1], 0].max() for r in range(ROWS) if deg[r] > 16) > 0.999
    assert np.abs(a_src[:, 0]).max() > 55 and np.abs(a_dst).max() > 55


def test_kink_logits_are_exactly_zero():
    a_src, a_dst = R.logits("kink")
    rp, col = R.gather_graph()
    assert (np.signbit(a_src) & (a_src == 0)).any() and ((a_src == 0) & ~np.signbit(a_src)).any()
    assert (np.signbit(a_dst) & (a_dst == 0)).any()
    deg = np.diff(rp)
    for i in range(R.N_GATHER):
        e = a_src[col[rp[i]:rp[i + 1]]] + a_dst[i]
        assert deg[i] == 0 or ((e == 0).any(0).all() and np.array_equal(e, np.float64(a_src[col[rp[i]:rp[i + 1]]]) + a_dst[i]))
    neg_zero = sum(int((np.signbit(e) & (e == 0)).sum()) for e in
                   (a_src[col[rp[i]:rp[i + 1]]] + a_dst[i] for i in range(R0, R1)))
    assert neg_zero > 0


def test_row_inputs_hold_signed_zeros():
    for rows in (1, 3, 9):
        y0 = R.row_inputs(rows)["y0"]
        assert ((y0 == 0) & ~np.signbit(y0)).any() and ((y0 == 0) & np.signbit(y0)).any()


@pytest.mark.parametrize("n", R.SLAB_N)
def test_slab_inputs(n):
    srp, perm, ds, x = R.slab_inputs(n)
    assert srp.dtype == np.int32 and perm.dtype == np.int32 and len(srp) == n + 1 and srp[-1] == len(perm) == len(ds)
    assert np.array_equal(np.sort(perm), np.arange(len(perm)))
    cnt = set(np.diff(srp).tolist())
    assert cnt <= set(R.SLAB_ROW_ENTRIES) and (n < 6 or cnt == set(R.SLAB_ROW_ENTRIES))
    assert x.shape == (n, 512)
    assert set().union(*(set(np.diff(R.slab_inputs(k)[0]).tolist()) for k in (1, 3, 4, 5))) >= {0, 1, 15, 16, 17, 33} - {16}


def _add_col_lg(rows, segs, weighted):
    """csrc/gemm.hip add_col, restated: lanes per row group by the rows of one segment."""
    srows = (rows + segs - 1) // segs
    if srows <= 16:
        return 8
    if srows <= 64:
        return 6
    if srows <= 256:
        return 4
    return 1 if (weighted and srows > 1024) else 2


def test_colsum_cases_select_their_form():
    seen = set()
    for name, (rows, cols, segs, ldp, lddp, weighted, lg) in R.COLSUM_CASES.items():
        assert _add_col_lg(rows, segs, weighted) == lg == R.colsum_lg(rows, segs, weighted), name
        assert rows >= segs or rows == 0
        seen.add((lg, weighted))
        src, wt, dst0 = R.colsum_inputs(name)
        assert src.shape == (rows, cols) and dst0.shape == (segs, cols) and (wt is not None) == weighted
    per_seg = {(-(-r // s), w) for r, c, s, _, _, w, _ in R.COLSUM_CASES.values()}
    assert {(1, False), (16, False), (17, False), (64, False), (65, False), (256, False), (257, False),
            (1024, True), (1025, True)} <= per_seg
    assert {8, 6, 4, 2, 1} == {lg for lg, _ in seen}
    assert {s for _, _, s, *_ in R.COLSUM_CASES.values()} == {1, 2, 3, 7}
    assert {c for _, c, *_ in R.COLSUM_CASES.values()} == {1, 3, 4, 5, 512, 1024, 1027}
    assert any(r == s for r, _, s, *_ in R.COLSUM_CASES.values())
    assert any((c + p) % 2 == 1 and p > 0 for _, c, _, p, *_ in R.COLSUM_CASES.values())


# ------------------------------------------------------------------------------- 3. the tolerance
def _stage_inputs(family):
    """The fp32 inputs of every gather stage on the 34 all-degree rows, as the GPU file feeds them."""
    rp, col = R.shard_csr(R0, R1)
    a_src, a_dst = R.logits(family)
    x, ri = R.features(), R.row_inputs(ROWS)
    fw = R.fwd_ref(rp, col, R0, R1, x, a_src, a_dst)
    _, delta, _ = R.rows_bwd_ref(1, ri["g"], ri["y0"], ri["bias"])
    st = dict(m=fw["m"].astype(np.float32), s=fw["s"].astype(np.float32), S3=fw["S3"].astype(np.float32),
              delta=delta.astype(np.float32), xa2=fw["X4"][:, 1].astype(np.float32))
    return rp, col, a_src, a_dst, x, ri, st


@functools.lru_cache(maxsize=None)
def _measured():
    """quantity -> largest (sequential fp32 - float64) / bound over the cases."""
    worst = {k: 0.0 for k in R.TOL}
    family = None

    def note(k, got, ref, bound):
        k = k if family is None else f"{k}/{family}"
        worst[k] = max(worst[k], R.worst(got, ref, bound)[0])

    rng = np.random.default_rng(9)
    W = (rng.standard_normal((512, 512)) / np.sqrt(512)).astype(np.float32)
    att_s, att_d = (rng.standard_normal((2, 256)).astype(np.float32) for _ in range(2))
    v64, va = R.vec_ref(W, att_s, att_d)
    note("vec", R.vec_ref(W, att_s, att_d, np.float32)[0], v64, va)
    v32 = v64.astype(np.float32)
    x = R.features()
    a64 = R.logits_ref(x, v32)
    a32 = R.logits_ref(x, v32, np.float32)
    note("logits", np.concatenate(a32[:2], 1), np.concatenate(a64[:2], 1), a64[2])
    for family in R.FAMILIES:
        rp, col, a_src, a_dst, x, ri, st = _stage_inputs(family)
        f64 = R.fwd_ref(rp, col, R0, R1, x, a_src, a_dst)
        f32 = R.fwd_ref(rp, col, R0, R1, x, a_src, a_dst, dt=np.float32)
        assert R.same_bits(f32["m"].astype(np.float64), f64["m"])
        note("sum", f32["s"], f64["s"], f64["s"])
        note("S3", f32["S3"], f64["S3"], f64["S3"])
        note("X4", f32["X4"], f64["X4"], f64["X4_abs"])
        kw = dict(S3=st["S3"], xa2=st["xa2"])
        e64 = R.edge_ref(rp, col, R0, R1, x, a_src, a_dst, st["m"], st["s"], st["delta"], ri["dxa"], **kw)
        e32 = R.edge_ref(rp, col, R0, R1, x, a_src, a_dst, st["m"], st["s"], st["delta"], ri["dxa"], dt=np.float32, **kw)
        note("ds", e32["ds"], e64["ds"], e64["ds_abs"])
        note("da_dst", e32["da_dst"], e64["da_dst"], e64["da_dst_abs"])
        g64 = R.gpart_ref(e64["G"], e64["G_abs"], (ROWS + 1) // 2)
        note("gpart", R.gpart_ref(e32["G"], e64["G_abs"], (ROWS + 1) // 2, np.float32)[0], g64[0], g64[1])
    family = None
    for rows in (1, 3, 9, 17):
        ri = R.row_inputs(rows)
        for act in (0, 1):
            _, d64, da = R.rows_bwd_ref(act, ri["g"], ri["y0"], ri["bias"])
            note("delta", R.rows_bwd_ref(act, ri["g"], ri["y0"], ri["bias"], np.float32)[1], d64, da)
    for n in R.SLAB_N:
        srp, perm, ds, xs = R.slab_inputs(n)
        da64, daa, g64, ga = R.slab_ref(srp, perm, ds, xs)
        da32, _, g32, _ = R.slab_ref(srp, perm, ds, xs, np.float32)
        note("da_src", da32, da64, daa)
        note("g_src", g32, g64, ga)
    for name, (rows, cols, segs, *_rest) in R.COLSUM_CASES.items():
        src, wt, dst0 = R.colsum_inputs(name)
        w = None if wt is None else wt[:, 6]
        for d0 in (None, dst0):
            ref, bound = R.colsum_ref(src, w, segs, d0)
            note("colsum", R.colsum_ref(src, w, segs, d0, np.float32)[0], ref, bound)
    for segs in (1, 2, 3):
        p = _param_inputs(segs)
        ref = R.param_finish_ref(*p)
        got = R.param_finish_ref(*p, dt=np.float32)
        note("dW", got[0], ref[0], ref[1])
        note("datt", np.stack(got[2:4]), np.stack(ref[2:4]), np.stack(ref[4:6]))
    return worst


def _param_inputs(segs):
    rng = np.random.default_rng(40 + segs)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (f(512, 512), f(2, 256), f(2, 256), f(segs, 1024), f(segs, 1024), f(512, 512), f(512), f(512))


def _round_up_2(v):
    e = np.floor(np.log10(v)) - 1
    return float(np.ceil(v / 10 ** e - 1e-9) * 10 ** e)


def test_tolerance_table():
    """xagg_ref.TOL is 8 x the fp32 rendition's largest error / bound, floor 2^-22, rounded up to two
    digits.  Printed, so the GPU file's docstring can be checked against it."""
    meas = _measured()
    for k, v in meas.items():
        want = _round_up_2(max(8 * v, R.FLOOR))
        print(f"{k:16s} fp32 rendition {v:.3e}  ->  tolerance {want:.1e}  (table {R.TOL[k]:.1e})")
    for k, v in meas.items():
        assert np.isclose(R.TOL[k], _round_up_2(max(8 * v, R.FLOOR)), rtol=1e-6), (k, v, R.TOL[k])


# ------------------------------------------------------------------------------- 4. the seeded faults
@functools.lru_cache(maxsize=None)
def _fault_case(family):
    rp, col, a_src, a_dst, x, ri, st = _stage_inputs(family)
    f = R.fwd_ref(rp, col, R0, R1, x, a_src, a_dst)
    e = R.edge_ref(rp, col, R0, R1, x, a_src, a_dst, st["m"], st["s"], st["delta"], ri["dxa"], S3=st["S3"], xa2=st["xa2"])
    return rp, col, a_src, a_dst, x.astype(np.float64), ri, st, f, e


def _row_of_degree(rp, d):
    deg = np.diff(rp)[R0:R1]
    return int(np.flatnonzero(deg == d)[0])


def _fails(k, got, ref, bound, family="boundary"):
    tol = R.tol(k, family)
    assert R.passes(ref, ref, bound, tol)
    return not R.passes(got, ref, bound, tol)


@pytest.mark.parametrize("deg", [65, 257, 1025])
def test_fault_last_edge_dropped(deg):
    rp, col, _, _, x, _, _, f, e = _fault_case("boundary")
    r = _row_of_degree(rp, deg)
    last = rp[R0 + r + 1] - 1
    X4 = f["X4"].copy()
    X4[:, 0, r] -= f["alpha"][last][:, None] * x[col[last]]
    assert _fails("X4", X4, f["X4"], f["X4_abs"])
    X4 = f["X4"].copy()
    X4[:, 1, r] -= f["q"][last][:, None] * x[col[last]]
    assert _fails("X4", X4, f["X4"], f["X4_abs"])
    S3 = f["S3"].copy()
    S3[r] -= f["q"][last]
    assert _fails("S3", S3, f["S3"], f["S3"])
    s = f["s"].copy()
    s[r] -= np.exp(np.log(f["alpha"][last] * (f["s"][r] + R.EPS)))
    assert _fails("sum", s, f["s"], f["s"])
    ds = e["ds"].copy()
    ds[last] = 0
    assert _fails("ds", ds, e["ds"], e["ds_abs"])
    G = e["G"].copy()
    G[r] -= (e["ds"][last][:, None] * x[col[last]]).reshape(-1)
    nb = (ROWS + 1) // 2
    ref, bound = R.gpart_ref(e["G"], e["G_abs"], nb)
    assert _fails("gpart", R.gpart_ref(G, e["G_abs"], nb)[0], ref, bound)


def test_fault_wave_1_chunk_dropped():
    rp, col, _, _, x, _, _, f, e = _fault_case("boundary")
    for deg in (128, 1025):
        r = _row_of_degree(rp, deg)
        b = rp[R0 + r]
        sl = slice(b + 64, b + 128)
        X4 = f["X4"].copy()
        X4[:, 0, r] -= f["alpha"][sl].T @ x[col[sl]]
        assert _fails("X4", X4, f["X4"], f["X4_abs"])
        G = e["G"].copy()
        G[r] -= (e["ds"][sl].T @ x[col[sl]]).reshape(-1)
        nb = (ROWS + 1) // 2
        ref, bound = R.gpart_ref(e["G"], e["G_abs"], nb)
        assert _fails("gpart", R.gpart_ref(G, e["G_abs"], nb)[0], ref, bound)


@pytest.mark.parametrize("pos", [0, 3, 4, 63, 64, 255, 256])
def test_fault_boundary_edge_counted_twice(pos):
    rp, col, _, _, x, _, _, f, e = _fault_case("boundary")
    r = _row_of_degree(rp, 1025)
    k = rp[R0 + r] + pos
    X4 = f["X4"].copy()
    X4[:, 0, r] += f["alpha"][k][:, None] * x[col[k]]
    assert _fails("X4", X4, f["X4"], f["X4_abs"])
    G = e["G"].copy()
    G[r] += (e["ds"][k][:, None] * x[col[k]]).reshape(-1)
    nb = (ROWS + 1) // 2
    ref, bound = R.gpart_ref(e["G"], e["G_abs"], nb)
    assert _fails("gpart", R.gpart_ref(G, e["G_abs"], nb)[0], ref, bound)


def test_fault_kink_decided_with_ge():
    rp, col, a_src, a_dst, x, ri, st, f, e = _fault_case("kink")
    bad = R.fwd_ref(rp, col, R0, R1, x, a_src, a_dst, ge=True)
    assert R.same_bits(bad["X4"][:, 0], f["X4"][:, 0])          # alpha itself does not see the kink
    assert _fails("X4", bad["X4"], f["X4"], f["X4_abs"], family="kink")
    assert _fails("S3", bad["S3"], f["S3"], f["S3"], family="kink")
    bad = R.edge_ref(rp, col, R0, R1, x, a_src, a_dst, st["m"], st["s"], st["delta"], ri["dxa"], ge=True)
    assert _fails("ds", bad["ds"], e["ds"], e["ds_abs"], family="kink")


def test_fault_head_1_given_head_0_delta():
    rp, col, a_src, a_dst, x, ri, st, f, e = _fault_case("boundary")
    bad = R.edge_ref(rp, col, R0, R1, x, a_src, a_dst, st["m"], st["s"], st["delta"][:, [0, 0]], ri["dxa"],
                     S3=st["S3"], xa2=st["xa2"])
    assert R.same_bits(bad["ds"][:, 0], e["ds"][:, 0])
    assert _fails("ds", bad["ds"], e["ds"], e["ds_abs"])
    assert _fails("da_dst", bad["da_dst"], e["da_dst"], e["da_dst_abs"])


def test_fault_slab_row_17th_entry_dropped():
    srp, perm, ds, x = R.slab_inputs(4097)
    da, daa, g, ga = R.slab_ref(srp, perm, ds, x)
    j = int(np.flatnonzero(np.diff(srp) == 17)[0])
    bad = da.copy()
    bad[j] -= ds[perm[srp[j] + 16]]
    assert _fails("da_src", bad, da, daa)
    assert _fails("g_src", g - np.concatenate([ds[perm[srp[j] + 16]][h] * np.float64(x[j]) for h in range(2)]), g, ga)


def test_fault_colsum_row_given_to_the_next_segment():
    for name in ("r33s2", "r65s3", "w1026s2", "rows_eq_segs"):
        rows, cols, segs, *_ = R.COLSUM_CASES[name]
        src, wt, _ = R.colsum_inputs(name)
        w = None if wt is None else wt[:, 6]
        ref, bound = R.colsum_ref(src, w, segs)
        last = rows * 1 // segs - 1
        t = src[last].astype(np.float64) * (1.0 if w is None else float(w[last]))
        bad = ref.copy()
        bad[0] -= t
        bad[1] += t
        assert _fails("colsum", bad, ref, bound), name


def test_fault_relu_derivative_at_zero():
    ri = R.row_inputs(9)
    dout, delta, da = R.rows_bwd_ref(1, ri["g"], ri["y0"], ri["bias"])
    bad, bdelta, _ = R.rows_bwd_ref(1, ri["g"], ri["y0"], ri["bias"], relu_ge=True)
    assert not R.same_bits(bad.astype(np.float32), dout.astype(np.float32))
    assert np.all(dout[ri["y0"] == 0] == 0) and np.any(bad[ri["y0"] == 0] != 0)
    assert _fails("delta", bdelta, delta, da)

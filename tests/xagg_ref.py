"""Float64 restatements of the aggregate-first GATConv kernels (csrc/gat_xagg.hip; contracts from its
comments and include/hicgat.h) and of the weighted, segmented column sum of hicgat_param_grads_grouped
(csrc/gemm.hip), and the one builder of the inputs that tests/test_gpu_xagg_edges.py (GPU) and
tests/test_xagg_ref_host.py (CPU) share.  The host file ties the chain of these functions to float64
autograd through an h-first dense GATConv; the GPU file compares each kernel with them through the C ABI.

  vec_ref           v [4][512] = W_h^T att_src^h (h = 0, 1), W_h^T att_dst^h
  logits_ref        a_src / a_dst [N][2] = x . v
  fwd_ref           softmax statistics (max, sum, S3) and X4 = (sum alpha x_j, sum alpha lrelu' x_j)
  bias_relu_ref     y = y0 + bias, o = relu(y)
  rows_bwd_ref      dout = g [y0 > 0] (act) or g, delta^h = <dout^h, y0^h - bias^h>
  edge_ref          ds_ij^h = alpha lrelu' (<dxa_i^h, x_j> - delta_i^h), da_dst^h = <dxa_i^h, xa2_i^h> -
                    delta_i^h S3_i^h, and the row's term of g_src, sum_j ds_ij x_j
  gpart_ref         the rows of one workgroup of hicgat_xagg_edge_acc added up (its ``rows b / G`` spans)
  slab_ref          da_src_j = sum of ds over the slab entries of row j, g_src^h = sum_j da_src_j^h x_j
  param_finish_ref  dW += att (x) g, datt += W_h g, with g in segments
  colsum_ref        dst[s][c] (+)= sum over segment s of wt_r src[r][c]

Rules every function keeps:
  * The inputs are taken exactly as the kernel receives them (float32 arrays convert to float64 without
    rounding) and everything after that is float64.  ``dt=np.float32`` evaluates the SAME expressions in
    plain sequential float32 (products rounded, sums left to right): the reference's own fp32 rendition,
    from which the host file measures the tolerances.  Float64 inputs pass through unrounded, which is
    what lets the host file chain the functions against autograd at 1e-10.
  * LeakyReLU's branch ``e > 0`` is decided on the exact sum e = a_src_j + a_dst_i of the two fp32
    logits (exact in float64).  The kernel decides on the fp32 sum, and an fp32 sum of two fp32 numbers
    is zero only when the exact sum is zero (gradual underflow; otherwise it keeps the exact sum's
    sign), so both take the same branch for every entry and no kink handling is needed.  At e = 0 (and
    -0.0) the derivative is the negative slope, as ``x > 0 ? x : x * slope`` gives it.
  * One field is formed in fp32 on purpose: the row maximum of lrelu(e).  A maximum of fp32 numbers has
    one right answer, so with fp32 logits the reference forms e = a_src_j + a_dst_i in fp32 and, where
    e <= 0, the ONE fp32 multiply e * slope, and returns that maximum; the sum and alpha are taken
    relative to it, as the kernels take them.
  * Next to every output element that is a sum, the float64 sum of the absolute values of its terms is
    returned (``*_abs``): errors are judged per element against that condition bound (``ratio``), not
    against the tensor's largest magnitude.

Graphs are explicit CSR with a prescribed degree per row, distinct sorted int32 columns, no Hi-C
synthesis.  Guard elements hold the finite non-zero sentinels SENT32 / SENT_I32.
"""
import functools

import numpy as np

F, H, C = 512, 2, 256
NS = float(np.float32(0.2))        # the negative slope as the kernels receive it (a float argument)
EPS = 1e-16                        # PyG's softmax denominator term; the kernels add 1e-16f
SENT32 = np.float32(-3.0e38)
SENT_I32 = np.int32(-7)
FLOOR = 2.0 ** -22
# An alpha below fp32's normal range (2^-126) may be flushed to zero or lose its low bits: an absolute
# error of up to 2^-126 = FLOOR * 2^-104 in a per-edge weight, which ds's per-edge bound carries as this
# addend to |alpha lrelu'| (it is below 1e-31: only the underflowing entries of the "extreme" logits see it)
TINY_Q = 2.0 ** -104

# Tolerances of the GPU file per compared quantity, as error / condition bound: 8 x the largest ratio of
# the sequential-fp32 rendition over the cases (floor 2^-22), rounded up to two digits.  Measured by
# tests/test_xagg_ref_host.py::test_tolerance_table, which fails when this table is not that.
GATHER_Q = ("sum", "S3", "X4", "ds", "da_dst", "gpart")     # measured per logit family: "X4/boundary", ...
TOL = {
    "vec": 1.2e-6, "logits": 1.8e-6, "delta": 7.6e-7, "da_src": 1.3e-6, "g_src": 9.5e-7, "colsum": 1.5e-6,
    "dW": 1.4e-6, "datt": 1.2e-6,
    "sum/boundary": 8.7e-6, "sum/extreme": 6.2e-5, "sum/kink": 3.1e-5,
    "S3/boundary": 1.1e-5, "S3/extreme": 7.1e-5, "S3/kink": 3.4e-5,
    "X4/boundary": 8.4e-6, "X4/extreme": 2.0e-5, "X4/kink": 6.5e-6,
    "ds/boundary": 1.9e-6, "ds/extreme": 7.3e-6, "ds/kink": 1.9e-6,
    "da_dst/boundary": 7.9e-7, "da_dst/extreme": 6.0e-7, "da_dst/kink": 6.4e-7,
    "gpart/boundary": 7.3e-7, "gpart/extreme": 3.8e-6, "gpart/kink": 3.3e-7,
}


def tol(quantity, family=None):
    return TOL[f"{quantity}/{family}" if quantity in GATHER_Q else quantity]


# ------------------------------------------------------------------------------- comparison
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


def ratio(got, ref, bound):
    """Per element |got - ref| / bound; 0 where both the error and the bound are 0, inf where only the
    bound is (or where ``got`` is not finite)."""
    got, ref, bound = (np.asarray(t, np.float64) for t in (got, ref, bound))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), r, np.inf)


def worst(got, ref, bound):
    """(largest ratio, its index)."""
    r = ratio(got, ref, bound)
    if r.size == 0:
        return 0.0, ()
    k = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[k]), tuple(int(t) for t in k)


def passes(got, ref, bound, tol):
    """The one comparison of the GPU file: every element within ``tol`` of its condition bound."""
    return worst(got, ref, bound)[0] <= tol


# ------------------------------------------------------------------------------- sums in dt
def _f(a, dt):
    return np.asarray(a).astype(dt, copy=False)


def _sum(a, axis, dt):
    """Sum along ``axis``: float64 by numpy's sum, float32 strictly left to right."""
    a = np.asarray(a, dt)
    if dt == np.float64 or a.shape[axis] == 0:
        return a.sum(axis, dtype=dt)
    return np.take(np.cumsum(a, axis=axis, dtype=dt), -1, axis=axis)


def _wsum(w, xj, dt):
    """[k, d] weights, [d, n] rows -> [k, n] = sum_d w[k, d] xj[d, :]."""
    if dt == np.float64:
        return np.asarray(w, dt) @ xj
    return np.stack([_sum(w[k][:, None] * xj, 0, dt) for k in range(w.shape[0])])


def xcd_remap(bid, nblocks):
    """common.hpp xcd_remap: workgroup ``bid`` of ``nblocks`` takes this logical block."""
    xcd, q, r = bid & 7, nblocks >> 3, nblocks & 7
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + (bid >> 3)


# ------------------------------------------------------------------------------- the kernels
def vec_ref(W, att_s, att_d, dt=np.float64):
    """(v [4, 512], v_abs): rows att_src head 0, 1, att_dst head 0, 1."""
    W, att = _f(W, dt), (_f(att_s, dt).reshape(2, 256), _f(att_d, dt).reshape(2, 256))
    v = np.concatenate([_wsum(att[k][h][None], W[256 * h:256 * h + 256], dt) for k in range(2) for h in range(2)])
    va = np.concatenate([np.abs(np.float64(att[k][h]))[None] @ np.abs(np.float64(W[256 * h:256 * h + 256]))
                         for k in range(2) for h in range(2)])
    return v, va


def logits_ref(x, v, dt=np.float64):
    """(a_src [N, 2], a_dst [N, 2], abs [N, 4])."""
    x, v = _f(x, dt), _f(v, dt)
    a = x @ v.T if dt == np.float64 else _sum(x[:, None, :] * v[None], 2, dt)
    return a[:, :2], a[:, 2:], np.abs(np.float64(x)) @ np.abs(np.float64(v)).T


def _row_logits(a_src, a_dst, i, j, ns, dt, ge=False):
    """Row i's (e > 0, lrelu(e) in dt, fp32 row maximum or None)."""
    e = _f(a_src[j], dt) + _f(a_dst[i], dt)
    pos = e >= 0 if ge else e > 0                      # ge: a seeded fault for the host file only
    l = np.where(pos, e, e * dt(ns))
    m32 = None
    if a_src.dtype == np.float32 and a_dst.dtype == np.float32 and len(j):
        e32 = a_src[j] + a_dst[i]                       # fp32 add
        m32 = np.where(e32 > 0, e32, e32 * np.float32(ns)).max(0)     # the one fp32 multiply
    return pos, l, m32


def fwd_ref(rowptr, col, r0, r1, x, a_src, a_dst, ns=NS, dt=np.float64, ge=False):
    """hicgat_xagg_fwd over own rows [r0, r1) (rowptr indexed by the global row, rowptr[r0] = 0).
    Returns a dict: X4 [2, 2, rows, 512] (+ X4_abs), m, s, S3 [rows, 2] (s and S3 are sums of positive
    terms: their own bound), and per edge alpha and q = alpha lrelu' [nnz, 2]."""
    rows, x = r1 - r0, _f(x, dt)
    X4, X4a = np.zeros((2, 2, rows, F), dt), np.zeros((2, 2, rows, F))
    m, s, S3 = np.full((rows, 2), -np.inf, dt), np.zeros((rows, 2), dt), np.zeros((rows, 2), dt)
    al_all, q_all = np.zeros((int(rowptr[r1]), 2), dt), np.zeros((int(rowptr[r1]), 2), dt)
    for r in range(rows):
        b, e = int(rowptr[r0 + r]), int(rowptr[r0 + r + 1])
        if e == b:
            continue
        j = col[b:e]
        pos, l, m32 = _row_logits(a_src, a_dst, r0 + r, j, ns, dt, ge)
        m[r] = l.max(0) if m32 is None else m32.astype(dt)
        ex = np.exp(l - m[r])
        s[r] = _sum(ex, 0, dt)
        al = ex / (s[r] + dt(EPS))
        q = al * np.where(pos, dt(1), dt(ns))
        S3[r] = _sum(q, 0, dt)
        xj = x[j]
        X4[:, 0, r], X4[:, 1, r] = _wsum(al.T, xj, dt), _wsum(q.T, xj, dt)
        xja = np.abs(np.float64(xj))
        X4a[:, 0, r], X4a[:, 1, r] = np.float64(al).T @ xja, np.float64(q).T @ xja
        al_all[b:e], q_all[b:e] = al, q
    return dict(X4=X4, X4_abs=X4a, m=m, s=s, S3=S3, alpha=al_all, q=q_all)


def bias_relu_ref(y0, bias, dt=np.float64):
    """(y, o).  One addition per element: with fp32 inputs float32(y) is what the kernel must store,
    bit for bit (relu as torch.relu: y <= 0 -> +0.0)."""
    y = _f(y0, dt) + _f(bias, dt)
    return y, np.where(y <= 0, dt(0), y)


def rows_bwd_ref(act, g, y0, bias, dt=np.float64, relu_ge=False):
    """(dout [rows, 512], delta [rows, 2], delta_abs).  dout is a selection: exact."""
    g, y0, bias = _f(g, dt), _f(y0, dt), _f(bias, dt)
    zero = (y0 < 0) if relu_ge else (y0 <= 0)           # relu_ge: a seeded fault for the host file only
    dout = np.where(zero, dt(0), g) if act else g.copy()
    t = (dout * (y0 - bias)).reshape(-1, 2, 256)
    ta = (np.abs(np.float64(dout)) * (np.abs(np.float64(y0)) + np.abs(np.float64(bias)))).reshape(-1, 2, 256)
    return dout, _sum(t, 2, dt), ta.sum(2)


def edge_ref(rowptr, col, r0, r1, x, a_src, a_dst, m, s, delta, dxa, ns=NS, S3=None, xa2=None, dt=np.float64,
             ge=False):
    """hicgat_xagg_edge / hicgat_xagg_edge_acc over own rows: m, s, delta (and S3) [rows, 2] are the
    row_stats fields the kernel reads, dxa [rows, 1024], xa2 [2, rows, 512] (X4's kind-1 planes).
    Returns ds [nnz, 2], the rows' g_src terms G [rows, 1024] = sum_j ds_ij x_j (head 0 | head 1),
    da_dst [rows, 2] (with xa2), each with its bound."""
    rows, x, dxa = r1 - r0, _f(x, dt), _f(dxa, dt)
    m, s, delta = _f(m, dt), _f(s, dt), _f(delta, dt)
    nnz = int(rowptr[r1])
    ds, dsa = np.zeros((nnz, 2), dt), np.zeros((nnz, 2))
    G, Ga = np.zeros((rows, 2 * F), dt), np.zeros((rows, 2 * F))
    for r in range(rows):
        b, e = int(rowptr[r0 + r]), int(rowptr[r0 + r + 1])
        if e == b:
            continue
        j = col[b:e]
        pos, l, _ = _row_logits(a_src, a_dst, r0 + r, j, ns, dt, ge)
        q = np.exp(l - m[r]) / (s[r] + dt(EPS)) * np.where(pos, dt(1), dt(ns))
        xj, d2 = x[j], dxa[r].reshape(2, F)
        dot = xj @ d2.T if dt == np.float64 else _sum(xj[:, None, :] * d2[None], 2, dt)
        ds[b:e] = q * (dot - delta[r])
        xja = np.abs(np.float64(xj))
        dsa[b:e] = (np.abs(np.float64(q)) + TINY_Q) * (xja @ np.abs(np.float64(d2)).T + np.abs(np.float64(delta[r])))
        G[r] = _wsum(ds[b:e].T, xj, dt).reshape(-1)
        Ga[r] = (dsa[b:e].T @ xja).reshape(-1)
    out = dict(ds=ds, ds_abs=dsa, G=G, G_abs=Ga)
    if xa2 is not None:
        xa2, S3 = _f(xa2, dt), _f(S3, dt)
        d3 = dxa.reshape(rows, 2, F).transpose(1, 0, 2)
        out["da_dst"] = (_sum(d3 * xa2, 2, dt) - delta.T * S3.T).T
        out["da_dst_abs"] = (np.abs(np.float64(d3 * xa2)).sum(2) + np.abs(np.float64(delta.T * S3.T))).T
    return out


def edge_acc_spans(rows, nblocks):
    """Own local rows [rb, re) whose terms workgroup ``bid`` of hicgat_xagg_edge_acc writes to gpart[bid]."""
    out = []
    for bid in range(nblocks):
        b = xcd_remap(bid, nblocks)
        out.append((rows * b // nblocks, rows * (b + 1) // nblocks))
    return out


def gpart_ref(G, G_abs, nblocks, dt=np.float64):
    """(gpart [nblocks, 1024], bound) from edge_ref's per-row terms."""
    spans = edge_acc_spans(G.shape[0], nblocks)
    return (np.stack([_sum(G[a:b], 0, dt) for a, b in spans]), np.stack([G_abs[a:b].sum(0) for a, b in spans]))


def slab_ref(rowptr_s, perm, ds, x, dt=np.float64, ds_abs=None):
    """hicgat_xagg_slab_sum: (da_src [N, 2], da_abs, g_src [1024], g_abs).  ``ds_abs``: the bound of
    ds itself when ds is a computed quantity (default |ds|: ds given exactly)."""
    n, ds, x = len(rowptr_s) - 1, _f(ds, dt), _f(x, dt)
    dsa = np.abs(np.float64(ds)) if ds_abs is None else ds_abs
    da, daa = np.zeros((n, 2), dt), np.zeros((n, 2))
    for j in range(n):
        k = perm[int(rowptr_s[j]):int(rowptr_s[j + 1])]
        if len(k):
            da[j], daa[j] = _sum(ds[k], 0, dt), dsa[k].sum(0)
    return da, daa, _wsum(da.T, x, dt).reshape(-1), (daa.T @ np.abs(np.float64(x))).reshape(-1)


def param_finish_ref(W, att_s, att_d, g_src, g_dst, dW, datt_s, datt_d, dt=np.float64):
    """hicgat_xagg_param_finish with g_src / g_dst [segs, 1024].  Returns (dW, dW_abs, datt_s, datt_d,
    datt_s_abs, datt_d_abs)."""
    W, dW = _f(W, dt), _f(dW, dt)
    a_s, a_d = _f(att_s, dt).reshape(-1), _f(att_d, dt).reshape(-1)
    gs = _sum(_f(g_src, dt).reshape(-1, 2, F), 0, dt)
    gd = _sum(_f(g_dst, dt).reshape(-1, 2, F), 0, dt)
    gsa = np.abs(np.float64(g_src)).reshape(-1, 2, F).sum(0)
    gda = np.abs(np.float64(g_dst)).reshape(-1, 2, F).sum(0)
    hd = np.arange(512) // 256
    out = dW + (a_s[:, None] * gs[hd] + a_d[:, None] * gd[hd])
    out_abs = np.abs(np.float64(dW)) + np.abs(np.float64(a_s))[:, None] * gsa[hd] + np.abs(np.float64(a_d))[:, None] * gda[hd]
    Wa = np.abs(np.float64(W))
    ds_ = _f(datt_s, dt).reshape(-1) + _sum(W * gs[hd], 1, dt)
    dd_ = _f(datt_d, dt).reshape(-1) + _sum(W * gd[hd], 1, dt)
    return (out, out_abs, ds_, dd_, np.abs(np.float64(datt_s)).reshape(-1) + (Wa * gsa[hd]).sum(1),
            np.abs(np.float64(datt_d)).reshape(-1) + (Wa * gda[hd]).sum(1))


def colsum_ref(src, wt=None, segs=1, dst0=None, dt=np.float64):
    """dst[s][c] = (dst0[s][c] +) sum over rows [rows s / segs, rows (s + 1) / segs) of wt_r src[r][c].
    Returns (dst [segs, cols], bound)."""
    src = _f(src, dt)
    rows, cols = src.shape
    segs = max(int(segs), 1)
    t = src if wt is None else _f(wt, dt)[:, None] * src
    out, bound = np.zeros((segs, cols), dt), np.zeros((segs, cols))
    for sg in range(segs):
        a, b = rows * sg // segs, rows * (sg + 1) // segs
        out[sg], bound[sg] = _sum(t[a:b], 0, dt), np.abs(t[a:b].astype(np.float64)).sum(0)
    if dst0 is not None:
        out, bound = out + _f(dst0, dt), bound + np.abs(_f(dst0, np.float64))
    return out, bound


# ------------------------------------------------------------------------------- the gather graph
N_GATHER = 1100
DEGREES = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257,
           258, 271, 272, 273, 511, 512, 513, 1023, 1025)
BOUNDARY = (0, 3, 4, 63, 64, 255, 256)     # and the row's last position
# Node ids in nine ranges, alternately "hot" and "cold"; a row of d entries takes its first d - 1 columns
# from the ranges in order (1, 2, 2, 58, 2, 190, 2, then the rest) and its last column from the last
# range, so that in EVERY row exactly the BOUNDARY positions and the last one hold hot nodes.
_RANGES = ((0, 4), (4, 14), (14, 20), (20, 88), (88, 94), (94, 294), (294, 300), (300, 1090), (1090, 1100))
_TAKE = (1, 2, 2, 58, 2, 190, 2, 790)
DEGREES_RANGE = (600, 634)                 # 34 consecutive rows: every degree of DEGREES once


def degree_of(i):
    """13 is coprime with 34: consecutive rows walk the degree list in a stride, small beside large."""
    return DEGREES[(13 * i) % len(DEGREES)]


def hot_nodes():
    hot = np.zeros(N_GATHER, bool)
    for k, (a, b) in enumerate(_RANGES):
        hot[a:b] = k % 2 == 0
    return hot


@functools.lru_cache(maxsize=None)
def gather_graph():
    """(rowptr [N + 1], col) int32 of the whole N_GATHER-node graph."""
    rng = np.random.default_rng(1234)
    rowptr, cols = np.zeros(N_GATHER + 1, np.int64), []
    for i in range(N_GATHER):
        d = degree_of(i)
        left, row = max(d - 1, 0), []
        for (a, b), take in zip(_RANGES[:-1], _TAKE):
            k = min(take, left)
            row.append(np.sort(rng.choice(np.arange(a, b), k, replace=False)))
            left -= k
        assert left == 0
        if d:
            row.append(rng.integers(_RANGES[-1][0], _RANGES[-1][1], 1))
        cols.append(np.concatenate(row) if row else np.zeros(0, np.int64))
        rowptr[i + 1] = rowptr[i] + d
    return rowptr.astype(np.int32), np.concatenate(cols).astype(np.int32)


def shard_csr(r0, r1):
    """Own rows [r0, r1) as hicgat.dist.ShardPlan.own_csr gives them: rowptr [N + 1] in global
    numbering with rowptr[r0] = 0 and entries in the own rows only, and the own columns."""
    rp, col = gather_graph()
    rp = rp.astype(np.int64)
    e0, e1 = rp[r0], rp[r1]
    return np.clip(rp - e0, 0, e1 - e0).astype(np.int32), col[e0:e1].copy()


def slab_of(rowptr, col, r0, r1, n):
    """The transpose of the own rows' entries: (rowptr_s [n + 1], perm) int32, slab row j listing the
    own-CSR indices of the edges (i, j) by ascending i."""
    perm = np.argsort(col, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))]).astype(np.int32), perm.astype(np.int32)


SHARD_ROWS = (1, 2, 3, 7, 8, 9, 17)
MID = 500


def row_ranges():
    """name -> (r0, r1): the whole graph, first / last / interior shards of 1 .. 17 rows, and the 34
    rows that hold every degree once."""
    out = {"whole": (0, N_GATHER), "degrees": DEGREES_RANGE}
    for k in SHARD_ROWS:
        out[f"first{k}"], out[f"last{k}"], out[f"mid{k}"] = (0, k), (N_GATHER - k, N_GATHER), (MID, MID + k)
    return out


FAMILIES = ("boundary", "extreme", "kink")


@functools.lru_cache(maxsize=None)
def features():
    return np.random.default_rng(5).standard_normal((N_GATHER, F)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def logits(family):
    """(a_src, a_dst) [N, 2] float32, given to the kernels directly.
    boundary: O(1) values; the hot nodes (every row's BOUNDARY and last positions) lie >= 3 above every
      other node, so a dropped or doubled boundary edge moves a row by far more than rounding.
    extreme: head 0 spread over +-60 on both sides (e in +-120: fp32 expf underflows to 0 in the longer
      rows, and many rows have one dominant entry), head 1 the same a_src for every node: every row's
      logits are all equal there.
    kink: a_src on the grid k / 4 (with -0.0 among the zeros) and a_dst_i = -a_src_j for one entry j of
      row i per head, so e = 0 exactly for every entry of the row that shares that grid value."""
    rng = np.random.default_rng({"boundary": 11, "extreme": 12, "kink": 13}[family])
    n = N_GATHER
    if family == "boundary":
        a_src = rng.uniform(-1, 1, (n, 2))
        hot = hot_nodes()
        a_src[hot] = rng.uniform(4.0, 4.5, (int(hot.sum()), 2))
        a_dst = rng.uniform(-2, 2, (n, 2))
    elif family == "extreme":
        a_src = np.stack([rng.uniform(-60, 60, n), np.full(n, 0.75)], 1)
        a_src[_RANGES[-1][0]:_RANGES[-1][0] + 3, 0] = 95.0     # a row that ends on one of these: one dominant entry
        a_dst = rng.uniform(-60, 60, (n, 2))
    else:
        a_src = rng.integers(-8, 9, (n, 2)) / 4.0
        a_src[(a_src == 0) & (rng.random((n, 2)) < 0.5)] = -0.0
        a_dst = np.full((n, 2), 0.25)
        rp, col = gather_graph()
        for i in range(n):
            d = rp[i + 1] - rp[i]
            for h in range(2):
                if d:
                    a_dst[i, h] = -a_src[col[rp[i] + int(rng.integers(0, d))], h]
    return a_src.astype(np.float32), a_dst.astype(np.float32)


@functools.lru_cache(maxsize=None)
def row_inputs(rows, seed=0):
    """Independent O(1) normals for ``rows`` own rows: g, y0 [rows, 512], bias [512], dxa [rows, 1024];
    y0 additionally holds exact 0.0 and -0.0 (about one entry in 16 each)."""
    rng = np.random.default_rng(100 + 7 * rows + seed)
    g, y0 = (rng.standard_normal((rows, F)).astype(np.float32) for _ in range(2))
    u = rng.random((rows, F))
    y0[u < 1 / 16] = 0.0
    y0[u > 15 / 16] = -0.0
    return dict(g=g, y0=y0, bias=rng.standard_normal(F).astype(np.float32),
                dxa=rng.standard_normal((rows, 2 * F)).astype(np.float32))


# ------------------------------------------------------------------------------- slab inputs
SLAB_N = (1, 3, 4, 5, 4095, 4096, 4097)
SLAB_ROW_ENTRIES = (0, 1, 15, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def slab_inputs(n):
    """(rowptr_s [n + 1], perm, ds [nnz, 2], x [n, 512]): slab row j has SLAB_ROW_ENTRIES[(j + n) % 6]
    entries (n = 1: 1 entry ... n = 5: ends on 0), perm a random permutation of the nnz ds entries."""
    rng = np.random.default_rng(300 + n)
    cnt = np.array([SLAB_ROW_ENTRIES[(j + n) % 6] for j in range(n)])
    nnz = int(cnt.sum())
    return (np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), rng.permutation(nnz).astype(np.int32),
            rng.standard_normal((nnz, 2)).astype(np.float32), rng.standard_normal((n, F)).astype(np.float32))


# ------------------------------------------------------------------------------- column-sum jobs
def colsum_lg(rows, segs, weighted):
    """log2 of the lanes per row group that a job must select (the case's intent; the host file holds
    it to its own restatement of add_col's rule)."""
    srows = -(-rows // max(segs, 1))
    return 8 if srows <= 16 else 6 if srows <= 64 else 4 if srows <= 256 else 1 if weighted and srows > 1024 else 2


# name: rows, cols, segs, ld - cols, ldd - cols, weighted, the lg it is there for
COLSUM_CASES = {
    "empty":        (0, 4, 1, 0, 0, False, 8),        # fewer rows than row groups: the one group is empty
    "r1":           (1, 1, 1, 0, 0, False, 8),
    "r16":          (16, 1027, 1, 0, 0, False, 8),    # two column chunks, ragged last float4 (scalar path)
    "r17":          (17, 3, 1, 0, 0, False, 6),
    "r33s2":        (33, 1, 2, 0, 4, False, 6),       # segments of 16 and 17 rows
    "r64s2":        (128, 512, 2, 0, 4, False, 6),
    "r65s3":        (195, 5, 3, 2, 4, False, 4),      # ld = 7: odd, scalar path
    "r256s7":       (1792, 1024, 7, 0, 4, False, 4),
    "r257":         (257, 4, 1, 0, 0, False, 2),
    "oddld":        (300, 512, 1, 3, 0, False, 2),    # cols % 4 == 0 but ld = 515: scalar path
    "rows_eq_segs": (7, 4, 7, 0, 8, False, 8),
    "rows_eq_3":    (3, 5, 3, 0, 3, False, 8),
    "w1024":        (1024, 512, 1, 0, 0, True, 2),
    "w1025":        (1025, 512, 1, 0, 0, True, 1),
    "w1026s2":      (2051, 1024, 2, 0, 4, True, 1),
    "w17":          (17, 1027, 1, 0, 0, True, 6),
}


@functools.lru_cache(maxsize=None)
def colsum_inputs(name):
    """(src [rows, cols], weight table [rows, 8] whose column 6 is the stride-8 weight view or None,
    dst0 [segs, cols])."""
    rows, cols, segs, _, _, weighted, _ = COLSUM_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    return (rng.standard_normal((rows, cols)).astype(np.float32),
            rng.standard_normal((rows, 8)).astype(np.float32) if weighted else None,
            rng.standard_normal((segs, cols)).astype(np.float32))

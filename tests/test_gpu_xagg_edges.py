"""The aggregate-first GATConv kernels (csrc/gat_xagg.hip) and the weighted, segmented column sum of
hicgat_param_grads_grouped (csrc/gemm.hip: colsum_grouped_kernel), one kernel per test through the C ABI --
pointers, row ranges and strides are the test's to choose -- against the float64 restatements of
tests/xagg_ref.py (tied to float64 autograd on the CPU by tests/test_xagg_ref_host.py).  Every kernel's
inputs come from the reference (rounded to fp32 once, and the reference takes them as rounded), so a
failure names one kernel; the two paired checks are edge + slab_sum against edge_acc and edge_acc's gpart
through the grouped column sum (test_slab_route_equals_edge_acc_route).

Every output lives in a ``Buf`` whose guard elements (and, for row_stats, the rows outside [r0, r1)) hold
a finite non-zero sentinel and must keep their bits; every call is made twice on fresh buffers and must
give the same bits.  Errors are judged per element against the condition bound the reference returns (the
float64 sum of the absolute values of the element's terms); a failure reports the worst row and its degree.

Graph (xagg_ref.gather_graph): 1100 nodes, row i of degree DEGREES[13 i mod 34] over 0, 1, 2, 3, 4, 5, 15,
16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 271, 272, 273, 511,
512, 513, 1023, 1025; row ranges: the whole graph, first / last / interior shards of 1, 2, 3, 7, 8, 9 and 17
rows, and rows 600..633 ("degrees": every degree once).  Logit families: "boundary" (positions 0, 3, 4, 63,
64, 255, 256 and the last of every row >= 3 above the rest), "extreme" (+-60 on both sides, head 1 all
equal), "kink" (e = 0 exactly, -0.0).

Branches reached on purpose, by the test (and case) that names them:
  xagg_fwd_kernel
    waves 1..3 own edges (> 64 / 128 / 192 entries), the second 256-edge round (> 256), the LDS merge of
      part[3][8][64] and red[wv] adding non-zeros -- test_fwd, rows of 65, 129, 193, 257 .. 1025 entries
      (every range but first1 / first2 holds some; "degrees" and "whole" all of them)
    padded slots of a partial 64-chunk, cnt % 4 != 0 -- test_fwd, rows of 1, 2, 3, 5, 15, 17, 65, 66, 129 ..
    a row without entries (max -inf, sum 0, X4 row 0) -- test_fwd first1 (that row alone), whole, degrees
    grids on both sides of the 8-way xcd_remap -- test_fwd rows 1, 2, 3, 7 (< 8), 8, 9, 17, 34, 1100
  xagg_edge_kernel
    the e0 += 32 rounds and row ends inside an 8-edge wave group -- test_edge, rows of 33, 63, 65, 66, 127 ..
    xa2 == NULL -- test_edge (every case: same ds bits, row_stats untouched)
  xagg_edge_acc_kernel
    kmax at its bounds 0 (a wave past the chunk's end), 1, 16, an odd kmax padded with the row itself at
      weight 0, the second cb += 256 chunk -- test_edge_acc, rows of 1 .. 5 (kmax 1 / 0), 15, 17, 31, 33,
      255, 256, 257, 258, 271 .. 273, 513, 1025
    rows b / G spans for odd rows, rows = 1, row_begin = 0 -- test_edge_acc first* / mid* / last* of 1, 3, 7, 9, 17
  xagg_slab_sum_kernel
    N % 4 != 0, the second persistent pass (N > 4096), slab rows of 0 and > 16 entries -- test_slab_sum,
      N = 1, 3, 5, 4095, 4097 / 4097 / entries 0, 1, 15, 16, 17, 33
  xagg_rows_bwd_kernel<0>, <1> and xagg_bias_relu_kernel at rows % 4 != 0, the y0 == 0 decisions (0.0 and
    -0.0) -- test_rows_bwd (act 0 and 1), test_bias_relu
  xagg_logits_kernel at N % 4 != 0 -- test_vec_and_logits, N = 1, 3, 5
  xagg_param_finish_kernel with segs > 1 and seg_stride > 1024 -- test_param_finish
  colsum_grouped_kernel: segs > 1 with ldd (r33s2, r64s2, r65s3, r256s7, rows_eq_segs, rows_eq_3, w1026s2),
    lg = 8 (empty, r1, r16, rows_eq_*), lg = 6 (r17, r33s2, r64s2, w17), lg = 4 (r65s3, r256s7), lg = 2 (r257,
    oddld, w1024), weighted lg = 1 (w1025, w1026s2), the scalar ld4 path with a ragged last float4 (r1, r16,
    r17, r65s3, rows_eq_3, w17; oddld by ld alone) -- test_colsum, test_colsum_jobs_in_one_launch (find_job
    over 16 jobs)

Tolerances (xagg_ref.TOL; error / condition bound): 8 x the largest ratio of the reference's own sequential
fp32 rendition over the cases, floor 2^-22, measured by test_xagg_ref_host.py::test_tolerance_table; beside
each the largest ratio measured on the MI355X by this file (MEASURED, from its first run; 156 tests, all passed):
  quantity   tolerance boundary / extreme / kink          measured on the MI355X
  vec        1.2e-6                                       6.5e-8
  logits     1.8e-6                                       2.5e-8
  sum        8.7e-6 / 6.2e-5 / 3.1e-5                     2.8e-7 / 7.6e-6 / 1.1e-7
  S3         1.1e-5 / 7.1e-5 / 3.4e-5                     2.2e-7 / 1.4e-7 / 1.6e-7
  X4         8.4e-6 / 2.0e-5 / 6.5e-6                     7.3e-7 / 2.6e-6 / 2.6e-7
  delta      7.6e-7                                       2.2e-8
  ds         1.9e-6 / 7.3e-6 / 1.9e-6                     1.1e-7 / 9.3e-7 / 5.7e-8
  da_dst     7.9e-7 / 6.0e-7 / 6.4e-7                     2.4e-8 / 2.9e-8 / 3.7e-8
  gpart      7.3e-7 / 3.8e-6 / 3.3e-7                     6.4e-8 / 4.3e-7 / 2.1e-8
  da_src     1.3e-6                                       9.0e-8
  g_src      9.5e-7                                       6.1e-8
  colsum     1.5e-6                                       1.1e-7
  dW         1.4e-6                                       1.9e-7
  datt       1.2e-6                                       2.8e-8
The gather quantities are measured per logit family (the "extreme" logits reach |e| = 120, whose fp32 sum
a_src + a_dst alone is 2^-17 off; one table entry for all three would hold the O(1) families to that).
The paired g_src routes measured 1.2e-8 (slab) and 1.2e-8 (edge_acc + column sum) of the bound; segs = 1 on
the summed g was bit-equal to segs = 3 on its parts.  No case exposed a kernel bug.
Exact (bit for bit): row_stats' max (the reference forms lrelu in fp32 for that field: one fp32 add and one
fp32 multiply e * slope), bias_relu's y and o (one fp32 addition each), rows_bwd's dout (a selection) and
its S3 move, every zero of a row without entries.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import xagg_ref as R
from guarded import Buf                  # the guarded output buffers (shared with test_gpu_gemm_edges.py)

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = R.N_GATHER
EINVAL, EUNSUPPORTED = -1, -3
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _L():
    from hicgat import _lib
    return _lib


def _rc(name, *args):
    L = _L()
    return getattr(L.lib(), name)(*args, L.stream())


def _call(name, *args):
    _L().check(_rc(name, *args), name)


_KEEP = []


def _dev(a):
    """A read-only input on the device (16-byte aligned), kept alive to the end of the module: the calls
    take raw pointers, and a freed block would be handed to the next buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    _KEEP.append(t)
    return t


def P(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes)


def _note(quantity, family, got, ref, bound):
    """Print the worst error / bound (the docstring's measured column) and return (ratio, index)."""
    w, k = R.worst(got, ref, bound)
    print(f"XAGG_RATIO {quantity} {family or '-'} {w:.3e}")
    return w, k


def _check(quantity, family, got, ref, bound, where=None):
    w, k = _note(quantity, family, got, ref, bound)
    assert w <= R.tol(quantity, family), (quantity, family, w, R.tol(quantity, family), k, where(k) if where else None)


# ------------------------------------------------------------------------------- shared inputs
RANGES = R.row_ranges()
GATHER_CASES = [("boundary", k) for k in RANGES] + [(f, k) for f in ("extreme", "kink") for k in ("degrees", "mid17")]


@functools.lru_cache(maxsize=None)
def _x_dev():
    return _dev(R.features())


@functools.lru_cache(maxsize=None)
def _logits_dev(family):
    return tuple(_dev(t) for t in R.logits(family))


@functools.lru_cache(maxsize=None)
def _csr_dev(name):
    rp, col = R.shard_csr(*RANGES[name])
    return Buf(1, len(rp), np.int32, R.SENT_I32, data=rp), Buf(1, len(col), np.int32, R.SENT_I32, data=col)


@functools.lru_cache(maxsize=None)
def _fwd_ref(family, name):
    r0, r1 = RANGES[name]
    return R.fwd_ref(*R.shard_csr(r0, r1), r0, r1, R.features(), *R.logits(family))


@functools.lru_cache(maxsize=None)
def _edge_inputs(family, name):
    """The fp32 values the edge kernels receive (rounded once from the reference's forward and row pass)
    and the float64 reference of their outputs computed from exactly those."""
    r0, r1 = RANGES[name]
    rows = r1 - r0
    fw, ri = _fwd_ref(family, name), R.row_inputs(rows)
    _, delta, _ = R.rows_bwd_ref(1, ri["g"], ri["y0"], ri["bias"])
    st = dict(m=fw["m"].astype(f32), s=fw["s"].astype(f32), S3=fw["S3"].astype(f32), delta=delta.astype(f32),
              xa2=fw["X4"][:, 1].astype(f32), dxa=ri["dxa"])
    ref = R.edge_ref(*R.shard_csr(r0, r1), r0, r1, R.features(), *R.logits(family), st["m"], st["s"], st["delta"],
                     st["dxa"], S3=st["S3"], xa2=st["xa2"])
    return st, ref


def _row_stats_buf(name, st):
    r0, r1 = RANGES[name]
    data = np.full((N, 8), R.SENT32, f32)
    data[r0:r1] = np.concatenate([st["m"], st["s"], st["delta"], st["S3"]], 1)
    return Buf(N, 8, data=data), data


def _x4_with_xa2(st):
    """An X4-shaped [2, 2, rows, 512] buffer whose kind-1 planes hold xa2 (kind 0: the sentinel)."""
    rows = st["xa2"].shape[1]
    x4 = np.full((2, 2, rows, R.F), R.SENT32, f32)
    x4[:, 1] = st["xa2"]
    return _dev(x4), rows * R.F * 4


def _degree_at(name):
    rp, _ = R.shard_csr(*RANGES[name])
    r0 = RANGES[name][0]
    return lambda r: int(rp[r0 + r + 1] - rp[r0 + r])


def _edge_row(name):
    rp, _ = R.shard_csr(*RANGES[name])
    r0, r1 = RANGES[name]

    def f(k):
        r = int(np.searchsorted(rp[r0:r1 + 1], k[0], side="right")) - 1
        return dict(row=r0 + r, degree=int(rp[r0 + r + 1] - rp[r0 + r]), position=int(k[0] - rp[r0 + r]))
    return f


# ------------------------------------------------------------------------------- 1. vec and logits
@pytest.mark.parametrize("n", [1, 3, 4, 5, N])
def test_vec_and_logits(n):
    """hicgat_xagg_logits (logits alone): vec against vec_ref, a_src / a_dst against x . (the vec the
    device wrote), N on and off a multiple of the 4 rows of a block."""
    rng = np.random.default_rng(21)
    W = (rng.standard_normal((512, 512)) / np.sqrt(512)).astype(f32)
    att_s, att_d = (rng.standard_normal((2, 256)).astype(f32) for _ in range(2))
    x = R.features()[:n]
    ins = [_dev(t) for t in (x, W, att_s, att_d)]
    outs = []
    for _ in range(2):
        vec, a_src, a_dst = Buf(4, 512), Buf(n, 2), Buf(n, 2)
        _call("hicgat_xagg_logits", *(P(t) for t in ins), n, 512, 2, 256, vec.ptr, a_src.ptr, a_dst.ptr, None, 0, None,
              None, None, None, 0)
        res = [b.read() for b in (vec, a_src, a_dst)]
        assert all(ok for _, ok in res), "wrote outside vec / a_src / a_dst"
        outs.append([m for m, _ in res])
    assert all(R.same_bits(a, b) for a, b in zip(*outs))
    v, a_s, a_d = outs[0]
    _check("vec", None, v, *R.vec_ref(W, att_s, att_d))
    rs, rd, bound = R.logits_ref(x, v)
    _check("logits", None, np.concatenate([a_s, a_d], 1), np.concatenate([rs, rd], 1), bound)


# ------------------------------------------------------------------------------- 2. forward gather
def _run_fwd(family, name):
    r0, r1 = RANGES[name]
    rp, col = _csr_dev(name)
    a_src, a_dst = _logits_dev(family)
    X4, rs = Buf(4 * (r1 - r0), R.F), Buf(N, 8)
    _call("hicgat_xagg_fwd", rp.ptr, col.ptr, N, 512, 2, 256, r0, r1, P(_x_dev()), P(a_src), P(a_dst), R.NS, X4.ptr, rs.ptr)
    (x4, ok1), (st, ok2) = X4.read(), rs.read()
    assert ok1, "xagg_fwd wrote X4 beyond [4 rows, 512]"
    assert ok2, "xagg_fwd wrote row_stats beyond [N, 8]"
    return x4.reshape(2, 2, r1 - r0, R.F), st


@pytest.mark.parametrize("family,name", GATHER_CASES)
def test_fwd(family, name):
    r0, r1 = RANGES[name]
    x4, st = _run_fwd(family, name)
    x4b, stb = _run_fwd(family, name)
    assert R.same_bits(x4, x4b) and R.same_bits(st, stb)
    ref = _fwd_ref(family, name)
    outside = np.ones(N, bool)
    outside[r0:r1] = False
    assert np.all(st[outside].view(np.uint32) == R.SENT32.view(np.uint32)), "row_stats rows outside [r0, r1) written"
    own = st[r0:r1]
    assert R.same_bits(own[:, 0:2], ref["m"].astype(f32)), "the row maximum is exact"
    assert np.all(own[:, 6:8].view(np.uint32) == 0)
    deg = _degree_at(name)
    where = lambda k: dict(row=r0 + k[0], degree=deg(k[0]))
    _check("sum", family, own[:, 2:4], ref["s"], ref["s"], where)
    _check("S3", family, own[:, 4:6], ref["S3"], ref["S3"], where)
    _check("X4", family, x4, ref["X4"], ref["X4_abs"], lambda k: dict(row=r0 + k[2], degree=deg(k[2])))
    empty = np.array([deg(r) == 0 for r in range(r1 - r0)])
    if empty.any():
        assert np.all(x4[:, :, empty].view(np.uint32) == 0) and np.all(own[empty, 2:6].view(np.uint32) == 0)
        assert np.all(own[empty, 0:2] == -np.inf)
    assert np.isfinite(x4).all() and np.isfinite(own[:, 2:]).all()


# ------------------------------------------------------------------------------- 3. bias + relu, row pass
@pytest.mark.parametrize("rows", [1, 2, 3, 5, 9])
def test_bias_relu(rows):
    """y0 + bias and relu(y0 + bias) bit for bit (one fp32 addition; torch.relu's y <= 0 -> +0.0, with
    exact 0.0 and -0.0 sums from the zero entries of y0 under a zero bias entry)."""
    ri = R.row_inputs(rows)
    bias = ri["bias"].copy()
    bias[::5] = 0.0
    bias[1::5] = -0.0
    y_ref, o_ref = R.bias_relu_ref(ri["y0"], bias)
    assert ((y_ref == 0) & np.signbit(y_ref)).any() and ((y_ref == 0) & ~np.signbit(y_ref)).any()
    y0, o = Buf(rows, 512, data=ri["y0"]), Buf(rows, 512)
    _call("hicgat_xagg_bias_relu", y0.ptr, P(_dev(bias)), o.ptr, rows, 512)
    (y, ok1), (ov, ok2) = y0.read(), o.read()
    assert ok1 and ok2
    assert R.same_bits(y, y_ref.astype(f32)) and R.same_bits(ov, o_ref.astype(f32))
    assert not np.signbit(ov[y_ref <= 0]).any()


@pytest.mark.parametrize("rows", [1, 2, 3, 5, 7, 9, 17])
@pytest.mark.parametrize("act", [0, 1])
def test_rows_bwd(act, rows):
    """dout = g [y0 > 0] (act 1; y0 = 0.0 and -0.0 give 0) or g, exactly; delta at tolerance; the
    forward's S3 moved from [4:6] to [6:8] and [0:4] left alone, bit for bit."""
    ri = R.row_inputs(rows)
    stats = np.random.default_rng(rows).standard_normal((rows, 8)).astype(f32)
    dout_ref, delta, bound = R.rows_bwd_ref(act, ri["g"], ri["y0"], ri["bias"])
    outs = []
    for _ in range(2):
        dout, rs = Buf(rows, 512), Buf(rows, 8, data=stats)
        _call("hicgat_xagg_rows_bwd", rows, 512, act, P(_dev(ri["g"])), P(_dev(ri["y0"])), P(_dev(ri["bias"])), dout.ptr,
              rs.ptr)
        (d, ok1), (s, ok2) = dout.read(), rs.read()
        assert ok1 and ok2, "rows_bwd wrote beyond dout / row_stats"
        outs.append((d, s))
    assert R.same_bits(outs[0][0], outs[1][0]) and R.same_bits(outs[0][1], outs[1][1])
    d, s = outs[0]
    assert R.same_bits(d, dout_ref.astype(f32))
    assert R.same_bits(s[:, 0:4], stats[:, 0:4]) and R.same_bits(s[:, 6:8], stats[:, 4:6])
    _check("delta", None, s[:, 4:6], delta, bound)


# ------------------------------------------------------------------------------- 4. edge passes
def _run_edge(family, name, with_xa2):
    r0, r1 = RANGES[name]
    rp, col = _csr_dev(name)
    a_src, a_dst = _logits_dev(family)
    st, _ = _edge_inputs(family, name)
    rs, rs_in = _row_stats_buf(name, st)
    x4, off = _x4_with_xa2(st)
    ds = Buf(1, 2 * col.cols)
    _call("hicgat_xagg_edge", rp.ptr, col.ptr, N, 512, 2, 256, r0, r1, P(_x_dev()), P(a_src), P(a_dst), rs.ptr,
          P(_dev(st["dxa"])), P(x4, off) if with_xa2 else None, R.NS, ds.ptr)
    (d, ok1), (s, ok2) = ds.read(), rs.read()
    assert ok1, "xagg_edge wrote ds beyond the own entries"
    assert ok2
    return d.reshape(-1, 2), s, rs_in


@pytest.mark.parametrize("family,name", GATHER_CASES)
def test_edge(family, name):
    r0, r1 = RANGES[name]
    _, ref = _edge_inputs(family, name)
    ds, rs, rs_in = _run_edge(family, name, True)
    ds2, rs2, _ = _run_edge(family, name, True)
    assert R.same_bits(ds, ds2) and R.same_bits(rs, rs2)
    ds0, rs0, _ = _run_edge(family, name, False)
    assert R.same_bits(ds0, ds), "xa2 = NULL changes ds"
    assert R.same_bits(rs0, rs_in), "xa2 = NULL must leave row_stats alone"
    keep = np.ones((N, 8), bool)
    keep[r0:r1, 6:8] = False
    assert np.array_equal(rs.view(np.uint32)[keep], rs_in.view(np.uint32)[keep]), "row_stats written outside [r0:r1, 6:8]"
    assert np.isfinite(ds).all()
    _check("ds", family, ds, ref["ds"], ref["ds_abs"], _edge_row(name))
    deg = _degree_at(name)
    _check("da_dst", family, rs[r0:r1, 6:8], ref["da_dst"], ref["da_dst_abs"], lambda k: dict(row=r0 + k[0], degree=deg(k[0])))
    empty = np.array([deg(r) == 0 for r in range(r1 - r0)])
    assert np.all(rs[r0:r1, 6:8][empty] == 0)


def _run_edge_acc(family, name):
    r0, r1 = RANGES[name]
    rp, col = _csr_dev(name)
    a_src, a_dst = _logits_dev(family)
    st, _ = _edge_inputs(family, name)
    rs, rs_in = _row_stats_buf(name, st)
    x4, off = _x4_with_xa2(st)
    nb = _L().lib().hicgat_xagg_edge_acc_blocks(r1 - r0)
    assert nb == max(1, (r1 - r0 + 1) // 2)
    gpart = Buf(nb, 1024)
    _call("hicgat_xagg_edge_acc", rp.ptr, col.ptr, N, 512, 2, 256, r0, r1, P(_x_dev()), P(a_src), P(a_dst), rs.ptr,
          P(_dev(st["dxa"])), P(x4, off), R.NS, gpart.ptr)
    (g, ok1), (s, ok2) = gpart.read(), rs.read()
    assert ok1, "xagg_edge_acc wrote gpart beyond [blocks, 1024]"
    assert ok2
    return g, s, rs_in, gpart


@pytest.mark.parametrize("family,name", GATHER_CASES)
def test_edge_acc(family, name):
    r0, r1 = RANGES[name]
    _, ref = _edge_inputs(family, name)
    g, rs, rs_in, _ = _run_edge_acc(family, name)
    g2, rs2, _, _ = _run_edge_acc(family, name)
    assert R.same_bits(g, g2) and R.same_bits(rs, rs2)
    keep = np.ones((N, 8), bool)
    keep[r0:r1, 6:8] = False
    assert np.array_equal(rs.view(np.uint32)[keep], rs_in.view(np.uint32)[keep])
    spans = R.edge_acc_spans(r1 - r0, g.shape[0])
    deg = _degree_at(name)
    gref, gbound = R.gpart_ref(ref["G"], ref["G_abs"], g.shape[0])
    _check("gpart", family, g, gref, gbound,
           lambda k: dict(block=k[0], rows=[(r0 + r, deg(r)) for r in range(*spans[k[0]])]))
    _check("da_dst", family, rs[r0:r1, 6:8], ref["da_dst"], ref["da_dst_abs"], lambda k: dict(row=r0 + k[0], degree=deg(k[0])))
    assert np.isfinite(g).all()


def _colsum_job(src_ptr, ld, rows, cols, dst_ptr, acc, wt_ptr=None, ldw=0, segs=1, ldd=0):
    v = lambda p: p.value if isinstance(p, ctypes.c_void_p) else p
    return _L().ColsumJob(v(src_ptr), ld, rows, cols, v(dst_ptr), acc, v(wt_ptr), ldw, segs, ldd)


def _grouped_colsum(jobs):
    L = _L()
    arr = (L.ColsumJob * len(jobs))(*jobs)
    return _rc("hicgat_param_grads_grouped", None, 0, arr, len(jobs), 0, None, 0)


@pytest.mark.parametrize("name", ["degrees", "mid17", "whole"])
def test_slab_route_equals_edge_acc_route(name):
    """The two routes to g_src on the device, each from its own kernels' outputs: edge -> ds -> slab_sum,
    and edge_acc -> gpart -> the grouped column sum.  Both within the sum of their stages' tolerances of
    the float64 g_src (bound: sum over the edges of ds's bound times |x_j|), and da_src against the
    float64 slab sum of the reference ds."""
    family = "boundary"
    r0, r1 = RANGES[name]
    rp, col = R.shard_csr(r0, r1)
    _, ref = _edge_inputs(family, name)
    ds, _, _ = _run_edge(family, name, True)
    srp, perm = R.slab_of(rp, col, r0, r1, N)
    ws_bytes = _L().lib().hicgat_xagg_slab_workspace_bytes()
    ws = _L().workspace(ws_bytes, DEV)
    da_src, g_slab = Buf(N, 2), Buf(1, 1024)
    _call("hicgat_xagg_slab_sum", P(_dev(srp)), P(_dev(perm)), N, P(_dev(ds)), P(_x_dev()), da_src.ptr, g_slab.ptr, P(ws),
          ws_bytes)
    (da, ok1), (gs, ok2) = da_src.read(), g_slab.read()
    assert ok1 and ok2
    _, _, _, gpart = _run_edge_acc(family, name)
    g_acc = Buf(1, 1024)
    assert _grouped_colsum([_colsum_job(gpart.ptr, 1024, gpart.rows, 1024, g_acc.ptr, 0)]) == 0
    ga, ok3 = g_acc.read()
    assert ok3
    g_ref, g_bound = ref["G"].sum(0), ref["G_abs"].sum(0)
    da_ref, _, _, _ = R.slab_ref(srp, perm, ref["ds"], R.features())
    _, da_bound, _, _ = R.slab_ref(srp, perm, ref["ds"], R.features(), ds_abs=ref["ds_abs"])
    t_slab = R.tol("ds", family) + R.tol("da_src") + R.tol("g_src")
    t_acc = R.tol("gpart", family) + R.tol("colsum")
    w_da, w_slab, w_acc = (R.worst(a, b, c)[0] for a, b, c in ((da, da_ref, da_bound), (gs[0], g_ref, g_bound), (ga[0], g_ref, g_bound)))
    print(f"XAGG_PAIRED {name} da_src {w_da:.3e} slab {w_slab:.3e} acc {w_acc:.3e}")
    assert w_da <= R.tol("ds", family) + R.tol("da_src")
    assert w_slab <= t_slab and w_acc <= t_acc
    assert R.worst(gs[0], ga[0], g_bound)[0] <= t_slab + t_acc


# ------------------------------------------------------------------------------- 5. slab sum
@pytest.mark.parametrize("n", R.SLAB_N)
def test_slab_sum(n):
    srp, perm, ds, x = R.slab_inputs(n)
    da_ref, da_bound, g_ref, g_bound = R.slab_ref(srp, perm, ds, x)
    ws_bytes = _L().lib().hicgat_xagg_slab_workspace_bytes()
    ins = [_dev(t) for t in (srp, perm, ds, x)]
    outs = []
    for _ in range(2):
        da, g = Buf(n, 2), Buf(1, 1024)
        ws = _L().workspace(ws_bytes, DEV)
        _call("hicgat_xagg_slab_sum", P(ins[0]), P(ins[1]), n, P(ins[2]), P(ins[3]), da.ptr, g.ptr, P(ws), ws_bytes)
        (a, ok1), (b, ok2) = da.read(), g.read()
        assert ok1, "slab_sum wrote da_src beyond [N, 2]"
        assert ok2, "slab_sum wrote g_src beyond 1024"
        outs.append((a, b))
    assert R.same_bits(outs[0][0], outs[1][0]) and R.same_bits(outs[0][1], outs[1][1])
    da, g = outs[0]
    cnt = np.diff(srp)
    _check("da_src", None, da, da_ref, da_bound, lambda k: dict(row=k[0], entries=int(cnt[k[0]])))
    assert np.all(da[cnt == 0].view(np.uint32) == 0)
    _check("g_src", None, g[0], g_ref, g_bound)


# ------------------------------------------------------------------------------- 6. param finish
def _param_inputs(segs, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(f32)
    return f(512, 512), f(2, 256), f(2, 256), f(segs, 1024), f(segs, 1024), f(512, 512), f(512), f(512)


def _run_param_finish(p, segs, stride):
    W, att_s, att_d, gs, gd, dW0, dl0, dr0 = p
    ins = [_dev(t) for t in (W, att_s, att_d)]
    gsb, gdb = Buf(segs, 1024, ld=stride, data=gs), Buf(segs, 1024, ld=stride, data=gd)
    dW, dl, dr = Buf(512, 512, data=dW0), Buf(1, 512, data=dl0), Buf(1, 512, data=dr0)
    _call("hicgat_xagg_param_finish", P(ins[0]), P(ins[1]), P(ins[2]), gsb.ptr, gdb.ptr, segs, stride if segs > 1 else 0,
          512, 2, 256, dW.ptr, dl.ptr, dr.ptr)
    res = [b.read() for b in (dW, dl, dr)]
    assert all(ok for _, ok in res), "param_finish wrote beyond dW / datt"
    return res[0][0], np.stack([res[1][0][0], res[2][0][0]])


@pytest.mark.parametrize("stride", [1024, 1088])
@pytest.mark.parametrize("segs", [1, 2, 3])
def test_param_finish(segs, stride):
    p = _param_inputs(segs, 50 + segs)
    dW, datt = _run_param_finish(p, segs, stride)
    dW2, datt2 = _run_param_finish(p, segs, stride)
    assert R.same_bits(dW, dW2) and R.same_bits(datt, datt2)
    ref = R.param_finish_ref(*p)
    _check("dW", None, dW, ref[0], ref[1])
    _check("datt", None, datt, np.stack(ref[2:4]), np.stack(ref[4:6]))


def test_param_finish_segments_add_up():
    """segs = 1 on the (fp32, segment-order) sum of three parts against segs = 3 on the parts: both within
    tolerance of the float64 result of the parts, and of each other to rounding."""
    p = _param_inputs(3, 61)
    summed = tuple(((g[0] + g[1]) + g[2])[None] for g in p[3:5])
    one = _run_param_finish(p[:3] + summed + p[5:], 1, 1024)
    three = _run_param_finish(p, 3, 1088)
    ref = R.param_finish_ref(*p)
    for got in (one, three):
        assert R.passes(got[0], ref[0], ref[1], R.tol("dW")) and R.passes(got[1], np.stack(ref[2:4]), np.stack(ref[4:6]), R.tol("datt"))
    print("param_finish segs = 1 on the summed g bit-equal to segs = 3:", R.same_bits(one[0], three[0]) and R.same_bits(one[1], three[1]))
    assert R.worst(one[0], three[0], ref[1])[0] <= 2 * R.tol("dW")
    assert R.worst(one[1], three[1], np.stack(ref[4:6]))[0] <= 2 * R.tol("datt")


# ------------------------------------------------------------------------------- 7. grouped column sum
def _colsum_bufs(name, acc):
    rows, cols, segs, ldp, lddp, weighted, lg = R.COLSUM_CASES[name]
    src, wt, dst0 = R.colsum_inputs(name)
    sb = Buf(rows, cols, ld=cols + ldp, data=src)
    db = Buf(segs, cols, ld=cols + lddp, data=dst0)
    wd = _dev(wt) if weighted else None
    job = _colsum_job(sb.ptr, cols + ldp, rows, cols, db.ptr, acc, P(wd, 6 * 4) if weighted else None, 8 if weighted else 0,
                      segs, cols + lddp)
    ref = R.colsum_ref(src, wt[:, 6] if weighted else None, segs, dst0 if acc else None)
    return job, (sb, db, wd), ref


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("name", list(R.COLSUM_CASES))
def test_colsum(name, acc):
    """One column-sum job per launch of hicgat_param_grads_grouped (no weight-gradient job): the form
    (lg), the segments, the strides ld / ldd and the stride-8 weight view of the case, overwrite and
    accumulate; the padding of dst (ldd > cols) and the guards keep their bits."""
    outs = []
    for _ in range(2):
        job, (sb, db, _w), (ref, bound) = _colsum_bufs(name, acc)
        assert _grouped_colsum([job]) == 0
        torch.cuda.synchronize()
        got, ok = db.read()
        assert ok, "the column sum wrote into dst's padding or guards"
        assert sb.untouched()
        outs.append(got)
    assert R.same_bits(outs[0], outs[1])
    _check("colsum", None, outs[0], ref, bound)
    if name == "empty":
        assert R.same_bits(outs[0], R.colsum_inputs(name)[2] if acc else np.zeros_like(outs[0]))


def test_colsum_jobs_in_one_launch():
    """All the cases as the jobs of ONE launch (find_job over 16 jobs): the same bits as one launch each."""
    names = list(R.COLSUM_CASES)
    single = []
    for k, name in enumerate(names):
        job, (_s, db, _w), _ = _colsum_bufs(name, k % 2)
        assert _grouped_colsum([job]) == 0
        single.append(db.read()[0])
    made = [_colsum_bufs(name, k % 2) for k, name in enumerate(names)]
    assert _grouped_colsum([m[0] for m in made]) == 0
    for name, m, want in zip(names, made, single):
        got, ok = m[1][1].read()
        assert ok and R.same_bits(got, want), name


# ------------------------------------------------------------------------------- 8. refusals
def test_refusals_come_before_any_launch():
    """Every argument check of the ABI returns its documented code and leaves the outputs untouched.
    Only arguments that the host code rejects are passed: no kernel runs in this test."""
    name, family = "first2", "boundary"
    r0, r1 = RANGES[name]
    rp, col = _csr_dev(name)
    a_src, a_dst = _logits_dev(family)
    st, _ = _edge_inputs(family, name)
    x = _x_dev()
    X4, rs, ds, gpart = Buf(4 * 2, 512), Buf(N, 8), Buf(1, 2 * col.cols), Buf(1, 1024)
    dxa = _dev(st["dxa"])
    x4, off = _x4_with_xa2(st)
    outs = [X4, rs, ds, gpart]
    bad = []

    def expect(code, fn, *args):
        rc = _rc(fn, *args)
        if rc != code:
            bad.append((fn, args, rc, code))

    def gather_args(fn, **kw):
        a = dict(rp=rp.ptr, col=col.ptr, N=N, F=512, H=2, C=256, r0=r0, r1=r1, x=P(x), a_src=P(a_src), a_dst=P(a_dst),
                 rs=rs.ptr, dxa=P(dxa), xa2=P(x4, off), X4=X4.ptr, ds=ds.ptr, gpart=gpart.ptr)
        a.update(kw)
        head = (a["rp"], a["col"], a["N"], a["F"], a["H"], a["C"], a["r0"], a["r1"], a["x"], a["a_src"], a["a_dst"])
        if fn == "hicgat_xagg_fwd":
            return head + (R.NS, a["X4"], a["rs"])
        if fn == "hicgat_xagg_edge":
            return head + (a["rs"], a["dxa"], a["xa2"], R.NS, a["ds"])
        return head + (a["rs"], a["dxa"], a["xa2"], R.NS, a["gpart"])

    for fn, ptrs in (("hicgat_xagg_fwd", ("rp", "col", "x", "a_src", "a_dst", "X4", "rs")),
                     ("hicgat_xagg_edge", ("rp", "col", "x", "a_src", "a_dst", "rs", "dxa", "ds")),
                     ("hicgat_xagg_edge_acc", ("rp", "col", "x", "a_src", "a_dst", "rs", "dxa", "gpart"))):
        expect(EINVAL, fn, *gather_args(fn, r1=N + 1))
        expect(EINVAL, fn, *gather_args(fn, r0=3, r1=2))
        expect(EINVAL, fn, *gather_args(fn, r0=-1))
        expect(EINVAL, fn, *gather_args(fn, N=-1, r1=-1, r0=-1))
        for k, v in (("F", 256), ("H", 4), ("C", 128)):
            expect(EUNSUPPORTED, fn, *gather_args(fn, **{k: v}))
        for k in ptrs:
            expect(EINVAL, fn, *gather_args(fn, **{k: None}))
    # logits: the checks in front of its first launch
    W, att = _dev(np.zeros((512, 512), f32)), _dev(np.zeros((2, 256), f32))
    vec, la, lb, zb = Buf(4, 512), Buf(N, 2), Buf(N, 2), Buf(1, 64)
    outs += [vec, la, lb, zb]
    lg = lambda **kw: tuple({**dict(x=P(x), W=P(W), a=P(att), b=P(att), N=N, F=512, H=2, C=256, vec=vec.ptr, s=la.ptr,
                                    d=lb.ptr, z=None, zn=0, ctr=None, w1=None, w2=None, pack=None, pb=0), **kw}.values())
    expect(EINVAL, "hicgat_xagg_logits", *lg(N=-1))
    expect(EINVAL, "hicgat_xagg_logits", *lg(zn=-1))
    expect(EINVAL, "hicgat_xagg_logits", *lg(zn=64))                                   # zero_n > 0 without zero_buf
    expect(EINVAL, "hicgat_xagg_logits", *lg(z=ctypes.c_void_p(zb.addr + 4), zn=32))    # misaligned zero_buf
    for k, v in (("F", 256), ("H", 1), ("C", 64)):
        expect(EUNSUPPORTED, "hicgat_xagg_logits", *lg(**{k: v}))
    for k in ("W", "a", "b", "vec"):
        expect(EINVAL, "hicgat_xagg_logits", *lg(**{k: None}))
    # bias_relu, rows_bwd
    y0, o, dout, rsl = Buf(2, 512), Buf(2, 512), Buf(2, 512), Buf(2, 8)
    outs += [y0, o, dout, rsl]
    bias = _dev(np.zeros(512, f32))
    expect(EUNSUPPORTED, "hicgat_xagg_bias_relu", y0.ptr, P(bias), o.ptr, 2, 256)
    expect(EINVAL, "hicgat_xagg_bias_relu", y0.ptr, P(bias), o.ptr, -1, 512)
    for k in range(3):
        a = [y0.ptr, P(bias), o.ptr]
        a[k] = None
        expect(EINVAL, "hicgat_xagg_bias_relu", *a, 2, 512)
    g = _dev(np.zeros((2, 512), f32))
    expect(EINVAL, "hicgat_xagg_rows_bwd", 2, 512, 2, P(g), P(g), P(bias), dout.ptr, rsl.ptr)
    expect(EINVAL, "hicgat_xagg_rows_bwd", 2, 512, -1, P(g), P(g), P(bias), dout.ptr, rsl.ptr)
    expect(EINVAL, "hicgat_xagg_rows_bwd", -1, 512, 1, P(g), P(g), P(bias), dout.ptr, rsl.ptr)
    expect(EUNSUPPORTED, "hicgat_xagg_rows_bwd", 2, 256, 1, P(g), P(g), P(bias), dout.ptr, rsl.ptr)
    for k in range(5):
        a = [P(g), P(g), P(bias), dout.ptr, rsl.ptr]
        a[k] = None
        expect(EINVAL, "hicgat_xagg_rows_bwd", 2, 512, 1, *a)
    # slab_sum
    srp, perm, dsv, xs = (_dev(t) for t in R.slab_inputs(5))
    da, gsrc = Buf(5, 2), Buf(1, 1024)
    outs += [da, gsrc]
    need = _L().lib().hicgat_xagg_slab_workspace_bytes()
    ws = _L().workspace(need, DEV)
    sl = [P(srp), P(perm), 5, P(dsv), P(xs), da.ptr, gsrc.ptr, P(ws), need]
    expect(EINVAL, "hicgat_xagg_slab_sum", *sl[:8], need - 1)
    expect(EINVAL, "hicgat_xagg_slab_sum", *sl[:8], 0)
    expect(EINVAL, "hicgat_xagg_slab_sum", *sl[:2], -1, *sl[3:])
    for k in (0, 1, 3, 4, 5, 6, 7):
        a = list(sl)
        a[k] = None
        expect(EINVAL, "hicgat_xagg_slab_sum", *a)
    # param_finish
    gs = Buf(3, 1024, ld=1088)
    dW, dl, dr = Buf(512, 512), Buf(1, 512), Buf(1, 512)
    outs += [dW, dl, dr]
    pf = lambda segs=1, stride=0, F=512, H=2, C=256, **kw: tuple(
        {**dict(W=P(W), a=P(att), b=P(att), gs=gs.ptr, gd=gs.ptr, segs=segs, stride=stride, F=F, H=H, C=C, dW=dW.ptr,
                dl=dl.ptr, dr=dr.ptr), **kw}.values())
    expect(EINVAL, "hicgat_xagg_param_finish", *pf(segs=0))
    expect(EINVAL, "hicgat_xagg_param_finish", *pf(segs=2, stride=1023))
    expect(EINVAL, "hicgat_xagg_param_finish", *pf(segs=3, stride=0))
    for k, v in (("F", 256), ("H", 4), ("C", 128)):
        expect(EUNSUPPORTED, "hicgat_xagg_param_finish", *pf(**{k: v}))
    for k in ("W", "a", "b", "gs", "gd", "dW", "dl", "dr"):
        expect(EINVAL, "hicgat_xagg_param_finish", *pf(**{k: None}))
    # the grouped column sum
    src, dst = Buf(8, 4), Buf(3, 4, ld=8)
    outs += [dst]
    for job in (_colsum_job(src.ptr, 4, 2, 4, dst.ptr, 0, None, 0, 3, 8),        # rows < segs
                _colsum_job(src.ptr, 4, 8, 4, dst.ptr, 0, None, 0, 2, 3),        # ldd < cols with segments
                _colsum_job(src.ptr, 4, -1, 4, dst.ptr, 0),
                _colsum_job(src.ptr, 4, 8, -1, dst.ptr, 0),
                _colsum_job(src.ptr, 4, 8, 4, None, 0),
                _colsum_job(None, 4, 8, 4, dst.ptr, 0)):
        rc = _grouped_colsum([job])
        if rc != EINVAL:
            bad.append(("colsum", rc))
    rc = _rc("hicgat_param_grads_grouped", None, 0, None, 1, 0, None, 0)
    if rc != EINVAL:
        bad.append(("colsum null jobs", rc))
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(b.untouched() for b in outs), [k for k, b in enumerate(outs) if not b.untouched()]

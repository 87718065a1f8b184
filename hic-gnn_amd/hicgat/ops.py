"""Autograd functions over the HIP kernels (the product compute path; no CPU fallback).

* ``gat_conv``        -- PyG 1.7.2 GATConv forward/backward (a2, a4, a5 and their backward).
* ``pairwise_dist``   -- torch.cdist(c, c, p=2) forward/backward (a7), D materialised.
* ``fused_dist_loss`` -- cdist + MSELoss (+ Pearson / combined loss value) fused (a7-a9), D never
                         materialised; returns the loss scalar and keeps the fp64 stats.
"""
import collections
import contextlib
import operator
import os

import torch

from . import _lib, kernels, paramgrads, streams
# the parameter-gradient scheduler's functions, so callers say ops.overlapped_param_grads() as before
# (its knobs -- BIG_GROUP, SIDE_GROUPED, ... -- live in paramgrads alone)
from .paramgrads import (ColsumJob, WeightGradJob, grouped_flush, grouped_param_grads,  # noqa: F401
                         overlapped_param_grads, param_launch, side_begin, side_flush, side_join, side_lane,
                         side_mark, side_record)


def _sink(p):
    """The parameter's own ``.grad`` when it is a view into ``FlatAdam``'s flat gradient buffer
    (marked ``_hicgat_grad_sink``): the backward kernels then ADD the gradient into it in place
    (accumulate epilogue) and return ``None`` to autograd, which saves one add kernel and one
    temporary per parameter.  Otherwise ``None`` (ordinary autograd accumulation)."""
    if p is not None and getattr(p, "_hicgat_grad_sink", False) and p.grad is not None:
        return p.grad
    return None


def _dev_check(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.HicgatUnavailable("hicgat ops need CUDA (HIP) tensors; got a CPU tensor")


_ACTS = {None: 0, "relu": 1}
# the single-GPU GATConv's gather-free rows pass (hicgat_gat_agg_bwd_rows) in the one-kernel tail
# backward's epilogue when that tail consumes the layer's output (hicgat_tail_bwd, HICGAT_TAIL_ROWS); 0: the
# separate pass
FUSE_ROWS = os.environ.get("HICGAT_FUSE_ROWS", "1") != "0"
# the tail's weight pack written by the step's first launch (step_pack); 0: its own launch in the forward
STEP_PACK = os.environ.get("HICGAT_STEP_PACK", "1") != "0"


class _GATConvFn(torch.autograd.Function):
    """PyG 1.7.2 GATConv (+ an optional fused relu epilogue, act=1).  With gradients enabled the
    aggregation also emits out2 / S3 (include/hicgat.h), so the destination half of the backward
    is a streaming pass (``agg_bwd_rows``) and only the source half gathers."""

    @staticmethod
    def forward(ctx, x, W, att_l, att_r, bias, rowptr, col, negative_slope, act, tiles=None, tmap=None, drop=None):
        # tmap: only from _GATConvAttnFn / _GATConvDropFn, which run this body and then add the attention
        # weights; drop: only from _GATConvDropFn, the (p, seed, step_ctr, step_value, site) of
        # kernels.agg_fwd_act -- attention dropout in the two gathers (never with tiles)
        _lib.lib()
        _dev_check(x, W, att_l, att_r, bias, rowptr, col)
        K = kernels.default()
        x = x.contiguous().float()
        W = W.contiguous()
        al = att_l.contiguous()
        ar = att_r.contiguous()
        N = x.shape[0]
        H = al.shape[-2]
        h, a_src, a_dst = K.linear_att(x, W, al, ar)
        D = h.shape[1]
        b = bias if bias is not None else torch.zeros(D, dtype=torch.float32, device=x.device)
        out = torch.empty((N, D), dtype=torch.float32, device=x.device)
        row_stats = torch.empty((N, 4 * H), dtype=torch.float32, device=x.device)
        train = any(ctx.needs_input_grad[:5])
        out2 = torch.empty((N, D), dtype=torch.float32, device=x.device) if train else None
        K.agg_fwd_act(rowptr, col, 0, N, h, a_src, a_dst, b, negative_slope, act, out, out2, row_stats, drop=drop,
                      tiles=tiles)
        ctx.tiles = tiles
        ctx.drop = drop
        ctx.rows_state = None
        if train:
            ctx.save_for_backward(x, W, al, ar, h, a_src, a_dst, row_stats, rowptr, col, out, out2, b)
            if FUSE_ROWS and (H, D // H) == (2, 256):
                # (only this shape: the fused epilogue writes (2, 256)-layout row stats)
                # the one-kernel tail that consumes ``out`` may run this layer's rows pass in its
                # backward's epilogue (_FusedTailFn; hicgat_tail_bwd, HICGAT_TAIL_ROWS): it finds these
                # operands on ``out`` and records the dout it wrote in the shared state
                ctx.rows_state = {"dout": None}
                out._hicgat_rows = (act, out2, row_stats, b, ctx.rows_state)
        ctx.has_bias = bias is not None
        ctx.ns = float(negative_slope)
        ctx.act = act
        ctx.params = (W, att_l, att_r, bias)
        if tmap is not None:
            alpha = torch.empty((col.numel(), H), dtype=torch.float32, device=x.device)
            K.gat_alpha(rowptr, col, D // H, a_src, a_dst, row_stats, negative_slope, alpha)
            if train:
                ctx.save_for_backward(x, W, al, ar, h, a_src, a_dst, row_stats, rowptr, col, out, out2, b, alpha, tmap)
            return out, alpha
        return out

    @staticmethod
    def backward(ctx, dout, G=None):
        # G: only from _GATConvAttnFn, dL/dalpha [nnz, H]; its share is added after the source pass
        K = kernels.default()
        x, W, al, ar, h, a_src, a_dst, row_stats, rowptr, col, out, out2, b = ctx.saved_tensors[:13]
        N = x.shape[0]
        H = al.shape[-2]
        fused = ctx.rows_state is not None and ctx.rows_state["dout"] is not None
        if fused:
            # the tail's backward ran this layer's rows pass: dout (relu'd) and row_stats[:, 4:8] are
            # written, and the gradient that reached us must be exactly the dout it returned (a second
            # consumer of ``out`` would have added into it: then the rows pass saw only a part)
            if dout.data_ptr() != ctx.rows_state["dout"].data_ptr():
                raise RuntimeError("the GATConv output fed more than the fused tail: its rows pass was fused "
                                   "into the tail's backward (set HICGAT_FUSE_ROWS=0 for such a model)")
            ctx.rows_state["dout"] = None
        elif ctx.act:
            g, dout = dout.contiguous(), torch.empty_like(dout)
            K.agg_bwd_rows(0, N, ctx.act, g, out, b, out2, dout, row_stats)
        else:
            dout = dout.contiguous()
            K.agg_bwd_rows(0, N, 0, dout, out, b, out2, None, row_stats)
        fork = side_mark()   # the tail's queued dW / db launches run beside the source pass below
        dh = torch.empty_like(h)
        da_src = torch.empty_like(a_src)
        pW, pl, pr, pb = ctx.params
        sinks = (_sink(pl), _sink(pr), _sink(pb) if ctx.has_bias else None)
        use_sinks = all(t is not None for t in sinks)
        stamped = ctx.tiles is None   # the untiled pass alone
        if stamped:
            streams.stamp("src_begin")
        K.agg_bwd_src(rowptr, col, 0, N, h, a_src, a_dst, row_stats, dout, al, ar, ctx.ns, dh, da_src, drop=ctx.drop,
                      tiles=ctx.tiles)
        if stamped:
            streams.stamp("src_end")
        side_flush(after=fork)
        if G is not None:
            # the backward is linear in (dout, G): G's share adds onto dh, da_src and row_stats' da_dst
            # slot, and the parameter gradients, lin_l's dW and dx below see the totals
            alpha, tmap = ctx.saved_tensors[13:]
            c, dd = torch.empty_like(a_src), torch.empty_like(a_src)
            K.gat_alpha_bwd_dst(rowptr, col, h.shape[1] // H, a_src, a_dst, alpha, G, ctx.ns, c, dd)
            K.gat_alpha_bwd_src(rowptr, col, tmap, a_src, a_dst, alpha, G, c, dd, al, ar, ctx.ns, dh, da_src,
                                row_stats)
        # after the gathers: the GAT column sums, then lin_l's dW on this stream (with the held
        # first-block dW: BIG_GROUP).  The column sums on a side stream beside the grouped dW launch:
        # 1.964 / 1.970 vs 1.877 / 1.872 ms per step (profiles/r04l_ab_single_gpu.txt)
        if use_sinks:
            K.param_grad(h, dout, da_src, row_stats, H, out=(sinks[0].view(-1), sinks[1].view(-1), sinks[2]),
                         accumulate=True)
            datt_l = datt_r = dbias = None
        else:
            datt_l, datt_r, dbias = K.param_grad(h, dout, da_src, row_stats, H)
            datt_l, datt_r = datt_l.view(al.shape), datt_r.view(ar.shape)
            dbias = dbias if ctx.has_bias else None
        dW = None
        if ctx.needs_input_grad[1]:
            gW = _sink(pW)
            # the held big dW jobs and lin_l's as one grouped launch (BIG_GROUP), else lin_l's alone
            if gW is None or not paramgrads.flush_held(K, [WeightGradJob(dh, x, gW)]):
                dW = weight_grad(K, dh, x, out=gW, accumulate=gW is not None)
                if gW is not None:
                    dW = None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.gemm(0, 1, N, x.shape[1], h.shape[1], dh, W, torch.empty_like(x), name="gemm_dx")
        return (dx, dW, datt_l, datt_r, dbias, None, None, None, None, None)


class _GATConvAttnFn(torch.autograd.Function):
    """``_GATConvFn`` that also returns the attention weights alpha [nnz, H] (self-looped CSR order;
    PyG's ``return_attention_weights=True``) as a second differentiable output.  The forward is
    ``_GATConvFn``'s plus one pass that writes alpha from the row statistics (gat_attn.hip).  The
    backward takes (dout, dalpha): without a dalpha it is ``_GATConvFn.backward`` launch for launch;
    with one, two more passes add its share after the source pass; a missing dout counts as zeros."""

    @staticmethod
    def forward(ctx, x, W, att_l, att_r, bias, rowptr, col, negative_slope, act, tiles, tmap):
        ctx.set_materialize_grads(False)    # an unused output's gradient arrives as None, not as zeros
        return _GATConvFn.forward(ctx, x, W, att_l, att_r, bias, rowptr, col, negative_slope, act, tiles, tmap)

    @staticmethod
    def backward(ctx, dout, dalpha):
        if dout is None:
            if dalpha is None:
                return (None,) * 11
            dout = torch.zeros_like(ctx.saved_tensors[10])
        G = None if dalpha is None else dalpha.contiguous().float()
        return _GATConvFn.backward(ctx, dout, G) + (None,)


class _GATConvDropFn(torch.autograd.Function):
    """``_GATConvFn`` with attention dropout (PyG's ``F.dropout(alpha, p, training)`` in ``message``): the
    DROP forms of the forward gather and of the source pass, the gather form at every shape (no tiles),
    the rows pass and its fused-tail link as they are.  The forward keeps its own copy of the state's
    step count, so its backward regenerates the forward's mask whatever the state has counted since.
    With a ``tmap`` it also returns alpha [nnz, H] -- the pre-dropout softmax, as PyG's ``_alpha`` -- and
    takes (dout, dalpha) like ``_GATConvAttnFn``; dalpha's share sees no mask."""

    @staticmethod
    def forward(ctx, x, W, att_l, att_r, bias, rowptr, col, negative_slope, act, tmap, p, state, site):
        ctx.set_materialize_grads(False)
        _dev_check(x, state.counter)
        drop = (p, state.seed, state.counter.clone(), 0, site)
        return _GATConvFn.forward(ctx, x, W, att_l, att_r, bias, rowptr, col, negative_slope, act, None, tmap, drop)

    @staticmethod
    def backward(ctx, dout, dalpha=None):
        if dout is None:
            if dalpha is None:
                return (None,) * 13
            dout = torch.zeros_like(ctx.saved_tensors[10])
        G = None if dalpha is None else dalpha.contiguous().float()
        return _GATConvFn.backward(ctx, dout, G) + (None,) * 3


def attention_entropy(alpha):
    """-sum(alpha * log(alpha + 1e-12)) over every (edge, head) of the attention weights, in plain torch
    ops (the eps of the reference's ``entropy_of_predictions``, HiC_GAT_generalize_directly.py:54-58)."""
    return -(alpha * torch.log(alpha + 1e-12)).sum()


# target workgroups of a split-K weight-gradient GEMM.  Alone, 512 measured best at N = 20000 (0.094
# vs 0.108 ms for 512x512x20000 at 1024, fewer fp32 slabs to add; profiles/r01_kbench_x3_sliced.txt);
# in the step, where the big dW GEMMs run two at a time beside each other after the source pass,
# 256 (half the slabs to add) is faster: 1.927 vs 1.942 ms per step, three A/B rounds
# (profiles/r02d_ab_step.txt)
_DW_BLOCKS = int(os.environ.get("HICGAT_DW_BLOCKS", "256"))


def _splits(m, n, k, target=None):
    """K-split for a weight-gradient GEMM whose K is the node count: enough workgroups to fill
    the 256 CUs, each split at least 256 rows deep (the library's hicgat_gemm_wgrad_splits)."""
    return _lib.load().hicgat_gemm_wgrad_splits(m, n, k, _DW_BLOCKS if target is None else target)


def weight_grad(K, dy, x, out=None, accumulate=False, impl=None):
    """dW = dy^T x (Linear / lin_l weight gradient), K = rows, split-K MFMA GEMM."""
    rows, m = dy.shape
    n = x.shape[1]
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=dy.device)
    return K.gemm(1, 1, m, n, rows, dy, x, out, accumulate=accumulate, splits=_splits(m, n, rows), name="gemm_dw",
                  impl=impl)


def _weight_grad_to(K, p, dy, x):
    """dW = dy^T x into the parameter's sink (returns None) or a new tensor (returned)."""
    g = _sink(p)
    if g is not None:
        param_launch(lambda: weight_grad(K, dy, x, out=g, accumulate=True), dy, x,
                     work=dy.shape[0] * dy.shape[1] * x.shape[1], job=WeightGradJob(dy, x, g))
        return None
    return weight_grad(K, dy, x)


def _wb_grad_to(K, pW, pb, dy, x, need_w=True, need_b=True):
    """A Linear's dW = dy^T x and db = column sums of dy: ONE fp32 GEMM launch computes both
    (``hicgat_gemm_wgrad``, db from the staged dY tiles).  Into the parameters' sinks (returns
    (None, None); on the side stream when overlapping) or new tensors (returned).  Falls back to
    separate GEMM / column-sum launches when only one of the two is wanted, when the sinks are
    mixed."""
    need_b = need_b and pb is not None
    if not need_w:
        return None, (_bias_grad_to(K, pb, dy) if need_b else None)
    gW = _sink(pW)
    gb = _sink(pb) if need_b else None
    rows, m = dy.shape
    n = x.shape[1]
    sp = _splits(m, n, rows)
    if gW is not None and (gb is not None or not need_b):
        param_launch(lambda: K.wgrad(dy, x, gW, gb, accumulate=True, splits=sp), dy, x, work=rows * m * n,
                     job=WeightGradJob(dy, x, gW, gb))
        return None, None
    if gW is None and (not need_b or _sink(pb) is None):
        dW = torch.empty((m, n), dtype=torch.float32, device=dy.device)
        db = torch.empty(m, dtype=torch.float32, device=dy.device) if need_b else None
        K.wgrad(dy, x, dW, db, splits=sp)
        return dW, db
    return _weight_grad_to(K, pW, dy, x), _bias_grad_to(K, pb, dy)


def _bias_grad_to(K, p, dy):
    """db = column sums of dy into the parameter's sink (returns None) or a new tensor."""
    g = _sink(p)
    if g is not None:
        param_launch(lambda: K.colsum(dy, g, accumulate=True), dy, job=ColsumJob(dy, g))
        return None
    return K.colsum(dy, torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device))


class _LinearFn(torch.autograd.Function):
    """torch.nn.Linear (models.py:616-632 layers) forward/backward on the fp32 MFMA GEMM."""

    @staticmethod
    def forward(ctx, x, W, b):
        K = kernels.default()
        x = x.contiguous()
        M = x.shape[0]
        n_out, n_in = W.shape
        y = torch.empty((M, n_out), dtype=torch.float32, device=x.device)
        K.gemm(0, 0, M, n_out, n_in, x, W.contiguous(), y, bias=b, name="gemm_fwd")
        ctx.save_for_backward(x, W)
        ctx.has_bias = b is not None
        ctx.params = (W, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, _ = ctx.saved_tensors
        need_dx, need_w, need_b = ctx.needs_input_grad
        return _linear_backward(*ctx.params, x, dy, need_dx, need_w, ctx.has_bias and need_b)


def _linear_backward(W, b, x, dy, need_dx=True, need_w=True, need_b=True):
    """``_LinearFn``'s backward on its operands: (dx, dW, db)."""
    K = kernels.default()
    dy = dy.contiguous()
    n_out, n_in = W.shape
    dx = None
    if need_dx:
        dx = K.gemm(0, 1, x.shape[0], n_in, n_out, dy, W.contiguous(), torch.empty_like(x), name="gemm_dx")
    return (dx,) + _wb_grad_to(K, W, b, dy, x, need_w=need_w, need_b=need_b)


def linear(x, W, b=None):
    """F.linear(x, W, b) on the MI355X GEMM kernels (CUDA tensors only)."""
    _dev_check(x, W, b)
    return _LinearFn.apply(x, W, b)


def _act_code(act):
    """``None`` / "none", "relu", "leaky_relu" (slope 0.01, torch's default) or ("leaky_relu", slope)
    -> (HICGAT_ACT_* code, slope)."""
    if isinstance(act, tuple) and len(act) == 2 and act[0] == "leaky_relu":
        return kernels.HipKernels.ACT_LEAKY_RELU, float(act[1])
    if act in (None, "none"):
        return kernels.HipKernels.ACT_NONE, 0.0
    if act == "relu":
        return kernels.HipKernels.ACT_RELU, 0.0
    if act == "leaky_relu":
        return kernels.HipKernels.ACT_LEAKY_RELU, 0.01
    raise ValueError(f"act must be None, 'relu', 'leaky_relu' or ('leaky_relu', slope); got {act!r}")


def _rows16(t):
    """``t`` as the dropout kernels read it: unit column stride, rows a multiple of 4 floats apart,
    16-byte aligned (a copy only if it is not)."""
    if t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


class _ActDropoutFn(torch.autograd.Function):
    """act -> Dropout(p) as one pass (dropout.hip); saves only its output: the backward reads the
    activation's branch and the mask from y's sign (include/hicgat.h hicgat_act_dropout_bwd)."""

    @staticmethod
    def forward(ctx, x, act, slope, p, state, site, row_offset):
        K = kernels.default()
        x = _rows16(x)
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        K.act_dropout_fwd(x, act, slope, p, state.seed, state.counter, 0, site, row_offset, y)
        ctx.save_for_backward(y)
        ctx.cfg = (act, slope, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        act, slope, p = ctx.cfg
        dy = _rows16(dy)
        dx = kernels.default().act_dropout_bwd(dy, y, act, slope, p, torch.empty_like(y))
        return dx, None, None, None, None, None, None


def act_dropout(x, act, p, state, site, row_offset=0):
    """dropout(act(x), p) of a training forward: ``y = kept ? act(x) / (1 - p) : 0`` with the mask of
    (state.seed, the state's device step count, site, row_offset + row, column) -- see
    ``dropout.DropoutState``.  ``x``: float32 [rows, W] on the device, W % 4 == 0.  ``site``: the index
    of this call within the forward; ``row_offset``: the global index of x's first row (a row shard
    gets the bits of the whole tensor)."""
    from .dropout import check_p
    p = check_p(p)
    code, slope = _act_code(act)
    _dev_check(x)
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] % 4:
        raise ValueError(f"act_dropout needs a float32 [rows, W] tensor with W % 4 == 0; got {x.dtype} "
                         f"{tuple(x.shape)}")
    if x.requires_grad and code == kernels.HipKernels.ACT_NONE:
        raise NotImplementedError("act_dropout(act=None) has no backward (a zero output is ambiguous there)")
    if int(site) < 0 or int(row_offset) < 0:
        raise ValueError("site and row_offset must be >= 0")
    return _ActDropoutFn.apply(x, code, slope, p, state, int(site), int(row_offset))


def dropout_mask(rows, W, p, seed, step, site, row_offset=0, device="cuda"):
    """The keep mask (bool [rows, W]) the dropout kernels use for these arguments (tests, tools)."""
    from .dropout import check_p
    p = check_p(p)
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.HicgatUnavailable("hicgat ops need a CUDA (HIP) device; got " + str(device))
    m = torch.empty((int(rows), int(W)), dtype=torch.uint8, device=device)
    kernels.default().dropout_mask(m, p, int(seed) & ((1 << 64) - 1), None, int(step), site, row_offset)
    return m.bool()


def attention_dropout_mask(adj, H, p, seed, step, site):
    """The keep mask (bool [nnz, H], self-looped CSR order: ``adj.rowptr32`` / ``adj.col32``) that
    attention dropout uses for these arguments (tests, tools)."""
    from .dropout import check_p
    p = check_p(p)
    if adj.rowptr32 is None or not adj.rowptr32.is_cuda:
        raise _lib.HicgatUnavailable("attention_dropout_mask needs an Adj on a CUDA (HIP) device")
    m = torch.empty((adj.col32.numel(), int(H)), dtype=torch.uint8, device=adj.col32.device)
    kernels.default().attn_mask(adj.rowptr32, adj.col32, int(H), m,
                                (p, int(seed) & ((1 << 64) - 1), None, int(step), _attn_site(site)))
    return m.bool()


class _DualLinearFn(torch.autograd.Function):
    """Two Linear layers on the same input (models.py:638-639 / 646-647: dense* and align_dense*)
    as ONE GEMM over [W1; W2]: the input is read once; the backward adds both input gradients
    inside the GEMM (accumulate) instead of a separate add."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2):
        K = kernels.default()
        x = x.contiguous()
        M = x.shape[0]
        n1, n2 = W1.shape[0], W2.shape[0]
        Wc = torch.cat([W1, W2]).contiguous()
        bc = torch.cat([b1, b2]).contiguous()
        Y = torch.empty((M, n1 + n2), dtype=torch.float32, device=x.device)
        K.gemm(0, 0, M, n1 + n2, x.shape[1], x, Wc, Y, bias=bc, name="gemm_fwd")
        ctx.save_for_backward(x, W1, W2)
        ctx.params = (W1, b1, W2, b2)
        return Y[:, :n1], Y[:, n1:]

    @staticmethod
    def backward(ctx, dy1, dy2):
        K = kernels.default()
        x, W1, W2 = ctx.saved_tensors
        M, n_in = x.shape
        dy1 = dy1.contiguous()
        dy2 = dy2.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.gemm(0, 1, M, n_in, W1.shape[0], dy1, W1, torch.empty_like(x), name="gemm_dx")
            K.gemm(0, 1, M, n_in, W2.shape[0], dy2, W2, dx, accumulate=True, name="gemm_dx")
        pW1, pb1, pW2, pb2 = ctx.params
        dW1, db1 = _wb_grad_to(K, pW1, pb1, dy1, x)
        dW2, db2 = _wb_grad_to(K, pW2, pb2, dy2, x)
        return dx, dW1, db1, dW2, db2


def dual_linear(x, lin1, lin2):
    _dev_check(x)
    return _DualLinearFn.apply(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias)


# ---- the LayerNorm row pass (ln_act.hip), the flagship's and the other zoo models': LayerNorm -> act (+ res)
# (-> LayerNorm) ----
LN_WIDTHS = (32, 64, 128, 256, 512)


def _ln_act_code(act):
    """The activation of the LayerNorm tails and of ``ops.act``: ``None`` / "none", "relu", "leaky_relu"
    (slope 0.01), ("leaky_relu", slope) or "gelu" (the erf form, F.gelu's default) -> (HICGAT_ACT_* code,
    slope).  A parser of its own: the dropout and BatchNorm ops (``_act_code``) have no gelu."""
    if isinstance(act, tuple) and len(act) == 2 and act[0] == "leaky_relu":
        if not float(act[1]) > 0.0:
            raise ValueError(f"leaky_relu needs a slope > 0; got {act[1]!r}")
        return kernels.HipKernels.ACT_LEAKY_RELU, float(act[1])
    if act in (None, "none"):
        return kernels.HipKernels.ACT_NONE, 0.0
    if act == "relu":
        return kernels.HipKernels.ACT_RELU, 0.0
    if act == "leaky_relu":
        return kernels.HipKernels.ACT_LEAKY_RELU, 0.01
    if act == "gelu":
        return kernels.HipKernels.ACT_GELU, 0.0
    raise ValueError(f"activation must be None, 'relu', 'leaky_relu', ('leaky_relu', slope) or 'gelu'; got {act!r}")


def _ln_check(norm, what="norm"):
    """The width of a ``torch.nn.LayerNorm`` the row pass takes; refuses everything else, by name."""
    if not isinstance(norm, torch.nn.LayerNorm):
        raise TypeError(f"{what} must be a torch.nn.LayerNorm; got {type(norm).__name__}")
    if not norm.elementwise_affine or norm.weight is None or norm.bias is None:
        raise NotImplementedError(f"{what}: LayerNorm(elementwise_affine=False) or without a bias is not implemented")
    if len(norm.normalized_shape) != 1:
        raise NotImplementedError(f"{what}: a {len(norm.normalized_shape)}-D normalized_shape "
                                  f"{tuple(norm.normalized_shape)} is not implemented (rows of one width only)")
    W = int(norm.normalized_shape[0])
    if W not in LN_WIDTHS:
        raise NotImplementedError(f"{what}: LayerNorm widths {LN_WIDTHS} are implemented; got {W}")
    return W


def _ln_pair_check(norm, norm2):
    W = _ln_check(norm)
    if norm2 is not None and _ln_check(norm2, "norm2") != W:
        raise ValueError(f"norm2 must have norm's width {W}; got {int(norm2.normalized_shape[0])}")
    return W


def _rows_f32(t, W, what):
    if t.dim() != 2 or t.dtype != torch.float32 or t.shape[1] != W:
        raise ValueError(f"{what} must be a float32 [rows, {W}] tensor; got {t.dtype} {tuple(t.shape)}")


def _ln_act_bwd(K, cfg, params, dz, y, stats, res, stats2, dy, dres=None):
    """The row pass of the backward (dy, and ``dres=``) with its parameter sums, which go: without every sink
    into new tensors (returned); with them and nothing overlapping straight into the sinks; while overlapping
    into a workspace as partials, and adding those to the sinks is queued side work (it has no grouped form).
    Returns (dgamma, dbeta, dgamma2, dbeta2) for autograd."""
    code, slope = cfg
    gamma, beta, gamma2, beta2 = params
    n2 = gamma2 is not None
    kw = dict(res=res if n2 else None, gamma2=gamma2, row_stats2=stats2, dres=dres)
    sinks = [_sink(p) for p in ((gamma, beta, gamma2, beta2) if n2 else (gamma, beta))]
    if any(s is None for s in sinks):
        dg, db = torch.empty_like(gamma), torch.empty_like(beta)
        dg2, db2 = (torch.empty_like(gamma2), torch.empty_like(beta2)) if n2 else (None, None)
        K.ln_act_res_bwd(dz, y, stats, gamma, beta, code, slope, dy, dg, db, dgamma2=dg2, dbeta2=db2, **kw)
        return dg, db, dg2, db2
    sinks += [None, None] if not n2 else []
    if not paramgrads.overlapping():
        K.ln_act_res_bwd(dz, y, stats, gamma, beta, code, slope, dy, sinks[0], sinks[1], dgamma2=sinks[2],
                         dbeta2=sinks[3], accumulate=True, **kw)
    else:
        W = y.shape[1]
        ws = K.ln_act_workspace(W, n2, y.device)
        K.ln_act_res_bwd(dz, y, stats, gamma, beta, code, slope, dy, None, None, ws=ws, **kw)
        param_launch(lambda: K.ln_act_res_bwd_params(W, *sinks, ws, accumulate=True), ws)
    return None, None, None, None


class _LnActResFn(torch.autograd.Function):
    """LN2(act(LN(y)) + res) in one pass (ln_act.hip); ``res`` and the second norm are optional."""

    @staticmethod
    def forward(ctx, y, res, gamma, beta, gamma2, beta2, eps, eps2, code, slope):
        K = kernels.default()
        M, W = y.shape
        n2 = gamma2 is not None
        z = torch.empty((M, W), dtype=torch.float32, device=y.device)
        stats = torch.empty((M, 2), dtype=torch.float32, device=y.device)
        stats2 = torch.empty((M, 2), dtype=torch.float32, device=y.device) if n2 else None
        K.ln_act_res_fwd(y, gamma, beta, eps, code, slope, res, z, stats, gamma2, beta2, eps2, stats2)
        ctx.save_for_backward(y, stats, res if n2 else None, stats2)
        ctx.has_res = res is not None
        ctx.cfg = (code, slope)
        ctx.params = (gamma, beta, gamma2, beta2)
        return z

    @staticmethod
    def backward(ctx, dz):
        dy, dres, dg, db, dg2, db2 = _ln_act_res_backward(ctx.cfg, ctx.params, ctx.has_res, *ctx.saved_tensors, dz)
        return dy, dres, dg, db, dg2, db2, None, None, None, None


def _ln_act_res_backward(cfg, params, has_res, y, stats, res, stats2, dz):
    """``_LnActResFn``'s backward on its operands (``res``: the forward's, read with the second norm only):
    (dy, dres, dgamma, dbeta, dgamma2, dbeta2)."""
    K = kernels.default()
    n2 = params[2] is not None
    dz = dz.contiguous()
    dy = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    # without the second norm d(res) is dz itself; with it the kernel writes du
    dres = torch.empty_like(dy) if (has_res and n2) else None
    dg, db, dg2, db2 = _ln_act_bwd(K, cfg, params, dz, y, stats, res, stats2, dy, dres)
    return dy, ((dres if n2 else dz) if has_res else None), dg, db, dg2, db2


def ln_act_res(y, norm, act, res=None, norm2=None):
    """``norm2(act(norm(y)) + res)`` for ``torch.nn.LayerNorm``s of one width in ``LN_WIDTHS`` (``res`` and
    ``norm2`` optional), as one row pass forward and one backward.  ``act``: None, "relu", "leaky_relu",
    ("leaky_relu", slope) or "gelu"."""
    W = _ln_pair_check(norm, norm2)
    code, slope = _ln_act_code(act)
    _rows_f32(y, W, "y")
    if res is not None:
        _rows_f32(res, W, "res")
        if res.shape != y.shape:
            raise ValueError(f"res must have y's shape {tuple(y.shape)}; got {tuple(res.shape)}")
    _dev_check(y, res)
    if y.stride(1) != 1:
        y = y.contiguous()
    if res is not None and res.stride(1) != 1:
        res = res.contiguous()
    g2, b2, e2 = (norm2.weight, norm2.bias, norm2.eps) if norm2 is not None else (None, None, 0.0)
    return _LnActResFn.apply(y, res, norm.weight, norm.bias, g2, b2, norm.eps, e2, code, slope)


class _ActFn(torch.autograd.Function):
    """Elementwise gelu / leaky_relu (ln_act.hip); the backward reads the saved input."""

    @staticmethod
    def forward(ctx, x, code, slope):
        x = x.contiguous()
        y = kernels.default().act_fwd(x, code, slope, torch.empty_like(x))
        ctx.save_for_backward(x)
        ctx.cfg = (code, slope)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        return kernels.default().act_bwd(dy.contiguous(), x, *ctx.cfg, torch.empty_like(x)), None, None


def act(x, act):
    """F.gelu(x) ("gelu", the erf form) or F.leaky_relu(x, slope) ("leaky_relu", ("leaky_relu", slope)) of a
    float32 [rows, W] device tensor, W % 4 == 0, as one launch each way."""
    code, slope = _ln_act_code(act)
    if code not in (kernels.HipKernels.ACT_GELU, kernels.HipKernels.ACT_LEAKY_RELU):
        raise ValueError(f"ops.act runs 'gelu' and 'leaky_relu'; got {act!r} (relu runs in the GATConv's epilogue)")
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] % 4:
        raise ValueError(f"ops.act needs a float32 [rows, W] tensor with W % 4 == 0; got {x.dtype} {tuple(x.shape)}")
    _dev_check(x)
    return _ActFn.apply(x, code, slope)


class _BnActDropoutFn(torch.autograd.Function):
    """BatchNorm1d -> act -> Dropout(p) (batchnorm.hip; models.py:288-291).  A training-mode forward
    takes the batch statistics (two launches), updates the module's buffers on the device and applies
    in one pass; an eval-mode one is the apply pass alone on the running buffers.  Saves its input y,
    the column statistics and its output z (the activation's branch and the mask are read from z's
    sign, as in ``_ActDropoutFn``; nothing for act = none)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, bn, act, slope, p, state, site, row_offset):
        K = kernels.default()
        y = _rows16(y)
        M, W = y.shape
        z = torch.empty((M, W), dtype=torch.float32, device=y.device)
        stats = None
        if bn.training:
            stats = torch.empty((4, W), dtype=torch.float32, device=y.device)
            K.bn_stats(y, bn.eps, bn.momentum, stats, bn.running_mean, bn.running_var, bn.num_batches_tracked)
        seed, ctr = (state.seed, state.counter) if p > 0.0 else (0, None)
        K.bn_act_dropout_fwd(y, gamma, beta, stats, bn.running_mean, bn.running_var, bn.eps, act, slope, p, seed, ctr,
                             0, site, row_offset, z)
        saved = [y, gamma] + ([stats] if stats is not None else []) + ([z] if act != K.ACT_NONE else [])
        ctx.save_for_backward(*saved)
        ctx.cfg = (act, slope, p, bn.eps, stats is not None)
        ctx.running = None if stats is not None else (bn.running_mean, bn.running_var)   # eval: fixed statistics
        ctx.params = (gamma, beta)
        return z

    @staticmethod
    def backward(ctx, dz):
        K = kernels.default()
        act, slope, p, eps, batch = ctx.cfg
        saved = list(ctx.saved_tensors)
        y, gamma = saved[:2]
        stats = saved[2] if batch else None
        z = saved[-1] if act != K.ACT_NONE else None
        rm, rv = ctx.running if ctx.running is not None else (None, None)
        dz = _rows16(dz)
        M, W = y.shape
        dy = torch.empty((M, W), dtype=torch.float32, device=y.device)
        sg, sb = _sink(ctx.params[0]), _sink(ctx.params[1])
        args = (dz, z, y, gamma, stats, rm, rv, eps, act, slope, p, dy)
        if sg is not None and sb is not None and not paramgrads.overlapping():
            K.bn_act_dropout_bwd(*args, sg, sb, accumulate=True)
            return (dy,) + (None,) * 9
        if sg is not None and sb is not None:
            # dy needs the sums on this stream; adding them to the sinks is side work like every
            # other parameter gradient (a one-row column sum of [dgamma | dbeta])
            ws = K.bn_workspace(M, W, y.device)
            K.bn_act_dropout_bwd(*args, None, None, ws=ws)
            sums = ws.view(torch.float32)[:2 * W].view(1, 2 * W)
            pairs = [(sums, _joined(sg, sb))] if _adjacent(sg, sb) else [(sums[:, :W], sg), (sums[:, W:], sb)]
            for src, dst in pairs:
                param_launch(lambda src=src, dst=dst: K.colsum(src, dst, accumulate=True), ws,
                             job=ColsumJob(src, dst))
            return (dy,) + (None,) * 9
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        K.bn_act_dropout_bwd(*args, dgamma, dbeta)
        return (dy, dgamma, dbeta) + (None,) * 7


def bn_act_dropout(y, bn, act, state=None, site=None, row_offset=0):
    """dropout(act(bn(y))) for a plain ``torch.nn.BatchNorm1d`` ``bn`` (it only holds the parameters
    and buffers) on y [rows, W], float32 on the device, W % 64 == 0, 64 <= W <= 1024.

    ``bn.training`` selects batch or running statistics as in torch; a training-mode call updates
    ``running_mean`` / ``running_var`` / ``num_batches_tracked`` on the device, with or without
    ``torch.no_grad()``.  ``act``: as ``act_dropout``.  ``state`` (a ``DropoutState`` with its ``p``),
    ``site``, ``row_offset``: the Dropout after the activation, with ``act_dropout``'s mask; without a
    state (or with p = 0) the result is act(bn(y))."""
    if not isinstance(bn, torch.nn.BatchNorm1d):
        raise TypeError(f"bn_act_dropout needs a torch.nn.BatchNorm1d; got {type(bn).__name__}")
    if not bn.affine:
        raise NotImplementedError("bn_act_dropout: BatchNorm1d(affine=False) is not implemented")
    if not bn.track_running_stats:
        raise NotImplementedError("bn_act_dropout: BatchNorm1d(track_running_stats=False) is not implemented")
    if bn.momentum is None:
        raise NotImplementedError("bn_act_dropout: BatchNorm1d(momentum=None) (cumulative average) is not "
                                  "implemented")
    code, slope = _act_code(act)
    p = 0.0
    if state is not None:
        from .dropout import check_p
        if state.p is None or site is None:
            raise ValueError("bn_act_dropout with a DropoutState needs the state's p and a site")
        p = check_p(state.p)
    site = 0 if site is None else int(site)
    if site < 0 or int(row_offset) < 0:
        raise ValueError("site and row_offset must be >= 0")
    W = bn.num_features
    if y.dim() != 2 or y.dtype != torch.float32 or y.shape[1] != W:
        raise ValueError(f"bn_act_dropout needs a float32 [rows, {W}] tensor; got {y.dtype} {tuple(y.shape)}")
    if W % 64 or not 64 <= W <= 1024:
        raise NotImplementedError(f"bn_act_dropout runs widths 64, 128, ..., 1024; got {W}")
    if bn.training and y.shape[0] < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(y.shape)}")
    if y.shape[0] < 1:
        raise ValueError("bn_act_dropout needs at least one row")
    if (y.requires_grad or bn.weight.requires_grad) and code == kernels.HipKernels.ACT_NONE and p > 0.0:
        raise NotImplementedError("bn_act_dropout(act=None) with dropout has no backward (a zero output is "
                                  "ambiguous there)")
    _dev_check(y, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked)
    return _BnActDropoutFn.apply(y, bn.weight, bn.bias, bn, code, slope, p, state, site, int(row_offset))


def _adjacent(a, b):
    """``b`` starts right where ``a`` ends in the SAME storage (two views into FlatAdam's flat
    buffer): the pair is then one [a; b] tensor without a copy.  Two separate allocations that
    merely happen to sit back to back (the caching allocator packs small blocks into one segment)
    do not qualify: a view cannot span two storages."""
    return (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
            and b.data_ptr() == a.data_ptr() + a.numel() * a.element_size())


def _joined(a, b):
    """[a; b] along dim 0 -- a view when the two are adjacent (``flat_parameters`` order)."""
    if _adjacent(a, b):
        return torch.as_strided(a, (a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a.stride())
    return torch.cat([a, b])


def _dual_param_grads(K, W1, b1, W2, b2, dY, x):
    """dW / db of a dual-Linear pair from its packed output gradient dY = [dy1 | dy2] and input x:
    into the parameters' sinks (queued side work; returns Nones) or new tensors (returned)."""
    M, w = dY.shape[0], W1.shape[0]
    sW1, sW2, sb1, sb2 = _sink(W1), _sink(W2), _sink(b1), _sink(b2)
    dW1 = dW2 = db1 = db2 = None
    w_pair = sW1 is not None and sW2 is not None and _adjacent(sW1, sW2)
    b_pair = sb1 is not None and sb2 is not None and _adjacent(sb1, sb2)
    if w_pair and b_pair:
        # [dW1; dW2] and [db1; db2] of the pair in ONE GEMM launch (hicgat_gemm_wgrad)
        gWj, gbj, sp = _joined(sW1, sW2), _joined(sb1, sb2), _splits(2 * w, x.shape[1], M)
        param_launch(lambda: K.wgrad(dY, x, gWj, gbj, accumulate=True, splits=sp), dY, x,
                     work=M * 2 * w * x.shape[1], job=WeightGradJob(dY, x, gWj, gbj))
    else:
        if w_pair:
            gWj = _joined(sW1, sW2)
            param_launch(lambda: weight_grad(K, dY, x, out=gWj, accumulate=True), dY, x,
                         job=WeightGradJob(dY, x, gWj))
        else:
            dW1 = _weight_grad_to(K, W1, dY[:, :w], x)
            dW2 = _weight_grad_to(K, W2, dY[:, w:], x)
        if b_pair:
            gbj = _joined(sb1, sb2)
            param_launch(lambda: K.colsum(dY, gbj, accumulate=True), dY, job=ColsumJob(dY, gbj))
        else:
            db1 = _bias_grad_to(K, b1, dY[:, :w].contiguous())
            db2 = _bias_grad_to(K, b2, dY[:, w:].contiguous())
    return dW1, db1, dW2, db2


def _ln_param_grads(K, gamma, beta, ws, rows):
    """A LayerNorm's dgamma / dbeta = the column sums of the first ``rows`` per-workgroup partial rows
    [dgamma | dbeta] that hicgat_tail_bwd left in ``ws``: into the (adjacent) sinks as queued
    side work (ONE colsum launch over the live rows, its size as the lane-balancing work) or new
    tensors (returned)."""
    W = gamma.shape[0]
    part = ws.view(torch.float32)[:rows * 2 * W].view(rows, 2 * W)
    sg, sb = _sink(gamma), _sink(beta)
    if sg is not None and sb is not None and _adjacent(sg, sb):
        gj = _joined(sg, sb)
        param_launch(lambda: K.colsum(part, gj, accumulate=True), ws, work=rows * 2 * W, job=ColsumJob(part, gj))
        return None, None
    out = K.colsum(part, torch.empty(2 * W, dtype=torch.float32, device=part.device))
    return out[:W], out[W:]


class _DualLnActResFn(torch.autograd.Function):
    """norm2(act(norm(lin1(x))) + lin2(x)) -- the residual blocks of models.py:638-649 (relu, no norm2),
    :437-526, :528-612 and :693-773 -- as ONE GEMM Y = x [W1; W2]^T + [b1; b2] and one row pass over
    Y = [y | res] (ln_act.hip).  The backward's row pass writes dY = [dy | dres] packed, so dx is ONE GEMM
    (K = 2W) and, with the pairs adjacent in FlatAdam's buffer (``flat_parameters``), dW and db one GEMM."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2, gamma, beta, gamma2, beta2, eps, eps2, code, slope):
        K = kernels.default()
        x = x.contiguous()
        M = x.shape[0]
        w = W1.shape[0]
        n2 = gamma2 is not None
        Y = torch.empty((M, 2 * w), dtype=torch.float32, device=x.device)
        K.gemm(0, 0, M, 2 * w, x.shape[1], x, _joined(W1, W2).contiguous(), Y, bias=_joined(b1, b2).contiguous(),
               name="gemm_fwd")
        z = torch.empty((M, w), dtype=torch.float32, device=x.device)
        stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
        stats2 = torch.empty((M, 2), dtype=torch.float32, device=x.device) if n2 else None
        K.ln_act_res_fwd(Y[:, :w], gamma, beta, eps, code, slope, Y[:, w:], z, stats, gamma2, beta2, eps2, stats2)
        ctx.save_for_backward(x, Y, stats, stats2)
        ctx.cfg = (code, slope)
        ctx.params = (W1, b1, W2, b2, gamma, beta, gamma2, beta2)
        return z

    @staticmethod
    def backward(ctx, dz):
        return _dual_ln_act_res_backward(ctx.cfg, ctx.params, ctx.needs_input_grad[0], *ctx.saved_tensors, dz) \
            + (None,) * 4


def _dual_ln_act_res_backward(cfg, params, need_dx, x, Y, stats, stats2, dz):
    """``_DualLnActResFn``'s backward on its operands: (dx, dW1, db1, dW2, db2, dgamma, dbeta, dgamma2, dbeta2)."""
    K = kernels.default()
    W1, b1, W2, b2 = params[:4]
    dz = dz.contiguous()
    M, w = dz.shape
    dY = torch.empty((M, 2 * w), dtype=torch.float32, device=dz.device)
    dg, db, dg2, db2 = _ln_act_bwd(K, cfg, params[4:], dz, Y[:, :w], stats, Y[:, w:], stats2, dY[:, :w], dres=dY[:, w:])
    dx = None
    if need_dx:
        dx = K.gemm(0, 1, M, x.shape[1], 2 * w, dY, _joined(W1, W2).contiguous(), torch.empty_like(x), name="gemm_dx")
    return (dx,) + _dual_param_grads(K, W1, b1, W2, b2, dY, x) + (dg, db, dg2, db2)


def dual_ln_act_res(x, lin1, lin2, norm, act, norm2=None):
    """``norm2(act(norm(lin1(x))) + lin2(x))`` (``norm2`` optional) on the fused kernels: one GEMM over
    [W1; W2], one row pass.  ``act`` as ``ln_act_res``."""
    W = _ln_pair_check(norm, norm2)
    code, slope = _ln_act_code(act)
    for lin, what in ((lin1, "lin1"), (lin2, "lin2")):
        if not isinstance(lin, torch.nn.Linear) or lin.bias is None or lin.out_features != W:
            raise ValueError(f"{what} must be a torch.nn.Linear with a bias and {W} outputs (the norm's width)")
    if lin1.in_features != lin2.in_features:
        raise ValueError("lin1 and lin2 must read the same input width")
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[1] != lin1.in_features:
        raise ValueError(f"x must be a float32 [rows, {lin1.in_features}] tensor; got {x.dtype} {tuple(x.shape)}")
    _dev_check(x)
    g2, b2, e2 = (norm2.weight, norm2.bias, norm2.eps) if norm2 is not None else (None, None, 0.0)
    return _DualLnActResFn.apply(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, norm.weight, norm.bias, g2, b2,
                                 norm.eps, e2, code, slope)


# The flagship's MLP tail forward as ONE launch (tail_fused.hip) for row counts in [MIN_M, MAX_M]
# (HICGAT_FUSED_TAIL=0: off).  Measured (profiles/r03r_ab_fused_tail.txt, 4-deep weight prefetch):
# a rank's shard at P = 8 (2 700 rows) 0.613 vs 0.650 ms per rank step, P = 4 (5 000) 0.877 vs
# 0.896, synth-2000 0.641 vs 0.664 ms per step; with the fused backward too (r03za) the P = 2 shard
# (10 000 rows) 1.302 / 1.307 vs 1.313 / 1.315 ms.  On the whole 20000-row graph it was slower
# (1.936 vs 1.913 ms per step) while its 16-row workgroups read the weights row-major -- a quarter
# of the load rate -- and is faster since they read packed copies (TAIL_PACK): 1.815 / 1.819 vs
# 1.871 / 1.876 ms per step (profiles/r05aa_fused_tail_20000_ab.txt), so MAX_M now covers it.
# Graphs below MIN_M (chr19: 58 / 114 loci) keep the per-layer kernels.
FUSED_TAIL = os.environ.get("HICGAT_FUSED_TAIL", "1") != "0"
FUSED_TAIL_MIN_M = int(os.environ.get("HICGAT_FUSED_TAIL_MIN_M", "1024"))
FUSED_TAIL_MAX_M = int(os.environ.get("HICGAT_FUSED_TAIL_MAX_M", "32768"))
# ... and its backward input-gradient chain in one launch too (tail_fused.hip; 0: the per-layer
# functions' backward steps on the fused forward's tensors): P = 8 rank step 0.583 vs 0.622 ms, P = 4
# 0.856 vs 0.889, synth-2000 0.628 vs 0.652 ms per step (profiles/r03t_ab_fused_tail_bwd.txt)
FUSED_TAIL_BWD = os.environ.get("HICGAT_FUSED_TAIL_BWD", "1") != "0"
# ... both reading W1c / W2c / the heads' W as packed copies (hicgat_tail_pack, one launch per
# forward; 0: the row-major weights)
TAIL_PACK = os.environ.get("HICGAT_TAIL_PACK", "1") != "0"

# The flagship tail's 18 parameters as (name, attribute path on the model), in the order ``_FusedTailFn``
# takes them and returns their gradients
TAIL_PARAMS = (("Wa", "densea.weight"), ("ba", "densea.bias"), ("Wal", "align_densea.weight"),
               ("bal", "align_densea.bias"), ("ga", "norm_a.weight"), ("bea", "norm_a.bias"),
               ("W1", "dense1.weight"), ("b1", "dense1.bias"), ("W1al", "align_dense1.weight"),
               ("b1al", "align_dense1.bias"), ("g1", "norm1.weight"), ("be1", "norm1.bias"),
               ("W2", "dense2.weight"), ("b2", "dense2.bias"), ("g2", "norm2.weight"), ("be2", "norm2.bias"),
               ("W3", "dense3.weight"), ("b3", "dense3.bias"))
_TailParams = collections.namedtuple("_TailParams", [name for name, _ in TAIL_PARAMS])


def _tail_params(model):
    return _TailParams(*(operator.attrgetter(path)(model) for _, path in TAIL_PARAMS))


class _FusedTailFn(torch.autograd.Function):
    """models.py:638-659 after the relu (GATNetSelectiveResidualsUpdated.post_act): the forward in
    one kernel (hicgat_tail_fwd), which writes the tensors the per-layer autograd functions
    would save; the backward runs those functions' own backward steps on them, in autograd's order
    (dense3, norm2, dense2, block 2, block 1), so its kernels, side-stream parameter gradients and
    sums are the per-layer path's."""

    @staticmethod
    def forward(ctx, x, *args):
        p, (eps, coords_out, heads, prepack) = _TailParams(*args[:len(TAIL_PARAMS)]), args[len(TAIL_PARAMS):]
        K = kernels.default()
        x = x.contiguous()
        # the kernels' operands, built once: the backward reads them from ctx
        w = kernels.TailWeights(
            W1c=_joined(p.Wa, p.Wal).contiguous(), b1c=_joined(p.ba, p.bal).contiguous(), g1=p.ga.contiguous(),
            be1=p.bea.contiguous(), W2c=_joined(p.W1, p.W1al).contiguous(), b2c=_joined(p.b1, p.b1al).contiguous(),
            g2=p.g1.contiguous(), be2=p.be1.contiguous(), W3=p.W2.contiguous(), b3=p.b2.contiguous(),
            g3=p.g2.contiguous(), be3=p.be2.contiguous(), W4=p.W3.contiguous(), b4=p.b3.contiguous())
        # heads: x's rows are formed (written) by the kernel from the xagg GATConv's aggregates
        # the weights as packed copies for both kernels (made once per forward -- or by the training
        # step's first launch, ``prepack``: step_pack -- the backward reuses them)
        if prepack is not None:
            pack = prepack          # (heads: a pack with the heads' W, else the launch is refused)
        else:
            pack = K.tail_pack(w.W1c, w.W2c, heads.W if heads is not None else None) if TAIL_PACK else None
        coords, saved = K.tail_fwd_fused(x, w, eps, coords=coords_out, heads=heads, pack=pack)
        ctx.heads = heads
        ctx.pack = pack
        ctx.weights = w
        link = getattr(x, "_hicgat_rows", None) if heads is None else None
        # the GATConv's rows pass in this backward's epilogue: its relu output is exactly our input rows
        ctx.rows = link if (link is not None and FUSE_ROWS and K.tail_waves() == 16 and x.shape[1] == 512) else None
        if coords_out is not None:
            # the kernel wrote into the caller's buffer (e.g. the all-gather rows); the output is a
            # fresh tensor object over the same memory, so autograd sees a new output (no view or
            # in-place bookkeeping on the caller's buffer, which a collective then fills around it)
            coords = torch.empty(0, dtype=coords_out.dtype, device=coords_out.device).set_(
                coords_out.untyped_storage(), coords_out.storage_offset(), coords_out.shape, coords_out.stride())
        ctx.save_for_backward(x, *saved)
        ctx.params = p
        return coords

    @staticmethod
    def backward(ctx, dcoords):
        x, Y1, st1, z1, Y2, st2, z2, y3, st3, z3 = ctx.saved_tensors
        p = ctx.params
        if FUSED_TAIL_BWD:
            # the input-gradient chain in one launch; the parameter gradients from its dY tensors
            # and LN partials, issued in the per-layer path's order (dense3, norm2, dense2, block 2,
            # block 1)
            K = kernels.default()
            dc = dcoords.contiguous()
            rows = None
            if ctx.rows is not None and ctx.needs_input_grad[0]:
                act, out2, rs, b, state = ctx.rows
                dout = torch.empty((dc.shape[0], 512), dtype=torch.float32, device=dc.device)
                rows = (act, x, out2, b, rs, dout)
            dx, dY1, dY2, dy3, (ws1, ws2, ws3) = K.tail_bwd_fused(dc, ctx.saved_tensors[1:], ctx.weights,
                                                                  heads=ctx.heads, pack=ctx.pack, rows=rows)
            if rows is not None:
                dx = dout               # the GATConv's backward finds it in the shared state and skips its rows pass
                state["dout"] = dout
            rows = K.tail_partial_rows(dc.shape[0])   # the kernel's partial rows: one per workgroup
            dW3, db3 = _wb_grad_to(K, p.W3, p.b3, dc, z3)
            dg2, dbe2 = _ln_param_grads(K, p.g2, p.be2, ws3, rows)
            dW2, db2 = _wb_grad_to(K, p.W2, p.b2, dy3, z2)
            dg1, dbe1 = _ln_param_grads(K, p.g1, p.be1, ws2, rows)
            dW1, db1, dW1al, db1al = _dual_param_grads(K, p.W1, p.b1, p.W1al, p.b1al, dY2, z1)
            dga, dbea = _ln_param_grads(K, p.ga, p.bea, ws1, rows)
            dWa, dba, dWal, dbal = _dual_param_grads(K, p.Wa, p.ba, p.Wal, p.bal, dY1, x)
            return (dx if ctx.needs_input_grad[0] else None, dWa, dba, dWal, dbal, dga, dbea, dW1, db1, dW1al, db1al,
                    dg1, dbe1, dW2, db2, dg2, dbe2, dW3, db3, None, None, None, None)
        relu = (kernels.HipKernels.ACT_RELU, 0.0)
        dz3, dW3, db3 = _linear_backward(p.W3, p.b3, z3, dcoords)
        dy3, _, dg2, dbe2, _, _ = _ln_act_res_backward(relu, (p.g2, p.be2, None, None), False, y3, st3, None, None, dz3)
        dz2, dW2, db2 = _linear_backward(p.W2, p.b2, z2, dy3)
        dz1, dW1, db1, dW1al, db1al, dg1, dbe1, _, _ = _dual_ln_act_res_backward(
            relu, (p.W1, p.b1, p.W1al, p.b1al, p.g1, p.be1, None, None), True, z1, Y2, st2, None, dz2)
        dx, dWa, dba, dWal, dbal, dga, dbea, _, _ = _dual_ln_act_res_backward(
            relu, (p.Wa, p.ba, p.Wal, p.bal, p.ga, p.bea, None, None), ctx.needs_input_grad[0], x, Y1, st1, None, dz1)
        return (dx, dWa, dba, dWal, dbal, dga, dbea, dW1, db1, dW1al, db1al, dg1, dbe1, dW2, db2, dg2, dbe2,
                dW3, db3, None, None, None, None)


def fused_tail_ok(model, x):
    return (FUSED_TAIL and getattr(model, "fused_tail", True)
            and x.is_cuda and x.dim() == 2 and FUSED_TAIL_MIN_M <= x.shape[0] <= FUSED_TAIL_MAX_M
            and x.shape[1] == 512
            and x.dtype == torch.float32 and x.stride(1) == 1
            and model.norm_a.eps == model.norm1.eps == model.norm2.eps)


class TailHeads:
    """The xagg GATConv's operands of the head-fused tail kernels (hicgat_tail_{fwd,bwd}, HICGAT_TAIL_HEADS):
    X4 [2, 2, M, 512] (xa^h = X4[h, 0]), lin_l's weight W [512, 512] and bias [512], and the buffers
    they write: Y0 [M, 512] (the forward; the tail's input rows relu(Y0) go into ``fused_tail``'s x),
    dout [M, 512], the own rows' row stats rs [M, 8] and dxa [M, 1024] (the backward)."""

    def __init__(self, X4, W, bias, Y0, dout, rs, dxa, act=1):
        self.X4, self.W, self.bias, self.Y0, self.dout, self.rs, self.dxa, self.act = X4, W, bias, Y0, dout, rs, dxa, act


# HICGAT_TAIL_HEADS=0: the xagg step keeps its per-head GEMM launches, rows pass and dxa GEMMs
TAIL_HEADS = os.environ.get("HICGAT_TAIL_HEADS", "1") != "0"


def tail_heads_ok(model, x):
    return TAIL_HEADS and FUSED_TAIL_BWD and fused_tail_ok(model, x) and kernels.default().tail_waves() >= 8


def fused_tail(model, x, coords_out=None, heads=None):
    """GATNetSelectiveResidualsUpdated.post_act on the fused forward (``fused_tail_ok`` first);
    ``coords_out``: a contiguous [M, 3] buffer the coordinates are written into (and returned);
    ``heads`` (``TailHeads``, ``tail_heads_ok`` first): x's rows are formed from the xagg GATConv's
    aggregates in the same launch (x is written), and the backward writes the GATConv's dout /
    delta / dxa instead of x's gradient."""
    return _FusedTailFn.apply(x, *_tail_params(model), model.norm_a.eps, coords_out, heads,
                              getattr(model, "_hicgat_prepack", None))


def step_pack(model, x):
    """The tail's packed weights as part of a training step's first launch: (W1c, W2c, None, buffer)
    for ``FlatAdam.zero_grad(pack=...)`` when the step's forward will run the one-kernel tail on x's
    N rows with packed weights (the flagship, ``fused_tail_ok``'s row range, the residual pairs
    adjacent in FlatAdam's buffer so [W; W_align] are views), else None.  The forward inside
    ``prepacked(model, job)`` then reads the buffer instead of packing again: one launch fewer per
    step (the weights change only at the previous step's Adam).  The sharded xagg step passes its
    own rows and hands the job to ``kernels.xagg_logits(pack=...)``, which adds lin_l's W (the
    head-fused tail's third weight)."""
    m = model
    if not (STEP_PACK and TAIL_PACK and FUSED_TAIL and x.is_cuda and hasattr(m, "align_densea") and hasattr(m, "norm_a")
            and getattr(m, "fused_tail", True)      # gat_models._LayerNormTail has these names and another tail
            and FUSED_TAIL_MIN_M <= x.shape[0] <= FUSED_TAIL_MAX_M
            and m.norm_a.eps == m.norm1.eps == m.norm2.eps):
        return None
    p = _tail_params(m)
    if not (_adjacent(p.Wa, p.Wal) and _adjacent(p.W1, p.W1al)):
        return None
    W1c, W2c = _joined(p.Wa, p.Wal), _joined(p.W1, p.W1al)
    buf = getattr(m, "_hicgat_pack_buf", None)
    if buf is None or buf.device != x.device:
        n = int(kernels.default().lib.hicgat_tail_pack_bytes())
        buf = m._hicgat_pack_buf = torch.empty(n // 4, dtype=torch.float32, device=x.device)
    return (W1c.detach(), W2c.detach(), None, buf)


@contextlib.contextmanager
def prepacked(model, job):
    """The forward inside reads the pack ``job`` (``step_pack``) wrote, if any."""
    if job is None:
        yield
        return
    model._hicgat_prepack = job[3]
    try:
        yield
    finally:
        model._hicgat_prepack = None


GAT_SHAPE_RULE = "out_channels % 128 == 0, heads * out_channels a multiple of 256 and <= 1024, heads <= 4"


ATTN_SITE_LIMIT = 1 << 31   # include/hicgat.h HICGAT_ATTN_SITE_BIT: attention-dropout sites lie below it


def gat_shape_supported(H, C):
    """Whether the aggregation kernels run GATConv(heads=H, out_channels=C) (include/hicgat.h; the
    rule of gat_launch.hpp, usable without the library loaded)."""
    H, C = int(H), int(C)
    return 1 <= H <= 4 and C > 0 and C % 128 == 0 and (H * C) % 256 == 0 and H * C <= 1024


def _attn_site(site):
    site = int(site)
    if not 0 <= site < ATTN_SITE_LIMIT:
        raise ValueError(f"an attention-dropout site must satisfy 0 <= site < 2**31, got {site}")
    return site


def gat_conv(x, W, att_l, att_r, bias, adj, negative_slope=0.2, act=None, return_attention_weights=False,
             dropout=0.0, training=False, state=None, site=0):
    """GATConv forward; ``act="relu"`` returns relu(GATConv(x)) with the relu fused.
    ``return_attention_weights=True`` returns ``(out, alpha)``: alpha [nnz, H] in the order of the
    self-looped device CSR (``adj.rowptr32`` / ``adj.col32``), attached to autograd.
    ``dropout`` = p with ``training``: attention dropout, every alpha_ij times its keep factor in
    {0, 1 / (1 - p)} per head, with the mask of (state.seed, the state's device step count, site, i, j,
    head) (``state``: a ``dropout.DropoutState`` the caller has advanced; ``attention_dropout_mask``);
    it follows ``training``, not the grad mode, and alpha is returned as it was before the dropout.
    Without ``training`` or with p = 0 the call is the plain one."""
    from .dropout import check_p
    p = check_p(dropout)
    H, C = att_l.shape[-2], att_l.shape[-1]
    if not gat_shape_supported(H, C):
        raise NotImplementedError(f"GATConv(heads={H}, out_channels={C}) is not supported by the aggregation "
                                  f"kernels: they need {GAT_SHAPE_RULE}")
    if adj.rowptr32 is None or adj.rowptr32.device != x.device:
        adj.to(x.device)
    # the matrix-core tiled form (gat_tiles.hip) is (2, 256) only: every other shape gathers
    if training and p > 0.0:
        if state is None:
            raise ValueError("gat_conv(dropout > 0, training=True) needs a DropoutState")
        site = _attn_site(site)
        _dev_check(x, W, att_l, att_r, bias)
        tmap = adj.transpose_map() if return_attention_weights else None
        return _GATConvDropFn.apply(x, W, att_l, att_r, bias, adj.rowptr32, adj.col32, negative_slope, _ACTS[act],
                                    tmap, p, state, site)
    tiles = adj.tiles() if (H, C) == (2, 256) else None
    if return_attention_weights:
        return _GATConvAttnFn.apply(x, W, att_l, att_r, bias, adj.rowptr32, adj.col32, negative_slope, _ACTS[act],
                                    tiles, adj.transpose_map())
    return _GATConvFn.apply(x, W, att_l, att_r, bias, adj.rowptr32, adj.col32, negative_slope, _ACTS[act], tiles)


class _PairDistFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords):
        _lib.lib()
        _dev_check(coords)
        c = coords.contiguous().float()
        ctx.save_for_backward(c)
        return kernels.default().pairdist_fwd(c)

    @staticmethod
    def backward(ctx, dD):
        (c,) = ctx.saved_tensors
        return kernels.default().pairdist_bwd(c, dD.contiguous().float())


def pairwise_dist(coords):
    """torch.cdist(coords, coords, p=2) on the GPU (models.py:661)."""
    return _PairDistFn.apply(coords)


class _FusedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, tbuf, n, loss_kind, tile_begin, tile_end, stats, support=None):
        c = coords.contiguous().float()
        dc = torch.empty_like(c)
        loss = torch.empty((), dtype=torch.float32, device=c.device)
        if support is not None:
            kernels.default().fused_loss_support(c, support, n, loss_kind, stats, loss, dc)
        else:
            kernels.default().fused_loss(c, tbuf, n, loss_kind, tile_begin, tile_end, stats, loss, dc)
        ctx.save_for_backward(dc)
        return loss

    @staticmethod
    def backward(ctx, gl):
        (dc,) = ctx.saved_tensors
        # seeded by backward_from_loss with its resident ones tensor, never written since (the
        # version counter catches an in-place change by a hook): d(loss) = 1 exactly
        if gl is _UNIT_SEEDS.get(gl.device) and gl._version == 0:
            return dc, None, None, None, None, None, None, None
        return dc * gl, None, None, None, None, None, None, None


# loss.backward() fills a fresh ones tensor and the loss node then multiplies dcoords by it: two
# launches per step.  backward_from_loss seeds with one resident ones tensor per device instead, which
# the loss node recognises by identity AND an unchanged version counter (any in-place write to it --
# e.g. by a gradient hook -- bumps ``_version``, and the node then multiplies as usual) and skips
# the multiply -- the same bits.
_UNIT_SEEDS = {}


def backward_from_loss(loss):
    """``loss.backward()`` for a scalar loss from ``fused_dist_loss``, without the seed fill and the
    dcoords scaling launches."""
    seed = _UNIT_SEEDS.get(loss.device)
    if seed is None or seed.dtype != loss.dtype or seed._version != 0:
        seed = _UNIT_SEEDS[loss.device] = torch.ones((), dtype=loss.dtype, device=loss.device)
    torch.autograd.backward(loss, grad_tensors=seed)


class _MomentLossFn(torch.autograd.Function):
    """The moment-dependent losses: value and d(loss)/d(coords) from one chain of launches."""

    @staticmethod
    def forward(ctx, coords, tbuf, n, mkind, alpha, stats, support=None):
        c = coords.contiguous().float()
        dc = torch.empty_like(c)
        loss = torch.empty((), dtype=torch.float32, device=c.device)
        if support is not None:
            kernels.default().moment_loss_support(c, support, n, mkind, alpha, stats, loss, dc)
        else:
            kernels.default().moment_loss(c, tbuf, n, mkind, alpha, stats, loss, dc)
        ctx.save_for_backward(dc)
        return loss

    @staticmethod
    def backward(ctx, gl):
        (dc,) = ctx.saved_tensors
        if gl is _UNIT_SEEDS.get(gl.device) and gl._version == 0:   # as _FusedLossFn
            return dc, None, None, None, None, None, None
        return dc * gl, None, None, None, None, None, None


LOSS_KINDS = {"mse": 0, "combined": 1, "contrastive": 2}   # include/hicgat.h loss_kind
MOMENT_LOSS_KINDS = {"mse+pearson": 0, "rmse": 1, "si_mse": 2}   # include/hicgat.h mloss_kind


def fused_dist_loss(coords, truth, kind="mse", tile_range=(0, -1), stats=None, alpha=1.0):
    """MSE(cdist(coords), truth) [kind="mse", HiC-GNN_main.py:127],
    MSE + alpha*(1 - pearson) [kind="combined", HiC_GAT_generalize_directly.py:219-225] with the
    gradient of the MSE only (the Pearson term is a detached host value in the reference), or
    0.1 * mean_{i<j} |T_ij - D_ij| [kind="contrastive", train_and_test_same_res_GAT_node2vec.py:107-134:
    differentiable; its fp64 value in stats[10], the returned scalar is its fp32 rounding].

    ``truth`` is a ``graph.Truth`` (stored symmetric; an asymmetric target is folded into the
    equivalent symmetric form there); with a background + support form (``truth.support``, e.g.
    cont2dist's target) the whole-matrix loss reads no truth in its O(N^2) pass.  ``stats`` (float64 [12], device) receives the moments, mse,
    r, alpha and total (see include/hicgat.h).

    The kinds of ``MOMENT_LOSS_KINDS`` are differentiable through the global moments of D and T:
    ``"mse+pearson"`` = mse + ``alpha`` * (1 - r) with the gradient through both terms (``alpha`` a
    fixed weight, not the reference's dynamic one), ``"rmse"`` = sqrt(mse + 1e-12) and ``"si_mse"`` =
    mean((e - mean e)^2), e = D - T over all N^2 entries (HiC_GAT_generalize_directly.py:60-68).  Still
    one O(N^2) pass; whole matrix only (no ``tile_range``), and a symmetric truth only."""
    if kind in MOMENT_LOSS_KINDS and truth.asymmetric_source:
        # the symmetric fold keeps the MSE and its gradient only, not the t-moments of these losses
        raise ValueError(f"loss {kind!r} needs a symmetric truth; this one was folded from an asymmetric target")
    _lib.lib()
    _dev_check(coords)
    if stats is None:
        stats = torch.empty(12, dtype=torch.float64, device=coords.device)
    if kind in MOMENT_LOSS_KINDS:
        if (int(tile_range[0]), int(tile_range[1])) not in ((0, -1), (0, kernels.default().num_tiles(truth.n))):
            raise ValueError(f"loss {kind!r} runs over the whole matrix only (tile_range {tuple(tile_range)})")
        loss = _MomentLossFn.apply(coords, truth.buf, truth.n, MOMENT_LOSS_KINDS[kind], float(alpha), stats,
                                   getattr(truth, "support", None))
        return loss, stats
    kind_i = LOSS_KINDS[kind]
    if kind == "contrastive":
        truth = truth.upper()       # the contrastive loss reads truth[triu] as given
    t0, t1 = int(tile_range[0]), int(tile_range[1])
    # the background + support form (no truth stream) when the truth has one and all tiles are wanted
    whole = t0 == 0 and t1 in (-1, kernels.default().num_tiles(truth.n))
    support = getattr(truth, "support", None) if whole else None
    loss = _FusedLossFn.apply(coords, truth.buf, truth.n, kind_i, t0, t1, stats, support)
    return loss, stats


class _SageConvFn(torch.autograd.Function):
    """SAGEConv.forward (layers.py:55-77) on the HIP path: one wave-per-row pass writes
    z = [N_adj x | trunc(x)] and lin_l + lin_r run as ONE GEMM over [W_l | W_r] (K = 2F).  The
    x.long() branch carries no gradient (as in the reference); d x = N_adj^T (d out W_l)."""

    @staticmethod
    def forward(ctx, x, W_l, b_l, W_r, rowptr, col, w, inv_deg):
        K = kernels.default()
        x = x.contiguous().float()
        N, F = x.shape
        root = W_r is not None
        z = torch.empty((N, 2 * F if root else F), dtype=torch.float32, device=x.device)
        K.sage_agg(rowptr, col, w, inv_deg, 0, N, x, z, transpose=False, write_trunc=root)
        Wc = torch.cat([W_l, W_r], dim=1).contiguous() if root else W_l.contiguous()
        out = torch.empty((N, W_l.shape[0]), dtype=torch.float32, device=x.device)
        K.gemm(0, 0, N, W_l.shape[0], z.shape[1], z, Wc, out, bias=b_l, name="gemm_fwd")
        ctx.save_for_backward(z, W_l, rowptr, col, w, inv_deg)
        ctx.dims = (N, F, root, b_l is not None)
        ctx.params = (W_l, b_l, W_r)
        return out

    @staticmethod
    def backward(ctx, dout):
        K = kernels.default()
        z, W_l, rowptr, col, w, inv_deg = ctx.saved_tensors
        N, F, root, has_b = ctx.dims
        dout = dout.contiguous()
        dx = dWl = db = dWr = None
        pWl, pbl, pWr = ctx.params
        dWl, db = _wb_grad_to(K, pWl, pbl, dout, z[:, :F], need_w=ctx.needs_input_grad[1],
                              need_b=has_b and ctx.needs_input_grad[2])
        if root and ctx.needs_input_grad[3]:
            dWr = _weight_grad_to(K, pWr, dout, z[:, F:])
        if ctx.needs_input_grad[0]:
            dagg = K.gemm(0, 1, N, F, dout.shape[1], dout, W_l.contiguous(),
                          torch.empty((N, F), dtype=torch.float32, device=dout.device), name="gemm_dx")
            dx = K.sage_agg(rowptr, col, w, inv_deg, 0, N, dagg, torch.empty_like(dagg), transpose=True)
        return dx, dWl, db, dWr, None, None, None, None


def sage_conv(x, W_l, b_l, W_r, adj):
    """SAGEConv (layers.py:12-79) over a ``hicgat.Adj`` that carries ``value32``/``inv_deg``."""
    _dev_check(x, W_l, b_l, W_r)
    if adj.value32 is None or adj.inv_deg is None:
        raise ValueError("SAGEConv needs the edge weights: build the Adj with values (load_input / "
                         "Adj.from_dense_device / Adj(row, col, value).to(device))")
    return _SageConvFn.apply(x, W_l, b_l, W_r, adj.rowptr32, adj.col32, adj.value32, adj.inv_deg)

"""The bits of the GATConv aggregation passes at every supported (H, C), against a recording.

``tests/golden/gat_agg_bits.json`` (written by ``tests/golden/make_gat_agg_bits.py``; its "about" entry
says at which commit, with which compiler and on which device) holds the SHA-256 of every output of the
four passes -- forward, rows, stand-alone destination, source -- and of the DROP forms of the forward
and the source pass, called through ``hicgat.kernels``.  A change of the launch layer (entry kernels,
dispatch, validation) must leave every one of them as it is; a change of a row body that moves a bit
has to say so and record again.

Inputs come from ``numpy.random.default_rng`` on the host and their SHA-256 is recorded too, so a
different draw reads differently from a different kernel.  Every output buffer is NaN-filled before
the call that writes it: a row that a launch skips shows in the hash.

The graph (n = 131 rows, no multiple of the 4 rows per workgroup, symmetric, self loops
in the list as ``Adj`` keeps them): a band of width 6; row 5 isolated (its self loop only); row 0 a
hub.  A hub joined to all 131 rows and an isolated row exclude each other in a symmetric graph, so the
hub leaves out rows 5 and 130: 129 = 2 * 64 + 1 entries, two full 64-edge chunks and a tail that is no
multiple of any gather unroll.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 131
NS = 0.2
DROP = (0.3, 0x5EED1234ABCD, None, 7, 0)     # (p, seed, step counter, step_value, site)
SHAPES = [(1, 256), (1, 512), (1, 768), (1, 1024), (2, 128), (2, 256), (2, 384), (2, 512), (3, 256), (4, 128),
          (4, 256)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gat_agg_bits.json")


def sha(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().contiguous().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def graph():
    """(rowptr, col) int32 on the host, columns sorted within a row."""
    i, j = np.indices((N, N))
    a = np.abs(i - j) <= 6
    a[0, :] = a[:, 0] = True
    a[0, N - 1] = a[N - 1, 0] = False
    a[5, :] = a[:, 5] = False
    a[np.arange(N), np.arange(N)] = True
    assert (a == a.T).all() and a[5].sum() == 1 and a[0].sum() == 2 * 64 + 1
    rowptr = np.concatenate([[0], np.cumsum(a.sum(1))]).astype(np.int32)
    col = np.nonzero(a)[1].astype(np.int32)
    return rowptr, col


def inputs(H, C):
    """Host float32 arrays of one shape, by name."""
    rng = np.random.default_rng(1000 * H + C)
    D = H * C
    f = lambda *s, scale=1.0: (scale * rng.standard_normal(s)).astype(np.float32)   # noqa: E731
    return {"h": f(N, D, scale=0.5), "a_src": f(N, H), "a_dst": f(N, H), "bias": f(D, scale=0.1), "g": f(N, D),
            "att_l": f(H, C, scale=0.1), "att_r": f(H, C, scale=0.1)}


def inputs_sha(H, C):
    rowptr, col = graph()
    return {"rowptr": sha(rowptr), "col": sha(col), **{k: sha(v) for k, v in inputs(H, C).items()}}


def outputs(H, C):
    """Run every pass once; {name: tensor} of everything a pass wrote."""
    from hicgat import kernels
    K = kernels.HipKernels()
    rowptr, col = (torch.tensor(a, device=DEV) for a in graph())
    x = {k: torch.tensor(v, device=DEV) for k, v in inputs(H, C).items()}
    h, a_s, a_d, bias, g, att_l, att_r = (x[k] for k in ("h", "a_src", "a_dst", "bias", "g", "att_l", "att_r"))
    D = H * C
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)   # noqa: E731
    got = {}

    def forward(tag, call):
        """TRAIN x ACT of one forward; returns what the TRAIN, relu call left (the backward's input)."""
        for train in (0, 1):
            for act in (0, 1):
                out, out2, rs = nan(N, D), nan(N, D) if train else None, nan(N, 4 * H)
                call(act, out, out2, rs)
                got[f"{tag}-train{train}-act{act}-out"] = out
                got[f"{tag}-train{train}-act{act}-row_stats"] = rs
                if train:
                    got[f"{tag}-train{train}-act{act}-out2"] = out2
        return out, out2, rs

    def rows(tag, act, y, out2, rs_fwd):
        rs, dout = rs_fwd.clone(), nan(N, D) if act else None
        K.agg_bwd_rows(0, N, act, g, y, bias, out2, dout, rs)
        got[f"{tag}-act{act}-row_stats"] = rs
        if act:
            got[f"{tag}-act{act}-dout"] = dout
        return (dout if act else g), rs

    def source(tag, call, dout, rs):
        for rr in (False, True):
            dh, da = nan(N, D), nan(N, H)
            call(rs, dout, dh, da, rr)
            got[f"{tag}-{'roundrobin' if rr else 'remap'}-dh"] = dh
            got[f"{tag}-{'roundrobin' if rr else 'remap'}-da_src"] = da

    y, out2, rs_f = forward("fwd", lambda act, out, o2, rs: K.agg_fwd_act(rowptr, col, 0, N, h, a_s, a_d, bias, NS, act,
                                                                          out, o2, rs))
    rows("rows", 0, got["fwd-train1-act0-out"], got["fwd-train1-act0-out2"], got["fwd-train1-act0-row_stats"])
    dout, rs = rows("rows", 1, y, out2, rs_f)
    rs_d = got["fwd-train0-act0-row_stats"].clone()     # the stand-alone form: max and sum only
    K.agg_bwd_dst(rowptr, col, 0, N, h, a_s, a_d, g, NS, rs_d)
    got["dst-row_stats"] = rs_d
    source("src", lambda rs, dout, dh, da, rr: K.agg_bwd_src(rowptr, col, 0, N, h, a_s, a_d, rs, dout, att_l, att_r, NS,
                                                             dh, da, round_robin=rr), dout, rs)

    y, out2, rs_f = forward("drop_fwd", lambda act, out, o2, rs: K.agg_fwd_act(rowptr, col, 0, N, h, a_s, a_d, bias,
                                                                              NS, act, out, o2, rs, drop=DROP))
    dout, rs = rows("drop_rows", 1, y, out2, rs_f)
    source("drop_src", lambda rs, dout, dh, da, rr: K.agg_bwd_src(rowptr, col, 0, N, h, a_s, a_d, rs, dout, att_l,
                                                                  att_r, NS, dh, da, round_robin=rr, drop=DROP),
           dout, rs)
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def recorded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("H,C", SHAPES, ids=[f"h{h}c{c}" for h, c in SHAPES])
def test_gat_agg_passes_keep_their_recorded_bits(recorded, H, C):
    """Forward TRAIN x ACT (out, out2, row_stats), rows at act 0 / 1, the stand-alone destination pass,
    the source pass in both block orders (dh, da_src), and the DROP forward and source pass (p = 0.3,
    step by value, site 0), and the rows pass between those two: 34 hashes per shape."""
    case = recorded["cases"][f"h{H}c{C}"]
    assert inputs_sha(H, C) == case["inputs_sha256"], "inputs differ from the recorded draw: not a kernel failure"
    got = {k: sha(v) for k, v in outputs(H, C).items()}
    assert sorted(got) == sorted(case["sha256"])
    assert len(got) == 34
    wrong = [k for k in sorted(got) if got[k] != case["sha256"][k]]
    assert not wrong, wrong

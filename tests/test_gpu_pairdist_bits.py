"""The bits of every entry point of csrc/pairdist.hip, against a recording.

``tests/golden/pairdist_bits.json`` (written by ``tests/golden/make_pairdist_bits.py``; its "about"
entry says at which commit, with which compiler and on which device) holds the SHA-256 of every output
(``stats`` through slot 11, ``loss``, ``dcoords`` / ``dcoords64``) of the fixed-weight chain
(``fused_loss``, ``fused_loss_support_range``), the moment-dependent chain (``moment_loss``,
``moment_loss_support``), ``loss_finalize`` and ``pairdist_bwd``, called through ``hicgat.kernels``.
Every sum of these chains has a fixed order, so a change that only moves code between functions must
leave every hash as it is; a change of the arithmetic has to say so and record again.

Inputs come from ``numpy.random.default_rng`` on the host and their SHA-256 is recorded too, so a
different draw reads differently from a different kernel.  Every output buffer is NaN-filled before
the call that writes it: a slot or row that a launch skips shows in the hash.

Sizes: n = 2 and 127 (one masked tile), 128 (one full diagonal tile), 129 (edge tiles of one row or
column), 300 (3 x 3 blocks: one interior tile beside ragged ones), 384 (every block full) and, for one
dense MSE, one background combined and one moment loss case, 2100 (17 column tiles: the second trip of
the reduce's J-group loop).  Coordinates are normal draws (no two points coincide; coincident and
collapsed points are tests/test_gpu_pairdist_edges.py's).  The sparse support is a symmetric band plus
row 0 as a hub (more than 256 entries from n = 300 on: the second round of the support loop's 4 x 64)
and row 5 empty (n > 8).

Not reached: the kMomBlocks moment path together with ``dcoords64`` needs a share of more than 4096
moment records (n > 11000), too large for this module; with a float64 ``dcoords`` every case here takes
the one-block path, and the fp32 whole-range cases cover ``moments_finalize_kernel``.

The recording also holds what the workspace size queries returned (``workspace_bytes``); that test is
host code and runs without a GPU.
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

DEV = "cuda"
BT = 128
BG = 1.0
ALPHA = 0.7
SMALL = (2, 127, 128, 129, 300, 384)
BIG = 2100
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairdist_bits.json")
WS_SIZES = (0, 1, 127, 128, 129, 300, 20000)
CASES = ([("dense", n) for n in SMALL + (BIG,)] + [("support", n) for n in SMALL + (BIG,)] +
         [("moment", n) for n in SMALL + (BIG,)] + [("moment_support", n) for n in SMALL] +
         [("bwd", 129), ("bwd", 300), ("finalize", 300)])


def sha(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().contiguous().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def padded_ld(n):
    return (n + BT - 1) // BT * BT


def _sym(rng, n, lo, hi):
    """An exactly symmetric float32 [n, n] with entries in (lo, hi)."""
    a = np.triu((lo + (hi - lo) * rng.random((n, n))).astype(np.float32), 1)
    return a + a.T + np.diag((lo + (hi - lo) * rng.random(n)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def inputs(n):
    """Host arrays of one size, by name: coordinates, dense truth, upstream gradient, the support form
    (rowptr, col, val, diag) of a truth that is BG elsewhere, a row permutation, and the fixed vectors
    of the finalize cases."""
    rng = np.random.default_rng(7000 + n)
    x = {"coords": (0.5 * rng.standard_normal((n, 3))).astype(np.float32), "truth": _sym(rng, n, 0.1, 2.0),
         "g": rng.standard_normal((n, n)).astype(np.float32)}
    i, j = np.indices((n, n))
    m = (np.abs(i - j) <= 2) & (i != j)
    m[0, 1:] = m[1:, 0] = True                      # the hub
    if n > 8:
        m[5, :] = m[:, 5] = False                   # the empty row
    v = _sym(rng, n, 0.05, 0.95)
    assert (m == m.T).all() and not (v[m] == BG).any()
    assert n < 300 or (m[0].sum() > 256 and m[5].sum() == 0)
    x["rowptr"] = np.concatenate([[0], np.cumsum(m.sum(1))]).astype(np.int32)
    x["col"] = np.nonzero(m)[1].astype(np.int32)
    x["val"] = v[m].astype(np.float32)
    x["diag"] = np.ascontiguousarray(np.diagonal(v)).astype(np.float32)
    x["cmap"] = rng.permutation(n).astype(np.int32)
    # moments of plausible size for the finalize forms: L, sd, sdd, sdt, st, stt, dg, then five slots to overwrite
    pairs = 0.5 * n * (n - 1)
    x["stats"] = np.concatenate([pairs * np.array([0.31, 1.2, 1.9, 1.4, 1.1, 1.5]) * (1 + 0.01 * rng.random(6)),
                                 [0.4 * n], np.full(5, np.nan)])
    x["dc64"] = rng.standard_normal((n, 3))
    x["cbuf"] = rng.standard_normal((n + 7, 3)).astype(np.float32)
    x["gidx"] = rng.permutation(n + 7)[:n].astype(np.int32)
    return x


@functools.lru_cache(maxsize=None)
def inputs_sha(n):
    return {k: sha(v) for k, v in inputs(n).items()}


def _dev(a):
    return torch.tensor(a, device=DEV)


def _padded(a, ld, fill=0.0):
    """[rows, ld] fp32 on the device holding ``a`` in its first columns (a fresh, 16-byte aligned buffer)."""
    buf = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=DEV)
    buf[:, :a.shape[1]] = _dev(a)
    assert buf.data_ptr() % 16 == 0
    return buf


def _outs(n, d64=False, dc=True):
    stats = torch.full((12,), float("nan"), dtype=torch.float64, device=DEV)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    dcoords = torch.full((n, 3), float("nan"), dtype=torch.float64 if d64 else torch.float32, device=DEV) if dc else None
    return stats, loss, dcoords


def _keep(got, tag, stats, loss, dcoords):
    got[f"{tag}-stats"], got[f"{tag}-loss"] = stats, loss
    if dcoords is not None:
        got[f"{tag}-dcoords"] = dcoords


def _support(x):
    from hicgat import graph
    return graph.SupportForm(BG, _dev(x["rowptr"]), _dev(x["col"]), _dev(x["val"]), _dev(x["diag"]), len(x["col"]))


def _dense(K, n, x, got):
    c, t = _dev(x["coords"]), x["truth"]
    forms = {"vec": _padded(t, padded_ld(n)), "glob": _padded(t, n | 1)}     # glob: an odd leading dimension
    kinds = (0, 1, 2) if n != BIG else (0,)
    for form, tbuf in forms.items():
        if n == BIG and form != "vec":
            continue
        for kind in kinds:
            o = _outs(n)
            K.fused_loss(c, tbuf, n, kind, 0, -1, *o)
            _keep(got, f"{form}-k{kind}-full", *o)
    if n != 300:
        return
    o = _outs(n, dc=False)
    K.fused_loss(c, forms["vec"], n, 1, 0, -1, *o)
    _keep(got, "vec-k1-full-nodc", *o)
    # tile ranges: (0, 3) = tile-row 0 of the whole truth; (3, 6) = tile-rows 1 and 2 from the band at (128, 128)
    bands = {"vec": forms["vec"][128:, 128:].contiguous(), "glob": _padded(t[128:, 128:], (n - 128) | 1)}
    assert bands["vec"].data_ptr() % 16 == 0 and bands["vec"].shape[1] == 256
    for form in forms:
        for kind in kinds:
            o = _outs(n)
            K.fused_loss(c, forms[form], n, kind, 0, 3, *o)
            _keep(got, f"{form}-k{kind}-t0_3", *o)
            o = _outs(n)
            K.fused_loss(c, bands[form], n, kind, 3, 6, *o, row0=128, col0=128)
            _keep(got, f"{form}-k{kind}-t3_6-band", *o)


def _support_cases(K, n, x, got):
    c, sf = _dev(x["coords"]), _support(x)
    kinds = (0, 1, 2) if n != BIG else (1,)
    for kind in kinds:      # whole range, fp32 dcoords: a support launch of its own, cpad written
        o = _outs(n)
        K.fused_loss_support_range(c, sf, n, kind, 0, -1, 0, n, *o)
        _keep(got, f"k{kind}-whole", *o)
    if n != 300:
        return
    cmap = _dev(x["cmap"])
    # fp64 dcoords (a rank's share, the one-block moments path): riding support blocks, with and without
    # cmap; no tiles (support only); no support rows (tiles only)
    shares = {"t0_3-s0_150": (0, 3, 0, 150, None), "t0_3-s0_150-cmap": (0, 3, 0, 150, cmap),
              "t2_2-s100_200": (2, 2, 100, 200, None), "t0_3-s0_0": (0, 3, 0, 0, None)}
    for tag, (t0, t1, s0, s1, cm) in shares.items():
        for kind in kinds:
            o = _outs(n, d64=True)
            K.fused_loss_support_range(c, sf, n, kind, t0, t1, s0, s1, *o, cmap=cm)
            _keep(got, f"k{kind}-{tag}-dc64", *o)


def _moment(K, n, x, got):
    c, t = _dev(x["coords"]), x["truth"]
    forms = {"vec": _padded(t, padded_ld(n)), "glob": _padded(t, n | 1)}
    for form, tbuf in forms.items():
        if n == BIG and form != "vec":
            continue
        for mk in ((0, 1, 2) if n != BIG else (0,)):
            o = _outs(n)
            K.moment_loss(c, tbuf, n, mk, ALPHA, *o)
            _keep(got, f"{form}-m{mk}", *o)


def _moment_support(K, n, x, got):
    c, sf = _dev(x["coords"]), _support(x)
    for mk in (0, 1, 2):
        o = _outs(n)
        K.moment_loss_support(c, sf, n, mk, ALPHA, *o)
        _keep(got, f"m{mk}", *o)


def _bwd(K, n, x, got):
    from hicgat import _lib
    c = _dev(x["coords"])
    forms = {"vec": _padded(x["g"], padded_ld(n), fill=1e6)}
    if n == 300:
        forms["glob"] = _padded(x["g"], n | 1, fill=1e6)
    for form, G in forms.items():
        dc = torch.full((n, 3), float("nan"), dtype=torch.float32, device=DEV)
        ws = _lib.workspace(K.lib.hicgat_pairdist_workspace_bytes(n, K.PD_SQUARE), c.device)
        _lib.check(K.lib.hicgat_pairdist_bwd(_lib.ptr(c), _lib.ptr(G), n, G.shape[1], _lib.ptr(dc), _lib.ptr(ws),
                                             ws.numel(), _lib.stream(c.device)), "hicgat_pairdist_bwd")
        got[f"{form}-dcoords"] = dc


def _finalize(K, n, x, got):
    for kind in (0, 1, 2):
        stats, loss, _ = _outs(n, dc=False)
        stats.copy_(_dev(x["stats"]))
        K.loss_finalize(n, kind, stats, loss)
        _keep(got, f"k{kind}-stats_only", stats, loss, None)
        for reorder in (False, True):
            stats, loss, dcoords = _outs(n)
            stats.copy_(_dev(x["stats"]))
            cglob = torch.full((n, 3), float("nan"), dtype=torch.float32, device=DEV)
            ro = (_dev(x["cbuf"]), _dev(x["gidx"]), cglob) if reorder else None
            K.loss_finalize(n, kind, stats, loss, dc64=_dev(x["dc64"]), r0=40, r1=170, dcoords=dcoords, reorder=ro)
            tag = f"k{kind}-rows40_170" + ("-reorder" if reorder else "")
            _keep(got, tag, stats, loss, dcoords)
            if reorder:
                got[f"{tag}-cglob"] = cglob


FAMILIES = {"dense": _dense, "support": _support_cases, "moment": _moment, "moment_support": _moment_support,
            "bwd": _bwd, "finalize": _finalize}


def outputs(family, n):
    """Run every call of one (family, n) once; {name: tensor} of everything the calls wrote."""
    from hicgat import kernels
    got = {}
    FAMILIES[family](kernels.default(), n, inputs(n), got)
    torch.cuda.synchronize()
    return got


def workspace_bytes():
    """{N: [bytes]} of the four workspace queries (the first in both tilings); host code, no GPU."""
    from hicgat import _lib
    L = _lib.load()
    return {str(n): [L.hicgat_pairdist_workspace_bytes(n, 0), L.hicgat_pairdist_workspace_bytes(n, 1),
                     L.hicgat_pairdist_support_workspace_bytes(n), L.hicgat_pairdist_moment_loss_workspace_bytes(n),
                     L.hicgat_pairdist_moment_loss_support_workspace_bytes(n)] for n in WS_SIZES}


def test_workspace_queries_return_the_recorded_sizes():
    """The sizes are part of the C ABI: callers allocate by them and the entry points carve by the same layout."""
    with open(GOLDEN) as f:
        assert workspace_bytes() == json.load(f)["workspace_bytes"]


@pytest.fixture(scope="module")
def recorded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("family,n", CASES, ids=[f"{f}-n{n}" for f, n in CASES])
def test_pairdist_entry_points_keep_their_recorded_bits(recorded, family, n):
    case = recorded["cases"][f"{family}-n{n}"]
    assert inputs_sha(n) == case["inputs_sha256"], "inputs differ from the recorded draw: not a kernel failure"
    got = {k: sha(v) for k, v in outputs(family, n).items()}
    assert sorted(got) == sorted(case["sha256"])
    wrong = [k for k in sorted(got) if got[k] != case["sha256"][k]]
    assert not wrong, wrong

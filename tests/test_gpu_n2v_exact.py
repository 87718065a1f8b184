"""GPU: the node2vec kernels (csrc/node2vec.hip) through the C ABI against tests/n2v_ref.py.

Walks: whole-array equality -- every random decision is a counter-based draw and every choice an
integer or single-rounding fp32 comparison.  Skip-gram: the kept tokens, windows, targets and skips
are reproduced exactly by the reference, so only float rounding separates the device from the fp64
restatement.  The error measure is, per matrix, max|got - ref64| / max|ref64 - start| (relative to
the update, so one lost update shows); the bound of a case is 8 x the same measure of n2v_ref's own
fp32 mode against its fp64 mode (the margin: the device's dot is a 64-lane transpose reduction of
fmaf chains and expf, not numpy's summation order), with a floor of 1e-6.  Measured on an MI355X:
errors 2.8e-7 .. 5.2e-6 over all cases, each at most 0.15 of its bound (2.3e-6 .. 3.6e-5); with the
launch that rounded max_waves up to whole blocks the sequential case measured 3.5e-1."""
import ctypes

import numpy as np
import pytest
import torch

import n2v_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, EINVAL, EUNSUPPORTED = 0, -1, -3
A0, A1 = 0.025, 1e-4
MARGIN, FLOOR = 8.0, 1e-6


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hicgat  # noqa: F401


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- walks --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def walk_graph():
    """The 40-node graph of test_gpu_node2vec (self loop at 2, node 7 isolated), 7 rounds: 280 walks,
    one full 256-thread block and a partial one.  cumw and starts are made once, for both sides."""
    from oracle import node2vec as on
    a = n2v_ref.weighted_graph(40, 1)
    a[7, :] = a[:, 7] = 0
    rowptr, col, w = on.graph_csr(a)
    cumw, starts = n2v_ref.walk_inputs(rowptr, w, 7, 5)
    assert len(starts) == 280
    return dict(rowptr=rowptr, col=col, cumw=cumw, starts=starts, n=40,
                dev=[_dev(rowptr.astype(np.int32)), _dev(col.astype(np.int32)), _dev(cumw), _dev(starts)])


def _gpu_walks(g, nwalks, L, p, q, seed, fill=-7):
    from hicgat import _lib
    t_rowptr, t_col, t_cumw, t_starts = g["dev"]
    out = torch.full((max(nwalks, 1), L), fill, dtype=torch.int32, device=DEV)
    rc = _lib.lib().hicgat_n2v_walks(_ptr(t_rowptr), _ptr(t_col), _ptr(t_cumw), g["n"], _ptr(t_starts), nwalks, L,
                                     float(p), float(q), seed, _ptr(out), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("L", [1, 2, 30])
@pytest.mark.parametrize("p,q", [(0.5, 2.0), (1.75, 0.4), (1.0, 1.0)])
def test_walks_equal_reference(walk_graph, p, q, L):
    g = walk_graph
    rc, got = _gpu_walks(g, 280, L, p, q, 7)
    assert rc == OK
    ref = n2v_ref.walks(g["rowptr"], g["col"], g["cumw"], g["starts"], L, p, q, 7)
    assert got.dtype == ref.dtype and np.array_equal(got, ref), np.argwhere(got != ref)[:5]
    if L == 30:
        assert ((ref[:, 0] == 7) & (ref[:, 1] == -1)).sum() == 7 and (ref[ref[:, 0] != 7] >= 0).all()


def test_walks_refusals_leave_the_buffer(walk_graph):
    for p, q in ((0.0, 1.0), (1.0, 0.0)):
        rc, got = _gpu_walks(walk_graph, 280, 4, p, q, 7)
        assert rc == EINVAL and (got == -7).all(), (p, q)
    rc, got = _gpu_walks(walk_graph, 0, 4, 1.0, 1.0, 7)
    assert rc == OK and (got == -7).all()


# ---- skip-gram ----------------------------------------------------------------------------------
def _tables(V, D, rng):
    """U(-1/D, 1/D) syn0 and a non-zero syn1 of the same scale (an all-zero syn1 makes the first dots
    vanish, whatever lane they are read from), and a unigram^0.75 cumulative table."""
    syn0 = ((rng.random((V, D), dtype=np.float32) * 2 - 1) / D).astype(np.float32)
    syn1 = ((rng.random((V, D), dtype=np.float32) * 2 - 1) / D).astype(np.float32)
    pw = rng.integers(1, 200, V).astype(np.float64) ** 0.75
    cum = np.round(np.cumsum(pw) / pw.sum() * (2 ** 31 - 1)).astype(np.uint32)
    return syn0, syn1, cum


def _gpu_sgns(walks, keep, cum, V, D, window, negative, epoch, epochs, seed, max_waves, syn0, syn1, L=None,
              nwalks=None):
    """One hicgat_n2v_sgns_epoch launch on copies of syn0 / syn1: (rc, syn0, syn1) as numpy."""
    from hicgat import _lib
    t_walks, t_keep, t_cum = _dev(walks.astype(np.int32)), _dev(keep.astype(np.float32)), _dev(cum.view(np.int32))
    t0, t1 = _dev(syn0), _dev(syn1)
    rc = _lib.lib().hicgat_n2v_sgns_epoch(_ptr(t_walks), walks.shape[0] if nwalks is None else nwalks,
                                          walks.shape[1] if L is None else L, _ptr(t_keep), _ptr(t_cum), V, D,
                                          window, negative, A0, A1, epoch, epochs, seed, max_waves, _ptr(t0),
                                          _ptr(t1), _stream())
    torch.cuda.synchronize()
    return rc, t0.cpu().numpy(), t1.cpu().numpy()


def _measure(got, ref, start):
    den = np.abs(ref - start).max()
    return float(np.abs(got.astype(np.float64) - ref).max() / den) if den > 0 else None


def _check(name, got, ref64, ref32, start):
    """got within the case's bound of ref64, per matrix; a matrix the reference leaves alone must
    come back bit-identical.  Prints the measured error and the bound."""
    for which, g, r64, r32, s in zip(("syn0", "syn1"), got, ref64, ref32, start):
        err = _measure(g, r64, s.astype(np.float64))
        if err is None:
            print(f"[n2v] {name} {which}: no update in the reference; device bit-identical: {np.array_equal(g, s)}")
            assert np.array_equal(g, s), (name, which)
            continue
        bound = max(MARGIN * _measure(r32, r64, s.astype(np.float64)), FLOOR)
        print(f"[n2v] {name} {which}: err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (name, which, err, bound)


def _keep_third(V):
    keep = np.ones(V, np.float32)
    keep[::3] = np.linspace(0.35, 0.85, len(keep[::3]), dtype=np.float32)
    return keep


# name: D, L, V, window, negative, (epoch, epochs), keep, walk
#   keep  "third": below 1 for every third word; "all": 1; "none": 0; "one": 1 for word 5 alone
#   walk  "full": L random words; "tail": -1 from position 70 on; "single": word 5 once, at 40
CASES = {
    "D64_L1024_ballot16":  (64, 1024, 58, 5, 5, (0, 1), "third", "full"),
    "D128_L150_w25":       (128, 150, 58, 25, 5, (1, 3), "third", "full"),
    "D256_L65_neg7":       (256, 65, 58, 5, 7, (2, 3), "third", "full"),
    "D512_L64_neg0":       (512, 64, 58, 25, 0, (0, 1), "third", "full"),
    "D1024_L63_w1":        (1024, 63, 58, 1, 5, (1, 3), "all", "full"),
    "D1024_L150_refcall":  (1024, 150, 58, 25, 5, (0, 1), "third", "full"),
    "D64_L150_V3_neg7":    (64, 150, 3, 5, 7, (2, 3), "all", "full"),
    "D128_L65_V3_w25":     (128, 65, 3, 25, 5, (0, 1), "third", "full"),
    "D256_L150_tail":      (256, 150, 58, 5, 5, (1, 3), "third", "tail"),
    "D64_L2":              (64, 2, 58, 1, 7, (0, 1), "all", "full"),
    "D64_L1_n1":           (64, 1, 58, 5, 5, (0, 1), "all", "full"),
    "D512_L65_n0":         (512, 65, 58, 5, 5, (1, 3), "none", "full"),
    "D128_L150_n1":        (128, 150, 58, 5, 5, (2, 3), "one", "single"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_sgns_one_walk_matches_fp64(name):
    """nwalks = 1: one wave has work, so the launch is deterministic whatever max_waves means."""
    D, L, V, window, negative, (epoch, epochs), keep_kind, walk_kind = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    syn0, syn1, cum = _tables(V, D, rng)
    walks = rng.integers(0, V, (1, L)).astype(np.int32)
    if walk_kind == "tail":
        walks[0, 70:] = -1
    elif walk_kind == "single":
        walks[walks == 5] = 6
        walks[0, 40] = 5
    keep = _keep_third(V) if keep_kind == "third" else np.full(V, 1 if keep_kind == "all" else 0, np.float32)
    if keep_kind == "one":
        keep[5] = 1
    seed = 1000 + L
    kept = n2v_ref.kept_tokens(walks[0], 0, keep, epoch, seed)
    dropped = [pos for pos, tok in enumerate(walks[0])
               if tok >= 0 and not n2v_ref.u24(n2v_ref.rng4(seed, 0x5A3F + epoch, 0, pos)) < keep[tok]]
    if keep_kind == "third":                                    # the compaction really drops tokens, chunk by chunk
        assert dropped and len({pos // 64 for pos in dropped}) >= min(L // 64, 70 // 64 if walk_kind == "tail" else 16)
    if keep_kind in ("none", "one") or L == 1:
        assert len(kept) == (0 if keep_kind == "none" else 1)
    if walk_kind == "tail":
        assert 40 < len(kept) <= 70
    args = (walks, keep, cum, V, D, window, negative, A0, A1, epoch, epochs, seed, syn0, syn1)
    ref64 = n2v_ref.sgns_epoch(*args, np.float64)
    ref32 = n2v_ref.sgns_epoch(*args, np.float32)
    rc, g0, g1 = _gpu_sgns(walks, keep, cum, V, D, window, negative, epoch, epochs, seed, 1, syn0, syn1)
    assert rc == OK
    _check(name, (g0, g1), ref64, ref32, (syn0, syn1))


def test_sgns_skips_dots_beyond_six():
    """Words 0 and 1 carry +-sqrt(10) in component 5 of syn0 and syn1, so every dot between them is
    about +10 or -10 and is skipped; all other dots stay small.  On the fp64 reference no dot of
    the run lies within 0.1 of +-6, so a pair the device treats differently is a device error."""
    D, V, L, window, negative, seed = 64, 8, 100, 3, 5, 77
    rng = np.random.default_rng(6)
    syn0, syn1, cum = _tables(V, D, rng)
    s = np.float32(np.sqrt(10.0))
    syn0[0, 5], syn0[1, 5], syn1[0, 5], syn1[1, 5] = s, -s, s, s
    walks = rng.integers(0, V, (1, L)).astype(np.int32)
    keep = np.ones(V, np.float32)
    args = (walks, keep, cum, V, D, window, negative, A0, A1, 0, 1, seed, syn0, syn1)
    trace = []
    ref64 = n2v_ref.sgns_epoch(*args, np.float64, trace=trace)
    dots = np.array([x for *_, tg, ds in trace for t, x in zip(tg, ds) if t >= 0])
    assert not ((np.abs(dots) >= 5.9) & (np.abs(dots) <= 6.1)).any()
    assert (dots >= 6).sum() > 20 and (dots <= -6).sum() > 20 and (np.abs(dots) < 6).sum() > 1000
    print(f"[n2v] dot6: {len(dots)} dots, {(dots >= 6).sum()} >= 6, {(dots <= -6).sum()} <= -6, "
          f"largest below 6: {np.abs(dots[np.abs(dots) < 6]).max():.3f}")
    ref32 = n2v_ref.sgns_epoch(*args, np.float32)
    rc, g0, g1 = _gpu_sgns(walks, keep, cum, V, D, window, negative, 0, 1, seed, 1, syn0, syn1)
    assert rc == OK
    _check("dot6", (g0, g1), ref64, ref32, (syn0, syn1))


def test_sgns_max_waves_one_is_sequential():
    """max_waves = 1 trains the walks one after the other (include/hicgat.h: at most max_waves walks
    in flight): 9 walks, two epochs, equal to the reference, which takes them in order, and
    bit-equal between two runs."""
    D, V, L, nwalks, window, negative, seed = 64, 20, 40, 9, 5, 5, 31
    rng = np.random.default_rng(9)
    syn0, syn1, cum = _tables(V, D, rng)
    walks = rng.integers(0, V, (nwalks, L)).astype(np.int32)
    keep = _keep_third(V)
    r64, r32 = (syn0, syn1), (syn0, syn1)
    for ep in range(2):
        r64 = n2v_ref.sgns_epoch(walks, keep, cum, V, D, window, negative, A0, A1, ep, 2, seed, *r64, np.float64)
        r32 = n2v_ref.sgns_epoch(walks, keep, cum, V, D, window, negative, A0, A1, ep, 2, seed, *r32, np.float32)
    runs = []
    for _ in range(2):
        g = (syn0, syn1)
        for ep in range(2):
            rc, *g = _gpu_sgns(walks, keep, cum, V, D, window, negative, ep, 2, seed, 1, *g)
            assert rc == OK
        runs.append(g)
    same = all(np.array_equal(a, b) for a, b in zip(*runs))
    print(f"[n2v] sequential: two runs bit-equal: {same}")
    _check("sequential", runs[0], r64, r32, (syn0, syn1))
    assert same


REFUSALS = [
    ("walk_length_1025", dict(L=1025), EINVAL),
    ("negative_8", dict(negative=8), EINVAL),
    ("max_waves_0", dict(max_waves=0), EINVAL),
    ("epoch_eq_epochs", dict(epoch=3, epochs=3), EINVAL),
    ("window_0", dict(window=0), EINVAL),
    ("D_192", dict(D=192), EUNSUPPORTED),
    ("D_32", dict(D=32), EUNSUPPORTED),
    ("nwalks_0", dict(nwalks=0), OK),
]


@pytest.mark.parametrize("name,change,want", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_sgns_refusals_leave_the_tables(name, change, want):
    """Refused (or empty) calls return before any launch: syn0 / syn1 come back bit-identical."""
    a = dict(D=64, L=40, V=20, window=5, negative=5, epoch=0, epochs=3, max_waves=1, nwalks=3)
    a.update(change)
    rng = np.random.default_rng(4)
    syn0, syn1, cum = _tables(a["V"], a["D"], rng)
    walks = rng.integers(0, a["V"], (3, max(a["L"], 40))).astype(np.int32)
    rc, g0, g1 = _gpu_sgns(walks, np.ones(a["V"], np.float32), cum, a["V"], a["D"], a["window"], a["negative"],
                           a["epoch"], a["epochs"], 1, a["max_waves"], syn0, syn1, L=a["L"], nwalks=a["nwalks"])
    assert rc == want
    assert np.array_equal(g0, syn0) and np.array_equal(g1, syn1)

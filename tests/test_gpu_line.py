"""GPU: the LINE embeddings (csrc/line.hip through hicgat.embed.Line / embed.line) against the
NumPy restatement tests/line_ref.py: the sample stream bit for bit, one optimiser step, Keras'
Adam form, a 60-step trajectory within a tolerance taken from the reference's own float32 error,
bit reproducibility, planted structure, and the reference's call on chr19 1 mb.

The float tolerances are 16 x max|ref_fp32 - ref_fp64| at the test's own shape: the device differs
from the float32 reference by the order of its 64-lane dot and by its exp, each a few ulp."""
import numpy as np
import pytest
import torch

import line_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

SEED = 42


def _five():
    """N = 5, E = 7: K4 on nodes 0..3 plus a self loop at 1; node 4 is isolated, node 3 heads nothing."""
    a = np.zeros((5, 5))
    for i, j, v in ((0, 1, 5.0), (0, 2, 1.0), (0, 3, 2.0), (1, 2, 7.0), (1, 3, 1.0), (2, 3, 3.0), (1, 1, 4.0)):
        a[i, j] = a[j, i] = v
    return a


def _twelve():
    rng = np.random.default_rng(11)
    a = np.triu(rng.integers(1, 40, (12, 12)) * (rng.random((12, 12)) < 0.5), 1).astype(np.float64)
    return a + a.T


def _run(a, D, B, seed=SEED, both=False, **kw):
    from hicgat import embed
    h, t, w = embed.line_edges(a, both)
    return embed.Line(h, t, w, a.shape[0], D, B, 5, seed, "cuda", **kw), (h, t, w)


def _ref(run, edges, s0, s1, dtype, U0=None, C0=None, **kw):
    """line_ref.train on the run's own tables (host data of the ABI) from the initial tables."""
    if U0 is None:
        U0, C0 = line_ref.init(run.N, run.D, run.seed)
    u, c, _ = line_ref.train(U0, C0, edges[0], edges[1], (run.edge_accept, run.edge_alias),
                             (run.node_accept, run.node_alias), run.B, run.neg, run.seed, s0, s1, dtype, **kw)
    return u, c


def test_sample_stream_matches_reference_bit_for_bit():
    run, (h, t, w) = _run(_five(), 64, 4)
    assert run.E == 7 and run.steps_per_pass == 12
    nsteps = 36                                             # three passes
    dh, dt, dy = (x.cpu().numpy() for x in run.samples(0, nsteps))
    perms = line_ref.permutations(7, SEED, 3)
    node_p = line_ref.node_probs(h, w, 5)
    assert node_p[3] == 0 and node_p[4] == 0
    dup = 0
    for s in range(nsteps):
        rh, rt, ry = line_ref.batch(s, h, t, (run.edge_accept, run.edge_alias), (run.node_accept, run.node_alias), 5,
                                    4, 5, SEED, perms)
        ln = 3 if (s % 12) >= 6 else 4                      # each pass's last chunk is short
        assert len(rh) == ln
        assert np.array_equal(dh[s, :ln], rh) and np.array_equal(dt[s, :ln], rt) and np.array_equal(dy[s, :ln], ry)
        assert np.all(dh[s, ln:] == -1) and np.all(dt[s, ln:] == -1) and np.all(dy[s, ln:] == 0)
        b = s % 6
        assert np.all(dy[s, :ln] == (1 if b == 0 else -1))
        assert np.array_equal(dh[s], dh[s - b])             # batches 1-5 repeat batch 0's heads
        if b:
            assert not np.isin(dt[s, :ln], (3, 4)).any()    # zero-probability nodes are never negatives
        dup += len(set(rh.tolist())) < ln
    assert dup > 0                                          # duplicate heads do occur
    # a pure function of (seed, step, slot): any sub-range gives the same samples
    sh, st_, sy = (x.cpu().numpy() for x in run.samples(5, 29))
    assert np.array_equal(sh, dh[5:29]) and np.array_equal(st_, dt[5:29]) and np.array_equal(sy, dy[5:29])


@pytest.mark.parametrize("D", [64, 192, 512])
def test_one_step_matches_fp64_reference(D):
    run, edges = _run(_five(), D, 4)
    U0, C0 = line_ref.init(5, D, SEED)
    assert np.array_equal(run.U.cpu().numpy(), U0) and np.array_equal(run.C.cpu().numpy(), C0)
    run.train(0, 1)
    U, C = run.U.cpu().numpy(), run.C.cpu().numpy()
    (u32, c32), (u64, c64) = _ref(run, edges, 0, 1, np.float32), _ref(run, edges, 0, 1, np.float64)
    tol = 16 * max(np.abs(u32 - u64).max(), np.abs(c32 - c64).max())
    err = max(np.abs(U - u64).max(), np.abs(C - c64).max())
    print(f"D={D}: device vs fp64 {err:.3e}, fp32 ref vs fp64 {tol / 16:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    h, t, _ = line_ref.batch(0, edges[0], edges[1], (run.edge_accept, run.edge_alias),
                             (run.node_accept, run.node_alias), 5, 4, 5, SEED, line_ref.permutations(7, SEED, 1))
    for n in range(5):                                      # untouched rows keep their bits, touched ones move
        assert np.array_equal(U[n], U0[n]) == (n not in h), n
        assert np.array_equal(C[n], C0[n]) == (n not in t), n
    assert len(set(h.tolist())) < len(h) and len(set(t.tolist())) < len(t)   # duplicates were summed


def test_adam_is_keras_form_not_torch_form():
    """eps = 1e-2: Keras adds eps to sqrt(v), torch to sqrt(v) / sqrt(1 - b2^t); at t = 1 the two
    updates differ by ~5e-4 on every touched element."""
    run, edges = _run(_five(), 64, 4, eps=1e-2)
    U0, C0 = line_ref.init(5, 64, SEED)
    run.train(0, 1)
    U, C = run.U.cpu().numpy(), run.C.cpu().numpy()
    (u32, c32), (uk, ck) = _ref(run, edges, 0, 1, np.float32, eps=1e-2), _ref(run, edges, 0, 1, np.float64, eps=1e-2)
    ut, ct = _ref(run, edges, 0, 1, np.float64, eps=1e-2, form="torch")
    tol = 16 * max(np.abs(u32 - uk).max(), np.abs(c32 - ck).max())
    gap = max(np.abs(uk - ut).max(), np.abs(ck - ct).max())
    print(f"keras err {max(np.abs(U - uk).max(), np.abs(C - ck).max()):.3e} tol {tol:.3e}; forms differ by {gap:.3e}")
    assert gap > 1e-4 > 100 * tol
    assert max(np.abs(U - uk).max(), np.abs(C - ck).max()) <= tol
    assert max(np.abs(U - ut).max(), np.abs(C - ct).max()) > gap / 2


@pytest.fixture(scope="module")
def trajectory():
    """60 steps at N = 12, D = 64, B = 4: the device tables and the two references."""
    run, edges = _run(_twelve(), 64, 4)
    run.train(0, 60)
    return (run.U.cpu().numpy(), run.C.cpu().numpy(), _ref(run, edges, 0, 60, np.float32),
            _ref(run, edges, 0, 60, np.float64))


def test_trajectory_within_reference_float32_error(trajectory):
    U, C, (u32, c32), (u64, c64) = trajectory
    dev = max(np.abs(u32 - u64).max(), np.abs(c32 - c64).max())
    err = max(np.abs(U - u64).max(), np.abs(C - c64).max())
    moved = np.abs(u64 - line_ref.init(12, 64, SEED)[0]).max()
    print(f"60 steps: device vs fp64 {err:.3e}; fp32 ref vs fp64 {dev:.3e}; tolerance {16 * dev:.3e}; moved {moved:.3e}")
    assert moved > 1e-2                                     # the run went somewhere
    assert err <= 16 * dev


def test_trajectory_is_bit_reproducible_and_seeded(trajectory):
    U, C = trajectory[:2]
    again, _ = _run(_twelve(), 64, 4)
    again.train(0, 25).train(25, 60)                        # a split step range is the same run
    assert np.array_equal(again.U.cpu().numpy(), U) and np.array_equal(again.C.cpu().numpy(), C)
    other, _ = _run(_twelve(), 64, 4, seed=SEED + 1)
    other.train(0, 60)
    assert not np.array_equal(other.U.cpu().numpy(), U)


def _planted():
    rng = np.random.default_rng(3)
    a = np.zeros((16, 16))
    for i in range(16):
        for j in range(i + 1, 16):
            a[i, j] = a[j, i] = (10.0 if (i < 8) == (j < 8) else 1.0) * (1 + 0.1 * rng.random())
    return a


def _block_cosines(u):
    c = np.asarray(u, dtype=np.float64)
    c = c - c.mean(0)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    s = c @ c.T
    same = (np.arange(16) < 8)[:, None] == (np.arange(16) < 8)[None, :]
    return s[same & ~np.eye(16, dtype=bool)].mean(), s[~same].mean()


def test_planted_blocks_embed_apart():
    """Two blocks of 8 (weights ~10 inside, ~1 across), every edge both ways, 7 epochs at B = 16 (630
    steps): the reference alone separates them (within 0.63, across -0.68 at these settings), and
    so must the device."""
    from hicgat import embed
    a = _planted()
    h, t, w = embed.line_edges(a, both_directions=True)
    assert embed.line_steps(len(h), 16, 7) == 630
    tabs = (embed.alias_table(line_ref.edge_probs(w)), embed.alias_table(line_ref.node_probs(h, w, 16)))
    U0, C0 = line_ref.init(16, 64, SEED)
    ref_u, _, _ = line_ref.train(U0, C0, h, t, tabs[0], tabs[1], 16, 5, SEED, 0, 630, np.float64)
    rin, rout = _block_cosines(ref_u)
    u = embed.line(a, 64, batch_size=16, epochs=7, both_directions=True, seed=SEED)
    din, dout = _block_cosines(u.cpu().numpy())
    print(f"reference within {rin:.3f} across {rout:.3f}; device within {din:.3f} across {dout:.3f}")
    assert rin > rout + 0.5
    assert din > dout


def test_reference_call_chr19_1mb():
    """line(mat, 512, batch_size=128, epochs=10) as HiC-GNN_main.py:91-96 calls it on chr19 1 mb."""
    from hicgat import embed
    a = np.array(load_golden("graph_chr19_1mb.npz")["matrix"], dtype=np.float64)
    np.fill_diagonal(a, 0)
    n = a.shape[0]
    x = embed.line(a, 512, batch_size=128, epochs=10)
    assert isinstance(x, torch.Tensor) and x.is_cuda and tuple(x.shape) == (n, 512) and x.dtype == torch.float32
    x = x.cpu().numpy()
    assert np.isfinite(x).all()
    U0, _ = embed.line_init(n, 512, 42)
    assert np.array_equal(x[n - 1], U0[n - 1])              # the last node heads no edge: never trained
    assert not np.array_equal(x[0], U0[0])
    from oracle import graph as ogr
    from oracle import kr as okr
    normed, _ = okr.krnorm(a.copy())
    truth = ogr.cont2dist(ogr.load_input(normed.copy(), x)["y"], 0.5).numpy()
    print("chr19 1mb LINE embedding_stats:", {k: round(v, 4) for k, v in embed.embedding_stats(x, truth).items()})

"""CPU: the host side of the LINE embeddings (hicgat.embed.line_edges / alias_table / line_steps,
the CLI's ``line`` route) against tests/line_ref.py and the formulas of HiC-GNN_main.py:91-96's
``ge.LINE(order='second')``."""
import numpy as np
import pytest
import torch

import line_ref


def _six():
    a = np.zeros((6, 6))
    a[0, 1], a[1, 0] = 2.0, 3.0          # both set: the lower entry wins
    a[0, 3] = 1.5                        # only the upper entry
    a[4, 1] = 0.5                        # only the lower entry
    a[2, 2] = 7.0                        # a self loop
    a[2, 4], a[4, 2] = np.nan, 4.0       # NaN above, a weight below
    a[3, 5] = np.nan                     # NaN alone: no edge (5 stays isolated)
    return a


def test_line_edges_follow_networkx_rule():
    from hicgat import embed
    h, t, w = embed.line_edges(_six())
    assert list(zip(h.tolist(), t.tolist(), w.tolist())) == [(0, 1, 3.0), (0, 3, 1.5), (1, 4, 0.5), (2, 2, 7.0),
                                                             (2, 4, 4.0)]
    assert np.all(h <= t)
    for x, y in zip((h, t, w), line_ref.edges(_six())):
        assert np.array_equal(x, y)
    # graph_csr's weights: the list is the CSR's upper triangle, row-major
    rowptr, col, cw = embed.graph_csr(_six())
    row = np.repeat(np.arange(6), np.diff(rowptr))
    up = col >= row
    assert np.array_equal(h, row[up]) and np.array_equal(t, col[up]) and np.array_equal(w, cw[up])
    # both orientations: the (v, u) copies of every u < v edge follow, the self loop stays single
    h2, t2, w2 = embed.line_edges(_six(), both_directions=True)
    assert len(h2) == 9 and np.array_equal(h2[:5], h) and np.array_equal(t2[:5], t)
    assert list(zip(h2[5:].tolist(), t2[5:].tolist(), w2[5:].tolist())) == [(1, 0, 3.0), (3, 0, 1.5), (4, 1, 0.5),
                                                                            (4, 2, 4.0)]
    for x, y in zip((h2, t2, w2), line_ref.edges(_six(), True)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("case", ["zero_entry", "uniform", "skewed", "single"])
def test_alias_table_samples_p(case):
    from hicgat import embed
    rng = np.random.default_rng(4)
    p = {"zero_entry": np.array([0.3, 0.0, 0.25, 0.05, 0.4, 0.0]), "uniform": np.full(7, 1.0 / 7),
         "skewed": rng.random(257) ** 6, "single": np.array([1.0])}[case]
    p = p / p.sum()
    accept, alias = embed.alias_table(p)
    assert accept.dtype == np.float32 and alias.dtype == np.int32 and len(accept) == len(alias) == len(p)
    assert np.all((accept >= 0) & (accept <= 1)) and np.all((alias >= 0) & (alias < len(p)))
    assert np.abs(line_ref.implied(accept, alias) - p).max() <= 1e-6
    for i in np.nonzero(p == 0)[0]:          # never drawn: never kept, and no entry's alias
        assert accept[i] == 0 and p[alias[i]] > 0 and not np.any(alias[np.arange(len(p)) != i] == i)


def test_line_node_probs_count_heads_only():
    from hicgat import embed
    h, t, w = embed.line_edges(_six())
    p = embed.line_node_probs(h, w, 6)
    deg = np.array([4.5, 0.5, 11.0, 0.0, 0.0, 0.0])      # 3 and 4 are tails only, 5 is isolated
    assert np.allclose(p, deg ** 0.75 / (deg ** 0.75).sum(), rtol=1e-15)
    assert np.allclose(p, line_ref.node_probs(h, w, 6), rtol=1e-15)


@pytest.mark.parametrize("E,bs,ep,times", [(128, 32, 3, 1), (7, 4, 1, 1), (1711, 128, 10, 1), (10, 3, 2, 2),
                                            (5, 64, 1, 1)])
def test_line_steps_formula(E, bs, ep, times):
    from hicgat import embed
    want = ep * (((E * 6 - 1) // bs + 1) * times)
    assert embed.line_steps(E, bs, ep, times) == want == line_ref.steps(E, bs, ep, times)
    assert embed.line_steps(E, bs, ep, times, negative_ratio=2) == ep * (((E * 3 - 1) // bs + 1) * times)


def test_line_init_range_and_determinism():
    from hicgat import embed
    u, c = embed.line_init(9, 64, seed=5)
    u2, c2 = embed.line_init(9, 64, seed=5)
    assert u.dtype == np.float32 and u.shape == c.shape == (9, 64)
    assert np.array_equal(u, u2) and np.array_equal(c, c2) and not np.array_equal(u, c)
    assert np.abs(u).max() <= 0.05 and np.abs(c).max() <= 0.05 and u.std() > 0.02
    for x, y in zip((u, c), line_ref.init(9, 64, 5)):
        assert np.array_equal(x, y)


def test_abi_limits_are_checked_before_any_launch():
    """D % 64, D <= 1024, batch_size >= 1 are refused, and E == 0 is a no-op, before anything touches
    a pointer or the device (so this runs without a GPU)."""
    from hicgat import _lib
    lib = _lib.load()

    def train(E, D, B, steps=(0, 1)):
        return lib.hicgat_line_train(None, None, None, None, E, None, None, 5, None, 0, 1, D, B, 5, 42, steps[0],
                                     steps[1], 1e-3, 0.9, 0.999, 1e-7, None, None, None, None, None, None, None, 0,
                                     None)
    EINVAL, EUNSUPPORTED = -1, -3
    for D in (0, 32, 96, 100, 1088, 2048):
        assert train(7, D, 4) == EUNSUPPORTED, D
    assert train(7, 64, 0) == EINVAL and train(7, 64, -3) == EINVAL
    assert train(7, 64, 4, steps=(3, 2)) == EINVAL
    assert train(7, 64, 4) == EINVAL                         # NULL tables
    assert train(0, 64, 4) == 0 and train(0, 1024, 1, steps=(0, 1000)) == 0     # E == 0: nothing to do
    assert train(7, 512, 4, steps=(5, 5)) == 0              # an empty step range
    assert lib.hicgat_line_samples(None, None, None, None, 0, None, None, 5, None, 0, 0, 4, 5, 42, 0, 9, None, None,
                                   None, None) == 0
    assert lib.hicgat_line_workspace_bytes(512, 128) >= 2 * 128 * 512 * 4 + 3 * 128 * 4


@pytest.mark.parametrize("order", ["first", "all"])
def test_line_first_order_is_out_of_scope(order):
    from hicgat import embed
    with pytest.raises(NotImplementedError, match="second"):
        embed.line(np.ones((4, 4)), order=order)


def test_cli_routes_line_with_batchsize_and_epochs(tmp_path, monkeypatch):
    """main([list, "line", "-bs", "4", "-ep", "2", "--no-kr"]) calls embed.line with the zero-diagonal
    matrix, embedding_size 512, order 'second' and those two values (HiC-GNN_main.py:34-35, :91-96)."""
    from hicgat import embed
    from hicgat import train as T
    from test_cli_host import _FakeModel, _tiny_list
    seen = {}

    class _Data:
        def __init__(self, x, y):
            self.x, self.y, self.edge_index = x, y, None

    def fake_line(mat, embedding_size=512, order="second", batch_size=1024, epochs=1, **kw):
        seen.update(diag=np.diag(np.asarray(mat)).copy(), n=np.asarray(mat).shape[0], D=embedding_size, order=order,
                    bs=batch_size, ep=epochs, offdiag=float(np.abs(np.asarray(mat)).sum()))
        return torch.zeros(np.asarray(mat).shape[0], embedding_size)

    monkeypatch.setattr(T.graph, "load_input", lambda mat, feats, device="cuda": _Data(torch.as_tensor(feats),
                                                                                     torch.as_tensor(mat)))
    monkeypatch.setattr(T.graph.Truth, "from_contacts",
                        staticmethod(lambda y, f: T.graph.Truth(torch.rand(y.shape[0], y.shape[0]).double())))
    monkeypatch.setattr(T, "train", lambda model, data, truth, lr, thresh, steps, loss: (None, [1.0, 0.5]))
    monkeypatch.setattr(T.metrics, "dscc", lambda coords, truth: 0.5)
    monkeypatch.setattr(embed, "line", fake_line)
    monkeypatch.setitem(T.MODELS, "GATNetSelectiveResidualsUpdated", _FakeModel)
    assert T.main([_tiny_list(tmp_path), "line", "-bs", "4", "-ep", "2", "--no-kr", "-c", "[.5]"]) == 0
    assert seen["n"] == 12 and not seen["diag"].any() and seen["offdiag"] > 0
    assert (seen["D"], seen["order"], seen["bs"], seen["ep"]) == (512, "second", 4, 2)
    a = T.make_parser().parse_args(["m", "line"])
    assert (a.batchsize, a.epochs) == (128, 10)            # the reference's defaults

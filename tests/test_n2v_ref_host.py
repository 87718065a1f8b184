"""CPU: tests/n2v_ref.py, the NumPy restatement the exact node2vec GPU tests compare against, tied to
what the suite already trusts -- splitmix64's published vector, oracle/node2vec.py's exact
transition tables -- and to closed forms of the skip-gram rule."""
import collections

import numpy as np

import n2v_ref

SEED = 11


_weighted = n2v_ref.weighted_graph           # the graph of tests/test_gpu_node2vec.py


def _graph(a, num_walks, seed):
    from oracle import node2vec as on
    rowptr, col, w = on.graph_csr(a)
    cumw, starts = n2v_ref.walk_inputs(rowptr, w, num_walks, seed)
    return rowptr, col, w, cumw, starts


def test_splitmix_vector():
    assert n2v_ref.splitmix(0) == 0xe220a8397b1dcdaf
    assert n2v_ref.rng4(1, 2, 3, 4) == n2v_ref.splitmix(1 ^ n2v_ref.splitmix(2 ^ n2v_ref.splitmix(
        3 ^ n2v_ref.splitmix(4))))
    assert n2v_ref.u24((1 << 64) - 1) == np.float32(1 - 2.0 ** -24) and n2v_ref.u24((1 << 40) - 1) == 0


def test_walk_transition_frequencies_match_node2vec_table():
    """The bound of test_gpu_node2vec's frequency test, 2 / sqrt(count) + 0.01 in total variation, on
    a quarter of its walks (second-order contexts from 500 samples instead of 2000)."""
    from oracle import node2vec as on
    p, q = 0.5, 2.5
    rowptr, col, w, cumw, starts = _graph(_weighted(), 1000, SEED)
    walks = n2v_ref.walks(rowptr, col, cumw, starts, 6, p, q, SEED)
    first = collections.defaultdict(collections.Counter)
    second = collections.defaultdict(collections.Counter)
    for walk in walks:
        first[walk[0]][walk[1]] += 1
        for t in range(2, walk.shape[0]):
            second[(walk[t - 2], walk[t - 1])][walk[t]] += 1
    checked = 0
    for cur, cnt in first.items():
        nb, pr = on.first_step(rowptr, col, w, cur)
        tot = sum(cnt.values())
        emp = np.array([cnt[k] for k in nb]) / tot
        assert set(cnt) <= set(nb)
        assert 0.5 * np.abs(emp - pr).sum() < 2.0 / np.sqrt(tot) + 0.01, cur
        checked += 1
    for (prev, cur), cnt in second.items():
        tot = sum(cnt.values())
        if tot < 500:
            continue
        nb, pr = on.second_step(rowptr, col, w, prev, cur, p, q)
        emp = np.array([cnt[k] for k in nb]) / tot
        assert set(cnt) <= set(nb)
        assert 0.5 * np.abs(emp - pr).sum() < 2.0 / np.sqrt(tot) + 0.01, (prev, cur)
        checked += 1
    assert checked > 40


def test_walks_deterministic_isolated_start_and_length_one():
    a = _weighted(20, 1)
    a[7, :] = a[:, 7] = 0
    rowptr, col, _, cumw, starts = _graph(a, 2, 5)
    w1 = n2v_ref.walks(rowptr, col, cumw, starts, 12, 0.5, 2.0, 7)
    w2 = n2v_ref.walks(rowptr, col, cumw, starts, 12, 0.5, 2.0, 7)
    w3 = n2v_ref.walks(rowptr, col, cumw, starts, 12, 0.5, 2.0, 8)
    assert w1.dtype == np.int32 and w1.shape == (40, 12)
    assert np.array_equal(w1, w2) and not np.array_equal(w1, w3)
    for walk in w1:
        if walk[0] == 7:
            assert (walk[1:] == -1).all()
        else:
            assert (walk >= 0).all()
    assert (w1[:, 0] == 7).sum() == 2
    one = n2v_ref.walks(rowptr, col, cumw, starts, 1, 0.5, 2.0, 7)
    assert one.shape == (40, 1) and np.array_equal(one[:, 0], starts)


def _tables(V, D, seed=0):
    rng = np.random.default_rng(seed)
    syn0 = (rng.random((V, D)) * 2 - 1) / D
    syn1 = (rng.random((V, D)) * 2 - 1) / D
    cum = np.round(np.arange(1, V + 1) / V * (2 ** 31 - 1)).astype(np.uint32)
    return syn0, syn1, cum


def test_one_pair_closed_form():
    """Walk [2, 0], both kept, window 1, negative 0: centre 2 with context 0 updates (syn0[0],
    syn1[2]), centre 0 with context 2 updates (syn0[2], syn1[0]); each by g = (1 - sigmoid(dot)) *
    alpha with the rows as they stood."""
    V, D = 4, 8
    syn0, syn1, cum = _tables(V, D)
    syn0 *= 4                                                      # dots away from 0
    syn1 *= 4
    alpha = float(np.float32(0.025))
    got0, got1 = n2v_ref.sgns_epoch(np.array([[2, 0]], np.int32), np.ones(V, np.float32), cum, V, D, 1, 0,
                                    0.025, 1e-4, 0, 1, 9, syn0, syn1, np.float64)
    want0, want1 = syn0.copy(), syn1.copy()
    for word, ctx in ((2, 0), (0, 2)):
        dot = float(syn0[ctx] @ syn1[word])
        g = (1.0 - 1.0 / (1.0 + np.exp(-dot))) * alpha
        want0[ctx] = syn0[ctx] + g * syn1[word]
        want1[word] = syn1[word] + g * syn0[ctx]
    assert np.abs(got0 - want0).max() <= 1e-15 and np.abs(got1 - want1).max() <= 1e-15
    assert np.abs(got0[[0, 2]] - syn0[[0, 2]]).min() > 1e-6        # both rows really moved
    assert np.array_equal(got0[[1, 3]], syn0[[1, 3]]) and np.array_equal(got1[[1, 3]], syn1[[1, 3]])


def test_alpha_schedule():
    a = [float(n2v_ref.alpha_of(w, 4, 0.025, 1e-4, ep, 2)) for ep in range(2) for w in range(4)]
    want = [0.025 - (0.025 - 1e-4) * k / 8 for k in range(8)]
    assert np.allclose(a, want, rtol=1e-6) and a[0] == float(np.float32(0.025))


def test_negative_zero_touches_only_centre_rows_of_syn1():
    V, D = 12, 8
    syn0, syn1, cum = _tables(V, D, 1)
    walks = np.array([[1, 3, 5, 3, 1, 7, -1, -1], [5, 5, 9, 1, 3, 7, 9, 5]], np.int32)
    _, got1 = n2v_ref.sgns_epoch(walks, np.ones(V, np.float32), cum, V, D, 3, 0, 0.025, 1e-4, 0, 1, 2,
                                 syn0, syn1, np.float64)
    moved = set(np.nonzero(np.any(got1 != syn1, axis=1))[0])
    assert moved == {1, 3, 5, 7, 9}


def test_keep_zero_token_is_never_centre_or_context():
    V, D = 6, 8
    syn0, syn1, cum = _tables(V, D, 2)
    keep = np.array([1, 1, 0, 1, 0.5, 1], np.float32)
    walks = np.random.default_rng(3).integers(0, V, (3, 50)).astype(np.int32)
    trace = []
    got0, got1 = n2v_ref.sgns_epoch(walks, keep, cum, V, D, 4, 0, 0.025, 1e-4, 0, 1, 4, syn0, syn1, np.float64,
                                    trace=trace)
    assert trace and all(word != 2 and ctx != 2 for _, _, _, word, ctx, _, _ in trace)
    assert np.array_equal(got0[2], syn0[2]) and np.array_equal(got1[2], syn1[2])
    kept = [n2v_ref.kept_tokens(walks[w], w, keep, 0, 4) for w in range(3)]
    n4 = sum(k.count(4) for k in kept)
    assert 0 < n4 < (walks == 4).sum()                             # keep 0.5 drops some, not all
    assert all(k.count(1) == (walks[w] == 1).sum() for w, k in enumerate(kept))


def test_negative_samples_drop_the_word_and_follow_the_table():
    V = 3
    cum = np.array([2 ** 29, 2 ** 30, 2 ** 31 - 1], np.uint32)     # word 2 holds half the mass
    drawn = collections.Counter()
    for i in range(400):
        tg = n2v_ref.pair_targets(0, i, i + 1, 1, cum, V, 7, 0, 5)
        assert tg[0] == 1 and len(tg) == 8 and 1 not in tg[1:]
        drawn.update(t for t in tg[1:])
    tot = sum(drawn.values())
    assert abs(drawn[0] / tot - 0.25) < 0.03 and abs(drawn[-1] / tot - 0.25) < 0.03
    assert abs(drawn[2] / tot - 0.5) < 0.03


def test_all_padding_walk_changes_nothing():
    V, D = 5, 8
    syn0, syn1, cum = _tables(V, D, 3)
    walks = np.full((2, 70), -1, np.int32)
    for dtype in (np.float64, np.float32):
        got0, got1 = n2v_ref.sgns_epoch(walks, np.ones(V, np.float32), cum, V, D, 5, 5, 0.025, 1e-4, 0, 1, 1,
                                        syn0, syn1, dtype)
        assert got0.dtype == dtype
        assert np.array_equal(got0, syn0.astype(dtype)) and np.array_equal(got1, syn1.astype(dtype))

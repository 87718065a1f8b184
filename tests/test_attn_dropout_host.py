"""CPU: attention dropout's public surface (``GATConv(dropout=p)``, ``train(attn_dropout=)``, the
sharded trainer's refusal) and the numpy restatement of its mask (tests/attn_dropout_ref.py) that
the GPU tests compare the device mask against."""
import math

import numpy as np
import pytest
import torch

import attn_dropout_ref as adr
import philox_ref


# ---------------------------------------------------------------- the module
def test_constructor_accepts_dropout():
    import hicgat
    conv = hicgat.GATConv(512, 256, heads=2, dropout=0.6)
    assert conv.dropout == 0.6 and conv.training
    assert hicgat.GATConv(512, 256, heads=2).dropout == 0.0


@pytest.mark.parametrize("p", [-0.1, 1.0, float("nan")])
def test_constructor_refuses_a_bad_probability(p):
    import hicgat
    with pytest.raises(ValueError, match="0 <= p < 1"):
        hicgat.GATConv(512, 256, heads=2, dropout=p)


def test_the_other_refusals_stay():
    import hicgat
    with pytest.raises(NotImplementedError, match="concat"):
        hicgat.GATConv(512, 256, heads=2, concat=False, dropout=0.5)
    with pytest.raises(NotImplementedError, match="add_self_loops"):
        hicgat.GATConv(512, 256, heads=2, add_self_loops=False, dropout=0.5)


def test_state_dict_and_seeded_init_are_those_of_dropout_0():
    import hicgat
    torch.manual_seed(7)
    a = hicgat.GATConv(64, 128, heads=2)
    after_a = torch.rand(3)
    torch.manual_seed(7)
    b = hicgat.GATConv(64, 128, heads=2, dropout=0.6)
    after_b = torch.rand(3)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) == ["att_l", "att_r", "bias", "lin_l.weight", "lin_r.weight"]
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert not list(b.buffers())
    assert torch.equal(after_a, after_b)      # the constructor drew nothing more


def test_cpu_tensors_are_refused_before_the_library(monkeypatch):
    import hicgat

    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(hicgat._lib, "load", no_library)
    n = 6
    adj = hicgat.Adj([0, 1, 1, 2], [1, 0, 2, 1], sparse_sizes=(n, n))
    conv = hicgat.GATConv(64, 128, heads=2, dropout=0.5)
    x = torch.zeros(n, 64)
    with pytest.raises(hicgat._lib.HicgatUnavailable):
        conv(x, adj)                                     # the conv's own state needs a device
    W, al, ar, b = conv.lin_l.weight, conv.att_l, conv.att_r, conv.bias

    class State:                                         # a caller's state that claims no device
        seed, counter = 1, torch.zeros(1, dtype=torch.int64)

    with pytest.raises(hicgat._lib.HicgatUnavailable):
        hicgat.ops.gat_conv(x, W, al, ar, b, adj, dropout=0.5, training=True, state=State())
    with pytest.raises(hicgat._lib.HicgatUnavailable):
        hicgat.ops.attention_dropout_mask(adj.to("cpu"), 2, 0.5, 1, 1, 0)
    for p in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="0 <= p < 1"):
            hicgat.ops.gat_conv(x, W, al, ar, b, adj, dropout=p, training=True, state=State())
        with pytest.raises(ValueError, match="0 <= p < 1"):
            hicgat.ops.attention_dropout_mask(adj, 2, p, 1, 1, 0)
    with pytest.raises(ValueError, match="DropoutState"):
        hicgat.ops.gat_conv(x, W, al, ar, b, adj, dropout=0.5, training=True)
    for site in (-1, 1 << 31):
        with pytest.raises(ValueError, match="site"):
            hicgat.ops.gat_conv(x, W, al, ar, b, adj, dropout=0.5, training=True, state=State(), site=site)
    conv.dropout = 1.5                                   # set on the module, read at forward time
    with pytest.raises(ValueError, match="0 <= p < 1"):
        conv(x, adj)


def test_sharded_trainer_refuses_attention_dropout_before_any_collective():
    import hicgat
    model = hicgat.GATNetSelectiveResidualsUpdated()
    model.conv.dropout = 0.5
    with pytest.raises(NotImplementedError, match="attention dropout"):
        hicgat.dist.ShardedTrainer(model, torch.zeros(8, 512), None, None)     # no process group exists here


def test_train_surface():
    import inspect

    import hicgat
    from hicgat import train
    assert inspect.signature(train.train).parameters["attn_dropout"].default == 0.0
    a = train.make_parser().parse_args(["m.txt", "f.txt", "--attn-dropout", "0.6"])
    assert a.attn_dropout == 0.6
    assert train.make_parser().parse_args(["m.txt", "f.txt"]).attn_dropout == 0.0
    with pytest.raises(ValueError, match="0 <= p < 1"):
        train.train(hicgat.GATNetSelectiveResidualsUpdated(), None, None, attn_dropout=1.0)
    with pytest.raises(ValueError, match="GATConv"):
        train.train(hicgat.Net(), None, None, attn_dropout=0.5)


def test_library_exports_the_entry_points():
    from hicgat import _lib
    lib = _lib.load()
    for s in ("hicgat_gat_agg_fwd", "hicgat_gat_agg_bwd_src", "hicgat_gat_attn_mask"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    # dropout and the dense tiles are operands of those two, not entry points of their own
    for form in ("drop_fwd", "fwd_tiled", "drop_bwd_src", "bwd_src_tiled"):
        s = "hicgat_gat_agg_" + form
        assert not hasattr(lib, s) and s not in _lib.SIGNATURES, s


# ---------------------------------------------------------------- the mask's restatement
def _ring(n, extra=()):
    a = np.zeros((n, n), bool)
    for i in range(n):
        a[i, (i + 1) % n] = a[(i + 1) % n, i] = True
    for i, j in extra:
        a[i, j] = a[j, i] = True
    np.fill_diagonal(a, True)
    r, c = np.nonzero(a)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=n))
    return rowptr, c


def test_counter_layout_and_threshold():
    rowptr, col = _ring(9, [(0, 4)])
    seed, step, site, p = 0x1234567890ABCDEF, 5, 3, 0.6
    m = adr.keep_mask(rowptr, col, 4, p, seed, step, site)
    rows = np.repeat(np.arange(9), np.diff(rowptr))
    T = philox_ref.threshold(p)
    for e in (0, 7, len(col) - 1):
        w = philox_ref.philox4x32_10([np.uint64(rows[e]), np.uint64(col[e]), np.uint64(step),
                                      np.uint64(site | 0x80000000)], (seed & 0xFFFFFFFF, seed >> 32))
        assert [bool(int(x) >= T) for x in w] == m[e].tolist()
    # head hh is word hh whatever H is; p = 0 keeps everything; the step enters modulo 2^32
    assert np.array_equal(adr.keep_mask(rowptr, col, 2, p, seed, step, site), m[:, :2])
    assert adr.keep_mask(rowptr, col, 4, 0.0, seed, step, site).all()
    assert np.array_equal(adr.keep_mask(rowptr, col, 4, p, seed, step + 2 ** 32, site), m)
    # the high site bit: an attention site is not the feature-dropout site of the same number
    plain = philox_ref.philox4x32_10([np.uint64(rows[0]), np.uint64(col[0]), np.uint64(step), np.uint64(site)],
                                     (seed & 0xFFFFFFFF, seed >> 32))
    assert [int(x) for x in plain] != [int(x) for x in adr.edge_words(rows[:1], col[:1], seed, step, site)[0]]
    with pytest.raises(AssertionError):
        adr.keep_mask(rowptr, col, 2, p, seed, step, 1 << 31)


def test_mask_depends_on_the_edge_not_on_its_position():
    """(i, j) are node ids: a row range, or the same edge in another CSR, has the same bits; (i, j) and
    (j, i) do not share theirs."""
    rowptr, col = _ring(40)
    rowptr2, col2 = _ring(40, [(3, 20), (0, 9)])
    m, m2 = adr.keep_mask(rowptr, col, 2, 0.5, 11, 1, 0), adr.keep_mask(rowptr2, col2, 2, 0.5, 11, 1, 0)
    rows, rows2 = np.repeat(np.arange(40), np.diff(rowptr)), np.repeat(np.arange(40), np.diff(rowptr2))
    look = {(int(i), int(j)): m2[e] for e, (i, j) in enumerate(zip(rows2, col2))}
    assert all(np.array_equal(look[(int(i), int(j))], m[e]) for e, (i, j) in enumerate(zip(rows, col)))
    rev = np.array([look[(int(j), int(i))] for i, j in zip(rows2, col2)])
    off = rows2 != col2
    assert 0.25 < (rev[off] != m2[off]).mean() < 0.75


@pytest.mark.parametrize("p", [0.5, 0.9, 0.6])
def test_keep_rate_and_independence(p):
    n = 150
    rowptr = np.arange(n + 1, dtype=np.int64) * n
    col = np.tile(np.arange(n), n)
    m = adr.keep_mask(rowptr, col, 4, p, 77, 1, 0)
    q = 1.0 - philox_ref.threshold(p) / 2.0 ** 32
    sig = abs(m.mean() - q) / math.sqrt(q * (1 - q) / m.size)
    print(f"p={p}: kept {m.mean():.5f}, {sig:.2f} sigma over {m.size} samples")
    assert sig < 5
    for what, o in {"step": adr.keep_mask(rowptr, col, 4, p, 77, 2, 0), "site": adr.keep_mask(rowptr, col, 4, p, 77, 1, 1),
                    "seed": adr.keep_mask(rowptr, col, 4, p, 78, 1, 0)}.items():
        c = abs(np.corrcoef(m.ravel().astype(float), o.ravel().astype(float))[0, 1]) * math.sqrt(m.size)
        assert c < 5, (what, c)

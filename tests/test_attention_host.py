"""Host side of the GATConv attention weights: the fp64 restatement the GPU tests compare against is
tied to ``oracle.gat.GATConv``, the closed-form backward of a gradient on alpha (what the two HIP passes
of gat_attn.hip compute) is checked against that restatement's autograd, and the public surface.  No GPU."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import attention_ref as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAME = "GATNetHeadsChanged3LayersEmbeddingDim256Entropy"


def _oracle_csr(name):
    a = ar.GRAPHS[name]()
    r, c = np.nonzero(a)
    rowptr = np.zeros(a.shape[0] + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=a.shape[0]))
    return torch.tensor(rowptr), torch.tensor(c.astype(np.int64))


def _problem(name, F, C, H, seed):
    from oracle import gat as og
    torch.manual_seed(seed)
    conv = og.GATConv(F, C, heads=H).double()
    with torch.no_grad():
        conv.bias.copy_(torch.randn_like(conv.bias) * 0.1)
    n = ar.GRAPHS[name]().shape[0]
    x = torch.tensor(0.1 * np.random.default_rng(seed).standard_normal((n, F)))
    return conv, x


@pytest.mark.parametrize("name", sorted(ar.GRAPHS))
@pytest.mark.parametrize("C,H", [(128, 2), (256, 4)])
def test_restatement_matches_the_oracle_gatconv(name, C, H):
    conv, x = _problem(name, 64, C, H, 3)
    with torch.no_grad():
        want = conv(x, _oracle_csr(name))
        out, alpha, _ = ar.gat_attention(x, conv.lin_l.weight, conv.att_l, conv.att_r, conv.bias,
                                         *ar.csr_with_self_loops(name))
    assert float((out - want).abs().max()) < 1e-12
    rowptr, _ = ar.csr_with_self_loops(name)
    sums = torch.zeros(len(rowptr) - 1, H, dtype=torch.float64).index_add(0, ar.rows_of(rowptr), alpha)
    assert float((sums - 1).abs().max()) < 1e-12
    if name == "n7":
        assert torch.equal(alpha[rowptr[6]:rowptr[7]], torch.ones(1, H, dtype=torch.float64))


@pytest.mark.parametrize("name", sorted(ar.GRAPHS))
@pytest.mark.parametrize("C,H", [(128, 2), (128, 1), (128, 4)])
def test_closed_form_alpha_backward_matches_autograd(name, C, H):
    conv, x = _problem(name, 32, C, H, 5)
    rowptr, col = ar.csr_with_self_loops(name)
    x.requires_grad_(True)
    out, alpha, z = ar.gat_attention(x, conv.lin_l.weight, conv.att_l, conv.att_r, conv.bias, rowptr, col)
    G = torch.tensor(np.random.default_rng(9).standard_normal(tuple(alpha.shape)))
    (alpha * G).sum().backward()
    got = ar.alpha_backward_np(x.detach(), conv.lin_l.weight.detach(), conv.att_l.detach(), conv.att_r.detach(),
                               rowptr, col, alpha.detach(), z.detach(), G)
    want = {"x": x.grad, "W": conv.lin_l.weight.grad, "att_l": conv.att_l.grad, "att_r": conv.att_r.grad}
    for k, w in want.items():
        err = np.abs(got[k] - w.numpy()).max() / max(float(w.abs().max()), 1e-300)
        assert err < 1e-10, (k, err)
    assert conv.bias.grad is None            # alpha does not depend on the bias


@pytest.mark.parametrize("name", sorted(ar.GRAPHS))
def test_numpy_transpose_map_is_an_involution(name):
    rowptr, col = ar.csr_with_self_loops(name)
    t = ar.transpose_map_np(rowptr, col)
    assert np.array_equal(t[t], np.arange(len(t)))
    row = ar.rows_of(rowptr).numpy()
    loops = row == col.numpy()
    assert np.array_equal(t[loops], np.nonzero(loops)[0])
    assert np.array_equal(row[t], col.numpy()) and np.array_equal(col.numpy()[t], row)


def test_fixture_graphs_have_the_rows_they_are_for():
    deg = {k: np.diff(ar.csr_with_self_loops(k)[0].numpy()) for k in ar.GRAPHS}
    assert deg["n7"][6] == 1
    assert set(deg["n70"]) == {70}
    assert set(deg["n130"]) == {2, 3, 4, 130} and len(deg["n130"]) % 4 != 0
    assert {63, 64, 65} <= set(deg["deg63"])
    for k in ar.GRAPHS:
        a = ar.GRAPHS[k]()
        assert np.array_equal(a, a.T) and not a.diagonal().any()


def test_public_surface():
    import hicgat
    from hicgat import train
    sig = inspect.signature(hicgat.GATConv.forward)
    assert "return_attention_weights" in sig.parameters and sig.parameters["return_attention_weights"].default is None
    assert list(sig.parameters)[:4] == ["self", "x", "edge_index", "act"]
    assert "return_attention_weights" in inspect.signature(hicgat.ops.gat_conv).parameters
    assert NAME in hicgat.MODELS and getattr(hicgat, NAME) is hicgat.MODELS[NAME]
    assert len(hicgat.MODELS) == 12
    assert NAME in next(a.choices for a in train.make_parser()._actions if "--model" in a.option_strings)


def test_entropy_model_layout_matches_the_reference_class():
    """Keys, shapes, parameter count and ``alpha`` recorded from the reference's models.py:1112-1148
    (tests/golden/make_entropy_layout.py), and the seeded init of the restatement the GPU test trains."""
    import hicgat
    with open(os.path.join(GOLDEN, f"layout_{NAME}.json")) as fh:
        fx = json.load(fh)
    torch.manual_seed(0)
    mine = hicgat.MODELS[NAME]()
    torch.manual_seed(0)
    ref = ar.EntropyRef()
    for m in (mine, ref):
        sd = m.state_dict()
        assert list(sd) == fx["keys"]
        assert [list(v.shape) for v in sd.values()] == fx["shapes"]
        assert sum(p.numel() for p in m.parameters()) == fx["parameters"]
        assert m.alpha == fx["alpha"]
        assert [n for n, _ in m.named_children()] == fx["children"]
    for k, v in mine.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k]), k


def test_attention_entropy_is_the_reference_expression():
    from hicgat import ops
    a = torch.rand(50, 2, dtype=torch.float64)
    assert torch.equal(ops.attention_entropy(a), -torch.sum(a * torch.log(a + 1e-12)))


def test_refusals_need_no_device():
    import hicgat
    conv = hicgat.GATConv(64, 96, heads=2)
    with pytest.raises(NotImplementedError, match="out_channels % 128"):
        conv(torch.zeros(4, 64), None, return_attention_weights=True)
    with pytest.raises(NotImplementedError, match=r"GATConv\(512, 256, heads=2\)"):
        hicgat.dist.ShardedTrainer(hicgat.MODELS[NAME](), torch.zeros(8, 256), None, None)

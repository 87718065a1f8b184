"""Host side of the LayerNorm tails on the HIP path: the six models on the public surface, their layout
against fixtures recorded from the reference's own classes (tests/golden/make_layernorm_layouts.py) and
against a module built with the reference's constructor lines over the oracle's GATConv, the library's
entry points, and the argument checks that come before the library.  No GPU."""
import json
import os

import pytest
import torch
import torch.nn.functional as F
from torch.nn import LayerNorm, Linear

from conftest import GOLDEN

RELU_LN, LEAKY_LN, EMBED512, SELECTIVE, WITH_RES, UPDATED_LN = NAMES = (
    "GATNetHeadsChanged4LayersReLU_LayerNorm", "GATNetHeadsChanged4LayersLeakyReLU_LayerNorm",
    "GATNetHeadsChanged4LayersReLU_LayerNormEmbed512", "GATNetSelectiveResiduals",
    "GATNetHeadsChanged4LayersReLU_LayerNormEmbed512WithResiduals", "GATNetSelectiveResidualsUpdatedLayerNorm")
COUNTS = dict(zip(NAMES, (110083, 110083, 437251, 609731, 873411, 602243)))
ENTRY_POINTS = ("hicgat_ln_act_res_fwd", "hicgat_ln_act_res_bwd", "hicgat_ln_act_res_bwd_params",
                "hicgat_ln_act_res_workspace_bytes", "hicgat_act_fwd", "hicgat_act_bwd")


def feats(name):
    """Feature columns of the model's input."""
    return 256 if name in (RELU_LN, LEAKY_LN) else 512


def ref_model(name):
    """The reference's constructor over the oracle's GATConv, submodules in its order."""
    from oracle import gat as og
    m = torch.nn.Module()
    if name in (RELU_LN, LEAKY_LN):                        # models.py:324-335, :779-790
        m.conv = og.GATConv(256, 128, heads=2, concat=True)
        m.densea = Linear(256, 128)
        m.norm_a = LayerNorm(128)
        m.dense1 = Linear(128, 64)
        m.norm1 = LayerNorm(64)
        m.dense2 = Linear(64, 32)
        m.norm2 = LayerNorm(32)
        m.dense3 = Linear(32, 3)
    elif name == EMBED512:                                 # models.py:383-394
        m.conv = og.GATConv(512, 256, heads=2, concat=True)
        m.densea = Linear(512, 256)
        m.norm_a = LayerNorm(256)
        m.dense1 = Linear(256, 128)
        m.norm1 = LayerNorm(128)
        m.dense2 = Linear(128, 64)
        m.norm2 = LayerNorm(64)
        m.dense3 = Linear(64, 3)
    elif name == WITH_RES:                                 # models.py:441-459
        m.conv1 = og.GATConv(512, 256, heads=2, concat=True)
        m.norm1 = LayerNorm(512)
        m.densea = Linear(512, 256)
        m.norm_a = LayerNorm(256)
        m.dense1 = Linear(256, 128)
        m.norm1_2 = LayerNorm(128)
        m.dense2 = Linear(128, 64)
        m.norm2 = LayerNorm(64)
        m.dense3 = Linear(64, 3)
        m.align1 = Linear(512, 512)
        m.align_a = Linear(512, 256)
        m.align1_2 = Linear(256, 128)
        m.align2 = Linear(128, 64)
    elif name == SELECTIVE:                                # models.py:532-549
        m.conv = og.GATConv(512, 256, heads=2, concat=True)
        m.densea = Linear(512, 256)
        m.norm_a = LayerNorm(256)
        m.align_densea = Linear(512, 256)
        m.dense1 = Linear(256, 128)
        m.norm1 = LayerNorm(128)
        m.align_dense1 = Linear(256, 128)
        m.dense2 = Linear(128, 64)
        m.norm2 = LayerNorm(64)
        m.align_dense2 = Linear(128, 64)
        m.dense3 = Linear(64, 3)
    else:                                                  # models.py:697-712
        assert name == UPDATED_LN
        m.conv = og.GATConv(512, 256, heads=2, concat=True)
        m.densea = Linear(512, 256)
        m.norm_a = LayerNorm(256)
        m.align_densea = Linear(512, 256)
        m.norm_residual_a = LayerNorm(256)
        m.dense1 = Linear(256, 128)
        m.norm1 = LayerNorm(128)
        m.align_dense1 = Linear(256, 128)
        m.norm_residual_1 = LayerNorm(128)
        m.dense2 = Linear(128, 64)
        m.norm2 = LayerNorm(64)
        m.dense3 = Linear(64, 3)
    return m


def ref_coords(name, m, x, adj, pre=None):
    """The reference's ``get_model`` (its ``forward`` before the cdist runs the same lines) on the restated
    module ``m``.  ``pre`` receives every tensor an activation with a kink (relu, leaky_relu) reads."""
    def kink(h):
        if pre is not None and name != UPDATED_LN:
            pre.append(h.detach())
        return h

    if name in (RELU_LN, LEAKY_LN, EMBED512):              # models.py:359-377, :814-832, :417-435
        act = F.leaky_relu if name == LEAKY_LN else F.relu
        h = act(kink(m.conv(x, adj)))
        h = act(kink(m.norm_a(m.densea(h))))
        h = act(kink(m.norm1(m.dense1(h))))
        h = act(kink(m.norm2(m.dense2(h))))
        return m.dense3(h)
    if name == WITH_RES:                                   # models.py:495-526
        h = F.relu(kink(m.norm1(m.conv1(x, adj)))) + m.align1(x)
        h = F.relu(kink(m.norm_a(m.densea(h)))) + m.align_a(h)
        h = F.relu(kink(m.norm1_2(m.dense1(h)))) + m.align1_2(h)
        h = F.relu(kink(m.norm2(m.dense2(h)))) + m.align2(h)
        return m.dense3(h)
    if name == SELECTIVE:                                  # models.py:583-612
        h = F.relu(kink(m.conv(x, adj)))
        h = F.relu(kink(m.norm_a(m.densea(h)))) + m.align_densea(h)
        h = F.relu(kink(m.norm1(m.dense1(h)))) + m.align_dense1(h)
        h = F.relu(kink(m.norm2(m.dense2(h)))) + m.align_dense2(h)
        return m.dense3(h)
    h = F.gelu(m.conv(x, adj))                             # models.py:745-773
    h = m.norm_residual_a(F.gelu(m.norm_a(m.densea(h))) + m.align_densea(h))
    h = m.norm_residual_1(F.gelu(m.norm1(m.dense1(h))) + m.align_dense1(h))
    h = F.gelu(m.norm2(m.dense2(h)))
    return m.dense3(h)


def test_models_on_the_public_surface():
    import hicgat
    from hicgat import align, train
    assert tuple(hicgat.LN_MODELS) == NAMES
    assert list(hicgat.ALL_MODELS) == list(hicgat.MODELS) + list(hicgat.LN_MODELS)
    assert len(hicgat.MODELS) == 12 and not set(hicgat.MODELS) & set(NAMES)
    for parser in (train.make_parser(), align.make_parser()):
        choices = next(a.choices for a in parser._actions if "--model" in a.option_strings)
        assert set(choices) == set(hicgat.ALL_MODELS)
    for name in NAMES:
        assert getattr(hicgat, name) is hicgat.LN_MODELS[name] is hicgat.ALL_MODELS[name]
        assert hicgat.gat_models.model_class(name) is hicgat.LN_MODELS[name]
        for attr in ("get_model", "forward", "loss", "flat_parameters"):
            assert callable(getattr(hicgat.LN_MODELS[name], attr))


@pytest.mark.parametrize("name", NAMES)
def test_layout_matches_the_reference_class(name):
    """Keys, shapes, child order and parameter count recorded from the reference's own class."""
    import hicgat
    with open(os.path.join(GOLDEN, f"layout_{name}.json")) as fh:
        fx = json.load(fh)
    mine = hicgat.LN_MODELS[name]()
    sd = mine.state_dict()
    assert list(sd) == fx["keys"]
    assert [list(v.shape) for v in sd.values()] == fx["shapes"]
    assert [n for n, _ in mine.named_children()] == fx["children"]
    assert sum(p.numel() for p in mine.parameters()) == fx["parameters"] == COUNTS[name]


@pytest.mark.parametrize("name", NAMES)
def test_children_keys_and_seeded_init_match_the_restated_constructor(name):
    import hicgat
    torch.manual_seed(11)
    ref = ref_model(name)
    torch.manual_seed(11)
    mine = hicgat.LN_MODELS[name]()
    assert [n for n, _ in ref.named_children()] == [n for n, _ in mine.named_children()]
    sr, sm = ref.state_dict(), mine.state_dict()
    assert list(sr) == list(sm)
    for k in sr:
        assert torch.equal(sr[k], sm[k]), k
    assert sum(p.numel() for p in ref.parameters()) == COUNTS[name]
    flat = mine.flat_parameters()                   # every parameter once, the residual pairs adjacent
    assert sorted(id(p) for p in flat) == sorted(id(p) for p in mine.parameters())
    for dense, _, align, _ in mine.stages:
        if align:
            k = next(i for i, p in enumerate(flat) if p is getattr(mine, dense).weight)
            assert flat[k + 1] is getattr(mine, align).weight
            assert flat[k + 2] is getattr(mine, dense).bias and flat[k + 3] is getattr(mine, align).bias


def test_library_exports_the_entry_points():
    from hicgat import _lib
    lib = _lib.load()
    for s in ENTRY_POINTS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    for W in (32, 64, 128, 256, 512):
        one, two = (lib.hicgat_ln_act_res_workspace_bytes(W, n2) for n2 in (0, 1))
        assert 0 < one < two
    assert lib.hicgat_ln_act_res_workspace_bytes(96, 0) == 0 == lib.hicgat_ln_act_res_workspace_bytes(96, 1)
    assert hicgat_kernels().ACT_GELU == 3


def hicgat_kernels():
    from hicgat import kernels
    return kernels.HipKernels


def test_refusals_come_before_the_library(monkeypatch):
    import hicgat

    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(hicgat._lib, "load", no_library)
    monkeypatch.setattr(hicgat._lib, "lib", no_library)
    monkeypatch.setattr(hicgat.kernels, "default", no_library)
    ops = hicgat.ops
    y, x = torch.zeros(4, 64), torch.zeros(4, 128)
    l1, l2 = Linear(128, 64), Linear(128, 64)

    def both(norm, act="relu", norm2=None):
        """The same refusal from the plain and the dual op."""
        yield lambda: ops.ln_act_res(y, norm, act, norm2=norm2)
        yield lambda: ops.dual_ln_act_res(x, l1, l2, norm, act, norm2)

    for f in both(torch.nn.BatchNorm1d(64)):
        with pytest.raises(TypeError, match="LayerNorm"):
            f()
    for f in both(LayerNorm(64, elementwise_affine=False)):
        with pytest.raises(NotImplementedError, match="elementwise_affine=False"):
            f()
    for f in both(LayerNorm((4, 64))):
        with pytest.raises(NotImplementedError, match="2-D normalized_shape"):
            f()
    for f in both(LayerNorm(96)):
        with pytest.raises(NotImplementedError, match="widths"):
            f()
    for f in both(LayerNorm(64), norm2=LayerNorm(128)):
        with pytest.raises(ValueError, match="norm2 must have norm's width 64"):
            f()
    for f in both(LayerNorm(64), norm2=torch.nn.BatchNorm1d(64)):
        with pytest.raises(TypeError, match="norm2"):
            f()
    for f in both(LayerNorm(64), act="tanh"):
        with pytest.raises(ValueError, match="activation must be"):
            f()
    for f in both(LayerNorm(64), act=("leaky_relu", 0.0)):
        with pytest.raises(ValueError, match="slope > 0"):
            f()
    with pytest.raises(ValueError, match=r"float32 \[rows, 64\]"):
        ops.ln_act_res(x, LayerNorm(64), "relu")
    with pytest.raises(ValueError, match="res must"):
        ops.ln_act_res(y, LayerNorm(64), "relu", res=torch.zeros(3, 64))
    with pytest.raises(ValueError, match="64 outputs"):
        ops.dual_ln_act_res(x, l1, Linear(128, 32), LayerNorm(64), "relu")
    with pytest.raises(ValueError, match="ops.act runs"):
        ops.act(y, "relu")
    with pytest.raises(ValueError, match="W % 4 == 0"):
        ops.act(torch.zeros(4, 6), "gelu")
    for f in list(both(LayerNorm(64), act="gelu", norm2=LayerNorm(64))) + [lambda: ops.act(y, "gelu")]:
        with pytest.raises(hicgat._lib.HicgatUnavailable):       # well-formed: CPU tensors do not run
            f()
    with pytest.raises(ValueError, match="act must be"):         # the dropout / BatchNorm parser has no gelu
        ops._act_code("gelu")
    assert ops._ln_act_code("gelu") == (3, 0.0) and ops._ln_act_code(("leaky_relu", 0.2)) == (2, 0.2)
    assert ops._ln_act_code("leaky_relu") == (2, 0.01) and ops._ln_act_code(None) == (0, 0.0)


def test_kink_free_inputs_exist_for_every_row_pass_case():
    """The draw of tests/test_gpu_ln_act.py's first test is CPU-only: it succeeds for every case with a
    kink, and what it returns is off the kink by the stated margin."""
    import ln_act_ref as lr
    for W in lr.WIDTHS:
        for act in ("relu", ("leaky_relu", 0.01)):
            for has_res in (False, True):
                for has_n2 in (False, True):
                    for M in lr.rows_of(W):
                        pre = lr.drawn(M, W, act, has_res, has_n2)[5]["pre"]
                        assert (pre.abs() > 1e-6 * pre.abs().max()).all(), (M, W, act, has_res, has_n2)


@pytest.mark.parametrize("name", NAMES)
def test_kink_free_model_seed_exists(name):
    """The seed search of the GPU model-step test, which is CPU-only too."""
    import ln_act_ref  # noqa: F401  (same directory: the search lives with the GPU test's helpers)
    from test_gpu_ln_act import seeded_reference, problem
    _, _, d, _ = problem(feats(name))
    radj = (torch.tensor(d["rowptr"]), torch.tensor(d["col"]))
    seed, ref = seeded_reference(name, d["x"], radj)
    assert 0 <= seed < 8 and ref.training


def test_sharded_trainer_refuses_the_six_before_any_collective():
    """By name and before it looks at a process group (none exists here): three of them have the
    flagship's norm_a / norm1 / norm2 and GATConv(512, 256, heads=2)."""
    import hicgat
    for name in NAMES:
        with pytest.raises(NotImplementedError, match="single-GPU hicgat.train only"):
            hicgat.dist.ShardedTrainer(hicgat.LN_MODELS[name](), torch.zeros(8, feats(name)), None, None)


def test_the_flagship_keeps_its_tail():
    """The new models' ``fused_tail = False`` switch leaves the flagship on the one-kernel tail's rule."""
    import hicgat
    assert getattr(hicgat.GATNetSelectiveResidualsUpdated(), "fused_tail", True) is True
    assert all(cls.fused_tail is False for cls in hicgat.LN_MODELS.values())

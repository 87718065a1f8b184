"""Host side of BatchNorm1d on the HIP path: the two BatchNorm models on the public surface, their
structure against a module built with the reference's constructor lines (models.py:270-281, :834-845),
the library's entry points, and the argument checks that come before the library.  No GPU."""
import pytest
import torch
from torch.nn import BatchNorm1d, Dropout, Linear

NAMES = ("GATNetHeadsChanged4LayersLeakyReLU", "GATNetHeadsChanged4LayersLeakyReLUHeads4")


def test_models_on_the_public_surface():
    import hicgat
    from hicgat import train
    choices = next(a.choices for a in train.make_parser()._actions if "--model" in a.option_strings)
    for name in NAMES:
        assert name in hicgat.MODELS and getattr(hicgat, name) is hicgat.MODELS[name]
        assert name in choices
        assert issubclass(hicgat.MODELS[name], hicgat.gat_models._DropoutMLP)   # train()'s rescoring rule


def ref_model(name):
    """The reference's constructor over the oracle's GATConv, submodules in its order."""
    from oracle import gat as og
    m = torch.nn.Module()
    if name == "GATNetHeadsChanged4LayersLeakyReLU":       # models.py:273-274
        m.conv = og.GATConv(512, 256, heads=2, concat=True)
        m.densea = Linear(512, 256)
    else:                                                  # models.py:837-838
        m.conv = og.GATConv(256, 256, heads=4, concat=True)
        m.densea = Linear(1024, 256)
    m.bn_a = BatchNorm1d(256)
    m.dense1 = Linear(256, 128)
    m.bn1 = BatchNorm1d(128)
    m.dense2 = Linear(128, 64)
    m.bn2 = BatchNorm1d(64)
    m.dense3 = Linear(64, 3)
    m.dropout = Dropout(p=0.4)
    return m


@pytest.mark.parametrize("name,count", [(NAMES[0], 437251), (NAMES[1], 569859)])
def test_parameter_count_children_keys_and_seeded_init(name, count):
    import hicgat
    torch.manual_seed(11)
    ref = ref_model(name)
    torch.manual_seed(11)
    mine = hicgat.MODELS[name]()
    assert sum(p.numel() for p in mine.parameters()) == count == sum(p.numel() for p in ref.parameters())
    assert [n for n, _ in mine.named_children()] == ["conv", "densea", "bn_a", "dense1", "bn1", "dense2", "bn2",
                                                     "dense3", "dropout"]
    assert [n for n, _ in ref.named_children()] == [n for n, _ in mine.named_children()]
    sr, sm = ref.state_dict(), mine.state_dict()
    assert list(sr) == list(sm)
    for bn in ("bn_a", "bn1", "bn2"):
        assert [k for k in sm if k.startswith(bn + ".")] == [f"{bn}.{s}" for s in (
            "weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
        assert type(getattr(mine, bn)) is BatchNorm1d
    for k in sr:
        assert torch.equal(sr[k], sm[k]), k
    assert mine.dropout.p == 0.4 and mine.training and mine.drop_sites == 2
    assert [getattr(mine, n) for n in mine.linears] == [c for c in mine.children() if isinstance(c, Linear)]
    assert [getattr(mine, n) for n in mine.norms] == [c for c in mine.children() if isinstance(c, BatchNorm1d)]


def test_cpu_state_dict_carries_the_buffers():
    import hicgat
    from hicgat.train import cpu_state_dict
    mine = hicgat.MODELS[NAMES[0]]()
    mine.bn1.running_mean.fill_(0.25)
    mine.bn1.num_batches_tracked.fill_(7)
    sd = cpu_state_dict(mine)
    assert sd["bn1.running_mean"].eq(0.25).all() and sd["bn1.num_batches_tracked"].item() == 7
    assert sd["bn1.num_batches_tracked"].dtype == torch.int64
    ref_model(NAMES[0]).load_state_dict(sd, strict=True)


def test_library_exports_the_batchnorm_entry_points():
    from hicgat import _lib
    lib = _lib.load()
    for s in ("hicgat_bn_workspace_bytes", "hicgat_bn_stats", "hicgat_bn_act_dropout_fwd",
              "hicgat_bn_act_dropout_bwd"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s
    assert lib.hicgat_bn_workspace_bytes(20000, 64) > 0
    assert lib.hicgat_bn_workspace_bytes(20000, 96) == 0 and lib.hicgat_bn_workspace_bytes(0, 64) == 0


def test_refusals_come_before_the_library(monkeypatch):
    import hicgat

    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(hicgat._lib, "load", no_library)
    monkeypatch.setattr(hicgat._lib, "lib", no_library)
    monkeypatch.setattr(hicgat.kernels, "default", no_library)
    f = hicgat.ops.bn_act_dropout
    y = torch.zeros(4, 64)
    with pytest.raises(NotImplementedError, match="affine=False"):
        f(y, BatchNorm1d(64, affine=False), "relu")
    with pytest.raises(NotImplementedError, match="track_running_stats=False"):
        f(y, BatchNorm1d(64, track_running_stats=False), "relu")
    with pytest.raises(NotImplementedError, match="momentum=None"):
        f(y, BatchNorm1d(64, momentum=None), "relu")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        f(y[:1], BatchNorm1d(64), "relu")
    with pytest.raises(hicgat._lib.HicgatUnavailable):           # eval mode takes one row; CPU tensors do not run
        f(y[:1], BatchNorm1d(64).eval(), "relu")
    with pytest.raises(hicgat._lib.HicgatUnavailable):
        f(y, BatchNorm1d(64), "leaky_relu")
    with pytest.raises(ValueError, match="act must be"):
        f(y, BatchNorm1d(64), "gelu")
    with pytest.raises(ValueError, match=r"float32 \[rows, 64\]"):
        f(torch.zeros(4, 128), BatchNorm1d(64), "relu")
    with pytest.raises(NotImplementedError, match="widths"):
        f(torch.zeros(4, 96), BatchNorm1d(96), "relu")
    with pytest.raises(TypeError, match="BatchNorm1d"):
        f(y, torch.nn.LayerNorm(64), "relu")


def test_sharded_trainer_refuses_both_models_before_any_collective():
    """Named for batch normalisation -- also the Heads4 model, whose conv shape the trainer would refuse
    next -- and before it looks at a process group (none exists here)."""
    import hicgat
    for name in NAMES:
        with pytest.raises(NotImplementedError, match="batch normalisation"):
            hicgat.dist.ShardedTrainer(hicgat.MODELS[name](), torch.zeros(8, 512), None, None)

"""Host side of the GATConv head / channel shapes: the supported-shape rule, the two zoo models that
use other shapes than the flagship's (2, 256) -- ``GATNetHeadsChangedLeakyReLU`` (models.py:181-222)
and ``GATNetReduced`` (models.py:1414-1459) -- on the public surface, and the sharded trainer's
refusal of a model it cannot run.  No GPU."""
import os
import socket

import pytest
import torch
from torch.nn import Dropout, LeakyReLU, Linear

# (in, out, heads) of every GATConv the reference's models.py instantiates
ZOO = [(512, 512, 1), (512, 256, 1), (512, 128, 2), (256, 128, 2), (128, 128, 2), (256, 256, 2), (512, 256, 2),
       (512, 512, 2), (256, 256, 4)]


def test_gat_shape_supported_rule():
    from hicgat import ops
    for _, c, h in ZOO:
        assert ops.gat_shape_supported(h, c), (h, c)
    for h, c in [(4, 128), (1, 1024), (2, 384), (3, 256), (1, 768)]:      # in the rule, not in the zoo
        assert ops.gat_shape_supported(h, c), (h, c)
    for h, c in [(2, 96), (8, 128), (3, 512), (1, 128), (3, 128), (4, 512), (2, 640), (0, 256), (1, 2048)]:
        assert not ops.gat_shape_supported(h, c), (h, c)


def test_models_on_the_public_surface():
    import hicgat
    from hicgat import train
    names = ("GATNetHeadsChangedLeakyReLU", "GATNetReduced")
    choices = next(a.choices for a in train.make_parser()._actions if "--model" in a.option_strings)
    for name in names:
        assert name in hicgat.MODELS and getattr(hicgat, name) is hicgat.MODELS[name]
        assert name in choices


class _RefHeadsChangedLeakyReLU(torch.nn.Module):
    """models.py:181-222 over the oracle's GATConv, submodules in the reference's order."""

    def __init__(self):
        from oracle import gat as og
        super().__init__()
        self.conv = og.GATConv(512, 128, heads=2, concat=True)
        self.densea = Linear(256, 128)
        self.dense1 = Linear(128, 64)
        self.dense2 = Linear(64, 32)
        self.dense3 = Linear(32, 3)
        self.leaky_relu = LeakyReLU()


class _RefReduced(torch.nn.Module):
    """models.py:1414-1459 over the oracle's GATConv."""

    def __init__(self):
        from oracle import gat as og
        super().__init__()
        self.conv = og.GATConv(512, 512, heads=2, concat=True)
        self.densea = Linear(1024, 256)
        self.dense1 = Linear(256, 64)
        self.dense2 = Linear(64, 3)
        self.dropout = Dropout(p=0.4)


@pytest.mark.parametrize("name,ref_cls,count", [("GATNetHeadsChangedLeakyReLU", _RefHeadsChangedLeakyReLU, 175171),
                                                ("GATNetReduced", _RefReduced, 806403)])
def test_parameter_count_keys_and_seeded_init(name, ref_cls, count):
    import hicgat
    torch.manual_seed(11)
    ref = ref_cls()
    torch.manual_seed(11)
    mine = hicgat.MODELS[name]()
    assert sum(p.numel() for p in mine.parameters()) == count
    sr, sm = ref.state_dict(), mine.state_dict()
    assert list(sr) == list(sm)
    for k in sr:
        assert torch.equal(sr[k], sm[k]), k
    assert [n for n, _ in ref.named_children()] == [n for n, _ in mine.named_children()]


def test_reduced_refuses_to_train_without_dropout():
    import hicgat
    m = hicgat.GATNetReduced()
    assert isinstance(m.dropout, Dropout) and m.dropout.p == 0.4
    m.train()
    x = torch.zeros(4, 512)
    with pytest.raises(NotImplementedError, match="[Dd]ropout"):
        m.loss(x, None, None)
    with pytest.raises(NotImplementedError, match="[Dd]ropout"):
        m(x, None)
    assert hicgat.GATNetReduced().eval().training is False


def test_gat_conv_refuses_an_unsupported_shape_before_the_library():
    """The rule is checked first: no library, no device and no graph are touched."""
    import hicgat
    conv = hicgat.GATConv(512, 96, heads=2)
    with pytest.raises(NotImplementedError, match="out_channels % 128"):
        conv(torch.zeros(4, 512), None)


def test_sharded_trainer_refuses_another_conv_before_any_collective():
    """gloo, world 1: a model whose conv is not GATConv(512, 256, heads=2) is refused at
    construction, with the group still untouched (no collective has run: the refusal comes before
    the trainer looks at the group at all)."""
    import torch.distributed as dist

    import hicgat
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        model = hicgat.GATNetHeadsChangedLeakyReLU()
        with pytest.raises(NotImplementedError, match=r"GATConv\(512, 256, heads=2\)"):
            hicgat.dist.ShardedTrainer(model, torch.zeros(8, 512), None, None)
        with pytest.raises(NotImplementedError, match=r"GATConv\(512, 256, heads=2\)"):
            hicgat.dist.ShardedTrainer(hicgat.Net(), torch.zeros(8, 512), None, None)
    finally:
        dist.destroy_process_group()

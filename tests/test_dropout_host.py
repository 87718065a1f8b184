"""Host side of feature dropout: the mask's definition (tests/philox_ref.py) against the published
Philox4x32-10 known answers and its statistics, and the public surface -- the four models that train
with dropout, the library's entry points, and the argument checks that come before the library.
No GPU."""
import math

import numpy as np
import pytest
import torch
from torch.nn import Dropout, Linear

import philox_ref

NAMES = ("GATNet", "GATNetHeadsChanged3LayersLeakyReLU", "GATNetHeadsChanged4LayerEmbedding512Dense",
         "GATNetMoreReduced")


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, out):
    words = philox_ref.philox4x32_10([np.uint64(c) for c in ctr], key)
    assert " ".join(f"{int(w):08x}" for w in words) == out


def test_threshold_and_scale():
    assert philox_ref.threshold(0.0) == 0 and philox_ref.threshold(0.5) == 1 << 31
    assert philox_ref.threshold(math.nextafter(1.0, 0.0)) == (1 << 32) - 1
    assert philox_ref.keep_mask(8, 16, 0.0, 3, 1, 0).all()
    assert philox_ref.scale(0.0) == 1.0 and philox_ref.scale(0.5) == 2.0


# ---------------------------------------------------------------- the definition's statistics
ROWS, WIDTH, SEED = 4096, 256, 0x1234


def _sigmas(mask, q, axis=None):
    """|keep rate - q| in standard deviations of a mean of Bernoulli(q) draws, per ``axis`` slice."""
    n = mask.size if axis is None else mask.shape[axis]
    return np.abs(mask.mean(axis=axis) - q) / math.sqrt(q * (1 - q) / n)


@pytest.mark.parametrize("p", [0.4, 0.3, 0.1])
@pytest.mark.parametrize("step", [1, 2])
def test_keep_rates(p, step):
    q = 1.0 - philox_ref.threshold(p) / 2.0 ** 32
    m = philox_ref.keep_mask(ROWS, WIDTH, p, SEED, step, 0)
    overall, col, row = _sigmas(m, q), _sigmas(m, q, axis=0).max(), _sigmas(m, q, axis=1).max()
    print(f"p={p} step={step}: overall {overall:.2f} sigma, worst column {col:.2f}, worst row {row:.2f}")
    assert overall < 4 and col < 5 and row < 6


def _corr_sqrt_n(a, b):
    a, b = a.ravel().astype(np.float64), b.ravel().astype(np.float64)
    return abs(np.corrcoef(a, b)[0, 1]) * math.sqrt(a.size)


def test_masks_are_uncorrelated_across_step_site_seed_and_shifts():
    m = philox_ref.keep_mask(ROWS, WIDTH, 0.4, SEED, 1, 0)
    others = {"step 2": philox_ref.keep_mask(ROWS, WIDTH, 0.4, SEED, 2, 0),
              "site 1": philox_ref.keep_mask(ROWS, WIDTH, 0.4, SEED, 1, 1),
              "seed + 1": philox_ref.keep_mask(ROWS, WIDTH, 0.4, SEED + 1, 1, 0)}
    for what, o in others.items():
        c = _corr_sqrt_n(m, o)
        print(f"{what}: |corr| sqrt(n) = {c:.2f}")
        assert c < 4, what
    for what, (a, b) in {"one column": (m[:, 1:], m[:, :-1]), "one row": (m[1:], m[:-1])}.items():
        c = _corr_sqrt_n(a, b)
        print(f"shift by {what}: |corr| sqrt(n) = {c:.2f}")
        assert c < 4, what


def test_row_offset_is_a_row_range_of_the_whole_mask():
    whole = philox_ref.keep_mask(130, 256, 0.3, 9, 1, 0)
    assert np.array_equal(whole[40:], philox_ref.keep_mask(90, 256, 0.3, 9, 1, 0, row_offset=40))
    assert np.array_equal(philox_ref.keep_mask(5, 64, 0.3, 9, 1, 0), philox_ref.keep_mask(5, 64, 0.3, 9, 2 ** 32 + 1, 0))


# ---------------------------------------------------------------- the public surface
def test_models_on_the_public_surface():
    import hicgat
    from hicgat import train
    choices = next(a.choices for a in train.make_parser()._actions if "--model" in a.option_strings)
    for name in NAMES:
        assert name in hicgat.MODELS and getattr(hicgat, name) is hicgat.MODELS[name]
        assert name in choices
    assert hicgat.DropoutState is hicgat.dropout.DropoutState


def _ref_model(name):
    """The reference's constructor (models.py) over the oracle's GATConv, submodules in its order."""
    from oracle import gat as og
    m = torch.nn.Module()
    if name == "GATNet":                                            # models.py:60-70
        m.conv = og.GATConv(512, 512)
        widths, p = (512, 256, 128, 64, 3), 0.3
    elif name == "GATNetHeadsChanged3LayersLeakyReLU":              # models.py:971-979
        m.conv = og.GATConv(512, 256, heads=2, concat=True)
        widths, p = (512, 256, 128, 3), 0.3
    elif name == "GATNetHeadsChanged4LayerEmbedding512Dense":       # models.py:1365-1375
        m.conv = og.GATConv(512, 256, heads=2, concat=True)
        widths, p = (512, 256, 128, 64, 32, 3), 0.3
    else:                                                           # GATNetMoreReduced, models.py:1461-1468
        m.conv = og.GATConv(512, 256, heads=2, concat=True)
        widths, p = (512, 128, 32, 3), 0.4
    for k, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        setattr(m, "densea" if k == 0 else f"dense{k}", Linear(a, b))
    m.dropout = Dropout(p=p)
    return m


@pytest.mark.parametrize("name,count", [("GATNet", 436355), ("GATNetHeadsChanged3LayersLeakyReLU", 428291),
                                        ("GATNetHeadsChanged4LayerEmbedding512Dense", 438339),
                                        ("GATNetMoreReduced", 333571)])
def test_parameter_count_keys_and_seeded_init(name, count):
    import hicgat
    torch.manual_seed(11)
    ref = _ref_model(name)
    torch.manual_seed(11)
    mine = hicgat.MODELS[name]()
    assert sum(p.numel() for p in mine.parameters()) == count
    sr, sm = ref.state_dict(), mine.state_dict()
    assert list(sr) == list(sm)
    for k in sr:
        assert torch.equal(sr[k], sm[k]), k
    assert [n for n, _ in ref.named_children()] == [n for n, _ in mine.named_children()]
    assert mine.dropout.p == ref.dropout.p and mine.training
    assert [getattr(mine, n) for n in mine.linears] == [c for c in mine.children() if isinstance(c, Linear)]


def test_library_exports_the_dropout_entry_points():
    from hicgat import _lib
    lib = _lib.load()
    for s in ("hicgat_act_dropout_fwd", "hicgat_act_dropout_bwd", "hicgat_dropout_mask", "hicgat_dropout_advance"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES, s


def test_bad_p_and_cpu_tensors_are_refused_before_the_library(monkeypatch):
    import hicgat

    def no_library(*a, **k):
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(hicgat._lib, "load", no_library)
    monkeypatch.setattr(hicgat._lib, "lib", no_library)
    monkeypatch.setattr(hicgat.kernels, "default", no_library)
    x = torch.zeros(4, 8)
    for p in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="0 <= p < 1"):
            hicgat.DropoutState("cuda", p=p)
        with pytest.raises(ValueError, match="0 <= p < 1"):
            hicgat.ops.act_dropout(x, "relu", p, None, 0)
        with pytest.raises(ValueError, match="0 <= p < 1"):
            hicgat.ops.dropout_mask(4, 8, p, 1, 1, 0)
    with pytest.raises(hicgat._lib.HicgatUnavailable):
        hicgat.DropoutState("cpu")
    with pytest.raises(hicgat._lib.HicgatUnavailable):
        hicgat.ops.act_dropout(x, "relu", 0.3, None, 0)
    with pytest.raises(hicgat._lib.HicgatUnavailable):
        hicgat.ops.dropout_mask(4, 8, 0.3, 1, 1, 0, device="cpu")
    with pytest.raises(ValueError, match="act must be"):
        hicgat.ops.act_dropout(x, "gelu", 0.3, None, 0)


def test_sharded_trainer_refuses_a_dropout_model_before_any_collective():
    """The three new models with the flagship's conv shape pass the trainer's conv check; it refuses
    them for their dropout, before it looks at the process group (none exists here)."""
    import hicgat
    for name in NAMES:
        with pytest.raises(NotImplementedError, match="GATConv|dropout"):
            hicgat.dist.ShardedTrainer(hicgat.MODELS[name](), torch.zeros(8, 512), None, None)
    with pytest.raises(NotImplementedError, match="feature dropout"):
        hicgat.dist.ShardedTrainer(hicgat.GATNetMoreReduced(), torch.zeros(8, 512), None, None)

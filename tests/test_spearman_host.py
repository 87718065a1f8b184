"""CPU: the host side of the fused dSCC path -- CLI flags, loss names, the no-device error and the
M < 2^31 arithmetic (no kernel runs)."""
import pytest
import torch


def test_parser_accepts_mse_plus_dscc():
    from hicgat import train
    a = train.make_parser().parse_args(["m.txt", "f.txt", "--loss", "mse+dscc", "--alpha", "0.5"])
    assert a.loss == "mse+dscc" and a.alpha == 0.5
    assert train.make_parser().parse_args(["m.txt", "f.txt"]).alpha == 1.0
    with pytest.raises(SystemExit):
        train.make_parser().parse_args(["m.txt", "f.txt", "--loss", "mse+drmsd"])


def test_train_rejects_unknown_loss():
    from hicgat import train
    assert "mse+dscc" in train.LOSSES
    with pytest.raises(KeyError):
        train.train(None, None, None, loss="mse+drmsd")


def test_scorer_without_device_is_unavailable(monkeypatch):
    from hicgat import _lib, metrics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.HicgatUnavailable):
        metrics.DsccScorer(torch.zeros(4, 4))
    with pytest.raises(_lib.HicgatUnavailable):
        metrics.spearman_fused(torch.zeros(4), torch.ones(4))


def test_pair_limit():
    """Doubled ranks and pair indices are uint32: M = N (N - 1) / 2 < 2^31, so N <= 65536."""
    from hicgat import _lib, metrics
    lib = _lib.load()
    assert metrics.dscc_pairs(65536) == 65536 * 65535 // 2 < 2 ** 31
    assert lib.hicgat_rank_workspace_bytes(metrics.dscc_pairs(65536)) > 0
    with pytest.raises(ValueError):
        metrics.dscc_pairs(65537)
    with pytest.raises(ValueError):
        metrics.dscc_pairs(1)
    assert lib.hicgat_rank_workspace_bytes(65537 * 65536 // 2) == 0
    assert lib.hicgat_rank_workspace_bytes(2 ** 31) == 0 and lib.hicgat_rank_workspace_bytes(0) == 0
    assert lib.hicgat_rank_workspace_bytes(2 ** 31 - 1) > 16 * (2 ** 31 - 1)
    assert lib.hicgat_rank_tile() % 256 == 0

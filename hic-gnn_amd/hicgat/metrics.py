"""Evaluation of a structure (a11): dSCC = Spearman of the triu true vs predicted distances.

Reference: HiC-GNN_main.py:135-139 (``spearmanr(dist_truth, cdist(coords)[triu])``) and
HiC_GAT_generalize_directly.py:242.  Ranks use scipy's tie rule (average rank of a tie group), so
the value equals scipy.stats.spearmanr on the same float32 distances; computed on the GPU.
"""
import torch

from . import _lib, ops

MAX_PAIRS = 2 ** 31   # doubled ranks and pair indices are uint32 on the device: M < 2^31


def _avg_rank(v):
    """Average ranks (1-based) with ties sharing their mean rank, in float64."""
    order = torch.argsort(v, stable=True)
    sv = v[order]
    n = v.numel()
    new_grp = torch.ones(n, dtype=torch.bool, device=v.device)
    new_grp[1:] = sv[1:] != sv[:-1]
    gid = torch.cumsum(new_grp.long(), 0) - 1
    pos = torch.arange(1, n + 1, dtype=torch.float64, device=v.device)
    ngrp = int(gid[-1].item()) + 1
    s = torch.zeros(ngrp, dtype=torch.float64, device=v.device).index_add_(0, gid, pos)
    c = torch.zeros(ngrp, dtype=torch.float64, device=v.device).index_add_(0, gid, torch.ones_like(pos))
    r = torch.empty(n, dtype=torch.float64, device=v.device)
    r[order] = (s / c)[gid]
    return r


def pearson(a, b):
    a = a.double() - a.double().mean()
    b = b.double() - b.double().mean()
    return float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum()))


def spearman(a, b):
    return pearson(_avg_rank(a), _avg_rank(b))


def triu_pairs(mat):
    n = mat.shape[0]
    idx = torch.triu_indices(n, n, offset=1, device=mat.device)
    return mat[idx[0], idx[1]]


def dscc(coords, truth):
    """HiC-GNN_main.py:135-139 on the GPU. ``truth`` is the [N, N] target (any float dtype)."""
    with torch.no_grad():
        d = ops.pairwise_dist(coords.detach())
        return spearman(triu_pairs(truth), triu_pairs(d))


# ---- the fused device path (spearman.hip): no host sync, no allocation, no N x N matrix ----------

def dscc_pairs(n):
    """M = n (n - 1) / 2, the pairs dSCC ranks; ``ValueError`` beyond the device path's M < 2^31
    (the largest n is 65536)."""
    m = int(n) * (int(n) - 1) // 2
    if n < 2 or m >= MAX_PAIRS:
        raise ValueError(f"dSCC over {n} nodes: the pair count {m} must be in [1, 2^31)")
    return m


class _RankedSide:
    """One side of a Spearman correlation, prepared once: doubled average ranks and their stats."""

    def __init__(self, v, m, ws=None):
        lib = _lib.lib()
        dev = v.device
        self.m = m
        self.rank2 = torch.empty(m, dtype=torch.int32, device=dev)        # uint32 on the device
        self.side_stats = torch.empty(4, dtype=torch.float64, device=dev)
        self.ws = ws if ws is not None else _lib.workspace(lib.hicgat_rank_workspace_bytes(m), dev)
        _lib.check(lib.hicgat_avg_rank2(_lib.ptr(v), m, _lib.ptr(self.rank2), _lib.ptr(self.side_stats),
                                        _lib.ptr(self.ws), self.ws.numel(), _lib.stream(dev)), "hicgat_avg_rank2")


def _f32_vector(v):
    v = v.detach().reshape(-1)
    return v if v.dtype == torch.float32 and v.is_contiguous() else v.float().contiguous()


def spearman_fused(a, b):
    """``scipy.stats.spearmanr(a, b)`` of two device vectors (ranked as float32) by the fused path."""
    lib = _lib.lib()
    a, b = _f32_vector(a), _f32_vector(b)
    if a.numel() != b.numel() or a.numel() < 1:
        raise ValueError("spearman_fused: two vectors of the same, non-zero length")
    m = a.numel()
    if m >= MAX_PAIRS:
        raise ValueError(f"spearman_fused: {m} elements, the device path ranks fewer than 2^31")
    side = _RankedSide(a, m)
    out = torch.empty(4, dtype=torch.float64, device=a.device)
    _lib.check(lib.hicgat_spearman_vs_rank2(_lib.ptr(b), _lib.ptr(side.rank2), _lib.ptr(side.side_stats), m,
                                            _lib.ptr(out), _lib.ptr(side.ws), side.ws.numel(),
                                            _lib.stream(a.device)), "hicgat_spearman_vs_rank2")
    return float(out[0].item())


class DsccScorer:
    """dSCC of coordinates against one target, every step (HiC_GAT_generalize_directly.py:242,
    combined_loss_training.py:130-135).

    ``truth_matrix``: what ``Truth.scoring()`` returns ([N, N], may be a strided view).  Its upper
    triangle is ranked once; ``score_into`` then runs the per-step form -- pair distances with
    ``ops.pairwise_dist``'s expression straight into sort keys, four radix passes, one tie-aware
    reduction -- with no host sync and no allocation, so it can sit in a captured step."""

    def __init__(self, truth_matrix):
        lib = _lib.lib()
        t = truth_matrix.detach()
        if t.dim() != 2 or t.shape[0] != t.shape[1]:
            raise ValueError("DsccScorer: a square [N, N] target")
        if t.dtype != torch.float32 or t.stride(1) != 1:
            t = t.float().contiguous()
        self.n = t.shape[0]
        self.m = dscc_pairs(self.n)
        dev = t.device
        v = torch.empty(self.m, dtype=torch.float32, device=dev)
        _lib.check(lib.hicgat_triu_gather(_lib.ptr(t), self.n, t.stride(0), _lib.ptr(v), _lib.stream(dev)),
                   "hicgat_triu_gather")
        side = _RankedSide(v, self.m)
        self.rank2, self.side_stats, self.ws = side.rank2, side.side_stats, side.ws
        self.out = torch.empty(4, dtype=torch.float64, device=dev)
        self._lib = lib

    def score_into(self, coords, out=None):
        """(rho, sum b^2, tie groups, NaN flag) as a 4-element fp64 device tensor (``out`` or the
        scorer's own); ``coords`` is the contiguous fp32 [N, 3] of a forward."""
        c = coords.detach()
        if c.shape != (self.n, 3) or c.dtype != torch.float32 or not c.is_contiguous():
            raise ValueError(f"DsccScorer: contiguous float32 coordinates [{self.n}, 3]")
        out = self.out if out is None else out
        if out.dtype != torch.float64 or out.numel() < 4 or not out.is_contiguous():
            raise ValueError("DsccScorer: out is a contiguous float64 tensor of 4 elements")
        _lib.check(self._lib.hicgat_dscc_coords(_lib.ptr(c), self.n, _lib.ptr(self.rank2), _lib.ptr(self.side_stats),
                                                _lib.ptr(out), _lib.ptr(self.ws), self.ws.numel(),
                                                _lib.stream(c.device)), "hicgat_dscc_coords")
        return out

    def score(self, coords):
        return float(self.score_into(coords)[0].item())

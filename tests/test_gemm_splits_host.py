"""CPU: the GEMM family's K-split and tile policy lives in the library (csrc/gemm.hip ``tile_for`` and
the host-only queries of include/hicgat.h) and returns what the Python formulas returned before they
moved there.

The three ``_frozen_*`` functions are copies of those formulas with every constant a literal.  A
change to a C constant that moves a split count fails here: moving the policy has to be meant, and
then this file changes with it.
"""
import itertools
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hic-gnn_amd")

MS = (1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2500, 2700, 4032, 4033, 7520, 7521, 20000, 30560, 30561)
NS = (3, 64, 127, 128, 129, 256, 512, 1024)
KS = (3, 64, 127, 128, 255, 256, 257, 512, 20000)
TARGETS = (1, 256, 512)
GRID = list(itertools.product(MS, NS, KS))


def _frozen_row_splits(M, N, K):
    if M < 1024 or K < 256:
        return 1
    if -(-M // 160) * (N // 128) >= 192:
        return 1
    wgs = -(-M // 64) * -(-N // (128 if N >= 128 else 64))
    if wgs >= 256:
        return 1
    return max(1, min(K // 128, -(-512 // wgs)))


def _frozen_wgrad_splits(m, n, k, target):
    bm = 128 if (m >= 128 and n >= 128) else 64
    tiles = -(-m // bm) * -(-n // bm)
    return max(1, min(k // 256, target // tiles))


def _frozen_grouped_splits(shapes, target):
    wgs = sum(-(-M // 64) * -(-N // 128) for M, N, _ in shapes)
    return max(1, min(shapes[0][2] // 128, -(-target // max(1, wgs)))) if target else 1


@pytest.fixture(scope="module")
def lib():
    from hicgat import _lib
    return _lib.load()


def test_row_splits_match_the_frozen_formula(lib):
    for M, N, K in GRID:
        assert lib.hicgat_gemm_row_splits(M, N, K) == _frozen_row_splits(M, N, K), (M, N, K)


def test_row_splits_cross_the_cut_offs_where_the_grid_says(lib):
    """The grid's M values sit on the rule's edges: the frozen formula itself moves there."""
    assert (lib.hicgat_gemm_row_splits(4032, 512, 512), lib.hicgat_gemm_row_splits(4033, 512, 512)) == (3, 1)
    for m_lo, n in ((7520, 512), (30560, 128)):      # 188 / 191 tall tiles -> 192
        assert -(-m_lo // 160) * (n // 128) < 192 <= -(-(m_lo + 1) // 160) * (n // 128)
        assert lib.hicgat_gemm_row_splits(m_lo + 1, n, 512) == 1


def test_python_row_splits_is_the_library(lib):
    from hicgat import kernels as hk
    for M, N, K in GRID:
        assert hk.row_splits(M, N, K) == (lib.hicgat_gemm_row_splits(M, N, K) if hk.ROW_SPLIT else 1)


def test_wgrad_splits_match_the_frozen_formula(lib):
    for (M, N, K), t in itertools.product(GRID, TARGETS):
        assert lib.hicgat_gemm_wgrad_splits(M, N, K, t) == _frozen_wgrad_splits(M, N, K, t), (M, N, K, t)


def test_python_wgrad_splits_is_the_library(lib):
    from hicgat import ops
    for M, N, K in GRID:
        assert ops._splits(M, N, K) == lib.hicgat_gemm_wgrad_splits(M, N, K, ops._DW_BLOCKS)
        assert ops._splits(M, N, K, 512) == lib.hicgat_gemm_wgrad_splits(M, N, K, 512)


def _job_lists():
    rng = random.Random(0)
    lists = [[s] for s in GRID]                       # every single job
    for n in (2, 8):
        lists += [[rng.choice(GRID) for _ in range(n)] for _ in range(200)]
    # the smallest and the largest workgroup counts of each length, and K bounds set by the first job
    for n in (1, 2, 8):
        lists += [[(1, 3, 20000)] * n, [(30561, 1024, 20000)] * n, [(64, 128, 3)] + [(2700, 512, 20000)] * (n - 1),
                  [(2700, 512, 20000)] + [(64, 128, 3)] * (n - 1)]
    return lists


def test_grouped_splits_match_the_frozen_formula(lib):
    from hicgat import _lib
    for shapes in _job_lists():
        G = (_lib.GemmJob * len(shapes))()
        for k, (M, N, K) in enumerate(shapes):
            G[k].M, G[k].N, G[k].K = M, N, K          # the query reads the shapes only
        for t in (0,) + TARGETS:
            assert lib.hicgat_gemm_rows_grouped_splits(G, len(shapes), t) == _frozen_grouped_splits(shapes, t), \
                (shapes, t)
    assert lib.hicgat_gemm_rows_grouped_splits(None, 0, 512) == 1


def test_tail_bwd_partial_rows(lib):
    for M in (0, 1, 15, 16, 17, 2700, 20000):
        assert lib.hicgat_tail_bwd_partial_rows(M) == -(-M // 16), M
        if M:       # the workspace holds exactly these rows of [dgamma | dbeta]
            assert lib.hicgat_tail_bwd_workspace_bytes(M, 64) == lib.hicgat_tail_bwd_partial_rows(M) * 2 * 64 * 4


def _read(*parts):
    with open(os.path.join(*parts)) as fh:
        return fh.read()


def test_tile_rule_is_written_once():
    """gemm.hip states the 128 x 128 condition once (``tile_for``); the package's Python restates no
    tile arithmetic."""
    assert _read(PKG, "csrc", "gemm.hip").count("M >= 128 && N >= 128 && M <= 1024") == 1
    pkg = os.path.join(PKG, "hicgat")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py"):
            text = _read(pkg, name)
            for needle in ("_TALL_MIN_TILES", "// 160", "// 64) * -(-"):
                assert needle not in text, (name, needle)

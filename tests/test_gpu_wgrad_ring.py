"""GPU: the LDS-DMA ring weight-gradient kernel (csrc/gemm_wgrad.hip) against the register-staged
gemm_kernel<128, 128, true, true, ...> it replaces for K-split weight gradients of whole 128 x 128
tiles.  Both run the same MFMAs on the same k in the same order, so dW must be equal bit for bit:
``impl=GEMM_AUTO`` routes to the ring kernel, ``impl=GEMM_F32`` keeps the old one (include/hicgat.h).

K values: 1 and 15 (one ragged stage), 16 (one full stage), 17 (a second stage of one row), 47 / 48 /
49 (three stages = the ring's slots, ragged / full / one more), 1250 (the flagship's rows per split);
with splits 2, 3 and 16 the small K leave splits with fewer stages than the ring has slots and
trailing splits with no rows at all (kchunk is rounded up to 16).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KS = (1, 15, 16, 17, 47, 48, 49, 1250)
SPLITS = (2, 3, 16)
KMAX = max(KS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hicgat  # noqa: F401  (fails loudly if libhicgat.so is missing)


def _rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-30))


def _both(K, dy, x, splits, **kw):
    """dW by the ring kernel and by the old kernel, outputs NaN-filled before each call."""
    from hicgat import kernels as hk
    k, m = dy.shape
    n = x.shape[1]
    out = []
    for impl in (hk.GEMM_AUTO, hk.GEMM_F32):
        dw = torch.full((m, n), float("nan"), device=DEV)
        out.append(K.gemm(1, 1, m, n, k, dy, x, dw, splits=splits, impl=impl, **kw))
    return out


@pytest.fixture(scope="module")
def operands():
    """[KMAX, 512] operands, random fp32 and exact small integers; the cases take leading slices."""
    g = torch.Generator(device="cpu").manual_seed(20)
    rnd = (torch.randn(KMAX, 512, generator=g), torch.randn(KMAX, 512, generator=g))
    ints = (torch.randint(-4, 5, (KMAX, 512), generator=g).float(), torch.randint(-4, 5, (KMAX, 512), generator=g).float())
    return {"random": tuple(t.to(DEV) for t in rnd), "integers": tuple(t.to(DEV) for t in ints)}


@pytest.mark.parametrize("kind", ["random", "integers"])
@pytest.mark.parametrize("m,n", [(128, 128), (256, 128), (512, 512)])
def test_ring_bit_equal_to_old_kernel(operands, m, n, kind):
    import hicgat
    K = hicgat.kernels.default()
    dy_all, x_all = operands[kind]
    for k in KS:
        dy, x = dy_all[:k, :m], x_all[:k, :n]          # ld 512: lda > M and ldb > N for the smaller tiles
        exact = (dy.double().t() @ x.double()).float() if kind == "integers" else None
        for splits in SPLITS:
            new, old = _both(K, dy, x, splits)
            assert torch.isfinite(new).all(), (k, splits)
            assert torch.equal(new, old), (k, splits, float((new - old).abs().max()))
            if exact is not None:      # |sums| <= 16 * 1250 < 2^24: every partial is exact in fp32
                assert torch.equal(new, exact), (k, splits)


def test_ring_strided_operands_bias_accumulate():
    """lda / ldb larger than M / N with a column offset, and the slab sum's bias and accumulate forms."""
    import hicgat
    K = hicgat.kernels.default()
    torch.manual_seed(3)
    m, n, k = 256, 384, 333
    dy = torch.randn(k, m + 8, device=DEV)[:, 4:4 + m]
    x = torch.randn(k, n + 12, device=DEV)[:, 8:8 + n]
    for splits in (2, 5):
        new, old = _both(K, dy, x, splits)
        assert torch.equal(new, old), splits
        assert _rel(new.cpu(), (dy.double().t() @ x.double()).cpu()) < 5e-6
    from hicgat import kernels as hk
    bias = torch.randn(n, device=DEV)
    c0 = torch.randn(m, n, device=DEV)
    got = [K.gemm(1, 1, m, n, k, dy, x, c0.clone(), bias=bias, accumulate=True, splits=4, impl=impl)
           for impl in (hk.GEMM_AUTO, hk.GEMM_F32)]
    assert torch.equal(got[0], got[1])
    assert _rel(got[0].cpu(), (dy.double().t() @ x.double() + bias.double() + c0.double()).cpu()) < 5e-6


def test_ring_flagship_tile_matches_fp64(operands):
    """(512, 512), K = 1250 in 16 splits against fp64, at the tolerance tests/test_gpu_parity.py holds the
    old kernel to (test_wgrad_ragged_strided: 5e-6 * max(1, sqrt(K / splits / 512)) = 5e-6 here)."""
    import hicgat
    K = hicgat.kernels.default()
    dy, x = operands["random"]
    k, splits = 1250, 16
    new, _ = _both(K, dy[:k], x[:k], splits)
    tol = 5e-6 * max(1.0, (k / splits / 512) ** 0.5)
    assert _rel(new.cpu(), (dy[:k].double().t() @ x[:k].double()).cpu()) < tol


def test_ragged_m_keeps_old_kernel_and_is_correct():
    """M = 130 is no whole number of 128-row tiles: the dispatch keeps gemm_kernel (whose tiles bound-check)
    for either impl, and the result is right."""
    import hicgat
    K = hicgat.kernels.default()
    torch.manual_seed(130)
    m, n, k = 130, 256, 1250
    dy = torch.randn(k, m, device=DEV)
    x = torch.randn(k, n, device=DEV)
    for splits in (2, 16):
        new, old = _both(K, dy, x, splits)
        assert torch.equal(new, old), splits
        tol = 5e-6 * max(1.0, (k / splits / 512) ** 0.5)
        assert _rel(new.cpu(), (dy.double().t() @ x.double()).cpu()) < tol

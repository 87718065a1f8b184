"""The GEMM family at its tile, stage, split and job edges: csrc/gemm.hip (gemm_kernel, wgrad_grouped_kernel,
gemm_rows_grouped_kernel + rows_reduce_kernel), csrc/gemm_tall.hip and csrc/gemm_wgrad.hip, through the C ABI
-- pointers, strides and offsets are the test's to choose -- against the float64 restatements of
tests/gemm_ref.py (tied to torch float64 on the CPU by tests/test_gemm_ref_host.py, which also holds every
case below to the form it names and the set of cases to every form gemm.hip can launch).

Every output lives in a ``Buf`` (tests/guarded.py) whose guard elements and row padding (ldc > N) hold a
finite non-zero sentinel and must keep their bits; an output that is not accumulated into starts as that
sentinel, so an element the kernel does not write fails its comparison.  Inputs sit in sentinel-padded
buffers too.  Every call is made twice on fresh buffers and must give the same bits.  Every hicgat_gemm /
hicgat_gemm_wgrad case first asserts, through hicgat_gemm_form with the call's real addresses, that it
reaches the form it names; the grouped weight jobs assert their staging the same way.

``integers`` inputs (integers in [-4, 4]: every partial sum exact in fp32) are compared bit for bit with
the float64 result; ``random`` inputs (standard normal) per element against the bound sum |a_k b_k| + |bias|
+ |c0| at the tolerance of gemm_ref.TOL.

Tolerances (gemm_ref.TOL; error / bound): 8 x the largest ratio of the reference's own sequential fp32
rendition over the quantity's random cases, floor 2^-22, measured on the CPU by
test_gemm_ref_host.py::test_tolerance_table; beside each the largest ratio this file measured on the MI355X
(the GEMM_RATIO lines of its first complete run):
  quantity   tolerance   measured on the MI355X
  C          3.1e-6      3.9e-7
  C_split    1.5e-6      1.7e-7
  dW         3.1e-6      3.8e-7
  db         1.3e-6      1.6e-7
  rows_C     1.7e-6      2.1e-7
(198 tests; every ``integers`` case bit-equal to float64, guards intact, repeated calls bit-equal.)
One case exposed a kernel bug, test_wgrad_grouped_mixed_launch: a weight job of hicgat_param_grads_grouped
with lddw > N is not split, but was handed the launch's common K-chunk depth, so beside split jobs (or alone
with a small target) it summed only the first chunk of its K rows (here 144 of 1000).  Fixed in gemm.hip: an
unsplit job's chunk is its whole K.  No other case failed.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gemm_ref as R
from guarded import Buf

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EUNSUPPORTED = -1, -3
f32 = np.float32
FAMILIES = ("integers", "random")
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    for k, v in sorted(WORST.items()):
        print(f"GEMM_RATIO {k} {v:.3e}")


def _L():
    from hicgat import _lib
    return _lib


def _rc(name, *args):
    L = _L()
    return getattr(L.lib(), name)(*args, L.stream())


_KEEP = []


class In:
    """A read-only rows x cols operand on the device: rows ld apart, starting ``col0`` floats into its
    row and ``off`` floats past a 16-byte boundary; everything around the data holds the sentinel."""

    def __init__(self, data, ld=None, col0=0, off=0):
        data = np.asarray(data, f32)
        rows, cols = data.shape
        self.ld = ld = cols if ld is None else ld
        assert ld >= col0 + cols
        host = np.full(4 + off + rows * ld + 8, R.SENT32, f32)
        host[4 + off:4 + off + rows * ld].reshape(rows, ld)[:, col0:col0 + cols] = data
        self.dev = torch.from_numpy(host).to(DEV)
        _KEEP.append(self.dev)
        assert self.dev.data_ptr() % 16 == 0
        self.addr = self.dev.data_ptr() + 4 * (4 + off + col0)
        self.ptr = ctypes.c_void_p(self.addr)


def _vec(a):
    t = torch.from_numpy(np.ascontiguousarray(a, f32)).to(DEV)
    _KEEP.append(t)
    return t


def _verify(family, quantity, got, ref, bound, what):
    if family == "random":
        w, k = R.worst(got, ref, bound)
        WORST[quantity] = max(WORST.get(quantity, 0.0), w)
        assert w <= R.tol(quantity), (quantity, what, w, R.tol(quantity), k)
    else:
        want = (np.asarray(ref, np.float64) + 0.0).astype(f32)
        bad = np.argwhere(np.asarray(got).view(np.uint32) != want.view(np.uint32))
        assert R.accept(family, quantity, got, ref, bound), (quantity, what, len(bad), bad[:4].tolist())


@functools.lru_cache(maxsize=4)
def _product(family, M, N, K):
    """(op(A) op(B), its bound) in float64: shared by every bias / accumulate / layout variant of a shape."""
    opA, opB = R.logical(family, M, N, K)[:2]
    return R.gemm_ref(0, 1, opA, opB)


# ------------------------------------------------------------------------------- hicgat_gemm
def _operands(c, family):
    opA, opB = R.logical(family, c.M, c.N, c.K)[:2]
    A, B = R.stored(c.a_km, c.b_km, opA, opB)
    _, _, lda, _, _, ldb = R.lds(c)
    return In(A, lda, c.a_col, c.a_off), In(B, ldb)


def _assert_form(c, a, b):
    code = _L().load().hicgat_gemm_form(c.a_km, c.b_km, c.M, c.N, c.K, a.ptr, a.ld, b.ptr, b.ld, c.splits, c.impl,
                                        0 if c.with_db is None else c.with_db)
    assert R.form_name(code) == c.form, (c.name, R.form_name(code))


def _gemm_once(c, a, b, bias, c0, ldc):
    L = _L()
    out = Buf(c.M, c.N, ld=ldc, data=c0)
    nb = L.lib().hicgat_gemm_workspace_bytes(c.M, c.N, c.splits)
    ws = L.workspace(nb, DEV) if c.splits > 1 else None
    rc = _rc("hicgat_gemm", c.a_km, c.b_km, c.M, c.N, c.K, a.ptr, a.ld, b.ptr, b.ld, None if bias is None else L.ptr(bias),
             out.ptr, ldc, int(c0 is not None), c.splits, c.impl, L.ptr(ws), nb)
    assert rc == 0, (c.name, rc)
    got, ok = out.read()
    assert ok, f"{c.name}: wrote into the guards or the padding between rows"
    return got


def _run_gemm_case(c, family, ldc_pad=3):
    """The case with bias on / off x accumulate on / off, each twice."""
    a, b = _operands(c, family)
    _assert_form(c, a, b)
    _, _, bias, c0, _ = R.logical(family, c.M, c.N, c.K)
    bias_d = _vec(bias)
    q = "C" if c.splits == 1 else "C_split"
    for use_bias in (0, 1):
        for acc in (0, 1):
            args = (c, a, b, bias_d if use_bias else None, c0 if acc else None, c.N + ldc_pad)
            got, again = _gemm_once(*args), _gemm_once(*args)
            assert R.same_bits(got, again), (c.name, "two calls differ")
            ref, bound = R.with_terms(*_product(family, c.M, c.N, c.K), bias if use_bias else None, c0 if acc else None)
            _verify(family, q, got, ref, bound, (c.name, "bias", use_bias, "accumulate", acc))
    _KEEP.clear()


_TALL = {c.name: c for c in R.tall_cases()}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", R.TALL_K)
@pytest.mark.parametrize("shape", R.TALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tall_kernel(shape, K, family):
    """gemm_tall.hip: last row tiles of 1, 159 and 160 rows, a grid of 195 (not a multiple of 8), 1 .. 5
    K stages on the 3-slot ring; both B layouts, bias and accumulate on and off, ldc > N."""
    for b in (0, 1):
        _run_gemm_case(_TALL[f"tall_{shape[0]}x{shape[1]}_k{K}_b{b}"], family, ldc_pad=4)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", [n for n in _TALL if not n.startswith("tall_1") or "lda" in n or "acol" in n])
def test_tall_strided_border_and_declines(name, family):
    """Row-strided A and A at a column offset (the tall kernel takes both); 176 tiles (one below the
    border) and every decline of the tall kernel, for values on the gemm_kernel tile each lands on."""
    _run_gemm_case(_TALL[name], family, ldc_pad=4)


_KCASES = R.kernel_cases()
_KGROUPS = sorted({(c.M, c.N, c.a_km, c.b_km) for c in _KCASES})


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,N,a,b", _KGROUPS)
def test_gemm_kernel(M, N, a, b, family):
    """gemm_kernel through hicgat_gemm: every K and split of the shape in this layout (gemm_ref.kernel_cases)."""
    for c in _KCASES:
        if (c.M, c.N, c.a_km, c.b_km) == (M, N, a, b):
            _run_gemm_case(c, family)


# ------------------------------------------------------------------------------- hicgat_gemm_wgrad
def _wgrad_once(c, dy, x, c0, db0, want_db, lddw):
    L = _L()
    dW = Buf(c.M, c.N, ld=lddw, data=c0)
    db = Buf(1, c.M, data=db0)
    nb = L.lib().hicgat_gemm_wgrad_workspace_bytes(c.M, c.N, c.splits)
    ws = L.workspace(nb, DEV) if c.splits > 1 else None
    rc = _rc("hicgat_gemm_wgrad", c.M, c.N, c.K, dy.ptr, dy.ld, x.ptr, x.ld, dW.ptr, lddw, db.ptr if want_db else None,
             int(c0 is not None), c.splits, L.ptr(ws), nb)
    assert rc == 0, (c.name, rc)
    (w, ok1), (d, ok2) = dW.read(), db.read()
    assert ok1 and ok2, f"{c.name}: wrote outside dW / db"
    if not want_db:
        assert db.untouched(), f"{c.name}: db = NULL, yet the db buffer changed"
    return w, d[0]


_WCASES = R.wgrad_cases()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,N", sorted({(c.M, c.N) for c in _WCASES}))
def test_gemm_wgrad(M, N, family):
    """dW and db from one launch: the CS form of every tile, float4 and scalar staging, splits 1 and 3 (the
    db partials ride in the slab), db given and NULL, accumulate on and off, lddw = N and > N."""
    opA, opB, _, c0, db0 = R.logical(family, M, N, 100)
    dy_h, x_h = R.stored(1, 1, opA, opB)
    prod = R.gemm_ref(1, 1, dy_h, x_h)
    for c in (c for c in _WCASES if (c.M, c.N) == (M, N)):
        dy, x = In(dy_h, c.M + c.lda_pad), In(x_h)
        _assert_form(c, dy, x)
        for acc in (0, 1):
            for pad in (0, 3):
                args = (c, dy, x, c0 if acc else None, db0 if acc else None, c.with_db, c.N + pad)
                (w, d), (w2, d2) = _wgrad_once(*args), _wgrad_once(*args)
                assert R.same_bits(w, w2) and R.same_bits(d, d2), (c.name, "two calls differ")
                ref, bound = R.with_terms(*prod, None, c0 if acc else None)
                _verify(family, "dW", w, ref, bound, (c.name, acc, pad))
                if c.with_db:
                    _, rdb, _, bdb = R.wgrad_ref(dy_h, x_h, None, db0 if acc else None)
                    _verify(family, "db", d, rdb, bdb, (c.name, acc, pad))
        _KEEP.clear()


# ------------------------------------------------------------------------------- wgrad_grouped_kernel
class WJ:
    """One weight job of hicgat_param_grads_grouped with its buffers and float64 reference."""

    def __init__(self, family, M, N, K, acc=0, want_db=True, lddw_pad=0, ldy_pad=0):
        self.M, self.N, self.K, self.acc, self.want_db, self.family = M, N, K, acc, want_db, family
        rng = np.random.default_rng([M, N, K, family == "random"])
        draw = (lambda *s: rng.integers(-4, 5, s).astype(f32)) if family == "integers" else (lambda *s: rng.standard_normal(s).astype(f32))
        self.dy_h, self.x_h, self.c0, self.db0 = draw(K, M), draw(K, N), draw(M, N), draw(M)
        self.dy = In(self.dy_h if M else np.zeros((K, 1), f32), max(M, 1) + ldy_pad)
        self.x = In(self.x_h if N else np.zeros((K, 1), f32))
        self.dW = Buf(max(M, 1), max(N, 1), ld=max(N, 1) + lddw_pad, data=self.c0 if (acc and M and N) else None)
        self.db = Buf(1, max(M, 1), data=self.db0 if (acc and M) else None)

    def job(self, **kw):
        f = dict(dy=self.dy.addr, ldy=self.dy.ld, x=self.x.addr, ldx=self.x.ld, dw=self.dW.addr, lddw=self.dW.ld,
                 db=self.db.addr if self.want_db else None, M=self.M, N=self.N, K=self.K, accumulate=self.acc)
        f.update(kw)
        return _L().WgradJob(**f)

    def vec(self):
        return bool(_L().load().hicgat_gemm_form(1, 1, self.M, self.N, max(self.K, 1), self.dy.ptr, self.dy.ld, self.x.ptr,
                                                 self.x.ld, 1, R.F32, 1) & 16)

    def check(self, what):
        if self.M == 0 or self.N == 0:
            assert self.dW.untouched() and self.db.untouched(), (what, "an empty job's outputs changed")
            return None
        (w, ok1), (d, ok2) = self.dW.read(), self.db.read()
        assert ok1 and ok2, (what, "wrote outside dW / db")
        dW, db, wb, bb = R.wgrad_ref(self.dy_h, self.x_h, self.c0 if self.acc else None, self.db0 if self.acc else None)
        _verify(self.family, "dW", w, dW, wb, what)
        if self.want_db:
            _verify(self.family, "db", d[0], db, bb, what)
        else:
            assert self.db.untouched(), (what, "db = NULL, yet the db buffer changed")
        return w, d


def _grouped(jobs, target, cjobs=(), short=0, ws_none=False):
    L = _L()
    W = (L.WgradJob * max(1, len(jobs)))(*jobs)
    C = (L.ColsumJob * max(1, len(cjobs)))(*cjobs)
    nb = L.lib().hicgat_param_grads_workspace_bytes(W, len(jobs), target)
    ws = L.workspace(nb, DEV)
    return _rc("hicgat_param_grads_grouped", W, len(jobs), C, len(cjobs), target, L.ptr(ws), nb - short), nb


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("name", list(R.WG_SINGLE))
def test_wgrad_grouped_single_job(name, acc, family):
    M, N, K, target, splits, vec = R.WG_SINGLE[name]
    res = []
    for _ in range(2):
        j = WJ(family, M, N, K, acc)
        assert j.vec() == vec
        rc, nb = _grouped([j.job()], target)
        assert rc == 0
        assert nb == (splits * (M * N + M) * 4 if splits > 1 else 0), "the split count read back from the workspace size"
        res.append(j.check(name))
    assert R.same_bits(res[0][0], res[1][0]) and R.same_bits(res[0][1], res[1][1])
    _KEEP.clear()


@pytest.mark.parametrize("acc", [0, 1])
def test_wgrad_grouped_k0(acc):
    """K = 0: dW and db become 0, or stay as they were under accumulate."""
    j = WJ("integers", 68, 132, 0, acc)
    rc, nb = _grouped([j.job()], 64)
    assert rc == 0 and nb == 0
    (w, ok1), (d, ok2) = j.dW.read(), j.db.read()
    assert ok1 and ok2
    assert R.same_bits(w, j.c0 if acc else np.zeros_like(w)) and R.same_bits(d[0], j.db0 if acc else np.zeros_like(d[0]))
    _KEEP.clear()


@pytest.mark.parametrize("family", FAMILIES)
def test_wgrad_grouped_mixed_launch(family):
    """One launch of: a float4 and a scalar job, a job with lddw > N (not split) beside split ones, db NULL
    beside db given, accumulate 0 beside 1, and jobs with M = 0 and N = 0 in the middle (their outputs
    untouched, the later jobs right)."""
    res = []
    for _ in range(2):
        jobs = [WJ(family, 132, 132, 1000, acc=0), WJ(family, 3, 64, 1000, acc=1), WJ(family, 0, 64, 1000),
                WJ(family, 68, 72, 1000, acc=0, want_db=False, lddw_pad=4), WJ(family, 64, 0, 1000),
                WJ(family, 256, 68, 1000, acc=1, want_db=False), WJ(family, 65, 67, 1000, acc=1, lddw_pad=1)]
        assert [j.vec() for j in jobs if j.M and j.N] == [True, False, True, True, False]
        rc, nb = _grouped([j.job() for j in jobs], 64)
        assert rc == 0
        # 9 tiles x K = 9000 over 64 workgroups -> chunks of 144 -> 7 splits, of the contiguous jobs only
        assert nb == 7 * 4 * sum(j.M * j.N + j.M for j in jobs if j.dW.ld == j.N and j.M and j.N)
        res.append([j.check(("mixed", k)) for k, j in enumerate(jobs)])
    assert all(a is None or (R.same_bits(a[0], b[0]) and R.same_bits(a[1], b[1])) for a, b in zip(*res))
    _KEEP.clear()


def _colsum_pair(family):
    rng = np.random.default_rng(77)
    src = rng.integers(-4, 5, (37, 20)).astype(f32) if family == "integers" else rng.standard_normal((37, 20)).astype(f32)
    s, d = In(src), Buf(1, 20)
    return src, d, _L().ColsumJob(s.addr, 20, 37, 20, d.addr, 0, None, 0, 1, 0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("with_colsum", [0, 1])
def test_wgrad_grouped_sixteen_jobs(with_colsum, family):
    """16 jobs of different tile counts, each split in two chunks (128 and 22 deep): every job's first and
    last workgroup is a find_job boundary; with column-sum jobs both grouped kernels run from one call."""
    res = []
    for _ in range(2):
        jobs = [WJ(family, M, N, K, acc=i % 2, want_db=i % 3 != 2) for i, (M, N, K) in enumerate(R.wg16_shapes())]
        assert [j.vec() for j in jobs] == [i % 4 != 3 for i in range(16)]
        src, dst, cj = _colsum_pair(family)
        rc, nb = _grouped([j.job() for j in jobs], 4096, [cj] if with_colsum else [])
        assert rc == 0 and nb == 2 * 4 * sum(j.M * j.N + j.M for j in jobs)
        res.append([j.check(("sixteen", k)) for k, j in enumerate(jobs)])
        got, ok = dst.read()
        if with_colsum:
            assert ok
            _verify(family, "db", got[0], src.astype(np.float64).sum(0), np.abs(src.astype(np.float64)).sum(0), "colsum job")
        else:
            assert dst.untouched()
    assert all(R.same_bits(a[0], b[0]) and R.same_bits(a[1], b[1]) for a, b in zip(*res))
    _KEEP.clear()


def test_wgrad_grouped_refusals():
    """Each refusal is returned by the host code before any launch; every output buffer keeps its bits."""
    jobs = [WJ("integers", 68, 68, 300, acc=0) for _ in range(17)]
    outs = [b for j in jobs for b in (j.dW, j.db)]
    _, dst, cj = _colsum_pair("integers")
    outs.append(dst)
    W = [j.job() for j in jobs]
    bad = []

    def expect(code, rc, what):
        if rc != code:
            bad.append((what, rc, code))

    expect(EUNSUPPORTED, _grouped(W, 4096)[0], "17 weight jobs")
    rc, nb = _grouped(W[:16], 4096, [cj])
    assert nb == 16 * 3 * (68 * 68 + 68) * 4       # 16 split jobs with db: 32 slab sums, no room for the column-sum job
    expect(EUNSUPPORTED, rc, "kMaxCJobs overflow")
    expect(EINVAL, _grouped(W[:2], 4096, short=1)[0], "workspace one byte short")
    expect(EINVAL, _grouped([jobs[0].job(lddw=67)], 64)[0], "lddw < N")
    for k in ("dy", "x", "dw"):
        expect(EINVAL, _grouped([jobs[0].job(**{k: None})], 64)[0], f"NULL {k}")
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(b.untouched() for b in outs)
    _KEEP.clear()


# ------------------------------------------------------------------------------- hicgat_gemm_rows_grouped
class RJ:
    def __init__(self, family, b_km, M, N, K, bias=True, relu=True, ldc_pad=4, ldr_pad=8):
        self.M, self.N, self.K, self.b_km, self.family = M, N, K, b_km, family
        opA, opB, bias_h, _, _ = R.logical(family, M, N, K)
        A, B = R.stored(0, b_km, opA, opB)
        self.bias_h = bias_h if bias else None
        self.ref = R.rows_ref(b_km, A, B, self.bias_h)
        self.a, self.b = In(A, K + 4), In(B, B.shape[1] + 8)
        self.bias = _vec(bias_h) if bias else None
        self.c = Buf(M, N, ld=N + ldc_pad)
        self.cr = Buf(M, N, ld=N + ldr_pad) if relu else None

    def job(self, **kw):
        f = dict(a=self.a.addr, lda=self.a.ld, b=self.b.addr, ldb=self.b.ld, c=self.c.addr, ldc=self.c.ld,
                 c_relu=self.cr.addr if self.cr else None, ldr=self.cr.ld if self.cr else 0,
                 bias=self.bias.data_ptr() if self.bias is not None else None, M=self.M, N=self.N, K=self.K)
        f.update(kw)
        return _L().GemmJob(**f)

    def outs(self):
        return [self.c] + ([self.cr] if self.cr else [])

    def check(self, what):
        got, ok = self.c.read()
        assert ok, (what, "wrote outside C")
        C, Cr, bound = self.ref
        _verify(self.family, "rows_C", got, C, bound, what)
        if self.cr is None:
            return got, None
        r, ok = self.cr.read()
        assert ok, (what, "wrote outside the relu copy")
        assert R.same_bits(r, np.maximum(got, f32(0))), (what, "the relu copy is not relu of the written C")
        assert not np.signbit(r).any()
        return got, r


def _rows(jobs, b_km, splits, short=0):
    L = _L()
    G = (L.GemmJob * len(jobs))(*jobs)
    nb = L.lib().hicgat_gemm_rows_grouped_workspace_bytes(G, len(jobs), max(splits, 1))
    ws = L.workspace(nb, DEV)
    return _rc("hicgat_gemm_rows_grouped", G, len(jobs), b_km, splits, L.ptr(ws), nb - short)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("splits", R.ROWS_SPLITS)
@pytest.mark.parametrize("shapes", [R.ROWS_JOBS, R.ROWS_JOBS_8], ids=["five", "eight"])
@pytest.mark.parametrize("b_km", [0, 1])
def test_rows_grouped(b_km, shapes, splits, family):
    """Unequal jobs in one launch (N off a multiple of 128, one job per start[] / rstart[] slot with 8):
    splits = 1 writes C, bias and the relu copy from the tile; 3 and 4 through the slabs (4: the K = 20, 16
    and 4 jobs leave trailing empty chunks); ldc and ldr strided; every other job without bias, every third
    without a relu copy."""
    res = []
    for _ in range(2):
        jobs = [RJ(family, b_km, M, N, K, bias=k % 2 == 0, relu=k % 3 != 2) for k, (M, N, K) in enumerate(shapes)]
        assert _rows([j.job() for j in jobs], b_km, splits) == 0
        res.append([j.check((b_km, splits, k)) for k, j in enumerate(jobs)])
    for a, b in zip(*res):
        assert R.same_bits(a[0], b[0]) and (a[1] is None or R.same_bits(a[1], b[1]))
    _KEEP.clear()


def test_rows_grouped_refusals():
    """Each refusal is returned by the host code before any launch; every output keeps its bits."""
    jobs = [RJ("integers", 0, 64, 128, 20) for _ in range(9)]
    j = jobs[0]
    odd = RJ("integers", 0, 8, 8, 8)
    bad = []

    def expect(code, rc, what):
        if rc != code:
            bad.append((what, rc, code))

    expect(EUNSUPPORTED, _rows([x.job() for x in jobs], 0, 1), "9 jobs")
    expect(EUNSUPPORTED, _rows([j.job(K=18)], 0, 1), "K % 4")
    expect(EUNSUPPORTED, _rows([j.job(N=126)], 0, 1), "N % 4")
    expect(EUNSUPPORTED, _rows([j.job(ldc=j.c.ld + 1)], 0, 1), "ldc % 4")
    expect(EUNSUPPORTED, _rows([j.job(ldr=j.cr.ld + 2)], 0, 1), "ldr % 4")
    expect(EUNSUPPORTED, _rows([j.job(bias=j.bias.data_ptr() + 4)], 0, 1), "bias 4 bytes off")
    expect(EINVAL, _rows([j.job()], 0, 0), "splits = 0")
    expect(EINVAL, _rows([j.job(), odd.job()], 0, 3, short=1), "workspace one byte short")
    torch.cuda.synchronize()
    assert not bad, bad
    assert all(b.untouched() for x in jobs + [odd] for b in x.outs())
    _KEEP.clear()

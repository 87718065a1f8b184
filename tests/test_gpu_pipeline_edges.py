"""The kernels that run once per run, before the first step -- csrc/graph_build.hip (csr_strip_kernel,
scan_kernel, c2d_max_kernel, c2d_map_kernel), csrc/sage.hip (sage_weights_kernel, sage_agg_f512_kernel,
sage_agg_generic_kernel) and csrc/kr.hip (kr_matvec_kernel<true/false>, kr_scale_kernel) -- through the
C ABI, so that strides and alignment are the test's to choose, against tests/pipeline_ref.py (tied to
``oracle/`` on the CPU by tests/test_pipeline_ref_host.py).

Every strided case is a ``[:, :N]`` view of a buffer with ld = N + 3 / N + 4 (whichever parity the case
needs) or N + 37 whose padding holds a finite non-zero sentinel (1e300 in float64: a NaN would be hidden
by ``nz()`` and ``!= 0``), and every output buffer carries guard elements in front, behind and in its
padding columns that must come back unchanged (``Buf.read``).

Branches reached on purpose, by the test that names them:
  lda > N of csr_from_dense / sage_weights / cont2dist / kr_matvec / kr_scale, ldo > N -- the ``pad`` cases
  scan_kernel per = 2 (N = 1025) and per = 3 with empty trailing threads (N = 2049) -- test_csr_from_dense
  csr_strip_kernel's last column of a partial 64-tile, column 64 k, N = 1, 2, 64 k +- 1, a non-zero
    diagonal, -0.0, NaN, +-inf -- test_csr_from_dense
  sage_weights_kernel's one-thread-per-row block edge N = 255 / 256 / 257 -- test_sage_weights
  c2d_max_kernel's ``i += gridDim.x`` iteration (nb capped at 1024: the unique maximum sits in row 1024 of
    N = 1025) and the last row of N = 2049 -- test_cont2dist
  every exponent of torch_pow_scalar and the generic pow -- test_cont2dist, test_device_pow_distance
  kr_matvec_kernel<true> with even n, with odd n (the ``(n & 1) && lane == 0`` tail), <false> by an odd
    lda and by a 16-byte-misaligned A -- test_kr_matvec
  sage_agg_f512_kernel's U = 4 groups and 64-entry chunks at 1..6, 63..68, 131 and 201 entries; the generic
    kernel's second c0 pass (F = 257, 300, 513), F = 512 through it by ldz % 4 != 0 and by a misaligned z,
    ldz > 2F -- test_sage_agg
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pipeline_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Max float64 ulp distance of the device's raw pow(x, f) from the correctly rounded power (mpmath, 160
# bits, rounded once), measured on the MI355X by test_device_pow_distance over 1 / (every value of
# pipeline_ref.contact_pool() that is >= 1); torch's own CPU pow measures 1 ulp for both exponents
# (test_pipeline_ref_host.py::test_torch_pow_distance_to_the_reference).  DESIGN.md section 4.
POW_ULP_DEVICE = {0.4: 1, 1.5: 1}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _L():
    from hicgat import _lib
    return _lib


def _call(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)


class Buf:
    """A rows x cols matrix inside a flat device buffer: ``lead`` guard elements in front, rows ld >= cols
    apart, 8 guard elements behind; everything outside ``data`` holds ``fill``.  An even ``lead`` keeps
    the matrix 16-byte aligned, lead = 9 puts it one element off."""

    def __init__(self, rows, cols, dtype, fill, ld=None, lead=8, data=None):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.lead = rows, cols, ld, lead
        host = np.full(lead + rows * ld + 8, fill, dtype)
        if data is not None:
            self._matrix(host)[:, :cols] = data
        self.host = host
        self.dev = torch.from_numpy(host.copy()).to(DEV)
        self.addr = self.dev.data_ptr() + lead * host.itemsize
        self.ptr = ctypes.c_void_p(self.addr)

    def _matrix(self, flat):
        return flat[self.lead:self.lead + self.rows * self.ld].reshape(self.rows, self.ld)

    def read(self):
        """(the matrix as it is now, whether every element outside it still has its first bits)."""
        got = self.dev.cpu().numpy()
        inner = self._matrix(got)[:, :self.cols].copy()
        was = self.host.copy()
        self._matrix(got)[:, :self.cols] = 0
        self._matrix(was)[:, :self.cols] = 0
        return inner, bool(np.array_equal(got.view(np.uint8), was.view(np.uint8)))

    def vector(self):
        m, ok = self.read()
        return m[0], ok


def _vec(data, dtype, fill):
    data = np.asarray(data, dtype)
    return Buf(1, len(data), dtype, fill, data=data)


# ------------------------------------------------------------------------------- 1. csr_from_dense
@functools.lru_cache(maxsize=None)
def _csr_ref(n, pattern):
    return R.csr_self_loops(R.csr_matrix(n, pattern))


@pytest.mark.parametrize("pad", [0, 3, 37])
@pytest.mark.parametrize("n,pattern", R.csr_cases(R.CSR_SIZES))
def test_csr_from_dense(n, pattern, pad):
    """hicgat_csr_from_dense (csr_strip_kernel<false> + scan_kernel, then csr_strip_kernel<true>) is
    csr_from_matrix + set_diag bit for bit, with lda = N and lda > N.  N = 1025 gives scan_kernel
    per = 2, N = 2049 per = 3 with 341 trailing threads whose range is empty."""
    a = R.csr_matrix(n, pattern)
    rp_ref, col_ref = _csr_ref(n, pattern)
    nnz = len(col_ref)
    A = Buf(n, n, np.float64, R.SENT64, ld=n + pad, data=a)
    rowptr = Buf(1, n + 1, np.int32, R.SENT_I32)
    _call("hicgat_csr_from_dense", A.ptr, n, n + pad, rowptr.ptr, None, None, 0)          # count pass
    rp, ok = rowptr.vector()
    assert ok, "count pass wrote outside rowptr[0..N]"
    assert np.array_equal(rp, rp_ref) and rp[n] == nnz
    col = Buf(1, nnz, np.int32, -1)
    _call("hicgat_csr_from_dense", A.ptr, n, n + pad, rowptr.ptr, col.ptr, None, 0)       # fill pass
    c, ok = col.vector()
    assert ok, "fill pass wrote past nnz or in front of col"
    assert np.array_equal(c, col_ref)
    rp, ok = rowptr.vector()
    assert ok and np.array_equal(rp, rp_ref)
    back, ok = A.read()
    assert ok and R.same_bits(back, a)


# ------------------------------------------------------------------------------- 2. sage_weights
@pytest.mark.parametrize("pad", [0, 3, 37])
@pytest.mark.parametrize("n,pattern", R.csr_cases(R.WEIGHT_SIZES))
def test_sage_weights(n, pattern, pad):
    """hicgat_sage_weights on the same matrices: ``value`` is csr_from_matrix's weight bit for bit (A[j, i]
    over A[i, j] when both are non-zero, either one alone), inv_deg is sage.degree_inverse bit for bit,
    +inf on a row without edges; N = 255 / 256 / 257 is the block edge of one thread per row."""
    a = R.csr_matrix(n, pattern)
    rp_ref, col_ref = _csr_ref(n, pattern)
    w_ref, inv_ref = R.sage_weights(a, rp_ref, col_ref)
    A = Buf(n, n, np.float64, R.SENT64, ld=n + pad, data=a)
    rowptr, col = _vec(rp_ref, np.int32, R.SENT_I32), _vec(col_ref, np.int32, R.SENT_I32)
    w = Buf(1, len(col_ref), np.float32, R.SENT32)
    inv = Buf(1, n, np.float32, R.SENT32)
    _call("hicgat_sage_weights", A.ptr, n, n + pad, rowptr.ptr, col.ptr, w.ptr, inv.ptr)
    (wv, ok_w), (iv, ok_i) = w.vector(), inv.vector()
    assert ok_w and ok_i
    assert R.same_bits(wv, w_ref)
    assert R.same_bits(iv, inv_ref)
    if pattern in ("zero", "isolated"):
        lone = np.diff(rp_ref) == 1
        assert lone.any() and np.all(iv[lone] == np.inf)


# ------------------------------------------------------------------------------- 3. cont2dist
def _cont2dist(y, n, f, ldy_pad, ldo_pad, want32, want64):
    L = _L()
    Y = Buf(n, n, np.float64, R.SENT64, ld=n + ldy_pad, data=y)
    o32 = Buf(n, n, np.float32, R.SENT32, ld=n + ldo_pad) if want32 else None
    o64 = Buf(n, n, np.float64, R.SENT64, ld=n + ldo_pad) if want64 else None
    nbytes = L.lib().hicgat_cont2dist_workspace_bytes(n)
    ws = L.workspace(nbytes, DEV)
    _call("hicgat_cont2dist", Y.ptr, n, n + ldy_pad, float(f), o32.ptr if o32 else None, o64.ptr if o64 else None,
          n + ldo_pad, L.ptr(ws), ws.numel())
    out = []
    for o in (o32, o64):
        if o is None:
            out.append(None)
        else:
            m, ok = o.read()
            assert ok, "cont2dist wrote into guards or padding"
            out.append(m)
    return out


@functools.lru_cache(maxsize=2)
def _c2d_torch(n, kind, f):
    from oracle import graph as og
    return og.cont2dist(torch.tensor(R.contacts(n, kind)), f).numpy()


@pytest.mark.parametrize("factor", R.C2D_FACTORS)
@pytest.mark.parametrize("kind", R.C2D_KINDS)
@pytest.mark.parametrize("n", R.C2D_SIZES)
def test_cont2dist(n, kind, factor):
    """hicgat_cont2dist with ldy > N and ldo > N, writing both outputs, out32 only and out64 only.
    Exponents 0, 1, 2, 3, -1, -2: bit-exact with oracle.graph.cont2dist (torch CPU float64), NaNs in the
    same places.  +-0.5: bit-exact with the IEEE numpy restatement and within 2 ulp of torch.  0.4 and
    1.5 (the device pow, not correctly rounded): within 2 * POW_ULP_DEVICE ulp of the high-precision map
    rounded to float64 -- measured max distance of the raw device power 1 ulp for both exponents, of
    torch's own 1 ulp for both; twice, because the maximum the entry is divided by carries the same
    error.  out32 is float32(out64) exactly.  At N = 1025 the unique maximum is in row 1024, which only
    the strided second iteration of c2d_max_kernel reads; at N = 2049 the last row is block 0's third."""
    y = R.contacts(n, kind)
    o32, o64 = _cont2dist(y, n, factor, 3, 37, True, True)
    special = ~(np.isfinite(y) & (y > 0)) | np.eye(n, dtype=bool)
    if factor in R.C2D_POW:
        ref = R.cont2dist_hp(y, factor)
        d = R.ulps(o64, ref)
        print(f"cont2dist N={n} {kind} f={factor}: max {int(d.max())} ulp from the high-precision map")
        assert np.array_equal(np.isnan(o64), np.isnan(ref))
        assert int(d.max()) <= 2 * POW_ULP_DEVICE[factor]
        assert R.same_bits(o64[special], ref[special])
    else:
        t = _c2d_torch(n, kind, factor)
        assert np.array_equal(np.isnan(o64), np.isnan(t))
        if factor in R.C2D_EXACT:
            assert R.same_bits(o64, t)
        else:
            assert R.same_bits(o64, R.cont2dist_ieee(y, factor))
            assert int(R.ulps(o64, t).max()) <= 2
        assert R.same_bits(o64[n - 1], (t if factor in R.C2D_EXACT else R.cont2dist_ieee(y, factor))[n - 1])
    if kind == "allzero" and factor != 0.0:
        assert np.isnan(o64).all()
    if kind != "allzero" and n >= 3 and factor != 0.0:      # the maximum, seen only in the last row
        assert o64[n - 1, 0 if factor > 0 else 1] == 1.0
        if kind == "positive":
            assert (o64 == 1.0).sum() == 1
    with np.errstate(over="ignore"):          # lowest / max overflows float32 to -inf on both sides
        assert R.same_bits(o32, o64.astype(np.float32))
    only32, _ = _cont2dist(y, n, factor, 37, 0, True, False)
    assert R.same_bits(only32, o32)
    _, only64 = _cont2dist(y, n, factor, 0, 3, False, True)
    assert R.same_bits(only64, o64)


@pytest.mark.parametrize("factor", R.C2D_POW)
def test_device_pow_distance(factor):
    """The raw device pow against the correctly rounded power: with every contact >= 1 and one equal to
    1 the maximum distance is exactly 1, so the map IS the raw power.  Measured on the MI355X: max 1 ulp
    for 0.4 and for 1.5 (torch's CPU pow: 1 ulp for both)."""
    pool = R.contact_pool()
    pool = pool[pool >= 1.0]
    n = 65
    assert n * (n - 1) >= len(pool)
    y = np.resize(pool, n * n).reshape(n, n).copy()
    y[0, 1] = 1.0
    _, o64 = _cont2dist(y, n, factor, 0, 0, False, True)
    with np.errstate(divide="ignore"):
        raw = R.pow_correctly_rounded(1.0 / y, factor)
    np.fill_diagonal(raw, 0.0)
    assert raw.max() == 1.0 and o64[0, 1] == 1.0
    d = R.ulps(o64, raw)
    dt = R.ulps(torch.pow(torch.tensor(1.0 / y), factor).fill_diagonal_(0).numpy(), raw)
    print(f"pow(x, {factor}) over {len(pool)} values: device max {int(d.max())} ulp ({(d > 0).mean():.2%} off), "
          f"torch max {int(dt.max())} ulp ({(dt > 0).mean():.2%} off)")
    assert int(d.max()) <= POW_ULP_DEVICE[factor]


# ------------------------------------------------------------------------------- 4. KR
KR_LAYOUTS = ("contiguous", "even_lda", "odd_lda", "misaligned")


def _kr_layout(n, layout):
    """(lda, lead, whether kr_matvec_kernel<true> runs)."""
    even, odd = (n + 4, n + 3) if n % 2 == 0 else (n + 3, n + 4)
    if layout == "contiguous":
        return n, 8, n % 2 == 0
    if layout == "even_lda":
        return even, 8, True
    if layout == "odd_lda":
        return odd, 8, False
    return even, 9, False


@pytest.mark.parametrize("with_v", [False, True])
@pytest.mark.parametrize("layout", KR_LAYOUTS)
@pytest.mark.parametrize("n", R.KR_SIZES)
def test_kr_matvec(n, layout, with_v):
    """hicgat_kr_matvec in its four forms -- even lda and 16-byte-aligned A with even n (vector path)
    and with odd n (its ``(n & 1) && lane == 0`` tail), odd lda (scalar path), even lda with A one
    double into its buffer (misaligned: scalar path) -- and contiguous, with v null and given, NaNs in A
    counting as 0, x and p of both signs.  Each row is within (n + 4) 2^-53 (|x_i| sum_j |A_ij x_j p_j|
    + |v_i p_i|) of the exact value (the bound of any summation order of n fused terms); two calls give
    the same bits; the guards round ``out`` are untouched."""
    a, x, p, v = R.kr_inputs(n)
    lda, lead, vec = _kr_layout(n, layout)
    A = Buf(n, n, np.float64, R.SENT64, ld=lda, lead=lead, data=a)
    assert (lda % 2 == 0 and A.addr % 16 == 0) == vec
    X, P, V = (_vec(t, np.float64, R.SENT64) for t in (x, p, v))
    outs = []
    for _ in range(2):
        out = Buf(1, n, np.float64, R.SENT64)
        _call("hicgat_kr_matvec", A.ptr, lda, n, X.ptr, P.ptr, V.ptr if with_v else None, out.ptr)
        o, ok = out.vector()
        assert ok, "kr_matvec wrote outside out[0..n)"
        outs.append(o)
    assert R.same_bits(outs[0], outs[1])
    ref, bound = R.kr_matvec_exact(n, with_v)
    worst = 0.0
    for i in range(n):
        err = abs(R.Fraction(float(outs[0][i])) - ref[i])
        assert err <= bound[i], (i, float(err), float(bound[i]))
        worst = max(worst, float(err / bound[i]) if bound[i] else 0.0)
    print(f"kr_matvec n={n} {layout} ({'vector' if vec else 'scalar'} path) v={with_v}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("lda_pad,ldo_pad", [(0, 0), (3, 37), (37, 4)])
@pytest.mark.parametrize("n", R.KR_SCALE_SIZES)
def test_kr_scale(n, lda_pad, ldo_pad):
    """hicgat_kr_scale is np.rint(((x_i A_ij) x_j) 1e6) / 1e6 bit for bit, NaN where A is NaN, with
    products exactly on k + 0.5 millionths (half to even, both signs), entries where x_i (A_ij x_j) would
    round to another millionth than the reference's (x_i A_ij) x_j, and padded lda / ldo; n = 257 leaves
    n * n no multiple of the 256-thread block."""
    a, x, _, _ = R.kr_scale_inputs(n)
    A = Buf(n, n, np.float64, R.SENT64, ld=n + lda_pad, data=a)
    out = Buf(n, n, np.float64, R.SENT64, ld=n + ldo_pad)
    X = _vec(x, np.float64, R.SENT64)
    _call("hicgat_kr_scale", A.ptr, n + lda_pad, n, X.ptr, out.ptr, n + ldo_pad)
    o, ok = out.read()
    assert ok, "kr_scale wrote into guards or padding"
    assert R.same_bits(o, R.kr_scale_ref(a, x))
    assert np.array_equal(np.isnan(o), np.isnan(a))


@pytest.mark.parametrize("n", R.KR_E2E_SIZES)
def test_krnorm_both_kernel_forms(n):
    """hicgat.kr.KRnorm end to end with no row dropped, so the parity of n picks the kernel: 64 and 130
    run kr_matvec_kernel<true>, 63, 65 and 129 <false>.  The assertions of test_kr_device_matches_oracle."""
    import hicgat
    from oracle import kr
    m = R.kr_e2e_input(n)
    ref, keep_r = kr.krnorm(m)
    out, keep, info = hicgat.kr.KRnorm(m, return_info=True)
    out = out.cpu().numpy()
    assert len(keep_r) == n and np.array_equal(keep.cpu().numpy(), keep_r)
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    ok = ~np.isnan(ref)
    diff = np.abs(out[ok] - ref[ok])
    print(f"KRnorm n={n}: {info['outer']} outer iterations, max diff {diff.max():.3g}, {(diff > 0).mean():.3%} differ")
    assert diff.max() <= 1.0000001e-6
    assert (diff > 0).mean() < 0.01
    assert np.array_equal(out[ok], np.rint(out[ok] * 1e6) / 1e6)


# ------------------------------------------------------------------------------- 5. sage_agg
SAGE_LAYOUTS = [(F, lay) for F in R.SAGE_F
                for lay in (("fast", "fast_pad36", "ldz_pad3", "z_misaligned") if F == 512 else ("tight", "pad3", "pad37"))]
_PAD = {"fast": 0, "tight": 0, "z_misaligned": 0, "fast_pad36": 36, "ldz_pad3": 3, "pad3": 3, "pad37": 37}


@pytest.fixture(scope="module")
def sage_dev():
    rowptr, col, value = R.sage_graph()
    inv = R.degree_inverse(rowptr, col, value, R.SAGE_N)
    rp, c, w = R.insert_loops(rowptr, col, value)
    bufs = (_vec(rp, np.int32, R.SENT_I32), _vec(c, np.int32, R.SENT_I32), _vec(w, np.float32, R.SENT32),
            _vec(inv, np.float32, R.SENT32))
    feats = {}

    def x(F):
        if F not in feats:
            feats[F] = torch.from_numpy(R.sage_features(F)).to(DEV)
        return feats[F]
    return bufs, x


def _sage_agg(sage_dev, F, layout, transpose, trunc, r0, r1):
    L = _L()
    (rp, c, w, inv), feat = sage_dev
    x = feat(F)
    width = 2 * F if trunc else F
    ldz = width + _PAD[layout]
    z = Buf(R.SAGE_N, width, np.float32, R.SENT32, ld=ldz, lead=9 if layout == "z_misaligned" else 8)
    fast = F == 512 and ldz % 4 == 0 and z.addr % 16 == 0 and x.data_ptr() % 16 == 0
    assert fast == (layout in ("fast", "fast_pad36"))
    _call("hicgat_sage_agg", rp.ptr, c.ptr, w.ptr, inv.ptr, R.SAGE_N, F, r0, r1, L.ptr(x), int(transpose), int(trunc),
          z.ptr, ldz)
    m, ok = z.read()
    assert ok, "sage_agg wrote into guards or padding"
    return m


@pytest.mark.parametrize("rows", list(R.SAGE_ROWS))
@pytest.mark.parametrize("trunc", [0, 1])
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("F,layout", SAGE_LAYOUTS)
def test_sage_agg(sage_dev, F, layout, transpose, trunc, rows):
    """hicgat_sage_agg on a hand-built CSR whose rows 0..12 have 0, 1, 2, 3, 4, 5, 62, 63, 64, 65, 67, 130
    and 200 neighbours (+ the loop), one weight per direction: each element within (deg + 2) 2^-24
    sum_j |p_ij x_j| of the float64 sum with the fp32 product p = inv * w formed as the kernel forms it;
    the trunc half equal to x.long().float() (as values: truncf keeps -0.0 for -0.25, .long() gives +0.0); rows outside [row_begin, row_end), the columns past the
    written width and the guards untouched.  F = 512 runs sage_agg_f512_kernel when contiguous or padded
    by a multiple of 4, sage_agg_generic_kernel with ldz % 4 != 0 or z one float off 16 bytes; F > 256
    other than 512 runs the generic kernel's second c0 pass."""
    r0, r1 = R.SAGE_ROWS[rows]
    m = _sage_agg(sage_dev, F, layout, transpose, trunc, r0, r1)
    ref, bound = R.sage_agg_ref(F, bool(transpose))
    inside = np.zeros(R.SAGE_N, bool)
    inside[r0:r1] = True
    assert np.all(m[~inside].view(np.uint32) == np.float32(R.SENT32).view(np.uint32))
    err = np.abs(m[inside, :F].astype(np.float64) - ref[inside])
    assert np.all(err <= bound[inside]), np.argwhere(err > bound[inside])[:5]
    if trunc:
        assert np.array_equal(m[inside, F:], R.trunc_ref(R.sage_features(F))[inside])


@pytest.mark.parametrize("transpose", [0, 1])
def test_sage_f512_fast_and_generic_recorded(sage_dev, transpose):
    """Whether sage_agg_f512_kernel and sage_agg_generic_kernel agree bit for bit at F = 512 is printed,
    not asserted (both add a row's entries in CSR order with one fma each); both are inside the bound."""
    fast = _sage_agg(sage_dev, 512, "fast", transpose, 1, 0, R.SAGE_N)
    gen = _sage_agg(sage_dev, 512, "ldz_pad3", transpose, 1, 0, R.SAGE_N)
    same = R.same_bits(fast, gen)
    differ = int((fast.view(np.uint32) != gen.view(np.uint32)).sum())
    print(f"sage_agg F=512 transpose={transpose}: fast and generic kernels bit-equal: {same} ({differ} of {fast.size} differ)")
    ref, bound = R.sage_agg_ref(512, bool(transpose))
    for m in (fast, gen):
        assert np.all(np.abs(m[:, :512].astype(np.float64) - ref) <= bound)

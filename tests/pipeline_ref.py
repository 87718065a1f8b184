"""Plain numpy / exact references of the run-once pipeline kernels (csrc/graph_build.hip, csrc/sage.hip,
csrc/kr.hip) and the one builder of the inputs that tests/test_gpu_pipeline_edges.py (GPU) and
tests/test_pipeline_ref_host.py (CPU) share.  The host file ties every function here to ``oracle/``;
the GPU file compares the kernels with them through the C ABI, where strides and alignment are the
test's to choose.

  csr_self_loops     pattern (A != 0) | (A^T != 0) | I, row-major: csr_from_matrix + set_diag
  sage_weights       w per CSR entry (0 on the loops), 1 / (sequential fp32 row sum)
  cont2dist_ieee     utils.cont2dist with the exponents ATen special-cases, every step IEEE
  cont2dist_hp       the same for a generic exponent, the power from mpmath rounded once
  kr_matvec_exact    x_i sum_j nz(A_ij) x_j p_j + v_i p_i in rationals, and the summation bound
  kr_scale_ref       round6((x_i A_ij) x_j), NaN kept
  sage_agg_ref       fp64 sum_j fl32(inv * w_ij) x_j and its fp32 summation bound

Every strided case is a ``[:, :N]`` view of a wider buffer whose padding holds a finite non-zero
sentinel (SENT64 / SENT32): a kernel that reads its padding gets a wrong answer, not a NaN that
``a == a`` or ``!= 0`` would hide.
"""
import functools
from fractions import Fraction

import numpy as np

SENT64 = 1e300
SENT32 = np.float32(-3.0e38)
SENT_I32 = np.int32(-7)


# ------------------------------------------------------------------------------- ulp distance
def _ordered(a):
    b = np.ascontiguousarray(a, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) == 1, ~b, b | np.uint64(1 << 63))


def ulps(a, b):
    """Distance in float64 steps (uint64).  NaN against NaN is 0, NaN against a number 2^63;
    -0.0 and +0.0 are one step apart."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ua, ub = _ordered(a), _ordered(b)
    d = np.maximum(ua, ub) - np.minimum(ua, ub)
    na, nb = np.isnan(a), np.isnan(b)
    d = np.where(na & nb, np.uint64(0), d)
    return np.where(na ^ nb, np.uint64(1 << 63), d)


def same_bits(a, b):
    """Bit equality outside the NaNs, and the NaNs in the same places (payloads are not compared)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


# ------------------------------------------------------------------------------- graph build
CSR_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2049)
WEIGHT_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2049)
CSR_PATTERNS = ("zero", "full", "asym", "diag", "negzero", "nonfinite", "isolated", "lastcol", "col64k")
FULL_MAX = 129


def csr_cases(sizes):
    return [(n, p) for n in sizes for p in CSR_PATTERNS if p != "full" or n <= FULL_MAX]


def _pairs(rng, nodes, m):
    """Up to m distinct pairs lo < hi among ``nodes``, in random order."""
    nodes = np.asarray(nodes)
    k = len(nodes)
    if k < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    i, j = rng.integers(0, k, 2 * m), rng.integers(0, k, 2 * m)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    key = rng.permutation(np.unique(lo[lo < hi] * k + hi[lo < hi]))[:m]
    return nodes[key // k], nodes[key % k]


def _values(rng, k):
    return rng.uniform(0.5, 100.0, k) * rng.choice([-1.0, 1.0], k)


def col64k_pairs(n):
    """(row, column): the row's only neighbour is column 64 k (k = 0: row 1; else the row before it)."""
    out = [(1, 0)] if n >= 2 else []
    return out + [(c - 1, c) for c in range(64, n, 64)]


@functools.lru_cache(maxsize=None)
def csr_matrix(n, pattern):
    """The dense float64 input of one (size, pattern) case; at most 4 n undirected edges but for 'full'."""
    rng = np.random.default_rng([n, CSR_PATTERNS.index(pattern)])
    a = np.zeros((n, n))
    if n == 0 or pattern == "zero":
        return a
    if pattern == "full":                       # every entry non-zero, the diagonal included
        a[:] = _values(rng, n * n).reshape(n, n)
        return a
    if pattern == "lastcol":
        special = [(0, n - 1)] if n >= 2 else []
    elif pattern == "col64k":
        special = col64k_pairs(n)
    else:
        special = []
    taken = {v for rc in special for v in rc}
    lo, hi = _pairs(rng, [v for v in range(n) if v not in taken], 4 * n)
    m = len(lo)
    if pattern == "negzero":
        a[:] = -0.0                             # -0.0 != 0 is false: no edge
    if pattern == "asym":
        t = m // 3
        a[lo[:t], hi[:t]] = _values(rng, t)                       # only A[i, j]
        a[hi[t:2 * t], lo[t:2 * t]] = _values(rng, t)             # only A[j, i]
        a[lo[2 * t:], hi[2 * t:]] = _values(rng, m - 2 * t)       # both, with different values
        a[hi[2 * t:], lo[2 * t:]] = _values(rng, m - 2 * t)
    else:
        h = m // 2
        a[lo[:h], hi[:h]] = a[hi[:h], lo[:h]] = _values(rng, h)   # symmetric
        a[lo[h:], hi[h:]] = _values(rng, m - h)                   # upper entry only
    if pattern == "diag":
        a[np.arange(n), np.arange(n)] = _values(rng, n)           # must be ignored
    elif pattern == "nonfinite":
        k = np.arange(m)
        for r, v in enumerate((np.nan, np.inf, -np.inf)):         # edges like any other non-zero
            a[lo[k % 6 == r], hi[k % 6 == r]] = v
    elif pattern == "isolated":
        a[n // 2, :] = 0.0
        a[:, n // 2] = 0.0
    for r, c in special:                        # one direction only: row c sees it through A^T
        a[r, c] = _values(rng, 1)[0]
    return a


def csr_self_loops(a):
    """(rowptr int32 [N + 1], col int32 [nnz]) of (A != 0) | (A^T != 0) | I, columns ascending."""
    a = np.asarray(a)
    n = a.shape[0]
    nz = a != 0
    pat = nz | nz.T | np.eye(n, dtype=bool)
    cols = np.nonzero(pat)[1]
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum(pat.sum(axis=1))
    return rowptr, cols.astype(np.int32)


def entry_rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def sage_weights(a, rowptr, col):
    """(w float32 [nnz], inv_deg float32 [N]) on a CSR with self loops: w_ij = float32(A[max, min]) when
    that is non-zero, else float32(A[min, max]); 0 on the loops; inv_deg_i = 1 / s_i with s_i the fp32
    sum of row i's off-diagonal entries in column order."""
    n = a.shape[0]
    row = entry_rows(rowptr)
    lo, hi = np.minimum(row, col), np.maximum(row, col)
    low = a[hi, lo]
    w = np.where(low != 0, low, a[lo, hi]).astype(np.float32)
    off = row != col
    w[~off] = 0.0
    s = np.zeros(n, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(s, row[off], w[off])          # unbuffered: one fp32 add per entry, in order
    with np.errstate(divide="ignore", invalid="ignore"):
        return w, np.float32(1.0) / s


# ------------------------------------------------------------------------------- cont2dist
C2D_SIZES = (1, 2, 3, 255, 256, 257, 1025, 2049)
C2D_FACTORS = (0.0, 1.0, 2.0, 3.0, -1.0, -2.0, 0.5, -0.5, 0.4, 1.5)
C2D_EXACT = (0.0, 1.0, 2.0, 3.0, -1.0, -2.0)     # bit-exact with torch
C2D_SQRT = (0.5, -0.5)                           # bit-exact with IEEE sqrt, <= 2 ulp of torch
C2D_POW = (0.4, 1.5)                             # the device pow
C2D_KINDS = ("positive", "zeros", "negzero", "negative", "nan", "allzero")
C2D_SMALLEST, C2D_LARGEST = 1e-3, 1e4            # the unique extremes, both in the last row


@functools.lru_cache(maxsize=None)
def contact_pool():
    """4096 contact values in [0.5, 200]: every matrix draws from them, so a high-precision power is
    needed once per value and not once per entry."""
    rng = np.random.default_rng(77)
    return np.concatenate((rng.uniform(0.5, 100.0, 3072), rng.integers(1, 201, 1024).astype(np.float64)))


@functools.lru_cache(maxsize=12)
def contacts(n, kind):
    """The float64 contact matrix of one case.  But for 'allzero' the last row holds the unique smallest
    positive contact (the maximum distance for factor > 0) at column 0 and, from N = 3, the unique
    largest (the maximum for factor < 0) at column 1: at N = 1025 only c2d_max_kernel's second, strided
    iteration (row 1024) sees either."""
    rng = np.random.default_rng([n, C2D_KINDS.index(kind)])
    pool = contact_pool()
    y = pool[rng.integers(0, len(pool), (n, n))]
    u = rng.random((n, n))
    if kind == "allzero":
        y[:] = 0.0
        return y
    if kind == "zeros":
        y[u < 0.7] = 0.0                        # 1 / 0 = inf -> the max
    elif kind == "negzero":
        y[u < 0.2] = -0.0                       # 1 / -0 = -inf
        y[u > 0.8] = 0.0
    elif kind == "negative":
        y[u < 0.3] *= -1.0                      # NaN under sqrt and fractional powers
    elif kind == "nan":
        y[u < 0.1] = np.nan
    if n >= 2:                                  # the kind's own entry, whatever the draw gave
        y[0, n - 1] = {"zeros": 0.0, "negzero": -0.0, "negative": -7.25, "nan": np.nan}.get(kind, 3.0)
        y[n - 1, 0] = C2D_SMALLEST
    if n >= 3 and kind == "negzero":
        y[1, n - 1] = 0.0
    if n >= 3:
        y[n - 1, 1] = C2D_LARGEST
    return y


def torch_pow_ieee(x, f):
    """ATen pow(Tensor, Scalar) for the exponents it special-cases, each step one IEEE operation."""
    with np.errstate(all="ignore"):
        if f == 0.0:
            return np.ones_like(x)
        if f == 1.0:
            return x.copy()
        if f == 2.0:
            return x * x
        if f == 3.0:
            return x * x * x
        if f == 0.5:
            return np.sqrt(x)
        if f == -0.5:
            return 1.0 / np.sqrt(x)
        if f == -1.0:
            return 1.0 / x
        if f == -2.0:
            return 1.0 / (x * x)
    raise ValueError(f"exponent {f} goes through pow")


def _normalise(d):
    """fill_diagonal_(0); / max over nan_to_num(., posinf=0); +inf -> that max (utils.py:77-80)."""
    np.fill_diagonal(d, 0.0)
    with np.errstate(all="ignore"):
        m = np.max(np.nan_to_num(d, posinf=0.0))
        return np.nan_to_num(d, posinf=m) / m, m


def cont2dist_ieee(y, f):
    with np.errstate(all="ignore"):
        d = torch_pow_ieee(1.0 / np.asarray(y, np.float64), f)
    return _normalise(d)[0]


_MP_CACHE = {}


def _mp():
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.prec = 160
    return ctx


def pow_mp(values, f):
    """x ** f for positive finite float64 x as mpmath numbers (160 bits), cached per (x, f)."""
    ctx = None
    out = []
    for v in values:
        key = (float(v), float(f))
        if key not in _MP_CACHE:
            ctx = ctx or _mp()
            _MP_CACHE[key] = ctx.power(ctx.mpf(key[0]), ctx.mpf(key[1]))
        out.append(_MP_CACHE[key])
    return out


def to_f64(m):
    """An mpmath number rounded once, to nearest even."""
    from mpmath.libmp import round_nearest, to_float
    return to_float(m._mpf_, rnd=round_nearest)


def pow_correctly_rounded(x, f):
    """x ** f elementwise with the finite positive entries correctly rounded; the others (0, inf, NaN,
    negative) take numpy's IEEE special values, which are exact."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        r = np.power(x, f)
    pos = np.isfinite(x) & (x > 0)
    u, inv = np.unique(x[pos], return_inverse=True)
    r[pos] = np.array([to_f64(p) for p in pow_mp(u, f)], np.float64)[inv.reshape(-1)]
    return r


def cont2dist_hp(y, f):
    """utils.cont2dist for a generic exponent: (1 / y) is the float64 quotient both sides form, its
    power and the ratio to the maximum power are taken in 160 bits and rounded to float64 once."""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    with np.errstate(all="ignore"):
        x = 1.0 / y
        d = np.power(x, f)
    pos = np.isfinite(x) & (x > 0) & ~np.eye(n, dtype=bool)
    u, inv = np.unique(x[pos], return_inverse=True)
    pu = pow_mp(u, f)
    d[pos] = np.array([to_f64(p) for p in pu], np.float64)[inv.reshape(-1)]
    out, m = _normalise(d)
    if len(pu) and m > 0:
        top = max(pu)
        assert to_f64(top) == m
        out[pos] = np.array([to_f64(p / top) for p in pu], np.float64)[inv.reshape(-1)]
    return out


# ------------------------------------------------------------------------------- KR
KR_SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 257)
KR_SCALE_SIZES = (1, 2, 65, 257)
KR_E2E_SIZES = (63, 64, 65, 129, 130)


@functools.lru_cache(maxsize=None)
def kr_inputs(n):
    """(A, x, p, v): mixed signs everywhere, ~30 % zeros and ~3 % NaN (counted as 0) in A."""
    rng = np.random.default_rng([n, 5])
    a = rng.uniform(-50.0, 100.0, (n, n)) * (rng.random((n, n)) < 0.7)
    a[rng.random((n, n)) < 0.03] = np.nan
    a[n - 1, n - 1] = 37.5                      # the odd-n tail element of the last row is not 0
    if n >= 2:
        a[0, n - 1] = np.nan
    sign = lambda: rng.choice([-1.0, 1.0], n)
    return a, rng.uniform(0.2, 3.0, n) * sign(), rng.uniform(0.1, 2.0, n) * sign(), rng.uniform(0.1, 5.0, n) * sign()


@functools.lru_cache(maxsize=None)
def kr_matvec_exact(n, with_v):
    """Per row the exact value of x_i sum_j nz(A_ij) x_j p_j (+ v_i p_i) and the bound
    (n + 4) 2^-53 (|x_i| sum_j |A_ij x_j p_j| + |v_i p_i|), both as Fractions."""
    a, x, p, v = kr_inputs(n)
    xp = [Fraction(float(x[j])) * Fraction(float(p[j])) for j in range(n)]
    ref, bound = [], []
    u = Fraction(n + 4, 2 ** 53)
    for i in range(n):
        s = mag = Fraction(0)
        for j in range(n):
            if a[i, j] == a[i, j] and a[i, j] != 0.0:
                t = Fraction(float(a[i, j])) * xp[j]
                s += t
                mag += abs(t)
        xi = Fraction(float(x[i]))
        vp = Fraction(float(v[i])) * Fraction(float(p[i])) if with_v else Fraction(0)
        ref.append(xi * s + vp)
        bound.append(u * (abs(xi) * mag + abs(vp)))
    return ref, bound


def half_values(count):
    """+-(k + 0.5) / 1e6 whose float64 times 1e6 is exactly k + 0.5: rint must round half to even."""
    out, k = [], 3
    while len(out) < count:                     # k runs through even and odd: ties go down and up
        h = (k + 0.5) / 1e6
        if h * 1e6 == k + 0.5:
            out.append(h if (len(out) // 2) % 2 == 0 else -h)
        k += 1
    return out


KR_SCALE_X_HEAD = (1.0, -2.0, 0.5, -1.0)        # powers of two: h / (x_i x_j) is exact


def order_sensitive(xi, xj, start):
    """(a, k): ((xi a) xj) 1e6 is exactly k + 0.5 in float64 while xi (a xj) is a neighbouring float64
    whose millionths round the other way: only the reference's order of the two products gives the
    reference's digit.  Searched from k = start upwards."""
    k = start
    while True:
        k += 1
        t = k + 0.5
        r0 = t / 1e6
        for r in (r0, np.nextafter(r0, np.inf), np.nextafter(r0, -np.inf)):
            if r * 1e6 != t:
                continue
            a = r / (xi * xj)
            for cand in [a] + [np.nextafter(a, s * np.inf) for s in (1, -1)]:
                other = xi * (cand * xj)
                if (xi * cand) * xj == r and np.rint(other * 1e6) != np.rint(t):
                    return float(cand), k


@functools.lru_cache(maxsize=None)
def kr_scale_inputs(n):
    """(A, x, ties): mixed-sign x and A, NaNs in A, and at (i, j) for i, j < min(n, 4) products that
    land exactly on k + 0.5 millionths; ``ties`` lists (i, j, k + 0.5 signed).  From n = 65 eight more
    entries (``sens``) are order-sensitive: x_i (A_ij x_j) would round to another millionth."""
    rng = np.random.default_rng([n, 6])
    a = rng.uniform(-5.0, 100.0, (n, n)) * (rng.random((n, n)) < 0.7)
    a[rng.random((n, n)) < 0.05] = np.nan
    x = rng.uniform(0.2, 3.0, n) * rng.choice([-1.0, 1.0], n)
    h = min(n, len(KR_SCALE_X_HEAD))
    x[:h] = KR_SCALE_X_HEAD[:h]
    ties = []
    for (i, j), hv in zip(((i, j) for i in range(h) for j in range(h)), half_values(h * h)):
        a[i, j] = hv / (x[i] * x[j])
        ties.append((i, j, hv * 1e6))
    if n >= 5:
        a[4, 0] = np.nan
    sens, k = [], 1000
    for m in range(8 if n >= 65 else 0):
        i, j = 5 + m, 20 + 3 * m
        a[i, j], k = order_sensitive(x[i], x[j], k)
        sens.append((i, j))
    return a, x, ties, sens


def kr_scale_ref(a, x):
    with np.errstate(invalid="ignore"):
        return np.rint(((x[:, None] * a) * x[None, :]) * 1e6) / 1e6


def kr_e2e_input(n):
    rng = np.random.default_rng(n)
    a = rng.random((n, n)) * (rng.random((n, n)) < 0.6) * 100
    a = np.triu(a, 1)
    return a + a.T


# ------------------------------------------------------------------------------- SAGE aggregation
SAGE_N = 260
SAGE_DEGREES = (0, 1, 2, 3, 4, 5, 62, 63, 64, 65, 67, 130, 200)   # rows 0..12; + 1 entry for the loop
SAGE_F = (1, 63, 64, 65, 256, 257, 300, 512, 513)
SAGE_ROWS = {"all": (0, SAGE_N), "empty": (7, 7), "one": (12, 13), "five_from_3": (3, 8)}


@functools.lru_cache(maxsize=None)
def sage_graph():
    """Hand-built symmetric pattern without loops: row r < 13 has exactly SAGE_DEGREES[r] neighbours,
    all among the ordinary nodes 13..259, which also share ~300 edges of their own; one float32 weight
    per direction (w_ij != w_ji).  Returns (rowptr int64, col int64, value float32)."""
    rng = np.random.default_rng(11)
    n, s = SAGE_N, len(SAGE_DEGREES)
    adj = np.zeros((n, n), bool)
    for r, d in enumerate(SAGE_DEGREES):
        c = s + rng.choice(n - s, d, replace=False)
        adj[r, c] = adj[c, r] = True
    lo, hi = _pairs(rng, np.arange(s, n), 300)
    adj[lo, hi] = adj[hi, lo] = True
    rows, cols = np.nonzero(adj)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(adj.sum(axis=1))
    return rowptr, cols.astype(np.int64), rng.uniform(0.25, 4.0, len(cols)).astype(np.float32)


def degree_inverse(rowptr, col, value, n):
    """1 / (fp32 sum over the entries with column i, in CSR order): layers.py:41-44."""
    s = np.zeros(n, np.float32)
    np.add.at(s, col, value)
    with np.errstate(divide="ignore"):
        return np.float32(1.0) / s


def insert_loops(rowptr, col, value):
    """(i, i) with weight 0 into every row at its sorted place; int32 CSR as the kernels take it."""
    n = len(rowptr) - 1
    row = np.concatenate((entry_rows(rowptr), np.arange(n)))
    c = np.concatenate((col, np.arange(n)))
    v = np.concatenate((value, np.zeros(n, np.float32)))
    order = np.lexsort((c, row))
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(np.diff(rowptr) + 1)
    return rp, c[order].astype(np.int32), v[order].astype(np.float32)


@functools.lru_cache(maxsize=None)
def sage_features(F):
    """[SAGE_N, F] finite float32: |x| < 1, negatives, halves below 2^23 and values >= 2^24."""
    rng = np.random.default_rng([F, 3])
    x = (2.0 * rng.standard_normal((SAGE_N, F))).astype(np.float32)
    x[5::9, 0] = np.float32(-0.25)
    x[1::9, F - 1] = np.float32(8388607.5)
    x[2::9, 0] = np.float32(2.0 ** 24)
    x[3::9, F // 2] = np.float32(-(2.0 ** 24) - 2.0)
    x[4::9, F - 1] = np.float32(3.0e9)
    return x


def trunc_ref(x):
    """x.long().float() (layers.py:64)."""
    return np.asarray(x, np.float32).astype(np.int64).astype(np.float32)


def sage_agg_on(rowptr, col, value, inv, x, transpose):
    """(ref, bound) of the aggregation on any loop-free CSR: see sage_agg_ref."""
    n = len(rowptr) - 1
    row = entry_rows(rowptr)
    p = (inv[col] if transpose else inv[row]) * value          # one fp32 product per entry
    assert p.dtype == np.float32 and np.isfinite(p).all()
    P = np.zeros((n, n))
    P[row, col] = p
    x = np.asarray(x, np.float64)
    deg = np.diff(rowptr) + 1
    return P @ x, (deg + 2)[:, None] * 2.0 ** -24 * (np.abs(P) @ np.abs(x))


@functools.lru_cache(maxsize=None)
def sage_agg_ref(F, transpose):
    """(ref float64 [N, F], bound float64 [N, F]): sum_j fl32(inv * w_ij) x_j in float64 with
    inv = inv_deg[j] (transpose) or inv_deg[i], and (deg_i + 2) 2^-24 sum_j |p_ij x_j| with deg_i the
    row's CSR entries, loop included."""
    rowptr, col, value = sage_graph()
    inv = degree_inverse(rowptr, col, value, SAGE_N)
    return sage_agg_on(rowptr, col, value, inv, sage_features(F), transpose)

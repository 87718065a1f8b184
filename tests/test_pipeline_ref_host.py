"""tests/pipeline_ref.py on the CPU: every reference that tests/test_gpu_pipeline_edges.py holds the
run-once kernels to is tied here to ``oracle/`` (graph.csr_from_matrix + set_diag, graph.cont2dist,
sage.degree_inverse, sage.sage_aggregate, kr.krnorm, kr.round6), at the golden matrices and at the
shapes the GPU file uses, and every input maker is checked to contain what its name promises (the
one-directional edges, the -0.0 entries, the last-column and column-64k rows, the unique maximum in
the last row, the exact half-way products), so a GPU failure there points at the kernel."""
import types

import numpy as np
import pytest
import torch

import pipeline_ref as R
from conftest import load_golden
from oracle import graph as og
from oracle import kr as okr
from oracle import sage as osg

GOLDEN = ("chr19_1mb", "chr19_500kb", "synth256")


def _golden_matrix(case):
    m = load_golden(f"graph_{case}.npz")["matrix"].copy()
    np.fill_diagonal(m, 0)
    return m


def _oracle_csr(a):
    if a.shape[0] == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return og.csr_from_matrix(a)


# ------------------------------------------------------------------------------- graph build
ALL_GRAPH_SIZES = tuple(sorted(set(R.CSR_SIZES) | set(R.WEIGHT_SIZES)))


@pytest.mark.parametrize("n,pattern", R.csr_cases(ALL_GRAPH_SIZES))
def test_csr_and_weights_match_oracle(n, pattern):
    a = R.csr_matrix(n, pattern)
    assert a.shape == (n, n)
    rp, c, val = _oracle_csr(a)
    rp2, c2 = og.set_diag(rp, c)
    rowptr, col = R.csr_self_loops(a)
    assert rowptr.dtype == np.int32 and col.dtype == np.int32
    assert np.array_equal(rowptr, rp2) and np.array_equal(col, c2) and rowptr[n] == len(col)
    if n == 0:
        return
    w, inv = R.sage_weights(a, rowptr, col)
    off = R.entry_rows(rowptr) != col
    assert R.same_bits(w[off], val) and np.all(w[~off] == 0.0)
    with np.errstate(invalid="ignore"):       # inf - inf in the 'nonfinite' rows
        assert R.same_bits(inv, osg.degree_inverse(rp, c, val, n))
    lone = np.diff(rowptr) == 1
    assert np.all(np.isinf(inv[lone])) and np.all(inv[lone] > 0)


@pytest.mark.parametrize("case", GOLDEN)
def test_csr_and_weights_match_golden(case):
    g = load_golden(f"graph_{case}.npz")
    a = _golden_matrix(case)
    rp2, c2 = og.set_diag(g["rowptr"], g["col"])
    rowptr, col = R.csr_self_loops(a)
    assert np.array_equal(rowptr, rp2) and np.array_equal(col, c2)
    _, _, val = og.csr_from_matrix(a)
    w, inv = R.sage_weights(a, rowptr, col)
    assert R.same_bits(w[R.entry_rows(rowptr) != col], val)
    assert R.same_bits(inv, osg.degree_inverse(g["rowptr"], g["col"], val, a.shape[0]))


@pytest.mark.parametrize("n", [s for s in ALL_GRAPH_SIZES if s >= 2])
def test_patterns_hold_what_they_name(n):
    deg = lambda a: np.diff(R.csr_self_loops(a)[0])
    row = lambda a, i: R.csr_self_loops(a)[1][R.csr_self_loops(a)[0][i]:R.csr_self_loops(a)[0][i + 1]]
    assert np.all(deg(R.csr_matrix(n, "zero")) == 1)
    if n <= R.FULL_MAX:
        a = R.csr_matrix(n, "full")
        assert np.all(a != 0) and np.all(deg(a) == n)
    a = R.csr_matrix(n, "asym")
    nz = a != 0
    if n >= 63:
        assert (nz & ~nz.T).any() and (np.triu(nz & ~nz.T)).any() and (np.tril(nz & ~nz.T)).any()
        both = nz & nz.T
        assert both.any() and np.all(a[both] != a.T[both])
    a = R.csr_matrix(n, "diag")
    assert np.all(np.diagonal(a) != 0)
    b = a.copy()
    np.fill_diagonal(b, 0)
    assert np.array_equal(R.csr_self_loops(a)[1], R.csr_self_loops(b)[1])
    a = R.csr_matrix(n, "negzero")
    assert (np.signbit(a) & (a == 0)).sum() > n * n // 2 and deg(a).sum() < 10 * n
    a = R.csr_matrix(n, "nonfinite")
    if n >= 63:
        assert np.isnan(a).any() and (a == np.inf).any() and (a == -np.inf).any()
    a = R.csr_matrix(n, "isolated")
    assert deg(a)[n // 2] == 1
    a = R.csr_matrix(n, "lastcol")
    assert list(row(a, 0)) == [0, n - 1] and a[n - 1, 0] == 0
    a = R.csr_matrix(n, "col64k")
    pairs = R.col64k_pairs(n)
    assert len(pairs) == 1 + (n - 1) // 64
    for r, c in pairs:
        assert list(row(a, r)) == sorted((r, c)) and list(row(a, c)) == sorted((r, c)) and a[c, r] == 0
    for p in R.CSR_PATTERNS:
        if p != "full":
            assert np.count_nonzero(R.csr_matrix(n, p)) <= max(0.01 * n * n, 9 * n)


# ------------------------------------------------------------------------------- cont2dist
HOST_C2D_SIZES = tuple(n for n in R.C2D_SIZES if n < 2049)   # 2049: the maker only (below)


def _torch_c2d(y, f):
    return og.cont2dist(torch.tensor(y), f).numpy()


@pytest.mark.parametrize("kind", R.C2D_KINDS)
@pytest.mark.parametrize("n", HOST_C2D_SIZES)
def test_cont2dist_ieee_matches_oracle(n, kind):
    """Exponents 0, 1, 2, 3, -1, -2: the numpy restatement is torch bit for bit, NaNs in the same
    places.  +-0.5: within 2 ulp (torch's float64 sqrt on the CPU is not always correctly rounded, and
    the maximum the entry is divided by carries the same step), NaNs in the same places."""
    y = R.contacts(n, kind)
    for f in R.C2D_EXACT + R.C2D_SQRT:
        ref, t = R.cont2dist_ieee(y, f), _torch_c2d(y, f)
        assert np.array_equal(np.isnan(ref), np.isnan(t)), f
        if f in R.C2D_EXACT:
            assert R.same_bits(ref, t), f
        else:
            assert int(R.ulps(ref, t).max()) <= 2, f
    if kind == "allzero":
        assert np.isnan(R.cont2dist_ieee(y, 1.0)).all() and np.isnan(R.cont2dist_ieee(y, -1.0)).all()
        one = R.cont2dist_ieee(y, 0.0)
        assert np.all(one[~np.eye(n, dtype=bool)] == 1.0) if n > 1 else np.isnan(one).all()


@pytest.mark.parametrize("kind", [k for k in R.C2D_KINDS if k != "allzero"])
@pytest.mark.parametrize("n", [n for n in R.C2D_SIZES if n >= 3])
def test_contacts_keep_the_maximum_in_the_last_row(n, kind):
    y = R.contacts(n, kind)
    pos = y[np.isfinite(y) & (y > 0)]
    assert (pos == pos.min()).sum() == 1 and y[n - 1, 0] == pos.min() == R.C2D_SMALLEST
    assert (np.abs(y[np.isfinite(y)]) >= R.C2D_LARGEST).sum() == 1 and y[n - 1, 1] == R.C2D_LARGEST
    if kind == "zeros" and n >= 255:
        assert (y == 0).mean() > 0.5
    if kind == "negzero":
        assert (np.signbit(y) & (y == 0)).any() and ((y == 0) & ~np.signbit(y)).any()
    if kind == "negative":
        assert (y < 0).any()
    if kind == "nan":
        assert np.isnan(y).any()


def test_pow_reference_rounds_once():
    """The mpmath power rounded to float64 against exactly representable cases, and the rounding mode:
    2^-53 above 1 rounds to 1 (half to even), anything more rounds up."""
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.prec = 160
    one = ctx.mpf(1)
    assert R.to_f64(one + ctx.mpf(2) ** -53) == 1.0
    assert R.to_f64(one + ctx.mpf(2) ** -53 + ctx.mpf(2) ** -100) == 1.0 + 2.0 ** -52
    assert R.to_f64(one + 3 * ctx.mpf(2) ** -53) == 1.0 + 2.0 ** -51
    x = np.array([4.0, 0.25, 1.0, 32.0, 1024.0 ** 2, 0.0, np.inf, -2.0, np.nan])
    assert R.same_bits(R.pow_correctly_rounded(x, 1.5), np.array([8.0, 0.125, 1.0, 32.0 ** 1.5, 1024.0 ** 3, 0.0,
                                                                   np.inf, np.nan, np.nan]))
    assert R.pow_correctly_rounded(np.array([32.0]), 0.4)[0] == 4.0
    assert R.same_bits(R.pow_correctly_rounded(np.array([-np.inf, -0.0]), 0.4), np.array([np.inf, 0.0]))


def test_torch_pow_distance_to_the_reference(capsys):
    """torch's own float64 pow on the CPU against the correctly rounded power, over 1 / (every pool
    value): measured, printed, and held to 1 ulp (a correctly rounded pow gives 0)."""
    x = 1.0 / R.contact_pool()
    for f in R.C2D_POW:
        cr = R.pow_correctly_rounded(x, f)
        d = R.ulps(torch.pow(torch.tensor(x), f).numpy(), cr)
        dn = R.ulps(np.power(x, f), cr)
        with capsys.disabled():
            print(f"\npow(x, {f}) over {len(x)} values: torch max {int(d.max())} ulp ({(d > 0).mean():.2%} off), "
                  f"numpy max {int(dn.max())} ulp")
        assert int(d.max()) <= 1


@pytest.mark.parametrize("kind", R.C2D_KINDS)
@pytest.mark.parametrize("n", [n for n in HOST_C2D_SIZES if n <= 257])
def test_cont2dist_hp_against_oracle(n, kind):
    """The high-precision map for 0.4 and 1.5 has torch's NaNs and special values and is within 3 ulp
    of it (1 from torch's pow of the entry, 1 from that of the maximum, the two quotients' roundings)."""
    y = R.contacts(n, kind)
    for f in R.C2D_POW:
        ref, t = R.cont2dist_hp(y, f), _torch_c2d(y, f)
        assert np.array_equal(np.isnan(ref), np.isnan(t))
        assert int(R.ulps(ref, t).max()) <= 3, f
        special = ~(np.isfinite(y) & (y > 0))
        assert R.same_bits(ref[special], t[special])
    for f in (2.0, -1.0):   # and for an exactly computable exponent it is the IEEE map but for the two roundings
        assert int(R.ulps(R.cont2dist_hp(y, f), R.cont2dist_ieee(y, f)).max()) <= 2


# ------------------------------------------------------------------------------- KR
@pytest.mark.parametrize("with_v", [False, True])
@pytest.mark.parametrize("n", R.KR_SIZES)
def test_kr_matvec_exact_is_the_oracle_expression(n, with_v):
    """r_utils.R:24/:42 as oracle.kr writes it, x * (A @ (x * p)) + v * p with NA -> 0, is within the
    summation bound of the exact value; x and p have both signs and A has NaNs."""
    a, x, p, v = R.kr_inputs(n)
    ref, bound = R.kr_matvec_exact(n, with_v)
    a0 = np.where(np.isnan(a), 0.0, a)
    w = x * (a0 @ (x * p)) + (v * p if with_v else 0.0)
    for i in range(n):
        assert abs(R.Fraction(float(w[i])) - ref[i]) <= bound[i], i
    assert (x < 0).any() or n < 3
    assert (p < 0).any() or n < 3
    if n >= 2:
        assert np.isnan(a[0, n - 1]) and a[n - 1, n - 1] != 0
    if n >= 63:
        assert np.isnan(a).sum() > 2 and all(b > 0 for b in bound)


@pytest.mark.parametrize("n", R.KR_SCALE_SIZES)
def test_kr_scale_ref_is_the_oracle_expression(n):
    a, x, ties, sens = R.kr_scale_inputs(n)
    na = np.isnan(a)
    res = x[:, None] * np.where(na, 0.0, a) * x[None, :]          # oracle.kr.krnorm :74, :76-80, :89
    res[na] = np.nan
    ref = R.kr_scale_ref(a, x)
    assert R.same_bits(ref, okr.round6(res)) and np.array_equal(np.isnan(ref), na)
    assert len(ties) == min(n, 4) ** 2
    for i, j, t in ties:
        assert ((x[i] * a[i, j]) * x[j]) * 1e6 == t and abs(t) % 1 == 0.5
        k = int(abs(t) - 0.5)
        assert ref[i, j] == np.sign(t) * (k if k % 2 == 0 else k + 1) / 1e6
    if n >= 2:
        assert {k % 2 for k in (int(abs(t) - 0.5) for _, _, t in ties)} == {0, 1}
        assert any(t < 0 for _, _, t in ties) and (res[~na] < 0).any()
    assert len(sens) == (8 if n >= 65 else 0)
    for i, j in sens:                           # the other order of the two products gives another digit
        assert ref[i, j] != np.rint((x[i] * (a[i, j] * x[j])) * 1e6) / 1e6
        assert abs(((x[i] * a[i, j]) * x[j]) * 1e6) % 1 == 0.5
    assert (n * n) % 256 != 0


@pytest.mark.parametrize("n", R.KR_E2E_SIZES)
def test_kr_oracle_converges_on_the_e2e_inputs(n):
    a = R.kr_e2e_input(n)
    assert np.array_equal(a, a.T) and np.all(np.diagonal(a) == 0)
    out, keep, info = okr.krnorm(a, return_info=True)
    assert len(keep) == n and 15 <= info["outer"] <= 30
    assert np.allclose(np.nansum(out, axis=0), 1.0, atol=1e-3)


# ------------------------------------------------------------------------------- SAGE aggregation
def test_sage_graph_is_what_the_gpu_test_names():
    rowptr, col, value = R.sage_graph()
    n = R.SAGE_N
    assert list(np.diff(rowptr)[:len(R.SAGE_DEGREES)]) == list(R.SAGE_DEGREES)
    dense = np.zeros((n, n), np.float32)
    row = R.entry_rows(rowptr)
    dense[row, col] = value
    assert np.array_equal(dense != 0, (dense != 0).T) and np.all(np.diagonal(dense) == 0)
    assert np.all(dense[row, col] != dense[col, row])             # one weight per direction
    assert R.same_bits(R.degree_inverse(rowptr, col, value, n), osg.degree_inverse(rowptr, col, value, n))
    rp2, c2, v2 = R.insert_loops(rowptr, col, value)
    orp, oc = og.set_diag(rowptr, col)
    assert np.array_equal(rp2, orp) and np.array_equal(c2, oc)
    off = R.entry_rows(rp2) != c2
    assert np.array_equal(v2[off], value) and np.all(v2[~off] == 0)
    inv = R.degree_inverse(rowptr, col, value, n)
    assert np.isinf(inv[0]) and np.isfinite(inv[np.diff(rowptr) > 0]).all()


@pytest.mark.parametrize("F", R.SAGE_F)
def test_sage_agg_ref_matches_oracle(F):
    """The fp64 sum is within the fp32 summation bound of oracle.sage's sequential fp32 aggregation
    (forward) and of its backward's index_add (the transposed product); the trunc half is
    x.long().float()."""
    rowptr, col, value = R.sage_graph()
    x = R.sage_features(F)
    assert np.isfinite(x).all() and (np.abs(x) < 1).any() and (x < 0).any() and (np.abs(x) >= 2.0 ** 24).any()
    xt = torch.tensor(x)
    ref, bound = R.sage_agg_ref(F, False)
    got = osg.sage_aggregate(xt, rowptr, col, value).numpy().astype(np.float64)
    assert np.all(np.abs(got - ref) <= bound)
    # the transposed product is the oracle's backward, d x_j = sum_i inv_i w_ij g_i, which reads row j's
    # entries only when w_ij == w_ji: tie it on the same pattern with symmetric weights
    n = R.SAGE_N
    dense = np.zeros((n, n), np.float32)
    row = R.entry_rows(rowptr)
    dense[row, col] = value
    vs = np.maximum(dense, dense.T)[row, col]
    ctx = types.SimpleNamespace(saved_tensors=(torch.tensor(rowptr), torch.tensor(col), torch.tensor(vs)))
    dx = osg._SageAggFn.backward(ctx, xt)[0].numpy().astype(np.float64)
    ref_t, bound_t = R.sage_agg_on(rowptr, col, vs, R.degree_inverse(rowptr, col, vs, n), x, True)
    assert np.all(np.abs(dx - ref_t) <= bound_t)
    assert np.array_equal(R.trunc_ref(x), xt.long().float().numpy())
    assert (ref != 0).any() and (ref[0] == 0).all() and (bound[0] == 0).all()
    ref_t, bound_t = R.sage_agg_ref(F, True)
    assert (ref_t != 0).any() and not np.array_equal(ref_t, ref)

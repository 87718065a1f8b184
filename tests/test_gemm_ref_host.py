"""CPU: tests/gemm_ref.py against torch float64, the integer family's exactness, the forms that the cases
of tests/test_gpu_gemm_edges.py reach (hicgat_gemm_form is host-only: the library answers without a GPU),
the tolerance table, and three seeded faults that the GPU file's comparison must reject."""
import functools

import numpy as np
import pytest
import torch

import gemm_ref as R

f32 = np.float32
FAMILIES = ("random", "integers")


@pytest.fixture(scope="module")
def lib():
    from hicgat import _lib
    return _lib.load()


def _shapes():
    """Every (M, N, K) whose inputs a case of the GPU file draws."""
    s = {(c.M, c.N, c.K) for c in R.call_cases()}
    s |= {v[:3] for v in R.WG_SINGLE.values()} | set(R.wg16_shapes()) | set(R.ROWS_JOBS_8)
    return sorted(s)


# ------------------------------------------------------------------------------- 1. the reference
def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(b).max(initial=0.0))


@pytest.mark.parametrize("family", FAMILIES)
def test_references_equal_torch_float64(family):
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).double()
    for M, N, K in _shapes():
        opA, opB, bias, c0, db0 = R.logical(family, M, N, K)
        want = t(opA) @ t(opB) + t(bias) + t(c0)
        wantb = t(opA).abs() @ t(opB).abs() + t(bias).abs() + t(c0).abs()
        for a, b in (R.LAYOUTS if M * N < 1 << 18 else ((0, 1),)):
            A, B = R.stored(a, b, opA, opB)
            C, bound = R.gemm_ref(a, b, A, B, bias, c0)
            assert _close(C, want.numpy()) and _close(bound, wantb.numpy()), (M, N, K, a, b)
        if M * N < 1 << 18:
            dy, x = R.stored(1, 1, opA, opB)
            dW, db, wb, bb = R.wgrad_ref(dy, x, c0, db0)
            assert _close(dW, (t(dy).t() @ t(x) + t(c0)).numpy()) and _close(db, (t(dy).sum(0) + t(db0)).numpy())
            assert _close(wb, (t(dy).abs().t() @ t(x).abs() + t(c0).abs()).numpy())
            assert _close(bb, (t(dy).abs().sum(0) + t(db0).abs()).numpy())
            for b in (0, 1):
                A, B = R.stored(0, b, opA, opB)
                C, Cr, bound = R.rows_ref(b, A, B, bias)
                assert _close(C, (t(opA) @ t(opB) + t(bias)).numpy()) and _close(Cr, torch.relu(t(opA) @ t(opB) + t(bias)).numpy())


def test_integer_family_partial_sums_stay_below_2_24():
    """|any partial sum, in any order| <= bound: the bound itself below 2^24 keeps every fp32 partial sum
    exact; and the inputs are integers of magnitude <= 4."""
    for M, N, K in _shapes():
        opA, opB, bias, c0, db0 = R.logical("integers", M, N, K)
        for v in (opA, opB, bias, c0, db0):
            assert np.array_equal(v, np.round(v)) and np.abs(v).max(initial=0) <= 4
        _, bound = R.gemm_ref(0, 1, opA, opB, bias, c0)
        _, _, _, bb = R.wgrad_ref(*R.stored(1, 1, opA, opB), c0, db0)
        assert bound.max() <= 16 * K + 8 < 2 ** 24 and bb.max() <= 4 * K + 4, (M, N, K)
        got = R.rendition32(0, 1, opA, opB, bias, c0, splits=3) if M * N < 1 << 18 else None
        if got is not None:
            assert R.accept("integers", "C_split", got, *R.gemm_ref(0, 1, opA, opB, bias, c0))


# ------------------------------------------------------------------------------- 2. forms
def _query(lib, c):
    """hicgat_gemm_form for the case, with synthetic addresses of the case's alignment."""
    _, _, lda, _, _, ldb = R.lds(c)
    A = 0x10000 + 4 * (c.a_col + c.a_off)
    return lib.hicgat_gemm_form(c.a_km, c.b_km, c.M, c.N, c.K, A, lda, 0x800000, ldb, c.splits, c.impl,
                                0 if c.with_db is None else c.with_db)


def test_every_case_reaches_the_form_it_names(lib):
    cases = R.call_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        assert R.form_name(_query(lib, c)) == c.form, c


def test_the_cases_reach_every_form_gemm_hip_can_launch(lib):
    reached = {}
    for c in R.call_cases():
        reached.setdefault((R.form_name(_query(lib, c)), c.a_km, c.b_km), c.name)
    for k in R.ALL_FORMS:
        print(f"{k[0]:32s} layout ({k[1]}, {k[2]})  <- {reached.get(k)}")
    assert sorted(reached) == R.ALL_FORMS, (set(R.ALL_FORMS) ^ set(reached))
    assert len(R.ALL_FORMS) == 33
    # both sides of a split reach every gemm_kernel tile x layout x staging
    for sp in (False, True):
        got = {(R.form_name(_query(lib, c)), c.a_km, c.b_km) for c in R.kernel_cases() if (c.splits > 1) == sp}
        assert {k for k in R.ALL_FORMS if k[0].startswith("gemm_kernel") and "cs" not in k[0]} <= got


def test_grouped_jobs_take_the_staging_they_name(lib):
    """The per-job ``vec`` of hicgat_param_grads_grouped is the VEC bit of the weight-gradient layout."""
    vec = lambda M, N, K: bool(lib.hicgat_gemm_form(1, 1, M, N, K, 0x10000, M, 0x800000, N, 1, R.F32, 1) & 16)
    for name, (M, N, K, _t, _s, v) in R.WG_SINGLE.items():
        assert vec(M, N, K) == v, name
    assert [vec(*s) for s in R.wg16_shapes()] == [i % 4 != 3 for i in range(16)]
    tiles = [-(-M // 128) * -(-N // 128) for M, N, _ in R.wg16_shapes()]
    assert len(set(tiles)) >= 8 and min(tiles) == 1


def test_query_refuses_what_the_calls_refuse(lib):
    q = lambda *a: lib.hicgat_gemm_form(*a)
    ok = (0, 0, 64, 64, 16, 0x1000, 16, 0x2000, 16, 1, 0, 0)
    assert R.form_name(q(*ok)) == "gemm_kernel 64x64 vec"
    bad = lambda k, v: q(*[v if i == k else x for i, x in enumerate(ok)])
    assert bad(10, 2) == -3 and bad(10, 7) == -1                    # impl X3, impl unknown
    assert bad(2, -1) == bad(3, -1) == bad(4, -1) == bad(9, 0) == -1
    assert bad(5, None) == bad(7, None) == -1 and bad(11, 1) == -1   # NULL operand; db outside the (1, 1) layout
    assert bad(2, 0) == bad(3, 0) == 0                              # no launch


# ------------------------------------------------------------------------------- 3. tolerances
def _round_up_2(v):
    e = int(np.floor(np.log10(v)))
    return float(np.ceil(v / 10.0 ** (e - 1) - 1e-9) * 10.0 ** (e - 1))


@functools.lru_cache(maxsize=None)
def _measured():
    """quantity -> the largest error / bound of rendition32 over the quantity's ``random`` cases (bias
    and c0 on: the longest chain)."""
    out = {k: 0.0 for k in R.TOL}

    def put(k, got, ref, bound):
        out[k] = max(out[k], R.worst(got, ref, bound)[0])

    seen = set()
    for c in R.call_cases():
        key = (c.M, c.N, c.K, c.splits, c.with_db is not None)
        if key in seen:
            continue
        seen.add(key)
        opA, opB, bias, c0, db0 = R.logical("random", c.M, c.N, c.K)
        if c.with_db is None:
            put("C" if c.splits == 1 else "C_split", R.rendition32(0, 1, opA, opB, bias, c0, c.splits),
                *R.gemm_ref(0, 1, opA, opB, bias, c0))
        else:
            dy, x = R.stored(1, 1, opA, opB)
            dW, db, wb, bb = R.wgrad_ref(dy, x, c0, db0)
            put("dW", R.rendition32(1, 1, dy, x, None, c0, c.splits), dW, wb)
            put("db", R.colsum32(dy, db0, c.splits), db, bb)
    for M, N, K in [v[:3] for v in R.WG_SINGLE.values()] + R.wg16_shapes():
        opA, opB, _, c0, db0 = R.logical("random", M, N, K)
        dy, x = R.stored(1, 1, opA, opB)
        dW, db, wb, bb = R.wgrad_ref(dy, x, c0, db0)
        sp = -(-K // R.WG_KCHUNK)
        put("dW", R.rendition32(1, 1, dy, x, None, c0, sp, R.WG_KCHUNK), dW, wb)
        put("db", R.colsum32(dy, db0, sp, R.WG_KCHUNK), db, bb)
    for M, N, K in R.ROWS_JOBS_8:
        opA, opB, bias, _, _ = R.logical("random", M, N, K)
        for sp in R.ROWS_SPLITS:
            put("rows_C", R.rendition32(0, 1, opA, opB, bias, None, sp), *R.gemm_ref(0, 1, opA, opB, bias))
    return out


def test_tolerance_table():
    """gemm_ref.TOL is 8 x the fp32 rendition's largest error / bound, floor 2^-22, rounded up to two
    digits.  Printed, so the GPU file's docstring can be checked against it."""
    meas = _measured()
    for k, v in meas.items():
        want = _round_up_2(max(8 * v, R.FLOOR))
        print(f"{k:8s} fp32 rendition {v:.3e}  ->  tolerance {want:.1e}  (table {R.TOL[k]:.1e})")
    for k, v in meas.items():
        assert np.isclose(R.TOL[k], _round_up_2(max(8 * v, R.FLOOR)), rtol=1e-6), (k, v, R.TOL[k])


# ------------------------------------------------------------------------------- 4. a wrong kernel fails
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("fault,shape,splits,quantity", [
    ("drop_last_k", (68, 132, 20), 1, "C"),         # the second stage of 4 rows loses its last k
    ("drop_last_k", (132, 132, 100), 3, "C_split"),  # the last chunk, 4 deep
    ("skip_last_row", (65, 129, 16), 1, "C"),       # the partial row tile of 1 row
    ("skip_last_row", (1761, 2048, 16), 1, "C"),    # the tall kernel's last row tile of 1 row
    ("ghost_slab", (68, 68, 40), 5, "C_split"),     # a trailing empty chunk's slab is not zero
])
def test_seeded_faults_are_rejected(family, fault, shape, splits, quantity):
    """The comparison the GPU file uses (gemm_ref.accept) passes the fp32 rendition and rejects each of
    three defects seeded into it -- with bias and c0 on, the weakest position for the check."""
    opA, opB, bias, c0, _ = R.logical(family, *shape)
    if shape[0] > 1024:          # the rows that matter: the last row tile (the rendition is per element)
        opA, c0 = opA[-161:], c0[-161:]
    ref, bound = R.gemm_ref(0, 1, opA, opB, bias, c0)
    assert R.accept(family, quantity, R.rendition32(0, 1, opA, opB, bias, c0, splits), ref, bound)
    assert not R.accept(family, quantity, R.rendition32(0, 1, opA, opB, bias, c0, splits, fault=fault), ref, bound)

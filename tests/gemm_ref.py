"""Float64 restatements of the GEMM family (csrc/gemm.hip, csrc/gemm_tall.hip, csrc/gemm_wgrad.hip and the
two grouped launches; contracts from include/hicgat.h), the reference's own sequential fp32 rendition, and
the case tables that tests/test_gpu_gemm_edges.py (GPU) and tests/test_gemm_ref_host.py (CPU) share.

  gemm_ref     C = op(A) op(B) (+ bias) (+ c0), bound = sum_k |a_k b_k| + |bias| + |c0| per element
  wgrad_ref    dW = dy^T x (+ dW0), db = column sums of dy (+ db0), each with its bound
  rows_ref     gemm_ref of the (0, b_km) layouts with relu(C) beside C
  rendition32  the same sums in plain fp32: sequential in k, the K chunks of a split formed separately and
               added in split order, then bias, then c0 (the host file measures TOL from it, and seeds
               its faults through ``fault``)

Inputs are fp32 values, rounded once; the reference takes them as rounded.  Two families:
  random    standard normal
  integers  uniform integers in [-4, 4] for operands, bias and c0 alike: every product is an integer of
            magnitude <= 16 and every partial sum, in any order, an integer of magnitude <= 16 K + 8 < 2^24,
            so fp32 holds each exactly and the fp32 result must equal the float64 one bit for bit whatever
            the tile, split or stage order (the host file asserts the 2^24 from the bounds).  Exact zeros
            then make the relu copy's decision well defined.
A case's operands are one logical pair op(A) [M, K], op(B) [K, N] per (family, M, N, K), stored in the
layout the case asks for: cases of one shape share their reference.

Errors are judged per element against ``bound`` (xagg_ref.ratio / worst), tolerances are TOL below.
"""
import collections
import functools

import numpy as np

from xagg_ref import FLOOR, SENT32, passes, ratio, same_bits, worst, xcd_remap  # noqa: F401  (shared, not copied)

f32 = np.float32
GK = 16                      # the K-step of every kernel of the family
AUTO, F32 = 0, 1             # include/hicgat.h HICGAT_GEMM_AUTO / HICGAT_GEMM_F32

# Tolerances per compared quantity, as error / bound: 8 x the largest ratio of rendition32 against the
# float64 reference over the quantity's ``random`` cases (floor 2^-22), rounded up to two digits.  Measured
# by tests/test_gemm_ref_host.py::test_tolerance_table, which fails when this table is not that.
TOL = {"C": 3.1e-6, "C_split": 1.5e-6, "dW": 3.1e-6, "db": 1.3e-6, "rows_C": 1.7e-6}


def tol(quantity):
    return TOL[quantity]


def accept(family, quantity, got, ref, bound):
    """The one comparison of the GPU file: ``integers`` bit for bit against the float64 result (which fp32
    holds exactly), ``random`` every element within tol(quantity) of its bound."""
    if family == "integers":   # ref + 0.0: a float64 sum of -0.0 products alone is +0.0 here, as a sum begun at +0.0 gives it
        return same_bits(np.asarray(got, f32), (np.asarray(ref, np.float64) + 0.0).astype(f32))
    return passes(got, ref, bound, tol(quantity))


# ------------------------------------------------------------------------------- forms (hicgat_gemm_form)
_KERNELS = {1: "gemm_kernel", 2: "tall", 3: "ring"}
_TILES = {0: "64x64", 1: "64x128", 2: "128x128", 3: "160x128"}


def form_name(code):
    """include/hicgat.h HICGAT_GEMM_FORM_* bits -> 'gemm_kernel 64x128 vec db' and the like."""
    if code <= 0:
        return {0: "none", -1: "EINVAL", -3: "EUNSUPPORTED"}.get(code, str(code))
    parts = [_KERNELS[code & 3], _TILES[(code >> 2) & 3], "vec" if code & 16 else "scalar"]
    return " ".join(parts + (["db"] if code & 32 else []) + (["cs"] if code & 64 else []))


def kernel_form(tile, a_km, b_km, vec, cs=False):
    """The form string of gemm_kernel on ``tile`` in this layout: float4 staging is double-buffered in
    the (0, 1) layout only."""
    return " ".join(["gemm_kernel", tile, "vec" if vec else "scalar"] + (["db"] if vec and not a_km and b_km else [])
                    + (["cs"] if cs else []))


# ------------------------------------------------------------------------------- inputs
def _draw(rng, family, *shape):
    if family == "integers":
        return rng.integers(-4, 5, shape).astype(f32)
    return rng.standard_normal(shape).astype(f32)


@functools.lru_cache(maxsize=6)
def logical(family, M, N, K):
    """op(A) [M, K], op(B) [K, N], bias [N], c0 [M, N], db0 [M] (fp32)."""
    rng = np.random.default_rng([{"random": 1, "integers": 2}[family], M, N, K])
    return (_draw(rng, family, M, K), _draw(rng, family, K, N), _draw(rng, family, N), _draw(rng, family, M, N),
            _draw(rng, family, M))


def stored(a_km, b_km, opA, opB):
    """The operands as the call receives them: A [K, M] if a_km else [M, K]; B [K, N] if b_km else [N, K]."""
    return (np.ascontiguousarray(opA.T) if a_km else opA), (opB if b_km else np.ascontiguousarray(opB.T))


# ------------------------------------------------------------------------------- float64 references
def _f64(a):
    return np.asarray(a, np.float64)


def _ops(a_km, b_km, A, B, dt):
    A, B = np.asarray(A).astype(dt, copy=False), np.asarray(B).astype(dt, copy=False)
    return (A.T if a_km else A), (B if b_km else B.T)


def with_terms(C, bound, bias=None, c0=None):
    """(C + bias + c0, bound + |bias| + |c0|): the addends of the epilogue."""
    if bias is not None:
        C, bound = C + _f64(bias)[None], bound + np.abs(_f64(bias))[None]
    if c0 is not None:
        C, bound = C + _f64(c0), bound + np.abs(_f64(c0))
    return C, bound


def gemm_ref(a_km, b_km, A, B, bias=None, c0=None):
    """(C, bound) in float64 from the operands as stored."""
    a, b = _ops(a_km, b_km, A, B, np.float64)
    return with_terms(a @ b, np.abs(a) @ np.abs(b), bias, c0)


def wgrad_ref(dy, x, dW0=None, db0=None):
    """(dW [M, N], db [M], dW bound, db bound) for dy [K, M], x [K, N]."""
    dW, wb = gemm_ref(1, 1, dy, x, None, dW0)
    d = _f64(dy)
    db, bb = d.sum(0), np.abs(d).sum(0)
    if db0 is not None:
        db, bb = db + _f64(db0), bb + np.abs(_f64(db0))
    return dW, db, wb, bb


def rows_ref(b_km, A, B, bias=None):
    """(C, relu(C), bound) of a job of hicgat_gemm_rows_grouped."""
    C, bound = gemm_ref(0, b_km, A, B, bias)
    return C, np.maximum(C, 0.0), bound


# ------------------------------------------------------------------------------- the fp32 rendition
def kchunk_of(K, splits):
    """The K-chunk depth of a split launch (launch<> / hicgat_gemm_rows_grouped): whole 16-deep stages."""
    return -(-(-(-K // splits)) // GK) * GK


FAULTS = ("drop_last_k", "skip_last_row", "ghost_slab")


def rendition32(a_km, b_km, A, B, bias=None, c0=None, splits=1, kchunk=None, fault=None):
    """op(A) op(B) (+ bias) (+ c0) in plain fp32: each chunk [z kchunk, min(K, (z + 1) kchunk)) summed
    sequentially in k (product rounded, then added), the chunks added in split order, then bias, then c0.
    ``fault`` (host file only) seeds one defect of the kind a tile kernel has at an edge:
      drop_last_k    the last k of a ragged last stage (K % 16 != 0) is left out
      skip_last_row  the last row of the output (a partial row tile) is not written: it keeps c0 (or 0)
      ghost_slab     a trailing empty chunk's slab holds the first chunk's values instead of zeros."""
    assert fault in (None,) + FAULTS
    a, b = _ops(a_km, b_km, A, B, f32)
    (M, K), N = a.shape, b.shape[1]
    kchunk = kchunk_of(K, splits) if kchunk is None else kchunk
    last = K - 1 if (fault == "drop_last_k" and K % GK) else K
    slabs = []
    for z in range(splits):
        acc = np.zeros((M, N), f32)
        for k in range(z * kchunk, min(last, (z + 1) * kchunk)):
            acc += a[:, k, None] * b[None, k, :]
        if fault == "ghost_slab" and z * kchunk >= K and z > 0:
            acc = slabs[0].copy()
        slabs.append(acc)
    out = slabs[0]
    for s in slabs[1:]:
        out = out + s
    if bias is not None:
        out = out + np.asarray(bias, f32)[None]
    if c0 is not None:
        out = out + np.asarray(c0, f32)
    if fault == "skip_last_row":
        out[M - 1] = 0 if c0 is None else np.asarray(c0, f32)[M - 1]
    return out


def colsum32(dy, db0=None, splits=1, kchunk=None):
    """db of the CS kernels in plain fp32: per chunk sequential in k, chunks in split order, then db0."""
    dy = np.asarray(dy, f32)
    K = dy.shape[0]
    kchunk = kchunk_of(K, splits) if kchunk is None else kchunk
    out = None
    for z in range(splits):
        acc = np.zeros(dy.shape[1], f32)
        for k in range(z * kchunk, min(K, (z + 1) * kchunk)):
            acc += dy[k]
        out = acc if out is None else out + acc
    return out if db0 is None else out + np.asarray(db0, f32)


# ------------------------------------------------------------------------------- cases: hicgat_gemm / _wgrad
# One call shape.  lda_pad / ldb_pad: leading dimension minus the row length; a_col: A starts this many
# floats into each row of a wider array (lda grows by it); a_off: the A pointer this many floats off a
# 16-byte boundary; with_db: a hicgat_gemm_wgrad call with db (None: a hicgat_gemm call).  ``form``: the
# form the case is there to reach, as form_name() spells it.  bias, accumulate and ldc do not move the
# form: the GPU file runs every case with each.
Case = collections.namedtuple("Case", "name a_km b_km M N K splits impl lda_pad ldb_pad a_col a_off with_db form")


def _case(name, a_km, b_km, M, N, K, form, splits=1, impl=AUTO, lda_pad=0, ldb_pad=0, a_col=0, a_off=0, with_db=None):
    return Case(name, a_km, b_km, M, N, K, splits, impl, lda_pad, ldb_pad, a_col, a_off, with_db, form)


def lds(c):
    """(rows of A, row length of A, lda, rows of B, row length of B, ldb) of the arrays the call reads."""
    ra, ca = (c.K, c.M) if c.a_km else (c.M, c.K)
    rb, cb = (c.K, c.N) if c.b_km else (c.N, c.K)
    return ra, ca, c.a_col + ca + c.lda_pad, rb, cb, cb + c.ldb_pad


TALL_SHAPES = ((1761, 2048), (1919, 2048), (1920, 2048), (10241, 384))   # last row tile 1 / 159 / 160 rows; 195 tiles
TALL_K = (16, 32, 48, 64, 80)                                            # 1 .. 5 stages on a 3-slot ring


def tall_cases():
    """The 160 x 128 LDS-DMA kernel: M >= 1024 and ceil(M / 160) (N / 128) >= 192, a_kmajor = 0, splits = 1."""
    out = []
    for (M, N), K, b in ((s, k, b) for s in TALL_SHAPES for k in TALL_K for b in (0, 1)):
        out.append(_case(f"tall_{M}x{N}_k{K}_b{b}", 0, b, M, N, K, "tall 160x128 vec"))
    for b in (0, 1):
        out.append(_case(f"tall_lda_b{b}", 0, b, 1761, 2048, 48, "tall 160x128 vec", lda_pad=8))
        out.append(_case(f"tall_acol_b{b}", 0, b, 1761, 2048, 48, "tall 160x128 vec", lda_pad=4, a_col=4))
        # one side of the border (176 tiles) and every decline, on the tile each lands on
        out.append(_case(f"border_1760_b{b}", 0, b, 1760, 2048, 16, kernel_form("64x128", 0, b, True)))
        out.append(_case(f"decline_k24_b{b}", 0, b, 1761, 2048, 24, kernel_form("64x128", 0, b, True)))
        out.append(_case(f"decline_lda_b{b}", 0, b, 1761, 2048, 16, kernel_form("64x128", 0, b, False), lda_pad=1))
        out.append(_case(f"decline_aoff_b{b}", 0, b, 1761, 2048, 16, kernel_form("64x128", 0, b, False), a_off=1))
        out.append(_case(f"decline_n2052_b{b}", 0, b, 1761, 2052, 16, kernel_form("64x128", 0, b, True)))
    return out


# tile -> ((M, N) with float4 staging ...), ((M, N) with scalar staging ...): one step past a tile
KERNEL_SHAPES = {"128x128": (((132, 132),), ((129, 131),)),
                 "64x128": (((68, 132), (1028, 128)), ((65, 129),)),
                 "64x64": (((68, 68),), ((65, 67), (5, 1)))}
K_VEC, K_SCALAR = (4, 16, 20, 32, 36), (1, 3, 4, 16, 20, 36)     # 20: a second stage of 4 rows; 32: two whole stages
K_SPLIT = ((100, 3), (40, 5))                                    # kchunk 48, last chunk 4 deep; kchunk 16, two empty chunks
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))


def dims_allow_vec(a_km, b_km, M, N, K):
    """Whether the row lengths of both operands are multiples of 4 (the case's intent; the host file
    holds the library to it through hicgat_gemm_form)."""
    return (M if a_km else K) % 4 == 0 and (N if b_km else K) % 4 == 0


def kernel_cases():
    """gemm_kernel through hicgat_gemm: tile x layout x staging x (splits 1, > 1)."""
    out = []
    for tile, (vs, ss) in KERNEL_SHAPES.items():
        for (a, b) in LAYOUTS:
            for vec, shapes, ks in ((True, vs, K_VEC), (False, ss, K_SCALAR)):
                for (M, N) in shapes:
                    form = kernel_form(tile, a, b, vec)
                    for K, sp in [(K, 1) for K in ks] + list(K_SPLIT):
                        # the odd M or N of a scalar shape is not in a row of the (0, 0) operands (nor M in
                        # (0, 1)'s A ...): where the dimensions alone allow float4, an odd lda keeps it scalar
                        pad = 0 if vec or not dims_allow_vec(a, b, M, N, K) else 1
                        out.append(_case(f"k_{M}x{N}_k{K}s{sp}_{a}{b}", a, b, M, N, K, form, splits=sp, lda_pad=pad))
    for (a, b) in LAYOUTS:   # scalar staging by an odd leading dimension / a pointer 4 bytes off, dimensions multiples of 4
        for K, sp in ((16, 1), (100, 3)):
            out.append(_case(f"k_oddld_k{K}_{a}{b}", a, b, 68, 132, K, kernel_form("64x128", a, b, False), splits=sp, lda_pad=1))
            out.append(_case(f"k_oddldb_k{K}_{a}{b}", a, b, 68, 132, K, kernel_form("64x128", a, b, False), splits=sp, ldb_pad=3))
            out.append(_case(f"k_aoff_k{K}_{a}{b}", a, b, 68, 132, K, kernel_form("64x128", a, b, False), splits=sp, a_off=1))
    # the LDS-DMA ring kernel behind the same entry (AUTO, whole 128 x 128 tiles, K split), and F32 beside it
    for K, sp in K_SPLIT:
        out.append(_case(f"ring_k{K}s{sp}", 1, 1, 128, 256, K, "ring 128x128 vec", splits=sp))
        out.append(_case(f"ring_f32_k{K}s{sp}", 1, 1, 128, 256, K, kernel_form("128x128", 1, 1, True), splits=sp, impl=F32))
    return out


WGRAD_SHAPES = (("128x128", 132, 132), ("64x128", 68, 132), ("64x128", 1028, 128), ("64x64", 68, 68), ("64x64", 3, 64))


def wgrad_cases():
    """hicgat_gemm_wgrad: the CS form on all three tiles, float4 and scalar staging (M = 3 cannot be read
    as float4: scalar only; the others turn scalar by an odd ldy), splits 1 and 3 at K = 100, db given and
    NULL.  accumulate and lddw (= N, > N) are the GPU file's loops."""
    out = []
    for tile, M, N in WGRAD_SHAPES:
        for vec in ((True, False) if M % 4 == 0 else (False,)):
            pad = 0 if (vec or M % 4) else 1
            for sp in (1, 3):
                for db in (1, 0):
                    out.append(_case(f"w_{M}x{N}_{'v' if vec else 's'}_s{sp}_db{db}", 1, 1, M, N, 100,
                                     kernel_form(tile, 1, 1, vec, cs=bool(db)), splits=sp, impl=F32, lda_pad=pad, with_db=db))
    return out


def call_cases():
    return tall_cases() + kernel_cases() + wgrad_cases()


# Every form gemm.hip can launch behind hicgat_gemm / hicgat_gemm_wgrad, as (form, a_kmajor, b_kmajor):
# gemm_kernel<BM, BN, AK, BK, VEC, DB, CS> on three tiles, four layouts, float4 (double-buffered in the
# (0, 1) layout) or scalar staging; the CS forms of the weight-gradient layout; the tall kernel's two B
# layouts; the ring kernel.
ALL_FORMS = sorted(
    [(kernel_form(t, a, b, v), a, b) for t in KERNEL_SHAPES for (a, b) in LAYOUTS for v in (True, False)]
    + [(kernel_form(t, 1, 1, v, cs=True), 1, 1) for t in KERNEL_SHAPES for v in (True, False)]
    + [("tall 160x128 vec", 0, 0), ("tall 160x128 vec", 0, 1), ("ring 128x128 vec", 1, 1)])


# ------------------------------------------------------------------------------- cases: the grouped launches
# hicgat_param_grads_grouped, single weight jobs: name -> (M, N, K, target_wgs, splits, float4 staging)
WG_SINGLE = {
    "132x132": (132, 132, 1000, 64, 8, True),     # 8 chunks of 128, the last 104 deep
    "3x64": (3, 64, 1000, 64, 8, False),          # the scalar tile with CS: the flagship's dense3 job
    "68x512": (68, 512, 1000, 64, 8, True),
    "256x68": (256, 68, 1000, 64, 8, True),
    "k1": (68, 68, 1, 64, 1, True),
}
WG_KCHUNK = 128


def wg16_shapes():
    """16 weight jobs of different tile counts (1 .. 12 tiles, K = 150 in two chunks of 128 and 22), every
    fourth one of an odd M (scalar staging)."""
    return [(60 + 40 * i + (i % 4 == 3), 68 if i % 2 == 0 else 132, 150) for i in range(16)]


# hicgat_gemm_rows_grouped: unequal jobs (M, N, K) of one launch, and three more for the 8-job launch
ROWS_JOBS = ((1, 4, 4), (63, 124, 16), (64, 128, 20), (65, 132, 260), (130, 260, 36))
ROWS_JOBS_8 = ROWS_JOBS + ((5, 8, 8), (128, 128, 16), (1, 260, 4))
ROWS_SPLITS = (1, 3, 4)                          # 4: K = 20 leaves two trailing empty chunks (K = 4, 16: three)

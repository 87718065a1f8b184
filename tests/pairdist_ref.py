"""fp64 reference of the all-pairs distance, its backward and the fused distance losses
(csrc/pairdist.hip), in explicit formulas with no autograd, and the one builder of the input sets
that tests/test_gpu_pairdist_edges.py (GPU) and tests/test_pairdist_ref_host.py (CPU) share.

With d_ij = |c_i - c_j| (d_ii = 0 exactly), a symmetric truth T and M = N (N - 1) / 2 pairs i < j:
  moments  L = sum (d - t)^2 (contrastive: sum |d - t|), sd, sdd, sdt, st, stt over i < j, dg = sum T_ii^2
  mse      (2 L + dg) / N^2;  Pearson r of (t, d) over i < j;  contrastive 0.1 * mean_{i<j} |t - d|
  gradients, a pair at d_ij == 0 contributing nothing (torch's cdist backward masks it):
    mse          4 / N^2 * sum_j (d - t) / d * (c_i - c_j)
    contrastive  float32(0.1 / M) * sum_j sgn(d - t) / d * (c_i - c_j),  sgn(0) = 0
    cdist        sum_j (G_ij + G_ji) / d * (c_i - c_j)
and the same moments and gradient partials over a range [t0, t1) of the upper-triangle 128 x 128 tiles
in the kernel's order (tile-row I after tile-row I - 1, J = I .. nb - 1 within it).

Every array of an input set is float32-representable, so the fp64 reference and the fp32 kernels
see the same numbers.  The seeds are fixed here: test_pairdist_ref_host.py pins, per contrastive
input, that the only pairs whose sign(d - t) an fp32 rounding could decide are the designed ones.
"""
import types

import numpy as np

BT = 128
KINDS = {"mse": 0, "combined": 1, "contrastive": 2}
BG = 1.0


# ------------------------------------------------------------------------------- input sets
def _coords(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


def _dense_truth(n, seed):
    """Random symmetric target in [0.05, 2.55), zero diagonal but for two entries (the dg moment)."""
    rng = np.random.default_rng(seed)
    t = np.triu(0.05 + 2.5 * rng.random((n, n)), 1)
    t = t + t.T
    t[n // 2, n // 2] = 0.25
    t[n - 1, n - 1] = 0.5
    return t.astype(np.float32)


def _bg_truth(n, seed):
    """The background 1 off the diagonal except at a ~5 % symmetric support (as in
    tests/test_gpu_pairdist_occ.py)."""
    rng = np.random.default_rng(seed)
    mask = np.triu(rng.random((n, n)) < 0.05, 1)
    vals = 0.05 + 2.5 * rng.random((n, n))
    t = np.ones((n, n))
    t[mask] = vals[mask]
    t = np.triu(t, 1)
    t = t + t.T
    t[n // 2, n // 2] = 0.25
    return t.astype(np.float32)


def _grad(n, seed):
    return np.random.default_rng(seed).standard_normal((n, n)).astype(np.float32)   # dense, asymmetric


def _set(a, i, j, v):
    a[i, j] = a[j, i] = v


# name -> seed of the set (committed: the near-tie counts of the host test hold for these)
SEEDS = {"lds128": 1128, "lds256": 1256, "lds384": 1384, "lds129": 1129, "lds300": 1300,
         "glob58": 2058, "glob129": 2129, "glob300": 2300, "glob301": 2301,
         "coin300": 3300, "coin256": 3256, "flat129": 4129, "flat300": 4300, "big2177": 5177}
NAMES = list(SEEDS)

_cache = {}


def inputs(name):
    """The input set ``name``: ``n``, ``c`` [n, 3] fp32, and whichever of ``t`` (dense symmetric
    truth), ``tb`` (background-form truth, background ``BG``) and ``g`` (upstream gradient of D) the
    set has; ``coincident`` lists its designed pairs i < j with c_i == c_j.  Built once; read-only."""
    if name in _cache:
        return _cache[name]
    seed = SEEDS[name]
    n = int(name.lstrip("abcdefghijklmnopqrstuvwxyz"))
    s = types.SimpleNamespace(name=name, n=n, c=_coords(n, seed), t=None, tb=None, g=None, coincident=[])
    if name.startswith("lds"):
        s.g = _grad(n, seed + 1)
    elif name.startswith("glob"):
        s.t = _dense_truth(n, seed + 1)
    elif name.startswith("coin"):
        # (5, 6): inside one thread's patch of the diagonal tile; {5, 6, 130, 131}: a cluster across
        # tile (0, 1); (140, n - 1): an edge tile at n = 300, the last diagonal tile at n = 256
        s.c[6] = s.c[5]
        s.c[130] = s.c[5]
        s.c[131] = s.c[5]
        s.c[n - 1] = s.c[140]
        cl = [5, 6, 130, 131]
        s.coincident = [(a, b) for k, a in enumerate(cl) for b in cl[k + 1:]] + [(140, n - 1)]
        s.g = _grad(n, seed + 1)
        if n == 300:
            s.t = _dense_truth(n, seed + 2)
            _set(s.t, 5, 130, 0.0)            # d == t == 0: sgn(0)
            assert s.t[5, 6] != 0.0
            s.tb = _bg_truth(n, seed + 3)
            _set(s.tb, 5, 130, 0.0)           # a support entry at a coincident pair, d == t == 0
            _set(s.tb, 5, 6, 0.75)            # a support entry (t != bg) at a coincident pair
            _set(s.tb, 140, n - 1, BG)        # a background pair at a coincident pair
    elif name.startswith("flat"):
        s.c[:] = s.c[0]
        s.coincident = [(a, b) for a in range(n) for b in range(a + 1, n)]
        s.t = _dense_truth(n, seed + 2)
        s.tb = _bg_truth(n, seed + 3)
    elif name.startswith("big"):
        s.t = _dense_truth(n, seed + 1)
        s.g = _grad(n, seed + 2)
    for a in (s.c, s.t, s.tb, s.g):
        if a is not None:
            a.setflags(write=False)
    _cache[name] = s
    return s


def designed_zero_ties(s, t):
    """Designed coincident pairs of ``s`` whose target in ``t`` is 0 (d == t == 0)."""
    return sum(1 for (a, b) in s.coincident if t[a, b] == 0.0)


# ------------------------------------------------------------------------------- the reference
def _f64(a):
    return np.asarray(a, np.float64)


def _deltas(c):
    c = _f64(c)
    return [c[:, k][:, None] - c[:, k][None, :] for k in range(3)]


def dist(c):
    """D [N, N] fp64; the diagonal (and every coincident pair) exactly 0."""
    dx, dy, dz = _deltas(c)
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def _inv(D):
    out = np.zeros_like(D)
    np.divide(1.0, D, out=out, where=D > 0.0)
    return out


def _rows(W, c):
    """sum_j W_ij (c_i - c_j), [N, 3]."""
    return np.stack([(W * d).sum(1) for d in _deltas(c)], 1)


def moments(D, T, kind="combined", pairs=None, diag=None):
    """stats[0..6] = L, sd, sdd, sdt, st, stt, dg over the pairs i < j (``pairs``: a boolean upper-
    triangle selection, default all) and the diagonal entries ``diag`` (boolean [N], default all).
    ``kind`` "contrastive": L = sum |d - t| and dg = 0 (that loss has no diagonal term)."""
    n = D.shape[0]
    T = _f64(T)
    sel = np.triu(np.ones((n, n), bool), 1) if pairs is None else pairs
    d, t = D[sel], T[sel]
    tii = np.diagonal(T) if diag is None else np.diagonal(T)[diag]
    if kind == "contrastive":
        return np.array([np.abs(d - t).sum(), d.sum(), (d * d).sum(), (d * t).sum(), t.sum(), (t * t).sum(), 0.0])
    return np.array([((d - t) ** 2).sum(), d.sum(), (d * d).sum(), (d * t).sum(), t.sum(), (t * t).sum(),
                     (tii * tii).sum()])


def mse(m, n):
    return (2.0 * m[0] + m[6]) / (float(n) * float(n))


def pearson(D, T):
    """Pearson r of (t, d) over i < j from centred sums; NaN when either has no variance."""
    iu = np.triu_indices(D.shape[0], 1)
    d, t = D[iu], _f64(T)[iu]
    d, t = d - d.mean(), t - t.mean()
    vd, vt = (d * d).sum(), (t * t).sum()
    return float((d * t).sum() / np.sqrt(vd * vt)) if vd > 0.0 and vt > 0.0 else float("nan")


def contrastive(D, T):
    iu = np.triu_indices(D.shape[0], 1)
    return 0.1 * float(np.abs(_f64(T)[iu] - D[iu]).mean())


def mse_scale(n):
    return 4.0 / (float(n) * float(n))


def contrastive_scale(n):
    """float32(0.1 / M): the value autograd hands to cdist's backward from an fp32 loss."""
    return float(np.float32(0.1 / (0.5 * n * (n - 1))))


def grad_mse(c, T, D=None):
    D = dist(c) if D is None else D
    return mse_scale(len(c)) * _rows((D - _f64(T)) * _inv(D), c)


def grad_contrastive(c, T, D=None):
    D = dist(c) if D is None else D
    return contrastive_scale(len(c)) * _rows(np.sign(D - _f64(T)) * _inv(D), c)


def grad_cdist(c, G, D=None):
    D = dist(c) if D is None else D
    G = _f64(G)
    return _rows((G + G.T) * _inv(D), c)


def near_ties(D, T):
    """Boolean [N, N], off the diagonal: |d - t| <= 1e-6 max(d, |t|), the pairs whose sign(d - t) an
    fp32 rounding of d can decide (the contrastive gradient's allowance is 2 x scale for each)."""
    T = _f64(T)
    near = np.abs(D - T) <= 1e-6 * np.maximum(D, np.abs(T))
    np.fill_diagonal(near, False)
    return near


# ------------------------------------------------------------------------------- tile ranges
def num_tiles(n):
    nb = (n + BT - 1) // BT
    return nb * (nb + 1) // 2


def tri_start(I, nb):
    return I * nb - I * (I - 1) // 2


def tile_index(n):
    """[N, N] int: the upper-triangle tile number of entry (i, j), i <= j, in the kernel's order;
    -1 below the diagonal."""
    nb = (n + BT - 1) // BT
    b = np.arange(n) // BT
    I, J = b[:, None], b[None, :]
    idx = I * nb - I * (I - 1) // 2 + (J - I)
    return np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], idx, -1)


def tile_range(c, T, t0, t1, kind="combined", D=None):
    """(moments, gradient) of the tiles [t0, t1): the moments over the range's pairs i < j and the
    diagonal entries of its diagonal tiles; the gradient with each such pair's term in rows i and j
    (already scaled as the whole loss's is)."""
    n = len(c)
    D = dist(c) if D is None else D
    T = _f64(T)
    idx = tile_index(n)
    inr = (idx >= t0) & (idx < t1)
    pairs = inr & np.triu(np.ones((n, n), bool), 1)
    m = moments(D, T, kind, pairs=pairs, diag=np.diagonal(inr))
    if kind == "contrastive":
        W, scale = np.sign(D - T) * _inv(D), contrastive_scale(n)
    else:
        W, scale = (D - T) * _inv(D), mse_scale(n)
    W = W * pairs
    return m, scale * _rows(W + W.T, c)

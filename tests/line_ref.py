"""NumPy restatement of second-order LINE as include/hicgat.h "LINE" defines it (the edge list and
the tables of ``ge.LINE``, the counter-based sample stream, the model, Keras' Adam), written from
those words alone: everything the LINE tests compare against comes from here, never from the
library.  ``dtype`` selects the arithmetic of the model and the optimiser (float32 / float64)."""
import numpy as np

import philox_ref

LINE_SITE = 0x4C494E45
_LO = 0xFFFFFFFF


def edges(A, both_directions=False):
    """(head, tail, weight): networkx's undirected graph of A -- edge {i, j} when A[i, j] or A[j, i]
    is non-zero (NaN: no edge), weight A[max, min] if non-zero else A[min, max] -- each edge once as
    (u, v), u <= v, row-major; ``both_directions`` appends (v, u) of every edge with u < v."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    h, t, w = [], [], []
    for u in range(n):
        for v in range(u, n):
            lo, up = A[v, u], A[u, v]
            lo = 0.0 if np.isnan(lo) else lo
            up = 0.0 if np.isnan(up) else up
            if lo != 0 or up != 0:
                h.append(u)
                t.append(v)
                w.append(lo if lo != 0 else up)
    if both_directions:
        extra = [(b, a, x) for a, b, x in zip(h, t, w) if a != b]
        h += [e[0] for e in extra]
        t += [e[1] for e in extra]
        w += [e[2] for e in extra]
    return np.array(h, dtype=np.int64), np.array(t, dtype=np.int64), np.array(w, dtype=np.float64)


def node_probs(head, w, n):
    deg = np.zeros(n)
    for u, x in zip(head, w):
        deg[u] += x
    p = deg ** 0.75
    return p / p.sum()


def edge_probs(w):
    return np.asarray(w, dtype=np.float64) / np.sum(w)


def alias_table(p):
    """The standard alias construction in float64; (accept float32, alias int32)."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    q = p * n
    accept, alias = np.ones(n), np.arange(n)
    small = [i for i in range(n) if 0 < q[i] < 1.0] + [i for i in range(n) if q[i] == 0]
    large = [i for i in range(n) if q[i] >= 1.0]
    while small and large:
        s, l = small.pop(), large.pop()
        accept[s], alias[s] = q[s], l
        q[l] = q[l] - (1.0 - q[s])
        (small if q[l] < 1.0 else large).append(l)
    return accept.astype(np.float32), alias.astype(np.int32)


def implied(accept, alias):
    """The distribution an (accept, alias) pair samples."""
    n = len(accept)
    p = np.zeros(n)
    for i in range(n):
        p[i] += float(accept[i]) / n
        p[alias[i]] += (1.0 - float(accept[i])) / n
    return p


def steps(E, batch_size, epochs=1, times=1, negative_ratio=5):
    return epochs * (((E * (1 + negative_ratio) - 1) // batch_size + 1) * times)


def _words(seed, step, nslots):
    j = np.arange(nslots, dtype=np.uint64)
    return philox_ref.philox4x32_10([j, np.full_like(j, step & _LO), np.full_like(j, (step >> 32) & _LO),
                                     np.full_like(j, LINE_SITE)], (seed & _LO, (seed >> 32) & _LO))


def _uniform(w):
    return ((w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def permutations(E, seed, n_pass):
    rng = np.random.default_rng(seed)
    return [rng.permutation(E) for _ in range(n_pass)]


def batch(step, head, tail, edge_tab, node_tab, n, batch_size, negative_ratio, seed, perms):
    """(h, t, y) int64 arrays of step ``step`` of the stream."""
    E, R = len(head), 1 + negative_ratio
    chunks = -(-E // batch_size)
    p, r = divmod(step, chunks * R)
    c, b = divmod(r, R)
    ln = min(batch_size, E - c * batch_size)
    ea, el = edge_tab
    na, nl = node_tab
    i = np.asarray(perms[p][c * batch_size:c * batch_size + ln], dtype=np.int64)
    u = _uniform(_words(seed, step - b, ln)[0])
    i = np.where(u >= ea[i], el[i].astype(np.int64), i)
    h = np.asarray(head)[i].astype(np.int64)
    if b == 0:
        return h, np.asarray(tail)[i].astype(np.int64), np.ones(ln, dtype=np.int64)
    w = _words(seed, step, ln)
    k = ((w[0] * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    t = np.where(_uniform(w[1]) < na[k], k, nl[k].astype(np.int64))
    return h, t, -np.ones(ln, dtype=np.int64)


def train(U, C, head, tail, edge_tab, node_tab, batch_size, negative_ratio, seed, step_begin, step_end,
          dtype=np.float64, lr=1e-3, betas=(0.9, 0.999), eps=1e-7, form="keras", state=None):
    """Steps [step_begin, step_end) from the tables (U, C); returns (U, C, state) in ``dtype``.
    ``form="torch"`` is torch.optim.Adam's update instead (for the test that tells the two apart)."""
    dt = np.dtype(dtype).type
    U, C = np.array(U, dtype=dt), np.array(C, dtype=dt)
    n = U.shape[0]
    E, R = len(head), 1 + negative_ratio
    n_pass = (max(step_end, 1) - 1) // (-(-E // batch_size) * R) + 1
    perms = permutations(E, seed, n_pass)
    if state is None:
        state = [np.zeros_like(U), np.zeros_like(U), np.zeros_like(C), np.zeros_like(C)]
    mU, vU, mC, vC = state
    b1, b2 = dt(betas[0]), dt(betas[1])
    c1, c2 = dt(1.0 - betas[0]), dt(1.0 - betas[1])
    for s in range(step_begin, step_end):
        h, t, y = batch(s, head, tail, edge_tab, node_tab, n, batch_size, negative_ratio, seed, perms)
        yf = y.astype(dt)
        sc = np.sum(U[h] * C[t], axis=1, dtype=dt)
        g = (-(yf / dt(len(h))) * (dt(1.0) / (dt(1.0) + np.exp(yf * sc)))).astype(dt)
        dU, dC = np.zeros_like(U), np.zeros_like(C)
        gu, gc = g[:, None] * C[t], g[:, None] * U[h]           # both from the pre-update tables
        for k in range(len(h)):                                  # ascending k
            dU[h[k]] += gu[k]
            dC[t[k]] += gc[k]
        tt = float(s + 1)
        for p, d, m, v in ((U, dU, mU, vU), (C, dC, mC, vC)):
            m[...] = b1 * m + c1 * d
            v[...] = b2 * v + c2 * (d * d)
            if form == "keras":
                lr_t = dt(lr * np.sqrt(1.0 - betas[1] ** tt) / (1.0 - betas[0] ** tt))
                p -= lr_t * m / (np.sqrt(v) + dt(eps))
            else:
                step_size = dt(lr / (1.0 - betas[0] ** tt))
                p -= step_size * m / (np.sqrt(v) / dt(np.sqrt(1.0 - betas[1] ** tt)) + dt(eps))
    return U, C, [mU, vU, mC, vC]


def init(n, d, seed):
    """U(-0.05, 0.05) float32 tables from default_rng([seed, 1]): U first, then C."""
    rng = np.random.default_rng([int(seed), 1])
    u = rng.random((n, d), dtype=np.float32) * np.float32(0.1) - np.float32(0.05)
    c = rng.random((n, d), dtype=np.float32) * np.float32(0.1) - np.float32(0.05)
    return u, c

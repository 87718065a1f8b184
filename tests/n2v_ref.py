"""NumPy restatement of the node2vec kernels as csrc/node2vec.hip and include/hicgat.h describe them
(the counter-based RNG, the rejection-sampled walks, one skip-gram negative-sampling epoch), in
Python integers and numpy: everything the exact node2vec tests compare against comes from here,
never from the library.

Every random decision is a function of (seed, walk, step, ...) and every discrete choice an integer
or single-rounding fp32 comparison, so ``walks`` reproduces the device's walks exactly, and
``sgns_epoch`` every kept token, window, target and skip; only its float updates depend on
``dtype`` (float64: the reference; float32: the same code, to size tolerances)."""
import numpy as np

_M64 = (1 << 64) - 1
F32 = np.float32
K_MAX_ATTEMPTS = 4096            # the walk kernel's rejection cap


def splitmix(z):
    """splitmix64's output function of the 64-bit integer z."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def rng4(seed, a, b, c):
    return splitmix(seed ^ splitmix(a ^ splitmix(b ^ splitmix(c))))


def u24(r):
    """The top 24 bits of r as an fp32 in [0, 1) (exact)."""
    return F32(r >> 40) * F32(2.0 ** -24)


def _has_col(rowptr, col, r, c):
    lo, hi = int(rowptr[r]), int(rowptr[r + 1])
    while lo < hi:
        mid = (lo + hi) >> 1
        v = int(col[mid])
        if v == c:
            return True
        if v < c:
            lo = mid + 1
        else:
            hi = mid
    return False


def weighted_graph(n=14, seed=3):
    """The node2vec tests' dense weighted graph: random symmetric weights, a connecting path, a self
    loop at node 2."""
    rng = np.random.default_rng(seed)
    a = rng.random((n, n)) * (rng.random((n, n)) < 0.45) * 3 + 0.0
    a = np.triu(a, 1)
    a = a + a.T
    for i in range(n - 1):
        a[i, i + 1] = a[i + 1, i] = max(a[i, i + 1], 0.5)
    a[2, 2] = 0.8
    return a


def walk_inputs(rowptr, weight, num_walks, seed):
    """The host tables both sides of a comparison are given: (cumw, starts) -- the inclusive per-row
    cumulative edge weights (float64 sums stored as fp32) and num_walks shuffled rounds of every
    node."""
    n = len(rowptr) - 1
    cumw = np.concatenate([np.cumsum(weight[rowptr[i]:rowptr[i + 1]]) for i in range(n)] + [np.zeros(0)])
    rng = np.random.default_rng(seed)
    starts = np.concatenate([rng.permutation(n) for _ in range(num_walks)]).astype(np.int32)
    return cumw.astype(F32), starts


def walks(rowptr, col, cumw, starts, L, p, q, seed):
    """[nwalks, L] int32 walks, -1 padded.  Walk w, step t: up to K_MAX_ATTEMPTS attempts, attempt a
    drawing r = rng4(seed, w, t, a); the candidate is the first neighbour k of the current node with
    cumw[k] > u24(r) * cumw[row end] (fp32 product, binary search); the first step takes it, a later
    one accepts it when fp32(low 24 bits of r * 2^-24 * fmax) < factor, factor = 1/p back to the
    previous node, 1 for a neighbour of it, 1/q otherwise, fmax = max(1, 1/p, 1/q); after the cap
    the last candidate stands.  A node without neighbours ends the walk."""
    cumw = np.asarray(cumw, dtype=F32)
    inv_p, inv_q = F32(1) / F32(p), F32(1) / F32(q)
    fmax = max(F32(1), inv_p, inv_q)
    seed = int(seed) & _M64
    out = np.full((len(starts), L), -1, dtype=np.int32)
    for w, start in enumerate(starts):
        cur, prev = int(start), -1
        out[w, 0] = cur
        for t in range(1, L):
            b, e = int(rowptr[cur]), int(rowptr[cur + 1])
            if b == e:
                break
            tot = cumw[e - 1]
            nxt = int(col[b])
            for attempt in range(K_MAX_ATTEMPTS):
                r = rng4(seed, w, t, attempt)
                u = u24(r) * tot
                lo, hi = b, e - 1
                while lo < hi:
                    mid = (lo + hi) >> 1
                    if cumw[mid] > u:
                        hi = mid
                    else:
                        lo = mid + 1
                nxt = int(col[lo])
                if prev < 0:
                    break
                f = inv_p if nxt == prev else (F32(1) if _has_col(rowptr, col, prev, nxt) else inv_q)
                if F32(r & 0xFFFFFF) * F32(2.0 ** -24) * fmax < f:
                    break
            prev, cur = cur, nxt
            out[w, t] = cur
    return out


def kept_tokens(walk, w, keep, epoch, seed):
    """The walk's tokens that survive downsampling, in order: position pos holds a node (>= 0) and
    u24(rng4(seed, 0x5A3F + epoch, w, pos)) < keep[token]."""
    return [int(tok) for pos, tok in enumerate(walk)
            if tok >= 0 and u24(rng4(seed, 0x5A3F + epoch, w, pos)) < F32(keep[tok])]


def pair_targets(w, i, j, word, cum, V, negative, epoch, seed):
    """Targets 0 .. negative of the pair (centre i, context j): the word itself, then bisect-left
    samples of rng4(...) % cum[V - 1] in the cumulative table; a sample equal to the word is dropped
    (-1)."""
    total = int(cum[V - 1])
    tg = [word]
    for d in range(1, negative + 1):
        x = rng4(seed, 0x9D + epoch, (w << 20) | i, (j << 8) | d) % total
        lo, hi = 0, V - 1
        while lo < hi:
            mid = (lo + hi) >> 1
            if int(cum[mid]) >= x:
                hi = mid
            else:
                lo = mid + 1
        tg.append(-1 if lo == word else lo)
    return tg


def alpha_of(w, nwalks, alpha0, alpha1, epoch, epochs):
    """Walk w's learning rate, in fp32 operation by operation (the integer products are exact below
    2^24, so a fused multiply-add gives the same progress)."""
    prog = (F32(epoch) * F32(nwalks) + F32(w)) / (F32(epochs) * F32(nwalks))
    return F32(alpha0) - (F32(alpha0) - F32(alpha1)) * prog


def sgns_epoch(walks, keep, cum, V, D, window, negative, alpha0, alpha1, epoch, epochs, seed, syn0, syn1,
               dtype=np.float64, trace=None):
    """One skip-gram negative-sampling epoch over the walks in order 0 .. nwalks - 1; returns the new
    (syn0, syn1) as ``dtype`` arrays (the inputs are not changed).

    Per walk: the kept tokens s[0 .. n); per centre i the reduced window red = rng4(seed,
    0x77 + epoch, w, i) % window, contexts j in [max(0, i - window + red), min(n, i + window + 1 -
    red)) without i; per pair the targets of ``pair_targets``.  The pair's rule: l1 = syn0[s[j]] and
    every target's syn1 row are read before the pair, the dots taken from those; a target with
    |dot| >= 6 is skipped; g = (label - sigmoid(dot)) * alpha; in target order work += g * row and
    syn1[target] = row + g * l1 (a target drawn twice reads its row once: the later write wins);
    syn0[s[j]] = l1 + work comes last.

    ``trace``, a list, receives one (w, i, j, word, context, targets, dots) per pair."""
    walks = np.asarray(walks)
    nwalks = walks.shape[0]
    seed = int(seed) & _M64
    syn0 = np.array(syn0, dtype=dtype).reshape(V, D)
    syn1 = np.array(syn1, dtype=dtype).reshape(V, D)
    one = dtype(1)
    for w in range(nwalks):
        alpha = dtype(alpha_of(w, nwalks, alpha0, alpha1, epoch, epochs))
        s = kept_tokens(walks[w], w, keep, epoch, seed)
        n = len(s)
        for i in range(n):
            word = s[i]
            red = rng4(seed, 0x77 + epoch, w, i) % window
            for j in range(max(0, i - window + red), min(n, i + window + 1 - red)):
                if j == i:
                    continue
                tg = pair_targets(w, i, j, word, cum, V, negative, epoch, seed)
                l1 = syn0[s[j]].copy()
                rows = [syn1[t].copy() if t >= 0 else None for t in tg]
                dots = [dtype(np.dot(l1, r)) if r is not None else None for r in rows]
                if trace is not None:
                    trace.append((w, i, j, word, s[j], tg, dots))
                work = np.zeros(D, dtype=dtype)
                for d, t in enumerate(tg):
                    if t < 0 or dots[d] <= -6 or dots[d] >= 6:
                        continue
                    g = (dtype(1 if d == 0 else 0) - one / (one + np.exp(-dots[d]))) * alpha
                    work += g * rows[d]
                    syn1[t] = rows[d] + g * l1
                syn0[s[j]] = l1 + work
    return syn0, syn1

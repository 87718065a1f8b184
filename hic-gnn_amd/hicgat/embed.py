"""node2vec embeddings on the GPU.

Reference call (HiC_GAT_generalize_directly.py:150-155; the same at evaluate_combined_loss.py:78 and
HiC-GNN_node2vec_conversion.py:118 with other p / q / walk lengths):

    G = nx.from_numpy_matrix(matrix)
    Node2Vec(G, dimensions=512, walk_length=150, num_walks=50, p=1.75, q=0.4, workers=1, seed=42)
        .fit(window=25, min_count=1, batch_words=4)      # gensim Word2Vec, sg=1
    embeddings = [model.wv[str(node)] for node in G.nodes()]

``node2vec(matrix, ...)`` returns the [N, dimensions] embedding matrix in node order.  The walks
(``hicgat_n2v_walks``) and the skip-gram epochs (``hicgat_n2v_sgns_epoch``) run in libhicgat.so;
the host builds the weighted CSR (networkx's edge / weight rule) and gensim's vocabulary tables
(downsampling keep probabilities, unigram^0.75 negative-sampling table) from the walk counts.
Differences from the reference, by construction: the random streams of the walks and of the
skip-gram (a counter-based RNG instead of Python's / gensim's LCG) and the update order of the
concurrent skip-gram waves (``max_waves``; the reference trains with one worker) -- node2vec output
is stochastic, so no two implementations agree bit for bit.  The initial vectors are gensim 4's
(``initial_vectors``: same generator, same vocabulary order, given the walks).

``line(matrix, ...)`` is the other generator, HiC-GNN_main.py:91-96's own: second-order LINE
(``ge.LINE(G, embedding_size=512, order='second').train(batch_size, epochs)``), restated from the
package's published source (``ge`` / TensorFlow are absent: unpinned by reference vectors).  The host
builds the edge list, the alias tables and the per-pass permutations (``line_edges``, ``alias_table``,
``line_steps``: usable without a GPU); sampling and the optimiser steps run in libhicgat.so
(``hicgat_line_train``, csrc/line.hip).
"""
import numpy as np
import torch

from . import _lib

P = _lib.ptr


def graph_csr(A):
    """Sorted CSR (rowptr, col, weight) of ``networkx.from_numpy_matrix(A)``: edge {i, j} when
    A[i, j] or A[j, i] is non-zero (self loops included), weight A[max, min] if non-zero else
    A[min, max] (the undirected Graph keeps the later assignment); NaN entries are no edge."""
    A = np.nan_to_num(np.asarray(A, dtype=np.float64), nan=0.0)
    n = A.shape[0]
    lo = np.tril(A, -1)
    wl = np.where(lo != 0, lo, np.triu(A, 1).T)
    W = wl + wl.T + np.diag(np.diag(A))
    rows, cols = np.nonzero(W)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), cols.astype(np.int64), W[rows, cols]


def random_walks(A, num_walks=50, walk_length=150, p=1.75, q=0.4, seed=42, device="cuda"):
    """[num_walks * N, walk_length] int32 walks (-1 padded): num_walks rounds, each starting one walk
    from every node in a shuffled order (node2vec's ``_generate_walks``)."""
    lib = _lib.lib()
    rowptr, col, w = graph_csr(A)
    n = len(rowptr) - 1
    # inclusive per-row cumulative weights (float64 prefix sums, stored as float32)
    cs = np.cumsum(w)
    base = np.repeat(np.concatenate([[0.0], cs])[rowptr[:-1]], np.diff(rowptr))
    cumw = (cs - base).astype(np.float32)
    rng = np.random.default_rng(seed)
    starts = np.concatenate([rng.permutation(n) for _ in range(num_walks)]).astype(np.int32)
    dev = torch.device(device)
    t_rowptr = torch.tensor(rowptr, dtype=torch.int32, device=dev)
    t_col = torch.tensor(col, dtype=torch.int32, device=dev)
    t_cumw = torch.tensor(cumw if len(cumw) else np.zeros(1, np.float32), device=dev)
    t_starts = torch.tensor(starts, device=dev)
    walks = torch.empty((len(starts), walk_length), dtype=torch.int32, device=dev)
    _lib.check(lib.hicgat_n2v_walks(P(t_rowptr), P(t_col), P(t_cumw), n, P(t_starts), len(starts), walk_length,
                                    float(p), float(q), int(seed) & (2 ** 64 - 1), P(walks), _lib.stream(dev)),
               "hicgat_n2v_walks")
    return walks


def vocab_tables(counts, sample=1e-3, ns_exponent=0.75):
    """gensim 4 ``prepare_vocab`` keep probabilities and ``make_cum_table`` (domain 2^31 - 1)."""
    counts = np.asarray(counts, dtype=np.float64)
    thr = sample * counts.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = np.where(counts > 0, np.minimum((np.sqrt(counts / thr) + 1.0) * (thr / counts), 1.0), 0.0)
    pw = counts ** ns_exponent
    cum = np.round(np.cumsum(pw) / pw.sum() * (2 ** 31 - 1)).astype(np.uint32)
    return keep.astype(np.float32), cum


def initial_vectors(walks, n_words, dimensions, w2v_seed=1):
    """gensim 4's initial input vectors: ``prep_vectors`` draws ``default_rng(seed).random((V, D))``
    mapped to U(-1/D, 1/D) for the vocabulary in its order, so node n gets row rank(n).  The order:
    ``prepare_vocab`` adds the words in first-appearance order of the corpus scan (the raw vocabulary
    dict), then ``sort_by_descending_frequency`` permutes them by ``np.argsort(count)[::-1]`` --
    numpy's default (unstable) sort, reversed, so tied words are NOT in first-appearance order; the
    same expression is applied here to the same count array.  The reference's
    ``.fit(window=25, min_count=1, batch_words=4)`` passes no seed, so Word2Vec's default seed 1
    applies.  (gensim is absent here: the rule is restated from its published source, unpinned.)"""
    flat = walks.reshape(-1)
    flat = flat[flat >= 0].cpu().numpy().astype(np.int64)
    counts = np.bincount(flat, minlength=n_words)
    words, first = np.unique(flat, return_index=True)
    scan = words[np.argsort(first)]                             # first-appearance order
    order = scan[np.argsort(counts[scan])[::-1]]                # gensim 4 sort_by_descending_frequency
    init = np.random.default_rng(seed=w2v_seed).random((len(order), dimensions), dtype=np.float32)
    init *= 2.0
    init -= 1.0
    init /= dimensions
    vec = np.zeros((n_words, dimensions), dtype=np.float32)     # a node no walk visits stays 0 (not in the vocab)
    vec[order] = init
    return vec


SMALL_VOCAB = 1024


def skipgram(walks, n_words, dimensions=512, window=25, epochs=5, negative=5, alpha=0.025, min_alpha=1e-4,
             sample=1e-3, seed=42, max_waves=None, w2v_seed=1):
    """Word2Vec(sg=1, hs=0) over the walks: returns the input vectors syn0 [n_words, dimensions].
    ``max_waves`` bounds the walks trained concurrently: on a Hi-C-sized vocabulary (58 loci for
    chr19 1 mb) concurrent Hogwild writers to the same rows would lose updates, so vocabularies
    below ``SMALL_VOCAB`` words train near-sequentially (n_words // 64 walks at once); larger ones
    keep n_words // 4 walks in flight (at most 4096)."""
    lib = _lib.lib()
    dev = walks.device
    nwalks, L = walks.shape
    counts = torch.bincount(walks[walks >= 0].long(), minlength=n_words).cpu().numpy()
    keep, cum = vocab_tables(counts, sample)
    t_keep = torch.tensor(keep, device=dev)
    t_cum = torch.tensor(cum.view(np.int32), device=dev)          # uint32 bits
    syn0 = torch.tensor(initial_vectors(walks, n_words, dimensions, w2v_seed), device=dev)
    syn1 = torch.zeros_like(syn0)
    st = _lib.stream(dev)
    if max_waves is None:
        # at most one concurrent walk per 64 words: sequential, like the reference's workers=1, for
        # a Hi-C chromosome at 1 mb / 500 kb (58 / 114 loci); measured on chr19 1 mb, 4 vs 14
        # concurrent walks give the same embedding structure (common-component share 0.984 vs
        # 0.980, profiles/r03b_n2v_study.json) at 20 vs 5 s; one walk at a time, as here, takes
        # 80 s (the reference's 5 epochs over 2900 walks of 150 nodes, D = 512)
        max_waves = max(1, n_words // 64) if n_words < SMALL_VOCAB else max(1, min(4096, n_words // 4))
    for ep in range(epochs):
        _lib.check(lib.hicgat_n2v_sgns_epoch(P(walks), nwalks, L, P(t_keep), P(t_cum), n_words, dimensions, window,
                                             negative, float(alpha), float(min_alpha), ep, epochs,
                                             int(seed) & (2 ** 64 - 1), int(max_waves), P(syn0), P(syn1), st),
                   "hicgat_n2v_sgns_epoch")
    return syn0


def node2vec(matrix, dimensions=512, walk_length=150, num_walks=50, p=1.75, q=0.4, window=25, epochs=5,
             negative=5, alpha=0.025, min_alpha=1e-4, sample=1e-3, seed=42, device="cuda", max_waves=None):
    """[N, dimensions] node2vec embeddings of ``matrix`` (node order), HiC_GAT_generalize_directly.py's
    defaults."""
    walks = random_walks(matrix, num_walks, walk_length, p, q, seed, device)
    return skipgram(walks, np.asarray(matrix).shape[0], dimensions, window, epochs, negative, alpha, min_alpha,
                    sample, seed, max_waves=max_waves)


# ---- LINE (second order): HiC-GNN_main.py:91-96 ----------------------------------------------------
def line_edges(A, both_directions=False):
    """(head, tail, weight) of ``nx.from_numpy_matrix(A).edges(data=True)``: every undirected edge
    once as (u, v) with u <= v (self loops included), in row-major order of ``graph_csr``'s upper
    triangle, with ``graph_csr``'s weight.  ``ge.LINE`` trains exactly this list, head u and tail v:
    the undirected graph in ONE direction.  ``both_directions`` appends the (v, u) orientation of
    every edge with u < v (the LINE paper's treatment of an undirected edge)."""
    rowptr, col, w = graph_csr(A)
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    up = col >= row
    head, tail, w = row[up], col[up], w[up]
    if both_directions:
        off = head != tail
        head, tail, w = (np.concatenate([head, tail[off]]), np.concatenate([tail, head[off]]),
                         np.concatenate([w, w[off]]))
    return head.astype(np.int32), tail.astype(np.int32), w.astype(np.float64)


def alias_table(p):
    """(accept float32, alias int32) of the alias method for the distribution ``p`` (normalised
    here; float64 construction): entry i is drawn uniformly, kept with probability accept[i], else
    replaced by alias[i].  Zero-probability entries are paired off first, so each of them gets
    accept 0 and an alias of positive probability: it is never drawn."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    accept, alias = np.ones(n, dtype=np.float64), np.arange(n, dtype=np.int32)
    if n == 0:
        return accept.astype(np.float32), alias
    if not (np.all(p >= 0) and p.sum() > 0):
        raise ValueError("alias_table needs non-negative weights with a positive sum")
    q = p / p.sum() * n
    small = [int(i) for i in np.nonzero((q < 1.0) & (q > 0.0))[0]] + [int(i) for i in np.nonzero(q == 0.0)[0]]
    large = [int(i) for i in np.nonzero(q >= 1.0)[0]]
    while small and large:
        s, l = small.pop(), large.pop()
        accept[s], alias[s] = q[s], l
        q[l] -= 1.0 - q[s]
        (small if q[l] < 1.0 else large).append(l)
    return accept.astype(np.float32), alias      # what rounding leaves over keeps accept 1


def line_node_probs(head, w, n, power=0.75):
    """ge.LINE's negative-sampling distribution: deg[u] += w for each edge's HEAD only, p ~ deg^0.75.
    A node that heads no edge has probability 0."""
    deg = np.zeros(n, dtype=np.float64)
    np.add.at(deg, np.asarray(head, dtype=np.int64), np.asarray(w, dtype=np.float64))
    pw = deg ** power
    return pw / pw.sum() if pw.sum() > 0 else pw


def line_steps(E, batch_size, epochs=1, times=1, negative_ratio=5):
    """Batches that ``line.train(batch_size, epochs, times)`` runs:
    epochs * ((E * (1 + negative_ratio) - 1) // batch_size + 1) * times."""
    return int(epochs) * (((int(E) * (1 + int(negative_ratio)) - 1) // int(batch_size) + 1) * int(times))


def line_init(n, embedding_size, seed=42):
    """The initial (U, C) float32 tables, each U(-0.05, 0.05) (Keras' Embedding default) from
    ``default_rng([seed, 1])`` -- a generator of its own, apart from the permutations'."""
    rng = np.random.default_rng([int(seed), 1])
    u = (rng.random((n, embedding_size), dtype=np.float32) * np.float32(0.1) - np.float32(0.05))
    c = (rng.random((n, embedding_size), dtype=np.float32) * np.float32(0.1) - np.float32(0.05))
    return u, c


class Line:
    """The device state of one LINE training run over an edge list: the sample tables, the
    embedding table ``U`` (``second_emb``), the context table ``C`` and Keras-Adam's moments.
    ``train(s0, s1)`` enqueues steps [s0, s1) of the one continuous sample stream (include/hicgat.h
    "LINE"); ``samples(s0, s1)`` returns their (h, t, y).  The per-pass permutations come from
    ``default_rng(seed)`` in pass order, ``PASS_CHUNK`` passes on the device at a time."""
    PASS_CHUNK = 256

    def __init__(self, head, tail, weight, n, embedding_size=512, batch_size=1024, negative_ratio=5, seed=42,
                 device="cuda", lr=1e-3, betas=(0.9, 0.999), eps=1e-7):
        self.lib = _lib.lib()
        self.dev = torch.device(device)
        head, tail = np.asarray(head, dtype=np.int32), np.asarray(tail, dtype=np.int32)
        weight = np.asarray(weight, dtype=np.float64)
        self.E, self.N, self.D = len(head), int(n), int(embedding_size)
        self.B, self.neg, self.seed = int(batch_size), int(negative_ratio), int(seed)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        if self.B < 1:
            raise ValueError("batch_size must be >= 1")
        if self.E and (min(head.min(), tail.min()) < 0 or max(head.max(), tail.max()) >= self.N):
            raise ValueError("edge endpoints outside [0, n)")
        self.edge_accept, self.edge_alias = alias_table(weight / weight.sum()) if self.E else alias_table([])
        self.node_accept, self.node_alias = alias_table(line_node_probs(head, weight, self.N)) if self.E else alias_table([])
        T = lambda a: torch.tensor(a if len(a) else np.zeros(1, a.dtype), device=self.dev)  # noqa: E731
        self._t = [T(head), T(tail), T(self.edge_accept), T(self.edge_alias), T(self.node_accept), T(self.node_alias)]
        u, c = line_init(self.N, self.D, self.seed)
        self.U, self.C = torch.tensor(u, device=self.dev), torch.tensor(c, device=self.dev)
        self._mom = [torch.zeros_like(self.U) for _ in range(4)]
        self._ws = None
        self.steps_per_pass = -(-self.E // self.B) * (1 + self.neg) if self.E else 1
        self._rng, self._next_pass = np.random.default_rng(self.seed), 0

    def _perms(self, p0, p1):
        """[p1 - p0, E] int32 device tensor of the permutations of passes [p0, p1)."""
        if p0 < self._next_pass:                     # an earlier pass again: replay the generator
            self._rng, self._next_pass = np.random.default_rng(self.seed), 0
        while self._next_pass < p0:
            self._rng.permutation(self.E)
            self._next_pass += 1
        out = np.stack([self._rng.permutation(self.E) for _ in range(p0, p1)]).astype(np.int32)
        self._next_pass = p1
        return torch.tensor(out, device=self.dev)

    def _ranges(self, s0, s1):
        """(perm tensor, first pass, step range) pieces covering steps [s0, s1)."""
        spp = self.steps_per_pass
        while s0 < s1:
            p0 = s0 // spp
            p1 = min((s1 - 1) // spp + 1, p0 + self.PASS_CHUNK)
            e = min(s1, p1 * spp)
            yield self._perms(p0, p1), p0, p1 - p0, s0, e
            s0 = e

    def _stream_args(self, perm, p0, npass):
        h, t, ea, el, na, nl = self._t
        return [P(h), P(t), P(ea), P(el), self.E, P(na), P(nl), self.N, P(perm), p0, npass]

    def samples(self, s0, s1):
        """(h, t, y) int32 tensors [s1 - s0, batch_size]; slots past a short batch hold (-1, -1, 0)."""
        shape = (max(s1 - s0, 0), self.B)
        h = torch.full(shape, -1, dtype=torch.int32, device=self.dev)
        t = torch.full(shape, -1, dtype=torch.int32, device=self.dev)
        y = torch.zeros(shape, dtype=torch.int32, device=self.dev)
        if self.E == 0:
            return h, t, y
        for perm, p0, npass, a, b in self._ranges(s0, s1):
            _lib.check(self.lib.hicgat_line_samples(*self._stream_args(perm, p0, npass), self.B, self.neg,
                                                    self.seed & (2 ** 64 - 1), a, b, P(h[a - s0:]), P(t[a - s0:]),
                                                    P(y[a - s0:]), _lib.stream(self.dev)), "hicgat_line_samples")
        return h, t, y

    def train(self, s0, s1):
        """Enqueue steps [s0, s1) on the current stream (no host sync)."""
        if self.E == 0 or s1 <= s0:
            return self
        if self._ws is None:
            self._ws = _lib.workspace(self.lib.hicgat_line_workspace_bytes(self.D, self.B), self.dev)
        mU, vU, mC, vC = self._mom
        for perm, p0, npass, a, b in self._ranges(s0, s1):
            _lib.check(self.lib.hicgat_line_train(*self._stream_args(perm, p0, npass), self.D, self.B, self.neg,
                                                  self.seed & (2 ** 64 - 1), a, b, self.lr, self.betas[0],
                                                  self.betas[1], self.eps, P(self.U), P(self.C), P(mU), P(vU), P(mC),
                                                  P(vC), P(self._ws), self._ws.numel(), _lib.stream(self.dev)),
                       "hicgat_line_train")
        return self


def line(matrix, embedding_size=512, order="second", batch_size=1024, epochs=1, times=1, negative_ratio=5, seed=42,
         device="cuda", both_directions=False):
    """[N, embedding_size] LINE embeddings of ``matrix`` (node order): HiC-GNN_main.py:91-96,

        G = nx.from_numpy_matrix(adj)
        line = LINE(G, embedding_size=512, order='second'); line.train(batch_size, epochs, verbose=1)
        embeddings = np.asarray(list(line.get_embeddings().values()))

    with ``ge``'s defaults (negative_ratio 5, times 1, Adam(1e-3) in Keras' form).  The sampling and
    the optimiser steps run in libhicgat.so (``hicgat_line_train``); the host builds the edge list,
    the two alias tables and the per-pass permutations.  Kept from ``ge.LINE``: each undirected edge
    is trained in one direction only (head u <= tail v), the negative-sampling degrees count heads
    only, so a node that heads no edge (the highest index, an isolated locus) keeps its initial row.
    ``both_directions=True`` lists every edge both ways instead (the LINE paper's form).

    ``ge`` / TensorFlow are not installed here: the algorithm is restated from the package's
    published source and is unpinned by reference vectors; its random streams (numpy's global
    generator, Keras' initialiser) are replaced by a counter-based one, so no two implementations
    agree number for number.  Scope: ``order='second'`` only."""
    if order != "second":
        raise NotImplementedError(f"hicgat.embed.line implements order='second' only (HiC-GNN_main.py:93); "
                                  f"order={order!r} ('first' / 'all') is out of scope")
    a = np.asarray(matrix)
    head, tail, w = line_edges(a, both_directions)
    run = Line(head, tail, w, a.shape[0], embedding_size, batch_size, negative_ratio, seed, device)
    run.train(0, line_steps(len(head), batch_size, epochs, times, negative_ratio))
    return run.U


def embedding_stats(emb, truth=None):
    """Structure of an embedding matrix [N, F] (SURVEY 8(f) f4 has no reference vectors to compare):
    ``shared`` -- the share of the rows' energy in their common mean, ||mean||^2 / mean ||x_i||^2;
    ``cos_mean`` -- the mean pairwise cosine; ``locality`` -- Spearman of the pairwise distances
    of the CENTRED rows against the genomic separation |i - j| (positive: nearby loci embed nearby);
    ``truth_rho`` -- Spearman of those distances against ``truth`` (e.g. cont2dist of the contacts)."""
    from scipy.stats import spearmanr
    e = np.asarray(emb, dtype=np.float64)
    n = e.shape[0]
    mu = e.mean(0)
    shared = float(mu @ mu / np.mean(np.sum(e * e, 1)))
    u = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-30)
    iu = np.triu_indices(n, 1)
    cos = (u @ u.T)[iu]
    c = e - mu
    d = np.sqrt(np.maximum(np.sum(c * c, 1)[:, None] + np.sum(c * c, 1)[None, :] - 2 * c @ c.T, 0))[iu]
    sep = (iu[1] - iu[0]).astype(np.float64)
    out = {"shared": shared, "cos_mean": float(cos.mean()), "cos_min": float(cos.min()),
           "norm_mean": float(np.linalg.norm(e, axis=1).mean()), "locality": float(spearmanr(d, sep)[0])}
    if truth is not None:
        out["truth_rho"] = float(spearmanr(d, np.asarray(truth, dtype=np.float64)[iu])[0])
    return out

"""References for the GATConv attention weights (TEST INFRASTRUCTURE ONLY).

* ``gat_attention``     -- PyG 1.7.2 GATConv restated in torch (any dtype; the tests run it in fp64) over
                           an int64 CSR that already holds the self loops; returns (out, alpha, z) with
                           autograd, alpha [nnz, H] in CSR order.
* ``alpha_backward_np`` -- the closed-form backward of a gradient G on alpha (DESIGN.md section 3,
                           "Attention weights"), in numpy.
* ``transpose_map_np``  -- tmap[e(r, i)] = e(i, r).
* ``EntropyRef``        -- models.py:1112-1148 over ``gat_attention`` with the objective of
                           ``hicgat.GATNetHeadsChanged3LayersEmbeddingDim256Entropy.loss``.
* ``GRAPHS``            -- the small symmetric graphs of the attention tests.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn import Linear


def rows_of(rowptr):
    n = rowptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])


def gat_attention(x, W, att_l, att_r, bias, rowptr, col, negative_slope=0.2):
    n = rowptr.numel() - 1
    H, C = att_l.shape[-2], att_l.shape[-1]
    h = (x @ W.t()).view(n, H, C)
    a_l = (h * att_l.view(1, H, C)).sum(-1)
    a_r = (h * att_r.view(1, H, C)).sum(-1)
    row = rows_of(rowptr)
    z = a_l[col] + a_r[row]                                                # [nnz, H]
    e = F.leaky_relu(z, negative_slope)
    idx = row.view(-1, 1).expand_as(e)
    e_max = torch.full((n, H), float("-inf"), dtype=e.dtype).scatter_reduce(0, idx, e.detach(), reduce="amax",
                                                                            include_self=True)
    u = (e - e_max[row]).exp()
    alpha = u / (torch.zeros((n, H), dtype=e.dtype).index_add(0, row, u)[row] + 1e-16)
    out = torch.zeros_like(h).index_add(0, row, h[col] * alpha.unsqueeze(-1)).reshape(n, H * C)
    if bias is not None:
        out = out + bias
    return out, alpha, z


def transpose_map_np(rowptr, col):
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    key = row * n + col                      # strictly increasing: the CSR is sorted
    assert np.all(np.diff(key) > 0)
    t = np.searchsorted(key, col * n + row)
    assert np.all(t < len(key)) and np.array_equal(key[np.minimum(t, len(key) - 1)], col * n + row), "not symmetric"
    return t


def alpha_backward_np(x, W, att_l, att_r, rowptr, col, alpha, z, G, negative_slope=0.2):
    """Gradients of sum(alpha * G) in closed form: dict of x, W, att_l, att_r (bias: zero)."""
    x, W, alpha, z, G = (np.asarray(t, np.float64) for t in (x, W, alpha, z, G))
    H, C = att_l.shape[-2], att_l.shape[-1]
    al, ar = np.asarray(att_l, np.float64).reshape(H, C), np.asarray(att_r, np.float64).reshape(H, C)
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    row = np.repeat(np.arange(n), np.diff(rowptr))
    s = np.where(z > 0, 1.0, negative_slope)
    c = np.zeros((n, H))
    np.add.at(c, row, alpha * G)
    dz = alpha * s * (G - c[row])
    da_dst = np.zeros((n, H))
    np.add.at(da_dst, row, dz)
    # row r's own list names the rows that have r as a neighbour; (i, r) sits at tmap[e(r, i)]
    t = transpose_map_np(rowptr, col)
    da_src = np.zeros((n, H))
    np.add.at(da_src, row, dz[t])
    h = (x @ W.T).reshape(n, H, C)
    dh = da_src[:, :, None] * al[None] + da_dst[:, :, None] * ar[None]
    return {"x": dh.reshape(n, H * C) @ W, "W": dh.reshape(n, H * C).T @ x,
            "att_l": (da_src[:, :, None] * h).sum(0).reshape(1, H, C),
            "att_r": (da_dst[:, :, None] * h).sum(0).reshape(1, H, C)}


class _Conv(torch.nn.Module):
    """The parameters of a GATConv (named as PyG names them) over ``gat_attention``."""

    def __init__(self, fin, out, heads):
        from oracle import gat as og
        super().__init__()
        ref = og.GATConv(fin, out, heads=heads)          # the reference's init, draw for draw
        self.lin_l = ref.lin_l
        self.lin_r = self.lin_l
        self.att_l, self.att_r, self.bias = ref.att_l, ref.att_r, ref.bias

    def forward(self, x, csr):
        return gat_attention(x, self.lin_l.weight, self.att_l, self.att_r, self.bias, *csr)


class EntropyRef(torch.nn.Module):
    """models.py:1112-1148; ``csr`` = (rowptr, col) int64 WITH the self loops."""

    def __init__(self):
        super().__init__()
        self.conv = _Conv(256, 128, 2)
        self.densea = Linear(256, 128)
        self.dense1 = Linear(128, 64)
        self.dense2 = Linear(64, 3)
        self.alpha = 0.01

    def coords_and_alpha(self, x, csr):
        x, alpha, _ = self.conv(x, csr)
        x = F.relu(self.densea(F.relu(x)))
        return self.dense2(F.relu(self.dense1(x))), alpha

    def loss(self, x, csr, truth):
        """MSE(cdist(coords), truth) + self.alpha * entropy(alpha) / (N * H), exact distances."""
        c, alpha = self.coords_and_alpha(x, csr)
        d = torch.cdist(c, c, p=2, compute_mode="donot_use_mm_for_euclid_dist")
        ent = -(alpha * torch.log(alpha + 1e-12)).sum()
        return F.mse_loss(d, truth) + self.alpha * ent / (x.shape[0] * alpha.shape[1]), c


# ---------------------------------------------------------------- graphs (dense symmetric 0/1, zero diagonal)
def _n7():
    a = np.zeros((7, 7))
    for i, j in [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (1, 4)]:   # node 6: the self loop only
        a[i, j] = a[j, i] = 1
    return a


def _n70():
    return np.ones((70, 70)) - np.eye(70)


def _n130():
    """Hub 0 is everybody's neighbour (degree 130 with its self loop); 1 - 2 - ... - 128 is a path (ends:
    degree 3, inner: 4); 129 hangs on the hub alone (degree 2)."""
    a = np.zeros((130, 130))
    a[0, 1:] = a[1:, 0] = 1
    for i in range(1, 128):
        a[i, i + 1] = a[i + 1, i] = 1
    return a


def _deg63():
    """Rows 0, 1, 2 have 62, 63, 64 neighbours among 10 ..: degree 63, 64, 65 with the self loop."""
    a = np.zeros((100, 100))
    for r, k in ((0, 62), (1, 63), (2, 64)):
        a[r, 10:10 + k] = a[10:10 + k, r] = 1
    for i in range(3, 99):
        a[i, i + 1] = a[i + 1, i] = 1
    return a


GRAPHS = {"n7": _n7, "n70": _n70, "n130": _n130, "deg63": _deg63}


@functools.lru_cache(maxsize=None)
def csr_with_self_loops(name):
    """(rowptr, col) int64 of GRAPHS[name] with one self loop per row, sorted: the device CSR's order."""
    a = GRAPHS[name]() + np.eye(GRAPHS[name]().shape[0])
    r, c = np.nonzero(a)
    rowptr = np.zeros(a.shape[0] + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=a.shape[0]))
    return torch.tensor(rowptr), torch.tensor(c.astype(np.int64))

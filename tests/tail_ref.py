"""fp64 reference of the one-kernel MLP tail (csrc/tail_fused.hip), one function per stage of the
kernel, each returning ``(value, bound)`` (TEST INFRASTRUCTURE ONLY).

A stage function receives that stage's inputs AS THE KERNEL SEES THEM: the test's tensors for the
first stage, the kernel's own fp32 output of the stage before (widened to fp64) for every later
one.  Rounding therefore does not chain from stage to stage, and each stage's tolerance is the
forward-error bound of its own formula, derived here and not tuned against the kernel.

The bound.  With u = 2^-24 (fp32 unit roundoff), every fp32 operation returns fl(a op b) =
(a op b)(1 + d), |d| <= u.  Carry beside every quantity q a magnitude m(q) >= |q|, the value the
same formula takes when every term enters with its absolute value:

  * an exact fp32 input:      m = |value|                       (no error yet)
  * a sum / reduction:        m = the sum of the terms' m       (|sum a_i| <= sum |a_i|)
  * a product:                m = the product of the m
  * r = rsqrt(v):             m = |r| m(v) / |v|                (dr = -r dv / 2v: the relative error
                                                                 of v, m(v)/|v| times its rounding,
                                                                 carries over to r)

The classical running error analysis (Higham, Accuracy and Stability of Numerical Algorithms,
sect. 3.1, 3.3) then bounds the error of a quantity computed through a chain of n roundings by
gamma_n m, gamma_n = n u / (1 - n u), whatever the order of summation: an n-term sum rounds every
partial sum once, each partial sum is at most the sum of the |terms|, so |error| <= (n - 1) u m to
first order, plus one rounding per product and one for a bias.  Here n is the number of terms of
the longest chain of reductions that feeds the element -- K for a GEMM stage, W for a LayerNorm
forward stage (mean, then variance, then the affine map: the W-term reductions dominate), K + W
for a GEMM followed by the LayerNorm backward (the dz GEMM feeds the two W-term row means) -- and
4 more for the handful of elementwise operations (bias, subtraction, scale, residual).  The
element's bound is

      bound = 4 (n + 4) 2^-24 m.

The factor 4 covers the first-order truncation (squares of u, the factor 2 of d(var) = 2 d dd / W
and the 1/2 of the rsqrt, both already below it) and the rounding inside the MFMA's four-term dot
product, which has not been measured.  For a pure GEMM stage y = A B^T + b the rule reduces to
4 (K + 4) 2^-24 (|A| |B|^T + |b|).

relu needs no kink mask in the forward: it is 1-Lipschitz, so an input within its bound of 0
gives an output within the same bound on either side; relu keeps m.  The backward's mask
[pre > 0] is discontinuous; the tests keep |pre| away from 0 (``backward_inputs``) except where pre
is 0 exactly, and there both the kernel and fp64 mask.
"""
import functools

import torch

U = 2.0 ** -24          # fp32 unit roundoff
FACTOR = 4.0
TILE = 16               # rows per workgroup of both tail kernels: one LayerNorm partial row per tile
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))   # the eps the kernel gets (a float argument)


class Q:
    """A quantity in fp64 with its magnitude m >= |v| (the module docstring's rules)."""

    def __init__(self, v, m=None):
        self.v = torch.as_tensor(v).double()
        self.m = self.v.abs() if m is None else m

    @staticmethod
    def of(x):
        return x if isinstance(x, Q) else Q(x)

    def __add__(self, o):
        o = Q.of(o)
        return Q(self.v + o.v, self.m + o.m)

    def __sub__(self, o):
        o = Q.of(o)
        return Q(self.v - o.v, self.m + o.m)

    def __mul__(self, o):
        o = Q.of(o)
        return Q(self.v * o.v, self.m * o.m)

    def __matmul__(self, o):
        o = Q.of(o)
        return Q(self.v @ o.v, self.m @ o.m)

    def __getitem__(self, i):
        return Q(self.v[i], self.m[i])

    def t(self):
        return Q(self.v.t(), self.m.t())

    def reshape(self, *s):
        return Q(self.v.reshape(*s), self.m.reshape(*s))

    def sum(self, dim, keepdim=False):
        return Q(self.v.sum(dim, keepdim), self.m.sum(dim, keepdim))

    def scale(self, c):          # by a constant (1 / W)
        return Q(self.v * c, self.m * abs(c))

    def rsqrt(self):
        r = self.v ** -0.5
        return Q(r, r.abs() * self.m / self.v.abs())

    def relu(self):
        return Q(torch.relu(self.v), self.m)

    def masked(self, mask):      # times an exact 0 / 1 mask
        return Q(self.v * mask, self.m * mask)

    def bound(self, n):
        return FACTOR * (n + 4) * U * self.m


def cat(qs, dim):
    return Q(torch.cat([q.v for q in qs], dim), torch.cat([q.m for q in qs], dim))


def _out(q, n):
    return q.v, q.bound(n)


# ---------------------------------------------------------------------------------- forward stages
def gemm_bias(a, w, b):
    """y = a w^T + b (a [M, K], w [N, K], b [N]): Y1, Y2, y3 and coords."""
    a = Q(a)
    return _out(a @ Q(w).t() + Q(b), a.v.shape[1])


def heads_fwd(xa, Wh, bh):
    """Y0[:, 256h:256h+256] = xa[h] Wh[256h:256h+256]^T + bh (xa [2, M, 512]); O = relu(Y0) has the
    same bound."""
    Wh, bh = Q(Wh), Q(bh)
    ys = [Q(xa[h]) @ Wh[256 * h:256 * h + 256].t() + bh[256 * h:256 * h + 256] for h in range(2)]
    return _out(cat(ys, 1), 512)


def ln_fwd(y, gamma, beta, eps, W, res):
    """ln_rows: mean and rstd = 1 / sqrt(biased var + eps) over y[:, :W]; z = relu(xhat gamma + beta)
    (+ y[:, W:2W] when res).  Returns (st, st_bound), (z, z_bound) with st = [mean | rstd]."""
    y = Q(y)
    h = y[:, :W]
    mean = h.sum(1, True).scale(1.0 / W)
    d = h - mean
    var = (d * d).sum(1, True).scale(1.0 / W)
    rstd = (var + Q(torch.tensor(eps))).rsqrt()
    z = (d * rstd * Q(gamma) + Q(beta)).relu()
    if res:
        z = z + y[:, W:2 * W]
    return _out(cat([mean, rstd], 1), W), _out(z, W)


# --------------------------------------------------------------------------------- backward stages
def tile_sum(q, tile=TILE):
    """[M, W] -> [ceil(M / tile), W]: the sum over each tile's LIVE rows (the rows past M add nothing)."""
    M, W = q.v.shape
    nt = -(-M // tile)
    pad = torch.zeros((nt * tile - M, W), dtype=torch.float64)
    p = Q(torch.cat([q.v, pad]), torch.cat([q.m, pad]))
    return p.reshape(nt, tile, W).sum(1)


def ln_bwd(dz_in, wt, y, st, gamma, beta, W, res):
    """ln_bwd_rows after its GEMM: dz = dz_in wt (dz_in [M, K], wt [K, W]); xhat = (y[:, :W] -
    mean) rstd from st as given (the kernel never recomputes statistics); g = dz [pre > 0], dh = g gamma,
    dy = rstd (dh - mean(dh) - xhat mean(dh xhat)); dY = [dy | dz] when res (the residual's gradient
    is dz itself).  The partial rows: p[t] = [sum g xhat | sum g] over tile t's live rows.  Returns
    dY, p (each (value, bound)) and pre."""
    dz_in = Q(dz_in)
    K = dz_in.v.shape[1]
    dz = dz_in @ Q(wt)
    y, st, gamma = Q(y), Q(st), Q(gamma)
    rstd = st[:, 1:2]
    xh = (y[:, :W] - st[:, 0:1]) * rstd
    pre = xh * gamma + Q(beta)
    g = dz.masked((pre.v > 0).double())
    dh = g * gamma
    m1 = dh.sum(1, True).scale(1.0 / W)
    m2 = (dh * xh).sum(1, True).scale(1.0 / W)
    dy = rstd * (dh - m1 - xh * m2)
    dY = cat([dy, dz], 1) if res else dy
    p = cat([tile_sum(g * xh), tile_sum(g)], 1)
    n = K + W
    return dict(dY=_out(dY, n), p=_out(p, n), pre=pre.v)


def gemm_t(dy, w):
    """dx = dy w (dy [M, K], w [K, N])."""
    dy = Q(dy)
    return _out(dy @ Q(w), dy.v.shape[1])


def dout_stage(dY1, W1c, y, act):
    """Both epilogues' dout = dx [y > 0] (act) or dx, dx = dY1 W1c (y: the rows form's y, the heads
    form's Y0)."""
    dY1 = Q(dY1)
    dx = dY1 @ Q(W1c)
    if act:
        dx = dx.masked((torch.as_tensor(y).double() > 0).double())
    return _out(dx, dY1.v.shape[1])


def _head_dots(a, b):
    M = a.v.shape[0]
    return (a * b).reshape(M, 2, 256).sum(2)


def rows_stats(dout, y, bias, out2, s3):
    """agg_bwd_rows_row<2, 256>: rs[:, 4:8] = (delta^0, delta^1, <dout^0, out2^0> - delta^0 S3^0, ...^1)
    with delta^h = <dout^h, y^h - b^h> and S3 = the incoming rs[:, 4:6]."""
    d = Q(dout)
    delta = _head_dots(d, Q(y) - Q(bias))
    da = _head_dots(d, Q(out2)) - delta * Q(s3)
    return _out(cat([delta, da], 1), 256)


def heads_delta(dout, Y0, bh):
    """The heads epilogue's rs[:, 4:6] = delta^h = <dout^h, Y0^h - bh^h>."""
    return _out(_head_dots(Q(dout), Q(Y0) - Q(bh)), 256)


def heads_moved(rs_in):
    """The heads epilogue's rs[:, 6:8]: the incoming rs[:, 4:6] (S3), moved -- a copy, so the bound is 0."""
    v = torch.as_tensor(rs_in)[:, 4:6].double()
    return v, torch.zeros_like(v)


def heads_dxa(dout, Wh):
    """dxa[:, 512h:512h+512] = dout^h Wh[256h:256h+256, :]."""
    d, Wh = Q(dout), Q(Wh)
    return _out(cat([d[:, 256 * h:256 * h + 256] @ Wh[256 * h:256 * h + 256] for h in range(2)], 1), 256)


# ------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def params(seed=5):
    """The tail's parameters as the existing tail tests draw them (fp32, CPU; read-only)."""
    g = torch.Generator().manual_seed(seed)

    def r(*s):
        return torch.randn(*s, generator=g)

    P = dict(W1c=r(512, 512) * 0.05, b1c=r(512) * 0.1, g1=1 + 0.1 * r(256), be1=0.1 * r(256),
             W2c=r(256, 256) * 0.05, b2c=r(256) * 0.1, g2=1 + 0.1 * r(128), be2=0.1 * r(128),
             W3=r(64, 128) * 0.1, b3=r(64) * 0.1, g3=1 + 0.1 * r(64), be3=0.1 * r(64),
             W4=r(3, 64) * 0.1, b4=r(3) * 0.1, Wh=r(512, 512) * 0.05, bh=r(512) * 0.1)
    return P


@functools.lru_cache(maxsize=None)
def forward_inputs(M, small=False):
    """(P, x, X4): x = relu(randn) [M, 512] for the plain forward, X4 [2, 2, M + 5, 512] for the heads
    form (xa^h = X4[h, 0, :M]).  small: x scaled by 1e-3 and b1c = 0, so that the first LayerNorm's
    row variance is of eps's order."""
    g = torch.Generator().manual_seed(1000 + M)
    P = dict(params())
    x = torch.relu(torch.randn(M, 512, generator=g))
    X4 = torch.randn(2, 2, M + 5, 512, generator=g)
    if small:
        x = x * 1e-3
        P["b1c"] = torch.zeros(512)
    return P, x, X4


def _stats32(y, W):
    h = y[:, :W].double()
    mean = h.mean(1, keepdim=True)
    rstd = ((h - mean).pow(2).mean(1, keepdim=True) + EPS32) ** -0.5
    return torch.cat([mean, rstd], 1).float()


PRE_MIN = 1e-4


def _off_kink(y, st, gamma, beta, W):
    """Move the elements of y[:, :W] whose fp64 pre = xhat gamma + beta is closer to 0 than PRE_MIN
    to |pre| = 2 PRE_MIN (st stays: the kernel reads statistics, it does not recompute them)."""
    mean, rstd = st[:, 0:1].double(), st[:, 1:2].double()
    ga, be = gamma.double(), beta.double()
    pre = (y[:, :W].double() - mean) * rstd * ga + be
    near = pre.abs() < PRE_MIN
    target = torch.where(pre < 0, -2 * PRE_MIN, 2 * PRE_MIN)
    moved = (mean + (target - be) / (rstd * ga)).float()
    y[:, :W] = torch.where(near, moved, y[:, :W])
    return y


@functools.lru_cache(maxsize=None)
def backward_inputs(M, zero_row=False):
    """Synthetic backward inputs: random saved Y1 / Y2 / y3 with st = their fp32 mean and rstd, dc, and
    the epilogues' y (= Y0), out2 and row_stats.  zero_row: the last row of every Y equals its st mean
    in every column and beta is 0 in four columns (pre = 0 exactly there; the other betas of that row
    are kept away from 0)."""
    g = torch.Generator().manual_seed(2000 + M + (500 if zero_row else 0))
    P = dict(params())
    B = dict(dc=torch.randn(M, 3, generator=g))
    for name, cols, W, ga, be in (("Y1", 512, 256, "g1", "be1"), ("Y2", 256, 128, "g2", "be2"),
                                  ("y3", 64, 64, "g3", "be3")):
        y = torch.randn(M, cols, generator=g)
        st = _stats32(y, W)
        if zero_row:
            be_ = P[be].clone()
            be_ = torch.where(be_.abs() < 1e-3, torch.full_like(be_, 1e-3), be_)
            be_[[1, 17, W // 2, W - 1]] = 0.0
            P[be] = be_
            st[M - 1, 0] = 0.5
            y[M - 1, :W] = 0.5
        y = _off_kink(y, st, P[ga], P[be], W)
        if zero_row:
            y[M - 1, :W] = 0.5
        B[name], B["st" + name[-1]] = y, st
    yy = torch.randn(M, 512, generator=g)
    yy.view(-1)[torch.randperm(M * 512, generator=g)[:max(3, M // 4)]] = 0.0   # exact zeros mask
    B["y"] = yy
    B["out2"] = torch.randn(M, 512, generator=g)
    B["rs"] = torch.randn(M, 8, generator=g)
    return P, B

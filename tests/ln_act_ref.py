"""The float64 CPU reference of the general LayerNorm row pass (ln_act.hip) and the kink-free inputs its
tests draw: torch.nn.LayerNorm, the activation and the residual add composed in float64 on the fp32
inputs.  Shared by tests/test_layernorm_models_host.py (the draws exist) and tests/test_gpu_ln_act.py."""
import copy
import functools

import torch
import torch.nn.functional as F
from torch.nn import LayerNorm

WIDTHS = (32, 64, 128, 256, 512)
ACTS = (None, "relu", ("leaky_relu", 0.01), "gelu")
ROWS = (1, 2, 3, 65, 257, 4099)      # odd counts: a half-filled last wave; 4099 > the backward grid's 4096 waves


def rows_of(W):
    """W = 32 runs two rows per wave, so its stride loop runs twice from 2 * 4096 rows on."""
    return ROWS + ((8197,) if W == 32 else ())


def act_fn(x, act):
    if act is None:
        return x
    if act == "relu":
        return F.relu(x)
    if act == "gelu":
        return F.gelu(x)                     # the erf form
    return F.leaky_relu(x, act[1] if isinstance(act, tuple) else 0.01)


def has_kink(act):
    return act == "relu" or act == "leaky_relu" or (isinstance(act, tuple) and act[0] == "leaky_relu")


def module(W, g):
    """A LayerNorm(W) with non-trivial gamma and beta."""
    n = LayerNorm(W)
    with torch.no_grad():
        n.weight.copy_(0.5 + torch.rand(W, generator=g))
        n.bias.copy_(0.3 * torch.randn(W, generator=g))
    return n


def ref(norm, norm2, y, res, dz, act):
    """torch in float64 on the fp32 inputs: a dict of z, the gradients and the pre-activation."""
    n = copy.deepcopy(norm).double()
    n2 = copy.deepcopy(norm2).double() if norm2 is not None else None
    y64 = y.double().requires_grad_()
    r64 = res.double().requires_grad_() if res is not None else None
    pre = n(y64)
    u = act_fn(pre, act)
    if r64 is not None:
        u = u + r64
    z = n2(u) if n2 is not None else u
    z.backward(dz.double())
    out = {"z": z.detach(), "dy": y64.grad, "dgamma": n.weight.grad, "dbeta": n.bias.grad, "pre": pre.detach()}
    if r64 is not None:
        out["dres"] = r64.grad
    if n2 is not None:
        out["dgamma2"], out["dbeta2"] = n2.weight.grad, n2.bias.grad
    return out


@functools.lru_cache(maxsize=16)
def drawn(M, W, act, has_res, has_n2):
    """(norm, norm2, y, res, dz, reference) of the first seed of 0..7 whose float64 reference has every
    pre-activation farther than 1e-6 of the layer's largest from the activation's kink; the few offenders
    of a large tensor are moved by 0.01 (a few rounds: that moves their row's statistics a little) before
    the seed is judged.  Nothing is left out of the comparison."""
    for seed in range(8):
        g = torch.Generator().manual_seed(1000 * seed + 7 * M + W)
        norm = module(W, g)
        norm2 = module(W, g) if has_n2 else None
        y = torch.randn(M, W, generator=g) * 1.5 + 0.5
        res = torch.randn(M, W, generator=g) if has_res else None
        dz = torch.randn(M, W, generator=g)
        for _ in range(4):
            r = ref(norm, norm2, y, res, dz, act)
            near = r["pre"].abs() <= 1e-6 * r["pre"].abs().max()
            if not has_kink(act) or not near.any():
                return norm, norm2, y, res, dz, r
            y = torch.where(near, y + 0.01, y)
    raise AssertionError(f"({M}, {W}) {act}: no seed of 0..7 keeps the pre-activations away from 0")

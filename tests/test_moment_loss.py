"""The moment-dependent distance losses (``ops.MOMENT_LOSS_KINDS``): "mse+pearson", "rmse", "si_mse".

The oracle is plain torch in fp64 on the CPU, written out below: d_ij from explicit differences over
``triu_indices``, the loss formulas of include/hicgat.h, the gradient from ``torch.autograd.grad``.  It
gets the same fp32 coordinates and truth the device gets.

Gradient error: ``max|dc - dc_oracle| / max_i(|B R_i| + |(A + B) U_i| + |C W_i|)`` with the three terms
of the decomposition dc_i = -B R_i + (A + B) U_i + C W_i formed by the test in fp64 -- the scale at
which the fp32 rounding of the three sums enters.  The bound is measured, not chosen: the same
normalised error of the existing ``kind="mse"`` gradient on the same inputs against its own fp64
oracle, times 16 (three separately rounded sums and fp32-stored R, W where the MSE has one).
Values and moments: 1e-5 relative, the tolerance tests/test_gpu_parity.py::test_fused_loss_matches_oracle
applies to stats[7]; r: 1e-6 absolute, as there.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

DEV = "cuda"
KINDS = ("mse+pearson", "rmse", "si_mse")
RTOL = 1e-5
R_ATOL = 1e-6
GRAD_FACTOR = 16.0


# ---- the oracle -------------------------------------------------------------------------------------
def _pairs(c, T):
    """d_ij, t_ij over i < j (d = 0 with no gradient where the points coincide) and the diagonal of T."""
    n = c.shape[0]
    iu = torch.triu_indices(n, n, 1)
    diff = c[iu[0]] - c[iu[1]]
    d2 = (diff * diff).sum(1)
    nz = d2 > 0
    d = torch.where(nz, torch.sqrt(torch.where(nz, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    return d, T[iu[0], iu[1]], T.diagonal(), iu


def _moments(d, t, diag):
    n = diag.shape[0]
    M = n * (n - 1) / 2
    m = {"s0": ((d - t) ** 2).sum(), "sd": d.sum(), "sdd": (d * d).sum(), "sdt": (d * t).sum(), "st": t.sum(),
         "stt": (t * t).sum(), "dg": (diag * diag).sum(), "sdiag": diag.sum(), "M": M, "n2": float(n * n)}
    m["mse"] = (2 * m["s0"] + m["dg"]) / m["n2"]
    if M > 0:
        m["vd"] = m["sdd"] / M - (m["sd"] / M) ** 2
        m["vt"] = m["stt"] / M - (m["st"] / M) ** 2
        m["cov"] = m["sdt"] / M - m["sd"] * m["st"] / (M * M)
    else:
        m["vd"] = m["vt"] = m["cov"] = torch.zeros((), dtype=torch.float64)
    m["ok"] = bool(m["vd"] > 0) and bool(m["vt"] > 0)
    m["r"] = m["cov"] / torch.sqrt(m["vd"] * m["vt"]) if m["ok"] else None
    m["ebar"] = (2 * (m["sd"] - m["st"]) - m["sdiag"]) / m["n2"]
    return m


def _value(kind, d, t, diag, alpha):
    m = _moments(d, t, diag)
    if kind == "mse":
        return m["mse"], m
    if kind == "mse+pearson":
        # a variance <= 0: r taken as 0 in the value, no gradient from the term
        return (m["mse"] + alpha * (1 - m["r"]) if m["ok"] else m["mse"] + alpha), m
    if kind == "rmse":
        return torch.sqrt(m["mse"] + 1e-12), m
    if kind == "si_mse":
        e, eb = d - t, m["ebar"]
        return (2 * ((e - eb) ** 2).sum() + ((-diag - eb) ** 2).sum()) / m["n2"], m
    raise KeyError(kind)


def oracle(c32, t32, kind, alpha=1.0):
    """(value, d value / d coords, moments) in fp64 from the fp32 inputs."""
    c = c32.detach().cpu().double().clone().requires_grad_(True)
    T = t32.detach().cpu().double()
    d, t, diag, _ = _pairs(c, T)
    v, m = _value(kind, d, t, diag, alpha)
    if v.requires_grad:
        (g,) = torch.autograd.grad(v, c, allow_unused=True)
        g = torch.zeros_like(c) if g is None else g
    else:       # N = 1: no pair, the value is a constant
        g = torch.zeros_like(c)
    return float(v), g.detach(), {k: (float(x) if torch.is_tensor(x) else x) for k, x in m.items()}


def coefficients(kind, m, alpha=1.0):
    """A, B, C of d value / d d_ij = A d_ij + B t_ij + C, from the fp64 moments."""
    g4 = 4.0 / m["n2"]
    if kind == "mse":
        return g4, -g4, 0.0
    if kind == "mse+pearson":
        if not m["ok"]:
            return g4, -g4, 0.0
        M, sq = m["M"], np.sqrt(m["vd"] * m["vt"])
        return (g4 + alpha * m["r"] / (m["vd"] * M), -g4 - alpha / (sq * M),
                alpha * ((m["st"] / M) / sq - m["r"] * (m["sd"] / M) / m["vd"]) / M)
    if kind == "rmse":
        a = g4 / (2.0 * np.sqrt(m["mse"] + 1e-12))
        return a, -a, 0.0
    if kind == "si_mse":
        return g4, -g4, -g4 * m["ebar"]
    raise KeyError(kind)


def row_sums(c32, t32):
    """R_i, U_i, W_i [N, 3] in fp64."""
    c = c32.detach().cpu().double().numpy()
    T = t32.detach().cpu().double().numpy()
    diff = c[:, None, :] - c[None, :, :]
    d = np.sqrt((diff * diff).sum(2))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(d[:, :, None] > 0, diff / d[:, :, None], 0.0)
    off = 1.0 - np.eye(len(c))
    R = (((d - T) * off)[:, :, None] * u).sum(1)
    U = len(c) * c - c.sum(0)
    W = u.sum(1)
    return R, U, W


def term_scale(kind, m, R, U, W, alpha=1.0):
    a, b, c = coefficients(kind, m, alpha)
    return float(np.max(np.abs(b * R) + np.abs((a + b) * U) + np.abs(c * W))) if len(R) else 0.0


def normalised(err, scale):
    """err / scale; a zero scale (N = 1, collapsed coordinates) admits a zero error only."""
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


# ---- inputs -----------------------------------------------------------------------------------------
def _coords(n, seed, scale=0.5):
    return torch.tensor((scale * np.random.default_rng(seed).standard_normal((n, 3))).astype(np.float32))


def _dense_truth(n, seed):
    """Symmetric, a non-zero diagonal."""
    rng = np.random.default_rng(100 + seed)
    t = rng.random((n, n)) + 0.25
    t = (t + t.T) / 2
    np.fill_diagonal(t, 0.1 + 0.5 * rng.random(n))
    return torch.tensor(t.astype(np.float32))


def _bg_truth(n, seed):
    """cont2dist-style: 1 off the diagonal except at a ~5 % symmetric support with values in (0, 1);
    a non-zero diagonal on top, so that the support form's diagonal terms are exercised too."""
    rng = np.random.default_rng(200 + seed)
    t = np.ones((n, n))
    iu = np.triu_indices(n, 1)
    hit = rng.random(len(iu[0])) < 0.05
    if n > 1 and not hit.any():
        hit[0] = True
    t[iu[0][hit], iu[1][hit]] = 0.05 + 0.9 * rng.random(int(hit.sum()))
    t = np.triu(t, 1)
    t = t + t.T
    np.fill_diagonal(t, 0.2 * rng.random(n))
    return torch.tensor(t.astype(np.float32))


# ---- host tests -------------------------------------------------------------------------------------
def test_mloss_kind_codes_match_the_header():
    from hicgat import ops
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "include", "hicgat.h")) as fh:
        h = fh.read()
    codes = {k.lower(): int(v) for k, v in re.findall(r"HICGAT_MLOSS_(\w+) = (\d+)", h)}
    names = {"pearson": "mse+pearson", "rmse": "rmse", "si_mse": "si_mse"}
    assert {names[k]: v for k, v in codes.items()} == ops.MOMENT_LOSS_KINDS
    assert tuple(ops.MOMENT_LOSS_KINDS) == KINDS
    assert ops.LOSS_KINDS == {"mse": 0, "combined": 1, "contrastive": 2}
    assert not re.findall(r"HICGAT_LOSS_(\w+) = (\d+)", h)[3:]      # no fourth HICGAT_LOSS_ constant


def test_train_offers_the_new_losses():
    from hicgat import train
    for k in KINDS:
        assert k in train.LOSSES
        a = train.make_parser().parse_args(["m.txt", "f.txt", "--loss", k, "--alpha", "0.5"])
        assert a.loss == k and a.alpha == 0.5
    assert "mse+dscc" in train.LOSSES


@pytest.mark.parametrize("kind", KINDS)
def test_asymmetric_truth_is_refused(kind):
    import hicgat
    t = np.random.default_rng(0).random((9, 9)).astype(np.float32)
    tr = hicgat.Truth(torch.tensor(t))
    assert tr.asymmetric_source
    with pytest.raises(ValueError, match="symmetric"):
        hicgat.ops.fused_dist_loss(torch.zeros(9, 3), tr, kind)


@pytest.mark.parametrize("n", [2, 3, 40, 129])
@pytest.mark.parametrize("kind", ("mse",) + KINDS)
def test_decomposition_identity_matches_autograd(n, kind):
    """dc_i = -B R_i + (A + B) U_i + C W_i, all in fp64, against autograd of the written-out loss."""
    c, T = _coords(n, n), _dense_truth(n, n)
    for alpha in (1.0, 0.5):
        _, g, m = oracle(c, T, kind, alpha)
        R, U, W = row_sums(c, T)
        a, b, cc = coefficients(kind, m, alpha)
        dc = -b * R + (a + b) * U + cc * W
        scale = term_scale(kind, m, R, U, W, alpha)
        assert np.max(np.abs(dc - g.numpy())) <= 1e-12 * scale, (kind, n, alpha)


def test_oracle_rmse_gradient_is_the_mse_gradient_over_twice_the_value():
    c, T = _coords(60, 3), _dense_truth(60, 3)
    v, g, _ = oracle(c, T, "rmse")
    vm, gm, _ = oracle(c, T, "mse")
    assert abs(v - np.sqrt(vm + 1e-12)) <= 1e-15 * v
    assert float((g - gm / (2 * v)).abs().max()) <= 1e-14 * float(g.abs().max())


def test_oracle_degenerate_pearson_has_the_mse_gradient():
    """Collapsed coordinates: the Pearson term is the constant alpha; coincident points carry no gradient."""
    c = torch.full((20, 3), 0.25)
    T = _dense_truth(20, 1)
    v, g, m = oracle(c, T, "mse+pearson", 0.7)
    assert not m["ok"] and abs(v - (m["mse"] + 0.7)) < 1e-15 and float(g.abs().max()) == 0.0


# ---- GPU tests --------------------------------------------------------------------------------------
FORMS = ("dense", "bg_support", "bg_dense")
SHAPES = (1, 2, 127, 128, 129, 300)


def _truth(form, T):
    """The ``Truth`` of a form: "dense" and "bg_dense" without a support (the dense kernel),
    "bg_support" with the background + support form whatever the support's density (N = 2's single pair
    is half the matrix).  N = 1 has no pair and no support form: it runs the dense kernel."""
    import hicgat
    from hicgat.graph import SupportForm
    tr = hicgat.Truth(T.to(DEV), background=None)
    assert not tr.asymmetric_source and tr.support is None
    if form == "bg_support" and tr.n > 1:
        tr.support = SupportForm.build(tr, 1.0, max_fraction=1.0)
        assert tr.support is not None
    return tr


def _device(c, tr, kind, alpha=1.0):
    import hicgat
    cm = c.to(DEV).requires_grad_(True)
    loss, stats = hicgat.ops.fused_dist_loss(cm, tr, kind, alpha=alpha)
    (dc,) = torch.autograd.grad(loss, cm)
    return loss.detach().cpu(), stats.detach().cpu().clone(), dc.detach().cpu()


@functools.lru_cache(maxsize=None)
def _case(n, form):
    """One shape and truth form: the inputs, the fp64 row sums, and the measured normalised error of the
    parent commit's ``kind="mse"`` gradient on them (the yardstick of the bound)."""
    c = _coords(n, n)
    T = _dense_truth(n, n) if form == "dense" else _bg_truth(n, n)
    tr = _truth(form, T)
    R, U, W = row_sums(c, T)
    _, g_mse, m = oracle(c, T, "mse")
    _, _, dc_mse = _device(c, tr, "mse")
    ref = normalised(float((dc_mse.double() - g_mse).abs().max()), term_scale("mse", m, R, U, W))
    return {"c": c, "T": T, "tr": tr, "RUW": (R, U, W), "mse_ratio": ref, "dc_mse": dc_mse, "m": m}


def _check_gradient(tag, dc, g, kind, m, RUW, mse_ratio, alpha=1.0):
    assert bool(torch.isfinite(dc).all()), tag
    ratio = normalised(float((dc.double() - g).abs().max()), term_scale(kind, m, *RUW, alpha))
    print(f"[moment-loss] {tag}: normalised gradient error {ratio:.3e}, kind=mse on the same inputs "
          f"{mse_ratio:.3e}, ratio {ratio / mse_ratio if mse_ratio > 0 else float('nan'):.2f}")
    assert ratio <= GRAD_FACTOR * mse_ratio, (tag, ratio, mse_ratio)
    return ratio


def _close(a, b, tag):
    assert abs(a - b) <= RTOL * abs(b), (tag, a, b)


def _check_stats(tag, kind, st, loss, v, m, alpha=1.0):
    st = st.numpy()
    for k, name in enumerate(("s0", "sd", "sdd", "sdt", "st", "stt", "dg")):
        _close(st[k], m[name], f"{tag} stats[{k}]")
    _close(st[7], m["mse"], f"{tag} mse")
    if m["ok"]:
        assert abs(st[8] - m["r"]) <= R_ATOL, (tag, st[8], m["r"])
    else:
        assert np.isnan(st[8]), (tag, st[8])
    if kind == "mse+pearson":
        assert st[9] == alpha, (tag, st[9])
    elif kind == "rmse":
        assert st[9] == 0.0, (tag, st[9])
    else:
        # ebar = (2 (sum d - sum t) - sum T_ii) / N^2 is a difference of sums that each carry RTOL
        assert abs(st[9] - m["ebar"]) <= RTOL * (2 * (m["sd"] + m["st"]) + abs(m["sdiag"])) / m["n2"], (tag, st[9])
    _close(st[10], v, f"{tag} value")
    _close(st[11], m["sdiag"], f"{tag} sum T_ii")
    _close(float(loss), v, f"{tag} fp32 loss")
    assert float(loss) == float(np.float32(st[10])), tag


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_value_moments_and_gradient_match_the_oracle(kind, form, n):
    z = _case(n, form)
    loss, st, dc = _device(z["c"], z["tr"], kind)
    v, g, m = oracle(z["c"], z["T"], kind)
    tag = f"{kind} {form} N={n}"
    _check_stats(tag, kind, st, loss, v, m)
    _check_gradient(tag, dc, g, kind, m, z["RUW"], z["mse_ratio"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHAPES[1:])
@pytest.mark.parametrize("kind", KINDS)
def test_support_form_agrees_with_the_dense_form(kind, n):
    zs, zd = _case(n, "bg_support"), _case(n, "bg_dense")
    ls, ss, ds = _device(zs["c"], zs["tr"], kind)
    ld, sd, dd = _device(zd["c"], zd["tr"], kind)
    for k in list(range(8)) + [10, 11]:
        _close(float(ss[k]), float(sd[k]), f"{kind} N={n} stats[{k}]")
    _, _, m = oracle(zs["c"], zs["T"], kind)
    ratio = normalised(float((ds.double() - dd.double()).abs().max()), term_scale(kind, m, *zs["RUW"]))
    print(f"[moment-loss] {kind} N={n} support vs dense: {ratio:.3e} (kind=mse yardstick {zs['mse_ratio']:.3e})")
    assert ratio <= GRAD_FACTOR * zs["mse_ratio"], (ratio, zs["mse_ratio"])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("dense", "bg_support"))
def test_alpha(form):
    """alpha = 0 is the MSE (value and gradient, against kind="mse" itself); alpha = 0.5 against the oracle."""
    z = _case(129, form)
    l0, s0, d0 = _device(z["c"], z["tr"], "mse+pearson", alpha=0.0)
    lm, sm, _ = _device(z["c"], z["tr"], "mse")
    _close(float(l0), float(lm), "alpha=0 loss")
    _close(float(s0[7]), float(sm[7]), "alpha=0 mse")
    ratio = normalised(float((d0.double() - z["dc_mse"].double()).abs().max()),
                       term_scale("mse", z["m"], *z["RUW"]))
    print(f"[moment-loss] alpha=0 {form}: vs kind=mse {ratio:.3e} (yardstick {z['mse_ratio']:.3e})")
    assert ratio <= GRAD_FACTOR * z["mse_ratio"], (ratio, z["mse_ratio"])
    loss, st, dc = _device(z["c"], z["tr"], "mse+pearson", alpha=0.5)
    v, g, m = oracle(z["c"], z["T"], "mse+pearson", 0.5)
    _check_stats(f"alpha=0.5 {form}", "mse+pearson", st, loss, v, m, 0.5)
    _check_gradient(f"alpha=0.5 {form}", dc, g, "mse+pearson", m, z["RUW"], z["mse_ratio"], 0.5)


def _mse_ratio(c, T, tr):
    R, U, W = row_sums(c, T)
    _, g_mse, m = oracle(c, T, "mse")
    _, _, dc_mse = _device(c, tr, "mse")
    return (R, U, W), normalised(float((dc_mse.double() - g_mse).abs().max()), term_scale("mse", m, R, U, W))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_near_fit(kind):
    """d ~ 1.3 t with 1 % noise: r ~ 1 and the three terms of the combine cancel."""
    n = 129
    c = _coords(n, 7)
    rng = np.random.default_rng(7)
    cd = c.double()
    D = torch.cdist(cd, cd, compute_mode="donot_use_mm_for_euclid_dist").numpy()
    noise = np.triu(0.01 * rng.standard_normal((n, n)), 1)
    t = D / 1.3 * (1.0 + noise + noise.T)
    np.fill_diagonal(t, 0.05 * rng.random(n))
    T = torch.tensor(t.astype(np.float32))
    tr = _truth("dense", T)
    RUW, ref = _mse_ratio(c, T, tr)
    loss, st, dc = _device(c, tr, kind)
    v, g, m = oracle(c, T, kind)
    assert m["r"] > 0.99
    _check_stats(f"near-fit {kind}", kind, st, loss, v, m)
    _check_gradient(f"near-fit {kind}", dc, g, kind, m, RUW, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("dense", "bg_support"))
@pytest.mark.parametrize("kind", KINDS)
def test_collapsed_coordinates(kind, form):
    n, alpha = 129, 0.7
    c = torch.tensor(np.tile(np.array([[0.3, -0.2, 0.1]], dtype=np.float32), (n, 1)))
    T = _dense_truth(n, 5) if form == "dense" else _bg_truth(n, 5)
    tr = _truth(form, T)
    loss, st, dc = _device(c, tr, kind, alpha)
    v, g, m = oracle(c, T, kind, alpha)
    assert np.isfinite(float(loss)) and bool(torch.isfinite(st[:8]).all()) and bool(torch.isfinite(st[9:]).all())
    assert np.isnan(float(st[8]))
    _close(float(st[10]), v, f"collapsed {kind} value")
    if kind == "mse+pearson":
        _close(float(st[10]), m["mse"] + alpha, "collapsed: mse + alpha")
    assert float(g.abs().max()) == 0.0
    assert bool((dc == 0).all()), dc.abs().max()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("dense", "bg_support"))
@pytest.mark.parametrize("kind", KINDS)
def test_two_coincident_points(kind, form):
    """Two equal rows among random ones: that pair has d = 0, u = 0 (the oracle masks it the same way)."""
    n = 129
    c = _coords(n, 11)
    c[77] = c[5]
    T = _dense_truth(n, 11) if form == "dense" else _bg_truth(n, 11)
    tr = _truth(form, T)
    RUW, ref = _mse_ratio(c, T, tr)
    loss, st, dc = _device(c, tr, kind)
    v, g, m = oracle(c, T, kind)
    assert np.isfinite(float(loss)) and bool(torch.isfinite(dc).all())
    _check_stats(f"coincident {kind} {form}", kind, st, loss, v, m)
    _check_gradient(f"coincident {kind} {form}", dc, g, kind, m, RUW, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("dense", "bg_support"))
@pytest.mark.parametrize("kind", KINDS)
def test_two_calls_give_the_same_bits(kind, form):
    z = _case(300, form)
    a, b = _device(z["c"], z["tr"], kind, 0.5), _device(z["c"], z["tr"], kind, 0.5)
    assert a[0].view(torch.int32).item() == b[0].view(torch.int32).item()
    assert torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


@functools.lru_cache(maxsize=None)
def _chr19():
    import hicgat
    mfx = load_golden("model_GATNetSelectiveResidualsUpdated.npz")
    g = load_golden("graph_chr19_1mb.npz")
    y = torch.tensor(g["matrix"], device=DEV)
    y.fill_diagonal_(0)
    data = hicgat.Data(x=torch.tensor(mfx["x"], device=DEV), edge_index=hicgat.Adj.from_dense_device(y), y=y)
    return mfx, g, data, hicgat.Truth.from_contacts(y, 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_training_graph_replay_equals_eager(kind):
    import hicgat
    _, _, data, tr = _chr19()
    runs = []
    for graph in (True, False):
        torch.manual_seed(0)
        model = hicgat.GATNetSelectiveResidualsUpdated().to(DEV)
        opt, hist = hicgat.train.train(model, data, tr, steps=6, loss=kind, graph=graph, alpha=0.5)
        runs.append((hist, opt.flat.detach().clone()))
    (hg, pg), (he, pe) = runs
    assert len(hg) == 6 and all(np.isfinite(hg))
    assert hg == he, (hg, he)
    assert torch.equal(pg.view(torch.int32), pe.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_training_first_step_matches_the_cpu_run(kind):
    """Step 1 on chr19 1 mb: the loss against the oracle loss on the device's own coordinates, and
    d loss / d dense3.weight against the CPU oracle model's backward of the oracle's d loss / d coords
    (the loss part of the chain in fp64).  1e-5 on the loss and 2e-4 on the gradient, the tolerances of
    tests/test_gpu_parity.py::test_train_loop_tracks_oracle for its teacher-forced steps."""
    import hicgat
    from oracle import gat as og
    mfx, g, data, tr = _chr19()
    alpha = 0.5
    torch.manual_seed(0)
    model = hicgat.GATNetSelectiveResidualsUpdated().to(DEV)
    model.train()
    loss, stats, coords = model.loss(data.x, data.edge_index, tr, kind, alpha=alpha)
    loss.backward()
    v, gc, _ = oracle(coords.detach().cpu(), tr.dense().cpu(), kind, alpha)
    assert abs(float(loss) - v) <= 1e-5 * abs(v), (float(loss), v)
    torch.manual_seed(0)
    ref = og.GATNetSelectiveResidualsUpdated()
    ref.train()
    radj = (torch.tensor(g["rowptr"]), torch.tensor(g["col"]))
    c_ref = ref.get_model(torch.tensor(mfx["x"]), radj)
    c_ref.backward(gc.to(c_ref.dtype))
    gw, gr = model.dense3.weight.grad.cpu().double(), ref.dense3.weight.grad.double()
    rel = float((gw - gr).abs().max() / gr.abs().max())
    print(f"[moment-loss] {kind} step 1: loss {float(loss):.7g} vs {v:.7g}, dense3.weight grad rel {rel:.2e}")
    assert rel < 2e-4, rel


@pytest.mark.gpu
def test_sharded_trainer_refuses_the_new_kinds():
    import hicgat
    from hicgat import dist
    _, _, data, tr = _chr19()
    model = hicgat.GATNetSelectiveResidualsUpdated().to(DEV)
    for kind in KINDS:
        with pytest.raises((NotImplementedError, KeyError), match=re.escape(kind)):
            dist.ShardedTrainer(model, data.x, data.edge_index, tr, kind=kind)

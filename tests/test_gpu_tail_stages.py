"""The one-kernel MLP tail (csrc/tail_fused.hip), every entry point, stage by stage against the fp64
reference of tests/tail_ref.py at small and ragged row counts.

Each stage of the kernel is compared with the fp64 value of ITS formula on the kernel's own output
of the stage before, element by element, within the bound derived in tail_ref's docstring (never a
fraction of the tensor's maximum): one wrong row, one wrong column, a LayerNorm partial that took a
padding row or a wrong statistic cannot hide.  The launches go through the C ABI with buffers
allocated here: every output sits between 16 guard rows (one fixed bit pattern) that must survive,
the workspaces have exactly hicgat_tail_bwd_workspace_bytes, x has ldx = 640, the heads' aggregates
a head stride that is not 2 M 512, and coords lies inside a larger buffer.  Every case runs with the
row-major weights and with a hicgat_tail_pack copy, which must agree bitwise.

M: 1 (one live row), 15, 16, 17 (around one tile), 47 (three tiles, ragged last), 2033 (128 tiles:
every value of the wave-to-column rotation (tile >> 3) & 15, and a last tile of one live row); the
plain forward also at 16 CUs + 1, the smallest M on its persistent path.

Each check prints ``tail-stage <form> M=<M> <stage>: max |err|/bound`` before it asserts."""
import pytest
import torch

import tail_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 16
PATTERN = 0x4B3C2D1E          # a finite float (about 1.2e7) no stage produces
MS = (1, 15, 16, 17, 47, 2033)
LDX640 = (17, 47, 2033)       # the plain forward reads x out of a [M, 640] buffer here (ldx > 512)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import hicgat  # noqa: F401  (fails loudly if libhicgat.so is missing)


def _L():
    from hicgat import _lib
    return _lib


class Guarded:
    """[rows, cols] floats between GUARD rows of PATTERN on either side, in one allocation."""

    def __init__(self, rows, cols, init=None):
        self.rows = rows
        self.buf = torch.empty((rows + 2 * GUARD, cols), dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(PATTERN)
        self.t = self.buf[GUARD:GUARD + rows]
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:GUARD] == PATTERN).all()) and bool((b[GUARD + self.rows:] == PATTERN).all())

    def cpu(self):
        return self.t.detach().cpu().clone()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).clone()


class Inputs:
    """Device copies of the inputs with their bits before the launch."""

    def __init__(self, **ts):
        self.t = {k: v.to(DEV) if not v.is_cuda else v for k, v in ts.items()}
        self.before = {k: _bits(v) for k, v in self.t.items()}

    def __getitem__(self, k):
        return self.t[k]

    def assert_unchanged(self, what):
        for k, v in self.t.items():
            assert torch.equal(_bits(v), self.before[k]), (what, "input changed", k)


def _addr(t):
    """A tensor's address for a field of the C ABI's operand structs (None: NULL)."""
    return None if t is None else t.data_ptr()


def _pack(P, heads):
    _lib = _L()
    lib = _lib.lib()
    n = int(lib.hicgat_tail_pack_bytes())
    pack = torch.empty(n // 4, dtype=torch.float32, device=DEV)
    _lib.check(lib.hicgat_tail_pack(_lib.ptr(P["W1c"]), _lib.ptr(P["W2c"]), _lib.ptr(P["Wh"]) if heads else None,
                                    _lib.ptr(pack), n, _lib.stream(pack.device)), "hicgat_tail_pack")
    return pack


def _within(form, M, stage, got, ref):
    """Every element of the kernel's fp32 ``got`` within the stage's bound of the fp64 value."""
    val, bnd = ref
    assert got.shape == val.shape, (form, M, stage, got.shape, val.shape)
    err = (got.double() - val).abs()
    ratio = err / bnd                                  # bound 0 (a copy): any error is infinitely far out
    ratio[(bnd == 0) & (err == 0)] = 0.0
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = float(ratio.max())
    at = divmod(int(ratio.argmax()), ratio.shape[1])
    print(f"tail-stage {form} M={M} {stage}: max |err|/bound = {worst:.4f} at row {at[0]} col {at[1]}")
    assert worst <= 1.0, (f"{form} M={M} stage {stage}: row {at[0]} col {at[1]} got {float(got[at]):.9g} "
                          f"fp64 {float(val[at]):.9g} bound {float(bnd[at]):.3g} ({int((ratio > 1).sum())} elements out)")


def _same_bits(form, M, a, b):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (form, M, "packed != row-major", k)


# ------------------------------------------------------------------------------------------ forward
FWD_OUT = (("Y1", 512), ("st1", 2), ("z1", 256), ("Y2", 256), ("st2", 2), ("z2", 128), ("y3", 64), ("st3", 2),
           ("z3", 64), ("coords", 3))
WKEYS = ("W1c", "b1c", "g1", "be1", "W2c", "b2c", "g2", "be2", "W3", "b3", "g3", "be3", "W4", "b4")


def _run_forward(M, small, heads, ldx, use_pack):
    _lib = _L()
    lib, p = _lib.lib(), _lib.ptr
    Pc, x, X4 = R.forward_inputs(M, small)
    ins = {k: Pc[k] for k in WKEYS + ("Wh", "bh")}
    if heads:
        ins["X4"] = X4
    else:
        xb = torch.full((M, ldx), float("nan"))      # the columns past 512 are never read
        xb[:, :512] = x
        ins["xbuf"] = xb
    I = Inputs(**ins)
    out = {k: Guarded(M, c) for k, c in FWD_OUT + ((("Y0", 512), ("O", 512)) if heads else ())}
    pack = _pack(I, heads) if use_pack else None
    w = _lib.TailWeights(eps=R.EPS32, pack=_addr(pack), **{k: _addr(I[k]) for k in WKEYS})
    acts = _lib.TailActs(**{k: _addr(out[k].t) for k, _ in FWD_OUT if k != "coords"})
    if heads:
        xa = I["X4"][:, :, :M]                        # head stride 2 (M + 5) 512, not 2 M 512
        assert xa.stride(0) != 2 * M * 512 and xa.stride(2) == 512
        xv, ld = xa, xa.stride(2)
        gat = _lib.TailGat(form=_lib.TAIL_HEADS, xa_head_stride=xa.stride(0), Wh=_addr(I["Wh"]), bh=_addr(I["bh"]),
                           Y0=_addr(out["Y0"].t), O=_addr(out["O"].t))
    else:
        xv, gat = I["xbuf"][:, :512], None
        ld = xv.stride(0)
    _lib.check(lib.hicgat_tail_fwd(w, p(xv), ld, M, acts, p(out["coords"].t), gat,
                                   _lib.stream(out["Y1"].buf.device)), "hicgat_tail_fwd")
    torch.cuda.synchronize()
    what = ("fwd", M, small, heads, use_pack)
    for k, g in out.items():
        assert g.intact(), (what, "guard rows overwritten", k)
    I.assert_unchanged(what)          # X4[:, 1] and the rows past M among them
    return {k: g.cpu() for k, g in out.items()}


def _forward_case(M, small=False, heads=False):
    form = "fwd_heads" if heads else ("fwd_small" if small else "fwd")
    ldx = 640 if (M in LDX640 or M > 2033) else 512
    o = _run_forward(M, small, heads, ldx, False)
    _same_bits(form, M, o, _run_forward(M, small, heads, ldx, True))
    P, x, X4 = R.forward_inputs(M, small)
    if heads:
        ref = R.heads_fwd(X4[:, 0, :M], P["Wh"], P["bh"])
        _within(form, M, "Y0", o["Y0"], ref)
        _within(form, M, "O", o["O"], (torch.relu(ref[0]), ref[1]))
        assert bool((o["O"] == torch.relu(o["Y0"])).all()), (form, M, "O != relu(Y0)")
        x = o["O"]
    T = dict(o, x=x)
    for out, a, w, b in (("Y1", "x", "W1c", "b1c"), ("Y2", "z1", "W2c", "b2c"), ("y3", "z2", "W3", "b3"),
                         ("coords", "z3", "W4", "b4")):
        _within(form, M, out, o[out], R.gemm_bias(T[a], P[w], P[b]))
        if out != "coords":
            i = out[-1]
            W = {"1": 256, "2": 128, "3": 64}[i]
            st, z = R.ln_fwd(o[out], P["g" + i], P["be" + i], R.EPS32, W, i != "3")
            _within(form, M, "st" + i, o["st" + i], st)
            _within(form, M, "z" + i, o["z" + i], z)


@pytest.mark.parametrize("M", MS + ("persist",))
def test_forward_stages(M):
    """hicgat_tail_fwd, the plain form; ``persist``: M = 16 CUs + 1, the smallest grid of more than one round,
    which takes the persistent kernel (its second tile per workgroup arrives by LDS-DMA)."""
    if M == "persist":
        M = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    _forward_case(M)


def test_forward_stages_small_scale():
    """M = 47 with x scaled by 1e-3 and b1c = 0: the first LayerNorm's row variance is of eps's order,
    so eps inside the square root matters (test_tail_ref_host: a kernel without it leaves the bound)."""
    _forward_case(47, small=True)


def _need_waves(n, exact=False):
    w = int(_L().lib().hicgat_tail_bwd_waves())
    if (w != n) if exact else (w < n):
        pytest.skip(f"this form needs {'' if exact else '>= '}{n} waves per workgroup; the library has {w}")


@pytest.mark.parametrize("M", MS)
def test_forward_heads_stages(M):
    """hicgat_tail_fwd with HICGAT_TAIL_HEADS: Y0, O = relu(Y0) and the tail on O."""
    _need_waves(8)
    _forward_case(M, heads=True)


# ----------------------------------------------------------------------------------------- backward
BWD_OUT = (("dY1", 512), ("dY2", 256), ("dy3", 64))
BKEYS = ("W4", "W3", "W2c", "W1c", "g1", "be1", "g2", "be2", "g3", "be3")


def _run_backward(M, zero_row, form, act, use_pack):
    """form: plain / rows / heads.  Returns the outputs' CPU copies."""
    _lib = _L()
    lib, p = _lib.lib(), _lib.ptr
    Pc, B = R.backward_inputs(M, zero_row)
    ins = {k: Pc[k] for k in BKEYS + ("Wh", "bh")}
    ins.update({k: B[k] for k in ("dc", "Y1", "st1", "Y2", "st2", "y3", "st3", "y", "out2")})
    I = Inputs(**ins)
    out = {k: Guarded(M, c) for k, c in BWD_OUT}
    nt = -(-M // 16)
    ws, ws_bytes = [], []
    for i, W in (("1", 256), ("2", 128), ("3", 64)):
        g = out["p" + i] = Guarded(nt, 2 * W)
        nbytes = int(lib.hicgat_tail_bwd_workspace_bytes(M, W))
        assert nbytes == g.t.numel() * 4              # exactly the size the library asks for
        ws.append(_addr(g.t))
        ws_bytes.append(nbytes)
    pack = _pack(I, form == "heads") if use_pack else None
    w = _lib.TailWeights(pack=_addr(pack), **{k: _addr(I[k]) for k in BKEYS})      # b*, eps: not read
    acts = _lib.TailActs(**{k: _addr(I[k]) for k in ("Y1", "st1", "Y2", "st2", "y3", "st3")})      # nor z*
    grads = _lib.TailGrads(ws=tuple(ws), ws_bytes=tuple(ws_bytes), **{k: _addr(out[k].t) for k, _ in BWD_OUT})
    if form == "plain":
        out["dx"] = Guarded(M, 512)
        grads.dx, gat = _addr(out["dx"].t), None
    else:
        out["dout"] = Guarded(M, 512)
        out["rs"] = Guarded(M, 8, init=B["rs"])
        gat = _lib.TailGat(act=act, Y0=_addr(I["y"]), bh=_addr(I["bh"]), dout=_addr(out["dout"].t),
                           row_stats=_addr(out["rs"].t))
        if form == "rows":
            gat.form, gat.out2 = _lib.TAIL_ROWS, _addr(I["out2"])
        else:
            out["dxa"] = Guarded(M, 1024)
            gat.form, gat.Wh, gat.dxa = _lib.TAIL_HEADS, _addr(I["Wh"]), _addr(out["dxa"].t)
    _lib.check(lib.hicgat_tail_bwd(w, acts, p(I["dc"]), M, grads, gat, _lib.stream(out["dY1"].buf.device)),
               "hicgat_tail_bwd")
    torch.cuda.synchronize()
    what = ("bwd", form, M, zero_row, act, use_pack)
    for k, g in out.items():
        assert g.intact(), (what, "guard rows overwritten", k)
    I.assert_unchanged(what)
    return {k: g.cpu() for k, g in out.items()}


def _check_chain(form, M, zero_row, o):
    """dy3 / dY2 / dY1 and the three partial workspaces; |pre| off the kink (or exactly 0)."""
    P, B = R.backward_inputs(M, zero_row)
    for dY, i, dzin, wt, y, W, res in (("dy3", "3", B["dc"], P["W4"], B["y3"], 64, False),
                                       ("dY2", "2", o["dy3"], P["W3"], B["Y2"], 128, True),
                                       ("dY1", "1", o["dY2"], P["W2c"], B["Y1"], 256, True)):
        s = R.ln_bwd(dzin, wt, y, B["st" + i], P["g" + i], P["be" + i], W, res)
        zero = s["pre"] == 0
        assert int(zero.sum()) == (4 if zero_row else 0)
        assert float(s["pre"][~zero].abs().min()) > 1e-5      # the kernel's own pre differs by a few 1e-7
        _within(form, M, dY, o[dY], s["dY"])
        _within(form, M, "p" + i, o["p" + i], s["p"])


def _backward_case(M, form, act=0, zero_row=False):
    name = f"bwd_{form}" + (f"_act{act}" if form != "plain" else "") + ("_zero_row" if zero_row else "")
    o = _run_backward(M, zero_row, form, act, False)
    _same_bits(name, M, o, _run_backward(M, zero_row, form, act, True))
    P, B = R.backward_inputs(M, zero_row)
    _check_chain(name, M, zero_row, o)
    if form == "plain":
        _within(name, M, "dx", o["dx"], R.gemm_t(o["dY1"], P["W1c"]))
        return o
    assert torch.equal(o["rs"][:, :4].contiguous().view(torch.int32), B["rs"][:, :4].contiguous().view(torch.int32)), \
        (name, M, "row_stats[:, 0:4] clobbered")
    _within(name, M, "dout", o["dout"], R.dout_stage(o["dY1"], P["W1c"], B["y"], act))
    if form == "rows":
        _within(name, M, "rs[4:8]", o["rs"][:, 4:8], R.rows_stats(o["dout"], B["y"], P["bh"], B["out2"], B["rs"][:, 4:6]))
    else:
        _within(name, M, "delta", o["rs"][:, 4:6], R.heads_delta(o["dout"], B["y"], P["bh"]))
        _within(name, M, "rs[6:8]", o["rs"][:, 6:8], R.heads_moved(B["rs"]))
        _within(name, M, "dxa", o["dxa"], R.heads_dxa(o["dout"], P["Wh"]))
    return o


@pytest.mark.parametrize("M", MS)
def test_backward_stages(M):
    """hicgat_tail_bwd, the plain form: dy3, dY2, dY1, dx and the LayerNorm partial rows."""
    _backward_case(M, "plain")


def test_backward_stages_pre_exactly_zero():
    """M = 47, the last live row of every Y equal to its st mean with beta = 0 in four columns: pre = 0
    exactly there, and the gradient is 0 (the fp64 stage masks with [pre > 0], as torch's relu)."""
    _backward_case(47, "plain", zero_row=True)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M", MS)
def test_backward_rows_epilogue(M, act):
    """hicgat_tail_bwd with HICGAT_TAIL_ROWS: the chain, dout and row_stats[:, 4:8] against fp64, and dout /
    row_stats[:, 4:8] bitwise hicgat_gat_agg_bwd_rows on the plain form's dx (the kernel's claim)."""
    _need_waves(16, exact=True)
    o = _backward_case(M, "rows", act)
    plain = _run_backward(M, False, "plain", 0, False)
    _lib = _L()
    lib, p = _lib.lib(), _lib.ptr
    P, B = R.backward_inputs(M)
    I = Inputs(dx=plain["dx"], y=B["y"], bh=P["bh"], out2=B["out2"])
    dout, rs = Guarded(M, 512), Guarded(M, 8, init=B["rs"])
    _lib.check(lib.hicgat_gat_agg_bwd_rows(M, 2, 256, 0, M, act, p(I["dx"]), p(I["y"]), p(I["bh"]), p(I["out2"]),
                                           p(dout.t), 512, p(rs.t), _lib.stream(rs.buf.device)),
               "hicgat_gat_agg_bwd_rows")
    torch.cuda.synchronize()
    assert dout.intact() and rs.intact()
    I.assert_unchanged(("agg_bwd_rows", M, act))
    want_dout = dout.cpu() if act else plain["dx"]      # act = 0: the separate pass leaves dout = dx unwritten
    assert torch.equal(o["dout"].view(torch.int32), want_dout.view(torch.int32)), (M, act, "dout")
    assert torch.equal(o["rs"].view(torch.int32), rs.cpu().view(torch.int32)), (M, act, "row_stats")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M", MS)
def test_backward_heads_epilogue(M, act):
    """hicgat_tail_bwd with HICGAT_TAIL_HEADS: the chain, dout, delta, the moved S3 and dxa."""
    _need_waves(8)
    _backward_case(M, "heads", act)

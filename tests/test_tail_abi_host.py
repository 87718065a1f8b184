"""CPU: what hicgat_tail_fwd / hicgat_tail_bwd (include/hicgat.h) refuse, and with which code.

Every rejection returns before any HIP call, so the operands are addresses inside one host buffer
that nothing dereferences.  Each case starts from an operand set that is valid for its form at M = 17
and breaks exactly one thing; no case passes a valid set with M > 0 (that would launch).  The expected
codes are the rules of the five positional entry points these two replaced: a NULL required pointer,
M < 0, a bad ldx or head stride, a short workspace, HEADS with a pack made without Wh -> EINVAL;
a pointer the kernels read as float4 off a 16-B boundary -> EUNSUPPORTED; M == 0 -> OK; and, checked
before all of that, a form the library's wave count cannot run -> EUNSUPPORTED.  New with the structs:
a NULL struct and an unknown form -> EINVAL."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
M = 17
PLAIN, HEADS, ROWS = 0, 1, 2                         # include/hicgat.h HICGAT_TAIL_*

_ARENA = ctypes.create_string_buffer(80 * 16)
_BASE = (ctypes.addressof(_ARENA) + 15) & ~15


def _slot(k):
    """The k-th 16-B aligned host address."""
    assert 0 < k < 78
    return _BASE + 16 * k


W_FWD = "W1c W2c W3 W4 g1 be1 g2 be2 g3 be3 b1c b2c b3 b4".split()
W_BWD = W_FWD[:10]                                   # the backward reads no bias (and no eps)
A_FWD = "Y1 st1 Y2 st2 y3 st3 z1 z2 z3".split()
A_BWD = A_FWD[:6]                                    # ... and no z
G_BWD = ["dY1", "dY2", "dy3", ("ws", 0), ("ws", 1), ("ws", 2)]
GAT_REQUIRED = {("fwd", HEADS): "Wh bh Y0 O".split(), ("bwd", HEADS): "dout Y0 Wh bh row_stats dxa".split(),
                ("bwd", ROWS): "dout Y0 bh out2 row_stats".split()}
# the pointers the launch code tests with & 15 (beside the pack)
GAT_ALIGNED = {("fwd", HEADS): "Wh Y0 O".split(), ("bwd", HEADS): "Y0 bh dout row_stats".split(),
               ("bwd", ROWS): "Y0 bh dout row_stats out2".split()}
CASES = [("fwd", PLAIN), ("fwd", HEADS), ("bwd", PLAIN), ("bwd", ROWS), ("bwd", HEADS)]


def _L():
    from hicgat import _lib
    _lib.load()
    return _lib


class Operands:
    """A valid operand set of one direction and form; ``call`` runs the entry point on it.  A field is
    (struct, name) or (struct, (name, index)); struct None: a plain argument."""

    def __init__(self, direction, form):
        L = _L()
        self.direction, self.form, self.M, self.ldx = direction, form, M, 512
        self.x, self.coords = _slot(1), _slot(2)     # bwd: coords is dcoords, x is not passed
        self.s = {"w": L.TailWeights(eps=1e-5), "a": L.TailActs(), "g": L.TailGrads(), "gat": None}
        if form != PLAIN:
            self.s["gat"] = L.TailGat(form=form, act=1, xa_head_stride=2 * M * 512)
        for k, (where, field) in enumerate(self.required()):
            self.set(where, field, _slot(3 + k))
        for i, W in enumerate((256, 128, 64)):
            self.s["g"].ws_bytes[i] = L.load().hicgat_tail_bwd_workspace_bytes(M, W)

    def required(self):
        """Every pointer this direction and form requires."""
        fwd = self.direction == "fwd"
        r = [(None, "coords")] + [("w", n) for n in (W_FWD if fwd else W_BWD)]
        r += [("a", n) for n in (A_FWD if fwd else A_BWD)]
        if fwd:
            r += [(None, "x")]
        else:
            r += [("g", n) for n in G_BWD] + ([("g", "dx")] if self.form == PLAIN else [])
        return r + [("gat", n) for n in GAT_REQUIRED.get((self.direction, self.form), [])]

    def aligned(self):
        """Every pointer the launch code tests with & 15."""
        r = [("w", "pack")] + [("gat", n) for n in GAT_ALIGNED.get((self.direction, self.form), [])]
        if self.direction == "fwd":
            r += [(None, "x"), ("w", "W1c"), ("w", "W2c"), ("w", "W3")]
        return r

    def set(self, where, field, value):
        obj = self if where is None else self.s[where]
        if isinstance(field, tuple):
            getattr(obj, field[0])[field[1]] = value
        else:
            setattr(obj, field, value)

    def get(self, where, field):
        obj = self if where is None else self.s[where]
        return getattr(obj, field[0])[field[1]] if isinstance(field, tuple) else getattr(obj, field)

    def call(self):
        lib, s = _L().load(), self.s
        if self.direction == "fwd":
            return lib.hicgat_tail_fwd(s["w"], self.x, self.ldx, self.M, s["a"], self.coords, s["gat"], None)
        return lib.hicgat_tail_bwd(s["w"], s["a"], self.coords, self.M, s["g"], s["gat"], None)


def _expect(form, code):
    """The wave-count rule comes first: HEADS needs >= 8 waves per workgroup, ROWS exactly 16."""
    waves = _L().load().hicgat_tail_bwd_waves()
    if (form == HEADS and waves < 8) or (form == ROWS and waves != 16):
        return EUNSUPPORTED
    return code


@pytest.mark.parametrize("direction,form", CASES)
def test_each_required_pointer_null_is_einval(direction, form):
    fields = Operands(direction, form).required()
    assert len(fields) >= 24 and len(set(fields)) == len(fields)
    for where, field in fields:
        o = Operands(direction, form)
        assert o.get(where, field), (where, field)
        o.set(where, field, None)
        assert o.call() == _expect(form, EINVAL), (where, field)


@pytest.mark.parametrize("direction,form", CASES)
def test_each_float4_pointer_off_16_bytes_is_eunsupported(direction, form):
    for where, field in Operands(direction, form).aligned():
        o = Operands(direction, form)
        o.set(where, field, (o.get(where, field) or _slot(70)) + 4)      # the pack is NULL in the valid set
        assert o.call() == EUNSUPPORTED, (where, field)


@pytest.mark.parametrize("direction,form", CASES)
def test_row_count_rules(direction, form):
    L = _L()
    o = Operands(direction, form)
    o.M = -1
    assert o.call() == _expect(form, EINVAL)
    o = Operands(direction, form)
    o.M, o.x, o.coords = 0, None, None
    o.s = {"w": L.TailWeights(), "a": L.TailActs(), "g": L.TailGrads(),
           "gat": None if form == PLAIN else L.TailGat(form=form)}
    assert o.call() == _expect(form, OK)             # nothing else is looked at


@pytest.mark.parametrize("form", [PLAIN, HEADS])
def test_forward_ldx_and_head_stride(form):
    for ldx in (508, 514):
        o = Operands("fwd", form)
        o.ldx = ldx
        assert o.call() == _expect(form, EINVAL), ldx
    if form == HEADS:
        o = Operands("fwd", form)
        o.s["gat"].xa_head_stride += 2
        assert o.call() == _expect(form, EINVAL)


@pytest.mark.parametrize("form", [PLAIN, ROWS, HEADS])
def test_each_workspace_one_byte_short_is_einval(form):
    for i in range(3):
        o = Operands("bwd", form)
        o.s["g"].ws_bytes[i] -= 1
        assert o.call() == _expect(form, EINVAL), i


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_heads_with_a_pack_made_without_wh_is_einval(direction):
    o = Operands(direction, HEADS)
    o.s["w"].pack = _slot(70)                        # no hicgat_tail_pack ever wrote there
    assert o.call() == _expect(HEADS, EINVAL)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_unknown_form_is_einval(direction):
    for bad in (ROWS + 1, -1) + ((ROWS,) if direction == "fwd" else ()):      # ROWS is a form of the backward
        o = Operands(direction, HEADS)
        o.s["gat"].form = bad
        assert o.call() == EINVAL, bad


@pytest.mark.parametrize("direction,form", CASES)
def test_null_struct_is_einval(direction, form):
    for name in ("w", "a") + (("g",) if direction == "bwd" else ()):
        o = Operands(direction, form)
        o.s[name] = None
        assert o.call() == _expect(form, EINVAL), name


def test_ctypes_structs_mirror_the_header():
    """Field names, order and types of the four operand structs, and the form constants."""
    L = _L()
    with open(os.path.join(ROOT, "include", "hicgat.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    scalars = {"int": L.c_int, "int64_t": L.c_i64, "float": L.c_f, "size_t": L.c_sz}
    for cname, cls in (("hicgat_tail_weights", L.TailWeights), ("hicgat_tail_acts", L.TailActs),
                       ("hicgat_tail_grads", L.TailGrads), ("hicgat_tail_gat", L.TailGat)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % cname, text).group(1)
        want = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, names = re.match(r"(?:const\s+)?(\w+)\s+(.*)", decl, re.S).groups()
            for nm in (n.strip() for n in names.split(",")):
                t = L.c_p if nm.startswith("*") else scalars[base]
                arr = re.search(r"\[(\d+)\]", nm)
                want.append((re.sub(r"[*\s]|\[\d+\]", "", nm), t * int(arr.group(1)) if arr else t))
        assert list(cls._fields_) == want, cname
    consts = {k: int(v) for k, v in re.findall(r"#define HICGAT_TAIL_(\w+) (\d+)", text)}
    assert consts == {"PLAIN": PLAIN, "HEADS": HEADS, "ROWS": ROWS} == \
        {"PLAIN": L.TAIL_PLAIN, "HEADS": L.TAIL_HEADS, "ROWS": L.TAIL_ROWS}

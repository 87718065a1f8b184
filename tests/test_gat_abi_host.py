"""CPU: what hicgat_gat_agg_fwd / hicgat_gat_agg_bwd_src / hicgat_gat_attn_mask (include/hicgat.h) refuse,
and with which code.

Every rejection returns before any HIP call, so the operands are 16-B aligned addresses inside one host
buffer that nothing dereferences.  Each case starts from an operand set that is valid for its pass and
form at N = 9, rows [0, 9), and breaks exactly one thing (two for the precedence cases); no case passes a
valid set with a non-empty range (that would launch).  The expected codes are the rules of the six
positional entry points these two replaced, in their order: the dropout parameters, the flags, the sizes
and the row range, act -> EINVAL; then the shape -> EUNSUPPORTED; the row strides -> EINVAL; an empty
range -> OK; a NULL required pointer, splits outside 1..64, a short, missing or misaligned workspace ->
EINVAL.  New with the structs: a NULL graph or feats, dropout together with tiles, and the round-robin
flag together with tiles -> EINVAL."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
N = 9
SHAPE = {"plain": (2, 128), "drop": (2, 128), "tiles": (2, 256)}
CASES = [(d, f) for d in ("fwd", "src") for f in ("plain", "drop", "tiles")]

_ARENA = ctypes.create_string_buffer(48 * 16)
_BASE = (ctypes.addressof(_ARENA) + 15) & ~15


def _slot(k):
    """The k-th 16-B aligned host address."""
    assert 0 < k < 46
    return _BASE + 16 * k


def _L():
    from hicgat import _lib
    _lib.load()
    return _lib


GRAPH = [("graph", "rowptr"), ("graph", "col")]
FEATS = [("feats", "h"), ("feats", "a_src"), ("feats", "a_dst")]
PLAIN = {"fwd": "bias out row_stats".split(), "src": "row_stats dout att_src att_dst dh da_src".split()}
TILES = [("tiles", n) for n in "rowptr_s col_s tptr tcol tmask".split()]
N_REQUIRED = {("fwd", "plain"): 8, ("fwd", "drop"): 8, ("fwd", "tiles"): 13,
              ("src", "plain"): 11, ("src", "drop"): 11, ("src", "tiles"): 14}


class Operands:
    """A valid operand set of one pass and form; ``call`` runs the entry point on it.  A field is
    (struct, name); struct None: a plain argument."""

    def __init__(self, direction, form):
        L = _L()
        H, C = SHAPE[form]
        self.direction, self.form = direction, form
        self.act, self.flags, self.ld_stats, self.ld_dout, self.out2 = 1, 0, 4 * H, H * C, None
        self.s = {"graph": L.GatGraph(N=N, nnz=40, row_begin=0, row_end=N),
                  "feats": L.GatFeats(H=H, C=C, neg_slope=0.2),
                  "drop": L.AttnDrop(p=0.5, seed=1, step_value=1, site=3) if form == "drop" else None,
                  "tiles": L.GatTiles(ntiles=3, splits=1) if form == "tiles" else None}
        for k, (where, field) in enumerate(self.required()):
            self.set(where, field, _slot(1 + k))
        if direction == "src" and form == "tiles":     # not required there, but given in the valid set
            self.s["graph"].rowptr, self.s["graph"].col = _slot(20), _slot(21)

    def required(self):
        """Every pointer this pass and form requires."""
        r = FEATS + [(None, n) for n in PLAIN[self.direction]]
        if self.form == "tiles":
            return r + TILES + (GRAPH if self.direction == "fwd" else [])
        return r + GRAPH

    def set(self, where, field, value):
        setattr(self if where is None else self.s[where], field, value)

    def get(self, where, field):
        return getattr(self if where is None else self.s[where], field)

    def null_everything(self):
        """Every pointer NULL and the tiles zeroed; the sizes, the shape and the dropout parameters stay."""
        L = _L()
        g, f = self.s["graph"], self.s["feats"]
        self.s["graph"] = L.GatGraph(N=g.N, nnz=g.nnz, row_begin=g.row_begin, row_end=g.row_end)
        self.s["feats"] = L.GatFeats(H=f.H, C=f.C)
        if self.form == "tiles":
            self.s["tiles"] = L.GatTiles()
        for n in PLAIN[self.direction]:
            setattr(self, n, None)

    def call(self):
        lib, s = _L().load(), self.s
        if self.direction == "fwd":
            return lib.hicgat_gat_agg_fwd(s["graph"], s["feats"], self.bias, self.act, self.out, self.out2,
                                          self.row_stats, s["drop"], s["tiles"], None)
        return lib.hicgat_gat_agg_bwd_src(s["graph"], s["feats"], self.row_stats, self.ld_stats, self.dout,
                                          self.ld_dout, self.att_src, self.att_dst, self.dh, self.da_src, self.flags,
                                          s["drop"], s["tiles"], None)


def _broken(direction, form, **changes):
    """The return code of the valid set with ``struct__field`` / plain attributes changed."""
    o = Operands(direction, form)
    for k, v in changes.items():
        where, _, field = k.rpartition("__")
        o.set(where or None, field, v)
    return o.call()


@pytest.mark.parametrize("direction,form", CASES)
def test_each_required_pointer_null_is_einval(direction, form):
    fields = Operands(direction, form).required()
    assert len(fields) == N_REQUIRED[direction, form] and len(set(fields)) == len(fields)
    for where, field in fields:
        o = Operands(direction, form)
        assert o.get(where, field), (where, field)
        o.set(where, field, None)
        assert o.call() == EINVAL, (where, field)


@pytest.mark.parametrize("direction,form", CASES)
def test_empty_range_is_ok_and_looks_at_nothing_else(direction, form):
    for r in (0, 5, N):
        o = Operands(direction, form)
        o.null_everything()                                   # out2 and, for the source pass, nnz among them
        o.s["graph"].row_begin = o.s["graph"].row_end = r
        if direction == "src":
            o.s["graph"].nnz = -1                             # the source pass never looked at nnz
        assert o.call() == OK, r
    # ... with tiles, the graph's CSR is not among the source pass's required pointers (the valid set
    # has it; test_each_required_pointer_null_is_einval's list has not), while the forward needs it
    assert ("graph", "rowptr") in Operands("fwd", "tiles").required()
    assert ("graph", "rowptr") not in Operands("src", "tiles").required()


@pytest.mark.parametrize("direction,form", CASES)
def test_null_struct_and_exclusive_forms(direction, form):
    L = _L()
    for name in ("graph", "feats"):
        o = Operands(direction, form)
        o.s[name] = None
        assert o.call() == EINVAL, name
    o = Operands(direction, form)                             # dropout together with tiles
    if form != "drop":
        o.s["drop"] = L.AttnDrop(p=0.5, seed=1, step_value=1)
    if form != "tiles":
        o.s["tiles"] = Operands(direction, "tiles").s["tiles"]
    assert o.call() == EINVAL
    o.s["graph"].row_end = 0                                  # ... even over an empty range
    assert o.call() == EINVAL


@pytest.mark.parametrize("direction", ["fwd", "src"])
def test_dropout_parameters(direction):
    for p in (-0.1, 1.0, float("nan")):
        assert _broken(direction, "drop", drop__p=p) == EINVAL, p
    assert _broken(direction, "drop", drop__site=1 << 31) == EINVAL
    assert _broken(direction, "drop", drop__step_counter=_slot(30) + 4) == EINVAL
    # checked before the shape and before the empty range's OK
    assert _broken(direction, "drop", drop__p=1.0, feats__C=96) == EINVAL
    assert _broken(direction, "drop", drop__p=1.0, graph__row_end=0) == EINVAL
    assert _broken(direction, "drop", feats__C=96) == EUNSUPPORTED


@pytest.mark.parametrize("form", ["plain", "drop", "tiles"])
def test_source_pass_flags(form):
    for flags in (2, 3, -1, 1 << 8):
        assert _broken("src", form, flags=flags) == EINVAL, flags
        assert _broken("src", form, flags=flags, graph__row_end=0) == EINVAL, flags     # before the range
    if form == "tiles":                                       # the tiled pass has one block order
        assert _broken("src", form, flags=1) == EINVAL
        assert _broken("src", form, flags=1, graph__row_end=0) == EINVAL
    else:
        assert _broken("src", form, flags=1, graph__row_end=0) == OK


@pytest.mark.parametrize("direction,form", CASES)
def test_sizes_and_row_range(direction, form):
    assert _broken(direction, form, graph__N=-1, graph__row_end=-1) == EINVAL
    assert _broken(direction, form, graph__row_begin=-1) == EINVAL
    assert _broken(direction, form, graph__row_end=N + 1) == EINVAL
    assert _broken(direction, form, graph__row_begin=5, graph__row_end=4) == EINVAL
    if direction == "fwd":
        assert _broken(direction, form, graph__nnz=-1) == EINVAL
    if form == "tiles":
        assert _broken(direction, form, tiles__ntiles=-1) == EINVAL
    # before the shape
    assert _broken(direction, form, graph__row_end=N + 1, feats__H=8) == EINVAL


@pytest.mark.parametrize("form", ["plain", "drop", "tiles"])
def test_forward_act(form):
    for act in (2, -1):
        assert _broken("fwd", form, act=act) == EINVAL, act
        assert _broken("fwd", form, act=act, feats__H=8) == EINVAL, act                 # before the shape
    assert _broken("fwd", form, act=0, graph__row_end=0) == OK


@pytest.mark.parametrize("direction,form", CASES)
def test_shape(direction, form):
    bad = [(2, 96), (8, 128), (0, 256), (2, 0), (3, 128), (2, 640)]
    if form == "tiles":                                       # the dense-tile form is (2, 256) alone
        bad += [(2, 128), (1, 256), (4, 256)]
    for H, C in bad:
        # valid strides for the shape, so the shape alone is wrong
        assert _broken(direction, form, feats__H=H, feats__C=C, ld_stats=4 * max(H, 1),
                       ld_dout=max(H * C, 4)) == EUNSUPPORTED, (H, C)
    # before the strides, the empty range's OK and the NULL pointers
    assert _broken(direction, form, feats__C=96, ld_stats=2) == EUNSUPPORTED
    assert _broken(direction, form, feats__C=96, graph__row_end=0) == EUNSUPPORTED
    assert _broken(direction, form, feats__C=96, feats__h=None) == EUNSUPPORTED


@pytest.mark.parametrize("form", ["plain", "drop", "tiles"])
def test_source_pass_row_strides(form):
    H, C = SHAPE[form]
    for ld in (4 * H - 4, 4 * H + 2):
        assert _broken("src", form, ld_stats=ld) == EINVAL, ld
        assert _broken("src", form, ld_stats=ld, graph__row_end=0) == EINVAL, ld       # before the empty range
    for ld in (H * C - 4, H * C + 2):
        assert _broken("src", form, ld_dout=ld) == EINVAL, ld
    assert _broken("src", form, ld_stats=4 * H + 4, ld_dout=H * C + 8, graph__row_end=0) == OK


@pytest.mark.parametrize("direction", ["fwd", "src"])
def test_tiles_splits_and_workspace(direction):
    lib = _L().load()
    need = lib.hicgat_gat_tiled_workspace_bytes(N, 2)
    assert need == 2 * N * (2 * 512 + 2) * 4 and lib.hicgat_gat_tiled_workspace_bytes(N, 1) == 0
    for splits in (0, 65, -1):
        assert _broken(direction, "tiles", tiles__splits=splits) == EINVAL, splits
    ws = _slot(40)
    assert _broken(direction, "tiles", tiles__splits=2, tiles__workspace=ws, tiles__workspace_bytes=need - 1) == EINVAL
    assert _broken(direction, "tiles", tiles__splits=2, tiles__workspace=None, tiles__workspace_bytes=need) == EINVAL
    assert _broken(direction, "tiles", tiles__splits=2, tiles__workspace=ws + 4, tiles__workspace_bytes=need) == EINVAL
    # without a tile tcol and tmask are not read; tptr still is
    assert _broken(direction, "tiles", tiles__ntiles=0, tiles__tcol=None, tiles__tmask=None, tiles__tptr=None) == EINVAL


def test_attn_mask():
    L = _L()
    lib = L.load()
    rp, cl, m = _slot(1), _slot(2), _slot(3)
    drop = L.AttnDrop(p=0.5, seed=1, step_value=1)
    assert lib.hicgat_gat_attn_mask(rp, cl, N, 2, None, m, None) == EINVAL
    assert lib.hicgat_gat_attn_mask(rp, cl, 0, 2, None, m, None) == EINVAL
    for H in (0, 5):
        assert lib.hicgat_gat_attn_mask(rp, cl, N, H, drop, m, None) == EUNSUPPORTED, H
    assert lib.hicgat_gat_attn_mask(rp, cl, -1, 2, drop, m, None) == EINVAL
    assert lib.hicgat_gat_attn_mask(rp, cl, N, 5, L.AttnDrop(p=1.0), m, None) == EINVAL      # p before H
    assert lib.hicgat_gat_attn_mask(None, None, 0, 2, drop, None, None) == OK
    for args in ((None, cl, m), (rp, None, m), (rp, cl, None)):
        assert lib.hicgat_gat_attn_mask(args[0], args[1], N, 2, drop, args[2], None) == EINVAL


def test_ctypes_structs_mirror_the_header():
    """Field names, order and types of the four operand structs, and the round-robin flag."""
    L = _L()
    from hicgat.kernels import HipKernels
    with open(os.path.join(ROOT, "include", "hicgat.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    scalars = {"int": L.c_int, "int64_t": L.c_i64, "float": L.c_f, "size_t": L.c_sz, "double": L.c_d,
               "uint64_t": L.c_u64, "uint32_t": L.c_u32}
    pointees = set(scalars) | {"void", "int32_t"}
    for cname, cls in (("hicgat_gat_graph", L.GatGraph), ("hicgat_gat_feats", L.GatFeats),
                       ("hicgat_attn_drop", L.AttnDrop), ("hicgat_gat_tiles", L.GatTiles)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % cname, text).group(1)
        want = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, names = re.match(r"(?:const\s+)?(\w+)\s+(.*)", decl, re.S).groups()
            assert base in pointees, decl
            for nm in (n.strip() for n in names.split(",")):
                want.append((nm.lstrip("* "), L.c_p if nm.startswith("*") else scalars[base]))
        assert list(cls._fields_) == want, cname
    flag = int(re.search(r"enum \{ HICGAT_SRC_ROUND_ROBIN = (\d+) \};", text).group(1))
    assert flag == 1 == HipKernels.SRC_ROUND_ROBIN

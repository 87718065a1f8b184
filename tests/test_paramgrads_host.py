"""hicgat.paramgrads -- where the step's parameter-gradient launches go -- on stand-in streams and a
recording kernels object (no GPU).  Every case feeds the scheduler the flagship tail's backward at
M = 48 rows (dense3 W+b, norm2 sums, dense2 W+b, norm1 sums, block 2's dual pair, norm_a sums,
block 1's dual pair, through ops' own helpers) and compares the trace of launches and stream
operations -- (what, stream, arguments) -- with a literal.  The literals were recorded from the
scheduler as it stood inside ops.py before it became a module, so they are the contract a change
of launch placement is checked against, not a description of the current code."""
import gc
import threading
import types
import weakref

import pytest
import torch

import hicgat
from hicgat import kernels, ops, paramgrads as pg, streams
from test_streams_host import FakeEvent, FakeStream

M, ROWS = 48, 3    # ROWS: the fused backward's LayerNorm partial rows (one per 16-row workgroup)


class Stream(FakeStream):
    def __init__(self, name, h):
        super().__init__(h)
        self.name, self.device = name, "dev0"


class Rig:
    """Stand-in streams behind hicgat.streams, a kernels object that records, one trace for both."""

    def __init__(self, mp):
        self.trace, self.names, self.made, self.depth, self.events = [], {}, {}, 0, 0
        self.stack = [Stream("main", 1)]
        mp.setattr(torch.cuda, "Event", FakeEvent)
        mp.setattr(streams, "get", self.get)
        mp.setattr(streams, "current", lambda: self.stack[-1])
        mp.setattr(streams, "use", self.use)
        for op in ("record", "wait", "fork", "join"):
            mp.setattr(streams, op, self.logged(op, getattr(streams, op)))
        mp.setattr(kernels, "_default", self)
        torch.manual_seed(0)
        m = self.model = hicgat.GATNetSelectiveResidualsUpdated()
        self.opt = hicgat.FlatAdam(m.flat_parameters())
        for k, p in m.named_parameters():
            self.names[p.grad.data_ptr()] = "d_" + k
        self.t = types.SimpleNamespace()
        for k, w in dict(dc=3, z3=64, dy3=64, z2=128, dY2=256, z1=256, dY1=512, x=512, dh=512, x0=512).items():
            self.new(k, M, w)
        for k, w in dict(ws3=64, ws2=128, ws1=256).items():
            self.new(k, ROWS * 2 * w)

    def new(self, name, *shape):
        v = torch.zeros(shape)
        self.names[v.data_ptr()] = name
        setattr(self.t, name, v)
        return v

    # -- streams -------------------------------------------------------------------------------
    def get(self, name, device=None):
        assert name in streams.NAMES
        return self.made.setdefault(name, Stream(name, 10 + len(self.made)))

    def use(self, stream):
        rig = self

        class Ctx:
            def __enter__(self):
                rig.stack.append(stream)

            def __exit__(self, *exc):
                rig.stack.pop()
        return Ctx()

    def logged(self, op, fn):
        def call(*a):
            self.depth += 1
            try:
                out = fn(*a)
            finally:
                self.depth -= 1
            if self.depth == 0:
                if op == "record":
                    self.events += 1
                    out.n = f"e{self.events}"
                    self.trace.append(("record", (a[0] if a and a[0] is not None else self.stack[-1]).name, out.n))
                elif op == "wait":
                    self.trace.append(("wait", a[0].name, a[1].n))
                else:
                    src = a[1] if len(a) > 1 and a[1] is not None else self.stack[-1]
                    self.trace.append((op, a[0].name, src.name))
            return out
        return call

    # -- the recording kernels object ----------------------------------------------------------------
    def f(self, v):
        if isinstance(v, torch.Tensor):
            return f"{self.names.get(v.data_ptr(), '?')}[{'x'.join(map(str, v.shape))}]"
        if isinstance(v, (tuple, list)):
            return "(" + " ".join(self.f(u) for u in v) + ")"
        return str(v)

    def log(self, what, *args):
        self.trace.append((what, self.stack[-1].name, " ".join(self.f(a) for a in args)))

    def wgrad(self, dy, x, W_out, b_out=None, accumulate=False, splits=1):
        self.log("wgrad", dy, x, W_out, b_out, f"acc={accumulate}", f"splits={splits}")

    def gemm(self, a_kmajor, b_kmajor, M_, N, K, A, B, C, bias=None, accumulate=False, splits=None, name="gemm",
             impl=None):
        self.log("gemm", a_kmajor, b_kmajor, M_, N, K, A, B, C, bias, f"acc={accumulate}", f"splits={splits}", name, impl)
        return C

    def colsum(self, A, out, accumulate=False):
        self.log("colsum", A, out, f"acc={accumulate}")
        return out

    def ln_act_res_bwd_params(self, W, dgamma, dbeta, ws, accumulate=False):
        self.log("ln_act_res_bwd_params", W, dgamma, dbeta, ws, f"acc={accumulate}")

    def param_grads_grouped(self, wjobs, cjobs, target_wgs=None, small_m=None):
        # a column-sum job always as (src, dst, accumulate, weights)
        self.log("param_grads_grouped", "w", *[tuple(j) for j in wjobs],
                 "c", *[(tuple(j) + (None,))[:4] for j in cjobs], f"wgs={target_wgs}", f"small_m={small_m}")

    # -- the tail's backward -----------------------------------------------------------------------------
    def tail(self, ln2_per_layer=False):
        """The fused tail backward's parameter-gradient calls, in its order (ops._FusedTailFn.backward);
        ``ln2_per_layer``: norm2's sums as the per-layer path queues them (an item without a job)."""
        m, t = self.model, self.t
        ops._wb_grad_to(self, m.dense3.weight, m.dense3.bias, t.dc, t.z3)
        if ln2_per_layer:
            sg, sb, ws = m.norm2.weight.grad, m.norm2.bias.grad, t.ws3
            pg.param_launch(lambda: self.ln_act_res_bwd_params(64, sg, sb, ws, accumulate=True), ws)
        else:
            ops._ln_param_grads(self, m.norm2.weight, m.norm2.bias, t.ws3, ROWS)
        ops._wb_grad_to(self, m.dense2.weight, m.dense2.bias, t.dy3, t.z2)
        ops._ln_param_grads(self, m.norm1.weight, m.norm1.bias, t.ws2, ROWS)
        ops._dual_param_grads(self, m.dense1.weight, m.dense1.bias, m.align_dense1.weight, m.align_dense1.bias,
                              t.dY2, t.z1)
        ops._ln_param_grads(self, m.norm_a.weight, m.norm_a.bias, t.ws1, ROWS)
        ops._dual_param_grads(self, m.densea.weight, m.densea.bias, m.align_densea.weight, m.align_densea.bias,
                              t.dY1, t.x)

    def lin_l(self):
        return pg.WeightGradJob(self.t.dh, self.t.x0, self.model.conv.lin_l.weight.grad)

    def backward(self, lanes=1, **kw):
        """The tail, then what the GATConv backward does around its source pass: mark, flush."""
        self.tail(**kw)
        n = len(self.trace)
        ev = pg.side_mark()
        self.log("source_pass")
        pg.side_flush(after=ev, lanes=lanes)
        return n, ev


def idle():
    s = pg._STATE
    return (s.on, s.no_big, s.grouped, len(s.queue), len(s.jobs), len(s.hold), len(s.mains)) == (0,) * 7


@pytest.fixture()
def rig(monkeypatch):
    assert idle()
    pg._STATE.streams.clear()                # the lanes' streams are made anew from this test's stand-ins
    for knob, v in dict(OVERLAP_DEFAULT=True, SIDE_GROUPED=True, BIG_GROUP=0.0, SIDE_GROUP_WGS=192, SIDE_SMALL_M=0,
                        SMALL_WORK=4e6).items():
        monkeypatch.setattr(pg, knob, v)     # the defaults, whatever the environment says
    yield Rig(monkeypatch)
    assert idle()


# the tail's jobs of one grouped launch, in backward order
W_TAIL = ("(dc[48x3] z3[48x64] d_dense3.weight[3x64] d_dense3.bias[3] True) "
          "(dy3[48x64] z2[48x128] d_dense2.weight[64x128] d_dense2.bias[64] True) "
          "(dY2[48x256] z1[48x256] d_dense1.weight[256x256] d_dense1.bias[256] True) "
          "(dY1[48x512] x[48x512] d_densea.weight[512x512] d_densea.bias[512] True)")
C_TAIL = ("(ws3[3x128] d_norm2.weight[128] True None) (ws2[3x256] d_norm1.weight[256] True None) "
          "(ws1[3x512] d_norm_a.weight[512] True None)")
GROUPED = f"w {W_TAIL} c {C_TAIL} wgs=192 small_m=0"
# ... and as one launch per item
DENSE3 = "dc[48x3] z3[48x64] d_dense3.weight[3x64] d_dense3.bias[3] acc=True splits=1"
NORM2 = "ws3[3x128] d_norm2.weight[128] acc=True"
DENSE2 = "dy3[48x64] z2[48x128] d_dense2.weight[64x128] d_dense2.bias[64] acc=True splits=1"
NORM1 = "ws2[3x256] d_norm1.weight[256] acc=True"
BLOCK2 = "dY2[48x256] z1[48x256] d_dense1.weight[256x256] d_dense1.bias[256] acc=True splits=1"
NORM_A = "ws1[3x512] d_norm_a.weight[512] acc=True"
BLOCK1 = "dY1[48x512] x[48x512] d_densea.weight[512x512] d_densea.bias[512] acc=True splits=1"


def per_item(s):
    return [("wgrad", s, DENSE3), ("colsum", s, NORM2), ("wgrad", s, DENSE2), ("colsum", s, NORM1),
            ("wgrad", s, BLOCK2), ("colsum", s, NORM_A), ("wgrad", s, BLOCK1)]


DEFAULT_TRACE = [("record", "main", "e1"), ("source_pass", "main", ""), ("wait", "side0", "e1"),
                 ("param_grads_grouped", "side0", GROUPED), ("join", "main", "side0")]


def test_default_single_gpu_one_grouped_launch_beside_the_source_pass(rig):
    t = rig.t
    kept = weakref.ref(t.dY1)
    with pg.overlapped_param_grads():
        assert pg.overlapping()
        n, ev = rig.backward()
        assert n == 0 and ev is not None            # nothing launched while queueing; the mark is an event
        del t.dY1
        gc.collect()
        assert kept() is not None                   # the side lane may still read it
        assert rig.trace == DEFAULT_TRACE[:-1]
    gc.collect()
    assert kept() is None                           # released by the join
    assert rig.trace == DEFAULT_TRACE and not pg.overlapping()


def test_per_item_launches_on_the_side_lane(rig, monkeypatch):
    monkeypatch.setattr(pg, "SIDE_GROUPED", False)
    with pg.overlapped_param_grads():
        assert rig.backward()[0] == 0
    assert rig.trace == [("record", "main", "e1"), ("source_pass", "main", ""), ("wait", "side0", "e1"),
                         *per_item("side0"), ("join", "main", "side0")]


LIN_L = "(dh[48x512] x0[48x512] d_conv.lin_l.weight[512x512] None True)"


def test_big_group_holds_jobs_for_lin_l(rig, monkeypatch):
    monkeypatch.setattr(pg, "BIG_GROUP", 1.0)
    with pg.overlapped_param_grads(hold_big=True):
        n, ev = rig.backward()
        assert (n, ev) == (0, None) and len(pg._STATE.jobs) == 7   # every item has a job and work >= 1: all held
        assert rig.trace == [("source_pass", "main", "")]
        keep = pg.grouped_flush(rig, [rig.lin_l()])
        assert not pg._STATE.jobs
        t = rig.t
        want = [t.dc, t.z3, t.ws3, t.dy3, t.z2, t.ws2, t.dY2, t.z1, t.ws1, t.dY1, t.x]
        assert len(keep) == len(want) and all(a is b for a, b in zip(keep, want))
    assert rig.trace == [("source_pass", "main", ""),
                         ("param_grads_grouped", "main", f"w {W_TAIL} {LIN_L} c {C_TAIL} wgs=None small_m=None")]


def test_big_group_without_hold_big_holds_nothing(rig, monkeypatch):
    monkeypatch.setattr(pg, "BIG_GROUP", 1.0)
    with pg.overlapped_param_grads(hold_big=False):
        rig.backward()
        assert not pg._STATE.jobs and not pg.flush_held(rig, [rig.lin_l()])    # nothing held: nothing launched
    assert rig.trace == DEFAULT_TRACE


def test_flush_held_is_the_gatconv_backwards_launch_and_keeps_until_the_join(rig, monkeypatch):
    monkeypatch.setattr(pg, "BIG_GROUP", 1.0)
    kept = weakref.ref(rig.t.dY1)
    with pg.overlapped_param_grads():
        rig.backward()
        assert pg.flush_held(rig, [rig.lin_l()]) and not pg._STATE.jobs
        del rig.t.dY1
        gc.collect()
        assert kept() is not None
    gc.collect()
    assert kept() is None
    assert rig.trace == [("source_pass", "main", ""),
                         ("param_grads_grouped", "main", f"w {W_TAIL} {LIN_L} c {C_TAIL} wgs=None small_m=None")]


def test_held_jobs_nobody_flushed_are_issued_by_the_join(rig, monkeypatch):
    monkeypatch.setattr(pg, "BIG_GROUP", 1.0)
    with pg.overlapped_param_grads():
        rig.tail()
        assert rig.trace == []
    assert rig.trace == [("param_grads_grouped", "main", f"w {W_TAIL} c {C_TAIL} wgs=None small_m=None")]


def test_an_item_without_a_job_makes_the_whole_flush_per_item(rig):
    with pg.overlapped_param_grads():
        assert rig.backward(ln2_per_layer=True)[0] == 0
    want = per_item("side0")
    want[1] = ("ln_act_res_bwd_params", "side0", "64 d_norm2.weight[64] d_norm2.bias[64] ws3[384] acc=True")
    assert rig.trace == [("record", "main", "e1"), ("source_pass", "main", ""), ("wait", "side0", "e1"), *want,
                         ("join", "main", "side0")]


@pytest.mark.parametrize("small_work", [4e6, 1e5])
def test_three_lanes_largest_first_then_small_first_within_a_lane(rig, monkeypatch, small_work):
    """work: block 1 12.6e6, block 2 3.1e6, dense2 393 216, dense3 9 216, norm_a / norm1 / norm2 1 536 /
    768 / 384: block 1 -> side0, block 2 -> side4, the rest -> side5 (its load stays the smallest), there
    in largest-first order unless below SMALL_WORK (at 1e5: dense2 moves behind the four small ones)."""
    monkeypatch.setattr(pg, "SMALL_WORK", small_work)
    with pg.overlapped_param_grads(hold_big=False):
        assert rig.backward(lanes=3)[0] == 0
        evs = pg.side_record()
        assert [e.n for e in evs] == ["e2", "e3", "e4"]
    side5 = [("wgrad", "side5", DENSE2), ("wgrad", "side5", DENSE3), ("colsum", "side5", NORM_A),
             ("colsum", "side5", NORM1), ("colsum", "side5", NORM2)]
    if small_work == 1e5:
        side5 = side5[1:] + side5[:1]
    assert rig.trace == [("record", "main", "e1"), ("source_pass", "main", ""),
                         ("wait", "side0", "e1"), ("wgrad", "side0", BLOCK1),
                         ("wait", "side4", "e1"), ("wgrad", "side4", BLOCK2),
                         ("wait", "side5", "e1"), *side5,
                         ("record", "side0", "e2"), ("record", "side4", "e3"), ("record", "side5", "e4"),
                         ("join", "main", "side0"), ("join", "main", "side4"), ("join", "main", "side5")]


def test_equal_loads_go_to_the_lane_with_fewer_items(rig):
    m = rig.model
    with pg.overlapped_param_grads():
        for p, dy in ((m.dense3.bias, rig.t.dc), (m.dense2.bias, rig.t.dy3), (m.norm2.bias, rig.t.z3)):
            ops._bias_grad_to(rig, p, dy)           # work 0 each
        pg.side_flush(lanes=3)
    assert rig.trace == [("fork", "side0", "main"), ("colsum", "side0", "dc[48x3] d_dense3.bias[3] acc=True"),
                         ("fork", "side4", "main"), ("colsum", "side4", "dy3[48x64] d_dense2.bias[64] acc=True"),
                         ("fork", "side5", "main"), ("colsum", "side5", "z3[48x64] d_norm2.bias[64] acc=True"),
                         ("join", "main", "side0"), ("join", "main", "side4"), ("join", "main", "side5")]


def test_side_record_is_empty_when_not_overlapping(rig):
    assert pg.side_record() == [] and pg.side_mark() is None and rig.trace == []


def test_side_lane_forks_a_named_lane_and_keeps_until_the_join(rig):
    """What the sharded steps use for lin_l's dW: lane 2 (slab) or 0 (allgather), forked from here."""
    kept = weakref.ref(rig.t.dh)
    with pg.side_lane(rig.t.dh, lane=2):            # not overlapping: no stream at all
        rig.log("lin_l_dw")
    with pg.overlapped_param_grads(hold_big=False):
        with pg.side_lane(rig.t.dh, rig.t.x0, lane=2):
            rig.log("lin_l_dw")
        del rig.t.dh
        gc.collect()
        assert kept() is not None
    gc.collect()
    assert kept() is None
    assert rig.trace == [("lin_l_dw", "main", ""), ("fork", "side2", "main"), ("lin_l_dw", "side2", ""),
                         ("join", "main", "side2")]


def test_grouped_param_grads_collects_jobs_and_launches_the_rest(rig):
    with pg.grouped_param_grads():
        rig.tail(ln2_per_layer=True)
        assert rig.trace == [("ln_act_res_bwd_params", "main",
                              "64 d_norm2.weight[64] d_norm2.bias[64] ws3[384] acc=True")]
    keep = pg.grouped_flush(rig, [rig.lin_l()], target_wgs=256, small_m=16)
    assert len(keep) == 10 and keep[0] is rig.t.dc
    c = C_TAIL.split(") (", 1)[1]
    assert rig.trace[1:] == [("param_grads_grouped", "main", f"w {W_TAIL} {LIN_L} c ({c} wgs=256 small_m=16")]
    assert pg.grouped_flush(rig) == [] and len(rig.trace) == 2      # all of them, once


def test_grouped_param_grads_drops_a_failed_steps_jobs(rig):
    with pytest.raises(KeyError):
        with pg.grouped_param_grads():
            rig.tail()
            raise KeyError("backward failed")
    assert pg.grouped_flush(rig) == [] and rig.trace == []


@pytest.mark.parametrize("how", ["disabled", "outside"])
def test_not_overlapping_launches_at_once_on_the_current_stream(rig, how):
    if how == "disabled":
        with pg.overlapped_param_grads(False):
            assert not pg.overlapping()
            rig.tail()
    else:
        rig.tail()
    assert rig.trace == per_item("main")


def test_overlap_default_off_means_not_overlapping(rig, monkeypatch):
    monkeypatch.setattr(pg, "OVERLAP_DEFAULT", False)
    with pg.overlapped_param_grads():
        rig.tail()
    assert rig.trace == per_item("main")


def test_an_exception_still_issues_the_queue_and_joins(rig):
    with pytest.raises(KeyError):
        with pg.overlapped_param_grads():
            with pg.overlapped_param_grads(hold_big=False):
                assert pg._STATE.on == 2 and pg._STATE.no_big == 1
                rig.tail()
                raise KeyError("backward failed")
    assert rig.trace == [("fork", "side0", "main"), ("param_grads_grouped", "side0", GROUPED),
                         ("join", "main", "side0")]
    assert idle()
    del rig.trace[:]
    rig.events = 0
    with pg.overlapped_param_grads():               # a clean block after it: the default trace again
        rig.backward()
    assert rig.trace == DEFAULT_TRACE


def test_nested_blocks_keep_the_count(rig):
    with pg.overlapped_param_grads():
        with pg.overlapped_param_grads():
            assert pg._STATE.on == 2
        assert pg._STATE.on == 1 and pg.overlapping()
    assert pg._STATE.on == 0


def test_items_queued_from_another_thread(rig):
    """The block is entered on the caller's thread and the backward bodies run on autograd's: the
    state is process-wide."""
    with pg.overlapped_param_grads():
        th = threading.Thread(target=rig.backward)
        th.start()
        th.join()
        assert rig.trace == DEFAULT_TRACE[:-1]
    assert rig.trace == DEFAULT_TRACE


def test_the_knobs_live_in_paramgrads_alone():
    """A stale ``monkeypatch.setattr(ops, "BIG_GROUP", ...)`` must fail, not patch a copy."""
    for knob in ("OVERLAP_DEFAULT", "BIG_GROUP", "SIDE_GROUPED", "SIDE_GROUP_WGS", "SIDE_SMALL_M", "SMALL_WORK"):
        assert hasattr(pg, knob) and not hasattr(ops, knob) and not hasattr(hicgat.dist, knob)

"""Where the step's parameter-gradient launches go.  The parameter-gradient kernels (split-K dW GEMMs,
bias column sums, GAT param_grad) feed only the optimizer, never the next backward op, so inside
``overlapped_param_grads`` they are issued on a side stream that forks from the backward's stream
and is joined back before anything reads the flat gradient buffer (Adam / the gradient
all-reduce).  The MFMA-bound GEMMs then run beside the L2-bound aggregation backward instead of in
series with it; in a captured step the fork and join are graph edges.  Only sink-bound gradients
(``ops._sink``) go to the side stream -- a gradient that is returned to autograd is consumed on the
backward's stream and must be produced there.  tests/test_paramgrads_host.py holds the rules."""
import contextlib
import os
import threading
from collections import namedtuple

from . import streams

# The jobs of a grouped launch (kernels.param_grads_grouped).  dW (+)= dy^T x, and db (+)= column sums of
# dy when ``db`` is given:
WeightGradJob = namedtuple("WeightGradJob", "dy x dW db accumulate", defaults=(None, True))
# dst (+)= column sums of src, its rows weighted by ``weights`` [rows] when given; a 2-D dst [segs, cols]
# takes the rows' sum in segments:
ColsumJob = namedtuple("ColsumJob", "src dst accumulate weights", defaults=(True, None))
# One queued launch: ``launch()`` issues it alone, ``job`` is the same work for a grouped launch (None: it
# has no grouped form), ``keep`` the tensors it reads, ``work`` its multiply-adds.
_Item = namedtuple("_Item", "launch keep work job")


class _State:
    """The scheduler's state.  Process-wide, NOT per thread: the ``with overlapped_param_grads():``
    block runs on the caller's thread and the ``backward`` bodies that queue the launches run on
    autograd's device thread, so a thread-local would silently queue nothing.  Every read and
    write is under ``lock``."""

    def __init__(self):
        self.lock = threading.Lock()
        self.on = self.no_big = self.grouped = 0   # open overlapped blocks; those with hold_big=False; grouped blocks
        self.streams, self.mains = {}, {}   # (device, lane) -> side stream; -> the stream it forked from, until the join
        self.hold = []                      # tensors the side lanes read, until the join
        self.queue, self.jobs = [], []      # _Item for side_flush; (job, keep) collected for grouped_flush


_STATE = _State()
OVERLAP_DEFAULT = True
# The tail's parameter-gradient launches (split-K dW GEMMs with their bias sums, the LayerNorm
# dgamma/dbeta sums, bias column sums) are DEFERRED: queued, and issued by ``side_flush`` on the side
# stream beside the GAT source-side gather (forked after the gather-free row pass).  Issued as they
# come, a captured step's graph placed some of them in front of the aggregation backward on its
# queue (2.036 vs 2.060 ms per step).  Measured slower and removed: largest-first
# or small-first issue order, the big dW GEMMs on a stream of their own or on the backward's stream,
# lin_l's dW queued behind the side work, the GAT param_grad on a second side stream or split around
# the gather, the source pass in row chunks, two side lanes on one GPU.


# single-GPU step: parameter-gradient jobs of at least this many multiply-adds (the first tail block's
# 512 x 512 dW, 5.2e9 at N = 20000) are held and issued with lin_l's dW as ONE grouped launch after
# the source gather (0: off -- they go to the side stream like the rest).  Round 4: 1.876 / 1.879 vs
# 1.889 / 1.888 ms per step with one side launch per item (profiles/r04i_ab_big_group.txt); with the
# side work as one grouped launch (SIDE_GROUPED) the big dW rides there: 0 since round 6
BIG_GROUP = float(os.environ.get("HICGAT_BIG_GROUP", "0"))
_FLUSH_LANES = (0, 4, 5, 6)
SMALL_WORK = 4e6   # side_flush(lanes > 1): items below this many multiply-adds go first in their lane
# single-GPU step (one lane): the queued side work -- every dW / db / LayerNorm sum of the MLP tail,
# the first block's 512 x 512 dW included (BIG_GROUP 0) -- as ONE grouped weight-gradient + ONE
# grouped column-sum launch (hicgat_param_grads_grouped) beside the source gather, when every item has
# a job descriptor, instead of ~13 launches that each waited for room beside the gather; 0: one
# launch per item.  SIDE_GROUP_WGS: the grouped launch's workgroup target (the K split): fewer
# workgroups take fewer CUs from the gather; SIDE_SMALL_M 0: dense3's 3-row dW as an MFMA tile, not
# three 20 000-row weighted column sums (single-block chains, 157 µs of the side lane).  1.730-1.732
# vs 1.769-1.771 ms per step (profiles/r06rst_ab_side_grouped.txt, r06u_ab_side_grouped.txt)
SIDE_GROUPED = os.environ.get("HICGAT_SIDE_GROUPED", "1") != "0"
SIDE_GROUP_WGS = int(os.environ.get("HICGAT_SIDE_GROUP_WGS", "192"))
SIDE_SMALL_M = int(os.environ.get("HICGAT_SIDE_SMALL_M", "0"))


def _kernels():
    from . import kernels
    return kernels.default()


def overlapping():
    """Inside an ``overlapped_param_grads`` block: sink-bound parameter gradients are side work."""
    with _STATE.lock:
        return _STATE.on > 0


def flush_held(K, extra):
    """The held jobs (BIG_GROUP) and ``extra`` as one grouped launch now, their inputs kept until the
    join; False, and nothing launched, when no job is held."""
    with _STATE.lock:
        if not _STATE.jobs:
            return False
    keep = grouped_flush(K, extra)
    with _STATE.lock:
        _STATE.hold.extend(keep)
    return True


def side_begin():
    """Route sink-bound parameter gradients to the side stream until ``side_join``."""
    with _STATE.lock:
        _STATE.on += 1


def side_mark():
    """An event on the current stream marking where queued side work may start (``side_flush``)."""
    with _STATE.lock:
        pending = _STATE.on > 0 and bool(_STATE.queue)
    return streams.record() if pending else None


def side_flush(after=None, lanes=1):
    """Issue the queued parameter-gradient launches on the side stream, forked from the current
    stream at this point, or from the earlier point ``after`` (an event from ``side_mark``): the
    caller can then enqueue its own next kernel first, so a captured graph lists that kernel
    ahead of the side branch (they read only tensors produced before the fork point).

    ``lanes`` > 1 spreads the launches over that many side streams (largest work first, each to the
    least-loaded lane; every launch writes its own parameters' gradients, so they are independent):
    a rank's shard of the multi-GPU slab step has a gather window too short for the tail's queued
    launches in one chain.  The single-GPU step keeps one lane (a second one measured slower there,
    DESIGN section 7)."""
    with _STATE.lock:
        queue, _STATE.queue = _STATE.queue, []
    if not queue:
        return
    n = max(1, min(lanes, len(_FLUSH_LANES)))
    if n == 1 and SIDE_GROUPED and all(q.job is not None for q in queue):
        with side_lane(*[t for q in queue for t in q.keep], after=after, lane=_FLUSH_LANES[0]):
            streams.stamp("side_begin")
            _grouped_launch(_kernels(), [q.job for q in queue], SIDE_GROUP_WGS, SIDE_SMALL_M)
            streams.stamp("side_end")
        return
    load, parts = [0] * n, [[] for _ in range(n)]
    if n == 1:
        parts[0] = queue                     # backward order
    else:
        for item in sorted(queue, key=lambda q: -q.work):
            k = min(range(n), key=lambda a: (load[a], len(parts[a])))
            parts[k].append(item)
            load[k] += item.work
    for lane, items in zip(_FLUSH_LANES, parts):
        if n > 1:
            # reductions without a GEMM (LayerNorm dgamma/dbeta sums: inputs ready, a few us each)
            # first in their lane, then the GEMMs
            items = [q for q in items if q.work < SMALL_WORK] + [q for q in items if q.work >= SMALL_WORK]
        if items:
            with side_lane(*[t for q in items for t in q.keep], after=after, lane=lane):
                streams.stamp("side_begin")
                for q in items:
                    q.launch()
                streams.stamp("side_end")


def side_record():
    """Events recorded now on every side stream in use: they complete when the side work issued
    so far (e.g. the tail's flushed dW GEMMs) has run.  [] when nothing went to a side stream."""
    with _STATE.lock:
        sides = [_STATE.streams[key] for key in _STATE.mains] if _STATE.on else []
    return [streams.record(st) for st in sides]


@contextlib.contextmanager
def grouped_param_grads():
    """Inside: the sink-bound parameter gradients that have a job descriptor (every dW / db / LayerNorm
    sum of the Linear, dual-Linear and fused-tail backward) are collected instead of launched;
    ``grouped_flush`` then issues ALL of them as two launches (hicgat_param_grads_grouped).  A rank's
    share of the sharded step is too small for ~15 separate launches: queued over side lanes they
    were the critical path after the edge pass (profiles/r03w_simprof_xagg_P8_rank0_timeline.txt)."""
    with _STATE.lock:
        _STATE.grouped += 1
    try:
        yield
    except BaseException:
        # a failed backward: drop the collected descriptors, so no later grouped_flush adds this
        # step's partial dW / db into another step's gradient
        with _STATE.lock:
            _STATE.jobs.clear()
        raise
    finally:
        with _STATE.lock:
            _STATE.grouped -= 1


def grouped_flush(K=None, extra=(), target_wgs=None, small_m=None):
    """Issue the collected jobs (plus the ``extra`` jobs) on the current stream: one grouped
    weight-gradient launch and one grouped column-sum launch.  Returns the tensors they read (the
    caller keeps them alive until the launches are ordered before any reuse)."""
    with _STATE.lock:
        jobs, _STATE.jobs = _STATE.jobs, []
    jobs = jobs + [(j, ()) for j in extra]
    if not jobs:
        return []
    _grouped_launch(K if K is not None else _kernels(), [j for j, _ in jobs], target_wgs, small_m)
    return [t for _, keep in jobs for t in keep]


def _grouped_launch(K, jobs, target_wgs=None, small_m=None):
    K.param_grads_grouped([j for j in jobs if isinstance(j, WeightGradJob)],
                          [j for j in jobs if isinstance(j, ColsumJob)], target_wgs, small_m)


def side_join():
    """Flush the queue, make every stream that forked work onto the side stream wait for it, and
    drop the held inputs.  Always runs the queued launches, even after an exception upstream, so
    no gradient kernel is left behind for a later step."""
    try:
        side_flush()
        with _STATE.lock:
            collecting = _STATE.grouped
        if not collecting:
            # held big jobs that no GATConv backward issued (BIG_GROUP with another model): now
            flush_held(None, ())
    finally:
        with _STATE.lock:
            _STATE.on = max(0, _STATE.on - 1)
            for key, main in _STATE.mains.items():
                streams.join(main, _STATE.streams[key])
            _STATE.mains.clear()
            _STATE.hold.clear()


@contextlib.contextmanager
def overlapped_param_grads(enabled=None, hold_big=True):
    """``with overlapped_param_grads(): loss.backward()`` -- parameter gradients overlap the rest
    of the backward and are complete (ordered before the caller's stream) on exit.

    ``hold_big=False``: no BIG_GROUP holding -- for a backward that has no ``_GATConvFn`` to issue
    the held jobs with lin_l's dW (the sharded step runs the GATConv backward itself; a held job
    would otherwise be issued by ``side_join`` on the main stream, after the caller recorded the
    side streams' completion for its gradient all-reduce)."""
    if not (OVERLAP_DEFAULT if enabled is None else enabled):
        yield
        return
    side_begin()
    with _STATE.lock:
        _STATE.no_big += not hold_big
    try:
        yield
    finally:
        try:
            side_join()
        finally:
            with _STATE.lock:
                _STATE.no_big -= not hold_big


def param_launch(fn, *keep, work=0, job=None):
    """Launch a sink-bound parameter-gradient kernel ``fn()``: now on the current stream when not
    overlapping; queued for ``side_flush`` when overlapping (``work``: its multiply-adds, for the
    lanes' balance and BIG_GROUP).  ``keep`` are the tensors ``fn`` reads (held until the join).
    ``job``: the same work as a ``WeightGradJob`` / ``ColsumJob``, for the grouped launches."""
    with _STATE.lock:
        if job is not None and (_STATE.grouped or (BIG_GROUP > 0 and _STATE.on and not _STATE.no_big
                                                   and work >= BIG_GROUP)):
            _STATE.jobs.append((job, keep))
            return
        if _STATE.on:
            _STATE.queue.append(_Item(fn, keep, work, job))
            return
    fn()


def side_lane(*keep, after=None, lane=0):
    """Stream context for a sink-bound gradient kernel: side stream ``lane`` (after a fork from the
    current stream, or from the event ``after``) while overlapping, else a no-op.  ``keep`` are
    the inputs the side kernels read; they stay referenced until the join so the caching
    allocator cannot hand their memory to a later backward kernel while the side stream still
    reads it."""
    cur = None
    with _STATE.lock:
        if _STATE.on:
            cur = streams.current()
            key = (cur.device, lane)
            side = _STATE.streams.get(key)
            if side is None:
                side = _STATE.streams[key] = streams.get(f"side{lane}", cur.device)
            _STATE.mains.setdefault(key, cur)
            _STATE.hold.extend(keep)
    if cur is None:
        return contextlib.nullcontext()
    if after is not None:
        streams.wait(side, after)
    else:
        streams.fork(side, cur)
    return streams.use(side)

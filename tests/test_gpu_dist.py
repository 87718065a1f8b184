"""GPU: hicgat.dist.ShardedTrainer on the HIP kernels.

* 1 rank over RCCL ("nccl") vs the single-GPU autograd step (same loss, same gradients), and the
  captured step (kernels + RCCL collectives + the comm-stream gradient bucket) vs eager steps;
* 2 and 3 ranks sharing the one GPU over gloo (CUDA tensors) vs 1 rank, both step forms ("slab":
  slab source pass + partial dW; "allgather": all-gathers of h and [dout | row stats]);
* the one-rank-at-a-time simulation (SimComm) used by bench.py --simulate-world.
The 8-GPU RCCL run itself is the driver's scaling bench.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inputs(n, dev):
    """The test graphs (5 % contacts, seed 3) -- or, for n = 20000, BASELINE configs[2]'s synth-20000
    workload exactly as bench.py builds it (1 % contacts, seed 0; configs[3] shards it)."""
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "hic-gnn_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import hicgat
    from hicgat import synth
    density, seed = (0.01, 0) if n == 20000 else (0.05, 3)
    i, j, c = synth.contact_pairs(n, density=density, seed=seed)
    A = synth.dense_contacts(n, i, j, c, device=dev)
    adj = hicgat.Adj.from_dense_device(A, keep_host=False)
    truth = hicgat.Truth.from_contacts(A, 0.5)
    del A
    x = torch.tensor(synth.features(n, seed=seed), device=dev)
    return hicgat, adj, truth, x


def _single_gpu_steps(n, steps=2):
    """The single-GPU flagship step (hicgat.train.train_step, seed-0 weights) on the same inputs:
    (losses, gradients after step 1, flat parameters after step 1, the model, the optimizer, the
    kink masks of step 1 -- tests/kinks.py, from the GATConv pre-relu output of the step-1 weights)."""
    hicgat, adj, truth, x = _inputs(n, "cuda")
    torch.manual_seed(0)
    model = hicgat.GATNetSelectiveResidualsUpdated().to("cuda")
    opt = hicgat.FlatAdam(model.flat_parameters(), lr=1e-3)   # the trainer's flat layout
    masks, counts, bounds = _kink_info(hicgat, model, x, adj, truth)
    losses, g1, p1, c1 = [], None, None, None
    for k in range(steps):
        loss, _, coords = hicgat.train.train_step(model, opt, x, adj, truth)
        losses.append(float(loss))
        if k == 0:
            g1, p1, c1 = opt.grad.clone(), opt.flat.clone(), coords.detach().clone()
    return dict(loss=losses, grad1=g1, flat1=p1, coords1=c1, model=model, opt=opt, masks=masks, kinks=counts,
                bounds=bounds, inputs=(x, adj, truth))


def _kink_info(hicgat, model, x, adj, truth):
    """tests/kinks.py's masks and flipped-term bounds of the step at the model's current weights."""
    from kinks import kink_bounds
    c = model.conv
    with torch.no_grad():
        out_pre = hicgat.ops.gat_conv(x, c.lin_l.weight, c.att_l, c.att_r, c.bias, adj)
        coords = model.get_model(x, adj)
    cd = coords.detach().requires_grad_(True)
    loss, _ = hicgat.ops.fused_dist_loss(cd, truth)
    loss.backward()
    return kink_bounds(model, out_pre, cd.grad, x, adj.rowptr32, adj.col32)


def _loss_at(ref, flat):
    """The single-GPU loss (forward + fused loss, no update) at the flat parameters ``flat``."""
    x, adj, truth = ref["inputs"]
    with torch.no_grad():
        ref["opt"].flat.copy_(flat.to(ref["opt"].flat.device))
        loss, _, _ = ref["model"].loss(x, adj, truth, "mse")
    return float(loss)


def _assert_step_matches(ref, res, loss_tol=1e-5, grad_tol=1e-4, label=""):
    """The kink-aware comparison (tests/kinks.py) of a sharded / other-form run ``res`` (rank 0's
    saved losses, step-1 gradient and parameters) against the single-GPU ``ref``: step-1 loss to
    ``loss_tol`` relative, every gradient to ``grad_tol`` of its max outside the kink-decided
    entries, dense3.bias (exactly 0 in exact arithmetic: translation invariance) to 1e-3 of the
    largest gradient, and the step-1 Adam update wherever it is not sensitive to the gradient's
    rounding (|g| above 1e-3 of its tensor's max and above 1e-6, unmasked: the update is then
    lr sign(g) to fp32 rounding).  Step 2: Adam's first update is lr sign(g), so every entry whose
    gradient is at rounding level (and every kink-decided one) takes a +-lr step of either sign in
    the two runs -- measured 1.1-1.3e-5 relative on the step-2 loss at synth-20000 P = 2 and n = 3000
    (gpurun_out/r04a_pytest_gpu.log).  So step 2 is checked teacher-forced: the single-GPU forward
    at the run's OWN step-1 parameters must give its step-2 loss to ``loss_tol``, and the free
    step-2 losses must agree to 1e-4."""
    from kinks import compare_flat
    model, opt, masks = ref["model"], ref["opt"], ref["masks"]
    g_ref, g = ref["grad1"], res["grad1"].to(ref["grad1"].device)
    per = compare_flat(model, zip(opt.params, opt.offsets), g_ref, g, masks, bounds=ref["bounds"])
    print(label, f"loss {ref['loss']} vs {res['loss']}; kinks {ref['kinks']};",
          {k: f"{d:.1e}/{m:.1e} ({c} masked)" for k, (d, m, c) in per.items()})
    assert abs(res["loss"][0] - ref["loss"][0]) <= loss_tol * abs(ref["loss"][0]), (res["loss"], ref["loss"])
    if "coords1" in res:     # step()'s coordinates: [N, 3] in global row order, the step-1 forward's
        c_ref, c = ref["coords1"], res["coords1"].to(ref["coords1"].device)
        assert c.shape == c_ref.shape and float((c - c_ref).abs().max()) <= 1e-5 * float(c_ref.abs().max())
    assert abs(res["loss"][1] - ref["loss"][1]) <= 1e-4 * abs(ref["loss"][1]), (res["loss"], ref["loss"])
    for name, (d, m, _) in per.items():
        assert d <= grad_tol * m, (label, name, d, m)
    names = {id(p): n for n, p in model.named_parameters()}
    gmax = float(g_ref.abs().max())
    for p, o in zip(opt.params, opt.offsets):
        name = names[id(p)]
        sl = slice(o, o + p.numel())
        if name == "dense3.bias":
            assert float(g[sl].abs().max()) <= 1e-3 * gmax
            continue
        gr = g_ref[sl].view(p.shape)
        sig = (gr.abs() > 1e-3 * gr.abs().max()) & (gr.abs() > 1e-6) & ~masks[name]
        if sig.any():
            dp = (ref["flat1"][sl].view(p.shape) - res["flat1"][sl].view(p.shape).to(gr.device)).abs()
            assert float(dp[sig].max()) < 1e-6, (label, name, float(dp[sig].max()))
    l2 = _loss_at(ref, res["flat1"])          # teacher-forced step 2 (the ref model's state is spent)
    print(label, f"step-2 loss at the run's own step-1 parameters: single GPU {l2:.9g} vs run {res['loss'][1]:.9g}")
    assert abs(res["loss"][1] - l2) <= loss_tol * abs(l2), (res["loss"][1], l2)


def _graph_worker(rank, world, port, n, out, mode):
    """RCCL, captured sharded step (kernels + collectives in one hipGraph) vs eager steps."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    try:
        hicgat, adj, truth, x = _inputs(n, dev)
        res = []
        for graphed in (False, True):
            torch.manual_seed(0)
            model = hicgat.GATNetSelectiveResidualsUpdated().to(dev)
            tr = hicgat.dist.ShardedTrainer(model, x, adj, truth, lr=1e-3, mode=mode)
            losses = []
            if graphed:
                step = tr.captured(warmup=2)
                losses += [None, None]
                for _ in range(3):
                    losses.append(float(step()[0]))
            else:
                tr.opt.enable_device_step()
                for _ in range(5):
                    losses.append(float(tr.step()[0]))
            torch.cuda.synchronize()
            res.append((losses, tr.opt.flat.clone().cpu()))
        if rank == 0:
            torch.save({"eager": res[0][0], "graph": res[1][0], "pe": res[0][1], "pg": res[1][1]}, out)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["slab", "xagg", "allgather"])
def test_sharded_rccl_graph_replay_equals_eager(tmp_path, mode):
    out = str(tmp_path / f"graph_{mode}.pt")
    mp.spawn(_graph_worker, args=(1, _port(), 700, out, mode), nprocs=1, join=True)
    r = torch.load(out, weights_only=True)
    assert r["eager"][2:] == r["graph"][2:]
    assert torch.equal(r["pe"], r["pg"])


def _worker(rank, world, port, backend, n, out, mode="slab", big_group=None):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        hicgat, adj, truth, x = _inputs(n, dev)
        if big_group is not None:
            hicgat.paramgrads.BIG_GROUP = big_group
        torch.manual_seed(0)
        model = hicgat.GATNetSelectiveResidualsUpdated().to(dev)
        tr = hicgat.dist.ShardedTrainer(model, x, adj, truth, lr=1e-3, mode=mode)
        loss, stats, coords = tr.step()
        coords1 = coords.clone().cpu()
        grad1 = tr.opt.grad.clone().cpu()
        flat1 = tr.opt.flat.clone().cpu()
        stats = stats.clone()           # the trainer's stats buffer is reused by the next step
        l1 = float(loss)
        loss2, _, _ = tr.step()
        torch.cuda.synchronize()
        if rank == 0:
            torch.save({"loss": [l1, float(loss2)], "grad1": grad1, "flat1": flat1, "stats": stats.cpu(), "coords1": coords1,
                        "mode": tr.mode, "rows": [int(v) for v in tr.plan.counts]}, out)
    finally:
        dist.destroy_process_group()


def _run(world, backend, n, tmp_path, mode="slab", big_group=None):
    out = str(tmp_path / f"{backend}{world}{mode}.pt")
    mp.spawn(_worker, args=(world, _port(), backend, n, out, mode, big_group), nprocs=world, join=True)
    return torch.load(out, weights_only=True)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("mode,n,big", [("slab", 777, None), ("slab", 777, 1.0), ("allgather", 777, 1.0),
                                        ("xagg", 777, None), ("xagg", 3000, None), ("xagg", 20000, None)])
def test_sharded_single_rank_rccl_equals_autograd_step(tmp_path, mode, n, big):
    """World 1 over RCCL vs the single-GPU step (two steps), compared kink-aware (tests/kinks.py):
    the aggregate-first form ("xagg": out = W (sum alpha x) + b, gat_xagg.hip) rounds the GATConv
    differently, so a relu input at rounding level from 0 may flip; those entries are masked and
    everything else must hold loss to the north star's 1e-5 and gradients to 1e-4 of their max.
    n = 777 is the size whose block-2 LN output at |z| = 6e-8 flipped in round 3; n = 20000 is the
    synth-20000 workload (BASELINE configs[2]).  ``big`` = 1: paramgrads.BIG_GROUP lowered so that EVERY
    parameter-gradient job of the MLP tail qualifies for holding -- the sharded step must not hold
    them (it has no GATConv backward to issue them before its gradient all-reduce's tail bucket)."""
    res = _run(1, "nccl", n, tmp_path, mode, big)
    ref = _single_gpu_steps(n)
    slab = mode == "slab"      # the h-first order of the single-GPU step: tighter
    _assert_step_matches(ref, res, loss_tol=1e-6 if slab else 1e-5, grad_tol=1e-5 if slab else 1e-4, label=f"{mode} n={n}")


_ORACLE20K = {}


def _oracle_step1_synth20000():
    """The CPU oracle's training step 1 on synth-20000 (oracle/gat.py, seed-0 weights, exact-formula
    distances as the device computes them; the same construction as
    tests/test_gpu_fullsize.py::test_synth20000_training_step_matches_oracle): loss, coordinates and
    every parameter's gradient, computed once per module."""
    if not _ORACLE20K:
        from hicgat import synth
        from oracle import gat as og
        from oracle import graph as ogr
        n = 20000
        i, j, c = synth.contact_pairs(n, density=0.01, seed=0)
        rows, cols = np.concatenate([i, j]), np.concatenate([j, i])
        order = np.lexsort((cols, rows))
        rows, cols = rows[order], cols[order]
        rp = np.zeros(n + 1, dtype=np.int64)
        np.add.at(rp, rows + 1, 1)
        radj = (torch.tensor(np.cumsum(rp)), torch.tensor(cols.astype(np.int64)))
        y = torch.zeros((n, n), dtype=torch.float64)
        y[torch.tensor(i), torch.tensor(j)] = torch.tensor(c)
        y[torch.tensor(j), torch.tensor(i)] = torch.tensor(c)
        t_ref = ogr.cont2dist(y, 0.5).float()
        del y
        torch.manual_seed(0)
        ref = og.GATNetSelectiveResidualsUpdated()
        og.CDIST_MODE = "donot_use_mm_for_euclid_dist"
        try:
            c_ref = ref.get_model(torch.tensor(synth.features(n, seed=0)), radj)
            l_ref = torch.nn.functional.mse_loss(torch.cdist(c_ref, c_ref, compute_mode=og.CDIST_MODE).float(), t_ref)
            l_ref.backward()
        finally:
            og.CDIST_MODE = "use_mm_for_euclid_dist_if_necessary"
        _ORACLE20K.update(loss=float(l_ref.item()), coords=c_ref.detach().clone(),
                          grads={k: p.grad.detach().clone() for k, p in ref.named_parameters()})
    return _ORACLE20K


def _assert_step1_matches_oracle(ref, res, label=""):
    """A sharded run's step 1 (rank 0: the all-gathered coordinates, the all-reduced flat gradient)
    against the CPU oracle directly: loss and coordinates to the north star's 1e-5 relative, every
    gradient to 2e-4 of its tensor's max outside the kink-decided entries of ``ref`` (bounded by
    their flipped term, tests/kinks.py) -- the bar of the single-GPU oracle test."""
    from kinks import compare_flat
    o = _oracle_step1_synth20000()
    rel_l = abs(res["loss"][0] - o["loss"]) / abs(o["loss"])
    c, c_ref = res["coords1"].double(), o["coords"].double()
    rel_c = float((c - c_ref).abs().max() / c_ref.abs().max())
    model, opt = ref["model"], ref["opt"]
    names = {id(p): k for k, p in model.named_parameters()}
    g_ref = torch.zeros_like(ref["grad1"])
    for p, off in zip(opt.params, opt.offsets):
        g_ref[off:off + p.numel()] = o["grads"][names[id(p)]].reshape(-1).to(g_ref.device)
    per = compare_flat(model, zip(opt.params, opt.offsets), g_ref, res["grad1"].to(g_ref.device), ref["masks"],
                       bounds=ref["bounds"])
    print(label, f"vs oracle: loss {res['loss'][0]:.9g} vs {o['loss']:.9g} (rel {rel_l:.2e}); coords rel {rel_c:.2e};",
          {k: f"{d / m:.1e} ({n_})" for k, (d, m, n_) in per.items()})
    assert rel_l < 1e-5 and rel_c < 1e-5, (rel_l, rel_c)
    for k, (d, m, _) in per.items():
        assert d <= 2e-4 * m, (label, k, d, m)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world,mode", [(2, "slab"), (2, "auto"), (8, "auto")])
def test_configs3_synth20000_sharded_matches_single_gpu(tmp_path, world, mode):
    """BASELINE configs[3]: the synth-20000 graph (bench.py's workload, N = 20000, 4.02 M edges)
    destination-row sharded over ``world`` ranks in the form bench.py --gpus runs ("auto": xagg --
    10 000-row shards at P = 2, 2 500-row shards at P = 8, the head-fused one-kernel tail, the edge
    pass) and the slab form at P = 2, gloo ranks sharing the one GPU, two training steps against
    the single-GPU step from the same seed (HiC-GNN_main.py:123-132): loss 1e-5 relative at both
    steps, every step-1 gradient to 1e-4 of its max with the kink-decided entries masked, the
    step-1 Adam update.  And step 1 against the CPU oracle itself (not only through the single-GPU
    step): loss and coordinates 1e-5, gradients 2e-4 of their max."""
    res = _run(world, "gloo", 20000, tmp_path, mode)
    assert res["mode"] == ("slab" if mode == "slab" else "xagg") and len(res["rows"]) == world
    ref = _single_gpu_steps(20000)
    label = f"P={world} {res['mode']} rows {res['rows']}"
    _assert_step_matches(ref, res, label=label)
    _assert_step1_matches_oracle(ref, res, label=label)


@pytest.mark.parametrize("world,mode,n", [(2, "slab", 777), (2, "xagg", 777), (2, "allgather", 777), (3, "slab", 777),
                                          (3, "xagg", 777), (3, "allgather", 777), (4, "xagg", 777), (8, "xagg", 777),
                                          (2, "xagg", 3000)])
def test_sharded_ranks_equal_one_rank(tmp_path, world, mode, n):
    """nnz-balanced shards over gloo on the one GPU, every step form, 2 and 3 (uneven) ranks, and the
    form bench.py's "auto" runs at the driver's 4 and 8 ranks (xagg), against world 1 of the same
    form; n = 3000 puts 1 500 / 3 000 rows on a rank: the one-kernel tail on both sides."""
    one = _run(1, "gloo", n, tmp_path, mode)
    many = _run(world, "gloo", n, tmp_path, mode)
    # the MLP tail runs on shards of the rows and the partial sums (dW, dcoords, loss moments) are
    # added across ranks: another fp32 summation order, so agreement to rounding, not bitwise
    assert abs(many["loss"][0] - one["loss"][0]) <= 1e-6 * abs(one["loss"][0])
    assert torch.allclose(many["stats"][:7], one["stats"][:7], rtol=1e-6)
    g1, g2 = one["grad1"], many["grad1"]
    assert (g2 - g1).abs().max().item() <= 1e-5 * g1.abs().max().item()
    np.testing.assert_allclose(many["loss"], one["loss"], rtol=1e-3)


@pytest.mark.parametrize("mode,n,world", [("slab", 777, 3), ("xagg", 777, 3), ("xagg", 3000, 2)])
def test_simulated_ranks_run_their_shares(mode, n, world):
    """bench.py --simulate-world: each rank's share of a sharded step runs captured on one GPU with
    each collective emulated on its stream (hicgat_sim_collective); the shards partition the edges, slabs, tiles and support rows.  n = 3000
    over 2 ranks puts 1 500 rows on a rank: the one-kernel tail forward / backward (ops.fused_tail)
    inside the captured sharded step."""
    from hicgat import ops
    hicgat, adj, truth, x = _inputs(n, "cuda")
    tot = {"nnz": 0, "slab": 0, "tiles": 0, "srows": 0}
    for r in range(world):
        torch.manual_seed(0)
        model = hicgat.GATNetSelectiveResidualsUpdated().to("cuda")
        tr = hicgat.dist.ShardedTrainer(model, x, adj, truth, lr=1e-3, comm=hicgat.dist.SimComm(world, r), mode=mode)
        assert ops.fused_tail_ok(model, torch.empty(tr.local_rows, 512, device="cuda")) == (n == 3000)
        step = tr.captured(warmup=1)
        for _ in range(2):
            loss = step()[0]
        torch.cuda.synchronize()
        assert torch.isfinite(loss).item()
        tot["nnz"] += tr.local_nnz
        tot["slab"] += tr.slab_nnz if mode == "slab" else tr.local_nnz    # the xagg form has no slab pass
        tot["tiles"] += tr.t1 - tr.t0
        tot["srows"] += tr.s1 - tr.s0
    assert tot["nnz"] == tot["slab"] == adj.device_nnz
    assert tot["srows"] == n and tot["tiles"] == tr.plan.tiles


@pytest.mark.parametrize("mode,n", [("slab", 300), ("slab", 777), ("xagg", 300), ("xagg", 777)])
def test_world1_step_matches_float64_standin(mode, n):
    """One world-1 step of each form on the HIP kernels against the same step on the float64 torch
    stand-ins (tests/cpu_kernels.py, tied to the autograd oracle by tests/test_dist_gloo.py), per
    parameter: localises a kernel / GEMM-call fault to the gradient it touches."""
    import torch.distributed as dist
    from cpu_kernels import CpuKernels, torch_tail
    hicgat, adj, truth, x = _inputs(n, "cuda")
    res = {}
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(_port())
    dist.init_process_group("gloo", rank=0, world_size=1)
    cls = hicgat.GATNetSelectiveResidualsUpdated
    saved = (cls.post_act, cls.tail)
    try:
        for dev in ("cuda", "cpu"):
            if dev == "cpu":
                torch_tail(hicgat)
                from hicgat import synth
                i, j, _ = synth.contact_pairs(n, density=0.05, seed=3)
                a2 = hicgat.Adj(torch.tensor(i), torch.tensor(j), None, (n, n)).to_symmetric().to("cpu")
                t2 = hicgat.Truth(truth.dense().cpu())
                kw = dict(kern=CpuKernels())
            else:
                a2, t2, kw = adj, truth, {}
            torch.manual_seed(0)
            model = cls().to(dev)
            tr = hicgat.dist.ShardedTrainer(model, x.to(dev), a2, t2, lr=1e-3, mode=mode, **kw)
            loss, stats, _ = tr.step()
            res[dev] = (float(loss), tr.opt.grad.detach().cpu().clone(), tr.opt, model)
    finally:
        cls.post_act, cls.tail = saved
        dist.destroy_process_group()
    (lg, gg, opt, model), (lc, gc, _, _) = res["cuda"], res["cpu"]
    # the float64 stand-in decides every relu exactly; the fp32 run may flip one at rounding level
    from kinks import compare_flat
    torch.manual_seed(0)
    m0 = cls().to("cuda")
    masks, counts, bounds = _kink_info(hicgat, m0, x, adj, truth)
    per = compare_flat(model, zip(opt.params, opt.offsets), gc, gg, {k: v.cpu() for k, v in masks.items()},
                       bounds={k: v.cpu() for k, v in bounds.items()})
    print(mode, f"loss {lg:.8e} vs {lc:.8e}; kinks {counts}", {k: f"{d:.1e}/{m:.1e} ({c})" for k, (d, m, c) in per.items()})
    assert abs(lg - lc) <= 1e-5 * abs(lc)
    for k, (d, m, _) in per.items():
        assert d <= 2e-4 * m, (k, d, m)


@pytest.mark.parametrize("n,world", [(3000, 1), (3000, 2)])
def test_xagg_head_fused_tail_matches_separate_launches(n, world):
    """The head-fused tail kernels (hicgat_tail_{fwd,bwd} with HICGAT_TAIL_HEADS: the xagg GATConv's per-head
    GEMMs + bias / relu before the tail, its rows backward and dxa GEMMs after the tail's backward)
    against the separate launches (grouped row GEMMs, xagg_rows_bwd), rank 0 of ``world`` simulated
    ranks, two eager steps and two graph replays: the same loss to 1e-6, gradients to 1e-5 of their
    max (the head GEMMs sum K in another order), and the captured form replays bit-equal to eager."""
    from hicgat import ops
    hicgat, adj, truth, x = _inputs(n, "cuda")
    res = {}
    saved = ops.TAIL_HEADS
    try:
        for heads in (False, True):
            ops.TAIL_HEADS = heads
            out = []
            for graphed in (False, True):
                torch.manual_seed(0)
                model = hicgat.GATNetSelectiveResidualsUpdated().to("cuda")
                tr = hicgat.dist.ShardedTrainer(model, x, adj, truth, lr=1e-3, comm=hicgat.dist.SimComm(world, 0),
                                                mode="xagg")
                assert ops.tail_heads_ok(model, tr.O) == heads
                losses, grads = [], []
                if graphed:
                    step = tr.captured(warmup=0)
                else:
                    tr.opt.enable_device_step()
                    step = tr.step
                for _ in range(2):
                    losses.append(float(step()[0]))
                    grads.append(tr.opt.grad.clone())
                torch.cuda.synchronize()
                out.append((losses, grads, tr.opt.flat.clone()))
            (le, ge, pe), (lg, gg, pg) = out
            assert le == lg and all(torch.equal(a, b) for a, b in zip(ge, gg)) and torch.equal(pe, pg), heads
            res[heads] = out[0]
    finally:
        ops.TAIL_HEADS = saved
    (l0, g0, _), (l1, g1, _) = res[False], res[True]
    assert abs(l1[0] - l0[0]) <= 1e-6 * abs(l0[0]), (l0, l1)
    assert (g1[0] - g0[0]).abs().max().item() <= 1e-5 * g0[0].abs().max().item()
    assert abs(l1[1] - l0[1]) <= 1e-4 * abs(l0[1]), (l0, l1)


def test_sim_collective_holds_for_the_modeled_time():
    """The emulated collective of SimComm (hicgat_sim_collective): resident for the requested wall
    time on its stream (bench.py --simulate-world puts the modeled collective times into the captured
    rank step through it), overlappable with work on another stream, and argument-checked."""
    from hicgat import _lib
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    _lib.check(lib.hicgat_sim_collective(1.0, 16, 256, _lib.stream(dev)), "hicgat_sim_collective")   # code load
    torch.cuda.synchronize()
    def busy():   # keeps the GPU ahead of the host, so the events time the device, not the launch gap
        _lib.check(lib.hicgat_sim_collective(500.0, 16, 256, _lib.stream(dev)), "hicgat_sim_collective")

    for us in (15.0, 120.0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        busy()
        e0.record()
        _lib.check(lib.hicgat_sim_collective(us, 16, 256, _lib.stream(dev)), "hicgat_sim_collective")
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) * 1e3
        assert us <= t <= us + 40, (us, t)
    # two 100 us emulations on two streams overlap (16 workgroups each: the chip has room for both).
    # In a fresh process: HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES = 4 on the
    # box), and after the suite's earlier tests have made many streams, two new ones may share a
    # queue and run in order (0.238 ms for the pair, r05m)
    import subprocess
    code = (
        "import sys, torch\n"
        f"sys.path[:0] = [{os.path.dirname(HERE)!r}, {os.path.join(os.path.dirname(HERE), 'hic-gnn_amd')!r}]\n"
        "from hicgat import _lib\n"
        "lib = _lib.lib(); dev = torch.device('cuda', 0)\n"
        "def sim(us):\n"
        "    _lib.check(lib.hicgat_sim_collective(us, 16, 256, _lib.stream(dev)), 'hicgat_sim_collective')\n"
        "s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()\n"
        "sim(1.0)\n"
        "for s in (s1, s2):\n"
        "    with torch.cuda.stream(s): sim(1.0)\n"
        "torch.cuda.synchronize()\n"
        "e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)\n"
        "sim(500.0)\n"
        "e0.record(); s1.wait_event(e0); s2.wait_event(e0)\n"
        "for s in (s1, s2):\n"
        "    with torch.cuda.stream(s): sim(100.0)\n"
        "torch.cuda.current_stream().wait_stream(s1); torch.cuda.current_stream().wait_stream(s2)\n"
        "e1.record(); torch.cuda.synchronize()\n"
        "print(e0.elapsed_time(e1) * 1e3)\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    t = float(out.stdout.strip().splitlines()[-1])
    assert t < 170, t
    for bad in ((-1.0, 16, 256), (10.0, 0, 256), (10.0, 16, 100), (10.0, 16, 2048)):
        assert lib.hicgat_sim_collective(*bad, None) == -1, bad

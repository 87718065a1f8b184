"""The HiC-GNN_main.py training loop on the HIP path (a14), plus a CLI mirroring its flags
(list -> convert_to_matrix -> KRnorm on the GPU -> load_input -> train per conversion -> dSCC).

Loop semantics kept from HiC-GNN_main.py:117-132:
  Adam(lr) over model.parameters(); oldloss, lossdiff = 1, 1; truth = cont2dist(y, 0.5);
  while lossdiff > thresh: zero_grad; loss = MSE(model(x, ei), truth); lossdiff = |old - loss|;
  backward; step; old = loss.
The step runs the fused distance/loss kernel (the N x N matrix is never stored) and FlatAdam; the
loss comparison is the one device->host sync per step, as in the reference.  ``steps=K`` runs a
fixed number of steps instead (the deterministic parity protocol of SURVEY.md section 8(d)).
``loss="combined"`` is the HiC_GAT_generalize_directly.py:206-239 objective (MSE + alpha*(1-r));
``loss="contrastive"`` the train_and_test_same_res_GAT_node2vec.py:98-134 one (0.1 * mean_{i<j}
|T - D|, float64 as the reference's float64 truth makes it: the lossdiff rule reads that fp64 value).
"""
import argparse
import ast
import sys

import numpy as np
import torch

from . import graph, metrics, ops
from .gat_models import ALL_MODELS, MODELS, model_class  # noqa: F401
from .optim import FlatAdam


def train_step(model, opt, x, edge_index, truth, kind="mse", stats=None, alpha=1.0):
    """One step without any host sync: returns (loss tensor, stats tensor, coords)."""
    model.train()
    pk = ops.step_pack(model, x) if x.is_cuda else None   # the tail's packed weights ride in the first launch
    if pk is not None:
        opt.zero_grad(pack=pk)
    else:
        opt.zero_grad()
    with ops.prepacked(model, pk):
        if kind in ops.MOMENT_LOSS_KINDS:
            loss, stats, coords = model.loss(x, edge_index, truth, kind, stats=stats, alpha=alpha)
        else:
            loss, stats, coords = model.loss(x, edge_index, truth, kind, stats=stats)
    with ops.overlapped_param_grads(None if x.is_cuda else False):   # dW, db beside the backward
        ops.backward_from_loss(loss)
    opt.step()
    return loss, stats, coords


GRAPH_WARMUP = 2   # eager steps before the step is captured (real training steps, in the history)


LOSSES = ("mse", "combined", "contrastive", "mse+dscc", "mse+pearson", "rmse", "si_mse")


def train(model, data, truth, lr=1e-3, thresh=1e-8, steps=None, loss="mse", max_steps=1_000_000,
          on_step=None, graph=None, dscc_history=None, print_interval=0, alpha=1.0, mse_history=None,
          attn_dropout=0.0):
    """Returns (optimizer, per-step loss list).  ``truth`` is a ``graph.Truth``.

    ``graph`` (default: on for device tensors): after ``GRAPH_WARMUP`` eager steps the step is
    captured once (``graphs.CapturedStep``) and replayed; the loss is still read on the host every
    step for the ``lossdiff`` rule (HiC-GNN_main.py:128) -- replays give the same bits as eager steps.
    ``dscc_history`` (a list): the dSCC of every step's forward coordinates against the target, as
    HiC_GAT_generalize_directly.py:242-247 appends it; ``print_interval`` > 0 prints its progress line
    (:256) every that many steps.  The score is ``metrics.DsccScorer``'s, built once for the run; it
    runs INSIDE the step (so inside the captured graph) and its rho rides in the same device buffer
    as the loss value: still one device -> host read per step.

    ``loss="mse+dscc"`` is the combined_loss_training.py:106-146 objective: the recorded value is
    MSE + ``alpha`` * (1 - rho) with a NaN rho replaced by 0 (:136-138), the gradient is the MSE's
    (the Spearman term is detached there too), rho is scored on ``model.get_model``'s coordinates
    (:132-133: the step's own for a model without dropout sites, a second no-grad forward for a
    ``_DropoutMLP``); fixed ``steps`` gives the script's epoch loop.  ``dscc_history`` then receives
    each step's rho and ``mse_history`` (a list) the MSE part.

    ``loss="mse+pearson"`` (mse + ``alpha`` * (1 - r), the gradient through both terms), ``"rmse"`` and
    ``"si_mse"`` are the moment-dependent kinds of ``ops.fused_dist_loss``; the recorded value is the fp32
    loss and ``dscc_history`` works as for ``"mse"``.

    ``attn_dropout`` = p > 0 sets ``model.conv.dropout`` (PyG's GATConv(dropout=p): dropout on the
    attention coefficients in training mode; 0 leaves the model as it is).  The conv's own
    ``DropoutState`` is made by the first eager step, so the captured step replays as the next step."""
    from .graphs import CapturedStep
    from .dropout import check_p
    from .nn import GATConv
    if check_p(attn_dropout) > 0.0:
        if not isinstance(getattr(model, "conv", None), GATConv):
            raise ValueError(f"attn_dropout needs a model whose ``conv`` is a GATConv; {type(model).__name__} has none")
        model.conv.dropout = check_p(attn_dropout)
    if loss not in LOSSES:       # a KeyError, as ops.LOSS_KINDS[kind] raises for the fused kinds
        raise KeyError(f"unknown loss {loss!r}: one of {', '.join(LOSSES)}")
    with_dscc = loss == "mse+dscc"
    kind = "mse" if with_dscc else loss
    opt = FlatAdam(model.flat_parameters(), lr=lr)
    use_graph = data.x.is_cuda if graph is None else bool(graph)
    if use_graph:
        opt.enable_device_step()
    old, diff, hist = 1.0, 1.0, []
    stats = torch.empty(12, dtype=torch.float64, device=data.x.device)
    scorer = metrics.DsccScorer(truth.scoring()) if (dscc_history is not None or with_dscc) else None
    # (rho, sum b^2, tie groups, NaN flag, the step's loss value): what the host reads per step
    host = torch.zeros(5, dtype=torch.float64, device=data.x.device) if scorer is not None else None
    from .gat_models import _DropoutMLP
    rescore = with_dscc and isinstance(model, _DropoutMLP)

    def step():
        scored = None
        if rescore:      # :132 get_model never drops; run on this step's parameters, before their update
            with torch.no_grad():
                scored = model.get_model(data.x, data.edge_index).contiguous()
        val, st, coords = train_step(model, opt, data.x, data.edge_index, truth, kind, stats, alpha)
        if scorer is not None:
            host[4].copy_(st[10] if kind == "contrastive" else val.detach())
            scorer.score_into(coords.detach().contiguous() if scored is None else scored, host)
        return val, st, coords

    replay = None
    while (diff > thresh if steps is None else len(hist) < steps) and len(hist) < max_steps:
        if use_graph and replay is None and len(hist) >= GRAPH_WARMUP:
            replay = CapturedStep(step, warmup=0)     # captured, not run: the replay below is this step
        val, st, coords = replay() if replay is not None else step()
        # the one device -> host read per step (the contrastive total is float64 in the reference)
        if scorer is not None:
            rho, _, _, _, lv = host.tolist()
        else:
            lv = float(st[10].item()) if loss == "contrastive" else float(val.item())
        if with_dscc:
            if mse_history is not None:
                mse_history.append(lv)
            lv = lv + alpha * (1.0 - (0.0 if rho != rho else rho))
        diff = abs(old - lv)
        old = lv
        hist.append(lv)
        if dscc_history is not None:
            dscc_history.append(rho)
            if print_interval and (len(hist) - 1) % print_interval == 0:
                print(f"Iteration [{len(hist) - 1}], Total Loss: {float(stats[7]):.6g}, dSCC: {dscc_history[-1]}, "
                      f"Loss Diff: {diff}")
        if on_step is not None:
            on_step(len(hist), lv)
    opt.sync_step_count()     # replays advanced only the device count
    return opt, hist


def cpu_state_dict(model):
    """The state_dict as plain CPU tensors (no views into FlatAdam's device buffers), so the saved
    .pt loads with a bare ``torch.load(path)`` on a CPU-only host, as the reference's evaluate /
    generalise scripts do (evaluate.py:87, HiC_GAT_generalize_directly.py:313)."""
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def parse_conversions(text):
    """HiC-GNN_main.py:51-58: '[a, step, b]' -> np.arange(a, b, step), '[f]' -> [f]."""
    conv = ast.literal_eval(text)
    if len(conv) == 3:
        return list(np.arange(conv[0], conv[2], conv[1]))
    if len(conv) == 1:
        return [conv[0]]
    raise ValueError("Invalid conversion input.")


def make_parser():
    """The CLI's argument parser (HiC-GNN_main.py's flags)."""
    p = argparse.ArgumentParser(description="Train a GAT-HiC model on the MI355X path "
                                            "(HiC-GNN_main.py flags).")
    p.add_argument("matrix", help="Hi-C list (bin_i bin_j count) or dense matrix text file")
    p.add_argument("features", help="N x F embedding text file (np.loadtxt), or 'node2vec' to generate the "
                                    "embeddings on the GPU from the zero-diagonal contact matrix (hicgat.embed, "
                                    "the HiC_GAT_generalize_directly.py:150-155 call), or 'line' for the LINE "
                                    "embeddings HiC-GNN_main.py:91-96 makes itself (hicgat.embed.line; -bs / -ep)")
    p.add_argument("-bs", "--batchsize", type=int, default=128, help="LINE batch size (HiC-GNN_main.py:34)")
    p.add_argument("-ep", "--epochs", type=int, default=10, help="LINE epochs (HiC-GNN_main.py:35)")
    p.add_argument("-c", "--conversions", default="[.1,.1,2]", help="conversion list, '[a, step, b]' or '[f]' "
                                                                    "(HiC-GNN_main.py:33)")
    p.add_argument("-lr", "--learningrate", type=float, default=1e-3)
    p.add_argument("-th", "--threshold", type=float, default=1e-8)
    p.add_argument("--steps", type=int, default=None, help="fixed step count instead of the threshold rule")
    p.add_argument("--model", default="GATNetSelectiveResidualsUpdated", choices=sorted(ALL_MODELS))
    p.add_argument("--loss", default="mse", choices=list(LOSSES))
    p.add_argument("--alpha", type=float, default=1.0, help="weight of the (1 - dSCC) term of --loss mse+dscc "
                                                            "(combined_loss_training.py:142) or of the (1 - r) "
                                                            "term of --loss mse+pearson")
    p.add_argument("--attn-dropout", type=float, default=0.0, metavar="P",
                   help="dropout on the GATConv's attention coefficients while training (PyG's "
                        "GATConv(dropout=P)); 0: none")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None, help="prefix for <out>_weights.pt / _structure.pdb / _log.txt")
    p.add_argument("--no-kr", action="store_true", help="the input is already KR-normalised (skip KRnorm)")
    return p


def main(argv=None):
    """HiC-GNN_main.py's pipeline: list -> convert_to_matrix -> zero diagonal -> KRnorm ->
    embeddings -> load_input -> one model per conversion value -> best dSCC -> weights / PDB / log.

    As in the reference (HiC-GNN_main.py:108-132), EVERY conversion value trains a fresh model
    against ``cont2dist(y, 0.5)`` and is scored against that same truth: the value only labels the
    run (the reference never passes it to cont2dist); the models differ by their random init (one
    seed for the whole sweep, the RNG stream continuing from model to model)."""
    p = make_parser()
    a = p.parse_args(argv)
    conv = parse_conversions(a.conversions)
    mat = np.loadtxt(a.matrix)
    if mat.shape[1] == 3:                       # HiC-GNN_main.py:75-78
        print("Converting coordinate list format to matrix.")
        mat = graph.convert_to_matrix(mat)
    np.fill_diagonal(mat, 0)                    # :80
    if a.features == "node2vec":                # node2vec on the zero-diagonal contact graph (:150-155)
        from .embed import node2vec
        feats = node2vec(mat, seed=a.seed if a.seed else 42).cpu().numpy()
    elif a.features == "line":                  # HiC-GNN_main.py:91-96: LINE(G, 512, order='second').train(bs, ep)
        from . import embed
        feats = embed.line(mat, embedding_size=512, order="second", batch_size=a.batchsize, epochs=a.epochs,
                           seed=a.seed if a.seed else 42).cpu().numpy()
    else:
        feats = np.loadtxt(a.features).astype(np.float32)
    if not a.no_kr:                             # :85-89 (Rscript normalize.R -> r_utils.R KRnorm)
        from .kr import KRnorm
        normed, keep = KRnorm(mat)
        mat = normed.cpu().numpy()
        feats = feats[keep.cpu().numpy()] if len(keep) != len(feats) else feats
    data = graph.load_input(mat, feats)
    truth = graph.Truth.from_contacts(data.y, 0.5)     # :120, the same for every conversion
    torch.manual_seed(a.seed)
    runs = []
    for f in conv:
        print(f"Training model using conversion value {f}.")
        model = model_class(a.model)().to(data.x.device)
        extra = {"alpha": a.alpha} if a.loss in ("mse+dscc", "mse+pearson") else {}
        if a.attn_dropout:
            extra["attn_dropout"] = a.attn_dropout
        _, hist = train(model, data, truth, a.learningrate, a.threshold, a.steps, a.loss, **extra)
        coords = model.get_model(data.x.float(), data.edge_index).detach()
        rho = metrics.dscc(coords, truth.scoring())
        print(f"conversion {f}: steps {len(hist)} loss {hist[-1]:.6g} dSCC {rho:.6f}")
        runs.append((rho, f, hist[-1], model, coords))
    k = [r[0] for r in runs].index(max(r[0] for r in runs))     # first maximum, as list.index(max)
    rho, f, loss, model, coords = runs[k]
    print(f"Optimal conversion factor: {f}")
    print(f"Optimal dSCC: {rho}")
    if a.out:
        from .io import write_pdb
        with open(f"{a.out}_log.txt", "w") as fh:        # :155-156
            fh.writelines([f"Optimal conversion factor: {f}\n", f"Optimal dSCC: {rho}\n", f"Final MSE loss: {loss}\n"])
        torch.save(cpu_state_dict(model), f"{a.out}_weights.pt")
        write_pdb(coords.cpu().numpy() * 100, f"{a.out}_structure.pdb")
        print(f"Saved trained model to {a.out}_weights.pt")
        print(f"Saved optimal structure to {a.out}_structure.pdb")
    return 0


if __name__ == "__main__":
    sys.exit(main())

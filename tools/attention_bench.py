#!/usr/bin/env python
"""Times of the attention-weight passes (gat_attn.hip) and of the Entropy model's step.

On the synth-20000 graph (bench.py's, seed 0):

* the alpha pass and the two passes of a gradient on alpha at (H, C) = (2, 256), each launch between
  two events, median of ``--reps`` after ``--warmup``, beside the byte model nnz * (4 + 8H) + row scalars;
* one eager training step (hicgat.train.train_step) of GATNetHeadsChanged3LayersEmbeddingDim256Entropy
  on 256 feature columns with the HIP passes, and, for scale, the same step with alpha and its backward
  formed by torch index ops on the materialised edge list (the GATConv output still from the plain HIP
  call; the torch side recomputes lin_l(x) for its logits), interleaved step by step.

Writes profiles/attention_bench.json (``--out``); ``--flagship FILE`` copies the lines of an A/B of
bench.py (this commit against its parent, alternated) into the same file.

    python tools/attention_bench.py [--reps 30] [--warmup 10] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hic-gnn_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--flagship", default=None, help="text file with the flagship A/B's bench.py JSON lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.json"))
    a = ap.parse_args()
    import hicgat
    from hicgat import ops, synth
    from hicgat.train import train_step
    dev = "cuda"
    spec = synth.WORKLOADS["synth-20000"]
    n = spec["n"]
    i, j, c = synth.contact_pairs(n, density=spec["density"], seed=0)
    A = synth.dense_contacts(n, i, j, c, device=dev)
    adj = hicgat.Adj.from_dense_device(A, keep_host=False)
    truth = hicgat.Truth.from_contacts(A, 0.5)
    del A
    nnz = adj.device_nnz
    K = hicgat.kernels.default()
    tmap = adj.transpose_map()

    # ---- the three passes at (2, 256)
    H, C = 2, 256
    torch.manual_seed(0)
    h = torch.randn(n, H * C, device=dev) * 0.1
    a_s, a_d = torch.randn(n, H, device=dev) * 0.1, torch.randn(n, H, device=dev) * 0.1
    al, ar = torch.randn(1, H, C, device=dev) * 0.1, torch.randn(1, H, C, device=dev) * 0.1
    out, rs = torch.empty(n, H * C, device=dev), torch.empty(n, 4 * H, device=dev)
    K.agg_fwd(adj.rowptr32, adj.col32, 0, n, h, a_s, a_d, torch.zeros(H * C, device=dev), 0.2, out, rs)
    alpha = torch.empty(nnz, H, device=dev)
    G = torch.randn(nnz, H, device=dev)
    cc, dd = torch.empty(n, H, device=dev), torch.empty(n, H, device=dev)
    dh, da = torch.zeros(n, H * C, device=dev), torch.zeros(n, H, device=dev)
    launches = {
        "gat_alpha": lambda: K.gat_alpha(adj.rowptr32, adj.col32, C, a_s, a_d, rs, 0.2, alpha),
        "gat_alpha_bwd_dst": lambda: K.gat_alpha_bwd_dst(adj.rowptr32, adj.col32, C, a_s, a_d, alpha, G, 0.2, cc, dd),
        "gat_alpha_bwd_src": lambda: K.gat_alpha_bwd_src(adj.rowptr32, adj.col32, tmap, a_s, a_d, alpha, G, cc, dd, al,
                                                         ar, 0.2, dh, da, rs),
    }
    # bytes each pass must move: col (+ tmap) and the [nnz, H] streams, plus per-row scalars and, for
    # the source pass, the read-modify-write of dh
    model_bytes = {
        "gat_alpha": nnz * (4 + 4 * H) + n * (4 + 4 * H * 4),
        "gat_alpha_bwd_dst": nnz * (4 + 8 * H) + n * (4 + 4 * H * 4),
        "gat_alpha_bwd_src": nnz * (8 + 8 * H) + n * (4 + 4 * H * 6) + 2 * n * H * C * 4,
    }
    passes = []
    for name, fn in launches.items():
        t = [_timed(fn) for _ in range(a.warmup + a.reps)][a.warmup:]
        row = {"pass": name, "H": H, "C": C, "N": n, "nnz": nnz, "median_us": statistics.median(t), "min_us": min(t),
               "model_bytes": model_bytes[name],
               "model_GBps_at_median": model_bytes[name] / statistics.median(t) / 1e3}
        passes.append(row)
        print(json.dumps(row))

    # ---- the Entropy model's step, HIP passes vs torch index ops
    name = "GATNetHeadsChanged3LayersEmbeddingDim256Entropy"
    x = torch.tensor(synth.features(n, f=256, seed=0), device=dev)
    row_idx = torch.repeat_interleave(torch.arange(n, device=dev), (adj.rowptr32[1:] - adj.rowptr32[:-1]).long())
    col_idx = adj.col32.long()

    class TorchAlpha(hicgat.MODELS[name]):
        def loss(self, x, edge_index, truth, kind="mse", tile_range=(0, -1), stats=None):
            conv = self.conv
            coords = self.post_act(conv(x, edge_index, act=self.conv_act))
            loss, stats = ops.fused_dist_loss(coords, truth, kind, tile_range, stats)
            hh = F.linear(x, conv.lin_l.weight).view(-1, conv.heads, conv.out_channels)
            z = (hh * conv.att_l).sum(-1)[col_idx] + (hh * conv.att_r).sum(-1)[row_idx]
            e = F.leaky_relu(z, conv.negative_slope)
            idx = row_idx.view(-1, 1).expand_as(e)
            m = torch.full((x.shape[0], conv.heads), float("-inf"), device=x.device).scatter_reduce(
                0, idx, e.detach(), reduce="amax", include_self=True)
            u = (e - m[row_idx]).exp()
            w = u / (torch.zeros_like(m).index_add(0, row_idx, u)[row_idx] + 1e-16)
            return loss + (self.alpha / (x.shape[0] * w.shape[1])) * ops.attention_entropy(w), stats, coords

    runs = {}
    for key, cls in (("hip", hicgat.MODELS[name]), ("torch_index_ops", TorchAlpha)):
        torch.manual_seed(0)
        m = cls().to(dev)
        runs[key] = (m, hicgat.FlatAdam(m.flat_parameters(), lr=1e-3))
    times = {k: [] for k in runs}
    losses = {k: [] for k in runs}
    for s in range(a.warmup + a.steps):
        for key, (m, opt) in runs.items():
            box = []
            t = _timed(lambda: box.append(train_step(m, opt, x, adj, truth)[0]))
            if s >= a.warmup:
                times[key].append(t)
            losses[key].append(float(box[0].detach()))
    step = {"model": name, "N": n, "nnz": nnz, "steps": a.steps, "mode": "eager train_step"}
    for key, t in times.items():
        step[f"{key}_median_us"] = statistics.median(t)
        step[f"{key}_min_us"] = min(t)
    step["first_loss"] = {k: v[0] for k, v in losses.items()}
    step["last_loss"] = {k: v[-1] for k, v in losses.items()}
    print(json.dumps(step))
    res = {"workload": "synth-20000 (seed 0)", "device": torch.cuda.get_device_name(0), "passes": passes,
           "entropy_model_step": step}
    if a.flagship and os.path.exists(a.flagship):
        with open(a.flagship) as fh:
            res["flagship_ab"] = [ln.rstrip("\n") for ln in fh if ln.strip()]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

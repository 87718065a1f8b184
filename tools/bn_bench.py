#!/usr/bin/env python
"""ops.bn_act_dropout against torch's own BatchNorm1d -> leaky_relu -> dropout on the same device.

Training mode, leaky_relu, p = 0.4, forward + backward, M = 20000 rows, W in {256, 128, 64}; the two
sides interleaved call by call in one process, each call between two events, median of ``--reps``
calls after ``--warmup``.  The tensors (5-20 MB) stay in L2 / MALL, so these are launch- and
latency-bound times, not HBM-bound ones.  Writes profiles/bn_bench.json.

    python tools/bn_bench.py [--rows 20000] [--reps 30] [--warmup 10] [--out profiles/bn_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bn_bench.json"))
    a = ap.parse_args()
    import hicgat
    dev = "cuda"
    results = []
    for W in (256, 128, 64):
        g = torch.Generator().manual_seed(W)
        y = torch.randn(a.rows, W, generator=g).to(dev).requires_grad_()
        dz = torch.randn(a.rows, W, generator=g).to(dev)
        bns = {k: torch.nn.BatchNorm1d(W).to(dev) for k in ("hip", "torch")}
        st = hicgat.DropoutState(dev, seed=1, p=0.4)

        def hip():
            st.advance()
            z = hicgat.ops.bn_act_dropout(y, bns["hip"], "leaky_relu", st, 0)
            return torch.autograd.grad(z, (y, bns["hip"].weight, bns["hip"].bias), dz)

        def ref():
            z = F.dropout(F.leaky_relu(bns["torch"](y)), 0.4, True)
            return torch.autograd.grad(z, (y, bns["torch"].weight, bns["torch"].bias), dz)

        times = {"hip": [], "torch": []}
        for k in range(a.warmup + a.reps):
            for name, fn in (("hip", hip), ("torch", ref)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if k >= a.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        row = {"rows": a.rows, "W": W, "reps": a.reps}
        for name, t in times.items():
            row[f"{name}_median_us"] = statistics.median(t)
            row[f"{name}_min_us"] = min(t)
        row["ratio_hip_over_torch"] = row["hip_median_us"] / row["torch_median_us"]
        results.append(row)
        print(json.dumps(row))
    out = {"workload": "BatchNorm1d -> leaky_relu -> Dropout(0.4), training mode, forward + backward",
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""LINE embeddings (hicgat.embed.line, csrc/line.hip) against the same optimiser steps done with
generic torch ops on the same device (gather, ``index_add_``, dense Adam in Keras' form).

Two cases: chr19 1 mb (tests/golden/graph_chr19_1mb.npz, N = 58) as HiC-GNN_main.py:91-96 calls it
(D = 512, B = 128, 10 epochs), and synth-2000 (bench.py's workload, D = 512, B = 1024, 1 epoch).
Per case: the wall time of ``embed.line()`` end to end (host tables + permutations + device steps,
ending in a synchronise), the device steps alone (``Line.train`` between two synchronises), and the
torch baseline over the SAME sample stream (its (h, t, y) precomputed by ``Line.samples`` outside the
timed window, so the baseline pays for no sampling).  Each timing is the median of ``--reps`` runs
after one warm-up run; the two sides alternate.  Writes profiles/line_bench.json.

    python tools/line_bench.py [--reps 5] [--out profiles/line_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hic-gnn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def torch_steps(U, C, h, t, y, lens, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """The steps of include/hicgat.h "LINE" with torch ops; (h, t, y) [steps, B] from Line.samples."""
    mU, vU, mC, vC = (torch.zeros_like(U) for _ in range(4))
    for s, n in enumerate(lens):
        hh, tt, yy = h[s, :n].long(), t[s, :n].long(), y[s, :n].float()
        u, c = U[hh], C[tt]
        g = -(yy / n) * torch.sigmoid(-yy * (u * c).sum(1))
        dU = torch.zeros_like(U).index_add_(0, hh, g[:, None] * c)
        dC = torch.zeros_like(C).index_add_(0, tt, g[:, None] * u)
        k = s + 1
        lr_t = lr * (1.0 - b2 ** k) ** 0.5 / (1.0 - b1 ** k)
        for p, d, m, v in ((U, dU, mU, vU), (C, dC, mC, vC)):
            m.mul_(b1).add_(d, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(d, d, value=1.0 - b2)
            p.addcdiv_(m, v.sqrt().add_(eps), value=-lr_t)
    return U


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def case(name, a, D, B, epochs, reps):
    from hicgat import embed
    head, tail, w = embed.line_edges(a)
    steps = embed.line_steps(len(head), B, epochs)
    chunks = -(-len(head) // B)
    lens = [min(B, len(head) - ((s % (chunks * 6)) // 6) * B) for s in range(steps)]
    probe = embed.Line(head, tail, w, a.shape[0], D, B)
    h, t, y = probe.samples(0, steps)
    U0, C0 = probe.U.clone(), probe.C.clone()
    times = {"line_wall": [], "line_steps": [], "torch_steps": []}
    last = {}
    for r in range(reps + 1):
        def hip_wall():
            last["hip"] = embed.line(a, D, batch_size=B, epochs=epochs)

        run = embed.Line(head, tail, w, a.shape[0], D, B)

        def hip_device():
            run.train(0, steps)

        def ref():
            last["torch"] = torch_steps(U0.clone(), C0.clone(), h, t, y, lens)

        for key, fn in (("line_wall", hip_wall), ("line_steps", hip_device), ("torch_steps", ref)):
            dt = timed(fn)
            if r > 0:
                times[key].append(dt)
    row = {"case": name, "N": int(a.shape[0]), "E": int(len(head)), "D": D, "batch_size": B, "epochs": epochs,
           "steps": steps, "reps": reps,
           "max_abs_diff_vs_torch": float((last["hip"] - last["torch"]).abs().max())}
    for key, ts in times.items():
        row[f"{key}_median_s"] = statistics.median(ts)
        row[f"{key}_min_s"] = min(ts)
    row["line_steps_per_s"] = steps / row["line_steps_median_s"]
    row["torch_steps_per_s"] = steps / row["torch_steps_median_s"]
    row["torch_over_line_steps"] = row["torch_steps_median_s"] / row["line_steps_median_s"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_bench.json"))
    a = ap.parse_args()
    from hicgat import synth
    with np.load(os.path.join(ROOT, "tests", "golden", "graph_chr19_1mb.npz")) as z:
        chr19 = np.array(z["matrix"], dtype=np.float64)
    np.fill_diagonal(chr19, 0)
    spec = synth.WORKLOADS["synth-2000"]
    i, j, c = synth.contact_pairs(spec["n"], density=spec["density"], seed=0)
    big = np.zeros((spec["n"], spec["n"]))
    big[i, j] = c
    big[j, i] = c
    results = [case("chr19_1mb", chr19, 512, 128, 10, a.reps), case("synth-2000", big, 512, 1024, 1, a.reps)]
    out = {"workload": "second-order LINE, D = 512: embed.line() vs gather + index_add_ + dense Keras-form Adam in torch",
           "device": torch.cuda.get_device_name(0), "results": results}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

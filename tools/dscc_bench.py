"""Time the per-step dSCC: the fused scorer (spearman.hip, metrics.DsccScorer.score_into) against the
generic torch path (metrics.dscc) on the same inputs.

    python tools/dscc_bench.py [--workloads synth-2000 synth-20000] [--iters 20] [--out profiles/dscc_bench.json]

Inputs per workload: the truth of bench.py's synthetic contacts (cont2dist, factor 0.5) and the
coordinates of a seeded 3-D random walk of N steps.  Every timed part runs in a child process of its
own under its own time limit, and the first part that fails (non-zero exit, time limit) ends the run:
nothing is started after it.  A torch path that runs out of device memory or of its time limit is
recorded as such (the fact replaces the ratio) and is not an error of the tool.  The fused time
is the median of ``iters`` event-timed calls after a warm-up; the torch path syncs the host inside
(its ``.item()``), so it is wall time around the call, after one warm-up call.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "hic-gnn_amd")]

LIMITS = {"fused": 240, "torch": 360}      # seconds per part (workload setup included)


def inputs(name, seed=0):
    import numpy as np
    import torch
    import hicgat
    from hicgat import synth
    spec = synth.WORKLOADS[name]
    n = spec["n"]
    i, j, c = synth.contact_pairs(n, density=spec["density"], seed=seed)
    A = synth.dense_contacts(n, i, j, c, device="cuda")
    truth = hicgat.Truth.from_contacts(A, 0.5)
    del A
    walk = np.cumsum(np.random.default_rng(seed).standard_normal((n, 3)), 0).astype(np.float32)
    return n, truth.scoring(), torch.tensor(walk, device="cuda")


def part(name, which, iters):
    import torch
    from hicgat import metrics
    n, t, coords = inputs(name)
    m = n * (n - 1) // 2
    res = {"workload": name, "n": n, "pairs": m, "path": which}
    if which == "fused":
        t0 = time.perf_counter()
        scorer = metrics.DsccScorer(t)
        torch.cuda.synchronize()
        res["prepare_truth_ms"] = (time.perf_counter() - t0) * 1e3
        res["workspace_bytes"] = scorer.ws.numel()
        for _ in range(3):
            scorer.score_into(coords)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in ev:
            e0.record()
            scorer.score_into(coords)
            e1.record()
        torch.cuda.synchronize()
        ts = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        res.update(status="ok", median_ms=ts[len(ts) // 2], min_ms=ts[0], rho=float(scorer.out[0]),
                   tie_groups=float(scorer.out[2]))
    else:
        try:
            rho = metrics.dscc(coords, t)            # warm-up (allocator, kernels)
            ts = []
            for _ in range(max(1, min(iters, 3))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rho = metrics.dscc(coords, t)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ts.sort()
            res.update(status="ok", median_ms=ts[len(ts) // 2], min_ms=ts[0], rho=rho,
                       peak_bytes=torch.cuda.max_memory_allocated())
        except torch.cuda.OutOfMemoryError as exc:
            res.update(status="out of device memory", detail=str(exc).splitlines()[0])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=["synth-2000", "synth-20000"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dscc_bench.json"))
    ap.add_argument("--part", nargs=2, metavar=("WORKLOAD", "PATH"), help="run one part in this process")
    a = ap.parse_args()
    if a.part:
        part(a.part[0], a.part[1], a.iters)
        return 0
    results, rc = [], 0
    for name in a.workloads:
        for which in ("fused", "torch"):
            cmd = [sys.executable, os.path.abspath(__file__), "--part", name, which, "--iters", str(a.iters)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[which])
            except subprocess.TimeoutExpired:
                results.append({"workload": name, "path": which, "status": f"time limit {LIMITS[which]} s"})
                rc = 1 if which == "fused" else 2
                break
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                results.append({"workload": name, "path": which, "status": f"exit {p.returncode}",
                                "stderr": p.stderr[-2000:]})
                rc = 1
                break
            results.append(json.loads(line[-1][7:]))
            print(results[-1], flush=True)
        if rc:
            break
    by = {(r["workload"], r["path"]): r for r in results}
    for name in a.workloads:
        f, t = by.get((name, "fused")), by.get((name, "torch"))
        if f and t and f.get("status") == "ok" and t.get("status") == "ok":
            f["speedup_vs_torch"] = t["median_ms"] / f["median_ms"]
            f["rho_abs_diff_vs_torch"] = abs(f["rho"] - t["rho"])
    with open(a.out, "w") as fh:
        json.dump({"results": results}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 1 if rc == 1 else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""The flagship on chr19 1 mb with LINE features: ``embed.line(mat, 512,
batch_size=128, epochs=10)`` as HiC-GNN_main.py:91-96 calls it, its ``embedding_stats``, then the
north-star protocol of tests/test_gpu_parity.py (KR, load_input, cont2dist(y, 0.5), K = 3000 fixed
steps, get_model, dSCC) over initial-weight seeds 0..7: per-seed dSCC and final loss, their median,
and whether the coordinates collapse.  Writes profiles/line_study.json.

    python tools/line_study.py [--out profiles/line_study.json] [--steps 3000]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hic-gnn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_study.json"))
    ap.add_argument("--steps", type=int, default=3000)
    a = ap.parse_args()
    import hicgat
    from hicgat import embed
    with np.load(os.path.join(ROOT, "tests", "golden", "graph_chr19_1mb.npz")) as z:
        mat = np.array(z["matrix"], dtype=np.float64)
    np.fill_diagonal(mat, 0)
    out = {"graph": "GM12878 chr19 1 mb", "steps": a.steps, "features": {}}
    for label, kw in (("line", {}), ("line_both_directions", {"both_directions": True})):
        x = embed.line(mat, 512, batch_size=128, epochs=10, **kw).cpu().numpy()
        normed, keep = hicgat.kr.KRnorm(mat.copy())
        keep = keep.cpu().numpy()
        xk = x[keep] if len(keep) != len(x) else x
        data = hicgat.load_input(normed.cpu().numpy(), xk)
        truth = hicgat.Truth.from_contacts(data.y, 0.5)
        stats = embed.embedding_stats(xk, truth.dense().cpu().numpy())
        rows = []
        for seed in range(8):
            torch.manual_seed(seed)
            model = hicgat.GATNetSelectiveResidualsUpdated().to("cuda")
            _, hist = hicgat.train.train(model, data, truth, steps=a.steps)
            with torch.no_grad():
                coords = model.get_model(data.x.float(), data.edge_index)
            rho = float(hicgat.metrics.dscc(coords, truth.scoring()))
            spread = float(coords.std(0).max())
            rows.append({"seed": seed, "dscc": rho, "loss": float(hist[-1]), "coord_std_max": spread})
            print(label, rows[-1], flush=True)
        d = np.array([r["dscc"] for r in rows])
        out["features"][label] = {"embedding_stats": stats, "runs": rows,
                                  "dscc_median": float(np.nanmedian(d)), "dscc_min": float(np.nanmin(d)),
                                  "dscc_max": float(np.nanmax(d)),
                                  "collapsed_runs": int(sum(r["coord_std_max"] < 1e-4 or r["dscc"] != r["dscc"]
                                                            for r in rows))}
        print(label, json.dumps(out["features"][label]["embedding_stats"]), "median dSCC",
              out["features"][label]["dscc_median"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

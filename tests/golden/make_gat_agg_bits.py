"""Record ``gat_agg_bits.json``: the SHA-256 of every output of the GATConv aggregation passes at every
supported (H, C), as tests/test_gpu_gat_agg_bits.py computes them (its ``outputs``; graph, inputs and
call sequence are that module's).  Needs an MI355X and the built library.

    python tests/golden/make_gat_agg_bits.py --commit <the commit the library was built from> [--out PATH]

Record before a change that must not move a bit, and let the test pass unchanged after it.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hic-gnn_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import test_gpu_gat_agg_bits as t  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=t.GOLDEN)
    a = ap.parse_args()
    hipcc = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    about = {
        "what": "SHA-256 of the raw little-endian bytes of every output of hicgat.kernels' agg_fwd_act, agg_bwd_rows, "
                "agg_bwd_dst and agg_bwd_src (the first and the last also with drop=DROP) on the graph and host-drawn inputs of "
                "tests/test_gpu_gat_agg_bits.py (n = 131; DROP = (p, seed, step counter, step_value, site) below), "
                "output buffers NaN-filled before each call; inputs_sha256: the same of every input",
        "commit": a.commit,
        "torch_hip": torch.version.hip,
        "compiler": [ln.strip() for ln in hipcc.splitlines() if "version" in ln],
        "device": torch.cuda.get_device_name(0),
        "arch": torch.cuda.get_device_properties(0).gcnArchName,
        "n": t.N, "neg_slope": t.NS, "drop": list(t.DROP),
    }
    cases = {}
    for H, C in t.SHAPES:
        got = t.outputs(H, C)
        again = t.outputs(H, C)
        assert all(t.sha(got[k]) == t.sha(again[k]) for k in got), (H, C, "two runs differ: nothing to record")
        cases[f"h{H}c{C}"] = {"inputs_sha256": t.inputs_sha(H, C), "sha256": {k: t.sha(v) for k, v in got.items()}}
        print(f"h{H}c{C}: {len(got)} outputs", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"about": about, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

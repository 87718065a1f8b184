"""Record ``pairdist_bits.json``: the SHA-256 of every output of csrc/pairdist.hip's entry points, as
tests/test_gpu_pairdist_bits.py computes them (its ``outputs``; inputs and call sequence are that
module's).  Needs an MI355X and the built library.

    python tests/golden/make_pairdist_bits.py --commit <the commit the library was built from> [--out PATH]

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

import test_gpu_pairdist_bits as t  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=t.GOLDEN)
    a = ap.parse_args()
    hipcc = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout
    about = {
        "what": "SHA-256 of the raw little-endian bytes of every output (stats[0..11], loss, dcoords / dcoords64, "
                "cglob) of hicgat.kernels' fused_loss, fused_loss_support_range, moment_loss, moment_loss_support, "
                "loss_finalize and hicgat_pairdist_bwd on the host-drawn inputs of tests/test_gpu_pairdist_bits.py, "
                "output buffers NaN-filled before each call; inputs_sha256: the same of every input of the size",
        "commit": a.commit,
        "torch_hip": torch.version.hip,
        "compiler": [ln.strip() for ln in hipcc.splitlines() if "version" in ln],
        "device": torch.cuda.get_device_name(0),
        "arch": torch.cuda.get_device_properties(0).gcnArchName,
        "background": t.BG, "alpha": t.ALPHA,
    }
    cases = {}
    for family, n in t.CASES:
        got = t.outputs(family, n)
        again = t.outputs(family, n)
        assert all(t.sha(got[k]) == t.sha(again[k]) for k in got), (family, n, "two runs differ: nothing to record")
        cases[f"{family}-n{n}"] = {"inputs_sha256": t.inputs_sha(n), "sha256": {k: t.sha(v) for k, v in got.items()}}
        print(f"{family}-n{n}: {len(got)} outputs", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"about": about, "cases": cases, "workspace_bytes": t.workspace_bytes()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Time the feature-dropout kernels (dropout.hip) with the project's event timing (kernels._timed).

    python tools/dropout_bench.py [--rows 20000] [--widths 512 256] [--iters 200]

Per width: median time of act_dropout_fwd / act_dropout_bwd (relu and leaky_relu) over ``iters``
launches after a warm-up, and the bytes/s of the traffic the kernel needs (forward 2 M W 4 bytes,
backward 3 M W 4), beside a device-to-device copy of the same tensor timed the same way.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "hic-gnn_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--widths", type=int, nargs="+", default=[512, 256])
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    from hicgat import kernels
    K = kernels.default()
    dev = "cuda"
    for W in a.widths:
        M = a.rows
        x = torch.randn(M, W, device=dev)
        dy = torch.randn(M, W, device=dev)
        y, dx, cp = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        ctr = torch.ones(1, dtype=torch.int64, device=dev)
        for act, name in ((K.ACT_RELU, "relu"), (K.ACT_LEAKY_RELU, "leaky_relu")):
            for it in (20, a.iters):           # warm-up, then the timed window
                kernels.TIMERS = {}
                for _ in range(it):
                    K.act_dropout_fwd(x, act, 0.01, 0.3, 0x1234, ctr, 0, 0, 0, y)
                    K.act_dropout_bwd(dy, y, act, 0.01, 0.3, dx)
                    with kernels._timed("copy"):
                        cp.copy_(x)
                torch.cuda.synchronize()
            for key, nbytes in (("act_dropout_fwd", 2 * M * W * 4), ("act_dropout_bwd", 3 * M * W * 4),
                                ("copy", 2 * M * W * 4)):
                ts = sorted(e0.elapsed_time(e1) * 1e-3 for e0, e1 in kernels.TIMERS[key])
                med = ts[len(ts) // 2]
                print(f"{M} x {W} {name:10s} {key:16s} median {med * 1e6:8.2f} us  min {ts[0] * 1e6:8.2f} us  "
                      f"{nbytes / med / 1e12:6.3f} TB/s ({nbytes / 1e6:.1f} MB)", flush=True)
        kernels.TIMERS = None


if __name__ == "__main__":
    main()

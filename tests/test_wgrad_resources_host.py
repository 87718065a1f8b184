"""CPU: the resources of the LDS-DMA ring weight-gradient kernel as a checked condition.

``gemm_wgrad_ring_kernel`` (csrc/gemm_wgrad.hip) runs lin_l's dW as 256 workgroups, one per CU, inside
the captured step.  It must leave room for a second workgroup per CU (other launches of the graph
co-reside): no scratch, no spills, at most 64 KB of the CU's 160 KB of LDS for its three-slot ring
(48 KB as written) and at most 256 VGPRs (two waves per SIMD of gfx950's 512-entry file; DESIGN §3,
"Weight gradients").  This compiles the file to gfx950 assembly with the flags the Makefile gives it
and reads the kernel's numeric metadata -- nothing else of the code object is looked at.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hic-gnn_amd")

FIELDS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


def _compile_command(out):
    """The Makefile's own command line for build/gemm_wgrad.o, turned into a device-only -S compile."""
    if shutil.which("make") is None:
        pytest.skip("no make")
    dry = subprocess.run(["make", "-C", PKG, "-n", "-B", "build/gemm_wgrad.o"], check=True, capture_output=True,
                         text=True).stdout
    lines = [ln for ln in dry.splitlines() if "csrc/gemm_wgrad.hip" in ln and " -c " in ln]
    assert len(lines) == 1, dry
    argv = lines[0].split()
    if shutil.which(argv[0]) is None:
        pytest.skip(f"no hipcc ({argv[0]})")
    assert "--offload-arch=gfx950" in argv, argv
    i = argv.index("-o")
    argv[i + 1] = out
    argv[argv.index("-c")] = "-S"
    return argv + ["--cuda-device-only"]


@pytest.fixture(scope="module")
def ring_kernel(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wgrad_asm") / "gemm_wgrad.s")
    subprocess.run(_compile_command(out), check=True, cwd=PKG, capture_output=True)
    with open(out) as f:
        text = f.read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = []
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:   # one list item per kernel (its .args nest deeper)
        fields = dict(re.findall(r"\n    \.(\w+):\s+(\S+)", "\n    " + entry))
        if "gemm_wgrad_ring_kernel" in fields.get("name", ""):
            found.append({k: int(fields[k]) for k in FIELDS if k in fields})
    assert len(found) == 1, found
    return found[0]


def test_ring_kernel_has_no_scratch_and_fits_two_workgroups_per_cu(ring_kernel):
    r = ring_kernel
    print(r)
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0, r
    # static LDS (the ring is a __shared__ array, no dynamic part at the launch)
    assert 0 < r["group_segment_fixed_size"] <= 65536, r
    # gfx950's unified register file: .vgpr_count is the allocation without AGPRs, which count into it
    assert r["vgpr_count"] + r.get("agpr_count", 0) <= 256, r

"""CPU: the occupancy of the fused loss's background-form tile kernel as a checked condition.

``pairdist_tile_kernel<MODE_SYM, false, KIND, BG = true, SUP>`` (csrc/pairdist.hip) is latency-bound
and needs four 256-thread workgroups per CU = four waves per SIMD on gfx950: at most 128 VGPRs (512
per SIMD lane / 4), no spills or scratch, and at most 40 KB of the CU's 160 KB of LDS (DESIGN §3,
"The fused loss chain and its floor").  This compiles the file to gfx950 assembly with the flags the
Makefile gives it and reads the numeric kernel metadata of every background instance -- nothing else
of the code object is looked at.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hic-gnn_amd")

FIELDS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
# pairdist_tile_kernel<int MODE, bool VEC, int KIND, bool BG, bool SUP> in the Itanium mangling
INSTANCE = re.compile(r"pairdist_tile_kernelILi(\d+)ELb([01])ELi(\d+)ELb([01])ELb([01])E")


def _compile_command(out):
    """The Makefile's own command line for build/pairdist.o, turned into a device-only -S compile."""
    if shutil.which("make") is None:
        pytest.skip("no make")
    dry = subprocess.run(["make", "-C", PKG, "-n", "-B", "build/pairdist.o"], check=True, capture_output=True,
                         text=True).stdout
    lines = [ln for ln in dry.splitlines() if "csrc/pairdist.hip" in ln and " -c " in ln]
    assert len(lines) == 1, dry
    argv = lines[0].split()
    if shutil.which(argv[0]) is None:
        pytest.skip(f"no hipcc ({argv[0]})")
    assert "-fno-slp-vectorize" in argv and "--offload-arch=gfx950" in argv, argv
    i = argv.index("-o")
    argv[i + 1] = out
    argv[argv.index("-c")] = "-S"
    return argv + ["--cuda-device-only"]


@pytest.fixture(scope="module")
def tile_instances(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pairdist_asm") / "pairdist.s")
    subprocess.run(_compile_command(out), check=True, cwd=PKG, capture_output=True)
    with open(out) as f:
        text = f.read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:   # one list item per kernel (its .args nest deeper)
        fields = dict(re.findall(r"\n    \.(\w+):\s+(\S+)", "\n    " + entry))
        m = INSTANCE.search(fields.get("name", ""))
        if m is None:
            continue
        key = tuple(int(v) for v in m.groups())   # (MODE, VEC, KIND, BG, SUP)
        found[key] = {k: int(fields[k]) for k in FIELDS if k in fields}
    return found


def test_background_tile_kernels_fit_four_workgroups_per_cu(tile_instances):
    bg = {k: v for k, v in tile_instances.items() if k[3] == 1}
    # MODE_SYM, no T image, the three loss kinds, with and without the support pass riding along
    assert sorted(bg) == [(0, 0, kind, 1, sup) for kind in (0, 1, 2) for sup in (0, 1)], sorted(tile_instances)
    for key, r in sorted(bg.items()):
        print(key, r)
        # gfx950's unified register file: .vgpr_count is the whole allocation; no instance uses AGPRs
        # (should one start to, count them into the 128 here)
        assert r.get("agpr_count", 0) == 0, (key, r)
        assert r["vgpr_count"] <= 128, (key, r)
        assert r["vgpr_spill_count"] == 0, (key, r)
        assert r["private_segment_fixed_size"] == 0, (key, r)
        assert r["group_segment_fixed_size"] <= 40960, (key, r)


def test_other_tile_kernels_still_compile(tile_instances):
    """The T-image forms (dynamic LDS tile) and MODE_FULL are not held to the limits, but every one
    the library launches is still there."""
    for key in [(1, 1, 0, 0, 0), (1, 0, 0, 0, 0)] + [(0, v, k, 0, 0) for v in (0, 1) for k in (0, 1, 2)]:
        assert key in tile_instances, key
        assert tile_instances[key]["vgpr_spill_count"] == 0, (key, tile_instances[key])

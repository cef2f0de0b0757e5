"""The record classification (plan::classify_records) without a GPU: tests/canonical_planner_driver.cpp, a stand-alone program with its own main, linked
with the pure host planners and the host generators only and built with ASan + UBSan, classifies the patches of the canonical-scatter meshes and
checks itself that the classes match a brute-force recomputation of every position from the CSR pattern, that the two counts add up to the patch
count and that the record order is stable inside each class.  This file checks the verdict per numbering."""
import os
import subprocess

import numpy as np
import pytest

import canonical_meshes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thunderbolt.jl_amd", "csrc")


@pytest.fixture(scope="module")
def verdicts(tb, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("canonical"))
    names = []
    for name, dh in canonical_meshes.build(tb).items():
        np.ascontiguousarray(dh.grid.xyz, dtype="<f8").tofile(os.path.join(d, name + ".xyz"))
        np.ascontiguousarray(dh.grid.conn, dtype="<i4").tofile(os.path.join(d, name + ".conn"))
        np.ascontiguousarray(dh.cell_dofs, dtype="<i4").tofile(os.path.join(d, name + ".dofs"))
        names.append(name)
    exe = os.path.join(d, "canonical_planner_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fopenmp", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-I", CSRC, os.path.join(ROOT, "tests", "canonical_planner_driver.cpp"),
                           os.path.join(CSRC, "tb_planners.cpp"), os.path.join(CSRC, "tb_hostgen.cpp"), "-o", exe])
    r = subprocess.run([exe, d, "--tile", canonical_meshes.TILE] + names, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="4"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]      # the driver's own checks, and a clean sanitizer run
    out = {}
    for line in r.stdout.splitlines():
        name, npatch, ngen, ncan = line.split()
        out[name] = (int(npatch), int(ngen), int(ncan))
    assert sorted(out) == sorted(names)
    return out


@pytest.mark.parametrize("name", sorted(canonical_meshes.EXPECT_CANONICAL))
def test_classes_per_numbering(verdicts, name):
    npatch, ngen, ncan = verdicts[name]
    assert ngen + ncan == npatch and npatch > 0
    if canonical_meshes.EXPECT_CANONICAL[name]:
        assert ncan > 0 and ngen > 0, verdicts[name]     # interior patches canonical, boundary patches general
    else:
        assert ncan == 0, verdicts[name]


def test_the_interior_tiles_are_the_canonical_ones(verdicts):
    """17 × 17 × 20 node layers in tiles of 5 × 5 × 6 are 4 × 4 × 4 patches; the 2 × 2 × 2 that touch no face of the box are canonical (the first tile of an axis
    owns the layers 0 and 1, numbered against the lexicographic order by close!(dh); the last one owns the short boundary rows).  The locality permutation
    gives the shuffled grid the generated numbering back, and with it the same classes."""
    assert verdicts["box"] == (64, 56, 8)
    assert verdicts["relocalised"] == verdicts["box"]

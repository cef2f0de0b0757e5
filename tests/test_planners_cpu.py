"""The host planners (thunderbolt.jl_amd/csrc/tb_planners.cpp, tb_spmv_planners.cpp) without a GPU: tests/planner_driver.cpp, a stand-alone program linked with the planners
and the host generators only, plans every case, checks the invariants of each plan itself and prints a digest of every plan array.  The digests are
compared with tests/golden/plan_digests.json, recorded from the plan builders before they were split into planners and an upload tail (every array that
reaches the device is byte for byte what it was; gather_nodes: from the three host functions of tb_mechanics.hip before they moved behind the same
seam; spmv: from the five plan functions of tb_spmv.hip before their host halves moved there), at 1 and at 4 OpenMP threads.  A change that alters a plan on purpose re-records the file from the
driver's output; the invariants hold either way."""
import json
import os
import subprocess

import numpy as np
import pytest

from helpers import hex_to_tets, pentagon_prism_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thunderbolt.jl_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_digests.json")
CASES = ["box", "box_two_blocks", "shuffled_box", "ring", "ideal_lv", "thin_wall", "tets", "long_rows", "colouring", "refusals", "gather_nodes", "spmv"]


def write_meshes(tb, out):
    """the meshes of the cases as raw little-endian arrays: <name>.xyz (float64), <name>.conn (int32)"""
    def put(name, xyz, conn):
        np.ascontiguousarray(xyz, dtype="<f8").tofile(os.path.join(out, name + ".xyz"))
        np.ascontiguousarray(conn, dtype="<i4").tofile(os.path.join(out, name + ".conn"))

    def box(nel, right=(1.0, 1.0, 1.0), perturb=0.2):
        return tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), right, perturb=perturb)

    g = box((12, 10, 8))
    put("box", g.xyz, g.conn)
    g0 = box((9, 8, 7), (1.0, 0.9, 0.8), 0.25)  # cells and nodes renumbered at random, as in test_patch_kernels_on_unstructured_hexahedral_meshes
    rng = np.random.default_rng(31)
    pn, pc = rng.permutation(g0.n_nodes), rng.permutation(g0.n_cells)
    inv = np.empty_like(pn)
    inv[pn] = np.arange(g0.n_nodes)
    put("shuffled_box", g0.xyz[pn], inv[g0.conn[pc]])
    g = tb.generate_ring_mesh(24, 3, 5)
    put("ring", g.xyz, g.conn)
    g = tb.generate_ideal_lv_mesh_hex(16, 4, 8)
    put("ideal_lv", g.xyz, g.conn)
    g = tb.generate_ideal_lv_mesh_hex(48, 6, 40)  # test_bisection_patcher_on_a_curved_thin_wall
    put("thin_wall", g.xyz, g.conn)
    g = box((6, 5, 4))
    put("tets", g.xyz, hex_to_tets(g.xyz, g.conn))
    g = box((3, 3, 2))
    put("q2_box", g.xyz, g.conn)
    g = box((4, 3, 3))
    put("q2_scalar", g.xyz, g.conn)  # (also the Q1 vector field of gather_nodes)
    g = pentagon_prism_mesh(tb)  # a vertex in ten cells: the staged gather does not apply
    put("prism", g.xyz, g.conn)


def build_driver(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-I", CSRC,
                           *extra, os.path.join(ROOT, "tests", "planner_driver.cpp"), os.path.join(CSRC, "tb_planners.cpp"), os.path.join(CSRC, "tb_spmv_planners.cpp"), os.path.join(CSRC, "tb_hostgen.cpp"), "-o", exe])


@pytest.fixture(scope="module")
def driver(tb, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("planners"))
    write_meshes(tb, d)
    exe = os.path.join(d, "planner_driver")
    build_driver(exe)
    return exe, d


def test_the_planners_need_no_hip_header(tmp_path):
    """tb_planners.cpp and tb_spmv_planners.cpp compile with nothing but the standard library on the include path"""
    for name in ("tb_planners", "tb_spmv_planners"):
        subprocess.check_call(["g++", "-std=c++17", "-fopenmp", "-Wall", "-Werror", "-c", os.path.join(CSRC, name + ".cpp"), "-o", str(tmp_path / (name + ".o"))])


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("case", CASES)
def test_plans_are_the_recorded_ones(driver, case, threads):
    exe, d = driver
    r = subprocess.run([exe, d, case], capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS=str(threads)))
    assert r.returncode == 0, r.stderr[-2000:]  # the driver's invariant checks
    got = dict(line.split(" ", 1) for line in r.stdout.splitlines())
    with open(GOLDEN) as f:
        want = {k: v for k, v in json.load(f).items() if k.startswith(case + "/")}
    assert want and got == want, sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


def test_the_sanitizer_pass_is_clean(driver):
    """scripts/sanitize/run.sh: the host generators, the oracle and the planner driver under ASan + UBSan, as stand-alone programs"""
    r = subprocess.run(["bash", os.path.join(ROOT, "scripts", "sanitize", "run.sh"), driver[1]], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "planners clean" in r.stdout, (r.stdout + r.stderr)[-3000:]

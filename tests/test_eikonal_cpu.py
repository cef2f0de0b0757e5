"""The eikonal unit without a GPU: the local solver through its host entry (tb_host_eikonal_local_solve shares its text with the kernel,
csrc/tb_eikonal.hpp) against brute force on the face, the host planner through a stand-alone driver (tests/eikonal_planner_driver.cpp) against an
independent NumPy incidence, the NumPy reference (tests/eikonal_reference.py) pinned on exact cases, and the ABI paperwork."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import eikonal_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thunderbolt.jl_amd", "csrc")
dp = C.POINTER(C.c_double)


def host_solve(tb, x4, x123, T, M6):
    x4, x123, T, M6 = (np.ascontiguousarray(v, dtype=np.float64) for v in (x4, x123, T, M6))
    val, lam = C.c_double(), np.zeros(3)
    tb._lib.check(tb.lib().tb_host_eikonal_local_solve(x4.ctypes.data_as(dp), x123.ctypes.data_as(dp), T.ctypes.data_as(dp), M6.ctypes.data_as(dp),
                                                       C.byref(val), lam.ctypes.data_as(dp)))
    return val.value, lam


# ------------------------------------------------------------------------------------------------ 1. local solver
def random_metric(rng, k):
    """M = R diag(1, a, b) Rᵀ, anisotropy up to 100 : 1 (every fourth one exactly 100 : 1)"""
    R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    ev = np.array([1.0, 100.0, rng.uniform(1.0, 100.0)]) if k % 4 == 0 else np.concatenate([[1.0], rng.uniform(1.0, 100.0, size=2)])
    M = (R * ev) @ R.T
    M = 0.5 * (M + M.T)
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def random_tetrahedron(rng, k):
    """every third tetrahedron is flat: x₄ at height 0, 1e-9 or 1e-4 over the plane of the face, its foot inside or outside the triangle"""
    x123 = rng.normal(size=(3, 3))
    if k % 3 == 0:
        bary = rng.dirichlet(np.ones(3)) if k % 2 == 0 else np.array([1.4, -0.3, -0.1])[rng.permutation(3)]
        nrm = np.cross(x123[1] - x123[0], x123[2] - x123[0])
        x4 = bary @ x123 + (0.0, 1e-9, 1e-4)[(k // 3) % 3] * nrm / np.linalg.norm(nrm)
    else:
        x4 = rng.normal(size=3)
    return x4, x123


def random_times(rng, k, scale):
    """time differences small against the edges (face branch), or one / two vertices late by more than an edge takes (edge and vertex branches)"""
    T = 5.0 + rng.uniform(0.0, 0.3, size=3) * scale
    mode = k % 5
    if mode in (1, 2):
        T[rng.integers(3)] += 30.0 * scale
    elif mode == 3:
        T[rng.permutation(3)[:2]] += 30.0 * scale
    elif mode == 4:
        T = 5.0 + rng.uniform(0.0, 3.0, size=3) * scale
    return T


BARY_GRID = np.array([(i, j, 100 - i - j) for i in range(101) for j in range(101 - i)], dtype=float) / 100.0


def face_points(rng, keep):
    """barycentric grid of step 1/100 and 1 000 random points of the face spanned by the vertices in `keep`"""
    pts = np.vstack([BARY_GRID, rng.dirichlet(np.ones(3), size=1000)])
    drop = [i for i in range(3) if i not in keep]
    if drop:
        pts = pts.copy()
        pts[:, drop] = 0.0
        pts = pts[pts.sum(axis=1) > 0]
        pts /= pts.sum(axis=1, keepdims=True)
    return pts


def check_one(tb, rng, x4, x123, T, M6):
    M = ref.sym6_to_33(M6)
    Y = x123 - x4
    val, lam = host_solve(tb, x4, x123, T, M6)
    assert val == val and not np.isnan(lam).any()
    fin = np.isfinite(T)
    if not fin.any():
        assert val == np.inf
        return val
    assert np.isfinite(val)
    assert (lam >= 0.0).all() and abs(lam.sum() - 1.0) <= 4e-16 * 3 and (lam[~fin] == 0.0).all()
    Tf = np.where(fin, T, 0.0)
    F = float(ref.objective(Y, Tf, M, lam))
    assert abs(val - F) <= 1e-13 * abs(F), (val, F)
    pts = face_points(rng, [i for i in range(3) if fin[i]])
    Fmu = ref.objective(Y[None], Tf[None], M[None], pts)
    worst = float((F - Fmu).max())
    assert worst <= 1e-13 * abs(F), "F(lambda) = %.17g exceeds the face minimum by %.3g" % (F, worst)
    return val


def test_local_solver_is_the_minimum_over_the_face(tb):
    rng = np.random.default_rng(20261021)
    for k in range(360):
        x4, x123 = random_tetrahedron(rng, k)
        M6 = random_metric(rng, k)
        scale = float(np.sqrt(np.einsum("id,de,ie->i", x123 - x4, ref.sym6_to_33(M6), x123 - x4)).mean())
        T = random_times(rng, k, scale)
        check_one(tb, rng, x4, x123, T, M6)


def test_local_solver_with_unreached_vertices(tb):
    rng = np.random.default_rng(7)
    for k in range(120):
        x4, x123 = random_tetrahedron(rng, k)
        M6 = random_metric(rng, k)
        T = random_times(rng, k, 1.0)
        for inf_at in ([0], [1], [2], [0, 1], [0, 2], [1, 2]):
            Ti = T.copy()
            Ti[inf_at] = np.inf
            v = check_one(tb, rng, x4, x123, Ti, M6)      # the minimum over the finite sub-face, λ = 0 at the unreached vertices
            if k % 3:                                      # a proper tetrahedron: the independent NumPy solver on the same data agrees
                want, _ = ref.local_solve((x123 - x4)[None], Ti[None], ref.sym6_to_33(M6)[None])
                assert abs(v - want[0]) <= 1e-12 * abs(want[0])
        assert check_one(tb, rng, x4, x123, np.full(3, np.inf), M6) == np.inf


def test_local_solver_agrees_with_the_reference_solver(tb):
    rng = np.random.default_rng(11)
    for k in range(200):
        x4, x123 = rng.normal(size=3), rng.normal(size=(3, 3))
        M6 = random_metric(rng, k)
        T = random_times(rng, k, 1.0)
        v, _ = host_solve(tb, x4, x123, T, M6)
        want, _ = ref.local_solve((x123 - x4)[None], T[None], ref.sym6_to_33(M6)[None])
        assert abs(v - want[0]) <= 1e-12 * abs(want[0])


def test_local_solver_refuses_bad_arguments(tb):
    z = np.zeros(9)
    val = C.c_double()
    assert tb.lib().tb_host_eikonal_local_solve(None, z.ctypes.data_as(dp), z.ctypes.data_as(dp), z.ctypes.data_as(dp), C.byref(val), None) == tb._lib.TB_ERR_BAD_ARG
    T = np.array([0.0, np.nan, 1.0])
    M6 = np.array([1.0, 0, 0, 1, 0, 1])
    assert tb.lib().tb_host_eikonal_local_solve(z.ctypes.data_as(dp), z.ctypes.data_as(dp), T.ctypes.data_as(dp), M6.ctypes.data_as(dp), C.byref(val), None) == tb._lib.TB_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ 2. planner
def planner_cases():
    rng = np.random.default_rng(3)
    xyz, hexes = ref.hex_box(3, 2, 2)
    _, tets = ref.tet_box(3, 2, 2)
    perm = rng.permutation(len(xyz)).astype(np.int32)
    renumbered = perm[hexes][rng.permutation(len(hexes))]
    _, one = ref.hex_box(1, 1, 1)
    return {"hex_3x2x2": (len(xyz), hexes), "tet_3x2x2": (len(xyz), tets), "hex_3x2x2_renumbered": (len(xyz), renumbered), "hex_1": (8, one),
            "hex_4x4x4": (125, ref.hex_box(4, 4, 4)[1])}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("eikplanner"))
    exe = os.path.join(d, "eikonal_planner_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "eikonal_planner_driver.cpp"),
                           os.path.join(CSRC, "tb_eikonal_planners.cpp"), "-o", exe])
    cases = planner_cases()
    for name, (n, conn) in cases.items():
        open(os.path.join(d, name + ".meta"), "w").write("%d %d %d\n" % (n, len(conn), conn.shape[1]))
        np.ascontiguousarray(conn, dtype=np.int32).tofile(os.path.join(d, name + ".conn"))

    def run(name):
        r = subprocess.run([exe, d, name], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert lines[0] == "rc 0", (lines[0], r.stderr)
        return cases[name], lines[1:]
    return run


@pytest.mark.parametrize("name", ["hex_3x2x2", "tet_3x2x2", "hex_3x2x2_renumbered", "hex_1", "hex_4x4x4"])
def test_planner_incidence_and_adjacency(planner, name):
    (n, conn), lines = planner(name)
    assert len(lines) == n
    tets, tet_cell = ref.tetrahedra(conn)
    ptr, others, _, _ = ref.corner_records(tets, tet_cell, n)
    # independent codes: tetrahedron index · 4 + corner, gathered per node in ascending (cell, tetrahedron) order
    code = (np.arange(len(tets))[:, None] * 4 + np.arange(4)[None, :]).ravel()[np.argsort(tets.ravel(), kind="stable")]
    seen = np.zeros(4 * len(tets), int)
    neighbours = []
    for v, line in enumerate(lines):
        left, right = line.split("|")
        recs = [(int(t.split(":")[0]), [int(x) for x in t.split(":")[1].split(",")]) for t in left.split()]
        assert [c for c, _ in recs] == code[ptr[v]:ptr[v + 1]].tolist()                       # each (tetrahedron, corner) under its node, ordered
        assert [o for _, o in recs] == others[ptr[v]:ptr[v + 1]].tolist()
        for c, _ in recs:
            seen[c] += 1
        adj = [int(x) for x in right.split()]
        assert adj == sorted(set(others[ptr[v]:ptr[v + 1]].ravel().tolist()) - {v})
        neighbours.append(set(adj))
    assert (seen == 1).all()
    for v, s in enumerate(neighbours):                                                        # symmetric
        assert all(v in neighbours[w] for w in s)
    if name == "hex_4x4x4":                                                                   # 24 tetrahedra around every interior lattice node
        I, J, K = np.meshgrid(range(5), range(5), range(5), indexing="ij")
        inner = ((I > 0) & (I < 4) & (J > 0) & (J < 4) & (K > 0) & (K < 4))
        ids = (I + 5 * (J + 5 * K))[inner]
        assert len(ids) == 27 and all(ptr[i + 1] - ptr[i] == 24 and len(lines[i].split("|")[0].split()) == 24 for i in ids)
        assert all(len(neighbours[i]) == 14 for i in ids)


def test_planner_driver_under_sanitizers(tmp_path):
    """the planner and its driver built with ASan + UBSan: a stand-alone host program, run on the renumbered box"""
    exe = str(tmp_path / "eikonal_planner_driver_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "eikonal_planner_driver.cpp"), os.path.join(CSRC, "tb_eikonal_planners.cpp"), "-o", exe])
    n, conn = planner_cases()["hex_3x2x2_renumbered"]
    open(str(tmp_path / "c.meta"), "w").write("%d %d %d\n" % (n, len(conn), 8))
    np.ascontiguousarray(conn, dtype=np.int32).tofile(str(tmp_path / "c.conn"))
    r = subprocess.run([exe, str(tmp_path), "c"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("rc 0"), r.stderr
    bad = conn.copy()
    bad[0, 0] = n                                                                             # a node id outside the mesh is refused, not read
    bad.astype(np.int32).tofile(str(tmp_path / "c.conn"))
    r = subprocess.run([exe, str(tmp_path), "c"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("rc -1"), r.stderr


# ------------------------------------------------------------------------------------------------ 3. the reference pins itself
PLANE_TENSORS = [2.0 * np.eye(3), np.diag([9.0, 1.0, 1.0]), np.diag([1.0, 4.0, 1.0])]


@pytest.mark.parametrize("mesh", ["hex_5x4x3_perturbed", "tet_3x3x2"])
@pytest.mark.parametrize("g", [0, 1, 2])
def test_reference_plane_waves_are_exact(mesh, g):
    xyz, conn = ref.hex_box(5, 4, 3, perturb=0.2, seed=1) if mesh.startswith("hex") else ref.tet_box(3, 3, 2)
    G = PLANE_TENSORS[g]
    src = np.flatnonzero(xyz[:, 0] == 0.0)
    T = ref.fixed_point(xyz, conn, ref.inverse6(G), src, np.zeros(len(src)))
    exact = xyz[:, 0] / np.sqrt(G[0, 0])
    assert np.abs(T - exact).max() <= 1e-13 * exact.max()


SPREAD_CASES = ["hex_5x4x3", "tet_3x3x2", "hex_11x10x9_fibres", "hex_1", "corner_4", "corner_8"]


@pytest.mark.parametrize("name", SPREAD_CASES)
def test_reference_sweep_orders_reach_one_fixed_point(name):
    """Gauss–Seidel forward, Gauss–Seidel reversed and Jacobi end at the same values on the meshes of the device tests.  The largest spread found is
    the yardstick written at the top of tests/test_eikonal_gpu.py (REFERENCE_SPREAD)."""
    sols = [ref.solution(name, order) for order in ("jacobi", "forward", "reversed")]
    assert all(np.isfinite(s).all() for s in sols)
    spread = max(float(np.abs(a - b).max()) for a in sols for b in sols)
    print("spread %s: %.3g (max T %.6g)" % (name, spread, sols[0].max()))
    assert spread <= 1e-14 * sols[0].max()
    c = ref.case(name)
    assert np.abs(ref.node_residual(c["xyz"], c["conn"], c["M6"], c["sources"], np.array(sols[0]))).max() == 0.0


def test_reference_unreached_nodes_stay_infinite():
    xyz, conn = ref.hex_box(2, 1, 1)
    xyz2 = np.vstack([xyz, xyz + np.array([5.0, 0, 0])])
    conn2 = np.vstack([conn, conn + len(xyz)])
    T = ref.fixed_point(xyz2, conn2, ref.inverse6(np.eye(3)), [0], [0.0])
    assert np.isfinite(T[:len(xyz)]).all() and np.isinf(T[len(xyz):]).all() and not np.isnan(T).any()


def test_reference_corner_source_is_never_early():
    for name in ("corner_4", "corner_8"):
        T = ref.solution(name)
        assert (T >= np.linalg.norm(ref.case(name)["xyz"], axis=1) - 1e-12).all()


# ------------------------------------------------------------------------------------------------ 4. paperwork
NEW_ENTRIES = ["tb_eikonal_create", "tb_eikonal_destroy", "tb_eikonal_solve", "tb_eikonal_residual", "tb_eikonal_last_counts", "tb_eikonal_potential", "tb_host_eikonal_local_solve"]


def test_new_entries_are_declared_bound_and_documented(tb):
    header = open(os.path.join(ROOT, "include", "tbhip.h"), encoding="utf-8").read()
    julia = open(os.path.join(ROOT, "julia", "ThunderboltHIPBackend.jl"), encoding="utf-8").read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    lib = C.CDLL(tb._lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name + "(" in header and name in tb._lib.SIGNATURES and ":" + name in julia and name in integration and hasattr(lib, name), name
    assert "typedef struct tb_eikonal tb_eikonal;" in header
    for name in ("EikonalModel", "EikonalActivationCache", "solve_activation", "ActionPotentialTemplate", "activation_potential"):
        assert hasattr(tb, name), name

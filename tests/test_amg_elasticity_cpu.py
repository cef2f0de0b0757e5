"""The smoothed aggregation with a near-null-space without a GPU: the block planner (csrc/tb_amg_block_planners.cpp) and the shared QR header
(csrc/tb_amg_qr.hpp) through a stand-alone driver (tests/amg_block_planner_driver.cpp, also built with the address and undefined-behaviour
sanitizers) against the restatement of tests/amg_elasticity_reference.py; the rigid-body modes against a host-assembled free-free stiffness; the
restatement's iteration counts on slender beams against the translations-only method of tests/amg_reference.py; the refusals decided on the host."""
import os
import subprocess

import numpy as np
import pytest

import amg_elasticity_reference as eref
import amg_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thunderbolt.jl_amd", "csrc")
MAX_COARSE = 32
CASES = {"cube": 0.25, "beam": 0.25, "roller": 0.25, "tet": 0.25, "small_aggregates": 0.7}


def face(tb, dh, axis, comps=(0, 1, 2)):
    X = tb.dof_coordinates(dh)
    comp = tb.amg.component_labels(dh)
    return np.flatnonzero((np.abs(X[:, axis]) < 1e-12) & np.isin(comp, comps))


def host_case(tb, name):
    """→ (dh, A eliminated, prescribed dofs): Q1 linear elasticity (ν = 0.3); `tet`: the P1 Laplacian coupled by a 3 × 3 block, for its pattern"""
    if name == "tet":
        g = tb.generate_mesh(tb.Tetrahedron, (4, 4, 4), (0, 0, 0), (1, 1, 1))
        dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
        K = ref.p1_stiffness(np.asarray(g.xyz, dtype=np.float64), np.asarray(g.conn))
        K = ref.canonical(K + 0.05 * ref.sp.diags(K.diagonal()))
        node, comp = tb.amg.dof_nodes(dh), tb.amg.component_labels(dh)
        C3 = np.array([[1.0, 0.3, 0.1], [0.3, 1.5, 0.2], [0.1, 0.2, 2.0]])
        Kd = K.toarray()
        A = ref.canonical(ref.sp.csr_matrix(Kd[np.ix_(node, node)] * C3[np.ix_(comp, comp)]))
    else:
        nel, ext = ((16, 4, 4), (4, 1, 1)) if name == "beam" else ((4, 4, 4), (1, 1, 1))
        g = tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), ext, perturb=0.1)
        dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
        A = eref.q1_elasticity(tb, dh)
    if name == "roller":
        pres = np.concatenate([face(tb, dh, a, (a,)) for a in range(3)])
    else:
        pres = face(tb, dh, 0)
    return dh, ref.eliminate(A, pres), pres


def restated(tb, name, max_coarse=MAX_COARSE):
    dh, A, pres = host_case(tb, name)
    levels = eref.hierarchy(A, tb.amg.dof_nodes(dh), len(dh.grid.xyz), tb.amg.rigid_body_modes(dh), None, CASES[name], max_coarse)
    return dh, A, pres, levels


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("amgblock"))
    src = [os.path.join(ROOT, "tests", "amg_block_planner_driver.cpp"), os.path.join(CSRC, "tb_amg_block_planners.cpp"), os.path.join(CSRC, "tb_amg_planners.cpp")]
    plain, san = os.path.join(d, "driver"), os.path.join(d, "driver_san")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC] + src + ["-o", plain])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC] + src + ["-o", san])
    return (plain, san), d


def run(exe, mode, d, name):
    r = subprocess.run([exe, mode, d, name], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def load(d, name, what, dtype):
    return np.fromfile(os.path.join(d, name + "." + what), dtype=dtype)


def write_level(d, name, A, node, n_nodes, k, per_node, node_S=None):
    A = ref.canonical(A)
    open(os.path.join(d, name + ".meta"), "w").write("%d %d %d %d %d\n" % (A.shape[0], A.nnz, n_nodes, k, per_node))
    A.indptr.astype(np.int64).tofile(os.path.join(d, name + ".ptr"))
    A.indices.astype(np.int32).tofile(os.path.join(d, name + ".col"))
    np.asarray(node, dtype=np.int32).tofile(os.path.join(d, name + ".node"))
    path = os.path.join(d, name + ".nstr")
    if node_S is not None:
        np.asarray(node_S, dtype=np.uint8).tofile(path)
    elif os.path.exists(path):
        os.remove(path)


def check_plan(exes, d, name, A, node, n_nodes, k, per_node, lev):
    """both builds of the driver on one level against the restatement's record `lev` (G, node_S, plan)"""
    for exe in exes:
        write_level(d, name, A, node, n_nodes, k, per_node, lev["node_S"])
        out = run(exe, "plan", d, name).split()
        pl, G = lev["plan"], lev["G"]
        assert out[:4] == ["rc", "0", "na", str(pl["na"])], out
        assert np.array_equal(load(d, name, "g_ptr", np.int64), G.indptr) and np.array_equal(load(d, name, "g_col", np.int32), G.indices)
        nz = load(d, name, "g_nz", np.int64)
        eptr, ent = load(d, name, "g_eptr", np.int64), load(d, name, "g_ent", np.int64)
        assert np.array_equal(lev["node_S"][nz], lev["S"])
        assert np.array_equal(np.diff(eptr), np.bincount(nz, minlength=G.nnz))
        for q in (0, G.nnz // 2, G.nnz - 1):
            assert np.array_equal(ent[eptr[q]:eptr[q + 1]], np.flatnonzero(nz == q))            # ascending: stored row-major order
        assert np.array_equal(load(d, name, "node_agg", np.int32), pl["node_agg"])
        assert np.array_equal(load(d, name, "agg", np.int32), pl["agg"])
        assert np.array_equal(load(d, name, "adof_ptr", np.int64), pl["adof_ptr"]) and np.array_equal(load(d, name, "adof", np.int32), pl["adof"])
        for key, pre in (("P", "p"), ("R", "r"), ("AP", "ap"), ("Ac", "c")):
            assert np.array_equal(load(d, name, pre + "_ptr", np.int64), pl[key][0]), key
            assert np.array_equal(load(d, name, pre + "_col", np.int32), pl[key][1]), key
        assert np.array_equal(load(d, name, "r_perm", np.int64), pl["r_perm"])
        cptr, ccol, cdiag = pl["Ac"][0], pl["Ac"][1], load(d, name, "c_diag", np.int64)
        assert all(ccol[cdiag[i]] == i and cptr[i] <= cdiag[i] < cptr[i + 1] for i in range(pl["nc"]))


_restated = {}


@pytest.fixture(params=list(CASES))
def case(request, tb):
    if request.param not in _restated:
        _restated[request.param] = restated(tb, request.param)
    return (request.param,) + _restated[request.param]


# ------------------------------------------------------------------------------------------------ 1. planner parity
def test_planner_equals_the_restatement_on_every_level(drivers, case):
    exes, d = drivers
    name, dh, A, pres, levels = case
    assert len(levels) >= 2
    for l, lev in enumerate(levels[:-1]):
        check_plan(exes, d, "%s_%d" % (name, l), lev["A"], lev["node"], lev["n_nodes"], 6, 3 if l == 0 else 6, lev)
    agg0 = levels[0]["agg"]
    if name == "roller":
        held = np.bincount(levels[0]["node"][pres], minlength=levels[0]["n_nodes"])[levels[0]["node"][pres]]
        assert (held < 3).sum() > 0 and (agg0[pres][held < 3] >= 0).all() and not levels[0]["B"][pres].any()   # a roller node stays in its aggregate, with a zero row of B
        assert (agg0[pres][held == 3] == -1).all()                                  # the corner, held in all three directions, is a clamped node
    else:
        assert (agg0[pres] == -1).all()                                             # a clamped node stays outside


@pytest.mark.parametrize("numbering", ["component_major", "random"])
def test_planner_under_a_permuted_numbering(drivers, tb, numbering):
    exes, d = drivers
    dh, A, pres = host_case(tb, "cube")
    node, n = tb.amg.dof_nodes(dh), dh.ndofs
    perm = np.argsort(tb.amg.component_labels(dh), kind="stable") if numbering == "component_major" else np.random.default_rng(3).permutation(n)
    Ap, nodep, Bp = ref.canonical(A[perm][:, perm]), node[perm], tb.amg.rigid_body_modes(dh)[perm]
    levels = eref.hierarchy(Ap, nodep, len(dh.grid.xyz), Bp, None, 0.25, MAX_COARSE)
    assert len(levels) >= 2
    check_plan(exes, d, "perm_" + numbering, Ap, nodep, len(dh.grid.xyz), 6, 3, levels[0])
    # the node aggregates do not depend on the numbering of the dofs within the nodes' blocks' norms beyond rounding: same node graph, same flags
    base = _restated.get("cube") or restated(tb, "cube")
    assert np.array_equal(levels[0]["plan"]["node_agg"], base[3][0]["plan"]["node_agg"])


# ------------------------------------------------------------------------------------------------ 2. QR parity
def test_qr_header_equals_the_restatement(drivers, tb):
    exes, d = drivers
    levels = (_restated.get("small_aggregates") or restated(tb, "small_aggregates"))[3]
    blocks = [b for lev in levels[:-1] for b in lev["blocks"]]
    rbm = levels[0]["blocks"][0]
    blocks += [rbm[:3].copy(), rbm[:6].copy(), np.zeros((4, 6)), np.random.default_rng(1).normal(size=(200, 6))]      # a single node, a pair, nothing, 200 rows (4 per lane)
    sizes = sorted({len(b) for b in blocks})
    print("QR blocks: %d, rows %s" % (len(blocks), sizes))
    assert 3 in sizes and 6 in sizes and max(sizes) > 64
    want = [eref.qr_block(b) for b in blocks]
    ratios = np.concatenate([w[3] for w in want])
    live = ratios[ratios > 1e-4]
    assert not ((ratios > 1e-12) & (ratios <= 1e-4)).any() and (ratios <= 1e-12).any()
    tol = 100 * np.finfo(float).eps / live.min()                                   # each normalisation divides the rounding of the projections by the ratio
    for exe in exes:
        open(os.path.join(d, "qr.qmeta"), "w").write("%d 6\n" % len(blocks))
        np.array([len(b) for b in blocks], dtype=np.int32).tofile(os.path.join(d, "qr.qm"))
        np.concatenate([b.ravel() for b in blocks]).tofile(os.path.join(d, "qr.qb"))
        run(exe, "qr", d, "qr")
        Q, R, dead = load(d, "qr", "qq", np.float64), load(d, "qr", "qr", np.float64).reshape(-1, 6, 6), load(d, "qr", "qdead", np.uint8).reshape(-1, 6)
        at, worst = 0, 0.0
        for b, (wq, wr, wd, _), r, dd in zip(blocks, want, R, dead):
            q = Q[at:at + b.size].reshape(b.shape)
            at += b.size
            assert np.array_equal(dd, wd)
            worst = max(worst, np.abs(q - wq).max(), np.abs(r - wr).max() / max(np.abs(wr).max(), 1e-300))
            assert np.abs(q @ r - b).max() <= 1e-14 * max(np.abs(b).max(), 1.0)                  # Q R = B, dead columns included
            assert (np.diag(r)[dd == 0] > 0).all() and not np.diag(r)[dd == 1].any() and not q[:, dd == 1].any()
        print("QR driver against the restatement: %.2e (bound %.2e, smallest live ratio %.3f)" % (worst, tol, live.min()))
        assert worst <= tol
    single, pair = want[len(blocks) - 4], want[len(blocks) - 3]
    assert single[2].sum() == 3 and pair[2].sum() == 1                             # a node keeps 3 of 6 columns, a pair loses the rotation about its axis


# ------------------------------------------------------------------------------------------------ 3. rigid-body modes
@pytest.mark.parametrize("kind", ["hex", "beam"])
def test_rigid_body_modes_lie_in_the_kernel_of_the_free_stiffness(tb, kind):
    nel, ext = ((4, 4, 4), (1, 1, 1)) if kind == "hex" else ((8, 2, 2), (4, 1, 1))
    dh = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, nel, (0.5, -1, 2), tuple(np.add((0.5, -1, 2), ext)), perturb=0.1), tb.LagrangeCollection(1) ** 3)
    K, B = eref.q1_elasticity(tb, dh), tb.amg.rigid_body_modes(dh)
    assert B.shape == (dh.ndofs, 6) and np.abs(B).max() <= 1.0 + 1e-12 and np.linalg.matrix_rank(B) == 6
    r = np.linalg.norm(K @ B) / (ref.sp.linalg.norm(K) * np.linalg.norm(B))
    print("%s: |K B| / (|K| |B|) = %.2e" % (kind, r))
    assert r <= 1e-12
    node = tb.amg.dof_nodes(dh)
    assert np.array_equal(np.bincount(node), np.full(len(dh.grid.xyz), 3)) and np.allclose(tb.dof_coordinates(dh), dh.grid.xyz[node])


# ------------------------------------------------------------------------------------------------ 4. iteration counts
@pytest.mark.parametrize("nel", [(16, 4, 4), (32, 4, 4)])
def test_counts_stay_below_the_translations_only_method(tb, nel):
    dh = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (nel[0] / 4.0, 1, 1), perturb=0.1), tb.LagrangeCollection(1) ** 3)
    pres = face(tb, dh, 0)
    A = ref.eliminate(eref.q1_elasticity(tb, dh), pres)
    b = np.random.default_rng(11).normal(size=dh.ndofs)
    b[pres] = 0.0
    rbm = eref.hierarchy(A, tb.amg.dof_nodes(dh), len(dh.grid.xyz), tb.amg.rigid_body_modes(dh), None, 0.25, MAX_COARSE)
    scalar = ref.hierarchy(A, tb.amg.component_labels(dh), None, 0.25, MAX_COARSE)
    _, it_rbm, _ = ref.pcg(A, b, lambda r: ref.vcycle(rbm, r, 2, 4.0), rtol=1e-8)
    _, it_scalar, _ = ref.pcg(A, b, lambda r: ref.vcycle(scalar, r, 2, 4.0), rtol=1e-8)
    print("%s cells, %d dofs: rigid-body modes %d iterations (%d levels, operator complexity %.2f), translations only %d (%d levels, %.2f)"
          % (nel, dh.ndofs, it_rbm, len(rbm), eref.operator_complexity(rbm), it_scalar, len(scalar), eref.operator_complexity(scalar)))
    assert it_rbm < it_scalar


# ------------------------------------------------------------------------------------------------ 5. refusals that need no device
def test_refusals_on_the_host(drivers, tb):
    exes, d = drivers
    g = tb.generate_mesh(tb.Hexahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1))
    scalar, vec, q2 = tb.DofHandler(g), tb.DofHandler(g, tb.LagrangeCollection(1) ** 3), tb.DofHandler(g, tb.LagrangeCollection(2) ** 3)
    with pytest.raises(ValueError, match="rigid_body"):
        tb.AMGPrecon(near_nullspace="rotations")
    with pytest.raises(ValueError, match="3-component"):
        tb.AMGPrecon(near_nullspace="rigid_body").check(scalar)
    with pytest.raises(ValueError, match="PMGPrecon"):
        tb.AMGPrecon(near_nullspace="rigid_body").check(q2)
    with pytest.raises(ValueError, match="k <= 6"):
        tb.AMGPrecon(near_nullspace=np.ones((vec.ndofs, 7))).check(vec)
    with pytest.raises(ValueError, match="ndofs"):
        tb.AMGPrecon(near_nullspace=np.ones((vec.ndofs - 1, 3))).check(vec)
    tb.AMGPrecon(near_nullspace="rigid_body").check(vec)
    tb.AMGPrecon(near_nullspace=np.ones((vec.ndofs, 3))).check(vec)
    with pytest.raises(NotImplementedError, match="near_nullspace"):
        tb.BidomainAMGPrecon(near_nullspace="rigid_body")
    # the planner's own checks, through the driver
    dh, A, _ = host_case(tb, "cube")
    node, nn = tb.amg.dof_nodes(dh), len(dh.grid.xyz)
    bad = node.copy()
    bad[0] = node[3]
    far = node.copy()
    far[5] = nn
    for exe in exes:
        for name, nd, k, text in (("two", bad, 6, "dofs, not 3"), ("far", far, 6, "outside 0.."), ("k7", node, 7, "1 to 6")):
            write_level(d, "bad_" + name, A, nd, nn, k, 3)
            out = run(exe, "plan", d, "bad_" + name)
            assert out.startswith("rc -1") and text in out, out

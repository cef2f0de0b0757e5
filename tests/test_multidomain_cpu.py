"""The host side of multi-domain electrophysiology without a GPU: insert_interfaces against an independent count (tests/multidomain_reference.py),
the interface planner (tests/interface_planner_driver.cpp, a stand-alone program linked with tb_interface_planners.cpp, built plainly and with
ASan + UBSan, checked against a dense NumPy scatter), the packed state map against the formula of src/discretization/fem.jl:514-521, the refusals
and the ABI additions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import multidomain_cases as cases
import multidomain_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thunderbolt.jl_amd", "csrc")
ALL = cases.MESHES + ["hex_3x2x2_perturbed", "quad_6x6"]


# ------------------------------------------------------------------------------------------------ insert_interfaces
@pytest.mark.parametrize("name", ALL)
def test_insert_interfaces(tb, name):
    g, g2 = cases.build(tb, name)
    kind = g.cell_kind
    a, b = g.getcellset("a"), g.getcellset("b")
    shared = ref.shared_facets(kind, g.conn, a, b)                     # counted independently, on the grid before the insertion
    it = g2.interfaces
    assert len(it) == len(shared) and it.nf == len(ref.FACETS[kind][0])
    assert {(r[0], r[1]): (r[2], r[3]) for r in it.records.tolist()} == shared
    assert it.records.tolist() == sorted(it.records.tolist())          # ascending (cell_a, local facet)
    on_interface = sorted({int(g.conn[c, v]) for (c, lf) in shared for v in ref.FACETS[kind][lf]})
    assert g2.n_nodes == g.n_nodes + len(on_interface) and g2.n_cells == g.n_cells
    # copies: appended, in ascending order of the node they copy, identical coordinates; everything else as it was
    assert np.array_equal(g2.xyz[:g.n_nodes], g.xyz) and np.array_equal(g2.xyz[g.n_nodes:], g.xyz[on_interface])
    copy_of = dict(zip(on_interface, range(g.n_nodes, g2.n_nodes)))
    others = np.setdiff1d(np.arange(g.n_cells), b)
    assert np.array_equal(g2.conn[others], g.conn[others])             # a (and cells of neither set) keep the old nodes
    want_b = np.vectorize(lambda v: copy_of.get(int(v), int(v)))(g.conn[b]) if len(b) else g.conn[b]
    assert np.array_equal(g2.conn[b], want_b)                          # EVERY cell of b gets the copy, also at an edge or a vertex only
    if len(shared):
        assert not np.intersect1d(g2.conn[a], g2.conn[b]).size         # no node is shared between a cell of a and a cell of b
    # the pairing: k-th node of a's facet ↔ local vertex of cell_b, the copy of that node, at the same place, on b's local facet
    for (ca, la, cb, lb), pair in zip(it.records, it.pairing):
        fa = ref.FACETS[kind][la]
        assert sorted(pair.tolist()) == sorted(ref.FACETS[kind][lb])
        for k in range(it.nf):
            va, vb = int(g2.conn[ca, fa[k]]), int(g2.conn[cb, pair[k]])
            assert vb == copy_of[va] and np.array_equal(g2.xyz[va], g2.xyz[vb])
    # sets and dims are carried over
    assert g2.dims == g.dims and set(g2.cellsets) == set(g.cellsets)
    for k in g.cellsets:
        assert np.array_equal(g2.cellsets[k], g.cellsets[k])
    if getattr(g, "facetsets", None):
        assert set(g2.facetsets) == set(g.facetsets) and all(np.array_equal(g2.facetsets[k], g.facetsets[k]) for k in g.facetsets)
    if name == "quad_3x3_centre":
        assert sorted(it.records[:, 1].tolist()) == [0, 1, 2, 3] and len(on_interface) == 4
    if name == "hex_4x4x4_inner":
        assert sorted(set(it.records[:, 1].tolist())) == [0, 1, 2, 3, 4, 5] and len(it) == 24 and len(on_interface) == 26
    if name == "quad_no_touch":
        assert len(it) == 0 and np.array_equal(g2.conn, g.conn) and np.array_equal(g2.xyz, g.xyz)


def test_insert_interfaces_refusals(tb):
    tets = tb.generate_mesh(tb.Tetrahedron, (1, 1, 1), (0, 0, 0), (1, 1, 1))
    tets.addcellset("a", np.array([0]))
    tets.addcellset("b", np.array([1]))
    with pytest.raises(NotImplementedError, match="Quadrilateral and Hexahedron"):
        tb.insert_interfaces(tets, ["a", "b"])
    g, g2 = cases.build(tb, "quad_2x1")
    with pytest.raises(NotImplementedError, match="one interface insertion per grid"):
        tb.insert_interfaces(g2, ["a", "b"])
    g.addcellset("c", np.array([0, 1]))
    with pytest.raises(ValueError, match="not disjoint"):
        tb.insert_interfaces(g, ["a", "c"])


@pytest.mark.parametrize("name", ["quad_3x3_centre", "hex_4x4x4_inner"])
def test_widened_pattern_is_the_union(tb, name):
    g, g2 = cases.build(tb, name)
    dh = tb.DofHandler(g2)
    narrow, wide = tb.allocate_matrix(dh), tb.allocate_matrix(dh, g2.interfaces)
    again = tb.allocate_matrix(dh)
    assert np.array_equal(narrow.rowptr, again.rowptr) and np.array_equal(narrow.colidx, again.colidx)
    ed = ref.interface_dofs(g2.cell_kind, dh.cell_dofs, g2.interfaces.records, g2.interfaces.pairing)
    assert np.array_equal(ed, tb.interface_dofs(dh, g2.interfaces)) and ed.shape[1] == dh.ndofs_per_cell
    want = ref.pattern_mask(narrow.rowptr, narrow.colidx)
    for d in ed:
        want[np.ix_(d, d)] = True
    assert np.array_equal(ref.pattern_mask(wide.rowptr, wide.colidx), want) and wide.nnz > narrow.nnz


# ------------------------------------------------------------------------------------------------ planner
def build_driver(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, *extra, os.path.join(ROOT, "tests", "interface_planner_driver.cpp"),
                           os.path.join(CSRC, "tb_interface_planners.cpp"), "-o", exe])


PLANNER_CASES = ["quad_2x1", "quad_3x3_centre", "hex_4x4x4_inner", "hex_3x2x2_perturbed", "quad_3x3_centre_narrow"]


@pytest.fixture(scope="module")
def planner(tb, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ifplanner"))
    want = {}
    for k, name in enumerate(PLANNER_CASES):
        g, g2 = cases.build(tb, name.replace("_narrow", ""))
        dh = tb.DofHandler(g2)
        if k % 2:                                                      # a numbering the generator did not make
            dh = tb.renumber_dofs(dh, np.random.default_rng(k).permutation(dh.ndofs).astype(np.int32))
        sp = tb.allocate_matrix(dh) if name.endswith("_narrow") else tb.allocate_matrix(dh, g2.interfaces)
        ed = ref.interface_dofs(g2.cell_kind, dh.cell_dofs, g2.interfaces.records, g2.interfaces.pairing)
        base = os.path.join(d, name)
        with open(base + ".meta", "w") as f:
            f.write("%d %d %d %d\n" % (len(ed), g2.interfaces.nf, dh.ndofs, sp.nnz))
        for ext, arr, dt in ((".edofs", ed, "<i4"), (".rowptr", sp.rowptr, "<i8"), (".colidx", sp.colidx, "<i4")):
            np.ascontiguousarray(arr, dtype=dt).tofile(base + ext)
        want[name] = ref.planner_scatter(ed, g2.interfaces.nf, sp.rowptr, sp.colidx)
    exe, exe_san = os.path.join(d, "if_driver"), os.path.join(d, "if_driver_san")
    build_driver(exe)
    build_driver(exe_san, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    return d, exe, exe_san, want


def run_driver(exe, d, case):
    r = subprocess.run([exe, d, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])     # the driver's own invariant checks
    return r.stdout


@pytest.mark.parametrize("case", PLANNER_CASES)
def test_interface_plan_lists_every_contribution_once_in_order(planner, case):
    d, exe, exe_san, want = planner
    out = run_driver(exe, d, case)
    assert run_driver(exe_san, d, case) == out                        # ASan + UBSan: clean, and the same plan
    lines = out.splitlines()
    if want[case] is None:                                            # a missing coupling is the pattern error
        assert lines == ["rc -4"]
        return
    assert lines[0] == "rc 0"
    got = []
    for ln in lines[1:]:
        tok = ln.split()
        got.append((int(tok[0]), [tuple(int(v) for v in t.split(":")) for t in tok[1:]]))
    assert got == want[case]


def test_the_interface_planner_needs_no_hip_header(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-c", os.path.join(CSRC, "tb_interface_planners.cpp"), "-o", str(tmp_path / "p.o")])


# ------------------------------------------------------------------------------------------------ packed state, refusals
def _models(tb, ion_a, ion_b, G=1.0, **kw):
    kap = tb.ConstantCoefficient(np.diag([4.5e-4, 2.0e-4]))
    one = tb.ConstantCoefficient(1.0)
    m = {"a": tb.MonodomainModel(one, one, kw.get("kappa_a", kap), tb.NoStimulationProtocol(), ion_a, "φₘ", "s1"),
         "b": tb.MonodomainModel(one, one, kap, tb.NoStimulationProtocol(), ion_b, "φₘ", "s2")}
    if G is not None:
        m["interfaces"] = tb.InterfaceDiffusionModel(tb.ConstantCoefficient(G), "φₘ", "φₘi")
    return m


@pytest.mark.parametrize("name", ["quad_3x3_centre", "quad_split_to_boundary", "hex_4x4x4_inner"])
def test_state_packing_and_heat_dofrange(tb, name):
    g, g2 = cases.build(tb, name)
    p = tb.plan_ep(tb.ReactionDiffusionSplit(_models(tb, tb.PCG2019(), tb.FHNModel())), g2)
    f, dh = p["functions"], p["dh"]
    assert [c.ode.nstates for c in f.functions] == [7, 2] and all(c.layout.code == tb._lib.TB_LAYOUT_AOS for c in f.functions)
    sub = [np.unique(dh.cell_dofs[g2.getcellset(s)]) for s in ("a", "b")]
    assert all(np.array_equal(x, y) for x, y in zip(sub, p["subdofs"])) and [c.npoints for c in f.functions] == [len(s) for s in sub]
    if name != "quad_2x1":
        assert any(np.any(np.diff(s) != 1) for s in sub)               # not contiguous: the reference would refuse, the general map does not
    want, total = ref.heat_dofrange(sub, [7, 2], [1, 1])
    assert tb.solution_size(f) == total == 7 * len(sub[0]) + 2 * len(sub[1]) and f.offsets.tolist() == [0, 7 * len(sub[0]), total]
    assert f.heat_dofrange.dtype == np.int32 and np.array_equal(f.heat_dofrange, want)
    # Aliev–Panfilov keeps φₘ in its SECOND state; StateBlocked for all children at once
    p2 = tb.plan_ep(tb.ReactionDiffusionSplit(_models(tb, tb.AlievPanfilovModel(), tb.FHNModel())), g2)
    assert np.array_equal(p2["functions"].heat_dofrange, ref.heat_dofrange(sub, [2, 2], [2, 1])[0])
    p3 = tb.plan_ep(tb.ReactionDiffusionSplit(_models(tb, tb.PCG2019(), tb.FHNModel())), g2, layout=tb.StateBlockedLayout())
    hd = np.empty(dh.ndofs, dtype=np.int64)
    hd[sub[0]] = np.arange(len(sub[0]))
    hd[sub[1]] = 7 * len(sub[0]) + np.arange(len(sub[1]))
    assert np.array_equal(p3["functions"].heat_dofrange, hd) and all(c.layout.code == tb._lib.TB_LAYOUT_SOA for c in p3["functions"].functions)


def test_a_dictionary_that_names_some_cell_sets_is_solved_on_those_cells(tb):
    g, g2 = cases.build(tb, "quad_3x3_centre")
    m = _models(tb, tb.AlievPanfilovModel(), None, G=None)
    del m["a"]
    m["b"].ion = tb.AlievPanfilovModel()
    p = tb.plan_ep(tb.ReactionDiffusionSplit(m), g2)
    sub = p["grid"]
    assert sub.n_cells == 8 and sub.n_nodes == 16 and p["dh"].ndofs == 16 and p["interfaces"] is None
    assert np.array_equal(sub.xyz, g2.xyz[p["parent_nodes"]]) and np.all(np.diff(p["parent_nodes"]) > 0)
    assert np.array_equal(p["parent_nodes"][sub.conn], g2.conn[g2.getcellset("b")])
    assert np.array_equal(np.sort(p["functions"].heat_dofrange), 2 * np.arange(16) + 1)


def test_refusals(tb):
    g, g2 = cases.build(tb, "quad_3x3_centre")
    S = tb.ReactionDiffusionSplit
    with pytest.raises(ValueError, match="no bulk model claims"):
        tb.plan_ep(S(_models(tb, tb.FHNModel(), None)), g2)
    m = _models(tb, tb.FHNModel(), tb.FHNModel())
    m["interfaces"].ion = tb.FHNModel()
    with pytest.raises(ValueError, match="coupling model .* pointwise reaction part"):
        tb.plan_ep(S(m), g2)
    with pytest.raises(NotImplementedError, match="differ between subdomains"):
        tb.plan_ep(S(_models(tb, tb.FHNModel(), tb.FHNModel(), kappa_a=tb.ConstantCoefficient(np.diag([1e-4, 1e-4])))), g2)
    with pytest.raises(NotImplementedError, match="one rank"):
        tb.plan_ep(S(_models(tb, tb.FHNModel(), tb.FHNModel())), g2, world_size=2)
    with pytest.raises(ValueError, match="share dofs"):                 # no interfaces inserted: the subdomains share their interface nodes
        tb.plan_ep(S(_models(tb, tb.FHNModel(), tb.FHNModel(), G=None)), g)
    with pytest.raises(ValueError, match="needs a grid from insert_interfaces"):
        tb.plan_ep(S(_models(tb, tb.FHNModel(), tb.FHNModel())), g)
    f = tb.PointwiseMultiODEFunction([tb.PointwiseODEFunction(3, tb.FHNModel(), layout=tb.PointBlockedLayout()), tb.PointwiseODEFunction(2, tb.PCG2019())])
    assert tb.solution_size(f) == 3 * 2 + 2 * 7 and f.npoints == 5
    with pytest.raises(NotImplementedError, match="SoA"):               # the single-domain stepper is untouched: StateBlocked only
        tb.LieTrotterGodunov(None, f.functions[0], None)


def test_abi_additions(tb):
    L = tb._lib
    lib = tb.lib()
    assert lib.tb_abi_revision() == 10
    for name in ("tb_interface_form_create", "tb_interface_assemble"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    h = C.c_void_p()
    assert lib.tb_interface_form_create(None, None, None, 0, 0, 1.0, None, 0, C.byref(h)) == L.TB_ERR_BAD_ARG
    assert lib.tb_interface_assemble(None, None, None) == L.TB_ERR_BAD_ARG
    assert b"NULL" in lib.tb_last_error_string()

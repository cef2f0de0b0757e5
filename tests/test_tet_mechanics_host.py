"""Tetrahedral mechanics, host side (no GPU): the generated tetrahedral box, its facet sets, the P2 dof numbering and pattern, the dof-position
helper — and the NumPy reference of tests/tet_reference.py checked against itself (consistency of its tangent, closed forms), so that the GPU
tests compare the device with a yardstick that has been validated on its own."""
import numpy as np
import pytest

import tet_reference as ref

NEL, LEFT, RIGHT = (3, 2, 2), (0.0, 0.0, 0.0), (1.5, 1.0, 0.8)
HO_P = [0.059, 8.023, 18.472, 16.026, 2.581, 11.120, 0.216, 11.436]
GUCCIONE_P = [0.1, 29.8, 14.9, 14.9, 9.3, 19.2, 14.4]


@pytest.fixture(scope="module")
def box(tb):
    return tb.generate_mesh(tb.Tetrahedron, NEL, LEFT, RIGHT)


def unique_edges(conn):
    e = np.sort(conn[:, np.asarray(ref.TET_EDGES)].reshape(-1, 2), axis=1)
    return np.unique(e, axis=0)


def test_generated_tet_box_is_positive_and_conforming(tb, box):
    nx, ny, nz = NEL
    assert box.conn.shape == (6 * nx * ny * nz, 4)
    vol = ref.volumes(box.xyz, box.conn)
    assert (vol > 0).all()
    assert abs(vol.sum() - np.prod(np.asarray(RIGHT) - np.asarray(LEFT))) <= 1e-14
    faces = np.sort(box.conn[:, np.asarray(ref.TET_FACETS)].reshape(-1, 3), axis=1)
    uniq, counts = np.unique(faces, axis=0, return_counts=True)
    assert set(counts.tolist()) <= {1, 2}                      # conforming: no face belongs to three cells, none hangs
    on_boundary = uniq[counts == 1]
    lo, hi = np.asarray(LEFT), np.asarray(RIGHT)
    X = box.xyz[on_boundary]                                    # every once-used face lies in a box face
    flat = [((X[:, :, d] == lo[d]).all(axis=1) | (X[:, :, d] == hi[d]).all(axis=1)) for d in range(3)]
    assert (flat[0] | flat[1] | flat[2]).all()
    # every lattice cell is cut around one main diagonal: its six tetrahedra share two nodes
    for h in range(nx * ny * nz):
        common = set(box.conn[6 * h].tolist())
        for k in range(1, 6):
            common &= set(box.conn[6 * h + k].tolist())
        assert len(common) == 2


def test_named_facet_sets_cover_the_box_faces(tb, box):
    lo, hi = np.asarray(LEFT), np.asarray(RIGHT)
    ext = hi - lo
    total = 0
    for name, axis, val in (("left", 0, lo[0]), ("right", 0, hi[0]), ("front", 1, lo[1]), ("back", 1, hi[1]), ("bottom", 2, lo[2]), ("top", 2, hi[2])):
        fs = box.facetset(name)
        assert fs.dtype == np.int32 and fs.shape[1] == 2 and len(fs) > 0
        nodes = box.conn[fs[:, 0][:, None], np.asarray(ref.TET_FACETS)[fs[:, 1]]]
        X = box.xyz[nodes]
        assert (X[:, :, axis] == val).all()
        nw = np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        area = 0.5 * np.linalg.norm(nw, axis=1)
        assert abs(area.sum() - np.prod(np.delete(ext, axis))) <= 1e-14
        outward = np.zeros(3)
        outward[axis] = -1.0 if val == lo[axis] else 1.0
        assert np.allclose(nw / np.linalg.norm(nw, axis=1)[:, None], outward)       # local facets are listed with outward orientation
        assert len(np.unique(fs, axis=0)) == len(fs)
        total += len(fs)
    nx, ny, nz = NEL
    assert total == 4 * (nx * ny + ny * nz + nx * nz)
    # addfacetset with a predicate finds the same set
    again = box.addfacetset("again", lambda x: x[2] == lo[2])
    assert sorted(map(tuple, again.tolist())) == sorted(map(tuple, box.facetset("bottom").tolist()))


def test_addfacetset_on_a_loaded_tetrahedral_mesh(tb):
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meshes", "mfem", "ref-tetrahedron.mesh")
    g = tb.meshio.load_mfem_grid(path).grid(tb.meshio.TETRAHEDRON)
    fs = g.addfacetset("z0", lambda x: abs(x[2]) < 1e-12)
    assert g.cell_kind == tb.Tetrahedron and len(fs) == 1 and g.facetset("z0") is fs
    nodes = g.conn[fs[0, 0], list(ref.TET_FACETS[fs[0, 1]])]
    assert np.allclose(g.xyz[nodes][:, 2], 0.0)


def test_p2_dofs_pattern_and_positions(tb, box):
    dh = tb.DofHandler(box, tb.LagrangeCollection(2) ** 3)
    assert dh.field_kind == tb._lib.TB_TET10 and dh.cell_dofs.shape == (box.n_cells, 30)
    edges = unique_edges(box.conn)
    assert dh.ndofs == 3 * (box.n_nodes + len(edges))
    cd = dh.cell_dofs
    assert (cd[:, 1::3] == cd[:, 0::3] + 1).all() and (cd[:, 2::3] == cd[:, 0::3] + 2).all() and (cd[:, 0::3] % 3 == 0).all()
    # one triple per mesh entity: the same vertex / edge carries the same dofs from every cell, different entities different dofs
    owner = {}
    for c in range(box.n_cells):
        ents = [("v", int(v)) for v in box.conn[c]] + [("e",) + tuple(sorted((int(box.conn[c, i]), int(box.conn[c, j])))) for i, j in ref.TET_EDGES]
        for a, ent in enumerate(ents):
            assert owner.setdefault(ent, int(cd[c, 3 * a])) == int(cd[c, 3 * a])
    assert len(set(owner.values())) == len(owner) == box.n_nodes + len(edges)
    assert sorted(owner.values()) == list(range(0, dh.ndofs, 3))
    sp = tb.allocate_matrix(dh)
    n = dh.ndofs
    import scipy.sparse as ssp
    A = ssp.csr_matrix((np.ones(sp.nnz), sp.colidx, sp.rowptr), shape=(n, n))
    assert (A != A.T).nnz == 0
    for c in range(box.n_cells):
        assert A[cd[c][:, None], cd[c][None, :]].nnz == 900
    # positions: vertices at vertices, edge dofs at edge midpoints
    X = tb.dof_coordinates(dh)
    assert X.shape == (n, 3)
    for c in range(box.n_cells):
        xc = box.xyz[box.conn[c]]
        for a in range(4):
            assert np.array_equal(X[cd[c, 3 * a: 3 * a + 3]], np.tile(xc[a], (3, 1)))
        for e, (i, j) in enumerate(ref.TET_EDGES):
            assert np.allclose(X[cd[c, 12 + 3 * e: 15 + 3 * e]], 0.5 * (xc[i] + xc[j]), rtol=0, atol=1e-15)
    # the same helper on hexahedra (second order): vertices, edge midpoints, face centres, cell centre of the unit cube
    gh = tb.generate_mesh(tb.Hexahedron, (1, 1, 1), (0, 0, 0), (1, 1, 1))
    dhh = tb.DofHandler(gh, tb.LagrangeCollection(2) ** 3)
    Xh = tb.dof_coordinates(dhh)
    assert sorted(map(tuple, np.round(2 * Xh[dhh.cell_dofs[0, 0::3]]).astype(int).tolist())) == sorted((i, j, k) for i in range(3) for j in range(3) for k in range(3))
    # first order on tetrahedra keeps working, scalar second order is refused
    assert tb.DofHandler(box, tb.LagrangeCollection(1) ** 3).field_kind == tb._lib.TB_TET4
    with pytest.raises(NotImplementedError):
        tb.DofHandler(box, tb.LagrangeCollection(2))


def _mesh(tb, order, nel=(2, 2, 2)):
    g = ref.perturbed_renumbered_box(tb, nel, (0.0, 0.0, 0.0), (1.0, 0.9, 0.6))
    assert (ref.volumes(g.xyz, g.conn) > 0).all()
    dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
    return g, dh, tb.allocate_matrix(dh)


def test_quadrature_rules_of_the_reference_are_exact(tb):
    from math import factorial
    for degree in (2, 3):
        lam, w = ref.tet_rule(degree)
        assert (w > 0).all()
        for a in range(degree + 1):
            for b in range(degree + 1 - a):
                for c in range(degree + 1 - a - b):
                    exact = factorial(a) * factorial(b) * factorial(c) / factorial(a + b + c + 3)
                    assert abs((w * lam[:, 1] ** a * lam[:, 2] ** b * lam[:, 3] ** c).sum() - exact) < 1e-16
    for degree in (2, 4):
        bary, w = ref.tri_rule(degree)
        for a in range(degree + 1):
            for b in range(degree + 1 - a):
                exact = 2.0 * factorial(a) * factorial(b) / factorial(a + b + 2)
                assert abs((w * bary[:, 1] ** a * bary[:, 2] ** b).sum() - exact) < 1e-15


@pytest.mark.parametrize("order", [1, 2])
def test_reference_tangent_is_consistent_and_closed_forms_hold(tb, oracle, order):
    """Checks 2 and 3 of the GPU suite on the NumPy reference alone."""
    g, dh, sp = _mesh(tb, order)
    rng = np.random.default_rng(0)
    u = rng.uniform(-1e-2, 1e-2, dh.ndofs)
    mats = [ref.Material(0, 0, HO_P, [1.0]), ref.Material(8, 0, GUCCIONE_P, [100.0], tension=0.3)]
    X = tb.dof_coordinates(dh)
    for mat in mats:
        nz, r = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u, mat, sp.rowptr, sp.colidx)
        v = rng.uniform(-1.0, 1.0, dh.ndofs)
        h = 1e-6
        rp = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u + h * v, mat)[1]
        rm = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u - h * v, mat)[1]
        Kv = ref.csr_matvec(sp.rowptr, sp.colidx, nz, v)
        assert np.abs(Kv - (rp - rm) / (2 * h)).max() <= 1e-7 * np.abs(Kv).max()
    # HO with a constant frame agrees with the oracle's hand-derived routine (so `energy` id 0 is the right energy)
    F = np.eye(3) + rng.uniform(-0.05, 0.05, (3, 3))
    _, P0, A0 = oracle.energy(0, 0, HO_P, [1.0], F, np.eye(3))
    _, P1, A1 = oracle.ho_energy(F)
    assert np.abs(P0 - P1).max() <= 1e-12 * np.abs(P1).max() and np.abs(A0 - A1).max() <= 1e-12 * np.abs(A1).max()
    mat = mats[0]
    # rigid rotation: zero residual
    th = 0.3
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    urot = np.empty(dh.ndofs)
    disp = X @ (R - np.eye(3)).T
    for c in range(3):
        urot[dh.cell_dofs[:, c::3].ravel()] = disp[dh.cell_dofs[:, c::3].ravel(), c]
    nz, r = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, urot, mat, sp.rowptr, sp.colidx)
    assert np.abs(r).max() <= 1e-12 * ref.assemble.kmax * np.abs(urot).max()
    # affine stretch: zero residual at interior dofs (patch test)
    G = np.array([[0.02, 0.01, 0.0], [0.0, -0.015, 0.005], [0.01, 0.0, 0.03]])
    ua = np.empty(dh.ndofs)
    disp = X @ G.T
    for c in range(3):
        ua[dh.cell_dofs[:, c::3].ravel()] = disp[dh.cell_dofs[:, c::3].ravel(), c]
    nz, r = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, ua, mat, sp.rowptr, sp.colidx)
    interior = interior_dofs(g, dh)
    assert len(interior) > 0
    assert np.abs(r[interior]).max() <= 1e-12 * ref.assemble.kmax * np.abs(ua).max()


def interior_dofs(g, dh):
    """dofs of the field nodes that lie on no boundary facet"""
    faces = np.sort(g.conn[:, np.asarray(ref.TET_FACETS)], axis=2)
    flat = faces.reshape(-1, 3)
    _, inv, cnt = np.unique(flat, axis=0, return_inverse=True, return_counts=True)
    once = (cnt[inv.ravel()] == 1).reshape(g.n_cells, 4)
    nb = dh.cell_dofs.shape[1] // 3
    on = np.zeros(dh.ndofs, dtype=bool)
    for c, lf in zip(*np.nonzero(once)):
        fv = ref.TET_FACETS[lf]
        local = list(fv)
        if nb == 10:
            local += [4 + e for e, (i, j) in enumerate(ref.TET_EDGES) if i in fv and j in fv]
        for a in local:
            on[dh.cell_dofs[c, 3 * a: 3 * a + 3]] = True
    return np.flatnonzero(~on)


@pytest.mark.parametrize("order", [1, 2])
def test_reference_facet_terms(tb, order):
    g = tb.generate_mesh(tb.Tetrahedron, (2, 2, 1), (0.0, 0.0, 0.0), (1.0, 0.9, 0.6))
    dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
    sp = tb.allocate_matrix(dh)
    fs = g.facetset("top")
    p = 0.7
    _, r = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, np.zeros(dh.ndofs), "pressure", p)
    tot = np.array([r[c::3].sum() for c in range(3)])
    assert np.allclose(tot, p * 0.9 * np.array([0.0, 0.0, 1.0]), rtol=0, atol=1e-14)
    # one facet: vertex / mid-edge shares
    c, lf = fs[0]
    X = g.xyz[g.conn[c]]
    fv = ref.TET_FACETS[lf]
    Af = 0.5 * np.linalg.norm(np.cross(X[fv[1]] - X[fv[0]], X[fv[2]] - X[fv[0]]))
    _, re = ref.facet_element(order, X, int(lf), np.zeros(3 * (4 if order == 1 else 10)), "pressure", p)
    rz = re[2::3]
    if order == 1:
        assert np.allclose(rz[list(fv)], p * Af / 3.0, atol=1e-15)
    else:
        assert np.allclose(rz[list(fv)], 0.0, atol=1e-15)
        mids = [4 + e for e, (i, j) in enumerate(ref.TET_EDGES) if i in fv and j in fv]
        assert np.allclose(rz[mids], p * Af / 3.0, atol=1e-15)
    # pressure tangent against the central difference of the facet residual; Robin / spring: r = K u exactly
    rng = np.random.default_rng(0)
    u = rng.uniform(-1e-2, 1e-2, dh.ndofs)
    v = rng.uniform(-1.0, 1.0, dh.ndofs)
    nz, _ = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, u, "pressure", p, sp.rowptr, sp.colidx)
    h = 1e-6
    rp = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, u + h * v, "pressure", p)[1]
    rm = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, u - h * v, "pressure", p)[1]
    Kv = ref.csr_matvec(sp.rowptr, sp.colidx, nz, v)
    assert np.abs(Kv - (rp - rm) / (2 * h)).max() <= 1e-8 * np.abs(Kv).max()
    for bc in ("robin", "spring"):
        nz, r = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, u, bc, 3.0, sp.rowptr, sp.colidx)
        Ku = ref.csr_matvec(sp.rowptr, sp.colidx, nz, u)
        assert np.abs(r - Ku).max() <= 1e-12 * np.abs(Ku).max()

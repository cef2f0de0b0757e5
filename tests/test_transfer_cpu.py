"""Nodal inter-grid interpolation, the parts that need no device: the NumPy reference itself (tests/transfer_reference.py), the dof set of
NodalIntergridInterpolation (transfer_operators.jl:69-89) and the three places that state the ABI revision."""
import os
import re

import numpy as np
import pytest

import transfer_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def linear(x):
    return 0.3 * x[:, 0] - 1.1 * x[:, 1] + 0.7 * x[:, 2] + 0.25


@pytest.fixture(scope="module")
def meshes(tb):
    hexes = tb.generate_mesh(tb.Hexahedron, (5, 4, 3), (0, 0, 0), (1, 1, 1), perturb=0.2)
    tets = tb.generate_mesh(tb.Tetrahedron, (3, 3, 2), (0.1, 0.1, 0.1), (0.9, 0.9, 0.9))
    quads = tb.generate_mesh(tb.Quadrilateral, (7, 5))
    return hexes, tets, quads


def test_reference_finds_its_own_vertices(tb, meshes):
    for g in meshes:
        cells, xi = R.locate(g, g.xyz)
        assert (cells >= 0).all()
        assert np.abs(R.position(g, cells, xi) - g.xyz).max() <= 1e-14
        # the lowest-numbered cell that has the vertex
        lowest = np.full(g.n_nodes, g.n_cells)
        np.minimum.at(lowest, g.conn.ravel(), np.repeat(np.arange(g.n_cells), g.conn.shape[1]))
        assert (cells == lowest).all()


@pytest.mark.parametrize("order,ncomp", [(1, 1), (2, 1), (2, 3)])
def test_reference_reproduces_linear_fields_hex(tb, meshes, order, ncomp):
    hexes, tets, _ = meshes
    dh = tb.DofHandler(hexes, tb.LagrangeCollection(order) ** ncomp if ncomp > 1 else tb.LagrangeCollection(order))
    X = tb.dof_coordinates(dh)
    u = linear(X)
    cells, xi = R.locate(hexes, tets.xyz)
    assert (cells >= 0).all()
    got = R.evaluate(dh, u, cells, xi)
    assert np.abs(got - linear(tets.xyz)[:, None]).max() <= 1e-13


@pytest.mark.parametrize("order,ncomp", [(1, 1), (1, 3), (2, 3)])
def test_reference_reproduces_linear_fields_tet(tb, meshes, order, ncomp):
    hexes, tets, _ = meshes
    dh = tb.DofHandler(tets, tb.LagrangeCollection(order) ** ncomp if ncomp > 1 else tb.LagrangeCollection(order))
    u = linear(tb.dof_coordinates(dh))
    pts = np.random.default_rng(1).uniform(0.1, 0.9, (50, 3))
    cells, xi = R.locate(tets, pts)
    assert (cells >= 0).all()
    assert np.abs(R.evaluate(dh, u, cells, xi) - linear(pts)[:, None]).max() <= 1e-13


def test_reference_points_outside_are_missing(tb, meshes):
    hexes = meshes[0]
    cells, _ = R.locate(hexes, np.array([[-0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 1.5, 0.5]]))
    assert cells[0] == -1 and cells[1] >= 0 and cells[2] == -1


def test_node_to_dof_map_with_and_without_a_cell_set(tb, meshes):
    """host part only: no device is touched"""
    hexes, tets, _ = meshes
    for dh in (tb.DofHandler(tets), tb.DofHandler(hexes, tb.LagrangeCollection(2)), tb.DofHandler(hexes, tb.LagrangeCollection(2) ** 3),
               tb.DofHandler(tets, tb.LagrangeCollection(2) ** 3)):
        g = dh.grid
        X = tb.dof_coordinates(dh)
        n2d, nodes = tb.intergrid_dofs(dh)
        assert (n2d == np.arange(dh.ndofs)).all()                    # every dof, sorted
        assert len(nodes) * dh.ip.ncomp == len(n2d) and (nodes == X[n2d[::dh.ip.ncomp]]).all()
        half = np.arange(g.n_cells // 2, dtype=np.int32)
        g.addcellset("half", half)
        for sub in (half, "half"):
            n2d, nodes = tb.intergrid_dofs(dh, sub)
            assert (n2d == np.unique(dh.cell_dofs[half])).all()      # sort(unique(dofs of the cells))
            assert len(n2d) < dh.ndofs
            assert (nodes == X[n2d[::dh.ip.ncomp]]).all()
            if dh.ip.ncomp == 3:                                     # the components of a node travel together
                assert (X[n2d[0::3]] == X[n2d[1::3]]).all() and (X[n2d[0::3]] == X[n2d[2::3]]).all()


def test_component_counts_must_agree(tb, meshes):
    hexes, tets, _ = meshes
    with pytest.raises(ValueError):
        tb.NodalIntergridInterpolation(None, tb.DofHandler(hexes), tb.DofHandler(tets, tb.LagrangeCollection(1) ** 3))


def test_abi_revision_is_10_everywhere(tb):
    header = open(os.path.join(ROOT, "include", "tbhip.h"), encoding="utf-8").read()
    julia = open(os.path.join(ROOT, "julia", "ThunderboltHIPBackend.jl"), encoding="utf-8").read()
    assert int(re.search(r"#define\s+TB_ABI_REVISION\s+(\d+)", header).group(1)) == 10
    assert int(re.search(r"const\s+TB_ABI_REVISION\s*=\s*(\d+)", julia).group(1)) == 10
    assert tb._lib.TB_ABI_REVISION == 10
    assert tb.lib().tb_abi_revision() == 10
    assert re.search(r"\b10: tb_locator_", header), "the revision history names what revision 10 added"
    for name in ("tb_locator_create", "tb_locator_relocate", "tb_locator_destroy", "tb_locator_npoints", "tb_locator_nmissing", "tb_locator_cells_device",
                 "tb_locator_xi_device", "tb_locator_evaluate"):
        assert name in tb._lib.SIGNATURES and name in julia, name

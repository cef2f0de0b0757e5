"""The meshes of the multi-domain tests (tests/test_multidomain_cpu.py, tests/test_multidomain_gpu.py): name → (grid with cell sets "a" and "b",
the grid after insert_interfaces(grid, ["a", "b"]))."""
import numpy as np


def _sets(g, a):
    a = np.asarray(a, dtype=np.int64)
    g.addcellset("a", a)
    g.addcellset("b", np.setdiff1d(np.arange(g.n_cells), a))
    return g


def build(tb, name):
    Q, H = tb.Quadrilateral, tb.Hexahedron
    if name == "quad_2x1":                      # one interface edge
        g = _sets(tb.generate_mesh(Q, (2, 1), (0, 0), (2, 1)), [0])
    elif name == "hex_2x1x1":                   # one interface face
        g = _sets(tb.generate_mesh(H, (2, 1, 1), (0, 0, 0), (2, 1, 1)), [0])
    elif name == "quad_3x3_centre":             # all four edge orientations, corner nodes shared by two interface edges
        g = _sets(tb.generate_mesh(Q, (3, 3), (0, 0), (3, 2)), [4])
    elif name == "hex_4x4x4_inner":             # all six local facets, nodes shared by three interface facets
        g = tb.generate_mesh(H, (4, 4, 4), (0, 0, 0), (4, 3, 2))
        c = np.arange(64).reshape(4, 4, 4)
        g = _sets(g, c[1:3, 1:3, 1:3].ravel())
    elif name == "quad_split_to_boundary":      # the interface reaches the boundary; b lies left of a (b's cells come first)
        g = tb.generate_mesh(Q, (4, 3), (0, 0), (2, 1))
        g = _sets(g, np.flatnonzero(g.xyz[g.conn].mean(axis=1)[:, 0] > 1.0))
    elif name == "hex_3x2x2_perturbed":         # non-planar facets, split by a lattice plane that reaches the boundary
        g = tb.generate_mesh(H, (3, 2, 2), (0, 0, 0), (1, 1, 1), perturb=0.2)
        g = _sets(g, np.flatnonzero(np.arange(12) % 3 == 0))
    elif name == "quad_no_touch":               # cells 1 and 2 lie between the sets
        g = tb.generate_mesh(Q, (4, 1), (0, 0), (4, 1))
        g.addcellset("a", np.array([0]))
        g.addcellset("b", np.array([3]))
    elif name == "quad_6x6":
        g = tb.generate_mesh(Q, (6, 6), (0, 0), (3, 2))
        c = np.arange(36).reshape(6, 6)
        g = _sets(g, c[2:4, 1:5].ravel())
    else:
        raise KeyError(name)
    if g.cell_kind == H:
        g.addfacetset("low", lambda x: x[2] == 0.0)
    return g, tb.insert_interfaces(g, ["a", "b"])


MESHES = ["quad_2x1", "hex_2x1x1", "quad_3x3_centre", "hex_4x4x4_inner", "quad_split_to_boundary", "quad_no_touch"]

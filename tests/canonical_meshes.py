"""Meshes of the canonical-scatter tests (test infrastructure): one lattice under the numberings that decide whether the record kernel's CANON
instance applies.  A patch is canonical when every row it owns has 27 entries with the column of vertex j at 13 + Δx + 3Δy + 9Δz of the row of
vertex i (plan::classify_records) — interior patches of a lattice whose dofs ascend lexicographically, under whatever numbering gives that order."""
import numpy as np

BOX = (16, 16, 19)     # with the pair plan's 5×5×6 node tiles: interior patches and patches on every face, edge and corner
SMALL = (4, 4, 4)      # one tile: no interior patch
SEED = 31
# The tile of the flagship's pair plan, fixed (TB_PATCH_TILE for the library, Options::tile for the planners): left to itself the fit gives a box of
# fewer than ≈ 30³ cells bisection leaves instead (poorly filled tiles), whose cuts depend on the order the cells are stored in.
TILE = "5,5,6"

# name -> the planner's verdict: True = some patches canonical (and some general), False = none
EXPECT_CANONICAL = {"box": True, "small": False, "shuffled": False, "relocalised": True, "reversed": False}


def _box(tb, nel):
    return tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1.0, 1.0, 1.0), perturb=0.2)


def _lattice_index(tb, nel):
    """(n_nodes, 3) integer lattice coordinates of the box's nodes, from the unperturbed mesh of the same numbering"""
    g0 = tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1.0, 1.0, 1.0), perturb=0.0)
    return np.rint(g0.xyz * np.asarray(nel, dtype=np.float64)).astype(np.int64)


def build(tb):
    """name -> DofHandler"""
    out = {}
    g = _box(tb, BOX)
    out["box"] = tb.DofHandler(g)
    out["small"] = tb.DofHandler(_box(tb, SMALL))
    # cells and nodes renumbered at random: rows are as long as before, their columns in no order the lattice knows
    rng = np.random.default_rng(SEED)
    pn, pc = rng.permutation(g.n_nodes), rng.permutation(g.n_cells)
    inv = np.empty_like(pn)
    inv[pn] = np.arange(g.n_nodes)
    gs = tb.Grid(tb.Hexahedron, np.ascontiguousarray(g.xyz[pn]), np.ascontiguousarray(inv[g.conn[pc]]).astype(np.int32))
    dhs = tb.DofHandler(gs)
    out["shuffled"] = dhs
    # the same shuffled grid with its dofs renamed by the locality permutation: the lexicographic order is back, cells and nodes stay shuffled
    _, _, dof_perm = tb.locality_permutation(gs, dhs)
    out["relocalised"] = tb.renumber_dofs(dhs, dof_perm)
    # dofs numbered lexicographically with the x axis reversed: every interior row is full, but its columns run the other way in x
    dh = out["box"]
    ijk = _lattice_index(tb, BOX)
    node_of_dof = np.empty(dh.ndofs, dtype=np.int64)
    node_of_dof[dh.cell_dofs.ravel()] = g.conn.ravel()
    i, j, k = ijk[node_of_dof].T
    nx, ny = BOX[0] + 1, BOX[1] + 1
    out["reversed"] = tb.renumber_dofs(dh, ((nx - 1 - i) + nx * (j + ny * k)).astype(np.int32))
    return out

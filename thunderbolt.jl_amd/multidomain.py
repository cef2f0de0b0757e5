"""Multi-domain electrophysiology: one ionic model per subdomain, subdomains coupled by diffusion across zero-thickness interface elements.

  reference (file:line)                                                        here
  --------------------------------------------------------------------------------------------------------------------
  insert_interfaces (FerriteInterfaceElements, third party)                      insert_interfaces(grid, [name_a, name_b])
  MonodomainModel / ReactionDiffusionSplit  src/modeling/electrophysiology.jl:338-379   MonodomainModel, ReactionDiffusionSplit
  InterfaceDiffusionModel / BilinearInterfaceDiffusionIntegrator  core/diffusion.jl:76-157   InterfaceDiffusionModel, InterfaceDiffusionForm
  semidiscretize(::ReactionDiffusionSplit{<:Dict})  src/discretization/fem.jl:434-542     semidiscretize_ep(split, strategy, grid)
  PointwiseMultiODEFunction                 src/modeling/functions.jl:68-77               PointwiseMultiODEFunction(functions)
  LieTrotterGodunov on the GenericSplitFunction                                          MultiDomainLieTrotterGodunov(heat_stage, multi_fun, caches)

FerriteInterfaceElements is not part of the reference tree, so the conventions below are this package's own (tests/multidomain_reference.py
restates them independently):

  * insert_interfaces duplicates every node of a facet shared by a cell of `a` and a cell of `b`.  Cells of `a` (and cells of neither set) keep the
    old node; EVERY cell of `b` that references such a node gets the copy, also where it touches the interface at an edge or a vertex only.  Copies
    are appended after the existing nodes, in ascending order of the node they copy, with identical coordinates.
  * one record per shared facet, (cell_a, local_facet_a, cell_b, local_facet_b), 0-based, ascending (cell_a, local_facet_a); local facets as
    Ferrite.reference_facets — hexahedra: Grid.HEX_FACETS, quadrilaterals: QUAD_FACETS below, the four edges (0,1), (1,2), (2,3), (3,0).
  * pairing[r, k]: the local vertex of cell_b that is the copy of the k-th node of a's facet in Ferrite's facet-node order.
  * the dofs of an interface element: a's facet dofs in that order, then their copies on b in the same order (2·nf = dofs of a cell of the mesh).
  * the packed state: one block per bulk model in the dictionary's order; a block's points are the subdomain's dofs in ascending order; children
    are PointBlocked (fem.jl:499-510) unless a layout is given for all of them; heat_dofrange[dof] is the position of that dof's φₘ in the packed
    state (0-based).  Unlike the reference, a subdomain's dofs need not be contiguous: the map is a general index vector.
  * G is used as given (the reference hands model.G to the integrator without the κ/(Cₘχ) wrap of the bulk term).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import check, lib
from . import api
from .api import (Grid, Hexahedron, Quadrilateral, DofHandler, allocate_matrix, ConstantCoefficient, ConductivityToDiffusivityCoefficient,
                  BilinearMassIntegrator, BilinearDiffusionIntegrator, setup_operator, update_operators, BackwardEulerStage, BackwardEulerSolver,
                  DeviceVector, PointwiseODEFunction, PointwiseSolverCache, PointBlockedLayout, perform_step,
                  perform_step_with_reaction_tangent, get_reaction_tangent, dof_coordinates)

# Ferrite.reference_facets(RefQuadrilateral), 0-based vertex ids, in Ferrite's facet order (Grid.reference_facets stays three-dimensional)
QUAD_FACETS = ((0, 1), (1, 2), (2, 3), (3, 0))


def _facets_of(cell_kind):
    if cell_kind == Hexahedron:
        return np.asarray(Grid.HEX_FACETS)
    if cell_kind == Quadrilateral:
        return np.asarray(QUAD_FACETS)
    raise NotImplementedError("interfaces: first-order Quadrilateral and Hexahedron grids only (tetrahedra and mixed-dimensional meshes are not implemented)")


# --------------------------------------------------------------------------------------- mesh
class InterfaceRecords:
    """`grid.interfaces`: records (n, 4) = (cell_a, local_facet_a, cell_b, local_facet_b) and pairing (n, nf), 0-based Int32 (module docstring)."""

    def __init__(self, records, pairing, names, nf):
        self.records = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, 4)
        self.pairing = np.ascontiguousarray(pairing, dtype=np.int32).reshape(-1, nf)
        self.names, self.nf = tuple(names), int(nf)

    def __len__(self):
        return self.records.shape[0]


def _copy_grid(grid, xyz, conn):
    g = Grid(grid.cell_kind, xyz, conn, dims=grid.dims)
    if hasattr(grid, "cellsets"):
        g.cellsets = {k: v.copy() for k, v in grid.cellsets.items()}
    if getattr(grid, "facetsets", None) is not None:
        g.facetsets = {k: v.copy() for k, v in grid.facetsets.items()}
    if hasattr(grid, "nodesets"):
        g.nodesets = {k: np.asarray(v).copy() for k, v in grid.nodesets.items()}
    return g


def insert_interfaces(grid, names):
    """insert_interfaces(grid, [name_a, name_b]): the grid with the nodes of the facets shared by the two cell sets duplicated, and `interfaces`,
    one record per shared facet (conventions: module docstring).  Two sets without a shared facet give an equal grid with zero records."""
    facets = _facets_of(grid.cell_kind)
    if getattr(grid, "interfaces", None) is not None:
        raise NotImplementedError("insert_interfaces: one interface insertion per grid (the reference carries the same FIXME)")
    if len(names) != 2:
        raise NotImplementedError("insert_interfaces: exactly two cell sets")
    a, b = (np.asarray(grid.getcellset(n), dtype=np.int64) for n in names)
    if np.intersect1d(a, b).size:
        raise ValueError("insert_interfaces: cell sets %r and %r are not disjoint" % tuple(names))
    nf = facets.shape[1]
    conn = grid.conn
    # only nodes that sit in a cell of both sets can lie on a shared facet: the facet search runs on those
    in_a, in_b = np.zeros(grid.n_nodes, dtype=bool), np.zeros(grid.n_nodes, dtype=bool)
    in_a[conn[a]] = True
    in_b[conn[b]] = True
    cand = in_a & in_b

    def candidate_facets(cells):
        fn = conn[cells][:, facets]                                  # (cells, facets, nf)
        ci, fi = np.nonzero(cand[fn].all(axis=2))
        return cells[ci], fi, fn[ci, fi]

    ca, fa, na = candidate_facets(a)
    cb, fb, nb = candidate_facets(b)
    of_b = {tuple(sorted(n.tolist())): (int(c), int(f)) for c, f, n in zip(cb, fb, nb)}
    records, pairing = [], []
    for c, f, n in sorted(zip(ca.tolist(), fa.tolist(), na.tolist())):
        hit = of_b.get(tuple(sorted(n)))
        if hit is None:
            continue
        cb_, fb_ = hit
        local_b = {int(v): k for k, v in enumerate(conn[cb_])}
        records.append((c, f, cb_, fb_))
        pairing.append([local_b[v] for v in n])
    rec = np.array(records, dtype=np.int32).reshape(-1, 4)
    if len(rec) == 0:
        g = _copy_grid(grid, grid.xyz.copy(), conn.copy())
        g.interfaces = InterfaceRecords(rec, np.zeros((0, nf), dtype=np.int32), names, nf)
        return g
    shared = np.unique(conn[rec[:, 0][:, None], facets[rec[:, 1]]])  # ascending old node ids
    remap = np.arange(grid.n_nodes, dtype=np.int64)
    remap[shared] = grid.n_nodes + np.arange(len(shared))
    new_conn = conn.copy()
    new_conn[b] = remap[conn[b]]
    g = _copy_grid(grid, np.vstack([grid.xyz, grid.xyz[shared]]), new_conn)
    g.interfaces = InterfaceRecords(rec, np.array(pairing, dtype=np.int32), names, nf)
    return g


def interface_dofs(dh, interfaces):
    """(n, 2·nf) dofs of the interface elements of a first-order scalar field: a's facet dofs in Ferrite's facet-node order, then their copies on b."""
    if dh.ip.order != 1 or dh.ip.ncomp != 1:
        raise NotImplementedError("interfaces: first-order scalar fields only")
    facets = _facets_of(dh.grid.cell_kind)
    r, p = interfaces.records, interfaces.pairing
    da = dh.cell_dofs[r[:, 0][:, None], facets[r[:, 1]]]
    db = dh.cell_dofs[r[:, 2][:, None], p]
    return np.ascontiguousarray(np.hstack([da, db]), dtype=np.int32)


def extract_subgrid(grid, cells):
    """The grid of `cells` alone (ascending), nodes renumbered in ascending order of their old ids; cell sets, facet sets and interface records are
    carried over where they lie inside.  Returns (subgrid, old node id of every new node)."""
    cells = np.unique(np.asarray(cells, dtype=np.int64))
    nodes = np.unique(grid.conn[cells])
    new_node = np.full(grid.n_nodes, -1, dtype=np.int64)
    new_node[nodes] = np.arange(len(nodes))
    new_cell = np.full(grid.n_cells, -1, dtype=np.int64)
    new_cell[cells] = np.arange(len(cells))
    g = Grid(grid.cell_kind, grid.xyz[nodes], new_node[grid.conn[cells]].astype(np.int32), dims=None)
    g.cellsets = {k: new_cell[v][new_cell[v] >= 0].astype(np.int32) for k, v in getattr(grid, "cellsets", {}).items()}
    if getattr(grid, "facetsets", None):
        g.facetsets = {}
        for k, v in grid.facetsets.items():
            keep = new_cell[v[:, 0]] >= 0
            g.facetsets[k] = np.stack([new_cell[v[keep, 0]], v[keep, 1]], axis=1).astype(np.int32).reshape(-1, 2)
    it = getattr(grid, "interfaces", None)
    if it is not None:
        keep = (new_cell[it.records[:, 0]] >= 0) & (new_cell[it.records[:, 2]] >= 0)
        rec = it.records[keep].copy()
        rec[:, 0], rec[:, 2] = new_cell[rec[:, 0]], new_cell[rec[:, 2]]
        g.interfaces = InterfaceRecords(rec, it.pairing[keep], it.names, it.nf)
    return g, nodes


# --------------------------------------------------------------------------------------- models
class NoStimulationProtocol:
    """NoStimulationProtocol() (src/modeling/electrophysiology.jl)."""


class MonodomainModel:
    """MonodomainModel(χ, Cₘ, κ, stim, ion, φsym, ssym) (src/modeling/electrophysiology.jl:338-362).  `cell_coordinates="cartesian"` hands every point
    of the subdomain its position (the child's `x`); None: the cell model ignores its coordinate.  `ion=None`: no pointwise reaction part."""

    def __init__(self, chi, Cm, kappa, stim, ion, phi_symbol, state_symbol, cell_coordinates=None):
        self.chi, self.Cm, self.kappa, self.stim, self.ion = chi, Cm, kappa, stim, ion
        self.transmembrane_solution_symbol, self.internal_state_symbol = phi_symbol, state_symbol
        self.cell_coordinates = cell_coordinates


class InterfaceDiffusionModel:
    """InterfaceDiffusionModel(G, φsym, interface_symbol) (src/modeling/core/diffusion.jl:143-157): ∫ [[δu]] G [[u]] dΓ over the interface elements.
    G: a number, ConstantCoefficient, or one value per interface record.  A coupling model: it owns no block of the state."""
    is_coupling_model = True

    def __init__(self, G, phi_symbol, interface_symbol, ion=None):
        self.G, self.solution_variable_symbol, self.interface_interpolation_symbol = G, phi_symbol, interface_symbol
        self.ion = ion   # a reaction part on a coupling model is refused by semidiscretize_ep (fem.jl:458-466)


class ReactionDiffusionSplit:
    """ReactionDiffusionSplit(models): models a dictionary cell set → MonodomainModel / InterfaceDiffusionModel (electrophysiology.jl:370-381)."""

    def __init__(self, models):
        self.model = models


def _value(c):
    return np.asarray(c.val if isinstance(c, ConstantCoefficient) else c, dtype=np.float64)


class InterfaceDiffusionForm:
    """The device form of the interface term (tb_interface_form_create); `assemble(pattern, nz)` ADDS it to a value array of the widened pattern."""

    def __init__(self, dmesh, interfaces, G=1.0, facet_qpoints=0):
        self.dmesh, self.interfaces = dmesh, interfaces
        g = _value(G)
        n = len(interfaces)
        per = None
        if g.ndim:
            if g.shape != (n,):
                raise ValueError("interface conductance: one value, or one per interface record (%d), got shape %r" % (n, g.shape))
            per = np.ascontiguousarray(g, dtype=np.float64)
        self.h = C.c_void_p()
        check(lib().tb_interface_form_create(dmesh.h, interfaces.records.ctypes.data_as(L.c_i32p), interfaces.pairing.ctypes.data_as(L.c_i32p), n,
                                             int(facet_qpoints), float(g) if per is None else 0.0, None if per is None else per.ctypes.data_as(L.c_dp),
                                             0, C.byref(self.h)))

    def assemble(self, pattern, nz):
        check(lib().tb_interface_assemble(self.h, pattern.h, api._ptr(nz)))

    def __del__(self):
        try:
            if self.h:
                lib().tb_form_destroy(self.h)
        except Exception:
            pass


# --------------------------------------------------------------------------------------- pointwise part
class PointwiseMultiODEFunction:
    """PointwiseMultiODEFunction(functions) (src/modeling/functions.jl:68-77): children packed one after the other, solution_size = the sum over the
    children.  `layout`: set for all children at once (default: each child's own — PointBlocked as semidiscretize_ep builds them)."""

    def __init__(self, functions, layout=None, heat_dofrange=None):
        self.functions = list(functions)
        if layout is not None:
            for f in self.functions:
                f.layout = layout
        self.offsets = np.concatenate([[0], np.cumsum([f.npoints * f.ode.nstates for f in self.functions])]).astype(np.int64)
        self.heat_dofrange = heat_dofrange

    @property
    def npoints(self):
        return int(sum(f.npoints for f in self.functions))

    @property
    def solution_size(self):
        return int(self.offsets[-1])

    def setup_solver_cache(self, solver, u=None, keep_du=True):
        return MultiSolverCache(self, solver, u=u, keep_du=keep_du)


class MultiSolverCache:
    """One PointwiseSolverCache per child, each on its view of the packed state `u`.  `solver`: one cell solver for all children, or one per child
    (a Rush–Larsen step beside a forward-Euler one: not every ionic model has a gate decomposition)."""

    def __init__(self, f, solver, u=None, keep_du=True):
        solvers = list(solver) if isinstance(solver, (list, tuple)) else [solver] * len(f.functions)
        if len(solvers) != len(f.functions):
            raise ValueError("%d cell solvers for %d children" % (len(solvers), len(f.functions)))
        self.solver = solver
        self.u = u if u is not None else solvers[0].device.zeros(f.solution_size)
        if self.u.n != f.solution_size:
            raise ValueError("packed state has %d entries, the children need %d" % (self.u.n, f.solution_size))
        self.children = [PointwiseSolverCache(c, s, u=self.u.view(int(o), c.npoints * c.ode.nstates), keep_du=keep_du)
                         for c, s, o in zip(f.functions, solvers, f.offsets[:-1])]

    @property
    def un(self):
        return self.u


def heat_dofrange_of(subdofs_per_child, nstates, phi_index, ndofs, layout_code=L.TB_LAYOUT_AOS):
    """heat_dofrange (0-based) and block offsets of the packed state: fem.jl:478-522 with StateBlock / state_range spelled out.  −1: unclaimed."""
    hd = np.full(ndofs, -1, dtype=np.int64)
    offsets, off = [], 0
    for dofs, ns, pi in zip(subdofs_per_child, nstates, phi_index):
        npts = len(dofs)
        k = np.arange(npts)
        hd[dofs] = off + (k * ns + pi if layout_code == L.TB_LAYOUT_AOS else pi * npts + k)
        offsets.append(off)
        off += npts * ns
    return hd, offsets, off


class MultiDomainFunction:
    """What semidiscretize_ep returns (the GenericSplitFunction of fem.jl:535-541): the heat function's pieces (dh, widened pattern, M, K with the
    interface term added) and the PointwiseMultiODEFunction with `heat_dofrange`."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def solution_size(self):
        return self.functions.solution_size

    def heat_stage(self, solver=None):
        return MultiDomainHeatStage(solver or BackwardEulerSolver(), self)

    def initial_condition(self, phi0=None):
        """Packed host state: every point at its model's default_initial_state, φₘ = phi0(x) where given (x: the dof's position)."""
        u = np.zeros(self.solution_size)
        x = dof_coordinates(self.dh)
        for f, o, dofs in zip(self.functions.functions, self.functions.offsets[:-1], self.subdofs):
            ns, n = f.ode.nstates, f.npoints
            blk = np.tile(f.ode.default_initial_state(), (n, 1))
            if phi0 is not None:
                blk[:, f.ode.phi_index] = [phi0(p) for p in x[dofs]]
            u[o:o + n * ns] = blk.ravel() if f.layout.code == L.TB_LAYOUT_AOS else blk.T.ravel()
        return u


def plan_ep(split, grid, layout=None, world_size=1):
    """The host half of semidiscretize_ep, no device: checks, the sub-grid, the DofHandler of φₘ, the children and heat_dofrange.  Returns a dict."""
    if world_size != 1:
        raise NotImplementedError("multi-domain electrophysiology runs on one rank")
    models = split.model
    for name, m in models.items():
        if getattr(m, "is_coupling_model", False) and getattr(m, "ion", None) is not None:
            raise ValueError("coupling model on %r carries a pointwise reaction part, which is not supported: a coupling model does not own a block "
                             "of the solution vector, so its reaction state has nowhere to live" % name)
    bulk = [(n, m) for n, m in models.items() if not getattr(m, "is_coupling_model", False)]
    coupling = [(n, m) for n, m in models.items() if getattr(m, "is_coupling_model", False)]
    if not bulk:
        raise ValueError("semidiscretize_ep: no bulk model")
    if len(coupling) > 1:
        raise NotImplementedError("one interface model per problem (one interface insertion per grid)")
    syms = {m.transmembrane_solution_symbol for _, m in bulk if m.ion is not None}
    if len(syms) != 1:
        raise ValueError("all EP models in a domain split must share the same transmembrane potential symbol, got %r" % (syms,))
    for _, m in bulk:
        if not isinstance(m.stim, NoStimulationProtocol) and m.stim is not None:
            raise NotImplementedError("multi-domain problems: NoStimulationProtocol only")
    first = bulk[0][1]
    for name, m in bulk[1:]:
        if not all(np.array_equal(_value(getattr(m, k)), _value(getattr(first, k))) for k in ("kappa", "Cm", "chi")):
            raise NotImplementedError("subdomain %r: κ, Cₘ or χ differ between subdomains — scalar forms have no cell sets" % name)
    for name, _ in bulk:
        if name not in getattr(grid, "cellsets", {}):
            raise KeyError("semidiscretize_ep: the grid has no cell set %r" % name)
    claimed = np.unique(np.concatenate([np.asarray(grid.getcellset(n), dtype=np.int64) for n, _ in bulk]))
    if sum(len(grid.getcellset(n)) for n, _ in bulk) != len(claimed):
        raise ValueError("semidiscretize_ep: the cell sets of the bulk models are not disjoint")
    nodes = None
    if len(claimed) != grid.n_cells:
        grid, nodes = extract_subgrid(grid, claimed)
    interfaces = getattr(grid, "interfaces", None)
    if coupling:
        if interfaces is None:
            raise ValueError("an InterfaceDiffusionModel needs a grid from insert_interfaces")
    else:
        interfaces = None
    dh = DofHandler(grid)
    lay = layout or PointBlockedLayout()
    children, subdofs = [], []
    xall = None
    for name, m in bulk:
        if m.ion is None:
            continue
        dofs = np.unique(dh.cell_dofs[np.asarray(grid.getcellset(name), dtype=np.int64)])
        x = None
        if m.cell_coordinates is not None:
            xall = dof_coordinates(dh) if xall is None else xall
            x = xall[dofs][:, :2 if grid.cell_kind == Quadrilateral else 3]
        children.append(PointwiseODEFunction(len(dofs), m.ion, x, layout=lay))
        subdofs.append(dofs)
    hd, offsets, total = heat_dofrange_of(subdofs, [c.ode.nstates for c in children], [c.ode.phi_index for c in children], dh.ndofs, lay.code)
    if subdofs and sum(len(d) for d in subdofs) != len(np.unique(np.concatenate(subdofs))):
        raise ValueError("subdomains share dofs of the transmembrane potential: insert_interfaces(grid, [a, b]) separates them")
    if (hd < 0).any():
        raise ValueError("the transmembrane potential field carries dofs that no bulk model claims, so the heat problem would read uninitialised "
                         "state: every dof has to lie on a subdomain with a pointwise reaction part")
    if total >= 2 ** 31:
        raise NotImplementedError("packed state of %d entries: the index vector is Int32" % total)
    fun = PointwiseMultiODEFunction(children, heat_dofrange=hd.astype(np.int32))
    return dict(grid=grid, dh=dh, interfaces=interfaces, functions=fun, subdofs=subdofs, parent_nodes=nodes, first=first,
                G=coupling[0][1].G if coupling else None)


def semidiscretize_ep(split, strategy, grid, layout=None, facet_qpoints=0, world_size=1, t0=0.0):
    """semidiscretize(ReactionDiffusionSplit(models), FiniteElementDiscretization(...), mesh) for a dictionary of subdomain models
    (src/discretization/fem.jl:434-542).  A dictionary that names only some cell sets is solved on those cells alone (sub-grid, nodes renumbered)."""
    p = plan_ep(split, grid, layout, world_size)
    dh, interfaces, first, fun = p["dh"], p["interfaces"], p["first"], p["functions"]
    sp = allocate_matrix(dh, interfaces)
    D = ConductivityToDiffusivityCoefficient(first.kappa, first.Cm, first.chi)
    M = setup_operator(strategy, BilinearMassIntegrator(ConstantCoefficient(1.0)), dh, sp)
    K = setup_operator(strategy, BilinearDiffusionIntegrator(D), dh, sp)
    update_operators(M, K, t0)                                            # the fused pair; interface-only entries stay 0.0
    iform = None
    if interfaces is not None and len(interfaces):
        iform = InterfaceDiffusionForm(K.dmesh, interfaces, p["G"], facet_qpoints)
        iform.assemble(K.pattern, K.A)
    return MultiDomainFunction(dh=dh, grid=p["grid"], pattern=sp, M=M, K=K, interface_form=iform, interfaces=interfaces, functions=fun,
                               heat_dofrange=fun.heat_dofrange, subdofs=p["subdofs"], strategy=strategy, device=strategy.device,
                               parent_nodes=p["parent_nodes"])


# --------------------------------------------------------------------------------------- time stepping
class MultiDomainHeatStage(BackwardEulerStage):
    """BackwardEulerStage on the operators semidiscretize_ep assembled (bulk M and K in one fused pair, the interface term added to K):
    perform_step is the parent's, unchanged, on the widened pattern."""

    def __init__(self, solver, fun):
        self.solver, self.device = solver, fun.device
        self.sp, self.M, self.K, self.source = fun.pattern, fun.M, fun.K, None
        self.A = DeviceVector(self.device, self.sp.nnz)
        self.b = DeviceVector(self.device, fun.dh.ndofs)
        if solver.mirror:
            self.K.pattern.mirror(self.K.A)
        self.dt_last = None
        self.last_iters = 0


class MultiDomainLieTrotterGodunov:
    """LieTrotterGodunov on the multi-domain split: gather φₘ out of the packed state into the heat vector (tb_gather_indexed), the heat step, scatter
    φₘ back (tb_scatter_indexed), then one reaction launch per child on its view."""

    def __init__(self, heat_stage, multi_fun, caches):
        if multi_fun.heat_dofrange is None:
            raise ValueError("the PointwiseMultiODEFunction carries no heat_dofrange (semidiscretize_ep sets it)")
        self.heat, self.f, self.cell = heat_stage, multi_fun, caches
        self.device = heat_stage.device
        hd = np.ascontiguousarray(multi_fun.heat_dofrange, dtype=np.int32)
        if hd.min() < 0 or hd.max() >= caches.u.n or len(np.unique(hd)) != len(hd):
            raise ValueError("heat_dofrange: positions must be distinct and inside the packed state")
        self.n = len(hd)
        self.idx = self.device.to_device(hd)
        self.phi = DeviceVector(self.device, self.n)

    def heat_step(self, t, dt):
        """gather φₘ, BackwardEulerStage.perform_step, scatter φₘ back; True on success"""
        u = self.cell.u
        check(lib().tb_gather_indexed(self.device.h, self.n, u.ptr, self.idx.ptr, self.phi.ptr))
        ok = self.heat.perform_step(self.phi, t, dt)
        check(lib().tb_scatter_indexed(self.device.h, self.n, self.phi.ptr, self.idx.ptr, u.ptr))
        return ok

    def reaction_step(self, t, dt):
        """one existing reaction launch per child on its view (the same kernels on the same data as a single-model step of that block)"""
        ok = True
        for f, c in zip(self.f.functions, self.cell.children):
            ok = perform_step(f, c, t, dt) and ok
        return ok

    def step(self, t, dt):
        return self.heat_step(t, dt) and self.reaction_step(t, dt)

    def reaction_step_with_tangent(self, t, dt):
        """(ok, R): the reaction step, R the maximum over the children of the child's signed maximum of du[:, φidx] (src/solver/time/rtc.jl:68-73);
        a NaN in one child is R."""
        R, ok = -np.inf, True
        for f, c in zip(self.f.functions, self.cell.children):
            if getattr(c.solver, "rush_larsen", False):
                raise NotImplementedError("the reaction tangent needs du: not with RushLarsenCellSolver")
            if c.xs is not None or f.ode.model_id == L.TB_CELL_FHN_HETEROGENEOUS:
                ok = perform_step(f, c, t, dt) and ok
                r = get_reaction_tangent(self.device, f, c)
            else:
                o, r = perform_step_with_reaction_tangent(f, c, t, dt)
                ok = o and ok
            if not np.isnan(R) and (np.isnan(r) or r > R):
                R = r
        return ok, float(R)

    def step_with_reaction_tangent(self, t, dt):
        """what ReactionTangentController.step calls: (ok, R) of one whole step"""
        if not self.heat_step(t, dt):
            return False, float("nan")
        return self.reaction_step_with_tangent(t, dt)

"""Moving a nodal field from one mesh to another on the device: point location and nodal inter-grid interpolation.

  reference (file:line)                                                              here
  ---------------------------------------------------------------------------------------------------------------
  PointEvalHandler(grid, points)          Ferrite; called at transfer_operators.jl:116   PointEvalHandler
  evaluate_at_points(ph, dh, u, field)    Ferrite; called at transfer_operators.jl:160   evaluate_at_points
  NodalIntergridInterpolation             src/ferrite-addons/transfer_operators.jl:45-148   same name
  transfer!                               transfer_operators.jl:153-161                  transfer

The search and the interpolation run on the device (tb_locator_*, csrc/tb_transfer.hip); the host part is the dof set of the target
(`node_to_dof_map`) and the positions of its nodes.  This project's DofHandler is ONE field on ONE subdomain, so the reference's field-name
arguments (`field_name_from`, `field_name_to`) and `subdomains_from` have no counterpart: the field is the handler's field.
"""
import ctypes as C
import warnings

import numpy as np

from . import _lib as L
from ._lib import check, lib
from .api import DeviceVector, DofHandler, Grid, _ptr, dof_coordinates


class PointEvalHandler:
    """PointEvalHandler(grid, points) on the device: for every point the lowest-numbered cell of the grid that contains it within `tol` (reference
    coordinates) and its reference coordinates there.  `grid_or_dh`: a Grid or any DofHandler over it (only the geometry is used).  `points`:
    (n, 3) — or (n, 2) on two-dimensional grids — host values or a DeviceVector of 3·n doubles.  A point in no cell is not an error: its cell
    is −1, `n_missing` counts it, and it evaluates to NaN.  `relocate(points)` finds other points with the same search structure."""

    def __init__(self, device, grid_or_dh, points, tol=1e-10):
        self.device = device
        self.grid = grid_or_dh if isinstance(grid_or_dh, Grid) else grid_or_dh.grid
        self._dh = DofHandler(self.grid) if isinstance(grid_or_dh, Grid) else grid_or_dh
        self._dmesh = self._dh.device_mesh(device)
        self.tol = float(tol)
        self.h = C.c_void_p()
        pts, n = self._points(points)
        check(lib().tb_locator_create(self._dmesh.h, n, _ptr(pts), self.tol, C.byref(self.h)))

    def _points(self, points):
        if isinstance(points, DeviceVector):
            assert points.n % 3 == 0, "device points are n × 3 doubles"
            return points, points.n // 3
        p = np.asarray(points, dtype=np.float64)
        p = p.reshape(-1, 3) if p.ndim == 1 else p
        if p.shape[1] == 2:
            p = np.hstack([p, np.zeros((len(p), 1))])
        p = np.ascontiguousarray(p)
        return (self.device.to_device(p.ravel()) if len(p) else None), len(p)

    def relocate(self, points):
        """tb_locator_relocate: locate another set of points (any number) in the same grid."""
        pts, n = self._points(points)
        check(lib().tb_locator_relocate(self.h, n, _ptr(pts)))
        return self

    @property
    def n_points(self):
        return int(lib().tb_locator_npoints(self.h))

    @property
    def n_missing(self):
        return int(lib().tb_locator_nmissing(self.h))

    def _download(self, ptr, count, dtype):
        out = np.empty(count, dtype=dtype)
        if count:
            check(lib().tb_memcpy_d2h(self.device.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes))
        return out

    @property
    def cells(self):
        """(n,) int32 cell ids, 0-based, −1 where the point was not found (host copy)"""
        return self._download(lib().tb_locator_cells_device(self.h), self.n_points, np.int32)

    @property
    def xi(self):
        """(n, 3) reference coordinates (host copy)"""
        return self._download(lib().tb_locator_xi_device(self.h), 3 * self.n_points, np.float64).reshape(-1, 3)

    def evaluate(self, dh, u, out, scatter=None):
        """tb_locator_evaluate: enqueue only (fits inside MI355XDevice.capture)."""
        assert dh.grid is self.grid or (dh.grid.cell_kind == self.grid.cell_kind and dh.grid.n_cells == self.grid.n_cells), "the field lives on another grid"
        assert u.n == dh.ndofs, "u has %d entries, the handler %d dofs" % (u.n, dh.ndofs)
        check(lib().tb_locator_evaluate(self.h, dh.device_mesh(self.device).h, _ptr(u), _ptr(out), _ptr(scatter)))
        return out

    def __del__(self):
        try:
            if self.h:
                lib().tb_locator_destroy(self.h)
        except Exception:
            pass


def evaluate_at_points(ph, dh, u, out=None):
    """evaluate_at_points(ph, dh, u): the field of `dh` (over ph's grid) with dof values `u` (DeviceVector) at ph's points → DeviceVector of
    n_points · ncomp values, point-major; NaN where a point was not found."""
    if out is None:
        out = DeviceVector(ph.device, ph.n_points * dh.ip.ncomp)
    assert out.n == ph.n_points * dh.ip.ncomp
    return ph.evaluate(dh, u, out)


def intergrid_dofs(dh_to, subdomains_to=None):
    """Host part of NodalIntergridInterpolation (transfer_operators.jl:69-114): (node_to_dof_map, nodes).
    node_to_dof_map = sort(unique(dofs of the cells of `subdomains_to`)) — an array of 0-based cell ids of dh_to, the name of one of its grid's cell
    sets, or None for all cells; `nodes` (n_nodes, 3): dof_coordinates(dh_to), one point per field node.  With ncomp == 3 the three dofs of a node travel
    together: node_to_dof_map is then ordered node by node (sorted by the first component's dof), components consecutive."""
    nc = dh_to.ip.ncomp
    if subdomains_to is None:
        cd = dh_to.cell_dofs
    else:
        cells = dh_to.grid.getcellset(subdomains_to) if isinstance(subdomains_to, str) else np.asarray(subdomains_to, dtype=np.int64)
        cd = dh_to.cell_dofs[cells]
    per_node = cd.reshape(-1, nc)                                              # the dofs of one field node, components interleaved (close!(dh))
    first, where = np.unique(per_node[:, 0], return_index=True)                # sorted, unique: the first dof of every field node touched
    node_to_dof_map = per_node[where].reshape(-1)
    nodes = dof_coordinates(dh_to)[first]
    return np.ascontiguousarray(node_to_dof_map, dtype=np.int32), np.ascontiguousarray(nodes)


class NodalIntergridInterpolation:
    """NodalIntergridInterpolation(dh_from, dh_to; subdomains_to) (transfer_operators.jl:45-148): moves the field of `dh_from` to the dofs of `dh_to` that
    belong to the cells `subdomains_to` (0-based cell ids of dh_to, the name of a cell set of its grid, or None: every cell), by evaluating it at the
    positions of those dofs.  Every position must lie in the mesh of dh_from — there is no extrapolation; positions that do not are counted
    (`n_missing`), warned about once, and receive NaN.  Both handlers carry the same number of components (1 or 3).

    This project's DofHandler is one field on one subdomain, so the reference's `field_name_from` / `field_name_to` / `subdomains_from`
    arguments have no counterpart here."""

    def __init__(self, device, dh_from, dh_to, subdomains_to=None, tol=1e-10):
        if dh_from.ip.ncomp != dh_to.ip.ncomp:
            raise ValueError("NodalIntergridInterpolation: %d components on the source, %d on the target" % (dh_from.ip.ncomp, dh_to.ip.ncomp))
        self.device, self.dh_from, self.dh_to = device, dh_from, dh_to
        self.node_to_dof_map, self.nodes = intergrid_dofs(dh_to, subdomains_to)
        self.ph = PointEvalHandler(device, dh_from, self.nodes, tol)
        self._scatter = device.to_device(self.node_to_dof_map) if len(self.node_to_dof_map) else None
        self.n_missing = self.ph.n_missing
        if self.n_missing:
            warnings.warn("Constructing the interpolation failed. %d (out of %d) points not found." % (self.n_missing, len(self.nodes)))


def transfer(u_to, operator, u_from):
    """transfer!(u_to, operator, u_from) (transfer_operators.jl:153-161): u_to[node_to_dof_map] = the field u_from at the target's nodes — one
    tb_locator_evaluate with the scatter map; DeviceVectors in and out, nothing visits the host, other entries of u_to are not touched."""
    assert u_to.n == operator.dh_to.ndofs, "u_to has %d entries, the target handler %d dofs" % (u_to.n, operator.dh_to.ndofs)
    operator.ph.evaluate(operator.dh_from, u_from, u_to, operator._scatter)
    return u_to

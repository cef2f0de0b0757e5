"""The 8³-cell heat problem that tests/test_amg_gpu.py and tests/test_mg_family_bits_gpu.py share, and the two small builders it needs."""
import numpy as np


def face_dofs(tb, dh, axis=0, value=0.0):
    return np.flatnonzero(np.abs(tb.dof_coordinates(dh)[:, axis] - value) < 1e-12)


def heat_values(tb, device, dh, sp, D, dt=0.1):
    """M − Δt·K on the host (K as the diffusion form leaves it: negative semidefinite) and the pattern"""
    st = tb.PatchAssemblyStrategy(device)
    K = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(D), dh, sp), 0.0)
    M = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
    return M.A.to_host() - dt * K.A.to_host(), K.pattern


def gmg_problem(tb, device):
    """the 8³-cell heat problem over a 4³-cell coarse grid (125 dofs: above max_coarse, below the dense inverse's limit) → (gh, dh, sp, pattern, dA, ch, b)"""
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (4, 4, 4), (0, 0, 0), (1, 1, 1)), 1)
    dh = tb.DofHandler(gh.grids[-1])
    sp = tb.allocate_matrix(dh)
    vals, pattern = heat_values(tb, device, dh, sp, tb.ConstantCoefficient(np.diag([9.0, 4.0, 4.0])))
    ch = tb.ConstraintHandler(dh, face_dofs(tb, dh))
    dA = device.to_device(vals)
    tb.apply_zero(dA, None, ch, pattern=pattern)
    b = np.random.default_rng(29).normal(size=dh.ndofs)
    b[ch.prescribed_dofs] = 0.0
    return gh, dh, sp, pattern, dA, ch, b

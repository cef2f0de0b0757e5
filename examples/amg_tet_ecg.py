#!/usr/bin/env python3
"""Algebraic multigrid on a tetrahedral mesh at toy size: backward-Euler heat steps (M − Δt·K) u⁺ = M u on a box of linear tetrahedra with one face
held at zero, solved by CG with the Jacobi preconditioner and with AMGPrecon().  A tetrahedral mesh has no GridHierarchy, so the geometric multigrid
does not apply; the AMG needs the matrix only.  The hierarchy is planned at the first step and reused by the later ones (the matrix does not change:
setup=False).  Prints one JSON line: iterations per step of both, the levels, and the largest difference of the two solutions."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import thunderbolt_jl_amd as tb  # noqa: E402


def main(n=8, dt=0.05, steps=3, rtol=1e-10):
    dev = tb.MI355XDevice(0)
    grid = tb.generate_mesh(tb.Tetrahedron, (n, n, n), (0, 0, 0), (1, 1, 1))
    dh = tb.DofHandler(grid)
    sp = tb.allocate_matrix(dh)
    st = tb.PatchAssemblyStrategy(dev)
    kappa = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(np.diag([4.0, 1.0, 1.0])), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
    K = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(kappa), dh, sp), 0.0)
    M = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
    Mh = M.A.to_host()
    X = tb.dof_coordinates(dh)
    ch = tb.ConstraintHandler(dh, np.flatnonzero(X[:, 0] == 0.0))
    A = dev.to_device(Mh - dt * K.A.to_host())
    tb.apply_zero(A, None, ch, pattern=K.pattern)
    rowptr, colidx = sp.rowptr, sp.colidx
    rows = np.repeat(np.arange(dh.ndofs), np.diff(rowptr))
    u0 = np.exp(-40.0 * ((X - 0.6) ** 2).sum(axis=1))
    u0[ch.prescribed_dofs] = 0.0
    amg = tb.AMGPrecon(max_coarse=64).materialize(K.pattern, ch)
    out = {}
    for name, precond in (("jacobi", "jacobi"), ("amg", amg)):
        u, its = u0.copy(), []
        for step in range(steps):
            b = np.bincount(rows, weights=Mh * u[colidx], minlength=dh.ndofs)      # M u
            b[ch.prescribed_dofs] = 0.0
            x = dev.to_device(u)
            if precond is amg:
                it, _ = amg.solve(A, dev.to_device(b), x, rtol=rtol, atol=0.0, setup=step == 0)
            else:
                it, _ = tb.pcg_solve(K.pattern, A, dev.to_device(b), x, rtol=rtol, atol=0.0, maxiter=5000, precond=precond)
            u = x.to_host()
            its.append(it)
        out[name] = (u, its)
    diff = float(np.abs(out["amg"][0] - out["jacobi"][0]).max() / np.abs(out["jacobi"][0]).max())
    print(json.dumps({"dofs": dh.ndofs, "cells": int(grid.n_cells), "levels": [amg.level_size(l)[0] for l in range(amg.n_levels)],
                      "iterations_jacobi": out["jacobi"][1], "iterations_amg": out["amg"][1], "max_relative_difference": diff}))


if __name__ == "__main__":
    main()

"""What tests/golden/amg_scalar_parent_bits.npz records and tests/test_amg_elasticity_gpu.py recomputes: AMGPrecon() without a near-null-space on the
`elasticity` and `hex9` systems of tests/test_amg_gpu.py, on the commit before the near-null-space existed.  Two assemblies may differ in their last
bits, so the eliminated matrix is rounded to binary32 values before the set-up: the input is then the same on every run (its SHA-256 is recorded and
compared first), every sum of the hierarchy has one order, and every comparison is `==`.  Large arrays are stored as their SHA-256 and their ends."""
import hashlib

import numpy as np

from gmg_case import face_dofs, heat_values

SYSTEMS = ("elasticity", "hex9")
MAX_COARSE, DEGREE, RATIO = 32, 2, 4.0


def put(out, key, a):
    a = np.ascontiguousarray(a)
    if a.size <= 64:
        out[key] = a
    else:
        out[key + ".sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
        out[key + ".ends"] = np.concatenate([a.ravel()[:8], a.ravel()[-8:]])


def system(tb, device, name):
    """→ (dh, pattern, ch, dA, keep): the eliminated matrix in binary32 values, as float64 on the device"""
    keep = None
    if name == "elasticity":
        grid = tb.generate_mesh(tb.Hexahedron, (5, 5, 5), (0, 0, 0), (1, 1, 1), perturb=0.1)
        dh = tb.DofHandler(grid, tb.LagrangeCollection(1) ** 3)
        sp = tb.allocate_matrix(dh)
        ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
        keep = tb.setup_operator(tb.ElementAssemblyStrategy(device), tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(a=1.0, b=1.0, af=0.0, as_=0.0, afs=0.0, beta=1.0), ms), []), dh, sp)
        u = np.random.default_rng(5).uniform(-5e-3, 5e-3, dh.ndofs)
        u[face_dofs(tb, dh)] = 0.0
        tb.update_linearization(keep, device.to_device(u), 0.0, residual=device.zeros(dh.ndofs))
        vals, pattern = keep.J.to_host(), keep.pattern
    else:
        grid = tb.generate_mesh(tb.Hexahedron, (8, 8, 8), (0, 0, 0), (1, 1, 1), perturb=0.1)
        dh = tb.DofHandler(grid)
        sp = tb.allocate_matrix(dh)
        vals, pattern = heat_values(tb, device, dh, sp, tb.ConstantCoefficient(np.eye(3)))
    ch = tb.ConstraintHandler(dh, face_dofs(tb, dh))
    dA = device.to_device(vals)
    tb.apply_zero(dA, None, ch, pattern=pattern)
    dA = device.to_device(dA.to_host().astype(np.float32).astype(np.float64))
    return dh, pattern, ch, dA, keep


def scalar_bits(tb, device, name):
    """AMGPrecon(max_coarse=32) as it is without a near-null-space: the input's hash, λmax per level, the last level's matrix, one cycle, the solve"""
    dh, pattern, ch, dA, keep = system(tb, device, name)
    amg = tb.AMGPrecon(max_coarse=MAX_COARSE, degree=DEGREE, interval_ratio=RATIO).materialize(pattern, ch)
    amg.setup(dA)
    nl = amg.n_levels
    out, k = {}, name + "."
    put(out, k + "input", dA.to_host())
    put(out, k + "n_levels", np.int64(nl))
    for l in range(nl):
        put(out, k + "A%d" % l, amg.level_matrix(l).data)
        if l < nl - 1:
            put(out, k + "lmax%d" % l, np.float64(amg.lambda_max(l)))
            put(out, k + "P%d" % l, amg.prolongator(l).data)
    b = np.random.default_rng(17).normal(size=dh.ndofs)
    b[ch.prescribed_dofs] = 0.0
    put(out, k + "z", amg.apply(device.to_device(b), device.zeros(dh.ndofs)).to_host())
    x = device.zeros(dh.ndofs)
    it, res = tb.pcg_solve(pattern, dA, device.to_device(b), x, rtol=1e-10, atol=0.0, maxiter=200, precond=amg)
    put(out, k + "iterations", np.int64(it))
    put(out, k + "resnorm", np.float64(res))
    put(out, k + "x", x.to_host())
    amg.close()
    return out


def record(tb, device, path):
    """writes the golden file: run once, on the parent commit's library"""
    out = {}
    for name in SYSTEMS:
        out.update(scalar_bits(tb, device, name))
    np.savez(path, **out)
    return out

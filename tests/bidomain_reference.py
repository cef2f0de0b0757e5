"""NumPy restatement of the parabolic–elliptic bidomain block system (thunderbolt.jl_amd/bidomain.py, csrc/tb_bidomain.hip): the dense grounded block
matrix from CSR arrays of M, Kᵢ, Kₑ, the a-posteriori error bound the solve tests hold the device to, and the meshes and coefficients of the tests.
Nothing here imports the package.  Unknowns are ordered BLOCKED here, (φₘ; φₑ): `interleave` / `deinterleave` go to and from the device's layout."""
import numpy as np

KAPPA_I = np.diag([3.0, 1.0, 1.0]) * 1e-3        # fibres along x; unequal anisotropy ratios: 3 : 1 against 4 : 3
KAPPA_E = np.diag([2.0, 1.5, 1.5]) * 1e-3
DT = 0.1
EPS = np.finfo(np.float64).eps


def dense_of_csr(rowptr, colidx, nz):
    n = len(rowptr) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rowptr)), colidx] = nz
    return A


def mean_diagonal(rowptr, colidx, nz):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return float(np.mean(nz[rows == colidx]))


def ground_diagonal(rowptr, colidx, Ki, Ke, dt):
    """what goes on the eliminated rows: the mean diagonal of the φₑφₑ block −Δt(Kᵢ + Kₑ)"""
    return -dt * (mean_diagonal(rowptr, colidx, Ki) + mean_diagonal(rowptr, colidx, Ke))


def block_matrix(rowptr, colidx, M, Ki, Ke, dt, ground=(), ground_diag=None):
    """[[M − ΔtKᵢ, −ΔtKᵢ], [−ΔtKᵢ, −Δt(Kᵢ + Kₑ)]] dense, 2n × 2n; the φₑ rows and columns of `ground` eliminated with `ground_diag` on the diagonal"""
    n = len(rowptr) - 1
    Md, Kid, Ked = (dense_of_csr(rowptr, colidx, a) for a in (M, Ki, Ke))
    A = np.block([[Md - dt * Kid, -dt * Kid], [-dt * Kid, -dt * (Kid + Ked)]])
    if len(ground):
        d = ground_diagonal(rowptr, colidx, Ki, Ke, dt) if ground_diag is None else ground_diag
        for g in ground:
            A[n + g, :] = 0.0
            A[:, n + g] = 0.0
            A[n + g, n + g] = d
    return A


def asymmetry(A):
    """max |A − Aᵀ| / max |A|.  The oracle sums the element contributions of a_ij and a_ji in different orders, so its matrices are symmetric to the
    rounding of those sums only (measured: ≤ 5e-17 relative, a quarter of ε); the tests allow ε."""
    return float(np.abs(A - A.T).max() / np.abs(A).max())


def heat_matrix(rowptr, colidx, M, K, dt):
    return dense_of_csr(rowptr, colidx, M) - dt * dense_of_csr(rowptr, colidx, K)


def interleave(v):
    n = len(v) // 2
    out = np.empty(2 * n)
    out[0::2], out[1::2] = v[:n], v[n:]
    return out


def deinterleave(v):
    return np.concatenate([v[0::2], v[1::2]])


def solve_refined(A, b, steps=2):
    """A⁻¹b with `steps` rounds of iterative refinement, the residual formed in extended precision: the error of a plain LU solve is of the order
    cond(A)·ε‖x‖, which for the grounded block matrix (condition 1e5 and more) is what a tightly converged device solve is to be compared AT — the
    refined solution is accurate to a few ε‖x‖, so a deviation measured against it is the device's"""
    x = np.linalg.solve(A, b)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(steps):
        r = (bl - Al @ x.astype(np.longdouble)).astype(np.float64)
        x = x + np.linalg.solve(A, r)
    return x


def error_bound(A, b, x, lam_min=None):
    """‖x − x*‖₂ ≤ (‖b − A x‖₂ + 4ε‖ |A||x| ‖₂)/λ_min(A) for symmetric positive definite A: the residual evaluated in floating point, its own
    rounding allowed for, divided by the smallest eigenvalue"""
    lam = float(np.linalg.eigvalsh(0.5 * (A + A.T))[0]) if lam_min is None else lam_min
    assert lam > 0.0
    return (np.linalg.norm(b - A @ x) + 4.0 * EPS * np.linalg.norm(np.abs(A) @ np.abs(x))) / lam


def row_bound(A, x):
    """Σⱼ |aᵢⱼ||xⱼ| per row"""
    return np.abs(A) @ np.abs(x)


# ---- the meshes: the smallest at which the kernels can go wrong
MESHES = {
    "hex_5x4x3": ("Hexahedron", (5, 4, 3)),       # 120 nodes, rows of 8, 12, 18 and 27 entries, two 64-row slices, the last one partial
    "tet_3x3x2": ("Tetrahedron", (3, 3, 2)),      # uneven row lengths
    "quad_7x5": ("Quadrilateral", (7, 5)),
    "hex_11x10x9": ("Hexahedron", (11, 10, 9)),   # 1 320 nodes, 2 640 unknowns: more than one workgroup of a 1 024-lane reduction (product only)
}
SOLVE_MESHES = ("hex_5x4x3", "tet_3x3x2", "quad_7x5")


def build_mesh(tb, name):
    kind, nel = MESHES[name]
    if kind == "Quadrilateral":
        g = tb.generate_mesh(tb.Quadrilateral, nel, (0.0, 0.0), (1.4, 1.0))
    else:
        g = tb.generate_mesh(getattr(tb, kind), nel, (0.0, 0.0, 0.0), (1.0 + 0.1 * nel[0], 1.0, 0.8))
    dh = tb.DofHandler(g)
    return g, dh, tb.allocate_matrix(dh)


def oracle_matrices(tb, oracle, g, dh, sp, kappa_i=KAPPA_I, kappa_e=KAPPA_E, chi=1.0, Cm=1.0):
    """(M, Kᵢ, Kₑ) as CSR value arrays from the CPU oracle, D = κ/(χCₘ)"""
    quad = g.cell_kind == tb.Quadrilateral
    okind = {tb.Quadrilateral: oracle.QUAD4, tb.Hexahedron: oracle.HEX8, tb.Tetrahedron: oracle.TET4}[g.cell_kind]
    om = oracle.Mesh(okind, 2, np.ascontiguousarray(g.xyz[:, :2]) if quad else g.xyz, g.conn, dh.cell_dofs)
    d = 2 if quad else 3
    M = oracle.assemble_matrix(om, 0, oracle.Coef(oracle.COEF_CONST_SCALAR, [1.0]), sp.rowptr, sp.colidx)
    Ki = oracle.assemble_matrix(om, 1, oracle.Coef(oracle.COEF_CONST_TENSOR, np.ascontiguousarray(kappa_i[:d, :d]).ravel(), Cm=Cm, chi=chi, wrap=True), sp.rowptr, sp.colidx)
    Ke = oracle.assemble_matrix(om, 1, oracle.Coef(oracle.COEF_CONST_TENSOR, np.ascontiguousarray(kappa_e[:d, :d]).ravel(), Cm=Cm, chi=chi, wrap=True), sp.rowptr, sp.colidx)
    return M, Ki, Ke

"""Shared test helpers (test infrastructure): comparison norms and small mesh builders."""
import numpy as np


def rel_err(got, ref):
    """SURVEY §8 parity norms: relative 2-norm (Frobenius for nz vectors) and max-entrywise relative to max|ref|."""
    got, ref = np.asarray(got), np.asarray(ref)
    d = np.abs(got - ref)
    scale2 = np.linalg.norm(ref) or 1.0
    scalem = np.abs(ref).max() or 1.0
    return max(np.linalg.norm(d) / scale2, d.max() / scalem)


def per_state_err(got, ref, nstates, n, layout):
    """One figure per state of a pointwise ODE array: max over the points of |got − ref| of that state, relative to max over the points of |ref| of that
    state.  `layout` is "SOA" (u[k·n + i]) or "AOS" (u[i·nstates + k]).  A state whose reference is zero at every point has no scale: it has to be exactly
    zero in `got` (figure 0), anything else is reported as inf.  A NaN in `got` gives a NaN figure, which fails every `<` it is asserted with."""
    got, ref = np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    assert got.size == ref.size
    return per_state_ratio(np.abs(got - ref), ref, nstates, n, layout)


def per_state_ratio(dev, ref, nstates, n, layout):
    """per_state_err for a deviation given entry by entry (`dev` ≥ 0): max over the points of dev, by max over the points of |ref|, for every state"""
    assert layout in ("SOA", "AOS")
    dev, ref = np.asarray(dev, dtype=np.float64).ravel(), np.asarray(ref, dtype=np.float64).ravel()
    assert dev.size == ref.size == nstates * n
    d, r = (dev.reshape(nstates, n), ref.reshape(nstates, n)) if layout == "SOA" else (dev.reshape(n, nstates).T, ref.reshape(n, nstates).T)
    out = np.empty(nstates)
    for k in range(nstates):
        dmax = np.nan if np.isnan(d[k]).any() else (d[k].max() if n else 0.0)      # (ndarray.max propagates a NaN as well; spelt out because the tests rely on it)
        scale = np.abs(r[k]).max() if n else 0.0
        out[k] = dmax / scale if scale > 0.0 else (0.0 if dmax == 0.0 else dmax * np.inf)
    return out


# The protocols of the reaction parity tests (tests/test_gpu_parity.py), by number of states: forward-Euler Δt, adaptive sub-stepper Δt and threshold,
# and the Rush–Larsen Δt of the models that have a gate decomposition (PCG2019 7 states, TT06 19, O'Hara–Rudy 41)
FE_DT = {2: 0.1, 7: 0.01, 19: 0.001, 41: 0.002}
ADAPTIVE_DT = {2: 0.05, 7: 0.05, 19: 0.007, 41: 0.007}
ADAPTIVE_THRESHOLD = {2: 0.05, 7: 1.0, 19: 20.0, 41: 20.0}
RL_DT = {7: 0.05, 19: 0.02, 41: 0.01}


def phi_rates(oracle, oid, params, u, nstates, n, layout, phi, xs=None):
    """dφₘ/dt of every point of the flat state array `u` (left unchanged), from the oracle's cell_rhs: what the adaptive sub-stepper compares with its threshold.
    With coordinates (`xs`) the rate is the one the oracle's forward-Euler step reports for a copy of `u`: cell_rhs takes no coordinate."""
    u = np.asarray(u, dtype=np.float64)
    if xs is not None:
        du = oracle.reaction_step_x(oid, params, u.copy(), n, xs, getattr(oracle, "LAYOUT_" + layout), t=0.0, dt=0.0, substeps=1, threshold=0.0)
        return (du.reshape(nstates, n)[phi] if layout == "SOA" else du.reshape(n, nstates)[:, phi]).copy()
    pts = u.reshape(nstates, n).T if layout == "SOA" else u.reshape(n, nstates)
    return np.array([oracle.cell_rhs(oid, params, np.ascontiguousarray(p))[phi] for p in pts])


def hex_to_tets(xyz, conn):
    """Split every hexahedron into 6 positively oriented tetrahedra around the 0–6 diagonal."""
    T = [(0, 1, 2, 6), (0, 2, 3, 6), (0, 3, 7, 6), (0, 7, 4, 6), (0, 4, 5, 6), (0, 5, 1, 6)]
    tets = np.concatenate([conn[:, list(t)] for t in T], axis=0).astype(np.int32)
    # orient: det > 0
    X = xyz[tets]
    det = np.einsum("ij,ij->i", np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), X[:, 3] - X[:, 0])
    flip = det < 0
    tets[flip] = tets[flip][:, [0, 2, 1, 3]]
    return np.ascontiguousarray(tets)


def pentagon_prism_mesh(tb, layers=2):
    """A pentagon cut into five quadrilaterals around its centre, extruded: the centre vertices of the inner layers sit in TEN hexahedra — more than the
    eight a structured grid ever has (the record-driven gather of the element strategy holds eight cells per node and must hand such meshes to the
    general kernel; unstructured ventricle meshes have such vertices)."""
    ang = 2 * np.pi * np.arange(5) / 5 + 0.3
    p2 = np.stack([np.cos(ang), np.sin(ang)], axis=1)
    m2 = 0.5 * (p2 + np.roll(p2, -1, axis=0))                    # m[i] between p[i] and p[i+1]
    pts2 = np.concatenate([[[0.05, -0.03]], p2, m2])             # 0: centre (slightly off), 1..5: corners, 6..10: edge midpoints
    xyz = np.concatenate([np.column_stack([pts2 + 0.02 * k, np.full(11, 0.45 * k)]) for k in range(layers + 1)])
    conn = []
    for k in range(layers):
        lo, hi = 11 * k, 11 * (k + 1)
        for i in range(5):
            quad = [0, 6 + (i - 1) % 5, 1 + i, 6 + i]            # centre, m[i-1], p[i], m[i]: counter-clockwise
            conn.append([lo + q for q in quad] + [hi + q for q in quad])
    return tb.Grid(tb.Hexahedron, np.ascontiguousarray(xyz), np.ascontiguousarray(np.array(conn, dtype=np.int32)))

"""The hexahedron source-vector kernel (k_vector_hex8_patch) has one instance per (HALO, source kind); the kind's time value is read once in front
of the cell loop.  Every instance against the CPU oracle on meshes that reach every trip of the cell loop, the time read under graph replay, the
determinism of the HALO flavour, and the forms the host dispatch must leave to the general kernels.  Tolerance: tests/test_gpu_parity.py's TOL."""
import numpy as np
import pytest

from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-12

# one full 8×8×8 tile plus one-cell-thick remainder tiles: with its halo cells the full tile's patch holds more than 512 instances, so the third trip
# of the cell loop (indices read in place, not from the prologue's registers) runs in the HALO flavour; the own-cells flavour makes two trips
MESHES = {"17x9x10": (17, 9, 10), "9x8x8": (9, 8, 8)}
KINDS = [("const", "SRC_CONST", 0.0), ("norm_plus_t", "SRC_NORM_PLUS_T", 0.0), ("norm_plus_t", "SRC_NORM_PLUS_T", 0.7), ("cos_exp", "SRC_COS_EXP", 0.1)]
TAB_T = 0.3


@pytest.fixture(scope="module")
def problems(tb, oracle):
    """mesh name → (dof handler, {(kind, t): oracle vector}); computed once, never written to"""
    out = {}
    for name, nel in MESHES.items():
        g = tb.generate_mesh(tb.Hexahedron, nel, (-1, -1, -1), (1, 1, 1), perturb=0.25)
        dh = tb.DofHandler(g)
        om = oracle.Mesh(oracle.HEX8, 2, g.xyz, g.conn, dh.cell_dofs)
        refs = {(kind, t): oracle.assemble_source(om, getattr(oracle, okind), [2.5], t=t) for kind, okind, t in KINDS}
        refs[("tabulated", TAB_T)] = oracle.assemble_source(om, oracle.SRC_NORM_PLUS_T, t=TAB_T)
        for r in refs.values():
            r.setflags(write=False)
        out[name] = (dh, refs)
    return out


def _strategy(tb, device, which):
    return tb.PatchAssemblyStrategy(device) if which == "patch" else tb.AtomicAssemblyStrategy(device)


@pytest.mark.parametrize("which", ["patch", "atomic"])
@pytest.mark.parametrize("mesh", list(MESHES))
def test_every_kind_and_flavour_matches_the_oracle(tb, device, problems, mesh, which):
    dh, refs = problems[mesh]
    st = _strategy(tb, device, which)
    for kind, _, t in KINDS:
        op = tb.setup_operator(st, tb.LinearIntegrator(tb.AnalyticalCoefficient(kind, 2.5)), dh)
        tb.update_operator(op, t)
        e = rel_err(op.b.to_host(), refs[(kind, t)])
        print(mesh, which, kind, t, "rel_err %.3e" % e)
        assert e < TOL, (mesh, which, kind, t, e)
    # host-tabulated closure: the one instance that reads the cell index of an instance
    op = tb.setup_operator(st, tb.LinearIntegrator(tb.AnalyticalCoefficient(lambda x, t: np.linalg.norm(x) + t)), dh)
    tb.update_operator(op, TAB_T)
    e = rel_err(op.b.to_host(), refs[("tabulated", TAB_T)])
    print(mesh, which, "tabulated", TAB_T, "rel_err %.3e" % e)
    assert e < TOL, (mesh, which, "tabulated", e)


@pytest.mark.parametrize("which", ["patch", "atomic"])
@pytest.mark.parametrize("kind", ["cos_exp", "norm_plus_t"])
def test_graph_replay_reads_the_time_of_each_launch(tb, device, problems, kind, which):
    """The time value is read once per workgroup in front of the cell loop: from the device slot when the launch is replayed from a graph.  One capture,
    two launches at different times, each equal to the plain call at that time."""
    dh, _ = problems["9x8x8"]
    op = tb.setup_operator(_strategy(tb, device, which), tb.LinearIntegrator(tb.AnalyticalCoefficient(kind, 2.5)), dh)
    times = (0.1, 0.45)
    plain = [tb.update_operator(op, t).b.to_host().copy() for t in times]          # also builds the plan before the capture
    assert np.abs(plain[0] - plain[1]).max() > 1e-6 * np.abs(plain[0]).max()        # the source does move with the time
    gr = device.capture(lambda: tb.update_operator(op, 123.0))                      # captured with a time no replay uses
    try:
        for t, ref in zip(times, plain):
            op.b.copy_from_host(np.full(dh.ndofs, np.nan))
            gr.launch(t)
            device.poll_status()
            e = rel_err(op.b.to_host(), ref)
            print(kind, which, t, "rel_err %.3e" % e)
            assert e < TOL, (kind, which, t, e)
    finally:
        gr.close()


def test_halo_flavour_is_bit_reproducible(tb, device, problems):
    """PATCH strategy: every owned dof is summed in LDS by its own patch, the waves adding in turn (a fixed order), and stored once.  With unordered waves
    (the kernel before its HALO instances took turns) two launches differed in the last bit at 35 of these 1 980 dofs, 3.6e-16 relative."""
    dh, refs = problems["17x9x10"]
    op = tb.setup_operator(tb.PatchAssemblyStrategy(device), tb.LinearIntegrator(tb.AnalyticalCoefficient("cos_exp", 2.5)), dh)
    b1 = tb.update_operator(op, 0.1).b.to_host().copy()
    b2 = tb.update_operator(op, 0.1).b.to_host().copy()
    np.testing.assert_array_equal(b1, b2)
    assert rel_err(b1, refs[("cos_exp", 0.1)]) < TOL


def test_a_cell_set_is_not_captured_by_the_patch_dispatch(tb, oracle, device):
    """Only hyperelastic forms take a cell set: tb_form_set_cellset refuses a source form, so none reaches the dispatch with one (the has_cellset guard
    in run_vector cannot be reached through the ABI).  The refused form stays usable and matches the oracle on the whole mesh."""
    from thunderbolt_jl_amd import _lib as L
    lib = tb.lib()
    g = tb.generate_mesh(tb.Hexahedron, (5, 4, 3), (-1, -1, -1), (1, 1, 1), perturb=0.2)
    dh = tb.DofHandler(g)
    cells = np.arange(0, g.n_cells, 2, dtype=np.int32)
    for st in (tb.PatchAssemblyStrategy(device), tb.AtomicAssemblyStrategy(device)):
        op = tb.setup_operator(st, tb.LinearIntegrator(tb.AnalyticalCoefficient("cos_exp")), dh)
        assert lib.tb_form_set_cellset(op.form.h, cells.ctypes.data_as(L.c_i32p), len(cells), 0) != 0
        assert b"hyperelastic" in lib.tb_last_error_string()
        tb.update_operator(op, 0.1)
        om = oracle.Mesh(oracle.HEX8, 2, g.xyz, g.conn, dh.cell_dofs)
        assert rel_err(op.b.to_host(), oracle.assemble_source(om, oracle.SRC_COS_EXP, t=0.1)) < TOL

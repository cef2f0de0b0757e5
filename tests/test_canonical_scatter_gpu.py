"""The CANON instances of the record kernel (tb_patch_fused.hip): canonical patches — every owned row 27 entries long with its columns in lexicographic
lattice order — scatter with compile-time LDS offsets; every other patch keeps the signature path.  Two child processes assemble the same cases, one
with TB_PATCH_CANON=1 (the canonical class in a launch of its own at any size: left alone, the library splits the classes only from 64 canonical patches
per CU on, where the gain exceeds the price of the second launch) and one with TB_PATCH_CANON=0 (the switch is read once per process), both with the
flagship's 5×5×6 tile fixed through TB_PATCH_TILE (canonical_meshes.TILE).  Checked here:
  * M and K of every case against the oracle: max |difference| over ALL entries ≤ 1e-12 · max |reference| (the suite's TOL and norm, helpers.rel_err);
  * canonical against general path: both add the same values to the same accumulators, only the order of the ≤ 8 additions per entry may differ, so the
    two agree to a few ulps — asserted at 1e-14 relative, the spread of two runs of the general path printed beside it;
  * through tb_last_kernel_name, that the CANON instance ran exactly where the planner finds canonical patches (tests/test_canonical_planner_cpu.py
    checks those verdicts against the CSR pattern) and nowhere under TB_PATCH_CANON=0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import canonical_meshes
from helpers import rel_err

ROOT_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TOL = 1e-12
KAPPA = {"iso": np.diag([4.5e-5, 2.0e-5, 2.0e-5]),                                    # positive definite: integrated in L⁻¹x (ISO instance)
         "diag": np.diag([4.5e-5, -2.0e-5, 2.0e-5]),                                  # indefinite and diagonal: DIAG instance
         "gen": np.array([[4.5e-5, 6e-5, 0], [6e-5, 2.0e-5, 1e-5], [0, 1e-5, 2.0e-5]])}  # indefinite with off-diagonal entries: general instance
INSTANCE = {"iso": "ISO", "diag": "DIAG", "gen": "GEN"}
RHO = 1.7


def _child(out):
    """every case once (the pair twice), results to <out>.npz, kernel names to <out>.json"""
    import thunderbolt_jl_amd as tb
    dev = tb.MI355XDevice(0)
    st = tb.PatchAssemblyStrategy(dev)
    arrays, names = {}, {}

    def operators(dh, sp, form):
        return (tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(RHO)), dh, sp),
                tb.setup_operator(st, tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(KAPPA[form])), dh, sp))

    def kernel():
        return tb.lib().tb_last_kernel_name().decode()

    for name, dh in canonical_meshes.build(tb).items():
        sp = tb.allocate_matrix(dh)
        M, K = operators(dh, sp, "iso")
        for rep in ("", "/again"):
            tb.update_operators(M, K, 0.0)
            arrays[name + "/pair/M" + rep], arrays[name + "/pair/K" + rep] = M.A.to_host(), K.A.to_host()
        names[name + "/pair"] = kernel()
        if name != "box":
            continue
        # K alone and M alone on the pair's plan
        M.A.fill_zero(); K.A.fill_zero()
        tb.update_operator(K, 0.0)
        names["box/K"] = kernel()
        tb.update_operator(M, 0.0)
        names["box/M"] = kernel()
        arrays["box/alone/M"], arrays["box/alone/K"] = M.A.to_host(), K.A.to_host()
        for form in ("diag", "gen"):
            Mf, Kf = operators(dh, sp, form)
            tb.update_operators(Mf, Kf, 0.0)
            names["box/" + form] = kernel()
            arrays["box/%s/M" % form], arrays["box/%s/K" % form] = Mf.A.to_host(), Kf.A.to_host()
        # HIP-graph replay of the pair call at two times
        gr = dev.capture(lambda: tb.update_operators(M, K, 123.0))
        names["box/graph_nodes"] = gr.nodes
        for k, t in enumerate((0.1, 0.7)):
            M.A.fill_zero(); K.A.fill_zero()
            gr.launch(t)
            dev.synchronize()
            arrays["box/graph%d/M" % k], arrays["box/graph%d/K" % k] = M.A.to_host(), K.A.to_host()
    np.savez(out + ".npz", **arrays)
    with open(out + ".json", "w") as f:
        json.dump(names, f)
    print("CANON_CHILD_OK")


def _run_child(out, canon):
    env = dict(os.environ, TB_PATCH_TILE=canonical_meshes.TILE, TB_PATCH_CANON="1" if canon else "0")
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_canonical_scatter_gpu as t; t._child(%r)" % (ROOT_DIR, os.path.join(ROOT_DIR, "tests"), out)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "CANON_CHILD_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    with open(out + ".json") as f:
        return dict(np.load(out + ".npz")), json.load(f)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("canonical_scatter")
    on = _run_child(str(d / "canon"), True)
    off = _run_child(str(d / "general"), False)
    return {"canon": on, "general": off}


@pytest.fixture(scope="module")
def reference(tb, oracle):
    """oracle matrices per (mesh, tensor form), computed once"""
    meshes = canonical_meshes.build(tb)
    cache = {}

    def get(name, form):
        if (name, form) not in cache:
            dh = meshes[name]
            sp = tb.allocate_matrix(dh)
            om = oracle.Mesh(oracle.HEX8, 2, dh.grid.xyz, dh.grid.conn, dh.cell_dofs)
            cache[(name, form)] = (oracle.assemble_matrix(om, 0, oracle.Coef(oracle.COEF_CONST_SCALAR, [RHO]), sp.rowptr, sp.colidx),
                                   oracle.assemble_matrix(om, 1, oracle.Coef(oracle.COEF_CONST_TENSOR, KAPPA[form].ravel()), sp.rowptr, sp.colidx))
        return cache[(name, form)]
    return get


def _check(runs, reference, mesh, case, form="iso"):
    refM, refK = reference(mesh, form)
    (a_on, _), (a_off, _) = runs["canon"], runs["general"]
    for which, ref in (("M", refM), ("K", refK)):
        key = "%s/%s/%s" % (mesh, case, which)
        e_on, e_off, d = rel_err(a_on[key], ref), rel_err(a_off[key], ref), rel_err(a_on[key], a_off[key])
        print("%-28s oracle: TB_PATCH_CANON=1 %.2e  =0 %.2e   1 against 0 %.2e" % (key, e_on, e_off, d))
        assert e_on < TOL and e_off < TOL, (key, e_on, e_off)
        assert d <= 1e-14, (key, d)


@pytest.mark.parametrize("mesh", sorted(canonical_meshes.EXPECT_CANONICAL))
def test_pair_on_every_numbering(runs, reference, mesh):
    """the 16×16×19 box (interior patches canonical), the 4×4×4 box (no interior patch), the box with cells and nodes shuffled (no canonical patch), the
    shuffled box with its dofs renamed by the locality permutation (canonical patches back, oracle on that numbering) and the lattice with the x axis
    of its numbering reversed (full rows in the wrong order: every patch rejected)"""
    _check(runs, reference, mesh, "pair")
    name_on, name_off = runs["canon"][1][mesh + "/pair"], runs["general"][1][mesh + "/pair"]
    assert name_off == "k_patch_hex8_record<K+M,ISO,RPH20,KOFF4096>", name_off
    assert name_on == name_off[:-1] + (",CANON>" if canonical_meshes.EXPECT_CANONICAL[mesh] else ">"), name_on
    # the spread of the general path itself: two runs of the same call
    a_off = runs["general"][0]
    for which in ("M", "K"):
        key = "%s/pair/%s" % (mesh, which)
        print("%-28s two runs under TB_PATCH_CANON=0 differ by %.2e" % (key, rel_err(a_off[key + "/again"], a_off[key])))
        assert rel_err(runs["canon"][0][key + "/again"], a_off[key]) <= 1e-14


def test_single_matrices(runs, reference):
    """K alone and M alone on the pair's plan: the single-block CANON instances (offsets without the mass block's distance)"""
    _check(runs, reference, "box", "alone")
    names = runs["canon"][1]
    assert names["box/K"] == "k_patch_hex8_record<K,ISO,RPH20,CANON>" and names["box/M"] == "k_patch_hex8_record<M,-,RPH20,CANON>", names
    assert "CANON" not in runs["general"][1]["box/K"] + runs["general"][1]["box/M"]


@pytest.mark.parametrize("form", ["diag", "gen"])
def test_tensor_forms(runs, reference, form):
    """the DIAG and the general-tensor instance (indefinite tensors; the isotropic form is the pair test's)"""
    _check(runs, reference, "box", form, form)
    assert runs["canon"][1]["box/" + form] == "k_patch_hex8_record<K+M,%s,RPH20,KOFF4096,CANON>" % INSTANCE[form]
    assert runs["general"][1]["box/" + form] == "k_patch_hex8_record<K+M,%s,RPH20,KOFF4096>" % INSTANCE[form]


def test_graph_replay(runs, reference):
    """the pair call captured once and replayed at two times into zeroed arrays: both launches of the call are in the graph"""
    assert runs["canon"][1]["box/graph_nodes"] == runs["general"][1]["box/graph_nodes"] + 1     # the second class is a launch of its own
    for k in (0, 1):
        _check(runs, reference, "box", "graph%d" % k)
        for which in ("M", "K"):
            a = runs["canon"][0]
            assert rel_err(a["box/graph%d/%s" % (k, which)], a["box/pair/%s" % which]) <= 1e-14


def test_small_plans_keep_one_launch(tb, oracle, device):
    """(in this process: the library's own choice, no switch set) left alone the library splits the classes only from 64 canonical patches per CU on (the second launch waits for the first to drain; measured on
    the 27-layer slab that costs more than 5 292 canonical patches gain): the box here stays on the general instance, and is right"""
    dh = canonical_meshes.build(tb)["box"]
    sp = tb.allocate_matrix(dh)
    st = tb.PatchAssemblyStrategy(device)
    M = tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(RHO)), dh, sp)
    K = tb.setup_operator(st, tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(KAPPA["iso"])), dh, sp)
    tb.update_operators(M, K, 0.0)
    assert tb.lib().tb_last_kernel_name().decode() == "k_patch_hex8_record<K+M,ISO,RPH20,KOFF4096>"
    om = oracle.Mesh(oracle.HEX8, 2, dh.grid.xyz, dh.grid.conn, dh.cell_dofs)
    assert rel_err(M.A.to_host(), oracle.assemble_matrix(om, 0, oracle.Coef(oracle.COEF_CONST_SCALAR, [RHO]), sp.rowptr, sp.colidx)) < TOL
    assert rel_err(K.A.to_host(), oracle.assemble_matrix(om, 1, oracle.Coef(oracle.COEF_CONST_TENSOR, KAPPA["iso"].ravel()), sp.rowptr, sp.colidx)) < TOL

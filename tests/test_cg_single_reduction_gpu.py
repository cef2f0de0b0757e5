"""The single-reduction (Chronopoulos–Gear) DistributedCG on the device path (tb_cg1_update / tb_cg1_fold / tb_cg1_iteration) with HIP-assembled heat
systems A = M − Δt·K: against the classic device solver at one rank (box and ideal ventricle), the one-call form against the separate calls and a
replayed HIP graph against the direct calls (bitwise), two ranks over gloo and three through the C ABI's communicator over the RCCL test double against
one rank, an empty part and an indefinite operator."""
import ctypes as C
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cg1_rccl_child as child  # noqa: E402


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture
def stream_dev(tb):
    """a device of its own on a torch side stream (DistributedCG puts the device on torch's current stream; a graph needs a stream that is not the
    legacy default one)"""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = tb.MI355XDevice(0)
        dev.set_stream(s.cuda_stream)
        yield dev
        torch.cuda.synchronize()


def _one_rank(tb, dev, g, variant, **kw):
    D = tb.distributed
    dh, K, A, diag, b, x0, n2d = child.assemble(tb, dev, g)
    cg = D.DistributedCG(None, diag, None, None, 0, 1, None, device=dev, operator=(K.pattern, A), variant=variant, **kw)
    return cg, b, x0, n2d


def _mesh(tb, name):
    if name == "box":
        return tb.generate_mesh(tb.Hexahedron, (24, 24, 24), (0.0, 0.0, 0.0), (1.0, 1.0, 2.0), perturb=0.2)
    return tb.generate_ideal_lv_mesh_hex(16, 2, 8)


@pytest.mark.parametrize("mesh", ["box", "lv"])
def test_one_rank_equals_classic(tb, stream_dev, mesh):
    g = _mesh(tb, mesh)
    res = {}
    for variant in ("classic", "single_reduction"):
        cg, b, x0, n2d = _one_rank(tb, stream_dev, g, variant)
        assert cg.reductions_per_iteration == (1 if variant == "single_reduction" else 2)
        x50, its50, _ = cg.solve(b, x0.clone(), rtol=0.0, atol=0.0, maxiter=50)
        _, its, rn = cg.solve(b, x0.clone(), rtol=1e-8, atol=0.0, maxiter=1000)
        res[variant] = (x50.cpu().numpy(), its50, its)
    xc, x1 = res["classic"][0], res["single_reduction"][0]
    assert res["classic"][1] == res["single_reduction"][1] == 50
    assert np.linalg.norm(x1 - xc) / np.linalg.norm(xc) <= 1e-10
    assert 5 < res["classic"][2] < 1000 and res["single_reduction"][2] == res["classic"][2]


def _one_call_and_separate(tb, dev, g, iters=25):
    import torch
    cg, b, x0, _ = _one_rank(tb, dev, g, "single_reduction")
    runs = {}
    for one_call in (True, False):
        cg.one_call = one_call
        x = x0.clone()
        st = cg.device_setup1(b, x)
        for _ in range(iters):
            cg.device_step1(x, *st)
        torch.cuda.synchronize()
        runs[one_call] = [t.clone() for t in (x,) + st]
    return cg, b, x0, runs


def test_one_call_equals_separate_calls_to_rounding_on_the_box(tb, stream_dev):
    """24³: the SpMV runs ~1 000 workgroups, so several land on one reduction slot and the order of their atomics — hence the last bits of δ — varies
    from run to run of either form; the two forms agree as two runs of one form do"""
    _, _, _, runs = _one_call_and_separate(tb, stream_dev, _mesh(tb, "box"))
    a, c = runs[True][0].cpu().numpy(), runs[False][0].cpu().numpy()
    assert np.linalg.norm(a - c) / np.linalg.norm(c) <= 1e-10


def test_one_call_equals_separate_calls_and_graph_replay_equals_direct_calls(tb, stream_dev):
    """bitwise on a box small enough that no launch has more than 64 workgroups (one partial per reduction slot: the sums are order-fixed)"""
    import torch
    dev = stream_dev
    g = tb.generate_mesh(tb.Hexahedron, (8, 8, 8), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), perturb=0.2)
    cg, b, x0, runs = _one_call_and_separate(tb, dev, g)
    for a, c in zip(runs[True], runs[False]):
        assert torch.equal(a, c)                                            # bitwise
    # a captured iteration replayed: the same bits as the direct calls from the same state
    cg.one_call = True
    x = x0.clone()
    st = cg.device_setup1(b, x)
    for _ in range(3):                                                       # plans exist before the capture
        cg.device_step1(x, *st)
    torch.cuda.synchronize()
    xg, stg = x.clone(), tuple(t.clone() for t in st)
    gr = dev.capture(lambda: cg.device_step1(xg, *stg))
    assert gr.nodes >= 3
    for _ in range(10):
        cg.device_step1(x, *st)
        gr.launch(0.0)
    torch.cuda.synchronize()
    gr.close()
    for a, c in zip((x,) + st, (xg,) + stg):
        assert torch.equal(a, c)
    assert float(st[-1][2]) > 0.0 and float(st[-1][3]) == 0.0              # ‖r‖² and no breakdown


def test_indefinite_operator_reported_like_classic(tb, stream_dev):
    import torch
    D = tb.distributed
    dev = stream_dev
    g = tb.generate_mesh(tb.Hexahedron, (10, 8, 6), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    dh, K, A, diag, b, x0, n2d = child.assemble(tb, dev, g)

    def neg(v):
        out = torch.zeros_like(v)
        tb._lib.check(tb.lib().tb_spmv_csr(K.pattern.h, A.ptr, v.data_ptr(), -1.0, 0.0, out.data_ptr()))
        return out
    flags = {}
    for variant in ("classic", "single_reduction"):
        cg = D.DistributedCG(neg, -diag, None, None, 0, 1, None, device=dev, look=2, variant=variant)
        with pytest.raises(ArithmeticError):
            cg.solve(b, x0.clone(), rtol=1e-10, atol=0.0, maxiter=50)
        flags[variant] = cg.breakdown
    # the first pᵀAp of both forms is z₀ᵀA z₀ (single-reduction: δ₀ = u₀ᵀA u₀, u₀ = z₀)
    assert flags["classic"] < 0.0
    np.testing.assert_allclose(flags["single_reduction"], flags["classic"], rtol=1e-12)


def test_empty_part(tb, stream_dev):
    """n == 0: accepted by every entry as by tb_cgd_*; the fold keeps γ, α and leaves zero partials; an indefinite iteration raises the flag on an empty
    part too (the breakdown test reads only the all-reduced scalars), so that it stops with its peers"""
    import torch
    dev, L = stream_dev, tb.lib()
    S = torch.tensor([2.0, 4.0, 9.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L.tb_cg1_update(dev.h, 0, None, None, None, None, None, None, None, None, p(S)) == 0
    assert L.tb_cg1_fold(dev.h, p(S)) == 0
    torch.cuda.synchronize()
    assert S.cpu().tolist() == [0.0, 0.0, 0.0, 0.0, 2.0, 0.5, 0.0]         # γ_prev = 2, α_prev = γ/δ = 0.5, the block holds this rank's (zero) partials
    assert L.tb_cg1_update(dev.h, -1, None, None, None, None, None, None, None, None, p(S)) != 0
    assert L.tb_cg1_update(dev.h, 4, None, None, None, None, None, None, None, None, p(S)) != 0
    assert L.tb_cgd_update(dev.h, 0, None, None, None, None, None, None, p(S[0:1]), p(S[1:2]), p(S[2:5])) == 0   # the classic entry: the same
    S2 = torch.tensor([2.0, -4.0, 9.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64, device="cuda")
    assert L.tb_cg1_update(dev.h, 0, None, None, None, None, None, None, None, None, p(S2)) == 0
    torch.cuda.synchronize()
    assert float(S2[3]) == -4.0


def _ranks(mode, world, tmp_path, iters, env=None):
    port = _free_port()
    outs = [str(tmp_path / ("%s_%d.npz" % (mode, r))) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "cg1_rccl_child.py"), mode, str(r), str(world), str(port), outs[r], str(iters)],
                              env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
             for r in range(world)]
    for pr in procs:
        o, e = pr.communicate(timeout=600)
        assert pr.returncode == 0, (o[-1500:], e[-3000:])
    return [dict(np.load(f)) for f in outs]


def _whole_box(tb, dev, iters):
    g = tb.generate_mesh(tb.Hexahedron, child.NEL, child.LEFT, child.RIGHT)
    cg, b, x0, n2d = _one_rank(tb, dev, g, "single_reduction")
    x, its, _ = cg.solve(b, x0.clone(), rtol=0.0, atol=0.0, maxiter=iters)
    return x.cpu().numpy()[n2d], its


def _compare(ref, res, iters):
    seen = np.zeros(len(ref), dtype=int)
    for r in res:
        assert int(r["its"]) == iters
        assert np.linalg.norm(r["x"] - ref[r["gnode"]]) / np.linalg.norm(ref[r["gnode"]]) <= 1e-10
        seen[r["gnode"]] += 1
    assert seen.min() == 1


def test_two_ranks_over_gloo_equal_one_rank(tb, stream_dev, tmp_path):
    iters = 30
    ref, its = _whole_box(tb, stream_dev, iters)
    assert its == iters
    _compare(ref, _ranks("gloo", 2, tmp_path, iters), iters)


def test_three_ranks_through_the_c_abi_over_the_rccl_test_double(tb, stream_dev, tmp_path):
    """tests/mock_rccl stands in for RCCL (three ranks on one GPU): the three ranks leave the one-rank iterate, and each issues exactly one
    tb_comm_allreduce per iteration (plus one in the set-up)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    so = str(tmp_path / "libmockrccl.so")
    bld = subprocess.run([hipcc, "-O1", "-shared", "-fPIC", "-I/opt/rocm/include", "-o", so, os.path.join(ROOT, "tests", "mock_rccl", "mock_rccl.cpp"), "-lrt"],
                         capture_output=True, text=True, timeout=600)
    assert bld.returncode == 0, bld.stderr[-2000:]
    iters = 30
    ref, _ = _whole_box(tb, stream_dev, iters)
    res = _ranks("abi", 3, tmp_path, iters, env={"TB_RCCL_LIBRARY": so})
    _compare(ref, res, iters)
    for r in res:
        assert int(r["allreduces"]) == 1 + iters

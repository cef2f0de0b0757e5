"""The single-reduction (Chronopoulos–Gear) form of DistributedCG on its plain-torch path: the oracle-assembled heat system A = M − Δt·K of a 12³ box,
at one rank and over gloo at two and three ranks (z-slabs).  It must take the iterations the classic form takes — same iterates to rounding — while
issuing ONE all-reduce per iteration where the classic form issues two."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEL = (12, 12, 12)
LEFT, RIGHT = (0.0, 0.0, 0.0), (1.0, 1.0, 2.0)
KAPPA = np.diag([4.5e-2, 2.0e-2, 2.0e-2])
DT = 0.5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class CountingDist:
    """torch.distributed as DistributedCG sees it, with the all-reduces counted"""

    def __init__(self, d):
        self._d, self.all_reduces = d, 0

    def all_reduce(self, *a, **k):
        self.all_reduces += 1
        return self._d.all_reduce(*a, **k)

    def __getattr__(self, name):
        return getattr(self._d, name)


def _problem(world, rank, dist_):
    import thunderbolt_jl_amd as tb
    from oracle import oracle as o
    D = tb.distributed
    part = D.SlabPartition(NEL, LEFT, RIGHT, world, rank)
    g = tb.generate_mesh(tb.Hexahedron, part.local_nel(), part.left, part.right)
    dh = tb.DofHandler(g)
    sp = tb.allocate_matrix(dh)
    om = o.Mesh(o.HEX8, 2, g.xyz, g.conn, dh.cell_dofs)
    n2d = D.node_to_dof(dh)
    lo, up = part.interface_nodes()
    lo_idx = None if lo is None else torch.from_numpy(n2d[lo])
    up_idx = None if up is None else torch.from_numpy(n2d[up])
    Mp = o.assemble_matrix(om, 0, o.Coef(o.COEF_CONST_SCALAR, [1.0]), sp.rowptr, sp.colidx)
    Kp = o.assemble_matrix(om, 1, o.Coef(o.COEF_CONST_TENSOR, KAPPA.ravel()), sp.rowptr, sp.colidx)
    Ap = o.heat_matrix(Mp, Kp, DT)
    diag = torch.from_numpy(np.array([Ap[sp.rowptr[r] + np.searchsorted(sp.colidx[sp.rowptr[r]:sp.rowptr[r + 1]], r)] for r in range(dh.ndofs)]))
    spmv = lambda x: torch.from_numpy(o.spmv_csr(sp.rowptr, sp.colidx, Ap, x.numpy()))  # noqa: E731
    u0 = np.empty(dh.ndofs)
    u0[n2d] = np.cos(2 * g.xyz[:, 0]) * (1 + g.xyz[:, 2])            # consistent initial state
    b = torch.from_numpy(o.spmv_csr(sp.rowptr, sp.colidx, Mp, u0))   # b = M u₀, assembled over the interface
    if world > 1:
        D.halo_sum(b, lo_idx, up_idx, rank, world, dist_)
    x0 = torch.from_numpy(u0)                                        # the previous time step as the initial guess
    gnode = np.arange(g.n_nodes) + part.z0 * part.plane

    def make(variant, negate=False):
        f = (lambda v: -spmv(v)) if negate else spmv
        return D.DistributedCG(f, -diag if negate else diag, lo_idx, up_idx, rank, world, dist_, variant=variant)
    return make, b, x0, gnode, n2d


def _run(world, rank, dist_):
    """everything the tests compare, from one rank's view"""
    make, b, x0, gnode, n2d = _problem(world, rank, dist_)
    out = {"gnode": gnode}
    counter = dist_ if isinstance(dist_, CountingDist) else None
    for variant in ("classic", "single_reduction"):
        cg = make(variant)
        out[variant + "/reductions_per_iteration"] = cg.reductions_per_iteration
        if counter is not None:
            counter.all_reduces = 0
        x, its, _ = cg.solve(b, x0.clone(), rtol=0.0, atol=0.0, maxiter=50)
        out[variant + "/x50"] = x.numpy()[n2d]
        out[variant + "/its50"] = its
        out[variant + "/all_reduces50"] = None if counter is None else counter.all_reduces
        x, its, rn = make(variant).solve(b, x0.clone(), rtol=1e-8, atol=0.0, maxiter=500)
        out[variant + "/its"] = its
        out[variant + "/rn0"] = make(variant).solve(b, x0.clone(), rtol=0.0, atol=0.0, maxiter=0)[2]
        out[variant + "/history"] = [make(variant).solve(b, x0.clone(), rtol=0.0, atol=0.0, maxiter=k)[2] for k in range(1, its + 1)]
        try:
            make(variant, negate=True).solve(b, x0.clone(), rtol=1e-8, atol=0.0, maxiter=50)
            out[variant + "/breakdown"] = False
        except ArithmeticError:
            out[variant + "/breakdown"] = True
    return out


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank, _run(world, rank, CountingDist(dist))))
    except BaseException as ex:                                       # the parent must not wait for a rank that died
        q.put((rank, repr(ex)))
        raise
    finally:
        dist.barrier()
        dist.destroy_process_group()


def _check(res, world):
    """the acceptance criteria on the results of every rank of one run"""
    def glob(key):
        n = (NEL[0] + 1) * (NEL[1] + 1) * (NEL[2] + 1)
        v = np.full(n, np.nan)
        for r in res:
            v[r["gnode"]] = r[key]
        assert not np.isnan(v).any()
        return v
    xc, x1 = glob("classic/x50"), glob("single_reduction/x50")
    assert np.linalg.norm(x1 - xc) / np.linalg.norm(xc) <= 1e-10
    for r in res:
        assert r["classic/its50"] == 50 and r["single_reduction/its50"] == 50
        assert r["classic/reductions_per_iteration"] == 2 and r["single_reduction/reductions_per_iteration"] == 1
        its = r["classic/its"]
        assert 5 < its < 500 and r["single_reduction/its"] == its
        rn0 = r["classic/rn0"]
        np.testing.assert_allclose(r["single_reduction/rn0"], rn0, rtol=1e-13)
        np.testing.assert_allclose(r["single_reduction/history"], r["classic/history"], rtol=0, atol=1e-8 * rn0)
        assert r["classic/breakdown"] and r["single_reduction/breakdown"]
        if world > 1:
            # set-up: classic r·z and ‖r‖² (two), the variant {γ, δ, ρ} (one); then two per iteration against one
            assert r["classic/all_reduces50"] == 2 + 2 * 50
            assert r["single_reduction/all_reduces50"] == 1 + 50


def test_variant_argument_is_checked():
    import thunderbolt_jl_amd as tb
    d = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        tb.distributed.DistributedCG(lambda v: v, d, None, None, 0, 1, None, variant="pipelined")
    assert tb.distributed.DistributedCG(lambda v: v, d, None, None, 0, 1, None).variant == "classic"


def test_single_reduction_equals_classic_one_rank():
    sys.path.insert(0, ROOT)
    _check([_run(1, 0, None)], 1)


@pytest.mark.parametrize("world", [2, 3])
def test_single_reduction_equals_classic_over_gloo_one_all_reduce_per_iteration(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, r in res:
        assert isinstance(r, dict), (rank, r)
    _check([r for _, r in sorted(res, key=lambda t: t[0])], world)

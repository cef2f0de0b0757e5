"""One rank of the single-reduction DistributedCG on a z-slab of a box, every rank on cuda:0 (tests/test_cg_single_reduction_gpu.py starts them).

    python tests/cg1_rccl_child.py <gloo|abi> <rank> <world> <port> <out.npz> <iterations>

gloo: the exchange and the all-reduce through torch.distributed (gloo, buffers staged through the host).  abi: through the C ABI's communicator
(tb_comm_*), whose RCCL library TB_RCCL_LIBRARY names — the test double of tests/mock_rccl on a one-GPU box; the communicator id travels over the gloo
group.  Writes x by global node, the iteration count and the number of tb_comm_allreduce calls (abi) to <out.npz>."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEL = (12, 10, 18)
LEFT, RIGHT = (0.0, 0.0, 0.0), (1.0, 1.0, 2.0)
KAPPA = np.diag([4.5e-2, 2.0e-2, 2.0e-2])
DT = 0.5


def assemble(tb, dev, g):
    """HIP-assembled heat system A = M − Δt·K, its diagonal, b = M·u₀ (local) and the consistent u₀ of the nodal field below"""
    import torch
    D = tb.distributed
    dh = tb.DofHandler(g)
    sp = tb.allocate_matrix(dh)
    st = tb.PatchAssemblyStrategy(dev)
    M = tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp)
    K = tb.setup_operator(st, tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(KAPPA)), dh, sp)
    tb.update_operators(M, K, 0.0)
    A = tb.heat_system_matrix(dev, M, K, DT)
    diag = torch.empty(dh.ndofs, dtype=torch.float64, device="cuda")
    tb._lib.check(tb.lib().tb_extract_diagonal(K.pattern.h, A.ptr, diag.data_ptr()))
    n2d = D.node_to_dof(dh)
    u0 = np.empty(dh.ndofs)
    u0[n2d] = np.cos(2 * g.xyz[:, 0]) * (1 + g.xyz[:, 2]) + g.xyz[:, 1] ** 2
    x0 = torch.from_numpy(u0).cuda()
    b = torch.zeros_like(x0)
    M.mul(tb.DeviceVector.wrap(dev, b), tb.DeviceVector.wrap(dev, x0))
    return dh, K, A, diag, b, x0, n2d


def main():
    mode, rank, world, port, out, iters = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], int(sys.argv[6])
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = port
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import thunderbolt_jl_amd as tb
    D = tb.distributed
    torch.cuda.set_device(0)
    torch.cuda.set_stream(torch.cuda.Stream())
    dev = tb.MI355XDevice(0)
    dev.set_stream(torch.cuda.current_stream().cuda_stream)
    calls = [0]

    class CountingComm(D.RcclComm):
        def allreduce(self, t, op="sum"):
            calls[0] += 1
            return super().allreduce(t, op)

    xd = CountingComm.from_torch(dev, dist) if mode == "abi" else dist
    part = D.SlabPartition(NEL, LEFT, RIGHT, world, rank)
    g = tb.generate_mesh(tb.Hexahedron, part.local_nel(), part.left, part.right)
    dh, K, A, diag, b, x0, n2d = assemble(tb, dev, g)
    lo, up = part.interface_nodes()
    lo_idx = None if lo is None else torch.from_numpy(n2d[lo]).cuda()
    up_idx = None if up is None else torch.from_numpy(n2d[up]).cuda()
    nb = D.slab_neighbours(lo_idx, up_idx, rank, world)
    D.HaloExchange(nb, xd, b, dev).exchange_sum(b)
    cg = D.DistributedCG(None, diag, lo_idx, up_idx, rank, world, xd, device=dev, operator=(K.pattern, A), variant="single_reduction")
    calls[0] = 0
    x, its, rn = cg.solve(b, x0.clone(), rtol=0.0, atol=0.0, maxiter=iters)
    torch.cuda.synchronize()
    np.savez(out, gnode=np.arange(g.n_nodes) + part.z0 * part.plane, x=x.cpu().numpy()[n2d], its=its, allreduces=calls[0])
    dist.barrier()
    if mode == "abi":
        xd.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

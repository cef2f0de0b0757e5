// tb_amg_block.hip — the smoothed aggregation of tb_amg.hip with a near-null-space of k ≤ 6 candidates on node blocks (Vaněk–Mandel–Brezina; the
// method as include/tbhip.h states it): candidates' zero rows, Frobenius strength of the node blocks, the per-aggregate QR that gives the tentative
// prolongator T and the candidates of the level below, the smoothed prolongator on dense T, and the unit diagonal of dead coarse dofs.  The host loop,
// λmax, the two products, the cycle and the last level are tb_amg.hip's.  No kernel uses a floating-point atomic; every sum has one order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "tb_amg_block_planners.hpp"
#include "tb_amg_internal.hpp"
#include "tb_amg_qr.hpp"
#include "tb_internal.h"
#include "tb_reduce.hpp"

namespace tb {

// step 1: a dof whose row has no non-zero off-diagonal entry is an eliminated Dirichlet dof: its row of B is zero
__global__ void __launch_bounds__(256)
k_amg_block_candidates(int64_t n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ A, int k, double *__restrict__ B)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool coupled = false;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1] && !coupled; ++e) coupled = colidx[e] != (int32_t)i && A[e] != 0.0;
    if (coupled) return;
    for (int c = 0; c < k; ++c) B[i * k + c] = 0.0;
}

// step 2: s_IJ = Frobenius norm of the entries of A between nodes I and J, the squares summed in stored row-major order; one work item per non-zero of
// the node graph
__global__ void __launch_bounds__(256)
k_amg_block_norm(int64_t gnnz, const int64_t *__restrict__ entry_ptr, const int64_t *__restrict__ entries, const double *__restrict__ A, double *__restrict__ s)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= gnnz) return;
    double sum = 0.0;
    for (int64_t p = entry_ptr[q]; p < entry_ptr[q + 1]; ++p) {
        const double a = A[entries[p]];
        sum = fma(a, a, sum);
    }
    s[q] = sqrt(sum);
}

// step 4: one wave per aggregate; the block B_a is copied into the aggregate's rows of T and factored there (every lane reads and writes its own rows
// only, the sums cross lanes by the butterfly of tb_amg_qr.hpp).  R_a goes to rows k·a … of B_{l+1}, the dead flags to dead[k·a …].
struct QrRows {
    double *T;
    const int32_t *dof;
    int k;
    __device__ __forceinline__ double get(int p, int c) const { return T[(int64_t)dof[p] * k + c]; }
    __device__ __forceinline__ void set(int p, int c, double v) { T[(int64_t)dof[p] * k + c] = v; }
};
struct WaveExec {
    int lane;
    template <class F>
    __device__ __forceinline__ double sum(F f)
    {
        double v = f(lane);
#pragma unroll
        for (int o = amgqr::LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, amgqr::LANES);
        return v;
    }
    template <class F>
    __device__ __forceinline__ void each(F f) { f(lane); }
};
__global__ void __launch_bounds__(64)
k_amg_block_qr(int64_t na, int k, const int64_t *__restrict__ adof_ptr, const int32_t *__restrict__ adof, const double *__restrict__ B, double *__restrict__ T,
               double *__restrict__ Bc, uint8_t *__restrict__ dead)
{
    const int64_t a = blockIdx.x;
    if (a >= na) return;
    const int lane = threadIdx.x;
    const int32_t *dof = adof + adof_ptr[a];
    const int m = (int)(adof_ptr[a + 1] - adof_ptr[a]);
    for (int p = lane; p < m; p += amgqr::LANES)
        for (int c = 0; c < k; ++c) T[(int64_t)dof[p] * k + c] = B[(int64_t)dof[p] * k + c];
    QrRows w{T, dof, k};
    WaveExec x{lane};
    double R[amgqr::MAX_K * amgqr::MAX_K];
    uint8_t dd[amgqr::MAX_K];
    amgqr::factor(w, m, k, x, R, dd);
    if (lane < k) {
        for (int c = 0; c < k; ++c) Bc[(a * k + lane) * k + c] = R[lane * k + c];
        dead[a * k + lane] = dd[lane];
    }
}

// step 5: P_iq = T_iq − ω d_i Σ_e a_ie T_eq over the columns e of row i whose node's aggregate is q / k, in stored order; one work item per non-zero of P
__global__ void __launch_bounds__(256)
k_amg_block_smooth_p(int64_t pnnz, const int32_t *__restrict__ prow, const int32_t *__restrict__ pcol, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                     const double *__restrict__ A, const int32_t *__restrict__ agg, int k, const double *__restrict__ T, const double *__restrict__ dinv, double omega,
                     double *__restrict__ P)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= pnnz) return;
    const int32_t i = prow[q], J = pcol[q] / k, c = pcol[q] - J * k;
    double s = 0.0;
    for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int32_t j = colidx[e];
        if (agg[j] == J) s += A[e] * T[(int64_t)j * k + c];
    }
    P[q] = (agg[i] == J ? T[(int64_t)i * k + c] : 0.0) - omega * dinv[i] * s;
}

// step 6: the diagonal of A_c at a dead coarse dof is 1 (its row and column are zero: the column of P is)
__global__ void __launch_bounds__(256) k_amg_dead_diag(int64_t nc, const uint8_t *__restrict__ dead, const int64_t *__restrict__ diag, double *__restrict__ A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nc && dead[i] && diag[i] >= 0) A[diag[i]] = 1.0;
}

template <class T>
static void free_dev(T *&p)
{
    if (p) (void)hipFree((void *)p);
    p = nullptr;
}

void amg_block_free_level(AmgLevel &L)
{
    free_dev(L.d_B); free_dev(L.d_T); free_dev(L.d_Bc); free_dev(L.d_dead); free_dev(L.d_adofptr); free_dev(L.d_adof);
}

int amg_block_plan(tb_amg *amg, int l)
{
    tb_device *dev = amg->dev;
    AmgLevel &L = amg->lv[(size_t)l];
    const int64_t n = L.n, nnz = L.nnz;
    const int k = amg->nns_k;
    const int64_t *hp = l == 0 ? amg->pat->h_rowptr.data() : L.h_rowptr.data();
    const int32_t *hc = l == 0 ? amg->pat->h_colidx.data() : L.h_colidx.data();
    hipLaunchKernelGGL(k_amg_block_candidates, dim3(blocks_of(n, 256)), dim3(256), 0, dev->stream, n, L.rowptr, L.colidx, L.A, k, L.d_B);
    amgplan::NodeGraph g;
    amgplan::node_graph(n, hp, hc, L.h_node.data(), L.n_nodes, g);
    const int64_t gnnz = (int64_t)g.col.size();
    int64_t *d_gptr = nullptr, *d_eptr = nullptr, *d_ent = nullptr;
    int32_t *d_gcol = nullptr;
    double *d_s = nullptr;
    uint8_t *d_flag = nullptr;
    std::vector<uint8_t> flag((size_t)gnnz);
    auto run = [&]() -> int {
        TB_TRY(upload_all(dev, g.ptr, &d_gptr, g.col, &d_gcol, g.entry_ptr, &d_eptr, g.entries, &d_ent));
        TB_HIP(hipMalloc((void **)&d_s, sizeof(double) * (size_t)std::max<int64_t>(gnnz, 1)));
        TB_HIP(hipMalloc((void **)&d_flag, (size_t)std::max<int64_t>(gnnz, 1)));
        hipLaunchKernelGGL(k_amg_block_norm, dim3(blocks_of(gnnz, 256)), dim3(256), 0, dev->stream, gnnz, (const int64_t *)d_eptr, (const int64_t *)d_ent, L.A, d_s);
        launch_amg_strength(dev, L.n_nodes, d_gptr, d_gcol, d_s, nullptr, amg->theta, L.w, d_flag); // (n_nodes ≤ n doubles of the level's scratch)
        TB_HIP(hipMemcpyAsync(flag.data(), d_flag, (size_t)gnnz, hipMemcpyDeviceToHost, dev->stream));
        TB_SYNC_STREAM(dev);
        return TB_OK;
    };
    const int rc = run();
    free_dev(d_gptr); free_dev(d_gcol); free_dev(d_eptr); free_dev(d_ent); free_dev(d_s); free_dev(d_flag);
    if (rc) return rc;
    L.h_strength.resize((size_t)nnz);
    for (int64_t e = 0; e < nnz; ++e) L.h_strength[(size_t)e] = flag[(size_t)g.nz_of_entry[(size_t)e]];
    amgplan::plan_block_level(n, hp, hc, L.h_node.data(), g, flag.data(), k, L.bplan);
    L.plan = std::move(L.bplan.L);
    L.bplan.L = amgplan::LevelPlan();
    return TB_OK;
}

int amg_block_tentative(tb_amg *amg, int l)
{
    tb_device *dev = amg->dev;
    AmgLevel &L = amg->lv[(size_t)l];
    const int k = amg->nns_k;
    const int64_t na = L.bplan.n_agg, nc = L.plan.nc;
    TB_TRY(upload_all(dev, L.bplan.adof_ptr, &L.d_adofptr, L.bplan.adof, &L.d_adof));
    TB_HIP(hipMalloc((void **)&L.d_T, sizeof(double) * (size_t)std::max<int64_t>(L.n * k, 1)));
    TB_HIP(hipMalloc((void **)&L.d_Bc, sizeof(double) * (size_t)std::max<int64_t>(nc * k, 1)));
    TB_HIP(hipMalloc((void **)&L.d_dead, (size_t)std::max<int64_t>(nc, 1)));
    TB_HIP(hipMemsetAsync(L.d_T, 0, sizeof(double) * (size_t)(L.n * k), dev->stream)); // rows outside every aggregate stay zero
    hipLaunchKernelGGL(k_amg_block_qr, dim3((unsigned)na), dim3(amgqr::LANES), 0, dev->stream, na, k, (const int64_t *)L.d_adofptr, (const int32_t *)L.d_adof,
                       (const double *)L.d_B, L.d_T, L.d_Bc, L.d_dead);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

void amg_block_smooth_p(tb_amg *amg, int l, double omega)
{
    AmgLevel &L = amg->lv[(size_t)l];
    hipLaunchKernelGGL(k_amg_block_smooth_p, dim3(blocks_of(L.pnnz, 256)), dim3(256), 0, amg->dev->stream, L.pnnz, (const int32_t *)L.d_prow, (const int32_t *)L.d_pcol,
                       L.rowptr, L.colidx, L.A, (const int32_t *)L.d_agg, amg->nns_k, (const double *)L.d_T, (const double *)L.dinv, omega, L.d_P);
}

void amg_block_dead_diag(tb_amg *amg, int l)
{
    AmgLevel &L = amg->lv[(size_t)l], &N = amg->lv[(size_t)l + 1];
    hipLaunchKernelGGL(k_amg_dead_diag, dim3(blocks_of(N.n, 256)), dim3(256), 0, amg->dev->stream, N.n, (const uint8_t *)L.d_dead, (const int64_t *)N.d_diag, N.d_A);
}

} // namespace tb

using namespace tb;

int tb_amg_set_near_nullspace(tb_amg *amg, int64_t n_nodes, const int32_t *node_of_dof, int k, const double *B)
{
    TB_REQUIRE(amg && node_of_dof && B, "tb_amg_set_near_nullspace: NULL argument");
    TB_REQUIRE(!amg->planned, "tb_amg_set_near_nullspace: the hierarchy is planned; the near-null-space changes before the first tb_amg_setup or after tb_amg_replan");
    TB_REQUIRE(!amg->products, "tb_amg_set_near_nullspace: not on the hierarchy of a block system");
    TB_REQUIRE(k >= 1 && k <= amgqr::MAX_K, "tb_amg_set_near_nullspace: k = %d candidates; 1 to %d are supported", k, amgqr::MAX_K);
    const int64_t n = amg->pat->n_rows;
    std::string err;
    if (amgplan::check_nodes(n, node_of_dof, n_nodes, 3, err)) {
        set_error("tb_amg_set_near_nullspace: %s (level 0 has 3 dofs per node)", err.c_str());
        return TB_ERR_BAD_ARG;
    }
    for (int64_t i = 0; i < n * k; ++i)
        if (!std::isfinite(B[i])) {
            set_error("tb_amg_set_near_nullspace: B holds a non-finite value at dof %lld, candidate %d", (long long)(i / k), (int)(i % k));
            return TB_ERR_BAD_ARG;
        }
    amg->nns_k = k;
    amg->nns_nodes = n_nodes;
    amg->nns_node.assign(node_of_dof, node_of_dof + n);
    amg->nns_B.assign(B, B + n * k);
    amg->comp.clear(); // the node blocks carry no component labels
    return TB_OK;
}

#define AMG_BLOCK_LEVEL(fn, fine)                                                                                                                   \
    TB_REQUIRE(amg, fn ": NULL argument");                                                                                                          \
    TB_REQUIRE(amg->ready, fn ": no numeric setup yet (tb_amg_setup)");                                                                             \
    TB_REQUIRE(amg->nns_k > 0, fn ": the hierarchy has no near-null-space (tb_amg_set_near_nullspace)");                                            \
    TB_REQUIRE(level >= 0 && level < (int)amg->lv.size() - (fine ? 1 : 0), fn ": level %d of %d%s", level, (int)amg->lv.size(),                     \
               fine ? " (the last level has no tentative prolongator)" : "");                                                                       \
    AmgLevel &L = amg->lv[(size_t)level];                                                                                                           \
    TB_NO_CAPTURE(amg->dev);                                                                                                                        \
    TB_HIP(hipSetDevice(amg->dev->id))

template <class T>
static int fetch(tb_device *dev, T *host, const T *d_src, size_t count)
{
    if (!host || !count) return TB_OK;
    TB_HIP(hipMemcpyAsync(host, d_src, count * sizeof(T), hipMemcpyDeviceToHost, dev->stream));
    TB_SYNC_STREAM(dev);
    return TB_OK;
}

int tb_amg_level_nodes(tb_amg *amg, int level, int64_t *n_nodes, int32_t *node_of_dof)
{
    AMG_BLOCK_LEVEL("tb_amg_level_nodes", false);
    if (n_nodes) *n_nodes = L.n_nodes;
    if (node_of_dof) memcpy(node_of_dof, L.h_node.data(), sizeof(int32_t) * (size_t)L.n);
    return TB_OK;
}

int tb_amg_level_near_nullspace(tb_amg *amg, int level, int *k, double *B)
{
    AMG_BLOCK_LEVEL("tb_amg_level_near_nullspace", false);
    if (k) *k = amg->nns_k;
    return fetch(amg->dev, B, (const double *)L.d_B, (size_t)(L.n * amg->nns_k));
}

int tb_amg_level_tentative(tb_amg *amg, int level, double *T)
{
    AMG_BLOCK_LEVEL("tb_amg_level_tentative", true);
    TB_REQUIRE(T, "tb_amg_level_tentative: NULL argument");
    return fetch(amg->dev, T, (const double *)L.d_T, (size_t)(L.n * amg->nns_k));
}

int tb_amg_level_dead(tb_amg *amg, int level, uint8_t *dead)
{
    AMG_BLOCK_LEVEL("tb_amg_level_dead", true);
    TB_REQUIRE(dead, "tb_amg_level_dead: NULL argument");
    return fetch(amg->dev, dead, (const uint8_t *)L.d_dead, (size_t)L.nc);
}

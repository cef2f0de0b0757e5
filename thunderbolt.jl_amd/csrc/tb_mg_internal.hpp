// tb_mg_internal.hpp — what tb_multigrid.hip shares with the units that build on its hierarchy (tb_bidomain_mg.hip: the block V-cycle of the bidomain
// system reuses the scalar hierarchy's transfers and its unflagged per-dof Galerkin term lists): the level record, the hierarchy object, the symbolic
// phase and the launchers of the kernels that work on a plan.  Nothing here changes what tb_mg_* computes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "tb_internal.h"

namespace tb {

constexpr int MG_COARSEST_MAX = 1024; // dofs of the coarsest level: its inverse is dense

struct MgLevel {
    tb_pattern *pat = nullptr;
    int64_t n = 0, nnz = 0;
    double *d_A = nullptr;          // the level's operator: owned below the finest level
    const double *A = nullptr;      // what the cycle reads (finest: the caller's array of the latest setup)
    double *d_vec = nullptr;        // dinv | d | w | x | r (x, r: below the finest level) and, during setup, the Lanczos scratch
    double *dinv = nullptr, *d = nullptr, *w = nullptr, *x = nullptr, *r = nullptr;
    uint8_t *d_presc = nullptr;     // flags of the level's prescribed dofs (NULL: none)
    std::vector<uint8_t> h_presc;
    double lmax = 0.0;
    // to the level below (levels ≥ 1)
    std::vector<int64_t> parent_ptr;
    std::vector<int32_t> parent_idx;
    bool has_transfer = false, p_transfer = false; // p_transfer: the level below carries the first-order field on the same cells (tb_mg_set_p_transfer)
    bool blocked = false;           // the Galerkin plan to the level below is per 3 × 3 block (k_mg_galerkin_b3)
    int32_t *d_brow = nullptr;      // block row of every 3 × 3 block of the level's pattern (levels on either side of a blocked plan)
    int64_t *d_pptr = nullptr, *d_rptr = nullptr, *d_gptr = nullptr, *d_cdiag = nullptr;
    int32_t *d_pcol = nullptr, *d_rcol = nullptr;
    uint8_t *d_pexp = nullptr, *d_rexp = nullptr;
    uint32_t *d_gterms = nullptr;
    int64_t n_terms = 0;
};

// 2^−e for e in 0…7 without a table: the exponent field of 1.0 lowered by e
__device__ __forceinline__ double pow2_neg(unsigned e) { return __longlong_as_double((long long)(1023u - e) << 52); }

// C ← C⁻¹ in place, dense n × n, by Gauss–Jordan elimination without pivoting, symmetrised at the end: the body of k_mg_dense_inverse once C holds the
// operator.  One workgroup; rows go to its waves, columns to the lanes; the workgroup's barriers order the global-memory phases.
__device__ __forceinline__ void mg_gauss_jordan(int n, double *__restrict__ C)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int k = 0; k < n; ++k) {
        const double piv = 1.0 / C[(size_t)k * n + k];
        for (int i = wv; i < n; i += nw) {
            if (i == k) continue;
            const double f = C[(size_t)i * n + k] * piv;
            for (int j = lane; j < n; j += 64)
                if (j != k) C[(size_t)i * n + j] -= f * C[(size_t)k * n + j];
        }
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += blockDim.x)
            if (j != k) { C[(size_t)k * n + j] *= piv; C[(size_t)j * n + k] *= -piv; }
        if (threadIdx.x == 0) C[(size_t)k * n + k] = piv;
        __syncthreads();
    }
    for (int i = wv; i < n; i += nw)
        for (int j = i + 1 + lane; j < n; j += 64) {
            const double s = 0.5 * (C[(size_t)i * n + j] + C[(size_t)j * n + i]);
            C[(size_t)i * n + j] = s; C[(size_t)j * n + i] = s;
        }
}

// tb_multigrid.hip
int build_plans(tb_mg *mg);                                                                  // symbolic phase (tb_mg_setup runs it on its first call): transfers, Galerkin plans, level storage
void launch_galerkin_plane(tb_mg *mg, int fine_level, const double *Af, double *Ac);        // Ac = Pᵀ Af P on the per-dof plan of fine_level, nothing else (no diagonal fill); enqueues only
void launch_dense_apply(tb_device *dev, int n, const double *C, const double *r, double *x); // x = C r, dense: one wavefront per row; enqueues only

} // namespace tb

struct tb_mg {
    tb_device *dev = nullptr;
    std::vector<tb::MgLevel> lv;
    bool planned = false, ready = false;
    int degree = 2;
    double ratio = 4.0;
    double *d_cinv = nullptr; // dense inverse of the coarsest operator
    double *d_scal = nullptr; // two scalars of the λmax estimate
    // tb_mg_set_coarse_amg: level 0 is solved by one cycle of a smoothed-aggregation hierarchy (tb_amg.hip) instead of the dense inverse
    bool coarse_amg = false;
    double amg_theta = 0.25;
    int amg_max_coarse = tb::MG_COARSEST_MAX, amg_max_levels = 16;
    struct tb_amg *amg = nullptr;
};

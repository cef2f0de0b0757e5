// tb_mg_internal.hpp — what tb_multigrid.hip shares with the units of the multigrid family.  tb_bidomain_mg.hip (the block V-cycle of the bidomain system)
// reuses the scalar hierarchy's transfers and its unflagged per-dof Galerkin term lists: the level record, the hierarchy object, the symbolic phase
// and the launchers of the kernels that work on a plan.  tb_amg.hip, tb_bidomain_mg.hip and the Chebyshev preconditioner of tb_krylov.hip share the
// pieces that exist once: the Chebyshev schedule and the scalar smoother around k_mg_cheb, the level's vector block, the dense inverse, the diagonal
// fill, the fold of per-workgroup partials and the argument checks.  The kernels live in tb_multigrid.hip behind the enqueue-only launchers below.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "tb_internal.h"

namespace tb {

constexpr int MG_COARSEST_MAX = 1024; // dofs of the coarsest level: its inverse is dense

// the vectors of a scalar level in one allocation: dinv | d | w | x | r | a sixth (the λmax estimates of setup borrow d, w, x, r and the sixth: none
// of them holds anything between applications)
struct MgVectors {
    double *d_vec = nullptr;
    double *dinv = nullptr, *d = nullptr, *w = nullptr, *x = nullptr, *r = nullptr;
    int alloc(int64_t n)
    {
        TB_HIP(hipMalloc((void **)&d_vec, sizeof(double) * 6 * (size_t)std::max<int64_t>(n, 1)));
        dinv = d_vec; d = dinv + n; w = d + n; x = w + n; r = x + n;
        return TB_OK;
    }
    void release()
    {
        if (d_vec) (void)hipFree(d_vec);
        d_vec = dinv = d = w = x = r = nullptr;
    }
};

struct MgLevel : MgVectors {
    tb_pattern *pat = nullptr;
    int64_t n = 0, nnz = 0;
    double *d_A = nullptr;          // the level's operator: owned below the finest level
    const double *A = nullptr;      // what the cycle reads (finest: the caller's array of the latest setup)
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

// The coefficients of the Chebyshev iteration on [lmax / ratio, lmax] (Saad, Iterative Methods, Alg. 12.1), step by step: first() belongs to the step
// that starts the recurrence (d = c2·D⁻¹(r − A x)), every next() to one further step (d = c1·d + c2·D⁻¹(r − A x)).
struct ChebSchedule {
    struct Step { double c1, c2; };
    double theta, delta, sigma1, rho;
    ChebSchedule(double lmax, double ratio)
    {
        const double lmin = lmax / ratio;
        theta = 0.5 * (lmax + lmin); delta = 0.5 * (lmax - lmin); sigma1 = theta / delta;
        rho = 1.0 / sigma1;
    }
    Step first() const { return Step{0.0, 1.0 / theta}; }
    Step next()
    {
        const double rho_new = 1.0 / (2.0 * sigma1 - rho);
        const Step s{rho_new * rho, 2.0 * rho_new / delta};
        rho = rho_new;
        return s;
    }
};

// tb_multigrid.hip: enqueue-only launchers of the kernels the family shares
void launch_cheb_step(tb_device *dev, int mode, int64_t n, ChebSchedule::Step c, const double *dinv, const double *r, const double *w, double *d, double *x); // k_mg_cheb<mode>
// C = A⁻¹ of a CSR with n ≤ MG_COARSEST_MAX rows.  general = false: no pivoting, symmetrised (a symmetric positive definite level).  general = true:
// partial pivoting, nothing symmetrised (any non-singular level); the kernel leaves 0, or 1 + the elimination step whose pivot was zero or not
// finite, in the device's read-back line, and dense_inverse_status reads it.
void launch_dense_inverse(tb_device *dev, int n, const int64_t *rowptr, const int32_t *colidx, const double *nz, double *C, bool general = false);
int dense_inverse_status(tb_device *dev, const char *who, int level, int n); // after a general launch_dense_inverse: TB_ERR_BAD_ARG and a message naming `who` and the level on a failed pivot; reads back
void launch_fill_diag(tb_device *dev, int64_t n, const int64_t *diagpos, const uint8_t *flags, double *A); // flagged diagonals ← mean |diagonal| of the others
void launch_fold_sum(tb_device *dev, int nb, const double *part, double *out);                              // *out = Σ part[0 … nb) in one fixed order
void launch_fold_max(tb_device *dev, int nb, const double *part, double *out);                              // *out = max part[0 … nb), part ≥ 0

// `degree` steps of the Chebyshev–Jacobi smoother for A x = r on the vectors v (dinv filled; d, w scratch) of n dofs, from x = 0 (no product before the
// first step) or from the x given.  product(x, y) enqueues y = A x and returns a status.  Enqueues only.
template <class Product>
int cheb_smooth(tb_device *dev, int64_t n, const MgVectors &v, double lmax, double ratio, int degree, const double *r, double *x, bool from_zero, Product product)
{
    ChebSchedule s(lmax, ratio);
    if (from_zero) launch_cheb_step(dev, 0, n, s.first(), v.dinv, r, nullptr, v.d, x);
    else {
        TB_TRY(product((const double *)x, v.w));
        launch_cheb_step(dev, 1, n, s.first(), v.dinv, r, v.w, v.d, x);
    }
    for (int k = 1; k < degree; ++k) {
        TB_TRY(product((const double *)x, v.w));
        launch_cheb_step(dev, 2, n, s.next(), v.dinv, r, v.w, v.d, x);
    }
    return TB_OK;
}

// the argument checks of the set-up entries (`who`: the entry's name)
inline int check_smoother_args(const char *who, int degree, double ratio)
{
    TB_REQUIRE(degree >= 1 && degree <= 64, "%s: smoother degree must be in 1..64 (got %d)", who, degree);
    TB_REQUIRE(ratio > 1.0 && std::isfinite(ratio), "%s: interval_ratio must be a finite number above 1 (got %g)", who, ratio);
    return TB_OK;
}
inline int check_amg_args(const char *who, double theta, int max_coarse, int max_levels)
{
    TB_REQUIRE(theta >= 0.0 && theta <= 1.0, "%s: theta must be in 0..1 (got %g)", who, theta);
    TB_REQUIRE(max_coarse >= 1, "%s: max_coarse must be positive (got %d)", who, max_coarse);
    TB_REQUIRE(max_levels >= 1 && max_levels <= 64, "%s: max_levels must be in 1..64 (got %d)", who, max_levels);
    return TB_OK;
}

int build_plans(tb_mg *mg);                                                                  // symbolic phase (tb_mg_setup runs it on its first call): transfers, Galerkin plans, level storage
void launch_galerkin_plane(tb_mg *mg, int fine_level, const double *Af, double *Ac);        // Ac = Pᵀ Af P on the per-dof plan of fine_level, nothing else (no diagonal fill); enqueues only
void launch_dense_apply(tb_device *dev, int n, const double *C, const double *r, double *x); // x = C r, dense: one wavefront per row; enqueues only

} // namespace tb

struct tb_mg {
    tb_device *dev = nullptr;
    std::vector<tb::MgLevel> lv;
    bool planned = false, ready = false;
    bool general = false;     // tb_mg_set_general: the operator need not be symmetric — the coarsest inverse is pivoted and not symmetrised
    int degree = 2;
    double ratio = 4.0;
    double *d_cinv = nullptr; // dense inverse of the coarsest operator
    double *d_scal = nullptr; // two scalars of the λmax estimate
    // tb_mg_set_coarse_amg: level 0 is solved by one cycle of a smoothed-aggregation hierarchy (tb_amg.hip) instead of the dense inverse
    bool coarse_amg = false;
    double amg_theta = 0.25;
    int amg_nns_k = 0;                   // tb_mg_set_coarse_amg_near_nullspace: handed to that hierarchy when it is created (0: none)
    int64_t amg_nns_nodes = 0;
    std::vector<int32_t> amg_nns_node;
    std::vector<double> amg_nns_B;
    int amg_max_coarse = tb::MG_COARSEST_MAX, amg_max_levels = 16;
    struct tb_amg *amg = nullptr;
};

// tb_amg.hip — smoothed-aggregation algebraic multigrid (SmoothedAggregationCoarseSolver, the default pcoarse_solver of the reference's PMGPrecon:
// src/solver/linear/multigrid.jl:27): a preconditioner that needs only the matrix.  Per level: strength of connection (device) → aggregates and
// patterns (tb_amg_planners.cpp, host, flags only) → smoothed prolongator P = T − ω D⁻¹ A T, R = Pᵀ, A_c = R (A P) (device, on planned patterns) → a
// V-cycle on the smoother, dense inverse, dense product and partial fold of tb_multigrid.hip (cheb_smooth, launch_dense_inverse, launch_dense_apply,
// launch_fold_*: tb_mg_internal.hpp).  Level 0 is the caller's matrix on its tb_pattern (products by launch_spmv); the levels below are bare CSRs
// owned here (k_amg_spmv).
// Every sum has one recorded order and no kernel uses a floating-point atomic: two setups, and two applications, give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "tb_amg_internal.hpp"
#include "tb_amg_planners.hpp"
#include "tb_internal.h"
#include "tb_mg_internal.hpp"
#include "tb_reduce.hpp"

namespace tb {

// ---- strength of connection ----
// m_i = max |a_ij| over j ≠ i of i's component (0: none)
__global__ void __launch_bounds__(256)
k_amg_rowmax(int64_t n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ A, const int8_t *__restrict__ comp,
             double *__restrict__ m)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ci = comp ? comp[i] : 0;
    double s = 0.0;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = colidx[k];
        if (j != i && (comp ? comp[j] : 0) == ci) s = fmax(s, fabs(A[k]));
    }
    m[i] = s;
}

// flag(i, j) = strong from i or strong from j; strong from i: m_i > 0 and |a_ij| ≥ θ·m_i (one multiply, one compare).  Entry (j, i) by binary search in
// row j (sorted columns, symmetric pattern: tb_amg_create checks both; a miss leaves the flag to i alone).
__global__ void __launch_bounds__(256)
k_amg_strength(int64_t n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ A, const int8_t *__restrict__ comp,
               const double *__restrict__ m, double theta, uint8_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ci = comp ? comp[i] : 0;
    const double ti = theta * m[i];
    const bool live_i = m[i] > 0.0;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = colidx[k];
        uint8_t f = 0;
        if (j != i && (comp ? comp[j] : 0) == ci) {
            if (live_i && fabs(A[k]) >= ti) f = 1;
            else if (m[j] > 0.0) {
                int64_t lo = rowptr[j], hi = rowptr[j + 1];
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (colidx[mid] < (int32_t)i) lo = mid + 1; else hi = mid;
                }
                const double tj = theta * m[j];
                if (lo < rowptr[j + 1] && colidx[lo] == (int32_t)i && fabs(A[lo]) >= tj) f = 1;
            }
        }
        flag[k] = f;
    }
}

// ---- numeric phase ----
// D⁻¹ of the smoother and of P's smoothing step: 1 / a_ii, 0 where no diagonal is stored or it is zero
__global__ void __launch_bounds__(256) k_amg_dinv(int64_t n, const int64_t *__restrict__ diag, const double *__restrict__ A, double *__restrict__ dinv)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t k = diag[i];
    const double a = k >= 0 ? A[k] : 0.0;
    dinv[i] = a != 0.0 ? 1.0 / a : 0.0;
}

// P_iJ = T_iJ − ω d_i Σ_k a_ik T_kJ: one work item per non-zero (i, J) of P, the sum over the k of row i with agg(k) = J in stored order
__global__ void __launch_bounds__(256)
k_amg_smooth_p(int64_t pnnz, const int32_t *__restrict__ prow, const int32_t *__restrict__ pcol, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
               const double *__restrict__ A, const int32_t *__restrict__ agg, const double *__restrict__ tval, const double *__restrict__ dinv, double omega,
               double *__restrict__ P)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= pnnz) return;
    const int32_t i = prow[q], J = pcol[q];
    const double t = tval[J];
    double s = 0.0;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
        if (agg[colidx[k]] == J) s += A[k] * t;
    P[q] = (agg[i] == J ? t : 0.0) - omega * dinv[i] * s;
}

__global__ void __launch_bounds__(256) k_amg_gather(int64_t n, const int64_t *__restrict__ perm, const double *__restrict__ src, double *__restrict__ dst)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) dst[q] = src[perm[q]];
}

// C = A·B on the planned pattern of C: one work item per non-zero (i, j) of C walks row i of A in stored order and finds b_kj by binary search in row k
// of B (sorted columns) — ordered by construction, no plan memory beyond C's pattern.  Used twice per level: A·P, then R·(A·P).
__global__ void __launch_bounds__(256)
k_amg_spgemm(int64_t cnnz, const int32_t *__restrict__ crow, const int32_t *__restrict__ ccol, const int64_t *__restrict__ aptr, const int32_t *__restrict__ acol,
             const double *__restrict__ aval, const int64_t *__restrict__ bptr, const int32_t *__restrict__ bcol, const double *__restrict__ bval, double *__restrict__ cval)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cnnz) return;
    const int32_t i = crow[q], j = ccol[q];
    double s = 0.0;
    for (int64_t k = aptr[i]; k < aptr[i + 1]; ++k) {
        const int32_t r = acol[k];
        int64_t lo = bptr[r];
        const int64_t end = bptr[r + 1];
        int64_t hi = end;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (bcol[mid] < j) lo = mid + 1; else hi = mid;
        }
        if (lo < end && bcol[lo] == j) s += aval[k] * bval[lo];
    }
    cval[q] = s;
}

// CSR products of the levels below the finest and of the transfers: 8 lanes per row, lane sums in stored order, a fixed butterfly over the 8 lanes.
// MODE 0: y = A x;  MODE 1: y = A (x − x2) (restriction of the residual);  MODE 2: y += A x (prolongation of the correction)
template <int MODE>
__global__ void __launch_bounds__(256)
k_amg_spmv(int64_t n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ A, const double *__restrict__ x,
           const double *__restrict__ x2, double *__restrict__ y)
{
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    if (i >= n) return; // (the 8 lanes of a row leave together)
    const int sub = threadIdx.x & 7;
    double s = 0.0;
    for (int64_t k = rowptr[i] + sub, hi = rowptr[i + 1]; k < hi; k += 8) {
        const int32_t j = colidx[k];
        s += A[k] * (MODE == 1 ? x[j] - x2[j] : x[j]);
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) s += __shfl_xor(s, o, 8);
    if (sub == 0) { if (MODE == 2) y[i] += s; else y[i] = s; }
}

// ---- ordered reductions of the λmax estimate: a partial per workgroup (strided lane sums, wave butterflies, the waves in order), then one workgroup
// folds the partials in a fixed tree (launch_fold_sum, launch_fold_max).  The grid depends on n and the device only. ----
constexpr int AMG_RED_BLOCKS = 256;
template <bool MAX>
__device__ __forceinline__ void amg_block_reduce(double v, double *__restrict__ partial)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const double u = __shfl_xor(v, o, 64); v = MAX ? fmax(v, u) : v + u; }
    __shared__ double sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = MAX ? fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3])) : ((sm[0] + sm[1]) + (sm[2] + sm[3]));
}
// Gershgorin row sums |d_i| Σ_j |a_ij| into g, their maximum into the partials
__global__ void __launch_bounds__(256)
k_amg_gershgorin(int64_t n, const int64_t *__restrict__ rowptr, const double *__restrict__ A, const double *__restrict__ dinv, double *__restrict__ g, double *__restrict__ partial)
{
    double mx = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double s = 0.0;
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) s += fabs(A[k]);
        s *= fabs(dinv[i]);
        g[i] = s;
        mx = fmax(mx, s);
    }
    amg_block_reduce<true>(mx, partial);
}
// partial maxima of |x|
__global__ void __launch_bounds__(256) k_amg_absmax(int64_t n, const double *__restrict__ x, double *__restrict__ partial)
{
    double mx = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) mx = fmax(mx, fabs(x[i]));
    amg_block_reduce<true>(mx, partial);
}
// sq = √(|D⁻¹| / c), v = the perturbed positive start vector of estimate_lambda_max, v₋₁ = 0; partial sums of v·v
__global__ void __launch_bounds__(256)
k_amg_lanczos_init(int64_t n, double c, const double *__restrict__ dinv, const double *__restrict__ start, double *__restrict__ sq, double *__restrict__ v,
                   double *__restrict__ vp, double *__restrict__ partial)
{
    double a = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        sq[i] = sqrt(fabs(dinv[i]) / c);
        const double vi = start[i] * (1.0 + 0.37 * (double)((i * 2654435761u) & 1023) / 1024.0);
        v[i] = vi;
        vp[i] = 0.0;
        a += vi * vi;
    }
    amg_block_reduce<false>(a, partial);
}
// y = s·a∘b (b NULL: s·a)
__global__ void __launch_bounds__(256) k_amg_scale_mul(int64_t n, double s, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ y)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = b ? s * a[i] * b[i] : s * a[i];
}
// w = sq∘(c w) − β v₋₁; partial sums of w·v
__global__ void __launch_bounds__(256)
k_amg_lanczos_a(int64_t n, double c, const double *__restrict__ sq, double beta, const double *__restrict__ vp, const double *__restrict__ v, double *__restrict__ w, double *__restrict__ partial)
{
    double a = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double wi = sq[i] * (c * w[i]) - beta * vp[i];
        w[i] = wi;
        a += wi * v[i];
    }
    amg_block_reduce<false>(a, partial);
}
// w −= α v; partial sums of w·w
__global__ void __launch_bounds__(256)
k_amg_lanczos_b(int64_t n, double alpha, const double *__restrict__ v, double *__restrict__ w, double *__restrict__ partial)
{
    double a = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double wi = w[i] - alpha * v[i];
        w[i] = wi;
        a += wi * wi;
    }
    amg_block_reduce<false>(a, partial);
}

static inline unsigned red_blocks(int64_t n) { return (unsigned)std::min<int64_t>(AMG_RED_BLOCKS, std::max<int64_t>(1, (n + 255) / 256)); }

template <class T>
static void free_dev(T *&p)
{
    if (p) (void)hipFree((void *)p);
    p = nullptr;
}

static void free_level(AmgLevel &L)
{
    L.release();
    amg_block_free_level(L);
    free_dev(L.d_rowptr); free_dev(L.d_colidx); free_dev(L.d_A); free_dev(L.d_comp); free_dev(L.d_diag); free_dev(L.d_strength);
    free_dev(L.d_agg); free_dev(L.d_tval); free_dev(L.d_pptr); free_dev(L.d_pcol); free_dev(L.d_prow); free_dev(L.d_P); free_dev(L.d_rptr); free_dev(L.d_rcol);
    free_dev(L.d_rperm); free_dev(L.d_R); free_dev(L.d_apptr); free_dev(L.d_apcol); free_dev(L.d_aprow); free_dev(L.d_AP); free_dev(L.d_crow);
}

static void free_plan(tb_amg *amg)
{
    for (AmgLevel &L : amg->lv) free_level(L);
    amg->lv.clear();
    free_dev(amg->d_cinv);
    amg->planned = amg->ready = false;
}

// y = A_l x; enqueues only
static int product(tb_amg *amg, int l, const double *x, double *y)
{
    AmgLevel &L = amg->lv[(size_t)l];
    if (l == 0) return launch_spmv(amg->pat, L.A, x, 1.0, 0.0, y);
    hipLaunchKernelGGL(k_amg_spmv<0>, dim3(blocks_of(L.n * 8, 256)), dim3(256), 0, amg->dev->stream, L.n, L.rowptr, L.colidx, L.A, x, (const double *)nullptr, y);
    return TB_OK;
}

template <bool MAX>
static int reduce_read(tb_amg *amg, unsigned nb, double *host)
{
    (MAX ? launch_fold_max : launch_fold_sum)(amg->dev, (int)nb, amg->d_red, amg->d_red + AMG_RED_BLOCKS);
    return read_back(amg->dev, host, amg->d_red + AMG_RED_BLOCKS, 1);
}

// The rule of estimate_lambda_max (tb_krylov.hip) on a level of this hierarchy: the Gershgorin bound of D⁻¹A, sharpened by the largest Ritz value of 24
// Lanczos steps on D^-½ A D^-½ inflated by 5 %.  The operator is applied as S (c A) S with c = max |D⁻¹| and S = √(|D⁻¹| / c): scaling A by a power of two
// scales c by its inverse and leaves S, c A and with them every bit of the estimate as they were (the square root of D⁻¹ itself would pick up a √2), so
// the hierarchy of 2 A is exactly twice that of A.  Scratch: the level's d, w, x, r and sixth vector.  Reads scalars back.
static int level_lambda_max(tb_amg *amg, int l, double *lmax_out)
{
    tb_device *dev = amg->dev;
    AmgLevel &L = amg->lv[(size_t)l];
    const int64_t n = L.n;
    double *w = L.w, *v = L.d, *vp = L.x, *t = L.r, *sq = L.r + n;
    const unsigned g = grid_for(dev, n, 256), nb = red_blocks(n);
    hipLaunchKernelGGL(k_amg_gershgorin, dim3(nb), dim3(256), 0, dev->stream, n, L.rowptr, L.A, (const double *)L.dinv, w, amg->d_red);
    double gersh = 0.0, h = 0.0;
    TB_TRY(reduce_read<true>(amg, nb, &gersh));
    double lmax = gersh, c = 0.0;
    hipLaunchKernelGGL(k_amg_absmax, dim3(nb), dim3(256), 0, dev->stream, n, (const double *)L.dinv, amg->d_red);
    TB_TRY(reduce_read<true>(amg, nb, &c));
    constexpr int KL = 24;
    double al[KL], be[KL + 1];
    if (c > 0.0 && std::isfinite(c)) {
        hipLaunchKernelGGL(k_amg_lanczos_init, dim3(nb), dim3(256), 0, dev->stream, n, c, (const double *)L.dinv, (const double *)w, sq, v, vp, amg->d_red);
        TB_TRY(reduce_read<false>(amg, nb, &h));
    }
    int kdone = 0;
    if (h > 0.0) {
        hipLaunchKernelGGL(k_amg_scale_mul, dim3(g), dim3(256), 0, dev->stream, n, 1.0 / std::sqrt(h), (const double *)v, (const double *)nullptr, v);
        be[0] = 0.0;
        for (int k = 0; k < KL; ++k) {
            hipLaunchKernelGGL(k_amg_scale_mul, dim3(g), dim3(256), 0, dev->stream, n, 1.0, (const double *)sq, (const double *)v, t); // t = D^-½ v
            TB_TRY(product(amg, l, t, w));
            hipLaunchKernelGGL(k_amg_lanczos_a, dim3(nb), dim3(256), 0, dev->stream, n, c, (const double *)sq, be[k], (const double *)vp, (const double *)v, w, amg->d_red);
            TB_TRY(reduce_read<false>(amg, nb, &h));
            al[k] = h;
            hipLaunchKernelGGL(k_amg_lanczos_b, dim3(nb), dim3(256), 0, dev->stream, n, al[k], (const double *)v, w, amg->d_red);
            TB_TRY(reduce_read<false>(amg, nb, &h));
            kdone = k + 1;
            be[k + 1] = std::sqrt(h);
            if (!(be[k + 1] > 1e-12 * std::fabs(al[k]))) break; // invariant subspace: the Ritz values are exact
            TB_HIP(hipMemcpyAsync(vp, v, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, dev->stream));
            hipLaunchKernelGGL(k_amg_scale_mul, dim3(g), dim3(256), 0, dev->stream, n, 1.0 / be[k + 1], (const double *)w, (const double *)nullptr, v);
        }
    }
    if (kdone > 0) lmax = std::min(gersh, 1.05 * largest_tridiagonal_eigenvalue(al, be, kdone));
    *lmax_out = lmax;
    return TB_OK;
}

// symbolic phase of level l (its matrix is in place): strength on the device, aggregates and patterns on the host, uploads, and the storage of level
// l + 1.  *coarsened = false: aggregation does not reduce n, the level stays the last one.
static int plan_level_below(tb_amg *amg, int l, bool *coarsened)
{
    tb_device *dev = amg->dev;
    *coarsened = false;
    const int64_t n = amg->lv[(size_t)l].n, nnz = amg->lv[(size_t)l].nnz;
    {
        AmgLevel &L = amg->lv[(size_t)l];
        if (amg->nns_k) TB_TRY(amg_block_plan(amg, l)); // node strength, node aggregates, k columns per aggregate
        else {
            if (!L.d_strength) TB_HIP(hipMalloc((void **)&L.d_strength, (size_t)std::max<int64_t>(nnz, 1)));
            launch_amg_strength(dev, n, L.rowptr, L.colidx, L.A, (const int8_t *)L.d_comp, amg->theta, L.w, L.d_strength);
            L.h_strength.resize((size_t)nnz);
            TB_HIP(hipMemcpyAsync(L.h_strength.data(), L.d_strength, (size_t)nnz, hipMemcpyDeviceToHost, dev->stream));
            TB_SYNC_STREAM(dev);
            free_dev(L.d_strength);
            const int64_t *hp = l == 0 ? amg->pat->h_rowptr.data() : L.h_rowptr.data();
            const int32_t *hc = l == 0 ? amg->pat->h_colidx.data() : L.h_colidx.data();
            amgplan::plan_level(n, hp, hc, L.h_comp.empty() ? nullptr : L.h_comp.data(), L.h_strength.data(), L.plan);
        }
        ++amg->aggregations;
        if (L.plan.nc <= 0 || L.plan.nc >= n) { L.plan = amgplan::LevelPlan(); L.plan.n = n; return TB_OK; }
        amgplan::LevelPlan &p = L.plan;
        std::vector<double> tval(amg->nns_k ? 0 : (size_t)p.nc);
        for (size_t J = 0; J < tval.size(); ++J) tval[J] = 1.0 / std::sqrt((double)p.agg_size[J]);
        if (amg->nns_k) TB_TRY(amg_block_tentative(amg, l)); // T, B_{l+1} and the dead flags instead of one constant per aggregate
        TB_TRY(upload_all(dev, p.agg, &L.d_agg, tval, &L.d_tval, p.p_ptr, &L.d_pptr, p.p_col, &L.d_pcol, p.p_row, &L.d_prow, p.r_ptr, &L.d_rptr, p.r_col, &L.d_rcol,
                          p.r_perm, &L.d_rperm, p.ap_ptr, &L.d_apptr, p.ap_col, &L.d_apcol, p.ap_row, &L.d_aprow, p.c_row, &L.d_crow));
        L.pnnz = (int64_t)p.p_col.size();
        L.apnnz = (int64_t)p.ap_col.size();
        L.nc = p.nc;
        TB_HIP(hipMalloc((void **)&L.d_P, sizeof(double) * (size_t)std::max<int64_t>(L.pnnz, 1)));
        TB_HIP(hipMalloc((void **)&L.d_R, sizeof(double) * (size_t)std::max<int64_t>(L.pnnz, 1)));
        TB_HIP(hipMalloc((void **)&L.d_AP, sizeof(double) * (size_t)std::max<int64_t>(L.apnnz, 1)));
    }
    amg->lv.emplace_back(); // (references into lv are stale from here)
    AmgLevel &L = amg->lv[(size_t)l], &N = amg->lv[(size_t)l + 1];
    amgplan::LevelPlan &p = L.plan;
    N.n = p.nc;
    N.nnz = (int64_t)p.c_col.size();
    N.h_rowptr.swap(p.c_ptr);
    N.h_colidx.swap(p.c_col);
    N.h_comp = L.h_comp.empty() ? std::vector<int8_t>() : p.ccomp;
    if (amg->nns_k) { // node = aggregate of this level, dofs k·a … k·a + k − 1; the candidates are the R factors
        N.n_nodes = p.nc / amg->nns_k;
        N.h_node.resize((size_t)N.n);
        for (int64_t i = 0; i < N.n; ++i) N.h_node[(size_t)i] = (int32_t)(i / amg->nns_k);
        N.d_B = L.d_Bc;
        L.d_Bc = nullptr;
    }
    TB_TRY(upload_all(dev, N.h_rowptr, &N.d_rowptr, N.h_colidx, &N.d_colidx, N.h_comp, &N.d_comp, p.c_diag, &N.d_diag));
    TB_HIP(hipMalloc((void **)&N.d_A, sizeof(double) * (size_t)std::max<int64_t>(N.nnz, 1)));
    N.rowptr = N.d_rowptr; N.colidx = N.d_colidx; N.A = N.d_A;
    TB_TRY(N.alloc(N.n));
    // the host keeps what the inspectors return (aggregates, P's pattern, strength); the product patterns live on the device only
    std::vector<int32_t>().swap(p.ap_col); std::vector<int32_t>().swap(p.ap_row); std::vector<int64_t>().swap(p.ap_ptr);
    std::vector<int32_t>().swap(p.c_row); std::vector<int64_t>().swap(p.c_diag); std::vector<int64_t>().swap(p.r_perm);
    std::vector<int32_t>().swap(p.r_col); std::vector<int64_t>().swap(p.r_ptr); std::vector<int32_t>().swap(p.p_row);
    *coarsened = true;
    return TB_OK;
}

void launch_amg_strength(tb_device *dev, int64_t n, const int64_t *rowptr, const int32_t *colidx, const double *val, const int8_t *comp, double theta, double *m,
                         uint8_t *flag)
{
    hipLaunchKernelGGL(k_amg_rowmax, dim3(blocks_of(n, 256)), dim3(256), 0, dev->stream, n, rowptr, colidx, val, comp, m);
    hipLaunchKernelGGL(k_amg_strength, dim3(blocks_of(n, 256)), dim3(256), 0, dev->stream, n, rowptr, colidx, val, comp, (const double *)m, theta, flag);
}

void launch_amg_spgemm(tb_device *dev, int64_t cnnz, const int32_t *crow, const int32_t *ccol, const int64_t *aptr, const int32_t *acol, const double *aval, const int64_t *bptr,
                       const int32_t *bcol, const double *bval, double *cval)
{
    hipLaunchKernelGGL(k_amg_spgemm, dim3(blocks_of(cnnz, 256)), dim3(256), 0, dev->stream, cnnz, crow, ccol, aptr, acol, aval, bptr, bcol, bval, cval);
}

// numeric phase between level l and l + 1: smoothed P, R, A·P, A_{l+1} = R (A·P); enqueues only (the products of a block hierarchy may allocate on their first call)
static int launch_level_numeric(tb_amg *amg, int l)
{
    tb_device *dev = amg->dev;
    AmgLevel &L = amg->lv[(size_t)l], &N = amg->lv[(size_t)l + 1];
    const double omega = 4.0 / (3.0 * L.lmax);
    if (amg->nns_k) amg_block_smooth_p(amg, l, omega);
    else
        hipLaunchKernelGGL(k_amg_smooth_p, dim3(blocks_of(L.pnnz, 256)), dim3(256), 0, dev->stream, L.pnnz, (const int32_t *)L.d_prow, (const int32_t *)L.d_pcol, L.rowptr,
                           L.colidx, L.A, (const int32_t *)L.d_agg, (const double *)L.d_tval, (const double *)L.dinv, omega, L.d_P);
    hipLaunchKernelGGL(k_amg_gather, dim3(blocks_of(L.pnnz, 256)), dim3(256), 0, dev->stream, L.pnnz, (const int64_t *)L.d_rperm, (const double *)L.d_P, L.d_R);
    if (amg->products) return amg->products(amg->products_ctx, l);
    launch_amg_spgemm(dev, L.apnnz, L.d_aprow, L.d_apcol, L.rowptr, L.colidx, L.A, L.d_pptr, L.d_pcol, L.d_P, L.d_AP);
    launch_amg_spgemm(dev, N.nnz, L.d_crow, N.colidx, L.d_rptr, L.d_rcol, L.d_R, L.d_apptr, L.d_apcol, L.d_AP, N.d_A);
    if (amg->nns_k) amg_block_dead_diag(amg, l);
    return TB_OK;
}

// x = M_l⁻¹ r: V(degree, degree) from x = 0; enqueues only
static int cycle(tb_amg *amg, int l, const double *r, double *x)
{
    tb_device *dev = amg->dev;
    AmgLevel &L = amg->lv[(size_t)l];
    if (l == (int)amg->lv.size() - 1) {
        launch_dense_apply(dev, (int)L.n, amg->d_cinv, r, x);
        return TB_OK;
    }
    AmgLevel &N = amg->lv[(size_t)l + 1];
    auto A = [&](const double *u, double *y) { return product(amg, l, u, y); };
    TB_TRY(cheb_smooth(dev, L.n, L, L.lmax, amg->ratio, amg->degree, r, x, true, A));
    TB_TRY(A(x, L.w));
    hipLaunchKernelGGL(k_amg_spmv<1>, dim3(blocks_of(N.n * 8, 256)), dim3(256), 0, dev->stream, N.n, (const int64_t *)L.d_rptr, (const int32_t *)L.d_rcol,
                       (const double *)L.d_R, r, (const double *)L.w, N.r);
    TB_TRY(cycle(amg, l + 1, N.r, N.x));
    hipLaunchKernelGGL(k_amg_spmv<2>, dim3(blocks_of(L.n * 8, 256)), dim3(256), 0, dev->stream, L.n, (const int64_t *)L.d_pptr, (const int32_t *)L.d_pcol,
                       (const double *)L.d_P, (const double *)N.x, (const double *)nullptr, x);
    return cheb_smooth(dev, L.n, L, L.lmax, amg->ratio, amg->degree, r, x, false, A);
}

int amg_apply_cb(void *ctx, const double *r, double *z)
{
    tb_amg *amg = (tb_amg *)ctx;
    const int rc = cycle(amg, 0, r, z);
    if (rc) return rc;
    TB_HIP(hipGetLastError());
    return TB_OK;
}

static int setup_levels(tb_amg *amg)
{
    tb_device *dev = amg->dev;
    for (int l = 0;; ++l) {
        bool last;
        if (amg->planned) last = l == (int)amg->lv.size() - 1;
        else {
            last = amg->lv[(size_t)l].n <= amg->max_coarse || l + 1 >= amg->max_levels;
            if (!last) {
                bool coarsened = false;
                TB_TRY(plan_level_below(amg, l, &coarsened));
                last = !coarsened;
            }
        }
        AmgLevel &L = amg->lv[(size_t)l];
        if (last) {
            if (L.n > amg->last_max) {
                set_error("%s: the last level (%d) has %lld %s; its dense inverse takes at most %d - the hierarchy stopped because %s", amg->who, l, (long long)L.n,
                          amg->unit, amg->last_max, l + 1 >= amg->max_levels ? "max_levels was reached (raise it)" : L.n <= amg->max_coarse ? "max_coarse allows it (lower it)"
                          : "aggregation no longer reduces the number of dofs (no strong couplings: lower theta)");
                return TB_ERR_UNSUPPORTED;
            }
            if (amg->products) break; // the block hierarchy inverts its own last level
            if (!amg->d_cinv) TB_HIP(hipMalloc((void **)&amg->d_cinv, sizeof(double) * (size_t)L.n * (size_t)L.n));
            launch_dense_inverse(dev, (int)L.n, L.rowptr, L.colidx, L.A, amg->d_cinv, amg->general);
            if (amg->general) TB_TRY(dense_inverse_status(dev, amg->who, l, (int)L.n));
            break;
        }
        hipLaunchKernelGGL(k_amg_dinv, dim3(blocks_of(L.n, 256)), dim3(256), 0, dev->stream, L.n, (const int64_t *)L.d_diag, L.A, L.dinv);
        TB_TRY(level_lambda_max(amg, l, &L.lmax));
        if (!(L.lmax > 0.0) || !std::isfinite(L.lmax)) {
            set_error("%s: the estimate of lambda_max(D^-1 A) on level %d is %g (a matrix without positive diagonal, or non-finite entries)", amg->who, l, L.lmax);
            return TB_ERR_BAD_ARG;
        }
        TB_TRY(launch_level_numeric(amg, l));
    }
    TB_HIP(hipGetLastError());
    amg->planned = true;
    return TB_OK;
}

} // namespace tb

using namespace tb;

int tb_amg_create(tb_pattern *pat, const int8_t *comp_host, double theta, int max_coarse, int max_levels, tb_amg **out)
{
    TB_REQUIRE(pat && out, "tb_amg_create: NULL argument");
    *out = nullptr;
    TB_TRY(check_amg_args("tb_amg_create", theta, max_coarse, max_levels));
    std::string err;
    if (amgplan::check_pattern(pat->n_rows, pat->h_rowptr.data(), pat->h_colidx.data(), err)) {
        set_error("tb_amg_create: %s (the aggregation needs sorted columns and a structurally symmetric pattern)", err.c_str());
        return TB_ERR_BAD_ARG;
    }
    tb_amg *amg = new tb_amg;
    amg->pat = pat;
    amg->dev = pat->mesh->dev;
    amg->theta = theta;
    amg->max_coarse = max_coarse;
    amg->max_levels = max_levels;
    if (comp_host) amg->comp.assign(comp_host, comp_host + pat->n_rows);
    *out = amg;
    return TB_OK;
}

int tb_amg_destroy(tb_amg *amg)
{
    if (!amg) return TB_OK;
    (void)hipSetDevice(amg->dev->id);
    free_plan(amg);
    free_dev(amg->d_red);
    delete amg;
    return TB_OK;
}

int tb_amg_replan(tb_amg *amg)
{
    TB_REQUIRE(amg, "tb_amg_replan: NULL argument");
    TB_NO_CAPTURE(amg->dev);
    TB_HIP(hipSetDevice(amg->dev->id));
    free_plan(amg);
    return TB_OK;
}

int tb_amg_setup(tb_amg *amg, const double *d_Anz, int degree, double interval_ratio)
{
    TB_REQUIRE(amg && d_Anz, "tb_amg_setup: NULL argument");
    TB_TRY(check_smoother_args("tb_amg_setup", degree, interval_ratio));
    tb_device *dev = amg->dev;
    TB_NO_CAPTURE(dev); // plans, reads strength flags and λmax back
    TB_HIP(hipSetDevice(dev->id));
    amg->ready = false;
    amg->degree = degree;
    amg->ratio = interval_ratio;
    if (!amg->d_red) TB_HIP(hipMalloc((void **)&amg->d_red, sizeof(double) * (AMG_RED_BLOCKS + 16)));
    TB_TRY(spmv_plans(amg->pat));
    if (!amg->planned) {
        free_plan(amg);
        amg->lv.emplace_back();
        AmgLevel &F = amg->lv[0];
        tb_pattern *pat = amg->pat;
        F.n = pat->n_rows; F.nnz = pat->nnz;
        F.rowptr = pat->d_rowptr; F.colidx = pat->d_colidx;
        F.h_comp = amg->comp;
        if (amg->nns_k) {
            F.h_node = amg->nns_node;
            F.n_nodes = amg->nns_nodes;
        }
        std::vector<int64_t> diag;
        amgplan::diagonal_positions(F.n, pat->h_rowptr.data(), pat->h_colidx.data(), diag);
        int rc = upload_all(dev, F.h_comp, &F.d_comp, diag, &F.d_diag);
        if (!rc && amg->nns_k) rc = upload(dev, amg->nns_B, &F.d_B);
        if (!rc) rc = F.alloc(F.n);
        if (rc) { free_plan(amg); return rc; }
    }
    amg->lv[0].A = d_Anz;
    const int rc = setup_levels(amg);
    if (rc) { free_plan(amg); return rc; }
    amg->ready = true;
    return TB_OK;
}

int tb_amg_set_general(tb_amg *amg, int general)
{
    TB_REQUIRE(amg, "tb_amg_set_general: NULL argument");
    if (amg->general == (general != 0)) return TB_OK;
    amg->general = general != 0;
    amg->ready = false; // the numeric phase is redone by the next tb_amg_setup (the plan stays)
    return TB_OK;
}

int tb_amg_apply(tb_amg *amg, const double *d_r, double *d_z)
{
    TB_REQUIRE(amg && d_r && d_z, "tb_amg_apply: NULL argument");
    TB_REQUIRE(amg->ready, "tb_amg_apply: no numeric setup yet (tb_amg_setup)");
    TB_REQUIRE(d_r != d_z, "tb_amg_apply: r and z alias");
    TB_HIP(hipSetDevice(amg->dev->id));
    return amg_apply_cb(amg, d_r, d_z);
}

int tb_pcg_solve_amg(tb_pattern *pat, const double *d_Anz, const double *d_b, double *d_x, double rtol, double atol, int maxiter, tb_amg *amg, int *iters,
                     double *resnorm)
{
    TB_REQUIRE(pat && d_Anz && d_b && d_x && amg, "tb_pcg_solve_amg: NULL argument");
    TB_REQUIRE(rtol >= 0 && atol >= 0 && maxiter >= 0, "tb_pcg_solve_amg: negative tolerance or iteration limit");
    TB_REQUIRE(amg->ready, "tb_pcg_solve_amg: no numeric setup yet (tb_amg_setup)");
    TB_REQUIRE(amg->pat == pat, "tb_pcg_solve_amg: the hierarchy was created for another pattern");
    TB_REQUIRE(amg->lv[0].A == d_Anz, "tb_pcg_solve_amg: the hierarchy was set up with another matrix array (tb_amg_setup follows every new matrix)");
    TB_HIP(hipSetDevice(pat->mesh->dev->id));
    return launch_pcg_apply(pat, d_Anz, d_b, d_x, rtol, atol, maxiter, amg_apply_cb, amg, "AMG preconditioner", iters, resnorm);
}

int tb_gmres_solve_amg(tb_pattern *pat, const double *d_Anz, const double *d_b, double *d_x, double rtol, double atol, int maxiter, int restart, tb_amg *amg,
                       int *iters, double *resnorm)
{
    TB_REQUIRE(pat && d_Anz && d_b && d_x && amg, "tb_gmres_solve_amg: NULL argument");
    TB_REQUIRE(rtol >= 0 && atol >= 0 && maxiter >= 0, "tb_gmres_solve_amg: negative tolerance or iteration limit");
    TB_REQUIRE(restart >= 1 && restart <= 1000, "tb_gmres_solve_amg: restart must be in 1..1000 (got %d)", restart);
    TB_REQUIRE(amg->ready, "tb_gmres_solve_amg: no numeric setup yet (tb_amg_setup; tb_amg_set_general asks for a new one)");
    TB_REQUIRE(amg->pat == pat, "tb_gmres_solve_amg: the hierarchy was created for another pattern");
    TB_REQUIRE(amg->lv[0].A == d_Anz, "tb_gmres_solve_amg: the hierarchy was set up with another matrix array (tb_amg_setup follows every new matrix)");
    TB_HIP(hipSetDevice(pat->mesh->dev->id));
    return launch_gmres_apply(pat, d_Anz, d_b, d_x, rtol, atol, maxiter, restart, amg_apply_cb, amg, "tb_gmres_solve_amg", iters, resnorm);
}

// ---- inspectors ----
#define AMG_LEVEL(fn)                                                                                             \
    TB_REQUIRE(amg, fn ": NULL argument");                                                                        \
    TB_REQUIRE(amg->ready, fn ": no numeric setup yet (tb_amg_setup)");                                           \
    TB_REQUIRE(level >= 0 && level < (int)amg->lv.size(), fn ": level %d of %d", level, (int)amg->lv.size());     \
    AmgLevel &L = amg->lv[(size_t)level]
#define AMG_FINE_LEVEL(fn)                                                                                                                                    \
    AMG_LEVEL(fn);                                                                                                                                            \
    TB_REQUIRE(level < (int)amg->lv.size() - 1, fn ": level %d is the last one (dense inverse): it has no aggregates, prolongator or smoother", level)

template <class T>
static int download(tb_device *dev, T *host, const T *d_src, size_t count)
{
    if (!host || !count) return TB_OK;
    TB_NO_CAPTURE(dev);
    TB_HIP(hipMemcpyAsync(host, d_src, count * sizeof(T), hipMemcpyDeviceToHost, dev->stream));
    TB_SYNC_STREAM(dev);
    return TB_OK;
}

int tb_amg_n_levels(tb_amg *amg, int *n_levels)
{
    TB_REQUIRE(amg && n_levels, "tb_amg_n_levels: NULL argument");
    TB_REQUIRE(amg->ready, "tb_amg_n_levels: no numeric setup yet (tb_amg_setup)");
    *n_levels = (int)amg->lv.size();
    return TB_OK;
}

int tb_amg_level_size(tb_amg *amg, int level, int64_t *n, int64_t *nnz, int64_t *n_aggregates)
{
    AMG_LEVEL("tb_amg_level_size");
    if (n) *n = L.n;
    if (nnz) *nnz = L.nnz;
    if (n_aggregates) *n_aggregates = L.nc;
    return TB_OK;
}

int tb_amg_level_csr(tb_amg *amg, int level, int64_t *rowptr, int32_t *colidx, double *values)
{
    AMG_LEVEL("tb_amg_level_csr");
    const int64_t *hp = level == 0 ? amg->pat->h_rowptr.data() : L.h_rowptr.data();
    const int32_t *hc = level == 0 ? amg->pat->h_colidx.data() : L.h_colidx.data();
    if (rowptr) memcpy(rowptr, hp, sizeof(int64_t) * (size_t)(L.n + 1));
    if (colidx) memcpy(colidx, hc, sizeof(int32_t) * (size_t)L.nnz);
    TB_HIP(hipSetDevice(amg->dev->id));
    return download(amg->dev, values, L.A, (size_t)L.nnz);
}

int tb_amg_level_prolongator(tb_amg *amg, int level, int64_t *nnz, int64_t *rowptr, int32_t *colidx, double *values)
{
    AMG_FINE_LEVEL("tb_amg_level_prolongator");
    if (nnz) *nnz = L.pnnz;
    if (rowptr) memcpy(rowptr, L.plan.p_ptr.data(), sizeof(int64_t) * (size_t)(L.n + 1));
    if (colidx) memcpy(colidx, L.plan.p_col.data(), sizeof(int32_t) * (size_t)L.pnnz);
    TB_HIP(hipSetDevice(amg->dev->id));
    return download(amg->dev, values, (const double *)L.d_P, (size_t)L.pnnz);
}

int tb_amg_level_aggregates(tb_amg *amg, int level, int32_t *aggregate)
{
    AMG_FINE_LEVEL("tb_amg_level_aggregates");
    TB_REQUIRE(aggregate, "tb_amg_level_aggregates: NULL argument");
    memcpy(aggregate, L.plan.agg.data(), sizeof(int32_t) * (size_t)L.n);
    return TB_OK;
}

int tb_amg_level_strength(tb_amg *amg, int level, uint8_t *flags)
{
    AMG_FINE_LEVEL("tb_amg_level_strength");
    TB_REQUIRE(flags, "tb_amg_level_strength: NULL argument");
    memcpy(flags, L.h_strength.data(), (size_t)L.nnz);
    return TB_OK;
}

int tb_amg_level_lambda_max(tb_amg *amg, int level, double *lmax)
{
    AMG_FINE_LEVEL("tb_amg_level_lambda_max");
    TB_REQUIRE(lmax, "tb_amg_level_lambda_max: NULL argument");
    *lmax = L.lmax;
    return TB_OK;
}

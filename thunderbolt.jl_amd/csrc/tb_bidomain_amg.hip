// tb_bidomain_amg.hip — algebraic multigrid preconditioner of the bidomain block system (tb_bidomain.hip) for meshes without nested grids: one
// smoothed-aggregation V(degree, degree) cycle on the node pairs (φₘ, φₑ), built from the matrix alone, and the conjugate gradients it preconditions.
//   auxiliary   the a₂₂ plane with the elimination of the ground baked in (launch_bd_csr_fine) drives a scalar hierarchy of tb_amg.hip, owned here,
//               unchanged and with one component label: strength, aggregates, T, P = T − ω D⁻¹ A T.  A grounded node has no strong neighbour there, stays
//               outside every aggregate and has an empty row of P.
//   transfer    𝒫 = P ⊗ I₂, no ground below the finest level, no masks: a grounded node gets no coarse correction in either unknown
//   operators   X_c = Pᵀ X_f P per plane on the scalar hierarchy's planned patterns; the three distinct planes (a₁₁, a₁₂, a₂₂) go through ONE walk of the
//               index streams (k_bdamg_spgemm3: three accumulators per output non-zero, one binary search), every accumulator in the stored order of
//               k_amg_spgemm.  The a₂₂ results land where the scalar hierarchy's own products would put them: its next level matrix IS the φₑφₑ plane.
//               a₂₁ is a copy of a₁₂ (the coarse φₘφₑ block is symmetric here); four planes are kept so that the sliced smoother kernel runs as it is.
//   cycle       smoother, λmax, coarsest inverse and recursion of the geometric block cycle (tb_bidomain_internal.hpp); transfers on 16-byte pairs in the
//               8-lanes-per-row layout of k_amg_spmv
// Levels are numbered as in tb_amg.hip: 0 is the finest.  No kernel of the set-up or of the cycle uses an atomic; every sum has one recorded order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>

#include "tb_amg_internal.hpp"
#include "tb_bidomain_internal.hpp"
#include "tb_internal.h"
#include "tb_mg_internal.hpp"

struct tb_bidomain_amg {
    tb_bidomain *bd = nullptr;
    tb_device *dev = nullptr;
    tb_amg *amg = nullptr;             // the scalar hierarchy on the masked a₂₂ plane (owned)
    std::vector<tb::BdMgLevel> lv;     // lv[0]: the finest level
    std::vector<double *> d_ap;        // per level with a level below: A·P of the planes a₁₁ | a₁₂ (2 · apnnz; a₂₂'s is the scalar hierarchy's)
    int degree = 2;
    double ratio = 4.0;
    bool ready = false;
    int64_t setups = 0;                // successful set-ups so far
    uint64_t set_for = 0;              // generation of the block system the set-up read
    double *d_cinv = nullptr;          // (2 n_last)²: dense inverse of the last level on interleaved unknowns
    double *d_scal = nullptr, *d_part = nullptr, *d_ws = nullptr;
    tb::BdCycle cycle_record() const { return tb::BdCycle{bd, dev, degree, ratio, false, d_scal, d_part, d_ws}; }
};

namespace tb {

// C = A·B on the planned pattern of C for three planes at once: the walk and the search of k_amg_spgemm once per output non-zero, three accumulators,
// each in k_amg_spgemm's stored order — every plane is bit for bit what a k_amg_spgemm launch on it alone gives.  A3: three planes of A times one B
// (A·P); otherwise one A times three planes of B (R·(A·P)).
template <bool A3>
__global__ void __launch_bounds__(256)
k_bdamg_spgemm3(int64_t cnnz, const int32_t *__restrict__ crow, const int32_t *__restrict__ ccol, const int64_t *__restrict__ aptr, const int32_t *__restrict__ acol,
                const double *__restrict__ a0, const double *__restrict__ a1, const double *__restrict__ a2, const int64_t *__restrict__ bptr, const int32_t *__restrict__ bcol,
                const double *__restrict__ b0, const double *__restrict__ b1, const double *__restrict__ b2, double *__restrict__ c0, double *__restrict__ c1,
                double *__restrict__ c2)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cnnz) return;
    const int32_t i = crow[q], j = ccol[q];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int64_t k = aptr[i]; k < aptr[i + 1]; ++k) {
        const int32_t r = acol[k];
        int64_t lo = bptr[r];
        const int64_t end = bptr[r + 1];
        int64_t hi = end;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (bcol[mid] < j) lo = mid + 1; else hi = mid;
        }
        if (lo < end && bcol[lo] == j) {
            if (A3) { const double b = b0[lo]; s0 += a0[k] * b; s1 += a1[k] * b; s2 += a2[k] * b; }
            else { const double a = a0[k]; s0 += a * b0[lo]; s1 += a * b1[lo]; s2 += a * b2[lo]; }
        }
    }
    c0[q] = s0; c1[q] = s1; c2[q] = s2;
}

// The transfers on interleaved pairs, (T ⊗ I₂): k_amg_spmv with 16-byte gathers — 8 lanes per row, lane sums in stored order, the fixed butterfly over
// the 8 lanes, so each component is bit for bit a scalar k_amg_spmv of that component.  MODE 1: y = T (x − x2) (restriction of the residual);
// MODE 2: y += T x (prolongation of the correction)
template <int MODE>
__global__ void __launch_bounds__(256)
k_bdamg_transfer(int64_t n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ T, const double2 *__restrict__ x,
                 const double2 *__restrict__ x2, double2 *__restrict__ y)
{
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    if (i >= n) return; // (the 8 lanes of a row leave together)
    const int sub = threadIdx.x & 7;
    double sm = 0.0, se = 0.0;
    for (int64_t k = rowptr[i] + sub, hi = rowptr[i + 1]; k < hi; k += 8) {
        const int32_t j = colidx[k];
        double2 v = x[j];
        if (MODE == 1) { const double2 u = x2[j]; v.x -= u.x; v.y -= u.y; }
        const double t = T[k];
        sm += t * v.x; se += t * v.y;
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 8); se += __shfl_xor(se, o, 8); }
    if (sub == 0) {
        if (MODE == 2) { double2 yi = y[i]; yi.x += sm; yi.y += se; y[i] = yi; }
        else y[i] = make_double2(sm, se);
    }
}

static void free_levels(tb_bidomain_amg *h)
{
    for (BdMgLevel &L : h->lv) {
        void *ptrs[] = {L.d_ground, L.d_csr, L.d_base, L.d_col, L.d_val, L.d_binv, L.d_vec};
        for (void *p : ptrs) if (p) (void)hipFree(p);
    }
    h->lv.clear();
    for (double *p : h->d_ap) if (p) (void)hipFree(p);
    h->d_ap.clear();
    if (h->d_cinv) (void)hipFree(h->d_cinv);
    h->d_cinv = nullptr;
    h->ready = false;
}

static void free_bdamg(tb_bidomain_amg *h)
{
    if (!h) return;
    free_levels(h);
    if (h->amg) (void)tb_amg_destroy(h->amg);
    (void)hipFree(h->d_scal); (void)hipFree(h->d_part); (void)hipFree(h->d_ws);
    delete h;
}

// the storage of block level l (its size is known: the scalar hierarchy has planned it)
static int alloc_level(tb_bidomain_amg *h, int l)
{
    tb_device *dev = h->dev;
    const AmgLevel &S = h->amg->lv[(size_t)l];
    h->lv.emplace_back();
    h->d_ap.push_back(nullptr);
    BdMgLevel &L = h->lv.back();
    L.n = S.n; L.nnz = S.nnz;
    L.fine = l == 0;
    TB_HIP(hipMalloc((void **)&L.d_csr, sizeof(double) * 4 * (size_t)std::max<int64_t>(L.nnz, 1)));
    TB_HIP(hipMalloc((void **)&L.d_vec, sizeof(double) * 10 * (size_t)L.n));
    L.d = L.d_vec; L.w = L.d + 2 * L.n; L.xt = L.w + 2 * L.n; L.x = L.xt + 2 * L.n; L.r = L.x + 2 * L.n;
    TB_HIP(hipMalloc((void **)&L.d_binv, sizeof(double) * 3 * (size_t)L.n));
    if (l == 0) {
        L.pat = h->bd->pat;
        L.ground = h->bd->d_ground;
        return TB_OK;
    }
    TB_HIP(hipMalloc((void **)&L.d_ground, (size_t)L.n)); // no ground below the finest level: the flags the λmax estimate's start vector reads are all 0
    TB_HIP(hipMemsetAsync(L.d_ground, 0, (size_t)L.n, dev->stream));
    L.ground = L.d_ground;
    L.n_slices = (L.n + 63) / 64;
    std::vector<int64_t> base;
    bd_slice_table(L.n, S.h_rowptr.data(), base);
    L.entries = base.back();
    TB_TRY(upload(dev, base, &L.d_base));
    TB_HIP(hipMalloc((void **)&L.d_col, std::max<size_t>(1, (size_t)L.entries) * sizeof(uint32_t)));
    TB_HIP(hipMalloc((void **)&L.d_val, std::max<size_t>(1, 4 * (size_t)L.entries) * sizeof(double)));
    return TB_OK;
}

// what the scalar set-up calls between level l and l + 1 once P and R are in place: A·P and R·(A·P) of the three planes
static int block_products(void *ctx, int l)
{
    tb_bidomain_amg *h = (tb_bidomain_amg *)ctx;
    tb_device *dev = h->dev;
    AmgLevel &S = h->amg->lv[(size_t)l], &N = h->amg->lv[(size_t)l + 1];
    if ((int)h->lv.size() < l + 2) {
        TB_TRY(alloc_level(h, l + 1));
        TB_HIP(hipMalloc((void **)&h->d_ap[(size_t)l], sizeof(double) * 2 * (size_t)std::max<int64_t>(S.apnnz, 1)));
    }
    const BdMgLevel &L = h->lv[(size_t)l], &C = h->lv[(size_t)l + 1];
    double *ap = h->d_ap[(size_t)l];
    // (level 0's a₂₂ plane is S.A itself; below, S.A is the scalar hierarchy's level matrix, of which the level's fourth plane is a copy)
    hipLaunchKernelGGL(k_bdamg_spgemm3<true>, dim3(blocks_of(S.apnnz, 256)), dim3(256), 0, dev->stream, S.apnnz, (const int32_t *)S.d_aprow, (const int32_t *)S.d_apcol, S.rowptr,
                       S.colidx, (const double *)L.d_csr, (const double *)(L.d_csr + L.nnz), S.A, (const int64_t *)S.d_pptr, (const int32_t *)S.d_pcol, (const double *)S.d_P,
                       (const double *)nullptr, (const double *)nullptr, ap, ap + S.apnnz, S.d_AP);
    hipLaunchKernelGGL(k_bdamg_spgemm3<false>, dim3(blocks_of(N.nnz, 256)), dim3(256), 0, dev->stream, N.nnz, (const int32_t *)S.d_crow, N.colidx, (const int64_t *)S.d_rptr,
                       (const int32_t *)S.d_rcol, (const double *)S.d_R, (const double *)nullptr, (const double *)nullptr, (const int64_t *)S.d_apptr, (const int32_t *)S.d_apcol,
                       (const double *)ap, (const double *)(ap + S.apnnz), (const double *)S.d_AP, C.d_csr, C.d_csr + C.nnz, N.d_A);
    TB_HIP(hipMemcpyAsync(C.d_csr + 2 * C.nnz, C.d_csr + C.nnz, sizeof(double) * (size_t)C.nnz, hipMemcpyDeviceToDevice, dev->stream)); // a₂₁ ≡ a₁₂
    TB_HIP(hipMemcpyAsync(C.d_csr + 3 * C.nnz, N.d_A, sizeof(double) * (size_t)C.nnz, hipMemcpyDeviceToDevice, dev->stream));
    return TB_OK;
}

// x = ℳ_l⁻¹ r: V(degree, degree) from x = 0; enqueues only.  The fused smoother ping-pongs as in the geometric cycle: it starts in the level's spare
// buffer and ends in x.
static void cycle(tb_bidomain_amg *h, int l, const double *r, double *x)
{
    tb_device *dev = h->dev;
    BdMgLevel &L = h->lv[(size_t)l];
    if (l == (int)h->lv.size() - 1) {
        launch_dense_apply(dev, (int)(2 * L.n), h->d_cinv, r, x);
        return;
    }
    const BdCycle cy = h->cycle_record();
    BdMgLevel &C = h->lv[(size_t)l + 1];
    const AmgLevel &S = h->amg->lv[(size_t)l];
    double *cur = L.xt, *other = x;
    bd_smooth(cy, L, r, cur, other, true);
    bd_level_product(cy, L, 0, cur, L.w, BdStep());
    hipLaunchKernelGGL(k_bdamg_transfer<1>, dim3(blocks_of(C.n * 8, 256)), dim3(256), 0, dev->stream, C.n, (const int64_t *)S.d_rptr, (const int32_t *)S.d_rcol,
                       (const double *)S.d_R, (const double2 *)r, (const double2 *)L.w, (double2 *)C.r);
    cycle(h, l + 1, C.r, C.x);
    hipLaunchKernelGGL(k_bdamg_transfer<2>, dim3(blocks_of(L.n * 8, 256)), dim3(256), 0, dev->stream, L.n, (const int64_t *)S.d_pptr, (const int32_t *)S.d_pcol,
                       (const double *)S.d_P, (const double2 *)C.x, (const double2 *)nullptr, (double2 *)cur);
    bd_smooth(cy, L, r, cur, other, false);
}

static void algebraic_cycle(void *ctx, const double *r, double *z) { cycle((tb_bidomain_amg *)ctx, 0, r, z); }

} // namespace tb

using namespace tb;

#define BDAMG_READY(h_, who_)                                                                                                                                      \
    do {                                                                                                                                                           \
        TB_REQUIRE((h_)->ready, who_ ": no numeric set-up yet (tb_bidomain_amg_setup)");                                                                           \
        TB_REQUIRE((h_)->set_for == (h_)->bd->generation, who_ ": tb_bidomain_set_matrices ran after the latest set-up (tb_bidomain_amg_setup follows every new matrix)"); \
    } while (0)
#define BDAMG_LEVEL(h_, who_)                                                                                    \
    TB_REQUIRE(h_, who_ ": NULL argument");                                                                      \
    BDAMG_READY(h_, who_);                                                                                       \
    TB_REQUIRE(level >= 0 && level < (int)(h_)->lv.size(), who_ ": level %d of %d", level, (int)(h_)->lv.size())

extern "C" {

int tb_bidomain_amg_create(tb_bidomain *bd, double theta, int max_coarse, int max_levels, tb_bidomain_amg **out)
{
    TB_REQUIRE(bd && out, "tb_bidomain_amg_create: NULL argument");
    *out = nullptr;
    TB_TRY(check_amg_args("tb_bidomain_amg_create", theta, max_coarse, max_levels));
    if (max_coarse > BD_COARSEST_NODES) {
        set_error("tb_bidomain_amg_create: max_coarse is %d nodes; the dense inverse of the last level takes at most %d nodes (%d unknowns)", max_coarse, BD_COARSEST_NODES,
                  2 * BD_COARSEST_NODES);
        return TB_ERR_UNSUPPORTED;
    }
    tb_device *dev = bd->pat->mesh->dev;
    TB_NO_CAPTURE(dev); // allocations
    TB_HIP(hipSetDevice(dev->id));
    std::unique_ptr<tb_bidomain_amg, void (*)(tb_bidomain_amg *)> h(new tb_bidomain_amg, free_bdamg);
    h->bd = bd; h->dev = dev;
    TB_TRY(tb_amg_create(bd->pat, nullptr, theta, max_coarse, max_levels, &h->amg));
    h->amg->products = block_products;
    h->amg->products_ctx = h.get();
    h->amg->last_max = BD_COARSEST_NODES;
    h->amg->who = "tb_bidomain_amg_setup";
    h->amg->unit = "nodes";
    TB_HIP(hipMalloc((void **)&h->d_scal, 8 * sizeof(double)));
    TB_HIP(hipMalloc((void **)&h->d_part, sizeof(double) * 8 * (size_t)std::max(dev->n_cu, 1))); // grid_for never launches more workgroups
    TB_HIP(hipMalloc((void **)&h->d_ws, sizeof(double) * 8 * (size_t)bd->n));
    *out = h.release();
    return TB_OK;
}

int tb_bidomain_amg_destroy(tb_bidomain_amg *h)
{
    if (h) (void)hipSetDevice(h->dev->id);
    free_bdamg(h);
    return TB_OK;
}

int tb_bidomain_amg_replan(tb_bidomain_amg *h)
{
    TB_REQUIRE(h, "tb_bidomain_amg_replan: NULL argument");
    TB_NO_CAPTURE(h->dev);
    TB_HIP(hipSetDevice(h->dev->id));
    TB_TRY(tb_amg_replan(h->amg));
    free_levels(h);
    return TB_OK;
}

int tb_bidomain_amg_setup(tb_bidomain_amg *h, int degree, double interval_ratio)
{
    TB_REQUIRE(h, "tb_bidomain_amg_setup: NULL argument");
    TB_TRY(check_smoother_args("tb_bidomain_amg_setup", degree, interval_ratio));
    tb_bidomain *bd = h->bd;
    tb_device *dev = h->dev;
    TB_NO_CAPTURE(dev); // plans, reads strength flags and λmax back
    TB_REQUIRE(bd->have_matrices, "tb_bidomain_amg_setup: no matrices yet (tb_bidomain_set_matrices comes first)");
    TB_HIP(hipSetDevice(dev->id));
    h->ready = false;
    h->degree = degree;
    h->ratio = interval_ratio;
    if (!h->amg->planned) {
        free_levels(h);
        h->lv.reserve((size_t)h->amg->max_levels);
        h->d_ap.reserve((size_t)h->amg->max_levels);
    }
    int rc = TB_OK;
    if (h->lv.empty()) {
        h->lv.emplace_back();
        h->d_ap.push_back(nullptr);
        BdMgLevel &F = h->lv[0];
        F.n = bd->n; F.nnz = bd->pat->nnz; F.fine = true; F.pat = bd->pat; F.ground = bd->d_ground;
        hipError_t e = hipMalloc((void **)&F.d_csr, sizeof(double) * 4 * (size_t)std::max<int64_t>(F.nnz, 1));
        if (e == hipSuccess) e = hipMalloc((void **)&F.d_vec, sizeof(double) * 10 * (size_t)F.n);
        if (e == hipSuccess) e = hipMalloc((void **)&F.d_binv, sizeof(double) * 3 * (size_t)F.n);
        if (e != hipSuccess) { (void)tb_amg_replan(h->amg); free_levels(h); TB_HIP(e); }
        F.d = F.d_vec; F.w = F.d + 2 * F.n; F.xt = F.w + 2 * F.n; F.x = F.xt + 2 * F.n; F.r = F.x + 2 * F.n;
    }
    // the scalar hierarchy on the masked a₂₂ plane; its numeric phase carries the other planes along (block_products)
    launch_bd_csr_fine(bd, h->lv[0].d_csr);
    rc = tb_amg_setup(h->amg, h->lv[0].d_csr + 3 * h->lv[0].nnz, degree, interval_ratio);
    if (rc) { (void)tb_amg_replan(h->amg); free_levels(h); return rc; } // (whether or not the failure came before tb_amg_setup dropped its own plan)
    const int nl = (int)h->amg->lv.size();
    const BdCycle cy = h->cycle_record();
    for (int l = 0; l < nl - 1 && !rc; ++l) {
        BdMgLevel &L = h->lv[(size_t)l];
        const AmgLevel &S = h->amg->lv[(size_t)l];
        if (l == 0) launch_bd_binv_fine(bd, L.d_binv);
        else launch_bd_fill_sliced(dev, L, S.rowptr, S.colidx);
        rc = bd_lambda_max(cy, L, "tb_bidomain_amg_setup", l, &L.lmax);
        if (!rc && (!(L.lmax > 0.0) || !std::isfinite(L.lmax))) {
            set_error("tb_bidomain_amg_setup: the estimate of lambda_max(B^-1 A) on level %d is %g (a block matrix that is not positive definite, or non-finite entries)", l, L.lmax);
            rc = TB_ERR_BAD_ARG;
        }
    }
    if (!rc) {
        BdMgLevel &Z = h->lv[(size_t)nl - 1];
        const AmgLevel &S = h->amg->lv[(size_t)nl - 1];
        if (!h->d_cinv) {
            const hipError_t e = hipMalloc((void **)&h->d_cinv, sizeof(double) * 4 * (size_t)Z.n * (size_t)Z.n);
            if (e != hipSuccess) { (void)tb_amg_replan(h->amg); free_levels(h); TB_HIP(e); }
        }
        launch_bd_dense_inverse(dev, (int)Z.n, S.rowptr, S.colidx, Z.nnz, Z.d_csr, h->d_cinv);
        if (hipGetLastError() != hipSuccess) { set_error("tb_bidomain_amg_setup: a kernel launch failed"); rc = TB_ERR_HIP; }
    }
    if (rc) { (void)tb_amg_replan(h->amg); free_levels(h); return rc; }
    h->set_for = bd->generation;
    h->ready = true;
    ++h->setups;
    return TB_OK;
}

int tb_bidomain_amg_apply(tb_bidomain_amg *h, const double *d_r, double *d_z)
{
    TB_REQUIRE(h && d_r && d_z, "tb_bidomain_amg_apply: NULL argument");
    BDAMG_READY(h, "tb_bidomain_amg_apply");
    TB_REQUIRE(d_r != d_z, "tb_bidomain_amg_apply: r and z alias");
    BD_ALIGNED(d_r, "tb_bidomain_amg_apply"); BD_ALIGNED(d_z, "tb_bidomain_amg_apply");
    TB_HIP(hipSetDevice(h->dev->id));
    cycle(h, 0, d_r, d_z);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_bidomain_amg_products(tb_bidomain_amg *h, int level, int fused)
{
    BDAMG_LEVEL(h, "tb_bidomain_amg_products");
    TB_REQUIRE(level < (int)h->lv.size() - 1, "tb_bidomain_amg_products: level %d is the last one: there is no level below it", level);
    TB_HIP(hipSetDevice(h->dev->id));
    if (fused) return block_products(h, level);
    tb_device *dev = h->dev;
    const AmgLevel &S = h->amg->lv[(size_t)level], &N = h->amg->lv[(size_t)level + 1];
    const BdMgLevel &L = h->lv[(size_t)level], &C = h->lv[(size_t)level + 1];
    double *ap = h->d_ap[(size_t)level];
    const double *planes[3] = {L.d_csr, L.d_csr + L.nnz, S.A};
    double *aps[3] = {ap, ap + S.apnnz, S.d_AP}, *cs[3] = {C.d_csr, C.d_csr + C.nnz, N.d_A};
    for (int q = 0; q < 3; ++q) {
        launch_amg_spgemm(dev, S.apnnz, S.d_aprow, S.d_apcol, S.rowptr, S.colidx, planes[q], S.d_pptr, S.d_pcol, S.d_P, aps[q]);
        launch_amg_spgemm(dev, N.nnz, S.d_crow, N.colidx, S.d_rptr, S.d_rcol, S.d_R, S.d_apptr, S.d_apcol, aps[q], cs[q]);
    }
    TB_HIP(hipMemcpyAsync(C.d_csr + 2 * C.nnz, C.d_csr + C.nnz, sizeof(double) * (size_t)C.nnz, hipMemcpyDeviceToDevice, dev->stream));
    TB_HIP(hipMemcpyAsync(C.d_csr + 3 * C.nnz, N.d_A, sizeof(double) * (size_t)C.nnz, hipMemcpyDeviceToDevice, dev->stream));
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_bidomain_amg_solve(tb_bidomain_amg *h, const double *d_b, double *d_x, double rtol, double atol, int maxiter, int *iters, double *resnorm)
{
    TB_REQUIRE(h && d_b && d_x, "tb_bidomain_amg_solve: NULL argument");
    BDAMG_READY(h, "tb_bidomain_amg_solve");
    TB_REQUIRE(rtol >= 0 && atol >= 0 && maxiter >= 0, "tb_bidomain_amg_solve: negative tolerance or iteration limit");
    TB_REQUIRE(d_b != d_x, "tb_bidomain_amg_solve: b and x alias");
    BD_ALIGNED(d_b, "tb_bidomain_amg_solve"); BD_ALIGNED(d_x, "tb_bidomain_amg_solve");
    TB_HIP(hipSetDevice(h->dev->id));
    return bd_pcg(h->cycle_record(), "tb_bidomain_amg_solve", algebraic_cycle, h, d_b, d_x, rtol, atol, maxiter, iters, resnorm);
}

// ---- inspectors (host outputs)
int tb_bidomain_amg_counts(tb_bidomain_amg *h, int64_t *setups, int64_t *aggregations)
{
    TB_REQUIRE(h, "tb_bidomain_amg_counts: NULL argument");
    if (setups) *setups = h->setups;
    if (aggregations) *aggregations = h->amg->aggregations;
    return TB_OK;
}

int tb_bidomain_amg_n_levels(tb_bidomain_amg *h, int *n_levels)
{
    TB_REQUIRE(h && n_levels, "tb_bidomain_amg_n_levels: NULL argument");
    BDAMG_READY(h, "tb_bidomain_amg_n_levels");
    *n_levels = (int)h->lv.size();
    return TB_OK;
}

int tb_bidomain_amg_level_size(tb_bidomain_amg *h, int level, int64_t *n, int64_t *nnz, int64_t *n_aggregates)
{
    BDAMG_LEVEL(h, "tb_bidomain_amg_level_size");
    return tb_amg_level_size(h->amg, level, n, nnz, n_aggregates);
}

int tb_bidomain_amg_level_csr(tb_bidomain_amg *h, int level, int64_t *rowptr, int32_t *colidx)
{
    BDAMG_LEVEL(h, "tb_bidomain_amg_level_csr");
    return tb_amg_level_csr(h->amg, level, rowptr, colidx, nullptr);
}

int tb_bidomain_amg_level_planes(tb_bidomain_amg *h, int level, double *a11, double *a12, double *a21, double *a22)
{
    BDAMG_LEVEL(h, "tb_bidomain_amg_level_planes");
    tb_device *dev = h->dev;
    TB_NO_CAPTURE(dev);
    TB_HIP(hipSetDevice(dev->id));
    const BdMgLevel &L = h->lv[(size_t)level];
    double *out[4] = {a11, a12, a21, a22};
    for (int q = 0; q < 4; ++q)
        if (out[q] && L.nnz) TB_HIP(hipMemcpyAsync(out[q], L.d_csr + q * L.nnz, sizeof(double) * (size_t)L.nnz, hipMemcpyDeviceToHost, dev->stream));
    TB_SYNC_STREAM(dev);
    return TB_OK;
}

int tb_bidomain_amg_level_prolongator(tb_bidomain_amg *h, int level, int64_t *nnz, int64_t *rowptr, int32_t *colidx, double *values)
{
    BDAMG_LEVEL(h, "tb_bidomain_amg_level_prolongator");
    return tb_amg_level_prolongator(h->amg, level, nnz, rowptr, colidx, values);
}

int tb_bidomain_amg_level_aggregates(tb_bidomain_amg *h, int level, int32_t *aggregate)
{
    BDAMG_LEVEL(h, "tb_bidomain_amg_level_aggregates");
    return tb_amg_level_aggregates(h->amg, level, aggregate);
}

int tb_bidomain_amg_level_lambda_max(tb_bidomain_amg *h, int level, double *lmax)
{
    BDAMG_LEVEL(h, "tb_bidomain_amg_level_lambda_max");
    TB_REQUIRE(lmax, "tb_bidomain_amg_level_lambda_max: NULL argument");
    TB_REQUIRE(level < (int)h->lv.size() - 1, "tb_bidomain_amg_level_lambda_max: level %d is the last one (dense inverse): it has no smoother", level);
    *lmax = h->lv[(size_t)level].lmax;
    return TB_OK;
}

} // extern "C"

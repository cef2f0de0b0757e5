// tb_krylov.hip — the Krylov solvers on a device CSR matrix: Jacobi-CG (launch_cg), restarted GMRES, ℓ₁ Gauss–Seidel and Chebyshev preconditioned CG,
// and the two distributed CG forms whose scalars live in caller-owned device memory (cgd: three all-reduces per iteration, cg1: one).  Products come
// from tb_spmv.hip (every CG form picks its product kernel through launch_spmv_dot_slots), workgroup sums and slot groups from tb_reduce.hpp.  The
// solvers of one pattern share one workspace (krylov_ws); each reads its scalars back through read_back.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "tb_internal.h"
#include "tb_mg_internal.hpp"
#include "tb_reduce.hpp"

namespace tb {

// The one solver workspace of a pattern: grow-only, and whoever takes it lays its vectors and scalars out from the start, so it holds the state of
// the solver that ran last.  The only state a later solve looks for is launch_cg's D⁻¹ (TB_JACOBI_REUSE, guarded by cg_dinv_of): growing loses it,
// and every taker other than launch_cg clears the guard itself.
double *krylov_ws(tb_pattern *pat, size_t doubles)
{
    if (doubles == 0) doubles = 1; // (an empty pattern still gets a pointer)
    if (doubles > pat->krylov_ws_doubles) {
        if (pat->d_krylov_ws) (void)hipFree(pat->d_krylov_ws);
        pat->d_krylov_ws = nullptr;
        pat->krylov_ws_doubles = 0;
        pat->cg_dinv_of = nullptr;
        const hipError_t e = hipMalloc((void **)&pat->d_krylov_ws, doubles * sizeof(double));
        if (e != hipSuccess) { set_error("Krylov workspace (%zu B): %s", doubles * sizeof(double), hipGetErrorString(e)); return nullptr; }
        pat->krylov_ws_doubles = doubles;
    }
    return pat->d_krylov_ws;
}

// (stopping_tolerance, the stopping rule of every solver here and of tb_bidomain.hip, is in tb_internal.h)

} // namespace tb

// ------------------------------------------------------------------------------------------------
// Preconditioned conjugate gradients for the heat step  (M − Δt K) uₙ = M uₙ₋₁ + f
// (src/solver/time/euler.jl:94-100; the tutorials use KrylovJL_CG(atol = 1e-6, rtol = 1e-5),
// docs/src/literate-tutorials/ep01_spiral-wave.jl:126-128).  Adjacent component: the
// Krylov method itself is third party (Krylov.jl) in the reference, so this is a plain textbook PCG
// with a Jacobi preconditioner; stopping test ‖r‖₂ ≤ atol + rtol·‖r₀‖₂ like Krylov.jl's cg.
// ------------------------------------------------------------------------------------------------
namespace tb {

// r = b − Ax (Ax given), z = D⁻¹ r, p = z;  out[0] += r·z, out[1] += r·r
__global__ void __launch_bounds__(256)
k_cg_init(int64_t n, const double *__restrict__ b, const double *__restrict__ Ax, const double *__restrict__ dinv, double *__restrict__ r,
          double *__restrict__ p, double *__restrict__ out)
{
    double rz = 0.0, rr = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double ri = b[i] - Ax[i];
        const double zi = dinv ? dinv[i] * ri : ri;
        r[i] = ri; p[i] = zi;
        rz += ri * zi; rr += ri * ri;
    }
    block_sum_to(rz, out);
    __syncthreads();
    block_sum_to(rr, out + 1);
}

// x += α p, r −= α Ap;  out[0] += r·(D⁻¹r), out[1] += r·r
__global__ void __launch_bounds__(1024)
k_cg_update(int64_t n, double alpha, const double *__restrict__ p, const double *__restrict__ Ap, const double *__restrict__ dinv,
            double *__restrict__ x, double *__restrict__ r, double *__restrict__ out)
{
    double rz = 0.0, rr = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * Ap[i];
        r[i] = ri;
        rz += ri * (dinv ? dinv[i] * ri : ri);
        rr += ri * ri;
    }
    block_sum_to(rz, out);
    __syncthreads();
    block_sum_to(rr, out + 1);
}

// p = D⁻¹ r + β p
__global__ void __launch_bounds__(256)
k_cg_direction(int64_t n, double beta, const double *__restrict__ r, const double *__restrict__ dinv, double *__restrict__ p)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = (dinv ? dinv[i] * r[i] : r[i]) + beta * p[i];
}

// ---- device-resident CG scalars: the host only reads (pᵀAp, rᵀr) once per iteration to decide whether to go on ----
// scal[0..2]: r·z of the current / next / retired iteration (rotating), scal[3] = pᵀAp, scal[4] = rᵀr
__global__ void __launch_bounds__(256)
k_cg_update_dev(int64_t n, const double *__restrict__ rz, const double *__restrict__ pAp, const double *__restrict__ p, const double *__restrict__ Ap,
                const double *__restrict__ dinv, double *__restrict__ x, double *__restrict__ r, double *__restrict__ rz_next, double *__restrict__ rr,
                double *__restrict__ flag)
{
    // pᵀAp ≤ 0 with a non-zero residual: the matrix is not positive definite — remembered in a sticky flag the host reads at its next
    // convergence check; at exact convergence (r = 0 ⇒ p = 0) the step is simply empty
    // rz, pAp, rz_next, rr: slot groups (see "reduction slots")
    const double pap = read_slots(pAp), rzv = read_slots(rz);
    const double alpha = pap > 0.0 ? rzv / pap : 0.0;
    if (!(pap > 0.0) && rzv != 0.0 && blockIdx.x == 0 && threadIdx.x == 0) *flag = pap == 0.0 ? -1e-300 : pap;
    double a = 0.0, c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * Ap[i];
        r[i] = ri;
        a += ri * (dinv ? dinv[i] * ri : ri);
        c += ri * ri;
    }
    block_sum2_slots(a, c, rz_next, rr);
}

// p = D⁻¹ r + (rz_next / rz) p; one thread retires the scalars the next iteration accumulates into
// (rz, rz_next, retired, pAp, rr: slot groups; rr_out: the scalar the host reads — ‖r‖² of this iteration)
__global__ void __launch_bounds__(256)
k_cg_direction_dev(int64_t n, const double *__restrict__ rz, const double *__restrict__ rz_next, double *__restrict__ retired, double *__restrict__ pAp,
                   double *__restrict__ rr, double *__restrict__ rr_out, const double *__restrict__ r, const double *__restrict__ dinv, double *__restrict__ p)
{
    const double rzv = read_slots(rz), rzn = read_slots(rz_next);
    const double beta = rzv > 0.0 ? rzn / rzv : 0.0;
    if (blockIdx.x == 0 && threadIdx.x < 64) { // nobody else touches these three groups during this launch
        const double v = read_slots(rr);
        const int l = RED_STRIDE * threadIdx.x;
        retired[l] = 0.0; pAp[l] = 0.0; rr[l] = 0.0;
        if (threadIdx.x == 0) *rr_out = v;
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = (dinv ? dinv[i] * r[i] : r[i]) + beta * p[i];
}

int launch_cg(tb_pattern *pat, const double *A, const double *b, double *x, double rtol, double atol, int maxiter, int jacobi, int *iters,
              double *resnorm, bool b_is_residual)
{
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // reads scalars back (convergence looks)
    const int64_t n = pat->n_rows;
    double *r = krylov_ws(pat, 4 * (size_t)n + 8); // r, p, Ap, D⁻¹, 6 scalars; D⁻¹ outlives the solve for TB_JACOBI_REUSE (cg_dinv_of)
    if (!r) return TB_ERR_HIP;
    double *p = r + n, *Ap = p + n, *dinv = Ap + n, *scal = dinv + n;
    const unsigned g = grid_for(dev, n, 256);
    // TB_JACOBI_REUSE keeps D⁻¹ only when the slot holds the diagonal of THIS nz array (another operator of the pattern, a mass projection or a
    // Newton solve may have run in between): validity is tied to the array, the caller vouches that its values are unchanged
    if (jacobi == 1 || (jacobi == 2 && pat->cg_dinv_of != A)) { const int rcd = launch_extract_inverse_diagonal(pat, A, dinv); if (rcd) return rcd; }
    if (jacobi) pat->cg_dinv_of = A;
    const double *dp = jacobi ? dinv : nullptr;
    if (b_is_residual) TB_HIP(hipMemsetAsync(Ap, 0, sizeof(double) * n, dev->stream)); // r₀ = b given: nothing to subtract
    else { const int rc = launch_spmv(pat, A, x, 1.0, 0.0, Ap); if (rc) return rc; }
    TB_HIP(hipMemsetAsync(scal, 0, 6 * sizeof(double), dev->stream)); // scal[5]: sticky "pᵀAp ≤ 0" flag
    // k_cg_init writes r·z to out[0] and r·r to out[1]: point it at (scal[0], scal[1]) and move r·r to its slot afterwards
    hipLaunchKernelGGL(k_cg_init, dim3(g), dim3(256), 0, dev->stream, n, b, Ap, dp, r, p, scal);
    double h[3];
    TB_TRY(read_back(dev, h, scal, 2));
    // the loop's sums live in slot groups of the device ("reduction slots"): pᵀAp, r·z of the current / next / retired iteration (rotating), rᵀr
    double *const g_pap = red_group(dev, 3), *const g_rr = red_group(dev, 7);
    auto g_rz = [&](int k) { return red_group(dev, 4 + k); };
    TB_HIP(hipMemsetAsync(g_pap, 0, 5 * RED_GROUP * sizeof(double), dev->stream));
    TB_HIP(hipMemcpyAsync(g_rz(0), scal, sizeof(double), hipMemcpyDeviceToDevice, dev->stream)); // r·z of the start: slot 0 of the current group
    double rnorm = std::sqrt(h[1]);
    const double tol = stopping_tolerance(atol, rtol, rnorm);
    pat->last_tol = tol;
    // The host looks at (‖r‖², flag) once per `check` iterations: small systems are bound by the host round trip, not by the kernels, so they
    // run a few iterations between looks (at most check − 1 iterations past the tolerance); large ones look every iteration.
    static const int check_env = tune_env("TB_CG_CHECK_EVERY") ? atoi(tune_env("TB_CG_CHECK_EVERY")) : 0;
    const int check0 = check_env > 0 ? check_env : (n >= 262144 ? 1 : 4);
    int it = 0, cur = 0, last_look = 0;
    while (rnorm > tol && it < maxiter) {
        // long solves (elasticity: thousands of iterations) look less often still — every 4th iteration after 32, every 8th after 128 —
        // so a solve overshoots its tolerance by at most 6 % of its length, while short ones (the heat step: ~5) are checked every time
        const int check = check_env > 0 ? check_env : (it >= 128 ? 8 : it >= 32 ? std::max(check0, 4) : check0);
        const int nxt = (cur + 1) % 3, ret = (cur + 2) % 3;
        TB_TRY(launch_spmv_dot_slots(pat, A, p, Ap, g_pap));
        hipLaunchKernelGGL(k_cg_update_dev, dim3(g), dim3(256), 0, dev->stream, n, g_rz(cur), g_pap, p, Ap, dp, x, r, g_rz(nxt), g_rr, scal + 5);
        const bool look = it + 1 - last_look >= check || it + 1 == maxiter;
        if (look) last_look = it + 1;
        hipLaunchKernelGGL(k_cg_direction_dev, dim3(g), dim3(256), 0, dev->stream, n, g_rz(cur), g_rz(nxt), g_rz(ret), g_pap, g_rr, scal + 4, r, dp, p);
        if (look) TB_TRY(read_back_enqueue(dev, h, scal + 3, 3)); // (‖r‖² lands in scal[4] in the direction kernel)
        cur = nxt;
        ++it;
        if (!look) continue;
        TB_TRY(read_back_wait(dev));
        if (h[2] != 0.0) { set_error("tb_cg_solve: matrix is not positive definite (pᵀAp = %g)", h[2] == -1e-300 ? 0.0 : h[2]); return TB_ERR_BAD_ARG; }
        rnorm = std::sqrt(h[1]);
    }
    TB_HIP(hipGetLastError());
    if (iters) *iters = it;
    if (resnorm) *resnorm = rnorm;
    return TB_OK;
}

// ------------------------------------------------------------------------------------------------
// Restarted GMRES — the default inner solver of the reference's Newton–Raphson (LinearSolve.KrylovJL_GMRES(),
// src/solver/nonlinear/newton_raphson.jl:61; Krylov.jl is third party).  Needed where the tangent is not positive definite
// (non-polyconvex energies, follower loads).  Right Jacobi preconditioning (A D⁻¹ y = b, x = D⁻¹ y: the monitored residual is the
// true one), classical Gram–Schmidt with one re-orthogonalisation pass so that a whole Arnoldi step is eight launches and one
// host read: h = Vᵀw and w −= V h are single kernels over all basis vectors.
// ------------------------------------------------------------------------------------------------
// out[j · GM_HS] += V[j]·w for j < k (blockIdx.y = j)
constexpr int GM_HS = 16; // doubles between two Arnoldi coefficients on the device
__global__ void __launch_bounds__(256)
k_multi_dot(int64_t n, const double *__restrict__ V, const double *__restrict__ w, double *__restrict__ out)
{
    const double *v = V + (int64_t)blockIdx.y * n;
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) s += v[i] * w[i];
    block_sum_to(s, out + (size_t)blockIdx.y * GM_HS); // one 128-byte line per result: atomics on one line serialise (tb_reduce.hpp, "reduction slots")
}
// w += sign · Σ_{j<k} c[j] V[j];  optionally ww += w·w of the result
__global__ void __launch_bounds__(1024)
k_multi_axpy(int64_t n, int k, double sign, const double *__restrict__ c, int cstride, const double *__restrict__ V, double *__restrict__ w, double *__restrict__ ww)
{
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double s = 0.0;
        for (int j = 0; j < k; ++j) s += c[(size_t)j * cstride] * V[(int64_t)j * n + i];
        const double r = w[i] + sign * s;
        w[i] = r;
        acc += r * r;
    }
    if (ww) block_sum_to(acc, ww);
}
// y = a · (d ? d .* x : x)
__global__ void __launch_bounds__(256)
k_scale_diag(int64_t n, double a, const double *__restrict__ d, const double *__restrict__ x, double *__restrict__ y)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = a * (d ? d[i] * x[i] : x[i]);
}
// r = b − Ax; rr += r·r
__global__ void __launch_bounds__(256)
k_residual(int64_t n, const double *__restrict__ b, const double *__restrict__ Ax, double *__restrict__ r, double *__restrict__ rr)
{
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { const double v = b[i] - Ax[i]; r[i] = v; acc += v * v; }
    block_sum_to(acc, rr);
}
// x += d ? d .* t : t
__global__ void __launch_bounds__(256)
k_add_diag(int64_t n, const double *__restrict__ d, const double *__restrict__ t, double *__restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] += d ? d[i] * t[i] : t[i];
}

// The restarted GMRES loop of every fixed right preconditioner M (A M⁻¹ y = b, x = M⁻¹ y: the monitored residual is the true one), as pcg_loop is the
// loop of every CG preconditioner applied by launches.  V: restart + 1 basis vectors; w, z: n doubles each; sc: h1[(m+2)·GM_HS] | h2[(m+2)·GM_HS] | y[m+2].
// precondition(v, z) enqueues z = M⁻¹ v; correct(t, x) enqueues x += M⁻¹ t, where t is z and w is free for it to use.  `who` names the entry in the
// breakdown message.
template <class Precondition, class Correct>
static int gmres_loop(tb_pattern *pat, const double *A, const double *b, double *x, double rtol, double atol, int maxiter, int restart, double *V, double *w,
                      double *z, double *sc, Precondition precondition, Correct correct, const char *who, int *iters, double *resnorm)
{
    tb_device *dev = pat->mesh->dev;
    const int64_t n = pat->n_rows;
    const int m = restart;
    double *h1 = sc, *h2 = sc + (size_t)(m + 2) * GM_HS, *yd = sc + 2 * (size_t)(m + 2) * GM_HS;
    const unsigned g = grid_for(dev, n, 256);
    std::vector<double> H((size_t)(m + 1) * m), cs(m), sn(m), gvec(m + 1), yh(m), hh(2 * (size_t)(m + 2) * GM_HS);
    int it = 0;
    double rnorm = 0.0, tol = 0.0;
    bool first = true;
    while (true) {
        // r = b − A x → V[0] = r/‖r‖
        int rc = launch_spmv(pat, A, x, 1.0, 0.0, z);
        if (rc) return rc;
        TB_HIP(hipMemsetAsync(h1, 0, sizeof(double), dev->stream));
        hipLaunchKernelGGL(k_residual, dim3(g), dim3(256), 0, dev->stream, n, b, z, w, h1);
        TB_TRY(read_back(dev, hh.data(), h1, 1));
        rnorm = std::sqrt(hh[0]);
        if (first) { tol = stopping_tolerance(atol, rtol, rnorm); pat->last_tol = tol; first = false; }
        if (!(rnorm > tol) || it >= maxiter) break;
        hipLaunchKernelGGL(k_scale_diag, dim3(g), dim3(256), 0, dev->stream, n, 1.0 / rnorm, (const double *)nullptr, w, V);
        std::fill(gvec.begin(), gvec.end(), 0.0);
        gvec[0] = rnorm;
        int j = 0;
        double res_est = rnorm;
        for (; j < m && it < maxiter && res_est > tol; ++j, ++it) {
            // w = A M⁻¹ v_j
            rc = precondition((const double *)(V + (size_t)j * n), z);
            if (rc) return rc;
            rc = launch_spmv(pat, A, z, 1.0, 0.0, w);
            if (rc) return rc;
            TB_HIP(hipMemsetAsync(sc, 0, sizeof(double) * 2 * (m + 2) * GM_HS, dev->stream));
            // every workgroup of a dot ends in one atomic on its vector's result: ≈ 8 per CU in all (j + 1 vectors share them), each result on a line of its own
            const unsigned gd = std::max(1u, std::min(g, (unsigned)dev->n_cu * 8u / (unsigned)(j + 1)));
            hipLaunchKernelGGL(k_multi_dot, dim3(gd, j + 1), dim3(256), 0, dev->stream, n, V, w, h1);
            hipLaunchKernelGGL(k_multi_axpy, dim3(grid_red(dev, n)), dim3(1024), 0, dev->stream, n, j + 1, -1.0, h1, GM_HS, V, w, (double *)nullptr);
            hipLaunchKernelGGL(k_multi_dot, dim3(gd, j + 1), dim3(256), 0, dev->stream, n, V, w, h2);
            hipLaunchKernelGGL(k_multi_axpy, dim3(grid_red(dev, n)), dim3(1024), 0, dev->stream, n, j + 1, -1.0, h2, GM_HS, V, w, h2 + (size_t)(m + 1) * GM_HS); // ‖w‖² in the last slot
            TB_TRY(read_back(dev, hh.data(), sc, 2 * (size_t)(m + 2) * GM_HS));
            double *Hj = H.data() + (size_t)j * (m + 1);
            for (int i = 0; i <= j; ++i) Hj[i] = hh[(size_t)i * GM_HS] + hh[((size_t)(m + 2) + i) * GM_HS];
            const double wn = std::sqrt(hh[((size_t)(m + 2) + (m + 1)) * GM_HS]);
            Hj[j + 1] = wn;
            if (!std::isfinite(wn)) { set_error("%s: breakdown (non-finite Arnoldi vector)", who); return TB_ERR_BAD_ARG; }
            for (int i = 0; i < j; ++i) { const double t = cs[i] * Hj[i] + sn[i] * Hj[i + 1]; Hj[i + 1] = -sn[i] * Hj[i] + cs[i] * Hj[i + 1]; Hj[i] = t; }
            const double den = std::hypot(Hj[j], Hj[j + 1]);
            cs[j] = den > 0 ? Hj[j] / den : 1.0; sn[j] = den > 0 ? Hj[j + 1] / den : 0.0;
            Hj[j] = den; Hj[j + 1] = 0.0;
            gvec[j + 1] = -sn[j] * gvec[j]; gvec[j] = cs[j] * gvec[j];
            res_est = std::fabs(gvec[j + 1]);
            if (wn > 0.0 && j + 1 <= m) hipLaunchKernelGGL(k_scale_diag, dim3(g), dim3(256), 0, dev->stream, n, 1.0 / wn, (const double *)nullptr, w, V + (size_t)(j + 1) * n);
            if (wn == 0.0) { ++j; ++it; break; } // lucky breakdown: the Krylov space is invariant, the solution is exact in it
        }
        // y = H⁻¹ g (upper triangular), x += M⁻¹ V y
        for (int i = j - 1; i >= 0; --i) {
            double sacc = gvec[i];
            for (int l = i + 1; l < j; ++l) sacc -= H[(size_t)l * (m + 1) + i] * yh[l];
            yh[i] = sacc / H[(size_t)i * (m + 1) + i];
        }
        TB_HIP(hipMemcpyAsync(yd, yh.data(), sizeof(double) * j, hipMemcpyHostToDevice, dev->stream));
        TB_HIP(hipMemsetAsync(z, 0, sizeof(double) * n, dev->stream));
        hipLaunchKernelGGL(k_multi_axpy, dim3(grid_red(dev, n)), dim3(1024), 0, dev->stream, n, j, 1.0, yd, 1, V, z, (double *)nullptr);
        rc = correct((const double *)z, x);
        if (rc) return rc;
        TB_SYNC_STREAM(dev); // yh is reused by the next cycle
    }
    TB_HIP(hipGetLastError());
    if (iters) *iters = it;
    if (resnorm) *resnorm = rnorm;
    return TB_OK;
}

int launch_gmres(tb_pattern *pat, const double *A, const double *b, double *x, double rtol, double atol, int maxiter, int restart, int jacobi,
                 int *iters, double *resnorm)
{
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // reads scalars back (convergence looks)
    const int64_t n = pat->n_rows;
    const int m = restart;
    double *V = krylov_ws(pat, (size_t)(m + 4) * n + (2 * GM_HS + 1) * (size_t)(m + 2)); // (restart + 1) basis vectors, 3 vectors, scalars
    if (!V) return TB_ERR_HIP;
    pat->cg_dinv_of = nullptr; // the workspace no longer holds launch_cg's D⁻¹
    double *w = V + (size_t)(m + 1) * n, *z = w + n, *dinv = z + n, *sc = dinv + n;
    const unsigned g = grid_for(dev, n, 256);
    if (jacobi) { const int rcd = launch_extract_inverse_diagonal(pat, A, dinv); if (rcd) return rcd; }
    const double *dp = jacobi ? dinv : nullptr;
    auto precondition = [&](const double *v, double *y) -> int { // y = D⁻¹ v
        hipLaunchKernelGGL(k_scale_diag, dim3(g), dim3(256), 0, dev->stream, n, 1.0, dp, v, y);
        return TB_OK;
    };
    auto correct = [&](const double *t, double *xx) -> int { // x += D⁻¹ t
        hipLaunchKernelGGL(k_add_diag, dim3(g), dim3(256), 0, dev->stream, n, dp, t, xx);
        return TB_OK;
    };
    return gmres_loop(pat, A, b, x, rtol, atol, maxiter, restart, V, w, z, sc, precondition, correct, "tb_gmres_solve", iters, resnorm);
}

// GMRES with the fixed right preconditioner supplied by the caller as enqueue-only launches (tb_gmres_solve_mg, tb_gmres_solve_amg: one multigrid
// cycle per Arnoldi step and one more per restart cycle for x += M⁻¹(V y); no second basis is stored, so M must not change during the solve)
int launch_gmres_apply(tb_pattern *pat, const double *A, const double *b, double *x, double rtol, double atol, int maxiter, int restart,
                       int (*apply)(void *ctx, const double *r, double *z), void *ctx, const char *what, int *iters, double *resnorm)
{
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // reads scalars back (convergence looks)
    const int64_t n = pat->n_rows;
    const int m = restart;
    double *V = krylov_ws(pat, (size_t)(m + 3) * n + (2 * GM_HS + 1) * (size_t)(m + 2)); // (restart + 1) basis vectors, 2 vectors, scalars
    if (!V) return TB_ERR_HIP;
    pat->cg_dinv_of = nullptr; // the workspace no longer holds launch_cg's D⁻¹
    double *w = V + (size_t)(m + 1) * n, *z = w + n, *sc = z + n;
    const unsigned g = grid_for(dev, n, 256);
    auto precondition = [&](const double *v, double *y) -> int { return apply(ctx, v, y); };
    auto correct = [&](const double *t, double *xx) -> int { // x += M⁻¹ t: the cycle reads t throughout, so it lands in w (free between two cycles)
        const int rc = apply(ctx, t, w);
        if (rc) return rc;
        hipLaunchKernelGGL(k_add_diag, dim3(g), dim3(256), 0, dev->stream, n, (const double *)nullptr, (const double *)w, xx);
        return TB_OK;
    };
    return gmres_loop(pat, A, b, x, rtol, atol, maxiter, restart, V, w, z, sc, precondition, correct, what, iters, resnorm);
}

// ------------------------------------------------------------------------------------------------
// ℓ₁ Gauss–Seidel preconditioner (Baker, Falgout, Kolev, Yang, "Multigrid smoothers for ultraparallel computing", SIAM J. Sci. Comput.
// 33 (2011), §6) — the preconditioner the reference's documentation lists for its Krylov solves (Thunderbolt.Preconditioners.L1GSPrecBuilder
// with ForwardSweep / BackwardSweep / SymmetricSweep, docs/src/api-reference/solver.md:13-22; its source is not part of the reference
// checkout, so this restates the published algorithm: parity unpinned).  Rows are cut into partitions of `ps` consecutive rows; inside a
// partition the sweep is exact Gauss–Seidel, couplings that leave the partition are moved onto the diagonal by their ℓ₁ norm:
//   D̃_ii = a_ii + Σ_{j ∉ part(i)} |a_ij|;  forward: (D̃ + L_p) y = r;  symmetric: then (D̃ + U_p) z = D̃ y,
// i.e. M = (D̃ + L_p) D̃⁻¹ (D̃ + U_p), symmetric positive definite whenever A is.  One wavefront per partition: the rows are visited in
// order, the lanes share a row's entries; the partition's part of the iterate lives in LDS.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_l1gs_diag(int64_t n, int ps, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz, double *__restrict__ dt)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t lo = r / ps * ps, hi = lo + ps;
    double d = 0.0;
    for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
        const int32_t c = colidx[k];
        if (c == r) d += nz[k];
        else if (c < lo || c >= hi) d += fabs(nz[k]);
    }
    dt[r] = d;
}

template <bool SYMMETRIC>
__global__ void __launch_bounds__(256)
k_l1gs_apply(int64_t n, int ps, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz,
             const double *__restrict__ dt, const double *__restrict__ r, double *__restrict__ z)
{
    extern __shared__ double s_y[]; // [waves per block][ps]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t part = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    const int64_t lo = part * ps;
    if (lo >= n) return;
    const int64_t hi = lo + ps < n ? lo + ps : n;
    double *y = s_y + (size_t)wv * ps;
    for (int64_t i = lo; i < hi; ++i) { // forward sweep
        double acc = 0.0;
        for (int64_t k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) {
            const int32_t c = colidx[k];
            if (c >= lo && c < i) acc += nz[k] * y[c - lo];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) y[i - lo] = (r[i] - acc) / dt[i];
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (SYMMETRIC) {
        for (int64_t i = hi - 1; i >= lo; --i) { // backward sweep: z_i = y_i − Σ_{j > i in the partition} a_ij z_j / D̃_ii, in place
            double acc = 0.0;
            for (int64_t k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) {
                const int32_t c = colidx[k];
                if (c > i && c < hi) acc += nz[k] * y[c - lo];
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
            if (lane == 0) y[i - lo] -= acc / dt[i];
            __builtin_amdgcn_wave_barrier();
        }
    }
    for (int64_t i = lo + lane; i < hi; i += 64) z[i] = y[i - lo];
}

int launch_l1gs_setup(tb_pattern *pat, const double *A, int ps, double *d_dtilde)
{
    tb_device *dev = pat->mesh->dev;
    const int64_t n = pat->n_rows;
    hipLaunchKernelGGL(k_l1gs_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dev->stream, n, ps, pat->d_rowptr, pat->d_colidx, A, d_dtilde);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int launch_l1gs_apply(tb_pattern *pat, const double *A, const double *d_dtilde, int ps, int symmetric, const double *r, double *z)
{
    tb_device *dev = pat->mesh->dev;
    const int64_t n = pat->n_rows, nparts = (n + ps - 1) / ps;
    const size_t lds = sizeof(double) * 4 * (size_t)ps;
    const dim3 grid((unsigned)((nparts + 3) / 4)), block(256);
    if (symmetric) hipLaunchKernelGGL(k_l1gs_apply<true>, grid, block, lds, dev->stream, n, ps, pat->d_rowptr, pat->d_colidx, A, d_dtilde, r, z);
    else hipLaunchKernelGGL(k_l1gs_apply<false>, grid, block, lds, dev->stream, n, ps, pat->d_rowptr, pat->d_colidx, A, d_dtilde, r, z);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

// preconditioned CG with a general preconditioner application (two host reads per iteration): z = M⁻¹ r by ℓ₁ Gauss–Seidel
int launch_pcg_l1gs(tb_pattern *pat, const double *A, const double *b, double *x, double rtol, double atol, int maxiter, int ps, int *iters, double *resnorm)
{
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // reads scalars back (convergence looks)
    const int64_t n = pat->n_rows;
    double *r = krylov_ws(pat, 5 * (size_t)n + 8); // r, z, p, Ap, D̃, scalars
    if (!r) return TB_ERR_HIP;
    pat->cg_dinv_of = nullptr; // the workspace no longer holds launch_cg's D⁻¹
    double *z = r + n, *p = z + n, *Ap = p + n, *dtl = Ap + n, *scal = dtl + n;
    const unsigned g = grid_for(dev, n, 256);
    int rc = launch_l1gs_setup(pat, A, ps, dtl);
    if (rc) return rc;
    rc = launch_spmv(pat, A, x, 1.0, 0.0, Ap);
    if (rc) return rc;
    double h[2];
    TB_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(double), dev->stream));
    hipLaunchKernelGGL(k_residual, dim3(g), dim3(256), 0, dev->stream, n, b, Ap, r, scal);
    TB_TRY(read_back(dev, h, scal, 1));
    double rnorm = std::sqrt(h[0]);
    const double tol = stopping_tolerance(atol, rtol, rnorm);
    pat->last_tol = tol;
    int it = 0;
    double rz = 0.0;
    while (rnorm > tol && it < maxiter) {
        rc = launch_l1gs_apply(pat, A, dtl, ps, 1, r, z);
        if (rc) return rc;
        TB_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(double), dev->stream));
        enqueue_dot(dev, n, r, z, scal);
        TB_TRY(read_back(dev, h, scal, 1));
        const double rz_new = h[0];
        if (it == 0) TB_HIP(hipMemcpyAsync(p, z, sizeof(double) * n, hipMemcpyDeviceToDevice, dev->stream));
        else hipLaunchKernelGGL(k_cg_direction, dim3(g), dim3(256), 0, dev->stream, n, rz_new / rz, z, (const double *)nullptr, p);
        rz = rz_new;
        rc = launch_spmv(pat, A, p, 1.0, 0.0, Ap);
        if (rc) return rc;
        TB_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(double), dev->stream));
        enqueue_dot(dev, n, p, Ap, scal);
        TB_TRY(read_back(dev, h, scal, 1));
        if (!(h[0] > 0.0)) { set_error("tb_pcg_solve: matrix is not positive definite (pᵀAp = %g)", h[0]); return TB_ERR_BAD_ARG; }
        const double alpha = rz / h[0];
        TB_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(double), dev->stream));
        hipLaunchKernelGGL(k_cg_update, dim3(grid_red(dev, n)), dim3(1024), 0, dev->stream, n, alpha, p, Ap, (const double *)nullptr, x, r, scal);
        TB_TRY(read_back(dev, h, scal, 2));
        rnorm = std::sqrt(h[1]);
        ++it;
    }
    TB_HIP(hipGetLastError());
    if (iters) *iters = it;
    if (resnorm) *resnorm = rnorm;
    return TB_OK;
}

// ------------------------------------------------------------------------------------------------
// Chebyshev polynomial preconditioner (the smoother the reference's multigrid extension uses, docs: "damped Jacobi with Chebyshev-optimal ω",
// src/solver/linear/multigrid.jl:28-33 — here as a preconditioner of its own: M⁻¹ = p_m(D⁻¹A)·D⁻¹ with the degree-m Chebyshev polynomial of
// the interval [λmax/ratio, λmax] of D⁻¹A).  A fixed symmetric positive-definite operator, so plain PCG applies; it needs SpMVs and one fused
// vector kernel per degree and no inner products — a degree-m application costs m − 1 products and removes about m of every m + 1 outer
// iterations, i.e. the same number of products as Jacobi-CG but 1/m of its dot products, host looks and vector kernels (elasticity tangents:
// ≈2 000 Jacobi-CG iterations on a 10⁵-dof Q2 block).  λmax from 24 Lanczos steps (largest Ritz value + 5 %), capped by the Gershgorin bound.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_gershgorin(int64_t n, const int64_t *__restrict__ rowptr, const double *__restrict__ nz, const double *__restrict__ dinv, double *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double s = 0.0;
    for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k) s += fabs(nz[k]);
    out[r] = s * fabs(dinv[r]);
}
// Lanczos helpers: sq = √D⁻¹, v = a positive start vector (the Gershgorin row sums), v₋₁ = 0
__global__ void __launch_bounds__(256)
k_lanczos_init(int64_t n, const double *__restrict__ dinv, const double *__restrict__ start, double *__restrict__ sq, double *__restrict__ v, double *__restrict__ vp)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        sq[i] = sqrt(fabs(dinv[i]));
        v[i] = start[i] * (1.0 + 0.37 * (double)((i * 2654435761u) & 1023) / 1024.0); // perturbed so that symmetric modes are not missed
        vp[i] = 0.0;
    }
}
__global__ void __launch_bounds__(256) k_mul_to(int64_t n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ y)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = a[i] * b[i];
}
// w = sq∘w − β v₋₁;  out += w·v
__global__ void __launch_bounds__(1024)
k_lanczos_a(int64_t n, const double *__restrict__ sq, double beta, const double *__restrict__ vp, const double *__restrict__ v, double *__restrict__ w, double *__restrict__ out)
{
    double a = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double wi = sq[i] * w[i] - beta * vp[i];
        w[i] = wi;
        a += wi * v[i];
    }
    block_sum_to(a, out);
}
// w −= α v;  out += w·w
__global__ void __launch_bounds__(1024)
k_lanczos_b(int64_t n, double alpha, const double *__restrict__ v, double *__restrict__ w, double *__restrict__ out)
{
    double a = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double wi = w[i] - alpha * v[i];
        w[i] = wi;
        a += wi * wi;
    }
    block_sum_to(a, out);
}
__global__ void __launch_bounds__(256) k_scale_to(int64_t n, double s, const double *__restrict__ x, double *__restrict__ y)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] = s * x[i];
}
// p = z + β p with β = rz_new / rz from device scalars (β = 0 when rz = 0: first iteration)
__global__ void __launch_bounds__(256)
k_pcg_direction_dev(int64_t n, const double *__restrict__ rz, const double *__restrict__ rz_new, const double *__restrict__ z, double *__restrict__ p)
{
    const double beta = *rz > 0.0 ? *rz_new / *rz : 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = z[i] + beta * p[i];
}
// x += α p, r −= α Ap with α = rz_new / pAp from device scalars; rr += r·r; a non-positive pAp is remembered in *flag
__global__ void __launch_bounds__(1024)
k_pcg_update_dev(int64_t n, const double *__restrict__ rz_new, const double *__restrict__ pAp, const double *__restrict__ p, const double *__restrict__ Ap,
                 double *__restrict__ x, double *__restrict__ r, double *__restrict__ rr, double *__restrict__ flag)
{
    const double pap = *pAp;
    const double alpha = pap > 0.0 ? *rz_new / pap : 0.0;
    if (!(pap > 0.0) && *rz_new != 0.0 && blockIdx.x == 0 && threadIdx.x == 0) *flag = pap == 0.0 ? -1e-300 : pap;
    double c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * Ap[i];
        r[i] = ri;
        c += ri * ri;
    }
    block_sum_to(c, rr);
}

// λmax(D⁻¹A) of the Chebyshev preconditioner and of the multigrid smoother (tb_multigrid.hip).  w, v, vp, t, sq: five scratch vectors of n doubles,
// S2: two device scalars; dinv may hold zeros (dofs the caller has masked out: they drop out of the spectrum).  Reads scalars back.
int estimate_lambda_max(tb_pattern *pat, const double *A, const double *dinv, double *w, double *v, double *vp, double *t, double *sq, double *S2, double *lmax_out)
{
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // reads scalars back
    const int64_t n = pat->n_rows;
    const unsigned g = grid_for(dev, n, 256);
    int rc;
    // λmax(D⁻¹A) = λmax(D^-½ A D^-½): Gershgorin bound (safe, loose), sharpened by the largest Ritz value of 24 Lanczos steps (converges from
    // below, within a per cent after a few tens of steps) inflated by 5 % — an interval that misses the top of the spectrum would make the
    // polynomial indefinite there
    hipLaunchKernelGGL(k_gershgorin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, dev->stream, n, pat->d_rowptr, A, dinv, w);
    double gersh = 0.0;
    rc = launch_absmax(dev, n, w, 1, &gersh);
    if (rc) return rc;
    double lmax = gersh;
    {
        constexpr int KL = 24;
        double al[KL], be[KL + 1], h[2];
        hipLaunchKernelGGL(k_lanczos_init, dim3(g), dim3(256), 0, dev->stream, n, dinv, w, sq, v, vp);
        TB_HIP(hipMemsetAsync(S2, 0, 2 * sizeof(double), dev->stream));
        enqueue_dot(dev, n, v, v, S2);
        TB_TRY(read_back(dev, h, S2, 1));
        int kdone = 0;
        if (h[0] > 0.0) {
            hipLaunchKernelGGL(k_scale_to, dim3(g), dim3(256), 0, dev->stream, n, 1.0 / std::sqrt(h[0]), v, v);
            be[0] = 0.0;
            for (int k = 0; k < KL; ++k) {
                hipLaunchKernelGGL(k_mul_to, dim3(g), dim3(256), 0, dev->stream, n, sq, v, t);            // t = D^-½ v
                rc = launch_spmv(pat, A, t, 1.0, 0.0, w);                                                    // w = A t
                if (rc) return rc;
                TB_HIP(hipMemsetAsync(S2, 0, 2 * sizeof(double), dev->stream));
                hipLaunchKernelGGL(k_lanczos_a, dim3(grid_red(dev, n)), dim3(1024), 0, dev->stream, n, sq, be[k], vp, v, w, S2); // w = D^-½ w − β v₋₁; α = w·v
                TB_TRY(read_back(dev, h, S2, 1));
                al[k] = h[0];
                hipLaunchKernelGGL(k_lanczos_b, dim3(grid_red(dev, n)), dim3(1024), 0, dev->stream, n, al[k], v, w, S2 + 1);  // w −= α v; ‖w‖²
                TB_TRY(read_back(dev, h, S2 + 1, 1));
                kdone = k + 1;
                be[k + 1] = std::sqrt(h[0]);
                if (!(be[k + 1] > 1e-12 * std::fabs(al[k]))) break;                                           // invariant subspace: the Ritz values are exact
                TB_HIP(hipMemcpyAsync(vp, v, sizeof(double) * n, hipMemcpyDeviceToDevice, dev->stream));
                hipLaunchKernelGGL(k_scale_to, dim3(g), dim3(256), 0, dev->stream, n, 1.0 / be[k + 1], w, v);
            }
        }
        if (kdone > 0) {
            const double hi = largest_tridiagonal_eigenvalue(al, be, kdone);
            lmax = std::min(gersh, 1.05 * hi);
        }
    }
    *lmax_out = lmax;
    return TB_OK;
}

// The device-scalar PCG loop of the preconditioners that are applied by launches alone (Chebyshev polynomial, multigrid cycle): precondition()
// leaves z = M⁻¹ r.  r, z, p, Ap: n doubles each; S: rz | rz_new | pAp | rr | flag (8 doubles).  `what` names the operator in the
// not-positive-definite message.
template <class Precondition>
static int pcg_loop(tb_pattern *pat, const double *A, const double *b, double *x, double rtol, double atol, int maxiter, double *r, double *z, double *p,
                    double *Ap, double *S, Precondition precondition, const char *what, int *iters, double *resnorm)
{
    tb_device *dev = pat->mesh->dev;
    const int64_t n = pat->n_rows;
    const unsigned g = grid_for(dev, n, 256);
    int rc = launch_spmv(pat, A, x, 1.0, 0.0, Ap);
    if (rc) return rc;
    double h[3];
    TB_HIP(hipMemsetAsync(S, 0, 8 * sizeof(double), dev->stream));
    hipLaunchKernelGGL(k_residual, dim3(g), dim3(256), 0, dev->stream, n, b, Ap, r, S + 3);
    TB_TRY(read_back(dev, h, S + 3, 1));
    double rnorm = std::sqrt(h[0]);
    const double tol = stopping_tolerance(atol, rtol, rnorm);
    pat->last_tol = tol;
    int it = 0;
    while (rnorm > tol && it < maxiter) {
        const int look_every = it >= 64 ? 4 : 1;
        for (int s2 = 0; s2 < look_every && it < maxiter; ++s2, ++it) {
            rc = precondition();
            if (rc) return rc;
            // rz ← rz_new of the previous iteration; rz_new = r·z
            TB_HIP(hipMemcpyAsync(S, S + 1, sizeof(double), hipMemcpyDeviceToDevice, dev->stream));
            TB_HIP(hipMemsetAsync(S + 1, 0, 3 * sizeof(double), dev->stream));
            enqueue_dot(dev, n, r, z, S + 1);
            hipLaunchKernelGGL(k_pcg_direction_dev, dim3(g), dim3(256), 0, dev->stream, n, S, S + 1, z, p);
            rc = launch_spmv(pat, A, p, 1.0, 0.0, Ap);
            if (rc) return rc;
            enqueue_dot(dev, n, p, Ap, S + 2);
            hipLaunchKernelGGL(k_pcg_update_dev, dim3(grid_red(dev, n)), dim3(1024), 0, dev->stream, n, S + 1, S + 2, p, Ap, x, r, S + 3, S + 4);
        }
        TB_TRY(read_back(dev, h, S + 3, 2));
        if (h[1] != 0.0) { set_error("tb_pcg_solve: matrix or %s is not positive definite (pᵀAp = %g)", what, h[1] == -1e-300 ? 0.0 : h[1]); return TB_ERR_BAD_ARG; }
        rnorm = std::sqrt(h[0]);
    }
    TB_HIP(hipGetLastError());
    if (iters) *iters = it;
    if (resnorm) *resnorm = rnorm;
    return TB_OK;
}

// PCG with z = M⁻¹ r supplied by the caller as enqueue-only launches (tb_pcg_solve_mg: one multigrid cycle)
int launch_pcg_apply(tb_pattern *pat, const double *A, const double *b, double *x, double rtol, double atol, int maxiter,
                     int (*apply)(void *ctx, const double *r, double *z), void *ctx, const char *what, int *iters, double *resnorm)
{
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // reads scalars back (convergence looks)
    const int64_t n = pat->n_rows;
    double *r = krylov_ws(pat, 4 * (size_t)n + 8); // r, z, p, Ap, scalars
    if (!r) return TB_ERR_HIP;
    pat->cg_dinv_of = nullptr; // the workspace no longer holds launch_cg's D⁻¹
    double *z = r + n, *p = z + n, *Ap = p + n, *S = Ap + n;
    TB_HIP(hipMemsetAsync(p, 0, sizeof(double) * n, dev->stream)); // the first direction is p = z + 0·p: whatever a fresh workspace holds (a NaN pattern) must not enter it
    return pcg_loop(pat, A, b, x, rtol, atol, maxiter, r, z, p, Ap, S, [&]() -> int { return apply(ctx, r, z); }, what, iters, resnorm);
}

int launch_pcg_chebyshev(tb_pattern *pat, const double *A, const double *b, double *x, double rtol, double atol, int maxiter, int degree, int *iters, double *resnorm)
{
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // reads scalars back (convergence looks)
    const int64_t n = pat->n_rows;
    double *r = krylov_ws(pat, 7 * (size_t)n + 16); // r, z, p, Ap, D⁻¹, d, w, scalars
    if (!r) return TB_ERR_HIP;
    pat->cg_dinv_of = nullptr; // the workspace no longer holds launch_cg's D⁻¹
    double *z = r + n, *p = z + n, *Ap = p + n, *dinv = Ap + n, *d = dinv + n, *w = d + n, *S = w + n; // S: rz | rz_new | pAp | rr | flag | power sums
    int rc = launch_extract_inverse_diagonal(pat, A, dinv);
    if (rc) return rc;
    double lmax = 0.0;
    rc = estimate_lambda_max(pat, A, dinv, w, z, p, Ap, d, S + 8, &lmax); // scratch: the solver's vectors are not in use yet
    if (rc) return rc;
    static const double ratio_env = tune_env("TB_CHEB_RATIO") ? atof(tune_env("TB_CHEB_RATIO")) : 0.0;
    const int m = degree < 1 ? 1 : degree;
    const double ratio = ratio_env > 1.0 ? ratio_env : std::max(4.0, 1.8 * m * m);
    MgVectors v; // of the smoother: D⁻¹ and its two scratch vectors
    v.dinv = dinv; v.d = d; v.w = w;
    auto precondition = [&]() -> int { // z = p_m(D⁻¹A) D⁻¹ r: the multigrid smoother started from zero
        return cheb_smooth(dev, n, v, lmax, ratio, m, r, z, true, [&](const double *x, double *y) { return launch_spmv(pat, A, x, 1.0, 0.0, y); });
    };
    return pcg_loop(pat, A, b, x, rtol, atol, maxiter, r, z, p, Ap, S, precondition, "Chebyshev preconditioner", iters, resnorm);
}

// ---- sub-structured CG over several devices: weighted sums (a dof held by k ranks counts 1/k), every scalar in caller-owned device memory ----
__global__ void __launch_bounds__(256)
k_cgd_dot(int64_t n, const double *__restrict__ w, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out /* slot group */)
{
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) s += (w ? w[i] : 1.0) * a[i] * b[i];
    block_sum_slots(s, out);
}

// α = rz / pAp (device scalars, already summed over the ranks); x += α p, r −= α Ap; out[0] += Σ w r·(D⁻¹r), out[1] += Σ w r·r
// SL: pᵀAp is still in its slot group (the fused iteration: nothing folded it); the two sums always leave through slot groups g_rz, g_rr
template <bool SL>
__global__ void __launch_bounds__(256)
k_cgd_update(int64_t n, const double *__restrict__ w, const double *__restrict__ dinv, const double *__restrict__ p, const double *__restrict__ Ap,
             double *__restrict__ x, double *__restrict__ r, const double *__restrict__ rz, const double *__restrict__ pAp, double *__restrict__ out,
             double *__restrict__ g_rz, double *__restrict__ g_rr)
{
    const double pap = SL ? read_slots(pAp) : *pAp;
    const double alpha = pap > 0.0 ? *rz / pap : 0.0;
    // pᵀAp ≤ 0 while r·z ≠ 0: the operator is not positive definite (or the iteration broke down) — sticky flag in out[2], read by the host with ‖r‖²
    if (!(pap > 0.0) && *rz != 0.0 && blockIdx.x == 0 && threadIdx.x == 0) out[2] = pap == 0.0 ? -1e-300 : pap;
    double a = 0.0, c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * Ap[i];
        r[i] = ri;
        const double wi = w ? w[i] : 1.0;
        a += wi * ri * (dinv ? dinv[i] * ri : ri);
        c += wi * ri * ri;
    }
    block_sum2_slots(a, c, g_rz, g_rr);
}

// β = rz_new / rz (device scalars); p = D⁻¹ r + β p
template <bool SL>
__global__ void __launch_bounds__(256)
k_cgd_direction(int64_t n, const double *__restrict__ dinv, const double *__restrict__ r, double *__restrict__ p, const double *__restrict__ rz,
                const double *__restrict__ rz_new)
{
    const double rzn = SL ? read_slots(rz_new) : *rz_new;
    const double beta = *rz > 0.0 ? rzn / *rz : 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = (dinv ? dinv[i] * r[i] : r[i]) + beta * p[i];
}

// end of an iteration: rz ← rz_new, ‖r‖² parked in S[5] for the host's next look, the three accumulators (pAp, rz_new, rr) back to zero — one
// launch for what would be two copies and a fill
__global__ void k_cgd_rotate(double *__restrict__ S)
{
    if (threadIdx.x == 0) { S[0] = S[2]; S[5] = S[3]; S[1] = 0.0; S[2] = 0.0; S[3] = 0.0; }
}
// the same at the end of a fused iteration, whose sums are still in slot groups 0 (pᵀAp), 1 (r·z), 2 (rᵀr): r·z and ‖r‖² folded into S, the groups zeroed
__global__ void __launch_bounds__(64) k_cgd_rotate_slots(double *__restrict__ S, double *__restrict__ groups)
{
    const double rz = read_slots(groups + RED_GROUP), rr = read_slots(groups + 2 * RED_GROUP);
    const int l = RED_STRIDE * threadIdx.x;
    groups[l] = 0.0; groups[RED_GROUP + l] = 0.0; groups[2 * RED_GROUP + l] = 0.0;
    if (threadIdx.x == 0) { S[0] = rz; S[5] = rr; S[1] = 0.0; S[2] = 0.0; S[3] = 0.0; }
}
int launch_cgd_rotate(tb_device *dev, double *d_S)
{
    hipLaunchKernelGGL(k_cgd_rotate, dim3(1), dim3(64), 0, dev->stream, d_S);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int launch_cgd_dot(tb_device *dev, int64_t n, const double *w, const double *a, const double *b, double *d_out)
{
    if (n > 0) {
        hipLaunchKernelGGL(k_cgd_dot, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, w, a, b, red_group(dev, 0));
        fold_slots(dev, 0, d_out, 1);
    }
    TB_HIP(hipGetLastError());
    return TB_OK;
}
int launch_cgd_update(tb_device *dev, int64_t n, const double *w, const double *dinv, const double *p, const double *Ap, double *x, double *r,
                      const double *d_rz, const double *d_pAp, double *d_out3)
{
    if (n > 0) {
        hipLaunchKernelGGL(k_cgd_update<false>, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, w, dinv, p, Ap, x, r, d_rz, d_pAp, d_out3,
                           red_group(dev, 1), red_group(dev, 2));
        fold_slots(dev, 1, d_out3, 2); // out3[0] += r·z, out3[1] += rᵀr
    }
    TB_HIP(hipGetLastError());
    return TB_OK;
}
int launch_cgd_direction(tb_device *dev, int64_t n, const double *dinv, const double *r, double *p, const double *d_rz, const double *d_rz_new)
{
    if (n > 0) hipLaunchKernelGGL(k_cgd_direction<false>, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, dinv, r, p, d_rz, d_rz_new);
    TB_HIP(hipGetLastError());
    return TB_OK;
}
// One iteration of the device CG on a sub-domain without shared dofs, its three sums kept in slot groups 0–2 from kernel to kernel (no fold launches):
// SpMV with pᵀAp → update (reads the group) → direction (reads the group) → rotate (folds r·z and ‖r‖² into S, zeroes the groups)
int launch_cgd_iteration(tb_pattern *pat, const double *A, const double *dinv, double *x, double *r, double *p, double *Ap, double *d_S)
{
    tb_device *dev = pat->mesh->dev;
    const int64_t n = pat->n_rows;
    if (n == 0) return launch_cgd_rotate(dev, d_S);
    int rc = launch_spmv_dot_slots(pat, A, p, Ap, red_group(dev, 0));
    if (rc) return rc;
    hipLaunchKernelGGL(k_cgd_update<true>, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, (const double *)nullptr, dinv, p, Ap, x, r, d_S,
                       red_group(dev, 0), d_S + 2, red_group(dev, 1), red_group(dev, 2));
    hipLaunchKernelGGL(k_cgd_direction<true>, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, dinv, r, p, d_S, red_group(dev, 1));
    hipLaunchKernelGGL(k_cgd_rotate_slots, dim3(1), dim3(64), 0, dev->stream, d_S, red_group(dev, 0));
    TB_HIP(hipGetLastError());
    return TB_OK;
}

// ---- single-reduction (Chronopoulos–Gear) form of the same Jacobi-CG: one all-reduce of {γ, δ, ρ} per iteration ----
// Scalar block S (SEVEN doubles, include/tbhip.h): γ | δ | ρ | flag | γ_prev | α_prev | δ accumulator.  S[0:3] is the block the caller all-reduces;
// γ_prev = 0 marks the first iteration (β = 0, α = γ/δ).  The recurrence s = A·p replaces the product A·p: the only product is w = A·u.
// α and β from the scalar block, the same expression in the update kernel (every workgroup: the same bits) and in the fold (which keeps α for the
// next iteration).  den = δ − β·γ/α_prev is pᵀAp of this iteration.
__device__ __forceinline__ void cg1_scalars(const double *__restrict__ S, double &alpha, double &beta, double &den)
{
    const double gam = S[0], gp = S[4];
    beta = gp != 0.0 ? gam / gp : 0.0;
    den = beta != 0.0 ? S[1] - beta * gam / S[5] : S[1];
    alpha = den > 0.0 ? gam / den : 0.0;
}

// p = u + β p, s = w + β s, x += α p, r −= α s, u = D⁻¹ r;  γ-partials Σ wt·r·u → group g_gam, ρ-partials Σ wt·r·r → group g_rho
__global__ void __launch_bounds__(256)
k_cg1_update(int64_t n, const double *__restrict__ wt, const double *__restrict__ dinv, const double *__restrict__ w, double *__restrict__ p,
             double *__restrict__ s, double *__restrict__ x, double *__restrict__ r, double *__restrict__ u, double *__restrict__ S,
             double *__restrict__ g_gam, double *__restrict__ g_rho)
{
    double alpha, beta, den;
    cg1_scalars(S, alpha, beta, den);
    // pᵀAp ≤ 0 while γ ≠ 0: not positive definite (or broken down) — the sticky flag of tb_cgd_update, in S[3]; the step is then empty in x and r
    if (!(den > 0.0) && S[0] != 0.0 && blockIdx.x == 0 && threadIdx.x == 0) S[3] = den == 0.0 ? -1e-300 : den;
    double a = 0.0, c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double pi = u[i] + beta * p[i];
        const double si = w[i] + beta * s[i];
        p[i] = pi; s[i] = si;
        x[i] += alpha * pi;
        const double ri = r[i] - alpha * si;
        r[i] = ri;
        const double ui = dinv ? dinv[i] * ri : ri;
        u[i] = ui;
        const double wi = wt ? wt[i] : 1.0;
        a += wi * ri * ui;
        c += wi * ri * ri;
    }
    block_sum2_slots(a, c, g_gam, g_rho);
}

// one wave: α of the iteration just updated is kept (α_prev ← α, γ_prev ← γ), then S[0:3] ← {Σ group g_gam, Σ group g_del + S[6], Σ group g_rho};
// S[6] and the three groups back to zero.  The δ partial arrives either in group g_del (the one-call form) or in S[6] (tb_spmv_csr_dot folds into a
// caller scalar); adding the other, zero, term is exact, so both forms leave the same sum.
__global__ void __launch_bounds__(64) k_cg1_fold(double *__restrict__ S, double *__restrict__ g_del, double *__restrict__ g_gam, double *__restrict__ g_rho)
{
    const double gam = read_slots(g_gam), del = read_slots(g_del), rho = read_slots(g_rho);
    const int l = RED_STRIDE * threadIdx.x;
    g_del[l] = 0.0; g_gam[l] = 0.0; g_rho[l] = 0.0;
    if (threadIdx.x == 0) {
        double alpha, beta, den;
        cg1_scalars(S, alpha, beta, den);
        S[4] = S[0]; S[5] = alpha;
        S[0] = gam; S[1] = del + S[6]; S[2] = rho; S[6] = 0.0;
    }
}

int launch_cg1_update(tb_device *dev, int64_t n, const double *wt, const double *dinv, const double *w, double *p, double *s, double *x, double *r,
                      double *u, double *d_S)
{
    // launched for n == 0 too (one workgroup, no elements): the breakdown test reads only the all-reduced scalars, so an empty part raises its flag
    // in the same iteration as its peers
    const unsigned g = n > 0 ? grid_for(dev, n, 256) : 1u;
    hipLaunchKernelGGL(k_cg1_update, dim3(g), dim3(256), 0, dev->stream, n, wt, dinv, w, p, s, x, r, u, d_S, red_group(dev, 1), red_group(dev, 2));
    TB_HIP(hipGetLastError());
    return TB_OK;
}
int launch_cg1_fold(tb_device *dev, double *d_S)
{
    hipLaunchKernelGGL(k_cg1_fold, dim3(1), dim3(64), 0, dev->stream, d_S, red_group(dev, 0), red_group(dev, 1), red_group(dev, 2));
    TB_HIP(hipGetLastError());
    return TB_OK;
}
// One iteration on a sub-domain without shared dofs: update (weights = 1) → w = A·u with the partial of uᵀAu left in slot group 0 → fold.  Three launches.
int launch_cg1_iteration(tb_pattern *pat, const double *A, const double *dinv, double *x, double *r, double *u, double *p, double *s, double *w, double *d_S)
{
    tb_device *dev = pat->mesh->dev;
    const int64_t n = pat->n_rows;
    int rc = launch_cg1_update(dev, n, nullptr, dinv, w, p, s, x, r, u, d_S);
    if (rc) return rc;
    if (n > 0 && (rc = launch_spmv_dot_slots(pat, A, u, w, red_group(dev, 0)))) return rc;
    return launch_cg1_fold(dev, d_S);
}

} // namespace tb

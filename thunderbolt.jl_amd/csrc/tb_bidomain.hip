// tb_bidomain.hip — the coupled solve of the parabolic–elliptic bidomain model (ParabolicEllipticBidomainModel, src/modeling/electrophysiology.jl:305-326,
// "Not implemented yet" in the reference): backward Euler on the transformed system,
//   [ M − Δt Kᵢ      −Δt Kᵢ        ] [φₘ⁺]   [ M φₘ + source_m ]
//   [ −Δt Kᵢ         −Δt (Kᵢ + Kₑ) ] [φₑ⁺] = [ source_e        ]
// with φₑ grounded at listed dofs (rows and columns of those φₑ dofs eliminated, `ground_diag` on the diagonal), over the scalar pattern of M, Kᵢ, Kₑ.
//   tb_bidomain_set_matrices   one pass over the three value arrays: the per-non-zero triple (a₁₁, a₁₂, a₂₂), the column stream and the inverse 2 × 2
//                              diagonal blocks (the preconditioner)
//   tb_bidomain_apply          y = A x, all four blocks in one pass over the index stream (k_bd_apply)
//   tb_bidomain_solve          block-Jacobi PCG: the loop of launch_cg (device scalars in slot groups, tb_reduce.hpp) with the look cadence of pcg_loop
//   tb_bidomain_pack / unpack  between the caller's two vectors (φₘ, φₑ) and the node-interleaved layout
// Layout.  The unknown is node-interleaved, (φₘ,ⱼ, φₑ,ⱼ) one aligned 16-byte pair, so a non-zero gathers once for four products.  The matrix is stored
// like the sliced mirror of tb_spmv.hip: per slice of 64 consecutive rows, entry k of all 64 rows side by side, padded to the longest row of the slice —
// three value planes (a₁₁, a₁₂, a₂₂) and one plane of 32-bit columns, every load of the product a coalesced run, a row summed by its one lane in entry
// order: no LDS, no shuffles, no atomics, the same bits every time.  Bit 31 of a column says "this φₑ column is grounded" (its φₑ counts as zero); a
// padding entry points at the lane's own row with zero values.  28 B per non-zero and one gather, against 48 B and four gathers of four CSR products.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tb_bidomain_internal.hpp"
#include "tb_internal.h"
#include "tb_reduce.hpp"

namespace tb {

// The triple of one non-zero, every operation rounded on its own (no contraction into fused multiply-adds): the −Δt kᵢ inside a₁₁ is then the very
// a₁₂, as the null vector (0, 1) of the ungrounded matrix wants it, and the stored operator is bit for bit the matrix a host forms from the same arrays
// — on a block matrix of condition 1e5 and more an ε-sized disagreement between the two shows as 1e-11 in the solution.
__device__ __forceinline__ void bd_combine(double m, double ki, double ke, double dt, double &a11, double &a12, double &a22)
{
    double tk = dt * ki;
    asm volatile("" : "+v"(tk)); // the product is a value of its own: the unit is built with -ffp-contract=fast, which fuses across a pragma as well
    a11 = m - tk; a12 = -tk; a22 = -(dt * (ki + ke));
}

// (M, Kᵢ, Kₑ) → value planes, column plane, block inverses, one lane per row of a slice.  CSR reads, slice-ordered coalesced writes.
__global__ void __launch_bounds__(256)
k_bd_fill(int64_t n, int64_t n_slices, const int64_t *__restrict__ base, int64_t entries, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
          const double *__restrict__ M, const double *__restrict__ Ki, const double *__restrict__ Ke, double dt, const uint8_t *__restrict__ ground, double gdiag,
          uint32_t *__restrict__ col, double *__restrict__ val, double *__restrict__ binv, uint8_t *__restrict__ gkeep)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_slices * 64) return;
    const int64_t slice = row >> 6, b0 = base[slice];
    const int W = (int)((base[slice + 1] - b0) >> 6), lane = (int)(row & 63);
    const bool valid = row < n;
    const int64_t rc = valid ? row : n - 1; // (lanes past the last row: padding only)
    const int64_t pa = rowptr[rc];
    const int len = valid ? (int)(rowptr[rc + 1] - pa) : 0;
    double d11 = 0.0, d12 = 0.0, d22 = 0.0;
    uint32_t *cs = col + b0 + lane;
    double *v11 = val + b0 + lane, *v12 = v11 + entries, *v22 = v12 + entries;
    for (int k = 0; k < W; ++k) {
        uint32_t c = (uint32_t)rc;
        double a11 = 0.0, a12 = 0.0, a22 = 0.0;
        if (k < len) {
            const int32_t j = colidx[pa + k];
            const double ki = Ki[pa + k];
            bd_combine(M[pa + k], ki, Ke[pa + k], dt, a11, a12, a22);
            c = (uint32_t)j | (ground[j] ? BD_GROUNDED : 0u);
            if (j == row) { d11 = a11; d12 = a12; d22 = a22; }
        }
        cs[64 * (int64_t)k] = c; v11[64 * (int64_t)k] = a11; v12[64 * (int64_t)k] = a12; v22[64 * (int64_t)k] = a22;
    }
    if (!valid) return;
    const uint8_t g = ground[row];
    gkeep[row] = g;
    if (g) { d12 = 0.0; d22 = gdiag; }
    const double det = d11 * d22 - d12 * d12;
    const bool ok = det != 0.0 && det == det; // (no stored diagonal: the identity, as launch_extract_inverse_diagonal leaves 1)
    binv[3 * row] = ok ? d22 / det : 1.0; binv[3 * row + 1] = ok ? -d12 / det : 0.0; binv[3 * row + 2] = ok ? d11 / det : 1.0;
}

// out = (m, e) interleaved; e = NULL: zeros; zero_ground: the φₑ entry of a grounded node becomes 0 (the right-hand side of an eliminated row)
__global__ void __launch_bounds__(256)
k_bd_pack(int64_t n, const double *__restrict__ m, const double *__restrict__ e, const uint8_t *__restrict__ ground, int zero_ground, double2 *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = make_double2(m[i], e && !(zero_ground && ground[i]) ? e[i] : 0.0);
}
__global__ void __launch_bounds__(256) k_bd_unpack(int64_t n, const double2 *__restrict__ in, double *__restrict__ m, double *__restrict__ e)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { const double2 v = in[i]; if (m) m[i] = v.x; if (e) e[i] = v.y; }
}

// the three vector kernels of launch_cg (tb_krylov.hip) on node pairs, B⁻¹ in the place of D⁻¹ — same scalars, same slot groups, same sticky flag
// r = b − Ax (Ax given), p = B⁻¹ r;  out[0] += r·z, out[1] += r·r
__global__ void __launch_bounds__(256)
k_bd_init(int64_t n, const double2 *__restrict__ b, const double2 *__restrict__ Ax, const double *__restrict__ binv, double2 *__restrict__ r, double2 *__restrict__ p,
          double *__restrict__ out)
{
    double rz = 0.0, rr = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double2 bi = b[i], ai = Ax[i];
        const double2 ri = make_double2(bi.x - ai.x, bi.y - ai.y), zi = bd_precondition(binv, i, ri);
        r[i] = ri; p[i] = zi;
        rz += ri.x * zi.x + ri.y * zi.y; rr += ri.x * ri.x + ri.y * ri.y;
    }
    block_sum_to(rz, out);
    __syncthreads();
    block_sum_to(rr, out + 1);
}
__global__ void __launch_bounds__(256)
k_bd_update(int64_t n, const double *__restrict__ rz, const double *__restrict__ pAp, const double2 *__restrict__ p, const double2 *__restrict__ Ap,
            const double *__restrict__ binv, double2 *__restrict__ x, double2 *__restrict__ r, double *__restrict__ rz_next, double *__restrict__ rr, double *__restrict__ flag)
{
    const double pap = read_slots(pAp), rzv = read_slots(rz);
    const double alpha = pap > 0.0 ? rzv / pap : 0.0;
    if (!(pap > 0.0) && rzv != 0.0 && blockIdx.x == 0 && threadIdx.x == 0) *flag = pap == 0.0 ? -1e-300 : pap;
    double a = 0.0, c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double2 pi = p[i], api = Ap[i];
        double2 xi = x[i], ri = r[i];
        xi.x += alpha * pi.x; xi.y += alpha * pi.y;
        ri.x -= alpha * api.x; ri.y -= alpha * api.y;
        x[i] = xi; r[i] = ri;
        const double2 zi = bd_precondition(binv, i, ri);
        a += ri.x * zi.x + ri.y * zi.y;
        c += ri.x * ri.x + ri.y * ri.y;
    }
    block_sum2_slots(a, c, rz_next, rr);
}
__global__ void __launch_bounds__(256)
k_bd_direction(int64_t n, const double *__restrict__ rz, const double *__restrict__ rz_next, double *__restrict__ retired, double *__restrict__ pAp, double *__restrict__ rr,
               double *__restrict__ rr_out, const double2 *__restrict__ r, const double *__restrict__ binv, double2 *__restrict__ p)
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
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double2 zi = bd_precondition(binv, i, r[i]), pi = p[i];
        p[i] = make_double2(zi.x + beta * pi.x, zi.y + beta * pi.y);
    }
}

static void free_bidomain(tb_bidomain *h)
{
    if (!h) return;
    (void)hipFree(h->d_base); (void)hipFree(h->d_col); (void)hipFree(h->d_val); (void)hipFree(h->d_binv); (void)hipFree(h->d_ground); (void)hipFree(h->d_ws);
    delete h;
}

// Block-Jacobi PCG on the interleaved system: launch_cg's loop (one look = one 24-byte copy behind the direction kernel), looking at every iteration
// up to the 64th and at every fourth from there, as pcg_loop does.
static int bidomain_pcg(tb_bidomain *h, const double *b, double *x, double rtol, double atol, int maxiter, int *iters, double *resnorm)
{
    tb_pattern *pat = h->pat;
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // reads scalars back (convergence looks)
    const int64_t n = h->n;
    double *r = h->d_ws, *p = r + 2 * n, *Ap = p + 2 * n, *scal = Ap + 2 * n; // scal: r·z, r·r of the start | – | – , rᵀr, flag
    const unsigned g = grid_for(dev, n, 256);
    enqueue_apply<false>(h, x, Ap, nullptr);
    TB_HIP(hipMemsetAsync(scal, 0, 6 * sizeof(double), dev->stream));
    hipLaunchKernelGGL(k_bd_init, dim3(g), dim3(256), 0, dev->stream, n, (const double2 *)b, (const double2 *)Ap, h->d_binv, (double2 *)r, (double2 *)p, scal);
    double hh[3];
    TB_TRY(read_back(dev, hh, scal, 2));
    double *const g_pap = red_group(dev, 3), *const g_rr = red_group(dev, 7);
    auto g_rz = [&](int k) { return red_group(dev, 4 + k); };
    TB_HIP(hipMemsetAsync(g_pap, 0, 5 * RED_GROUP * sizeof(double), dev->stream));
    TB_HIP(hipMemcpyAsync(g_rz(0), scal, sizeof(double), hipMemcpyDeviceToDevice, dev->stream));
    double rnorm = std::sqrt(hh[1]);
    const double tol = stopping_tolerance(atol, rtol, rnorm);
    pat->last_tol = tol;
    int it = 0, cur = 0;
    while (rnorm > tol && it < maxiter) {
        const int nxt = (cur + 1) % 3, ret = (cur + 2) % 3;
        enqueue_apply<true>(h, p, Ap, g_pap);
        hipLaunchKernelGGL(k_bd_update, dim3(g), dim3(256), 0, dev->stream, n, g_rz(cur), g_pap, (const double2 *)p, (const double2 *)Ap, h->d_binv, (double2 *)x, (double2 *)r,
                           g_rz(nxt), g_rr, scal + 5);
        hipLaunchKernelGGL(k_bd_direction, dim3(g), dim3(256), 0, dev->stream, n, g_rz(cur), g_rz(nxt), g_rz(ret), g_pap, g_rr, scal + 4, (const double2 *)r, h->d_binv,
                           (double2 *)p);
        cur = nxt;
        ++it;
        const bool look = it <= 64 || it % 4 == 0 || it == maxiter;
        if (!look) continue;
        TB_TRY(read_back(dev, hh, scal + 3, 3)); // (‖r‖² lands in scal[4] in the direction kernel)
        if (hh[2] != 0.0) { set_error("tb_bidomain_solve: matrix or block-Jacobi preconditioner is not positive definite (pᵀAp = %g)", hh[2] == -1e-300 ? 0.0 : hh[2]); return TB_ERR_BAD_ARG; }
        rnorm = std::sqrt(hh[1]);
    }
    TB_HIP(hipGetLastError());
    if (iters) *iters = it;
    if (resnorm) *resnorm = rnorm;
    return TB_OK;
}

} // namespace tb

using namespace tb;

extern "C" {

int tb_bidomain_create(tb_pattern *pat, tb_bidomain **out)
{
    TB_REQUIRE(pat && out, "tb_bidomain_create: NULL argument");
    *out = nullptr;
    tb_mesh *m = pat->mesh;
    if (m->ncomp != 1 || kind_order(m->field_kind) != 1) {
        set_error("tb_bidomain_create: field kind %d with %d component(s) - the bidomain block system is built over the pattern of a scalar first-order field", m->field_kind, m->ncomp);
        return TB_ERR_UNSUPPORTED;
    }
    tb_device *dev = m->dev;
    TB_NO_CAPTURE(dev); // allocates and uploads the slice table
    TB_HIP(hipSetDevice(dev->id));
    const int64_t n = pat->n_rows;
    TB_REQUIRE(n > 0 && (int64_t)pat->h_rowptr.size() == n + 1, "tb_bidomain_create: the pattern has no rows");
    std::unique_ptr<tb_bidomain, void (*)(tb_bidomain *)> h(new tb_bidomain, free_bidomain);
    h->pat = pat; h->n = n; h->n_slices = (n + 63) / 64;
    std::vector<int64_t> base((size_t)h->n_slices + 1, 0);
    for (int64_t s = 0; s < h->n_slices; ++s) {
        int64_t w = 0;
        for (int64_t r = 64 * s; r < std::min<int64_t>(n, 64 * s + 64); ++r) w = std::max(w, pat->h_rowptr[r + 1] - pat->h_rowptr[r]);
        base[s + 1] = base[s] + 64 * w;
    }
    h->entries = base.back();
    TB_TRY(upload(dev, base, &h->d_base));
    TB_HIP(hipMalloc((void **)&h->d_col, std::max<size_t>(1, (size_t)h->entries) * sizeof(uint32_t)));
    TB_HIP(hipMalloc((void **)&h->d_val, std::max<size_t>(1, 3 * (size_t)h->entries) * sizeof(double)));
    TB_HIP(hipMalloc((void **)&h->d_binv, 3 * (size_t)n * sizeof(double)));
    TB_HIP(hipMalloc((void **)&h->d_ground, (size_t)n));
    TB_HIP(hipMalloc((void **)&h->d_ws, (6 * (size_t)n + 8) * sizeof(double)));
    *out = h.release();
    return TB_OK;
}

int tb_bidomain_destroy(tb_bidomain *h)
{
    free_bidomain(h);
    return TB_OK;
}

int tb_bidomain_set_matrices(tb_bidomain *h, tb_pattern *pat, const double *d_M, const double *d_Ki, const double *d_Ke, double dt, const uint8_t *d_ground, double ground_diag)
{
    TB_REQUIRE(h && pat && d_M && d_Ki && d_Ke && d_ground, "tb_bidomain_set_matrices: NULL argument");
    TB_REQUIRE(pat == h->pat, "tb_bidomain_set_matrices: the value arrays belong to another pattern than the one this block system was created for");
    TB_REQUIRE(std::isfinite(dt) && dt > 0.0, "tb_bidomain_set_matrices: dt = %g (needs a finite dt > 0)", dt);
    TB_REQUIRE(std::isfinite(ground_diag) && ground_diag > 0.0, "tb_bidomain_set_matrices: ground_diag = %g (needs a finite value > 0: the diagonal of the eliminated rows)", ground_diag);
    tb_device *dev = pat->mesh->dev;
    TB_HIP(hipSetDevice(dev->id));
    h->ground_diag = ground_diag;
    hipLaunchKernelGGL(k_bd_fill, dim3((unsigned)((h->n_slices * 64 + 255) / 256)), dim3(256), 0, dev->stream, h->n, h->n_slices, h->d_base, h->entries, pat->d_rowptr, pat->d_colidx,
                       d_M, d_Ki, d_Ke, dt, d_ground, ground_diag, h->d_col, h->d_val, h->d_binv, h->d_ground);
    TB_HIP(hipGetLastError());
    h->have_matrices = true;
    ++h->generation;
    return TB_OK;
}

int tb_bidomain_apply(tb_bidomain *h, const double *d_x, double *d_y)
{
    TB_REQUIRE(h && d_x && d_y, "tb_bidomain_apply: NULL argument");
    TB_REQUIRE(h->have_matrices, "tb_bidomain_apply: no matrices yet (tb_bidomain_set_matrices)");
    TB_REQUIRE(d_x != d_y, "tb_bidomain_apply: x and y must not alias");
    BD_ALIGNED(d_x, "tb_bidomain_apply"); BD_ALIGNED(d_y, "tb_bidomain_apply");
    enqueue_apply<false>(h, d_x, d_y, nullptr);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_bidomain_solve(tb_bidomain *h, const double *d_b, double *d_x, double rtol, double atol, int maxiter, int *iters, double *resnorm)
{
    TB_REQUIRE(h && d_b && d_x, "tb_bidomain_solve: NULL argument");
    TB_REQUIRE(h->have_matrices, "tb_bidomain_solve: no matrices yet (tb_bidomain_set_matrices)");
    TB_REQUIRE(rtol >= 0 && atol >= 0 && maxiter >= 0, "tb_bidomain_solve: negative tolerance or iteration limit");
    BD_ALIGNED(d_b, "tb_bidomain_solve"); BD_ALIGNED(d_x, "tb_bidomain_solve");
    TB_HIP(hipSetDevice(h->pat->mesh->dev->id));
    return bidomain_pcg(h, d_b, d_x, rtol, atol, maxiter, iters, resnorm);
}

int tb_bidomain_pack(tb_bidomain *h, const double *d_m, const double *d_e, int zero_ground, double *d_out)
{
    TB_REQUIRE(h && d_m && d_out, "tb_bidomain_pack: NULL argument");
    TB_REQUIRE(!zero_ground || h->have_matrices, "tb_bidomain_pack: zero_ground needs the ground of tb_bidomain_set_matrices");
    BD_ALIGNED(d_out, "tb_bidomain_pack");
    tb_device *dev = h->pat->mesh->dev;
    hipLaunchKernelGGL(k_bd_pack, dim3(grid_for(dev, h->n, 256)), dim3(256), 0, dev->stream, h->n, d_m, d_e, h->d_ground, zero_ground, (double2 *)d_out);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_bidomain_unpack(tb_bidomain *h, const double *d_in, double *d_m, double *d_e)
{
    TB_REQUIRE(h && d_in && (d_m || d_e), "tb_bidomain_unpack: NULL argument");
    BD_ALIGNED(d_in, "tb_bidomain_unpack");
    tb_device *dev = h->pat->mesh->dev;
    hipLaunchKernelGGL(k_bd_unpack, dim3(grid_for(dev, h->n, 256)), dim3(256), 0, dev->stream, h->n, (const double2 *)d_in, d_m, d_e);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

} // extern "C"

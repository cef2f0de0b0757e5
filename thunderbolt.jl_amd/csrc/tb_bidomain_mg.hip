// tb_bidomain_mg.hip — geometric multigrid preconditioner of the bidomain block system (tb_bidomain.hip) on the nested hexahedral grids of a tb_mg:
// one V(degree, degree) cycle on node pairs (φₘ, φₑ) and the conjugate gradients it preconditions.
//   hierarchy   levels 0 … L−1 of the tb_mg (finest: the block system's pattern); ground flags g_l — a coarse node is grounded iff the fine node it
//               coincides with is; block transfer 𝒫 = diag(P, G_f P G_c) with P the scalar nodal transfer and G the 0/1 diagonal of the free nodes: φₘ
//               interpolates everywhere, φₑ neither into a grounded fine node nor from a grounded coarse node; 𝒜_c = 𝒫ᵀ𝒜_f𝒫, the eliminated φₑφₑ
//               diagonal entries set to the mean |diagonal| of the level's free φₑφₑ entries (k_mg_fill_diag, as on a scalar level)
//   storage     the fine level is the block system's own (three planes, one a₁₂ for both off-diagonal blocks, ground flags in flight).  Pᵀ A₁₂ G_f P G_c
//               is NOT a symmetric n × n matrix once a grounded fine node is no coarse node, so coarse levels keep full 2 × 2 blocks per non-zero
//               (a₁₁, a₁₂, a₂₁, a₂₂) with the elimination baked in: k_bd_apply<·, true>.  Every level also keeps the four planes in CSR order: the
//               input of the next Galerkin product and what the read-outs return.
//   set-up      per level, top down: masked CSR planes → the scalar hierarchy's unflagged per-dof Galerkin plan once per plane (launch_galerkin_plane:
//               the term lists are reused, not rebuilt) → coarse rows and columns masked → diagonal fill → sliced planes, masked block inverses,
//               λmax(B⁻¹𝒜) by 24 Lanczos steps in the B inner product; dense inverse of the coarsest level (at most 512 nodes)
//   smoother    Chebyshev on B⁻¹𝒜 over [λmax/ratio, λmax], B the 2 × 2 node diagonal blocks; a step is ONE pass over the matrix (k_bd_apply<·, ·, STEP>:
//               the row's lane finishes d ← c₁d + c₂B⁻¹(r − 𝒜x), x_out ← x_in + d in registers, x ping-pongs between two buffers)
// No kernel of the set-up or of the cycle uses an atomic and every sum of theirs has one recorded order at every size: two set-ups give the same level planes
// and the same λmax, two applications the same bits.  The solve keeps its scalars in slot groups as tb_bidomain_solve does (ordered up to 64 workgroups).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "tb_bidomain_internal.hpp"
#include "tb_internal.h"
#include "tb_mg_internal.hpp"
#include "tb_reduce.hpp"

struct tb_bidomain_mg {
    tb_bidomain *bd = nullptr;
    tb_mg *mg = nullptr;
    tb_device *dev = nullptr;
    std::vector<tb::BdMgLevel> lv;
    int degree = 2;
    double ratio = 4.0;
    bool ready = false, split = false; // split: product + vector kernel per smoothing step (profiling build, TB_BDMG_SMOOTHER=split)
    uint64_t set_for = 0;              // generation of the block system the set-up read
    double *d_cinv = nullptr;          // (2 n₀)²: dense inverse of the coarsest operator on interleaved unknowns
    double *d_scal = nullptr;          // 8 scalars: λmax estimate, solve
    double *d_part = nullptr;          // one partial sum per workgroup of the λmax estimate's ordered reductions (8 · CUs)
    double *d_ws = nullptr;            // z, p, Ap, r of the solve (2n each)
    tb::BdCycle cycle_record() const { return tb::BdCycle{bd, dev, degree, ratio, split, d_scal, d_part, d_ws}; }
};

namespace tb {

// g_c[I] = g_f[i] for the fine dof i that coincides with the coarse dof I: the one row of P with a single entry of weight 1 in column I
__global__ void __launch_bounds__(256)
k_bdmg_coarse_ground(int64_t nf, const int64_t *__restrict__ pptr, const int32_t *__restrict__ pcol, const uint8_t *__restrict__ pexp, const uint8_t *__restrict__ gf,
                     uint8_t *__restrict__ gc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const int64_t q = pptr[i];
    if (pptr[i + 1] - q == 1 && pexp[q] == 0) gc[pcol[q]] = gf[i] ? 1 : 0;
}

// the fine level's sliced planes → CSR planes with the elimination baked in; the φₑφₑ diagonal of a grounded node stays 0 (the Galerkin product reads
// G_f A₂₂ G_f) until k_bdmg_set_ground_diag
__global__ void __launch_bounds__(256)
k_bdmg_csr_fine(int64_t n, const int64_t *__restrict__ base, int64_t entries, const uint32_t *__restrict__ col, const double *__restrict__ val,
                const uint8_t *__restrict__ ground, const int64_t *__restrict__ rowptr, int64_t nnz, double *__restrict__ csr)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const int64_t b0 = base[row >> 6] + (row & 63), pa = rowptr[row];
    const int len = (int)(rowptr[row + 1] - pa);
    const bool gi = ground[row] != 0;
    for (int k = 0; k < len; ++k) {
        const int64_t o = b0 + 64 * (int64_t)k;
        const bool gj = (col[o] & BD_GROUNDED) != 0;
        const double a11 = val[o], a12 = val[entries + o], a22 = val[2 * entries + o];
        csr[pa + k] = a11;
        csr[nnz + pa + k] = gj ? 0.0 : a12;
        csr[2 * nnz + pa + k] = gi ? 0.0 : a12;
        csr[3 * nnz + pa + k] = (gi || gj) ? 0.0 : a22;
    }
}

// the raw Galerkin planes of a coarse level: φₑ columns and rows of grounded nodes out (selected, not multiplied by 0)
__global__ void __launch_bounds__(256)
k_bdmg_mask_csr(int64_t n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const uint8_t *__restrict__ ground, int64_t nnz, double *__restrict__ csr)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const bool gi = ground[row] != 0;
    for (int64_t k = rowptr[row]; k < rowptr[row + 1]; ++k) {
        const bool gj = ground[colidx[k]] != 0;
        if (gj) csr[nnz + k] = 0.0;
        if (gi) csr[2 * nnz + k] = 0.0;
        if (gi || gj) csr[3 * nnz + k] = 0.0;
    }
}

// the fine level, whose fill is known (ground_diag): every grounded row finds its own diagonal (the scalar hierarchy holds no diagonal positions for its
// finest level; the coarse levels go through launch_fill_diag with the positions of the Galerkin plan)
__global__ void __launch_bounds__(256)
k_bdmg_set_ground_diag(int64_t n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const uint8_t *__restrict__ ground, double fill, double *__restrict__ a22)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !ground[i]) return;
    for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
        if (colidx[k] == i) a22[k] = fill;
}

// B⁻¹ of a node from its diagonal block, zero in the φₑ row and column of a grounded node (z_e stays exactly 0 there); a singular or missing block:
// the identity, as k_bd_fill leaves it
__device__ __forceinline__ void bdmg_store_binv(double *__restrict__ binv, int64_t row, bool grounded, double d11, double d12, double d22)
{
    if (grounded) {
        binv[3 * row] = d11 != 0.0 && d11 == d11 ? 1.0 / d11 : 1.0; binv[3 * row + 1] = 0.0; binv[3 * row + 2] = 0.0;
        return;
    }
    const double det = d11 * d22 - d12 * d12;
    const bool ok = det != 0.0 && det == det;
    binv[3 * row] = ok ? d22 / det : 1.0; binv[3 * row + 1] = ok ? -d12 / det : 0.0; binv[3 * row + 2] = ok ? d11 / det : 1.0;
}

// CSR planes of a coarse level → its sliced planes, columns and block inverses (k_bd_fill with four planes): one lane per row of a slice
__global__ void __launch_bounds__(256)
k_bdmg_fill_sliced(int64_t n, int64_t n_slices, const int64_t *__restrict__ base, int64_t entries, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                   int64_t nnz, const double *__restrict__ csr, const uint8_t *__restrict__ ground, uint32_t *__restrict__ col, double *__restrict__ val, double *__restrict__ binv)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_slices * 64) return;
    const int64_t slice = row >> 6, b0 = base[slice];
    const int W = (int)((base[slice + 1] - b0) >> 6), lane = (int)(row & 63);
    const bool valid = row < n;
    const int64_t rc = valid ? row : n - 1; // (lanes past the last row: padding only)
    const int64_t pa = rowptr[rc];
    const int len = valid ? (int)(rowptr[rc + 1] - pa) : 0;
    double d11 = 0.0, d12 = 0.0, d21 = 0.0, d22 = 0.0;
    for (int k = 0; k < W; ++k) {
        uint32_t c = (uint32_t)rc;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        if (k < len) {
            c = (uint32_t)colidx[pa + k];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = csr[q * nnz + pa + k];
            if ((int64_t)c == row) { d11 = a[0]; d12 = a[1]; d21 = a[2]; d22 = a[3]; }
        }
        const int64_t o = b0 + lane + 64 * (int64_t)k;
        col[o] = c;
#pragma unroll
        for (int q = 0; q < 4; ++q) val[q * entries + o] = a[q];
    }
    if (valid) bdmg_store_binv(binv, row, ground[row] != 0, d11, 0.5 * (d12 + d21), d22);
}

// the fine level's block inverses with the ground masked
__global__ void __launch_bounds__(256) k_bdmg_binv_fine(int64_t n, const double *__restrict__ bd_binv, const uint8_t *__restrict__ ground, double *__restrict__ binv)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool g = ground[i] != 0;
    binv[3 * i] = bd_binv[3 * i]; binv[3 * i + 1] = g ? 0.0 : bd_binv[3 * i + 1]; binv[3 * i + 2] = g ? 0.0 : bd_binv[3 * i + 2];
}

// One step of the Chebyshev iteration on B⁻¹𝒜 apart from the product (k_mg_cheb on node pairs).  MODE 0: first step from x = 0 (d = c₂B⁻¹r, x = d, no
// product at all); MODE 1, 2: the steps of the fused kernel with 𝒜x given in w, in place — the composition the fused step is measured against.
template <int MODE>
__global__ void __launch_bounds__(256)
k_bdmg_cheb(int64_t n, double c1, double c2, const double *__restrict__ binv, const double2 *__restrict__ r, const double2 *__restrict__ w, double2 *__restrict__ d,
            double2 *__restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double2 ri = r[i];
        if (MODE != 0) { const double2 wi = w[i]; ri.x -= wi.x; ri.y -= wi.y; }
        const double2 g = bd_precondition(binv, i, ri);
        double2 di = make_double2(c2 * g.x, c2 * g.y);
        if (MODE == 2) { const double2 dp = d[i]; di.x += c1 * dp.x; di.y += c1 * dp.y; }
        d[i] = di;
        if (MODE == 0) x[i] = di;
        else { const double2 xi = x[i]; x[i] = make_double2(xi.x + di.x, xi.y + di.y); }
    }
}

// r_c = 𝒫ᵀ(r − w): one thread per coarse node gathers its at most 27 fine nodes as 16-byte pairs; the φₑ component skips grounded fine nodes and is 0
// at a grounded coarse node
__global__ void __launch_bounds__(256)
k_bdmg_restrict(int64_t nc, const int64_t *__restrict__ rptr, const int32_t *__restrict__ rcol, const uint8_t *__restrict__ rexp, const double2 *__restrict__ r,
                const double2 *__restrict__ w, const uint8_t *__restrict__ gf, const uint8_t *__restrict__ gc, double2 *__restrict__ rc)
{
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nc) return;
    double sm = 0.0, se = 0.0;
    for (int64_t q = rptr[I]; q < rptr[I + 1]; ++q) {
        const int32_t i = rcol[q];
        const double wt = pow2_neg(rexp[q]);
        const double2 ri = r[i], wi = w[i];
        sm += wt * (ri.x - wi.x);
        se += gf[i] ? 0.0 : wt * (ri.y - wi.y);
    }
    rc[I] = make_double2(sm, gc[I] ? 0.0 : se);
}

// x_f += 𝒫 x_c: one thread per fine node gathers its at most 8 parents; the φₑ component skips grounded parents and stays as it is at a grounded fine node
__global__ void __launch_bounds__(256)
k_bdmg_prolong_add(int64_t nf, const int64_t *__restrict__ pptr, const int32_t *__restrict__ pcol, const uint8_t *__restrict__ pexp, const double2 *__restrict__ xc,
                   const uint8_t *__restrict__ gf, const uint8_t *__restrict__ gc, double2 *__restrict__ xf)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    double sm = 0.0, se = 0.0;
    for (int64_t q = pptr[i]; q < pptr[i + 1]; ++q) {
        const int32_t I = pcol[q];
        const double wt = pow2_neg(pexp[q]);
        const double2 v = xc[I];
        sm += wt * v.x;
        se += gc[I] ? 0.0 : wt * v.y;
    }
    double2 xi = xf[i];
    xi.x += sm;
    if (!gf[i]) xi.y += se;
    xf[i] = xi;
}

// One workgroup: C = 𝒜₀⁻¹ on the 2 n₀ interleaved unknowns of the coarsest level (n₀ ≤ 512), dense: the four planes scattered, then the Gauss–Jordan
// elimination of k_mg_dense_inverse (the operator is symmetric positive definite; a grounded φₑ is a row of the identity scaled by its diagonal)
__global__ void __launch_bounds__(1024)
k_bdmg_dense_inverse(int n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, int64_t nnz, const double *__restrict__ csr, double *__restrict__ C)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6, N = 2 * n;
    for (int i = wv; i < N; i += nw)
        for (int j = lane; j < N; j += 64) C[(size_t)i * N + j] = 0.0;
    __syncthreads();
    for (int i = wv; i < n; i += nw)
        for (int64_t k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) {
            const int j = colidx[k];
            C[(size_t)(2 * i) * N + 2 * j] = csr[k]; C[(size_t)(2 * i) * N + 2 * j + 1] = csr[nnz + k];
            C[(size_t)(2 * i + 1) * N + 2 * j] = csr[2 * nnz + k]; C[(size_t)(2 * i + 1) * N + 2 * j + 1] = csr[3 * nnz + k];
        }
    __syncthreads();
    mg_gauss_jordan(N, C);
}

// ---- λmax(B⁻¹𝒜): Lanczos in the B inner product with B⁻¹ alone — v_k B-orthonormal, u_k = B v_k carried beside it
// The three sums of a step are ORDERED at every size: a workgroup leaves its partial (xor tree in the wave, the four wave sums left to right) in its own
// slot of a buffer, and one workgroup folds the buffer in a fixed order (launch_fold_sum) — no atomic, so two set-ups give the same λmax and the same cycle.
__device__ __forceinline__ void block_partial(double v, double *__restrict__ part)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __shared__ double smp[4];
    if ((threadIdx.x & 63) == 0) smp[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((smp[0] + smp[1]) + smp[2]) + smp[3];
}
// part[workgroup] = Σ a·b over its node pairs (α = vᵀ𝒜v of a step)
__global__ void __launch_bounds__(256) k_bdmg_dot_partial(int64_t n, const double2 *__restrict__ a, const double2 *__restrict__ b, double *__restrict__ part)
{
    double c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { const double2 ai = a[i], bi = b[i]; c += ai.x * bi.x + ai.y * bi.y; }
    block_partial(c, part);
}
// s = start vector (every lane its own fixed value in (−1, 1), the φₑ of a grounded node 0), t = B⁻¹ s; part[workgroup] = its share of tᵀs
__global__ void __launch_bounds__(256)
k_bdmg_lanczos_start(int64_t n, const double *__restrict__ binv, const uint8_t *__restrict__ ground, double2 *__restrict__ s, double2 *__restrict__ t, double *__restrict__ part)
{
    double a = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t h0 = (uint32_t)(2 * i) * 2654435761u, h1 = (uint32_t)(2 * i + 1) * 2654435761u;
        const double2 si = make_double2((double)((h0 >> 8) & 0xffff) / 32768.0 - 1.0 + 0x1p-17, ground[i] ? 0.0 : (double)((h1 >> 8) & 0xffff) / 32768.0 - 1.0 + 0x1p-17);
        const double2 ti = bd_precondition(binv, i, si);
        s[i] = si; t[i] = ti;
        a += si.x * ti.x + si.y * ti.y;
    }
    block_partial(a, part);
}
// s ← s − α u − β u₋₁, t = B⁻¹ s; part[workgroup] = its share of tᵀs (= β₊²)
__global__ void __launch_bounds__(256)
k_bdmg_lanczos_step(int64_t n, double alpha, double beta, const double2 *__restrict__ u, const double2 *__restrict__ up, const double *__restrict__ binv, double2 *__restrict__ s,
                    double2 *__restrict__ t, double *__restrict__ part)
{
    double a = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        double2 si = s[i];
        const double2 ui = u[i];
        si.x -= alpha * ui.x; si.y -= alpha * ui.y;
        if (beta != 0.0) { const double2 pi = up[i]; si.x -= beta * pi.x; si.y -= beta * pi.y; }
        const double2 ti = bd_precondition(binv, i, si);
        s[i] = si; t[i] = ti;
        a += si.x * ti.x + si.y * ti.y;
    }
    block_partial(a, part);
}
// v = c t, u = c s
__global__ void __launch_bounds__(256)
k_bdmg_lanczos_scale(int64_t n, double c, const double2 *__restrict__ t, const double2 *__restrict__ s, double2 *__restrict__ v, double2 *__restrict__ u)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double2 ti = t[i], si = s[i];
        v[i] = make_double2(c * ti.x, c * ti.y); u[i] = make_double2(c * si.x, c * si.y);
    }
}

// ---- the vector kernels of the solve: pcg_loop of tb_krylov.hip on the 2n interleaved values, every scalar in a slot group as in tb_bidomain_solve
// (r·z in a ring of three groups, pᵀ𝒜p from k_bd_apply<true>, r·r).  A slot group gives each of up to 64 workgroups its own slot: up to there (about
// 16 000 nodes) every sum has one order and two solves give the same bits; beyond, several workgroups add into one slot, as in tb_bidomain_solve.
// r = b − Ax (Ax given); rr += r·r
__global__ void __launch_bounds__(256)
k_bdmg_residual(int64_t n2, const double *__restrict__ b, const double *__restrict__ Ax, double *__restrict__ r, double *__restrict__ rr)
{
    double c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        const double ri = b[i] - Ax[i];
        r[i] = ri;
        c += ri * ri;
    }
    block_sum_slots(c, rr);
}
// rz += r·z
__global__ void __launch_bounds__(256) k_bdmg_dot(int64_t n2, const double *__restrict__ r, const double *__restrict__ z, double *__restrict__ rz)
{
    double c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) c += r[i] * z[i];
    block_sum_slots(c, rz);
}
// p = z + β p with β = rz_next / rz (β = 0 when rz = 0: first iteration); the group retired from the ring and the one of the coming product go back to zero
__global__ void __launch_bounds__(256)
k_bdmg_direction(int64_t n2, const double *__restrict__ rz, const double *__restrict__ rz_next, double *__restrict__ retired, double *__restrict__ pAp,
                 const double *__restrict__ z, double *__restrict__ p)
{
    const double rzv = read_slots(rz), rzn = read_slots(rz_next);
    const double beta = rzv > 0.0 ? rzn / rzv : 0.0;
    if (blockIdx.x == 0 && threadIdx.x < 64) { retired[RED_STRIDE * threadIdx.x] = 0.0; pAp[RED_STRIDE * threadIdx.x] = 0.0; } // nobody else touches them during this launch
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) p[i] = z[i] + beta * p[i];
}
// x += α p, r −= α Ap with α = rz_next / pAp; rr += r·r; a non-positive pAp is remembered in *flag
__global__ void __launch_bounds__(256)
k_bdmg_update(int64_t n2, const double *__restrict__ rz_next, const double *__restrict__ pAp, const double *__restrict__ p, const double *__restrict__ Ap, double *__restrict__ x,
              double *__restrict__ r, double *__restrict__ rr, double *__restrict__ flag)
{
    const double pap = read_slots(pAp), rzv = read_slots(rz_next);
    const double alpha = pap > 0.0 ? rzv / pap : 0.0;
    if (!(pap > 0.0) && rzv != 0.0 && blockIdx.x == 0 && threadIdx.x == 0) *flag = pap == 0.0 ? -1e-300 : pap;
    double c = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * Ap[i];
        r[i] = ri;
        c += ri * ri;
    }
    block_sum_slots(c, rr);
}

static void free_bdmg(tb_bidomain_mg *h)
{
    if (!h) return;
    for (BdMgLevel &L : h->lv) {
        void *ptrs[] = {L.d_ground, L.d_csr, L.d_base, L.d_col, L.d_val, L.d_binv, L.d_vec};
        for (void *p : ptrs) if (p) (void)hipFree(p);
    }
    (void)hipFree(h->d_cinv); (void)hipFree(h->d_scal); (void)hipFree(h->d_part); (void)hipFree(h->d_ws);
    delete h;
}

// y = 𝒜_l x (step 0) or one fused smoother step x → y (step 1, 2): the fine level on the block system's three planes and flags, every other level on its
// four planes
template <int STEP>
static void level_product_step(const BdCycle &cy, const BdMgLevel &L, const double *x, double *y, const BdStep &st)
{
    if (L.fine) {
        tb_bidomain *bd = cy.bd;
        hipLaunchKernelGGL((k_bd_apply<false, false, STEP>), dim3((unsigned)((bd->n_slices + 3) / 4)), dim3(256), 0, cy.dev->stream, bd->n, bd->n_slices, bd->d_base, bd->entries,
                           bd->d_col, bd->d_val, bd->d_ground, bd->ground_diag, (const double2 *)x, (double2 *)y, (double *)nullptr, st);
    } else
        hipLaunchKernelGGL((k_bd_apply<false, true, STEP>), dim3((unsigned)((L.n_slices + 3) / 4)), dim3(256), 0, cy.dev->stream, L.n, L.n_slices, L.d_base, L.entries, L.d_col,
                           L.d_val, (const uint8_t *)nullptr, 0.0, (const double2 *)x, (double2 *)y, (double *)nullptr, st);
}
void bd_level_product(const BdCycle &cy, const BdMgLevel &L, int step, const double *x, double *y, const BdStep &st)
{
    if (step == 0) level_product_step<0>(cy, L, x, y, st);
    else if (step == 1) level_product_step<1>(cy, L, x, y, st);
    else level_product_step<2>(cy, L, x, y, st);
}

// `degree` Chebyshev steps on B⁻¹𝒜_l for 𝒜_l x = r (the ChebSchedule of the scalar cycle's cheb_smooth), from zero or from *cur.  Fused: a step reads *cur and writes *other, then the two swap; split: product into w, vector kernel in place.
void bd_smooth(const BdCycle &cy, BdMgLevel &L, const double *r, double *&cur, double *&other, bool from_zero)
{
    tb_device *dev = cy.dev;
    const unsigned g = grid_for(dev, L.n, 256);
    ChebSchedule sched(L.lmax, cy.ratio);
    auto step = [&](bool first, ChebSchedule::Step c) {
        if (cy.split) {
            bd_level_product(cy, L, 0, cur, L.w, BdStep());
            if (first) hipLaunchKernelGGL(k_bdmg_cheb<1>, dim3(g), dim3(256), 0, dev->stream, L.n, c.c1, c.c2, L.d_binv, (const double2 *)r, (const double2 *)L.w, (double2 *)L.d, (double2 *)cur);
            else hipLaunchKernelGGL(k_bdmg_cheb<2>, dim3(g), dim3(256), 0, dev->stream, L.n, c.c1, c.c2, L.d_binv, (const double2 *)r, (const double2 *)L.w, (double2 *)L.d, (double2 *)cur);
            return;
        }
        BdStep st;
        st.c1 = c.c1; st.c2 = c.c2; st.binv = L.d_binv; st.r = (const double2 *)r; st.d = (double2 *)L.d;
        bd_level_product(cy, L, first ? 1 : 2, cur, other, st);
        std::swap(cur, other);
    };
    if (from_zero)
        hipLaunchKernelGGL(k_bdmg_cheb<0>, dim3(g), dim3(256), 0, dev->stream, L.n, sched.first().c1, sched.first().c2, L.d_binv, (const double2 *)r, (const double2 *)nullptr, (double2 *)L.d,
                           (double2 *)cur);
    else
        step(true, sched.first());
    for (int k = 1; k < cy.degree; ++k) step(false, sched.next());
}

// x = ℳ_l⁻¹ r: V(degree, degree) from x = 0; enqueues only.  The fused smoother swaps its two buffers 2·degree − 1 times on a level, so it starts in the
// level's spare buffer and ends in x.
static void cycle(tb_bidomain_mg *h, int l, const double *r, double *x)
{
    tb_device *dev = h->dev;
    BdMgLevel &L = h->lv[l];
    const BdCycle cy = h->cycle_record();
    if (l == 0) {
        launch_dense_apply(dev, (int)(2 * L.n), h->d_cinv, r, x);
        return;
    }
    BdMgLevel &Cl = h->lv[l - 1];
    const MgLevel &T = h->mg->lv[l]; // the transfer plans between l and l − 1
    double *cur = h->split ? x : L.xt, *other = h->split ? L.xt : x;
    bd_smooth(cy, L, r, cur, other, true);
    bd_level_product(cy, L, 0, cur, L.w, BdStep());
    hipLaunchKernelGGL(k_bdmg_restrict, dim3(blocks_of(Cl.n, 256)), dim3(256), 0, dev->stream, Cl.n, T.d_rptr, T.d_rcol, T.d_rexp, (const double2 *)r, (const double2 *)L.w, L.ground,
                       Cl.ground, (double2 *)Cl.r);
    cycle(h, l - 1, Cl.r, Cl.x);
    hipLaunchKernelGGL(k_bdmg_prolong_add, dim3(blocks_of(L.n, 256)), dim3(256), 0, dev->stream, L.n, T.d_pptr, T.d_pcol, T.d_pexp, (const double2 *)Cl.x, L.ground, Cl.ground,
                       (double2 *)cur);
    bd_smooth(cy, L, r, cur, other, false);
}

// λmax(B⁻¹𝒜_l): the largest Ritz value of 24 Lanczos steps in the B inner product (it converges from below), inflated by 5 % — the recipe of
// estimate_lambda_max; its Gershgorin cap has no cheap counterpart for 2 × 2 blocks (a bound needs the norms of B_i^-½ 𝒜_ij B_j^-½) and is left out.
// With t = B⁻¹s: β² = tᵀs, v = t/β, u = s/β = B v;  s ← 𝒜v − αu − βu₋₁, α = vᵀ𝒜v.  Reads scalars back.
int bd_lambda_max(const BdCycle &cy, BdMgLevel &L, const char *who, int l, double *out)
{
    tb_device *dev = cy.dev;
    constexpr int KL = 24;
    const unsigned g = grid_for(dev, L.n, 256);
    double *v = L.d, *s = L.w, *t = L.xt, *u = L.x, *up = L.r, *S = cy.d_scal, *part = cy.d_part;
    double al[KL], be[KL + 1], hh[1];
    auto fold = [&](double *out) { launch_fold_sum(dev, (int)g, part, out); };
    hipLaunchKernelGGL(k_bdmg_lanczos_start, dim3(g), dim3(256), 0, dev->stream, L.n, L.d_binv, L.ground, (double2 *)s, (double2 *)t, part);
    fold(S);
    TB_TRY(read_back(dev, hh, S, 1));
    int kdone = 0;
    be[0] = 0.0;
    double beta = std::sqrt(hh[0]);
    if (hh[0] > 0.0 && std::isfinite(hh[0])) {
        for (int k = 0; k < KL; ++k) {
            hipLaunchKernelGGL(k_bdmg_lanczos_scale, dim3(g), dim3(256), 0, dev->stream, L.n, 1.0 / beta, (const double2 *)t, (const double2 *)s, (double2 *)v, (double2 *)up);
            std::swap(u, up); // u = B v; up: the previous one
            bd_level_product(cy, L, 0, v, s, BdStep()); // s = 𝒜 v
            hipLaunchKernelGGL(k_bdmg_dot_partial, dim3(g), dim3(256), 0, dev->stream, L.n, (const double2 *)v, (const double2 *)s, part); // α = vᵀ𝒜v, ordered (the fused sum of
            fold(S);                                                                                                                    // k_bd_apply<true> is not, above 64 workgroups)
            TB_TRY(read_back(dev, hh, S, 1));
            al[k] = hh[0];
            hipLaunchKernelGGL(k_bdmg_lanczos_step, dim3(g), dim3(256), 0, dev->stream, L.n, al[k], be[k], (const double2 *)u, (const double2 *)up, L.d_binv, (double2 *)s, (double2 *)t,
                               part);
            fold(S + 1);
            TB_TRY(read_back(dev, hh, S + 1, 1));
            kdone = k + 1;
            be[k + 1] = beta = hh[0] > 0.0 ? std::sqrt(hh[0]) : 0.0;
            if (!(be[k + 1] > 1e-12 * std::fabs(al[k]))) break; // invariant subspace: the Ritz values are exact
        }
    }
    TB_HIP(hipGetLastError());
    if (kdone == 0) { set_error("%s: the λmax estimate of level %d found no start vector (non-finite operator?)", who, l); return TB_ERR_BAD_ARG; }
    *out = 1.05 * largest_tridiagonal_eigenvalue(al, be, kdone);
    return TB_OK;
}

// CG on 𝒜x = b with z = ℳ⁻¹r from one cycle: the loop of pcg_loop (tb_krylov.hip) with the slot groups of tb_bidomain_solve — r·z in the ring 4, 5, 6,
// pᵀ𝒜p in 3, r·r in 7, folded into S[3] for the look (S[4]: the sticky flag); a look at every iteration up to the 64th and at every fourth from there
int bd_pcg(const BdCycle &cy, const char *who, void (*cycle)(void *ctx, const double *r, double *z), void *ctx, const double *b, double *x, double rtol, double atol, int maxiter,
           int *iters, double *resnorm)
{
    tb_bidomain *bd = cy.bd;
    tb_device *dev = cy.dev;
    TB_NO_CAPTURE(dev); // reads scalars back (convergence looks)
    const int64_t n2 = 2 * bd->n;
    double *z = cy.d_ws, *p = z + n2, *Ap = p + n2, *r = Ap + n2, *S = cy.d_scal, *const g_pap = red_group(dev, 3), *const g_rr = red_group(dev, 7);
    auto g_rz = [&](int k) { return red_group(dev, 4 + k); };
    const unsigned g = grid_for(dev, n2, 256);
    TB_HIP(hipMemsetAsync(p, 0, sizeof(double) * n2, dev->stream)); // the first direction is p = z + 0·p
    enqueue_apply<false>(bd, x, Ap, nullptr);
    TB_HIP(hipMemsetAsync(S, 0, 8 * sizeof(double), dev->stream));
    TB_HIP(hipMemsetAsync(g_pap, 0, 5 * RED_GROUP * sizeof(double), dev->stream));
    hipLaunchKernelGGL(k_bdmg_residual, dim3(g), dim3(256), 0, dev->stream, n2, b, (const double *)Ap, r, g_rr);
    fold_slots(dev, 7, S + 3, 1);
    double hh[2];
    TB_TRY(read_back(dev, hh, S + 3, 1));
    double rnorm = std::sqrt(hh[0]);
    const double tol = stopping_tolerance(atol, rtol, rnorm);
    bd->pat->last_tol = tol;
    int it = 0, cur = 0, rc = TB_OK;
    while (rnorm > tol && it < maxiter) {
        const int look_every = it >= 64 ? 4 : 1;
        for (int s2 = 0; s2 < look_every && it < maxiter; ++s2, ++it) {
            const int nxt = (cur + 1) % 3, ret = (cur + 2) % 3;
            cycle(ctx, r, z);
            hipLaunchKernelGGL(k_bdmg_dot, dim3(g), dim3(256), 0, dev->stream, n2, (const double *)r, (const double *)z, g_rz(nxt));
            hipLaunchKernelGGL(k_bdmg_direction, dim3(g), dim3(256), 0, dev->stream, n2, (const double *)g_rz(cur), (const double *)g_rz(nxt), g_rz(ret), g_pap, (const double *)z, p);
            enqueue_apply<true>(bd, p, Ap, g_pap);
            TB_HIP(hipMemsetAsync(S + 3, 0, sizeof(double), dev->stream));
            hipLaunchKernelGGL(k_bdmg_update, dim3(g), dim3(256), 0, dev->stream, n2, (const double *)g_rz(nxt), (const double *)g_pap, (const double *)p, (const double *)Ap, x, r, g_rr,
                               S + 4);
            fold_slots(dev, 7, S + 3, 1);
            cur = nxt;
        }
        TB_TRY(read_back(dev, hh, S + 3, 2));
        if (hh[1] != 0.0) {
            set_error("%s: matrix or multigrid preconditioner is not positive definite (pᵀAp = %g)", who, hh[1] == -1e-300 ? 0.0 : hh[1]);
            rc = TB_ERR_BAD_ARG;
            break;
        }
        rnorm = std::sqrt(hh[0]);
    }
    TB_HIP(hipMemsetAsync(g_pap, 0, 5 * RED_GROUP * sizeof(double), dev->stream)); // the slot groups are zero between uses
    TB_HIP(hipGetLastError());
    if (rc) return rc;
    if (iters) *iters = it;
    if (resnorm) *resnorm = rnorm;
    return TB_OK;
}

static void geometric_cycle(void *ctx, const double *r, double *z)
{
    tb_bidomain_mg *h = (tb_bidomain_mg *)ctx;
    cycle(h, (int)h->lv.size() - 1, r, z);
}

// ---- enqueue-only launchers of the kernels the algebraic block cycle (tb_bidomain_amg.hip) shares
void launch_bd_csr_fine(tb_bidomain *bd, double *csr)
{
    tb_pattern *pat = bd->pat;
    hipStream_t st = pat->mesh->dev->stream;
    const unsigned gn = blocks_of(bd->n, 256);
    hipLaunchKernelGGL(k_bdmg_csr_fine, dim3(gn), dim3(256), 0, st, bd->n, bd->d_base, bd->entries, bd->d_col, bd->d_val, bd->d_ground, pat->d_rowptr, pat->nnz, csr);
    hipLaunchKernelGGL(k_bdmg_set_ground_diag, dim3(gn), dim3(256), 0, st, bd->n, pat->d_rowptr, pat->d_colidx, bd->d_ground, bd->ground_diag, csr + 3 * pat->nnz);
}
void launch_bd_binv_fine(tb_bidomain *bd, double *binv)
{
    hipLaunchKernelGGL(k_bdmg_binv_fine, dim3(blocks_of(bd->n, 256)), dim3(256), 0, bd->pat->mesh->dev->stream, bd->n, bd->d_binv, bd->d_ground, binv);
}
void launch_bd_fill_sliced(tb_device *dev, const BdMgLevel &L, const int64_t *rowptr, const int32_t *colidx)
{
    hipLaunchKernelGGL(k_bdmg_fill_sliced, dim3(blocks_of(L.n_slices * 64, 256)), dim3(256), 0, dev->stream, L.n, L.n_slices, L.d_base, L.entries, rowptr, colidx, L.nnz, L.d_csr,
                       L.ground, L.d_col, L.d_val, L.d_binv);
}
void launch_bd_dense_inverse(tb_device *dev, int n, const int64_t *rowptr, const int32_t *colidx, int64_t nnz, const double *csr, double *C)
{
    hipLaunchKernelGGL(k_bdmg_dense_inverse, dim3(1), dim3(1024), 0, dev->stream, n, rowptr, colidx, nnz, csr, C);
}

} // namespace tb

using namespace tb;

#define BDMG_READY(h_, who_)                                                                                                                                     \
    do {                                                                                                                                                         \
        TB_REQUIRE((h_)->ready, who_ ": no numeric set-up yet (tb_bidomain_mg_setup)");                                                                          \
        TB_REQUIRE((h_)->set_for == (h_)->bd->generation, who_ ": tb_bidomain_set_matrices ran after the latest set-up (tb_bidomain_mg_setup follows every new matrix)"); \
        TB_REQUIRE((h_)->mg->planned, who_ ": the tb_mg of this hierarchy was changed after tb_bidomain_mg_create (its plans are gone)");                        \
    } while (0)

extern "C" {

int tb_bidomain_mg_create(tb_bidomain *bd, tb_mg *mg, tb_bidomain_mg **out)
{
    TB_REQUIRE(bd && mg && out, "tb_bidomain_mg_create: NULL argument");
    *out = nullptr;
    const int nl = (int)mg->lv.size();
    TB_REQUIRE(mg->lv.back().pat == bd->pat, "tb_bidomain_mg_create: the finest pattern of the hierarchy is not the pattern of the block system");
    tb_device *dev = bd->pat->mesh->dev;
    TB_REQUIRE(mg->dev == dev, "tb_bidomain_mg_create: the hierarchy lives on another device");
    TB_NO_CAPTURE(dev); // plans, allocations
    for (int l = 0; l < nl; ++l) {
        const MgLevel &M = mg->lv[l];
        TB_REQUIRE(M.pat, "tb_bidomain_mg_create: level %d has no pattern (tb_mg_set_level)", l);
        TB_REQUIRE(l == 0 || (M.has_transfer && !M.p_transfer), "tb_bidomain_mg_create: level %d has no h-transfer to level %d (tb_mg_set_transfer)", l, l - 1);
        if (M.pat->mesh->ncomp != 1 || M.pat->mesh->field_kind != TB_HEX8) {
            set_error("tb_bidomain_mg_create: level %d carries field kind %d with %d component(s) - the levels are scalar first-order fields on hexahedra", l,
                      M.pat->mesh->field_kind, M.pat->mesh->ncomp);
            return TB_ERR_UNSUPPORTED;
        }
    }
    TB_REQUIRE(mg->lv.back().h_presc.empty(), "tb_bidomain_mg_create: the hierarchy has prescribed dofs (tb_mg_set_prescribed): the block cycle runs on its unflagged plans, the ground "
                                              "comes from tb_bidomain_set_matrices");
    if (mg->lv[0].pat->n_rows > BD_COARSEST_NODES) {
        set_error("tb_bidomain_mg_create: the coarsest level has %lld nodes (%lld unknowns); its dense inverse takes at most %d nodes - add a level",
                  (long long)mg->lv[0].pat->n_rows, 2 * (long long)mg->lv[0].pat->n_rows, BD_COARSEST_NODES);
        return TB_ERR_UNSUPPORTED;
    }
    TB_HIP(hipSetDevice(dev->id));
    if (!mg->planned) TB_TRY(build_plans(mg));
    std::unique_ptr<tb_bidomain_mg, void (*)(tb_bidomain_mg *)> h(new tb_bidomain_mg, free_bdmg);
    h->bd = bd; h->mg = mg; h->dev = dev;
    h->split = tune_env("TB_BDMG_SMOOTHER") && !strcmp(tune_env("TB_BDMG_SMOOTHER"), "split");
    h->lv.resize((size_t)nl);
    for (int l = 0; l < nl; ++l) {
        BdMgLevel &L = h->lv[l];
        tb_pattern *pat = mg->lv[l].pat;
        L.pat = pat; L.n = pat->n_rows; L.nnz = pat->nnz;
        TB_REQUIRE(L.n > 0 && (int64_t)pat->h_rowptr.size() == L.n + 1, "tb_bidomain_mg_create: the pattern of level %d has no rows", l);
        TB_HIP(hipMalloc((void **)&L.d_csr, sizeof(double) * 4 * (size_t)std::max<int64_t>(L.nnz, 1)));
        TB_HIP(hipMalloc((void **)&L.d_vec, sizeof(double) * 10 * (size_t)L.n));
        L.d = L.d_vec; L.w = L.d + 2 * L.n; L.xt = L.w + 2 * L.n; L.x = L.xt + 2 * L.n; L.r = L.x + 2 * L.n;
        L.fine = l == nl - 1;
        if (l == nl - 1) L.ground = bd->d_ground;
        else {
            TB_HIP(hipMalloc((void **)&L.d_ground, (size_t)L.n));
            L.ground = L.d_ground;
        }
        if (l == 0) continue; // inverted, not smoothed
        TB_HIP(hipMalloc((void **)&L.d_binv, sizeof(double) * 3 * (size_t)L.n));
        if (l == nl - 1) continue; // the block system's own sliced planes
        L.n_slices = (L.n + 63) / 64;
        std::vector<int64_t> base;
        bd_slice_table(L.n, pat->h_rowptr.data(), base);
        L.entries = base.back();
        TB_TRY(upload(dev, base, &L.d_base));
        TB_HIP(hipMalloc((void **)&L.d_col, std::max<size_t>(1, (size_t)L.entries) * sizeof(uint32_t)));
        TB_HIP(hipMalloc((void **)&L.d_val, std::max<size_t>(1, 4 * (size_t)L.entries) * sizeof(double)));
    }
    const size_t N0 = 2 * (size_t)h->lv[0].n;
    TB_HIP(hipMalloc((void **)&h->d_cinv, sizeof(double) * N0 * N0));
    TB_HIP(hipMalloc((void **)&h->d_scal, 8 * sizeof(double)));
    TB_HIP(hipMalloc((void **)&h->d_part, sizeof(double) * 8 * (size_t)std::max(dev->n_cu, 1))); // grid_for never launches more workgroups
    TB_HIP(hipMalloc((void **)&h->d_ws, sizeof(double) * 8 * (size_t)bd->n));
    *out = h.release();
    return TB_OK;
}

int tb_bidomain_mg_destroy(tb_bidomain_mg *h)
{
    if (h) (void)hipSetDevice(h->dev->id);
    free_bdmg(h);
    return TB_OK;
}

int tb_bidomain_mg_setup(tb_bidomain_mg *h, int degree, double interval_ratio)
{
    TB_REQUIRE(h, "tb_bidomain_mg_setup: NULL argument");
    TB_TRY(check_smoother_args("tb_bidomain_mg_setup", degree, interval_ratio));
    tb_bidomain *bd = h->bd;
    tb_device *dev = h->dev;
    TB_NO_CAPTURE(dev); // reads λmax back
    TB_REQUIRE(bd->have_matrices, "tb_bidomain_mg_setup: no matrices yet (tb_bidomain_set_matrices comes first)");
    TB_REQUIRE(h->mg->planned, "tb_bidomain_mg_setup: the tb_mg of this hierarchy was changed after tb_bidomain_mg_create (its plans are gone)");
    TB_HIP(hipSetDevice(dev->id));
    h->ready = false;
    h->degree = degree;
    h->ratio = interval_ratio;
    const int nl = (int)h->lv.size();
    for (int l = nl - 1; l >= 0; --l) {
        BdMgLevel &L = h->lv[l];
        const unsigned gn = blocks_of(L.n, 256);
        if (l == nl - 1)
            hipLaunchKernelGGL(k_bdmg_csr_fine, dim3(gn), dim3(256), 0, dev->stream, L.n, bd->d_base, bd->entries, bd->d_col, bd->d_val, bd->d_ground, L.pat->d_rowptr, L.nnz, L.d_csr);
        if (l > 0) { // 𝒜_{l−1} = 𝒫ᵀ𝒜_l𝒫: the masked planes through the scalar plan, then the coarse masks
            BdMgLevel &Cl = h->lv[l - 1];
            const MgLevel &T = h->mg->lv[l];
            TB_HIP(hipMemsetAsync(Cl.d_ground, 0, (size_t)Cl.n, dev->stream));
            hipLaunchKernelGGL(k_bdmg_coarse_ground, dim3(gn), dim3(256), 0, dev->stream, L.n, T.d_pptr, T.d_pcol, T.d_pexp, L.ground, Cl.d_ground);
            for (int q = 0; q < 4; ++q) launch_galerkin_plane(h->mg, l, L.d_csr + q * L.nnz, Cl.d_csr + q * Cl.nnz);
            hipLaunchKernelGGL(k_bdmg_mask_csr, dim3(blocks_of(Cl.n, 256)), dim3(256), 0, dev->stream, Cl.n, Cl.pat->d_rowptr, Cl.pat->d_colidx, Cl.ground, Cl.nnz, Cl.d_csr);
        }
        if (l == nl - 1)
            hipLaunchKernelGGL(k_bdmg_set_ground_diag, dim3(gn), dim3(256), 0, dev->stream, L.n, L.pat->d_rowptr, L.pat->d_colidx, L.ground, bd->ground_diag, L.d_csr + 3 * L.nnz);
        else
            launch_fill_diag(dev, L.n, h->mg->lv[l + 1].d_cdiag, L.ground, L.d_csr + 3 * L.nnz);
        if (l == 0) break;
        if (l == nl - 1) hipLaunchKernelGGL(k_bdmg_binv_fine, dim3(gn), dim3(256), 0, dev->stream, L.n, bd->d_binv, L.ground, L.d_binv);
        else
            hipLaunchKernelGGL(k_bdmg_fill_sliced, dim3(blocks_of(L.n_slices * 64, 256)), dim3(256), 0, dev->stream, L.n, L.n_slices, L.d_base, L.entries, L.pat->d_rowptr,
                               L.pat->d_colidx, L.nnz, L.d_csr, L.ground, L.d_col, L.d_val, L.d_binv);
        TB_HIP(hipGetLastError());
        TB_TRY(bd_lambda_max(h->cycle_record(), L, "tb_bidomain_mg_setup", l, &L.lmax));
    }
    BdMgLevel &C0 = h->lv[0];
    hipLaunchKernelGGL(k_bdmg_dense_inverse, dim3(1), dim3(1024), 0, dev->stream, (int)C0.n, C0.pat->d_rowptr, C0.pat->d_colidx, C0.nnz, C0.d_csr, h->d_cinv);
    TB_HIP(hipGetLastError());
    h->set_for = bd->generation;
    h->ready = true;
    return TB_OK;
}

int tb_bidomain_mg_apply(tb_bidomain_mg *h, const double *d_r, double *d_z)
{
    TB_REQUIRE(h && d_r && d_z, "tb_bidomain_mg_apply: NULL argument");
    BDMG_READY(h, "tb_bidomain_mg_apply");
    TB_REQUIRE(d_r != d_z, "tb_bidomain_mg_apply: r and z alias");
    BD_ALIGNED(d_r, "tb_bidomain_mg_apply"); BD_ALIGNED(d_z, "tb_bidomain_mg_apply");
    TB_HIP(hipSetDevice(h->dev->id));
    cycle(h, (int)h->lv.size() - 1, d_r, d_z);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_bidomain_mg_cycle_below(tb_bidomain_mg *h, int level)
{
    TB_REQUIRE(h, "tb_bidomain_mg_cycle_below: NULL argument");
    TB_REQUIRE(level >= 0 && level < (int)h->lv.size() - 1, "tb_bidomain_mg_cycle_below: level %d of 0..%d (the finest level takes tb_bidomain_mg_apply)", level, (int)h->lv.size() - 2);
    BDMG_READY(h, "tb_bidomain_mg_cycle_below");
    TB_HIP(hipSetDevice(h->dev->id));
    cycle(h, level, h->lv[level].r, h->lv[level].x);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_bidomain_mg_n_levels(tb_bidomain_mg *h, int *n_levels)
{
    TB_REQUIRE(h && n_levels, "tb_bidomain_mg_n_levels: NULL argument");
    *n_levels = (int)h->lv.size();
    return TB_OK;
}

int tb_bidomain_mg_level_planes(tb_bidomain_mg *h, int level, const double **d_planes, int64_t *nnz)
{
    TB_REQUIRE(h && d_planes && nnz, "tb_bidomain_mg_level_planes: NULL argument");
    TB_REQUIRE(level >= 0 && level < (int)h->lv.size(), "tb_bidomain_mg_level_planes: level %d of %d", level, (int)h->lv.size());
    BDMG_READY(h, "tb_bidomain_mg_level_planes");
    *d_planes = h->lv[level].d_csr;
    *nnz = h->lv[level].nnz;
    return TB_OK;
}

int tb_bidomain_mg_level_lambda_max(tb_bidomain_mg *h, int level, double *lmax)
{
    TB_REQUIRE(h && lmax, "tb_bidomain_mg_level_lambda_max: NULL argument");
    TB_REQUIRE(level >= 1 && level < (int)h->lv.size(), "tb_bidomain_mg_level_lambda_max: level %d of 1..%d (the coarsest level is inverted, not smoothed)", level, (int)h->lv.size() - 1);
    BDMG_READY(h, "tb_bidomain_mg_level_lambda_max");
    *lmax = h->lv[level].lmax;
    return TB_OK;
}

int tb_bidomain_mg_solve(tb_bidomain_mg *h, const double *d_b, double *d_x, double rtol, double atol, int maxiter, int *iters, double *resnorm)
{
    TB_REQUIRE(h && d_b && d_x, "tb_bidomain_mg_solve: NULL argument");
    BDMG_READY(h, "tb_bidomain_mg_solve");
    TB_REQUIRE(rtol >= 0 && atol >= 0 && maxiter >= 0, "tb_bidomain_mg_solve: negative tolerance or iteration limit");
    TB_REQUIRE(d_b != d_x, "tb_bidomain_mg_solve: b and x alias");
    BD_ALIGNED(d_b, "tb_bidomain_mg_solve"); BD_ALIGNED(d_x, "tb_bidomain_mg_solve");
    TB_HIP(hipSetDevice(h->dev->id));
    return bd_pcg(h->cycle_record(), "tb_bidomain_mg_solve", geometric_cycle, h, d_b, d_x, rtol, atol, maxiter, iters, resnorm);
}

} // extern "C"

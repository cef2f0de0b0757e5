// tb_newmark.hip — what a Newmark-β step of M ü + f_int(u) = f_ext needs beyond the quasi-static stack (gfx950):
//   mass matrix of a 3-component field    Mₑ[(i,c),(j,d)] = ρ NᵢNⱼ δ_cd dΩ             src/modeling/core/mass.jl:28-43 with vector shape functions
//   predictors                            ũ = uₙ + Δt vₙ + (½−β)Δt² aₙ, ṽ = vₙ + (1−γ)Δt aₙ   src/solver/time/newmark.jl:580-581
//   inertia stage                         r += c·M(u−ũ), Jnz += c·Mnz, c = 1/(βΔt²), ONE pass  newmark.jl:89-110
//   corrector                             a = (u−ũ)/(βΔt²), v = ṽ + γΔt a                     newmark.jl:91-95,171-180
//   cubic Hermite interpolant             D-th derivative through (u₀, v₀), (u₁, v₁)          newmark.jl:305-382
// Every entry only enqueues on the device's stream (no allocation, no wait, no read-back once the plans it uses exist): all of them may be captured.
//
// Design notes (DESIGN.md "Newmark elastodynamics"):
//  * The mass is assembled once per run: one 64-lane workgroup per cell, shape values and ρ·detJ·w of the points staged in LDS, each lane a share of
//    the node pairs.  Reference-element values are evaluated at run time — one kernel serves the four field kinds.  Only the three same-component
//    entries of a node pair are touched (through the pattern's cell → nz map), so every other entry of the mechanics pattern stays the 0.0 of the
//    zero fill.  The dof table is the caller's: nothing here assumes dof = 3·node + c.
//  * The stage is a pure stream over Mnz and Jnz with a lane group per row (no floating-point atomics: two calls give the same bits).  On a node-major
//    numbering (a CSR of 3 × 3 blocks whose mass blocks are m·I₃) one double of nine is read from M and three of nine are rewritten in J.  Other
//    patterns run the composition (difference, SpMV, axpy): the fused general kernel lost to it at one measured size and is kept for measurement only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "tb_internal.h"
#include "tb_reduce.hpp"

namespace tb {

// ------------------------------------------------------------------------------------------------
// reference elements at run time (conventions of include/tbhip.h and tb_elem.hpp)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double gauss_x(int n, int i)
{
    if (n == 1) return 0.0;
    if (n == 2) return i == 0 ? -0.5773502691896258 : 0.5773502691896258;
    return i == 0 ? -0.7745966692414834 : i == 1 ? 0.0 : 0.7745966692414834;
}
__device__ __forceinline__ double gauss_w(int n, int i)
{
    if (n == 1) return 2.0;
    if (n == 2) return 1.0;
    return i == 1 ? 0.8888888888888888 : 0.5555555555555556;
}
__device__ __forceinline__ int hex8_sign(int a, int d)
{
    // vertices (-,-,-),(+,-,-),(+,+,-),(-,+,-),(-,-,+),(+,-,+),(+,+,+),(-,+,+): one bit per vertex and direction
    const unsigned bits = d == 0 ? 0x66u : d == 1 ? 0xCCu : 0xF0u;
    return (bits >> a) & 1u ? 1 : -1;
}
__device__ __forceinline__ int hex27_tix(int a, int d)
{
    // Lagrange{RefHexahedron, 2}: vertices, edges, faces, volume — tensor index per direction, two bits each (x | y << 2 | z << 4)
    constexpr unsigned char T[27] = {0x00, 0x02, 0x0A, 0x08, 0x20, 0x22, 0x2A, 0x28, 0x01, 0x06, 0x09, 0x04, 0x21, 0x26,
                                     0x29, 0x24, 0x10, 0x12, 0x1A, 0x18, 0x05, 0x11, 0x16, 0x19, 0x14, 0x25, 0x15};
    return (T[a] >> (2 * d)) & 3;
}
__device__ __forceinline__ double quad1d(int i, double x) { return i == 0 ? 0.5 * x * (x - 1.0) : i == 1 ? (1.0 - x * x) : 0.5 * x * (x + 1.0); }

// Quadrature point q of the tetrahedron rules as barycentric coordinates λ[4] and weight (fractions of the reference volume 1/6 folded in):
//   degree 2: the 4-point rule of the mechanics path;  degree 4: Keast's 11-point rule (Keast 1986) in closed form — centroid, weight −74/5625;
//   four points (a,a,a,1−3a), a = 1/14, weight 343/45000; six points (b,b,c,c), b, c = (1 ± √(5/14))/4, weight 56/2250.
__device__ __forceinline__ double tet_point(int degree, int q, double (&lam)[4])
{
    if (degree == 2) {
        const double a = 0.1381966011250105;
        for (int v = 0; v < 4; ++v) lam[v] = v == q ? 1.0 - 3.0 * a : a;
        return 1.0 / 24.0;
    }
    if (q == 0) {
        lam[0] = lam[1] = lam[2] = lam[3] = 0.25;
        return -74.0 / 5625.0;
    }
    if (q < 5) {
        const double a = 1.0 / 14.0;
        for (int v = 0; v < 4; ++v) lam[v] = v == q - 1 ? 1.0 - 3.0 * a : a;
        return 343.0 / 45000.0;
    }
    const double s = 0.5976143046671968 /* √(5/14) */, b = 0.25 * (1.0 + s), c = 0.25 * (1.0 - s);
    // pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) carry b
    const int p = q - 5, i = p < 3 ? 0 : p < 5 ? 1 : 2, j = p < 3 ? p + 1 : p < 5 ? p - 1 : 3;
    for (int v = 0; v < 4; ++v) lam[v] = (v == i || v == j) ? b : c;
    return 56.0 / 2250.0;
}

struct VMassArgs {
    const double *xyz;
    const int32_t *conn;
    const double *field; // first-order nodal density per cell (8 / 4 values), or NULL
    int64_t n_cells;
    int kind, nb, ng;    // field kind, basis functions per component, Gauss points per direction (hexahedra) / degree of the rule (tetrahedra)
    int nq;
    double rho;
};

// One workgroup of 64 lanes per cell.  Phase 1: lane q < nq evaluates point q — N_a(ξ_q) for every a and ρ(ξ_q)·detJ·w_q — into LDS.
// Phase 2: lane p takes node pairs (i, j) = (p / nb, p % nb), sums m = Σ_q (ρ detJ w)_q (N_i N_j)_q in point order and adds it at the three
// same-component positions (3i + c, 3j + c) of the cell → nz map.
template <class MapT>
__global__ void __launch_bounds__(64)
k_vector_mass(VMassArgs a, const MapT *__restrict__ emap, const int32_t *__restrict__ list, int64_t n, double *__restrict__ nz, int atomic, Status *st)
{
    __shared__ double sN[27 * 27];
    __shared__ double sW[27];
    const int64_t item = blockIdx.x;
    if (item >= n) return;
    const int64_t cell = list ? list[item] : item;
    const int nb = a.nb, q = threadIdx.x;
    const bool hex = a.kind == TB_HEX8 || a.kind == TB_HEX27;
    if (q < a.nq) {
        double rho = a.rho, dOmega;
        double *Nq = sN + q * nb;
        if (hex) {
            const int ng = a.ng;
            const int qi[3] = {q % ng, (q / ng) % ng, q / (ng * ng)};
            const double xi[3] = {gauss_x(ng, qi[0]), gauss_x(ng, qi[1]), gauss_x(ng, qi[2])};
            const double w = gauss_w(ng, qi[0]) * gauss_w(ng, qi[1]) * gauss_w(ng, qi[2]);
            // trilinear geometry: J = Σ xₐ ⊗ ∂Mₐ/∂ξ
            double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
            double rq = 0.0;
            for (int v = 0; v < 8; ++v) {
                const double f0 = 1.0 + hex8_sign(v, 0) * xi[0], f1 = 1.0 + hex8_sign(v, 1) * xi[1], f2 = 1.0 + hex8_sign(v, 2) * xi[2];
                const double dM[3] = {0.125 * hex8_sign(v, 0) * f1 * f2, 0.125 * f0 * hex8_sign(v, 1) * f2, 0.125 * f0 * f1 * hex8_sign(v, 2)};
                const double *x = a.xyz + 3 * (int64_t)a.conn[cell * 8 + v];
                for (int r = 0; r < 3; ++r)
                    for (int d = 0; d < 3; ++d) J[r][d] += x[r] * dM[d];
                if (a.field) rq += 0.125 * f0 * f1 * f2 * a.field[cell * 8 + v];
            }
            if (a.field) rho = rq;
            const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                               J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
            dOmega = det * w;
            if (a.kind == TB_HEX8)
                for (int b = 0; b < 8; ++b) Nq[b] = 0.125 * (1.0 + hex8_sign(b, 0) * xi[0]) * (1.0 + hex8_sign(b, 1) * xi[1]) * (1.0 + hex8_sign(b, 2) * xi[2]);
            else
                for (int b = 0; b < 27; ++b) Nq[b] = quad1d(hex27_tix(b, 0), xi[0]) * quad1d(hex27_tix(b, 1), xi[1]) * quad1d(hex27_tix(b, 2), xi[2]);
        } else {
            double lam[4];
            const double w = tet_point(a.ng, q, lam);
            const int32_t *c = a.conn + cell * 4;
            const double *x0 = a.xyz + 3 * (int64_t)c[0], *x1 = a.xyz + 3 * (int64_t)c[1], *x2 = a.xyz + 3 * (int64_t)c[2], *x3 = a.xyz + 3 * (int64_t)c[3];
            const double e1[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]}, e2[3] = {x2[0] - x0[0], x2[1] - x0[1], x2[2] - x0[2]},
                         e3[3] = {x3[0] - x0[0], x3[1] - x0[1], x3[2] - x0[2]};
            const double det = e1[0] * (e2[1] * e3[2] - e2[2] * e3[1]) - e1[1] * (e2[0] * e3[2] - e2[2] * e3[0]) + e1[2] * (e2[0] * e3[1] - e2[1] * e3[0]);
            dOmega = det * w;
            if (a.field) {
                rho = 0.0;
                for (int v = 0; v < 4; ++v) rho += lam[v] * a.field[cell * 4 + v];
            }
            if (a.kind == TB_TET4) {
                for (int v = 0; v < 4; ++v) Nq[v] = lam[v];
            } else { // vertices, then the edge nodes of (0,1), (1,2), (2,0), (0,3), (1,3), (2,3)
                for (int v = 0; v < 4; ++v) Nq[v] = lam[v] * (2.0 * lam[v] - 1.0);
                Nq[4] = 4.0 * lam[0] * lam[1]; Nq[5] = 4.0 * lam[1] * lam[2]; Nq[6] = 4.0 * lam[2] * lam[0];
                Nq[7] = 4.0 * lam[0] * lam[3]; Nq[8] = 4.0 * lam[1] * lam[3]; Nq[9] = 4.0 * lam[2] * lam[3];
            }
        }
        // the sign of detJ·w is the sign of detJ except at the centroid of the degree-4 rule (negative weight)
        const bool neg_w = !hex && a.ng == 4 && q == 0;
        // (negated comparisons: a NaN or ±∞ coordinate gives a NaN detJ, which flags the cell like every other assembly kernel's !(det > 0))
        if (neg_w ? !(dOmega < 0.0) : !(dOmega > 0.0)) { st->neg_detj = 1; st->cell = cell; }
        sW[q] = rho * dOmega;
    }
    __syncthreads();
    const int ndpc = 3 * nb;
    for (int p = threadIdx.x; p < nb * nb; p += 64) {
        const int i = p / nb, j = p - i * nb;
        double m = 0.0;
        for (int k = 0; k < a.nq; ++k) m += sW[k] * (sN[k * nb + i] * sN[k * nb + j]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t k = (int64_t)emap[(int64_t)((3 * i + c) * ndpc + 3 * j + c) * a.n_cells + cell];
            if (atomic) unsafeAtomicAdd(nz + k, m); else nz[k] += m;
        }
    }
}

// tb_assemble_matrix of a TB_FORM_MASS form on a 3-component field (called from tb_api.cpp)
int launch_assemble_vector_mass(tb_form *f, tb_pattern *p, int strategy, double *d_nz)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    if (f->kind != TB_FORM_MASS) { set_error("tb_assemble_matrix: 3-component fields assemble the mass form only (tb_linearize holds their stiffness)"); return TB_ERR_UNSUPPORTED; }
    if (f->has_cellset) { set_error("tb_assemble_matrix: the vector mass takes no cell set (a density per subdomain is a TB_COEF_FIELD_SCALAR coefficient)"); return TB_ERR_UNSUPPORTED; }
    VMassArgs a{};
    a.xyz = m->d_xyz; a.conn = m->d_conn; a.field = f->field ? f->d_field : nullptr; a.n_cells = m->n_cells;
    a.kind = m->field_kind; a.nb = m->nb; a.rho = f->coef.p[0];
    if (m->field_kind == TB_HEX8 || m->field_kind == TB_HEX27) {
        if (m->geom_kind != TB_HEX8) { set_error("vector mass: field kind %d needs hexahedral geometry (got geometry kind %d)", m->field_kind, m->geom_kind); return TB_ERR_UNSUPPORTED; }
        if (f->qorder < 1 || f->qorder > 3) { set_error("vector mass: %d Gauss points per direction not implemented (1 to 3)", f->qorder); return TB_ERR_UNSUPPORTED; }
        a.ng = f->qorder; a.nq = f->qorder * f->qorder * f->qorder;
    } else if (m->field_kind == TB_TET4 || m->field_kind == TB_TET10) {
        a.ng = m->field_kind == TB_TET4 ? 2 : 4; a.nq = m->field_kind == TB_TET4 ? 4 : 11; // the rule exact for the integrand of degree 2p, whatever qorder says
    } else {
        set_error("vector mass: field kind %d not implemented", m->field_kind);
        return TB_ERR_UNSUPPORTED;
    }
    TB_TRY(ensure_emap(p)); // resets and reads the status itself
    TB_TRY(reset_status(dev));
    TB_HIP(hipMemsetAsync(d_nz, 0, (size_t)p->nnz * sizeof(double), dev->stream));
    // PATCH: there is no LDS-accumulating patch kernel for this form; the colours are the reproducible choice and the mass is assembled once
    const bool atomic = strategy == TB_STRATEGY_ATOMIC;
    auto go = [&](const int32_t *list, int64_t n) -> int {
        if (n == 0) return TB_OK;
        if (p->map64)
            hipLaunchKernelGGL((k_vector_mass<int64_t>), dim3((unsigned)n), dim3(64), 0, dev->stream, a, (const int64_t *)p->d_emap, list, n, d_nz, atomic ? 1 : 0, dev->d_status);
        else
            hipLaunchKernelGGL((k_vector_mass<int32_t>), dim3((unsigned)n), dim3(64), 0, dev->stream, a, (const int32_t *)p->d_emap, list, n, d_nz, atomic ? 1 : 0, dev->d_status);
        TB_HIP(hipGetLastError());
        return TB_OK;
    };
    if (m->n_cells > (int64_t)0x7fffffff) { set_error("vector mass: %lld cells exceed one launch", (long long)m->n_cells); return TB_ERR_UNSUPPORTED; }
    if (atomic) {
        TB_TRY(go(nullptr, m->n_cells));
        set_last_kernel("k_vector_mass<atomic>");
    } else {
        if (!m->colors) TB_TRY(build_color_plan(m));
        for (int c = 0; c < m->colors->ncolors; ++c) TB_TRY(go(m->colors->d_cells + m->colors->offsets[c], m->colors->offsets[c + 1] - m->colors->offsets[c]));
        set_last_kernel("k_vector_mass<colours>");
    }
    return check_status(dev);
}

// ------------------------------------------------------------------------------------------------
// predictor / corrector / Hermite interpolant: one pass over the vectors each
// ------------------------------------------------------------------------------------------------
// A product that must not be contracted into a fused multiply-add with the sum that follows (the unit is built with -ffp-contract=fast): the value
// passes through an empty statement the optimiser cannot see through.
__device__ __forceinline__ double rounded(double x)
{
    asm volatile("" : "+v"(x));
    return x;
}

__global__ void __launch_bounds__(256)
k_newmark_predict(int64_t n, double dt, double cu, double cv, const double *__restrict__ u, const double *__restrict__ v, const double *__restrict__ acc,
                  double *__restrict__ ut, double *__restrict__ vt)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        // every product and sum rounded on its own (`rounded`: no fused multiply-adds): the predictors are (u + Δt·v) + cu·a and v + cv·a to
        // the bit on any host that evaluates them in this order; the kernel is a stream, the extra roundings cost nothing
        const double ui = u[i], vi = v[i], ai = acc[i];
        ut[i] = (ui + rounded(dt * vi)) + rounded(cu * ai);
        vt[i] = vi + rounded(cv * ai);
    }
}

__global__ void __launch_bounds__(256)
k_newmark_correct(int64_t n, double bdt2, double gdt, const double *__restrict__ u, const double *__restrict__ ut, const double *__restrict__ vt,
                  double *__restrict__ acc, double *__restrict__ v)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double ai = (u[i] - ut[i]) / bdt2;
        acc[i] = ai;
        v[i] = vt[i] + rounded(gdt * ai); // separately rounded, like the predictors
    }
}

// d = u − ũ of the composition path (plain 8-byte accesses: the vectors are the caller's, at any 8-byte alignment)
__global__ void __launch_bounds__(256) k_newmark_diff(int64_t n, const double *__restrict__ u, const double *__restrict__ ut, double *__restrict__ d)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) d[i] = u[i] - ut[i];
}

__global__ void __launch_bounds__(256)
k_hermite(int64_t n, double c0, double c1, double c2, double c3, const double *__restrict__ u0, const double *__restrict__ v0, const double *__restrict__ u1,
          const double *__restrict__ v1, double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = c0 * u0[i] + c1 * v0[i] + c2 * u1[i] + c3 * v1[i];
}

// ------------------------------------------------------------------------------------------------
// inertia stage: r += c·M(u − ũ), Jnz += c·Mnz in one pass over the rows of M
// ------------------------------------------------------------------------------------------------
// general CSR (TB_NEWMARK_STAGE=rows, and patterns first seen inside a capture): G lanes per row, consecutive lanes on consecutive non-zeros (coalesced M, J and column loads); the row sum is folded by wave
// shuffles inside the lane group — the order of the additions is a function of the row alone
template <int G>
__global__ void __launch_bounds__(256)
k_newmark_stage_csr(int64_t n_rows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ M, double c,
                    const double *__restrict__ u, const double *__restrict__ ut, double *__restrict__ J, double *__restrict__ r)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = threadIdx.x % G;
    const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) / G;
    for (int64_t row = gid / G; row < n_rows; row += ngroups) {
        const int64_t k0 = rowptr[row], k1 = rowptr[row + 1];
        double acc = 0.0;
        for (int64_t k = k0 + sub; k < k1; k += G) {
            const double m = M[k];
            if (J) J[k] += c * m;
            if (r) {
                const int32_t col = colidx[k];
                acc += m * (u[col] - ut[col]);
            }
        }
        if (r) { // uniform over the grid: every lane takes part in the shuffles
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o, G);
            if (sub == 0) r[row] += c * acc;
        }
    }
}

// CSR of 3 × 3 blocks whose mass blocks are m·I₃ (vector mass on a node-major numbering): G lanes per node row, a lane per block.  M is read at the
// first row of the block only (one double of nine), J is rewritten on the block diagonals only (c·0 added elsewhere would leave the entry as it is)
template <int G>
__global__ void __launch_bounds__(256)
k_newmark_stage_b3(int64_t n_brows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ bcol, const double *__restrict__ M, double c,
                   const double *__restrict__ u, const double *__restrict__ ut, double *__restrict__ J, double *__restrict__ r)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = threadIdx.x % G;
    const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) / G;
    for (int64_t R = gid / G; R < n_brows; R += ngroups) {
        const int64_t k0 = rowptr[3 * R], k1 = rowptr[3 * R + 1], k2 = rowptr[3 * R + 2];
        const int nblk = (int)((k1 - k0) / 3);
        const int32_t *bc = bcol + k0 / 9;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int j = sub; j < nblk; j += G) {
            const double m = M[k0 + 3 * j];
            if (J) {
                const double cm = c * m;
                J[k0 + 3 * j] += cm;
                J[k1 + 3 * j + 1] += cm;
                J[k2 + 3 * j + 2] += cm;
            }
            if (r) {
                const int64_t col = 3 * (int64_t)bc[j];
                a0 += m * (u[col] - ut[col]);
                a1 += m * (u[col + 1] - ut[col + 1]);
                a2 += m * (u[col + 2] - ut[col + 2]);
            }
        }
        if (r) {
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) {
                a0 += __shfl_xor(a0, o, G);
                a1 += __shfl_xor(a1, o, G);
                a2 += __shfl_xor(a2, o, G);
            }
            if (sub == 0) {
                double *rr = r + 3 * R;
                rr[0] += c * a0; rr[1] += c * a1; rr[2] += c * a2;
            }
        }
    }
}

// Which kernel serves a pattern (tb_pattern::stage_path; decided at the pattern's first stage call).  The block kernel needs more than a CSR of
// 3 × 3 blocks: it reads one entry per block, which is right only where the mass blocks are m·I₃, i.e. where every field node's three dofs are
// 3k, 3k + 1, 3k + 2 in component order.  (A dense pattern — one cell — is a block CSR under ANY numbering; a numbering that puts one component of
// three different nodes into a triple then leaves mass blocks that are not multiples of the identity.)  The dof table decides, not the structure.
static int stage_plan(tb_pattern *pat)
{
    TB_TRY(spmv_plans(pat));
    const tb_mesh *m = pat->mesh;
    const char *force = getenv("TB_NEWMARK_STAGE");
    const bool rows = force && !strcmp(force, "rows");
    bool blocks = pat->b3 > 0 && m->ncomp == 3 && !rows;
    if (blocks) {
        const int64_t nn = m->n_cells * m->nb;
        for (int64_t i = 0; i < nn && blocks; ++i) {
            const int32_t *d = &m->h_cell_dofs[3 * i];
            blocks = d[0] % 3 == 0 && d[1] == d[0] + 1 && d[2] == d[0] + 2;
        }
    }
    if (!blocks && !rows) {
        // Every other pattern runs the composition the stage was measured against — d = u − ũ, r += c·M·d by the pattern's SpMV, J += c·M entry-wise:
        // the fused general kernel beat it at three of four sizes on a component-separated numbering and lost at the fourth (Q1 80³ shuffled: 2.07
        // against 1.28 ms — its two gathers per non-zero against the stream SpMV's one), and a stage must never be slower than what
        // it replaces.  The fused kernel stays reachable for measurement: TB_NEWMARK_STAGE=rows.
        TB_HIP(hipMalloc((void **)&pat->d_stage_d, sizeof(double) * (size_t)pat->n_rows));
    }
    pat->stage_path = blocks ? 1 : rows ? 2 : 3;
    return TB_OK;
}

} // namespace tb

using namespace tb;

extern "C" {

int tb_newmark_predict(tb_device *dev, int64_t n, double dt, double beta, double gamma, const double *d_u, const double *d_v, const double *d_a,
                       double *d_utilde, double *d_vtilde)
{
    TB_REQUIRE(dev && n >= 0 && ((d_u && d_v && d_a && d_utilde && d_vtilde) || n == 0), "tb_newmark_predict: NULL argument");
    TB_REQUIRE(std::isfinite(dt) && std::isfinite(beta) && std::isfinite(gamma), "tb_newmark_predict: non-finite dt, beta or gamma");
    if (n == 0) return TB_OK;
    TB_HIP(hipSetDevice(dev->id));
    hipLaunchKernelGGL(k_newmark_predict, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, dt, (0.5 - beta) * dt * dt, (1.0 - gamma) * dt, d_u, d_v, d_a,
                       d_utilde, d_vtilde);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_newmark_correct(tb_device *dev, int64_t n, double dt, double beta, double gamma, const double *d_u, const double *d_utilde, const double *d_vtilde,
                       double *d_a, double *d_v)
{
    TB_REQUIRE(dev && n >= 0 && ((d_u && d_utilde && d_vtilde && d_a && d_v) || n == 0), "tb_newmark_correct: NULL argument");
    TB_REQUIRE(std::isfinite(dt) && std::isfinite(gamma) && std::isfinite(beta) && beta * dt * dt > 0.0, "tb_newmark_correct: beta·dt² must be positive and finite");
    if (n == 0) return TB_OK;
    TB_HIP(hipSetDevice(dev->id));
    hipLaunchKernelGGL(k_newmark_correct, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, beta * dt * dt, gamma * dt, d_u, d_utilde, d_vtilde, d_a, d_v);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_hermite_interpolate(tb_device *dev, int64_t n, double theta, double dt, int derivative, const double *d_u0, const double *d_v0, const double *d_u1,
                           const double *d_v1, double *d_out)
{
    TB_REQUIRE(dev && n >= 0 && ((d_u0 && d_v0 && d_u1 && d_v1 && d_out) || n == 0), "tb_hermite_interpolate: NULL argument");
    TB_REQUIRE(derivative >= 0 && derivative <= 2, "tb_hermite_interpolate: derivative %d (0, 1 or 2)", derivative);
    TB_REQUIRE(std::isfinite(theta) && std::isfinite(dt) && dt != 0.0, "tb_hermite_interpolate: dt must be finite and non-zero, theta finite");
    if (n == 0) return TB_OK;
    const double th = theta, th2 = th * th, th3 = th2 * th;
    double c[4];
    if (derivative == 0) { c[0] = 2 * th3 - 3 * th2 + 1; c[1] = dt * (th3 - 2 * th2 + th); c[2] = -2 * th3 + 3 * th2; c[3] = dt * (th3 - th2); }
    else if (derivative == 1) { c[0] = (6 * th2 - 6 * th) / dt; c[1] = 3 * th2 - 4 * th + 1; c[2] = (-6 * th2 + 6 * th) / dt; c[3] = 3 * th2 - 2 * th; }
    else { c[0] = (12 * th - 6) / (dt * dt); c[1] = (6 * th - 4) / dt; c[2] = (-12 * th + 6) / (dt * dt); c[3] = (6 * th - 2) / dt; }
    TB_HIP(hipSetDevice(dev->id));
    hipLaunchKernelGGL(k_hermite, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, c[0], c[1], c[2], c[3], d_u0, d_v0, d_u1, d_v1, d_out);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_newmark_stage(tb_pattern *pat, const double *d_Mnz, double c, const double *d_u, const double *d_utilde, double *d_Jnz, double *d_r)
{
    TB_REQUIRE(pat && d_Mnz, "tb_newmark_stage: NULL pattern or mass");
    TB_REQUIRE(std::isfinite(c) && c > 0.0, "tb_newmark_stage: c = 1/(beta dt^2) must be positive and finite (got %g)", c);
    TB_REQUIRE(!d_r || (d_u && d_utilde), "tb_newmark_stage: the residual needs u and the predictor");
    TB_REQUIRE(d_Jnz != d_Mnz && (!d_r || (d_r != d_u && d_r != d_utilde)), "tb_newmark_stage: an output aliases an input");
    if ((!d_Jnz && !d_r) || pat->n_rows == 0) return TB_OK;
    tb_device *dev = pat->mesh->dev;
    TB_HIP(hipSetDevice(dev->id));
    if (d_Jnz) // the value array is rewritten: a sliced mirror of it (tb_spmv_mirror) no longer reflects it
        for (const double *&q : pat->mir_nz) if (q == d_Jnz) q = nullptr;
    if (pat->stage_path == 0 && !dev->capturing) TB_TRY(stage_plan(pat)); // host work, once per pattern: decided before any capture
    const bool blocks = pat->stage_path == 1;                             // a pattern first seen inside a capture runs the fused general kernel (no workspace)
    const double avg = (double)pat->nnz / (double)pat->n_rows;
    if (blocks) {
        const int64_t nbr = pat->n_rows / 3;
#define TB_STAGE_B3(G) hipLaunchKernelGGL((k_newmark_stage_b3<G>), dim3(grid_for(dev, nbr * G, 256)), dim3(256), 0, dev->stream, nbr, pat->d_rowptr, pat->d_bcol, d_Mnz, c, d_u, d_utilde, d_Jnz, d_r)
        if (avg > 108.0) { TB_STAGE_B3(32); } else { TB_STAGE_B3(16); } // blocks per node row: 27 for Q1, 64…125 for Q2
#undef TB_STAGE_B3
        set_last_kernel("k_newmark_stage_b3");
    } else if (pat->stage_path == 3) {
        if (d_r) {
            hipLaunchKernelGGL(k_newmark_diff, dim3(grid_for(dev, pat->n_rows, 256)), dim3(256), 0, dev->stream, pat->n_rows, d_u, d_utilde, pat->d_stage_d);
            TB_HIP(hipGetLastError());
            TB_TRY(launch_spmv(pat, d_Mnz, pat->d_stage_d, c, 1.0, d_r));
        }
        if (d_Jnz) TB_TRY(launch_axpy(dev, pat->nnz, c, d_Mnz, d_Jnz));
        set_last_kernel("newmark stage composition: k_newmark_diff + tb_spmv_csr + k_axpy");
    } else {
#define TB_STAGE_CSR(G) hipLaunchKernelGGL((k_newmark_stage_csr<G>), dim3(grid_for(dev, pat->n_rows * G, 256)), dim3(256), 0, dev->stream, pat->n_rows, pat->d_rowptr, pat->d_colidx, d_Mnz, c, d_u, d_utilde, d_Jnz, d_r)
        if (avg > 96.0) { TB_STAGE_CSR(64); } else if (avg > 40.0) { TB_STAGE_CSR(32); } else { TB_STAGE_CSR(16); }
#undef TB_STAGE_CSR
        set_last_kernel("k_newmark_stage_csr");
    }
    TB_HIP(hipGetLastError());
    return TB_OK;
}

} // extern "C"

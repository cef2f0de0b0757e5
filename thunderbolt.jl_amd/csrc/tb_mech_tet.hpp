// tb_mech_tet.hpp — quasi-static hyperelastic residual / tangent and the weak boundary conditions on tetrahedra:
// vector-valued P1 (TB_TET4) and P2 (TB_TET10) Lagrange fields on the affine four-node geometry.
//
// Same integrals as tb_mechanics.hip (src/modeling/solid/elements.jl:177-313, src/modeling/core/weak_boundary_conditions.jl), same material
// routines (tb_material.hpp hand-derived Holzapfel–Ogden, tb_energy.hpp hyper-dual evaluation of every other energy).  What the simplex changes:
//  * the geometry is affine — J, J⁻¹, detJ and the barycentric gradients ∇λ_v are computed ONCE per cell; the mapped basis gradients follow from
//    them in closed form (P1: ∇N_a = ∇λ_a, constant; P2: (4λ_a − 1)∇λ_a at vertices, 4(λ_j∇λ_i + λ_i∇λ_j) on edges), no reference tables;
//  * P1: F is constant per cell, so a cell with a constant frame and uniform activation evaluates the material ONCE (NQ = 1, weight = volume);
//    nodal microstructure or activation fields evaluate it at the four points of the degree-2 rule;
//  * the element matrix is small (12 × 12 / 30 × 30): it never leaves the registers.  A cell is worked by a group of lanes inside a workgroup
//    (P1: 16 lanes, 8 cells per 128-thread workgroup; P2: one wave, 4 cells per 256-thread workgroup); one lane owns one node pair a ≤ b — ten
//    pairs for P1, 55 for P2 — accumulates its 3 × 3 block over the points and scatters the block and its transpose (𝔸 has major symmetry).
// Strategies: the scatter is a hardware atomic (TB_STRATEGY_ATOMIC) or a plain read-modify-write inside one colour of the cell conflict graph,
// colours in sequence (TB_STRATEGY_PER_COLOR, TB_STRATEGY_ELEMENT: an ordered sum, bit-reproducible); TB_STRATEGY_PATCH takes the faster of the two.
#pragma once
#include <hip/hip_runtime.h>

#include "tb_internal.h"
#include "tb_energy.hpp"
#include "tb_material.hpp"
#include "tb_math.hpp"
#include "tb_mech_common.hpp"

namespace tb {
using namespace tbk;

HOParams make_params(const tb_form *f);      // tb_mechanics.hip
bool form_is_fast_path(const tb_form *f);
EnergyParams make_energy_params(const tb_form *f);

// ---- quadrature (include/tbhip.h names the rules): barycentric coordinate v of point q, weight as a fraction of the reference volume 1/6
// (first-order field: nq = 1, the centroid with the whole volume, or the 4-point degree-2 rule; second-order field: Keast's 8 points)
template <int NB> __device__ __forceinline__ double tet_lambda(int nq, int q, int v)
{
    if (NB == 4) return nq == 1 ? 0.25 : v == q ? 0.5854101966249685 : 0.1381966011250105;
    const double a = q < 4 ? 0.328054696711427 : 0.106952273932930;
    return v == (q & 3) ? 1.0 - 3.0 * a : a;
}
template <int NB> __device__ __forceinline__ double tet_weight(int nq, int q)
{
    if (NB == 4) return nq == 1 ? 1.0 / 6.0 : 1.0 / 24.0;
    return (q < 4 ? 0.138527966511862 : 0.111472033488138) / 6.0;
}
// vertices of edge node a ≥ 4 of the quadratic tetrahedron: (0,1) (1,2) (2,0) (0,3) (1,3) (2,3)
__device__ __forceinline__ int tet_edge_i(int a) { const int e = a - 4; return e < 3 ? e : e - 3; }
__device__ __forceinline__ int tet_edge_j(int a) { const int e = a - 4; return e < 2 ? e + 1 : e == 2 ? 0 : 3; }
// vertex i of local facet lf: (0,2,1) (0,1,3) (1,2,3) (0,3,2), two bits per entry
__device__ __forceinline__ int tet_facet_vertex(int lf, int i)
{
    constexpr uint32_t packed = (0u << 0) | (2u << 2) | (1u << 4) | (0u << 6) | (1u << 8) | (3u << 10) | (1u << 12) | (2u << 14) | (3u << 16) | (0u << 18) | (3u << 20) | (2u << 22);
    return (int)((packed >> (2 * (3 * lf + i))) & 3u);
}

template <int NB> __device__ __forceinline__ double tet_shape(int a, const double (&lam)[4])
{
    if (NB == 4) return lam[0] * (a == 0) + lam[1] * (a == 1) + lam[2] * (a == 2) + lam[3] * (a == 3);
    if (a < 4) { const double l = lam[0] * (a == 0) + lam[1] * (a == 1) + lam[2] * (a == 2) + lam[3] * (a == 3); return l * (2.0 * l - 1.0); }
    const int i = tet_edge_i(a), j = tet_edge_j(a);
    const double li = lam[0] * (i == 0) + lam[1] * (i == 1) + lam[2] * (i == 2) + lam[3] * (i == 3);
    const double lj = lam[0] * (j == 0) + lam[1] * (j == 1) + lam[2] * (j == 2) + lam[3] * (j == 3);
    return 4.0 * li * lj;
}
// mapped gradient of basis function a from the barycentric gradients L[v][k] (LDS) and the barycentric coordinates of the point
template <int NB> __device__ __forceinline__ void tet_grad(int a, const double (&lam)[4], const double *L, double (&g)[3])
{
    if (NB == 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = L[3 * a + k];
    } else if (a < 4) {
        const double l = lam[0] * (a == 0) + lam[1] * (a == 1) + lam[2] * (a == 2) + lam[3] * (a == 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = (4.0 * l - 1.0) * L[3 * a + k];
    } else {
        const int i = tet_edge_i(a), j = tet_edge_j(a);
        const double li = lam[0] * (i == 0) + lam[1] * (i == 1) + lam[2] * (i == 2) + lam[3] * (i == 3);
        const double lj = lam[0] * (j == 0) + lam[1] * (j == 1) + lam[2] * (j == 2) + lam[3] * (j == 3);
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = 4.0 * (lj * L[3 * i + k] + li * L[3 * j + k]);
    }
}
// J = [x₁−x₀ | x₂−x₀ | x₃−x₀]; returns detJ and the barycentric gradients ∇λ_v (rows of J⁻¹ for v = 1…3, minus their sum for v = 0)
__device__ __forceinline__ double tet_geometry(const double *x, double *L)
{
    double J[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) J[i][k] = x[3 * (k + 1) + i] - x[i];
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, id = 1.0 / det;
    const double Ji[9] = {c00 * id, (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id, (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id,
                          c01 * id, (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id, (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id,
                          c02 * id, (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id, (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        L[k] = -(Ji[k] + Ji[3 + k] + Ji[6 + k]);
        L[3 + k] = Ji[k]; L[6 + k] = Ji[3 + k]; L[9 + k] = Ji[6 + k];
    }
    return det;
}

struct TetMesh {
    const double *xyz;
    const int32_t *conn;
    const int32_t *cell_dofs;
    const double *fsn_field; // [cell][vertex 0..3][f|s|n][3]; NULL → constant frame of the material
    const double *act_field; // [cell][vertex 0..3] state multiplying the active tension; NULL → 1
};

template <int NB> struct TetShape {
    static constexpr int LPC = NB == 4 ? 16 : 64;        // lanes per cell
    static constexpr int THREADS = NB == 4 ? 128 : 256;  // 8 / 4 cells per workgroup
    static constexpr int CPW = THREADS / LPC;
    static constexpr int NPAIR = NB * (NB + 1) / 2;
};

// mode: 0 read-modify-write (one colour), 1 hardware atomics
// NEED_K: tangent, plus the residual when r != NULL; !NEED_K: residual only.  AD: the energy EN of tb_energy.hpp fixed at compile time (EN = −1: read from
// the parameter block — prestressed materials), differentiated by hyper-dual evaluation; !AD: hand-derived Holzapfel–Ogden 2009 + SimpleCompressionPenalty.
// nq: points of the rule (first-order field: 1 or 4; second-order: 8)
template <int NB, bool NEED_K, bool AD, int EN>
__global__ void __launch_bounds__(TetShape<NB>::THREADS)
k_tet_mech(TetMesh m, HOParams mat, EnergyParams en, const int32_t *__restrict__ list, int64_t n_cells, int nq, const double *__restrict__ u, double *__restrict__ nz,
           double *__restrict__ r, const int64_t *__restrict__ rowptr, const uint16_t *__restrict__ blockpos, int mode, Status *st)
{
    constexpr int ND = 3 * NB, LPC = TetShape<NB>::LPC, CPW = TetShape<NB>::CPW, NPAIR = TetShape<NB>::NPAIR;
    constexpr int NQ = NB == 4 ? 4 : 8, NG = NB == 4 ? 1 : NQ;            // gradient sets per cell: the first-order gradients do not depend on the point
    constexpr int CS = AD ? 12 : HOC_SIZE;
    static_assert(ND <= LPC && NPAIR <= LPC && NQ <= LPC, "one lane per element unknown / node pair / point");
    __shared__ double s_ue[CPW][ND], s_x[CPW][12], s_L[CPW][12], s_F[CPW][NQ][10], s_G[CPW][NG][NB][3], s_P[CPW][NQ][9], s_C[CPW][NQ][CS];
    __shared__ double s_A[CPW][NEED_K ? NQ : 1][81];
    __shared__ int32_t s_dof[CPW][ND];
    const int g = threadIdx.x / LPC, lt = threadIdx.x % LPC;
    const int64_t ci = (int64_t)blockIdx.x * CPW + g;
    const bool valid = ci < n_cells;                 // idle groups of the last workgroup run cell 0 of the launch and store nothing
    const int64_t cell = list ? list[valid ? ci : 0] : (valid ? ci : 0);

    // load_element_unknowns! (elements.jl:125-132) + vertex coordinates
    if (lt < ND) { const int32_t d = m.cell_dofs[cell * ND + lt]; s_dof[g][lt] = d; s_ue[g][lt] = u[d]; }
    if (lt < 12) s_x[g][lt] = m.xyz[3 * (int64_t)m.conn[cell * 4 + lt / 3] + lt % 3];
    __syncthreads();
    // geometry once per cell (affine map)
    if (lt == 0) {
        const double det = tet_geometry(s_x[g], s_L[g]);
        if (!(det > 0.0)) { st->neg_detj = 1; st->cell = cell; }
        s_F[g][0][9] = det;
    }
    __syncthreads();
    const double det = s_F[g][0][9];
    // mapped gradients of every (point, node)
    for (int idx = lt; idx < NG * NB; idx += LPC) {
        const int q = idx / NB, a = idx - q * NB;
        const double lam[4] = {tet_lambda<NB>(nq, q, 0), tet_lambda<NB>(nq, q, 1), tet_lambda<NB>(nq, q, 2), tet_lambda<NB>(nq, q, 3)};
        double gr[3];
        tet_grad<NB>(a, lam, s_L[g], gr);
#pragma unroll
        for (int k = 0; k < 3; ++k) s_G[g][q][a][k] = gr[k];
    }
    __syncthreads();
    // F = I + Σₐ uₐ ⊗ ∇Nₐ, one lane per (point, c, k); dΩ in slot 9
    for (int t = lt; t < nq * 9; t += LPC) {
        const int q = t / 9, ck = t - 9 * q, c = ck / 3, k = ck - 3 * c;
        double v = c == k ? 1.0 : 0.0;
        for (int a = 0; a < NB; ++a) v += s_ue[g][3 * a + c] * s_G[g][NG == 1 ? 0 : q][a][k];
        s_F[g][q][ck] = v;
    }
    __syncthreads(); // (slot 9 of point 0 was read by every lane above)
    if (lt < nq) s_F[g][lt][9] = det * tet_weight<NB>(nq, lt);
    // frame and active tension of every point: constant, or first-order nodal data interpolated with λ (microstructure.jl:176-187)
    if (lt < nq) {
        const int q = lt;
        double f[3] = {mat.f[0], mat.f[1], mat.f[2]}, sv[3] = {mat.s[0], mat.s[1], mat.s[2]}, nv[3] = {mat.n[0], mat.n[1], mat.n[2]};
        if (m.fsn_field) {
#pragma unroll
            for (int d = 0; d < 3; ++d) { f[d] = 0.0; sv[d] = 0.0; nv[d] = 0.0; }
            const double *fc = m.fsn_field + cell * 36;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const double Na = tet_lambda<NB>(nq, q, a);
#pragma unroll
                for (int d = 0; d < 3; ++d) { f[d] += Na * fc[9 * a + d]; sv[d] += Na * fc[9 * a + 3 + d]; nv[d] += Na * fc[9 * a + 6 + d]; }
            }
            ho_orthonormal_frame(f, sv, nv);
        }
        double ta = AD ? en.Ta : mat.Ta;
        if (m.act_field) {
            double ca = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) ca += tet_lambda<NB>(nq, q, a) * m.act_field[cell * 4 + a];
            ta *= ca;
        }
        if constexpr (AD) {
            double *o = s_C[g][q];
#pragma unroll
            for (int d = 0; d < 3; ++d) { o[d] = f[d]; o[3 + d] = sv[d]; o[6 + d] = nv[d]; }
            o[9] = ta;
        } else {
            double F[3][3];
#pragma unroll
            for (int e = 0; e < 9; ++e) F[e / 3][e % 3] = s_F[g][q][e];
            HOParams mq = mat;
            mq.Ta = ta;
#pragma unroll
            for (int d = 0; d < 3; ++d) { mq.f[d] = f[d]; mq.s[d] = sv[d]; mq.n[d] = nv[d]; }
            ho_common<false>(mq, F, s_C[g][q]);
        }
    }
    __syncthreads();
    if constexpr (AD) {
        // one lane per (point, pair of components of F): Ψ.a = P_m, Ψ.ab = 𝔸_mn = 𝔸_nm
        constexpr int NP = NEED_K ? 45 : 9;
        for (int t = lt; t < nq * NP; t += LPC) {
            const int q = t / NP, pr = t - q * NP;
            int mm = pr, nn = pr;
            if constexpr (NEED_K) pair_components(pr, mm, nn);
            const double *o = s_C[g][q];
            const double f[3] = {o[0], o[1], o[2]}, sv[3] = {o[3], o[4], o[5]}, nv[3] = {o[6], o[7], o[8]};
            HD hd;
            if constexpr (EN >= 0) {
                double da[9], db[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) { da[e] = e == mm ? 1.0 : 0.0; db[e] = e == nn ? 1.0 : 0.0; }
                hd = energy_pair_dir<EN>(en, s_F[g][q], da, db, f, sv, nv, o[9]);
            } else {
                hd = energy_pair(en, s_F[g][q], mm, nn, f, sv, nv, o[9]);
            }
            const double dO = s_F[g][q][9];
            if constexpr (NEED_K) { s_A[g][q][9 * mm + nn] = hd.ab * dO; s_A[g][q][9 * nn + mm] = hd.ab * dO; }
            if (mm == nn) s_P[g][q][mm] = hd.a * dO;
        }
    } else {
        // one lane per (point, i, j): row (i, j) of P·dΩ and 𝔸·dΩ
        for (int t = lt; t < nq * 9; t += LPC) {
            const int q = t / 9, ij = t - 9 * q;
            double Pij;
            if constexpr (NEED_K) {
                double row[9];
                ho_row<true>(mat, s_C[g][q], s_F[g][q], ij / 3, ij % 3, s_F[g][q][9], Pij, row);
#pragma unroll
                for (int e = 0; e < 9; ++e) s_A[g][q][9 * ij + e] = row[e];
            } else {
                ho_row<false>(mat, s_C[g][q], s_F[g][q], ij / 3, ij % 3, s_F[g][q][9], Pij, nullptr);
            }
            s_P[g][q][ij] = Pij;
        }
    }
    __syncthreads();
    // rₑ[(a,c)] = Σ_q ∇Nₐ · P_q[c][·] dΩ
    if (r) {
        if (lt < ND) {
            const int a = lt / 3, c = lt - 3 * a;
            double acc = 0.0;
            for (int q = 0; q < nq; ++q) {
                const double *gr = s_G[g][NG == 1 ? 0 : q][a], *p = s_P[g][q] + 3 * c;
                acc += gr[0] * p[0] + gr[1] * p[1] + gr[2] * p[2];
            }
            if (valid) { if (mode) unsafeAtomicAdd(r + s_dof[g][lt], acc); else r[s_dof[g][lt]] += acc; }
        }
    }
    // Kₑ[(a,c)][(b,d)] = Σ_q Σ_kl ∇Nₐ[k] 𝔸_q[c][k][d][l] ∇N_b[l] dΩ for the lane's node pair a ≤ b; the block (b, a) is its transpose
    if constexpr (NEED_K) {
        if (lt < NPAIR) {
            int a = 0, b = lt;
            while (b >= NB - a) { b -= NB - a; ++a; }
            b += a;
            double K[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) K[e] = 0.0;
            for (int q = 0; q < nq; ++q) {
                const double *ga = s_G[g][NG == 1 ? 0 : q][a], *gb = s_G[g][NG == 1 ? 0 : q][b], *A = s_A[g][q];
                const double a0 = ga[0], a1 = ga[1], a2 = ga[2], b0 = gb[0], b1 = gb[1], b2 = gb[2];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const double *A0 = A + 9 * (3 * c) + 3 * d, *A1 = A0 + 9, *A2 = A0 + 18;
                        K[3 * c + d] += (a0 * A0[0] + a1 * A1[0] + a2 * A2[0]) * b0 + (a0 * A0[1] + a1 * A1[1] + a2 * A2[1]) * b1 +
                                        (a0 * A0[2] + a1 * A1[2] + a2 * A2[2]) * b2;
                    }
            }
            if (valid) {
                // assemble!(assembler, dofs, Kₑ): rows (a, c) / columns (b, d) and the mirrored block
                const int64_t pab = blockpos[cell * (NB * NB) + a * NB + b], pba = blockpos[cell * (NB * NB) + b * NB + a];
                const int32_t da = s_dof[g][3 * a], db = s_dof[g][3 * b];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int64_t k1 = rowptr[da + c] + pab;
#pragma unroll
                    for (int d = 0; d < 3; ++d) { if (mode) unsafeAtomicAdd(nz + k1 + d, K[3 * c + d]); else nz[k1 + d] += K[3 * c + d]; }
                }
                if (a != b) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const int64_t k2 = rowptr[db + d] + pba;
#pragma unroll
                        for (int c = 0; c < 3; ++c) { if (mode) unsafeAtomicAdd(nz + k2 + c, K[3 * c + d]); else nz[k2 + c] += K[3 * c + d]; }
                    }
                }
            }
        }
    }
}

template <int NB, bool NEED_K, bool AD, int EN>
static int run_tet(int nq, tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    const TetMesh tm{m->d_xyz, m->d_conn, m->d_cell_dofs, f->d_field, f->d_act_field};
    const HOParams hp = make_params(f);
    const EnergyParams ep = make_energy_params(f);
    if (NEED_K) {
        int rc = ensure_blockpos(p);
        if (rc) return rc;
        if (!f->accumulate) TB_HIP(hipMemsetAsync(d_nz, 0, (size_t)p->nnz * sizeof(double), dev->stream));
    }
    if (d_r && !f->accumulate) TB_HIP(hipMemsetAsync(d_r, 0, (size_t)m->ndofs * sizeof(double), dev->stream));
    const int64_t *rowptr = p ? p->d_rowptr : nullptr;
    const uint16_t *bp = p ? p->d_blockpos : nullptr;
    constexpr int CPW = TetShape<NB>::CPW;
    auto go = [&](const int32_t *list, int64_t n, int mode) -> int {
        if (!n) return TB_OK;
        hipLaunchKernelGGL((k_tet_mech<NB, NEED_K, AD, EN>), dim3((unsigned)((n + CPW - 1) / CPW)), dim3(TetShape<NB>::THREADS), 0, dev->stream, tm, hp, ep,
                           list, n, nq, d_u, d_nz, d_r, rowptr, bp, mode, dev->d_status);
        TB_HIP(hipGetLastError());
        return TB_OK;
    };
    // TB_STRATEGY_PATCH (the callers' default) takes the scatter measured faster for the field (DESIGN.md §4.4b, 24³ lattice): atomics for the first-order
    // field (0.51 against 0.55 ms), colours for the second-order one (1.59 against 2.58 ms: 900 FP64 atomics per cell contend in L2)
    const bool coloured = strategy == TB_STRATEGY_PER_COLOR || strategy == TB_STRATEGY_ELEMENT || (strategy == TB_STRATEGY_PATCH && NB == 10);
    set_last_kernel("k_tet_mech<%s,%s,%s,EN%d>(nq=%d,%s)", NB == 4 ? "P1" : "P2", NEED_K ? (d_r ? "K+r" : "K") : "r", AD ? "AD" : "HO", EN, nq, coloured ? "colours" : "atomic");
    if (coloured) {
        const ColorPlan *cp;
        if (f->has_cellset) {
            if (!f->set_colors) { int rc = build_color_plan_subset(m, f->h_cellset, f->set_colors); if (rc) return rc; }
            cp = f->set_colors.get();
        } else {
            if (!m->colors) { int rc = build_color_plan(m); if (rc) return rc; }
            cp = m->colors.get();
        }
        for (int c = 0; c < cp->ncolors; ++c) {
            int rc = go(cp->d_cells + cp->offsets[c], cp->offsets[c + 1] - cp->offsets[c], 0);
            if (rc) return rc;
        }
        return TB_OK;
    }
    if (strategy == TB_STRATEGY_ATOMIC || strategy == TB_STRATEGY_PATCH) return f->has_cellset ? go(f->d_cellset, f->n_set, 1) : go(nullptr, m->n_cells, 1);
    set_error("hyperelastic assembly: unknown strategy %d", strategy);
    return TB_ERR_UNSUPPORTED;
}

// material dispatch of one field: hand-derived Holzapfel–Ogden, or the energy fixed at compile time (run-time form for prestressed materials)
template <int NB>
static int dispatch_tet(tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r)
{
    const int nq = NB == 10 ? 8 : (f->d_field || f->d_act_field) ? 4 : 1; // first-order field: one material evaluation per cell unless nodal data vary inside it
#define TB_TET_RUN(ADV, ENV) (d_nz ? run_tet<NB, true, ADV, ENV>(nq, f, p, strategy, d_u, d_nz, d_r) : run_tet<NB, false, ADV, ENV>(nq, f, p, strategy, d_u, d_nz, d_r))
    if (form_is_fast_path(f)) return TB_TET_RUN(false, -1);
    if (f->prestressed) return TB_TET_RUN(true, -1);
    switch (f->mat.kind) {
    case EN_NULL: return TB_TET_RUN(true, EN_NULL);
    case EN_BIO_NEOHOOKEAN: return TB_TET_RUN(true, EN_BIO_NEOHOOKEAN);
    case EN_TI_NEOHOOKEAN: return TB_TET_RUN(true, EN_TI_NEOHOOKEAN);
    case EN_LIN_YIN_PASSIVE: return TB_TET_RUN(true, EN_LIN_YIN_PASSIVE);
    case EN_LIN_YIN_ACTIVE: return TB_TET_RUN(true, EN_LIN_YIN_ACTIVE);
    case EN_HUMPHREY_STRUMPF_YIN: return TB_TET_RUN(true, EN_HUMPHREY_STRUMPF_YIN);
    case EN_LINEAR_SPRING: return TB_TET_RUN(true, EN_LINEAR_SPRING);
    case EN_GUCCIONE_1991: return TB_TET_RUN(true, EN_GUCCIONE_1991);
    default: return TB_TET_RUN(true, EN_HOLZAPFEL_OGDEN); // (with another penalty than the fast path's)
    }
#undef TB_TET_RUN
}

int launch_hyperelastic_tet4(tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r); // tb_mech_tet4.hip: the first-order instances

} // namespace tb

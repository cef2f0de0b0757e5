// tb_mechanics.hip — quasi-static hyperelastic residual / tangent element kernels (Holzapfel–Ogden 2009),
// vector-valued Q1 and Q2 Lagrange fields on trilinear hexahedra.
//
// Restates src/modeling/solid/elements.jl:177-225 (K and r), :227-273 (K), :275-313 (r):
//   per quadrature point  ∇u = Σ uₑᵢ ∇δuᵢ,  F = I + ∇u,  (P, 𝔸) = material_routine(F)   (materials.jl:442-453,1025-1040)
//   rₑ[i] += ∇δuᵢ ⊡ P dΩ,   Kₑ[i,j] += (∇δuᵢ ⊡ 𝔸) ⊡ ∇δuⱼ dΩ,   dof i = 3a + c ↔ ∇δuᵢ = e_c ⊗ ∇Nₐ.
// The cell loop / load_element_unknowns! / assemble! belong to FerriteOperators (third party); call sites
// src/solver/nonlinear/newton_raphson.jl:234-238, src/solver/time/homotopy.jl:61-67.
//
// One workgroup per cell (k_hyperelastic).  The tangent of a cell is contracted
//  * Q2: by sum factorisation over the tensor-product structure of the triquadratic basis and the 3×3×3 Gauss rule, with the tangent pulled
//    back to the reference cell (comment at "B (sum factorisation)" below); on the element strategy a symmetric tangent goes through the two
//    kernels of tb_mech_split.hip instead, the fused kernel keeps the rate-coupled (non-symmetric) one and the other strategies;
//  * Q1: in two steps over the quadrature points, T[a][c][d][l] = Σ_k ∇Nₐ[k] 𝔸[c][k][d][l] staged in LDS and then
//    Kₑ[(a,c)][(b,d)] += Σ_l T[a][c][d][l] ∇N_b[l] with 3×3 blocks in registers — 27·NB² FMAs per point instead of 81·NB².
// The contractions that were built, measured and removed (matrix cores, the plain sweep for Q2, symmetric-packed storage): DESIGN.md §4.4.
// This unit: the kernel, the pre-pass of the condensed internal variables, the dispatch.  Second pass of the element strategy:
// tb_mech_gather.hip; weak boundary conditions: tb_mech_facets.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tb_internal.h"
#include "tb_energy.hpp"
#include "tb_material.hpp"
#include "tb_math.hpp"
#include "tb_mech_common.hpp"
#include "tb_mech_gather.hpp"
#include "tb_mech_split.hpp"

namespace tb {
using namespace tbk;

// position of column dof(b,0) inside row dof(a,0), per cell and node pair (the three component rows of a node
// share one column set, so the same position serves rows +1, +2 and columns +1, +2)
__global__ void k_build_blockpos(const int32_t *__restrict__ cell_dofs, int64_t n_cells, int nb, const int64_t *__restrict__ rowptr,
                                 const int32_t *__restrict__ colidx, uint16_t *__restrict__ pos, Status *st)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_cells * nb * nb) return;
    const int64_t cell = tid / (nb * nb);
    const int a = (int)(tid % (nb * nb)) / nb, b = (int)(tid % nb);
    const int32_t *d = cell_dofs + cell * 3 * nb;
    const int32_t row = d[3 * a], col = d[3 * b];
    const int64_t lo0 = rowptr[row], hi0 = rowptr[row + 1];
    int64_t lo = lo0, hi = hi0;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (colidx[mid] < col) lo = mid + 1; else hi = mid;
    }
    if (lo >= hi0 || colidx[lo] != col || lo - lo0 > 0xFFFF) { st->pattern_missing = 1; st->cell = cell; lo = lo0; }
    pos[tid] = (uint16_t)(lo - lo0);
}

// AD: the material is any energy of tb_energy.hpp, differentiated per pair of components of F by hyper-dual evaluation (the
// reference's Tensors.hessian path); !AD: Holzapfel–Ogden 2009 + SimpleCompressionPenalty with the hand-derived routines.
template <class FE, bool NEED_K, bool NEED_R, bool AD>
__global__ void __launch_bounds__(FE::THREADS, FE::WAVES)
k_hyperelastic(MechMesh m, HOParams mat, EnergyParams en, const int32_t *__restrict__ list, const double *__restrict__ u, double *__restrict__ nz,
               double *__restrict__ r, const int64_t *__restrict__ rowptr, const uint16_t *__restrict__ blockpos, int atomic /*0 rmw, 1 atomic, 2 store Kₑ/rₑ*/,
               double *__restrict__ ke, double *__restrict__ re, Status *st)
{
    constexpr int NB = FE::NB, NQ = FE::NQ, ND = FE::ND, PB = FE::PB, T = FE::THREADS, NG = NB / PB;
    constexpr bool SF = NEED_K && NB == 27; // tangent of the triquadratic field: sum-factorised contraction; otherwise the sweep over the points
    // sum-factorised tangent: the mapped gradients ∇N = ∂̂N·J⁻¹ are never formed.  ∇u = Ĥ·J⁻¹ with Ĥ[c][s] = Σₐ uₐ[c] ∂̂ₛNₐ (reference gradients from the
    // 1-D factors in registers, concurrent with the Jacobians), the tangent and the stress are pulled back to the reference cell (stage 0), and the
    // residual contracts the pulled-back stress with the reference gradients: two barriers and the 729-task gradient pass less per cell
    constexpr bool REFGRAD = SF || (!NEED_K && NEED_R && NB == 27 && NQ == 27 && T == 256); // (the residual-only kernel of the quadratic field too)
    const MechTables<FE> &tb = g_mech_tables<FE>;
    const int64_t cell = list ? list[blockIdx.x] : m.cell0 + blockIdx.x;
    const int tid = threadIdx.x;
#ifdef TB_ABLATION
#define TB_MS(k) do { if (m.prof && tid == 0 && (blockIdx.x & 255) == 7) m.prof[(blockIdx.x >> 8) * 16 + (k)] = wall_clock64(); } while (0)
#else
#define TB_MS(k) do { } while (0)
#endif
    TB_MS(0);
    __shared__ double s_ue[ND], s_x[24], s_JI[NQ][10], s_P[NQ][9];
    // 𝔸·dΩ per point and the mapped gradients (sum-factorised contraction: its stage buffer Z1) share one block
    // (dynamic LDS: with the stage buffers of the sum-factorised contraction the kernel's block exceeds the 64 KB a static allocation may have)
    constexpr int AN = (NEED_K ? NQ : 1) * 81;
    extern __shared__ double s_AG[];
    double (*s_A)[81] = reinterpret_cast<double (*)[81]>(s_AG);
    double (*s_G)[NB][3] = reinterpret_cast<double (*)[NB][3]>(s_AG + AN);
    // phase A scratch (common blocks + F) and phase B's double-buffered T share one region
    constexpr int TC_SIZE = (NEED_K && !SF && 2 * NB * 27 > NQ * HOC_SIZE) ? 2 * NB * 27 : NQ * HOC_SIZE;
    __shared__ double s_Ji[REFGRAD ? NQ : 1][9]; // J⁻¹ kept for the pull-backs of 𝔸 and P (the slots of s_JI carry F)
    __shared__ double s_TC[TC_SIZE];
    double (*s_T)[NB][27] = reinterpret_cast<double (*)[NB][27]>(s_TC);
    double (*s_C)[HOC_SIZE] = reinterpret_cast<double (*)[HOC_SIZE]>(s_TC);
    __shared__ int32_t s_dof[ND];

    __shared__ uint8_t s_node[32], s_tix[32]; // tensor index t₀ + 3t₁ + 9t₂ → Ferrite node and back (LDS copies: a load from the constant table in the
                                              // middle of the kernel queues behind the element-matrix stores of the other workgroups, ≈ 1.5 µs)
    if constexpr (REFGRAD) {
        // load_element_unknowns! (elements.jl:125-132): dofs → u is two dependent trips; the Jacobians of the points are computed inside the second
        // one — vertex coordinates from the cell-major array with wave-uniform addresses (scalar loads: one trip, no connectivity chase, no LDS
        // staging), ∂M/∂ξ and the weights from the vertex signs and the 1-D rule in registers (no table loads with lane-varying addresses)
        static_assert(ND <= T && NB == 27, "one lane per element unknown");
        int32_t dof = 0;
        double uv = 0.0;
        if (tid < ND) { dof = m.cell_dofs[cell * ND + tid]; uv = u[dof]; }
        if (tid < 27) { const int a = g_hex27_node[tid]; s_node[tid] = (uint8_t)a; s_tix[a] = (uint8_t)tid; }
        if (tid < NQ) { // A1: J, J⁻¹, dΩ per point (PR883.jl:253-263,367-387)
            const int q = tid, qd[3] = {q % 3, (q / 3) % 3, q / 9};
            double mm_[3], pp_[3], wq = 1.0;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double xi = qd[d] == 0 ? G3::x(0) : qd[d] == 1 ? G3::x(1) : G3::x(2);
                mm_[d] = 1.0 - xi; pp_[d] = 1.0 + xi;
                wq *= qd[d] == 1 ? G3::w(1) : G3::w(0);
            }
            const double *X = m.cell_xyz + cell * 24;
            double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const double f0 = hex_sgn(a, 0) > 0 ? pp_[0] : mm_[0], f1 = hex_sgn(a, 1) > 0 ? pp_[1] : mm_[1], f2 = hex_sgn(a, 2) > 0 ? pp_[2] : mm_[2];
                const double dm[3] = {0.125 * hex_sgn(a, 0) * f1 * f2, 0.125 * hex_sgn(a, 1) * f0 * f2, 0.125 * hex_sgn(a, 2) * f0 * f1};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double xa = X[3 * a + i];
#pragma unroll
                    for (int k = 0; k < 3; ++k) J[i][k] += xa * dm[k];
                }
            }
            const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
            const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, id = 1.0 / det;
            double o[10];
            o[0] = c00 * id; o[1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id; o[2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
            o[3] = c01 * id; o[4] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id; o[5] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
            o[6] = c02 * id; o[7] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id; o[8] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
            o[9] = det * wq;
            if (!(o[9] > 0.0)) { st->neg_detj = 1; st->cell = cell; }
#pragma unroll
            for (int e = 0; e < 9; ++e) s_Ji[q][e] = o[e];
            s_JI[q][9] = o[9];
        }
        if (tid < ND) { s_dof[tid] = dof; s_ue[tid] = uv; }
        __syncthreads();
        TB_MS(1);
    } else {
    // load_element_unknowns! (elements.jl:125-132) + cell coordinates
    for (int i = tid; i < ND; i += T) {
        const int32_t d = m.cell_dofs[cell * ND + i];
        s_dof[i] = d;
        s_ue[i] = u[d];
    }
    for (int i = tid; i < 24; i += T) s_x[i] = m.xyz[3 * (int64_t)m.conn[cell * 8 + i / 3] + i % 3];
    __syncthreads();
    TB_MS(1);
    }

    // A1: J, J⁻¹, dΩ per point (PR883.jl:253-263,367-387)
    if (!REFGRAD && tid < NQ) {
        const int q = tid;
        double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) J[i][k] += s_x[3 * a + i] * tb.dM[q][a][k];
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, id = 1.0 / det;
        double *o = s_JI[q];
        o[0] = c00 * id; o[1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id; o[2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
        o[3] = c01 * id; o[4] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id; o[5] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
        o[6] = c02 * id; o[7] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id; o[8] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
        o[9] = det * tb.w[q];
        if (!(o[9] > 0.0)) { st->neg_detj = 1; st->cell = cell; }
    }
    if constexpr (REFGRAD) {
        // A2': Ĥ[c][s] = Σₐ uₐ[c] ∂̂ₛNₐ(ξ_q), one lane per (point, c, s) — needs the element unknowns only, so it shares the phase with A1
        if (tid < NQ * 9) {
            const int q = tid / 9, cs = tid - 9 * q, c = cs / 3, s_ = cs - 3 * c;
            const int q0 = q % 3, q1 = (q / 3) % 3, q2 = q / 9;
            auto PHq = [](int i, int qq) { return qq == 0 ? quad1d(i, G3::x(0)) : qq == 1 ? quad1d(i, G3::x(1)) : quad1d(i, G3::x(2)); };
            auto DPq = [](int i, int qq) { return qq == 0 ? dquad1d(i, G3::x(0)) : qq == 1 ? dquad1d(i, G3::x(1)) : dquad1d(i, G3::x(2)); };
            double f0[3], f1[3], f2[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                f0[i] = s_ == 0 ? DPq(i, q0) : PHq(i, q0);
                f1[i] = s_ == 1 ? DPq(i, q1) : PHq(i, q1);
                f2[i] = s_ == 2 ? DPq(i, q2) : PHq(i, q2);
            }
            double h = 0.0;
#pragma unroll
            for (int a2 = 0; a2 < 3; ++a2) {
                double h1 = 0.0;
#pragma unroll
                for (int a1 = 0; a1 < 3; ++a1) {
                    double h0 = 0.0;
#pragma unroll
                    for (int a0 = 0; a0 < 3; ++a0) h0 += f0[a0] * s_ue[3 * make_hex27_nodes().v[(a0 + 3 * a1 + 9 * a2) % (NB == 27 ? 27 : 1)] + c];
                    h1 += f1[a1] * h0;
                }
                h += f2[a2] * h1;
            }
            s_P[q][cs] = h; // the stress block is free until A3c
        }
    } else {
    __syncthreads();
    // A2: mapped gradients ∇Nₐ = ∂Nₐ/∂ξ · J⁻¹ for every (point, node)
    for (int idx = tid; idx < NQ * NB; idx += T) {
        const int q = idx / NB, a = idx % NB;
        const double *ji = s_JI[q];
        const double d0 = tb.dN[q][a][0], d1 = tb.dN[q][a][1], d2 = tb.dN[q][a][2];
#pragma unroll
        for (int k = 0; k < 3; ++k) s_G[q][a][k] = d0 * ji[k] + d1 * ji[3 + k] + d2 * ji[6 + k];
    }
    __syncthreads();
    // A3a: F = I + ∇u, one lane per (point, component c, direction k)
    for (int t = tid; t < NQ * 9; t += T) {
        const int q = t / 9, ck = t % 9, c = ck / 3, k = ck % 3;
        double v = c == k ? 1.0 : 0.0;
        for (int a = 0; a < NB; ++a) v += s_ue[3 * a + c] * s_G[q][a][k];
        s_JI[q][ck] = v; // J⁻¹ is dead after A2: its slots carry F from here on
    }
    }
    __syncthreads();
    TB_MS(2);
    // F = I + Ĥ·J⁻¹ by the lane of the point (the lanes that evaluate the material next), into the slots of s_JI like A3a
    auto deformation_gradient = [&](int q) {
        const double *ji = s_Ji[q], *H = s_P[q];
        double Fv[9];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) Fv[3 * c + k] = (c == k ? 1.0 : 0.0) + H[3 * c] * ji[k] + H[3 * c + 1] * ji[3 + k] + H[3 * c + 2] * ji[6 + k];
#pragma unroll
        for (int e = 0; e < 9; ++e) s_JI[q][e] = Fv[e];
    };
    if constexpr (AD) {
        // A3b': frame and active tension of every point (constant, or interpolated nodal data like OrthotropicMicrostructureModel)
        if (tid < NQ) {
            if constexpr (REFGRAD) deformation_gradient(tid);
            double f[3] = {mat.f[0], mat.f[1], mat.f[2]}, sv[3] = {mat.s[0], mat.s[1], mat.s[2]}, n[3] = {mat.n[0], mat.n[1], mat.n[2]};
            if (m.fsn_field) {
                for (int d = 0; d < 3; ++d) { f[d] = 0.0; sv[d] = 0.0; n[d] = 0.0; }
                const double *fc = m.fsn_field + cell * 72;
                for (int a = 0; a < 8; ++a) {
                    const double Na = tb.M[tid][a];
                    for (int d = 0; d < 3; ++d) { f[d] += Na * fc[9 * a + d]; sv[d] += Na * fc[9 * a + 3 + d]; n[d] += Na * fc[9 * a + 6 + d]; }
                }
                ho_orthonormal_frame(f, sv, n);
            }
            double ta = en.Ta;
            if (m.act_field) { double ca = 0.0; for (int a = 0; a < 8; ++a) ca += tb.M[tid][a] * m.act_field[cell * 8 + a]; ta *= ca; }
            double *o = s_C[tid];
            for (int d = 0; d < 3; ++d) { o[d] = f[d]; o[3 + d] = sv[d]; o[6 + d] = n[d]; }
            o[9] = ta;
            o[10] = 0.0;
            if (m.qp_act) { o[9] = m.qp_act[m.qp_stride * (cell * NQ + tid)]; o[10] = m.qp_act[m.qp_stride * (cell * NQ + tid) + 1]; }
        }
        __syncthreads();
        // A3c': one lane per (point, pair of components of F): Ψ.a = P_m, Ψ.ab = 𝔸_mn = 𝔸_nm
        constexpr int NP = NEED_K ? 45 : 9;
        for (int t = tid; t < NQ * NP; t += T) {
            const int q = t / NP, pr = t - q * NP;
            int mm = pr, nn = pr;
            if constexpr (NEED_K) pair_components(pr, mm, nn);
            const double *o = s_C[q];
            const double f[3] = {o[0], o[1], o[2]}, sv[3] = {o[3], o[4], o[5]}, n[3] = {o[6], o[7], o[8]};
            const HD r = energy_pair(en, s_JI[q], mm, nn, f, sv, n, o[9]);
            const double dO = s_JI[q][9];
            if constexpr (NEED_K) {
                double ab = r.ab;
                if (o[10] != 0.0) { // condensed internal variable: + b (∂λ/∂F)_m (∂λ/∂F)_n, ∂λ/∂F = (F f₀) ⊗ f₀ / λ
                    const double *Fq = s_JI[q];
                    const double g0 = Fq[0] * f[0] + Fq[1] * f[1] + Fq[2] * f[2], g1 = Fq[3] * f[0] + Fq[4] * f[1] + Fq[5] * f[2],
                                 g2 = Fq[6] * f[0] + Fq[7] * f[1] + Fq[8] * f[2];
                    const double gv[3] = {g0, g1, g2};
                    ab += o[10] * (gv[mm / 3] * f[mm % 3]) * (gv[nn / 3] * f[nn % 3]) / (g0 * g0 + g1 * g1 + g2 * g2);
                }
                if (m.qp_act && m.qp_stride == 5) { // rate-coupled internal variable: the non-symmetric rank-one term, both orderings of the pair
                    const double *Fq = s_JI[q], *cw = m.qp_act + 5 * (cell * NQ + q) + 2;
                    const double g0 = Fq[0] * f[0] + Fq[1] * f[1] + Fq[2] * f[2], g1 = Fq[3] * f[0] + Fq[4] * f[1] + Fq[5] * f[2],
                                 g2 = Fq[6] * f[0] + Fq[7] * f[1] + Fq[8] * f[2];
                    const double gv[3] = {g0, g1, g2}, il = 1.0 / sqrt(g0 * g0 + g1 * g1 + g2 * g2);
                    const double amn = gv[mm / 3] * f[mm % 3] * il * cw[nn / 3] * f[nn % 3], anm = gv[nn / 3] * f[nn % 3] * il * cw[mm / 3] * f[mm % 3];
                    s_A[q][9 * mm + nn] = (ab + amn) * dO;
                    if (mm != nn) s_A[q][9 * nn + mm] = (ab + anm) * dO;
                } else {
                s_A[q][9 * mm + nn] = ab * dO; s_A[q][9 * nn + mm] = ab * dO;
                }
            }
            if (mm == nn) s_P[q][mm] = r.a * dO;
        }
        __syncthreads();
    } else {
    // A3b: the quantities shared by all entries of P and 𝔸 at a point.  256-thread workgroups: four independent parts of the block, one per wave
    // (lane = point), instead of the whole block on one lane per point while three waves wait; 64-thread workgroups: one lane per point
    {
        constexpr bool SPLIT = T >= 256;
        const int part = SPLIT ? tid >> 6 : 0, q = SPLIT ? tid & 63 : tid;
        if (q < NQ && part < 4) {
            double F[3][3];
            if constexpr (REFGRAD) { // F = I + Ĥ·J⁻¹ (every part for itself; part 0 also leaves it in the slots of s_JI, where A3c reads it)
                const double *ji = s_Ji[q], *H = s_P[q];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int k = 0; k < 3; ++k) F[c][k] = (c == k ? 1.0 : 0.0) + H[3 * c] * ji[k] + H[3 * c + 1] * ji[3 + k] + H[3 * c + 2] * ji[6 + k];
                if (part == 0) {
#pragma unroll
                    for (int e = 0; e < 9; ++e) s_JI[q][e] = F[e / 3][e % 3];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 9; ++e) F[e / 3][e % 3] = s_JI[q][e];
            }
            HOParams mq = mat;
            if (m.act_field) { // Ta(x_q) = Tmax·Σₐ Mₐ(ξ_q)·state[cell][a] (coefficients.jl:85-99, contraction.jl:166-175)
                double ca = 0.0;
                for (int a = 0; a < 8; ++a) ca += tb.M[q][a] * m.act_field[cell * 8 + a];
                mq.Ta = mat.Ta * ca;
            }
            if (m.qp_act) { mq.Ta = m.qp_act[m.qp_stride * (cell * NQ + q)]; mq.Tb = m.qp_act[m.qp_stride * (cell * NQ + q) + 1]; }
            if (m.fsn_field) { // interpolate the nodal frame, normalise, Gram–Schmidt (microstructure.jl:176-187)
                double f[3] = {0, 0, 0}, s[3] = {0, 0, 0}, n[3] = {0, 0, 0};
                const double *fc = m.fsn_field + cell * 72;
                for (int a = 0; a < 8; ++a) {
                    const double Na = tb.M[q][a];
#pragma unroll
                    for (int d = 0; d < 3; ++d) { f[d] += Na * fc[9 * a + d]; s[d] += Na * fc[9 * a + 3 + d]; n[d] += Na * fc[9 * a + 6 + d]; }
                }
                ho_orthonormal_frame(f, s, n);
#pragma unroll
                for (int d = 0; d < 3; ++d) { mq.f[d] = f[d]; mq.s[d] = s[d]; mq.n[d] = n[d]; }
            }
            if constexpr (SPLIT) {
                if (part == 0) ho_common_part<0>(mq, F, s_C[q]);
                else if (part == 1) ho_common_part<1>(mq, F, s_C[q]);
                else if (part == 2) ho_common_part<2>(mq, F, s_C[q]);
                else ho_common_part<3>(mq, F, s_C[q]);
            } else {
                ho_common<false>(mq, F, s_C[q]);
            }
        }
    }
    __syncthreads();
    TB_MS(3);
    // A3c: one lane per (point, i, j): row (i,j) of P·dΩ and 𝔸·dΩ
    for (int t = tid; t < NQ * 9; t += T) {
        const int q = t / 9, ij = t % 9;
        double Pij;
        if constexpr (NEED_K) {
            double row[9];
            ho_row<true>(mat, s_C[q], s_JI[q], ij / 3, ij % 3, s_JI[q][9], Pij, row);
            if (m.qp_act && m.qp_stride == 5) { // rate-coupled internal variable: + (∂λ/∂F)_ij (c·w)_k f_l, the only non-symmetric part of the tangent
                const double *Fq = s_JI[q], *fv = s_C[q] + HOC_FV, *cw = m.qp_act + 5 * (cell * NQ + q) + 2;
                const int i = ij / 3, j = ij % 3;
                const double g0 = Fq[0] * fv[0] + Fq[1] * fv[1] + Fq[2] * fv[2], g1 = Fq[3] * fv[0] + Fq[4] * fv[1] + Fq[5] * fv[2],
                             g2 = Fq[6] * fv[0] + Fq[7] * fv[1] + Fq[8] * fv[2];
                const double dl = (i == 0 ? g0 : i == 1 ? g1 : g2) * fv[j] / sqrt(g0 * g0 + g1 * g1 + g2 * g2) * s_JI[q][9];
#pragma unroll
                for (int e = 0; e < 9; ++e) row[e] += dl * cw[e / 3] * fv[e % 3];
            }
#pragma unroll
            for (int e = 0; e < 9; ++e) s_A[q][9 * ij + e] = row[e];
        } else {
            ho_row<false>(mat, s_C[q], s_JI[q], ij / 3, ij % 3, s_JI[q][9], Pij, nullptr);
        }
        s_P[q][ij] = Pij;
    }
    __syncthreads();

    }
    TB_MS(4);
    double racc = 0.0;
    // rₑ[(a,c)] = Σ_q Σ_s ∂̂ₛNₐ(ξ_q) P̂_q[c][s] for the lane's element unknown (reference-gradient path; P̂ = the pulled-back stress in s_P): the reference
    // gradients of the lane's node come from its 1-D factors
    auto residual_refgrad = [&]() {
        auto PHr = [](int i, int q) constexpr { return quad1d(i, G3::x(q)); };
        auto DPr = [](int i, int q) constexpr { return dquad1d(i, G3::x(q)); };
        double acc = 0.0;
        if (tid < ND) {
            const int a = tid / 3, c = tid - 3 * a;
            double fa[3][3], da[3][3]; // [direction][point]
            const int ta = s_tix[a];
#pragma unroll
            for (int dir = 0; dir < 3; ++dir) {
                const int i = dir == 0 ? ta % 3 : dir == 1 ? (ta / 3) % 3 : ta / 9;
#pragma unroll
                for (int qq = 0; qq < 3; ++qq) {
                    fa[dir][qq] = i == 0 ? PHr(0, qq) : i == 1 ? PHr(1, qq) : PHr(2, qq);
                    da[dir][qq] = i == 0 ? DPr(0, qq) : i == 1 ? DPr(1, qq) : DPr(2, qq);
                }
            }
#pragma unroll
            for (int q2 = 0; q2 < 3; ++q2)
#pragma unroll
                for (int q1 = 0; q1 < 3; ++q1) {
                    const double m12 = fa[1][q1] * fa[2][q2], d1 = da[1][q1] * fa[2][q2], d2 = fa[1][q1] * da[2][q2];
#pragma unroll
                    for (int q0 = 0; q0 < 3; ++q0) {
                        const double *pp = s_P[(q0 + 3 * q1 + 9 * q2) % NQ] + 3 * c;
                        acc += da[0][q0] * m12 * pp[0] + fa[0][q0] * (d1 * pp[1] + d2 * pp[2]);
                    }
                }
        }
        return acc;
    };
    if constexpr (SF) {
        // B (sum factorisation).  Kₑ[(a,c)][(b,d)] = Σ_q Σ_su ∂̂ₛNₐ(ξ_q) Â_q[c][s][d][u] ∂̂ᵤN_b(ξ_q) with the tangent pulled back to the reference cell,
        // Â_q[c][s][d][u] = Σ_kl J⁻¹[s][k] 𝔸_q[c][k][d][l] J⁻¹[u][l] dΩ.  Basis and Gauss rule are tensor products — node a ↔ (a₀,a₁,a₂), point
        // q ↔ (q₀,q₁,q₂), ∂̂ₛNₐ(ξ_q) = Π_dim ψ(dim == s)_{a_dim}(q_dim), ψ(false) = φ, ψ(true) = φ′ — so the sum over q is three one-dimensional
        // contractions.  After direction 1 only "s is 2 or not" (μ) still matters, so the nine (s, u) pairs collapse to four (μ, ν):
        //   stage 1  Z1[s][d][u][q₁][q₂][a₀][b₀]       = Σ_q₀ ψ(s==0)_{a₀}(q₀) ψ(u==0)_{b₀}(q₀) Â_q[c][s][d][u]
        //   stage 2  Z2[d][μ][ν][a₀][b₀][a₁][b₁][q₂]   = Σ_{s∈μ} Σ_{u∈ν} Σ_q₁ ψ(s==1)_{a₁}(q₁) ψ(u==1)_{b₁}(q₁) Z1
        //   stage 3  Kₑ[(a,c)][(b,d)]                  = Σ_μν Σ_q₂ ψ(μ)_{a₂}(q₂) ψ(ν)_{b₂}(q₂) Z2
        // per row component c: 243 lane-tasks (one per thread) for stage 1 — 36 multiply-adds out of 3 LDS reads, 9 writes — and 243 for stages 2 + 3
        // together, in registers — 81 + 90 multiply-adds out of 81 reads (no Z2 in LDS), the nine entries stored straight to Kₑ: ≈ 1.5·10⁵
        // multiply-adds per cell instead of the 1.2·10⁶ of the dense 81 × 27 × 81 products, on the vector ALUs, 53 KB of LDS (three workgroups per
        // CU), no symmetry assumed (so the rate-coupled, non-symmetric tangent runs here too).  Same sums as elements.jl:211-223 in another order.
        static_assert(T == 256 && NB == 27 && NQ == 27, "sum-factorised contraction: triquadratic field, 3×3×3 Gauss rule");
        // stage 0: 𝔸·dΩ → Â, in place, one lane per (point, c, d); the lanes d = 0 also pull the stress back, P̂[c][s] = Σ_k J⁻¹[s][k] P[c][k]·dΩ
        if (tid < NQ * 9) {
            const int q = tid / 9, cd = tid - 9 * q, c = cd / 3, d = cd - 3 * c;
            const double *ji = s_Ji[q];
            if (NEED_R && d == 0) {
                double *pp = s_P[q] + 3 * c;
                const double p0 = pp[0], p1 = pp[1], p2 = pp[2];
#pragma unroll
                for (int s_ = 0; s_ < 3; ++s_) pp[s_] = ji[3 * s_] * p0 + ji[3 * s_ + 1] * p1 + ji[3 * s_ + 2] * p2;
            }
            double *Aq = s_A[q];
            double a9[3][3], t9[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int l = 0; l < 3; ++l) a9[k][l] = Aq[9 * (3 * c + k) + 3 * d + l];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int u = 0; u < 3; ++u) t9[k][u] = a9[k][0] * ji[3 * u] + a9[k][1] * ji[3 * u + 1] + a9[k][2] * ji[3 * u + 2];
#pragma unroll
            for (int s_ = 0; s_ < 3; ++s_)
#pragma unroll
                for (int u = 0; u < 3; ++u) Aq[9 * (3 * c + s_) + 3 * d + u] = ji[3 * s_] * t9[0][u] + ji[3 * s_ + 1] * t9[1][u] + ji[3 * s_ + 2] * t9[2][u];
        }
        lds_barrier(); // LDS traffic only: the stores of the previous rows stay in flight
        TB_MS(5);
        double *Z1 = &s_G[0][0][0];
        auto PH = [](int i, int q) constexpr { return quad1d(i, G3::x(q)); };
        auto DP = [](int i, int q) constexpr { return dquad1d(i, G3::x(q)); };
        if constexpr (NEED_R) racc = residual_refgrad();
        // task of stages 2 + 3 (fixed for the three row components): lanes of a wave share (a₀, a₁) where they can — their stores then fall into the
        // same rows of Kₑ — and the nine lanes (a₁, b₁) of one (d, a₀, b₀) read the same Z1 words (LDS broadcast)
        int t23 = tid < 243 ? tid : 0;
        const int tb1 = t23 % 3; t23 /= 3;
        const int tb0 = t23 % 3; t23 /= 3;
        const int td = t23 % 3; t23 /= 3;
        const int ta1 = t23 % 3;
        const int ta0 = t23 / 3;
        double c2[2][2][3]; // ψ(s==1)_{a₁}(q₁) · ψ(u==1)_{b₁}(q₁)
#pragma unroll
        for (int q1 = 0; q1 < 3; ++q1) {
            const double pa = ta1 == 0 ? PH(0, q1) : ta1 == 1 ? PH(1, q1) : PH(2, q1), da = ta1 == 0 ? DP(0, q1) : ta1 == 1 ? DP(1, q1) : DP(2, q1);
            const double pb = tb1 == 0 ? PH(0, q1) : tb1 == 1 ? PH(1, q1) : PH(2, q1), db = tb1 == 0 ? DP(0, q1) : tb1 == 1 ? DP(1, q1) : DP(2, q1);
            c2[0][0][q1] = pa * pb; c2[0][1][q1] = pa * db; c2[1][0][q1] = da * pb; c2[1][1][q1] = da * db;
        }
        int rowa[3], colb[3]; // Ferrite nodes of (a₀, a₁, ·) and (b₀, b₁, ·)
#pragma unroll
        for (int k = 0; k < 3; ++k) { rowa[k] = s_node[ta0 + 3 * ta1 + 9 * k]; colb[k] = s_node[tb0 + 3 * tb1 + 9 * k]; }
        TB_MS(6);
        for (int c = 0; c < 3; ++c) {
            if (tid < 243) { // stage 1: task (s, d, u, q₁, q₂)
                int t = tid;
                const int q2 = t % 3; t /= 3;
                const int q1 = t % 3; t /= 3;
                const int u = t % 3; t /= 3;
                const int d = t % 3;
                const int s_ = t / 3;
                double in[3], tb0_[3][3];
#pragma unroll
                for (int q0 = 0; q0 < 3; ++q0) in[q0] = s_A[q0 + 3 * q1 + 9 * q2][9 * (3 * c + s_) + 3 * d + u];
#pragma unroll
                for (int b0 = 0; b0 < 3; ++b0)
#pragma unroll
                    for (int q0 = 0; q0 < 3; ++q0) tb0_[b0][q0] = (u == 0 ? DP(b0, q0) : PH(b0, q0)) * in[q0];
#pragma unroll
                for (int a0 = 0; a0 < 3; ++a0)
#pragma unroll
                    for (int b0 = 0; b0 < 3; ++b0) {
                        double v = 0.0;
#pragma unroll
                        for (int q0 = 0; q0 < 3; ++q0) v += (s_ == 0 ? DP(a0, q0) : PH(a0, q0)) * tb0_[b0][q0];
                        Z1[9 * tid + 3 * a0 + b0] = v;
                    }
            }
            lds_barrier();
            TB_MS(7 + 2 * c);
            if (tid < 243) { // stages 2 + 3 in registers: 81 LDS reads, nine entries (a₂, b₂) of row component c out
                double z[2][2][3];
#pragma unroll
                for (int e = 0; e < 12; ++e) (&z[0][0][0])[e] = 0.0;
#pragma unroll
                for (int s_ = 0; s_ < 3; ++s_)
#pragma unroll
                    for (int u = 0; u < 3; ++u)
#pragma unroll
                        for (int q1 = 0; q1 < 3; ++q1) {
                            const double cf = c2[s_ == 1][u == 1][q1];
                            const double *zp = Z1 + 9 * ((((s_ * 3 + td) * 3 + u) * 3 + q1) * 3) + 3 * ta0 + tb0;
#pragma unroll
                            for (int q2 = 0; q2 < 3; ++q2) z[s_ == 2][u == 2][q2] += cf * zp[9 * q2];
                        }
                double w[2][3][3]; // w[μ][b₂][q₂] = Σ_ν ψ(ν)_{b₂}(q₂) z[μ][ν][q₂]
#pragma unroll
                for (int mu = 0; mu < 2; ++mu)
#pragma unroll
                    for (int b2 = 0; b2 < 3; ++b2)
#pragma unroll
                        for (int q2 = 0; q2 < 3; ++q2) w[mu][b2][q2] = PH(b2, q2) * z[mu][0][q2] + DP(b2, q2) * z[mu][1][q2];
#pragma unroll
                for (int a2 = 0; a2 < 3; ++a2)
#pragma unroll
                    for (int b2 = 0; b2 < 3; ++b2) {
                        double v = 0.0;
#pragma unroll
                        for (int q2 = 0; q2 < 3; ++q2) v += PH(a2, q2) * w[0][b2][q2] + DP(a2, q2) * w[1][b2][q2];
                        // assemble!(assembler, dofs, Kₑ): entry ((a, c), (b, d))
                        if (atomic == 2) ke[((int64_t)cell * ND + 3 * (ta0 + 3 * ta1 + 9 * a2) + c) * ND + 27 * b2 + (tid < 243 ? tid : 0) % 27] = v; // tensor-order layout (tb_mech_common.hpp)
                        else {
                            const int64_t k = rowptr[s_dof[3 * rowa[a2]] + c] + blockpos[cell * (NB * NB) + rowa[a2] * NB + colb[b2]] + td;
                            if (atomic) unsafeAtomicAdd(nz + k, v); else nz[k] += v;
                        }
                    }
            }
            lds_barrier(); // Z1 is rewritten by the next component's stage 1
            TB_MS(8 + 2 * c);
        }
    } else if constexpr (REFGRAD && !NEED_K) {
        // residual only, reference-gradient path: pull the stress back (one lane per (point, c)), then contract with the reference gradients
        if (tid < NQ * 3) {
            const int q = tid / 3, c = tid - 3 * q;
            const double *ji = s_Ji[q];
            double *pp = s_P[q] + 3 * c;
            const double p0 = pp[0], p1 = pp[1], p2 = pp[2];
#pragma unroll
            for (int s_ = 0; s_ < 3; ++s_) pp[s_] = ji[3 * s_] * p0 + ji[3 * s_ + 1] * p1 + ji[3 * s_ + 2] * p2;
        }
        __syncthreads();
        racc = residual_refgrad();
    } else {
    // B: sweep the points
    const int a_own = tid / NG, bg = tid % NG;
    const bool pair_thread = tid < NB * NG;
    double Kacc[NEED_K ? PB : 1][9];
#pragma unroll
    for (int pb = 0; pb < (NEED_K ? PB : 1); ++pb)
#pragma unroll
        for (int e = 0; e < 9; ++e) Kacc[pb][e] = 0.0;
    auto stage_T = [&](int q, int buf) {
        for (int idx = tid; idx < NB * 27; idx += T) {
            const int a = idx / 27, e = idx % 27, c = e / 9, dl = e % 9; // T[a][c][d][l], dl = 3d + l
            const double *g = s_G[q][a];
            s_T[buf][a][e] = g[0] * s_A[q][9 * (3 * c + 0) + dl] + g[1] * s_A[q][9 * (3 * c + 1) + dl] + g[2] * s_A[q][9 * (3 * c + 2) + dl];
        }
    };
    if constexpr (NEED_K) { stage_T(0, 0); __syncthreads(); }
    for (int q = 0; q < NQ; ++q) {
        if constexpr (NEED_K) {
            if (q + 1 < NQ) stage_T(q + 1, (q + 1) & 1);
            if (pair_thread) {
                double Ta[27];
#pragma unroll
                for (int e = 0; e < 27; ++e) Ta[e] = s_T[q & 1][a_own][e];
#pragma unroll
                for (int pb = 0; pb < PB; ++pb) {
                    const double *gb = s_G[q][bg * PB + pb];
                    const double g0 = gb[0], g1 = gb[1], g2 = gb[2];
#pragma unroll
                    for (int cd = 0; cd < 9; ++cd) Kacc[pb][cd] += Ta[3 * cd] * g0 + Ta[3 * cd + 1] * g1 + Ta[3 * cd + 2] * g2;
                }
            }
        }
        if constexpr (NEED_R) {
            if (tid < ND) {
                const double *g = s_G[q][tid / 3];
                const double *p = s_P[q] + 3 * (tid % 3);
                racc += g[0] * p[0] + g[1] * p[1] + g[2] * p[2];
            }
        }
        if constexpr (NEED_K) __syncthreads();
    }

    // C: assemble!(assembler, dofs, Kₑ, rₑ).  The 3×3 node-pair blocks are re-dealt through LDS one component row c at a
    // time so that three consecutive lanes write the three consecutive columns (d = 0,1,2) of a block row: a
    // wave-instruction then touches 21 24-byte segments instead of 63 scattered doubles (3× fewer memory-side requests).
    if constexpr (NEED_K) {
        double *kbuf = &s_A[0][0]; // 𝔸 is dead after the sweep; NB·NB·3 ≤ NQ·81 doubles
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            __syncthreads();
            if (pair_thread) {
#pragma unroll
                for (int pb = 0; pb < PB; ++pb)
#pragma unroll
                    for (int d = 0; d < 3; ++d) kbuf[(a_own * NB + bg * PB + pb) * 3 + d] = Kacc[pb][3 * c + d];
            }
            __syncthreads();
            if (atomic == 2) { // element assembly: Kₑ rows leave as contiguous ND-long runs
                for (int idx = tid; idx < NB * NB * 3; idx += T) {
                    const int a = idx / ND, j = idx % ND;
                    ke[((int64_t)cell * ND + 3 * a + c) * ND + j] = kbuf[idx];
                }
            } else {
                for (int idx = tid; idx < NB * NB * 3; idx += T) {
                    const int d = idx % 3, ab = idx / 3, a = ab / NB;
                    const int64_t k = rowptr[s_dof[3 * a] + c] + blockpos[cell * (NB * NB) + ab] + d;
                    if (atomic) unsafeAtomicAdd(nz + k, kbuf[idx]); else nz[k] += kbuf[idx];
                }
            }
        }
    }
    }
    if constexpr (NEED_R) {
        if (tid < ND) {
            if (atomic == 2) re[cell * ND + tid] = racc;
            else if (atomic) unsafeAtomicAdd(r + s_dof[tid], racc);
            else r[s_dof[tid]] += racc;
        }
    }
#ifdef TB_ABLATION
    if (m.prof) { TB_MS(13); __builtin_amdgcn_s_waitcnt(0); TB_MS(14); }
#endif
#undef TB_MS
}


// ------------------------------------------------------------------------------------------------ host side
HOParams make_params(const tb_form *f)
{
    HOParams p{};
    const double *q = f->mat.p;
    p.a = q[0]; p.b = q[1]; p.af = q[2]; p.bf = q[3]; p.as = q[4]; p.bs = q[5]; p.afs = q[6]; p.bfs = q[7]; p.beta = q[8];
    for (int i = 0; i < 3; ++i) { p.f[i] = f->mat.f[i]; p.s[i] = f->mat.s[i]; p.n[i] = f->mat.n[i]; }
    p.Ta = f->cond_model ? 0.0 : f->act_tension; // condensed: the per-point (a, b) replace the uniform tension
    p.Tb = 0.0;
    return p;
}

static bool material_is_fast_path(const tb_material &mat) { return mat.kind == TB_MATERIAL_HOLZAPFEL_OGDEN_2009 && mat.reserved == PEN_SIMPLE; }
bool form_is_fast_path(const tb_form *f) { return material_is_fast_path(f->mat) && f->hill == 0 && !f->prestressed; }

EnergyParams make_energy_params(const tb_form *f)
{
    EnergyParams e{};
    e.energy = f->mat.kind; e.penalty = f->mat.reserved;
    for (int i = 0; i < 9; ++i) e.p[i] = f->mat.p[i];
    for (int i = 0; i < 3; ++i) e.u[i] = f->mat.p[10 + i];
    e.Ta = f->cond_model ? 0.0 : f->act_tension;
    e.hill = f->hill; e.act_energy = f->act_energy; e.act_penalty = f->act_penalty; e.adg = f->adg; e.sarc = f->sarc;
    for (int i = 0; i < 9; ++i) e.ap[i] = f->act_p[i];
    for (int i = 0; i < 3; ++i) e.au[i] = f->act_p[9 + i];
    e.kappa = f->hill_kappa; e.sp[0] = f->sarc_p[0]; e.sp[1] = f->sarc_p[1];
    e.prestressed = f->prestressed;
    for (int i = 0; i < 9; ++i) e.G[i] = f->prestress_G[i];
    return e;
}

int host_material_eval(const tb_material *mat, const double *F9, double *psi, double *P, double *A)
{
    tb_form tmpf;
    tmpf.mat = *mat;
    return host_material_eval_form(&tmpf, F9, psi, P, A);
}

int host_material_eval_form(tb_form *form, const double *F9, double *psi, double *P, double *A)
{
    const tb_material *mat = &form->mat;
    form->act_tension = mat->p[9];
    if (!form_is_fast_path(form)) { // any energy of tb_energy.hpp: the same hyper-dual evaluation the kernels run, on the host
        const EnergyParams e = make_energy_params(form);
        const double f0[3] = {mat->f[0], mat->f[1], mat->f[2]}, s0[3] = {mat->s[0], mat->s[1], mat->s[2]}, n0[3] = {mat->n[0], mat->n[1], mat->n[2]};
        for (int pr = 0; pr < 45; ++pr) {
            int mm, nn;
            pair_components(pr, mm, nn);
            const HD r = energy_pair(e, F9, mm, nn, f0, s0, n0, e.Ta);
            if (psi) *psi = r.v;
            if (P && mm == nn) P[mm] = r.a;
            if (A) { A[9 * mm + nn] = r.ab; A[9 * nn + mm] = r.ab; }
        }
        return TB_OK;
    }
    const HOParams p = make_params(form);
    double F[3][3], Pl[9], Al[81];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) F[i][j] = F9[3 * i + j];
    // evaluated through the same split routines the kernels use (ho_common + ho_row)
    double C[HOC_SIZE];
    ho_common(p, F, C);
    for (int ij = 0; ij < 9; ++ij) ho_row<true>(p, C, F9, ij / 3, ij % 3, 1.0, Pl[ij], Al + 9 * ij);
    const double v = C[HOC_PSI];
    if (psi) *psi = v;
    if (P) for (int i = 0; i < 9; ++i) P[i] = Pl[i];
    if (A) for (int i = 0; i < 81; ++i) A[i] = Al[i];
    return TB_OK;
}


int ensure_blockpos(tb_pattern *p)
{
    if (p->d_blockpos) return TB_OK;
    tb_mesh *m = p->mesh;
    const int64_t n = m->n_cells * m->nb * m->nb;
    TB_HIP(hipMalloc((void **)&p->d_blockpos, sizeof(uint16_t) * n));
    hipLaunchKernelGGL(k_build_blockpos, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->dev->stream, m->d_cell_dofs, m->n_cells, m->nb,
                       p->d_rowptr, p->d_colidx, p->d_blockpos, m->dev->d_status);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

// ---- dispatch: one assembly call = the arguments below, handed to one of the three strategies
struct MechCall {
    tb_form *f;
    tb_pattern *p; // NULL when only the residual is asked for
    const double *d_u;
    double *d_nz, *d_r;
    MechMesh mm;
    HOParams hp;
    EnergyParams ep;
};

// residual-only kernel of the triquadratic field: reference-gradient path, no block of mapped gradients
template <class FE, bool NEED_K, bool NEED_R> constexpr bool refgrad_r = !NEED_K && NEED_R && FE::NB == 27 && FE::NQ == 27 && FE::THREADS == 256;

// cells list[0..n), or [cell0, cell0 + n) without a list, through k_hyperelastic
template <class FE, bool NEED_K, bool NEED_R, bool AD>
static int launch_cells(const MechCall &c, const int32_t *list, int64_t cell0, int64_t n, int atomic, double *kebuf = nullptr, double *rebuf = nullptr)
{
    if (!n) return TB_OK;
    constexpr size_t dyn_lds = sizeof(double) * ((NEED_K ? FE::NQ : 1) * 81 + (refgrad_r<FE, NEED_K, NEED_R> ? 0 : FE::NQ * FE::NB * 3)); // 𝔸·dΩ + mapped gradients (s_AG)
    tb_device *dev = c.f->mesh->dev;
    MechMesh mm = c.mm;
    mm.cell0 = cell0;
    auto kern = k_hyperelastic<FE, NEED_K, NEED_R, AD>;
    TB_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds));
    hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(FE::THREADS), dyn_lds, dev->stream, mm, c.hp, c.ep, list, c.d_u, c.d_nz, c.d_r,
                       c.p ? c.p->d_rowptr : nullptr, c.p ? c.p->d_blockpos : nullptr, atomic, kebuf, rebuf, dev->d_status);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

#ifdef TB_ABLATION
// TB_PROF_STAMPS (profiling build): 16 phase time stamps of every 256th workgroup of the fused tangent kernel
static int prof_stamps_begin(tb_mesh *m, MechMesh &mm)
{
    static long long *d_mprof = nullptr;
    static size_t have = 0;
    const size_t need = (size_t)((m->n_cells >> 8) + 1) * 16 * sizeof(long long);
    if (!getenv("TB_PROF_STAMPS")) return TB_OK;
    if (d_mprof && have < need) { (void)hipFree(d_mprof); d_mprof = nullptr; }
    if (!d_mprof) { TB_HIP(hipMalloc((void **)&d_mprof, need)); have = need; }
    TB_HIP(hipMemsetAsync(d_mprof, 0, need, m->dev->stream));
    mm.prof = d_mprof;
    return TB_OK;
}

// average phase durations of the sampled workgroups (µs; wall clock 100 MHz)
static int prof_stamps_report(tb_mesh *m, const MechMesh &mm)
{
    if (!mm.prof) return TB_OK;
    tb_device *dev = m->dev;
    const int nmprof = (int)(m->n_cells >> 8) + 1;
    std::vector<long long> h((size_t)nmprof * 16);
    TB_SYNC_STREAM(dev);
    TB_HIP(hipMemcpy(h.data(), mm.prof, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    double ph[14] = {0};
    int cnt = 0;
    for (int w = 0; w < nmprof; ++w) {
        const long long *a = &h[(size_t)w * 16];
        if (!a[0] || !a[14]) continue;
        for (int k = 0; k < 14; ++k) ph[k] += (double)(a[k + 1] - a[k]) * 0.01;
        ++cnt;
    }
    if (cnt) {
        fprintf(stderr, "[tbhip] mechanics phases (us, n=%d): load %.2f | A1+H %.2f | F+common %.2f | rows %.2f | stage0 %.2f | racc+setup %.2f |", cnt,
                ph[0] / cnt, ph[1] / cnt, ph[2] / cnt, ph[3] / cnt, ph[4] / cnt, ph[5] / cnt);
        for (int c = 0; c < 3; ++c) fprintf(stderr, " c%d: s1 %.2f s23 %.2f |", c, ph[6 + 2 * c] / cnt, ph[7 + 2 * c] / cnt);
        fprintf(stderr, " tail %.2f | drain %.2f\n", ph[12] / cnt, ph[13] / cnt);
    }
    return TB_OK;
}
#endif

// ElementAssemblyStrategy (default for mechanics): Kₑ / rₑ stored per cell, then gathered per node row / per dof (tb_mech_gather.hip)
template <class FE, bool NEED_K, bool NEED_R, bool AD>
static int run_element(const MechCall &c)
{
    tb_form *f = c.f;
    tb_pattern *p = c.p;
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    if (!m->ea) TB_TRY(build_ea_plan(m));
    double *const rebuf = m->ea->d_ea;
    double *kebuf = nullptr;
    if constexpr (NEED_K) {
        TB_TRY(ensure_buffer(p->d_kebuf, p->kebuf_bytes, sizeof(double) * (size_t)m->n_cells * FE::ND * FE::ND, "element-matrix buffer"));
        kebuf = p->d_kebuf;
    }
    // split linearisation (comment above k_mech_points in tb_mech_split.hip): point kernel + contraction kernel instead of the fused one — every
    // symmetric tangent of the triquadratic field (the rate-coupled internal variable adds a non-symmetric term: fused kernel)
    constexpr bool Q2K = NEED_K && FE::NB == 27;
    const bool split = Q2K && !(f->cond_model && f->d_u_prev);
    auto integrate = [&](int64_t c0, int64_t n) -> int { // cells [c0, c0 + n) → stored Kₑ / rₑ
        if constexpr (Q2K) {
            if (split) {
                if (!n) return TB_OK;
                MechMesh mm = c.mm;
                mm.cell0 = c0;
                TB_TRY(launch_mech_points(dev, mm, c.hp, AD ? &c.ep : nullptr, c.d_u, n, p->d_qpbuf));
                return launch_mech_contract(dev, p->d_qpbuf, c0, n, kebuf, NEED_R ? rebuf : nullptr);
            }
        }
        return launch_cells<FE, NEED_K, NEED_R, AD>(c, nullptr, c0, n, 2, kebuf, rebuf);
    };
    // Chunked linearisation (TB_MECH_CHUNKS=n; default 8 for large Q2 meshes, see below; 0 / 1 = one launch): the cells go in n launches, and behind each the
    // staged gather of the node rows that chunk completes runs on a second queue — the HBM-bound gather (46 GB at 80³) beside the LDS / VALU-bound
    // integration of the next chunk.  Same kernels, same sums (a node's cells are still added in cell order): the unchunked result bit for bit.
    // Measured at 80³ (kernel trace, profiles/r04_v2/mechanics_chunk_timeline.txt): the pairs do run side by side, but a CU that holds three
    // integration workgroups has neither LDS (3 × 53 KB) nor registers (3 × 168) left, so every gather workgroup displaces an integration one —
    // 2.55 ms per pair against 1.42 + 1.18 ms alone; the gain is what the pipeline ends and the dispatch gaps cost before: 21.3 → 20.7 ms.
    // default: the triquadratic field from 262 144 cells (below that, and for the first-order field, sixteen small launches cost more than the overlap returns:
    // the 111 616-cell ventricle with a Q1 displacement took 1.26 instead of 1.11 ms)
    const int chunks_default = FE::NB == 27 && m->n_cells >= 262144 ? 8 : 0;
    const int chunks = [&] { const char *e = getenv("TB_MECH_CHUNKS"); return e ? atoi(e) : chunks_default; }(); // read per call: a 20 ms operation
    bool chunked = false;
    if constexpr (NEED_K) {
        if (chunks > 1 && m->n_cells >= 4096 * (int64_t)chunks) {
            TB_TRY(prepare_tangent_gather(p));
            chunked = p->gnodes_state > 0; // the direct gather cannot take a range of nodes before all cells are stored
        }
    }
    if (chunked) TB_TRY(ensure_aux_stream(dev));
    if (split) TB_TRY(ensure_buffer(p->d_qpbuf, p->qpbuf_bytes, sizeof(double) * (size_t)(chunked ? m->n_cells / chunks + 1 : m->n_cells) * QP_REC, "quadrature-point record buffer"));
    if (chunked) {
        int64_t n_done = 0;
        const int rcl = [&]() -> int {
            for (int k = 0; k < chunks; ++k) {
                const int64_t c0 = m->n_cells * k / chunks, c1 = m->n_cells * (k + 1) / chunks;
                TB_TRY(integrate(c0, c1 - c0));
                TB_HIP(hipEventRecord(dev->aux_ev[0], dev->stream));
                TB_HIP(hipStreamWaitEvent(dev->aux_stream, dev->aux_ev[0], 0));
                const int64_t n1 = k + 1 == chunks ? m->n_nodes_field : std::upper_bound(p->h_gn_last.begin(), p->h_gn_last.end(), (int32_t)(c1 - 1)) - p->h_gn_last.begin();
                if (n1 > n_done) {
                    TB_TRY(launch_tangent_gather(p, dev->aux_stream, n_done, n1, kebuf, c.d_nz));
                    n_done = n1;
                }
            }
            return TB_OK;
        }();
        // the second queue is joined on every path, also behind an error half way through the chunks
        TB_HIP(hipEventRecord(dev->aux_ev[1], dev->aux_stream));
        TB_HIP(hipStreamWaitEvent(dev->stream, dev->aux_ev[1], 0));
        if (rcl) return rcl;
    } else {
        TB_TRY(integrate(0, m->n_cells));
    }
#ifdef TB_ABLATION
    TB_TRY(prof_stamps_report(m, c.mm));
#endif
    if constexpr (NEED_K) {
        if (!chunked) {
            TB_TRY(prepare_tangent_gather(p));
            TB_TRY(launch_tangent_gather(p, dev->stream, 0, m->n_nodes_field, kebuf, c.d_nz));
        }
    }
    if (NEED_R) TB_TRY(launch_residual_gather(m, rebuf, c.d_r));
    return TB_OK;
}

// PerColorAssemblyStrategy: one launch per colour, read-modify-write without atomics
template <class FE, bool NEED_K, bool NEED_R, bool AD>
static int run_per_color(const MechCall &c)
{
    tb_form *f = c.f;
    tb_mesh *m = f->mesh;
    const ColorPlan *cp;
    if (f->has_cellset) {
        if (!f->set_colors) TB_TRY(build_color_plan_subset(m, f->h_cellset, f->set_colors));
        cp = f->set_colors.get();
    } else {
        if (!m->colors) TB_TRY(build_color_plan(m));
        cp = m->colors.get();
    }
    for (int k = 0; k < cp->ncolors; ++k) TB_TRY((launch_cells<FE, NEED_K, NEED_R, AD>(c, cp->d_cells + cp->offsets[k], 0, cp->offsets[k + 1] - cp->offsets[k], 0)));
    return TB_OK;
}

// AtomicAssemblyStrategy: all cells (of the subdomain) in one launch
template <class FE, bool NEED_K, bool NEED_R, bool AD>
static int run_atomic(const MechCall &c)
{
    const tb_form *f = c.f;
    return f->has_cellset ? launch_cells<FE, NEED_K, NEED_R, AD>(c, f->d_cellset, 0, f->n_set, 1) : launch_cells<FE, NEED_K, NEED_R, AD>(c, nullptr, 0, f->mesh->n_cells, 1);
}

template <class FE, bool NEED_K, bool NEED_R, bool AD>
static int run(tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    if ((NEED_K && FE::NB == 27) || refgrad_r<FE, NEED_K, NEED_R>) TB_TRY(ensure_cell_xyz(m)); // the kernels on the reference-gradient path read the cell-major coordinates
    MechCall c{f, p, d_u, d_nz, d_r,
               MechMesh{m->d_xyz, m->d_conn, m->d_cell_dofs, f->d_field, f->cond_model ? nullptr : f->d_act_field, f->cond_model ? f->d_qp_act : nullptr, f->d_u_prev ? 5 : 2, m->d_cell_xyz},
               make_params(f), make_energy_params(f)};
#ifdef TB_ABLATION
    if (NEED_K) TB_TRY(prof_stamps_begin(m, c.mm));
#endif
    const bool ea = strategy == TB_STRATEGY_ELEMENT || strategy == TB_STRATEGY_PATCH;
    if (ea && (f->has_cellset || f->accumulate)) {
        set_error("hyperelastic assembly: subdomain / accumulating forms need TB_STRATEGY_PER_COLOR or TB_STRATEGY_ATOMIC (the element strategy writes whole rows)");
        return TB_ERR_UNSUPPORTED;
    }
    if (NEED_K) {
        TB_TRY(ensure_blockpos(p));
        if (!ea && !f->accumulate) TB_HIP(hipMemsetAsync(d_nz, 0, (size_t)p->nnz * sizeof(double), dev->stream));
    }
    if (NEED_R && !ea && !f->accumulate) TB_HIP(hipMemsetAsync(d_r, 0, (size_t)m->ndofs * sizeof(double), dev->stream));
    if (ea) return run_element<FE, NEED_K, NEED_R, AD>(c);
    if (strategy == TB_STRATEGY_PER_COLOR) return run_per_color<FE, NEED_K, NEED_R, AD>(c);
    if (strategy == TB_STRATEGY_ATOMIC) return run_atomic<FE, NEED_K, NEED_R, AD>(c);
    set_error("hyperelastic assembly: unknown strategy %d", strategy);
    return TB_ERR_UNSUPPORTED;
}


// ---- condensed internal variables, stage 0: fibre stretch λ = ‖F f₀‖ and calcium at every quadrature point (the inputs of the local
// problem; solve_local_constraint, materials.jl:1575-1590).  One workgroup per cell, one lane per quadrature point.
template <class FE>
__global__ void __launch_bounds__(64)
k_fiber_stretch(MechMesh m, HOParams mat, const double *__restrict__ act_field, double act_scale, const double *__restrict__ u, double *__restrict__ lam,
                double *__restrict__ ca, const double *__restrict__ u_prev, double inv_dt, double *__restrict__ vel, double *__restrict__ wout, Status *st,
                const int32_t *__restrict__ list)
{
    constexpr int NB = FE::NB, NQ = FE::NQ, ND = FE::ND;
    const MechTables<FE> &tb = g_mech_tables<FE>;
    const int64_t cell = list ? list[blockIdx.x] : blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ double s_ue[ND], s_x[24], s_up[ND];
    for (int i = tid; i < ND; i += 64) { const int32_t d = m.cell_dofs[cell * ND + i]; s_ue[i] = u[d]; s_up[i] = u_prev ? u_prev[d] : 0.0; }
    for (int i = tid; i < 24; i += 64) s_x[i] = m.xyz[3 * (int64_t)m.conn[cell * 8 + i / 3] + i % 3];
    __syncthreads();
    if (tid >= NQ) return;
    const int q = tid;
    double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) J[i][k] += s_x[3 * a + i] * tb.dM[q][a][k];
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, id = 1.0 / det;
    if (!(det > 0.0)) { st->neg_detj = 1; st->cell = cell; }
    const double ji[9] = {c00 * id, (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id, (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id,
                          c01 * id, (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id, (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id,
                          c02 * id, (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id, (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id};
    double f[3] = {mat.f[0], mat.f[1], mat.f[2]};
    if (m.fsn_field) {
        f[0] = f[1] = f[2] = 0.0;
        const double *fc = m.fsn_field + cell * 72;
        for (int a = 0; a < 8; ++a) for (int d = 0; d < 3; ++d) f[d] += tb.M[q][a] * fc[9 * a + d];
        const double nf = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
        for (int d = 0; d < 3; ++d) f[d] /= nf;
    }
    // F f₀ = f₀ + Σₐ uₐ (∇Nₐ · f₀)
    double g[3] = {f[0], f[1], f[2]}, gp[3] = {f[0], f[1], f[2]};
    for (int a = 0; a < NB; ++a) {
        const double d0 = tb.dN[q][a][0], d1 = tb.dN[q][a][1], d2 = tb.dN[q][a][2];
        double gf = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) gf += (d0 * ji[k] + d1 * ji[3 + k] + d2 * ji[6 + k]) * f[k];
#pragma unroll
        for (int c = 0; c < 3; ++c) { g[c] += s_ue[3 * a + c] * gf; gp[c] += s_up[3 * a + c] * gf; }
    }
    double c = act_scale;
    if (act_field) { double s2 = 0.0; for (int a = 0; a < 8; ++a) s2 += tb.M[q][a] * act_field[cell * 8 + a]; c *= s2; }
    const double l = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    lam[cell * NQ + q] = l;
    ca[cell * NQ + q] = c;
    if (u_prev) { // rate-coupled: Ḟ f₀ = (F − F_prev) f₀ / Δt; dλ/dt = ∂λ/∂F : Ḟ = g·ġ/λ; ∂²λ/∂F² : Ḟ = w ⊗ f₀, w = ġ/λ − g (g·ġ)/λ³
        const double gd[3] = {(g[0] - gp[0]) * inv_dt, (g[1] - gp[1]) * inv_dt, (g[2] - gp[2]) * inv_dt};
        const double ggd = g[0] * gd[0] + g[1] * gd[1] + g[2] * gd[2];
        vel[cell * NQ + q] = ggd / l;
#pragma unroll
        for (int d = 0; d < 3; ++d) wout[3 * (cell * NQ + q) + d] = gd[d] / l - g[d] * ggd / (l * l * l);
    }
}

// (a, b, c) of the local solve and w of stage 0 → the (a, b, c·w) records the element kernels read
__global__ void __launch_bounds__(256) k_pack_rate_terms(int64_t n, const double *__restrict__ abc, const double *__restrict__ w, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double c = abc[3 * i + 2];
    out[5 * i] = abc[3 * i]; out[5 * i + 1] = abc[3 * i + 1];
    out[5 * i + 2] = c * w[3 * i]; out[5 * i + 3] = c * w[3 * i + 1]; out[5 * i + 4] = c * w[3 * i + 2];
}

// stage 0 + stage 1 (the pointwise local solves, tb_sarcomere.hip) ahead of the element kernels
template <class FE> static int condensed_prepass(tb_form *f, const double *d_u, bool need_tangent)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    const int64_t npts = m->n_cells * FE::NQ;
    if (!f->d_Q || !f->d_Qknown) { set_error("condensed internal variable: no internal state set (tb_hyperelastic_set_internal_state)"); return TB_ERR_BAD_ARG; }
    if (!(f->cond_dt > 0.0)) { set_error("condensed internal variable: the time step must be positive (got %g)", f->cond_dt); return TB_ERR_BAD_ARG; }
    const bool rate = f->d_u_prev != nullptr;
    // layout: λ | Ca | records (2 or 5 per point; rate-free: at 2·npts) | [rate: velocity | w (3) | (a,b,c) (3)] | status
    const size_t ndbl = rate ? 14 : 4;
    if (!f->d_qp_buf) {
        hipError_t e = hipMalloc((void **)&f->d_qp_buf, sizeof(double) * ndbl * (size_t)npts + sizeof(int32_t) * (size_t)npts);
        if (e != hipSuccess) { set_error("quadrature-point buffers: %s", hipGetErrorString(e)); return TB_ERR_NOMEM; }
        f->d_qp_act = f->d_qp_buf + 2 * npts;
        TB_HIP(hipMemsetAsync(f->d_qp_buf, 0, sizeof(double) * ndbl * (size_t)npts + sizeof(int32_t) * (size_t)npts, dev->stream)); // points outside a subdomain stay zero / TB_LOCAL_SUCCESS
    }
    double *lam = f->d_qp_buf, *ca = f->d_qp_buf + npts;
    double *vel = rate ? f->d_qp_buf + 7 * npts : nullptr, *w = rate ? f->d_qp_buf + 8 * npts : nullptr, *abc = rate ? f->d_qp_buf + 11 * npts : nullptr;
    int32_t *status = (int32_t *)(f->d_qp_buf + (rate ? 14 : 4) * npts);
    const MechMesh mm{m->d_xyz, m->d_conn, m->d_cell_dofs, f->d_field, nullptr, nullptr, 2, nullptr};
    const int64_t ncell_work = f->has_cellset ? f->n_set : m->n_cells;
    if (ncell_work == 0) { f->cond_n_failed = 0; return TB_OK; }
    hipLaunchKernelGGL(k_fiber_stretch<FE>, dim3((unsigned)ncell_work), dim3(64), 0, dev->stream, mm, make_params(f), f->d_act_field, f->act_tension, d_u, lam, ca,
                       f->d_u_prev, 1.0 / f->cond_dt, vel, w, dev->d_status, f->has_cellset ? f->d_cellset : nullptr);
    TB_HIP(hipGetLastError());
    int64_t nfail = 0;
    int rc = launch_sarcomere_implicit(dev, f->cond_params, f->d_Q, f->d_Qknown, npts, lam, vel, ca, 0.0, 0.0, 0.0, f->cond_dt, f->cond_tol, f->cond_max_iters,
                                       f->cond_tmax, nullptr, nullptr, rate ? abc : f->d_qp_act, rate ? 3 : 2, status, &nfail, need_tangent,
                                       f->has_cellset ? f->d_cellset : nullptr, FE::NQ, f->n_set);
    if (rc) return rc;
    if (rate) {
        hipLaunchKernelGGL(k_pack_rate_terms, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, dev->stream, npts, abc, w, f->d_qp_act);
        TB_HIP(hipGetLastError());
    }
    f->cond_n_failed = nfail;
    return rc;
}

int launch_hyperelastic(tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r)
{
    tb_mesh *m = f->mesh;
    if (m->geom_kind == TB_TET4) return launch_hyperelastic_tet(f, p, strategy, d_u, d_nz, d_r);
    int rc = reset_status(m->dev);
    if (rc) return rc;
    const bool q2 = m->field_kind == TB_HEX27;
    if (!q2 && !(m->field_kind == TB_HEX8 && f->qorder == 2)) { set_error("hyperelastic: Q1 field needs quadrature order 2"); return TB_ERR_UNSUPPORTED; }
    if (q2 && f->qorder != 3) { set_error("hyperelastic: Q2 field needs quadrature order 3"); return TB_ERR_UNSUPPORTED; }
    const bool ad = !form_is_fast_path(f);
    if (f->cond_model) {
        rc = q2 ? condensed_prepass<Q2Vec>(f, d_u, d_nz != nullptr) : condensed_prepass<Q1Vec>(f, d_u, d_nz != nullptr);
        if (rc) return rc;
    }
#define TB_RUN(FEV, K, R) (ad ? run<FEV, K, R, true>(f, p, strategy, d_u, d_nz, d_r) : run<FEV, K, R, false>(f, p, strategy, d_u, d_nz, d_r))
    if (d_nz && d_r) rc = q2 ? TB_RUN(Q2Vec, true, true) : TB_RUN(Q1Vec, true, true);
    else if (d_nz) rc = q2 ? TB_RUN(Q2Vec, true, false) : TB_RUN(Q1Vec, true, false);
    else rc = q2 ? TB_RUN(Q2Vec, false, true) : TB_RUN(Q1Vec, false, true);
#undef TB_RUN
    if (rc) return rc;
    return check_status(m->dev);
}

} // namespace tb

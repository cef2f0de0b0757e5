// tb_viscoelastic.hip — quasi-static small-strain viscoelasticity (LinearMaxwellMaterial, src/modeling/solid/materials.jl:1816-2008): residual and
// condensed tangent of a three-component Lagrange field on hexahedra (Q1: 2×2×2 Gauss, Q2: 3×3×3) and tetrahedra (P1: 4-point rule, P2: Keast 8).
//
// Same element integrals as tb_mechanics.hip (src/modeling/solid/elements.jl:177-313) with the stress of tb_maxwell.hpp in the place of P:
//   per quadrature point  ∇u = Σ uₑᵢ ∇δuᵢ,  εᵛ₁ = local backward-Euler step from the accepted εᵛ₀ (solve_local_constraint, materials.jl:1881-1936),
//   σ = E₀ ℂ:ε + E₁ ℂ:(ε − εᵛ₁),   rₑ[i] += ∇δuᵢ ⊡ σ dΩ,   Kₑ[i,j] += (∇δuᵢ ⊡ ∂σ/∂ε) ⊡ ∇δuⱼ dΩ.
// One launch does all of it: the local update, the stress and the tangent are fused — no pre-pass, no per-point scratch.  Every launch (the
// residual-only one too: solve_local_constraint_state_only, :1938-1955) writes εᵛ₁ of the cells it visits into the state array; points of other
// cells are neither read nor written.
//
// The condensed tangent is isotropic and the same at every point (it depends on the parameters and Δt only), so the 3 × 3 block of a node pair is
//   Kₑ[(a,·)][(b,·)] = λ* G_ab + μ* G_abᵀ + μ* tr(G_ab) I,   G_ab = Σ_q dΩ ∇Nₐ ⊗ ∇N_b
// — nine sums per pair instead of the 81-entry 𝔸 of the hyperelastic kernels, and no tangent in LDS.
//
// A cell is worked by a group of lanes inside a 256-thread workgroup (Q1: one wave, 4 cells; Q2: the workgroup; P1: 16 lanes, 16 cells; P2: one wave,
// 4 cells); the idle groups of the last workgroup run the launch's first cell and store nothing.  A lane owns node pairs (a, b); the blocks leave
// through LDS one row component at a time so that a wave writes runs of consecutive doubles.  Scatter modes as k_hyperelastic: 0 plain
// read-modify-write (one colour of the cell conflict graph), 1 hardware atomics, 2 store Kₑ / rₑ for the ordered gather of tb_mech_gather.hip
// (hexahedra; Q2 in the tensor order of tb_mech_common.hpp).  Element descriptors and tables: tb_mech_common.hpp, tb_mech_tet.hpp.
#include <hip/hip_runtime.h>

#include "tb_internal.h"
#include "tb_maxwell.hpp"
#include "tb_mech_common.hpp"
#include "tb_mech_gather.hpp"
#include "tb_mech_tet.hpp"

namespace tb {
using namespace tbk;

namespace {

// KIND: TB_HEX8, TB_HEX27, TB_TET4, TB_TET10 (the field; the geometry is the first-order cell of the family)
template <int KIND> struct VisElem;
template <> struct VisElem<TB_HEX8> { using FE = Q1Vec; static constexpr bool HEX = true; static constexpr int NB = 8, NQ = 8, NV = 8, NG = 8, LPC = 64; };
template <> struct VisElem<TB_HEX27> { using FE = Q2Vec; static constexpr bool HEX = true; static constexpr int NB = 27, NQ = 27, NV = 8, NG = 27, LPC = 256; };
template <> struct VisElem<TB_TET4> { using FE = void; static constexpr bool HEX = false; static constexpr int NB = 4, NQ = 4, NV = 4, NG = 1, LPC = 16; };  // constant gradients
template <> struct VisElem<TB_TET10> { using FE = void; static constexpr bool HEX = false; static constexpr int NB = 10, NQ = 8, NV = 4, NG = 8, LPC = 64; };
constexpr int VIS_THREADS = 256;

struct VisArgs {
    const double *xyz;
    const int32_t *conn;
    const int32_t *cell_dofs;
    const int32_t *list;   // cells of the launch, or NULL: [cell0, cell0 + n)
    int64_t cell0, n;
    const double *u;
    const double *Q0;      // accepted state, 6 × npts, point-fastest
    double *Q1;            // state of this assembly
    int64_t npts;
    double *nz, *r;        // modes 0, 1
    const int64_t *rowptr;
    const uint16_t *blockpos;
    double *ke, *re;       // mode 2
    int mode;
    Status *st;
};

template <int KIND, bool NEED_K>
__global__ void __launch_bounds__(VIS_THREADS)
k_viscoelastic(VisArgs A, MaxwellCoef mc)
{
    using E = VisElem<KIND>;
    constexpr int NB = E::NB, NQ = E::NQ, NV = E::NV, NG = E::NG, LPC = E::LPC, ND = 3 * NB, CPW = VIS_THREADS / LPC;
    constexpr int NPAIR = NB * NB, NPR = (NPAIR + LPC - 1) / LPC;
    static_assert(ND <= LPC && NQ <= LPC && 3 * NV <= LPC, "one lane per element unknown / point / coordinate");
    __shared__ double s_ue[CPW][ND], s_x[CPW][3 * NV], s_geo[CPW][E::HEX ? NQ * 9 : 12], s_dO[CPW][NQ], s_G[CPW][NG][NB][3], s_H[CPW][NQ][9], s_P[CPW][NQ][9];
    __shared__ double s_K[NEED_K ? CPW : 1][NEED_K ? NPAIR * 3 : 1];
    __shared__ int32_t s_dof[CPW][ND];
    __shared__ uint8_t s_node[32];
    const int g = threadIdx.x / LPC, lt = threadIdx.x % LPC;
    const int64_t ci = (int64_t)blockIdx.x * CPW + g;
    const bool valid = ci < A.n;
    const int64_t cell = A.list ? A.list[valid ? ci : 0] : A.cell0 + (valid ? ci : 0);
    const bool need_r = A.mode == 2 ? A.re != nullptr : A.r != nullptr;

    // load_element_unknowns! (elements.jl:125-132) + vertex coordinates
    if (lt < ND) { const int32_t d = A.cell_dofs[cell * ND + lt]; s_dof[g][lt] = d; s_ue[g][lt] = A.u[d]; }
    if (lt < 3 * NV) s_x[g][lt] = A.xyz[3 * (int64_t)A.conn[cell * NV + lt / 3] + lt % 3];
    if constexpr (KIND == TB_HEX27) { if (threadIdx.x < 27) s_node[threadIdx.x] = (uint8_t)g_hex27_node[threadIdx.x]; }
    __syncthreads();

    // geometry: J⁻¹ and dΩ per point (trilinear hexahedron), or once per cell (affine tetrahedron)
    if constexpr (E::HEX) {
        const MechTables<typename E::FE> &tb = g_mech_tables<typename E::FE>;
        if (lt < NQ) {
            const int q = lt;
            double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k) J[i][k] += s_x[g][3 * a + i] * tb.dM[q][a][k];
            const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
            const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, id = 1.0 / det;
            double *o = s_geo[g] + 9 * q;
            o[0] = c00 * id; o[1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id; o[2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
            o[3] = c01 * id; o[4] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id; o[5] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
            o[6] = c02 * id; o[7] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id; o[8] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
            const double dO = det * tb.w[q];
            s_dO[g][q] = dO;
            if (!(dO > 0.0)) { A.st->neg_detj = 1; A.st->cell = cell; }
        }
        __syncthreads();
        // mapped gradients ∇Nₐ = ∂Nₐ/∂ξ · J⁻¹ for every (point, node)
        for (int idx = lt; idx < NQ * NB; idx += LPC) {
            const int q = idx / NB, a = idx - q * NB;
            const double *ji = s_geo[g] + 9 * q;
            const double d0 = tb.dN[q][a][0], d1 = tb.dN[q][a][1], d2 = tb.dN[q][a][2];
#pragma unroll
            for (int k = 0; k < 3; ++k) s_G[g][q][a][k] = d0 * ji[k] + d1 * ji[3 + k] + d2 * ji[6 + k];
        }
    } else {
        if (lt == 0) {
            const double det = tet_geometry(s_x[g], s_geo[g]);
            if (!(det > 0.0)) { A.st->neg_detj = 1; A.st->cell = cell; }
            s_dO[g][0] = det;
        }
        __syncthreads();
        const double det = s_dO[g][0];
        for (int idx = lt; idx < NG * NB; idx += LPC) {
            const int q = idx / NB, a = idx - q * NB;
            const double lam[4] = {tet_lambda<NB>(NQ, q, 0), tet_lambda<NB>(NQ, q, 1), tet_lambda<NB>(NQ, q, 2), tet_lambda<NB>(NQ, q, 3)};
            double gr[3];
            tet_grad<NB>(a, lam, s_geo[g], gr);
#pragma unroll
            for (int k = 0; k < 3; ++k) s_G[g][q][a][k] = gr[k];
        }
        __syncthreads(); // (slot 0 of s_dO was read by every lane above)
        if (lt < NQ) s_dO[g][lt] = det * tet_weight<NB>(NQ, lt);
    }
    __syncthreads();

    // ∇u = Σₐ uₐ ⊗ ∇Nₐ, one lane per (point, c, k)
    for (int t = lt; t < NQ * 9; t += LPC) {
        const int q = t / 9, ck = t - 9 * q, c = ck / 3, k = ck - 3 * c;
        double v = 0.0;
        for (int a = 0; a < NB; ++a) v += s_ue[g][3 * a + c] * s_G[g][NG == 1 ? 0 : q][a][k];
        s_H[g][q][ck] = v;
    }
    __syncthreads();

    // local problem and stress, one lane per point: εᵛ₁ from the accepted state, σ·dΩ
    if (lt < NQ) {
        const int q = lt;
        const int64_t pt = cell * NQ + q;
        double q0[6], q1[6], sig[9];
#pragma unroll
        for (int s = 0; s < 6; ++s) q0[s] = A.Q0[s * A.npts + pt];
        maxwell_point(mc, s_H[g][q], q0, q1, sig);
        if (valid) {
#pragma unroll
            for (int s = 0; s < 6; ++s) A.Q1[s * A.npts + pt] = q1[s];
        }
        const double dO = s_dO[g][q];
#pragma unroll
        for (int e = 0; e < 9; ++e) s_P[g][q][e] = sig[e] * dO;
    }
    __syncthreads();

    // rₑ[(a,c)] = Σ_q ∇Nₐ · σ_q[c][·] dΩ
    if (need_r && lt < ND) {
        const int a = lt / 3, c = lt - 3 * a;
        double acc = 0.0;
        for (int q = 0; q < NQ; ++q) {
            const double *gr = s_G[g][NG == 1 ? 0 : q][a], *p = s_P[g][q] + 3 * c;
            acc += gr[0] * p[0] + gr[1] * p[1] + gr[2] * p[2];
        }
        if (valid) {
            if (A.mode == 2) A.re[cell * ND + lt] = acc;
            else if (A.mode) unsafeAtomicAdd(A.r + s_dof[g][lt], acc);
            else A.r[s_dof[g][lt]] += acc;
        }
    }

    if constexpr (NEED_K) {
        // G_ab of the lane's node pairs
        double G[NPR][9];
        int oa[NPR], ob[NPR]; // offsets of ∇Nₐ, ∇N_b inside a point's gradient block
#pragma unroll
        for (int i = 0; i < NPR; ++i) {
            const int pr = lt + i * LPC, prc = pr < NPAIR ? pr : 0, a = prc / NB, b = prc - a * NB;
            oa[i] = 3 * a; ob[i] = 3 * b;
#pragma unroll
            for (int e = 0; e < 9; ++e) G[i][e] = 0.0;
        }
        // (the point loop stays rolled: unrolled, its loads are hoisted and the accumulators spill)
#pragma unroll 1
        for (int q = 0; q < NQ; ++q) {
            const double *gq = &s_G[g][NG == 1 ? 0 : q][0][0];
            const double dO = s_dO[g][q];
#pragma unroll
            for (int i = 0; i < NPR; ++i) {
                const double *ga = gq + oa[i], *gb = gq + ob[i];
                const double a0 = ga[0] * dO, a1 = ga[1] * dO, a2 = ga[2] * dO, b0 = gb[0], b1 = gb[1], b2 = gb[2];
                G[i][0] += a0 * b0; G[i][1] += a0 * b1; G[i][2] += a0 * b2;
                G[i][3] += a1 * b0; G[i][4] += a1 * b1; G[i][5] += a1 * b2;
                G[i][6] += a2 * b0; G[i][7] += a2 * b1; G[i][8] += a2 * b2;
            }
        }
        // assemble!(assembler, dofs, Kₑ): row component c of every block through LDS, then out in runs of consecutive doubles
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPR; ++i) {
                const int pr = lt + i * LPC;
                if (pr < NPAIR) {
                    const double mt = mc.mu_s * (G[i][0] + G[i][4] + G[i][8]);
#pragma unroll
                    for (int d = 0; d < 3; ++d) s_K[g][3 * pr + d] = mc.lam_s * G[i][3 * c + d] + mc.mu_s * G[i][3 * d + c] + (c == d ? mt : 0.0);
                }
            }
            __syncthreads();
            if (!valid) {
                // idle group of the last workgroup: nothing leaves (the barriers above are reached by every lane)
            } else if (A.mode == 2) {
                if constexpr (KIND == TB_HEX27) { // tensor-order layout of the stored element matrices: row 3·tix(a) + c, column cb(b) + 9d
                    for (int idx = lt; idx < NB * ND; idx += LPC) {
                        const int ta = idx / ND, j = idx - ta * ND, b2 = j / 27, d = (j % 27) / 9, b0 = (j % 9) / 3, b1 = j % 3;
                        const int a = s_node[ta], b = s_node[b0 + 3 * b1 + 9 * b2];
                        A.ke[((int64_t)cell * ND + 3 * ta + c) * ND + j] = s_K[g][(a * NB + b) * 3 + d];
                    }
                } else {
                    for (int idx = lt; idx < NB * ND; idx += LPC) {
                        const int a = idx / ND, j = idx - a * ND;
                        A.ke[((int64_t)cell * ND + 3 * a + c) * ND + j] = s_K[g][idx];
                    }
                }
            } else {
                for (int idx = lt; idx < NPAIR * 3; idx += LPC) {
                    const int ab = idx / 3, d = idx - 3 * ab, a = ab / NB;
                    const int64_t k = A.rowptr[s_dof[g][3 * a] + c] + A.blockpos[cell * NPAIR + ab] + d;
                    if (A.mode) unsafeAtomicAdd(A.nz + k, s_K[g][idx]); else A.nz[k] += s_K[g][idx];
                }
            }
        }
    }
}

template <int KIND>
int run_viscoelastic(tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r)
{
    using E = VisElem<KIND>;
    constexpr int ND = 3 * E::NB, CPW = VIS_THREADS / E::LPC;
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    const bool need_k = d_nz != nullptr;
    const bool ea = E::HEX && (strategy == TB_STRATEGY_ELEMENT || strategy == TB_STRATEGY_PATCH); // store Kₑ / rₑ, ordered gather
    if ((strategy == TB_STRATEGY_ELEMENT || strategy == TB_STRATEGY_PATCH) && (f->has_cellset || f->accumulate)) {
        set_error("hyperelastic assembly: subdomain / accumulating forms need TB_STRATEGY_PER_COLOR or TB_STRATEGY_ATOMIC (the element strategy writes whole rows)");
        return TB_ERR_UNSUPPORTED;
    }
    // tetrahedra (tb_mech_tet.hpp): ELEMENT and PER_COLOR are the coloured ordered sweep; PATCH takes the scatter measured faster (DESIGN.md §4.4g, 24³
    // lattice): atomics for both fields — P1 0.26 against 0.43 ms, P2 0.98 against 1.12 ms (270 atomics per cell here, not the 900 of the general tangent)
    const bool coloured = !ea && (strategy == TB_STRATEGY_PER_COLOR || strategy == TB_STRATEGY_ELEMENT);
    if (!ea && !coloured && strategy != TB_STRATEGY_ATOMIC && strategy != TB_STRATEGY_PATCH) {
        set_error("hyperelastic assembly: unknown strategy %d", strategy);
        return TB_ERR_UNSUPPORTED;
    }
    if (need_k) {
        TB_TRY(ensure_blockpos(p));
        if (!ea && !f->accumulate) TB_HIP(hipMemsetAsync(d_nz, 0, (size_t)p->nnz * sizeof(double), dev->stream));
    }
    if (d_r && !ea && !f->accumulate) TB_HIP(hipMemsetAsync(d_r, 0, (size_t)m->ndofs * sizeof(double), dev->stream));
    VisArgs A{};
    A.xyz = m->d_xyz; A.conn = m->d_conn; A.cell_dofs = m->d_cell_dofs;
    A.u = d_u; A.Q0 = f->d_Qknown; A.Q1 = f->d_Q; A.npts = m->n_cells * E::NQ;
    A.nz = d_nz; A.r = d_r;
    A.rowptr = p ? p->d_rowptr : nullptr; A.blockpos = p ? p->d_blockpos : nullptr;
    A.st = dev->d_status;
    const MaxwellCoef mc = maxwell_coef(f->vis_p, f->cond_dt);
    auto go = [&](const int32_t *list, int64_t cell0, int64_t n, int mode) -> int {
        if (!n) return TB_OK;
        VisArgs a = A;
        a.list = list; a.cell0 = cell0; a.n = n; a.mode = mode;
        const dim3 grid((unsigned)((n + CPW - 1) / CPW));
        if (need_k) hipLaunchKernelGGL((k_viscoelastic<KIND, true>), grid, dim3(VIS_THREADS), 0, dev->stream, a, mc);
        else hipLaunchKernelGGL((k_viscoelastic<KIND, false>), grid, dim3(VIS_THREADS), 0, dev->stream, a, mc);
        TB_HIP(hipGetLastError());
        return TB_OK;
    };
    set_last_kernel("k_viscoelastic<%s,%s>(%s)", KIND == TB_HEX8 ? "Q1" : KIND == TB_HEX27 ? "Q2" : KIND == TB_TET4 ? "P1" : "P2", need_k ? (d_r ? "K+r" : "K") : "r",
                    ea ? "element" : coloured ? "colours" : "atomic");
    if (ea) {
        if (!m->ea) TB_TRY(build_ea_plan(m));
        if (need_k) {
            TB_TRY(ensure_buffer(p->d_kebuf, p->kebuf_bytes, sizeof(double) * (size_t)m->n_cells * ND * ND, "element-matrix buffer"));
            A.ke = p->d_kebuf;
        }
        A.re = d_r ? m->ea->d_ea : nullptr;
        TB_TRY(go(nullptr, 0, m->n_cells, 2));
        if (need_k) {
            TB_TRY(prepare_tangent_gather(p));
            TB_TRY(launch_tangent_gather(p, dev->stream, 0, m->n_nodes_field, p->d_kebuf, d_nz));
        }
        if (d_r) TB_TRY(launch_residual_gather(m, m->ea->d_ea, d_r));
        return TB_OK;
    }
    if (coloured) {
        const ColorPlan *cp;
        if (f->has_cellset) {
            if (!f->set_colors) TB_TRY(build_color_plan_subset(m, f->h_cellset, f->set_colors));
            cp = f->set_colors.get();
        } else {
            if (!m->colors) TB_TRY(build_color_plan(m));
            cp = m->colors.get();
        }
        for (int k = 0; k < cp->ncolors; ++k) TB_TRY(go(cp->d_cells + cp->offsets[k], 0, cp->offsets[k + 1] - cp->offsets[k], 0));
        return TB_OK;
    }
    return f->has_cellset ? go(f->d_cellset, 0, f->n_set, 1) : go(nullptr, 0, m->n_cells, 1);
}

} // namespace

int launch_viscoelastic(tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r)
{
    tb_mesh *m = f->mesh;
    if (!f->d_Q || !f->d_Qknown) { set_error("condensed internal variable: no internal state set (tb_hyperelastic_set_internal_state)"); return TB_ERR_BAD_ARG; }
    if (!(f->cond_dt > 0.0)) { set_error("condensed internal variable: the time step must be positive (got %g)", f->cond_dt); return TB_ERR_BAD_ARG; }
    TB_TRY(reset_status(m->dev));
    int rc;
    switch (m->field_kind) {
    case TB_HEX8: rc = run_viscoelastic<TB_HEX8>(f, p, strategy, d_u, d_nz, d_r); break;
    case TB_HEX27: rc = run_viscoelastic<TB_HEX27>(f, p, strategy, d_u, d_nz, d_r); break;
    case TB_TET4: rc = run_viscoelastic<TB_TET4>(f, p, strategy, d_u, d_nz, d_r); break;
    case TB_TET10: rc = run_viscoelastic<TB_TET10>(f, p, strategy, d_u, d_nz, d_r); break;
    default: set_error("viscoelastic assembly: field kind %d", m->field_kind); return TB_ERR_UNSUPPORTED;
    }
    if (rc) return rc;
    return check_status(m->dev);
}

int host_maxwell_eval(const double *params, const double *F, const double *Qknown6, double dt, double *Q6, double *P, double *A)
{
    const MaxwellCoef mc = maxwell_coef(params, dt);
    double H[9], q0[6], q1[6], sig[9];
    for (int i = 0; i < 9; ++i) H[i] = F[i] - (i % 4 == 0 ? 1.0 : 0.0);
    for (int s = 0; s < 6; ++s) q0[s] = Qknown6 ? Qknown6[s] : 0.0;
    maxwell_point(mc, H, q0, q1, sig);
    if (Q6) for (int s = 0; s < 6; ++s) Q6[s] = q1[s];
    if (P) for (int i = 0; i < 9; ++i) P[i] = sig[i];
    if (A)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                for (int k = 0; k < 3; ++k)
                    for (int l = 0; l < 3; ++l)
                        A[9 * (3 * i + j) + 3 * k + l] = mc.lam_s * (i == j) * (k == l) + mc.mu_s * ((i == k) * (j == l) + (i == l) * (j == k));
    return TB_OK;
}

} // namespace tb

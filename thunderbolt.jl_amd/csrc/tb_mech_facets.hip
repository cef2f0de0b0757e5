// tb_mech_facets.hip — weak boundary conditions of the hyperelastic problem on hexahedral meshes: facet integrals.
#include <hip/hip_runtime.h>

#include "tb_internal.h"
#include "tb_mech_common.hpp"
#include "tb_facet_geom.hpp"

namespace tb {
using namespace tbk;

// Facet integrals of src/modeling/core/weak_boundary_conditions.jl (RobinBC :102-198, NormalSpringBC :200-300, pressure
// follower load :419-515).  One 64-thread workgroup per (cell, local facet): per facet Gauss point the shape values,
// mapped gradients and the few tensors the integrand needs are parked in LDS, then every thread sums its (i, j) pairs over
// the points and adds the result to the CSR entry / residual entry with one atomic each (surface terms are O(n²) work, the
// volume term O(n³): this kernel is not on the critical path).  FacetValues conventions are Ferrite's (tbhip.h).
// (numbering, Gauss points and the geometry stage: tb_facet_geom.hpp)
template <int NB>
__global__ void __launch_bounds__(64)
k_facets(MechMesh m, const int32_t *__restrict__ facets, int bc, double param, int fq, const double *__restrict__ pfield, const double *__restrict__ u, double *__restrict__ nz,
         double *__restrict__ r, const int64_t *__restrict__ rowptr, const uint16_t *__restrict__ blockpos, Status *st)
{
    constexpr int ND = 3 * NB, MAXQ = 9;
    const int tid = threadIdx.x;
    const int64_t cell = facets[2 * blockIdx.x];
    const int lf = facets[2 * blockIdx.x + 1];
    __shared__ double s_ue[ND], s_x[24], s_N[MAXQ][NB], s_G[MAXQ][NB][3];
    __shared__ double s_q[MAXQ][32]; // per point: dΓ, n₀[3], grad[3] (Robin / spring) or J·cofF·n₀ [3], H[9] / invF[9], J, invFᵀ… (see below)
    __shared__ int32_t s_dof[ND];
    for (int i = tid; i < ND; i += 64) { const int32_t d = m.cell_dofs[cell * ND + i]; s_dof[i] = d; s_ue[i] = u[d]; }
    for (int i = tid; i < 24; i += 64) s_x[i] = m.xyz[3 * (int64_t)m.conn[cell * 8 + i / 3] + i % 3];
    __syncthreads();
    const int nq = fq * fq;
    facet_geometry_stage<NB>(tid, cell, lf, fq, s_x, s_N, s_G, s_q, st); // shape values, mapped gradients, dΓ and n₀ per point
    __syncthreads();
    // field values per point (one thread per point): u_q, F, and the tensors of the integrand
    //   slots: [4..6] g = residual vector density (δuᵢ·g), [7..15] H (Robin / spring: Hessian; pressure: invF), [16] J, [17..19] cofF·n₀,
    //          [20..22] invFᵀ-weighted normal  fin[d] = Σ_r invF[r][d] n₀[r]
    if (tid < nq) {
        const int q = tid;
        double uq[3] = {0, 0, 0}, F[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int a = 0; a < NB; ++a)
            for (int c = 0; c < 3; ++c) {
                uq[c] += s_N[q][a] * s_ue[3 * a + c];
                for (int k = 0; k < 3; ++k) F[c][k] += s_ue[3 * a + c] * s_G[q][a][k];
            }
        const double *n0 = &s_q[q][1];
        double *o = s_q[q];
        if (bc == TB_BC_ROBIN) {
            for (int c = 0; c < 3; ++c) o[4 + c] = 2.0 * param * uq[c];
            for (int e = 0; e < 9; ++e) o[7 + e] = (e % 4 == 0) ? 2.0 * param : 0.0;
        } else if (bc == TB_BC_NORMAL_SPRING) {
            const double un = uq[0] * n0[0] + uq[1] * n0[1] + uq[2] * n0[2];
            for (int c = 0; c < 3; ++c) o[4 + c] = param * un * n0[c];
            for (int c = 0; c < 3; ++c) for (int d = 0; d < 3; ++d) o[7 + 3 * c + d] = param * n0[c] * n0[d];
        } else {
            double pq = param;
            if (bc == TB_BC_PRESSURE_FIELD && pfield) { // evaluate_coefficient(pc, cell, qp, t): nodal data × M_a at the facet point
                double xi[3];
                facet_xi(lf, fq, q, xi);
                double v = 0.0;
                for (int a = 0; a < 8; ++a) { double Ma, dMa[3]; shape_at<8>(a, xi, Ma, dMa); v += Ma * pfield[cell * 8 + a]; }
                pq = param * v;
            }
            const double c00 = F[1][1] * F[2][2] - F[1][2] * F[2][1], c01 = F[1][2] * F[2][0] - F[1][0] * F[2][2], c02 = F[1][0] * F[2][1] - F[1][1] * F[2][0];
            const double Jf = F[0][0] * c00 + F[0][1] * c01 + F[0][2] * c02, id = 1.0 / Jf;
            const double Fi[9] = {c00 * id, (F[0][2] * F[2][1] - F[0][1] * F[2][2]) * id, (F[0][1] * F[1][2] - F[0][2] * F[1][1]) * id,
                                  c01 * id, (F[0][0] * F[2][2] - F[0][2] * F[2][0]) * id, (F[0][2] * F[1][0] - F[0][0] * F[1][2]) * id,
                                  c02 * id, (F[0][1] * F[2][0] - F[0][0] * F[2][1]) * id, (F[0][0] * F[1][1] - F[0][1] * F[1][0]) * id};
            for (int e = 0; e < 9; ++e) o[7 + e] = Fi[e];
            o[16] = bc == TB_BC_BENDING_SPRING ? Jf : pq * Jf;      // pressure: p·J folded here
            double vv[3];
            for (int c = 0; c < 3; ++c) {
                const double cn = Fi[0 + c] * n0[0] + Fi[3 + c] * n0[1] + Fi[6 + c] * n0[2]; // v = F⁻ᵀ n₀
                vv[c] = cn;
                o[17 + c] = cn;
                o[4 + c] = pq * Jf * cn;
            }
            if (bc == TB_BC_BENDING_SPRING) { // w = v − N, z = F⁻¹ w, B = F⁻¹ F⁻ᵀ (slots 20..22, 23..31)
                const double w[3] = {vv[0] - n0[0], vv[1] - n0[1], vv[2] - n0[2]};
                for (int j = 0; j < 3; ++j) o[20 + j] = Fi[3 * j + 0] * w[0] + Fi[3 * j + 1] * w[1] + Fi[3 * j + 2] * w[2];
                for (int j = 0; j < 3; ++j)
                    for (int l = 0; l < 3; ++l) o[23 + 3 * j + l] = Fi[3 * j + 0] * Fi[3 * l + 0] + Fi[3 * j + 1] * Fi[3 * l + 1] + Fi[3 * j + 2] * Fi[3 * l + 2];
            }
        }
    }
    __syncthreads();
    // residual: rₑ[i] += δuᵢ·g dΓ   (bending spring: ∇δuᵢ ⊡ P dΓ with P = −kᵇ v ⊗ z)
    if (r)
        for (int i = tid; i < ND; i += 64) {
            const int a = i / 3, c = i % 3;
            double v = 0.0;
            if (bc == TB_BC_BENDING_SPRING) {
                for (int q = 0; q < nq; ++q) {
                    const double *o = s_q[q], *g = s_G[q][a];
                    v -= param * o[17 + c] * (g[0] * o[20] + g[1] * o[21] + g[2] * o[22]) * o[0];
                }
            } else {
                for (int q = 0; q < nq; ++q) v += s_N[q][a] * s_q[q][4 + c] * s_q[q][0];
            }
            if (v != 0.0) unsafeAtomicAdd(r + s_dof[i], v);
        }
    // tangent
    if (nz)
        for (int ij = tid; ij < ND * ND; ij += 64) {
            const int i = ij / ND, j = ij % ND, a = i / 3, c = i % 3, b = j / 3, d = j % 3;
            double v = 0.0;
            if (bc == TB_BC_ROBIN || bc == TB_BC_NORMAL_SPRING) {
                for (int q = 0; q < nq; ++q) v += s_N[q][a] * s_q[q][7 + 3 * c + d] * s_N[q][b] * s_q[q][0];
            } else if (bc == TB_BC_BENDING_SPRING) {
                // 𝔸[c][k][d][l] = kᵇ [ v_d F⁻¹_lc z_k + v_c (F⁻¹_kd z_l + v_d B_kl) ],  Kₑ += ∇N_a[k] 𝔸 ∇N_b[l] dΓ
                for (int q = 0; q < nq; ++q) {
                    const double *o = s_q[q], *Fi = o + 7, *ga = s_G[q][a], *gb = s_G[q][b], *z = o + 20, *B = o + 23;
                    const double gaz = ga[0] * z[0] + ga[1] * z[1] + ga[2] * z[2], gbz = gb[0] * z[0] + gb[1] * z[1] + gb[2] * z[2];
                    const double gaFd = ga[0] * Fi[0 + d] + ga[1] * Fi[3 + d] + ga[2] * Fi[6 + d];
                    const double gbFc = gb[0] * Fi[0 + c] + gb[1] * Fi[3 + c] + gb[2] * Fi[6 + c];
                    double gaBgb = 0.0;
                    for (int k = 0; k < 3; ++k) gaBgb += ga[k] * (B[3 * k] * gb[0] + B[3 * k + 1] * gb[1] + B[3 * k + 2] * gb[2]);
                    v += param * (o[17 + d] * gbFc * gaz + o[17 + c] * (gaFd * gbz + o[17 + d] * gaBgb)) * o[0];
                }
            } else {
                for (int q = 0; q < nq; ++q) {
                    const double *o = s_q[q], *Fi = o + 7, *g = s_G[q][b];
                    double gF[3];
                    for (int k = 0; k < 3; ++k) gF[k] = g[0] * Fi[0 + k] + g[1] * Fi[3 + k] + g[2] * Fi[6 + k];
                    // δJ·cofF·n₀ + J·δcofF·n₀ for δF = e_d ⊗ ∇N_b
                    v += o[16] * (gF[d] * o[17 + c] - gF[c] * o[17 + d]) * s_N[q][a] * o[0];
                }
            }
            if (v != 0.0) unsafeAtomicAdd(nz + rowptr[s_dof[3 * a] + c] + blockpos[cell * (NB * NB) + a * NB + b] + d, v);
        }
}

int launch_facets(tb_form *f, tb_pattern *p, const double *d_u, double *d_nz, double *d_r)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    int rc = reset_status(dev);
    if (rc) return rc;
    if (d_nz) { rc = ensure_blockpos(p); if (rc) return rc; }
    const MechMesh mm{m->d_xyz, m->d_conn, m->d_cell_dofs, nullptr, nullptr};
    const int64_t *rowptr = p ? p->d_rowptr : nullptr;
    const uint16_t *bp = p ? p->d_blockpos : nullptr;
    if (m->field_kind == TB_HEX27)
        hipLaunchKernelGGL((k_facets<27>), dim3((unsigned)f->n_facets), dim3(64), 0, dev->stream, mm, f->d_facets, f->bc_kind, f->bc_param, f->facet_q, f->d_field,
                           d_u, d_nz, d_r, rowptr, bp, dev->d_status);
    else
        hipLaunchKernelGGL((k_facets<8>), dim3((unsigned)f->n_facets), dim3(64), 0, dev->stream, mm, f->d_facets, f->bc_kind, f->bc_param, f->facet_q, f->d_field,
                           d_u, d_nz, d_r, rowptr, bp, dev->d_status);
    TB_HIP(hipGetLastError());
    return check_status(dev);
}

} // namespace tb

// tb_mech_tet.hip — tetrahedral mechanics: entry point of the volume term (kernels in tb_mech_tet.hpp; this unit holds the second-order instances,
// tb_mech_tet4.hip the first-order ones) and the weak boundary conditions on triangular facets.
#include "tb_mech_tet.hpp"

namespace tb {

int launch_hyperelastic_tet(tb_form *f, tb_pattern *p, int strategy, const double *d_u, double *d_nz, double *d_r)
{
    tb_mesh *m = f->mesh;
    const bool p2 = m->field_kind == TB_TET10;
    if (f->cond_model || f->hill) { set_error("hyperelastic on tetrahedra: condensed internal variables and Hill frameworks are not implemented"); return TB_ERR_UNSUPPORTED; }
    if (f->qorder != (p2 ? 3 : 2)) {
        set_error("hyperelastic on tetrahedra: the %s field integrates with the degree-%d rule (qorder %d asked)", p2 ? "TB_TET10" : "TB_TET4", p2 ? 3 : 2, f->qorder);
        return TB_ERR_UNSUPPORTED;
    }
    int rc = reset_status(m->dev);
    if (rc) return rc;
    rc = p2 ? dispatch_tet<10>(f, p, strategy, d_u, d_nz, d_r) : launch_hyperelastic_tet4(f, p, strategy, d_u, d_nz, d_r);
    if (rc) return rc;
    return check_status(m->dev);
}

// ------------------------------------------------------------------------------------------------ weak boundary conditions
// Robin, normal spring and the pressure follower load (weak_boundary_conditions.jl:102-198, :200-300, :419-632) on the triangular facets of a
// tetrahedron: one 64-thread workgroup per (cell, local facet), like k_facets of the hexahedra.  The facet is flat and its normal constant.
template <int NQF> __device__ __forceinline__ double tri_bary(int q, int i)
{
    if (NQF == 3) return i == q ? 2.0 / 3.0 : 1.0 / 6.0;
    const double a = q < 3 ? 0.445948490915965 : 0.091576213509771;
    return i == (q < 3 ? q : q - 3) ? 1.0 - 2.0 * a : a;
}
template <int NQF> __device__ __forceinline__ double tri_weight(int q) // fraction of the facet area
{
    if (NQF == 3) return 1.0 / 3.0;
    return q < 3 ? 0.223381589678011 : 0.109951743655322;
}

template <int NB>
__global__ void __launch_bounds__(64)
k_facets_tet(TetMesh m, const int32_t *__restrict__ facets, int bc, double param, const double *__restrict__ pfield, const double *__restrict__ u,
             double *__restrict__ nz, double *__restrict__ r, const int64_t *__restrict__ rowptr, const uint16_t *__restrict__ blockpos, Status *st)
{
    constexpr int ND = 3 * NB, NQF = NB == 4 ? 3 : 6;
    const int tid = threadIdx.x;
    const int64_t cell = facets[2 * blockIdx.x];
    const int lf = facets[2 * blockIdx.x + 1];
    __shared__ double s_ue[ND], s_x[12], s_L[12], s_N[NQF][NB], s_G[NQF][NB][3];
    __shared__ double s_q[NQF][24]; // per point: dΓ, n₀[3], g[3] residual density, H[9] (Robin / spring: Hessian; pressure: F⁻¹), p·J, F⁻ᵀn₀[3]
    __shared__ double s_geo[5];     // detJ, area-weighted normal, its length
    __shared__ int32_t s_dof[ND];
    if (tid < ND) { const int32_t d = m.cell_dofs[cell * ND + tid]; s_dof[tid] = d; s_ue[tid] = u[d]; }
    if (tid < 12) s_x[tid] = m.xyz[3 * (int64_t)m.conn[cell * 4 + tid / 3] + tid % 3];
    __syncthreads();
    const int v0 = tet_facet_vertex(lf, 0), v1 = tet_facet_vertex(lf, 1), v2 = tet_facet_vertex(lf, 2);
    if (tid == 0) {
        const double det = tet_geometry(s_x, s_L);
        if (!(det > 0.0)) { st->neg_detj = 1; st->cell = cell; }
        const double e1[3] = {s_x[3 * v1] - s_x[3 * v0], s_x[3 * v1 + 1] - s_x[3 * v0 + 1], s_x[3 * v1 + 2] - s_x[3 * v0 + 2]};
        const double e2[3] = {s_x[3 * v2] - s_x[3 * v0], s_x[3 * v2 + 1] - s_x[3 * v0 + 1], s_x[3 * v2 + 2] - s_x[3 * v0 + 2]};
        const double nw[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = sqrt(nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2]);
        s_geo[0] = det; s_geo[1] = nw[0] / len; s_geo[2] = nw[1] / len; s_geo[3] = nw[2] / len; s_geo[4] = 0.5 * len; // facet area
    }
    __syncthreads();
    // shape values and mapped gradients per (point, node); the point's barycentric coordinates sit on the facet's three vertices
    for (int idx = tid; idx < NQF * NB; idx += 64) {
        const int q = idx / NB, a = idx - q * NB;
        double lam[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int v = 0; v < 4; ++v) lam[v] = (v == v0 ? tri_bary<NQF>(q, 0) : 0.0) + (v == v1 ? tri_bary<NQF>(q, 1) : 0.0) + (v == v2 ? tri_bary<NQF>(q, 2) : 0.0);
        double gr[3];
        tet_grad<NB>(a, lam, s_L, gr);
        s_N[q][a] = tet_shape<NB>(a, lam);
#pragma unroll
        for (int k = 0; k < 3; ++k) s_G[q][a][k] = gr[k];
    }
    __syncthreads();
    if (tid < NQF) {
        const int q = tid;
        double uq[3] = {0, 0, 0}, F[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
        for (int a = 0; a < NB; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uq[c] += s_N[q][a] * s_ue[3 * a + c];
#pragma unroll
                for (int k = 0; k < 3; ++k) F[c][k] += s_ue[3 * a + c] * s_G[q][a][k];
            }
        const double n0[3] = {s_geo[1], s_geo[2], s_geo[3]};
        double *o = s_q[q];
        o[0] = s_geo[4] * tri_weight<NQF>(q);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[1 + k] = n0[k];
        if (bc == TB_BC_ROBIN) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[4 + c] = 2.0 * param * uq[c];
#pragma unroll
            for (int e = 0; e < 9; ++e) o[7 + e] = (e % 4 == 0) ? 2.0 * param : 0.0;
        } else if (bc == TB_BC_NORMAL_SPRING) {
            const double un = uq[0] * n0[0] + uq[1] * n0[1] + uq[2] * n0[2];
#pragma unroll
            for (int c = 0; c < 3; ++c) o[4 + c] = param * un * n0[c];
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int d = 0; d < 3; ++d) o[7 + 3 * c + d] = param * n0[c] * n0[d];
        } else {
            double pq = param;
            if (bc == TB_BC_PRESSURE_FIELD && pfield) // evaluate_coefficient(pc, cell, qp, t): first-order nodal data at the facet point
                pq = param * (tri_bary<NQF>(q, 0) * pfield[cell * 4 + v0] + tri_bary<NQF>(q, 1) * pfield[cell * 4 + v1] + tri_bary<NQF>(q, 2) * pfield[cell * 4 + v2]);
            const double c00 = F[1][1] * F[2][2] - F[1][2] * F[2][1], c01 = F[1][2] * F[2][0] - F[1][0] * F[2][2], c02 = F[1][0] * F[2][1] - F[1][1] * F[2][0];
            const double Jf = F[0][0] * c00 + F[0][1] * c01 + F[0][2] * c02, id = 1.0 / Jf;
            const double Fi[9] = {c00 * id, (F[0][2] * F[2][1] - F[0][1] * F[2][2]) * id, (F[0][1] * F[1][2] - F[0][2] * F[1][1]) * id,
                                  c01 * id, (F[0][0] * F[2][2] - F[0][2] * F[2][0]) * id, (F[0][2] * F[1][0] - F[0][0] * F[1][2]) * id,
                                  c02 * id, (F[0][1] * F[2][0] - F[0][0] * F[2][1]) * id, (F[0][0] * F[1][1] - F[0][1] * F[1][0]) * id};
#pragma unroll
            for (int e = 0; e < 9; ++e) o[7 + e] = Fi[e];
            o[16] = pq * Jf;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double cn = Fi[0 + c] * n0[0] + Fi[3 + c] * n0[1] + Fi[6 + c] * n0[2]; // F⁻ᵀ n₀
                o[17 + c] = cn;
                o[4 + c] = pq * Jf * cn;
            }
        }
    }
    __syncthreads();
    // residual: rₑ[i] += δuᵢ·g dΓ
    if (r && tid < ND) {
        const int a = tid / 3, c = tid - 3 * a;
        double v = 0.0;
        for (int q = 0; q < NQF; ++q) v += s_N[q][a] * s_q[q][4 + c] * s_q[q][0];
        if (v != 0.0) unsafeAtomicAdd(r + s_dof[tid], v);
    }
    // tangent
    if (nz)
        for (int ij = tid; ij < ND * ND; ij += 64) {
            const int i = ij / ND, j = ij - i * ND, a = i / 3, c = i - 3 * a, b = j / 3, d = j - 3 * b;
            double v = 0.0;
            if (bc == TB_BC_ROBIN || bc == TB_BC_NORMAL_SPRING) {
                for (int q = 0; q < NQF; ++q) v += s_N[q][a] * s_q[q][7 + 3 * c + d] * s_N[q][b] * s_q[q][0];
            } else {
                for (int q = 0; q < NQF; ++q) {
                    const double *o = s_q[q], *Fi = o + 7, *gb = s_G[q][b];
                    // δ(J F⁻ᵀ n₀) for δF = e_d ⊗ ∇N_b
                    const double gFd = gb[0] * Fi[0 + d] + gb[1] * Fi[3 + d] + gb[2] * Fi[6 + d], gFc = gb[0] * Fi[0 + c] + gb[1] * Fi[3 + c] + gb[2] * Fi[6 + c];
                    v += o[16] * (gFd * o[17 + c] - gFc * o[17 + d]) * s_N[q][a] * o[0];
                }
            }
            if (v != 0.0) unsafeAtomicAdd(nz + rowptr[s_dof[3 * a] + c] + blockpos[cell * (NB * NB) + a * NB + b] + d, v);
        }
}

int launch_facets_tet(tb_form *f, tb_pattern *p, const double *d_u, double *d_nz, double *d_r)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    int rc = reset_status(dev);
    if (rc) return rc;
    if (d_nz) { rc = ensure_blockpos(p); if (rc) return rc; }
    const TetMesh tm{m->d_xyz, m->d_conn, m->d_cell_dofs, nullptr, nullptr};
    const int64_t *rowptr = p ? p->d_rowptr : nullptr;
    const uint16_t *bp = p ? p->d_blockpos : nullptr;
    if (m->field_kind == TB_TET10)
        hipLaunchKernelGGL((k_facets_tet<10>), dim3((unsigned)f->n_facets), dim3(64), 0, dev->stream, tm, f->d_facets, f->bc_kind, f->bc_param, f->d_field, d_u, d_nz, d_r,
                           rowptr, bp, dev->d_status);
    else
        hipLaunchKernelGGL((k_facets_tet<4>), dim3((unsigned)f->n_facets), dim3(64), 0, dev->stream, tm, f->d_facets, f->bc_kind, f->bc_param, f->d_field, d_u, d_nz, d_r,
                           rowptr, bp, dev->d_status);
    TB_HIP(hipGetLastError());
    return check_status(dev);
}

} // namespace tb

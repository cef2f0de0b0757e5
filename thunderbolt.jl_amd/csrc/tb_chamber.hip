// tb_chamber.hip — facet integrals of the 3D–0D chamber coupling (Regazzoni et al. 2022) for gfx950.
//
// Restates Pressure3D0DVolumeCouplerIntegrator of the reference (src/modeling/coupler/fsi.jl:118-185) with the volume integrands of
// RSAFDQ2022SurrogateVolume (src/modeling/rsafdq2022.jl:75-85) and Hirschvogel2017SurrogateVolume (fsi.jl:53-58).  With the chamber pressure p an
// unknown next to the displacement d, one pass over the chamber's facets produces
//   volume  V³ᴰ = Σ V(x, d, F, n₀) dΓ,               V = −J (H (x + d − b)) · F⁻ᵀ n₀     (H = h ⊗ h, or H = I, b = 0 for Hirschvogel)
//   row[j]  = Σ (∂V/∂d · δuⱼ + ∂V/∂F : ∇δuⱼ) dΓ       the J_pd block
//   col[i]  = Σ J (F⁻ᵀ n₀) · δuᵢ dΓ                   the J_dp block
//   r[i]   += p col-integrand, nz += p (δJ cofF + J δcofF) n₀ · δuᵢ dΓ   (what TB_BC_PRESSURE adds with param = p)
// The two partials are written out by hand.  With v = F⁻ᵀ n₀, w = H (x + d − b) and g = ∇N_b F⁻¹ (gF below):
//   ∂V/∂d · (N_b e_d)        = −N_b J (Hᵀ v)[d]
//   ∂V/∂F : (e_d ⊗ ∇N_b)     = −w · ∂(J F⁻ᵀ n₀)/∂F : (e_d ⊗ ∇N_b) = −J (g[d] (w·v) − (w·g) v[d])
// the second being the follower-load tangent of k_facets contracted with w instead of δuᵢ.
//
// One 64-lane workgroup per (cell, local facet), the geometry stage shared with k_facets (tb_facet_geom.hpp).  The volume partial of a workgroup goes to
// one of 64 slots 128 B apart (the reduction-slot scheme of tb_reduce.hpp: same-line atomics serialise in L2) and k_chamber_fold adds the slots to the
// caller's scalar; the host never reads it here.
#include <hip/hip_runtime.h>

#include "tb_facet_geom.hpp"
#include "tb_internal.h"
#include "tb_mech_common.hpp"

namespace tb {

struct ChamberParams { double H[9], b[3]; };

template <int NB>
__global__ void __launch_bounds__(64)
k_chamber(MechMesh m, const int32_t *__restrict__ facets, int fq, ChamberParams cp, const double *__restrict__ u, double p, double *__restrict__ nz,
          double *__restrict__ r, double *__restrict__ col, double *__restrict__ row, double *__restrict__ vol_slots, const int64_t *__restrict__ rowptr,
          const uint16_t *__restrict__ blockpos, Status *st)
{
    constexpr int ND = 3 * NB, MAXQ = 9;
    const int tid = threadIdx.x;
    const int64_t cell = facets[2 * blockIdx.x];
    const int lf = facets[2 * blockIdx.x + 1];
    __shared__ double s_ue[ND], s_x[24], s_N[MAXQ][NB], s_G[MAXQ][NB][3];
    // per point: [0] dΓ, [1..3] n₀, [4..6] J v, [7..15] F⁻¹, [16] J, [17..19] v = F⁻ᵀ n₀, [20..22] w, [23..25] J Hᵀ v, [26] w·v
    __shared__ double s_q[MAXQ][32];
    __shared__ int32_t s_dof[ND];
    for (int i = tid; i < ND; i += 64) { const int32_t d = m.cell_dofs[cell * ND + i]; s_dof[i] = d; s_ue[i] = u[d]; }
    for (int i = tid; i < 24; i += 64) s_x[i] = m.xyz[3 * (int64_t)m.conn[cell * 8 + i / 3] + i % 3];
    __syncthreads();
    const int nq = fq * fq;
    facet_geometry_stage<NB>(tid, cell, lf, fq, s_x, s_N, s_G, s_q, st);
    __syncthreads();
    double vq = 0.0; // this lane's share of the volume
    if (tid < nq) {
        const int q = tid;
        double xi[3];
        facet_xi(lf, fq, q, xi);
        double xd[3] = {-cp.b[0], -cp.b[1], -cp.b[2]}, F[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}; // xd = x + d − b
        for (int a = 0; a < 8; ++a) {
            double Ma, dMa[3];
            shape_at<8>(a, xi, Ma, dMa);
            for (int c = 0; c < 3; ++c) xd[c] += Ma * s_x[3 * a + c];
        }
        for (int a = 0; a < NB; ++a)
            for (int c = 0; c < 3; ++c) {
                xd[c] += s_N[q][a] * s_ue[3 * a + c];
                for (int k = 0; k < 3; ++k) F[c][k] += s_ue[3 * a + c] * s_G[q][a][k];
            }
        double *o = s_q[q];
        const double *n0 = o + 1;
        double Fi[9];
        const double Jf = inverse3(F, Fi);
        if (!(Jf > 0.0)) { st->neg_detj = 1; st->cell = cell; }
        for (int e = 0; e < 9; ++e) o[7 + e] = Fi[e];
        o[16] = p * Jf; // p·J, as k_facets folds it
        double v[3], w[3], wv = 0.0;
        for (int c = 0; c < 3; ++c) {
            v[c] = Fi[0 + c] * n0[0] + Fi[3 + c] * n0[1] + Fi[6 + c] * n0[2];
            w[c] = cp.H[3 * c] * xd[0] + cp.H[3 * c + 1] * xd[1] + cp.H[3 * c + 2] * xd[2];
            o[17 + c] = v[c];
            o[4 + c] = Jf * v[c];
            o[20 + c] = Jf * w[c];
            wv += w[c] * v[c];
        }
        for (int c = 0; c < 3; ++c) o[23 + c] = Jf * (cp.H[c] * v[0] + cp.H[3 + c] * v[1] + cp.H[6 + c] * v[2]);
        o[26] = Jf * wv;
        vq = -Jf * wv * o[0];
    }
    __syncthreads();
    if (vol_slots) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) vq += __shfl_xor(vq, s, 64);
        if (tid == 0) unsafeAtomicAdd(vol_slots + RED_STRIDE * (blockIdx.x & (RED_SLOTS - 1)), vq);
    }
    // col[i] += J v · δuᵢ dΓ, r[i] += p · the same
    if (col || r)
        for (int i = tid; i < ND; i += 64) {
            const int a = i / 3, c = i % 3;
            double cv = 0.0, rv = 0.0;
            for (int q = 0; q < nq; ++q) {
                cv += s_N[q][a] * s_q[q][4 + c] * s_q[q][0];
                rv += s_N[q][a] * (p * s_q[q][4 + c]) * s_q[q][0]; // the operation order of k_facets (g = p J v)
            }
            if (col && cv != 0.0) unsafeAtomicAdd(col + s_dof[i], cv);
            if (r && rv != 0.0) unsafeAtomicAdd(r + s_dof[i], rv);
        }
    // row[j] += (∂V/∂d · δuⱼ + ∂V/∂F : ∇δuⱼ) dΓ
    if (row)
        for (int j = tid; j < ND; j += 64) {
            const int b = j / 3, d = j % 3;
            double rv = 0.0;
            for (int q = 0; q < nq; ++q) {
                const double *o = s_q[q], *Fi = o + 7, *g = s_G[q][b];
                double gF[3];
                for (int k = 0; k < 3; ++k) gF[k] = g[0] * Fi[0 + k] + g[1] * Fi[3 + k] + g[2] * Fi[6 + k];
                const double wg = o[20] * gF[0] + o[21] * gF[1] + o[22] * gF[2]; // J w·g
                rv -= (s_N[q][b] * o[23 + d] + sel3(gF, d) * o[26] - wg * o[17 + d]) * o[0];
            }
            if (rv != 0.0) unsafeAtomicAdd(row + s_dof[j], rv);
        }
    // follower-load tangent p (δJ cofF + J δcofF) n₀ · δuᵢ, entry by entry as k_facets adds it for TB_BC_PRESSURE
    if (nz)
        for (int ij = tid; ij < ND * ND; ij += 64) {
            const int i = ij / ND, j = ij % ND, a = i / 3, c = i % 3, b = j / 3, d = j % 3;
            double v = 0.0;
            for (int q = 0; q < nq; ++q) {
                const double *o = s_q[q], *Fi = o + 7, *g = s_G[q][b];
                double gF[3];
                for (int k = 0; k < 3; ++k) gF[k] = g[0] * Fi[0 + k] + g[1] * Fi[3 + k] + g[2] * Fi[6 + k];
                v += o[16] * (sel3(gF, d) * o[17 + c] - sel3(gF, c) * o[17 + d]) * s_N[q][a] * o[0];
            }
            if (v != 0.0) unsafeAtomicAdd(nz + rowptr[s_dof[3 * a] + c] + blockpos[cell * (NB * NB) + a * NB + b] + d, v);
        }
}

// out[0] += the sum of the slot group; the slots return to zero (one wave)
__global__ void __launch_bounds__(64) k_chamber_fold(double *__restrict__ slots, double *__restrict__ out)
{
    const int l = threadIdx.x;
    double v = slots[RED_STRIDE * l];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    slots[RED_STRIDE * l] = 0.0;
    if (l == 0) out[0] += v;
}

int launch_chamber(tb_form *f, tb_pattern *pat, const double *d_u, double p, double *d_nz, double *d_r, double *d_col, double *d_row, double *d_volume)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    int rc = reset_status(dev);
    if (rc) return rc;
    if (d_nz) { rc = ensure_blockpos(pat); if (rc) return rc; }
    const MechMesh mm{m->d_xyz, m->d_conn, m->d_cell_dofs, nullptr, nullptr};
    const int64_t *rowptr = pat ? pat->d_rowptr : nullptr;
    const uint16_t *bp = pat ? pat->d_blockpos : nullptr;
    ChamberParams cp;
    for (int e = 0; e < 9; ++e) cp.H[e] = f->chamber_H[e];
    for (int e = 0; e < 3; ++e) cp.b[e] = f->chamber_b[e];
    // Group 0 of the device's reduction slots, which tb_dot and the CG kernels fold too: every user launches on dev->stream and leaves the group zero, so
    // the stream orders them.  A second stream would need a group of its own here.
    double *slots = d_volume ? dev->d_slots + (size_t)0 * RED_GROUP : nullptr;
    if (m->field_kind == TB_HEX27)
        hipLaunchKernelGGL((k_chamber<27>), dim3((unsigned)f->n_facets), dim3(64), 0, dev->stream, mm, f->d_facets, f->facet_q, cp, d_u, p, d_nz, d_r, d_col, d_row,
                           slots, rowptr, bp, dev->d_status);
    else
        hipLaunchKernelGGL((k_chamber<8>), dim3((unsigned)f->n_facets), dim3(64), 0, dev->stream, mm, f->d_facets, f->facet_q, cp, d_u, p, d_nz, d_r, d_col, d_row,
                           slots, rowptr, bp, dev->d_status);
    TB_HIP(hipGetLastError());
    if (d_volume) {
        hipLaunchKernelGGL(k_chamber_fold, dim3(1), dim3(64), 0, dev->stream, slots, d_volume);
        TB_HIP(hipGetLastError());
    }
    return check_status(dev);
}

} // namespace tb

// tb_facet_geom.hpp — FacetValues of a hexahedron facet, shared by the facet kernels (k_facets in tb_mech_facets.hip, k_chamber in tb_chamber.hip):
// Ferrite's local facet numbering, the Gauss points on the facet, shape values / mapped gradients of the field and dΓ, n₀ of the trilinear geometry.
#pragma once
#include <hip/hip_runtime.h>

#include "tb_mech_common.hpp"

namespace tb {

// local facet lf of Ferrite.reference_facets(RefHexahedron): the fixed reference coordinate, its value, and the two in-facet directions (s × t points outwards)
__host__ __device__ constexpr int facet_fix(int lf) { constexpr int v[6] = {2, 1, 0, 1, 0, 2}; return v[lf]; }
__host__ __device__ constexpr double facet_val(int lf) { constexpr double v[6] = {-1, -1, 1, 1, -1, 1}; return v[lf]; }
__host__ __device__ constexpr int facet_s(int lf) { constexpr int v[6] = {1, 0, 1, 2, 2, 0}; return v[lf]; }
__host__ __device__ constexpr int facet_t(int lf) { constexpr int v[6] = {0, 2, 2, 0, 1, 1}; return v[lf]; }

// Gauss–Legendre rule with fq = 1…3 points per facet direction (selects: a table indexed by fq would live in private memory)
__host__ __device__ constexpr double facet_gx(int fq, int i)
{
    return fq == 1 ? 0.0 : fq == 2 ? (i == 0 ? -0.5773502691896258 : 0.5773502691896258) : (i == 0 ? -0.7745966692414834 : i == 1 ? 0.0 : 0.7745966692414834);
}
__host__ __device__ constexpr double facet_gw(int fq, int i)
{
    return fq == 1 ? 2.0 : fq == 2 ? 1.0 : (i == 1 ? 0.8888888888888888 : 0.5555555555555556);
}
// reference coordinates of facet point q (q = s-index + fq · t-index)
__device__ inline void facet_xi(int lf, int fq, int q, double (&xi)[3])
{
    const int fx = facet_fix(lf), fs = facet_s(lf);
    const double vf = facet_val(lf), vs = facet_gx(fq, q % fq), vt = facet_gx(fq, q / fq);
#pragma unroll
    for (int k = 0; k < 3; ++k) xi[k] = k == fx ? vf : k == fs ? vs : vt; // selects, not indexed stores: xi stays in registers
}
__device__ inline double sel3(const double (&v)[3], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : v[2]; }

template <int NB>
__device__ inline void shape_at(int a, const double (&xi)[3], double &N, double (&dN)[3])
{
    if (NB == 8) {
        const double f[3] = {1.0 + hex_sgn(a, 0) * xi[0], 1.0 + hex_sgn(a, 1) * xi[1], 1.0 + hex_sgn(a, 2) * xi[2]};
        N = 0.125 * f[0] * f[1] * f[2];
        dN[0] = 0.125 * hex_sgn(a, 0) * f[1] * f[2];
        dN[1] = 0.125 * f[0] * hex_sgn(a, 1) * f[2];
        dN[2] = 0.125 * f[0] * f[1] * hex_sgn(a, 2);
    } else {
        double v[3], d[3];
        for (int k = 0; k < 3; ++k) { v[k] = quad1d(hex27_tix(a, k), xi[k]); d[k] = dquad1d(hex27_tix(a, k), xi[k]); }
        N = v[0] * v[1] * v[2];
        dN[0] = d[0] * v[1] * v[2];
        dN[1] = v[0] * d[1] * v[2];
        dN[2] = v[0] * v[1] * d[2];
    }
}

// Geometry stage of a 64-thread facet workgroup, thread (q, a): s_N[q][a] = Nₐ, s_G[q][a] = ∇Nₐ (mapped) at the fq² facet points, and per point
// s_q[q][0] = dΓ, s_q[q][1..3] = n₀.  s_x: the 8 vertex coordinates of the cell.  A non-positive geometry Jacobian raises the status block.
// The caller synchronises the workgroup before (s_x) and after.
template <int NB>
__device__ inline void facet_geometry_stage(int tid, int64_t cell, int lf, int fq, const double *s_x, double (*s_N)[NB], double (*s_G)[NB][3], double (*s_q)[32], Status *st)
{
    const int nq = fq * fq;
    for (int idx = tid; idx < nq * NB; idx += 64) {
        const int q = idx / NB, a = idx % NB;
        double xi[3];
        facet_xi(lf, fq, q, xi);
        double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int v = 0; v < 8; ++v) {
            double Mv, dM[3];
            shape_at<8>(v, xi, Mv, dM);
            for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) J[i][k] += s_x[3 * v + i] * dM[k];
        }
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02, id = 1.0 / det;
        const double Ji[3][3] = {{c00 * id, (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id, (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id},
                                 {c01 * id, (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id, (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id},
                                 {c02 * id, (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id, (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id}};
        double Na, dNa[3];
        shape_at<NB>(a, xi, Na, dNa);
        s_N[q][a] = Na;
        for (int k = 0; k < 3; ++k) s_G[q][a][k] = dNa[0] * Ji[0][k] + dNa[1] * Ji[1][k] + dNa[2] * Ji[2][k];
        if (a == 0) {
            if (!(det > 0.0)) { st->neg_detj = 1; st->cell = cell; }
            const int cs = facet_s(lf), ct = facet_t(lf);
            const double av[3] = {sel3(J[0], cs), sel3(J[1], cs), sel3(J[2], cs)}, bv[3] = {sel3(J[0], ct), sel3(J[1], ct), sel3(J[2], ct)};
            const double nw[3] = {av[1] * bv[2] - av[2] * bv[1], av[2] * bv[0] - av[0] * bv[2], av[0] * bv[1] - av[1] * bv[0]};
            const double len = sqrt(nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2]);
            s_q[q][0] = len * facet_gw(fq, q % fq) * facet_gw(fq, q / fq);
            for (int k = 0; k < 3; ++k) s_q[q][1 + k] = nw[k] / len;
        }
    }
}

// F⁻¹ (row-major) and det F
__device__ inline double inverse3(const double (&F)[3][3], double (&Fi)[9])
{
    const double c00 = F[1][1] * F[2][2] - F[1][2] * F[2][1], c01 = F[1][2] * F[2][0] - F[1][0] * F[2][2], c02 = F[1][0] * F[2][1] - F[1][1] * F[2][0];
    const double Jf = F[0][0] * c00 + F[0][1] * c01 + F[0][2] * c02, id = 1.0 / Jf;
    Fi[0] = c00 * id; Fi[1] = (F[0][2] * F[2][1] - F[0][1] * F[2][2]) * id; Fi[2] = (F[0][1] * F[1][2] - F[0][2] * F[1][1]) * id;
    Fi[3] = c01 * id; Fi[4] = (F[0][0] * F[2][2] - F[0][2] * F[2][0]) * id; Fi[5] = (F[0][2] * F[1][0] - F[0][0] * F[1][2]) * id;
    Fi[6] = c02 * id; Fi[7] = (F[0][1] * F[2][0] - F[0][0] * F[2][1]) * id; Fi[8] = (F[0][0] * F[1][1] - F[0][1] * F[1][0]) * id;
    return Jf;
}

} // namespace tb

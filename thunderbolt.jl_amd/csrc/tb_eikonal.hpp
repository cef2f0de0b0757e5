// tb_eikonal.hpp — the local solver of the anisotropic eikonal equation √(∇Tᵀ G ∇T) = 1 on one tetrahedron, host and device.
//
// The node to update sits at x₄, the other three vertices at xᵢ with arrival times Tᵢ; M = G⁻¹ (six doubles: xx, xy, xz, yy, yz, zz).  The update is
//   min over λ in the unit simplex of  F(λ) = Σ λᵢTᵢ + √(e(λ)ᵀ M e(λ)),   e(λ) = x₄ − Σ λᵢxᵢ = −Σ λᵢYᵢ,  Yᵢ = xᵢ − x₄
// — the arrival time of the fastest straight ray from the opposite face with T interpolated linearly on it (Fu, Kirby, Whitaker, SIAM J. Sci.
// Comput. 35 (2013); Jeong, Whitaker 30 (2008)).  F is convex, so its minimum over the simplex is a stationary point of F restricted to the face, to
// one of its three edges, or one of its three vertices.  With Q = YᵀMY the stationary point of a sub-simplex S is  λ_S ∝ Q_S⁻¹(μ1 − T_S),  F = μ,
// μ the larger root of (μ1 − T_S)ᵀ Q_S⁻¹ (μ1 − T_S) = 1, admissible iff the discriminant is non-negative and λ_S ≥ 0.
//
// That point is formed here relative to the sub-simplex itself, which stays well conditioned when the tetrahedron is flat (x₄ in or near the plane
// of the face: Q is then singular, while the face is as good as ever).  With the sub-simplex spanned from its first vertex Y_a by the edge vectors
// E (one for an edge, two for the face), P = EᵀME and g the differences of T along E:
//   foot of the M-perpendicular from x₄:  α₀ = −P⁻¹EᵀMY_a,  its length h = ‖Y_a + Eα₀‖_M taken from the vector itself (exact to rounding of the
//   coordinates even where h is tiny),  γ = gᵀP⁻¹g (the squared slope of T; γ < 1 is the non-negative discriminant),  α = α₀ − h P⁻¹g/√(1 − γ).
// Every admissible candidate is turned into its λ and the value returned is F AT THAT λ, evaluated through e(λ): what is returned is always the
// length of an admissible path — never below the true minimum — and an error of the candidate's λ enters to second order.
// The Tᵢ are shifted by their smallest finite member first.  A vertex with Tᵢ = +∞ (not reached yet) drops out of every candidate that would use
// it; with no finite Tᵢ the result is +∞.  No NaN is produced for finite coordinates and a positive definite M.
// The candidates are taken in a fixed order (vertices 1 2 3, edges 12 13 23, face) and a later one wins only where it is strictly smaller.
#pragma once
#include <hip/hip_runtime.h>

namespace tb {

// √(eᵀMe), e = Σ lᵢYᵢ (the sign of e does not matter)
__host__ __device__ inline double eikonal_norm(const double (&Y)[3][3], const double *M, double l0, double l1, double l2)
{
    const double e0 = l0 * Y[0][0] + l1 * Y[1][0] + l2 * Y[2][0];
    const double e1 = l0 * Y[0][1] + l1 * Y[1][1] + l2 * Y[2][1];
    const double e2 = l0 * Y[0][2] + l1 * Y[1][2] + l2 * Y[2][2];
    const double q = e0 * (M[0] * e0 + 2.0 * (M[1] * e1 + M[2] * e2)) + e1 * (M[3] * e1 + 2.0 * M[4] * e2) + M[5] * e2 * e2;
    return sqrt(q > 0.0 ? q : 0.0);
}

__host__ __device__ inline double eikonal_dot(const double *a, const double *Mb) { return a[0] * Mb[0] + a[1] * Mb[1] + a[2] * Mb[2]; }
__host__ __device__ inline void eikonal_mul(const double *M, const double *a, double *Ma)
{
    Ma[0] = M[0] * a[0] + M[1] * a[1] + M[2] * a[2];
    Ma[1] = M[1] * a[0] + M[3] * a[1] + M[4] * a[2];
    Ma[2] = M[2] * a[0] + M[4] * a[1] + M[5] * a[2];
}

// Y[i] = xᵢ − x₄ (rows), T[i], M6 → the minimum; lam (3 doubles, may be NULL) receives the minimiser (zeros when the result is +∞)
__host__ __device__ inline double eikonal_local_solve(const double (&Y)[3][3], const double (&T)[3], const double *M, double *lam)
{
    const double INF = __builtin_huge_val();
    const bool fin[3] = {T[0] < INF, T[1] < INF, T[2] < INF}; // false for +∞ (and for NaN, which no caller passes)
    double best = INF, bl[3] = {0.0, 0.0, 0.0};
    if (!(fin[0] || fin[1] || fin[2])) {
        if (lam) { lam[0] = 0.0; lam[1] = 0.0; lam[2] = 0.0; }
        return INF;
    }
    double T0 = INF;
    for (int i = 0; i < 3; ++i) if (fin[i] && T[i] < T0) T0 = T[i];
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = fin[i] ? T[i] - T0 : 0.0;
    double MY[3][3];
    for (int i = 0; i < 3; ++i) eikonal_mul(M, Y[i], MY[i]);
    // vertices
    for (int i = 0; i < 3; ++i) {
        if (!fin[i]) continue;
        const double q = eikonal_dot(Y[i], MY[i]);
        const double v = t[i] + sqrt(q > 0.0 ? q : 0.0);
        if (v < best) { best = v; bl[0] = bl[1] = bl[2] = 0.0; bl[i] = 1.0; }
    }
    // edges (i, j) = (0,1) (0,2) (1,2): the point Y_i + α (Y_j − Y_i)
    for (int k = 0; k < 3; ++k) {
        const int i = k == 2 ? 1 : 0, j = k == 0 ? 1 : 2;
        if (!(fin[i] && fin[j])) continue;
        const double a[3] = {Y[j][0] - Y[i][0], Y[j][1] - Y[i][1], Y[j][2] - Y[i][2]};
        const double Ma[3] = {MY[j][0] - MY[i][0], MY[j][1] - MY[i][1], MY[j][2] - MY[i][2]};
        const double P = eikonal_dot(a, Ma);
        const double g = t[j] - t[i];
        if (!(P > 0.0) || !(g * g < P)) continue; // a degenerate edge, or T steeper along it than a ray can follow: the minimum is at an end
        const double a0 = -eikonal_dot(Y[i], Ma) / P;
        double l[3] = {0.0, 0.0, 0.0};
        l[i] = 1.0 - a0; l[j] = a0;
        const double h = eikonal_norm(Y, M, l[0], l[1], l[2]);
        const double al = a0 - h * g / (P * sqrt(1.0 - g * g / P));
        if (!(al >= 0.0 && al <= 1.0)) continue;
        l[i] = 1.0 - al; l[j] = al;
        const double v = l[i] * t[i] + l[j] * t[j] + eikonal_norm(Y, M, l[0], l[1], l[2]);
        if (v < best) { best = v; bl[0] = l[0]; bl[1] = l[1]; bl[2] = l[2]; }
    }
    // face: the point Y_0 + α (Y_1 − Y_0) + β (Y_2 − Y_0)
    if (fin[0] && fin[1] && fin[2]) {
        const double a[3] = {Y[1][0] - Y[0][0], Y[1][1] - Y[0][1], Y[1][2] - Y[0][2]}, b[3] = {Y[2][0] - Y[0][0], Y[2][1] - Y[0][1], Y[2][2] - Y[0][2]};
        const double Ma[3] = {MY[1][0] - MY[0][0], MY[1][1] - MY[0][1], MY[1][2] - MY[0][2]}, Mb[3] = {MY[2][0] - MY[0][0], MY[2][1] - MY[0][1], MY[2][2] - MY[0][2]};
        const double Paa = eikonal_dot(a, Ma), Pab = eikonal_dot(a, Mb), Pbb = eikonal_dot(b, Mb);
        const double det = Paa * Pbb - Pab * Pab;
        if (det > 0.0 && Paa > 0.0) {
            const double ca = eikonal_dot(Y[0], Ma), cb = eikonal_dot(Y[0], Mb);
            const double a0 = -(Pbb * ca - Pab * cb) / det, b0 = -(Paa * cb - Pab * ca) / det; // the foot
            const double ga = t[1] - t[0], gb = t[2] - t[0];
            const double ua = (Pbb * ga - Pab * gb) / det, ub = (Paa * gb - Pab * ga) / det;   // P⁻¹ g
            const double gamma = ga * ua + gb * ub;
            if (gamma < 1.0) {
                const double h = eikonal_norm(Y, M, 1.0 - a0 - b0, a0, b0);
                const double f = h / sqrt(1.0 - gamma);
                const double al = a0 - f * ua, be = b0 - f * ub;
                const double l0 = 1.0 - al - be;
                if (l0 >= 0.0 && al >= 0.0 && be >= 0.0) {
                    const double v = l0 * t[0] + al * t[1] + be * t[2] + eikonal_norm(Y, M, l0, al, be);
                    if (v < best) { best = v; bl[0] = l0; bl[1] = al; bl[2] = be; }
                }
            }
        }
    }
    if (lam) { lam[0] = bl[0]; lam[1] = bl[1]; lam[2] = bl[2]; }
    return T0 + best;
}

#ifdef TB_ABLATION
// The same candidates from the Gram matrix Q = YMYᵀ alone (Q00, Q01, Q02, Q11, Q12, Q22) — what a per-tetrahedron table of the six edge products
// supplies (profiling build: the layout that was measured against the coordinates).  Norms are taken as √(lᵀQl), which cancels
// where the tetrahedron is flat; the product library does not contain this function.
__host__ __device__ inline double eikonal_local_solve_gram(const double (&Q)[6], const double (&T)[3])
{
    const double INF = __builtin_huge_val();
    const bool fin[3] = {T[0] < INF, T[1] < INF, T[2] < INF};
    if (!(fin[0] || fin[1] || fin[2])) return INF;
    double T0 = INF, t[3];
    for (int i = 0; i < 3; ++i) if (fin[i] && T[i] < T0) T0 = T[i];
    for (int i = 0; i < 3; ++i) t[i] = fin[i] ? T[i] - T0 : 0.0;
    const double q[3][3] = {{Q[0], Q[1], Q[2]}, {Q[1], Q[3], Q[4]}, {Q[2], Q[4], Q[5]}};
    double best = INF;
    for (int i = 0; i < 3; ++i)
        if (fin[i]) { const double v = t[i] + sqrt(q[i][i] > 0.0 ? q[i][i] : 0.0); if (v < best) best = v; }
    for (int k = 0; k < 3; ++k) {
        const int i = k == 2 ? 1 : 0, j = k == 0 ? 1 : 2;
        if (!(fin[i] && fin[j])) continue;
        const double P = q[i][i] - 2.0 * q[i][j] + q[j][j], g = t[j] - t[i];
        if (!(P > 0.0) || !(g * g < P)) continue;
        const double c = q[i][j] - q[i][i], a0 = -c / P;
        const double h2 = q[i][i] - c * c / P, h = sqrt(h2 > 0.0 ? h2 : 0.0);
        const double al = a0 - h * g / (P * sqrt(1.0 - g * g / P));
        if (!(al >= 0.0 && al <= 1.0)) continue;
        const double li = 1.0 - al, n2 = li * li * q[i][i] + 2.0 * li * al * q[i][j] + al * al * q[j][j];
        const double v = li * t[i] + al * t[j] + sqrt(n2 > 0.0 ? n2 : 0.0);
        if (v < best) best = v;
    }
    if (fin[0] && fin[1] && fin[2]) {
        const double Paa = q[1][1] - 2.0 * q[0][1] + q[0][0], Pbb = q[2][2] - 2.0 * q[0][2] + q[0][0], Pab = q[1][2] - q[0][1] - q[0][2] + q[0][0];
        const double det = Paa * Pbb - Pab * Pab;
        if (det > 0.0 && Paa > 0.0) {
            const double ca = q[0][1] - q[0][0], cb = q[0][2] - q[0][0];
            const double a0 = -(Pbb * ca - Pab * cb) / det, b0 = -(Paa * cb - Pab * ca) / det;
            const double ga = t[1] - t[0], gb = t[2] - t[0];
            const double ua = (Pbb * ga - Pab * gb) / det, ub = (Paa * gb - Pab * ga) / det;
            const double gamma = ga * ua + gb * ub;
            if (gamma < 1.0) {
                const double h2 = q[0][0] + ca * a0 + cb * b0;
                const double f = sqrt(h2 > 0.0 ? h2 : 0.0) / sqrt(1.0 - gamma);
                const double al = a0 - f * ua, be = b0 - f * ub, l0 = 1.0 - al - be;
                if (l0 >= 0.0 && al >= 0.0 && be >= 0.0) {
                    const double n2 = l0 * (l0 * q[0][0] + 2.0 * (al * q[0][1] + be * q[0][2])) + al * (al * q[1][1] + 2.0 * be * q[1][2]) + be * be * q[2][2];
                    const double v = l0 * t[0] + al * t[1] + be * t[2] + sqrt(n2 > 0.0 ? n2 : 0.0);
                    if (v < best) best = v;
                }
            }
        }
    }
    return T0 + best;
}
#endif

} // namespace tb

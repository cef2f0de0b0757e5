// tb_maxwell.hpp — LinearMaxwellMaterial (src/modeling/solid/materials.jl:1816-2008) at one quadrature point, host and device.
//
// Small strain ε = sym(∇u); ℂ = λ̃ I⊗I + 2μ̃ 𝕀ˢʸᵐ with λ̃ = ν/((1+ν)(1−2ν)), 2μ̃ = 1/(1+ν).
//   stress (materials.jl:1960-1967)              σ = E₀ ℂ:ε + E₁ ℂ:(ε − εᵛ₁)
//   local problem, backward Euler (:1854-1879)   (𝕀/Δt + aℂ) : εᵛ₁ = εᵛ₀/Δt + aℂ : ε,  a = E₁/η₁
//   condensed tangent (:1881-1936, :1976-1985)   ∂σ/∂ε = (E₀+E₁)ℂ − E₁ ℂ : (𝕀/Δt + aℂ)⁻¹ : aℂ
// ℂ is isotropic: the spherical and the deviatoric part are its eigenspaces (k_v = 1/(1−2ν), k_d = 1/(1+ν)), so the reference's 6 × 6 Mandel
// solve is two scalar divisions.  Per part p: gₚ = a kₚ Δt/(1 + a kₚ Δt), εᵛ₁ₚ = εᵛ₀ₚ + gₚ (εₚ − εᵛ₀ₚ), kₚ* = kₚ (E₀ + E₁ (1 − gₚ)); the tangent is the
// isotropic tensor with 2μ* = k_d*, λ* = (k_v* − k_d*)/3.  All of it depends on the parameters and Δt only — the coefficients are computed once per
// launch on the host.  The update is written as an increment of εᵛ₀ so that both limits are reached with finite values: Δt → 0 gives g = 0 and
// εᵛ₁ = εᵛ₀ bit for bit (so does E₁ = 0), Δt → ∞ gives g → 1, εᵛ₁ → ε and the tangent → E₀ℂ.
// State components in the order of SymmetricTensor{2,3}.data: (11, 21, 31, 22, 32, 33).
#pragma once
#include <hip/hip_runtime.h>

namespace tb {

struct MaxwellCoef {
    double lam, mu2; // ℂ = lam I⊗I + mu2 𝕀ˢʸᵐ
    double E0, E1;
    double gv, gd;   // relaxed fraction of the spherical / deviatoric part over the step
    double lam_s, mu_s; // condensed tangent λ*, μ*
};

// p = {E₀, E₁, μ, η₁, ν}; μ is carried and unused, as in the reference
__host__ __device__ inline MaxwellCoef maxwell_coef(const double *p, double dt)
{
    MaxwellCoef c;
    const double E0 = p[0], E1 = p[1], eta = p[3], nu = p[4];
    const double kv = 1.0 / (1.0 - 2.0 * nu), kd = 1.0 / (1.0 + nu), a = E1 / eta;
    c.lam = nu / ((1.0 + nu) * (1.0 - 2.0 * nu));
    c.mu2 = kd;
    c.E0 = E0; c.E1 = E1;
    const double xv = a * kv * dt, xd = a * kd * dt;
    const double hv = 1.0 / (1.0 + xv), hd = 1.0 / (1.0 + xd); // 1 − g
    c.gv = xv * hv; c.gd = xd * hd;
    const double kvs = kv * (E0 + E1 * hv), kds = kd * (E0 + E1 * hd);
    c.mu_s = 0.5 * kds;
    c.lam_s = (kvs - kds) / 3.0;
    return c;
}

// ∇u (row-major H[3c+k]) and the accepted viscous strain Q0 → the new viscous strain Q1 and σ (full 3 × 3, row-major)
__host__ __device__ inline void maxwell_point(const MaxwellCoef &c, const double *H, const double (&Q0)[6], double (&Q1)[6], double (&sig)[9])
{
    // components s = 0…5 ↔ (i, j) = (0,0) (1,0) (2,0) (1,1) (2,1) (2,2)
    const double e[6] = {H[0], 0.5 * (H[3] + H[1]), 0.5 * (H[6] + H[2]), H[4], 0.5 * (H[7] + H[5]), H[8]};
    const double ev = (e[0] + e[3] + e[5]) / 3.0, qv = (Q0[0] + Q0[3] + Q0[5]) / 3.0;
    const double dv = c.gv * (ev - qv);
    double s[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const bool diag = k == 0 || k == 3 || k == 5;
        const double ed = e[k] - (diag ? ev : 0.0), qd = Q0[k] - (diag ? qv : 0.0);
        Q1[k] = Q0[k] + c.gd * (ed - qd) + (diag ? dv : 0.0);
        s[k] = (c.E0 + c.E1) * e[k] - c.E1 * Q1[k];
    }
    const double lt = c.lam * (s[0] + s[3] + s[5]);
    sig[0] = lt + c.mu2 * s[0]; sig[4] = lt + c.mu2 * s[3]; sig[8] = lt + c.mu2 * s[5];
    sig[1] = sig[3] = c.mu2 * s[1];
    sig[2] = sig[6] = c.mu2 * s[2];
    sig[5] = sig[7] = c.mu2 * s[4];
}

} // namespace tb

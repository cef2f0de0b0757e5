// tb_math.hpp — bounded-argument exponential and refined reciprocal shared by the reaction and the source-term kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

// The header also compiles with a plain host C++ compiler (tests/test_tt06_derived_constants.py measures the functions against long double there,
// and on the device through tests/tb_math_device.hip): the polynomials and Newton steps are the same code, only the two hardware seeds are stood in
// for (below).
#if defined(__HIP_DEVICE_COMPILE__) || (defined(__clang__) && defined(__HIP__))
#define TB_MATH_DEVICE 1
#else
#define TB_MATH_DEVICE 0
#endif

namespace tb {

#if TB_MATH_DEVICE
__device__ __forceinline__ double hw_rcp(double y) { return __builtin_amdgcn_rcp(y); }
__device__ __forceinline__ double hw_rsq(double y) { return __builtin_amdgcn_rsq(y); }
#else
// host stand-ins of v_rcp_f64 / v_rsq_f64: the exact value cut to 23 significant bits (relative error < 2⁻²², no better than the hardware's seeds)
inline double hw_cut23(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, 8);
    b &= ~((uint64_t(1) << 30) - 1);
    std::memcpy(&v, &b, 8);
    return v;
}
inline double hw_rcp(double y) { return hw_cut23(1.0 / y); }
inline double hw_rsq(double y) { return hw_cut23(1.0 / std::sqrt(y)); }
#endif

#if TB_MATH_DEVICE
// workgroup barrier that orders LDS traffic only: __syncthreads() also drains vmcnt, i.e. waits for every global store and prefetch load in flight
__device__ __forceinline__ void lds_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
#endif

// exp for bounded arguments (|x| ≲ 700; ionic-model arguments stay within ±100): k = rint(x·log₂e), r = x − k·ln2 in two
// pieces (|r| ≤ 0.347), 1 + r + r²·P(r) with P the degree-10 polynomial through the Chebyshev points of (eʳ − 1 − r)/r² on ±0.34658 (a near-minimax
// polynomial of degree 12 in all; relative truncation 3.3·10⁻¹⁹ with the coefficients as rounded), one ldexp.  ≈20 instructions against ≈40 of the
// library routine, which spends the rest on special cases that cannot occur here.  Largest error against long double over 1.7·10⁶ arguments of
// [−700, 700], 8·10⁵ of them within a few ulp to 10⁻³ of a reduction boundary (k + ½)·ln2: 0.862 ulp; the degree-13 Taylor polynomial this replaces
// (truncation 5.7·10⁻¹⁸): 0.870 ulp on the same arguments.  Degree 11 of the same construction truncates at 1.6·10⁻¹⁷, above the Taylor form: not taken.
// tests/test_tt06_derived_constants.py repeats the measurement with the Taylor form as its comparison copy; tests/test_gpu_parity.py compares whole
// trajectories at 1e-12.  On the device (gfx950, -O3 -ffp-contract=fast; tests/tb_math_device.hip): bit for bit the host build's values on 2¹⁸ arguments
// of the same kind, 0.857 ulp on them.
__device__ __forceinline__ double exp_b(double x)
{
    x = fmin(fmax(x, -700.0), 700.0);
    const double kf = rint(x * 1.4426950408889634);
    double r = fma(kf, -6.93147180369123816490e-01, x);
    r = fma(kf, -1.90821492927058770002e-10, r);
    const double c[11] = {2.0914680780540263e-09, 2.5105208339987698e-08, 2.7557273657975953e-07, 2.7557255421023506e-06, 2.4801587325536023e-05, 0.00019841269874804214, 0.0013888888888883752, 0.00833333333332614, 0.04166666666666667, 0.1666666666666667, 0.5};
    double q = c[0];
#pragma unroll
    for (int i = 1; i < 11; ++i) q = fma(q, r, c[i]);
    q = fma(q, r, 1.0); // … + r
    q = fma(q, r, 1.0); // 1 + r·(…)
    return ldexp(q, (int)kf);
}

// 1/y for well-scaled arguments: hardware reciprocal refined by two Newton steps (≤ 1–2 ulp), 5 instructions against the
// ≈12 of the IEEE division sequence (no scaling / fix-up: gate and buffer denominators are O(1) numbers).  Measured on the device with v_rcp_f64 as the
// seed: 0.500 ulp over 10⁻¹² ≤ |y| ≤ 10¹² of both signs and [1, 2] (2¹⁸ arguments; the host stand-in gives the same, one value of them differs); the
// test holds it to 2 ulp
__device__ __forceinline__ double rcp_b(double y)
{
    double r = hw_rcp(y);
    r = fma(fma(-y, r, 1.0), r, r);
    r = fma(fma(-y, r, 1.0), r, r);
    return r;
}

// 1/√y for well-scaled positive arguments: hardware reciprocal square root refined by two Newton steps r ← r + (r/2)(1 − y r²) (≤ 1 ulp,
// tests/test_tt06_derived_constants.py), 9 instructions in place of an IEEE square root followed by an IEEE division (1.49 ulp).  Measured on the device
// with v_rsq_f64 as the seed: 0.986 ulp over [1, 4] and 10⁻⁶ … 10⁶ (2¹⁸ arguments; host stand-in 0.968 ulp, 16 % of the values differ in the last
// place), 1.0 / sqrt(y) in the same kernel 1.471 ulp
__device__ __forceinline__ double rsqrt_b(double y)
{
    double r = hw_rsq(y);
    r = fma(0.5 * r, fma(-(y * r), r, 1.0), r);
    r = fma(0.5 * r, fma(-(y * r), r, 1.0), r);
    return r;
}

// log for positive normal arguments (concentrations, 10⁻⁷ … 10³): x = m·2ᵉ with m ∈ [√½, √2), log m = 2 atanh f, f = (m − 1)/(m + 1), |f| ≤ 0.172,
// odd series to f²¹ (truncation 4·10⁻¹⁸).  ≈ 27 instructions; no special cases (zero, negative, subnormal, infinite arguments cannot occur).
// Against long double: 2.38 ulp over 10⁻⁷ … 10³ and 2.42 ulp over [0.7, 1.3] (host build, 3·10⁶ arguments each; libm's log 0.52 ulp); the error is
// that of f (a rounded difference times a rounded reciprocal) carried one to one into 2f(1 + …).  On the device 2.327 ulp, bit for bit the host build's
// values (2¹⁸ arguments, both sides of every m = √½ cut among them).  The tests hold the host build to 3 ulp and the device to the host figure + 3
__device__ __forceinline__ double log_b(double x)
{
    int e;
    double m = frexp(x, &e); // [0.5, 1)
    if (m < 0.70710678118654752) { m += m; --e; }
    const double f = (m - 1.0) * rcp_b(m + 1.0), f2 = f * f;
    const double c[10] = {1.0 / 21.0, 1.0 / 19.0, 1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0};
    double q = c[0];
#pragma unroll
    for (int i = 1; i < 10; ++i) q = fma(q, f2, c[i]);
    q = fma(q * f2, f, f); // f + f³(…)
    const double ef = (double)e;
    return fma(ef, 6.93147180369123816490e-01, fma(ef, 1.90821492927058770002e-10, q + q));
}

// expm1 for the Rush–Larsen factor: series for small arguments (no cancellation), exp − 1 otherwise.  Against long double: 1.48 ulp for |z| < 0.3,
// 3.31 ulp for 0.3 ≤ |z| ≤ 50 (host build, 3·10⁶ arguments each; exp(z) − 1 with libm 2.01 ulp: just above the switch 0.86 ulp of exp_b at 1.35 are
// 3.4 ulp of the difference 0.35).  On the device bit for bit the host build's values, 2.580 ulp on 2¹⁸ arguments (±0.3 ± a few ulp among them); the test holds the host
// build to 4 ulp
__device__ __forceinline__ double expm1_b(double z)
{
    if (fabs(z) < 0.3) {
        double q = 1.6059043836821613e-10;
        const double c[11] = {2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06, 2.48015873015873e-05,
                              0.0001984126984126984, 0.001388888888888889, 0.008333333333333333, 0.041666666666666664, 0.16666666666666666, 0.5};
#pragma unroll
        for (int i = 0; i < 11; ++i) q = fma(q, z, c[i]);
        q = fma(q, z, 1.0);
        return q * z;
    }
    return exp_b(z) - 1.0;
}

} // namespace tb

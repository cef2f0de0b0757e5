// Host build of thunderbolt.jl_amd/csrc/tb_math.hpp for tests/test_tt06_derived_constants.py: the values of all five functions (eval_*), and the largest
// error, in units of the last place of the exact result, of exp_b and rsqrt_b against long double (64-bit significand: the truth is good to 2⁻¹¹ of a double's last place), next to the
// same figure of the forms they replace, measured in the same run on the same arguments.
#include <cmath>

#include "tb_math.hpp"

namespace before {

// exp_b as it stood before the minimax coefficients (degree-13 Taylor polynomial): the comparison copy
inline double exp_b(double x)
{
    x = fmin(fmax(x, -700.0), 700.0);
    const double kf = rint(x * 1.4426950408889634);
    double r = fma(kf, -6.93147180369123816490e-01, x);
    r = fma(kf, -1.90821492927058770002e-10, r);
    const double c[12] = {1.6059043836821613e-10, 2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06, 2.48015873015873e-05, 0.0001984126984126984, 0.001388888888888889, 0.008333333333333333, 0.041666666666666664, 0.16666666666666666, 0.5};
    double q = c[0];
    for (int i = 1; i < 12; ++i) q = fma(q, r, c[i]);
    q = fma(q, r, 1.0);
    q = fma(q, r, 1.0);
    return ldexp(q, (int)kf);
}

// 1/√y as the xs-gate time constant had it: an IEEE division by an IEEE square root
inline double rsqrt(double y) { return 1.0 / sqrt(y); }

} // namespace before

static double ulps(double got, long double truth)
{
    const long double ulp = ldexpl(1.0L, ilogbl(truth) - 52);
    return (double)(fabsl((long double)got - truth) / ulp);
}

template <class F, class T> static double max_ulps(const double *x, long n, F f, T truth)
{
    double m = 0.0;
    for (long i = 0; i < n; ++i) {
        const double e = ulps(f(x[i]), truth(x[i]));
        if (!(e <= m)) m = e; // (a NaN sticks)
    }
    return m;
}

extern "C" {
double max_ulps_exp_b(const double *x, long n) { return max_ulps(x, n, [](double v) { return tb::exp_b(v); }, [](double v) { return expl((long double)v); }); }
double max_ulps_exp_b_before(const double *x, long n) { return max_ulps(x, n, [](double v) { return before::exp_b(v); }, [](double v) { return expl((long double)v); }); }
double max_ulps_rsqrt_b(const double *x, long n) { return max_ulps(x, n, [](double v) { return tb::rsqrt_b(v); }, [](double v) { return 1.0L / sqrtl((long double)v); }); }
double max_ulps_rsqrt_before(const double *x, long n) { return max_ulps(x, n, [](double v) { return before::rsqrt(v); }, [](double v) { return 1.0L / sqrtl((long double)v); }); }
// y[i] = f(x[i]): the values themselves, for the comparison with the device build (tests/tb_math_device.hip) and for errors measured by the caller
void eval_exp_b(const double *x, long n, double *y) { for (long i = 0; i < n; ++i) y[i] = tb::exp_b(x[i]); }
void eval_rcp_b(const double *x, long n, double *y) { for (long i = 0; i < n; ++i) y[i] = tb::rcp_b(x[i]); }
void eval_rsqrt_b(const double *x, long n, double *y) { for (long i = 0; i < n; ++i) y[i] = tb::rsqrt_b(x[i]); }
void eval_log_b(const double *x, long n, double *y) { for (long i = 0; i < n; ++i) y[i] = tb::log_b(x[i]); }
void eval_expm1_b(const double *x, long n, double *y) { for (long i = 0; i < n; ++i) y[i] = tb::expm1_b(x[i]); }
}

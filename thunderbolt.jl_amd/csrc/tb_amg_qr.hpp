// tb_amg_qr.hpp — the column arithmetic of the per-aggregate QR of tb_amg_block.hip (step 4 of the near-null-space method in include/tbhip.h), shared by
// the device kernel and a host driver: modified Gram–Schmidt on an m × k block (k ≤ 6), columns in order, R_jj > 0, dead columns zeroed.
// 64 lanes stride the rows; every dot product is a lane sum in stride order (fused multiply-adds, written out so that host and device round alike)
// folded by the butterfly of offsets 32 … 1.  The executor X says what "every lane" means: one wave on the device (WaveExec in tb_amg_block.hip), a loop
// over 64 emulated lanes on the host (HostExec below) — the same sums in the same order, so the same bits.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TB_QR_HD __host__ __device__
#else
#define TB_QR_HD
#endif

namespace tb {
namespace amgqr {

constexpr int MAX_K = 6;
constexpr int LANES = 64;
constexpr double DEAD_RATIO = 1e-8;     // a column is dead when its norm after orthogonalisation is ≤ DEAD_RATIO × its norm before

// the share of one lane: rows lane, lane + 64, …
template <class W>
TB_QR_HD inline double lane_dot(const W &w, int m, int lane, int a, int b)
{
    double s = 0.0;
    for (int p = lane; p < m; p += LANES) s = fma(w.get(p, a), w.get(p, b), s);
    return s;
}
template <class W>
TB_QR_HD inline void lane_axpy(W &w, int m, int lane, int j, int i, double r) // column j −= r · column i
{
    for (int p = lane; p < m; p += LANES) w.set(p, j, fma(-r, w.get(p, i), w.get(p, j)));
}
template <class W>
TB_QR_HD inline void lane_divide(W &w, int m, int lane, int j, double d) // column j /= d (d = 0: the column is set to zero)
{
    for (int p = lane; p < m; p += LANES) w.set(p, j, d != 0.0 ? w.get(p, j) / d : 0.0);
}

// B_a = Q_a R_a in place: w holds B_a on entry and Q_a on return; R (k × k, row-major, upper triangular) and dead (k bytes) are the same in every lane.
// The projections on a dead column are zero (its q is), those of a dead column on the live ones before it are kept: Q R = B holds for dead columns too.
template <class W, class X>
TB_QR_HD inline void factor(W &w, int m, int k, X &x, double *R, uint8_t *dead)
{
    for (int i = 0; i < k * k; ++i) R[i] = 0.0;
    for (int j = 0; j < k; ++j) {
        const double before = sqrt(x.sum([&](int lane) { return lane_dot(w, m, lane, j, j); }));
        for (int i = 0; i < j; ++i) {
            if (dead[i]) continue;
            const double r = x.sum([&](int lane) { return lane_dot(w, m, lane, i, j); });
            R[i * k + j] = r;
            x.each([&](int lane) { lane_axpy(w, m, lane, j, i, r); });
        }
        const double after = sqrt(x.sum([&](int lane) { return lane_dot(w, m, lane, j, j); }));
        dead[j] = after <= DEAD_RATIO * before ? 1 : 0;
        const double d = dead[j] ? 0.0 : after;
        R[j * k + j] = d;
        x.each([&](int lane) { lane_divide(w, m, lane, j, d); });
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// the host's 64 lanes: the lane values in an array, folded as the wave's __shfl_xor butterfly folds them (v_l += v_{l ^ o}, o = 32 … 1)
struct HostExec {
    template <class F>
    double sum(F f)
    {
        double v[LANES], u[LANES];
        for (int l = 0; l < LANES; ++l) v[l] = f(l);
        for (int o = LANES / 2; o > 0; o >>= 1) {
            for (int l = 0; l < LANES; ++l) u[l] = v[l] + v[l ^ o];
            for (int l = 0; l < LANES; ++l) v[l] = u[l];
        }
        return v[0];
    }
    template <class F>
    void each(F f)
    {
        for (int l = 0; l < LANES; ++l) f(l);
    }
};
#endif

} // namespace amgqr
} // namespace tb

// tb_bidomain_internal.hpp — what tb_bidomain.hip shares with tb_bidomain_mg.hip (the multigrid preconditioner of the block system): the block system's
// record, the sliced block product with its two storage variants and its smoother epilogue, and the 2 × 2 block preconditioner of one node.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tb_internal.h"
#include "tb_reduce.hpp"

struct tb_bidomain {
    tb_pattern *pat = nullptr;
    int64_t n = 0, n_slices = 0, entries = 0; // rows, slices of 64 rows, value slots per plane (Σ 64 · width)
    int64_t *d_base = nullptr;                // n_slices + 1: first slot of every slice (multiples of 64)
    uint32_t *d_col = nullptr;                // entries: column | grounded << 31
    double *d_val = nullptr;                  // 3 · entries: planes a₁₁, a₁₂ (= a₂₁ off the ground), a₂₂
    double *d_binv = nullptr;                 // 3 n: inverse of every node's diagonal block (b₁₁, b₁₂, b₂₂)
    uint8_t *d_ground = nullptr;              // n: the flags of the latest tb_bidomain_set_matrices
    double *d_ws = nullptr;                   // r, p, Ap (2n each) and 8 scalars of the solve
    double ground_diag = 1.0;
    bool have_matrices = false;
    uint64_t generation = 0;                  // counts tb_bidomain_set_matrices: what a multigrid set-up remembers (tb_bidomain_mg.hip)
};

namespace tb {

constexpr uint32_t BD_GROUNDED = 0x80000000u;

// the interleaved vectors are read and written as 16-byte pairs
#define BD_ALIGNED(ptr_, who_) TB_REQUIRE(((uintptr_t)(ptr_) & 15) == 0, who_ ": an interleaved vector must be 16-byte aligned")

// z = B⁻¹ r of one node
__device__ __forceinline__ double2 bd_precondition(const double *__restrict__ binv, int64_t i, double2 r)
{
    const double b11 = binv[3 * i], b12 = binv[3 * i + 1], b22 = binv[3 * i + 2];
    return make_double2(b11 * r.x + b12 * r.y, b12 * r.x + b22 * r.y);
}

// the smoother epilogue of k_bd_apply (STEP > 0): the Chebyshev recurrence of k_mg_cheb on node pairs, B⁻¹ in the place of D⁻¹
struct BdStep {
    double c1 = 0.0, c2 = 0.0;
    const double *binv = nullptr; // 3 n
    const double2 *r = nullptr;
    double2 *d = nullptr;
};

// y = A x, one slice per wave, one row per lane, the entries of a row in their stored order.  DOT: the partials of xᵀy go to the slot group xy.
// FULL: the storage of a coarse multigrid level — four value planes (a₁₁, a₁₂, a₂₁, a₂₂) with the elimination of the ground baked in, no flag in the
// columns, no ground flags (the coarse φₘφₑ block is not symmetric once a grounded fine node is no coarse node); the three-plane instance is the
// fine level's, its arithmetic and its order untouched.  STEP: instead of storing A x the row's lane finishes one Chebyshev step in registers,
// d ← c₁ d + c₂ B⁻¹(r − A x) (STEP 1: the first step, d ← c₂ B⁻¹(r − A x)), y ← x + d: y is the other buffer of the ping-pong, other rows still gather x.
template <bool DOT, bool FULL = false, int STEP = 0>
__global__ void __launch_bounds__(256)
k_bd_apply(int64_t n, int64_t n_slices, const int64_t *__restrict__ base, int64_t entries, const uint32_t *__restrict__ col, const double *__restrict__ val,
           const uint8_t *__restrict__ ground, double gdiag, const double2 *__restrict__ x, double2 *__restrict__ y, double *__restrict__ xy, BdStep st)
{
    constexpr int U = 9; // entries in flight per lane: 4 · U loads, then U gathers (first-order rows: 9, 15, 27 entries)
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    double acc = 0.0;
    for (int64_t slice = wave0; slice < n_slices; slice += nwaves) {
        const int64_t b0 = base[slice]; // wave-uniform: scalar loads
        const int W = (int)((base[slice + 1] - b0) >> 6);
        const int64_t row = slice * 64 + lane;
        const bool ok = row < n;
        const uint32_t *cs = col + b0 + lane;
        const double *v11 = val + b0 + lane, *v12 = v11 + entries, *v21 = FULL ? v12 + entries : v12, *v22 = v21 + entries;
        double ym = 0.0, ye = 0.0;
        for (int k0 = 0; k0 < W; k0 += U) {
            uint32_t c[U];
            double a11[U], a12[U], a21[U], a22[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const bool on = k0 + j < W; // wave-uniform
                const int64_t o = 64 * (int64_t)(on ? k0 + j : k0);
                c[j] = cs[o];
                a11[j] = on ? __builtin_nontemporal_load(v11 + o) : 0.0;
                a12[j] = on ? __builtin_nontemporal_load(v12 + o) : 0.0;
                if constexpr (FULL) a21[j] = on ? __builtin_nontemporal_load(v21 + o) : 0.0;
                a22[j] = on ? __builtin_nontemporal_load(v22 + o) : 0.0;
            }
            double2 xv[U];
#pragma unroll
            for (int j = 0; j < U; ++j) xv[j] = x[FULL ? c[j] : c[j] & ~BD_GROUNDED];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const double xm = xv[j].x, xe = (!FULL && (c[j] & BD_GROUNDED)) ? 0.0 : xv[j].y;
                ym += a11[j] * xm; ym += a12[j] * xe;
                ye += (FULL ? a21[j] : a12[j]) * xm; ye += a22[j] * xe;
            }
        }
        if (ok) {
            const double2 xr = x[row];
            if constexpr (!FULL)
                if (ground[row]) ye = gdiag * xr.y; // an eliminated φₑ row: the diagonal alone
            if constexpr (STEP == 0) {
                y[row] = make_double2(ym, ye);
                if constexpr (DOT) acc += xr.x * ym + xr.y * ye;
            } else {
                const double2 rr = st.r[row];
                const double2 g = bd_precondition(st.binv, row, make_double2(rr.x - ym, rr.y - ye));
                double2 di = make_double2(st.c2 * g.x, st.c2 * g.y);
                if constexpr (STEP == 2) { const double2 dp = st.d[row]; di.x += st.c1 * dp.x; di.y += st.c1 * dp.y; }
                st.d[row] = di;
                y[row] = make_double2(xr.x + di.x, xr.y + di.y);
            }
        }
    }
    if constexpr (DOT) block_sum_slots(acc, xy);
}

// the fine level's product (tb_bidomain.hip and the finest level of the cycle)
template <bool DOT>
static void enqueue_apply(tb_bidomain *h, const double *x, double *y, double *xy)
{
    hipLaunchKernelGGL((k_bd_apply<DOT>), dim3((unsigned)((h->n_slices + 3) / 4)), dim3(256), 0, h->pat->mesh->dev->stream, h->n, h->n_slices, h->d_base, h->entries, h->d_col,
                       h->d_val, h->d_ground, h->ground_diag, (const double2 *)x, (double2 *)y, xy, BdStep());
}

} // namespace tb

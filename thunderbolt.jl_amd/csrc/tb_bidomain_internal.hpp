// tb_bidomain_internal.hpp — what tb_bidomain.hip shares with tb_bidomain_mg.hip and tb_bidomain_amg.hip (the multigrid preconditioners of the block system):
// the block system's record, the sliced block product with its two storage variants and its smoother epilogue, the 2 × 2 block preconditioner of one
// node, and the level record, smoother, λmax estimate and conjugate gradients of a block cycle.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "tb_internal.h"
#include "tb_mg_internal.hpp"
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

// ---- what the two multigrid preconditioners of the block system share (tb_bidomain_mg.hip: nested hexahedral grids; tb_bidomain_amg.hip: smoothed
// aggregation).  The kernels live in tb_bidomain_mg.hip behind the functions below.
constexpr int BD_COARSEST_NODES = MG_COARSEST_MAX / 2; // 512 nodes, 1 024 unknowns: the dense inverse of tb_multigrid.hip

// a level of a block cycle
struct BdMgLevel {
    tb_pattern *pat = nullptr;       // the level's scalar pattern (geometric levels and the finest level)
    int64_t n = 0, nnz = 0, n_slices = 0, entries = 0;
    bool fine = false;               // the finest level: products run on the block system's own three planes and flags
    const uint8_t *ground = nullptr; // what the kernels read (finest: the block system's flags)
    uint8_t *d_ground = nullptr;     // owned, below the finest level
    double *d_csr = nullptr;         // 4 · nnz: planes a₁₁, a₁₂, a₂₁, a₂₂ in the pattern's CSR order, elimination baked in
    int64_t *d_base = nullptr;       // sliced storage of the smoothed levels below the finest (the finest level's is the block system's)
    uint32_t *d_col = nullptr;
    double *d_val = nullptr;         // 4 · entries
    double *d_binv = nullptr;        // 3 n: inverse diagonal blocks, zero in the φₑ row and column of a grounded node
    double *d_vec = nullptr;         // d | w | xt | x | r, 2n each (the Lanczos estimate of set-up borrows all five)
    double *d = nullptr, *w = nullptr, *xt = nullptr, *x = nullptr, *r = nullptr;
    double lmax = 0.0;
};

// what the smoother, the λmax estimate and the solve need of the hierarchy they run in
struct BdCycle {
    tb_bidomain *bd;
    tb_device *dev;
    int degree;
    double ratio;
    bool split;     // product + vector kernel per smoothing step (profiling build of the geometric cycle)
    double *d_scal; // 8 scalars
    double *d_part; // one partial per workgroup of the ordered reductions (8 · CUs)
    double *d_ws;   // z, p, Ap, r of the solve (2n each)
};

// base[s] = first value slot of slice s (64 rows, 64 · the widest row of the slice): n_slices + 1 entries
inline void bd_slice_table(int64_t n, const int64_t *rowptr, std::vector<int64_t> &base)
{
    const int64_t n_slices = (n + 63) / 64;
    base.assign((size_t)n_slices + 1, 0);
    for (int64_t s = 0; s < n_slices; ++s) {
        int64_t w = 0;
        for (int64_t r = 64 * s; r < std::min<int64_t>(n, 64 * s + 64); ++r) w = std::max(w, rowptr[r + 1] - rowptr[r]);
        base[(size_t)s + 1] = base[(size_t)s] + 64 * w;
    }
}

void bd_level_product(const BdCycle &cy, const BdMgLevel &L, int step, const double *x, double *y, const BdStep &st); // y = 𝒜_l x (step 0) or a fused smoother step (1, 2)
void bd_smooth(const BdCycle &cy, BdMgLevel &L, const double *r, double *&cur, double *&other, bool from_zero);      // `degree` Chebyshev steps on B⁻¹𝒜_l
int bd_lambda_max(const BdCycle &cy, BdMgLevel &L, const char *who, int l, double *out);                              // 1.05 × the Lanczos estimate of λmax(B⁻¹𝒜_l); reads back
// CG on 𝒜x = b with z = ℳ⁻¹r from `cycle` (enqueue-only); `who` names the entry in the not-positive-definite report
int bd_pcg(const BdCycle &cy, const char *who, void (*cycle)(void *ctx, const double *r, double *z), void *ctx, const double *b, double *x, double rtol, double atol, int maxiter,
           int *iters, double *resnorm);
void launch_bd_csr_fine(tb_bidomain *bd, double *csr);    // the block system's planes → 4 CSR planes with the elimination baked in, ground_diag on the eliminated φₑφₑ diagonals
void launch_bd_binv_fine(tb_bidomain *bd, double *binv);  // the block system's block inverses with the ground masked
void launch_bd_fill_sliced(tb_device *dev, const BdMgLevel &L, const int64_t *rowptr, const int32_t *colidx); // CSR planes → sliced planes, columns, block inverses
void launch_bd_dense_inverse(tb_device *dev, int n, const int64_t *rowptr, const int32_t *colidx, int64_t nnz, const double *csr, double *C); // C = 𝒜⁻¹, n ≤ BD_COARSEST_NODES

} // namespace tb

// tb_spmv.hip — everything that computes a product with a device CSR matrix, and every plan a product needs:
//   y = α·A·x + β·y                   src/utils.jl:185-231  (`b = M uₙ₋₁`, src/solver/time/euler.jl:85): launch_spmv
//   y = A·x with xᵀy on the way       the pᵀAp of every CG form (tb_krylov.hip): launch_spmv_dot_slots, launch_spmv_dot folds the sum
//   listed rows of a product          interface rows of the multi-GPU path: launch_spmv_rows
//   the diagonal and its inverse      Jacobi preconditioner: launch_extract_diagonal, launch_extract_inverse_diagonal
// Kernels: lanes-per-row CSR (k_spmv, k_spmv_dot), the stream pair (CSR rows, signature rows), 3×3 blocks (k_spmv_b3), the sliced mirror.  Plans
// (3×3 blocks, row runs, signatures, mirror slices, diagonal positions) are planned on the host by tb_spmv_planners.cpp and uploaded here at a
// pattern's first product; select_product is the one place that plans and names the kernel of a product.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "tb_internal.h"
#include "tb_reduce.hpp"
#include "tb_spmv_planners.hpp"

namespace tb {

static plan::PatternView view(const tb_pattern *p) { return {p->n_rows, p->h_rowptr.data(), p->h_colidx.data(), p->max_row_len}; }

// CSR SpMV, LANES lanes per row (FE rows hold ~27 nz): row-contiguous reads of nzval / colidx
template <int LANES>
__global__ void __launch_bounds__(256)
k_spmv(int64_t nrows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz,
       const double *__restrict__ x, double alpha, double beta, double *__restrict__ y)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = threadIdx.x % LANES;
    const int64_t nsub = ((int64_t)gridDim.x * blockDim.x) / LANES;
    for (int64_t r = gid / LANES; r < nrows; r += nsub) {
        const int64_t k0 = rowptr[r], k1 = rowptr[r + 1];
        double v = 0.0;
        for (int64_t k = k0 + sub; k < k1; k += LANES) v += nz[k] * x[colidx[k]];
#pragma unroll
        for (int o = LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LANES);
        if (sub == 0) y[r] = beta == 0.0 ? alpha * v : alpha * v + beta * y[r];
    }
}

// CSR "stream" SpMV, row-per-lane form (patterns whose rows share no signatures, and TB_SPMV_KERNEL=rows).  A workgroup owns a run of consecutive rows
// holding ≤ CAP − 2 non-zeros, one 16-byte record {first row, rows | entries << 16, first nz} per run, the record of the NEXT run requested at the top of the
// current one.  The entries of the run are parked in LDS as they come (values and columns, every lane busy and fully coalesced: lane i takes entry i,
// whatever row it belongs to), and the products are taken row-wise: three lanes per row, lane (row, s) the entries s, s + 3, …, so the lanes of a wave — 21
// consecutive rows — gather x at three stencil offsets of 21 consecutive rows: a few cache lines per instruction on FE numberings.  (Taking the products
// entry-wise instead makes the 64 gathers of one instruction follow 2.4 rows through all their columns, ≈ 21 scattered 24-byte pieces: DESIGN.md, "SpMV forms
// that lost".)  Row sums stay in registers (no product array, no second LDS pass), the three partial sums meet by two lane shifts, y is stored by the lanes
// s = 0.  The entry loads are unconditional but for the wave-uniform len > 0, their indices clamped into the run: a load inside `if (i < len)` is followed
// by its own wait, which makes the U entry / column pairs of a lane 2·U trips one after the other.  DOT: also accumulates
// xᵀy (the pᵀAp of CG) into the slot group xy.
template <int CAP, bool DOT>
__global__ void __launch_bounds__(256)
k_spmv_stream_rows(int n_blk, const uint4 *__restrict__ blkrec, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz,
                   const double *__restrict__ x, double alpha, double beta, double *__restrict__ y, double *__restrict__ xy)
{
    __shared__ double s_v[CAP];
    __shared__ int32_t s_c[CAP];
    constexpr int U = CAP / 256, SUB = 3, RW = 21, RP = 4 * RW, NK = 9; // 21 rows per wave (lane 63 idle): no row triple straddles two waves
    const int tid = threadIdx.x, lane = tid & 63, rl = RW * (tid >> 6) + lane / SUB, sub = lane % SUB;
    const bool lane_ok = lane < SUB * RW;
    double acc = 0.0;
    int b = blockIdx.x;
    uint4 rec = blkrec[b < n_blk ? b : 0];
    for (; b < n_blk; b += gridDim.x) {
        const int bn = b + gridDim.x;
        const uint4 recn = blkrec[bn < n_blk ? bn : b];
        const int r0 = (int)rec.x, nr = (int)(rec.y & 0xffffu), len = (int)(rec.y >> 16);
        const int64_t k0 = (int64_t)(((uint64_t)rec.w << 32) | rec.z);
        const int rc0 = rl < nr ? rl : nr - 1;
        const int64_t pa0 = rowptr[r0 + rc0], pe0 = rowptr[r0 + rc0 + 1];
        const double *nzb = nz + k0;
        const int32_t *cb = colidx + k0;
        int32_t cj[U];
        double vj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = tid + u * 256, ic = i < len ? i : len - 1;
            cj[u] = 0; vj[u] = 0.0;
            if (len > 0) { cj[u] = cb[ic]; vj[u] = nzb[ic]; } // wave-uniform condition
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = tid + u * 256;
            if (i < len) { s_c[i] = cj[u]; s_v[i] = vj[u]; }
        }
        __syncthreads();
        for (int p0 = 0; p0 < nr; p0 += RP) {
            const int r = rl + p0;
            const bool active = lane_ok && r < nr && len > 0;
            int64_t pa = pa0, pe = pe0;
            if (p0 > 0) { const int rc = r < nr ? r : nr - 1; pa = rowptr[r0 + rc]; pe = rowptr[r0 + rc + 1]; } // runs of short rows
            const int a = (int)(pa - k0), e = (int)(pe - k0);
            int kc[NK], cc[NK];
            double vv[NK], xx[NK];
#pragma unroll
            for (int t_ = 0; t_ < NK; ++t_) {
                const int k = a + sub + SUB * t_;
                kc[t_] = active && k < e ? k : -1;
                const int kk = kc[t_] >= 0 ? kc[t_] : 0;
                cc[t_] = s_c[kk]; vv[t_] = s_v[kk];
            }
#pragma unroll
            for (int t_ = 0; t_ < NK; ++t_) xx[t_] = len > 0 ? x[cc[t_]] : 0.0;
            double v = 0.0;
#pragma unroll
            for (int t_ = 0; t_ < NK; ++t_) v += kc[t_] >= 0 ? vv[t_] * xx[t_] : 0.0;
            if (active) for (int k = a + sub + SUB * NK; k < e; k += SUB) v += s_v[k] * x[s_c[k]]; // rows longer than 27 entries
            v += __shfl_down(v, 1, 64) + __shfl_down(v, 2, 64);
            if (active && sub == 0) {
                if constexpr (DOT) { y[r0 + r] = v; acc += x[r0 + r] * v; }
                else y[r0 + r] = beta == 0.0 ? alpha * v : alpha * v + beta * y[r0 + r];
            }
        }
        __syncthreads();
        rec = recn;
    }
    if constexpr (DOT) block_sum_slots(acc, xy); // xy: a slot group (tb_reduce.hpp)
}

// Index-compressed form of k_spmv_stream_rows (default when the pattern compresses).  On a finite-element numbering almost every row holds the same
// column offsets relative to its own index — the 27-point stencil of a hexahedral mesh: one signature covers 97 % of the rows at 216³, the boundary
// layers of the first-visit numbering add ≈ 10⁵ more — so the 4 B column index per non-zero is redundant: a row carries the position of its
// signature in a table (4 B per row; the table is a few MB and stays in L2), the kernel streams 8 B per non-zero instead of 12 and parks values
// only in LDS.  Runs and records, lane mapping (three lanes per row, 21 rows per wave), order of the products and of the partial sums are those of
// k_spmv_stream_rows: the two kernels give identical bits.  Same interface (tb_spmv_csr: the plan is built with the pattern's first product); patterns
// that do not compress keep the CSR kernel.
template <int CAP, bool DOT>
__global__ void __launch_bounds__(256)
k_spmv_sig_rows(int n_blk, const uint4 *__restrict__ blkrec, const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ rowsig, const int32_t *__restrict__ sigoff,
                const double *__restrict__ nz, int64_t nnz, const double *__restrict__ x, double alpha, double beta, double *__restrict__ y, double *__restrict__ xy)
{
    __shared__ double2 s_v2[CAP / 2 + 1];
    double *s_v = (double *)s_v2;
    constexpr int U = CAP / 512, SUB = 3, RW = 21, RP = 4 * RW, NK = 9; // 21 rows per wave (lane 63 idle): no row triple straddles two waves
    const int tid = threadIdx.x, lane = tid & 63, rl = RW * (tid >> 6) + lane / SUB, sub = lane % SUB;
    const bool lane_ok = lane < SUB * RW;
    const int G = gridDim.x;
    double acc = 0.0;
    // column offsets of the wave's current signature, lane (row, sub) holding entries sub, sub + 3, …: re-read from the table only when a pass meets
    // another signature (97 % of the rows of a hexahedral mesh carry the interior stencil, so almost never)
    int of[NK];
    uint32_t cur = 0xFFFFFFFFu;
#pragma unroll
    for (int t_ = 0; t_ < NK; ++t_) of[t_] = 0;
    // A run costs two dependent trips to memory — its values (+ the row offsets and signatures of its first pass), then the gather of x — and the
    // kernel is bound by them, not by bytes (8 µs per run and workgroup at 216³ with 12 B or 8 B per non-zero alike).  The values of the NEXT run
    // are therefore requested while the current one is multiplied: records two runs ahead, values one run ahead (16 bytes per lane from the
    // 16-byte boundary at or below the run's first entry — 8-byte loads stream at ≈ 0.6 of that rate —, the run then sits in LDS shifted by
    // o = k0 & 1, its entry e at s_v[e + o]; the launcher guarantees a 16-byte aligned nz and runs of at most CAP − 2 entries; the one pair that
    // would reach past the array (odd nnz) is read as a single value).
    auto request = [&](const uint4 &rc, bool live, double2(&v)[U], int64_t &pa, int64_t &pe, uint32_t &sg) {
        const int r0 = (int)rc.x, nr = (int)(rc.y & 0xffffu), len = (int)(rc.y >> 16);
        const int64_t k0 = (int64_t)(((uint64_t)rc.w << 32) | rc.z);
        const int rc0 = rl < nr ? rl : nr - 1;
        pa = pe = 0; sg = 0;
        if (live) { pa = rowptr[r0 + rc0]; pe = rowptr[r0 + rc0 + 1]; sg = rowsig[r0 + rc0]; }
        const int64_t ka = k0 - (k0 & 1);
        const int npairs = (len + (int)(k0 & 1) + 1) >> 1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = tid + u * 256;
            v[u] = make_double2(0.0, 0.0);
            if (live && i < npairs) {
                if (ka + 2 * (int64_t)i + 1 < nnz) v[u] = *(const double2 *)(nz + ka + 2 * (int64_t)i);
                else v[u].x = nz[ka + 2 * (int64_t)i];
            }
        }
    };
    int b = blockIdx.x;
    uint4 rec = blkrec[b < n_blk ? b : 0];
    uint4 recn = blkrec[b + G < n_blk ? b + G : 0];
    double2 vj[U];
    int64_t pa0, pe0;
    uint32_t sg0;
    request(rec, b < n_blk, vj, pa0, pe0, sg0);
    for (; b < n_blk; b += G) {
        const uint4 recnn = blkrec[b + 2 * G < n_blk ? b + 2 * G : 0];
        const int r0 = (int)rec.x, nr = (int)(rec.y & 0xffffu), len = (int)(rec.y >> 16);
        const int64_t k0 = (int64_t)(((uint64_t)rec.w << 32) | rec.z);
        const int o = (int)(k0 & 1);
        const int npairs = (len + o + 1) >> 1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = tid + u * 256;
            if (i < npairs) s_v2[i] = vj[u];
        }
        __syncthreads();
        double2 vjn[U];
        int64_t pa0n = 0, pe0n = 0;
        uint32_t sg0n = 0;
        for (int p0 = 0; p0 < nr; p0 += RP) {
            const int r = rl + p0;
            const bool active = lane_ok && r < nr && len > 0;
            int64_t pa = pa0, pe = pe0;
            uint32_t sg = sg0;
            const int rc = r < nr ? r : nr - 1;
            if (p0 > 0) { pa = rowptr[r0 + rc]; pe = rowptr[r0 + rc + 1]; sg = rowsig[r0 + rc]; } // runs of short rows
            const int a = (int)(pa - k0) + o, n = (int)(pe - pa), row = r0 + rc;
            {
                const uint32_t sg1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)sg);
                const bool uniform = __ballot(sg != sg1) == 0ull; // every lane carries a valid row's signature (rc is clamped)
                if (!uniform || sg1 != cur) {
#pragma unroll
                    for (int t_ = 0; t_ < NK; ++t_) { const int k = sub + SUB * t_; of[t_] = sigoff[sg + (k < n ? k : 0)]; }
                    cur = uniform ? sg1 : 0xFFFFFFFFu;
                }
            }
            int kc[NK], cc[NK];
            double vv[NK], xx[NK];
#pragma unroll
            for (int t_ = 0; t_ < NK; ++t_) {
                const int k = sub + SUB * t_;
                kc[t_] = active && k < n ? k : -1;
                const int kk = kc[t_] >= 0 ? kc[t_] : 0;
                cc[t_] = row + (kc[t_] >= 0 ? of[t_] : 0); // masked entries read x[row]
                vv[t_] = s_v[a + kk];
            }
#pragma unroll
            for (int t_ = 0; t_ < NK; ++t_) xx[t_] = len > 0 ? x[cc[t_]] : 0.0;
            if (p0 == 0) request(recn, b + G < n_blk, vjn, pa0n, pe0n, sg0n); // behind the gather in program order: the wait for x does not include these
            double v = 0.0;
#pragma unroll
            for (int t_ = 0; t_ < NK; ++t_) v += kc[t_] >= 0 ? vv[t_] * xx[t_] : 0.0;
            if (active) for (int k = sub + SUB * NK; k < n; k += SUB) v += s_v[a + k] * x[row + sigoff[sg + k]]; // rows longer than 27 entries
            v += __shfl_down(v, 1, 64) + __shfl_down(v, 2, 64);
            if (active && sub == 0) {
                if constexpr (DOT) { y[r0 + r] = v; acc += x[r0 + r] * v; }
                else y[r0 + r] = beta == 0.0 ? alpha * v : alpha * v + beta * y[r0 + r];
            }
        }
        if (nr == 0) request(recn, b + G < n_blk, vjn, pa0n, pe0n, sg0n);
        __syncthreads();
        rec = recn; recn = recnn;
#pragma unroll
        for (int u = 0; u < U; ++u) vj[u] = vjn[u];
        pa0 = pa0n; pe0 = pe0n; sg0 = sg0n;
    }
    if constexpr (DOT) block_sum_slots(acc, xy); // xy: a slot group (tb_reduce.hpp)
}

// Vector fields (3 dofs per node, interleaved): rows 3R, 3R+1, 3R+2 share one set of columns and the columns come in triples, so the matrix
// is a CSR of 3×3 blocks stored row by row.  The block SpMV reads one column index per block (4 B per 9 values instead of 36 B) and gathers
// each x triple once for the three rows: 8.4 B per non-zero instead of 12.  G lanes per node row, each lane one block per pass.
template <int G, bool DOT>
__global__ void __launch_bounds__(256)
k_spmv_b3(int64_t n_brows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ bcol, const double *__restrict__ nz,
          const double *__restrict__ x, double alpha, double beta, double *__restrict__ y, double *__restrict__ xy)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = threadIdx.x % G;
    const int64_t ngroups = ((int64_t)gridDim.x * blockDim.x) / G;
    double acc = 0.0;
    for (int64_t R = gid / G; R < n_brows; R += ngroups) {
        const int64_t k0 = rowptr[3 * R], k1 = rowptr[3 * R + 1], k2 = rowptr[3 * R + 2];
        const int nb = (int)((k1 - k0) / 3);
        const int32_t *bc = bcol + k0 / 9; // the three rows of every node row above have equal lengths: block offset = k0 / 9
        double v0 = 0.0, v1 = 0.0, v2 = 0.0;
        for (int j = sub; j < nb; j += G) {
            const int64_t c = 3 * (int64_t)bc[j];
            const double x0 = x[c], x1 = x[c + 1], x2 = x[c + 2];
            const double *a0 = nz + k0 + 3 * j, *a1 = nz + k1 + 3 * j, *a2 = nz + k2 + 3 * j;
            v0 += a0[0] * x0 + a0[1] * x1 + a0[2] * x2;
            v1 += a1[0] * x0 + a1[1] * x1 + a1[2] * x2;
            v2 += a2[0] * x0 + a2[1] * x1 + a2[2] * x2;
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            v0 += __shfl_xor(v0, o, G);
            v1 += __shfl_xor(v1, o, G);
            v2 += __shfl_xor(v2, o, G);
        }
        if (sub == 0) {
            double *yr = y + 3 * R;
            if constexpr (DOT) {
                yr[0] = v0; yr[1] = v1; yr[2] = v2;
                acc += x[3 * R] * v0 + x[3 * R + 1] * v1 + x[3 * R + 2] * v2;
            } else if (beta == 0.0) {
                yr[0] = alpha * v0; yr[1] = alpha * v1; yr[2] = alpha * v2;
            } else {
                yr[0] = alpha * v0 + beta * yr[0]; yr[1] = alpha * v1 + beta * yr[1]; yr[2] = alpha * v2 + beta * yr[2];
            }
        }
    }
    if constexpr (DOT) block_sum_slots(acc, xy); // xy: a slot group (tb_reduce.hpp)
}

// ---- plans: early return, no capture, environment, planner (tb_spmv_planners.cpp), uploads ------------------------------------------------------
// is the pattern a CSR of 3×3 blocks?  (checked once on the host; b3 = 1 yes / −1 no)
static int block3_plan(tb_pattern *p)
{
    if (p->b3 != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev); // a plan is built (host work + blocking uploads) at its first use: make that use before the capture
    static const bool off = tune_env("TB_SPMV_B3") && atoi(tune_env("TB_SPMV_B3")) == 0;
    p->b3 = -1;
    std::vector<int32_t> bcol;
    if (off || !plan::block3_columns(view(p), bcol)) return TB_OK;
    TB_TRY(upload(p->mesh->dev, bcol, &p->d_bcol));
    const double avg = (double)bcol.size() / (double)(p->n_rows / 3); // blocks per node row: 27 for Q1, 64…125 for Q2
    static const int lanes_env = tune_env("TB_SPMV_B3_LANES") ? atoi(tune_env("TB_SPMV_B3_LANES")) : 0;
    p->b3_lanes = lanes_env ? lanes_env : (avg > 36 ? 32 : 16); // measured: 16 ≈ 32 > 64 on Q2 (24³ contraction solve 4.7 / 4.7 / 5.2 s), 16 best on Q1
    p->b3 = 1;
    return TB_OK;
}

template <bool DOT>
static void launch_b3(tb_pattern *p, const double *nz, const double *x, double alpha, double beta, double *y, double *xy)
{
    tb_device *dev = p->mesh->dev;
    const int64_t nbr = p->n_rows / 3;
#define TB_B3(G) hipLaunchKernelGGL((k_spmv_b3<G, DOT>), dim3(grid_for(dev, nbr * G, 256)), dim3(256), 0, dev->stream, nbr, p->d_rowptr, p->d_bcol, nz, x, alpha, beta, y, xy)
    if (p->b3_lanes == 64) TB_B3(64);
    else if (p->b3_lanes == 32) TB_B3(32);
    else TB_B3(16);
#undef TB_B3
}

// row runs of the stream kernels (plan::row_runs); n_blk = −1 (lanes-per-row kernel instead) if a single row exceeds the capacity
#ifndef TB_SPMV_CAP
#define TB_SPMV_CAP 2048
#endif
constexpr int SPMV_CAP = TB_SPMV_CAP;
static_assert(SPMV_CAP < 65536, "row and entry counts of a run share one 32-bit word");
static int stream_plan(tb_pattern *p)
{
    if (p->n_blk != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev);
    PlanTimer timer("stream_plan");
    std::vector<uint32_t> rec;
    if (!plan::row_runs(view(p), SPMV_CAP, rec)) { p->n_blk = -1; return TB_OK; }
    TB_TRY(upload(p->mesh->dev, rec, &p->d_blkrec));
    p->n_blk = (int64_t)rec.size() / 4;
    return TB_OK;
}

// Signature plan of the index-compressed SpMV (plan::row_signatures), built with the pattern's first product.  The pattern "compresses" when the
// table is at most a quarter of the column array (row length ≤ SPMV_CAP is checked by the stream plan); otherwise n_sig = −1.
// TB_SPMV_KERNEL=rows keeps the CSR rows kernel on a pattern that compresses — read per pattern: tests build one pattern of each kind in one process.
static int sig_plan(tb_pattern *p)
{
    if (p->n_sig != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev);
    PlanTimer timer("sig_plan");
    const char *env = getenv("TB_SPMV_KERNEL");
    plan::SigHost h;
    if ((env && !strcmp(env, "rows")) || !plan::row_signatures(view(p), std::max<int64_t>(p->nnz / 4, 64), h)) { p->n_sig = -1; return TB_OK; }
    TB_TRY(upload_all(p->mesh->dev, h.rowsig, &p->d_rowsig, h.tab, &p->d_sigoff));
    p->n_sig = h.n_sig; p->sig_entries = (int64_t)h.tab.size();
    p->h_rowsig = std::move(h.rowsig); // (the slice table of the mirror marks the slices whose rows share one signature)
    if (getenv("TB_PLAN_VERBOSE"))
        fprintf(stderr, "[tbhip] SpMV signature plan: %lld rows, %lld signatures, table %lld entries (%.4f of the column array)\n", (long long)p->n_rows, (long long)p->n_sig,
                (long long)p->sig_entries, (double)p->sig_entries / (double)std::max<int64_t>(p->nnz, 1));
    return TB_OK;
}

// ---- sliced mirror (tb_spmv_mirror) ----------------------------------------------------------------------------------------------------------
// The Krylov solves multiply one fixed matrix many times, and the CSR order is the wrong order for that on a wide machine: a lane that owns a row
// meets its values 216 bytes apart, so every kernel above parks the run in LDS first (load → LDS → barrier → LDS → product; 0.68 ms at 216³, 3.5
// TB/s).  The mirror stores the same values slice by slice — 64 consecutive rows, entry k of all 64 rows side by side, zero-padded to the longest
// row of the slice — so the product is one coalesced 512-byte load per entry and wave, the x gather, and the sums: no LDS, no barrier (0.47 ms,
// 5 TB/s; scripts/microbench/sell_spmv.hip).  Column offsets come from the row's signature as in k_spmv_sig_rows (scalar loads when the slice
// shares one signature, which is the rule on a hexahedral mesh), and a row's partial sums are formed in that kernel's order — entries k ≡ 0, 1, 2
// (mod 3) ascending, then s₀ + (s₁ + s₂) — so the two products agree bit for bit.  The mirror is a second copy of the values (built in ≈ 1 ms
// at 216³) bound to the array it was taken from: the caller re-binds after changing the matrix (include/tbhip.h).
// The slice records (plan::mirror_slices): a slice of one signature takes its offsets by scalar loads from the signature table; a mixed slice — the two
// ends of a grid line meet in one slice out of three at 216³ — carries them entry-major like the values, so both kinds cost two trips: record → values
// and offsets → x.
static int mirror_plan(tb_pattern *p)
{
    if (p->n_slices != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev);
    PlanTimer timer("mirror_plan");
    TB_TRY(spmv_plans(p));
    const bool have_sig = p->n_sig > 0 && (int64_t)p->h_rowsig.size() == p->n_rows; // a numbering without shared signatures: every slice carries its offsets
    plan::MirrorHost h;
    if (p->b3 > 0 || p->n_rows == 0 || !plan::mirror_slices(view(p), have_sig ? p->h_rowsig.data() : nullptr, h)) { p->n_slices = -1; return TB_OK; }
    MirrorSlice *db = nullptr;
    TB_TRY(upload(p->mesh->dev, h.slices, &db));
    p->d_mir_base = db;
    TB_TRY(upload(p->mesh->dev, h.offs, &p->d_mir_off));
    p->mir_entries = h.entries; p->n_slices = (int64_t)h.slices.size() - 1;
    if (getenv("TB_PLAN_VERBOSE")) {
        int64_t mixed = 0;
        for (int64_t s = 0; s < p->n_slices; ++s) mixed += h.slices[s].sig == MIRROR_MIXED;
        fprintf(stderr, "[tbhip] SpMV mirror plan: %lld slices (%lld of mixed signatures), %lld value slots for %lld non-zeros\n", (long long)p->n_slices, (long long)mixed,
                (long long)h.entries, (long long)p->nnz);
    }
    return TB_OK;
}

// values of one slice, CSR → [k][lane]: the slice's entries are one contiguous range of the value array — copied to LDS coalesced, read back
// transposed (slices wider than the LDS block read their rows directly)
__global__ void __launch_bounds__(256)
k_mirror_fill(int64_t n_rows, int64_t n_slices, const MirrorSlice *__restrict__ slices, const int64_t *__restrict__ rowptr, const double *__restrict__ nz,
              double *__restrict__ mir)
{
    constexpr int CAPW = 64 * 32;
    __shared__ double s[4][CAPW];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t slice = (int64_t)blockIdx.x * 4 + wv;
    if (slice >= n_slices) return; // waves are independent (no workgroup barrier below)
    const int64_t r0 = slice * 64, r1 = r0 + 64 < n_rows ? r0 + 64 : n_rows;
    const int64_t row = r0 + lane < n_rows ? r0 + lane : n_rows - 1;
    const int64_t pa = rowptr[row], k0 = rowptr[r0];
    const int n = r0 + lane < n_rows ? (int)(rowptr[row + 1] - pa) : 0;
    const int total = (int)(rowptr[r1] - k0);
    const int64_t b0 = slices[slice].base;
    const int W = (int)slices[slice].width;
    double *dst = mir + b0 + lane;
    if (total <= CAPW) {
        for (int i0 = 0; i0 < total; i0 += 64 * 8) { // eight loads in flight per lane
            double t[8];
#pragma unroll
            for (int u_ = 0; u_ < 8; ++u_) { const int i = i0 + 64 * u_ + lane; t[u_] = i < total ? __builtin_nontemporal_load(nz + k0 + i) : 0.0; }
#pragma unroll
            for (int u_ = 0; u_ < 8; ++u_) { const int i = i0 + 64 * u_ + lane; if (i < total) s[wv][i] = t[u_]; }
        }
        __builtin_amdgcn_wave_barrier();
        const int a = (int)(pa - k0);
#pragma unroll 9
        for (int k = 0; k < W; ++k) __builtin_nontemporal_store(k < n ? s[wv][a + k] : 0.0, dst + 64 * k);
    } else {
        for (int k = 0; k < W; ++k) dst[64 * k] = k < n ? nz[pa + k] : 0.0;
    }
}

template <bool DOT>
__global__ void __launch_bounds__(256)
k_spmv_mirror(int64_t n_rows, int64_t n_slices, const MirrorSlice *__restrict__ slices, const int32_t *__restrict__ moff, const int32_t *__restrict__ sigoff,
              const double *__restrict__ mir, const double *__restrict__ x, double alpha, double beta, double *__restrict__ y, double *__restrict__ xy)
{
    constexpr int NK = 27;
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    double acc = 0.0;
    for (int64_t slice = wave0; slice < n_slices; slice += nwaves) {
        const MirrorSlice rec = slices[slice]; // wave-uniform: scalar loads
        const int W = (int)rec.width;
        const double *vs = mir + rec.base + lane;
        const int64_t row = slice * 64 + lane;
        const bool ok = row < n_rows;
        const int64_t rc = ok ? row : n_rows - 1; // (lanes past the last row: all their entries are padding)
        double vv[NK], xx[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) vv[k] = k < W ? __builtin_nontemporal_load(vs + 64 * k) : 0.0;
        bool on[NK]; // entry k belongs to the lane's row (k < its length)
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (rec.sig != MIRROR_MIXED) { // 64 rows of one signature: offsets by scalar loads, every row as wide as the slice
#pragma unroll
            for (int k = 0; k < NK; ++k) { on[k] = k < W; xx[k] = on[k] ? x[row + sigoff[rec.sig + k]] : 0.0; }
        } else {
            const int32_t *os = moff + rec.obase + lane;
            int32_t oo[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) oo[k] = k < W ? __builtin_nontemporal_load(os + 64 * k) : MIRROR_NONE;
#pragma unroll
            for (int k = 0; k < NK; ++k) { on[k] = oo[k] != MIRROR_NONE; xx[k] = on[k] ? x[rc + oo[k]] : 0.0; }
        }
#pragma unroll
        for (int t_ = 0; t_ < NK / 3; ++t_) { // (the expressions of k_spmv_sig_rows: identical rounding)
            s0 += on[3 * t_] ? vv[3 * t_] * xx[3 * t_] : 0.0;
            s1 += on[3 * t_ + 1] ? vv[3 * t_ + 1] * xx[3 * t_ + 1] : 0.0;
            s2 += on[3 * t_ + 2] ? vv[3 * t_ + 2] * xx[3 * t_ + 2] : 0.0;
        }
        for (int k = NK; k < W; k += 3) { // rows longer than 27 entries
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (k + j >= W) break;
                const int32_t o = rec.sig != MIRROR_MIXED ? sigoff[rec.sig + k + j] : moff[rec.obase + 64 * (k + j) + lane];
                if (o != MIRROR_NONE) {
                    const double a = vs[64 * (k + j)], b = x[rc + o];
                    if (j == 0) s0 += a * b; else if (j == 1) s1 += a * b; else s2 += a * b;
                }
            }
        }
        const double v = s0 + (s1 + s2);
        if (ok) {
            if constexpr (DOT) { y[row] = v; acc += x[row] * v; }
            else y[row] = beta == 0.0 ? alpha * v : alpha * v + beta * y[row];
        }
    }
    if constexpr (DOT) block_sum_slots(acc, xy); // xy: a slot group (tb_reduce.hpp)
}

int launch_mirror_bind(tb_pattern *p, const double *nz)
{
    tb_device *dev = p->mesh->dev;
    if (!nz) { for (const double *&q : p->mir_nz) q = nullptr; return TB_OK; }
    int rc = mirror_plan(p);
    if (rc) return rc;
    if (p->n_slices <= 0) { set_error("tb_spmv_mirror: this pattern has no sliced mirror (3x3-block rows, or rows longer than 255 entries)"); return TB_ERR_UNSUPPORTED; }
    // the slot already bound to this array (a refresh), else a free one, else the one bound longest ago
    int slot = -1;
    for (int i = 0; i < tb_pattern::MIRRORS; ++i) if (p->mir_nz[i] == nz) slot = i;
    if (slot < 0) for (int i = 0; i < tb_pattern::MIRRORS; ++i) if (!p->mir_nz[i]) { slot = i; break; }
    if (slot < 0) { slot = 0; for (int i = 1; i < tb_pattern::MIRRORS; ++i) if (p->mir_stamp[i] < p->mir_stamp[slot]) slot = i; } // least recently bound OR refreshed
    p->mir_stamp[slot] = ++p->mir_clock;
    if (!p->d_mir[slot]) {
        const size_t bytes = (size_t)p->mir_entries * sizeof(double);
        hipError_t e = hipMalloc((void **)&p->d_mir[slot], bytes);
        if (e != hipSuccess) { set_error("tb_spmv_mirror: value mirror (%zu B): %s", bytes, hipGetErrorString(e)); return TB_ERR_NOMEM; }
    }
    hipLaunchKernelGGL(k_mirror_fill, dim3((unsigned)((p->n_slices + 3) / 4)), dim3(256), 0, dev->stream, p->n_rows, p->n_slices, (const MirrorSlice *)p->d_mir_base, p->d_rowptr, nz,
                       p->d_mir[slot]);
    TB_HIP(hipGetLastError());
    p->mir_nz[slot] = nz;
    return TB_OK;
}

template <bool DOT>
static void launch_mirror(tb_pattern *p, const double *mir, const double *x, double alpha, double beta, double *y, double *xy)
{
    // one slice per wave (measured at 216³: 0.52 ms against 0.57 ms with resident workgroups only).  The fused xᵀAx form was capped at 48 workgroups per CU
    // while every workgroup ended in an atomic on ONE scalar (all 40 000: 0.62 ms); with the partials in reduction slots the cap costs 2–4 % and is gone
    const int64_t grid_env = tune_env("TB_SPMV_MIRROR_GRID") ? atoll(tune_env("TB_SPMV_MIRROR_GRID")) : 0; // (read per launch: sweeps)
    const int64_t cap = grid_env > 0 ? grid_env : (int64_t)1 << 30;
    const unsigned grid = (unsigned)std::min<int64_t>((p->n_slices + 3) / 4, cap);
    hipLaunchKernelGGL((k_spmv_mirror<DOT>), dim3(grid), dim3(256), 0, p->mesh->dev->stream, p->n_rows, p->n_slices, (const MirrorSlice *)p->d_mir_base, p->d_mir_off, p->d_sigoff,
                       mir, x, alpha, beta, y, xy);
}

// lanes-per-row CSR product with xᵀy (patterns with a row longer than a run of the stream kernels); launched with 16 lanes per row, measured best for
// 27-entry rows (0.96 vs 1.03 ms at 216³ with 8)
template <int LANES>
__global__ void __launch_bounds__(256)
k_spmv_dot(int64_t nrows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz,
           const double *__restrict__ x, double *__restrict__ y, double *__restrict__ xy)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = threadIdx.x % LANES;
    const int64_t nsub = ((int64_t)gridDim.x * blockDim.x) / LANES;
    double acc = 0.0;
    for (int64_t r = gid / LANES; r < nrows; r += nsub) {
        const int64_t k0 = rowptr[r], k1 = rowptr[r + 1];
        double v = 0.0;
        for (int64_t k = k0 + sub; k < k1; k += LANES) v += nz[k] * x[colidx[k]];
#pragma unroll
        for (int o = LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LANES);
        if (sub == 0) { y[r] = v; acc += x[r] * v; }
    }
    block_sum_slots(acc, xy); // xy: a slot group
}

int spmv_plans(tb_pattern *p)
{
    int rc = block3_plan(p);
    if (rc || p->b3 > 0) return rc;
    rc = stream_plan(p);
    if (rc || p->n_blk <= 0) { if (p->n_sig == 0) p->n_sig = -1; return rc; }
    return sig_plan(p);
}

// The one selector of every product (launch_spmv, launch_spmv_dot_slots): it builds the plans the product needs at its first use, passes a plan's
// refusal on — inside an open graph capture an unplanned product is refused, nothing is enqueued — and names the kernel: 3×3 blocks, else row runs
// (the mirror bound to this very array, else signature rows where the pattern compresses and the values are 16-byte aligned, else CSR rows), else lanes
// per row (a row longer than a run; TB_SPMV_LANES forces it in the profiling build).
enum class Route { B3, MIRROR, SIG_ROWS, CSR_ROWS, LANES };
struct Product { Route route; int arg; }; // arg: MIRROR: the slot; LANES: TB_SPMV_LANES (0: unset)
static int select_product(tb_pattern *p, const double *nz, Product &out)
{
    static const int lanes = tune_env("TB_SPMV_LANES") ? atoi(tune_env("TB_SPMV_LANES")) : 0;
    out = Product{Route::LANES, lanes};
    if (lanes != 0) return TB_OK;
    TB_TRY(block3_plan(p));
    if (p->b3 > 0) { out.route = Route::B3; return TB_OK; }
    TB_TRY(stream_plan(p));
    if (p->n_blk <= 0) return TB_OK;
    for (int i = 0; i < tb_pattern::MIRRORS; ++i)
        if (p->mir_nz[i] == nz && nz) { out = Product{Route::MIRROR, i}; return TB_OK; }
    out.route = Route::CSR_ROWS;
    if (((uintptr_t)nz & 15) == 0) { TB_TRY(sig_plan(p)); if (p->n_sig > 0) out.route = Route::SIG_ROWS; }
    return TB_OK;
}

template <bool DOT>
static void launch_product(tb_pattern *p, const Product &pr, const double *nz, const double *x, double alpha, double beta, double *y, double *xy)
{
    tb_device *dev = p->mesh->dev;
    switch (pr.route) {
    case Route::B3: launch_b3<DOT>(p, nz, x, alpha, beta, y, xy); break;
    case Route::MIRROR: launch_mirror<DOT>(p, p->d_mir[pr.arg], x, alpha, beta, y, xy); break;
    case Route::SIG_ROWS: { // 16 KB of LDS per workgroup
        // persistent: exactly the workgroups that are resident together (the runs are dealt round-robin, every workgroup gets the same share ± 1)
        static int per_cu = 0;
        if (!per_cu) {
            if (tune_env("TB_SPMV_WG_PER_CU")) per_cu = atoi(tune_env("TB_SPMV_WG_PER_CU"));
            if (per_cu <= 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_spmv_sig_rows<SPMV_CAP, DOT>, 256, 0) != hipSuccess || per_cu <= 0)) per_cu = 3;
        }
        const unsigned gmax = (unsigned)(dev->n_cu * per_cu);
        hipLaunchKernelGGL((k_spmv_sig_rows<SPMV_CAP, DOT>), dim3(std::min<unsigned>((unsigned)p->n_blk, gmax)), dim3(256), 0, dev->stream, (int)p->n_blk, (const uint4 *)p->d_blkrec,
                           p->d_rowptr, p->d_rowsig, p->d_sigoff, nz, (int64_t)p->nnz, x, alpha, beta, y, xy);
        break;
    }
    case Route::CSR_ROWS: { // 24 KB of LDS per workgroup: six resident per CU
        static const int64_t cap = tune_env("TB_SPMV_GRID") ? atoi(tune_env("TB_SPMV_GRID")) : 2048; // 256 CUs × 8 resident workgroups
        hipLaunchKernelGGL((k_spmv_stream_rows<SPMV_CAP, DOT>), dim3((unsigned)std::min<int64_t>(std::min<int64_t>(p->n_blk, cap), 1536)), dim3(256), 0, dev->stream, (int)p->n_blk,
                           (const uint4 *)p->d_blkrec, p->d_rowptr, p->d_colidx, nz, x, alpha, beta, y, xy);
        break;
    }
    case Route::LANES: // 16 lanes per row unless the profiling build says otherwise (the xᵀy form has the one instance)
#define TB_SPMV(LN) hipLaunchKernelGGL(k_spmv<LN>, dim3(grid_for(dev, p->n_rows * LN, 256)), dim3(256), 0, dev->stream, p->n_rows, p->d_rowptr, p->d_colidx, nz, x, alpha, beta, y)
        if constexpr (DOT) hipLaunchKernelGGL(k_spmv_dot<16>, dim3(grid_for(dev, p->n_rows * 16, 256)), dim3(256), 0, dev->stream, p->n_rows, p->d_rowptr, p->d_colidx, nz, x, y, xy);
        else switch (pr.arg) {
        case 2: TB_SPMV(2); break;
        case 4: TB_SPMV(4); break;
        case 8: TB_SPMV(8); break;
        case 32: TB_SPMV(32); break;
        default: TB_SPMV(16);
        }
#undef TB_SPMV
        break;
    }
}

int launch_spmv(tb_pattern *p, const double *nz, const double *x, double alpha, double beta, double *y)
{
    Product pr;
    TB_TRY(select_product(p, nz, pr));
    launch_product<false>(p, pr, nz, x, alpha, beta, y, nullptr);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

// y = A x with the partials of xᵀy left in a slot group: the product of launch_cg and of the distributed CG forms
int launch_spmv_dot_slots(tb_pattern *pat, const double *A, const double *x, double *y, double *d_dot /* a slot group */)
{
    if (pat->n_rows == 0) return TB_OK;
    Product pr;
    TB_TRY(select_product(pat, A, pr));
    launch_product<true>(pat, pr, A, x, 1.0, 0.0, y, d_dot);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

// y = A x and *d_dot += xᵀy: the kernels leave the sum in slot group 0, one wave folds it into the caller's scalar
int launch_spmv_dot(tb_pattern *pat, const double *A, const double *x, double *y, double *d_dot)
{
    if (pat->n_rows == 0) return TB_OK;
    tb_device *dev = pat->mesh->dev;
    int rc = launch_spmv_dot_slots(pat, A, x, y, red_group(dev, 0));
    if (rc) return rc;
    fold_slots(dev, 0, d_dot, 1);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

// out[k] = Σ_j A[rows[k], j] x[j]: 16 lanes per listed row
__global__ void __launch_bounds__(256)
k_spmv_rows(int64_t n, const int32_t *__restrict__ rows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz,
            const double *__restrict__ x, double *__restrict__ out)
{
    constexpr int LN = 16;
    const int sub = threadIdx.x % LN;
    const int64_t nsub = ((int64_t)gridDim.x * blockDim.x) / LN;
    for (int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / LN; k < n; k += nsub) {
        const int32_t r = rows[k];
        double v = 0.0;
        for (int64_t e = rowptr[r] + sub; e < rowptr[r + 1]; e += LN) v += nz[e] * x[colidx[e]];
#pragma unroll
        for (int o = LN / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LN);
        if (sub == 0) out[k] = v;
    }
}

int launch_spmv_rows(tb_pattern *p, const double *nz, const double *x, int64_t n, const int32_t *rows, double *out)
{
    tb_device *dev = p->mesh->dev;
    if (n > 0) hipLaunchKernelGGL(k_spmv_rows, dim3(grid_for(dev, n * 16, 256)), dim3(256), 0, dev->stream, n, rows, p->d_rowptr, p->d_colidx, nz, x, out);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

// D⁻¹ for the Jacobi preconditioner: the position of each row's diagonal entry is a property of the pattern, found once on the host
// (scanning the rows on the device, one thread per row, cost 1.7 ms per solve at 216³ — more than a CG iteration); −1 = no diagonal stored
template <bool INVERT>
__global__ void __launch_bounds__(256)
k_extract_diag(int64_t nrows, const int64_t *__restrict__ diagpos, const double *__restrict__ nz, double *__restrict__ dinv)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const int64_t k = diagpos[r];
    if constexpr (INVERT) dinv[r] = 1.0 / (k >= 0 ? nz[k] : 1.0);
    else dinv[r] = k >= 0 ? nz[k] : 0.0;
}

template <bool INVERT>
static int launch_extract_diag(tb_pattern *p, const double *nz, double *dinv)
{
    tb_device *dev = p->mesh->dev;
    if (!p->d_diagpos) {
        TB_NO_CAPTURE(dev);
        TB_TRY(upload(dev, plan::diagonal_positions(view(p)), &p->d_diagpos));
    }
    if (p->n_rows == 0) return TB_OK;
    hipLaunchKernelGGL(k_extract_diag<INVERT>, dim3((unsigned)((p->n_rows + 255) / 256)), dim3(256), 0, dev->stream, p->n_rows, p->d_diagpos, nz, dinv);
    TB_HIP(hipGetLastError());
    return TB_OK;
}
int launch_extract_diagonal(tb_pattern *p, const double *nz, double *diag) { return launch_extract_diag<false>(p, nz, diag); }
int launch_extract_inverse_diagonal(tb_pattern *p, const double *nz, double *dinv) { return launch_extract_diag<true>(p, nz, dinv); }

} // namespace tb

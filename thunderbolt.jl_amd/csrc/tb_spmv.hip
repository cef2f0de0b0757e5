// tb_spmv.hip — everything that computes a product with a device CSR matrix, and every plan a product needs:
//   y = α·A·x + β·y                   src/utils.jl:185-231  (`b = M uₙ₋₁`, src/solver/time/euler.jl:85): launch_spmv
//   y = A·x with xᵀy on the way       the pᵀAp of every CG form (tb_krylov.hip): launch_spmv_dot_slots picks the kernel, launch_spmv_dot folds the sum
//   listed rows of a product          interface rows of the multi-GPU path: launch_spmv_rows
//   the diagonal and its inverse      Jacobi preconditioner: launch_extract_diagonal, launch_extract_inverse_diagonal
// Kernels: lanes-per-row CSR (k_spmv, k_spmv_dot), the stream family (chain / rec / rows / signature rows / wave), 3×3 blocks (k_spmv_b3), the
// sliced mirror.  Plans (3×3 blocks, row runs, signatures, wave runs, mirror slices) are built on the host at a pattern's first product.
#include <hip/hip_runtime.h>

#include <unordered_map>

#include <cmath>
#include <cstring>

#include "tb_internal.h"
#include "tb_reduce.hpp"

namespace tb {

// TB_SPMV_KERNEL: the product library honours "rows" only — the CSR rows kernel, which is also what a pattern without shared row signatures runs (the
// switch lets a test put it on a compressible pattern and compare bits); the older entry-per-lane kernels ("rec", "chain") and the wave-private form
// ("wave", measured slower on thin slabs) are comparison builds: profiling library only
static const char *spmv_kernel_env()
{
    const char *e = getenv("TB_SPMV_KERNEL");
#ifndef TB_ABLATION
    if (e && strcmp(e, "rows") != 0 && strcmp(e, "sig") != 0) return nullptr;
#endif
    return e;
}

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

// CSR "stream" SpMV: a workgroup owns a run of consecutive rows holding ≤ CAP non-zeros.  Phase 1 streams nzval / colidx of the whole run with
// every lane busy and fully coalesced (lane i takes entry i, whatever row it belongs to), gathers x and parks the products in LDS; phase 2 sums
// each row's segment with 8 lanes.  Against the lanes-per-row kernel (27-entry rows fill 27 of 32 lane slots and issue two dependent passes)
// this keeps CAP/256 independent loads in flight per lane.  DOT: also accumulates xᵀy (the pᵀAp of CG) into *xy.
template <int CAP, bool DOT>
__global__ void __launch_bounds__(256)
k_spmv_stream(int n_blk, const int32_t *__restrict__ blkrow, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz,
              const double *__restrict__ x, double alpha, double beta, double *__restrict__ y, double *__restrict__ xy)
{
    __shared__ double s[CAP];
    constexpr int LN = 8;
    const int sub = threadIdx.x % LN;
    double acc = 0.0;
    for (int b = blockIdx.x; b < n_blk; b += gridDim.x) {
        const int r0 = blkrow[b], r1 = blkrow[b + 1];
        const int64_t k0 = rowptr[r0];
        const int len = (int)(rowptr[r1] - k0);
        const double *nzb = nz + k0;
        const int32_t *cb = colidx + k0;
#pragma unroll
        for (int u = 0; u < CAP / 256; ++u) {
            const int i = threadIdx.x + u * 256;
#ifdef TB_SPMV_NT
            if (i < len) s[i] = __builtin_nontemporal_load(nzb + i) * x[__builtin_nontemporal_load(cb + i)];
#else
            if (i < len) s[i] = nzb[i] * x[cb[i]];
#endif
        }
        __syncthreads();
        for (int r = r0 + threadIdx.x / LN; r < r1; r += 256 / LN) {
            const int a = (int)(rowptr[r] - k0), e = (int)(rowptr[r + 1] - k0);
            double v = 0.0;
            for (int i = a + sub; i < e; i += LN) v += s[i];
#pragma unroll
            for (int o = LN / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LN);
            if (sub == 0) {
                if constexpr (DOT) { y[r] = v; acc += x[r] * v; }
                else y[r] = beta == 0.0 ? alpha * v : alpha * v + beta * y[r];
            }
        }
        __syncthreads();
    }
    if constexpr (DOT) block_sum_slots(acc, xy); // xy: a slot group (tb_reduce.hpp)
}

#ifdef TB_ABLATION
__device__ int g_spmv_nogather = 0;
#endif
// The same kernel with the dependent trips of a block cut from five to two.  Above, a block walks block → row range → row pointers → entries → x,
// and after the barrier every row group loads its two row pointers again: with eight resident workgroups per CU the waves sit in metadata trips four
// fifths of the time.  Here a block is ONE 16-byte record {first row, rows | entries << 16, first nz} whose load for the NEXT block is issued at the top
// of the current one, and the row offsets of the first three passes of phase 2 are requested together with the entries (NPRE·32 rows: every row of
// a 27-entries-per-row block), so a block costs record (hidden) → entries + offsets → x.  What is left is the gather itself: a profiling build that reads x
// coalesced instead runs at 0.57 instead of 0.81 ms at 216³.  A windowed form (x of the block's ≈ 9 runs of consecutive columns copied into LDS, 16-bit
// window positions instead of 32-bit columns, 10 B per entry) was built and is correct, but not faster: 0.74–0.75 ms against 0.73 ms on the same box with
// register staging (run scan by readlane, LDS gather, a third barrier, four workgroups per CU), 0.98 ms with LDS-DMA staging (hipcc 7.2 follows every
// `global_load_lds` in a loop by `s_waitcnt vmcnt(0)`); removed again.
template <int CAP, bool DOT>
__global__ void __launch_bounds__(256)
k_spmv_stream_rec(int n_blk, const uint4 *__restrict__ blkrec, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz,
                  const double *__restrict__ x, double alpha, double beta, double *__restrict__ y, double *__restrict__ xy)
{
    __shared__ double s[CAP];
    constexpr int LN = 8, NG = 256 / LN, NPRE = 3;
    const int sub = threadIdx.x % LN, g = threadIdx.x / LN;
    double acc = 0.0;
    int b = blockIdx.x;
    uint4 rec = blkrec[b < n_blk ? b : 0];
    for (; b < n_blk; b += gridDim.x) {
        const int bn = b + gridDim.x;
        const uint4 recn = blkrec[bn < n_blk ? bn : b];
        const int r0 = (int)rec.x, nr = (int)(rec.y & 0xffffu), len = (int)(rec.y >> 16);
        const int64_t k0 = (int64_t)(((uint64_t)rec.w << 32) | rec.z);
        // every load below is unconditional (indices clamped into the block): a load inside `if (i < len)` is followed by its own wait, which made the
        // eight entry / gather pairs of a lane sixteen trips one after the other
        int64_t pa[NPRE], pe[NPRE];
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int r = g + NG * j, rc = r < nr ? r : nr - 1;
            pa[j] = rowptr[r0 + rc]; pe[j] = rowptr[r0 + rc + 1];
        }
        const double *nzb = nz + k0;
        const int32_t *cb = colidx + k0;
        constexpr int U = CAP / 256;
        int32_t cj[U];
        double vj[U], xj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = threadIdx.x + u * 256, ic = i < len ? i : len - 1;
            cj[u] = 0; vj[u] = 0.0;
            if (len > 0) { cj[u] = cb[ic]; vj[u] = nzb[ic]; } // wave-uniform condition (a run of empty rows has no entries to read)
        }
#ifdef TB_ABLATION
        if (g_spmv_nogather) { // profiling build: what the kernel costs without the gather of x (coalesced reads of the same volume instead)
#pragma unroll
            for (int u = 0; u < U; ++u) xj[u] = x[(cj[u] & 0) + r0 + ((threadIdx.x + u * 256) & 63)];
        } else
#endif
#pragma unroll
        for (int u = 0; u < U; ++u) xj[u] = x[cj[u]];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = threadIdx.x + u * 256;
            if (i < len) s[i] = vj[u] * xj[u];
        }
        int ra[NPRE], re[NPRE];
#pragma unroll
        for (int j = 0; j < NPRE; ++j) { ra[j] = (int)(pa[j] - k0); re[j] = (int)(pe[j] - k0); }
        __syncthreads();
        auto row = [&](int r, int a, int e) {
            double v = 0.0;
            for (int i = a + sub; i < e; i += LN) v += s[i];
#pragma unroll
            for (int o = LN / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LN);
            if (sub == 0) {
                if constexpr (DOT) { y[r0 + r] = v; acc += x[r0 + r] * v; }
                else y[r0 + r] = beta == 0.0 ? alpha * v : alpha * v + beta * y[r0 + r];
            }
        };
#pragma unroll
        for (int j = 0; j < NPRE; ++j) { const int r = g + NG * j; if (r < nr) row(r, ra[j], re[j]); }
        for (int r = g + NG * NPRE; r < nr; r += NG) row(r, (int)(rowptr[r0 + r] - k0), (int)(rowptr[r0 + r + 1] - k0)); // blocks of short rows
        __syncthreads();
        rec = recn;
    }
    if constexpr (DOT) block_sum_slots(acc, xy); // xy: a slot group (tb_reduce.hpp)
}

// Row-per-lane form of the same run (default).  In the kernels above lane i takes entry i, so the 64 gathers of x in one instruction follow 2.4 rows
// through all their columns: ≈ 21 scattered 24-byte pieces, and the texture-address path spends more on them than on the coalesced entry loads
// (profiling build without the gather: 0.57 instead of 0.81 ms).  Here the entries of the run are parked in LDS as they come (values and columns,
// coalesced), and the products are taken row-wise: three lanes per row, lane (row, s) the entries s, s + 3, …, so the lanes of a wave — 21 consecutive
// rows — gather x at three stencil offsets of 21 consecutive rows: a few cache lines per instruction on FE numberings.  Row sums stay in registers
// (no product array, no second LDS pass), the three partial sums meet by two lane shifts, y is stored by the lanes s = 0.
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

// Index-compressed form of the row-per-lane run (default when the pattern compresses).  On a finite-element numbering almost every row holds the same
// column offsets relative to its own index — the 27-point stencil of a hexahedral mesh: one signature covers 97 % of the rows at 216³, the boundary
// layers of the first-visit numbering add ≈ 10⁵ more — so the 4 B column index per non-zero is redundant: a row carries the position of its
// signature in a table (4 B per row; the table is a few MB and stays in L2), the kernel streams 8 B per non-zero instead of 12 and parks values
// only in LDS.  Lane mapping, order of the products and of the partial sums are those of k_spmv_stream_rows: the two kernels give identical bits.
// Same interface (tb_spmv_csr: the plan is built with the pattern's first product); patterns that do not compress keep the CSR kernel.
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

// Wave-private form of k_spmv_sig_rows (TB_SPMV_KERNEL=wave; measured: 0.668 against 0.682 ms at 216³, 0.112 against 0.098 ms on the 27-layer slab — not the
// default; with the values requested TWO runs ahead it took 0.857 ms: gfx9 retires vector-memory operations in order, so the wait for a run's gather of x then
// includes the value loads issued just before it).  A run is what ONE wave multiplies — at most 21 rows and WCAP entries — and a wave
// walks its runs on its own: values of the next run requested while the current one is multiplied, its LDS slice written and read by the same wave, so the
// kernel has no workgroup barrier at all (the block form waits twice per run of ≈ 75 rows for its slowest wave).  Same lane mapping inside the wave, same
// order of products and sums: identical bits.
constexpr int SPMV_WCAP = 640;
template <bool DOT>
__global__ void __launch_bounds__(256)
k_spmv_sig_wave(int n_run, const uint4 *__restrict__ runrec, const int64_t *__restrict__ rowptr, const uint32_t *__restrict__ rowsig, const int32_t *__restrict__ sigoff,
                const double *__restrict__ nz, int64_t nnz, const double *__restrict__ x, double alpha, double beta, double *__restrict__ y, double *__restrict__ xy)
{
    constexpr int U = SPMV_WCAP / 128, SUB = 3, RW = 21, NK = 9;
    __shared__ double2 s_all[4][SPMV_WCAP / 2 + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, rl = lane / SUB, sub = lane % SUB;
    double2 *s_v2 = s_all[wv];
    const double *s_v = (const double *)s_v2;
    const bool lane_ok = lane < SUB * RW;
    const int G = gridDim.x * 4;
    double acc = 0.0;
    int of[NK];
    uint32_t cur = 0xFFFFFFFFu;
#pragma unroll
    for (int t_ = 0; t_ < NK; ++t_) of[t_] = 0;
    auto request = [&](const uint4 &rc, bool live, double2(&v)[U], int64_t &pa, int64_t &pe, uint32_t &sg) {
        const int r0 = (int)rc.x, nr = (int)(rc.y & 0xffffu), len = (int)(rc.y >> 16);
        const int64_t k0 = (int64_t)(((uint64_t)rc.w << 32) | rc.z);
        const int rc0 = rl < nr ? rl : nr - 1;
        pa = pe = 0; sg = 0;
        if (live && nr > 0) { pa = rowptr[r0 + rc0]; pe = rowptr[r0 + rc0 + 1]; sg = rowsig[r0 + rc0]; }
        const int64_t ka = k0 - (k0 & 1);
        const int npairs = (len + (int)(k0 & 1) + 1) >> 1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = lane + u * 64;
            v[u] = make_double2(0.0, 0.0);
            if (live && i < npairs) {
                if (ka + 2 * (int64_t)i + 1 < nnz) v[u] = *(const double2 *)(nz + ka + 2 * (int64_t)i);
                else v[u].x = nz[ka + 2 * (int64_t)i];
            }
        }
    };
    int b = blockIdx.x * 4 + wv;
    uint4 rec = runrec[b < n_run ? b : 0];
    uint4 recn = runrec[b + G < n_run ? b + G : 0];
    double2 vj[U];
    int64_t pa0, pe0;
    uint32_t sg0;
    request(rec, b < n_run, vj, pa0, pe0, sg0);
    for (; b < n_run; b += G) {
        const uint4 recnn = runrec[b + 2 * G < n_run ? b + 2 * G : 0];
        const int r0 = (int)rec.x, nr = (int)(rec.y & 0xffffu), len = (int)(rec.y >> 16);
        const int64_t k0 = (int64_t)(((uint64_t)rec.w << 32) | rec.z);
        const int o = (int)(k0 & 1);
        const int npairs = (len + o + 1) >> 1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = lane + u * 64;
            if (i < npairs) s_v2[i] = vj[u];
        }
        __builtin_amdgcn_wave_barrier(); // LDS operations of one wave execute in order; this only keeps the compiler from moving the reads up
        double2 vjn[U];
        int64_t pa0n = 0, pe0n = 0;
        uint32_t sg0n = 0;
        {
            const int r = rl;
            const bool active = lane_ok && r < nr && len > 0;
            const int rc = r < nr ? r : (nr > 0 ? nr - 1 : 0);
            const int a = (int)(pa0 - k0) + o, n = (int)(pe0 - pa0), row = r0 + rc;
            {
                const uint32_t sg1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)sg0);
                const bool uniform = __ballot(sg0 != sg1) == 0ull;
                if (nr > 0 && (!uniform || sg1 != cur)) {
#pragma unroll
                    for (int t_ = 0; t_ < NK; ++t_) { const int k = sub + SUB * t_; of[t_] = sigoff[sg0 + (k < n ? k : 0)]; }
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
                cc[t_] = row + (kc[t_] >= 0 ? of[t_] : 0);
                vv[t_] = len > 0 ? s_v[a + kk] : 0.0;
            }
#pragma unroll
            for (int t_ = 0; t_ < NK; ++t_) xx[t_] = len > 0 ? x[cc[t_]] : 0.0;
            request(recn, b + G < n_run, vjn, pa0n, pe0n, sg0n); // behind the gather in program order
            double v = 0.0;
#pragma unroll
            for (int t_ = 0; t_ < NK; ++t_) v += kc[t_] >= 0 ? vv[t_] * xx[t_] : 0.0;
            if (active) for (int k = sub + SUB * NK; k < n; k += SUB) v += s_v[a + k] * x[row + sigoff[sg0 + k]]; // rows longer than 27 entries
            v += __shfl_down(v, 1, 64) + __shfl_down(v, 2, 64);
            if (active && sub == 0) {
                if constexpr (DOT) { y[r0 + r] = v; acc += x[r0 + r] * v; }
                else y[r0 + r] = beta == 0.0 ? alpha * v : alpha * v + beta * y[r0 + r];
            }
        }
        __builtin_amdgcn_wave_barrier();
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

// is the pattern a CSR of 3×3 blocks?  (checked once on the host; b3 = 1 yes / −1 no)
static int block3_plan(tb_pattern *p)
{
    if (p->b3 != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev); // a plan is built (host work + blocking uploads) at its first use: make that use before the capture
    static const bool off = tune_env("TB_SPMV_B3") && atoi(tune_env("TB_SPMV_B3")) == 0;
    p->b3 = -1;
    if (off || p->n_rows % 3 != 0 || p->nnz % 9 != 0 || p->nnz == 0) return TB_OK;
    std::vector<int32_t> bcol((size_t)(p->nnz / 9));
    const int64_t nbr = p->n_rows / 3;
    for (int64_t R = 0; R < nbr; ++R) {
        const int64_t k0 = p->h_rowptr[3 * R], k1 = p->h_rowptr[3 * R + 1], k2 = p->h_rowptr[3 * R + 2], k3 = p->h_rowptr[3 * R + 3];
        const int64_t L = k1 - k0;
        if (L % 3 != 0 || k2 - k1 != L || k3 - k2 != L || k0 % 9 != 0) return TB_OK;
        for (int64_t j = 0; j < L; j += 3) {
            const int32_t c = p->h_colidx[k0 + j];
            if (c % 3 != 0 || p->h_colidx[k0 + j + 1] != c + 1 || p->h_colidx[k0 + j + 2] != c + 2) return TB_OK;
        }
        for (int64_t j = 0; j < L; ++j)
            if (p->h_colidx[k1 + j] != p->h_colidx[k0 + j] || p->h_colidx[k2 + j] != p->h_colidx[k0 + j]) return TB_OK;
        for (int64_t j = 0; j < L; j += 3) bcol[(size_t)(k0 / 9 + j / 3)] = p->h_colidx[k0 + j] / 3;
    }
    TB_HIP(hipMalloc((void **)&p->d_bcol, bcol.size() * sizeof(int32_t)));
    TB_HIP(hipMemcpy(p->d_bcol, bcol.data(), bcol.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    const double avg = (double)bcol.size() / (double)nbr; // blocks per node row: 27 for Q1, 64…125 for Q2
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

// row runs of the stream SpMV: greedy cuts of the row sequence at ≤ SPMV_CAP non-zeros; n_blk = −1 (lanes-per-row kernel instead) if a single
// row exceeds the capacity
#ifndef TB_SPMV_CAP
#define TB_SPMV_CAP 2048
#endif
constexpr int SPMV_CAP = TB_SPMV_CAP;
static int stream_plan(tb_pattern *p)
{
    PlanTimer timer("stream_plan");
    if (p->n_blk != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev);
    std::vector<int32_t> cut{0};
    int64_t start = 0;
    for (int64_t r = 0; r < p->n_rows; ++r) {
        if (p->h_rowptr[r + 1] - p->h_rowptr[r] > SPMV_CAP - 2) { p->n_blk = -1; return TB_OK; }
        // − 2: the 16-byte loads of the compressed kernel start one entry early and end one late (empty rows: the record holds 16 bits of row count)
        if (p->h_rowptr[r + 1] - p->h_rowptr[start] > SPMV_CAP - 2 || r - start >= 60000) { cut.push_back((int32_t)r); start = r; }
    }
    cut.push_back((int32_t)p->n_rows);
    TB_HIP(hipMalloc((void **)&p->d_blkrow, cut.size() * sizeof(int32_t)));
    TB_HIP(hipMemcpy(p->d_blkrow, cut.data(), cut.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    // one record per block for k_spmv_stream_rec: first row, rows | entries << 16, first nz (low, high word)
    static_assert(SPMV_CAP < 65536, "row and entry counts of a block share one 32-bit word");
    std::vector<uint32_t> rec(4 * (cut.size() - 1));
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
        const int64_t k0 = p->h_rowptr[cut[b]], len = p->h_rowptr[cut[b + 1]] - k0;
        rec[4 * b] = (uint32_t)cut[b];
        rec[4 * b + 1] = (uint32_t)(cut[b + 1] - cut[b]) | (uint32_t)len << 16;
        rec[4 * b + 2] = (uint32_t)((uint64_t)k0 & 0xffffffffu);
        rec[4 * b + 3] = (uint32_t)((uint64_t)k0 >> 32);
    }
    TB_HIP(hipMalloc((void **)&p->d_blkrec, rec.size() * sizeof(uint32_t)));
    TB_HIP(hipMemcpy(p->d_blkrec, rec.data(), rec.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    p->n_blk = (int64_t)cut.size() - 1;
    return TB_OK;
}

// Signature plan of the index-compressed SpMV: rows with the same list of column offsets (colidx[k] − row) share one table entry.  Built on the
// host with the pattern's first product: per row a 64-bit hash (parallel), de-duplication in row order with the neighbouring row as the fast path
// (consecutive rows of a finite-element numbering nearly always repeat the signature).  The pattern "compresses" when the table is at most a
// quarter of the column array and every offset list fits the kernel (row length ≤ SPMV_CAP is checked by the stream plan); otherwise n_sig = −1.
static int sig_plan(tb_pattern *p, bool forced = false)
{
    PlanTimer timer("sig_plan");
    if (p->n_sig != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev);
    const bool off = !forced && spmv_kernel_env() && strcmp(spmv_kernel_env(), "sig") != 0; // "rows" / "rec" / "chain": the CSR kernels (read per pattern: A/B runs and the bit-identity test build one pattern of each kind in one process)
    const int64_t n = p->n_rows;
    if (off || n == 0 || p->nnz >= (int64_t)0xffffffffll) { p->n_sig = -1; return TB_OK; }
    const int64_t *rp = p->h_rowptr.data();
    const int32_t *ci = p->h_colidx.data();
    std::vector<uint64_t> hsh((size_t)n);
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < n; ++r) {
        uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t)(rp[r + 1] - rp[r]);
        for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
            h ^= (uint64_t)(uint32_t)(ci[k] - (int32_t)r) + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
            h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
        }
        hsh[r] = h;
    }
    std::vector<uint32_t> rowsig((size_t)n);
    std::vector<int32_t> tab;
    std::unordered_map<uint64_t, std::vector<uint32_t>> seen; // hash → positions of the signatures with that hash
    const int64_t budget = std::max<int64_t>(p->nnz / 4, 64);
    auto same = [&](uint32_t at, int64_t r) {
        const int64_t len = rp[r + 1] - rp[r];
        if ((int64_t)at + len > (int64_t)tab.size()) return false;
        for (int64_t k = 0; k < len; ++k) if (tab[at + k] != ci[rp[r] + k] - (int32_t)r) return false;
        return true;
    };
    std::vector<int32_t> siglen; // length of the signature starting at a table position is implied by the row: equal hash + equal length + equal offsets
    std::unordered_map<uint32_t, int32_t> len_at;
    int64_t nsig = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = rp[r + 1] - rp[r];
        if (r > 0 && hsh[r] == hsh[r - 1] && rp[r] - rp[r - 1] == len && same(rowsig[r - 1], r)) { rowsig[r] = rowsig[r - 1]; continue; }
        auto &cand = seen[hsh[r]];
        bool found = false;
        for (uint32_t at : cand) if (len_at[at] == (int32_t)len && same(at, r)) { rowsig[r] = at; found = true; break; }
        if (found) continue;
        const uint32_t at = (uint32_t)tab.size();
        for (int64_t k = 0; k < len; ++k) tab.push_back(ci[rp[r] + k] - (int32_t)r);
        if (len == 0) tab.push_back(0); // an empty row still owns a (never read) position
        cand.push_back(at); len_at[at] = (int32_t)len; rowsig[r] = at; ++nsig;
        if ((int64_t)tab.size() > budget) { p->n_sig = -1; return TB_OK; } // an unstructured numbering: every row its own signature
    }
    tab.resize(tab.size() + 32, 0); // the kernel reads offset 0 of a row's signature for its masked entries, and whole triples: slack at the end
    TB_HIP(hipMalloc((void **)&p->d_rowsig, rowsig.size() * sizeof(uint32_t)));
    TB_HIP(hipMemcpy(p->d_rowsig, rowsig.data(), rowsig.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    TB_HIP(hipMalloc((void **)&p->d_sigoff, tab.size() * sizeof(int32_t)));
    TB_HIP(hipMemcpy(p->d_sigoff, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    p->n_sig = nsig; p->sig_entries = (int64_t)tab.size();
    p->h_rowsig = std::move(rowsig); // (the slice table of the mirror marks the slices whose rows share one signature)
    if (getenv("TB_PLAN_VERBOSE"))
        fprintf(stderr, "[tbhip] SpMV signature plan: %lld rows, %lld signatures, table %lld entries (%.4f of the column array)\n", (long long)n, (long long)nsig,
                (long long)tab.size(), (double)tab.size() / (double)std::max<int64_t>(p->nnz, 1));
    return TB_OK;
}

static int sig_plan_forced(tb_pattern *p) { return sig_plan(p, true); }
// runs of the wave-private kernel: ≤ 21 rows and ≤ SPMV_WCAP − 2 entries each; n_wrun = −1 when a row is longer than that
static int wave_plan(tb_pattern *p)
{
    if (p->n_wrun != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev);
    std::vector<uint32_t> rec;
    int64_t start = 0;
    auto push = [&](int64_t r0, int64_t r1) {
        const int64_t k0 = p->h_rowptr[r0], len = p->h_rowptr[r1] - k0;
        rec.push_back((uint32_t)r0); rec.push_back((uint32_t)(r1 - r0) | (uint32_t)len << 16);
        rec.push_back((uint32_t)((uint64_t)k0 & 0xffffffffu)); rec.push_back((uint32_t)((uint64_t)k0 >> 32));
    };
    for (int64_t r = 0; r < p->n_rows; ++r) {
        if (p->h_rowptr[r + 1] - p->h_rowptr[r] > SPMV_WCAP - 2) { p->n_wrun = -1; return TB_OK; }
        if (p->h_rowptr[r + 1] - p->h_rowptr[start] > SPMV_WCAP - 2 || r - start >= 21) { push(start, r); start = r; }
    }
    if (p->n_rows > start) push(start, p->n_rows);
    TB_HIP(hipMalloc((void **)&p->d_wrunrec, rec.size() * sizeof(uint32_t)));
    TB_HIP(hipMemcpy(p->d_wrunrec, rec.data(), rec.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    p->n_wrun = (int64_t)rec.size() / 4;
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
struct MirrorSlice { int64_t base, obase; uint32_t sig, width; uint32_t pad[2]; }; // 32 bytes
constexpr uint32_t MIRROR_MIXED = 0xFFFFFFFFu;
constexpr int32_t MIRROR_NONE = INT32_MIN; // column offset of a padding entry
static int mirror_plan(tb_pattern *p)
{
    PlanTimer timer("mirror_plan");
    if (p->n_slices != 0) return TB_OK;
    TB_NO_CAPTURE(p->mesh->dev);
    int rc = spmv_plans(p);
    if (rc) return rc;
    if (p->b3 > 0 || p->n_rows == 0) { p->n_slices = -1; return TB_OK; }
    const bool have_sig = p->n_sig > 0 && (int64_t)p->h_rowsig.size() == p->n_rows; // a numbering without shared signatures: every slice carries its offsets
    const int64_t ns = (p->n_rows + 63) / 64;
    // one record per slice: {first value, first column offset, signature shared by its 64 rows or MIXED, width}.  A slice of one signature needs no
    // per-row metadata (offsets by scalar loads from the signature table); a mixed slice — the two ends of a grid line meet in one slice out of three at
    // 216³ — carries its column offsets entry-major like the values (4 B per entry, padding marked), so both kinds cost two trips: record → values
    // and offsets → x
    std::vector<MirrorSlice> rec((size_t)ns + 1);
    std::vector<int32_t> offs;
    int64_t at = 0;
    for (int64_t s = 0; s < ns; ++s) {
        const int64_t r0 = 64 * s, r1 = std::min<int64_t>(r0 + 64, p->n_rows);
        int64_t w = 0;
        bool uni = have_sig && r1 - r0 == 64;
        for (int64_t r = r0; r < r1; ++r) {
            w = std::max<int64_t>(w, p->h_rowptr[r + 1] - p->h_rowptr[r]);
            uni = uni && p->h_rowsig[r] == p->h_rowsig[r0];
        }
        if (w > 255) { p->n_slices = -1; return TB_OK; }
        rec[s] = MirrorSlice{at, uni ? -1 : (int64_t)offs.size(), uni ? p->h_rowsig[r0] : MIRROR_MIXED, (uint32_t)w, {0, 0}};
        if (!uni) {
            const size_t o0 = offs.size();
            offs.resize(o0 + (size_t)(64 * w), MIRROR_NONE);
            for (int64_t r = r0; r < r1; ++r)
                for (int64_t k = p->h_rowptr[r]; k < p->h_rowptr[r + 1]; ++k) offs[o0 + (size_t)(64 * (k - p->h_rowptr[r]) + (r - r0))] = p->h_colidx[k] - (int32_t)r;
        }
        at += 64 * w;
    }
    rec[ns] = MirrorSlice{at, -1, MIRROR_MIXED, 0, {0, 0}};
    MirrorSlice *db = nullptr;
    TB_HIP(hipMalloc((void **)&db, rec.size() * sizeof(MirrorSlice)));
    TB_HIP(hipMemcpy(db, rec.data(), rec.size() * sizeof(MirrorSlice), hipMemcpyHostToDevice));
    if (offs.empty()) offs.push_back(0);
    TB_HIP(hipMalloc((void **)&p->d_mir_off, offs.size() * sizeof(int32_t)));
    TB_HIP(hipMemcpy(p->d_mir_off, offs.data(), offs.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    p->d_mir_base = db; p->mir_entries = at; p->n_slices = ns;
    if (getenv("TB_PLAN_VERBOSE")) {
        int64_t mixed = 0;
        for (int64_t s = 0; s < ns; ++s) mixed += rec[s].sig == MIRROR_MIXED;
        fprintf(stderr, "[tbhip] SpMV mirror plan: %lld slices (%lld of mixed signatures), %lld value slots for %lld non-zeros\n", (long long)ns, (long long)mixed, (long long)at,
                (long long)p->nnz);
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

// TB_SPMV_KERNEL=chain: the five-trip kernel, kept as the comparison build
static bool spmv_chain_kernel()
{
    static const bool chain = spmv_kernel_env() && !strcmp(spmv_kernel_env(), "chain");
    return chain;
}
template <bool DOT>
static void launch_stream(tb_pattern *p, const double *nz, const double *x, double alpha, double beta, double *y, double *xy, unsigned grid)
{
    hipStream_t st = p->mesh->dev->stream;
#ifdef TB_ABLATION
    static bool once = false;
    if (!once) { once = true; const int v = getenv("TB_SPMV_NOGATHER") ? 1 : 0; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_spmv_nogather), &v, sizeof(int)); }
#endif
    for (int i = 0; i < tb_pattern::MIRRORS; ++i) // the caller bound a sliced mirror of this very array
        if (p->mir_nz[i] == nz && nz) { launch_mirror<DOT>(p, p->d_mir[i], x, alpha, beta, y, xy); return; }
    static const bool rows_kernel = !(spmv_kernel_env() && strcmp(spmv_kernel_env(), "rows") != 0 && strcmp(spmv_kernel_env(), "sig") != 0 &&
                                      strcmp(spmv_kernel_env(), "wave") != 0); // "rec" / "chain": entry-per-lane kernels
    const bool wave_kernel = spmv_kernel_env() && !strcmp(spmv_kernel_env(), "wave"); // read per launch: the bit-identity test switches it inside one process
    if (wave_kernel && ((uintptr_t)nz & 15) == 0 && sig_plan_forced(p) == TB_OK && p->n_sig > 0 && wave_plan(p) == TB_OK && p->n_wrun > 0) {
        static int per_cu_w = 0;
        if (!per_cu_w) {
            if (tune_env("TB_SPMV_WG_PER_CU")) per_cu_w = atoi(tune_env("TB_SPMV_WG_PER_CU"));
            if (per_cu_w <= 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_w, (const void *)k_spmv_sig_wave<DOT>, 256, 0) != hipSuccess || per_cu_w <= 0)) per_cu_w = 3;
        }
        const unsigned gmaxw = (unsigned)(p->mesh->dev->n_cu * per_cu_w);
        hipLaunchKernelGGL((k_spmv_sig_wave<DOT>), dim3(std::min<unsigned>((unsigned)((p->n_wrun + 3) / 4), gmaxw)), dim3(256), 0, st, (int)p->n_wrun, (const uint4 *)p->d_wrunrec,
                           p->d_rowptr, p->d_rowsig, p->d_sigoff, nz, (int64_t)p->nnz, x, alpha, beta, y, xy);
        return;
    }
    if (rows_kernel && ((uintptr_t)nz & 15) == 0 && sig_plan(p) == TB_OK && p->n_sig > 0) { // default where the pattern compresses: 16 KB of LDS per workgroup
        // persistent: exactly the workgroups that are resident together (the runs are dealt round-robin, every workgroup gets the same share ± 1)
        static int per_cu = 0;
        if (!per_cu) {
            if (tune_env("TB_SPMV_WG_PER_CU")) per_cu = atoi(tune_env("TB_SPMV_WG_PER_CU"));
            if (per_cu <= 0 && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_spmv_sig_rows<SPMV_CAP, DOT>, 256, 0) != hipSuccess || per_cu <= 0)) per_cu = 3;
        }
        const unsigned gmax = (unsigned)(p->mesh->dev->n_cu * per_cu);
        hipLaunchKernelGGL((k_spmv_sig_rows<SPMV_CAP, DOT>), dim3(std::min<unsigned>((unsigned)p->n_blk, gmax)), dim3(256), 0, st, (int)p->n_blk, (const uint4 *)p->d_blkrec, p->d_rowptr,
                           p->d_rowsig, p->d_sigoff, nz, (int64_t)p->nnz, x, alpha, beta, y, xy);
    } else if (rows_kernel) // 24 KB of LDS per workgroup: six resident per CU
        hipLaunchKernelGGL((k_spmv_stream_rows<SPMV_CAP, DOT>), dim3(grid > 1536 ? 1536 : grid), dim3(256), 0, st, (int)p->n_blk, (const uint4 *)p->d_blkrec, p->d_rowptr,
                           p->d_colidx, nz, x, alpha, beta, y, xy);
    else if (spmv_chain_kernel())
        hipLaunchKernelGGL((k_spmv_stream<SPMV_CAP, DOT>), dim3(grid), dim3(256), 0, st, (int)p->n_blk, p->d_blkrow, p->d_rowptr, p->d_colidx, nz, x, alpha, beta, y, xy);
    else
        hipLaunchKernelGGL((k_spmv_stream_rec<SPMV_CAP, DOT>), dim3(grid), dim3(256), 0, st, (int)p->n_blk, (const uint4 *)p->d_blkrec, p->d_rowptr, p->d_colidx, nz, x,
                           alpha, beta, y, xy);
}

static unsigned stream_grid(const tb_pattern *p)
{
    static const int64_t cap = tune_env("TB_SPMV_GRID") ? atoi(tune_env("TB_SPMV_GRID")) : 2048; // 256 CUs × 8 resident workgroups
    return (unsigned)std::min<int64_t>(p->n_blk, cap);
}

int spmv_plans(tb_pattern *p)
{
    int rc = block3_plan(p);
    if (rc || p->b3 > 0) return rc;
    rc = stream_plan(p);
    if (rc || p->n_blk <= 0) { if (p->n_sig == 0) p->n_sig = -1; return rc; }
    return sig_plan(p);
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

int launch_spmv(tb_pattern *p, const double *nz, const double *x, double alpha, double beta, double *y)
{
    tb_device *dev = p->mesh->dev;
    static const int lanes = tune_env("TB_SPMV_LANES") ? atoi(tune_env("TB_SPMV_LANES")) : 0;
    if (lanes == 0 && block3_plan(p) == TB_OK && p->b3 > 0) {
        launch_b3<false>(p, nz, x, alpha, beta, y, nullptr);
        TB_HIP(hipGetLastError());
        return TB_OK;
    }
    if (lanes == 0 && stream_plan(p) == TB_OK && p->n_blk > 0) {
        launch_stream<false>(p, nz, x, alpha, beta, y, nullptr, stream_grid(p));
        TB_HIP(hipGetLastError());
        return TB_OK;
    }
#define TB_SPMV(LN) hipLaunchKernelGGL(k_spmv<LN>, dim3(grid_for(dev, p->n_rows * LN, 256)), dim3(256), 0, dev->stream, p->n_rows, p->d_rowptr, p->d_colidx, nz, x, alpha, beta, y)
    switch (lanes) {
    case 2: TB_SPMV(2); break;
    case 4: TB_SPMV(4); break;
    case 8: TB_SPMV(8); break;
    case 32: TB_SPMV(32); break;
    default: TB_SPMV(16);
    }
#undef TB_SPMV
    TB_HIP(hipGetLastError());
    return TB_OK;
}

// y = A x with the partials of xᵀy left in a slot group: the one selector of the product kernel of launch_cg and of the distributed CG forms
// (3×3 blocks, else row runs — mirror, signature rows, CSR rows —, else 16 lanes per row); it plans on first use
int launch_spmv_dot_slots(tb_pattern *pat, const double *A, const double *x, double *y, double *d_dot /* a slot group */)
{
    tb_device *dev = pat->mesh->dev;
    const int64_t n = pat->n_rows;
    if (n == 0) return TB_OK;
    static const int lanes_env = tune_env("TB_SPMV_LANES") ? atoi(tune_env("TB_SPMV_LANES")) : 0;
    if (lanes_env == 0) { int rc = block3_plan(pat); if (rc) return rc; if (pat->b3 <= 0) { rc = stream_plan(pat); if (rc) return rc; } }
    if (lanes_env == 0 && pat->b3 > 0)
        launch_b3<true>(pat, A, x, 1.0, 0.0, y, d_dot);
    else if (lanes_env == 0 && pat->n_blk > 0)
        launch_stream<true>(pat, A, x, 1.0, 0.0, y, d_dot, stream_grid(pat));
    else
        hipLaunchKernelGGL(k_spmv_dot<16>, dim3(grid_for(dev, n * 16, 256)), dim3(256), 0, dev->stream, n, pat->d_rowptr, pat->d_colidx, A, x, y, d_dot);
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
        std::vector<int64_t> pos((size_t)p->n_rows, -1);
        for (int64_t r = 0; r < p->n_rows; ++r)
            for (int64_t k = p->h_rowptr[r]; k < p->h_rowptr[r + 1]; ++k)
                if (p->h_colidx[k] == r) { pos[r] = k; break; }
        TB_HIP(hipMalloc((void **)&p->d_diagpos, pos.size() * sizeof(int64_t)));
        TB_HIP(hipMemcpy(p->d_diagpos, pos.data(), pos.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    if (p->n_rows == 0) return TB_OK;
    hipLaunchKernelGGL(k_extract_diag<INVERT>, dim3((unsigned)((p->n_rows + 255) / 256)), dim3(256), 0, dev->stream, p->n_rows, p->d_diagpos, nz, dinv);
    TB_HIP(hipGetLastError());
    return TB_OK;
}
int launch_extract_diagonal(tb_pattern *p, const double *nz, double *diag) { return launch_extract_diag<false>(p, nz, diag); }
int launch_extract_inverse_diagonal(tb_pattern *p, const double *nz, double *dinv) { return launch_extract_diag<true>(p, nz, dinv); }

} // namespace tb

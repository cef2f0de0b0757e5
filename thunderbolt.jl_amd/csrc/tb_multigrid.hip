// tb_multigrid.hip — multigrid preconditioner on hexahedral grids (GMGPrecon, PMGPrecon and ChainedMGPrecon of the reference: src/solver/linear/multigrid.jl,
// ext/ThunderboltFerriteMultigridExt.jl): h-levels of first-order fields on nested grids and, at the top, one p-level from a second-order field to the
// first-order field on the same cells.  The plans come from tb_mg_planners.cpp (P row-wise, Pᵀ row-wise, the gather plan of PᵀAP, per dof or per
// 3 × 3 block); this file holds the hierarchy object, the two numeric Galerkin kernels, the transfers, the V-cycle driver, and the kernels the whole
// multigrid family calls through the launchers of tb_mg_internal.hpp (tb_amg.hip, tb_bidomain_mg.hip, the Chebyshev preconditioner of tb_krylov.hip):
// the Chebyshev–Jacobi smoother step, the dense coarsest inverse and its product, the diagonal fill and the fold of per-workgroup partials.
// Every sum of this file's kernels has one recorded order and none of them uses an atomic: two applications of one setup give the same bits, and two
// setups the same level matrices and the same coarsest inverse.  λmax is not this file's: tb_mg_setup takes it from estimate_lambda_max
// (tb_krylov.hip), whose Lanczos sums leave through block_sum_to — one unsafeAtomicAdd per 1 024-thread workgroup on grid_red workgroups.  Up to two
// workgroups (levels of at most 2 048 dofs) that is one order; three or more add in arrival order, so on larger levels two setups may differ in the
// last bits of λmax and, through the smoother's coefficients, of the cycle.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "tb_amg_internal.hpp"
#include "tb_internal.h"
#include "tb_mg_internal.hpp"
#include "tb_mg_planners.hpp"
#include "tb_reduce.hpp"

namespace tb {

static_assert(mgplan::ERR_BAD_ARG == TB_ERR_BAD_ARG && mgplan::ERR_PATTERN == TB_ERR_PATTERN && mgplan::ERR_UNSUPPORTED == TB_ERR_UNSUPPORTED, "planner codes");

// A_c[k] = Σ over the recorded terms of 2^−e · A_f[fine nz]: 16 lanes share a coarse non-zero (≈ 90 terms each on a scalar field: the term words
// are read as 64-byte runs), lane sums in term order, then a fixed butterfly over the 16 lanes.
__global__ void __launch_bounds__(256)
k_mg_galerkin(int64_t cnnz, const int64_t *__restrict__ gptr, const uint32_t *__restrict__ terms, const double *__restrict__ Af, double *__restrict__ Ac)
{
    const int64_t k = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (k >= cnnz) return; // (the 16 lanes of a group leave together)
    const int sub = threadIdx.x & 15;
    const int64_t lo = gptr[k], hi = gptr[k + 1];
    double s = 0.0;
    for (int64_t q = lo + sub; q < hi; q += 16) {
        const uint32_t t = terms[q];
        s += pow2_neg(t >> mgplan::TERM_BITS) * Af[t & ((1u << mgplan::TERM_BITS) - 1u)];
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 16);
    if (sub == 0) Ac[k] = s;
}

// The same product on CSRs of 3 × 3 blocks: 16 lanes share a coarse block, a term names a fine block and moves its nine values — three 24-byte runs
// in the rows 3i, 3i + 1, 3i + 2, whose lengths are equal, so the block offset of a row triple is rowptr[3i] / 9 as in k_spmv_b3.  Nine lane sums in term
// order, the fixed butterfly, nine stores by the lanes 0, 1, 2 (a row each).  FLAGS: prescribed dofs may cut through a block; an entry enters only when
// its fine row and column and its coarse row and column are free — selected, not multiplied by 0: whatever a dropped position holds stays out.
template <bool FLAGS>
__global__ void __launch_bounds__(256)
k_mg_galerkin_b3(int64_t ncb, const int64_t *__restrict__ gptr, const uint32_t *__restrict__ terms, const int32_t *__restrict__ fbrow, const int32_t *__restrict__ fbcol,
                 const int64_t *__restrict__ frowptr, const double *__restrict__ Af, const uint8_t *__restrict__ fpresc, const int32_t *__restrict__ cbrow,
                 const int32_t *__restrict__ cbcol, const int64_t *__restrict__ crowptr, const uint8_t *__restrict__ cpresc, double *__restrict__ Ac)
{
    const int64_t kb = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    if (kb >= ncb) return; // (the 16 lanes of a group leave together)
    const int sub = threadIdx.x & 15;
    const int64_t I = cbrow[kb];
    unsigned keep = 0x1ffu; // bit 3a + b: entry (a, b) of the block
    if (FLAGS) {
        const int64_t J = cbcol[kb];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (cpresc[3 * I + a]) keep &= ~(7u << (3 * a));
            if (cpresc[3 * J + a]) keep &= ~(0x49u << a);
        }
    }
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t q = gptr[kb] + sub, hi = gptr[kb + 1]; q < hi; q += 16) {
        const uint32_t t = terms[q];
        const int64_t B = t & ((1u << mgplan::TERM_BITS) - 1u);
        const double w = pow2_neg(t >> mgplan::TERM_BITS);
        const int64_t i = fbrow[B], k0 = frowptr[3 * i], len = frowptr[3 * i + 1] - k0;
        const double *p = Af + k0 + 3 * (B - k0 / 9);
        unsigned m = keep;
        if (FLAGS) {
            const int64_t j = fbcol[B];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (fpresc[3 * i + a]) m &= ~(7u << (3 * a));
                if (fpresc[3 * j + a]) m &= ~(0x49u << a);
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const double v = w * p[a * len + b];
                s[3 * a + b] += (!FLAGS || ((m >> (3 * a + b)) & 1u)) ? v : 0.0;
            }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e)
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s[e] += __shfl_xor(s[e], o, 16);
    if (sub < 3) {
        const int64_t K0 = crowptr[3 * I], clen = crowptr[3 * I + 1] - K0;
        double *out = Ac + K0 + sub * clen + 3 * (kb - K0 / 9);
        out[0] = sub == 0 ? s[0] : sub == 1 ? s[3] : s[6];
        out[1] = sub == 0 ? s[1] : sub == 1 ? s[4] : s[7];
        out[2] = sub == 0 ? s[2] : sub == 1 ? s[5] : s[8];
    }
}

// one workgroup: the diagonal of every prescribed dof of a coarse level becomes the mean |diagonal| of its free dofs (fixed order: strided lane sums, LDS tree)
__global__ void __launch_bounds__(1024)
k_mg_fill_diag(int64_t n, const int64_t *__restrict__ diagpos, const uint8_t *__restrict__ presc, double *__restrict__ A)
{
    __shared__ double ssum[1024];
    __shared__ double scnt[1024];
    double s = 0.0, c = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024)
        if (!presc[i]) { s += fabs(A[diagpos[i]]); c += 1.0; }
    ssum[threadIdx.x] = s; scnt[threadIdx.x] = c;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { ssum[threadIdx.x] += ssum[threadIdx.x + o]; scnt[threadIdx.x] += scnt[threadIdx.x + o]; }
        __syncthreads();
    }
    const double fill = scnt[0] > 0.0 ? ssum[0] / scnt[0] : 1.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024)
        if (presc[i]) A[diagpos[i]] = fill;
}

__global__ void __launch_bounds__(256) k_mg_mask(int64_t n, const uint8_t *__restrict__ presc, double *__restrict__ dinv)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (presc[i]) dinv[i] = 0.0;
}

// One step of the Chebyshev iteration on D⁻¹A (Saad, Iterative Methods, Alg. 12.1).  MODE 0: first step from x = 0 (d = c2·D⁻¹r, x = d, no product
// needed); MODE 1: first step from a given x (w = A x; d = c2·D⁻¹(r − w), x += d); MODE 2: d = c1·d + c2·D⁻¹(r − w), x += d.
template <int MODE>
__global__ void __launch_bounds__(256)
k_mg_cheb(int64_t n, double c1, double c2, const double *__restrict__ dinv, const double *__restrict__ r, const double *__restrict__ w, double *__restrict__ d,
          double *__restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (MODE == 0) {
            const double di = c2 * dinv[i] * r[i];
            d[i] = di; x[i] = di;
        } else {
            const double g = c2 * dinv[i] * (r[i] - w[i]);
            const double di = MODE == 1 ? g : c1 * d[i] + g;
            d[i] = di; x[i] += di;
        }
    }
}

// r_c = Pᵀ(r − w) (w NULL: Pᵀ r): one thread per coarse dof gathers its fine dofs (at most 27 on either kind of level: the nodes of the 8 children
// around a coarse node, or the Q2 nodes of the 8 cells around a vertex)
__global__ void __launch_bounds__(256)
k_mg_restrict(int64_t nc, const int64_t *__restrict__ rptr, const int32_t *__restrict__ rcol, const uint8_t *__restrict__ rexp, const double *__restrict__ r,
              const double *__restrict__ w, double *__restrict__ rc)
{
    const int64_t I = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nc) return;
    double s = 0.0;
    for (int64_t q = rptr[I]; q < rptr[I + 1]; ++q) {
        const int32_t i = rcol[q];
        s += pow2_neg(rexp[q]) * (w ? r[i] - w[i] : r[i]);
    }
    rc[I] = s;
}

// x_f (+)= P x_c: one thread per fine dof gathers its at most 8 parents (h-level: the vertices of the parent cell's edge, face or cell the node lies on;
// p-level: the vertices of the edge, face or cell the Q2 node belongs to)
template <bool ADD>
__global__ void __launch_bounds__(256)
k_mg_prolong(int64_t nf, const int64_t *__restrict__ pptr, const int32_t *__restrict__ pcol, const uint8_t *__restrict__ pexp, const double *__restrict__ xc,
             double *__restrict__ xf)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    double s = 0.0;
    for (int64_t q = pptr[i]; q < pptr[i + 1]; ++q) s += pow2_neg(pexp[q]) * xc[pcol[q]];
    if (ADD) xf[i] += s; else xf[i] = s;
}

// One workgroup: C = A⁻¹ of the coarsest operator (n ≤ 1024), dense, by Gauss–Jordan elimination in place without pivoting (the operator is symmetric
// positive definite; a prescribed dof is a row of the identity scaled by its diagonal), symmetrised at the end.  Rows go to the 16 waves, columns to
// the lanes; the workgroup's barriers order the global-memory phases.
__global__ void __launch_bounds__(1024)
k_mg_dense_inverse(int n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz, double *__restrict__ C)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int i = wv; i < n; i += nw)
        for (int j = lane; j < n; j += 64) C[(size_t)i * n + j] = 0.0;
    __syncthreads();
    for (int i = wv; i < n; i += nw)
        for (int64_t k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) C[(size_t)i * n + colidx[k]] = nz[k];
    __syncthreads();
    mg_gauss_jordan(n, C);
}

// The same for an operator that need not be symmetric (tb_mg_set_general, tb_amg_set_general): Gauss–Jordan elimination in place with partial (row)
// pivoting, nothing symmetrised.  Step k: every thread holds one row and offers |C[row][k]| for the rows k … n − 1 (a NaN counts as +∞, so that it is
// chosen and reported); a butterfly picks the wave's largest, a fold over the 16 waves in LDS the workgroup's — ties go to the lowest row in both, so
// two set-ups choose the same pivots and give the same bits.  Rows k and p are swapped, the step is mg_gauss_jordan's.  In-place elimination keeps
// the identity columns implicit, so a row swap at step k is a column swap (k, p) of the result: the swaps are composed in reverse order into one
// column map in LDS and every row is gathered through it at the end (a wave per row: the whole row is in registers before any of it is stored).
// *status = 0, or 1 + the step whose pivot was zero or not finite (the workgroup leaves there; C is then of no use).
__global__ void __launch_bounds__(1024)
k_mg_dense_inverse_pivot(int n, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz, double *__restrict__ C,
                         double *__restrict__ status)
{
    __shared__ double s_val[16];
    __shared__ int s_row[16];
    __shared__ int s_piv[MG_COARSEST_MAX], s_map[MG_COARSEST_MAX]; // the row swapped with row k at step k; the column map of the end
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6; // (launched with MG_COARSEST_MAX threads: a row each)
    for (int i = wv; i < n; i += nw)
        for (int j = lane; j < n; j += 64) C[(size_t)i * n + j] = 0.0;
    __syncthreads();
    for (int i = wv; i < n; i += nw)
        for (int64_t k = rowptr[i] + lane; k < rowptr[i + 1]; k += 64) C[(size_t)i * n + colidx[k]] = nz[k];
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        double a = -1.0;
        int row = 0x7fffffff;
        if (tid >= k && tid < n) {
            a = fabs(C[(size_t)tid * n + k]);
            if (a != a) a = __builtin_inf();
            row = tid;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double a2 = __shfl_xor(a, o, 64);
            const int r2 = __shfl_xor(row, o, 64);
            if (a2 > a || (a2 == a && r2 < row)) { a = a2; row = r2; }
        }
        if (lane == 0) { s_val[wv] = a; s_row[wv] = row; }
        __syncthreads();
        a = s_val[0]; row = s_row[0];
        for (int q = 1; q < nw; ++q) {
            const double a2 = s_val[q];
            const int r2 = s_row[q];
            if (a2 > a || (a2 == a && r2 < row)) { a = a2; row = r2; }
        }
        const int p = row; // (the same in every thread; k ≤ p < n because row k itself is offered)
        if (!(a > 0.0) || a == __builtin_inf()) {
            if (tid == 0) *status = (double)(k + 1);
            return;
        }
        if (tid == 0) s_piv[k] = p;
        if (p != k)
            for (int j = tid; j < n; j += blockDim.x) {
                const double t = C[(size_t)k * n + j];
                C[(size_t)k * n + j] = C[(size_t)p * n + j];
                C[(size_t)p * n + j] = t;
            }
        __syncthreads(); // (also: nobody overwrites s_val of this step before everyone has folded it)
        const double piv = 1.0 / C[(size_t)k * n + k];
        for (int i = wv; i < n; i += nw) {
            if (i == k) continue;
            const double f = C[(size_t)i * n + k] * piv;
            for (int j = lane; j < n; j += 64)
                if (j != k) C[(size_t)i * n + j] -= f * C[(size_t)k * n + j];
        }
        __syncthreads();
        for (int j = tid; j < n; j += blockDim.x)
            if (j != k) { C[(size_t)k * n + j] *= piv; C[(size_t)j * n + k] *= -piv; }
        if (tid == 0) C[(size_t)k * n + k] = piv;
        __syncthreads();
    }
    if (tid == 0) { // result[:, j] = C[:, map[j]]: the column swaps (k, p_k) for k = n − 1 … 0, composed
        for (int j = 0; j < n; ++j) s_map[j] = j;
        for (int k = n - 1; k >= 0; --k) {
            const int p = s_piv[k];
            const int t = s_map[k]; s_map[k] = s_map[p]; s_map[p] = t;
        }
        *status = 0.0;
    }
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += nw) { // (uniform trip count: the barrier below is reached by every wave)
        const int i = i0 + wv;
        double v[MG_COARSEST_MAX / 64];
#pragma unroll
        for (int t = 0; t < MG_COARSEST_MAX / 64; ++t) {
            const int j = lane + 64 * t;
            v[t] = i < n && j < n ? C[(size_t)i * n + s_map[j]] : 0.0;
        }
        // A lane stores to column j what another lane of the same wave loaded from column s_map[j], and a lane's store depends on its own loads only:
        // the barrier brings the wait for every lane's loads (vmcnt 0) in front of the first store.  Nothing is ordered between waves: a row is one wave's.
        __syncthreads();
#pragma unroll
        for (int t = 0; t < MG_COARSEST_MAX / 64; ++t) {
            const int j = lane + 64 * t;
            if (i < n && j < n) C[(size_t)i * n + j] = v[t];
        }
    }
}

// x = C r, dense: one wavefront per row
__global__ void __launch_bounds__(256)
k_mg_dense_apply(int n, const double *__restrict__ C, const double *__restrict__ r, double *__restrict__ x)
{
    const int lane = threadIdx.x & 63;
    const int i = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (i >= n) return;
    double s = 0.0;
    for (int j = lane; j < n; j += 64) s += C[(size_t)i * n + j] * r[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) x[i] = s;
}

// one workgroup: *out = the sum (MAX: the maximum; the partials folded here are absolute values) of part[0 … nb) in one fixed order — strided lane
// folds from the lane's own partial, then an LDS tree
template <bool MAX>
__global__ void __launch_bounds__(256) k_fold_partials(int nb, const double *__restrict__ part, double *__restrict__ out)
{
    __shared__ double sm[256];
    double v = (int)threadIdx.x < nb ? part[threadIdx.x] : 0.0;
    for (int k = threadIdx.x + 256; k < nb; k += 256) v = MAX ? fmax(v, part[k]) : v + part[k];
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] = MAX ? fmax(sm[threadIdx.x], sm[threadIdx.x + o]) : sm[threadIdx.x] + sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sm[0];
}

static void free_plans(tb_mg *mg)
{
    for (MgLevel &L : mg->lv) {
        L.release();
        void *ptrs[] = {L.d_A, L.d_presc, L.d_pptr, L.d_rptr, L.d_gptr, L.d_cdiag, L.d_pcol, L.d_rcol, L.d_pexp, L.d_rexp, L.d_gterms, L.d_brow};
        for (void *p : ptrs) if (p) (void)hipFree(p);
        L.d_A = nullptr; L.d_presc = nullptr; L.d_pptr = L.d_rptr = L.d_gptr = L.d_cdiag = nullptr;
        L.d_pcol = L.d_rcol = nullptr; L.d_pexp = L.d_rexp = nullptr; L.d_gterms = nullptr; L.d_brow = nullptr;
        L.blocked = false; L.n_terms = 0;
        L.A = nullptr;
    }
    if (mg->d_cinv) (void)hipFree(mg->d_cinv);
    mg->d_cinv = nullptr;
    if (mg->amg) (void)tb_amg_destroy(mg->amg);
    mg->amg = nullptr;
    mg->planned = mg->ready = false;
}

// tb_mg_set_coarse_amg: the AMG hierarchy on the level-0 pattern, labelled by the components of its field
static int create_coarse_amg(tb_mg *mg)
{
    tb_pattern *pat = mg->lv[0].pat;
    const tb_mesh *m = pat->mesh;
    std::vector<int8_t> comp;
    if (m->ncomp > 1) {
        comp.assign((size_t)m->ndofs, 0);
        for (size_t q = 0; q < m->h_cell_dofs.size(); ++q) // local dof l of a cell carries component l mod ncomp, in any numbering
            comp[(size_t)m->h_cell_dofs[q]] = (int8_t)((q % (size_t)m->ndpc) % (size_t)m->ncomp);
    }
    TB_TRY(tb_amg_create(pat, comp.empty() ? nullptr : comp.data(), mg->amg_theta, mg->amg_max_coarse, mg->amg_max_levels, &mg->amg));
    TB_TRY(tb_amg_set_general(mg->amg, mg->general ? 1 : 0)); // the mode the hierarchy has when its plans are built; tb_mg_set_general forwards every later change
    if (mg->amg_nns_k) {
        TB_REQUIRE((int64_t)mg->amg_nns_node.size() == pat->n_rows, "tb_mg_set_coarse_amg_near_nullspace: the arrays were sized for %lld dofs, level 0 has %lld",
                   (long long)mg->amg_nns_node.size(), (long long)pat->n_rows);
        TB_TRY(tb_amg_set_near_nullspace(mg->amg, mg->amg_nns_nodes, mg->amg_nns_node.data(), mg->amg_nns_k, mg->amg_nns_B.data()));
    }
    return TB_OK;
}

static mgplan::LevelView view_of(const tb_pattern *p)
{
    const tb_mesh *m = p->mesh;
    return mgplan::LevelView{m->n_nodes, m->n_cells, m->ndofs, m->nverts, m->ncomp, m->h_conn.data(), m->h_cell_dofs.data(), p->h_rowptr.data(), p->h_colidx.data(), m->nb};
}

// symbolic phase: transfers, Galerkin plans, level storage, the SpMV plan of every level
int build_plans(tb_mg *mg)
{
    tb_device *dev = mg->dev;
    TB_NO_CAPTURE(dev);
    const int nl = (int)mg->lv.size();
    for (int l = 0; l < nl; ++l) {
        TB_REQUIRE(mg->lv[l].pat, "tb_mg_setup: level %d has no pattern (tb_mg_set_level)", l);
        TB_REQUIRE(l == 0 || mg->lv[l].has_transfer, "tb_mg_setup: level %d has no transfer to level %d (tb_mg_set_transfer, tb_mg_set_p_transfer)", l, l - 1);
        if (mg->lv[l].pat->mesh->field_kind == TB_HEX27)
            TB_REQUIRE(l == nl - 1 && mg->lv[l].p_transfer, "tb_mg_setup: level %d carries a second-order field: it must be the finest level, with a p-transfer below it (tb_mg_set_p_transfer)", l);
        else
            TB_REQUIRE(l == 0 || !mg->lv[l].p_transfer, "tb_mg_setup: level %d has a p-transfer below it but carries a first-order field", l);
    }
    if (!mg->coarse_amg && mg->lv[0].pat->n_rows > MG_COARSEST_MAX) {
        set_error("tb_mg_setup: the coarsest level has %lld dofs; its dense inverse takes at most %d - add a level%s", (long long)mg->lv[0].pat->n_rows, MG_COARSEST_MAX,
                  nl == 2 && mg->lv[1].p_transfer ? " (h-levels below the p-level: ChainedMGPrecon(PMGPrecon(), GMGPrecon(gh)))" : "");
        return TB_ERR_UNSUPPORTED;
    }
    PlanTimer timer("multigrid");
    for (int l = nl - 1; l >= 0; --l) {
        MgLevel &L = mg->lv[l];
        L.n = L.pat->n_rows;
        L.nnz = L.pat->nnz;
        if (l > 0) {
            MgLevel &Cl = mg->lv[l - 1];
            const mgplan::LevelView fv = view_of(L.pat), cv = view_of(Cl.pat);
            const uint8_t *flags = L.h_presc.empty() ? nullptr : L.h_presc.data();
            mgplan::Transfer t;
            mgplan::Galerkin g;
            if (L.p_transfer) TB_TRY(mgplan::build_p_transfer(fv, cv, flags, t));
            else {
                TB_REQUIRE((int64_t)L.parent_ptr.size() == fv.n_nodes + 1, "tb_mg_setup: the transfer of level %d lists %lld nodes, its pattern's grid has %lld", l,
                           (long long)L.parent_ptr.size() - 1, (long long)fv.n_nodes);
                TB_TRY(mgplan::build_transfer(fv, cv, L.parent_ptr.data(), L.parent_idx.data(), flags, t));
            }
            timer.lap("transfer");
            // The blocked plan where both patterns are CSRs of 3 × 3 blocks (what the SpMV's examination decides) and P moves node triples: the
            // p-level, whose fine matrix is the one that outgrows the per-dof term word.  h-levels stay on the per-dof plan.  TB_MG_GALERKIN=dof
            // keeps the p-level there too (measurements).
            TB_TRY(spmv_plans(L.pat));
            TB_TRY(spmv_plans(Cl.pat));
            const bool dof_only = tune_env("TB_MG_GALERKIN") && !strcmp(tune_env("TB_MG_GALERKIN"), "dof"); // (read per hierarchy: one process times both)
            L.blocked = L.p_transfer && !dof_only && L.pat->b3 > 0 && Cl.pat->b3 > 0 && mgplan::node_blocked(t);
            if (L.blocked) TB_TRY(mgplan::build_galerkin_blocked(fv, cv, t, g));
            else TB_TRY(mgplan::build_galerkin(fv, cv, t, flags, g));
            timer.lap("galerkin plan");
            if (L.blocked) {
                TB_TRY(upload(dev, g.fine_brow, &L.d_brow));
                TB_TRY(upload(dev, g.coarse_brow, &Cl.d_brow));
            }
            if (flags) Cl.h_presc = t.coarse_prescribed; else Cl.h_presc.clear();
            L.n_terms = (int64_t)g.terms.size();
            TB_TRY(upload_all(dev, t.p_ptr, &L.d_pptr, t.p_col, &L.d_pcol, t.p_exp, &L.d_pexp, t.r_ptr, &L.d_rptr, t.r_col, &L.d_rcol, t.r_exp, &L.d_rexp,
                              g.ptr, &L.d_gptr, g.terms, &L.d_gterms, g.diag_pos, &L.d_cdiag));
        }
        if (!L.h_presc.empty() && l < nl - 1) TB_TRY(upload(dev, L.h_presc, &L.d_presc));
        TB_TRY(L.alloc(L.n));
        if (l < nl - 1) TB_HIP(hipMalloc((void **)&L.d_A, sizeof(double) * (size_t)std::max<int64_t>(L.nnz, 1)));
        TB_TRY(spmv_plans(L.pat));
    }
    if (mg->coarse_amg) TB_TRY(create_coarse_amg(mg));
    else TB_HIP(hipMalloc((void **)&mg->d_cinv, sizeof(double) * (size_t)mg->lv[0].n * (size_t)mg->lv[0].n));
    if (!mg->d_scal) TB_HIP(hipMalloc((void **)&mg->d_scal, 16 * sizeof(double)));
    mg->planned = true;
    return TB_OK;
}

// A_{l−1} = Pᵀ A_l P by the plan of level l (fine_level), then the diagonal of the prescribed coarse dofs; enqueues only
static void launch_galerkin(tb_mg *mg, int fine_level)
{
    tb_device *dev = mg->dev;
    MgLevel &U = mg->lv[fine_level], &L = mg->lv[fine_level - 1];
    if (U.blocked) {
        const int64_t ncb = L.nnz / 9;
        if (U.d_presc)
            hipLaunchKernelGGL(k_mg_galerkin_b3<true>, dim3(blocks_of(ncb * 16, 256)), dim3(256), 0, dev->stream, ncb, U.d_gptr, U.d_gterms, U.d_brow, U.pat->d_bcol,
                               U.pat->d_rowptr, U.A, U.d_presc, L.d_brow, L.pat->d_bcol, L.pat->d_rowptr, L.d_presc, L.d_A);
        else
            hipLaunchKernelGGL(k_mg_galerkin_b3<false>, dim3(blocks_of(ncb * 16, 256)), dim3(256), 0, dev->stream, ncb, U.d_gptr, U.d_gterms, U.d_brow, U.pat->d_bcol,
                               U.pat->d_rowptr, U.A, (const uint8_t *)nullptr, L.d_brow, L.pat->d_bcol, L.pat->d_rowptr, (const uint8_t *)nullptr, L.d_A);
    } else
        hipLaunchKernelGGL(k_mg_galerkin, dim3(blocks_of(L.nnz * 16, 256)), dim3(256), 0, dev->stream, L.nnz, U.d_gptr, U.d_gterms, U.A, L.d_A);
    if (L.d_presc) launch_fill_diag(dev, L.n, U.d_cdiag, L.d_presc, L.d_A);
}

// (tb_mg_internal.hpp) one value plane through the per-dof plan of fine_level for the block cycle of tb_bidomain_mg.hip, and the kernels the family shares
void launch_galerkin_plane(tb_mg *mg, int fine_level, const double *Af, double *Ac)
{
    MgLevel &U = mg->lv[fine_level], &L = mg->lv[fine_level - 1];
    hipLaunchKernelGGL(k_mg_galerkin, dim3(blocks_of(L.nnz * 16, 256)), dim3(256), 0, mg->dev->stream, L.nnz, U.d_gptr, U.d_gterms, Af, Ac);
}
void launch_dense_apply(tb_device *dev, int n, const double *C, const double *r, double *x)
{
    hipLaunchKernelGGL(k_mg_dense_apply, dim3(blocks_of((int64_t)n * 64, 256)), dim3(256), 0, dev->stream, n, C, r, x);
}

void launch_cheb_step(tb_device *dev, int mode, int64_t n, ChebSchedule::Step c, const double *dinv, const double *r, const double *w, double *d, double *x)
{
    auto *k = mode == 0 ? k_mg_cheb<0> : mode == 1 ? k_mg_cheb<1> : k_mg_cheb<2>;
    hipLaunchKernelGGL(k, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, c.c1, c.c2, dinv, r, w, d, x);
}
void launch_dense_inverse(tb_device *dev, int n, const int64_t *rowptr, const int32_t *colidx, const double *nz, double *C, bool general)
{
    if (general) hipLaunchKernelGGL(k_mg_dense_inverse_pivot, dim3(1), dim3(MG_COARSEST_MAX), 0, dev->stream, n, rowptr, colidx, nz, C, dev->d_readback);
    else hipLaunchKernelGGL(k_mg_dense_inverse, dim3(1), dim3(1024), 0, dev->stream, n, rowptr, colidx, nz, C);
}
int dense_inverse_status(tb_device *dev, const char *who, int level, int n)
{
    double step = 0.0;
    TB_TRY(read_back(dev, &step, dev->d_readback, 1));
    if (step != 0.0) {
        set_error("%s: the operator of level %d (%d dofs, inverted densely) is singular or not finite: no usable pivot at elimination step %d of the pivoted "
                  "Gauss-Jordan inverse (general mode)", who, level, n, (int)step - 1);
        return TB_ERR_BAD_ARG;
    }
    return TB_OK;
}
void launch_fill_diag(tb_device *dev, int64_t n, const int64_t *diagpos, const uint8_t *flags, double *A)
{
    hipLaunchKernelGGL(k_mg_fill_diag, dim3(1), dim3(1024), 0, dev->stream, n, diagpos, flags, A);
}
void launch_fold_sum(tb_device *dev, int nb, const double *part, double *out) { hipLaunchKernelGGL(k_fold_partials<false>, dim3(1), dim3(256), 0, dev->stream, nb, part, out); }
void launch_fold_max(tb_device *dev, int nb, const double *part, double *out) { hipLaunchKernelGGL(k_fold_partials<true>, dim3(1), dim3(256), 0, dev->stream, nb, part, out); }

// x = M_l⁻¹ r: V(degree, degree) from x = 0; enqueues only
static int cycle(tb_mg *mg, int l, const double *r, double *x)
{
    tb_device *dev = mg->dev;
    MgLevel &L = mg->lv[l];
    if (l == 0) {
        if (mg->amg) return amg_apply_cb(mg->amg, r, x);
        launch_dense_apply(dev, (int)L.n, mg->d_cinv, r, x);
        return TB_OK;
    }
    MgLevel &Cl = mg->lv[l - 1];
    auto product = [&](const double *u, double *y) { return launch_spmv(L.pat, L.A, u, 1.0, 0.0, y); };
    TB_TRY(cheb_smooth(dev, L.n, L, L.lmax, mg->ratio, mg->degree, r, x, true, product));
    TB_TRY(product(x, L.w));
    hipLaunchKernelGGL(k_mg_restrict, dim3(blocks_of(Cl.n, 256)), dim3(256), 0, dev->stream, Cl.n, L.d_rptr, L.d_rcol, L.d_rexp, r, (const double *)L.w, Cl.r);
    TB_TRY(cycle(mg, l - 1, Cl.r, Cl.x));
    hipLaunchKernelGGL(k_mg_prolong<true>, dim3(blocks_of(L.n, 256)), dim3(256), 0, dev->stream, L.n, L.d_pptr, L.d_pcol, L.d_pexp, (const double *)Cl.x, x);
    return cheb_smooth(dev, L.n, L, L.lmax, mg->ratio, mg->degree, r, x, false, product);
}

static int mg_apply_cb(void *ctx, const double *r, double *z)
{
    tb_mg *mg = (tb_mg *)ctx;
    const int rc = cycle(mg, (int)mg->lv.size() - 1, r, z);
    if (rc) return rc;
    TB_HIP(hipGetLastError());
    return TB_OK;
}

} // namespace tb

using namespace tb;

int tb_mg_create(tb_device *dev, int n_levels, tb_mg **out)
{
    TB_REQUIRE(dev && out, "tb_mg_create: NULL argument");
    *out = nullptr;
    TB_REQUIRE(n_levels >= 2 && n_levels <= 32, "tb_mg_create: n_levels must be in 2..32 (got %d)", n_levels);
    tb_mg *mg = new tb_mg;
    mg->dev = dev;
    mg->lv.resize((size_t)n_levels);
    *out = mg;
    return TB_OK;
}

int tb_mg_destroy(tb_mg *mg)
{
    if (!mg) return TB_OK;
    (void)hipSetDevice(mg->dev->id);
    free_plans(mg);
    if (mg->d_scal) (void)hipFree(mg->d_scal);
    delete mg;
    return TB_OK;
}

int tb_mg_set_level(tb_mg *mg, int level, tb_pattern *pat)
{
    TB_REQUIRE(mg && pat, "tb_mg_set_level: NULL argument");
    TB_REQUIRE(level >= 0 && level < (int)mg->lv.size(), "tb_mg_set_level: level %d of %d", level, (int)mg->lv.size());
    TB_REQUIRE(pat->mesh && pat->mesh->dev == mg->dev, "tb_mg_set_level: the pattern lives on another device");
    if (pat->mesh->geom_kind != TB_HEX8 || (pat->mesh->field_kind != TB_HEX8 && pat->mesh->field_kind != TB_HEX27)) {
        set_error("tb_mg_set_level: the multigrid covers first-order fields on hexahedra and a second-order field on the finest level (no tetrahedra)");
        return TB_ERR_UNSUPPORTED;
    }
    TB_HIP(hipSetDevice(mg->dev->id));
    free_plans(mg);
    mg->lv[level].pat = pat;
    return TB_OK;
}

int tb_mg_set_transfer(tb_mg *mg, int fine_level, int64_t n_fine_nodes, const int64_t *parent_ptr, const int32_t *parent_idx)
{
    TB_REQUIRE(mg && parent_ptr && parent_idx, "tb_mg_set_transfer: NULL argument");
    TB_REQUIRE(fine_level >= 1 && fine_level < (int)mg->lv.size(), "tb_mg_set_transfer: fine_level %d of 1..%d", fine_level, (int)mg->lv.size() - 1);
    MgLevel &L = mg->lv[fine_level], &Cl = mg->lv[fine_level - 1];
    TB_REQUIRE(L.pat && Cl.pat, "tb_mg_set_transfer: set the patterns of levels %d and %d first (tb_mg_set_level)", fine_level, fine_level - 1);
    if (L.pat->mesh->field_kind != TB_HEX8 || Cl.pat->mesh->field_kind != TB_HEX8) {
        set_error("tb_mg_set_transfer: an h-transfer joins two first-order fields; level %d carries a second-order field (tb_mg_set_p_transfer joins it to the first-order field on its grid)",
                  L.pat->mesh->field_kind != TB_HEX8 ? fine_level : fine_level - 1);
        return TB_ERR_UNSUPPORTED;
    }
    TB_REQUIRE(L.pat->mesh->ncomp == Cl.pat->mesh->ncomp, "tb_mg_set_transfer: the levels carry %d and %d components", L.pat->mesh->ncomp, Cl.pat->mesh->ncomp);
    TB_REQUIRE(n_fine_nodes == L.pat->mesh->n_nodes, "tb_mg_set_transfer: %lld fine nodes, but the grid of level %d has %lld: the pattern does not match the transfer",
               (long long)n_fine_nodes, fine_level, (long long)L.pat->mesh->n_nodes);
    TB_REQUIRE(parent_ptr[0] == 0, "tb_mg_set_transfer: parent_ptr does not start at 0");
    const int64_t ncn = Cl.pat->mesh->n_nodes;
    TB_REQUIRE(ncn <= n_fine_nodes, "tb_mg_set_transfer: level %d has more nodes than level %d", fine_level - 1, fine_level);
    for (int64_t v = 0; v < n_fine_nodes; ++v) {
        const int64_t np = parent_ptr[v + 1] - parent_ptr[v];
        TB_REQUIRE(np == 1 || np == 2 || np == 4 || np == 8, "tb_mg_set_transfer: node %lld has %lld parents (1, 2, 4 or 8)", (long long)v, (long long)np);
        for (int64_t q = parent_ptr[v]; q < parent_ptr[v + 1]; ++q)
            TB_REQUIRE(parent_idx[q] >= 0 && parent_idx[q] < ncn, "tb_mg_set_transfer: parent %d of node %lld is not a node of level %d (%lld nodes): the pattern does not match the transfer",
                       parent_idx[q], (long long)v, fine_level - 1, (long long)ncn);
        TB_REQUIRE(v >= ncn || (np == 1 && parent_idx[parent_ptr[v]] == v), "tb_mg_set_transfer: coarse node %lld is not its own parent (coarse nodes must be a prefix of the fine nodes)", (long long)v);
    }
    TB_HIP(hipSetDevice(mg->dev->id));
    free_plans(mg);
    L.parent_ptr.assign(parent_ptr, parent_ptr + n_fine_nodes + 1);
    L.parent_idx.assign(parent_idx, parent_idx + parent_ptr[n_fine_nodes]);
    L.has_transfer = true;
    L.p_transfer = false;
    return TB_OK;
}

int tb_mg_set_p_transfer(tb_mg *mg, int fine_level)
{
    TB_REQUIRE(mg, "tb_mg_set_p_transfer: NULL argument");
    const int nl = (int)mg->lv.size();
    TB_REQUIRE(fine_level >= 1 && fine_level < nl, "tb_mg_set_p_transfer: fine_level %d of 1..%d", fine_level, nl - 1);
    MgLevel &L = mg->lv[fine_level], &Cl = mg->lv[fine_level - 1];
    TB_REQUIRE(L.pat && Cl.pat, "tb_mg_set_p_transfer: set the patterns of levels %d and %d first (tb_mg_set_level)", fine_level, fine_level - 1);
    const tb_mesh *f = L.pat->mesh, *c = Cl.pat->mesh;
    if (f->field_kind != TB_HEX27 || c->field_kind != TB_HEX8) {
        set_error("tb_mg_set_p_transfer: a p-transfer joins a second-order field (level %d) to a first-order field (level %d) on hexahedra; the levels carry field kinds %d and %d",
                  fine_level, fine_level - 1, f->field_kind, c->field_kind);
        return TB_ERR_UNSUPPORTED;
    }
    if (fine_level != nl - 1) {
        set_error("tb_mg_set_p_transfer: one p-level, from order 2 to order 1, at the top of the hierarchy: fine_level must be %d (got %d)", nl - 1, fine_level);
        return TB_ERR_UNSUPPORTED;
    }
    TB_REQUIRE(f->n_cells == c->n_cells, "tb_mg_set_p_transfer: levels %d and %d have %lld and %lld cells (a p-transfer joins two fields on the same cells)", fine_level,
               fine_level - 1, (long long)f->n_cells, (long long)c->n_cells);
    TB_REQUIRE(f->ncomp == c->ncomp, "tb_mg_set_p_transfer: the levels carry %d and %d components", f->ncomp, c->ncomp);
    TB_HIP(hipSetDevice(mg->dev->id));
    free_plans(mg);
    L.parent_ptr.clear();
    L.parent_idx.clear();
    L.has_transfer = true;
    L.p_transfer = true;
    return TB_OK;
}

int tb_mg_level_plan(tb_mg *mg, int fine_level, int *blocked, int64_t *n_terms)
{
    TB_REQUIRE(mg && blocked && n_terms, "tb_mg_level_plan: NULL argument");
    TB_REQUIRE(fine_level >= 1 && fine_level < (int)mg->lv.size(), "tb_mg_level_plan: fine_level %d of 1..%d", fine_level, (int)mg->lv.size() - 1);
    TB_REQUIRE(mg->planned, "tb_mg_level_plan: the Galerkin products are planned by tb_mg_setup");
    *blocked = mg->lv[fine_level].blocked ? 1 : 0;
    *n_terms = mg->lv[fine_level].n_terms;
    return TB_OK;
}

int tb_mg_set_prescribed(tb_mg *mg, const uint8_t *d_prescribed_fine)
{
    TB_REQUIRE(mg, "tb_mg_set_prescribed: NULL argument");
    MgLevel &L = mg->lv.back();
    TB_REQUIRE(L.pat, "tb_mg_set_prescribed: set the pattern of the finest level first (tb_mg_set_level)");
    tb_device *dev = mg->dev;
    TB_NO_CAPTURE(dev);
    TB_HIP(hipSetDevice(dev->id));
    free_plans(mg);
    L.h_presc.clear();
    if (!d_prescribed_fine) return TB_OK;
    const size_t n = (size_t)L.pat->n_rows;
    L.h_presc.resize(n);
    TB_HIP(hipMemcpyAsync(L.h_presc.data(), d_prescribed_fine, n, hipMemcpyDeviceToHost, dev->stream));
    TB_SYNC_STREAM(dev);
    bool any = false;
    for (uint8_t &f : L.h_presc) { f = f ? 1 : 0; any |= f != 0; }
    if (!any) L.h_presc.clear();
    return TB_OK;
}

int tb_mg_set_coarse_amg(tb_mg *mg, double theta, int max_coarse, int max_levels)
{
    TB_REQUIRE(mg, "tb_mg_set_coarse_amg: NULL argument");
    TB_TRY(check_amg_args("tb_mg_set_coarse_amg", theta, max_coarse, max_levels));
    TB_NO_CAPTURE(mg->dev);
    TB_HIP(hipSetDevice(mg->dev->id));
    free_plans(mg);
    mg->coarse_amg = true;
    mg->amg_theta = theta;
    mg->amg_max_coarse = max_coarse;
    mg->amg_max_levels = max_levels;
    return TB_OK;
}

int tb_mg_set_coarse_amg_near_nullspace(tb_mg *mg, int64_t n_nodes, const int32_t *node_of_dof, int k, const double *B)
{
    TB_REQUIRE(mg && node_of_dof && B, "tb_mg_set_coarse_amg_near_nullspace: NULL argument");
    TB_REQUIRE(mg->coarse_amg, "tb_mg_set_coarse_amg_near_nullspace: no AMG on level 0 (tb_mg_set_coarse_amg comes first)");
    TB_REQUIRE(k >= 1 && k <= 6, "tb_mg_set_coarse_amg_near_nullspace: k = %d candidates; 1 to 6 are supported", k);
    TB_REQUIRE(n_nodes >= 0, "tb_mg_set_coarse_amg_near_nullspace: negative node count");
    TB_NO_CAPTURE(mg->dev);
    TB_HIP(hipSetDevice(mg->dev->id));
    free_plans(mg);
    const int64_t n = 3 * n_nodes; // (3 dofs per node: tb_amg_set_near_nullspace checks the map against level 0 when the hierarchy is created)
    mg->amg_nns_k = k;
    mg->amg_nns_nodes = n_nodes;
    mg->amg_nns_node.assign(node_of_dof, node_of_dof + n);
    mg->amg_nns_B.assign(B, B + n * k);
    return TB_OK;
}

int tb_mg_set_general(tb_mg *mg, int general)
{
    TB_REQUIRE(mg, "tb_mg_set_general: NULL argument");
    if (mg->general == (general != 0)) return TB_OK;
    mg->general = general != 0;
    mg->ready = false; // the numeric phase is redone by the next tb_mg_setup (the plans stay); the AMG below level 0 takes the flag there
    if (mg->amg) TB_TRY(tb_amg_set_general(mg->amg, general));
    return TB_OK;
}

int tb_mg_coarse_amg(tb_mg *mg, tb_amg **out)
{
    TB_REQUIRE(mg && out, "tb_mg_coarse_amg: NULL argument");
    TB_REQUIRE(mg->ready, "tb_mg_coarse_amg: no numeric setup yet (tb_mg_setup)");
    *out = mg->amg;
    return TB_OK;
}

int tb_mg_setup(tb_mg *mg, const double *d_Anz_fine, int degree, double interval_ratio)
{
    TB_REQUIRE(mg && d_Anz_fine, "tb_mg_setup: NULL argument");
    TB_TRY(check_smoother_args("tb_mg_setup", degree, interval_ratio));
    tb_device *dev = mg->dev;
    TB_NO_CAPTURE(dev); // builds plans, reads λmax back
    TB_HIP(hipSetDevice(dev->id));
    mg->ready = false;
    if (!mg->planned) {
        const int rc = build_plans(mg);
        if (rc) { free_plans(mg); return rc; }
    }
    const int nl = (int)mg->lv.size();
    mg->degree = degree;
    mg->ratio = interval_ratio;
    MgLevel &F = mg->lv[nl - 1];
    F.A = d_Anz_fine;
    if (!F.h_presc.empty() && !F.d_presc) TB_TRY(upload(dev, F.h_presc, &F.d_presc));
    for (int l = nl - 1; l >= 0; --l) {
        MgLevel &L = mg->lv[l];
        if (l < nl - 1) { // A_l = Pᵀ A_{l+1} P
            launch_galerkin(mg, l + 1);
            L.A = L.d_A;
        }
        if (l == 0) break;
        TB_TRY(launch_extract_inverse_diagonal(L.pat, L.A, L.dinv));
        if (L.d_presc) hipLaunchKernelGGL(k_mg_mask, dim3(grid_for(dev, L.n, 256)), dim3(256), 0, dev->stream, L.n, L.d_presc, L.dinv);
        // scratch of the estimate: w | d, x, r and the sixth vector of the level's block (none of them holds anything between applications)
        TB_TRY(estimate_lambda_max(L.pat, L.A, L.dinv, L.w, L.d, L.x, L.r, L.r + L.n, mg->d_scal, &L.lmax));
    }
    MgLevel &C0 = mg->lv[0];
    if (mg->amg) { // the AMG below level 0: planned at its first setup, numeric phase only afterwards
        const int rc = tb_amg_setup(mg->amg, C0.A, degree, interval_ratio);
        if (rc) { free_plans(mg); return rc; }
    } else {
        launch_dense_inverse(dev, (int)C0.n, C0.pat->d_rowptr, C0.pat->d_colidx, C0.A, mg->d_cinv, mg->general);
        if (mg->general) TB_TRY(dense_inverse_status(dev, "tb_mg_setup", 0, (int)C0.n));
    }
    TB_HIP(hipGetLastError());
    mg->ready = true;
    return TB_OK;
}

int tb_mg_apply(tb_mg *mg, const double *d_r, double *d_z)
{
    TB_REQUIRE(mg && d_r && d_z, "tb_mg_apply: NULL argument");
    TB_REQUIRE(mg->ready, "tb_mg_apply: no numeric setup yet (tb_mg_setup)");
    TB_REQUIRE(d_r != d_z, "tb_mg_apply: r and z alias");
    TB_HIP(hipSetDevice(mg->dev->id));
    return mg_apply_cb(mg, d_r, d_z);
}

int tb_mg_level_matrix(tb_mg *mg, int level, const double **d_nzval)
{
    TB_REQUIRE(mg && d_nzval, "tb_mg_level_matrix: NULL argument");
    TB_REQUIRE(level >= 0 && level < (int)mg->lv.size(), "tb_mg_level_matrix: level %d of %d", level, (int)mg->lv.size());
    TB_REQUIRE(mg->ready, "tb_mg_level_matrix: no numeric setup yet (tb_mg_setup)");
    *d_nzval = mg->lv[level].A;
    return TB_OK;
}

int tb_mg_galerkin(tb_mg *mg, int fine_level)
{
    TB_REQUIRE(mg, "tb_mg_galerkin: NULL argument");
    TB_REQUIRE(fine_level >= 1 && fine_level < (int)mg->lv.size(), "tb_mg_galerkin: fine_level %d of 1..%d", fine_level, (int)mg->lv.size() - 1);
    TB_REQUIRE(mg->ready, "tb_mg_galerkin: no numeric setup yet (tb_mg_setup)");
    TB_HIP(hipSetDevice(mg->dev->id));
    launch_galerkin(mg, fine_level);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_mg_level_lambda_max(tb_mg *mg, int level, double *lmax)
{
    TB_REQUIRE(mg && lmax, "tb_mg_level_lambda_max: NULL argument");
    TB_REQUIRE(level >= 1 && level < (int)mg->lv.size(), "tb_mg_level_lambda_max: level %d of 1..%d (the coarsest level is inverted, not smoothed)", level, (int)mg->lv.size() - 1);
    TB_REQUIRE(mg->ready, "tb_mg_level_lambda_max: no numeric setup yet (tb_mg_setup)");
    *lmax = mg->lv[level].lmax;
    return TB_OK;
}

int tb_mg_prolong(tb_mg *mg, int fine_level, const double *d_xc, double *d_xf)
{
    TB_REQUIRE(mg && d_xc && d_xf, "tb_mg_prolong: NULL argument");
    TB_REQUIRE(fine_level >= 1 && fine_level < (int)mg->lv.size(), "tb_mg_prolong: fine_level %d of 1..%d", fine_level, (int)mg->lv.size() - 1);
    TB_REQUIRE(mg->planned, "tb_mg_prolong: the transfers are planned by tb_mg_setup");
    TB_HIP(hipSetDevice(mg->dev->id));
    MgLevel &L = mg->lv[fine_level];
    hipLaunchKernelGGL(k_mg_prolong<false>, dim3(blocks_of(L.n, 256)), dim3(256), 0, mg->dev->stream, L.n, L.d_pptr, L.d_pcol, L.d_pexp, d_xc, d_xf);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_mg_restrict(tb_mg *mg, int fine_level, const double *d_rf, double *d_rc)
{
    TB_REQUIRE(mg && d_rf && d_rc, "tb_mg_restrict: NULL argument");
    TB_REQUIRE(fine_level >= 1 && fine_level < (int)mg->lv.size(), "tb_mg_restrict: fine_level %d of 1..%d", fine_level, (int)mg->lv.size() - 1);
    TB_REQUIRE(mg->planned, "tb_mg_restrict: the transfers are planned by tb_mg_setup");
    TB_HIP(hipSetDevice(mg->dev->id));
    MgLevel &L = mg->lv[fine_level], &Cl = mg->lv[fine_level - 1];
    hipLaunchKernelGGL(k_mg_restrict, dim3(blocks_of(Cl.n, 256)), dim3(256), 0, mg->dev->stream, Cl.n, L.d_rptr, L.d_rcol, L.d_rexp, d_rf, (const double *)nullptr, d_rc);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_pcg_solve_mg(tb_pattern *pat, const double *d_Anz, const double *d_b, double *d_x, double rtol, double atol, int maxiter, tb_mg *mg, int *iters,
                    double *resnorm)
{
    TB_REQUIRE(pat && d_Anz && d_b && d_x && mg, "tb_pcg_solve_mg: NULL argument");
    TB_REQUIRE(rtol >= 0 && atol >= 0 && maxiter >= 0, "tb_pcg_solve_mg: negative tolerance or iteration limit");
    TB_REQUIRE(mg->ready, "tb_pcg_solve_mg: no numeric setup yet (tb_mg_setup)");
    TB_REQUIRE(mg->lv.back().pat == pat, "tb_pcg_solve_mg: the pattern is not the finest level of the hierarchy");
    TB_REQUIRE(mg->lv.back().A == d_Anz, "tb_pcg_solve_mg: the hierarchy was set up with another matrix array (tb_mg_setup follows every new matrix)");
    TB_HIP(hipSetDevice(pat->mesh->dev->id));
    return launch_pcg_apply(pat, d_Anz, d_b, d_x, rtol, atol, maxiter, mg_apply_cb, mg, "multigrid preconditioner", iters, resnorm);
}

int tb_gmres_solve_mg(tb_pattern *pat, const double *d_Anz, const double *d_b, double *d_x, double rtol, double atol, int maxiter, int restart, tb_mg *mg,
                      int *iters, double *resnorm)
{
    TB_REQUIRE(pat && d_Anz && d_b && d_x && mg, "tb_gmres_solve_mg: NULL argument");
    TB_REQUIRE(rtol >= 0 && atol >= 0 && maxiter >= 0, "tb_gmres_solve_mg: negative tolerance or iteration limit");
    TB_REQUIRE(restart >= 1 && restart <= 1000, "tb_gmres_solve_mg: restart must be in 1..1000 (got %d)", restart);
    TB_REQUIRE(mg->ready, "tb_gmres_solve_mg: no numeric setup yet (tb_mg_setup; tb_mg_set_general asks for a new one)");
    TB_REQUIRE(mg->lv.back().pat == pat, "tb_gmres_solve_mg: the pattern is not the finest level of the hierarchy");
    TB_REQUIRE(mg->lv.back().A == d_Anz, "tb_gmres_solve_mg: the hierarchy was set up with another matrix array (tb_mg_setup follows every new matrix)");
    TB_HIP(hipSetDevice(pat->mesh->dev->id));
    return launch_gmres_apply(pat, d_Anz, d_b, d_x, rtol, atol, maxiter, restart, mg_apply_cb, mg, "tb_gmres_solve_mg", iters, resnorm);
}

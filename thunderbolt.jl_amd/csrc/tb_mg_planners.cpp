// tb_mg_planners.cpp — prolongation, restriction and Galerkin plans of the multigrid: h-levels on nested first-order hexahedral grids and the p-level
// from a second-order to a first-order field on the same cells (src/solver/linear/multigrid.jl, ext/ThunderboltFerriteMultigridExt.jl: the reference
// forms PᵀAP with sparse products for every new Jacobian; here the product is planned once per hierarchy — per dof, or per 3 × 3 block — and
// evaluated by a gather kernel).  Pure host code, standard library only.
#include "tb_mg_planners.hpp"

#include <algorithm>
#include <cmath>
#ifdef _OPENMP
#include <omp.h>
#endif

namespace tb {
namespace mgplan {

// the planners share the host with the caller's own threads: at most 16, as the other planners run under
static int plan_threads()
{
#ifdef _OPENMP
    return std::max(1, std::min(16, omp_get_max_threads()));
#else
    return 1;
#endif
}

int node_dof_table(const LevelView &lv, std::vector<int32_t> &node_dofs)
{
    const int nc = lv.ncomp;
    node_dofs.assign((size_t)lv.n_nodes * nc, -1);
    for (int64_t c = 0; c < lv.n_cells; ++c)
        for (int a = 0; a < lv.nverts; ++a) {
            const int32_t v = lv.conn[c * lv.nverts + a];
            if (v < 0 || v >= lv.n_nodes) { set_error("multigrid plan: node id %d out of range in cell %lld", v, (long long)c); return ERR_BAD_ARG; }
            for (int k = 0; k < nc; ++k) {
                const int32_t d = lv.cell_dofs[(c * lv.nverts + a) * nc + k];
                if (d < 0 || d >= lv.ndofs) { set_error("multigrid plan: dof id %d out of range in cell %lld", d, (long long)c); return ERR_BAD_ARG; }
                int32_t &slot = node_dofs[(size_t)v * nc + k];
                if (slot >= 0 && slot != d) { set_error("multigrid plan: node %d carries two dofs for component %d (a discontinuous field)", v, k); return ERR_BAD_ARG; }
                slot = d;
            }
        }
    for (int64_t v = 0; v < lv.n_nodes; ++v)
        if (node_dofs[(size_t)v * nc] < 0) { set_error("multigrid plan: node %lld belongs to no cell", (long long)v); return ERR_BAD_ARG; }
    return 0;
}

static int exponent_of(int64_t nparents)
{
    return nparents == 1 ? 0 : nparents == 2 ? 1 : nparents == 4 ? 2 : nparents == 8 ? 3 : -1;
}

// Pᵀ row-wise from P row-wise: a counting transpose visits the fine dofs in ascending order, so every row of Pᵀ is ascending
static void transpose(Transfer &out)
{
    out.r_ptr.assign((size_t)out.n_coarse + 1, 0);
    for (int32_t c : out.p_col) ++out.r_ptr[(size_t)c + 1];
    for (int64_t I = 0; I < out.n_coarse; ++I) out.r_ptr[I + 1] += out.r_ptr[I];
    out.r_col.resize(out.p_col.size());
    out.r_exp.resize(out.p_col.size());
    std::vector<int64_t> cur(out.r_ptr.begin(), out.r_ptr.end() - 1);
    for (int64_t d = 0; d < out.n_fine; ++d)
        for (int64_t q = out.p_ptr[d]; q < out.p_ptr[d + 1]; ++q) {
            const int64_t w = cur[out.p_col[q]]++;
            out.r_col[w] = (int32_t)d;
            out.r_exp[w] = out.p_exp[q];
        }
}

int build_transfer(const LevelView &fine, const LevelView &coarse, const int64_t *parent_ptr, const int32_t *parent_idx, const uint8_t *fine_prescribed,
                   Transfer &out)
{
    if (fine.ncomp != coarse.ncomp) { set_error("multigrid plan: the levels carry %d and %d components", fine.ncomp, coarse.ncomp); return ERR_BAD_ARG; }
    if (coarse.n_nodes > fine.n_nodes) { set_error("multigrid plan: the coarse level has more nodes than the fine one"); return ERR_BAD_ARG; }
    const int nc = fine.ncomp;
    std::vector<int32_t> fd, cd;
    if (int rc = node_dof_table(fine, fd)) return rc;
    if (int rc = node_dof_table(coarse, cd)) return rc;
    out = Transfer();
    out.n_fine = fine.ndofs;
    out.n_coarse = coarse.ndofs;
    // a coarse node is the fine node of the same number (uniform_refinement appends): its dofs inherit the flags
    out.coarse_prescribed.assign((size_t)coarse.ndofs, 0);
    for (int64_t v = 0; v < coarse.n_nodes; ++v) {
        if (parent_ptr[v + 1] - parent_ptr[v] != 1 || parent_idx[parent_ptr[v]] != v) {
            set_error("multigrid plan: coarse node %lld is not its own single parent (the coarse nodes must be a prefix of the fine nodes)", (long long)v);
            return ERR_BAD_ARG;
        }
        if (fine_prescribed)
            for (int k = 0; k < nc; ++k) out.coarse_prescribed[cd[(size_t)v * nc + k]] = fine_prescribed[fd[(size_t)v * nc + k]] ? 1 : 0;
    }
    // rows of P, by fine dof
    std::vector<int32_t> dof_node((size_t)fine.ndofs, -1), dof_comp((size_t)fine.ndofs, 0);
    for (int64_t v = 0; v < fine.n_nodes; ++v)
        for (int k = 0; k < nc; ++k) { dof_node[fd[(size_t)v * nc + k]] = (int32_t)v; dof_comp[fd[(size_t)v * nc + k]] = k; }
    out.p_ptr.assign((size_t)fine.ndofs + 1, 0);
    for (int64_t d = 0; d < fine.ndofs; ++d) {
        const int32_t v = dof_node[d];
        if (v < 0) { set_error("multigrid plan: fine dof %lld belongs to no node", (long long)d); return ERR_BAD_ARG; }
        const int64_t np = parent_ptr[v + 1] - parent_ptr[v];
        if (exponent_of(np) < 0) { set_error("multigrid plan: fine node %d has %lld parents (1, 2, 4 or 8 expected)", v, (long long)np); return ERR_BAD_ARG; }
        int64_t kept = 0;
        if (!(fine_prescribed && fine_prescribed[d]))
            for (int64_t q = parent_ptr[v]; q < parent_ptr[v + 1]; ++q) {
                const int32_t pv = parent_idx[q];
                if (pv < 0 || pv >= coarse.n_nodes) { set_error("multigrid plan: parent node %d of fine node %d is not a coarse node", pv, v); return ERR_BAD_ARG; }
                if (!out.coarse_prescribed[cd[(size_t)pv * nc + dof_comp[d]]]) ++kept;
            }
        out.p_ptr[d + 1] = out.p_ptr[d] + kept;
    }
    out.p_col.resize((size_t)out.p_ptr.back());
    out.p_exp.resize((size_t)out.p_ptr.back());
    const int nt = plan_threads();
    (void)nt;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (int64_t d = 0; d < fine.ndofs; ++d) {
        if (out.p_ptr[d + 1] == out.p_ptr[d]) continue;
        const int32_t v = dof_node[d];
        const int e = exponent_of(parent_ptr[v + 1] - parent_ptr[v]);
        int64_t w = out.p_ptr[d];
        for (int64_t q = parent_ptr[v]; q < parent_ptr[v + 1]; ++q) {
            const int32_t cdof = cd[(size_t)parent_idx[q] * nc + dof_comp[d]];
            if (out.coarse_prescribed[cdof]) continue;
            out.p_col[w] = cdof;
            out.p_exp[w] = (uint8_t)e;
            ++w;
        }
        // ascending columns inside a row: the order of the sums does not depend on how the parents were listed
        for (int64_t a = out.p_ptr[d] + 1; a < w; ++a)
            for (int64_t b = a; b > out.p_ptr[d] && out.p_col[b - 1] > out.p_col[b]; --b) std::swap(out.p_col[b - 1], out.p_col[b]);
    }
    transpose(out);
    return 0;
}

// the 27 nodes of the second-order hexahedron as tensor indices (vertices, edges, faces, volume: the order include/tbhip.h documents) and the
// signs of the 8 vertices
static const int8_t HEX27_TIX[27][3] = {{0, 0, 0}, {2, 0, 0}, {2, 2, 0}, {0, 2, 0}, {0, 0, 2}, {2, 0, 2}, {2, 2, 2}, {0, 2, 2}, {1, 0, 0},
                                        {2, 1, 0}, {1, 2, 0}, {0, 1, 0}, {1, 0, 2}, {2, 1, 2}, {1, 2, 2}, {0, 1, 2}, {0, 0, 1}, {2, 0, 1},
                                        {2, 2, 1}, {0, 2, 1}, {1, 1, 0}, {1, 0, 1}, {2, 1, 1}, {1, 2, 1}, {0, 1, 1}, {1, 1, 2}, {1, 1, 1}};
static const int8_t HEX8_SIGNS[8][3] = {{-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, {-1, -1, 1}, {1, -1, 1}, {1, 1, 1}, {-1, 1, 1}};

int build_p_transfer(const LevelView &fine, const LevelView &coarse, const uint8_t *fine_prescribed, Transfer &out)
{
    if (fine.ncomp != coarse.ncomp) { set_error("multigrid p-plan: the levels carry %d and %d components", fine.ncomp, coarse.ncomp); return ERR_BAD_ARG; }
    if (fine.n_cells != coarse.n_cells) { set_error("multigrid p-plan: the levels have %lld and %lld cells (a p-level joins two fields on the same cells)", (long long)fine.n_cells, (long long)coarse.n_cells); return ERR_BAD_ARG; }
    if (fine.basis() != 27 || coarse.basis() != 8) {
        set_error("multigrid p-plan: %d and %d basis functions per cell (27 over 8: a second-order over a first-order hexahedral field)", fine.basis(), coarse.basis());
        return ERR_UNSUPPORTED;
    }
    const int nc = fine.ncomp;
    int nv[27], vl[27][8];
    for (int b = 0; b < 27; ++b) {
        nv[b] = 0;
        for (int a = 0; a < 8; ++a) {
            bool in = true;
            for (int d = 0; d < 3; ++d) in = in && (HEX27_TIX[b][d] == 1 || (HEX27_TIX[b][d] == 0) == (HEX8_SIGNS[a][d] < 0));
            if (in) vl[b][nv[b]++] = a;
        }
    }
    out = Transfer();
    out.n_fine = fine.ndofs;
    out.n_coarse = coarse.ndofs;
    // the parents of every fine dof, ascending, from the first cell that holds it; every later cell must list the same
    std::vector<int32_t> par((size_t)fine.ndofs * 8, -1), twin((size_t)coarse.ndofs, -1); // twin: the fine vertex dof a coarse dof coincides with
    std::vector<uint8_t> npar((size_t)fine.ndofs, 0);
    for (int64_t c = 0; c < fine.n_cells; ++c)
        for (int b = 0; b < 27; ++b)
            for (int k = 0; k < nc; ++k) {
                const int32_t d = fine.cell_dofs[(c * 27 + b) * nc + k];
                if (d < 0 || d >= fine.ndofs) { set_error("multigrid p-plan: fine dof id %d out of range in cell %lld", d, (long long)c); return ERR_BAD_ARG; }
                int32_t loc[8];
                const int n = nv[b];
                for (int q = 0; q < n; ++q) {
                    loc[q] = coarse.cell_dofs[(c * 8 + vl[b][q]) * nc + k];
                    if (loc[q] < 0 || loc[q] >= coarse.ndofs) { set_error("multigrid p-plan: coarse dof id %d out of range in cell %lld", loc[q], (long long)c); return ERR_BAD_ARG; }
                    for (int s = q; s > 0 && loc[s - 1] > loc[s]; --s) std::swap(loc[s - 1], loc[s]);
                }
                for (int q = 1; q < n; ++q)
                    if (loc[q] == loc[q - 1]) { set_error("multigrid p-plan: cell %lld lists coarse dof %d twice", (long long)c, loc[q]); return ERR_PATTERN; }
                int32_t *p = &par[(size_t)d * 8];
                if (npar[d] == 0) { std::copy(loc, loc + n, p); npar[d] = (uint8_t)n; }
                else if (npar[d] != n || !std::equal(loc, loc + n, p)) {
                    set_error("multigrid p-plan: the cells of fine dof %d disagree on its parents (cell %lld): the two fields do not live on the same grid", d, (long long)c);
                    return ERR_PATTERN;
                }
                if (b < 8) {
                    if (twin[loc[0]] >= 0 && twin[loc[0]] != d) { set_error("multigrid p-plan: coarse dof %d coincides with the fine dofs %d and %d", loc[0], twin[loc[0]], d); return ERR_PATTERN; }
                    twin[loc[0]] = d;
                }
            }
    for (int64_t d = 0; d < fine.ndofs; ++d)
        if (!npar[d]) { set_error("multigrid p-plan: fine dof %lld belongs to no cell", (long long)d); return ERR_BAD_ARG; }
    out.coarse_prescribed.assign((size_t)coarse.ndofs, 0);
    for (int64_t I = 0; I < coarse.ndofs; ++I) {
        if (twin[I] < 0) { set_error("multigrid p-plan: coarse dof %lld belongs to no cell", (long long)I); return ERR_BAD_ARG; }
        if (fine_prescribed) out.coarse_prescribed[I] = fine_prescribed[twin[I]] ? 1 : 0;
    }
    out.p_ptr.assign((size_t)fine.ndofs + 1, 0);
    for (int64_t d = 0; d < fine.ndofs; ++d) {
        int64_t kept = 0;
        if (!(fine_prescribed && fine_prescribed[d]))
            for (int q = 0; q < npar[d]; ++q) kept += !out.coarse_prescribed[par[(size_t)d * 8 + q]];
        out.p_ptr[d + 1] = out.p_ptr[d] + kept;
    }
    out.p_col.resize((size_t)out.p_ptr.back());
    out.p_exp.resize((size_t)out.p_ptr.back());
    const int nt = plan_threads();
    (void)nt;
#pragma omp parallel for schedule(static) num_threads(nt)
    for (int64_t d = 0; d < fine.ndofs; ++d) {
        if (out.p_ptr[d + 1] == out.p_ptr[d]) continue;
        int64_t w = out.p_ptr[d];
        for (int q = 0; q < npar[d]; ++q) {
            const int32_t cdof = par[(size_t)d * 8 + q];
            if (out.coarse_prescribed[cdof]) continue;
            out.p_col[w] = cdof;
            out.p_exp[w] = (uint8_t)exponent_of(npar[d]);
            ++w;
        }
    }
    transpose(out);
    return 0;
}

// position of column c in the sorted row [lo, hi) of a CSR pattern, −1 when absent
static inline int64_t find_col(const int32_t *colidx, int64_t lo, int64_t hi, int32_t c)
{
    const int32_t *p = std::lower_bound(colidx + lo, colidx + hi, c);
    return (p != colidx + hi && *p == c) ? (int64_t)(p - colidx) : -1;
}

// The terms of PᵀAP on the coarse pattern (c_rowptr, c_colidx) from the fine pattern (f_rowptr, f_colidx) and P: of dofs for the per-dof plan, of
// nodes and blocks for the blocked one.
struct Csr { int64_t ndofs; const int64_t *rowptr; const int32_t *colidx; };

static int plan_terms(const Csr &fine, const Csr &coarse, const Transfer &t, const uint8_t *fine_prescribed, Galerkin &out)
{
    const int64_t cnnz = coarse.rowptr[coarse.ndofs];
    out.ptr.assign((size_t)cnnz + 1, 0);
    const int nt = plan_threads();
    (void)nt;
    int64_t missing = 0, expected = 0;
    // Every coarse row is planned by one thread: first the term counts of its non-zeros, then — behind a prefix sum — the terms themselves, in
    // the same traversal.  Nothing depends on the team size.
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int64_t> cursor;
        if (pass == 1) {
            for (int64_t k = 0; k < cnnz; ++k) out.ptr[k + 1] += out.ptr[k];
            out.terms.resize((size_t)out.ptr[cnnz]);
            cursor.assign(out.ptr.begin(), out.ptr.end() - 1);
        }
#pragma omp parallel for schedule(dynamic, 64) num_threads(nt) reduction(+ : missing, expected)
        for (int64_t I = 0; I < coarse.ndofs; ++I) {
            const int64_t clo = coarse.rowptr[I], chi = coarse.rowptr[I + 1];
            for (int64_t q = t.r_ptr[I]; q < t.r_ptr[I + 1]; ++q) {
                const int32_t i = t.r_col[q];
                const int ei = t.r_exp[q];
                for (int64_t k = fine.rowptr[i]; k < fine.rowptr[i + 1]; ++k) {
                    const int32_t j = fine.colidx[k];
                    if (fine_prescribed && fine_prescribed[j]) continue; // (a prescribed row i has no entry in Pᵀ at all)
                    for (int64_t s = t.p_ptr[j]; s < t.p_ptr[j + 1]; ++s) {
                        const int64_t pos = find_col(coarse.colidx, clo, chi, t.p_col[s]);
                        if (pos < 0) { ++missing; continue; }
                        if (pass == 0) { ++out.ptr[pos + 1]; ++expected; }
                        else out.terms[cursor[pos]++] = (uint32_t)k | ((uint32_t)(ei + t.p_exp[s]) << TERM_BITS);
                    }
                }
            }
        }
        if (missing) {
            set_error("multigrid plan: %lld couplings of PᵀAP are missing from the coarse pattern (the levels are not nested grids of one field)", (long long)missing);
            return ERR_PATTERN;
        }
    }
    out.expected_terms = expected;
    return 0;
}

static int diagonal_positions(const LevelView &coarse, Galerkin &out)
{
    out.diag_pos.resize((size_t)coarse.ndofs);
    for (int64_t I = 0; I < coarse.ndofs; ++I) {
        const int64_t pos = find_col(coarse.colidx, coarse.rowptr[I], coarse.rowptr[I + 1], (int32_t)I);
        if (pos < 0) { set_error("multigrid plan: coarse row %lld stores no diagonal", (long long)I); return ERR_PATTERN; }
        out.diag_pos[I] = pos;
    }
    return 0;
}

int build_galerkin(const LevelView &fine, const LevelView &coarse, const Transfer &t, const uint8_t *fine_prescribed, Galerkin &out)
{
    const int64_t fnnz = fine.rowptr[fine.ndofs];
    if (fnnz >= MAX_FINE_NNZ) {
        set_error("multigrid plan: the fine level has %lld non-zeros; a Galerkin term holds the fine index in %d bits (fewer than %lld non-zeros per level); "
                  "a node-blocked numbering of a 3-component field on both levels lifts the limit (one term per 3 x 3 block)",
                  (long long)fnnz, TERM_BITS, (long long)MAX_FINE_NNZ);
        return ERR_UNSUPPORTED;
    }
    out = Galerkin();
    if (int rc = plan_terms(Csr{fine.ndofs, fine.rowptr, fine.colidx}, Csr{coarse.ndofs, coarse.rowptr, coarse.colidx}, t, fine_prescribed, out)) return rc;
    return diagonal_positions(coarse, out);
}

// the diagonal of a prescribed coarse dof: the mean |diagonal| of the free ones
static void fill_prescribed_diagonal(const Galerkin &g, const Transfer &t, double *Ac)
{
    double sum = 0.0;
    int64_t nfree = 0;
    for (int64_t I = 0; I < t.n_coarse; ++I)
        if (!t.coarse_prescribed[I]) { sum += std::fabs(Ac[g.diag_pos[I]]); ++nfree; }
    const double fill = nfree ? sum / (double)nfree : 1.0;
    for (int64_t I = 0; I < t.n_coarse; ++I)
        if (t.coarse_prescribed[I]) Ac[g.diag_pos[I]] = fill;
}

bool block_csr(const LevelView &lv)
{
    const int64_t nnz = lv.rowptr[lv.ndofs];
    if (lv.ncomp != 3 || lv.ndofs % 3 != 0 || nnz % 9 != 0 || nnz == 0) return false;
    for (int64_t R = 0; R < lv.ndofs / 3; ++R) {
        const int64_t k0 = lv.rowptr[3 * R], k1 = lv.rowptr[3 * R + 1], k2 = lv.rowptr[3 * R + 2], k3 = lv.rowptr[3 * R + 3];
        const int64_t L = k1 - k0;
        if (L % 3 != 0 || k2 - k1 != L || k3 - k2 != L || k0 % 9 != 0) return false;
        for (int64_t j = 0; j < L; ++j) {
            const int32_t c = lv.colidx[k0 + j];
            if (c != lv.colidx[k0 + j - j % 3] + (int32_t)(j % 3) || (j % 3 == 0 && c % 3 != 0) || lv.colidx[k1 + j] != c || lv.colidx[k2 + j] != c) return false;
        }
    }
    return true;
}

// P of nodes from P of dofs: row i is the union of the rows 3i, 3i + 1, 3i + 2 (a node pair is missing only where every entry of it was dropped);
// false when P is not node-blocked
static bool node_transfer(const Transfer &t, Transfer &nt)
{
    if (t.n_fine % 3 != 0 || t.n_coarse % 3 != 0) return false;
    nt = Transfer();
    nt.n_fine = t.n_fine / 3;
    nt.n_coarse = t.n_coarse / 3;
    nt.p_ptr.assign((size_t)nt.n_fine + 1, 0);
    for (int64_t i = 0; i < nt.n_fine; ++i) {
        int32_t col[24];
        uint8_t ex[24];
        int n = 0;
        for (int k = 0; k < 3; ++k)
            for (int64_t q = t.p_ptr[3 * i + k]; q < t.p_ptr[3 * i + k + 1]; ++q) {
                if (t.p_col[q] % 3 != k || n == 24) return false;
                col[n] = t.p_col[q] / 3;
                ex[n++] = t.p_exp[q];
            }
        for (int a = 1; a < n; ++a)
            for (int b = a; b > 0 && col[b - 1] > col[b]; --b) { std::swap(col[b - 1], col[b]); std::swap(ex[b - 1], ex[b]); }
        for (int a = 0; a < n; ++a) {
            if (a > 0 && col[a] == col[a - 1]) { if (ex[a] != ex[a - 1]) return false; continue; }
            nt.p_col.push_back(col[a]);
            nt.p_exp.push_back(ex[a]);
        }
        nt.p_ptr[i + 1] = (int64_t)nt.p_col.size();
    }
    transpose(nt);
    return true;
}

bool node_blocked(const Transfer &t)
{
    Transfer nt;
    return node_transfer(t, nt);
}

int build_galerkin_blocked(const LevelView &fine, const LevelView &coarse, const Transfer &t, Galerkin &out)
{
    Transfer nt;
    if (!block_csr(fine) || !block_csr(coarse) || !node_transfer(t, nt)) {
        set_error("multigrid plan: the blocked Galerkin plan needs 3-component fields in a node-blocked numbering on both levels");
        return ERR_PATTERN;
    }
    const int64_t fblocks = fine.rowptr[fine.ndofs] / 9;
    if (fblocks >= MAX_FINE_NNZ) {
        set_error("multigrid plan: the fine level has %lld blocks of 3 x 3; a Galerkin term holds the fine block index in %d bits (fewer than %lld blocks per level)",
                  (long long)fblocks, TERM_BITS, (long long)MAX_FINE_NNZ);
        return ERR_UNSUPPORTED;
    }
    // the two patterns as CSRs of blocks
    std::vector<int64_t> bptr[2];
    std::vector<int32_t> bcol[2];
    out = Galerkin();
    out.blocked = true;
    const LevelView *lv[2] = {&fine, &coarse};
    std::vector<int32_t> *brow[2] = {&out.fine_brow, &out.coarse_brow};
    for (int s = 0; s < 2; ++s) {
        const int64_t nbr = lv[s]->ndofs / 3;
        bptr[s].resize((size_t)nbr + 1);
        for (int64_t R = 0; R <= nbr; ++R) bptr[s][R] = lv[s]->rowptr[3 * R] / 9;
        bcol[s].resize((size_t)bptr[s][nbr]);
        brow[s]->resize((size_t)bptr[s][nbr]);
        for (int64_t R = 0; R < nbr; ++R)
            for (int64_t B = bptr[s][R]; B < bptr[s][R + 1]; ++B) {
                bcol[s][B] = lv[s]->colidx[lv[s]->rowptr[3 * R] + 3 * (B - bptr[s][R])] / 3;
                (*brow[s])[B] = (int32_t)R;
            }
    }
    if (int rc = plan_terms(Csr{fine.ndofs / 3, bptr[0].data(), bcol[0].data()}, Csr{coarse.ndofs / 3, bptr[1].data(), bcol[1].data()}, nt, nullptr, out)) return rc;
    return diagonal_positions(coarse, out);
}

void apply_galerkin_blocked_host(const Galerkin &g, const Transfer &t, const LevelView &fine, const LevelView &coarse, const uint8_t *fine_prescribed,
                                 const double *Af, double *Ac)
{
    constexpr uint32_t MASK = ((uint32_t)1 << TERM_BITS) - 1;
    const int64_t cblocks = coarse.rowptr[coarse.ndofs] / 9;
    for (int64_t kb = 0; kb < cblocks; ++kb) {
        const int64_t I = g.coarse_brow[kb], K0 = coarse.rowptr[3 * I], Lc = coarse.rowptr[3 * I + 1] - K0, J = coarse.colidx[K0 + 3 * (kb - K0 / 9)] / 3;
        double s[3][3] = {};
        for (int64_t q = g.ptr[kb]; q < g.ptr[kb + 1]; ++q) {
            const int64_t B = g.terms[q] & MASK, i = g.fine_brow[B], k0 = fine.rowptr[3 * i], L = fine.rowptr[3 * i + 1] - k0;
            const int64_t j = fine.colidx[k0 + 3 * (B - k0 / 9)] / 3;
            const int e = (int)(g.terms[q] >> TERM_BITS);
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    const bool keep = !(fine_prescribed && (fine_prescribed[3 * i + a] || fine_prescribed[3 * j + b])) && !t.coarse_prescribed[3 * I + a] && !t.coarse_prescribed[3 * J + b];
                    if (keep) s[a][b] += std::ldexp(Af[k0 + a * L + 3 * (B - k0 / 9) + b], -e);
                }
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) Ac[K0 + a * Lc + 3 * (kb - K0 / 9) + b] = s[a][b];
    }
    fill_prescribed_diagonal(g, t, Ac);
}

void apply_galerkin_host(const Galerkin &g, const Transfer &t, const double *Af, int64_t coarse_nnz, double *Ac)
{
    constexpr uint32_t MASK = ((uint32_t)1 << TERM_BITS) - 1;
    for (int64_t k = 0; k < coarse_nnz; ++k) {
        double s = 0.0;
        for (int64_t q = g.ptr[k]; q < g.ptr[k + 1]; ++q) s += std::ldexp(Af[g.terms[q] & MASK], -(int)(g.terms[q] >> TERM_BITS));
        Ac[k] = s;
    }
    fill_prescribed_diagonal(g, t, Ac);
}

} // namespace mgplan
} // namespace tb

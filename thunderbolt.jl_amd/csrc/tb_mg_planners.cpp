// tb_mg_planners.cpp — prolongation, restriction and Galerkin plans of the geometric multigrid on nested first-order hexahedral grids
// (src/solver/linear/multigrid.jl, ext/ThunderboltFerriteMultigridExt.jl: the reference forms PᵀAP with sparse products for every new Jacobian;
// here the product is planned once per hierarchy and evaluated by a gather kernel).  Pure host code, standard library only.
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
    // Pᵀ row-wise: a counting transpose visits the fine dofs in ascending order, so every row of Pᵀ is ascending
    out.r_ptr.assign((size_t)coarse.ndofs + 1, 0);
    for (int32_t c : out.p_col) ++out.r_ptr[(size_t)c + 1];
    for (int64_t I = 0; I < coarse.ndofs; ++I) out.r_ptr[I + 1] += out.r_ptr[I];
    out.r_col.resize(out.p_col.size());
    out.r_exp.resize(out.p_col.size());
    std::vector<int64_t> cur(out.r_ptr.begin(), out.r_ptr.end() - 1);
    for (int64_t d = 0; d < fine.ndofs; ++d)
        for (int64_t q = out.p_ptr[d]; q < out.p_ptr[d + 1]; ++q) {
            const int64_t w = cur[out.p_col[q]]++;
            out.r_col[w] = (int32_t)d;
            out.r_exp[w] = out.p_exp[q];
        }
    return 0;
}

// position of column c in the sorted row [lo, hi) of a CSR pattern, −1 when absent
static inline int64_t find_col(const int32_t *colidx, int64_t lo, int64_t hi, int32_t c)
{
    const int32_t *p = std::lower_bound(colidx + lo, colidx + hi, c);
    return (p != colidx + hi && *p == c) ? (int64_t)(p - colidx) : -1;
}

int build_galerkin(const LevelView &fine, const LevelView &coarse, const Transfer &t, const uint8_t *fine_prescribed, Galerkin &out)
{
    const int64_t fnnz = fine.rowptr[fine.ndofs], cnnz = coarse.rowptr[coarse.ndofs];
    if (fnnz >= MAX_FINE_NNZ) {
        set_error("multigrid plan: the fine level has %lld non-zeros; a Galerkin term holds the fine index in %d bits (fewer than %lld non-zeros per level)",
                  (long long)fnnz, TERM_BITS, (long long)MAX_FINE_NNZ);
        return ERR_UNSUPPORTED;
    }
    out = Galerkin();
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
    out.diag_pos.resize((size_t)coarse.ndofs);
    for (int64_t I = 0; I < coarse.ndofs; ++I) {
        const int64_t pos = find_col(coarse.colidx, coarse.rowptr[I], coarse.rowptr[I + 1], (int32_t)I);
        if (pos < 0) { set_error("multigrid plan: coarse row %lld stores no diagonal", (long long)I); return ERR_PATTERN; }
        out.diag_pos[I] = pos;
    }
    return 0;
}

void apply_galerkin_host(const Galerkin &g, const Transfer &t, const double *Af, int64_t coarse_nnz, double *Ac)
{
    constexpr uint32_t MASK = ((uint32_t)1 << TERM_BITS) - 1;
    for (int64_t k = 0; k < coarse_nnz; ++k) {
        double s = 0.0;
        for (int64_t q = g.ptr[k]; q < g.ptr[k + 1]; ++q) s += std::ldexp(Af[g.terms[q] & MASK], -(int)(g.terms[q] >> TERM_BITS));
        Ac[k] = s;
    }
    double sum = 0.0;
    int64_t nfree = 0;
    for (int64_t I = 0; I < t.n_coarse; ++I)
        if (!t.coarse_prescribed[I]) { sum += std::fabs(Ac[g.diag_pos[I]]); ++nfree; }
    const double fill = nfree ? sum / (double)nfree : 1.0;
    for (int64_t I = 0; I < t.n_coarse; ++I)
        if (t.coarse_prescribed[I]) Ac[g.diag_pos[I]] = fill;
}

} // namespace mgplan
} // namespace tb

// tb_amg_planners.cpp — aggregation and pattern planning of the smoothed-aggregation multigrid (see tb_amg_planners.hpp).  Everything runs in index
// order on flags and indices: the same input gives the same plan on every host.
#include "tb_amg_planners.hpp"

#include <algorithm>
#include <cstdio>

namespace tb {
namespace amgplan {

int64_t find_entry(const int64_t *rowptr, const int32_t *colidx, int64_t i, int32_t j)
{
    const int32_t *lo = colidx + rowptr[i], *hi = colidx + rowptr[i + 1];
    const int32_t *p = std::lower_bound(lo, hi, j);
    return p != hi && *p == j ? (int64_t)(p - colidx) : -1;
}

int check_pattern(int64_t n, const int64_t *rowptr, const int32_t *colidx, std::string &err)
{
    char buf[160];
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            if (colidx[k] < 0 || colidx[k] >= n) {
                snprintf(buf, sizeof buf, "row %lld holds column %d outside 0..%lld", (long long)i, colidx[k], (long long)n - 1);
                err = buf;
                return -1;
            }
            if (k > rowptr[i] && colidx[k] <= colidx[k - 1]) {
                snprintf(buf, sizeof buf, "the columns of row %lld are not sorted and distinct", (long long)i);
                err = buf;
                return -1;
            }
        }
    }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
            if (find_entry(rowptr, colidx, colidx[k], (int32_t)i) < 0) {
                snprintf(buf, sizeof buf, "the pattern is not structurally symmetric: row %lld stores column %d, row %d does not store column %lld", (long long)i,
                         colidx[k], colidx[k], (long long)i);
                err = buf;
                return -1;
            }
    return 0;
}

void diagonal_positions(int64_t n, const int64_t *rowptr, const int32_t *colidx, std::vector<int64_t> &diag)
{
    diag.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) diag[(size_t)i] = find_entry(rowptr, colidx, i, (int32_t)i);
}

void aggregate(int64_t n, const int64_t *rowptr, const int32_t *colidx, const uint8_t *strength, std::vector<int32_t> &agg, int64_t &n_agg)
{
    agg.assign((size_t)n, -1);
    n_agg = 0;
    // pass 1: a dof whose strong neighbourhood is entirely free roots an aggregate
    for (int64_t i = 0; i < n; ++i) {
        if (agg[(size_t)i] >= 0) continue;
        bool any = false, all_free = true;
        for (int64_t k = rowptr[i]; k < rowptr[i + 1] && all_free; ++k)
            if (strength[k]) { any = true; all_free = agg[(size_t)colidx[k]] < 0; }
        if (!any || !all_free) continue;
        agg[(size_t)i] = (int32_t)n_agg;
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
            if (strength[k]) agg[(size_t)colidx[k]] = (int32_t)n_agg;
        ++n_agg;
    }
    // pass 2: against the state after pass 1, a free dof joins the aggregate of its lowest-numbered aggregated strong neighbour
    const std::vector<int32_t> snap(agg);
    for (int64_t i = 0; i < n; ++i) {
        if (snap[(size_t)i] >= 0) continue;
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
            if (strength[k] && snap[(size_t)colidx[k]] >= 0) { agg[(size_t)i] = snap[(size_t)colidx[k]]; break; }
    }
    // pass 3: what is still free and has strong neighbours forms aggregates with its still-free strong neighbours
    for (int64_t i = 0; i < n; ++i) {
        if (agg[(size_t)i] >= 0) continue;
        bool any = false;
        for (int64_t k = rowptr[i]; k < rowptr[i + 1] && !any; ++k) any = strength[k] != 0;
        if (!any) continue;
        agg[(size_t)i] = (int32_t)n_agg;
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
            if (strength[k] && agg[(size_t)colidx[k]] < 0) agg[(size_t)colidx[k]] = (int32_t)n_agg;
        ++n_agg;
    }
}

namespace {
// the sorted union of the rows of (bptr, bcol) named by `rows`, appended to col; mark: one slot per column, all −1 between calls
template <class Rows>
void union_rows(const Rows &rows, const std::vector<int64_t> &bptr, const std::vector<int32_t> &bcol, std::vector<int32_t> &mark, int32_t stamp,
                std::vector<int32_t> &col)
{
    const size_t first = col.size();
    for (int32_t k : rows)
        for (int64_t q = bptr[(size_t)k]; q < bptr[(size_t)k + 1]; ++q)
            if (mark[(size_t)bcol[(size_t)q]] != stamp) { mark[(size_t)bcol[(size_t)q]] = stamp; col.push_back(bcol[(size_t)q]); }
    std::sort(col.begin() + (std::ptrdiff_t)first, col.end());
}
void rows_of(const std::vector<int64_t> &ptr, std::vector<int32_t> &row)
{
    row.resize((size_t)ptr.back());
    for (size_t i = 0; i + 1 < ptr.size(); ++i)
        for (int64_t q = ptr[i]; q < ptr[i + 1]; ++q) row[(size_t)q] = (int32_t)i;
}
} // namespace

void plan_level(int64_t n, const int64_t *rowptr, const int32_t *colidx, const int8_t *comp, const uint8_t *strength, LevelPlan &L)
{
    L = LevelPlan();
    L.n = n;
    aggregate(n, rowptr, colidx, strength, L.agg, L.nc);
    const int64_t nc = L.nc;
    L.agg_size.assign((size_t)nc, 0);
    L.ccomp.assign((size_t)nc, 0);
    for (int64_t i = 0; i < n; ++i)
        if (L.agg[(size_t)i] >= 0) {
            ++L.agg_size[(size_t)L.agg[(size_t)i]];
            L.ccomp[(size_t)L.agg[(size_t)i]] = comp ? comp[i] : 0;
        }
    // A·T row by row: the aggregates of the row's columns; P keeps the rows of aggregated dofs
    std::vector<int64_t> at_ptr((size_t)n + 1, 0);
    std::vector<int32_t> at_col, mark((size_t)std::max<int64_t>(nc, 1), -1);
    L.p_ptr.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        const size_t first = at_col.size();
        for (int64_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const int32_t J = L.agg[(size_t)colidx[k]];
            if (J >= 0 && mark[(size_t)J] != (int32_t)i) { mark[(size_t)J] = (int32_t)i; at_col.push_back(J); }
        }
        std::sort(at_col.begin() + (std::ptrdiff_t)first, at_col.end());
        at_ptr[(size_t)i + 1] = (int64_t)at_col.size();
        if (L.agg[(size_t)i] >= 0) L.p_col.insert(L.p_col.end(), at_col.begin() + (std::ptrdiff_t)first, at_col.end());
        L.p_ptr[(size_t)i + 1] = (int64_t)L.p_col.size();
    }
    complete_patterns(n, rowptr, colidx, L);
}

void complete_patterns(int64_t n, const int64_t *rowptr, const int32_t *colidx, LevelPlan &L)
{
    const int64_t nc = L.nc;
    std::vector<int32_t> mark((size_t)std::max<int64_t>(nc, 1), -1);
    rows_of(L.p_ptr, L.p_row);
    // R = Pᵀ: a counting transpose keeps the fine dofs of a row ascending; r_perm remembers where each value sits in P
    L.r_ptr.assign((size_t)nc + 1, 0);
    for (int32_t J : L.p_col) ++L.r_ptr[(size_t)J + 1];
    for (int64_t J = 0; J < nc; ++J) L.r_ptr[(size_t)J + 1] += L.r_ptr[(size_t)J];
    L.r_col.resize(L.p_col.size());
    L.r_perm.resize(L.p_col.size());
    {
        std::vector<int64_t> fill(L.r_ptr.begin(), L.r_ptr.end() - 1);
        for (int64_t q = 0; q < (int64_t)L.p_col.size(); ++q) {
            const int64_t at = fill[(size_t)L.p_col[(size_t)q]]++;
            L.r_col[(size_t)at] = L.p_row[(size_t)q];
            L.r_perm[(size_t)at] = q;
        }
    }
    // A·P: the union of P's rows over the columns of A's row
    L.ap_ptr.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        struct Cols { const int32_t *b, *e; const int32_t *begin() const { return b; } const int32_t *end() const { return e; } };
        union_rows(Cols{colidx + rowptr[i], colidx + rowptr[i + 1]}, L.p_ptr, L.p_col, mark, (int32_t)i, L.ap_col);
        L.ap_ptr[(size_t)i + 1] = (int64_t)L.ap_col.size();
    }
    rows_of(L.ap_ptr, L.ap_row);
    // A_c = R·(A·P)
    L.c_ptr.assign((size_t)nc + 1, 0);
    std::fill(mark.begin(), mark.end(), -1);
    for (int64_t I = 0; I < nc; ++I) {
        struct Cols { const int32_t *b, *e; const int32_t *begin() const { return b; } const int32_t *end() const { return e; } };
        union_rows(Cols{L.r_col.data() + L.r_ptr[(size_t)I], L.r_col.data() + L.r_ptr[(size_t)I + 1]}, L.ap_ptr, L.ap_col, mark, (int32_t)I, L.c_col);
        L.c_ptr[(size_t)I + 1] = (int64_t)L.c_col.size();
    }
    rows_of(L.c_ptr, L.c_row);
    diagonal_positions(nc, L.c_ptr.data(), L.c_col.data(), L.c_diag);
}

} // namespace amgplan
} // namespace tb

// tb_amg_planners.hpp — the symbolic phase of the smoothed-aggregation multigrid (tb_amg.hip), pure host code: no HIP, no device, no matrix values.
// What a level's plan is made from: the CSR pattern of A (sorted columns, structurally symmetric), one component label per dof and the strength
// byte per non-zero the device wrote.  What it holds: the aggregates, the patterns of P (that of A·T, rows of dofs outside every aggregate empty),
// of R = Pᵀ with the permutation that gathers its values from P's, of A·P and of A_c = R·(A·P), and A_c's diagonal positions.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace tb {
namespace amgplan {

struct LevelPlan {
    int64_t n = 0, nc = 0;               // dofs of the level, aggregates (dofs of the level below)
    std::vector<int32_t> agg;            // aggregate of every dof, −1: outside (no strong neighbour)
    std::vector<int32_t> agg_size;       // dofs per aggregate
    std::vector<int8_t> ccomp;           // component label per aggregate (that of its dofs)
    // CSR patterns; *_row names the row of every non-zero (one work item per non-zero on the device)
    std::vector<int64_t> p_ptr, r_ptr, ap_ptr, c_ptr;
    std::vector<int32_t> p_col, p_row, r_col, ap_col, ap_row, c_col, c_row;
    std::vector<int64_t> r_perm;         // R's k-th value is P's r_perm[k]-th
    std::vector<int64_t> c_diag;         // position of the diagonal in every row of A_c (−1: none stored)
};

// sorted columns, structurally symmetric: 0, or −1 with the offending row named in err
int check_pattern(int64_t n, const int64_t *rowptr, const int32_t *colidx, std::string &err);
// position of column j in row i (binary search), −1: not stored
int64_t find_entry(const int64_t *rowptr, const int32_t *colidx, int64_t i, int32_t j);
// position of the diagonal per row (−1: none stored)
void diagonal_positions(int64_t n, const int64_t *rowptr, const int32_t *colidx, std::vector<int64_t> &diag);
// the three passes, in index order, on the strength flags alone
void aggregate(int64_t n, const int64_t *rowptr, const int32_t *colidx, const uint8_t *strength, std::vector<int32_t> &agg, int64_t &n_agg);
// aggregates and every pattern of one level (comp NULL: one component)
void plan_level(int64_t n, const int64_t *rowptr, const int32_t *colidx, const int8_t *comp, const uint8_t *strength, LevelPlan &out);
// from n, nc and P's pattern (p_ptr, p_col): p_row, R with its permutation, A·P, A_c and its diagonal positions
void complete_patterns(int64_t n, const int64_t *rowptr, const int32_t *colidx, LevelPlan &L);

} // namespace amgplan
} // namespace tb

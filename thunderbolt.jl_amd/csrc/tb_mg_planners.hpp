// tb_mg_planners.hpp — the planning half of the geometric multigrid (tb_multigrid.hip): pure host functions from the dof tables of two nested
// first-order hexahedral levels and the parent nodes of the fine nodes to the prolongation P, its transpose and the gather plan of the Galerkin
// product A_c = PᵀA_fP.  Standard library only, no device, no environment: tests/multigrid_planner_driver.cpp calls them without a GPU.
// tb::set_error is the only tie to the rest of the library.
#pragma once
#include <cstdint>
#include <vector>

namespace tb {

void set_error(const char *fmt, ...);

namespace mgplan {

enum { ERR_BAD_ARG = -1, ERR_PATTERN = -4, ERR_UNSUPPORTED = -5 }; // the TB_ERR_* codes of include/tbhip.h

// one level: the dof table of a first-order field on the level's grid and the level's CSR pattern
struct LevelView {
    int64_t n_nodes, n_cells, ndofs;
    int nverts, ncomp;             // vertices per cell (8), components per node (1 or 3); cell_dofs holds nverts·ncomp dofs per cell, node-major
    const int32_t *conn, *cell_dofs;
    const int64_t *rowptr;
    const int32_t *colidx;
};

// A weight is 2^−e: a fine node has 1, 2, 4 or 8 parents, so e ≤ 3 in P and e ≤ 6 in a Galerkin term.
struct Transfer {
    int64_t n_fine = 0, n_coarse = 0;
    std::vector<int64_t> p_ptr, r_ptr;   // P row-wise (fine dof → coarse dofs), Pᵀ row-wise (coarse dof → fine dofs, ascending)
    std::vector<int32_t> p_col, r_col;
    std::vector<uint8_t> p_exp, r_exp;
    std::vector<uint8_t> coarse_prescribed; // a coarse dof is prescribed iff the fine dof it coincides with is
};

constexpr int TERM_BITS = 29;                       // a Galerkin term: fine nz index in the low 29 bits, the exponent e in the high 3
constexpr int64_t MAX_FINE_NNZ = (int64_t)1 << TERM_BITS;

struct Galerkin {
    std::vector<int64_t> ptr;     // coarse nnz + 1: the terms of every coarse non-zero, in the order they are summed
    std::vector<uint32_t> terms;
    std::vector<int64_t> diag_pos; // nz index of every coarse row's diagonal: a prescribed coarse dof (row and column otherwise empty) gets the mean |diagonal| of the free ones there
    int64_t expected_terms = 0;   // Σ |parents(i)|·|parents(j)| over the kept fine non-zeros (free parents only): what terms.size() must equal
};

// node → first dof of the node (the components of a node are consecutive entries of cell_dofs, not necessarily consecutive dofs): dof of
// (node v, component c) = node_dofs[v·ncomp + c].  Fails when a node has no cell.
int node_dof_table(const LevelView &lv, std::vector<int32_t> &node_dofs);

// P between two levels.  parent_ptr / parent_idx: the parents (coarse nodes) of every fine node; fine_prescribed: one flag per fine dof or NULL.
// Rows of prescribed fine dofs and columns of prescribed coarse dofs are dropped.
int build_transfer(const LevelView &fine, const LevelView &coarse, const int64_t *parent_ptr, const int32_t *parent_idx, const uint8_t *fine_prescribed,
                   Transfer &out);

// The gather plan of A_c = PᵀA_fP on the coarse level's own pattern.  Every coarse non-zero (I, J) sums w_iI·a_ij·w_jJ over the fine rows i of
// column I of P in ascending order, inside a row over its non-zeros in storage order: one recorded order, whatever the number of host threads.
int build_galerkin(const LevelView &fine, const LevelView &coarse, const Transfer &t, const uint8_t *fine_prescribed, Galerkin &out);

// host evaluation of the plan (tests; the device kernel is k_mg_galerkin): Ac[k] = Σ terms, diagonal of the prescribed coarse dofs = mean |diagonal|
// of the free ones
void apply_galerkin_host(const Galerkin &g, const Transfer &t, const double *Af, int64_t coarse_nnz, double *Ac);

} // namespace mgplan
} // namespace tb

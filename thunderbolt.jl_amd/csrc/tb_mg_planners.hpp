// tb_mg_planners.hpp — the planning half of the multigrid (tb_multigrid.hip): pure host functions from the dof tables of two levels to the
// prolongation P, its transpose and the gather plan of the Galerkin product A_c = PᵀA_fP.  An h-level joins two nested first-order hexahedral grids
// through the parent nodes of the fine nodes (build_transfer); the p-level joins a second-order and a first-order field on the same cells through
// the two cell-dof tables (build_p_transfer).  Standard library only, no device, no environment: tests/multigrid_planner_driver.cpp and
// tests/pmultigrid_planner_driver.cpp call them without a GPU.
// tb::set_error is the only tie to the rest of the library.
#pragma once
#include <cstdint>
#include <vector>

namespace tb {

void set_error(const char *fmt, ...);

namespace mgplan {

enum { ERR_BAD_ARG = -1, ERR_PATTERN = -4, ERR_UNSUPPORTED = -5 }; // the TB_ERR_* codes of include/tbhip.h

// one level: the dof table of a field on the level's grid and the level's CSR pattern
struct LevelView {
    int64_t n_nodes, n_cells, ndofs;
    int nverts, ncomp;             // vertices per cell (8), components per node (1 or 3); cell_dofs holds nbasis·ncomp dofs per cell, node-major
    const int32_t *conn, *cell_dofs;
    const int64_t *rowptr;
    const int32_t *colidx;
    int nbasis = 0;                // basis functions per cell and component: 27 for a second-order field; 0 = nverts (a first-order field)
    int basis() const { return nbasis ? nbasis : nverts; }
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

// Per-dof plan: one term per (coarse non-zero, fine non-zero) pair.  Blocked plan (both patterns CSRs of 3 × 3 blocks): one term per (coarse block,
// fine block) pair, the term holds the fine block index: a ninth of the terms, and the 29 bits reach nine times as many fine non-zeros.
struct Galerkin {
    std::vector<int64_t> ptr;     // coarse nnz (blocked: coarse blocks) + 1: the terms of every coarse non-zero (block), in the order they are summed
    std::vector<uint32_t> terms;
    bool blocked = false;
    std::vector<int32_t> fine_brow, coarse_brow; // blocked: the block row of every block of the two patterns (a term names a block, its rows follow from this)
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

// P of the p-level: `fine` a second-order (27 basis functions per cell) and `coarse` a first-order field on the same cells, same ncomp.  A Q1 function at
// the Q2 node of tensor index (t_x, t_y, t_z) ∈ {0, 1, 2}³ is the mean of the 1, 2, 4 or 8 vertices the index selects (0: the low side, 2: the high
// side, 1: both), on any trilinear geometry.  Fine dof cell_dofs_f[c][b·ncomp + k] has the parents cell_dofs_c[c][a·ncomp + k]; cells that share a dof must
// agree on them (ERR_PATTERN).  Any numbering on either level.  A coarse dof is prescribed iff the fine vertex dof it coincides with is.
int build_p_transfer(const LevelView &fine, const LevelView &coarse, const uint8_t *fine_prescribed, Transfer &out);

// The gather plan of A_c = PᵀA_fP on the coarse level's own pattern.  Every coarse non-zero (I, J) sums w_iI·a_ij·w_jJ over the fine rows i of
// column I of P in ascending order, inside a row over its non-zeros in storage order: one recorded order, whatever the number of host threads.
int build_galerkin(const LevelView &fine, const LevelView &coarse, const Transfer &t, const uint8_t *fine_prescribed, Galerkin &out);

// is the pattern a CSR of 3 × 3 blocks (rows 3R, 3R+1, 3R+2 of equal length over the same columns, the columns in triples 3C, 3C+1, 3C+2)?
bool block_csr(const LevelView &lv);
// does P move node triples: every entry of row 3i + k sits in a column 3J + k, with one weight per node pair (i, J)?
bool node_blocked(const Transfer &t);

// The blocked plan: both patterns block CSRs, P node-blocked (ERR_PATTERN otherwise).  One term per (coarse block, fine block) pair in the order of
// the per-dof plan: fine block rows of the column ascending, storage order inside a row.  Prescribed dofs may cut through a block: the plan stays per
// node pair (a pair is left out only where every entry of it is dropped) and the evaluation selects per entry from the flags of the four dofs.
int build_galerkin_blocked(const LevelView &fine, const LevelView &coarse, const Transfer &t, Galerkin &out);

// host evaluation of the blocked plan (tests; the device kernel is k_mg_galerkin_b3)
void apply_galerkin_blocked_host(const Galerkin &g, const Transfer &t, const LevelView &fine, const LevelView &coarse, const uint8_t *fine_prescribed,
                                 const double *Af, double *Ac);

// host evaluation of the plan (tests; the device kernel is k_mg_galerkin): Ac[k] = Σ terms, diagonal of the prescribed coarse dofs = mean |diagonal|
// of the free ones
void apply_galerkin_host(const Galerkin &g, const Transfer &t, const double *Af, int64_t coarse_nnz, double *Ac);

} // namespace mgplan
} // namespace tb

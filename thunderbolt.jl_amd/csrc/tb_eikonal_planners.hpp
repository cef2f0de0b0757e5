// tb_eikonal_planners.hpp — the planning half of the eikonal unit (tb_eikonal.hip): a pure host function from a connectivity to the
// node → (tetrahedron, corner) incidence the sweep kernel reads and the node adjacency its activation test reads.  Standard library only, no
// device, no environment, no global state; tests/eikonal_planner_driver.cpp calls it without a GPU.
#pragma once
#include <cstdint>
#include <vector>

#include "tb_planners.hpp"

namespace tb {
namespace eikplan {

// The six Kuhn tetrahedra of a hexahedron by its LOCAL vertex order (include/tbhip.h, tb_host_generate_grid_tet): no tetrahedral mesh is
// materialised, tetrahedron k of cell c is (conn[8c + KUHN[k][0 … 3]]).
constexpr int KUHN[6][4] = {{0, 1, 2, 6}, {0, 5, 1, 6}, {0, 2, 3, 6}, {0, 3, 7, 6}, {0, 4, 5, 6}, {0, 7, 4, 6}};

// A corner record is code = (cell · ntet + k) · 4 + corner (ntet = 1 for tetrahedra, 6 for hexahedra) with the three OTHER vertices of that
// tetrahedron in ascending corner order.  The records of a node stand in ascending (cell, k) order — the order of the traversal that builds
// them — so the operands of the sweep's minimum come in a fixed order.  adj: the distinct nodes that share a tetrahedron with the node, ascending
// (symmetric by construction: it is the union of `others`).
struct IncidenceHost {
    int ntet = 0;
    std::vector<int64_t> ptr;    // n_nodes + 1 → code / others
    std::vector<int32_t> code;   // one per record
    std::vector<int32_t> others; // three per record
    std::vector<int64_t> adj_ptr; // n_nodes + 1 → adj
    std::vector<int32_t> adj;
};

// conn: n_cells × nverts node ids, 0-based; nverts 4 (tetrahedra) or 8 (hexahedra, cut implicitly).  0, or plan::ERR_BAD_ARG with the message
// set: a node id outside [0, n_nodes), more cells than the 31-bit codes hold.
int incidence(int64_t n_nodes, int64_t n_cells, int nverts, const int32_t *conn, IncidenceHost &out);

} // namespace eikplan
} // namespace tb

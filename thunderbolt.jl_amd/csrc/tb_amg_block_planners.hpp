// tb_amg_block_planners.hpp — the symbolic phase of the node-wise smoothed aggregation with a near-null-space (tb_amg_block.hip), pure host code: no
// HIP, no device, no matrix values.  A level has `k` candidate vectors; its dofs belong to nodes through a dof → node map (level 0: 3 dofs per node in
// any numbering; below: node = aggregate of the level above, dofs k·a … k·a + k − 1).  What the plan is made from: the CSR pattern of A (sorted
// columns, structurally symmetric), the node map and one strength byte per non-zero of the node graph (written by the device).  What it holds: the
// node graph with, per non-zero, the non-zeros of A in it (stored row-major order); the aggregates of the nodes and of the dofs; the dofs of every
// aggregate (CSR, ascending) — the block pattern of the dense tentative prolongator T (row i lies in the column block of agg[i]); and the patterns of P,
// R with its permutation, A·P and A_c with its diagonal positions, as amgplan::plan_level records them (LevelPlan; nc = k · aggregates).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "tb_amg_planners.hpp"

namespace tb {
namespace amgplan {

struct NodeGraph {
    int64_t n_nodes = 0;
    std::vector<int64_t> ptr;            // CSR of the node graph (sorted columns, the diagonal included where A couples a node with itself)
    std::vector<int32_t> col;
    std::vector<int64_t> entry_ptr;      // per node-graph non-zero: its non-zeros of A …
    std::vector<int64_t> entries;        // … ascending, which is stored row-major order when the node's dofs are taken in ascending order
    std::vector<int64_t> nz_of_entry;    // per non-zero of A: its node-graph non-zero
};

struct BlockPlan {
    int k = 0;
    int64_t n_agg = 0;
    std::vector<int32_t> node_agg;       // aggregate of every node, −1: outside
    std::vector<int64_t> adof_ptr;       // dofs of every aggregate, ascending
    std::vector<int32_t> adof;
    LevelPlan L;                         // agg: per dof; agg_size: dofs per aggregate; ccomp empty; nc = k · n_agg
};

// 0, or −1 with a message: node ids outside 0..n_nodes − 1, or (dofs_per_node > 0) a node with another number of dofs
int check_nodes(int64_t n, const int32_t *node_of_dof, int64_t n_nodes, int dofs_per_node, std::string &err);
void node_graph(int64_t n, const int64_t *rowptr, const int32_t *colidx, const int32_t *node_of_dof, int64_t n_nodes, NodeGraph &g);
// aggregates of the node graph (amgplan::aggregate, unchanged) and every pattern of one level
void plan_block_level(int64_t n, const int64_t *rowptr, const int32_t *colidx, const int32_t *node_of_dof, const NodeGraph &g, const uint8_t *node_strength,
                      int k, BlockPlan &out);

} // namespace amgplan
} // namespace tb

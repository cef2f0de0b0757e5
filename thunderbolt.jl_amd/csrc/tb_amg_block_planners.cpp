// tb_amg_block_planners.cpp — node graph, node aggregation and pattern planning of the smoothed aggregation with a near-null-space (see
// tb_amg_block_planners.hpp).  Everything runs in index order on flags and indices: the same input gives the same plan on every host.
#include "tb_amg_block_planners.hpp"

#include <algorithm>
#include <cstdio>

namespace tb {
namespace amgplan {

int check_nodes(int64_t n, const int32_t *node_of_dof, int64_t n_nodes, int dofs_per_node, std::string &err)
{
    char buf[160];
    std::vector<int32_t> count((size_t)std::max<int64_t>(n_nodes, 0), 0);
    for (int64_t i = 0; i < n; ++i) {
        if (node_of_dof[i] < 0 || node_of_dof[i] >= n_nodes) {
            snprintf(buf, sizeof buf, "dof %lld names node %d outside 0..%lld", (long long)i, node_of_dof[i], (long long)n_nodes - 1);
            err = buf;
            return -1;
        }
        ++count[(size_t)node_of_dof[i]];
    }
    if (dofs_per_node > 0)
        for (int64_t v = 0; v < n_nodes; ++v)
            if (count[(size_t)v] != dofs_per_node) {
                snprintf(buf, sizeof buf, "node %lld has %d dofs, not %d", (long long)v, count[(size_t)v], dofs_per_node);
                err = buf;
                return -1;
            }
    return 0;
}

void node_graph(int64_t n, const int64_t *rowptr, const int32_t *colidx, const int32_t *node_of_dof, int64_t n_nodes, NodeGraph &g)
{
    g = NodeGraph();
    g.n_nodes = n_nodes;
    // the dofs of every node, ascending (counting sort)
    std::vector<int64_t> nd_ptr((size_t)n_nodes + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++nd_ptr[(size_t)node_of_dof[i] + 1];
    for (int64_t v = 0; v < n_nodes; ++v) nd_ptr[(size_t)v + 1] += nd_ptr[(size_t)v];
    std::vector<int32_t> nd((size_t)n);
    {
        std::vector<int64_t> fill(nd_ptr.begin(), nd_ptr.end() - 1);
        for (int64_t i = 0; i < n; ++i) nd[(size_t)fill[(size_t)node_of_dof[i]]++] = (int32_t)i;
    }
    // the columns of every node row: the sorted nodes of its dofs' columns
    g.ptr.assign((size_t)n_nodes + 1, 0);
    std::vector<int32_t> mark((size_t)std::max<int64_t>(n_nodes, 1), -1);
    for (int64_t I = 0; I < n_nodes; ++I) {
        const size_t first = g.col.size();
        for (int64_t p = nd_ptr[(size_t)I]; p < nd_ptr[(size_t)I + 1]; ++p) {
            const int64_t i = nd[(size_t)p];
            for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
                const int32_t J = node_of_dof[colidx[e]];
                if (mark[(size_t)J] != (int32_t)I) { mark[(size_t)J] = (int32_t)I; g.col.push_back(J); }
            }
        }
        std::sort(g.col.begin() + (std::ptrdiff_t)first, g.col.end());
        g.ptr[(size_t)I + 1] = (int64_t)g.col.size();
    }
    // the non-zeros of A in every node-graph non-zero: count, then fill in ascending order of the non-zero (the rows of a node are visited ascending,
    // and a row's non-zeros lie behind those of every lower row)
    const int64_t gnnz = (int64_t)g.col.size(), nnz = rowptr[n];
    g.nz_of_entry.resize((size_t)nnz);
    g.entry_ptr.assign((size_t)gnnz + 1, 0);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            const int64_t q = find_entry(g.ptr.data(), g.col.data(), node_of_dof[i], node_of_dof[colidx[e]]);
            g.nz_of_entry[(size_t)e] = q;
            ++g.entry_ptr[(size_t)q + 1];
        }
    for (int64_t q = 0; q < gnnz; ++q) g.entry_ptr[(size_t)q + 1] += g.entry_ptr[(size_t)q];
    g.entries.resize((size_t)nnz);
    std::vector<int64_t> fill(g.entry_ptr.begin(), g.entry_ptr.end() - 1);
    for (int64_t e = 0; e < nnz; ++e) g.entries[(size_t)fill[(size_t)g.nz_of_entry[(size_t)e]]++] = e;
}

void plan_block_level(int64_t n, const int64_t *rowptr, const int32_t *colidx, const int32_t *node_of_dof, const NodeGraph &g, const uint8_t *node_strength,
                      int k, BlockPlan &B)
{
    B = BlockPlan();
    B.k = k;
    aggregate(g.n_nodes, g.ptr.data(), g.col.data(), node_strength, B.node_agg, B.n_agg);
    LevelPlan &L = B.L;
    L.n = n;
    L.nc = (int64_t)k * B.n_agg;
    L.agg.resize((size_t)n);
    L.agg_size.assign((size_t)B.n_agg, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t a = B.node_agg[(size_t)node_of_dof[i]];
        L.agg[(size_t)i] = a;
        if (a >= 0) ++L.agg_size[(size_t)a];
    }
    B.adof_ptr.assign((size_t)B.n_agg + 1, 0);
    for (int64_t a = 0; a < B.n_agg; ++a) B.adof_ptr[(size_t)a + 1] = B.adof_ptr[(size_t)a] + L.agg_size[(size_t)a];
    B.adof.resize((size_t)B.adof_ptr[(size_t)B.n_agg]);
    {
        std::vector<int64_t> fill(B.adof_ptr.begin(), B.adof_ptr.end() - 1);
        for (int64_t i = 0; i < n; ++i)
            if (L.agg[(size_t)i] >= 0) B.adof[(size_t)fill[(size_t)L.agg[(size_t)i]]++] = (int32_t)i;
    }
    // P on the pattern of A·T, rows of aggregated dofs only: the k columns of every aggregate met in the row
    std::vector<int32_t> mark((size_t)std::max<int64_t>(B.n_agg, 1), -1), aggs;
    L.p_ptr.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (L.agg[(size_t)i] >= 0) {
            aggs.clear();
            for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
                const int32_t J = L.agg[(size_t)colidx[e]];
                if (J >= 0 && mark[(size_t)J] != (int32_t)i) { mark[(size_t)J] = (int32_t)i; aggs.push_back(J); }
            }
            std::sort(aggs.begin(), aggs.end());
            for (int32_t J : aggs)
                for (int c = 0; c < k; ++c) L.p_col.push_back(J * k + c);
        }
        L.p_ptr[(size_t)i + 1] = (int64_t)L.p_col.size();
    }
    complete_patterns(n, rowptr, colidx, L);
}

} // namespace amgplan
} // namespace tb

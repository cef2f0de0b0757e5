// tb_eikonal_planners.cpp — the host planner of the eikonal unit (tb_eikonal_planners.hpp): corner incidence and node adjacency.
#include "tb_eikonal_planners.hpp"

#include <algorithm>

namespace tb {
namespace eikplan {

int incidence(int64_t n_nodes, int64_t n_cells, int nverts, const int32_t *conn, IncidenceHost &out)
{
    out = IncidenceHost();
    if (n_nodes < 0 || n_cells < 0 || (nverts != 4 && nverts != 8) || (n_cells > 0 && !conn)) { set_error("eikonal plan: bad argument"); return plan::ERR_BAD_ARG; }
    const int ntet = nverts == 8 ? 6 : 1;
    out.ntet = ntet;
    if (n_cells > (int64_t)0x7FFFFFFF / (4 * ntet)) { set_error("eikonal plan: %lld cells exceed the 31-bit corner codes", (long long)n_cells); return plan::ERR_BAD_ARG; }
    for (int64_t i = 0; i < n_cells * nverts; ++i)
        if (conn[i] < 0 || conn[i] >= n_nodes) { set_error("eikonal plan: node %d of cell %lld outside [0, %lld)", conn[i], (long long)(i / nverts), (long long)n_nodes); return plan::ERR_BAD_ARG; }
    static const int TET[1][4] = {{0, 1, 2, 3}};
    const int (*loc)[4] = ntet == 6 ? KUHN : TET;
    out.ptr.assign((size_t)n_nodes + 1, 0);
    for (int64_t c = 0; c < n_cells; ++c)
        for (int k = 0; k < ntet; ++k)
            for (int a = 0; a < 4; ++a) ++out.ptr[(size_t)conn[c * nverts + loc[k][a]] + 1];
    for (int64_t v = 0; v < n_nodes; ++v) out.ptr[(size_t)v + 1] += out.ptr[(size_t)v];
    const int64_t nrec = out.ptr[(size_t)n_nodes];
    out.code.resize((size_t)nrec);
    out.others.resize((size_t)nrec * 3);
    std::vector<int64_t> fill(out.ptr.begin(), out.ptr.end() - 1);
    for (int64_t c = 0; c < n_cells; ++c)       // ascending (cell, k): every node's records arrive in that order
        for (int k = 0; k < ntet; ++k)
            for (int a = 0; a < 4; ++a) {
                const int32_t v = conn[c * nverts + loc[k][a]];
                const int64_t r = fill[(size_t)v]++;
                out.code[(size_t)r] = (int32_t)((c * ntet + k) * 4 + a);
                int o = 0;
                for (int b = 0; b < 4; ++b)
                    if (b != a) out.others[(size_t)r * 3 + o++] = conn[c * nverts + loc[k][b]];
            }
    out.adj_ptr.assign((size_t)n_nodes + 1, 0);
    out.adj.reserve((size_t)nrec);
    std::vector<int32_t> tmp;
    for (int64_t v = 0; v < n_nodes; ++v) {
        tmp.assign(out.others.begin() + 3 * out.ptr[(size_t)v], out.others.begin() + 3 * out.ptr[(size_t)v + 1]);
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        tmp.erase(std::remove(tmp.begin(), tmp.end(), (int32_t)v), tmp.end()); // a cell that names a node twice
        out.adj.insert(out.adj.end(), tmp.begin(), tmp.end());
        out.adj_ptr[(size_t)v + 1] = (int64_t)out.adj.size();
    }
    return 0;
}

} // namespace eikplan
} // namespace tb

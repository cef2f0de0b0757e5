// tb_interface_planners.cpp — the host planner of the interface unit (tb_interface_planners.hpp): contribution list of the ordered gather.
#include "tb_interface_planners.hpp"

#include <algorithm>

namespace tb {
namespace ifplan {

int contributions(int64_t n, int nf, const int32_t *edofs, const plan::PatternView &p, InterfaceHost &out)
{
    out.nz.clear(); out.ptr.assign(1, 0); out.src.clear();
    if (n < 0 || (nf != 2 && nf != 4) || (n > 0 && !edofs)) { set_error("interface plan: bad argument"); return plan::ERR_BAD_ARG; }
    const int nd = 2 * nf;
    if (n > (int64_t)(0x7FFFFFFF / (nf * nf))) { set_error("interface plan: %lld interface elements exceed the 31-bit positions", (long long)n); return plan::ERR_BAD_ARG; }
    struct Item { int64_t nz; int64_t seq; uint32_t src; };
    std::vector<Item> items((size_t)n * nd * nd);
    for (int64_t e = 0; e < n; ++e) {
        const int32_t *d = edofs + e * nd;
        for (int I = 0; I < nd; ++I)
            if (d[I] < 0 || d[I] >= p.n_rows) { set_error("interface plan: dof %d of interface element %lld outside the pattern", d[I], (long long)e); return plan::ERR_BAD_ARG; }
        for (int I = 0; I < nd; ++I) {
            const int32_t *b = p.colidx + p.rowptr[d[I]], *en = p.colidx + p.rowptr[d[I] + 1];
            for (int J = 0; J < nd; ++J) {
                const int32_t *it = std::lower_bound(b, en, d[J]);
                if (it == en || *it != d[J]) {
                    set_error("interface plan: coupling (%d, %d) of interface element %lld missing from the CSR pattern", d[I], d[J], (long long)e);
                    return plan::ERR_PATTERN;
                }
                const uint32_t pos = (uint32_t)(e * nf * nf + (I % nf) * nf + (J % nf));
                items[(size_t)(e * nd + I) * nd + J] = Item{(int64_t)(it - p.colidx), (e * nd + I) * nd + J, pos << 1 | (I / nf == J / nf ? 1u : 0u)};
            }
        }
    }
    std::sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.nz != b.nz ? a.nz < b.nz : a.seq < b.seq; });
    out.src.reserve(items.size());
    for (size_t k = 0; k < items.size(); ++k) {
        if (k == 0 || items[k].nz != items[k - 1].nz) {
            if (k) out.ptr.push_back((int64_t)k);
            out.nz.push_back(items[k].nz);
        }
        out.src.push_back(items[k].src);
    }
    if (!items.empty()) out.ptr.push_back((int64_t)items.size());
    return 0;
}

} // namespace ifplan
} // namespace tb

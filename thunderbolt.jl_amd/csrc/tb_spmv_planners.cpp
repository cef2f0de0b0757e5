// tb_spmv_planners.cpp — the host planners of the SpMV unit (tb_spmv_planners.hpp): block columns, row runs, row signatures, mirror slices, diagonal
// positions.  Every array is what the product kernels of tb_spmv.hip read, byte for byte.
#include "tb_spmv_planners.hpp"

#include <algorithm>
#include <unordered_map>

namespace tb {
namespace plan {

bool block3_columns(const PatternView &p, std::vector<int32_t> &bcol)
{
    const int64_t nnz = nnz_of(p);
    bcol.clear();
    if (p.n_rows % 3 != 0 || nnz % 9 != 0 || nnz == 0) return false;
    const int64_t *rp = p.rowptr;
    const int32_t *ci = p.colidx;
    bcol.resize((size_t)(nnz / 9));
    const int64_t nbr = p.n_rows / 3;
    for (int64_t R = 0; R < nbr; ++R) {
        const int64_t k0 = rp[3 * R], k1 = rp[3 * R + 1], k2 = rp[3 * R + 2], k3 = rp[3 * R + 3];
        const int64_t L = k1 - k0;
        bool ok = L % 3 == 0 && k2 - k1 == L && k3 - k2 == L && k0 % 9 == 0;
        for (int64_t j = 0; ok && j < L; j += 3) {
            const int32_t c = ci[k0 + j];
            ok = c % 3 == 0 && ci[k0 + j + 1] == c + 1 && ci[k0 + j + 2] == c + 2;
        }
        for (int64_t j = 0; ok && j < L; ++j) ok = ci[k1 + j] == ci[k0 + j] && ci[k2 + j] == ci[k0 + j];
        if (!ok) { bcol.clear(); return false; }
        for (int64_t j = 0; j < L; j += 3) bcol[(size_t)(k0 / 9 + j / 3)] = ci[k0 + j] / 3;
    }
    return true;
}

bool row_runs(const PatternView &p, int cap, std::vector<uint32_t> &rec)
{
    const int64_t *rp = p.rowptr;
    rec.clear();
    std::vector<int32_t> cut{0};
    int64_t start = 0;
    for (int64_t r = 0; r < p.n_rows; ++r) {
        if (rp[r + 1] - rp[r] > cap - 2) return false;
        if (rp[r + 1] - rp[start] > cap - 2 || r - start >= 60000) { cut.push_back((int32_t)r); start = r; }
    }
    cut.push_back((int32_t)p.n_rows);
    rec.resize(4 * (cut.size() - 1));
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
        const int64_t k0 = rp[cut[b]], len = rp[cut[b + 1]] - k0;
        rec[4 * b] = (uint32_t)cut[b];
        rec[4 * b + 1] = (uint32_t)(cut[b + 1] - cut[b]) | (uint32_t)len << 16;
        rec[4 * b + 2] = (uint32_t)((uint64_t)k0 & 0xffffffffu);
        rec[4 * b + 3] = (uint32_t)((uint64_t)k0 >> 32);
    }
    return true;
}

bool row_signatures(const PatternView &p, int64_t budget, SigHost &out)
{
    out = SigHost();
    const int64_t n = p.n_rows;
    if (n == 0 || nnz_of(p) >= (int64_t)0xffffffffll) return false;
    const int64_t *rp = p.rowptr;
    const int32_t *ci = p.colidx;
    std::vector<uint64_t> hsh((size_t)n);
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < n; ++r) {
        uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t)(rp[r + 1] - rp[r]);
        for (int64_t k = rp[r]; k < rp[r + 1]; ++k) {
            h ^= (uint64_t)(uint32_t)(ci[k] - (int32_t)r) + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
            h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
        }
        hsh[r] = h;
    }
    std::vector<uint32_t> rowsig((size_t)n);
    std::vector<int32_t> tab;
    std::unordered_map<uint64_t, std::vector<uint32_t>> seen; // hash → positions of the signatures with that hash
    std::unordered_map<uint32_t, int32_t> len_at;             // position → length of the signature that starts there
    auto same = [&](uint32_t at, int64_t r) {
        const int64_t len = rp[r + 1] - rp[r];
        if ((int64_t)at + len > (int64_t)tab.size()) return false;
        for (int64_t k = 0; k < len; ++k) if (tab[at + k] != ci[rp[r] + k] - (int32_t)r) return false;
        return true;
    };
    int64_t nsig = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = rp[r + 1] - rp[r];
        if (r > 0 && hsh[r] == hsh[r - 1] && rp[r] - rp[r - 1] == len && same(rowsig[r - 1], r)) { rowsig[r] = rowsig[r - 1]; continue; }
        auto &cand = seen[hsh[r]];
        bool found = false;
        for (uint32_t at : cand) if (len_at[at] == (int32_t)len && same(at, r)) { rowsig[r] = at; found = true; break; }
        if (found) continue;
        const uint32_t at = (uint32_t)tab.size();
        for (int64_t k = 0; k < len; ++k) tab.push_back(ci[rp[r] + k] - (int32_t)r);
        if (len == 0) tab.push_back(0); // an empty row still owns a (never read) position
        cand.push_back(at); len_at[at] = (int32_t)len; rowsig[r] = at; ++nsig;
        if ((int64_t)tab.size() > budget) return false;
    }
    tab.resize(tab.size() + SIG_SLACK, 0);
    out.n_sig = nsig;
    out.rowsig = std::move(rowsig);
    out.tab = std::move(tab);
    return true;
}

bool mirror_slices(const PatternView &p, const uint32_t *rowsig, MirrorHost &out)
{
    out = MirrorHost();
    const int64_t *rp = p.rowptr;
    const int64_t ns = (p.n_rows + 63) / 64;
    std::vector<MirrorSlice> rec((size_t)ns + 1);
    std::vector<int32_t> offs;
    int64_t at = 0;
    for (int64_t s = 0; s < ns; ++s) {
        const int64_t r0 = 64 * s, r1 = std::min<int64_t>(r0 + 64, p.n_rows);
        int64_t w = 0;
        bool uni = rowsig && r1 - r0 == 64;
        for (int64_t r = r0; r < r1; ++r) {
            w = std::max<int64_t>(w, rp[r + 1] - rp[r]);
            uni = uni && rowsig[r] == rowsig[r0];
        }
        if (w > 255) return false;
        rec[s] = MirrorSlice{at, uni ? -1 : (int64_t)offs.size(), uni ? rowsig[r0] : MIRROR_MIXED, (uint32_t)w, {0, 0}};
        if (!uni) {
            const size_t o0 = offs.size();
            offs.resize(o0 + (size_t)(64 * w), MIRROR_NONE);
            for (int64_t r = r0; r < r1; ++r)
                for (int64_t k = rp[r]; k < rp[r + 1]; ++k) offs[o0 + (size_t)(64 * (k - rp[r]) + (r - r0))] = p.colidx[k] - (int32_t)r;
        }
        at += 64 * w;
    }
    rec[ns] = MirrorSlice{at, -1, MIRROR_MIXED, 0, {0, 0}};
    if (offs.empty()) offs.push_back(0);
    out.entries = at;
    out.slices = std::move(rec);
    out.offs = std::move(offs);
    return true;
}

std::vector<int64_t> diagonal_positions(const PatternView &p)
{
    std::vector<int64_t> pos((size_t)p.n_rows, -1);
    for (int64_t r = 0; r < p.n_rows; ++r)
        for (int64_t k = p.rowptr[r]; k < p.rowptr[r + 1]; ++k)
            if (p.colidx[k] == r) { pos[r] = k; break; }
    return pos;
}

} // namespace plan
} // namespace tb

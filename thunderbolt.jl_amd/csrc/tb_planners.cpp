// tb_planners.cpp — host-side assembly plans as pure functions (the analogue of setup_operator, src/solver/interface.jl:17-94:
// colouring, element-assembly maps, patch decomposition).  tb_plans.cpp owns the environment, the caches and the device copies.
#include <algorithm>
#include <parallel/algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "tb_planners.hpp"

namespace tb {
namespace plan {

static Outcome refused(int code) { Outcome o; o.kind = Outcome::REFUSED; o.code = code; return o; }

// dof → contributing element-vector slots (cell*ndpc + local), ordered by cell
void dof_slots(const MeshView &m, std::vector<int64_t> &ptr, std::vector<int32_t> &src)
{
    const int64_t n = m.n_cells * m.ndpc;
    ptr.assign(m.ndofs + 1, 0);
    for (int64_t i = 0; i < n; ++i) ptr[m.cell_dofs[i] + 1]++;
    for (int64_t d = 0; d < m.ndofs; ++d) ptr[d + 1] += ptr[d];
    std::vector<int64_t> pos(ptr.begin(), ptr.end() - 1);
    src.resize(n);
    for (int64_t i = 0; i < n; ++i) src[pos[m.cell_dofs[i]]++] = (int32_t)i;
}

// fixed-width form of the slot lists (width = the largest number of cells at a dof, rounded up to a multiple of 8)
SlotTable slot_table(const MeshView &m)
{
    std::vector<int64_t> ptr;
    std::vector<int32_t> src;
    dof_slots(m, ptr, src);
    int64_t w = 0;
    for (int64_t d = 0; d < m.ndofs; ++d) w = std::max(w, ptr[d + 1] - ptr[d]);
    w = (w + 7) / 8 * 8;
    SlotTable t;
    t.w = (int)w;
    t.ell.assign((size_t)m.ndofs * w, -1);
    for (int64_t d = 0; d < m.ndofs; ++d) std::copy(src.begin() + ptr[d], src.begin() + ptr[d + 1], t.ell.begin() + d * w);
    t.h_done.resize((size_t)m.ndofs);
    int32_t run = 0;
    for (int64_t d = 0; d < m.ndofs; ++d) { // slots of a dof are cell-ordered: the last one is its last cell
        if (ptr[d + 1] > ptr[d]) run = std::max(run, src[ptr[d + 1] - 1] / m.ndpc);
        t.h_done[d] = run;
    }
    return t;
}

// scalar Q2 element strategy: the slot table for element matrices stored in tensor order (slot = cell · 27 + i₀ + 3 i₁ + 9 i₂ of the local row)
void tensor_order(std::vector<int32_t> &ell)
{
    static const uint8_t trow[27] = {0, 2, 8, 6, 18, 20, 26, 24, 1, 5, 7, 3, 19, 23, 25, 21, 9, 11, 17, 15, 4, 10, 14, 16, 12, 22, 13}; // Ferrite node → tensor index
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < (int64_t)ell.size(); ++k)
        if (ell[k] >= 0) ell[k] = ell[k] / 27 * 27 + trow[ell[k] % 27];
}

// Greedy colouring of the cell conflict graph (two cells conflict iff they share a dof): smallest colour not used by any neighbour, neighbours
// found through a per-dof colour bitmask.  Over all cells, or over a subset (subdomain forms: one integrator per SubDofHandler in the reference).
int color_cells(const MeshView &m, const int32_t *cells, int64_t n, ColorHost &out)
{
    auto cell = [&](int64_t i) { return cells ? cells[i] : (int32_t)i; };
    std::vector<uint64_t> used(m.ndofs, 0);
    std::vector<int32_t> color(n);
    int ncolors = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t *d = &m.cell_dofs[(int64_t)cell(i) * m.ndpc];
        uint64_t mask = 0;
        for (int l = 0; l < m.ndpc; ++l) mask |= used[d[l]];
        const int col = mask == ~0ull ? 64 : __builtin_ctzll(~mask);
        if (col >= 64) { set_error("colouring needs more than 64 colours"); return ERR_UNSUPPORTED; }
        color[i] = col;
        ncolors = std::max(ncolors, col + 1);
        for (int l = 0; l < m.ndpc; ++l) used[d[l]] |= 1ull << col;
    }
    out.ncolors = ncolors;
    out.offsets.assign(ncolors + 1, 0);
    for (int64_t i = 0; i < n; ++i) out.offsets[color[i] + 1]++;
    for (int k = 0; k < ncolors; ++k) out.offsets[k + 1] += out.offsets[k];
    std::vector<int64_t> pos(out.offsets.begin(), out.offsets.end() - 1);
    out.cells.resize(n);
    for (int64_t i = 0; i < n; ++i) out.cells[pos[color[i]]++] = cell(i);
    return 0;
}

static inline uint64_t spread21(uint64_t v)
{
    v &= 0x1fffff;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}

// Extent of a hexahedron along the three coordinate axes for the layer count of the bucket construction: per axis the largest component of the
// three face-centre-to-face-centre vectors.  On a distorted structured grid these average to the layer spacing exactly (they telescope along a
// grid line), so extent / mean comes out as the number of layers; the bounding box of a sheared cell is larger than the spacing (216 layers of a
// mesh perturbed by 0.2 h counted as ≈ 200 buckets: tiles then cut through the layers, ragged faces, patches of 270 instances and 158 rows).
static inline void hex_axis_extents(const double *xyz, const int32_t *cn, double (&ext)[3])
{
    static const int lo_hi[3][2][4] = {{{0, 3, 4, 7}, {1, 2, 5, 6}}, {{0, 1, 4, 5}, {3, 2, 7, 6}}, {{0, 1, 2, 3}, {4, 5, 6, 7}}};
    ext[0] = ext[1] = ext[2] = 0.0;
    for (int k = 0; k < 3; ++k) {
        double e[3] = {0, 0, 0};
        for (int a = 0; a < 4; ++a)
            for (int d = 0; d < 3; ++d) e[d] += 0.25 * (xyz[3 * (int64_t)cn[lo_hi[k][1][a]] + d] - xyz[3 * (int64_t)cn[lo_hi[k][0][a]] + d]);
        for (int d = 0; d < 3; ++d) ext[d] = std::max(ext[d], std::fabs(e[d]));
    }
}

// Tile of bucket b (0 ≤ b < R) along one axis, for tiles of at most `tile` layers, split evenly instead of cutting full tiles and leaving a sliver:
//   by_nodes: the R + 1 node layers are dealt to ⌈(R + 1) / tile⌉ tiles in balanced groups and a cell goes with its upper node layer (rows are
//   owned by first touch, so the tile of cell b owns node layer b + 1 and the first tile node layer 0 as well) — no tile owns more than `tile`
//   layers of rows, the domain-boundary tiles included (cutting at multiples of `tile` gave the first tile tile + 1 layers: too many rows for the
//   LDS block, so those patches were split again, and 216 = 43 × 5 + 1 left a one-cell sliver of tiles along two faces);
//   otherwise the R cell layers are dealt to ⌈R / tile⌉ tiles (patches that own cells, not rows).
static inline uint64_t balanced_tile(uint32_t b, int64_t R, int tile, bool by_nodes)
{
    if (by_nodes) { const int64_t nt = (R + 1 + tile - 1) / tile; return (uint64_t)(((int64_t)b + 1) * nt / (R + 1)); }
    const int64_t nt = (R + tile - 1) / tile;
    return (uint64_t)((int64_t)b * nt / R);
}

// Recursive bisection of the cell centroids into ⌈nc / target⌉ leaves of equal size (± 1 cell).  Every split cuts the current subset across the axis
// along which it holds the most cell LAYERS (extent ÷ mean cell extent: the halo of a patch counts cells, and anisotropic cells — the ventricle's are
// ≈ 2 : 2 : 1 — would otherwise give leaves twice as long in cells), in proportion to the leaves either side receives.  Tiles of per-axis buckets fill a
// curved thin-walled mesh badly (the idealised ventricle: 132 instances per 256-lane patch, 2.28 per cell); leaves follow the geometry.
static void bisect_cells(const std::vector<double> &cen, const std::vector<double> &cext, int64_t nc, int64_t target, std::vector<int32_t> &leaf)
{
    const int64_t L = (nc + target - 1) / target;
    std::vector<int32_t> ids(nc);
    for (int64_t c = 0; c < nc; ++c) ids[c] = (int32_t)c;
    struct Job { int64_t b, e, l0, nl; };
    std::vector<Job> stack{{0, nc, 0, L}};
    leaf.assign(nc, 0);
    while (!stack.empty()) {
        const Job j = stack.back(); stack.pop_back();
        if (j.nl <= 1 || j.e - j.b <= 1) { for (int64_t k = j.b; k < j.e; ++k) leaf[ids[k]] = (int32_t)j.l0; continue; }
        double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300}, es[3] = {0, 0, 0};
        for (int64_t k = j.b; k < j.e; ++k)
            for (int d = 0; d < 3; ++d) {
                const double v = cen[3 * (size_t)ids[k] + d];
                mn[d] = std::min(mn[d], v); mx[d] = std::max(mx[d], v); es[d] += cext[3 * (size_t)ids[k] + d];
            }
        int ax = 0;
        double best = -1.0;
        for (int d = 0; d < 3; ++d) {
            const double layers = es[d] > 0.0 ? (mx[d] - mn[d]) * (double)(j.e - j.b) / es[d] : 0.0;
            if (layers > best) { best = layers; ax = d; }
        }
        const int64_t nl_left = j.nl / 2, mid = j.b + (j.e - j.b) * nl_left / j.nl;
        std::nth_element(ids.begin() + j.b, ids.begin() + mid, ids.begin() + j.e,
                         [&](int32_t a, int32_t b) { const double va = cen[3 * (size_t)a + ax], vb = cen[3 * (size_t)b + ax]; return va < vb || (va == vb && a < b); });
        stack.push_back({mid, j.e, j.l0 + nl_left, j.nl - nl_left});
        stack.push_back({j.b, mid, j.l0, nl_left});
    }
}

// Quantile buckets.  Per axis the cells are ranked by centroid coordinate and cut into R_d equal-count buckets, R_d = extent / mean cell extent:
// on (mildly distorted) structured grids the buckets are exactly the cell layers (i,j,k), on unstructured meshes they adapt to the local density.
struct CellBuckets {
    std::vector<double> cen, cext; // centroid and axis extents of every cell
    std::vector<uint32_t> bucket;  // 3 per cell
    int64_t Rv[3] = {1, 1, 1};
};

static void cell_buckets(const MeshView &m, CellBuckets &B)
{
    const int64_t nc = m.n_cells;
    const int nv = m.nverts;
    B.cen.resize((size_t)nc * 3); B.cext.resize((size_t)nc * 3); B.bucket.resize((size_t)nc * 3);
    std::vector<double> &cen = B.cen, &cext = B.cext;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, hsum[3] = {0, 0, 0};
#pragma omp parallel for schedule(static) reduction(min : lo[:3]) reduction(max : hi[:3]) reduction(+ : hsum[:3])
    for (int64_t c = 0; c < nc; ++c) {
        double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300}, sum[3] = {0, 0, 0};
        for (int a = 0; a < nv; ++a)
            for (int d = 0; d < 3; ++d) {
                const double v = m.xyz[3 * (int64_t)m.conn[c * nv + a] + d];
                sum[d] += v; mn[d] = std::min(mn[d], v); mx[d] = std::max(mx[d], v);
            }
        double ext[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
        if (nv == 8) hex_axis_extents(m.xyz, &m.conn[c * 8], ext);
        for (int d = 0; d < 3; ++d) {
            cen[3 * c + d] = sum[d] / nv;
            cext[3 * c + d] = ext[d];
            lo[d] = std::min(lo[d], mn[d]); hi[d] = std::max(hi[d], mx[d]); hsum[d] += ext[d];
        }
    }
    for (int d = 0; d < 3; ++d) { // one axis after the other, every sort on the whole team — three one-thread sorts of 10⁷ pairs took 1.0 s
        const double hmean = hsum[d] / (double)std::max<int64_t>(nc, 1);
        int64_t R = hmean > 0 ? (int64_t)std::llround((hi[d] - lo[d]) / hmean) : 1;
        R = std::min<int64_t>(std::max<int64_t>(R, 1), 1 << 21);
        B.Rv[d] = R;
        std::vector<std::pair<double, int32_t>> byc(nc);
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < nc; ++c) byc[c] = {cen[3 * c + d], (int32_t)c};
        __gnu_parallel::sort(byc.begin(), byc.end());
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < nc; ++r) B.bucket[3 * (size_t)byc[r].second + d] = (uint32_t)((r * R) / nc);
    }
}

// Inside a patch, cells (= threads) and hence row slots are ordered lexicographically (x fastest): lanes of a
// wave then hit consecutive rows of the LDS accumulator block — stride-27 addresses, free of bank conflicts.
struct LexLess {
    const uint32_t *bucket;
    bool operator()(int32_t a, int32_t b) const
    {
        const uint32_t *A = &bucket[3 * (size_t)a], *B = &bucket[3 * (size_t)b];
        if (A[2] != B[2]) return A[2] < B[2];
        if (A[1] != B[1]) return A[1] < B[1];
        if (A[0] != B[0]) return A[0] < B[0];
        return a < b;
    }
};

using Keyed = std::vector<std::pair<uint64_t, int32_t>>;

static void leaf_keys(const CellBuckets &B, int64_t nc, int64_t target, Keyed &keyed)
{
    std::vector<int32_t> leaf;
    bisect_cells(B.cen, B.cext, nc, target, leaf);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nc; ++c) keyed[c] = {(uint64_t)leaf[c], (int32_t)c};
}

// Patch decomposition.  Cells are ordered along a Morton curve through their centroids (works for any
// unstructured mesh), cut into runs of `cells_per_patch`; a dof is owned by the first patch (in that
// order) that touches it; a patch's element list = every cell touching one of its rows.
// Patch shape.  Default: tiles of 7×7×7 bucket cells — 343 owned rows (≈80 KB of LDS accumulators, two
// workgroups per CU) and 8³ = 512 cell instances = exactly two full 256-thread sweeps.
int patch_plan(const MeshView &m, const Options &o, int leaf, int shrink, PatchHost &out)
{
    int tile[3] = {o.tile[0], o.tile[1], o.tile[2]};
    const bool default_tile = shrink == 0 && !o.tile_set;
    bool use_tiles = !o.morton;
    if (leaf == 0) // the k-th reduction of the tile: the largest extent, first of equals
        for (int k = 0; k < shrink; ++k) { int d = 0; for (int j = 1; j < 3; ++j) if (tile[j] > tile[d]) d = j; if (tile[d] > 1) --tile[d]; }
    int cells_per_patch = use_tiles ? tile[0] * tile[1] * tile[2] : o.cells;
    const int64_t nc = m.n_cells;
    const int ndpc = m.ndpc;
    StageTimer timer("build_patch_plan", o.verbose, false); // the upload of the plan closes the builder's lines
    // 1. Morton order over quantile buckets
    Keyed keyed(nc);
    CellBuckets B;
    cell_buckets(m, B);
    // A bucket holds more than one cell where cells overlap in every coordinate — the six tetrahedra of a split hexahedron span the same box.  A
    // tile is then cut only at its boundary, not after tile-volume cells (runs of 343 tetrahedra were flat slabs with four times their own
    // number of halo instances), and is 5×5×5 buckets by default (6·10⁶ tetrahedra: mass 0.25 → 0.19 ms, diffusion 0.36 → 0.25 ms, source
    // 0.26 → 0.16 ms; 7×7×7: 0.28 / 0.32 / 0.14 ms; scripts/bench_tets.py)
    if (use_tiles) {
        const int64_t per_bucket = nc / (B.Rv[0] * B.Rv[1] * B.Rv[2]); // 1 on hexahedral meshes, 6 on their tetrahedral splits
        if (per_bucket >= 2) {
            if (default_tile) tile[0] = tile[1] = tile[2] = 5;
            cells_per_patch = (int)std::min<int64_t>((int64_t)tile[0] * tile[1] * tile[2] * per_bucket, 1 << 20);
        }
    }
    if (leaf > 0) { // chosen by fit_fused when the tile plan's fill is poor
        leaf_keys(B, nc, leaf, keyed);
        use_tiles = true; // a leaf is a tile: a patch ends where the key changes
        cells_per_patch = leaf + 1;
    } else {
        auto tile_of = [&](uint32_t b, int d) -> uint64_t { return o.full_cut ? (uint64_t)(b / tile[d]) : balanced_tile(b, B.Rv[d], tile[d], o.by_nodes); };
#pragma omp parallel for schedule(static)
        for (int64_t c = 0; c < nc; ++c) {
            const uint32_t *b = &B.bucket[3 * c];
            if (use_tiles) { // tile id (z-major), 21 bits per axis
                const uint64_t ti = tile_of(b[0], 0), tj = tile_of(b[1], 1), tk = tile_of(b[2], 2);
                keyed[c] = {(tk << 42) | (tj << 21) | ti, (int32_t)c};
            } else {
                keyed[c] = {spread21(b[0]) | spread21(b[1]) << 1 | spread21(b[2]) << 2, (int32_t)c};
            }
        }
    }
    std::vector<double>().swap(B.cen); std::vector<double>().swap(B.cext);
    timer.lap("buckets, keys");
    __gnu_parallel::sort(keyed.begin(), keyed.end());
    timer.lap("key sort");
    // 2. patch boundaries + row ownership by first touch, in Morton order.  A patch closes after `cells_per_patch`
    //    cells or when it would own more than 9/8 of that many rows (domain-boundary patches own the extra
    //    boundary layers), which bounds the LDS accumulator block of every workgroup.
    const int max_rows_cfg = leaf > 0 ? leaf + leaf / 4 // leaves at the surface of the domain own its extra node layers
                                      : use_tiles ? cells_per_patch + 8 : cells_per_patch + cells_per_patch / 8;
    std::vector<int32_t> owner(m.ndofs, -1);
    std::vector<int64_t> pstart(1, 0);
    {
        int rows_in = 0, cells_in = 0;
        for (int64_t k = 0; k < nc; ++k) {
            const int32_t c = keyed[k].second;
            int newrows = 0;
            for (int l = 0; l < ndpc; ++l) newrows += owner[m.cell_dofs[(int64_t)c * ndpc + l]] < 0;
            const bool new_tile = use_tiles && k > 0 && keyed[k].first != keyed[k - 1].first;
            if (cells_in == cells_per_patch || new_tile || (cells_in > 0 && rows_in + newrows > max_rows_cfg)) {
                pstart.push_back(k);
                rows_in = 0; cells_in = 0;
            }
            const int32_t pid = (int32_t)pstart.size() - 1;
            for (int l = 0; l < ndpc; ++l) {
                int32_t &ow = owner[m.cell_dofs[(int64_t)c * ndpc + l]];
                if (ow < 0) { ow = pid; ++rows_in; }
            }
            ++cells_in;
        }
        pstart.push_back(nc);
    }
    const int64_t np = (int64_t)pstart.size() - 1;
    timer.lap("ownership sweep");
    const LexLess lex_less{B.bucket.data()};
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < np; ++q)
        std::sort(keyed.begin() + pstart[q], keyed.begin() + pstart[q + 1],
                  [&](const std::pair<uint64_t, int32_t> &a, const std::pair<uint64_t, int32_t> &b) { return lex_less(a.second, b.second); });
    timer.lap("per-patch sorts");
    // 3. dof → cells
    std::vector<int64_t> sptr;
    std::vector<int32_t> ssrc;
    dof_slots(m, sptr, ssrc);
    timer.lap("dof -> cells");

    PatchHost plan;
    plan.cells_per_patch = cells_per_patch;
    plan.n_patches = np;
    plan.h_elem_ptr.assign(np + 1, 0);
    plan.h_row_ptr.assign(np + 1, 0);
    plan.h_elem_cell.reserve((size_t)(nc * 1.7) + 1024);
    plan.h_row_dof.reserve(m.ndofs);
    plan.h_elem_lrow.reserve((size_t)(nc * 1.7 * ndpc) + 1024);
    std::vector<int32_t> slot_of(m.ndofs, -1);
    std::vector<int32_t> cell_stamp(nc, -1);
    for (int64_t p = 0; p < np; ++p) {
        const int64_t k0 = pstart[p], k1 = pstart[p + 1];
        const size_t row_begin = plan.h_row_dof.size(), elem_begin = plan.h_elem_cell.size();
        // owned rows in first-touch order; own cells first in the element list
        for (int64_t k = k0; k < k1; ++k) {
            const int32_t c = keyed[k].second;
            cell_stamp[c] = (int32_t)p;
            plan.h_elem_cell.push_back(c);
            for (int l = 0; l < ndpc; ++l) {
                const int32_t d = m.cell_dofs[(int64_t)c * ndpc + l];
                if (owner[d] == p && slot_of[d] < 0) {
                    slot_of[d] = (int32_t)(plan.h_row_dof.size() - row_begin);
                    plan.h_row_dof.push_back(d);
                }
            }
        }
        // halo cells: every other cell touching an owned row
        const size_t row_end = plan.h_row_dof.size();
        for (size_t r = row_begin; r < row_end; ++r) {
            const int32_t d = plan.h_row_dof[r];
            for (int64_t s = sptr[d]; s < sptr[d + 1]; ++s) {
                const int32_t c = ssrc[s] / ndpc;
                if (cell_stamp[c] != p) { cell_stamp[c] = (int32_t)p; plan.h_elem_cell.push_back(c); }
            }
        }
        const size_t elem_end = plan.h_elem_cell.size();
        std::sort(plan.h_elem_cell.begin() + elem_begin + (k1 - k0), plan.h_elem_cell.begin() + elem_end, lex_less); // halo cells
        if (row_end - row_begin >= 0xFFFF) { set_error("patch owns too many rows (%zu)", row_end - row_begin); return ERR_UNSUPPORTED; }
        for (size_t e = elem_begin; e < elem_end; ++e) {
            const int32_t c = plan.h_elem_cell[e];
            for (int l = 0; l < ndpc; ++l) {
                const int32_t d = m.cell_dofs[(int64_t)c * ndpc + l];
                plan.h_elem_lrow.push_back(owner[d] == p ? (uint16_t)slot_of[d] : (uint16_t)0xFFFF);
            }
        }
        for (size_t r = row_begin; r < row_end; ++r) slot_of[plan.h_row_dof[r]] = -1;
        plan.h_elem_ptr[p + 1] = (int64_t)elem_end;
        plan.h_row_ptr[p + 1] = (int64_t)row_end;
        plan.max_elems = std::max<int>(plan.max_elems, (int)(elem_end - elem_begin));
        plan.max_rows = std::max<int>(plan.max_rows, (int)(row_end - row_begin));
    }
    timer.lap("instances of every patch");
    // 256-thread workgroups (two resident per CU at the kernels' register / LDS budget, so one patch's write-out
    // overlaps the other's arithmetic); measured best on MI355X among 64…512
    plan.threads = std::min(256, std::max(64, (plan.max_elems + 63) / 64 * 64));
    if (o.threads >= 64 && o.threads <= 512 && o.threads % 64 == 0) plan.threads = o.threads;
    plan.total_elems = (int64_t)plan.h_elem_cell.size();
    plan.total_rows = (int64_t)plan.h_row_dof.size();
    if (plan.total_rows != m.ndofs) { set_error("patch plan: %lld rows owned, %lld dofs", (long long)plan.total_rows, (long long)m.ndofs); return ERR_BAD_ARG; }
    out = std::move(plan);
    return 0;
}

// LDS offsets of the owned rows: per patch the running sum of the row lengths
std::vector<RowDesc> row_descs(const PatchHost &pp, const PatternView &p, int64_t &maxlen, int64_t &max_entries)
{
    std::vector<RowDesc> row_desc(pp.total_rows);
    maxlen = max_entries = 0;
    for (int64_t q = 0; q < pp.n_patches; ++q) {
        uint64_t off = 0;
        for (int64_t r = pp.h_row_ptr[q]; r < pp.h_row_ptr[q + 1]; ++r) {
            const int32_t d = pp.h_row_dof[r];
            const int64_t len = p.rowptr[d + 1] - p.rowptr[d];
            row_desc[r] = RowDesc{p.rowptr[d], (uint32_t)off, (uint32_t)len};
            off += (uint64_t)len;
            maxlen = std::max(maxlen, len);
        }
        max_entries = std::max<int64_t>(max_entries, (int64_t)off);
    }
    return row_desc;
}

// position of every column dof(j) of a cell inside row `row`; false when a coupling is missing from the pattern (its position is 0)
template <class T>
static bool row_positions(const PatternView &p, int32_t row, const int32_t *d, int n, T *pos)
{
    bool found = true;
    const int32_t *b = &p.colidx[p.rowptr[row]];
    const int32_t *en = &p.colidx[p.rowptr[row + 1]];
    for (int j = 0; j < n; ++j) {
        const int32_t *it = std::lower_bound(b, en, d[j]);
        if (it == en || *it != d[j]) { found = false; pos[j] = 0; continue; }
        pos[j] = (T)(it - b);
    }
    return found;
}

// Matrix extension of the patch plan: LDS offsets of the owned rows and, per element instance, the
// position of every (i,j) coupling inside its row.
Outcome mat_extension(const MeshView &m, const PatternView &p, const PatchHost &pp, const Options &o, MatHost &out)
{
    StageTimer timer("build_patch_mat_plan", o.verbose);
    const int ndpc = m.ndpc;
    int64_t maxlen = 0, max_entries = 0;
    MatHost plan;
    plan.row_desc = row_descs(pp, p, maxlen, max_entries);
    plan.max_lds_entries = (int)max_entries;
    Outcome res;
    res.lds_need = max_entries * 8 + (int64_t)pp.max_rows * 16;
    if (res.lds_need > 160 * 1024 || max_entries >= 0xFFFF) {
        set_error("patch plan needs %lld B of LDS per patch (>160 KiB): lower TB_PATCH_TILE / TB_PATCH_CELLS", (long long)(max_entries * 8));
        res.kind = Outcome::TOO_BIG;
        return res;
    }
    const bool wide = maxlen > 255;
    const size_t n = (size_t)pp.total_elems * ndpc * ndpc;
    if (wide) plan.cp16.assign(n, 0); else plan.cp8.assign(n, 0);
    plan.rowoff.assign((size_t)pp.total_elems * ndpc, 0xFFFF);
    std::vector<int32_t> patch_of_elem(pp.total_elems);
    for (int64_t q = 0; q < pp.n_patches; ++q)
        for (int64_t e = pp.h_elem_ptr[q]; e < pp.h_elem_ptr[q + 1]; ++e) patch_of_elem[e] = (int32_t)q;
    bool missing = false;
#pragma omp parallel for schedule(static) reduction(|| : missing)
    for (int64_t e = 0; e < pp.total_elems; ++e) {
        const int32_t *d = &m.cell_dofs[(int64_t)pp.h_elem_cell[e] * ndpc];
        const int64_t r0 = pp.h_row_ptr[patch_of_elem[e]];
        for (int i = 0; i < ndpc; ++i) {
            const uint16_t slot = pp.h_elem_lrow[e * ndpc + i];
            if (slot == 0xFFFF) continue;
            plan.rowoff[e * ndpc + i] = (uint16_t)plan.row_desc[r0 + slot].off;
            const size_t k = ((size_t)e * ndpc + i) * ndpc;
            if (!(wide ? row_positions(p, d[i], d, ndpc, &plan.cp16[k]) : row_positions(p, d[i], d, ndpc, &plan.cp8[k]))) missing = true;
        }
    }
    if (missing) { set_error("patch plan: a cell coupling is missing from the CSR pattern"); return refused(ERR_PATTERN); }
    out = std::move(plan);
    return res;
}

static inline uint64_t mix64(uint64_t h, uint64_t v)
{
    h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
    h *= 0xff51afd7ed558ccdull;
    return h ^ (h >> 33);
}

// Fused-kernel extension of the patch plan (see PatchFusedPlan).  Needs a scalar first-order field whose local dof a sits on
// local vertex a (Ferrite: vertex dofs in vertex order), i.e. a one-to-one node ↔ dof relation; rows of at most 255 entries.
Outcome fused_extension(const MeshView &m, const PatternView &p, const PatchHost &pp, const Options &o, int nregions, FusedHost &out)
{
    StageTimer timer("build_patch_fused_plan_impl", o.verbose);
    const int ndpc = m.ndpc;
    const bool hex = ndpc == 8 && m.nverts == 8, tet = ndpc == 4 && m.nverts == 4;
    if (!(hex || tet) || m.ncomp != 1) { set_error("fused patch plan: needs a scalar first-order field on hexahedra or tetrahedra"); return refused(ERR_UNSUPPORTED); }
    const int NV = ndpc, NS = NV * NV; // nodes per cell, bytes per position signature
    FusedHost plan;
    // 1. row descriptors and the LDS need
    int64_t maxlen = 0, max_entries = 0;
    plan.row_desc = row_descs(pp, p, maxlen, max_entries);
    if (maxlen > 255) { set_error("fused patch plan: a row has %lld entries (> 255)", (long long)maxlen); return refused(ERR_UNSUPPORTED); }
    plan.max_lds_entries = (int)((max_entries + 1) & ~(int64_t)1);
    // 2. per-patch node lists and patch-local node indices of every instance
    std::vector<int64_t> &node_ptr = plan.node_ptr;
    std::vector<int32_t> &pnode = plan.pnode;
    std::vector<uint16_t> &ln = plan.ln;
    node_ptr.assign(pp.n_patches + 1, 0);
    pnode.reserve((size_t)(m.n_nodes * 2.2) + 1024);
    ln.resize((size_t)pp.total_elems * NV);
    std::vector<int32_t> local_of(m.n_nodes, -1);
    bool bad = false;
    int max_nodes = 0;
    for (int64_t q = 0; q < pp.n_patches; ++q) {
        const int64_t r0 = pp.h_row_ptr[q], nrows = pp.h_row_ptr[q + 1] - r0;
        const size_t base = pnode.size();
        pnode.resize(base + nrows, -1);
        for (int64_t e = pp.h_elem_ptr[q]; e < pp.h_elem_ptr[q + 1]; ++e) { // owned slots first
            const int32_t c = pp.h_elem_cell[e];
            for (int a = 0; a < NV; ++a) {
                const uint16_t slot = pp.h_elem_lrow[e * NV + a];
                if (slot == 0xFFFF) continue;
                const int32_t node = m.conn[(int64_t)c * NV + a];
                int32_t &dst = pnode[base + slot];
                if (dst < 0) { dst = node; local_of[node] = slot; }
                else if (dst != node) bad = true;
            }
        }
        for (int64_t e = pp.h_elem_ptr[q]; e < pp.h_elem_ptr[q + 1]; ++e) {
            const int32_t c = pp.h_elem_cell[e];
            for (int a = 0; a < NV; ++a) {
                const int32_t node = m.conn[(int64_t)c * NV + a];
                if (local_of[node] < 0) { local_of[node] = (int32_t)(pnode.size() - base); pnode.push_back(node); }
                else if (pp.h_elem_lrow[e * NV + a] == 0xFFFF && local_of[node] < nrows) bad = true; // an owned node reached through a dof the patch does not own
                ln[(size_t)e * NV + a] = (uint16_t)local_of[node];
            }
        }
        const size_t nn = pnode.size() - base;
        if (nn >= 0xFFFF) { set_error("fused patch plan: a patch touches %zu nodes", nn); return refused(ERR_UNSUPPORTED); }
        max_nodes = std::max(max_nodes, (int)nn);
        for (size_t k = base; k < pnode.size(); ++k) if (pnode[k] >= 0) local_of[pnode[k]] = -1; else bad = true;
        node_ptr[q + 1] = (int64_t)pnode.size();
    }
    if (bad) { set_error("fused patch plan: dofs and vertices of the field are not in one-to-one correspondence"); return refused(ERR_UNSUPPORTED); }
    plan.max_nodes = max_nodes;
    const int64_t acc_entries = plan.max_lds_entries;
    Outcome res;
    res.lds_need = (int64_t)nregions * acc_entries * 8 + (int64_t)pp.max_rows * 16 + (int64_t)max_nodes * 24; // + coordinates of the patch's nodes
    if (res.lds_need > LDS_BUDGET || acc_entries >= 0x7fff) { res.kind = Outcome::TOO_BIG; return res; } // the fit shrinks the tile and retries
    // 3. signatures: position of column dof(j) inside row dof(i) for every pair of a cell, de-duplicated
    const int64_t nc = m.n_cells;
    std::vector<uint8_t> sig((size_t)nc * NS);
    std::vector<uint64_t> hash(nc);
    bool missing = false;
#pragma omp parallel for schedule(static) reduction(|| : missing)
    for (int64_t c = 0; c < nc; ++c) {
        uint8_t *sg = &sig[(size_t)c * NS];
        const int32_t *d = &m.cell_dofs[c * NV];
        for (int i = 0; i < NV; ++i) if (!row_positions(p, d[i], d, NV, sg + i * NV)) missing = true;
        uint64_t h = 0x243f6a8885a308d3ull;
        for (int k = 0; k < NS / 8; ++k) { uint64_t v; memcpy(&v, sg + 8 * k, 8); h = mix64(h, v); }
        hash[c] = h;
    }
    if (missing) { set_error("patch plan: a cell coupling is missing from the CSR pattern"); return refused(ERR_PATTERN); }
    std::vector<int32_t> order(nc);
    std::iota(order.begin(), order.end(), 0);
    __gnu_parallel::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        if (hash[a] != hash[b]) return hash[a] < hash[b];
        const int r = memcmp(&sig[(size_t)a * NS], &sig[(size_t)b * NS], NS);
        return r != 0 ? r < 0 : a < b;
    });
    std::vector<uint32_t> cell_sig(nc);
    int64_t nsig = 0;
    for (int64_t k = 0; k < nc; ++k) {
        const int32_t c = order[k];
        if (k == 0 || memcmp(&sig[(size_t)c * NS], &sig[(size_t)order[k - 1] * NS], NS) != 0) {
            plan.sigtab.insert(plan.sigtab.end(), &sig[(size_t)c * NS], &sig[(size_t)c * NS] + NS);
            ++nsig;
        }
        cell_sig[c] = (uint32_t)(nsig - 1);
    }
    plan.nsig = nsig;
    if (o.verbose)
        fprintf(stderr, "[tbhip] fused patch plan: %lld patches, %lld instances (%.3f per cell), max instances/rows/nodes per patch %d/%d/%d, %lld signatures, LDS %lld B for %d block(s)\n",
                (long long)pp.n_patches, (long long)pp.total_elems, (double)pp.total_elems / (double)std::max<int64_t>(nc, 1), pp.max_elems, pp.max_rows, max_nodes,
                (long long)nsig, (long long)res.lds_need, nregions);
    plan.elem_sig.resize(pp.total_elems);
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < pp.total_elems; ++e) plan.elem_sig[e] = cell_sig[pp.h_elem_cell[e]];
    if (pp.max_rows < 1024 && max_nodes < 2048 && pp.max_elems < 2048 && pp.total_elems < (int64_t)0x7fffffff && (int64_t)pnode.size() < (int64_t)0x7fffffff) {
        // inputs of the staged kernels: packed headers, pre-gathered coordinates
        plan.hdr.resize((size_t)pp.n_patches * 4);
        for (int64_t q = 0; q < pp.n_patches; ++q) {
            uint32_t *h = &plan.hdr[4 * q];
            h[0] = (uint32_t)pp.h_elem_ptr[q]; h[1] = (uint32_t)pp.h_row_ptr[q]; h[2] = (uint32_t)node_ptr[q];
            const uint32_t ne = (uint32_t)(pp.h_elem_ptr[q + 1] - pp.h_elem_ptr[q]), nr = (uint32_t)(pp.h_row_ptr[q + 1] - pp.h_row_ptr[q]),
                           nn = (uint32_t)(node_ptr[q + 1] - node_ptr[q]);
            h[3] = nr | nn << 10 | ne << 21;
        }
        plan.pcoord.resize(pnode.size() * 3);
#pragma omp parallel for schedule(static)
        for (int64_t k = 0; k < (int64_t)pnode.size(); ++k)
            for (int d = 0; d < 3; ++d) plan.pcoord[3 * k + d] = m.xyz[3 * (int64_t)pnode[k] + d];
    }
    out = std::move(plan);
    return res;
}

// One-trip records: the arrays of the staged kernel copied patch by patch into fixed-stride records —
//   [0,16) {nrows | nnodes << 10 | ne << 21, first instance, 0, 0} · ne × 16 B local node indices · ne × 4 B signature ids ·
//   rm × 16 B row descriptors · nm × 24 B vertex coordinates; zero padding behind the patch's own counts.
Records record_layout(const PatchHost &pp, int max_nodes)
{
    Records rec;
    if (pp.max_elems > 1024 || pp.max_rows > 256) return rec;
    rec.rm = (pp.max_rows + 3) & ~3; rec.nm = (max_nodes + 3) & ~3; rec.ne = std::max(256, (pp.max_elems + 63) & ~63);
    const size_t raw = 16 + (size_t)rec.ne * 20 + (size_t)rec.rm * 16 + (size_t)rec.nm * 24, stride = (raw + 127) & ~(size_t)127;
    if (stride * (size_t)pp.n_patches > ((size_t)8 << 30)) return rec; // > 8 GiB of records: keep the compact arrays
    rec.stride = (int)stride;
    return rec;
}

// Position of column dof(j) in row dof(i) on a lattice whose rows hold their 27 columns in ascending lexicographic order: 13 + Δx + 3Δy + 9Δz, with the
// vertex bits of Ferrite's hexahedron (-,-,-),(+,-,-),(+,+,-),(-,+,-),(-,-,+),… — the table tb_patch_fused.hip compiles into its CANON instances
static inline int canonical_pos(int i, int j)
{
    static const int bit[3][8] = {{0, 1, 1, 0, 0, 1, 1, 0}, {0, 0, 1, 1, 0, 0, 1, 1}, {0, 0, 0, 0, 1, 1, 1, 1}};
    return 13 + (bit[0][j] - bit[0][i]) + 3 * (bit[1][j] - bit[1][i]) + 9 * (bit[2][j] - bit[2][i]);
}

// Reads the plan's own arrays only (headers, local node indices, signature ids and table, row descriptors): nothing about how the mesh was generated.
RecordClasses classify_records(int64_t np, const uint32_t *hdr, const uint16_t *ln, const uint32_t *sig, const RowDesc *desc, const uint8_t *sigtab)
{
    std::vector<uint8_t> canon((size_t)np, 0);
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < np; ++q) {
        const uint32_t e0 = hdr[4 * q], r0 = hdr[4 * q + 1], w = hdr[4 * q + 3];
        const uint32_t nr = w & 0x3ff, ne = w >> 21;
        bool ok = ne <= 256;
        for (uint32_t k = 0; k < nr && ok; ++k) ok = desc[(size_t)r0 + k].len == 27;
        for (uint32_t e = 0; e < ne && ok; ++e) {
            const uint8_t *sg = sigtab + (size_t)sig[(size_t)e0 + e] * 64;
            for (int i = 0; i < 8 && ok; ++i) {
                if (ln[((size_t)e0 + e) * 8 + i] >= nr) continue; // a row of another patch: this instance adds nothing to it
                for (int j = 0; j < 8; ++j) ok = ok && sg[i * 8 + j] == canonical_pos(i, j);
            }
        }
        canon[q] = ok;
    }
    RecordClasses rc;
    rc.order.reserve((size_t)np);
    for (int64_t q = 0; q < np; ++q) if (!canon[q]) rc.order.push_back(q);
    rc.n_general = (int64_t)rc.order.size();
    for (int64_t q = 0; q < np; ++q) if (canon[q]) rc.order.push_back(q);
    rc.n_canonical = np - rc.n_general;
    return rc;
}

void pack_records(Records &rec, int64_t np, const uint32_t *hdr, const uint16_t *ln, const uint32_t *sig, const RowDesc *desc, const double *xyz, const int64_t *order)
{
    const size_t stride = (size_t)rec.stride, o_ln = 16, o_sig = o_ln + (size_t)rec.ne * 16, o_desc = o_sig + (size_t)rec.ne * 4, o_xyz = o_desc + (size_t)rec.rm * 16;
    rec.bytes.assign(stride * (size_t)np, 0);
#pragma omp parallel for schedule(static)
    for (int64_t s = 0; s < np; ++s) {
        const int64_t q = order ? order[s] : s;
        uint8_t *r = &rec.bytes[stride * (size_t)s];
        const uint32_t e0 = hdr[4 * q], r0 = hdr[4 * q + 1], n0 = hdr[4 * q + 2], w = hdr[4 * q + 3];
        const uint32_t nr = w & 0x3ff, nn = (w >> 10) & 0x7ff, ne = w >> 21;
        const uint32_t h4[4] = {w, e0, 0, 0}; // e0: first instance of the patch in the plan's instance arrays (the kernel names the offending cell through it)
        memcpy(r, h4, 16);
        memcpy(r + o_ln, &ln[(size_t)e0 * 8], (size_t)ne * 16);
        memcpy(r + o_sig, &sig[e0], (size_t)ne * 4);
        memcpy(r + o_desc, &desc[r0], (size_t)nr * 16);
        memcpy(r + o_xyz, &xyz[(size_t)n0 * 3], (size_t)nn * 24);
    }
}

// Patch plan of the vector kernels.  Tiles of 8×8×8 bucket cells, cells ordered lexicographically inside a tile — the same bucket construction
// as patch_plan (quantile buckets per axis: exact layers on structured boxes, density-adaptive on unstructured meshes).
int vec_patch_plan(const MeshView &m, const Options &o, bool halo, VecHost &out)
{
    if (m.ndpc != 8 || m.nverts != 8 || m.ncomp != 1) { set_error("vector patch plan: needs a scalar trilinear hexahedron field"); return ERR_UNSUPPORTED; }
    StageTimer timer("ensure_vec_patch_plan", o.verbose);
    const int *tile = o.vtile;
    const int64_t nc = m.n_cells;
    Keyed keyed(nc);
    CellBuckets B;
    cell_buckets(m, B);
#pragma omp parallel for schedule(static)
    for (int64_t c = 0; c < nc; ++c) {
        uint64_t t3[3];
        for (int d = 0; d < 3; ++d) t3[d] = o.full_cut ? (uint64_t)(B.bucket[3 * c + d] / tile[d]) : balanced_tile(B.bucket[3 * c + d], B.Rv[d], tile[d], halo);
        keyed[c] = {(t3[2] << 42) | (t3[1] << 21) | t3[0], (int32_t)c};
    }
    // Poorly filled tiles (a curved thin wall: most tiles of the bucket grid hold a fraction of their volume, and the halo of a fragment is as large
    // as a full tile's): equal leaves of the recursive bisection instead (bisect_cells; the matrix plan's rule, decided here on this plan's own fill
    // so that the outcome does not depend on which plan of the mesh is built first).
    {
        std::vector<uint64_t> keys(nc);
        for (int64_t c = 0; c < nc; ++c) keys[c] = keyed[c].first;
        __gnu_parallel::sort(keys.begin(), keys.end());
        const int64_t ntiles = std::unique(keys.begin(), keys.end()) - keys.begin();
        const int64_t vol = (int64_t)tile[0] * tile[1] * tile[2];
        const double fill = ntiles > 0 ? (double)nc / ((double)ntiles * (double)vol) : 1.0;
        if (nc >= 4096 && fill < 0.75 && o.vec_rcb) {
            leaf_keys(B, nc, vol * 7 / 8, keyed);
            if (o.verbose) fprintf(stderr, "[tbhip] vector patch plan: tile fill %.2f -> bisection, %ld leaves of <= %ld cells\n", fill, (long)((nc + vol * 7 / 8 - 1) / (vol * 7 / 8)), (long)(vol * 7 / 8));
        }
    }
    std::vector<double>().swap(B.cen); std::vector<double>().swap(B.cext);
    const LexLess lex_less{B.bucket.data()};
    __gnu_parallel::sort(keyed.begin(), keyed.end(), [&](const std::pair<uint64_t, int32_t> &a, const std::pair<uint64_t, int32_t> &b) {
        return a.first != b.first ? a.first < b.first : lex_less(a.second, b.second);
    });
    // patches: one per tile, cut further so that no patch exceeds 1000 cells (16-bit local node indices, LDS)
    const int cap = std::min(1000, tile[0] * tile[1] * tile[2]);
    std::vector<int64_t> pstart(1, 0);
    for (int64_t k = 1; k < nc; ++k)
        if (keyed[k].first != keyed[k - 1].first || k - pstart.back() >= cap) pstart.push_back(k);
    if (nc > 0) pstart.push_back(nc);
    const int64_t np = (int64_t)pstart.size() - 1;
    // first-touch ownership (halo variant)
    std::vector<int32_t> owner;
    std::vector<int64_t> sptr;
    std::vector<int32_t> ssrc;
    if (halo) {
        owner.assign(m.ndofs, -1);
        for (int64_t q = 0; q < np; ++q)
            for (int64_t k = pstart[q]; k < pstart[q + 1]; ++k)
                for (int l = 0; l < 8; ++l) {
                    int32_t &ow = owner[m.cell_dofs[(int64_t)keyed[k].second * 8 + l]];
                    if (ow < 0) ow = (int32_t)q;
                }
        dof_slots(m, sptr, ssrc);
    }
    VecHost plan;
    plan.halo = halo;
    plan.n_patches = np;
    std::vector<uint32_t> &hdr = plan.hdr;
    std::vector<uint16_t> &ln = plan.ln;
    std::vector<int32_t> &ecell = plan.ecell, &pdof = plan.pdof, pnode;
    hdr.resize((size_t)np * 4);
    ln.reserve((size_t)nc * 8 * (halo ? 3 : 2) / 2);
    ecell.reserve((size_t)nc * (halo ? 3 : 2) / 2);
    std::vector<int32_t> local_of(m.n_nodes, -1), cell_stamp(halo ? nc : 0, -1);
    std::vector<int32_t> cells;
    bool bad = false;
    for (int64_t q = 0; q < np; ++q) {
        cells.clear();
        for (int64_t k = pstart[q]; k < pstart[q + 1]; ++k) cells.push_back(keyed[k].second);
        const size_t nbase = pnode.size();
        if (halo) { // owned nodes first (slot order = first touch inside the patch), then the halo cells
            for (int32_t c : cells) {
                cell_stamp[c] = (int32_t)q;
                for (int a = 0; a < 8; ++a) {
                    const int32_t d = m.cell_dofs[(int64_t)c * 8 + a], node = m.conn[(int64_t)c * 8 + a];
                    if (owner[d] == q && local_of[node] < 0) { local_of[node] = (int32_t)(pnode.size() - nbase); pnode.push_back(node); pdof.push_back(d); }
                }
            }
            const size_t nown = pnode.size() - nbase;
            const size_t nown_cells = cells.size();
            for (size_t r = 0; r < nown; ++r) {
                const int32_t d = pdof[nbase + r];
                for (int64_t s2 = sptr[d]; s2 < sptr[d + 1]; ++s2) {
                    const int32_t c = ssrc[s2] / 8;
                    if (cell_stamp[c] != q) { cell_stamp[c] = (int32_t)q; cells.push_back(c); }
                }
            }
            std::sort(cells.begin() + nown_cells, cells.end(), lex_less);
            hdr[4 * q + 2] = (uint32_t)nown;
        }
        for (int32_t c : cells)
            for (int a = 0; a < 8; ++a) {
                const int32_t d = m.cell_dofs[(int64_t)c * 8 + a], node = m.conn[(int64_t)c * 8 + a];
                if (local_of[node] < 0) { local_of[node] = (int32_t)(pnode.size() - nbase); pnode.push_back(node); pdof.push_back(d); }
                else if (pdof[nbase + local_of[node]] != d) bad = true;
                ln.push_back((uint16_t)local_of[node]);
            }
        for (int32_t c : cells) ecell.push_back(c);
        const size_t nn = pnode.size() - nbase;
        if (nn >= 0xFFFF || cells.size() >= 0xFFFF) { set_error("vector patch plan: patch too large (%zu nodes)", nn); return ERR_UNSUPPORTED; }
        hdr[4 * q] = (uint32_t)(ecell.size() - cells.size());
        hdr[4 * q + 1] = (uint32_t)nbase;
        if (!halo) hdr[4 * q + 2] = (uint32_t)nn; // every touched node is accumulated and added
        hdr[4 * q + 2] |= (uint32_t)nn << 16;
        hdr[4 * q + 3] = (uint32_t)cells.size();
        plan.max_nodes = std::max(plan.max_nodes, (int)nn);
        plan.max_elems = std::max(plan.max_elems, (int)cells.size());
        for (size_t k = nbase; k < pnode.size(); ++k) local_of[pnode[k]] = -1;
    }
    if (bad) { set_error("vector patch plan: dofs and vertices of the field are not in one-to-one correspondence"); return ERR_UNSUPPORTED; }
    // the kernel keeps 32 B per patch node in LDS and is built for three workgroups per CU: fragmented patches (quantile buckets on hollow or
    // strongly graded meshes, a large TB_VPATCH_TILE) that need more than a third of the 160 KiB take the general kernels instead of a launch failure
    if ((int64_t)plan.max_nodes * 32 > 160 * 1024 / 3) {
        set_error("vector patch plan: a patch touches %d nodes (%d B of LDS, more than a third of a CU's 160 KiB)", plan.max_nodes, plan.max_nodes * 32);
        return ERR_UNSUPPORTED;
    }
    if ((int64_t)ecell.size() >= (int64_t)0x7fffffff || (int64_t)pnode.size() >= (int64_t)0x7fffffff) { set_error("vector patch plan: too many instances for 32-bit offsets"); return ERR_UNSUPPORTED; }
    plan.total_elems = (int64_t)ecell.size();
    plan.total_nodes = (int64_t)pnode.size();
    plan.pcoord.resize(pnode.size() * 3);
#pragma omp parallel for schedule(static)
    for (int64_t k = 0; k < (int64_t)pnode.size(); ++k)
        for (int d = 0; d < 3; ++d) plan.pcoord[3 * k + d] = m.xyz[3 * (int64_t)pnode[k] + d];
    if (o.verbose)
        fprintf(stderr, "[tbhip] vector patch plan (%s): %lld patches, %.3f instances per cell, %.3f patch nodes per dof, max %d instances / %d nodes per patch\n",
                halo ? "halo" : "own cells", (long long)np, (double)ecell.size() / (double)std::max<int64_t>(nc, 1), (double)pnode.size() / (double)std::max<int64_t>(m.ndofs, 1),
                plan.max_elems, plan.max_nodes);
    out = std::move(plan);
    return 0;
}

// the current plan released, then the next one built in its place (one plan's host arrays at a time)
static Outcome rebuild(const MeshView &m, const Options &o, int leaf, int shrink, PatchHost &cur, bool &replaced)
{
    cur = PatchHost();
    replaced = true;
    const int rc = patch_plan(m, o, leaf, shrink, cur);
    if (rc) { cur = PatchHost(); return refused(rc); }
    cur.shrink = shrink;
    return Outcome();
}

// one more reduction: a smaller leaf under the bisection plan, the next smaller tile otherwise
static Outcome rebuild_smaller(const MeshView &m, const Options &o, FitState &st, int shrink, PatchHost &cur, bool &replaced)
{
    if (st.patch_rcb > 0) st.patch_rcb = std::max(16, st.patch_rcb * 7 / 8);
    return rebuild(m, o, st.patch_rcb, shrink, cur, replaced);
}

// The patch plan and its matrix extension; the tile shrinks until one patch's LDS block (row accumulators + descriptors) is ≤ 80 KiB.
Outcome fit_mat(const MeshView &m, const PatternView &p, const Options &o, FitState &st, PatchHost &cur, bool &replaced, MatHost &mat)
{
    replaced = false;
    if (cur.h_elem_ptr.empty()) { const Outcome r = rebuild(m, o, st.patch_rcb, 0, cur, replaced); if (!r.ok()) return r; }
    for (int attempt = 0; attempt < 12; ++attempt) {
        mat = MatHost();
        const Outcome r = mat_extension(m, p, cur, o, mat);
        if (r.ok() && (o.fixed || r.lds_need <= LDS_BUDGET)) return r;
        if (r.kind == Outcome::REFUSED) return r;
        if (o.fixed) return refused(ERR_UNSUPPORTED); // too big (the extension said so), and the shape is the user's
        mat = MatHost();
        const int shrink = cur.shrink + 1;
        const Outcome b = rebuild_smaller(m, o, st, shrink, cur, replaced);
        if (!b.ok()) return b;
        if (st.patch_rcb == 0) st.patch_tile_shrink = shrink;
    }
    set_error("patch plan: could not fit the LDS budget");
    return refused(ERR_UNSUPPORTED);
}

// The patch plan and its fused extension so that `nregions` blocks of row accumulators, the row descriptors and the node list of any patch fit 80 KiB of LDS.
Outcome fit_fused(const MeshView &m, const PatternView &p, const Options &o, int nregions, FitState &st, PatchHost &cur, bool &replaced, FusedHost &fused)
{
    replaced = false;
    if (cur.h_elem_ptr.empty()) {
        // Start from the largest tile whose full patch fits the budget by the pattern's longest row, instead of from 7×7×7 with one whole plan build per
        // reduction (216³: six builds of 2.5 s each, 15 of the 21 s of the first assembly).  The estimate is the need of a patch that owns every row of
        // its tile; a plan that still does not fit is reduced further by the loop below.
        int k0 = 0;
        if (!o.fixed && st.patch_rcb == 0 && st.patch_tile_shrink == 0 && m.nverts == 8 && m.ndpc == 8) {
            int64_t max_row_len = p.max_row_len;
            if (!max_row_len) for (int64_t r = 0; r < p.n_rows; ++r) max_row_len = std::max<int64_t>(max_row_len, p.rowptr[r + 1] - p.rowptr[r]);
            int t[3] = {7, 7, 7};
            auto fits = [&]() {
                const int64_t rows = (int64_t)t[0] * t[1] * t[2], nodes = (int64_t)(t[0] + 2) * (t[1] + 2) * (t[2] + 2);
                return (int64_t)nregions * rows * max_row_len * 8 + rows * 16 + nodes * 24 <= LDS_BUDGET;
            };
            while (!fits() && (t[0] > 1 || t[1] > 1 || t[2] > 1)) { // the same reduction patch_plan applies: the largest extent, first of equals
                int d = 0;
                for (int j = 1; j < 3; ++j) if (t[j] > t[d]) d = j;
                --t[d];
                ++k0;
            }
        }
        const Outcome b = rebuild(m, o, st.patch_rcb, k0, cur, replaced);
        if (!b.ok()) return b;
        if (k0) st.patch_tile_shrink = k0;
    }
    for (int attempt = 0; attempt < 16; ++attempt) {
        fused = FusedHost();
        Outcome r = fused_extension(m, p, cur, o, nregions, fused);
        if (r.ok()) {
            // fill of the 256-lane sweeps: tiles of per-axis buckets are full on box-like meshes (236 of 256 at 216³) and half empty on curved thin-walled
            // ones; there the cells are bisected into equal leaves instead (patch_plan, leaf) if that needs clearly fewer patches
            const double fill = (double)cur.total_elems / ((double)cur.n_patches * 256.0);
            if (o.fixed || st.patch_rcb != 0 || st.patch_rcb_tried || !(fill < 0.75) || m.nverts != 8 || m.n_cells < 4096) return r;
            st.patch_rcb_tried = true;
            const int64_t np_tiles = cur.n_patches, inst_tiles = cur.total_elems;
            st.patch_rcb = 128; // ≈ the own cells of a full 5×5×6-node tile; shrunk by the LDS-fit loop like a tile
            fused = FusedHost();
            Outcome b = rebuild(m, o, st.patch_rcb, 0, cur, replaced);
            if (!b.ok()) return b;
            Outcome r2 = refused(ERR_UNSUPPORTED);
            for (int a2 = 0; a2 < 12; ++a2) {
                r2 = fused_extension(m, p, cur, o, nregions, fused);
                if (r2.ok() && cur.max_elems > o.rcb_max_inst && st.patch_rcb > 16) r2.kind = Outcome::TOO_BIG; // a second sweep for many patches: smaller leaves too
                if (r2.ok()) break;
                fused = FusedHost();
                if (r2.kind == Outcome::REFUSED) return r2;
                b = rebuild_smaller(m, o, st, 0, cur, replaced);
                if (!b.ok()) return b;
            }
            const bool better = r2.ok() && cur.n_patches * 10 < np_tiles * 9;
            if (o.verbose)
                fprintf(stderr, "[tbhip] patch plan: tiles %lld patches / %lld instances (fill %.2f), bisection (leaf %d) %lld patches / %lld instances -> %s\n", (long long)np_tiles,
                        (long long)inst_tiles, fill, st.patch_rcb, r2.ok() ? (long long)cur.n_patches : -1LL, r2.ok() ? (long long)cur.total_elems : -1LL,
                        better ? "bisection" : "tiles");
            if (better) return r2;
            // back to the tiles
            st.patch_rcb = 0;
            fused = FusedHost();
            b = rebuild(m, o, 0, st.patch_tile_shrink, cur, replaced);
            if (!b.ok()) return b;
            continue;
        }
        fused = FusedHost();
        if (r.kind == Outcome::REFUSED) return r;
        if (o.fixed) { set_error("patch plan needs %lld B of LDS per patch (> 80 KiB): lower TB_PATCH_TILE / TB_PATCH_CELLS", (long long)r.lds_need); return refused(ERR_UNSUPPORTED); }
        const Outcome b = rebuild_smaller(m, o, st, cur.shrink + 1, cur, replaced);
        if (!b.ok()) return b;
    }
    set_error("patch plan: could not fit the LDS budget");
    return refused(ERR_UNSUPPORTED);
}

// ---- tangent gather of the element strategy on three-component fields (tb_mech_gather.hip) ----

// first-component dof of every node of the vector field (rows of a node are dof0, dof0+1, dof0+2), ascending
std::vector<int32_t> node_list(const MeshView &m)
{
    std::vector<int32_t> d0;
    d0.reserve((size_t)m.ndofs / 3);
    std::vector<uint8_t> seen(m.ndofs, 0);
    for (int64_t i = 0; i < m.n_cells * (m.ndpc / 3); ++i) {
        const int32_t d = m.cell_dofs[3 * i];
        if (!seen[d]) { seen[d] = 1; d0.push_back(d); }
    }
    std::sort(d0.begin(), d0.end());
    return d0;
}

// the gather kernels rely on the three rows of a node being equal-length runs of whole nodes
int node_row_check(const PatternView &p, const std::vector<int32_t> &dof0, int64_t &max_row_len)
{
    max_row_len = 0;
    for (int32_t d : dof0) {
        const int64_t L = p.rowptr[d + 1] - p.rowptr[d];
        if (L % 3 || L != p.rowptr[d + 2] - p.rowptr[d + 1] || L != p.rowptr[d + 3] - p.rowptr[d + 2] || L / 3 > 254) {
            set_error("element assembly gather: rows of node dof %d are not three equal runs of whole nodes (L = %lld)", d, (long long)L);
            return ERR_PATTERN;
        }
        max_row_len = std::max<int64_t>(max_row_len, L);
    }
    return 0;
}

// node records of the staged gather, cells in ascending order like the slot lists.  Not applicable: a node row of more than 384 positions, slots
// beyond int32, or a node in more than 8 cells (the direct gather takes those meshes).
GatherHost gather_nodes(const MeshView &m, const PatternView &p, const std::vector<int32_t> &dof0)
{
    GatherHost out;
    const int nd = m.ndpc, nb = nd / 3;
    const int64_t nn = (int64_t)dof0.size();
    if (p.max_row_len > 384 || m.n_cells * (int64_t)nd >= (int64_t)0x7fffffff) return out;
    std::vector<int32_t> node_of((size_t)m.ndofs, -1);
    for (int64_t i = 0; i < nn; ++i) node_of[dof0[i]] = (int32_t)i;
    std::vector<GatherNode> recs((size_t)nn);
    for (int64_t i = 0; i < nn; ++i) {
        const int32_t d = dof0[i];
        recs[i].g0 = p.rowptr[d];
        recs[i].L = (int32_t)(p.rowptr[d + 1] - p.rowptr[d]);
        recs[i].nk = 0;
        for (int k = 0; k < 8; ++k) recs[i].slot[k] = 0;
    }
    for (int64_t c = 0; c < m.n_cells; ++c)
        for (int a = 0; a < nb; ++a) {
            GatherNode &g = recs[node_of[m.cell_dofs[c * nd + 3 * a]]];
            if (g.nk >= 8) return out;
            g.slot[g.nk++] = (int32_t)(c * nd + 3 * a);
        }
    // running maximum of the last contributing cell over the records (dof order): the records before the first one whose value reaches c are complete
    // once cells [0, c) are integrated — the prefix the chunked linearisation gathers behind the integration front.  On a mesh numbered cell by cell
    // the prefix trails the front by about one layer of cells.
    out.last.resize((size_t)nn);
    int32_t run = 0;
    for (int64_t i = 0; i < nn; ++i) { run = std::max(run, recs[i].slot[recs[i].nk - 1] / nd); out.last[i] = run; }
    out.recs = std::move(recs);
    out.applicable = true;
    return out;
}

} // namespace plan
} // namespace tb

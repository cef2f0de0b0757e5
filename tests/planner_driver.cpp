// Stand-alone driver of the host planners (thunderbolt.jl_amd/csrc/tb_planners.cpp, tb_spmv_planners.cpp): no GPU, no HIP.  Links the two planner files and
// tb_hostgen.cpp only.
//   planner_driver <mesh directory> [case]
// reads the meshes tests/test_planners_cpu.py wrote (<name>.xyz: float64 × 3 per node, <name>.conn: int32 per cell vertex), plans every case, checks
// the invariants a plan must keep whatever its layout (they do not depend on the recorded digests) and prints "case/part/array value" lines:
// FNV-1a-64 digests of the raw bytes of every plan array, and the plan scalars.  Exit status 0: every invariant holds.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "tbhip.h"
#include "tb_planners.hpp"
#include "tb_spmv_planners.hpp"

namespace tb { void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); } }
using namespace tb;
using namespace tb::plan;

struct Mesh {
    int kind = 0, ncomp = 1, nverts = 0, ndpc = 0;
    int64_t n_nodes = 0, n_cells = 0, ndofs = 0;
    std::vector<double> xyz;
    std::vector<int32_t> conn, cd, colidx;
    std::vector<int64_t> rowptr;
    MeshView view() const { return {n_nodes, n_cells, ndofs, nverts, ndpc, ncomp, xyz.data(), conn.data(), cd.data()}; }
    PatternView pattern() const { return {ndofs, rowptr.data(), colidx.data(), 0}; }
};

struct Fit { // what a fit leaves behind: the return code, the state the mesh remembers, the plans
    int rc = 0;
    FitState st;
    PatchHost patch;
    MatHost mat;
    FusedHost fused;
    Records rec;
};

// ---- the planners under test ----
// f is empty, or holds the plan and the state an earlier fit left, as a mesh does at a refit
static void mat_into(const Mesh &M, const Options &o, Fit &f)
{
    bool replaced;
    const Outcome r = fit_mat(M.view(), M.pattern(), o, f.st, f.patch, replaced, f.mat);
    f.rc = r.ok() ? 0 : r.code;
}

static void fused_into(const Mesh &M, int nregions, Fit &f)
{
    bool replaced;
    const Outcome r = fit_fused(M.view(), M.pattern(), Options(), nregions, f.st, f.patch, replaced, f.fused);
    f.rc = r.ok() ? 0 : r.code;
    f.rec = Records();
    if (r.ok() && M.ndpc == 8 && !f.fused.hdr.empty()) { // the one-trip records of the hexahedron kernel
        f.rec = record_layout(f.patch, f.fused.max_nodes);
        if (f.rec.stride > 0) pack_records(f.rec, f.patch.n_patches, f.fused.hdr.data(), f.fused.ln.data(), f.fused.elem_sig.data(), f.fused.row_desc.data(), f.fused.pcoord.data());
    }
}

static Fit run_mat(const Mesh &M, const Options &o = Options()) { Fit f; mat_into(M, o, f); return f; }
static Fit run_fused(const Mesh &M, int nregions) { Fit f; fused_into(M, nregions, f); return f; }
// one mesh through its life: the fused plan for one block, refitted for three, then the matrix extension on the plan that is there
static void run_refit(const Mesh &M, Fit &fused2, Fit &mat3)
{
    Fit f;
    fused_into(M, 1, f);
    if (!f.rc) fused_into(M, 3, f);
    fused2 = f;
    if (!f.rc) mat_into(M, Options(), f);
    mat3 = f;
}

static int run_vec(const Mesh &M, bool halo, VecHost &out) { return vec_patch_plan(M.view(), Options(), halo, out); }
static int run_colors(const Mesh &M, const std::vector<int32_t> *cells, ColorHost &out)
{
    return color_cells(M.view(), cells ? cells->data() : nullptr, cells ? (int64_t)cells->size() : M.n_cells, out);
}
static void run_slots(const Mesh &M, std::vector<int64_t> &ptr, std::vector<int32_t> &src) { dof_slots(M.view(), ptr, src); }
static void run_slot_table(const Mesh &M, SlotTable &t, std::vector<int32_t> &ell_t)
{
    t = slot_table(M.view());
    ell_t = t.ell;
    tensor_order(ell_t);
}
// ---- output ----

static std::string g_case;
static int g_failed = 0;

#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (g_failed++ < 20) { fprintf(stderr, "%s: ", g_case.c_str()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
            return;                                                                   \
        }                                                                             \
    } while (0)

static void scalar(const char *part, const char *name, long long v) { printf("%s/%s/%s %lld\n", g_case.c_str(), part, name, v); }

template <class T>
static void digest(const char *part, const char *name, const std::vector<T> &v)
{
    uint64_t h = 0xcbf29ce484222325ull;
    const uint8_t *b = (const uint8_t *)v.data();
    for (size_t k = 0; k < v.size() * sizeof(T); ++k) { h ^= b[k]; h *= 0x100000001b3ull; }
    printf("%s/%s/%s %zu:%016llx\n", g_case.c_str(), part, name, v.size(), (unsigned long long)h);
}

// ---- invariants ----

static void check_patch(const Mesh &M, const PatchHost &pp)
{
    const int n = M.ndpc;
    CHECK((int64_t)pp.h_elem_ptr.size() == pp.n_patches + 1 && (int64_t)pp.h_row_ptr.size() == pp.n_patches + 1, "patch pointer arrays");
    CHECK(pp.total_rows == M.ndofs && (int64_t)pp.h_row_dof.size() == M.ndofs && pp.h_row_ptr.back() == M.ndofs, "rows owned: %lld of %lld", (long long)pp.total_rows, (long long)M.ndofs);
    CHECK(pp.total_elems == (int64_t)pp.h_elem_cell.size() && pp.h_elem_ptr.back() == pp.total_elems && (int64_t)pp.h_elem_lrow.size() == pp.total_elems * n, "instance arrays");
    std::vector<int32_t> owner(M.ndofs, -1), stamp(M.n_cells, -1), seen(M.n_cells, 0);
    for (int64_t q = 0; q < pp.n_patches; ++q)
        for (int64_t r = pp.h_row_ptr[q]; r < pp.h_row_ptr[q + 1]; ++r) {
            const int32_t d = pp.h_row_dof[r];
            CHECK(d >= 0 && d < M.ndofs && owner[d] < 0, "dof %d is owned twice", d); // with total_rows == ndofs: every dof exactly once
            owner[d] = (int32_t)q;
        }
    std::vector<int64_t> inst(pp.total_elems); // (patch, cell) of every instance
    for (int64_t q = 0; q < pp.n_patches; ++q)
        for (int64_t e = pp.h_elem_ptr[q]; e < pp.h_elem_ptr[q + 1]; ++e) inst[e] = q << 32 | pp.h_elem_cell[e];
    std::sort(inst.begin(), inst.end());
    int max_elems = 0, max_rows = 0;
    for (int64_t q = 0; q < pp.n_patches; ++q) {
        const int64_t r0 = pp.h_row_ptr[q], nrows = pp.h_row_ptr[q + 1] - r0;
        int next_slot = 0; // own cells first: the row slots are numbered in first-touch order of the instance list
        for (int64_t e = pp.h_elem_ptr[q]; e < pp.h_elem_ptr[q + 1]; ++e) {
            const int32_t c = pp.h_elem_cell[e];
            CHECK(c >= 0 && c < M.n_cells && stamp[c] != q, "patch %lld lists cell %d twice", (long long)q, c);
            stamp[c] = (int32_t)q; seen[c] = 1;
            for (int l = 0; l < n; ++l) {
                const int32_t d = M.cd[(int64_t)c * n + l];
                const uint16_t s = pp.h_elem_lrow[e * n + l];
                if (owner[d] != q) { CHECK(s == 0xFFFF, "patch %lld: slot of a row it does not own", (long long)q); continue; }
                CHECK(s < nrows && pp.h_row_dof[r0 + s] == d, "patch %lld instance %lld: slot %d does not hold dof %d", (long long)q, (long long)e, (int)s, d);
                CHECK(s <= next_slot, "patch %lld: row slots are not in first-touch order", (long long)q);
                if (s == next_slot) ++next_slot;
            }
        }
        CHECK(next_slot == nrows, "patch %lld: %d of %lld rows touched", (long long)q, next_slot, (long long)nrows);
        max_elems = std::max(max_elems, (int)(pp.h_elem_ptr[q + 1] - pp.h_elem_ptr[q]));
        max_rows = std::max(max_rows, (int)nrows);
    }
    CHECK(max_elems == pp.max_elems && max_rows == pp.max_rows, "max_elems / max_rows");
    for (int64_t c = 0; c < M.n_cells; ++c) { // every cell touching an owned row is an instance of the patch that owns the row
        CHECK(seen[c], "cell %lld is in no patch", (long long)c);
        for (int l = 0; l < n; ++l) CHECK(std::binary_search(inst.begin(), inst.end(), (int64_t)owner[M.cd[c * n + l]] << 32 | c), "patch %d misses cell %lld", owner[M.cd[c * n + l]], (long long)c);
    }
}

static void check_row_desc(const Mesh &M, const PatchHost &pp, const std::vector<RowDesc> &desc, int64_t max_lds_entries, bool even)
{
    CHECK((int64_t)desc.size() == pp.total_rows, "row descriptors: count");
    int64_t mx = 0;
    for (int64_t q = 0; q < pp.n_patches; ++q) {
        int64_t off = 0;
        for (int64_t r = pp.h_row_ptr[q]; r < pp.h_row_ptr[q + 1]; ++r) {
            const int32_t d = pp.h_row_dof[r];
            CHECK(desc[r].nz0 == M.rowptr[d] && desc[r].len == M.rowptr[d + 1] - M.rowptr[d] && desc[r].off == off, "row descriptor %lld", (long long)r);
            off += desc[r].len;
        }
        mx = std::max(mx, off);
    }
    CHECK(max_lds_entries == (even ? (mx + 1) & ~(int64_t)1 : mx), "max_lds_entries %lld, rows sum to %lld", (long long)max_lds_entries, (long long)mx);
}

static void check_mat(const Mesh &M, const PatchHost &pp, const MatHost &h, bool fixed)
{
    const int n = M.ndpc;
    check_row_desc(M, pp, h.row_desc, h.max_lds_entries, false);
    const int64_t need = (int64_t)h.max_lds_entries * 8 + (int64_t)pp.max_rows * 16; // a fixed shape (TB_PATCH_TILE) is accepted up to a CU's 160 KiB
    CHECK(need <= (fixed ? 2 * LDS_BUDGET : LDS_BUDGET), "the chosen plan needs %lld B of LDS", (long long)need);
    const bool wide = !h.cp16.empty();
    CHECK((wide ? h.cp16.size() : h.cp8.size()) == (size_t)pp.total_elems * n * n && h.cp8.empty() == wide && h.rowoff.size() == (size_t)pp.total_elems * n, "matrix extension: sizes");
    for (int64_t q = 0; q < pp.n_patches; ++q)
        for (int64_t e = pp.h_elem_ptr[q]; e < pp.h_elem_ptr[q + 1]; ++e) {
            const int32_t *d = &M.cd[(int64_t)pp.h_elem_cell[e] * n];
            for (int i = 0; i < n; ++i) {
                const uint16_t s = pp.h_elem_lrow[e * n + i];
                CHECK(h.rowoff[e * n + i] == (s == 0xFFFF ? 0xFFFF : h.row_desc[pp.h_row_ptr[q] + s].off), "row offset of instance %lld", (long long)e);
                if (s == 0xFFFF) continue;
                for (int j = 0; j < n; ++j) {
                    const size_t k = ((size_t)e * n + i) * n + j;
                    const int64_t pos = wide ? h.cp16[k] : h.cp8[k];
                    CHECK(M.rowptr[d[i]] + pos < M.rowptr[d[i] + 1] && M.colidx[M.rowptr[d[i]] + pos] == d[j], "column position of instance %lld (%d,%d)", (long long)e, i, j);
                }
            }
        }
}

// `cap` bytes at r: the first `used` equal src, the rest is zero
static bool section(const uint8_t *r, size_t cap, const void *src, size_t used)
{
    if (used > cap || (used && memcmp(r, src, used) != 0)) return false;
    for (size_t k = used; k < cap; ++k) if (r[k]) return false;
    return true;
}

static void check_fused(const Mesh &M, const PatchHost &pp, const FusedHost &h, const Records &rec, int nregions)
{
    const int n = M.ndpc, ns = n * n;
    const int64_t np = pp.n_patches;
    check_row_desc(M, pp, h.row_desc, h.max_lds_entries, true);
    CHECK((int64_t)nregions * h.max_lds_entries * 8 + (int64_t)pp.max_rows * 16 + (int64_t)h.max_nodes * 24 <= LDS_BUDGET, "the chosen plan does not fit 80 KiB for %d block(s)", nregions);
    CHECK((int64_t)h.node_ptr.size() == np + 1 && h.node_ptr.back() == (int64_t)h.pnode.size() && h.ln.size() == (size_t)pp.total_elems * n &&
          h.elem_sig.size() == (size_t)pp.total_elems && h.sigtab.size() == (size_t)h.nsig * ns, "fused extension: sizes");
    int max_nodes = 0;
    for (int64_t q = 0; q < np; ++q) {
        const int64_t n0 = h.node_ptr[q], nn = h.node_ptr[q + 1] - n0, nrows = pp.h_row_ptr[q + 1] - pp.h_row_ptr[q];
        max_nodes = std::max(max_nodes, (int)nn);
        for (int64_t e = pp.h_elem_ptr[q]; e < pp.h_elem_ptr[q + 1]; ++e) {
            const int32_t c = pp.h_elem_cell[e], *d = &M.cd[(int64_t)c * n];
            CHECK(h.elem_sig[e] < h.nsig, "signature id of instance %lld", (long long)e);
            const uint8_t *sg = &h.sigtab[(size_t)h.elem_sig[e] * ns];
            for (int a = 0; a < n; ++a) {
                const uint16_t l = h.ln[(size_t)e * n + a], s = pp.h_elem_lrow[e * n + a];
                CHECK(l < nn && h.pnode[n0 + l] == M.conn[(int64_t)c * n + a], "local node of instance %lld", (long long)e);
                CHECK(s == 0xFFFF ? l >= nrows : l == s, "owned rows come first in the node list (instance %lld)", (long long)e);
                for (int j = 0; j < n; ++j) CHECK(M.rowptr[d[a]] + sg[a * n + j] < M.rowptr[d[a] + 1] && M.colidx[M.rowptr[d[a]] + sg[a * n + j]] == d[j], "signature of instance %lld (%d,%d)", (long long)e, a, j);
            }
        }
    }
    CHECK(max_nodes == h.max_nodes, "max_nodes");
    if (h.hdr.empty()) return;
    CHECK(h.hdr.size() == (size_t)np * 4 && h.pcoord.size() == h.pnode.size() * 3, "staged inputs: sizes");
    for (int64_t q = 0; q < np; ++q) {
        const uint32_t ne = (uint32_t)(pp.h_elem_ptr[q + 1] - pp.h_elem_ptr[q]), nr = (uint32_t)(pp.h_row_ptr[q + 1] - pp.h_row_ptr[q]), nn = (uint32_t)(h.node_ptr[q + 1] - h.node_ptr[q]);
        CHECK(h.hdr[4 * q] == pp.h_elem_ptr[q] && h.hdr[4 * q + 1] == pp.h_row_ptr[q] && h.hdr[4 * q + 2] == h.node_ptr[q] && h.hdr[4 * q + 3] == (nr | nn << 10 | ne << 21) && nr < 1024 && nn < 2048 && ne < 2048, "header of patch %lld", (long long)q);
    }
    for (size_t k = 0; k < h.pnode.size(); ++k) CHECK(memcmp(&h.pcoord[3 * k], &M.xyz[3 * (size_t)h.pnode[k]], 24) == 0, "coordinates of patch node %zu", k);
    if (rec.stride <= 0) return;
    CHECK(rec.bytes.size() == (size_t)rec.stride * np && rec.stride % 128 == 0 && rec.rm >= pp.max_rows && rec.nm >= h.max_nodes && rec.ne >= pp.max_elems, "records: layout");
    const size_t o_sig = 16 + (size_t)rec.ne * 16, o_desc = o_sig + (size_t)rec.ne * 4, o_xyz = o_desc + (size_t)rec.rm * 16, end = o_xyz + (size_t)rec.nm * 24;
    CHECK(end <= (size_t)rec.stride, "records: stride");
    for (int64_t q = 0; q < np; ++q) {
        const uint8_t *r = &rec.bytes[(size_t)rec.stride * q];
        const uint32_t e0 = h.hdr[4 * q], r0 = h.hdr[4 * q + 1], n0 = h.hdr[4 * q + 2], w = h.hdr[4 * q + 3], h4[4] = {w, e0, 0, 0};
        const size_t nr = w & 0x3ff, nn = (w >> 10) & 0x7ff, ne = w >> 21;
        CHECK(section(r, 16, h4, 16) && section(r + 16, o_sig - 16, &h.ln[(size_t)e0 * 8], ne * 16) && section(r + o_sig, o_desc - o_sig, &h.elem_sig[e0], ne * 4) &&
              section(r + o_desc, o_xyz - o_desc, &h.row_desc[r0], nr * 16) && section(r + o_xyz, (size_t)rec.stride - o_xyz, &h.pcoord[(size_t)n0 * 3], nn * 24), "record of patch %lld", (long long)q);
    }
}

static void check_vec(const Mesh &M, const VecHost &h)
{
    const int64_t np = h.n_patches;
    CHECK(h.hdr.size() == (size_t)np * 4 && (int64_t)h.ecell.size() == h.total_elems && h.ln.size() == (size_t)h.total_elems * 8 && (int64_t)h.pdof.size() == h.total_nodes &&
          h.pcoord.size() == (size_t)h.total_nodes * 3, "vector plan: sizes");
    std::vector<int32_t> owned(M.ndofs, 0), own_cell(M.n_cells, 0);
    std::vector<const double *> at(M.ndofs, nullptr); // coordinates of the vertex a dof sits on
    for (int64_t c = 0; c < M.n_cells; ++c)
        for (int a = 0; a < 8; ++a) at[M.cd[c * 8 + a]] = &M.xyz[3 * (size_t)M.conn[c * 8 + a]];
    int64_t e0 = 0, n0 = 0;
    int max_nodes = 0, max_elems = 0;
    for (int64_t q = 0; q < np; ++q) {
        const uint32_t nown = h.hdr[4 * q + 2] & 0xFFFF, nn = h.hdr[4 * q + 2] >> 16, ne = h.hdr[4 * q + 3];
        CHECK(h.hdr[4 * q] == e0 && h.hdr[4 * q + 1] == n0 && nown <= nn && (h.halo || nown == nn) && e0 + ne <= h.total_elems && n0 + nn <= h.total_nodes, "vector plan: header of patch %lld", (long long)q);
        for (uint32_t k = 0; k < nn; ++k) {
            const int32_t d = h.pdof[n0 + k];
            CHECK(d >= 0 && d < M.ndofs && memcmp(&h.pcoord[3 * (n0 + k)], at[d], 24) == 0, "vector plan: patch node %lld", (long long)(n0 + k));
            if (k < nown) ++owned[d];
        }
        for (int64_t e = e0; e < e0 + ne; ++e)
            for (int a = 0; a < 8; ++a) {
                const uint16_t l = h.ln[e * 8 + a];
                CHECK(l < nn && h.pdof[n0 + l] == M.cd[(int64_t)h.ecell[e] * 8 + a], "vector plan: local node of instance %lld", (long long)e);
            }
        if (!h.halo) for (int64_t e = e0; e < e0 + ne; ++e) ++own_cell[h.ecell[e]];
        e0 += ne; n0 += nn;
        max_nodes = std::max(max_nodes, (int)nn); max_elems = std::max(max_elems, (int)ne);
    }
    CHECK(e0 == h.total_elems && n0 == h.total_nodes && max_nodes == h.max_nodes && max_elems == h.max_elems, "vector plan: totals");
    if (h.halo) for (int64_t d = 0; d < M.ndofs; ++d) CHECK(owned[d] == 1, "vector plan: dof %lld is stored %d times", (long long)d, owned[d]);
    if (h.halo) { // every (cell, dof) pair is integrated by the patch that stores the dof
        int64_t pairs = 0, e = 0;
        for (int64_t q = 0; q < np; e += h.hdr[4 * q + 3], ++q)
            for (uint32_t k = 0; k < h.hdr[4 * q + 3] * 8; ++k) pairs += h.ln[e * 8 + k] < (h.hdr[4 * q + 2] & 0xFFFF);
        CHECK(pairs == M.n_cells * 8, "vector plan: %lld of %lld (cell, dof) pairs reach their owner", (long long)pairs, (long long)M.n_cells * 8);
    } else
        for (int64_t c = 0; c < M.n_cells; ++c) CHECK(own_cell[c] == 1, "vector plan: cell %lld is integrated %d times", (long long)c, own_cell[c]);
}

static void check_colors(const Mesh &M, const ColorHost &h, int64_t n)
{
    CHECK((int)h.offsets.size() == h.ncolors + 1 && h.offsets.back() == n && (int64_t)h.cells.size() == n, "colour plan: sizes");
    std::vector<int32_t> stamp(M.ndofs, -1);
    for (int k = 0; k < h.ncolors; ++k)
        for (int64_t i = h.offsets[k]; i < h.offsets[k + 1]; ++i)
            for (int l = 0; l < M.ndpc; ++l) {
                int32_t &s = stamp[M.cd[(int64_t)h.cells[i] * M.ndpc + l]];
                CHECK(s != k, "colour %d: two cells share dof %d", k, M.cd[(int64_t)h.cells[i] * M.ndpc + l]);
                s = k;
            }
}

// ---- cases ----

static void emit_patch(const char *part, const Fit &f)
{
    const PatchHost &pp = f.patch;
    scalar(part, "rc", f.rc);
    scalar(part, "patch_rcb", f.st.patch_rcb); scalar(part, "patch_rcb_tried", f.st.patch_rcb_tried); scalar(part, "patch_tile_shrink", f.st.patch_tile_shrink);
    if (f.rc) return;
    scalar(part, "cells_per_patch", pp.cells_per_patch); scalar(part, "shrink", pp.shrink); scalar(part, "n_patches", pp.n_patches); scalar(part, "max_elems", pp.max_elems);
    scalar(part, "max_rows", pp.max_rows); scalar(part, "threads", pp.threads); scalar(part, "total_elems", pp.total_elems); scalar(part, "total_rows", pp.total_rows);
    digest(part, "elem_ptr", pp.h_elem_ptr); digest(part, "row_ptr", pp.h_row_ptr); digest(part, "elem_cell", pp.h_elem_cell); digest(part, "row_dof", pp.h_row_dof); digest(part, "elem_lrow", pp.h_elem_lrow);
}

static void case_mat(const Mesh &M, const Fit &f, const char *part = "mat", bool fixed = false)
{
    emit_patch(part, f);
    if (f.rc) return;
    scalar(part, "max_lds_entries", f.mat.max_lds_entries);
    digest(part, "row_desc", f.mat.row_desc); digest(part, "rowoff", f.mat.rowoff); digest(part, "colpos8", f.mat.cp8); digest(part, "colpos16", f.mat.cp16);
    check_patch(M, f.patch);
    check_mat(M, f.patch, f.mat, fixed);
}

static void case_fused(const Mesh &M, const Fit &f, int nregions, const char *part = "fused")
{
    const FusedHost &h = f.fused;
    emit_patch(part, f);
    if (f.rc) return;
    scalar(part, "max_lds_entries", h.max_lds_entries); scalar(part, "max_nodes", h.max_nodes); scalar(part, "nsig", h.nsig);
    digest(part, "node_ptr", h.node_ptr); digest(part, "pnode", h.pnode); digest(part, "elem_ln", h.ln); digest(part, "elem_sig", h.elem_sig); digest(part, "sigtab", h.sigtab);
    digest(part, "row_desc", h.row_desc); digest(part, "hdr", h.hdr); digest(part, "pcoord", h.pcoord);
    scalar(part, "rec_stride", f.rec.stride); scalar(part, "rec_rm", f.rec.rm); scalar(part, "rec_nm", f.rec.nm); scalar(part, "rec_ne", f.rec.ne);
    digest(part, "rec", f.rec.bytes);
    check_patch(M, f.patch);
    check_fused(M, f.patch, h, f.rec, nregions);
}

static void case_vec(const Mesh &M, bool halo)
{
    const char *part = halo ? "vec_halo" : "vec_own";
    VecHost h;
    const int rc = run_vec(M, halo, h);
    scalar(part, "rc", rc);
    if (rc) return;
    scalar(part, "n_patches", h.n_patches); scalar(part, "total_elems", h.total_elems); scalar(part, "total_nodes", h.total_nodes); scalar(part, "max_nodes", h.max_nodes); scalar(part, "max_elems", h.max_elems);
    digest(part, "hdr", h.hdr); digest(part, "elem_ln", h.ln); digest(part, "elem_cell", h.ecell); digest(part, "pcoord", h.pcoord); digest(part, "pdof", h.pdof);
    check_vec(M, h);
}

static void case_colors(const Mesh &M, const char *part, const std::vector<int32_t> *cells)
{
    ColorHost h;
    const int rc = run_colors(M, cells, h);
    scalar(part, "rc", rc);
    if (rc) return;
    scalar(part, "ncolors", h.ncolors);
    digest(part, "offsets", h.offsets); digest(part, "cells", h.cells);
    check_colors(M, h, cells ? (int64_t)cells->size() : M.n_cells);
}

// the host planning of the tangent gather on a three-component field: node list, row check, node records.  Everything is checked against a brute-force
// pass over cell_dofs and rowptr that shares nothing with the planner.
static void case_gather(const Mesh &M, const char *part, bool applies)
{
    const int nd = M.ndpc, nb = nd / 3;
    const std::vector<int32_t> d0 = node_list(M.view());
    scalar(part, "n_nodes", (long long)d0.size());
    digest(part, "node_dof0", d0);
    std::vector<int32_t> want;
    for (int64_t c = 0; c < M.n_cells; ++c) for (int a = 0; a < nb; ++a) want.push_back(M.cd[c * nd + 3 * a]);
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    CHECK(d0 == want, "%s: the node list is not the sorted set of first-component dofs", part);
    int64_t L = -1;
    const int rc = node_row_check(M.pattern(), d0, L);
    scalar(part, "check_rc", rc);
    if (rc) return;
    scalar(part, "max_row_len", L);
    int64_t longest = 0;
    for (int32_t d : d0) {
        const int64_t l = M.rowptr[d + 1] - M.rowptr[d];
        CHECK(l % 3 == 0 && l / 3 <= 254 && M.rowptr[d + 2] - M.rowptr[d + 1] == l && M.rowptr[d + 3] - M.rowptr[d + 2] == l, "%s: rows of node dof %d passed the check", part, d);
        longest = std::max(longest, l);
    }
    CHECK(L == longest, "%s: max_row_len %lld, longest node row %lld", part, (long long)L, (long long)longest);
    PatternView pv = M.pattern();
    pv.max_row_len = L;
    const GatherHost h = gather_nodes(M.view(), pv, d0);
    scalar(part, "applicable", h.applicable);
    std::vector<std::vector<int32_t>> slots(d0.size()); // per node: cell·ND + 3a of every cell holding it, in cell order
    for (int64_t c = 0; c < M.n_cells; ++c)
        for (int a = 0; a < nb; ++a) slots[std::lower_bound(d0.begin(), d0.end(), M.cd[c * nd + 3 * a]) - d0.begin()].push_back((int32_t)(c * nd + 3 * a));
    size_t most = 0;
    for (const auto &s : slots) most = std::max(most, s.size());
    CHECK(h.applicable == (L <= 384 && most <= 8), "%s: applicable = %d with rows of %lld and %zu cells at a node", part, (int)h.applicable, (long long)L, most);
    CHECK(h.applicable == applies, "%s: applicable = %d", part, (int)h.applicable);
    if (!h.applicable) { CHECK(h.recs.empty() && h.last.empty(), "%s: arrays of a plan that does not apply", part); return; }
    digest(part, "recs", h.recs);
    digest(part, "last", h.last);
    CHECK(h.recs.size() == d0.size() && h.last.size() == d0.size(), "%s: one record per node", part);
    int32_t run = 0;
    for (size_t i = 0; i < d0.size(); ++i) {
        const GatherNode &g = h.recs[i];
        const int32_t d = d0[i];
        CHECK(g.nk >= 1 && (size_t)g.nk == slots[i].size(), "%s: node %zu sits in %zu cells, nk = %d", part, i, slots[i].size(), g.nk);
        for (int k = 0; k < 8; ++k) {
            if (k >= g.nk) { CHECK(g.slot[k] == 0, "%s: node %zu: unused slot %d", part, i, k); continue; }
            const int32_t s = g.slot[k];
            CHECK(s == slots[i][k] && s % nd % 3 == 0 && M.cd[s] == d && (k == 0 || s / nd > g.slot[k - 1] / nd), "%s: node %zu: slot %d", part, i, k);
        }
        CHECK(g.g0 == M.rowptr[d] && g.L == M.rowptr[d + 1] - M.rowptr[d], "%s: node %zu: row pointers", part, i);
        run = std::max(run, g.slot[g.nk - 1] / nd);
        CHECK(h.last[i] == run, "%s: node %zu: running maximum of the last cell", part, i);
    }
}

template <class T>
static bool read_file(const std::string &path, std::vector<T> &v)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); return false; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    const bool ok = fread(v.data(), sizeof(T), v.size(), f) == v.size();
    fclose(f);
    return ok;
}

static bool load(const std::string &dir, const char *name, int kind, int ncomp, Mesh &M)
{
    M = Mesh();
    M.kind = kind; M.ncomp = ncomp;
    M.nverts = kind == TB_TET4 ? 4 : 8;
    M.ndpc = (kind == TB_HEX27 ? 27 : M.nverts) * ncomp;
    if (!read_file(dir + "/" + name + ".xyz", M.xyz) || !read_file(dir + "/" + name + ".conn", M.conn)) return false;
    M.n_nodes = (int64_t)M.xyz.size() / 3;
    M.n_cells = (int64_t)M.conn.size() / M.nverts;
    M.cd.resize((size_t)M.n_cells * M.ndpc);
    M.ndofs = tb_host_close_dofs(kind, ncomp, M.n_cells, M.n_nodes, M.conn.data(), M.cd.data());
    if (M.ndofs <= 0) return false;
    M.rowptr.resize(M.ndofs + 1);
    const int64_t nnz = tb_host_build_pattern(M.n_cells, M.ndpc, M.cd.data(), M.ndofs, M.rowptr.data(), nullptr);
    M.colidx.resize(nnz);
    return tb_host_build_pattern(M.n_cells, M.ndpc, M.cd.data(), M.ndofs, M.rowptr.data(), M.colidx.data()) == nnz;
}

// ---- the SpMV plans (tb_spmv_planners.cpp): block columns, row runs, signatures, mirror slices, diagonal positions of one CSR pattern ----

struct Csr {
    std::vector<int64_t> rp{0};
    std::vector<int32_t> ci;
    int64_t n() const { return (int64_t)rp.size() - 1; }
    PatternView view() const { return {n(), rp.data(), ci.data(), 0}; }
    void row(const std::vector<int32_t> &cols) { ci.insert(ci.end(), cols.begin(), cols.end()); rp.push_back((int64_t)ci.size()); }
    static Csr of(const Mesh &M) { Csr A; A.rp = M.rowptr; A.ci = M.colidx; return A; }
};
static std::vector<int32_t> span(int32_t first, int32_t count) { std::vector<int32_t> v(count); for (int32_t k = 0; k < count; ++k) v[k] = first + k; return v; }

constexpr int SPMV_CAP = 2048; // what tb_spmv.hip passes: the capacity of a run, and the table budget max(nnz / 4, 64)
enum { NO = 0, YES = 1, ANY = -1 };
struct Expect { int b3, streams, compresses, mirror; };

static void check_block3(const char *part, const Csr &A, bool is, const std::vector<int32_t> &bcol, int expect)
{
    CHECK(expect == ANY || is == (expect == YES), "%s: block-3 = %d", part, (int)is);
    if (!is) { CHECK(bcol.empty(), "%s: block columns of a pattern that has none", part); return; }
    CHECK(A.n() % 3 == 0 && bcol.size() * 9 == A.ci.size(), "%s: block columns: size", part);
    for (int64_t r = 0; r < A.n(); ++r) {
        const int64_t k0 = A.rp[r - r % 3];
        CHECK(k0 % 9 == 0 && A.rp[r + 1] - A.rp[r] == A.rp[r - r % 3 + 1] - k0, "%s: row %lld of a block pattern", part, (long long)r);
        for (int64_t j = 0; j < A.rp[r + 1] - A.rp[r]; ++j) CHECK(A.ci[A.rp[r] + j] == 3 * bcol[k0 / 9 + j / 3] + j % 3, "%s: bcol does not rebuild row %lld", part, (long long)r);
    }
}

static void check_runs(const char *part, const Csr &A, bool ok, const std::vector<uint32_t> &rec, int expect)
{
    int64_t longest = 0;
    for (int64_t r = 0; r < A.n(); ++r) longest = std::max(longest, A.rp[r + 1] - A.rp[r]);
    CHECK(ok == (longest <= SPMV_CAP - 2) && (expect == ANY || ok == (expect == YES)), "%s: streams = %d with a row of %lld entries", part, (int)ok, (long long)longest);
    if (!ok) { CHECK(rec.empty(), "%s: records of a pattern that does not stream", part); return; }
    CHECK(!rec.empty() && rec.size() % 4 == 0, "%s: run records: size", part);
    int64_t next = 0;
    for (size_t b = 0; b < rec.size() / 4; ++b) {
        const int64_t r0 = rec[4 * b], nr = rec[4 * b + 1] & 0xffffu, len = rec[4 * b + 1] >> 16, k0 = (int64_t)((uint64_t)rec[4 * b + 3] << 32 | rec[4 * b + 2]);
        CHECK(r0 == next && r0 + nr <= A.n() && (nr > 0 || A.n() == 0), "%s: run %zu does not continue the partition", part, b);
        CHECK(nr <= 60000 && len <= SPMV_CAP - 2, "%s: run %zu exceeds a limit (%lld rows, %lld entries)", part, b, (long long)nr, (long long)len);
        CHECK(k0 == A.rp[r0] && len == A.rp[r0 + nr] - k0, "%s: run %zu: record fields", part, b);
        next = r0 + nr;
    }
    CHECK(next == A.n(), "%s: the runs end at row %lld of %lld", part, (long long)next, (long long)A.n());
}

static void check_sig(const char *part, const Csr &A, int64_t budget, bool ok, const SigHost &h, int expect)
{
    // brute force: the table of the distinct offset lists in order of first appearance (an empty row owns one position)
    std::map<std::vector<int32_t>, int64_t> first;
    int64_t total = 0;
    for (int64_t r = 0; r < A.n(); ++r) {
        std::vector<int32_t> sg;
        for (int64_t k = A.rp[r]; k < A.rp[r + 1]; ++k) sg.push_back(A.ci[k] - (int32_t)r);
        if (first.emplace(sg, total).second) total += std::max<int64_t>((int64_t)sg.size(), 1);
    }
    // (the planner gives up at the first signature that takes the table past the budget; the table only grows, so that is total > budget)
    CHECK(ok == (A.n() > 0 && total <= budget) && (expect == ANY || ok == (expect == YES)), "%s: compresses = %d with a table of %lld entries, budget %lld", part, (int)ok, (long long)total, (long long)budget);
    if (!ok) { CHECK(h.n_sig == 0 && h.rowsig.empty() && h.tab.empty(), "%s: arrays of a pattern that does not compress", part); return; }
    CHECK((int64_t)h.rowsig.size() == A.n() && (int64_t)h.tab.size() == total + SIG_SLACK && h.n_sig == (int64_t)first.size(), "%s: signature plan: %lld signatures in %zu entries, expected %zu in %lld + slack",
          part, (long long)h.n_sig, h.tab.size(), first.size(), (long long)total);
    for (int k = 0; k < SIG_SLACK; ++k) CHECK(h.tab[h.tab.size() - 1 - k] == 0, "%s: the slack is not zero", part);
    for (int64_t r = 0; r < A.n(); ++r) {
        std::vector<int32_t> sg;
        for (int64_t k = A.rp[r]; k < A.rp[r + 1]; ++k) sg.push_back(A.ci[k] - (int32_t)r);
        CHECK(h.rowsig[r] == first[sg], "%s: row %lld: signature at %u, first stored at %lld", part, (long long)r, h.rowsig[r], (long long)first[sg]); // equal signatures are stored once
        for (size_t k = 0; k < sg.size(); ++k) CHECK(h.tab[h.rowsig[r] + k] == sg[k], "%s: row %lld entry %zu: the table does not reproduce colidx - row", part, (long long)r, k);
    }
}

static void check_mirror(const char *part, const Csr &A, const uint32_t *rowsig, bool ok, const MirrorHost &h, int expect)
{
    const int64_t n = A.n(), ns = (n + 63) / 64;
    int64_t longest = 0;
    for (int64_t r = 0; r < n; ++r) longest = std::max(longest, A.rp[r + 1] - A.rp[r]);
    CHECK(ok == (longest <= 255) && (expect == ANY || ok == (expect == YES)), "%s: mirror = %d with a row of %lld entries", part, (int)ok, (long long)longest);
    if (!ok) { CHECK(h.slices.empty() && h.offs.empty() && h.entries == 0, "%s: arrays of a pattern without a mirror", part); return; }
    CHECK((int64_t)h.slices.size() == ns + 1, "%s: %zu slice records for %lld slices", part, h.slices.size(), (long long)ns);
    int64_t base = 0, obase = 0;
    for (int64_t s = 0; s < ns; ++s) {
        const MirrorSlice &m = h.slices[s];
        const int64_t r0 = 64 * s, r1 = std::min(r0 + 64, n);
        int64_t w = 0;
        bool uni = rowsig && r1 - r0 == 64;
        for (int64_t r = r0; r < r1; ++r) { w = std::max(w, A.rp[r + 1] - A.rp[r]); uni = uni && rowsig[r] == rowsig[r0]; }
        CHECK(m.base == base && m.width == w && m.pad[0] == 0 && m.pad[1] == 0, "%s: slice %lld: base / width", part, (long long)s);
        CHECK(uni ? m.sig == rowsig[r0] && m.obase == -1 : m.sig == MIRROR_MIXED && m.obase == obase, "%s: slice %lld: uniform = %d", part, (long long)s, (int)uni);
        if (!uni) {
            CHECK(obase + 64 * w <= (int64_t)h.offs.size(), "%s: slice %lld: offsets past the array", part, (long long)s);
            for (int64_t k = 0; k < w; ++k)
                for (int64_t l = 0; l < 64; ++l) {
                    const int64_t r = r0 + l;
                    const bool on = r < r1 && k < A.rp[r + 1] - A.rp[r];
                    CHECK(h.offs[obase + 64 * k + l] == (on ? A.ci[A.rp[r] + k] - (int32_t)r : MIRROR_NONE), "%s: slice %lld entry %lld lane %lld", part, (long long)s, (long long)k, (long long)l);
                }
            obase += 64 * w;
        }
        base += 64 * w;
    }
    const MirrorSlice &t = h.slices[ns];
    CHECK(t.base == base && t.obase == -1 && t.sig == MIRROR_MIXED && t.width == 0 && t.pad[0] == 0 && t.pad[1] == 0 && h.entries == base, "%s: terminator record", part);
    CHECK(obase ? (int64_t)h.offs.size() == obase : h.offs.size() == 1 && h.offs[0] == 0, "%s: offsets: %zu entries, the mixed slices hold %lld", part, h.offs.size(), (long long)obase);
}

static void check_diag(const char *part, const Csr &A, const std::vector<int64_t> &pos)
{
    CHECK((int64_t)pos.size() == A.n(), "%s: diagonal positions: size", part);
    for (int64_t r = 0; r < A.n(); ++r) {
        bool stored = false;
        for (int64_t k = A.rp[r]; k < A.rp[r + 1]; ++k) stored = stored || A.ci[k] == r;
        CHECK(pos[r] == -1 ? !stored : pos[r] >= A.rp[r] && pos[r] < A.rp[r + 1] && A.ci[pos[r]] == r, "%s: diagonal position of row %lld", part, (long long)r);
    }
}

// every plan of one pattern, as the upload tails of tb_spmv.hip call the planners (the mirror gets the signatures only where the pattern compresses)
static void spmv_pattern(const char *part, const Csr &A, const Expect &e, bool block3_only = false)
{
    const PatternView v = A.view();
    std::vector<int32_t> bcol;
    const bool b3 = block3_columns(v, bcol);
    scalar(part, "b3", b3); digest(part, "bcol", bcol);
    check_block3(part, A, b3, bcol, e.b3);
    if (block3_only) return;
    std::vector<uint32_t> rec;
    const bool streams = row_runs(v, SPMV_CAP, rec);
    scalar(part, "streams", streams); scalar(part, "n_runs", (long long)rec.size() / 4); digest(part, "runrec", rec);
    check_runs(part, A, streams, rec, e.streams);
    const int64_t budget = std::max<int64_t>(nnz_of(v) / 4, 64);
    SigHost sg;
    const bool compresses = row_signatures(v, budget, sg);
    scalar(part, "compresses", compresses); scalar(part, "n_sig", sg.n_sig); digest(part, "rowsig", sg.rowsig); digest(part, "sigoff", sg.tab);
    check_sig(part, A, budget, compresses, sg, e.compresses);
    MirrorHost mh;
    const uint32_t *rowsig = compresses ? sg.rowsig.data() : nullptr;
    const bool mirror = mirror_slices(v, rowsig, mh);
    scalar(part, "mirror", mirror); scalar(part, "mir_entries", mh.entries); digest(part, "slices", mh.slices); digest(part, "mir_off", mh.offs);
    check_mirror(part, A, rowsig, mirror, mh, e.mirror);
    const std::vector<int64_t> pos = diagonal_positions(v);
    digest(part, "diagpos", pos);
    check_diag(part, A, pos);
}

static bool case_spmv(const std::string &dir)
{
    Mesh M;
    if (!load(dir, "box", TB_HEX8, 1, M)) return false;
    const Csr box = Csr::of(M);
    spmv_pattern("box", box, {NO, YES, NO, YES}); // 13·11·9 = 1287 rows: a ragged last slice; so small a box is mostly boundary layers of the first-visit numbering: the budget refuses
    if (box.n() % 64 == 0) { fprintf(stderr, "spmv: the box is meant to end in a ragged slice\n"); ++g_failed; }
    { // the same with one row emptied
        Csr A;
        for (int64_t r = 0; r < box.n(); ++r) A.row(r == 70 ? std::vector<int32_t>() : std::vector<int32_t>(box.ci.begin() + box.rp[r], box.ci.begin() + box.rp[r + 1]));
        spmv_pattern("empty_row", A, {NO, YES, NO, YES});
    }
    if (!load(dir, "shuffled_box", TB_HEX8, 1, M)) return false;
    spmv_pattern("shuffled_box", Csr::of(M), {NO, YES, NO, YES}); // every row its own signature: the budget refuses
    if (!load(dir, "thin_wall", TB_HEX8, 1, M)) return false;
    spmv_pattern("thin_wall", Csr::of(M), {NO, YES, ANY, YES});
    { // the 27-point stencil on 12 × 10 × 8 nodes numbered lexicographically, row 70 emptied: compresses to a handful of signatures (28: 27 positions in the box and the empty row)
        Csr A;
        for (int32_t z = 0; z < 8; ++z) for (int32_t y = 0; y < 10; ++y) for (int32_t x = 0; x < 12; ++x) {
            std::vector<int32_t> cols;
            for (int32_t c = std::max(z - 1, 0); c <= std::min(z + 1, 7); ++c) for (int32_t b = std::max(y - 1, 0); b <= std::min(y + 1, 9); ++b) for (int32_t a = std::max(x - 1, 0); a <= std::min(x + 1, 11); ++a) cols.push_back(a + 12 * (b + 10 * c));
            A.row(A.n() == 70 ? std::vector<int32_t>() : cols);
        }
        spmv_pattern("lexicographic_box", A, {NO, YES, YES, YES});
    }
    if (!load(dir, "q2_scalar", TB_HEX27, 1, M)) return false;
    spmv_pattern("q2_scalar", Csr::of(M), {NO, YES, ANY, YES});
    if (!load(dir, "q2_box", TB_HEX27, 3, M)) return false;
    spmv_pattern("long_rows", Csr::of(M), {YES, YES, ANY, NO}); // rows of 375 entries
    if (!load(dir, "box", TB_HEX8, 3, M)) return false;
    const Csr box3 = Csr::of(M);
    spmv_pattern("box3", box3, {YES, YES, ANY, YES});
    { // one row's column triple broken: the last column of the first block of row 4 names the next node
        Csr A = box3;
        A.ci[A.rp[4] + 2] += 3;
        spmv_pattern("box3_broken_triple", A, {NO, ANY, ANY, ANY}, true);
    }
    { // a node row that does not start at a multiple of nine: three entries in front of row 0's, six behind the last row's
        Csr A = box3;
        A.ci.insert(A.ci.begin(), 3, 0);
        A.ci.insert(A.ci.end(), 6, 0);
        for (int64_t &k : A.rp) k += 3;
        A.rp.back() += 6;
        spmv_pattern("box3_k0_not_9", A, {NO, ANY, ANY, ANY}, true);
    }
    { // 130 rows of a tridiagonal matrix: three signatures; slice 0 mixed, slice 1 of one signature, slice 2 ragged
        Csr A;
        for (int32_t r = 0; r < 130; ++r) A.row(span(std::max(r - 1, 0), (r > 0) + 1 + (r < 129)));
        spmv_pattern("tridiagonal", A, {NO, YES, YES, YES});
    }
    { // a 256-entry row among diagonal rows: no mirror
        Csr A;
        for (int32_t r = 0; r < 3000; ++r) A.row(r == 10 ? span(0, 256) : span(r, 1));
        spmv_pattern("row_of_256", A, {NO, YES, YES, NO});
    }
    for (int extra = 0; extra < 2; ++extra) { // rows of exactly cap − 2 entries stream, a run each; one entry more and the pattern falls back
        Csr A;
        for (int32_t r = 0; r < 2100; ++r) A.row(r < 3 ? span(r, SPMV_CAP - 2 + (r == 1 ? extra : 0)) : span(r, 1));
        spmv_pattern(extra ? "row_of_cap_minus_1" : "rows_of_cap_minus_2", A, {NO, extra ? NO : YES, extra ? NO : YES, NO});
    }
    { // 130000 rows, every hundredth with a diagonal entry: the 60000-row limit cuts the runs
        Csr A;
        for (int32_t r = 0; r < 130000; ++r) A.row(r % 100 == 0 ? span(r, 1) : std::vector<int32_t>());
        spmv_pattern("mostly_empty", A, {NO, YES, YES, YES});
    }
    spmv_pattern("zero_rows", Csr(), {NO, YES, NO, YES});
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <mesh directory> [case]\n", argv[0]); return 2; }
    const std::string dir = argv[1], only = argc > 2 ? argv[2] : "";
    struct Case { const char *name, *mesh; int kind, ncomp, nregions; bool mat, vec; };
    const Case cases[] = {
        {"box", "box", TB_HEX8, 1, 1, true, true},            // 12×10×8
        {"box_two_blocks", "box", TB_HEX8, 1, 2, false, false}, // the starting-tile reduction
        {"shuffled_box", "shuffled_box", TB_HEX8, 1, 2, true, true},
        {"ring", "ring", TB_HEX8, 1, 2, true, true},
        {"ideal_lv", "ideal_lv", TB_HEX8, 1, 2, true, true},
        {"thin_wall", "thin_wall", TB_HEX8, 1, 2, true, true}, // ≥ 4096 cells: the bisection branches
        {"tets", "tets", TB_TET4, 1, 2, true, true},           // per_bucket ≥ 2, 5×5×5 tiles; the vector plan refuses
        {"long_rows", "q2_box", TB_HEX27, 3, 1, true, true},   // rows of more than 255 entries: the shrink loop runs out of tiles; fused and vector plans refuse
    };
    Mesh M;
    for (const Case &c : cases) {
        if (!only.empty() && only != c.name) continue;
        g_case = c.name;
        if (!load(dir, c.mesh, c.kind, c.ncomp, M)) return 2;
        if (c.mat) case_mat(M, run_mat(M));
        case_fused(M, run_fused(M, c.nregions), c.nregions);
        if (c.vec) { case_vec(M, false); case_vec(M, true); }
        if (!strcmp(c.name, "thin_wall") || !strcmp(c.name, "box")) { // refits: the fits start from the plan and the state (bisection leaves on the thin wall) of the fit before
            Fit fused2, mat3;
            run_refit(M, fused2, mat3);
            case_fused(M, fused2, 3, "refit_fused");
            case_mat(M, mat3, "refit_mat");
        }
        if (c.kind == TB_HEX27) { // the same with TB_PATCH_TILE=1,1,1: a fixed shape is accepted up to 160 KiB, column positions are 16-bit
            Options o;
            o.tile[0] = o.tile[1] = o.tile[2] = 1;
            o.tile_set = o.fixed = true;
            case_mat(M, run_mat(M, o), "mat_tile_1", true);
        }
    }
    if (only.empty() || only == "colouring") { // colour plans and slot lists on the box, the slot table on a scalar Q2 field
        g_case = "colouring";
        if (!load(dir, "box", TB_HEX8, 1, M)) return 2;
        case_colors(M, "all", nullptr);
        std::vector<int32_t> third;
        for (int32_t c = 0; c < M.n_cells; c += 3) third.push_back(c);
        case_colors(M, "every_third", &third);
        std::vector<int64_t> ptr;
        std::vector<int32_t> src, ell_t;
        run_slots(M, ptr, src);
        digest("slots", "ptr", ptr); digest("slots", "src", src);
        if (!load(dir, "q2_scalar", TB_HEX27, 1, M)) return 2;
        SlotTable t;
        run_slot_table(M, t, ell_t);
        scalar("slots", "ell_w", t.w);
        digest("slots", "ell", t.ell); digest("slots", "h_done", t.h_done); digest("slots", "ell_t", ell_t);
    }
    if (only.empty() || only == "gather_nodes") { // three-component fields: the host planning of the element strategy's tangent gather
        g_case = "gather_nodes";
        struct Field { const char *part, *mesh; int kind; bool applies; };
        const Field fields[] = {{"q2_box", "q2_box", TB_HEX27, true},     // 3×3×2, Q2
                                {"q1_box", "q2_scalar", TB_HEX8, true},   // 4×3×3, Q1
                                {"prism_q1", "prism", TB_HEX8, false},    // a vertex in ten cells
                                {"prism_q2", "prism", TB_HEX27, false}};
        for (const Field &fd : fields) {
            if (!load(dir, fd.mesh, fd.kind, 3, M)) return 2;
            case_gather(M, fd.part, fd.applies);
        }
    }
    if (only.empty() || only == "spmv") {
        g_case = "spmv";
        if (!case_spmv(dir)) return 2;
    }
    if (only.empty() || only == "refusals") { // return codes only
        g_case = "refusals";
        if (!load(dir, "box", TB_HEX8, 1, M)) return 2;
        Mesh P = M; // one coupling removed from the pattern: the last entry of row 0
        P.colidx.erase(P.colidx.begin() + P.rowptr[1] - 1);
        for (int64_t r = 1; r <= P.ndofs; ++r) --P.rowptr[r];
        scalar("coupling_removed", "fused_rc", run_fused(P, 1).rc);
        scalar("coupling_removed", "mat_rc", run_mat(P).rc);
        Mesh D = M; // dofs and vertices not one-to-one: in cell 0 alone, vertex 6 carries the dof of a far vertex
        D.cd[6] = M.cd.back();
        scalar("not_one_to_one", "fused_rc", run_fused(D, 1).rc);
        VecHost v;
        scalar("not_one_to_one", "vec_rc", run_vec(D, true, v));
    }
    if (g_failed) fprintf(stderr, "%d invariant(s) failed\n", g_failed);
    return g_failed ? 1 : 0;
}

// Stand-alone driver of the record classification (plan::classify_records, thunderbolt.jl_amd/csrc/tb_planners.cpp): no GPU, no HIP.  Links tb_planners.cpp
// and tb_hostgen.cpp only.
//   canonical_planner_driver <mesh directory> <name>...
// reads the meshes tests/test_canonical_planner_cpu.py wrote (<name>.xyz: float64 × 3 per node, <name>.conn: int32 per cell vertex, <name>.dofs: int32
// per cell dof — the DofHandler's table, so that renumbered fields arrive as they are), fits the fused plan for two accumulator blocks, classifies its
// patches and checks
//   * the classification against a brute-force recomputation of every position from the CSR pattern (no signature table, no row descriptors),
//   * that the two class counts add up to the patch count and `order` is a permutation,
//   * that the order is stable inside each class, and that record slot s holds exactly the record of patch order[s].
// Prints "<name> <patches> <general> <canonical>" per mesh.  Exit status 0: every check holds.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tbhip.h"
#include "tb_planners.hpp"

namespace tb { void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); } }
using namespace tb;
using namespace tb::plan;

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

static int fail(const std::string &name, const char *fmt, ...)
{
    fprintf(stderr, "%s: ", name.c_str());
    va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap);
    fputc('\n', stderr);
    return 1;
}

// vertex signs of Ferrite's hexahedron, written out here on purpose: the check shares no table with the planner
static const int SGN[8][3] = {{-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, {-1, -1, 1}, {1, -1, 1}, {1, 1, 1}, {-1, 1, 1}};

static Options g_options; // --tile x,y,z: what TB_PATCH_TILE does to the library's options (a fixed tile shape)

static int run(const std::string &dir, const std::string &name)
{
    std::vector<double> xyz;
    std::vector<int32_t> conn, cd;
    if (!read_file(dir + "/" + name + ".xyz", xyz) || !read_file(dir + "/" + name + ".conn", conn) || !read_file(dir + "/" + name + ".dofs", cd)) return 2;
    const int64_t n_nodes = (int64_t)xyz.size() / 3, n_cells = (int64_t)conn.size() / 8;
    if ((int64_t)cd.size() != n_cells * 8) return fail(name, "dof table of %zu entries for %lld cells", cd.size(), (long long)n_cells);
    const int64_t ndofs = (int64_t)*std::max_element(cd.begin(), cd.end()) + 1;
    std::vector<int64_t> rowptr(ndofs + 1);
    const int64_t nnz = tb_host_build_pattern(n_cells, 8, cd.data(), ndofs, rowptr.data(), nullptr);
    if (nnz <= 0) return fail(name, "pattern");
    std::vector<int32_t> colidx(nnz);
    if (tb_host_build_pattern(n_cells, 8, cd.data(), ndofs, rowptr.data(), colidx.data()) != nnz) return fail(name, "pattern");
    const MeshView mv{n_nodes, n_cells, ndofs, 8, 8, 1, xyz.data(), conn.data(), cd.data()};
    const PatternView pv{ndofs, rowptr.data(), colidx.data(), 0};

    FitState st;
    PatchHost pp;
    FusedHost fh;
    bool replaced;
    const Outcome r = fit_fused(mv, pv, g_options, 2, st, pp, replaced, fh);
    if (!r.ok() || fh.hdr.empty()) return fail(name, "fused plan refused (%d)", r.code);
    const int64_t np = pp.n_patches;
    const RecordClasses cls = classify_records(np, fh.hdr.data(), fh.ln.data(), fh.elem_sig.data(), fh.row_desc.data(), fh.sigtab.data());

    // counts and permutation
    if (cls.n_general + cls.n_canonical != np || (int64_t)cls.order.size() != np) return fail(name, "%lld general + %lld canonical of %lld patches", (long long)cls.n_general, (long long)cls.n_canonical, (long long)np);
    std::vector<int8_t> got(np, -1);
    for (int64_t s = 0; s < np; ++s) {
        const int64_t q = cls.order[s];
        if (q < 0 || q >= np || got[q] >= 0) return fail(name, "order is no permutation at slot %lld", (long long)s);
        got[q] = s >= cls.n_general;
    }
    // stable inside each class
    for (int64_t s = 1; s < np; ++s)
        if (s != cls.n_general && cls.order[s] <= cls.order[s - 1]) return fail(name, "order of slot %lld breaks the plan order of its class", (long long)s);

    // brute force from the CSR pattern
    for (int64_t q = 0; q < np; ++q) {
        const int64_t e0 = pp.h_elem_ptr[q], e1 = pp.h_elem_ptr[q + 1];
        bool canon = e1 - e0 <= 256;
        for (int64_t e = e0; e < e1 && canon; ++e) {
            const int32_t *d = &cd[(size_t)pp.h_elem_cell[e] * 8];
            for (int i = 0; i < 8 && canon; ++i) {
                if (pp.h_elem_lrow[e * 8 + i] == 0xFFFF) continue; // not a row of this patch
                const int64_t k0 = rowptr[d[i]], k1 = rowptr[d[i] + 1];
                if (k1 - k0 != 27) { canon = false; break; }
                for (int j = 0; j < 8 && canon; ++j) {
                    int64_t pos = -1;
                    for (int64_t k = k0; k < k1; ++k) if (colidx[k] == d[j]) { pos = k - k0; break; }
                    const int want = 13 + (SGN[j][0] - SGN[i][0]) / 2 + 3 * ((SGN[j][1] - SGN[i][1]) / 2) + 9 * ((SGN[j][2] - SGN[i][2]) / 2);
                    canon = pos == want;
                }
            }
        }
        if ((int)canon != (int)got[q]) return fail(name, "patch %lld: planner says %s, the pattern says %s", (long long)q, got[q] ? "canonical" : "general", canon ? "canonical" : "general");
    }

    // records: slot s of the ordered array is the record of patch order[s] in the plain array
    Records plain = record_layout(pp, fh.max_nodes), ordered = plain;
    if (plain.stride > 0) {
        pack_records(plain, np, fh.hdr.data(), fh.ln.data(), fh.elem_sig.data(), fh.row_desc.data(), fh.pcoord.data());
        pack_records(ordered, np, fh.hdr.data(), fh.ln.data(), fh.elem_sig.data(), fh.row_desc.data(), fh.pcoord.data(), cls.order.data());
        if (ordered.bytes.size() != plain.bytes.size()) return fail(name, "record arrays differ in size");
        for (int64_t s = 0; s < np; ++s)
            if (memcmp(&ordered.bytes[(size_t)s * plain.stride], &plain.bytes[(size_t)cls.order[s] * plain.stride], (size_t)plain.stride) != 0)
                return fail(name, "record slot %lld is not the record of patch %lld", (long long)s, (long long)cls.order[s]);
    } else if (cls.n_canonical > 0)
        return fail(name, "canonical patches without the record form");
    printf("%s %lld %lld %lld\n", name.c_str(), (long long)np, (long long)cls.n_general, (long long)cls.n_canonical);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <mesh directory> [--tile x,y,z] <name>...\n", argv[0]); return 2; }
    int first = 2;
    if (!strcmp(argv[2], "--tile")) {
        if (argc < 5 || sscanf(argv[3], "%d,%d,%d", &g_options.tile[0], &g_options.tile[1], &g_options.tile[2]) != 3) { fprintf(stderr, "bad --tile\n"); return 2; }
        g_options.tile_set = g_options.fixed = true;
        first = 4;
    }
    for (int k = first; k < argc; ++k)
        if (const int rc = run(argv[1], argv[k])) return rc;
    return 0;
}

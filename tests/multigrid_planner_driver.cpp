// multigrid_planner_driver.cpp — the multigrid planners (thunderbolt.jl_amd/csrc/tb_mg_planners.cpp) without a GPU.  A stand-alone program linked
// with the planner file and the host generators: reads one case (two nested levels as raw arrays written by tests/test_multigrid_cpu.py), builds the
// patterns, P, Pᵀ and the Galerkin plan, checks the plan's invariants itself (exit status 1 with a message otherwise), applies the plan on the host to
// the seeded fine values and prints A_c, one value per line.
//   usage: multigrid_planner_driver <dir> <case>
//   files: <case>.meta (text: n_fine_nodes n_fine_cells n_fine_dofs n_coarse_nodes n_coarse_cells n_coarse_dofs ncomp has_prescribed)
//          <case>.fconn .fdofs .cconn .cdofs .pidx (int32)  .pptr (int64)  .presc (uint8, when has_prescribed)  .A (float64, fine CSR values)
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tbhip.h"
#include "tb_mg_planners.hpp"

namespace tb { void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); } }
using namespace tb::mgplan;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "invariant failed: " __VA_ARGS__); fputc('\n', stderr); return 1; } } while (0)

template <class T>
static std::vector<T> read_raw(const std::string &path, size_t count)
{
    std::vector<T> v(count);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f || fread(v.data(), sizeof(T), count, f) != count) { fprintf(stderr, "cannot read %zu entries of %s\n", count, path.c_str()); exit(2); }
    fclose(f);
    return v;
}

struct Level {
    int64_t n_nodes, n_cells, ndofs;
    int ncomp;
    std::vector<int32_t> conn, cd, colidx;
    std::vector<int64_t> rowptr;
    void pattern()
    {
        rowptr.resize((size_t)ndofs + 1);
        const int64_t nnz = tb_host_build_pattern(n_cells, 8 * ncomp, cd.data(), ndofs, rowptr.data(), nullptr);
        if (nnz < 0) exit(2);
        colidx.resize((size_t)nnz);
        tb_host_build_pattern(n_cells, 8 * ncomp, cd.data(), ndofs, rowptr.data(), colidx.data());
    }
    LevelView view() const { return LevelView{n_nodes, n_cells, ndofs, 8, ncomp, conn.data(), cd.data(), rowptr.data(), colidx.data()}; }
};

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <dir> <case>\n", argv[0]); return 2; }
    const std::string base = std::string(argv[1]) + "/" + argv[2];
    long long m[8];
    {
        FILE *f = fopen((base + ".meta").c_str(), "r");
        if (!f) { fprintf(stderr, "no %s.meta\n", base.c_str()); return 2; }
        for (int k = 0; k < 8; ++k) if (fscanf(f, "%lld", &m[k]) != 1) { fprintf(stderr, "short meta file\n"); return 2; }
        fclose(f);
    }
    Level F{m[0], m[1], m[2], (int)m[6], {}, {}, {}, {}}, Cl{m[3], m[4], m[5], (int)m[6], {}, {}, {}, {}};
    const int nc = (int)m[6];
    F.conn = read_raw<int32_t>(base + ".fconn", (size_t)F.n_cells * 8);
    F.cd = read_raw<int32_t>(base + ".fdofs", (size_t)F.n_cells * 8 * nc);
    Cl.conn = read_raw<int32_t>(base + ".cconn", (size_t)Cl.n_cells * 8);
    Cl.cd = read_raw<int32_t>(base + ".cdofs", (size_t)Cl.n_cells * 8 * nc);
    const std::vector<int64_t> pptr = read_raw<int64_t>(base + ".pptr", (size_t)F.n_nodes + 1);
    const std::vector<int32_t> pidx = read_raw<int32_t>(base + ".pidx", (size_t)pptr.back());
    std::vector<uint8_t> presc;
    if (m[7]) presc = read_raw<uint8_t>(base + ".presc", (size_t)F.ndofs);
    const uint8_t *flags = presc.empty() ? nullptr : presc.data();
    F.pattern();
    Cl.pattern();
    const int64_t fnnz = F.rowptr.back(), cnnz = Cl.rowptr.back();
    const std::vector<double> Af = read_raw<double>(base + ".A", (size_t)fnnz);

    Transfer t;
    Galerkin g;
    if (build_transfer(F.view(), Cl.view(), pptr.data(), pidx.data(), flags, t)) return 1;
    if (build_galerkin(F.view(), Cl.view(), t, flags, g)) return 1;

    // ---- invariants
    CHECK((int64_t)t.p_ptr.size() == F.ndofs + 1 && (int64_t)t.r_ptr.size() == Cl.ndofs + 1, "transfer pointer sizes");
    CHECK(t.p_col.size() == t.r_col.size() && (int64_t)t.p_col.size() == t.p_ptr.back() && t.r_ptr.back() == t.p_ptr.back(), "P and its transpose hold different counts");
    for (int64_t i = 0; i < F.ndofs; ++i) {
        CHECK(t.p_ptr[i + 1] >= t.p_ptr[i] && t.p_ptr[i + 1] - t.p_ptr[i] <= 8, "row %lld of P", (long long)i);
        if (flags && flags[i]) CHECK(t.p_ptr[i + 1] == t.p_ptr[i], "prescribed fine dof %lld has a row in P", (long long)i);
        for (int64_t q = t.p_ptr[i]; q < t.p_ptr[i + 1]; ++q) {
            CHECK(t.p_col[q] >= 0 && t.p_col[q] < Cl.ndofs, "column of P out of range");
            CHECK(t.p_exp[q] <= 3, "exponent of P above 3");
            CHECK(!t.coarse_prescribed[t.p_col[q]], "P has a column at a prescribed coarse dof");
        }
    }
    for (int64_t I = 0; I < Cl.ndofs; ++I)
        for (int64_t q = t.r_ptr[I]; q < t.r_ptr[I + 1]; ++q) {
            CHECK(t.r_col[q] >= 0 && t.r_col[q] < F.ndofs, "column of the restriction out of range");
            CHECK(q == t.r_ptr[I] || t.r_col[q] > t.r_col[q - 1], "row %lld of the restriction is not ascending", (long long)I);
        }
    CHECK((int64_t)g.ptr.size() == cnnz + 1 && g.ptr[0] == 0 && g.ptr[cnnz] == (int64_t)g.terms.size(), "Galerkin pointer");
    CHECK((int64_t)g.terms.size() == g.expected_terms, "term count %zu, expected %lld", g.terms.size(), (long long)g.expected_terms);
    {   // the expected count once more, straight from the parent lists: Σ |free parents(i)|·|free parents(j)| over the kept fine non-zeros
        int64_t want = 0;
        for (int64_t i = 0; i < F.ndofs; ++i)
            for (int64_t k = F.rowptr[i]; k < F.rowptr[i + 1]; ++k) want += (t.p_ptr[i + 1] - t.p_ptr[i]) * (t.p_ptr[F.colidx[k] + 1] - t.p_ptr[F.colidx[k]]);
        CHECK(want == (int64_t)g.terms.size(), "term count %zu, the parent lists give %lld", g.terms.size(), (long long)want);
    }
    for (int64_t k = 0; k < cnnz; ++k) CHECK(g.ptr[k + 1] >= g.ptr[k], "Galerkin pointer not monotone");
    for (uint32_t w : g.terms) {
        CHECK((int64_t)(w & ((1u << TERM_BITS) - 1u)) < fnnz, "fine index of a term out of range");
        CHECK((w >> TERM_BITS) <= 6, "exponent of a term above 6");
    }
    for (int64_t I = 0; I < Cl.ndofs; ++I)
        for (int64_t k = Cl.rowptr[I]; k < Cl.rowptr[I + 1]; ++k) {
            const bool empty = t.coarse_prescribed[I] || t.coarse_prescribed[Cl.colidx[k]];
            CHECK(empty ? g.ptr[k + 1] == g.ptr[k] : g.ptr[k + 1] > g.ptr[k], "coarse non-zero (%lld, %d): %lld terms", (long long)I, Cl.colidx[k], (long long)(g.ptr[k + 1] - g.ptr[k]));
        }
    CHECK((int64_t)g.diag_pos.size() == Cl.ndofs, "diagonal positions");
    for (int64_t I = 0; I < Cl.ndofs; ++I) CHECK(g.diag_pos[I] >= Cl.rowptr[I] && g.diag_pos[I] < Cl.rowptr[I + 1] && Cl.colidx[g.diag_pos[I]] == I, "diagonal position of row %lld", (long long)I);

    std::vector<double> Ac((size_t)cnnz);
    apply_galerkin_host(g, t, Af.data(), cnnz, Ac.data());
    printf("terms %zu fine_nnz %lld coarse_nnz %lld\n", g.terms.size(), (long long)fnnz, (long long)cnnz);
    for (double v : Ac) printf("%.17g\n", v);
    return 0;
}

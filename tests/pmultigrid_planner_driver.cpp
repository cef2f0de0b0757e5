// pmultigrid_planner_driver.cpp — the p-level planners (thunderbolt.jl_amd/csrc/tb_mg_planners.cpp) without a GPU.  A stand-alone program linked with
// the planner file and the host generators: reads one case (a second-order and a first-order field on the same cells, as raw arrays written by
// tests/test_pmultigrid_cpu.py), builds the patterns, P, Pᵀ and the Galerkin plan — the blocked one where both patterns are CSRs of 3 × 3 blocks and P
// moves node triples, the per-dof one otherwise or when asked —, checks the invariants itself (exit status 1 with a message otherwise), applies the
// plan on the host to the seeded fine values and prints P and A_c.
//   usage: pmultigrid_planner_driver <dir> <case> [dof]
//   files: <case>.meta (text: n_nodes n_cells n_fine_dofs n_coarse_dofs ncomp has_prescribed)
//          <case>.conn .fdofs .cdofs (int32)  .presc (uint8, when has_prescribed)  .A (float64, fine CSR values)
//   output: "blocked <0|1> terms <n> dof_terms <n> fine_nnz <n> coarse_nnz <n> p_entries <n>", then p_entries lines "row col exponent", then A_c
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    int ncomp, nbasis;
    const std::vector<int32_t> *conn;
    std::vector<int32_t> cd, colidx;
    std::vector<int64_t> rowptr;
    void pattern()
    {
        rowptr.resize((size_t)ndofs + 1);
        const int64_t nnz = tb_host_build_pattern(n_cells, nbasis * ncomp, cd.data(), ndofs, rowptr.data(), nullptr);
        if (nnz < 0) exit(2);
        colidx.resize((size_t)nnz);
        tb_host_build_pattern(n_cells, nbasis * ncomp, cd.data(), ndofs, rowptr.data(), colidx.data());
    }
    LevelView view() const
    {
        LevelView v{n_nodes, n_cells, ndofs, 8, ncomp, conn->data(), cd.data(), rowptr.data(), colidx.data()};
        v.nbasis = nbasis;
        return v;
    }
};

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s <dir> <case> [dof]\n", argv[0]); return 2; }
    const bool force_dof = argc == 4 && !strcmp(argv[3], "dof");
    const std::string base = std::string(argv[1]) + "/" + argv[2];
    long long m[6];
    {
        FILE *f = fopen((base + ".meta").c_str(), "r");
        if (!f) { fprintf(stderr, "no %s.meta\n", base.c_str()); return 2; }
        for (int k = 0; k < 6; ++k) if (fscanf(f, "%lld", &m[k]) != 1) { fprintf(stderr, "short meta file\n"); return 2; }
        fclose(f);
    }
    const int nc = (int)m[4];
    const std::vector<int32_t> conn = read_raw<int32_t>(base + ".conn", (size_t)m[1] * 8);
    Level F{m[0], m[1], m[2], nc, 27, &conn, {}, {}, {}}, Cl{m[0], m[1], m[3], nc, 8, &conn, {}, {}, {}};
    F.cd = read_raw<int32_t>(base + ".fdofs", (size_t)F.n_cells * 27 * nc);
    Cl.cd = read_raw<int32_t>(base + ".cdofs", (size_t)Cl.n_cells * 8 * nc);
    std::vector<uint8_t> presc;
    if (m[5]) presc = read_raw<uint8_t>(base + ".presc", (size_t)F.ndofs);
    const uint8_t *flags = presc.empty() ? nullptr : presc.data();
    F.pattern();
    Cl.pattern();
    const int64_t fnnz = F.rowptr.back(), cnnz = Cl.rowptr.back();
    const std::vector<double> Af = read_raw<double>(base + ".A", (size_t)fnnz);
    const LevelView fv = F.view(), cv = Cl.view();

    Transfer t;
    Galerkin g, gb;
    if (build_p_transfer(fv, cv, flags, t)) return 1;
    if (build_galerkin(fv, cv, t, flags, g)) return 1;
    const bool blocked = !force_dof && block_csr(fv) && block_csr(cv) && node_blocked(t);
    if (blocked && build_galerkin_blocked(fv, cv, t, gb)) return 1;

    // ---- invariants of the transfer
    CHECK((int64_t)t.p_ptr.size() == F.ndofs + 1 && (int64_t)t.r_ptr.size() == Cl.ndofs + 1, "transfer pointer sizes");
    CHECK(t.p_col.size() == t.r_col.size() && (int64_t)t.p_col.size() == t.p_ptr.back() && t.r_ptr.back() == t.p_ptr.back(), "P and its transpose hold different counts");
    for (int64_t i = 0; i < F.ndofs; ++i) {
        CHECK(t.p_ptr[i + 1] >= t.p_ptr[i] && t.p_ptr[i + 1] - t.p_ptr[i] <= 8, "row %lld of P", (long long)i);
        if (flags && flags[i]) CHECK(t.p_ptr[i + 1] == t.p_ptr[i], "prescribed fine dof %lld has a row in P", (long long)i);
        for (int64_t q = t.p_ptr[i]; q < t.p_ptr[i + 1]; ++q) {
            CHECK(t.p_col[q] >= 0 && t.p_col[q] < Cl.ndofs, "column of P out of range");
            CHECK(q == t.p_ptr[i] || t.p_col[q] > t.p_col[q - 1], "row %lld of P is not ascending", (long long)i);
            CHECK(t.p_exp[q] <= 3, "exponent of P above 3");
            CHECK(!t.coarse_prescribed[t.p_col[q]], "P has a column at a prescribed coarse dof");
        }
    }
    for (int64_t I = 0; I < Cl.ndofs; ++I) {
        CHECK(t.r_ptr[I + 1] - t.r_ptr[I] <= 27, "row %lld of the restriction gathers more than 27 fine dofs", (long long)I);
        for (int64_t q = t.r_ptr[I]; q < t.r_ptr[I + 1]; ++q) {
            CHECK(t.r_col[q] >= 0 && t.r_col[q] < F.ndofs, "column of the restriction out of range");
            CHECK(q == t.r_ptr[I] || t.r_col[q] > t.r_col[q - 1], "row %lld of the restriction is not ascending", (long long)I);
        }
    }
    // ---- invariants of the per-dof plan
    CHECK((int64_t)g.ptr.size() == cnnz + 1 && g.ptr[0] == 0 && g.ptr[cnnz] == (int64_t)g.terms.size(), "Galerkin pointer");
    CHECK((int64_t)g.terms.size() == g.expected_terms, "term count %zu, expected %lld", g.terms.size(), (long long)g.expected_terms);
    {
        int64_t want = 0;
        for (int64_t i = 0; i < F.ndofs; ++i)
            for (int64_t k = F.rowptr[i]; k < F.rowptr[i + 1]; ++k) want += (t.p_ptr[i + 1] - t.p_ptr[i]) * (t.p_ptr[F.colidx[k] + 1] - t.p_ptr[F.colidx[k]]);
        CHECK(want == (int64_t)g.terms.size(), "term count %zu, the parent lists give %lld", g.terms.size(), (long long)want);
    }
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
    // ---- invariants of the blocked plan
    if (blocked) {
        const int64_t fb = fnnz / 9, cb = cnnz / 9;
        CHECK(gb.blocked && (int64_t)gb.ptr.size() == cb + 1 && gb.ptr[0] == 0 && gb.ptr[cb] == (int64_t)gb.terms.size(), "blocked Galerkin pointer");
        CHECK((int64_t)gb.terms.size() == gb.expected_terms, "blocked term count %zu, expected %lld", gb.terms.size(), (long long)gb.expected_terms);
        CHECK((int64_t)gb.fine_brow.size() == fb && (int64_t)gb.coarse_brow.size() == cb, "block row tables");
        for (int64_t B = 0; B < fb; ++B) CHECK(gb.fine_brow[B] >= 0 && F.rowptr[3 * gb.fine_brow[B]] / 9 <= B && B < F.rowptr[3 * gb.fine_brow[B] + 3] / 9, "block row of fine block %lld", (long long)B);
        for (int64_t B = 0; B < cb; ++B) CHECK(gb.coarse_brow[B] >= 0 && Cl.rowptr[3 * gb.coarse_brow[B]] / 9 <= B && B < Cl.rowptr[3 * gb.coarse_brow[B] + 3] / 9, "block row of coarse block %lld", (long long)B);
        for (uint32_t w : gb.terms) {
            CHECK((int64_t)(w & ((1u << TERM_BITS) - 1u)) < fb, "fine block index of a term out of range");
            CHECK((w >> TERM_BITS) <= 6, "exponent of a blocked term above 6");
        }
        CHECK(gb.diag_pos == g.diag_pos, "diagonal positions of the blocked plan");
        if (!flags) CHECK(9 * gb.terms.size() == g.terms.size(), "blocked plan: %zu terms, per-dof plan %zu (not nine times as many)", gb.terms.size(), g.terms.size());
    }

    std::vector<double> Ac((size_t)cnnz);
    if (blocked) apply_galerkin_blocked_host(gb, t, fv, cv, flags, Af.data(), Ac.data());
    else apply_galerkin_host(g, t, Af.data(), cnnz, Ac.data());
    printf("blocked %d terms %zu dof_terms %zu fine_nnz %lld coarse_nnz %lld p_entries %lld\n", blocked ? 1 : 0, blocked ? gb.terms.size() : g.terms.size(), g.terms.size(),
           (long long)fnnz, (long long)cnnz, (long long)t.p_col.size());
    for (int64_t i = 0; i < F.ndofs; ++i)
        for (int64_t q = t.p_ptr[i]; q < t.p_ptr[i + 1]; ++q) printf("%lld %d %d\n", (long long)i, t.p_col[q], (int)t.p_exp[q]);
    for (double v : Ac) printf("%.17g\n", v);
    return 0;
}

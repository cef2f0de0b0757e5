// eikonal_planner_driver.cpp — the eikonal planner (thunderbolt.jl_amd/csrc/tb_eikonal_planners.cpp) without a GPU.  A stand-alone program linked
// with the planner file: reads one case (raw arrays written by tests/test_eikonal_cpu.py), builds the corner incidence and the node adjacency,
// checks the plan's invariants itself (exit status 1 with a message otherwise) and prints it.
//   usage: eikonal_planner_driver <dir> <case>
//   files: <case>.meta (text: n_nodes n_cells nverts)  <case>.conn (int32, n_cells × nverts)
//   output: "rc <code>", then — rc 0 — one line per node: "<code>:<a>,<b>,<c> ... | <neighbour> ..."
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tb_eikonal_planners.hpp"

namespace tb { void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); } }

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "invariant failed: " __VA_ARGS__); fputc('\n', stderr); return 1; } } while (0)

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <dir> <case>\n", argv[0]); return 2; }
    const std::string base = std::string(argv[1]) + "/" + argv[2];
    long long n_nodes, n_cells, nverts;
    {
        FILE *f = fopen((base + ".meta").c_str(), "r");
        if (!f || fscanf(f, "%lld %lld %lld", &n_nodes, &n_cells, &nverts) != 3) { fprintf(stderr, "cannot read %s.meta\n", base.c_str()); return 2; }
        fclose(f);
    }
    std::vector<int32_t> conn((size_t)(n_cells * nverts));
    {
        FILE *f = fopen((base + ".conn").c_str(), "rb");
        if (!f || fread(conn.data(), sizeof(int32_t), conn.size(), f) != conn.size()) { fprintf(stderr, "cannot read %s.conn\n", base.c_str()); return 2; }
        fclose(f);
    }
    tb::eikplan::IncidenceHost h;
    const int rc = tb::eikplan::incidence(n_nodes, n_cells, (int)nverts, conn.data(), h);
    printf("rc %d\n", rc);
    if (rc) return 0;
    const int ntet = nverts == 8 ? 6 : 1;
    const size_t total = (size_t)(n_cells * ntet * 4);
    CHECK(h.ntet == ntet, "ntet");
    CHECK(h.ptr.size() == (size_t)n_nodes + 1 && h.ptr.front() == 0 && (size_t)h.ptr.back() == total && h.code.size() == total && h.others.size() == 3 * total, "sizes");
    CHECK(h.adj_ptr.size() == (size_t)n_nodes + 1 && h.adj_ptr.front() == 0 && (size_t)h.adj_ptr.back() == h.adj.size(), "adjacency sizes");
    std::vector<int> seen(total, 0);
    for (long long v = 0; v < n_nodes; ++v) {
        CHECK(h.ptr[(size_t)v + 1] >= h.ptr[(size_t)v], "record pointer of node %lld", v);
        for (int64_t r = h.ptr[(size_t)v]; r < h.ptr[(size_t)v + 1]; ++r) {
            const int32_t code = h.code[(size_t)r];
            CHECK(code >= 0 && (size_t)code < total, "code out of range");
            ++seen[(size_t)code];
            CHECK(r == h.ptr[(size_t)v] || code / 4 > h.code[(size_t)r - 1] / 4, "records of node %lld are not in ascending (cell, tetrahedron) order", v);
            const int64_t cell = code / (4 * ntet);
            const int k = (code / 4) % ntet, a = code % 4;
            const int la = ntet == 6 ? tb::eikplan::KUHN[k][a] : a;
            CHECK(conn[(size_t)(cell * nverts + la)] == v, "record %lld does not stand under its node", (long long)r);
            printf("%s%d:%d,%d,%d", r == h.ptr[(size_t)v] ? "" : " ", code, h.others[3 * (size_t)r], h.others[3 * (size_t)r + 1], h.others[3 * (size_t)r + 2]);
        }
        printf(" |");
        for (int64_t k = h.adj_ptr[(size_t)v]; k < h.adj_ptr[(size_t)v + 1]; ++k) {
            const int32_t w = h.adj[(size_t)k];
            CHECK(w >= 0 && w < n_nodes && w != v, "neighbour out of range");
            CHECK(k == h.adj_ptr[(size_t)v] || w > h.adj[(size_t)k - 1], "neighbours of node %lld are not ascending and distinct", v);
            printf(" %d", w);
        }
        putchar('\n');
    }
    for (int s : seen) CHECK(s == 1, "a (tetrahedron, corner) does not appear exactly once");
    return 0;
}

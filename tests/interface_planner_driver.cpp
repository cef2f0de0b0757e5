// interface_planner_driver.cpp — the interface planner (thunderbolt.jl_amd/csrc/tb_interface_planners.cpp) without a GPU.  A stand-alone program
// linked with the planner file: reads one case (raw arrays written by tests/test_multidomain_cpu.py), builds the contribution list, checks the
// plan's invariants itself (exit status 1 with a message otherwise) and prints it.
//   usage: interface_planner_driver <dir> <case>
//   files: <case>.meta (text: n nf n_rows nnz)  <case>.edofs (int32, n × 2nf)  <case>.rowptr (int64)  <case>.colidx (int32)
//   output: "rc <code>", then — rc 0 — one line per touched non-zero: "<nz> <position>:<sign> <position>:<sign> ..."
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "tb_interface_planners.hpp"

namespace tb { void set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); } }

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

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <dir> <case>\n", argv[0]); return 2; }
    const std::string base = std::string(argv[1]) + "/" + argv[2];
    long long n, nf, n_rows, nnz;
    {
        FILE *f = fopen((base + ".meta").c_str(), "r");
        if (!f || fscanf(f, "%lld %lld %lld %lld", &n, &nf, &n_rows, &nnz) != 4) { fprintf(stderr, "cannot read %s.meta\n", base.c_str()); return 2; }
        fclose(f);
    }
    const auto edofs = read_raw<int32_t>(base + ".edofs", (size_t)(n * 2 * nf));
    const auto rowptr = read_raw<int64_t>(base + ".rowptr", (size_t)n_rows + 1);
    const auto colidx = read_raw<int32_t>(base + ".colidx", (size_t)nnz);
    const tb::plan::PatternView pv{n_rows, rowptr.data(), colidx.data(), 0};
    tb::ifplan::InterfaceHost h;
    const int rc = tb::ifplan::contributions(n, (int)nf, edofs.data(), pv, h);
    printf("rc %d\n", rc);
    if (rc) return 0;
    const size_t nd = (size_t)(2 * nf), total = (size_t)n * nd * nd;
    CHECK(h.ptr.size() == h.nz.size() + 1 && h.ptr.front() == 0 && (size_t)h.ptr.back() == total && h.src.size() == total, "sizes");
    std::vector<int> seen((size_t)(n * nf * nf) * 2, 0);
    for (size_t k = 0; k < h.nz.size(); ++k) {
        CHECK(h.nz[k] >= 0 && h.nz[k] < nnz && (k == 0 || h.nz[k] > h.nz[k - 1]), "non-zero %zu out of range or out of order", k);
        CHECK(h.ptr[k + 1] > h.ptr[k], "empty record %zu", k);
        printf("%lld", (long long)h.nz[k]);
        for (int64_t c = h.ptr[k]; c < h.ptr[k + 1]; ++c) {
            const uint32_t u = h.src[(size_t)c];
            CHECK((long long)(u >> 1) < n * nf * nf, "position out of the facet-matrix buffer");
            ++seen[u];
            printf(" %u:%d", u >> 1, (u & 1u) ? -1 : 1);
        }
        putchar('\n');
    }
    for (int s : seen) CHECK(s == 2, "an entry of a facet matrix is not used exactly twice with each sign");
    return 0;
}

// amg_planner_driver.cpp — stand-alone driver of the host planner of the algebraic multigrid (csrc/tb_amg_planners.cpp) for tests/test_amg_cpu.py.
// usage: amg_planner_driver DIR NAME — reads DIR/NAME.meta ("n nnz has_comp"), NAME.ptr (int64), NAME.col (int32), NAME.comp (int8, if has_comp) and
// NAME.str (one strength byte per non-zero); prints "rc 0 nc <aggregates>" (or "rc -1 <message>" when the pattern is refused) and writes the plan as
// raw arrays NAME.agg, .p_ptr, .p_col, .p_row, .r_ptr, .r_col, .r_perm, .ap_ptr, .ap_col, .c_ptr, .c_col, .c_diag, .ccomp, .size.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "tb_amg_planners.hpp"

template <class T>
static bool read_all(const std::string &path, std::vector<T> &v, size_t count)
{
    v.resize(count);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = count ? fread(v.data(), sizeof(T), count, f) : 0;
    fclose(f);
    return got == count;
}

template <class T>
static void write_all(const std::string &path, const std::vector<T> &v)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return;
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s DIR NAME\n", argv[0]); return 2; }
    const std::string base = std::string(argv[1]) + "/" + argv[2];
    long long n = 0, nnz = 0;
    int has_comp = 0;
    FILE *f = fopen((base + ".meta").c_str(), "r");
    if (!f || fscanf(f, "%lld %lld %d", &n, &nnz, &has_comp) != 3 || n < 0 || nnz < 0) { fprintf(stderr, "bad meta file\n"); return 2; }
    fclose(f);
    std::vector<int64_t> ptr;
    std::vector<int32_t> col;
    std::vector<int8_t> comp;
    std::vector<uint8_t> str;
    if (!read_all(base + ".ptr", ptr, (size_t)n + 1) || !read_all(base + ".col", col, (size_t)nnz) || !read_all(base + ".str", str, (size_t)nnz) ||
        (has_comp && !read_all(base + ".comp", comp, (size_t)n))) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    if (ptr[0] != 0 || ptr[(size_t)n] != nnz) { printf("rc -1 row pointers do not span the non-zeros\n"); return 0; }
    for (long long i = 0; i < n; ++i)
        if (ptr[(size_t)i + 1] < ptr[(size_t)i]) { printf("rc -1 row pointers decrease at row %lld\n", i); return 0; }
    std::string err;
    if (tb::amgplan::check_pattern(n, ptr.data(), col.data(), err)) { printf("rc -1 %s\n", err.c_str()); return 0; }
    tb::amgplan::LevelPlan L;
    tb::amgplan::plan_level(n, ptr.data(), col.data(), has_comp ? comp.data() : nullptr, str.data(), L);
    printf("rc 0 nc %lld\n", (long long)L.nc);
    write_all(base + ".agg", L.agg);
    write_all(base + ".size", L.agg_size);
    write_all(base + ".ccomp", L.ccomp);
    write_all(base + ".p_ptr", L.p_ptr);   write_all(base + ".p_col", L.p_col);   write_all(base + ".p_row", L.p_row);
    write_all(base + ".r_ptr", L.r_ptr);   write_all(base + ".r_col", L.r_col);   write_all(base + ".r_perm", L.r_perm);
    write_all(base + ".ap_ptr", L.ap_ptr); write_all(base + ".ap_col", L.ap_col);
    write_all(base + ".c_ptr", L.c_ptr);   write_all(base + ".c_col", L.c_col);   write_all(base + ".c_diag", L.c_diag);
    return 0;
}

// amg_block_planner_driver.cpp — stand-alone driver of the host side of the smoothed aggregation with a near-null-space for
// tests/test_amg_elasticity_cpu.py: the block planner (csrc/tb_amg_block_planners.cpp) and the shared QR header (csrc/tb_amg_qr.hpp, with its host
// executor of 64 emulated lanes).
// usage: amg_block_planner_driver plan DIR NAME — reads DIR/NAME.meta ("n nnz n_nodes k dofs_per_node"), NAME.ptr (int64), NAME.col (int32), NAME.node
//   (int32) and NAME.nstr (one strength byte per non-zero of the node graph, in its CSR order); prints "rc 0 na <aggregates> gnnz <node-graph
//   non-zeros>" (or "rc -1 <message>") and writes NAME.g_ptr, .g_col, .g_eptr, .g_ent, .g_nz, .node_agg, .agg, .adof_ptr, .adof, .p_ptr, .p_col, .p_row,
//   .r_ptr, .r_col, .r_perm, .ap_ptr, .ap_col, .c_ptr, .c_col, .c_diag.  Without NAME.nstr it stops after the node graph ("rc 0 gnnz <…>").
// usage: amg_block_planner_driver qr DIR NAME — reads NAME.qmeta ("blocks k"), NAME.qm (int32 rows per block) and NAME.qb (the blocks, row-major,
//   one after the other); writes NAME.qq (the Q factors, same layout), NAME.qr (k × k per block) and NAME.qdead (k bytes per block).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "tb_amg_block_planners.hpp"
#include "tb_amg_qr.hpp"

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

struct Rows {
    double *w;
    int k;
    double get(int p, int c) const { return w[(size_t)p * k + c]; }
    void set(int p, int c, double v) { w[(size_t)p * k + c] = v; }
};

static int run_qr(const std::string &base)
{
    long long nb = 0;
    int k = 0;
    FILE *f = fopen((base + ".qmeta").c_str(), "r");
    if (!f || fscanf(f, "%lld %d", &nb, &k) != 2 || nb < 0 || k < 1 || k > tb::amgqr::MAX_K) { fprintf(stderr, "bad qmeta file\n"); return 2; }
    fclose(f);
    std::vector<int32_t> m;
    if (!read_all(base + ".qm", m, (size_t)nb)) { fprintf(stderr, "short input\n"); return 2; }
    size_t total = 0;
    for (int32_t r : m) { if (r < 0) { fprintf(stderr, "negative block size\n"); return 2; } total += (size_t)r * k; }
    std::vector<double> w;
    if (!read_all(base + ".qb", w, total)) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<double> R((size_t)nb * k * k);
    std::vector<uint8_t> dead((size_t)nb * k);
    size_t at = 0;
    for (long long b = 0; b < nb; ++b) {
        Rows rows{w.data() + at, k};
        tb::amgqr::HostExec x;
        tb::amgqr::factor(rows, m[(size_t)b], k, x, R.data() + (size_t)b * k * k, dead.data() + (size_t)b * k);
        at += (size_t)m[(size_t)b] * k;
    }
    write_all(base + ".qq", w);
    write_all(base + ".qr", R);
    write_all(base + ".qdead", dead);
    printf("rc 0 blocks %lld\n", nb);
    return 0;
}

static int run_plan(const std::string &base)
{
    long long n = 0, nnz = 0, n_nodes = 0;
    int k = 0, per_node = 0;
    FILE *f = fopen((base + ".meta").c_str(), "r");
    if (!f || fscanf(f, "%lld %lld %lld %d %d", &n, &nnz, &n_nodes, &k, &per_node) != 5 || n < 0 || nnz < 0 || n_nodes < 0) { fprintf(stderr, "bad meta file\n"); return 2; }
    fclose(f);
    std::vector<int64_t> ptr;
    std::vector<int32_t> col, node;
    if (!read_all(base + ".ptr", ptr, (size_t)n + 1) || !read_all(base + ".col", col, (size_t)nnz) || !read_all(base + ".node", node, (size_t)n)) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    if (ptr[0] != 0 || ptr[(size_t)n] != nnz) { printf("rc -1 row pointers do not span the non-zeros\n"); return 0; }
    for (long long i = 0; i < n; ++i)
        if (ptr[(size_t)i + 1] < ptr[(size_t)i]) { printf("rc -1 row pointers decrease at row %lld\n", i); return 0; }
    std::string err;
    if (tb::amgplan::check_pattern(n, ptr.data(), col.data(), err)) { printf("rc -1 %s\n", err.c_str()); return 0; }
    if (k < 1 || k > tb::amgqr::MAX_K) { printf("rc -1 k = %d candidates; 1 to %d are supported\n", k, tb::amgqr::MAX_K); return 0; }
    if (tb::amgplan::check_nodes(n, node.data(), n_nodes, per_node, err)) { printf("rc -1 %s\n", err.c_str()); return 0; }
    tb::amgplan::NodeGraph g;
    tb::amgplan::node_graph(n, ptr.data(), col.data(), node.data(), n_nodes, g);
    write_all(base + ".g_ptr", g.ptr);      write_all(base + ".g_col", g.col);
    write_all(base + ".g_eptr", g.entry_ptr); write_all(base + ".g_ent", g.entries); write_all(base + ".g_nz", g.nz_of_entry);
    std::vector<uint8_t> str;
    if (!read_all(base + ".nstr", str, g.col.size())) { printf("rc 0 gnnz %lld\n", (long long)g.col.size()); return 0; }
    tb::amgplan::BlockPlan B;
    tb::amgplan::plan_block_level(n, ptr.data(), col.data(), node.data(), g, str.data(), k, B);
    const tb::amgplan::LevelPlan &L = B.L;
    printf("rc 0 na %lld gnnz %lld\n", (long long)B.n_agg, (long long)g.col.size());
    write_all(base + ".node_agg", B.node_agg); write_all(base + ".agg", L.agg);
    write_all(base + ".adof_ptr", B.adof_ptr); write_all(base + ".adof", B.adof);
    write_all(base + ".p_ptr", L.p_ptr);   write_all(base + ".p_col", L.p_col);   write_all(base + ".p_row", L.p_row);
    write_all(base + ".r_ptr", L.r_ptr);   write_all(base + ".r_col", L.r_col);   write_all(base + ".r_perm", L.r_perm);
    write_all(base + ".ap_ptr", L.ap_ptr); write_all(base + ".ap_col", L.ap_col);
    write_all(base + ".c_ptr", L.c_ptr);   write_all(base + ".c_col", L.c_col);   write_all(base + ".c_diag", L.c_diag);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s plan|qr DIR NAME\n", argv[0]); return 2; }
    const std::string base = std::string(argv[2]) + "/" + argv[3];
    if (!strcmp(argv[1], "qr")) return run_qr(base);
    if (!strcmp(argv[1], "plan")) return run_plan(base);
    fprintf(stderr, "unknown mode %s\n", argv[1]);
    return 2;
}

// tb_planners.hpp — the planning half of the assembly plans: pure host functions from views of a mesh and a CSR pattern to plan arrays.
// No device, no environment, no global state: tb_plans.cpp turns the environment into Options, calls these and uploads what they return;
// tests/planner_driver.cpp calls them on a machine without a GPU.  tb::set_error is the only tie to the rest of the library.
#pragma once
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <vector>

namespace tb {

void set_error(const char *fmt, ...);

struct RowDesc {      // one owned row of a patch
    int64_t nz0;      // first nz of the row in the global CSR arrays
    uint32_t off;     // offset of its accumulators in the patch's LDS block (in entries)
    uint32_t len;     // row length
};

// Staged tangent gather of the element strategy on three-component fields (k_gather_node_rows_lds): one record per field node
struct GatherNode {
    int64_t g0;      // first nz of row dof0 (rows dof0+1, dof0+2 follow, L entries each)
    int32_t L, nk;   // row length, number of cells at the node
    int32_t slot[8]; // cell·ND + 3a: row offset of the node's run in the stored element matrices, cell-ordered
};

// wall time of the plan builders, stage by stage, on stderr (TB_PLAN_VERBOSE; what `setup_s.first_step_incl_plan_build` of bench.py is made of)
struct StageTimer {
    const char *name;
    double t0;
    bool on, rest; // rest: the destructor prints what is left as "(rest)"
    static double now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
    StageTimer(const char *n, bool enabled, bool rest_line = true) : name(n), t0(0.0), on(enabled), rest(rest_line) { if (on) t0 = now(); }
    void lap(const char *what) { if (on) { const double t = now(); fprintf(stderr, "[tbhip] plan time: %-28s %-34s %8.3f s\n", name, what, t - t0); t0 = t; } }
    ~StageTimer() { if (rest) lap("(rest)"); }
};

namespace plan {

constexpr int64_t LDS_BUDGET = 80 * 1024; // one patch's block: two workgroups fit a CU's 160 KiB

struct MeshView { int64_t n_nodes, n_cells, ndofs; int nverts, ndpc, ncomp; const double *xyz; const int32_t *conn, *cell_dofs; };
struct PatternView { int64_t n_rows; const int64_t *rowptr; const int32_t *colidx; int64_t max_row_len; }; // max_row_len: 0 = not known
enum { ERR_BAD_ARG = -1, ERR_PATTERN = -4, ERR_UNSUPPORTED = -5 }; // the TB_ERR_* codes of include/tbhip.h (tb_plans.cpp asserts the match)

struct Options {               // what the environment decides (tb_plans.cpp: env_options)
    int tile[3] = {7, 7, 7};   // TB_PATCH_TILE
    bool tile_set = false;     // TB_PATCH_TILE is present (the tetrahedral default of 5×5×5 then does not apply)
    bool morton = false;       // TB_PATCH_CELLS without a valid TB_PATCH_TILE: Morton runs of `cells` cells instead of tiles
    int cells = 256;
    bool fixed = false;        // either of the two is present: the fit loops do not change the patch shape
    bool full_cut = false;     // TB_PATCH_CUT=full: full tiles and a sliver instead of balanced tiles
    bool by_nodes = true;      // balanced tiles of the matrix plan deal node layers (patches own rows)
    int threads = 0;           // TB_PATCH_THREADS, 0 = from the largest patch
    int vtile[3] = {8, 8, 8};  // TB_VPATCH_TILE
    bool vec_rcb = true;       // TB_PATCH_RCB=0 keeps the vector plan on tiles
    int rcb_max_inst = 384;    // TB_RCB_MAX_INST: largest patch (instances) a leaf size may produce before it is shrunk
    bool verbose = false;      // TB_PLAN_VERBOSE: stage times and plan summaries on stderr
};

struct FitState {                 // what tb_mesh remembers between fits
    int patch_rcb = 0;            // > 0: the matrix patch plan bisects the cells into leaves of this many cells instead of tiling per-axis buckets
    bool patch_rcb_tried = false; // the bisection was compared with the tiles once
    int patch_tile_shrink = 0;    // tile reductions the LDS-fit loop applied to the tile plan (restored when the bisection loses)
};

struct Outcome {
    enum Kind { OK, TOO_BIG, REFUSED } kind = OK;
    int code = 0;         // REFUSED: the TB_ERR_* code (the message is set)
    int64_t lds_need = 0; // bytes of LDS per patch
    bool ok() const { return kind == OK; }
};

// Patch plan: cells in Morton order are cut into patches; every dof (row) is owned by exactly one
// patch, which (re)computes all cells touching its rows, accumulates in LDS and stores once.
struct PatchHost {
    int cells_per_patch = 0;
    int shrink = 0;    // tile reductions applied so far
    int64_t n_patches = 0;
    int max_elems = 0, max_rows = 0, threads = 256; // threads: workgroup size used by the patch kernels
    int64_t total_elems = 0, total_rows = 0;
    std::vector<int64_t> h_elem_ptr, h_row_ptr;  // per patch: n_patches+1 → element instances / owned rows
    std::vector<int32_t> h_elem_cell, h_row_dof; // global cell of every instance, global dof of every owned row
    std::vector<uint16_t> h_elem_lrow;           // ndpc local-row slots per instance (0xFFFF = row not owned here)
};
// the extensions and the other plans: the arrays of PatchMatPlan, PatchFusedPlan, VecPatchPlan, ColorPlan and EAPlan (tb_internal.h) before their upload
struct MatHost { int max_lds_entries = 0; std::vector<RowDesc> row_desc; std::vector<uint16_t> rowoff, cp16; std::vector<uint8_t> cp8; }; // cp8 or cp16 (a row longer than 255)
struct FusedHost {
    int max_lds_entries = 0, max_nodes = 0;
    int64_t nsig = 0;
    std::vector<int64_t> node_ptr;
    std::vector<int32_t> pnode;
    std::vector<uint16_t> ln;
    std::vector<uint32_t> elem_sig, hdr; // hdr (and pcoord): empty when some count does not fit the packed word
    std::vector<uint8_t> sigtab;
    std::vector<RowDesc> row_desc;
    std::vector<double> pcoord;
};
struct Records { int stride = -1, rm = 0, nm = 0, ne = 0; std::vector<uint8_t> bytes; }; // stride −1: the patches do not take the record form
// The two classes of hexahedron patches (classify_records).  A patch is CANONICAL when it has at most 256 instances and, for every instance and every local
// node i the patch owns, the row has exactly 27 entries and the signature places column dof(j) at 13 + Δx + 3Δy + 9Δz of the row (Δ: vertex bits of j
// minus those of i in Ferrite's vertex order) — the interior rows of a lattice whose columns ascend lexicographically, under whatever numbering gives that
// order.  order[s] is the patch whose record sits in slot s: general patches first, canonical ones behind them, plan order within each class.
struct RecordClasses { int64_t n_general = 0, n_canonical = 0; std::vector<int64_t> order; };
struct VecHost {
    bool halo = false;
    int64_t n_patches = 0, total_elems = 0, total_nodes = 0;
    int max_nodes = 0, max_elems = 0;
    std::vector<uint32_t> hdr;
    std::vector<uint16_t> ln;
    std::vector<int32_t> ecell, pdof;
    std::vector<double> pcoord;
};
struct ColorHost { int ncolors = 0; std::vector<int64_t> offsets; std::vector<int32_t> cells; }; // offsets: ncolors+1, into cells (grouped by colour)
struct SlotTable { int w = 0; std::vector<int32_t> ell, h_done; }; // ell: ndofs × w, −1 padded; h_done: running maximum of the last contributing cell
struct GatherHost { bool applicable = false; std::vector<GatherNode> recs; std::vector<int32_t> last; }; // last: running maximum of the records' last contributing cell

void dof_slots(const MeshView &m, std::vector<int64_t> &ptr, std::vector<int32_t> &src); // dof → (cell·ndpc + local) slots, cell-ordered
SlotTable slot_table(const MeshView &m);
void tensor_order(std::vector<int32_t> &ell); // 27 dofs per cell: the local row of every slot replaced by its tensor index i₀ + 3 i₁ + 9 i₂
// three-component fields: the first dofs of the field nodes; the "three equal runs of whole nodes, ≤ 254 neighbours" condition on their rows (0 or
// ERR_PATTERN with the message set; max_row_len: the longest node row); the node records of the staged gather (p.max_row_len from the check)
std::vector<int32_t> node_list(const MeshView &m);
int node_row_check(const PatternView &p, const std::vector<int32_t> &dof0, int64_t &max_row_len);
GatherHost gather_nodes(const MeshView &m, const PatternView &p, const std::vector<int32_t> &dof0);
int color_cells(const MeshView &m, const int32_t *cells, int64_t n, ColorHost &out); // cells == nullptr: all n = n_cells cells
int patch_plan(const MeshView &m, const Options &o, int leaf, int shrink, PatchHost &out); // leaf > 0: bisection leaves of that size (shrink is then ignored)
std::vector<RowDesc> row_descs(const PatchHost &pp, const PatternView &p, int64_t &maxlen, int64_t &max_entries);
Outcome mat_extension(const MeshView &m, const PatternView &p, const PatchHost &pp, const Options &o, MatHost &out);
Outcome fused_extension(const MeshView &m, const PatternView &p, const PatchHost &pp, const Options &o, int nregions, FusedHost &out);
Records record_layout(const PatchHost &pp, int max_nodes);
RecordClasses classify_records(int64_t np, const uint32_t *hdr, const uint16_t *ln, const uint32_t *sig, const RowDesc *desc, const uint8_t *sigtab);
// order (np entries, a permutation) puts patch order[s] into record slot s; nullptr keeps the plan's order
void pack_records(Records &rec, int64_t np, const uint32_t *hdr, const uint16_t *ln, const uint32_t *sig, const RowDesc *desc, const double *xyz, const int64_t *order = nullptr);
int vec_patch_plan(const MeshView &m, const Options &o, bool halo, VecHost &out);
// The fit policies.  `cur` is the mesh's patch plan, or empty where it has none yet; a fit that has to change the patch shape builds the new plan in place and sets
// `replaced` — the caller then owes the device a new copy.  After a failed patch planner `cur` is empty.
Outcome fit_mat(const MeshView &m, const PatternView &p, const Options &o, FitState &st, PatchHost &cur, bool &replaced, MatHost &mat);
Outcome fit_fused(const MeshView &m, const PatternView &p, const Options &o, int nregions, FitState &st, PatchHost &cur, bool &replaced, FusedHost &fused);

} // namespace plan
} // namespace tb

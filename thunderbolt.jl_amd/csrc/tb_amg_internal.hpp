// tb_amg_internal.hpp — the hierarchy object of tb_amg.hip and what tb_multigrid.hip needs of it (the AMG cycle as the coarse solver of a geometric
// or p-hierarchy: tb_mg_set_coarse_amg).
#pragma once
#include <cstdint>
#include <vector>

#include "tb_amg_block_planners.hpp"
#include "tb_amg_planners.hpp"
#include "tb_internal.h"
#include "tb_mg_internal.hpp"

namespace tb {

struct AmgLevel : MgVectors {
    int64_t n = 0, nnz = 0, nc = 0;      // dofs, non-zeros, aggregates (0 on the last level)
    // the level's operator: level 0 reads the caller's pattern and array, the levels below own theirs
    const int64_t *rowptr = nullptr;
    const int32_t *colidx = nullptr;
    const double *A = nullptr;
    int64_t *d_rowptr = nullptr;
    int32_t *d_colidx = nullptr;
    double *d_A = nullptr;
    std::vector<int64_t> h_rowptr;
    std::vector<int32_t> h_colidx;
    std::vector<int8_t> h_comp;          // component labels (empty: one component)
    int8_t *d_comp = nullptr;
    int64_t *d_diag = nullptr;           // position of every row's diagonal
    double lmax = 0.0;
    uint8_t *d_strength = nullptr;       // (lives during planning only)
    std::vector<uint8_t> h_strength;
    // to the level below
    amgplan::LevelPlan plan;             // the host keeps the aggregates and P's pattern
    int64_t pnnz = 0, apnnz = 0;
    int32_t *d_agg = nullptr, *d_pcol = nullptr, *d_prow = nullptr, *d_rcol = nullptr, *d_apcol = nullptr, *d_aprow = nullptr, *d_crow = nullptr;
    int64_t *d_pptr = nullptr, *d_rptr = nullptr, *d_rperm = nullptr, *d_apptr = nullptr;
    double *d_tval = nullptr, *d_P = nullptr, *d_R = nullptr, *d_AP = nullptr;
    // with a near-null-space of k candidates (tb_amg_block.hip; all empty without one)
    std::vector<int32_t> h_node;         // node of every dof (level 0: the caller's map; below: dof / k)
    int64_t n_nodes = 0;
    double *d_B = nullptr;               // candidates B_l, n × k row-major (rows of eliminated dofs zeroed when the level is planned)
    double *d_T = nullptr;               // tentative prolongator, dense n × k: row i lies in the column block of its node's aggregate
    double *d_Bc = nullptr;              // B_{l+1} on its way to the level below (which owns it from its creation on)
    uint8_t *d_dead = nullptr;           // one byte per dof of level l + 1: a dead column of its aggregate's QR
    int64_t *d_adofptr = nullptr;        // the dofs of every aggregate, ascending
    int32_t *d_adof = nullptr;
    amgplan::BlockPlan bplan;            // (its LevelPlan moves into `plan`)
};

// k_amg_rowmax and k_amg_strength on any CSR with one value per non-zero (the node graph and its block norms); m: n doubles of scratch; enqueues only
void launch_amg_strength(tb_device *dev, int64_t n, const int64_t *rowptr, const int32_t *colidx, const double *val, const int8_t *comp, double theta, double *m,
                         uint8_t *flag);
// tb_amg_block.hip — the steps a near-null-space replaces.  amg_block_plan: candidates' zero rows, node strength (device), node graph, aggregates and
// patterns (host) into lv[l].h_strength, .plan, .bplan; amg_block_tentative: uploads, the per-aggregate QR into d_T, d_Bc and d_dead;
// amg_block_smooth_p and amg_block_dead_diag enqueue only.
int amg_block_plan(tb_amg *amg, int l);
int amg_block_tentative(tb_amg *amg, int l);
void amg_block_smooth_p(tb_amg *amg, int l, double omega);
void amg_block_dead_diag(tb_amg *amg, int l);
void amg_block_free_level(AmgLevel &L);

int amg_apply_cb(void *ctx, const double *r, double *z); // z = one V-cycle on r (ctx: the tb_amg); enqueues only
// k_amg_spgemm, C = A·B on the planned pattern of C (crow, ccol: row and column of every non-zero of C); enqueues only
void launch_amg_spgemm(tb_device *dev, int64_t cnnz, const int32_t *crow, const int32_t *ccol, const int64_t *aptr, const int32_t *acol, const double *aval, const int64_t *bptr,
                       const int32_t *bcol, const double *bval, double *cval);

} // namespace tb

struct tb_amg {
    tb_device *dev = nullptr;
    tb_pattern *pat = nullptr;
    double theta = 0.25;
    int max_coarse = tb::MG_COARSEST_MAX, max_levels = 16;
    std::vector<int8_t> comp;
    std::vector<tb::AmgLevel> lv;        // lv[0]: the caller's matrix
    bool planned = false, ready = false;
    bool general = false;                // tb_amg_set_general: the operator need not be symmetric — the last level's inverse is pivoted and not symmetrised
    int degree = 2;
    double ratio = 4.0;
    double *d_cinv = nullptr;            // dense inverse of the last level's operator
    double *d_red = nullptr;             // partials and result of the ordered reductions
    // a block hierarchy on top of this one (tb_bidomain_amg.hip): `products(ctx, l)` replaces the two products of launch_level_numeric between level l and
    // l + 1 — it carries further planes through the same walk and leaves this hierarchy's own A·P and A_{l+1} where the scalar products would; the last
    // level is inverted there (at most last_max of its units here), and the set-up's messages carry its entry's name and unit
    int (*products)(void *ctx, int l) = nullptr;
    void *products_ctx = nullptr;
    int last_max = tb::MG_COARSEST_MAX;
    const char *who = "tb_amg_setup", *unit = "dofs";
    // tb_amg_set_near_nullspace: k candidates on node blocks (k = 0: none — the scalar method, one constant per aggregate and component)
    int nns_k = 0;
    int64_t nns_nodes = 0;
    std::vector<int32_t> nns_node;
    std::vector<double> nns_B;
    int64_t aggregations = 0;            // host aggregation runs so far (one per level planned): what a numeric-only set-up leaves as it is
};

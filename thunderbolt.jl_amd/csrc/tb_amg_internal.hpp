// tb_amg_internal.hpp — the hierarchy object of tb_amg.hip and what tb_multigrid.hip needs of it (the AMG cycle as the coarse solver of a geometric
// or p-hierarchy: tb_mg_set_coarse_amg).
#pragma once
#include <cstdint>
#include <vector>

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
};

int amg_apply_cb(void *ctx, const double *r, double *z); // z = one V-cycle on r (ctx: the tb_amg); enqueues only

} // namespace tb

struct tb_amg {
    tb_device *dev = nullptr;
    tb_pattern *pat = nullptr;
    double theta = 0.25;
    int max_coarse = tb::MG_COARSEST_MAX, max_levels = 16;
    std::vector<int8_t> comp;
    std::vector<tb::AmgLevel> lv;        // lv[0]: the caller's matrix
    bool planned = false, ready = false;
    int degree = 2;
    double ratio = 4.0;
    double *d_cinv = nullptr;            // dense inverse of the last level's operator
    double *d_red = nullptr;             // partials and result of the ordered reductions
};

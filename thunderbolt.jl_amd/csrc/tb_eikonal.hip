// tb_eikonal.hip — activation times from the anisotropic eikonal equation √(∇Tᵀ G ∇T) = 1 for gfx950: the fast iterative method (Jeong, Whitaker
// 2008; Fu, Kirby, Whitaker 2013) as a Jacobi iteration on two buffers, and the potential φₘ(x) = U(t − T(x)) recovered from a template.
//
// Nodes are the dofs of the form's scalar first-order field (T is a vector the ECG caches and the operators take as it is).  First order on
// tetrahedra: a TB_TET4 mesh as it is, a TB_HEX8 mesh cut implicitly, cell by cell and by LOCAL vertex order, into the six Kuhn tetrahedra
// (tb_eikonal_planners.hpp).  Per cell M = G⁻¹ (6 doubles), G the symmetric part of the form's constant tensor or of the mean of its table over the
// cell's quadrature points (k_eik_metric).  The local solver is tb_eikonal.hpp.
//
// Data of a sweep (one lane per node): the node's coordinates (24 B), then per incident (tetrahedron, corner) one 16-byte record {the three other
// nodes, corner code}, their coordinates and times (3 × 32 B, gathered — neighbours in a lattice numbering sit in a few cache lines that the 24
// records of a node share) and the cell's M (48 B, shared by the 6 × 4 records of a hexahedron).  Edge vectors are formed from the coordinates;
// the alternative, a per-tetrahedron table of the six edge products (48 B per tetrahedron), was measured against it and lives in the profiling
// build only (TB_EIKONAL_LAYOUT=table).
//
// k_eik_sweep: a node is ACTIVE iff one of its neighbours (adjacency list) changed in the previous sweep.  An active node takes the minimum of its
// local solves in incidence order — ascending (cell, tetrahedron), the planner's order — and accepts it iff T_old = ∞ or T_old − t > rtol·t; every
// other node copies its old value.  Source nodes are never updated.  The values only decrease, each time by more than the relative rtol, and are
// bounded below: the iteration ends on its own; max_sweeps is the guard.
//
// Determinism: the active set is a flag array (two, swapped like the two T buffers), a node's minimum has a fixed operand order and a Jacobi sweep
// reads only the previous buffer — no value of T depends on the order in which lanes or workgroups run.  The only atomic is the count of changed
// nodes (reduction slots of tb_reduce.hpp: an integer-valued double below 2⁵³, exact in any order), which no T depends on.
//
// Loop: the host enqueues EIK_CHECK_EVERY sweeps, each followed by a fold of its counts (changed, evaluated, local solves) into its own doubles, and
// reads the counts back once per batch.  The first sweep without a change ends the solve (the ones enqueued behind it changed nothing either).  No kernel waits for another
// workgroup, nothing spins, nothing is persistent: a sweep is a plain grid over the nodes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "tb_eikonal.hpp"
#include "tb_eikonal_planners.hpp"
#include "tb_internal.h"
#include "tb_reduce.hpp"

struct tb_eikonal {
    tb_form *form = nullptr;
    tb_mesh *mesh = nullptr;
    int64_t n = 0, n_cells = 0, n_rec = 0;
    int ntet = 1;
    double *d_x = nullptr;         // 3 per node (dof order)
    double *d_M = nullptr;         // 6 per cell
    int64_t *d_ptr = nullptr;      // n + 1 → records
    int4 *d_rec = nullptr;         // {other nodes a, b, c; (cell · ntet + k) · 4 + corner}
    int64_t *d_adj_ptr = nullptr;  // n + 1 → neighbours
    int32_t *d_adj = nullptr;
    double *d_T2 = nullptr;        // the second buffer of the Jacobi sweeps
    uint8_t *d_chg[2] = {nullptr, nullptr}; // changed in the previous / this sweep
    uint8_t *d_fixed = nullptr;    // source nodes of the latest solve
    double *d_counts = nullptr;    // per sweep of a batch: changed nodes, evaluated nodes, local solves
    int32_t *d_src = nullptr;      // sources of the latest solve (grown on demand)
    double *d_src_t = nullptr;
    int64_t src_cap = 0;
    int64_t last_counts[3] = {0, 0, 0}; // latest solve: nodes evaluated, updates accepted, local solves made
    double *d_tet6 = nullptr;      // profiling build: M-lengths² of the six edges of every tetrahedron (TB_EIKONAL_LAYOUT=table)
};

namespace tb {

constexpr int EIK_BLOCK = 256;
constexpr int EIK_CHECK_EVERY = 16; // sweeps between two looks at the counts

// M = sym(G)⁻¹ per cell, G the constant tensor (dtab == NULL) or the mean of the cell's nq table entries (xx, xy, xz, yy, yz, zz);
// *bad = 1 + the highest cell whose tensor is not positive definite (integer atomic; its M is left zero)
struct EikTensor { double D[9]; };
__global__ void __launch_bounds__(EIK_BLOCK)
k_eik_metric(int64_t n_cells, int nq, const double *__restrict__ dtab, EikTensor Dc, double *__restrict__ M, unsigned long long *__restrict__ bad)
{
    const int64_t c = (int64_t)blockIdx.x * EIK_BLOCK + threadIdx.x;
    if (c >= n_cells) return;
    double g[6];
    if (dtab) {
        for (int s = 0; s < 6; ++s) g[s] = 0.0;
        for (int q = 0; q < nq; ++q)
            for (int s = 0; s < 6; ++s) g[s] += dtab[(c * nq + q) * 6 + s];
        for (int s = 0; s < 6; ++s) g[s] /= (double)nq;
    } else {
        g[0] = Dc.D[0]; g[1] = 0.5 * (Dc.D[1] + Dc.D[3]); g[2] = 0.5 * (Dc.D[2] + Dc.D[6]);
        g[3] = Dc.D[4]; g[4] = 0.5 * (Dc.D[5] + Dc.D[7]); g[5] = Dc.D[8];
    }
    const double A0 = g[3] * g[5] - g[4] * g[4], A1 = g[2] * g[4] - g[1] * g[5], A2 = g[1] * g[4] - g[2] * g[3];
    const double A3 = g[0] * g[5] - g[2] * g[2], A4 = g[1] * g[2] - g[0] * g[4], A5 = g[0] * g[3] - g[1] * g[1];
    const double det = g[0] * A0 + g[1] * A1 + g[2] * A2;
    const bool spd = g[0] > 0.0 && A5 > 0.0 && det > 0.0 && det < __builtin_huge_val(); // Sylvester; false for NaN
    double *m = M + 6 * c;
    if (spd) {
        const double id = 1.0 / det;
        m[0] = A0 * id; m[1] = A1 * id; m[2] = A2 * id; m[3] = A3 * id; m[4] = A4 * id; m[5] = A5 * id;
    } else {
        for (int s = 0; s < 6; ++s) m[s] = 0.0;
        atomicMax(bad, (unsigned long long)c + 1ull);
    }
}

// the minimum of the local solves of node i on T, in incidence order
template <int NTET>
__device__ __forceinline__ double node_minimum(int64_t i, const double *__restrict__ x, const double *__restrict__ M, const int64_t *__restrict__ ptr,
                                               const int4 *__restrict__ rec, const double *__restrict__ T, int &nsolves)
{
    const double xi0 = x[3 * i], xi1 = x[3 * i + 1], xi2 = x[3 * i + 2];
    double best = __builtin_huge_val();
    const int64_t r1 = ptr[i + 1];
    for (int64_t r = ptr[i]; r < r1; ++r) {
        const int4 q = rec[r];
        const double Tv[3] = {T[q.x], T[q.y], T[q.z]};
        if (!(Tv[0] < __builtin_huge_val() || Tv[1] < __builtin_huge_val() || Tv[2] < __builtin_huge_val())) continue;
        const double *xa = x + 3 * (int64_t)q.x, *xb = x + 3 * (int64_t)q.y, *xc = x + 3 * (int64_t)q.z;
        const double Y[3][3] = {{xa[0] - xi0, xa[1] - xi1, xa[2] - xi2}, {xb[0] - xi0, xb[1] - xi1, xb[2] - xi2}, {xc[0] - xi0, xc[1] - xi1, xc[2] - xi2}};
        const double v = eikonal_local_solve(Y, Tv, M + 6 * (int64_t)(q.w / (4 * NTET)), nullptr);
        ++nsolves;
        if (v < best) best = v;
    }
    return best;
}

template <int NTET>
__global__ void __launch_bounds__(EIK_BLOCK)
k_eik_sweep(int64_t n, const double *__restrict__ x, const double *__restrict__ M, const int64_t *__restrict__ ptr, const int4 *__restrict__ rec,
            const int64_t *__restrict__ adj_ptr, const int32_t *__restrict__ adj, const uint8_t *__restrict__ fixed, const double *__restrict__ T_old,
            double *__restrict__ T_new, const uint8_t *__restrict__ chg_prev, uint8_t *__restrict__ chg_cur, double rtol, double *__restrict__ slots)
{
    const int64_t i = (int64_t)blockIdx.x * EIK_BLOCK + threadIdx.x;
    double cnt = 0.0, evals = 0.0;
    int nsolves = 0;
    if (i < n) {
        const double Ti = T_old[i];
        double out = Ti;
        bool changed = false;
        if (!fixed[i]) {
            bool active = false;
            const int64_t a1 = adj_ptr[i + 1];
            for (int64_t k = adj_ptr[i]; k < a1; ++k) active |= chg_prev[adj[k]] != 0;
            if (active) {
                evals = 1.0;
                const double t = node_minimum<NTET>(i, x, M, ptr, rec, T_old, nsolves);
                if (t < __builtin_huge_val() && (!(Ti < __builtin_huge_val()) || Ti - t > rtol * t)) { out = t; changed = true; }
            }
        }
        T_new[i] = out;
        chg_cur[i] = changed ? 1 : 0;
        cnt = changed ? 1.0 : 0.0;
    }
    // slot groups 0, 1, 2: changed nodes (what ends the loop), evaluated nodes, local solves — counts below 2⁵³ are exact in a double
    block_sum2_slots(cnt, evals, slots, slots + RED_GROUP);
    block_sum_slots((double)nsolves, slots + 2 * RED_GROUP);
}

#ifdef TB_ABLATION
// ---- the layout that was measured against the one above: a table of the six squared M-lengths of every tetrahedron's edges, pairs (0,1) (0,2) (0,3)
// (1,2) (1,3) (2,3) of its corners (48 B per tetrahedron, built once), from which a corner's Gram matrix follows: Q_ij = ½ (d²_ci + d²_cj − d²_ij)
template <int NTET>
__global__ void __launch_bounds__(EIK_BLOCK)
k_eik_tet_table(int64_t n_tets, const int32_t *__restrict__ cell_dofs, const double *__restrict__ x, const double *__restrict__ M, double *__restrict__ tet6)
{
    const int64_t tt = (int64_t)blockIdx.x * EIK_BLOCK + threadIdx.x;
    if (tt >= n_tets) return;
    const int64_t cell = tt / NTET;
    const int k = (int)(tt % NTET);
    const double *xv[4];
    for (int a = 0; a < 4; ++a) xv[a] = x + 3 * (int64_t)cell_dofs[cell * (NTET == 6 ? 8 : 4) + (NTET == 6 ? eikplan::KUHN[k][a] : a)];
    const double *m = M + 6 * cell;
    int o = 0;
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b) {
            const double e[3] = {xv[b][0] - xv[a][0], xv[b][1] - xv[a][1], xv[b][2] - xv[a][2]};
            double Me[3];
            eikonal_mul(m, e, Me);
            tet6[6 * tt + o++] = eikonal_dot(e, Me);
        }
}
__device__ __forceinline__ int pair_index(int a, int b) { return a == 0 ? b - 1 : a == 1 ? b + 1 : 5; } // a < b
template <int NTET>
__global__ void __launch_bounds__(EIK_BLOCK)
k_eik_sweep_table(int64_t n, const double *__restrict__ tet6, const int64_t *__restrict__ ptr, const int4 *__restrict__ rec,
                  const int64_t *__restrict__ adj_ptr, const int32_t *__restrict__ adj, const uint8_t *__restrict__ fixed, const double *__restrict__ T_old,
                  double *__restrict__ T_new, const uint8_t *__restrict__ chg_prev, uint8_t *__restrict__ chg_cur, double rtol, double *__restrict__ slots)
{
    const int64_t i = (int64_t)blockIdx.x * EIK_BLOCK + threadIdx.x;
    double cnt = 0.0, evals = 0.0;
    int nsolves = 0;
    if (i < n) {
        const double Ti = T_old[i];
        double out = Ti;
        bool changed = false;
        if (!fixed[i]) {
            bool active = false;
            const int64_t a1 = adj_ptr[i + 1];
            for (int64_t k = adj_ptr[i]; k < a1; ++k) active |= chg_prev[adj[k]] != 0;
            if (active) {
                evals = 1.0;
                double t = __builtin_huge_val();
                const int64_t r1 = ptr[i + 1];
                for (int64_t r = ptr[i]; r < r1; ++r) {
                    const int4 q = rec[r];
                    const double Tv[3] = {T_old[q.x], T_old[q.y], T_old[q.z]};
                    if (!(Tv[0] < __builtin_huge_val() || Tv[1] < __builtin_huge_val() || Tv[2] < __builtin_huge_val())) continue;
                    const double *d = tet6 + 6 * (int64_t)(q.w >> 2);
                    const int c = q.w & 3;
                    const int o0 = c == 0 ? 1 : 0, o1 = c <= 1 ? 2 : 1, o2 = c == 3 ? 2 : 3; // the other corners, ascending
                    const double dc0 = d[pair_index(c < o0 ? c : o0, c < o0 ? o0 : c)], dc1 = d[pair_index(c < o1 ? c : o1, c < o1 ? o1 : c)],
                                 dc2 = d[pair_index(c < o2 ? c : o2, c < o2 ? o2 : c)];
                    const double Q[6] = {dc0, 0.5 * (dc0 + dc1 - d[pair_index(o0, o1)]), 0.5 * (dc0 + dc2 - d[pair_index(o0, o2)]), dc1,
                                         0.5 * (dc1 + dc2 - d[pair_index(o1, o2)]), dc2};
                    const double v = eikonal_local_solve_gram(Q, Tv);
                    ++nsolves;
                    if (v < t) t = v;
                }
                if (t < __builtin_huge_val() && (!(Ti < __builtin_huge_val()) || Ti - t > rtol * t)) { out = t; changed = true; }
            }
        }
        T_new[i] = out;
        chg_cur[i] = changed ? 1 : 0;
        cnt = changed ? 1.0 : 0.0;
    }
    block_sum2_slots(cnt, evals, slots, slots + RED_GROUP);
    block_sum_slots((double)nsolves, slots + 2 * RED_GROUP);
}
#endif

// res[i] = T[i] − min(local solves on T) for the nodes that are not sources (0 there, and 0 where both are ∞)
template <int NTET>
__global__ void __launch_bounds__(EIK_BLOCK)
k_eik_residual(int64_t n, const double *__restrict__ x, const double *__restrict__ M, const int64_t *__restrict__ ptr, const int4 *__restrict__ rec,
               const uint8_t *__restrict__ fixed, const double *__restrict__ T, double *__restrict__ res)
{
    const int64_t i = (int64_t)blockIdx.x * EIK_BLOCK + threadIdx.x;
    if (i >= n) return;
    double r = 0.0;
    if (!fixed[i]) {
        int nsolves = 0;
        const double Ti = T[i], t = node_minimum<NTET>(i, x, M, ptr, rec, T, nsolves);
        const bool fi = Ti < __builtin_huge_val(), ft = t < __builtin_huge_val();
        r = (fi || ft) ? Ti - t : 0.0;
    }
    res[i] = r;
}

__global__ void __launch_bounds__(EIK_BLOCK)
k_eik_init(int64_t n, double *__restrict__ T, uint8_t *__restrict__ chg, uint8_t *__restrict__ fixed)
{
    const int64_t i = (int64_t)blockIdx.x * EIK_BLOCK + threadIdx.x;
    if (i >= n) return;
    T[i] = __builtin_huge_val(); chg[i] = 0; fixed[i] = 0;
}
// the sources: fixed, and "changed" before the first sweep so that their neighbours are active in it (the host has checked range and uniqueness)
__global__ void __launch_bounds__(EIK_BLOCK)
k_eik_sources(int64_t ns, const int32_t *__restrict__ src, const double *__restrict__ times, double *__restrict__ T, uint8_t *__restrict__ chg,
              uint8_t *__restrict__ fixed)
{
    const int64_t k = (int64_t)blockIdx.x * EIK_BLOCK + threadIdx.x;
    if (k >= ns) return;
    const int32_t i = src[k];
    T[i] = times[k]; chg[i] = 1; fixed[i] = 1;
}

// φ[i] = U(t − T[i]): U tabulated at t0 + k·dt, k < ns, linear between the samples, the first sample before t0 (and where T = ∞), the last beyond
__global__ void __launch_bounds__(EIK_BLOCK)
k_eik_potential(int64_t n, const double *__restrict__ T, double t, const double *__restrict__ tslot, int64_t ns, double t0, double dt,
                const double *__restrict__ U, double *__restrict__ phi)
{
    const int64_t i = (int64_t)blockIdx.x * EIK_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (tslot) t = tslot[0]; // replayed from a graph: the time of this launch sits on the device (tb_graph.hip)
    const double Ti = T[i];
    double v = U[0];
    if (Ti < __builtin_huge_val()) { // false for ∞ and NaN
        const double tau = t - Ti, s = (tau - t0) / dt;
        if (s >= (double)(ns - 1)) v = U[ns - 1];
        else if (s > 0.0) {
            int64_t k = (int64_t)s;
            if (k > ns - 2) k = ns - 2;
            const double xk = t0 + (double)k * dt;
            v = U[k] + (U[k + 1] - U[k]) / dt * (tau - xk);
        }
    }
    phi[i] = v;
}

static void free_eikonal(tb_eikonal *e)
{
    if (!e) return;
    (void)hipFree(e->d_x); (void)hipFree(e->d_M); (void)hipFree(e->d_ptr); (void)hipFree(e->d_rec); (void)hipFree(e->d_adj_ptr); (void)hipFree(e->d_adj);
    (void)hipFree(e->d_T2); (void)hipFree(e->d_chg[0]); (void)hipFree(e->d_chg[1]); (void)hipFree(e->d_fixed); (void)hipFree(e->d_counts);
    (void)hipFree(e->d_src); (void)hipFree(e->d_src_t); (void)hipFree(e->d_tet6);
    delete e;
}

static unsigned eik_grid(int64_t n) { return (unsigned)((n + EIK_BLOCK - 1) / EIK_BLOCK); }

static int build_metric(tb_eikonal *e)
{
    tb_device *dev = e->mesh->dev;
    unsigned long long *d_bad = nullptr;
    TB_HIP(hipMalloc((void **)&d_bad, sizeof(unsigned long long)));
    std::unique_ptr<unsigned long long, void (*)(unsigned long long *)> hold(d_bad, [](unsigned long long *p) { (void)hipFree(p); });
    TB_HIP(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), dev->stream));
    EikTensor Dc;
    for (int i = 0; i < 9; ++i) Dc.D[i] = e->form->Dconst[i];
    hipLaunchKernelGGL(k_eik_metric, dim3(eik_grid(e->n_cells)), dim3(EIK_BLOCK), 0, dev->stream, e->n_cells, e->ntet == 6 ? 8 : 4,
                       e->form->field ? e->form->d_dtab : (const double *)nullptr, Dc, e->d_M, d_bad);
    TB_HIP(hipGetLastError());
    unsigned long long bad = 0;
    static_assert(sizeof(unsigned long long) == sizeof(double), "read_back moves 8-byte words");
    TB_TRY(read_back(dev, (double *)&bad, (const double *)d_bad, 1));
    if (bad) {
        set_error("tb_eikonal_create: the tensor G of cell %lld (0-based) is not positive definite", (long long)bad - 1);
        return TB_ERR_BAD_ARG;
    }
    return TB_OK;
}

template <int NTET>
static void enqueue_sweep(tb_eikonal *e, const double *T_old, double *T_new, int parity, double rtol)
{
    tb_device *dev = e->mesh->dev;
#ifdef TB_ABLATION
    if (e->d_tet6) {
        hipLaunchKernelGGL((k_eik_sweep_table<NTET>), dim3(eik_grid(e->n)), dim3(EIK_BLOCK), 0, dev->stream, e->n, e->d_tet6, e->d_ptr, e->d_rec, e->d_adj_ptr,
                           e->d_adj, e->d_fixed, T_old, T_new, e->d_chg[parity], e->d_chg[parity ^ 1], rtol, red_group(dev, 0));
        return;
    }
#endif
    hipLaunchKernelGGL((k_eik_sweep<NTET>), dim3(eik_grid(e->n)), dim3(EIK_BLOCK), 0, dev->stream, e->n, e->d_x, e->d_M, e->d_ptr, e->d_rec, e->d_adj_ptr,
                       e->d_adj, e->d_fixed, T_old, T_new, e->d_chg[parity], e->d_chg[parity ^ 1], rtol, red_group(dev, 0));
}

} // namespace tb

using namespace tb;

extern "C" {

int tb_eikonal_create(tb_form *diffusion, tb_eikonal **out)
{
    TB_REQUIRE(diffusion && out, "tb_eikonal_create: NULL argument");
    *out = nullptr;
    if (diffusion->has_cellset) { // reachable with the forms that take a cell set today; named first, whatever the form's kind
        set_error("tb_eikonal_create: the form has a cell set - the eikonal solver works over all cells (cell sets and subdomains are out of scope)");
        return TB_ERR_UNSUPPORTED;
    }
    TB_REQUIRE(diffusion->kind == TB_FORM_DIFFUSION, "tb_eikonal_create: form kind %d is not TB_FORM_DIFFUSION (G is the tensor of a diffusion form)", diffusion->kind);
    tb_mesh *m = diffusion->mesh;
    const bool hex = m->geom_kind == TB_HEX8 && m->field_kind == TB_HEX8, tet = m->geom_kind == TB_TET4 && m->field_kind == TB_TET4;
    if (!(hex || tet) || m->ncomp != 1 || diffusion->has_cellset || (diffusion->field && diffusion->qorder != 2)) {
        set_error("tb_eikonal_create: geometry kind %d, field kind %d, %d component(s), quadrature order %d%s - the eikonal solver is built for scalar first-order "
                  "fields on TB_HEX8 and TB_TET4 meshes (3-D), over all cells, field tensors tabulated with the 2-point rule; TB_QUAD4, second-order fields, "
                  "cell sets and subdomains are out of scope", m->geom_kind, m->field_kind, m->ncomp, diffusion->qorder, diffusion->has_cellset ? ", cell set" : "");
        return TB_ERR_UNSUPPORTED;
    }
    tb_device *dev = m->dev;
    TB_NO_CAPTURE(dev); // allocates, uploads the plan, tabulates G on first use and reads the SPD flag back
    TB_HIP(hipSetDevice(dev->id));
    TB_REQUIRE(m->n_cells > 0 && m->ndofs > 0, "tb_eikonal_create: the mesh has no cells");
    TB_REQUIRE(m->ndofs < 0x7FFFFFFF, "tb_eikonal_create: %lld nodes exceed Int32", (long long)m->ndofs);
    if (diffusion->field && !diffusion->d_dtab) TB_TRY(hex ? tabulate_diffusion_field(diffusion) : tabulate_diffusion_field_tet4(diffusion));
    std::unique_ptr<tb_eikonal, void (*)(tb_eikonal *)> e(new tb_eikonal, free_eikonal);
    e->form = diffusion; e->mesh = m;
    e->n = m->ndofs; e->n_cells = m->n_cells; e->ntet = hex ? 6 : 1;
    // nodes are the field's dofs: the plan is built on the dof table, the coordinates are put in dof order
    eikplan::IncidenceHost h;
    {
        const int rc = eikplan::incidence(m->ndofs, m->n_cells, m->nverts, m->h_cell_dofs.data(), h);
        if (rc) return rc;
    }
    e->n_rec = (int64_t)h.code.size();
    std::vector<double> x((size_t)m->ndofs * 3, 0.0);
    for (size_t k = 0; k < m->h_conn.size(); ++k)
        for (int d = 0; d < 3; ++d) x[3 * (size_t)m->h_cell_dofs[k] + d] = m->h_xyz[3 * (size_t)m->h_conn[k] + d];
    std::vector<int4> rec(h.code.size());
    for (size_t r = 0; r < rec.size(); ++r) rec[r] = make_int4(h.others[3 * r], h.others[3 * r + 1], h.others[3 * r + 2], h.code[r]);
    TB_TRY(upload_all(dev, x, &e->d_x, h.ptr, &e->d_ptr, rec, &e->d_rec, h.adj_ptr, &e->d_adj_ptr));
    if (h.adj.empty()) h.adj.push_back(0); // a one-node mesh cannot occur (a cell has four vertices); keeps the pointer valid
    TB_TRY(upload(dev, h.adj, &e->d_adj));
    TB_HIP(hipMalloc((void **)&e->d_M, (size_t)e->n_cells * 6 * sizeof(double)));
    TB_HIP(hipMalloc((void **)&e->d_T2, (size_t)e->n * sizeof(double)));
    TB_HIP(hipMalloc((void **)&e->d_chg[0], (size_t)e->n));
    TB_HIP(hipMalloc((void **)&e->d_chg[1], (size_t)e->n));
    TB_HIP(hipMalloc((void **)&e->d_fixed, (size_t)e->n));
    TB_HIP(hipMemsetAsync(e->d_fixed, 0, (size_t)e->n, dev->stream));
    TB_HIP(hipMalloc((void **)&e->d_counts, 3 * EIK_CHECK_EVERY * sizeof(double)));
    TB_TRY(build_metric(e.get()));
#ifdef TB_ABLATION
    if (tune_env("TB_EIKONAL_LAYOUT") && !strcmp(tune_env("TB_EIKONAL_LAYOUT"), "table")) { // scripts/bench_eikonal.py: the per-tetrahedron table
        const int64_t nt = e->n_cells * e->ntet;
        TB_HIP(hipMalloc((void **)&e->d_tet6, (size_t)nt * 6 * sizeof(double)));
        if (hex) hipLaunchKernelGGL((k_eik_tet_table<6>), dim3(eik_grid(nt)), dim3(EIK_BLOCK), 0, dev->stream, nt, m->d_cell_dofs, e->d_x, e->d_M, e->d_tet6);
        else hipLaunchKernelGGL((k_eik_tet_table<1>), dim3(eik_grid(nt)), dim3(EIK_BLOCK), 0, dev->stream, nt, m->d_cell_dofs, e->d_x, e->d_M, e->d_tet6);
        TB_HIP(hipGetLastError());
    }
#endif
    *out = e.release();
    return TB_OK;
}

int tb_eikonal_destroy(tb_eikonal *e)
{
    free_eikonal(e);
    return TB_OK;
}

int tb_eikonal_solve(tb_eikonal *e, int64_t n_sources, const int32_t *source_nodes, const double *source_times, double rtol, int max_sweeps, double *d_T,
                     int *sweeps, int *converged)
{
    TB_REQUIRE(e && d_T && sweeps && converged, "tb_eikonal_solve: NULL argument");
    TB_REQUIRE(n_sources >= 1 && source_nodes && source_times, "tb_eikonal_solve: needs at least one source node (got %lld)", (long long)n_sources);
    TB_REQUIRE(rtol > 0.0 && rtol < 1.0, "tb_eikonal_solve: rtol = %g (needs 0 < rtol < 1)", rtol);
    TB_REQUIRE(max_sweeps >= 1, "tb_eikonal_solve: max_sweeps = %d (needs >= 1)", max_sweeps);
    TB_REQUIRE(n_sources <= e->n, "tb_eikonal_solve: %lld sources on %lld nodes", (long long)n_sources, (long long)e->n);
    {
        std::vector<int32_t> s(source_nodes, source_nodes + n_sources);
        std::sort(s.begin(), s.end());
        TB_REQUIRE(s.front() >= 0 && s.back() < e->n, "tb_eikonal_solve: source node %d outside [0, %lld)", s.front() < 0 ? s.front() : s.back(), (long long)e->n);
        for (size_t k = 1; k < s.size(); ++k) TB_REQUIRE(s[k] != s[k - 1], "tb_eikonal_solve: source node %d is listed twice", s[k]);
        for (int64_t k = 0; k < n_sources; ++k)
            TB_REQUIRE(source_times[k] >= 0.0 && source_times[k] < __builtin_huge_val(), "tb_eikonal_solve: source time %g of node %d (needs a finite time >= 0)",
                       source_times[k], source_nodes[k]);
    }
    tb_device *dev = e->mesh->dev;
    TB_NO_CAPTURE(dev); // reads the counts of changed nodes back
    TB_HIP(hipSetDevice(dev->id));
    *sweeps = 0; *converged = 0;
    if (n_sources > e->src_cap) {
        TB_HIP(hipStreamSynchronize(dev->stream));
        (void)hipFree(e->d_src); (void)hipFree(e->d_src_t);
        e->d_src = nullptr; e->d_src_t = nullptr; e->src_cap = 0;
        TB_HIP(hipMalloc((void **)&e->d_src, (size_t)n_sources * sizeof(int32_t)));
        TB_HIP(hipMalloc((void **)&e->d_src_t, (size_t)n_sources * sizeof(double)));
        e->src_cap = n_sources;
    }
    TB_HIP(hipMemcpyAsync(e->d_src, source_nodes, (size_t)n_sources * sizeof(int32_t), hipMemcpyHostToDevice, dev->stream));
    TB_HIP(hipMemcpyAsync(e->d_src_t, source_times, (size_t)n_sources * sizeof(double), hipMemcpyHostToDevice, dev->stream));
    TB_HIP(hipStreamSynchronize(dev->stream)); // the caller's arrays are free again
    hipLaunchKernelGGL(k_eik_init, dim3(eik_grid(e->n)), dim3(EIK_BLOCK), 0, dev->stream, e->n, d_T, e->d_chg[0], e->d_fixed);
    hipLaunchKernelGGL(k_eik_sources, dim3(eik_grid(n_sources)), dim3(EIK_BLOCK), 0, dev->stream, n_sources, e->d_src, e->d_src_t, d_T, e->d_chg[0], e->d_fixed);
    TB_HIP(hipGetLastError());
    // sweep s reads buffer s & 1 (0: d_T, 1: d_T2) and flag array s & 1, and writes the other ones
    double *buf[2] = {d_T, e->d_T2};
    int done = 0;
    bool conv = false;
    double h_counts[3 * EIK_CHECK_EVERY];
    e->last_counts[0] = e->last_counts[1] = e->last_counts[2] = 0;
    while (done < max_sweeps && !conv) {
        const int nb = std::min(EIK_CHECK_EVERY, max_sweeps - done);
        TB_HIP(hipMemsetAsync(e->d_counts, 0, sizeof(double) * 3 * EIK_CHECK_EVERY, dev->stream));
        for (int j = 0; j < nb; ++j) {
            const int s = done + j;
            if (e->ntet == 6) enqueue_sweep<6>(e, buf[s & 1], buf[(s & 1) ^ 1], s & 1, rtol);
            else enqueue_sweep<1>(e, buf[s & 1], buf[(s & 1) ^ 1], s & 1, rtol);
            fold_slots(dev, 0, e->d_counts + 3 * j, 3);
        }
        TB_HIP(hipGetLastError());
        TB_TRY(read_back(dev, h_counts, e->d_counts, (size_t)nb * 3));
        for (int j = 0; j < nb; ++j) {
            if (!conv && h_counts[3 * j] == 0.0) { conv = true; *sweeps = done + j + 1; }
            e->last_counts[0] += (int64_t)h_counts[3 * j + 1]; e->last_counts[1] += (int64_t)h_counts[3 * j]; e->last_counts[2] += (int64_t)h_counts[3 * j + 2];
        }
        done += nb;
    }
    if (!conv) *sweeps = done;
    *converged = conv ? 1 : 0;
    if (done & 1) TB_HIP(hipMemcpyAsync(d_T, e->d_T2, (size_t)e->n * sizeof(double), hipMemcpyDeviceToDevice, dev->stream)); // the latest buffer
    return TB_OK;
}

int tb_eikonal_last_counts(const tb_eikonal *e, int64_t *counts3)
{
    TB_REQUIRE(e && counts3, "tb_eikonal_last_counts: NULL argument");
    for (int k = 0; k < 3; ++k) counts3[k] = e->last_counts[k];
    return TB_OK;
}

int tb_eikonal_residual(tb_eikonal *e, const double *d_T, double *d_res)
{
    TB_REQUIRE(e && d_T && d_res, "tb_eikonal_residual: NULL argument");
    tb_device *dev = e->mesh->dev;
    if (e->ntet == 6)
        hipLaunchKernelGGL((k_eik_residual<6>), dim3(eik_grid(e->n)), dim3(EIK_BLOCK), 0, dev->stream, e->n, e->d_x, e->d_M, e->d_ptr, e->d_rec, e->d_fixed, d_T, d_res);
    else
        hipLaunchKernelGGL((k_eik_residual<1>), dim3(eik_grid(e->n)), dim3(EIK_BLOCK), 0, dev->stream, e->n, e->d_x, e->d_M, e->d_ptr, e->d_rec, e->d_fixed, d_T, d_res);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_eikonal_potential(tb_device *dev, int64_t n, const double *d_T, double t, int64_t n_samples, double t0, double dt, const double *d_template,
                         double *d_phi)
{
    TB_REQUIRE(dev && (n == 0 || (d_T && d_phi)) && d_template, "tb_eikonal_potential: NULL argument");
    TB_REQUIRE(n >= 0 && n_samples >= 2 && dt > 0.0, "tb_eikonal_potential: n = %lld, n_samples = %lld, dt = %g (needs n >= 0, at least two samples, dt > 0)",
               (long long)n, (long long)n_samples, dt);
    if (n == 0) return TB_OK;
    const double *ts = dev->capturing ? (dev->tslot_used = true, (const double *)dev->d_tslot) : (const double *)nullptr;
    hipLaunchKernelGGL(k_eik_potential, dim3(eik_grid(n)), dim3(EIK_BLOCK), 0, dev->stream, n, d_T, t, ts, n_samples, t0, dt, d_template, d_phi);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_host_eikonal_local_solve(const double *x4, const double *x123, const double *T123, const double *M6, double *value, double *lambda3)
{
    TB_REQUIRE(x4 && x123 && T123 && M6 && value, "tb_host_eikonal_local_solve: NULL argument");
    double Y[3][3], T[3];
    for (int i = 0; i < 3; ++i) {
        T[i] = T123[i];
        TB_REQUIRE(T[i] == T[i] && T[i] > -__builtin_huge_val(), "tb_host_eikonal_local_solve: T[%d] = %g (a time is finite or +inf)", i, T[i]);
        for (int d = 0; d < 3; ++d) Y[i][d] = x123[3 * i + d] - x4[d];
    }
    *value = eikonal_local_solve(Y, T, M6, lambda3);
    return TB_OK;
}

} // extern "C"

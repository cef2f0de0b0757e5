// tb_transfer.hip — point location in a mesh and evaluation of a nodal field at the located points, for gfx950.
//
// The device form of what the reference builds NodalIntergridInterpolation / transfer! on (src/ferrite-addons/transfer_operators.jl:20-161):
// Ferrite's PointEvalHandler (find, per point, a cell that contains it and the point's reference coordinates there) and evaluate_at_points
// (interpolate a field of the source DofHandler at those coordinates).  Ferrite is third party; the call sites are transfer_operators.jl:116 and :159-160.
//
// Search structure: a uniform grid of bins over the bounding box of the source nodes; bin b holds the CSR list binptr[b] … binptr[b + 1] of the cells
// whose axis-aligned box, widened by tol × its size, overlaps the bin.  Built on the device in three launches — count (one lane per cell, integer
// atomics), exclusive scan (one workgroup), fill (integer atomics again: the order inside a list is arbitrary, and nothing below depends on it).
// It depends on the source mesh alone and is kept when the points change (tb_locator_relocate).
//
// k_locate, one lane per point: walk the point's bin, reject by the widened cell box, invert the geometry map (affine tetrahedron: directly;
// trilinear hexahedron / bilinear quadrilateral: Newton from ξ = 0, ≤ 20 iterations, until ‖Δξ‖∞ < 1e-14), test containment within tol in reference
// coordinates and keep the LOWEST cell id among all containing candidates — the result does not depend on the list order, so it is the same in
// every run.  A candidate whose Jacobian is singular or inverted at an iterate does not contain the point.  Points in no cell get cell −1 and are
// counted through a reduction-slot group (tb_reduce.hpp), not one atomic address.
//
// k_evaluate, one lane per point, the per-time-step kernel: (cell, ξ) is what is stored per point — 28 B against 12·nb B of weights and dof ids —
// and the basis is recomputed in registers: out[idx(i, c)] = Σₐ Nₐ(ξᵢ) u[cell_dofs[cellᵢ, a·ncomp + c]], a = 0 … nb − 1 in that order (bit-identical
// between runs); NaN where the point has no cell.  Enqueue only: nothing is allocated, awaited or read back, so it may sit inside a graph capture.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "tb_elem.hpp"
#include "tb_internal.h"
#include "tb_reduce.hpp"

struct tb_locator {
    tb_mesh *from = nullptr;
    double tol = 0.0;
    // bins
    double lo[3] = {0, 0, 0}, inv_h[3] = {0, 0, 0};
    int nbin[3] = {1, 1, 1};
    int64_t nbins = 0, n_entries = 0;
    int32_t *d_count = nullptr;   // per bin: list length while building, zero afterwards
    int64_t *d_binptr = nullptr;  // nbins + 1
    int32_t *d_bincells = nullptr;
    double *d_cellbox = nullptr;  // per cell: lower corner, upper corner of its axis-aligned box (not widened)
    // points
    int64_t n_points = 0, capacity = 0, n_missing = 0;
    int32_t *d_cells = nullptr;   // per point: source cell, −1 = none
    double *d_xi = nullptr;       // per point: ξ[3]
    double *d_nmiss = nullptr;    // one double: where the slot group is folded
};

namespace tb {

struct BinGrid {
    double lo[3], inv_h[3];
    int nbin[3];
};

// bin index along direction d.  Monotone in x (one subtraction, one product, one truncation — no contraction possible), so a point inside a widened cell
// box lands between the bins of the box's two corners.  NaN goes to bin 0.
__device__ __forceinline__ int bin_coord(const BinGrid &g, int d, double x)
{
    const double t = (x - g.lo[d]) * g.inv_h[d];
    return t > 0.0 ? (t < (double)g.nbin[d] ? (int)t : g.nbin[d] - 1) : 0;
}

template <int KIND> struct GeomTraits;
template <> struct GeomTraits<TB_HEX8> { static constexpr int NV = 8, DIM = 3; };
template <> struct GeomTraits<TB_TET4> { static constexpr int NV = 4, DIM = 3; };
template <> struct GeomTraits<TB_QUAD4> { static constexpr int NV = 4, DIM = 2; };

// count (FILL = false: also computes and stores the cell boxes) and fill passes over the cells
template <int KIND, bool FILL>
__global__ void __launch_bounds__(256)
k_bin_cells(BinGrid g, int64_t n_cells, const double *__restrict__ xyz, const int32_t *__restrict__ conn, double tol, double *__restrict__ cellbox,
            int32_t *__restrict__ count, const int64_t *__restrict__ binptr, int32_t *__restrict__ bincells)
{
    constexpr int NV = GeomTraits<KIND>::NV, DIM = GeomTraits<KIND>::DIM;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    double lo[3], hi[3];
    if constexpr (!FILL) {
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            const double *x = xyz + 3 * (int64_t)conn[c * NV + a];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                lo[d] = a == 0 ? x[d] : fmin(lo[d], x[d]);
                hi[d] = a == 0 ? x[d] : fmax(hi[d], x[d]);
            }
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) { cellbox[6 * c + d] = lo[d]; cellbox[6 * c + 3 + d] = hi[d]; }
    } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) { lo[d] = cellbox[6 * c + d]; hi[d] = cellbox[6 * c + 3 + d]; }
    }
    int b0[3] = {0, 0, 0}, b1[3] = {0, 0, 0};
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        const double w = tol * (hi[d] - lo[d]);
        b0[d] = bin_coord(g, d, lo[d] - w);
        b1[d] = bin_coord(g, d, hi[d] + w);
    }
    for (int k = b0[2]; k <= b1[2]; ++k)
        for (int j = b0[1]; j <= b1[1]; ++j)
            for (int i = b0[0]; i <= b1[0]; ++i) {
                const int64_t b = ((int64_t)k * g.nbin[1] + j) * g.nbin[0] + i;
                const int32_t pos = atomicAdd(count + b, 1);
                if constexpr (FILL) {
                    const int64_t at = binptr[b] + pos;
                    if (at < binptr[b + 1]) bincells[at] = (int32_t)c; // the two passes see the same boxes, so the list is exactly full
                }
            }
}

// binptr = exclusive scan of count, count back to zero (the fill pass uses it as its cursors).  One workgroup: set-up code.
__global__ void __launch_bounds__(1024) k_bin_scan(int64_t nbins, int32_t *__restrict__ count, int64_t *__restrict__ binptr)
{
    __shared__ long long sm[1024];
    const int tid = threadIdx.x;
    const int64_t chunk = (nbins + 1023) / 1024;
    const int64_t j0 = (int64_t)tid * chunk < nbins ? (int64_t)tid * chunk : nbins, j1 = j0 + chunk < nbins ? j0 + chunk : nbins;
    long long s = 0;
    for (int64_t j = j0; j < j1; ++j) s += count[j];
    sm[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const long long v = tid >= off ? sm[tid - off] : 0;
        __syncthreads();
        sm[tid] += v;
        __syncthreads();
    }
    long long base = sm[tid] - s;
    for (int64_t j = j0; j < j1; ++j) {
        binptr[j] = base;
        base += count[j];
        count[j] = 0;
    }
    if (tid == 1023) binptr[nbins] = sm[1023];
}

// ---- inverse geometry maps: ξ with x(ξ) = p; false = the Jacobian was singular or inverted (at an iterate) ----
__device__ __forceinline__ bool invert_tet(const double (&X)[4][3], const double (&p)[3], double (&xi)[3])
{
    double J[3][3], r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        J[i][0] = X[1][i] - X[0][i]; J[i][1] = X[2][i] - X[0][i]; J[i][2] = X[3][i] - X[0][i];
        r[i] = p[i] - X[0][i];
    }
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    if (!(det > 0.0)) return false;
    const double id = 1.0 / det;
    xi[0] = (c00 * r[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r[1] + (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r[2]) * id;
    xi[1] = (c01 * r[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r[1] + (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r[2]) * id;
    xi[2] = (c02 * r[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r[2]) * id;
    return true;
}

constexpr int NEWTON_MAX = 20;
constexpr double NEWTON_STOP = 1e-14;

__device__ __forceinline__ bool invert_hex(const double (&X)[8][3], const double (&p)[3], double (&xi)[3])
{
    using E = tbk::Hex8<2>;
    xi[0] = xi[1] = xi[2] = 0.0;
    for (int it = 0; it < NEWTON_MAX; ++it) {
        double r[3] = {-p[0], -p[1], -p[2]}, J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const double f0 = 1.0 + E::sgn(a, 0) * xi[0], f1 = 1.0 + E::sgn(a, 1) * xi[1], f2 = 1.0 + E::sgn(a, 2) * xi[2];
            const double N = 0.125 * f0 * f1 * f2;
            const double d0 = 0.125 * E::sgn(a, 0) * f1 * f2, d1 = 0.125 * f0 * E::sgn(a, 1) * f2, d2 = 0.125 * f0 * f1 * E::sgn(a, 2);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                r[i] += N * X[a][i];
                J[i][0] += d0 * X[a][i]; J[i][1] += d1 * X[a][i]; J[i][2] += d2 * X[a][i];
            }
        }
        const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
        const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
        if (!(det > 0.0)) return false;
        const double id = 1.0 / det;
        const double dx0 = (c00 * r[0] + (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * r[1] + (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * r[2]) * id;
        const double dx1 = (c01 * r[0] + (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * r[1] + (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * r[2]) * id;
        const double dx2 = (c02 * r[0] + (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * r[1] + (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * r[2]) * id;
        xi[0] -= dx0; xi[1] -= dx1; xi[2] -= dx2;
        if (fmax(fabs(dx0), fmax(fabs(dx1), fabs(dx2))) < NEWTON_STOP) break;
    }
    return true;
}

__device__ __forceinline__ bool invert_quad(const double (&X)[4][3], const double (&p)[3], double (&xi)[3])
{
    using E = tbk::Quad4<2>;
    xi[0] = xi[1] = xi[2] = 0.0;
    for (int it = 0; it < NEWTON_MAX; ++it) {
        double r[2] = {-p[0], -p[1]}, J[2][2] = {{0, 0}, {0, 0}};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double f0 = 1.0 + E::sgn(a, 0) * xi[0], f1 = 1.0 + E::sgn(a, 1) * xi[1];
            const double N = 0.25 * f0 * f1, d0 = 0.25 * E::sgn(a, 0) * f1, d1 = 0.25 * f0 * E::sgn(a, 1);
#pragma unroll
            for (int i = 0; i < 2; ++i) { r[i] += N * X[a][i]; J[i][0] += d0 * X[a][i]; J[i][1] += d1 * X[a][i]; }
        }
        const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
        if (!(det > 0.0)) return false;
        const double id = 1.0 / det;
        const double dx0 = (J[1][1] * r[0] - J[0][1] * r[1]) * id, dx1 = (J[0][0] * r[1] - J[1][0] * r[0]) * id;
        xi[0] -= dx0; xi[1] -= dx1;
        if (fmax(fabs(dx0), fabs(dx1)) < NEWTON_STOP) break;
    }
    return true;
}

template <int KIND>
__global__ void __launch_bounds__(256)
k_locate(BinGrid g, const double *__restrict__ xyz, const int32_t *__restrict__ conn, const double *__restrict__ cellbox, const int64_t *__restrict__ binptr,
         const int32_t *__restrict__ bincells, int64_t n, const double *__restrict__ pts, double tol, int32_t *__restrict__ cells, double *__restrict__ xi_out,
         double *__restrict__ slots)
{
    constexpr int NV = GeomTraits<KIND>::NV, DIM = GeomTraits<KIND>::DIM;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double miss = 0.0;
    if (i < n) { // tail lanes stay for the workgroup sum below
        double p[3] = {pts[3 * i], pts[3 * i + 1], DIM == 3 ? pts[3 * i + 2] : 0.0};
        int bc[3] = {0, 0, 0};
#pragma unroll
        for (int d = 0; d < DIM; ++d) bc[d] = bin_coord(g, d, p[d]);
        const int64_t b = ((int64_t)bc[2] * g.nbin[1] + bc[1]) * g.nbin[0] + bc[0];
        int32_t best = 0x7fffffff;
        double bxi[3] = {0.0, 0.0, 0.0};
        for (int64_t k = binptr[b], ke = binptr[b + 1]; k < ke; ++k) {
            const int32_t c = bincells[k];
            if (c >= best) continue; // only a lower id can replace what was found
            const double *box = cellbox + 6 * (int64_t)c;
            bool out = false;
#pragma unroll
            for (int d = 0; d < DIM; ++d) {
                const double w = tol * (box[3 + d] - box[d]);
                out = out || p[d] < box[d] - w || p[d] > box[3 + d] + w;
            }
            if (out) continue;
            double X[NV][3], xi[3];
#pragma unroll
            for (int a = 0; a < NV; ++a) {
                const double *x = xyz + 3 * (int64_t)conn[(int64_t)c * NV + a];
                X[a][0] = x[0]; X[a][1] = x[1]; X[a][2] = x[2];
            }
            bool in;
            if constexpr (KIND == TB_TET4) {
                in = invert_tet(X, p, xi) && xi[0] >= -tol && xi[1] >= -tol && xi[2] >= -tol && xi[0] + xi[1] + xi[2] <= 1.0 + tol;
            } else if constexpr (KIND == TB_HEX8) {
                in = invert_hex(X, p, xi) && fabs(xi[0]) <= 1.0 + tol && fabs(xi[1]) <= 1.0 + tol && fabs(xi[2]) <= 1.0 + tol;
            } else {
                in = invert_quad(X, p, xi) && fabs(xi[0]) <= 1.0 + tol && fabs(xi[1]) <= 1.0 + tol;
            }
            if (in) { best = c; bxi[0] = xi[0]; bxi[1] = xi[1]; bxi[2] = xi[2]; }
        }
        const bool found = best != 0x7fffffff;
        cells[i] = found ? best : -1;
        xi_out[3 * i] = bxi[0]; xi_out[3 * i + 1] = bxi[1]; xi_out[3 * i + 2] = bxi[2];
        miss = found ? 0.0 : 1.0;
    }
    block_sum_slots(miss, slots); // a count below 2⁵³ is exact in a double
}

// ---- field bases at a run-time ξ, local order of include/tbhip.h ----
template <int KIND> struct FieldBasis;
template <> struct FieldBasis<TB_HEX8> {
    static constexpr int NB = 8;
    __device__ __forceinline__ static void eval(const double *xi, double (&N)[NB])
    {
        using E = tbk::Hex8<2>;
#pragma unroll
        for (int a = 0; a < 8; ++a) N[a] = 0.125 * (1.0 + E::sgn(a, 0) * xi[0]) * (1.0 + E::sgn(a, 1) * xi[1]) * (1.0 + E::sgn(a, 2) * xi[2]);
    }
};
template <> struct FieldBasis<TB_QUAD4> {
    static constexpr int NB = 4;
    __device__ __forceinline__ static void eval(const double *xi, double (&N)[NB])
    {
        using E = tbk::Quad4<2>;
#pragma unroll
        for (int a = 0; a < 4; ++a) N[a] = 0.25 * (1.0 + E::sgn(a, 0) * xi[0]) * (1.0 + E::sgn(a, 1) * xi[1]);
    }
};
template <> struct FieldBasis<TB_TET4> {
    static constexpr int NB = 4;
    __device__ __forceinline__ static void eval(const double *xi, double (&N)[NB])
    {
        N[0] = 1.0 - xi[0] - xi[1] - xi[2]; N[1] = xi[0]; N[2] = xi[1]; N[3] = xi[2];
    }
};
template <> struct FieldBasis<TB_HEX27> {
    static constexpr int NB = 27;
    __device__ __forceinline__ static void eval(const double *xi, double (&N)[NB])
    {
        using E = tbk::Hex27;
        double q[3][3];
#pragma unroll
        for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int k = 0; k < 3; ++k) q[d][k] = E::q1(k, xi[d]);
#pragma unroll
        for (int a = 0; a < 27; ++a) N[a] = q[0][E::tix(a, 0)] * q[1][E::tix(a, 1)] * q[2][E::tix(a, 2)];
    }
};
template <> struct FieldBasis<TB_TET10> {
    static constexpr int NB = 10;
    __device__ __forceinline__ static void eval(const double *xi, double (&N)[NB])
    {
        const double l[4] = {1.0 - xi[0] - xi[1] - xi[2], xi[0], xi[1], xi[2]};
#pragma unroll
        for (int v = 0; v < 4; ++v) N[v] = l[v] * (2.0 * l[v] - 1.0);
        N[4] = 4.0 * l[0] * l[1]; N[5] = 4.0 * l[1] * l[2]; N[6] = 4.0 * l[2] * l[0];
        N[7] = 4.0 * l[0] * l[3]; N[8] = 4.0 * l[1] * l[3]; N[9] = 4.0 * l[2] * l[3];
    }
};

template <int KIND, int NCOMP>
__global__ void __launch_bounds__(256)
k_evaluate(int64_t n, const int32_t *__restrict__ cells, const double *__restrict__ xis, const int32_t *__restrict__ cell_dofs, const double *__restrict__ u,
           double *__restrict__ out, const int32_t *__restrict__ scatter)
{
    constexpr int NB = FieldBasis<KIND>::NB;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t c = cells[i];
    double v[NCOMP];
    if (c < 0) {
#pragma unroll
        for (int k = 0; k < NCOMP; ++k) v[k] = __builtin_nan("");
    } else {
        const double xi[3] = {xis[3 * i], xis[3 * i + 1], xis[3 * i + 2]};
        double N[NB];
        FieldBasis<KIND>::eval(xi, N);
        const int32_t *dofs = cell_dofs + (int64_t)c * (NB * NCOMP);
#pragma unroll
        for (int k = 0; k < NCOMP; ++k) v[k] = 0.0;
#pragma unroll
        for (int a = 0; a < NB; ++a)
#pragma unroll
            for (int k = 0; k < NCOMP; ++k) v[k] += N[a] * u[dofs[a * NCOMP + k]];
    }
#pragma unroll
    for (int k = 0; k < NCOMP; ++k) {
        const int64_t at = scatter ? (int64_t)scatter[i * NCOMP + k] : i * NCOMP + k;
        out[at] = v[k];
    }
}

// ---- host side ----
static void free_locator(tb_locator *l)
{
    if (!l) return;
    for (void *p : {(void *)l->d_count, (void *)l->d_binptr, (void *)l->d_bincells, (void *)l->d_cellbox, (void *)l->d_cells, (void *)l->d_xi, (void *)l->d_nmiss}) (void)hipFree(p);
    delete l;
}

static BinGrid grid_of(const tb_locator *l)
{
    BinGrid g;
    for (int d = 0; d < 3; ++d) { g.lo[d] = l->lo[d]; g.inv_h[d] = l->inv_h[d]; g.nbin[d] = l->nbin[d]; }
    return g;
}

// Bin size: the edge of a cube (square) of the bounding box's volume (area) divided by the number of cells — one bin per cell on a box mesh, where a
// cell's box then touches two bins per direction and a bin lists about eight cells, all but the right one rejected by their boxes.  Never more
// than 2 · n_cells + 64 bins: a thin curved wall fills a small part of its bounding box, and its many empty bins cost 8 B each.
static void size_bins(tb_locator *l)
{
    const tb_mesh *m = l->from;
    const int dim = m->geom_kind == TB_QUAD4 ? 2 : 3;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int64_t v = 0; v < m->n_nodes; ++v)
        for (int d = 0; d < 3; ++d) {
            const double x = m->h_xyz[3 * v + d];
            lo[d] = v == 0 ? x : std::min(lo[d], x);
            hi[d] = v == 0 ? x : std::max(hi[d], x);
        }
    double vol = 1.0;
    int nd = 0;
    for (int d = 0; d < dim; ++d)
        if (hi[d] > lo[d]) { vol *= hi[d] - lo[d]; ++nd; }
    const int64_t nc = std::max<int64_t>(m->n_cells, 1), cap = 2 * nc + 64;
    double h = nd ? std::pow(vol / (double)nc, 1.0 / nd) : 1.0;
    for (;;) {
        int64_t total = 1;
        for (int d = 0; d < 3; ++d) {
            const double ext = d < dim ? hi[d] - lo[d] : 0.0;
            l->nbin[d] = ext > 0.0 ? (int)std::min(std::max(std::ceil(ext / h), 1.0), 1048576.0) : 1;
            total *= l->nbin[d];
        }
        if (total <= cap) { l->nbins = total; break; }
        h *= 1.25;
    }
    for (int d = 0; d < 3; ++d) {
        const double ext = d < dim ? hi[d] - lo[d] : 0.0;
        l->lo[d] = lo[d];
        l->inv_h[d] = ext > 0.0 ? (double)l->nbin[d] / ext : 0.0;
    }
}

template <int KIND>
static int build_bins(tb_locator *l)
{
    tb_mesh *m = l->from;
    tb_device *dev = m->dev;
    const BinGrid g = grid_of(l);
    TB_HIP(hipMalloc((void **)&l->d_count, (size_t)l->nbins * sizeof(int32_t)));
    TB_HIP(hipMalloc((void **)&l->d_binptr, (size_t)(l->nbins + 1) * sizeof(int64_t)));
    TB_HIP(hipMalloc((void **)&l->d_cellbox, (size_t)std::max<int64_t>(m->n_cells, 1) * 6 * sizeof(double)));
    TB_HIP(hipMemsetAsync(l->d_count, 0, (size_t)l->nbins * sizeof(int32_t), dev->stream));
    const unsigned grid = (unsigned)((m->n_cells + 255) / 256);
    if (grid) hipLaunchKernelGGL((k_bin_cells<KIND, false>), dim3(grid), dim3(256), 0, dev->stream, g, m->n_cells, m->d_xyz, m->d_conn, l->tol, l->d_cellbox, l->d_count, nullptr, nullptr);
    hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, dev->stream, l->nbins, l->d_count, l->d_binptr);
    TB_HIP(hipGetLastError());
    long long total = 0;
    static_assert(sizeof(long long) == sizeof(double), "read_back moves 8-byte words");
    TB_TRY(read_back(dev, (double *)&total, (const double *)(l->d_binptr + l->nbins), 1));
    l->n_entries = total;
    TB_HIP(hipMalloc((void **)&l->d_bincells, (size_t)std::max<int64_t>(total, 1) * sizeof(int32_t)));
    TB_HIP(hipMemsetAsync(l->d_bincells, 0, (size_t)std::max<int64_t>(total, 1) * sizeof(int32_t), dev->stream)); // every entry a valid cell id whatever happens
    if (grid) hipLaunchKernelGGL((k_bin_cells<KIND, true>), dim3(grid), dim3(256), 0, dev->stream, g, m->n_cells, m->d_xyz, m->d_conn, l->tol, l->d_cellbox, l->d_count, l->d_binptr, l->d_bincells);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

template <int KIND>
static void enqueue_locate(tb_locator *l, const double *d_points)
{
    tb_mesh *m = l->from;
    hipLaunchKernelGGL((k_locate<KIND>), dim3((unsigned)((l->n_points + 255) / 256)), dim3(256), 0, m->dev->stream, grid_of(l), m->d_xyz, m->d_conn, l->d_cellbox,
                       l->d_binptr, l->d_bincells, l->n_points, d_points, l->tol, l->d_cells, l->d_xi, red_group(m->dev, 0));
}

static int locate(tb_locator *l, int64_t n_points, const double *d_points)
{
    tb_mesh *m = l->from;
    tb_device *dev = m->dev;
    TB_HIP(hipSetDevice(dev->id));
    if (n_points > l->capacity) {
        TB_HIP(hipStreamSynchronize(dev->stream)); // an evaluation enqueued earlier may still read the old arrays
        (void)hipFree(l->d_cells); (void)hipFree(l->d_xi);
        l->d_cells = nullptr; l->d_xi = nullptr; l->capacity = 0;
        TB_HIP(hipMalloc((void **)&l->d_cells, (size_t)n_points * sizeof(int32_t)));
        TB_HIP(hipMalloc((void **)&l->d_xi, (size_t)n_points * 3 * sizeof(double)));
        l->capacity = n_points;
    }
    l->n_points = n_points;
    l->n_missing = 0;
    if (n_points == 0) return TB_OK;
    TB_HIP(hipMemsetAsync(l->d_nmiss, 0, sizeof(double), dev->stream));
    // slot group 0, like tb_dot and the chamber volume: every user runs on the device's stream and leaves the group zero
    if (m->geom_kind == TB_HEX8) enqueue_locate<TB_HEX8>(l, d_points);
    else if (m->geom_kind == TB_TET4) enqueue_locate<TB_TET4>(l, d_points);
    else enqueue_locate<TB_QUAD4>(l, d_points);
    TB_HIP(hipGetLastError());
    fold_slots(dev, 0, l->d_nmiss, 1);
    TB_HIP(hipGetLastError());
    double nm = 0.0;
    TB_TRY(read_back(dev, &nm, l->d_nmiss, 1));
    l->n_missing = (int64_t)nm;
    return TB_OK;
}

template <int KIND>
static void enqueue_evaluate(tb_locator *l, tb_mesh *f, const double *d_u, double *d_out, const int32_t *d_scatter)
{
    const dim3 grid((unsigned)((l->n_points + 255) / 256)), block(256);
    if (f->ncomp == 1)
        hipLaunchKernelGGL((k_evaluate<KIND, 1>), grid, block, 0, f->dev->stream, l->n_points, l->d_cells, l->d_xi, f->d_cell_dofs, d_u, d_out, d_scatter);
    else
        hipLaunchKernelGGL((k_evaluate<KIND, 3>), grid, block, 0, f->dev->stream, l->n_points, l->d_cells, l->d_xi, f->d_cell_dofs, d_u, d_out, d_scatter);
}

} // namespace tb

using namespace tb;

extern "C" {

int tb_locator_create(tb_mesh *from, int64_t n_points, const double *d_points, double tol, tb_locator **out)
{
    TB_REQUIRE(from && out && (d_points || n_points == 0), "tb_locator_create: NULL argument");
    *out = nullptr;
    TB_REQUIRE(n_points >= 0, "tb_locator_create: negative point count");
    TB_REQUIRE(tol >= 0.0 && tol < 1.0, "tb_locator_create: tol = %g (reference coordinates; 0 ≤ tol < 1)", tol);
    TB_REQUIRE(from->geom_kind == TB_HEX8 || from->geom_kind == TB_TET4 || from->geom_kind == TB_QUAD4, "tb_locator_create: geometry kind %d", from->geom_kind);
    TB_NO_CAPTURE(from->dev); // builds the bins and reads the number of missing points back
    TB_HIP(hipSetDevice(from->dev->id));
    std::unique_ptr<tb_locator, void (*)(tb_locator *)> l(new tb_locator, free_locator);
    l->from = from;
    l->tol = tol;
    size_bins(l.get());
    TB_HIP(hipMalloc((void **)&l->d_nmiss, sizeof(double)));
    if (from->geom_kind == TB_HEX8) TB_TRY(build_bins<TB_HEX8>(l.get()));
    else if (from->geom_kind == TB_TET4) TB_TRY(build_bins<TB_TET4>(l.get()));
    else TB_TRY(build_bins<TB_QUAD4>(l.get()));
    TB_TRY(locate(l.get(), n_points, d_points));
    *out = l.release();
    return TB_OK;
}

int tb_locator_relocate(tb_locator *l, int64_t n_points, const double *d_points)
{
    TB_REQUIRE(l && (d_points || n_points == 0), "tb_locator_relocate: NULL argument");
    TB_REQUIRE(n_points >= 0, "tb_locator_relocate: negative point count");
    TB_NO_CAPTURE(l->from->dev);
    return locate(l, n_points, d_points);
}

int tb_locator_destroy(tb_locator *l)
{
    free_locator(l);
    return TB_OK;
}

int64_t tb_locator_npoints(const tb_locator *l) { return l ? l->n_points : -1; }
int64_t tb_locator_nmissing(const tb_locator *l) { return l ? l->n_missing : -1; }
const int32_t *tb_locator_cells_device(const tb_locator *l) { return l ? l->d_cells : nullptr; }
const double *tb_locator_xi_device(const tb_locator *l) { return l ? l->d_xi : nullptr; }

int tb_locator_evaluate(tb_locator *l, tb_mesh *field_mesh, const double *d_u, double *d_out, const int32_t *d_scatter)
{
    TB_REQUIRE(l && field_mesh && d_u && d_out, "tb_locator_evaluate: NULL argument");
    TB_REQUIRE(field_mesh->dev == l->from->dev, "tb_locator_evaluate: the field's mesh lives on another device");
    TB_REQUIRE(field_mesh->geom_kind == l->from->geom_kind && field_mesh->n_cells == l->from->n_cells,
               "tb_locator_evaluate: the field's mesh (geometry kind %d, %lld cells) is not over the located grid (kind %d, %lld cells)", field_mesh->geom_kind,
               (long long)field_mesh->n_cells, l->from->geom_kind, (long long)l->from->n_cells);
    if (l->n_points == 0) return TB_OK;
    switch (field_mesh->field_kind) {
    case TB_HEX8: enqueue_evaluate<TB_HEX8>(l, field_mesh, d_u, d_out, d_scatter); break;
    case TB_QUAD4: enqueue_evaluate<TB_QUAD4>(l, field_mesh, d_u, d_out, d_scatter); break;
    case TB_TET4: enqueue_evaluate<TB_TET4>(l, field_mesh, d_u, d_out, d_scatter); break;
    case TB_HEX27: enqueue_evaluate<TB_HEX27>(l, field_mesh, d_u, d_out, d_scatter); break;
    case TB_TET10: enqueue_evaluate<TB_TET10>(l, field_mesh, d_u, d_out, d_scatter); break;
    default: set_error("tb_locator_evaluate: field kind %d", field_mesh->field_kind); return TB_ERR_BAD_ARG;
    }
    TB_HIP(hipGetLastError());
    return TB_OK;
}

} // extern "C"

// tb_interface.hip — diffusion across zero-thickness interface elements between two subdomains (InterfaceDiffusionModel /
// BilinearInterfaceDiffusionIntegrator, src/modeling/core/diffusion.jl:76-157): the jump–jump form  Kₑ[I, J] −= [[N_I]] G [[N_J]] dΓ.
//
// An interface element pairs the nf nodes of a facet of a cell of subdomain a (Ferrite's facet-node order) with their copies on a cell of
// subdomain b.  With N_k the first-order shape functions of the facet and F = G ∫ N_i N_j dΓ (nf × nf):
//   Kₑ[a_i, a_j] −= F[i][j]   Kₑ[b_i, b_j] −= F[i][j]   Kₑ[a_i, b_j] += F[i][j]   Kₑ[b_i, a_j] += F[i][j]
// dΓ is the average of the two sides' facet measures at the paired point (getdetJdV_average): |∂x/∂s × ∂x/∂t| of the bilinear facet on
// hexahedra, the edge length element on quadrilaterals.  Both sides are parametrised in a's facet-node order, so paired points coincide; the
// tensor Gauss rule is symmetric under the facet's symmetries, so F does not depend on which corner the parametrisation starts from.
//
// Two kernels, no floating-point atomics, no scratch memory:
//   k_interface_facet   one lane per (interface element, i, j): F[e][i][j] into the facet-matrix buffer
//   k_interface_gather  one lane per touched non-zero: its contributions summed in the planner's fixed order (ascending interface element, then
//                       local entry; tb_interface_planners.hpp), then added to the value array
// Surface work (interface elements ≪ cells): the aim is an ordered, bit-reproducible sum, not throughput.
#include <hip/hip_runtime.h>

#include <cmath>

#include "tb_internal.h"
#include "tb_facet_geom.hpp"
#include "tb_interface_planners.hpp"

namespace tb {

// facet nodes as local vertices: Ferrite.reference_facets(RefHexahedron) / (RefQuadrilateral), 0-based
static constexpr int HEX_FACET_NODES[6][4] = {{0, 3, 2, 1}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {0, 4, 7, 3}, {4, 5, 6, 7}};
static constexpr int QUAD_FACET_NODES[4][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}};

// corner k of the bilinear facet sits at (s, t) = (ss, st): (−1, −1), (1, −1), (1, 1), (−1, 1) — arithmetic, so a run-time k indexes nothing
__device__ inline double corner_s(int k) { return (k == 1 || k == 2) ? 1.0 : -1.0; }
__device__ inline double corner_t(int k) { return k >= 2 ? 1.0 : -1.0; }

template <int NF>
__device__ inline double facet_measure(const double (&x)[NF][3], double s, double t)
{
    if (NF == 2) { // edge: |dx/ds| of x(s) = ½(1 − s) x₀ + ½(1 + s) x₁
        const double d[3] = {0.5 * (x[1][0] - x[0][0]), 0.5 * (x[1][1] - x[0][1]), 0.5 * (x[1][2] - x[0][2])};
        return sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    }
    double a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const double ds = 0.25 * corner_s(k) * (1.0 + corner_t(k) * t), dt = 0.25 * corner_t(k) * (1.0 + corner_s(k) * s);
#pragma unroll
        for (int c = 0; c < 3; ++c) { a[c] += ds * x[k][c]; b[c] += dt * x[k][c]; }
    }
    const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    return sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
}

template <int NF>
__device__ inline double facet_shape(int k, double s, double t)
{
    if (NF == 2) return 0.5 * (1.0 + (k == 1 ? s : -s));
    return 0.25 * (1.0 + corner_s(k) * s) * (1.0 + corner_t(k) * t);
}

template <int NF>
__global__ void __launch_bounds__(256)
k_interface_facet(int64_t n, int fq, const double *__restrict__ xyz, const int32_t *__restrict__ nodes, const int32_t *__restrict__ cell_a, double G,
                  const double *__restrict__ Ge, double *__restrict__ fm, Status *st)
{
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= n * (NF * NF)) return;
    const int64_t e = tid / (NF * NF);
    const int ij = (int)(tid % (NF * NF)), i = ij / NF, j = ij % NF;
    double xa[NF][3], xb[NF][3];
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const int64_t va = nodes[e * (2 * NF) + k], vb = nodes[e * (2 * NF) + NF + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) { xa[k][c] = xyz[3 * va + c]; xb[k][c] = xyz[3 * vb + c]; }
    }
    const int nt = NF == 2 ? 1 : fq;
    double acc = 0.0;
    bool bad = false;
    for (int qt = 0; qt < nt; ++qt)
        for (int qs = 0; qs < fq; ++qs) {
            const double s = facet_gx(fq, qs), t = NF == 2 ? 0.0 : facet_gx(fq, qt);
            const double w = NF == 2 ? facet_gw(fq, qs) : facet_gw(fq, qs) * facet_gw(fq, qt);
            const double ma = facet_measure<NF>(xa, s, t), mb = facet_measure<NF>(xb, s, t);
            bad = bad || !(ma > 0.0 && ma < INFINITY) || !(mb > 0.0 && mb < INFINITY);
            acc += facet_shape<NF>(i, s, t) * facet_shape<NF>(j, s, t) * (0.5 * (ma + mb)) * w;
        }
    if (bad && ij == 0) { st->neg_detj = 1; st->cell = cell_a[e]; }
    fm[tid] = (Ge ? Ge[e] : G) * acc;
}

__global__ void __launch_bounds__(256)
k_interface_gather(int64_t n_touched, const int64_t *__restrict__ nzidx, const int64_t *__restrict__ ptr, const uint32_t *__restrict__ src,
                   const double *__restrict__ fm, double *__restrict__ nz)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_touched) return;
    double sum = 0.0;
    for (int64_t c = ptr[k]; c < ptr[k + 1]; ++c) {
        const uint32_t u = src[c];
        const double v = fm[u >> 1];
        sum += (u & 1u) ? -v : v;
    }
    nz[nzidx[k]] += sum; // one lane per non-zero: no other lane of this launch touches it
}

void free_interface_data(InterfaceData *d)
{
    if (!d) return;
    (void)hipFree(d->d_nodes); (void)hipFree(d->d_cell_a); (void)hipFree(d->d_G); (void)hipFree(d->d_fm);
    (void)hipFree(d->d_nz); (void)hipFree(d->d_ptr); (void)hipFree(d->d_src);
    d->d_nodes = d->d_cell_a = nullptr; d->d_G = d->d_fm = nullptr; d->d_nz = d->d_ptr = nullptr; d->d_src = nullptr;
}

// the contribution list of `pat`, built on the host seam and uploaded; kept until the form meets another pattern
static int ensure_interface_plan(tb_form *f, tb_pattern *pat)
{
    InterfaceData *d = f->iface.get();
    if (d->planned_for == pat->serial) return TB_OK;
    const plan::PatternView pv{pat->n_rows, pat->h_rowptr.data(), pat->h_colidx.data(), 0};
    ifplan::InterfaceHost h;
    TB_TRY(ifplan::contributions(d->n, d->nf, d->h_edofs.data(), pv, h));
    (void)hipFree(d->d_nz); (void)hipFree(d->d_ptr); (void)hipFree(d->d_src);
    d->d_nz = d->d_ptr = nullptr; d->d_src = nullptr; d->planned_for = 0;
    TB_TRY(upload_all(f->mesh->dev, h.nz, &d->d_nz, h.ptr, &d->d_ptr, h.src, &d->d_src));
    d->n_touched = (int64_t)h.nz.size();
    d->planned_for = pat->serial;
    return TB_OK;
}

} // namespace tb

using namespace tb;

extern "C" {

int tb_interface_form_create(tb_mesh *mesh, const int32_t *records, const int32_t *pairing, int64_t n, int facet_qpoints, double G,
                             const double *G_per_element, int index_base, tb_form **out)
{
    TB_REQUIRE(mesh && out && ((records && pairing) || n == 0), "tb_interface_form_create: NULL argument");
    *out = nullptr;
    TB_REQUIRE(n >= 0, "tb_interface_form_create: negative interface count");
    TB_REQUIRE(index_base == 0 || index_base == 1, "tb_interface_form_create: index_base must be 0 or 1");
    TB_REQUIRE(mesh->ncomp == 1 && ((mesh->geom_kind == TB_HEX8 && mesh->field_kind == TB_HEX8) || (mesh->geom_kind == TB_QUAD4 && mesh->field_kind == TB_QUAD4)),
               "tb_interface_form_create: needs a first-order scalar field on hexahedra or quadrilaterals");
    if (facet_qpoints == 0) facet_qpoints = 2; // max(2p − 1, 2) of the first-order field (src/discretization/fem.jl:52-55)
    TB_REQUIRE(facet_qpoints >= 1 && facet_qpoints <= 3, "tb_interface_form_create: 1…3 Gauss points per facet direction (got %d)", facet_qpoints);
    const bool hex = mesh->geom_kind == TB_HEX8;
    const int nf = hex ? 4 : 2, nlf = hex ? 6 : 4, nv = mesh->nverts;
    auto f = std::make_unique<tb_form>();
    f->mesh = mesh; f->kind = TB_FORM_INTERFACE;
    f->iface = std::make_unique<InterfaceData>();
    InterfaceData *d = f->iface.get();
    d->nf = nf; d->fq = facet_qpoints; d->n = n; d->G = G;
    d->h_edofs.resize((size_t)n * 2 * nf);
    std::vector<int32_t> nodes((size_t)n * 2 * nf), cells((size_t)n);
    for (int64_t e = 0; e < n; ++e) {
        const int64_t ca = (int64_t)records[4 * e] - index_base, cb = (int64_t)records[4 * e + 2] - index_base;
        const int la = records[4 * e + 1] - index_base, lb = records[4 * e + 3] - index_base;
        TB_REQUIRE(ca >= 0 && ca < mesh->n_cells && cb >= 0 && cb < mesh->n_cells && la >= 0 && la < nlf && lb >= 0 && lb < nlf,
                   "tb_interface_form_create: record %lld = (%d, %d, %d, %d) out of range", (long long)e, records[4 * e], records[4 * e + 1], records[4 * e + 2], records[4 * e + 3]);
        cells[(size_t)e] = (int32_t)ca;
        for (int k = 0; k < nf; ++k) {
            const int lva = hex ? HEX_FACET_NODES[la][k] : QUAD_FACET_NODES[la][k];
            const int lvb = pairing[e * nf + k] - index_base;
            TB_REQUIRE(lvb >= 0 && lvb < nv, "tb_interface_form_create: pairing %d of record %lld is no local vertex", pairing[e * nf + k], (long long)e);
            bool on_facet = false;
            for (int q = 0; q < nf; ++q) on_facet = on_facet || lvb == (hex ? HEX_FACET_NODES[lb][q] : QUAD_FACET_NODES[lb][q]);
            TB_REQUIRE(on_facet, "tb_interface_form_create: record %lld pairs local vertex %d of cell b, which is not on its local facet %d", (long long)e, lvb, lb);
            const int32_t va = mesh->h_conn[ca * nv + lva], vb = mesh->h_conn[cb * nv + lvb];
            double scale = 1.0, dist = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double xa = mesh->h_xyz[3 * (size_t)va + c], xb = mesh->h_xyz[3 * (size_t)vb + c];
                scale = std::max(scale, std::fabs(xa));
                dist = std::max(dist, std::fabs(xa - xb));
            }
            TB_REQUIRE(dist <= 1e-12 * scale, "tb_interface_form_create: record %lld: node %d of side a and its copy %d on side b do not coincide in space (distance %g)",
                       (long long)e, va, vb, dist);
            nodes[(size_t)e * 2 * nf + k] = va;
            nodes[(size_t)e * 2 * nf + nf + k] = vb;
            d->h_edofs[(size_t)e * 2 * nf + k] = mesh->h_cell_dofs[ca * mesh->ndpc + lva];      // first-order scalar field: local dof = local vertex
            d->h_edofs[(size_t)e * 2 * nf + nf + k] = mesh->h_cell_dofs[cb * mesh->ndpc + lvb];
        }
        for (int k = 0; k < 2 * nf; ++k)
            for (int q = 0; q < k; ++q)
                TB_REQUIRE(d->h_edofs[(size_t)e * 2 * nf + k] != d->h_edofs[(size_t)e * 2 * nf + q],
                           "tb_interface_form_create: record %lld lists dof %d twice (the two sides must not share nodes)", (long long)e, d->h_edofs[(size_t)e * 2 * nf + k]);
    }
    TB_HIP(hipSetDevice(mesh->dev->id));
    int rc = TB_OK;
    if (n > 0) {
        rc = upload_all(mesh->dev, nodes, &d->d_nodes, cells, &d->d_cell_a);
        if (!rc && G_per_element) rc = upload(mesh->dev, std::vector<double>(G_per_element, G_per_element + n), &d->d_G);
        if (!rc && hipMalloc((void **)&d->d_fm, sizeof(double) * (size_t)n * nf * nf) != hipSuccess) {
            (void)hipGetLastError();
            set_error("tb_interface_form_create: facet-matrix buffer (%zu B)", sizeof(double) * (size_t)n * nf * nf);
            rc = TB_ERR_NOMEM;
        }
    }
    if (rc) { free_interface_data(d); return rc; }
    *out = f.release();
    return TB_OK;
}

int tb_interface_assemble(tb_form *form, tb_pattern *pat, double *d_nzval)
{
    TB_REQUIRE(form && pat && (d_nzval || pat->nnz == 0), "tb_interface_assemble: NULL argument");
    TB_REQUIRE(form->kind == TB_FORM_INTERFACE && form->iface, "tb_interface_assemble: form is not an interface form");
    TB_REQUIRE(pat->mesh == form->mesh, "tb_interface_assemble: form and pattern belong to different meshes");
    InterfaceData *d = form->iface.get();
    if (d->n == 0) return TB_OK;
    tb_device *dev = form->mesh->dev;
    TB_HIP(hipSetDevice(dev->id));
    TB_TRY(ensure_interface_plan(form, pat));
    for (const double *&q : pat->mir_nz) if (q == d_nzval) q = nullptr; // the value array changes: its sliced mirror (tb_spmv_mirror) is stale
    TB_TRY(reset_status(dev));
    const int64_t lanes = d->n * d->nf * d->nf;
    if (d->nf == 4)
        hipLaunchKernelGGL((k_interface_facet<4>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, dev->stream, d->n, d->fq, form->mesh->d_xyz, d->d_nodes,
                           d->d_cell_a, d->G, d->d_G, d->d_fm, dev->d_status);
    else
        hipLaunchKernelGGL((k_interface_facet<2>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, dev->stream, d->n, d->fq, form->mesh->d_xyz, d->d_nodes,
                           d->d_cell_a, d->G, d->d_G, d->d_fm, dev->d_status);
    TB_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_interface_gather, dim3((unsigned)((d->n_touched + 255) / 256)), dim3(256), 0, dev->stream, d->n_touched, d->d_nz, d->d_ptr, d->d_src,
                       d->d_fm, d_nzval);
    TB_HIP(hipGetLastError());
    set_last_kernel("k_interface_facet<%d> + k_interface_gather", d->nf);
    return check_status(dev);
}

} // extern "C"

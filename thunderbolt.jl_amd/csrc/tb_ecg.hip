// tb_ecg.hip — the arithmetic of the pseudo-ECG (src/modeling/electrophysiology/ecg.jl) for gfx950: the fluxes κ∇φₘ at the quadrature points
// (compute_quadrature_fluxes!, ecg.jl:1-37), the Plonsey volume integral for a set of electrodes (evaluate_ecg, ecg.jl:80-137), the lead products
// −Z·(Kᵢφₘ) of the lead-field method (ecg.jl:617-619) and the NaN scrub both torso methods apply to their source (ecg.jl:345-347, 612).
//
// Points.  A cache numbers the quadrature points of its form's mesh p = cell · n_qp + q (first-order hexahedra: 8 points, tetrahedra: 4 — the rules of
// the diffusion assembly, tb_elem.hpp) and keeps two arrays: geo = {x̃, dΩ = detJ·w} (4 doubles, built once — the geometry does not change) and
// flux = κ∇φₘ (3 doubles), 56 bytes per point together.  Every kernel below that visits points runs ONE LANE PER POINT: consecutive lanes store
// consecutive 24- and 32-byte records (a lane per cell would store 192 bytes apart), the 8 (4) lanes of a cell load the same connectivity,
// coordinates and φ (one request per wave-instruction, served by L1), and the point's ∂N/∂ξ are formed from the bits of q — no table, no LDS.
//
// k_ecg_update:  flux[p] = Σᵢ (D(x_q)·∇Nᵢ) φ[dof(cell, i)], i = 0 … nb − 1 in that order; D multiplies from the LEFT (a non-symmetric constant
// tensor gives D·∇N, not ∇N·D).  D is the form's: its folded constant tensor or its table at the quadrature points (6 doubles, symmetric).
//
// k_ecg_evaluate<T>:  out[e] = −1/(4πκₜ) Σ_p flux[p]·(x̃_p − x_e)/‖x̃_p − x_e‖³ dΩ_p.  One pass over the points serves a register tile of T
// electrodes: a lane reads its point's 56 bytes once and adds to T accumulators; the electrode coordinates of the tile are the same in every lane
// (scalar registers).  More electrodes than T: blockIdx.y walks the tiles, each passing over the points again.  sqrt and the division are the
// correctly rounded ones (no fast-math in this library's flags) — the bare reciprocal-square-root approximation is never used.  A point that
// coincides with an electrode gives Inf / NaN exactly as in the reference: there is no guard.
//
// k_ecg_leads<T>:  out[i] = α Σⱼ Z[i·ldz + j] v[j], the same shape — one pass reads v once for a tile of T rows of Z.
//
// Reductions are ORDERED (the reference's test asserts == between two evaluations, test/integration/test_ecg.jl): no floating-point atomic anywhere,
// the reduction slots of tb_reduce.hpp included (their arrival order is free).  A workgroup sums its lanes by wave shuffles (a fixed xor tree),
// its four waves through LDS in wave order, and writes its partial sums with plain vector stores to ws[workgroup][output]; k_ecg_fold then adds
// the workgroups in index order, one wave per output, and applies the factor.  The grid is min(⌈n / 256⌉, 8 · CUs) — a function of the point
// count and the device alone — so two calls give identical bits.  The workspace belongs to the device (tb_device::d_ecg_ws), grows outside a
// graph capture only, and is shared by every cache: the calls of one device are ordered by its one stream.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tb_elem.hpp"
#include "tb_internal.h"

struct tb_ecg {
    tb_form *form = nullptr;
    tb_mesh *mesh = nullptr;
    int64_t n_points = 0;
    double *d_geo = nullptr;  // per point: x̃[3], dΩ
    double *d_flux = nullptr; // per point: κ∇φₘ[3]
};

namespace tb {

constexpr int ECG_BLOCK = 256;
constexpr int ECG_TILE = 16; // electrodes (rows of Z) per pass; 4, 8 and 16 were timed

// ---- reference element at a run-time point q (the point order and rules of tbk::Hex8<2> / tbk::Tet4<2>) ----
template <int KIND> struct EcgElem;
template <> struct EcgElem<TB_HEX8> {
    static constexpr int NV = 8, NQ = 8;
    __device__ __forceinline__ static double ref(int q, double (&N)[8], double (&dN)[8][3])
    {
        using E = tbk::Hex8<2>;
        constexpr double G = 0.5773502691896258;
        const double x0 = (q & 1) ? G : -G, x1 = (q & 2) ? G : -G, x2 = (q & 4) ? G : -G;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const double f0 = 1.0 + E::sgn(a, 0) * x0, f1 = 1.0 + E::sgn(a, 1) * x1, f2 = 1.0 + E::sgn(a, 2) * x2;
            N[a] = 0.125 * f0 * f1 * f2;
            dN[a][0] = 0.125 * E::sgn(a, 0) * f1 * f2; dN[a][1] = 0.125 * f0 * E::sgn(a, 1) * f2; dN[a][2] = 0.125 * f0 * f1 * E::sgn(a, 2);
        }
        return 1.0; // Gauss weights of the 2-point rule
    }
};
template <> struct EcgElem<TB_TET4> {
    static constexpr int NV = 4, NQ = 4;
    __device__ __forceinline__ static double ref(int q, double (&N)[4], double (&dN)[4][3])
    {
        constexpr double A = 0.5854101966249685, B = 0.1381966011250105;
        const double x0 = q == 1 ? A : B, x1 = q == 2 ? A : B, x2 = q == 3 ? A : B;
        N[0] = 1.0 - x0 - x1 - x2; N[1] = x0; N[2] = x1; N[3] = x2;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int d = 0; d < 3; ++d) dN[a][d] = a == 0 ? -1.0 : (a - 1 == d ? 1.0 : 0.0);
        return 1.0 / 24.0;
    }
};

// vertex coordinates of a cell, N and ∇N = ∂N/∂ξ·J⁻¹ (PR883.jl:253-263, 280-291) at point q; returns detJ · w
template <int KIND>
__device__ __forceinline__ double point_geometry(const double *__restrict__ xyz, const int32_t *__restrict__ conn, int64_t cell, int q,
                                                 double (&X)[EcgElem<KIND>::NV][3], double (&N)[EcgElem<KIND>::NV], double (&grad)[EcgElem<KIND>::NV][3])
{
    constexpr int NV = EcgElem<KIND>::NV;
    double dN[NV][3];
    const double w = EcgElem<KIND>::ref(q, N, dN);
    double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int a = 0; a < NV; ++a) {
        const double *x = xyz + 3 * (int64_t)conn[cell * NV + a];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            X[a][i] = x[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) J[i][k] += X[a][i] * dN[a][k];
        }
    }
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    const double id = 1.0 / det;
    double Ji[3][3];
    Ji[0][0] = c00 * id; Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id; Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
    Ji[1][0] = c01 * id; Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id; Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
    Ji[2][0] = c02 * id; Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id; Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
#pragma unroll
    for (int a = 0; a < NV; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) grad[a][k] = dN[a][0] * Ji[0][k] + dN[a][1] * Ji[1][k] + dN[a][2] * Ji[2][k];
    return det * w;
}

// x̃ and dΩ of every point (ecg.jl:127-132), once per cache; *bad = 1 + the highest cell with detJ ≤ 0 at some point (integer atomic)
template <int KIND>
__global__ void __launch_bounds__(ECG_BLOCK)
k_ecg_geometry(int64_t n_points, const double *__restrict__ xyz, const int32_t *__restrict__ conn, double *__restrict__ geo, unsigned long long *__restrict__ bad)
{
    constexpr int NV = EcgElem<KIND>::NV, NQ = EcgElem<KIND>::NQ;
    const int64_t p = (int64_t)blockIdx.x * ECG_BLOCK + threadIdx.x;
    if (p >= n_points) return;
    const int64_t cell = p / NQ;
    double X[NV][3], N[NV], grad[NV][3];
    const double dO = point_geometry<KIND>(xyz, conn, cell, (int)(p % NQ), X, N, grad);
    double xq[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < NV; ++a)
#pragma unroll
        for (int i = 0; i < 3; ++i) xq[i] += N[a] * X[a][i];
    reinterpret_cast<double4 *>(geo)[p] = make_double4(xq[0], xq[1], xq[2], dO);
    if (!(dO > 0.0)) atomicMax(bad, (unsigned long long)cell + 1ull);
}

struct EcgTensor {
    double D[9];        // the form's folded constant tensor, row-major
    const double *dtab; // or its table: 6 doubles (xx, xy, xz, yy, yz, zz) per point
};

template <int KIND, bool FIELD>
__global__ void __launch_bounds__(ECG_BLOCK)
k_ecg_update(int64_t n_points, const double *__restrict__ xyz, const int32_t *__restrict__ conn, const int32_t *__restrict__ cell_dofs, EcgTensor dt,
             const double *__restrict__ phi, double *__restrict__ flux)
{
    constexpr int NV = EcgElem<KIND>::NV, NQ = EcgElem<KIND>::NQ;
    const int64_t p = (int64_t)blockIdx.x * ECG_BLOCK + threadIdx.x;
    if (p >= n_points) return;
    const int64_t cell = p / NQ;
    double X[NV][3], N[NV], grad[NV][3];
    (void)point_geometry<KIND>(xyz, conn, cell, (int)(p % NQ), X, N, grad);
    double D[3][3];
    if constexpr (FIELD) {
        const double *dq = dt.dtab + p * 6;
        D[0][0] = dq[0]; D[0][1] = D[1][0] = dq[1]; D[0][2] = D[2][0] = dq[2];
        D[1][1] = dq[3]; D[1][2] = D[2][1] = dq[4]; D[2][2] = dq[5];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) D[i][j] = dt.D[3 * i + j];
    }
    double f[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < NV; ++a) { // ecg.jl:31-34: κ∇ucell[qp] += D_loc ⋅ ∇Nᵢ ⊗ uₑ[i]
        const double u = phi[cell_dofs[cell * NV + a]];
#pragma unroll
        for (int r = 0; r < 3; ++r) f[r] += (D[r][0] * grad[a][0] + D[r][1] * grad[a][1] + D[r][2] * grad[a][2]) * u;
    }
    flux[3 * p] = f[0]; flux[3 * p + 1] = f[1]; flux[3 * p + 2] = f[2];
}

// ---- ordered workgroup sum of T accumulators: xor tree inside a wave, the four waves in wave order, plain stores of the first `valid` sums ----
template <int T>
__device__ __forceinline__ void block_sum_store(double (&acc)[T], double *__restrict__ out, int64_t valid)
{
    __shared__ double sm[ECG_BLOCK / 64][T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        double v = acc[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < T && (int64_t)threadIdx.x < valid) out[threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

template <int T>
__global__ void __launch_bounds__(ECG_BLOCK)
k_ecg_evaluate(int64_t n_points, const double *__restrict__ flux, const double *__restrict__ geo, int64_t n_el, const double *__restrict__ x,
               double *__restrict__ ws)
{
    const int64_t e0 = (int64_t)blockIdx.y * T;
    double xe[T][3], acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) { // a tile that runs past the last electrode repeats it; those sums are not stored
        const int64_t e = e0 + t < n_el ? e0 + t : n_el - 1;
        xe[t][0] = x[3 * e]; xe[t][1] = x[3 * e + 1]; xe[t][2] = x[3 * e + 2];
        acc[t] = 0.0;
    }
    for (int64_t p = (int64_t)blockIdx.x * ECG_BLOCK + threadIdx.x; p < n_points; p += (int64_t)gridDim.x * ECG_BLOCK) {
        const double4 g = reinterpret_cast<const double4 *>(geo)[p];
        const double f0 = flux[3 * p], f1 = flux[3 * p + 1], f2 = flux[3 * p + 2];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const double d0 = g.x - xe[t][0], d1 = g.y - xe[t][1], d2 = g.z - xe[t][2];
            const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
            acc[t] += (f0 * d0 + f1 * d1 + f2 * d2) / (r2 * sqrt(r2)) * g.w; // ecg.jl:134
        }
    }
    block_sum_store<T>(acc, ws + (int64_t)blockIdx.x * n_el + e0, n_el - e0);
}

template <int T>
__global__ void __launch_bounds__(ECG_BLOCK)
k_ecg_leads(int64_t n, int64_t n_leads, const double *__restrict__ Z, int64_t ldz, const double *__restrict__ v, double *__restrict__ ws)
{
    const int64_t i0 = (int64_t)blockIdx.y * T;
    const double *row[T];
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        row[t] = Z + (i0 + t < n_leads ? i0 + t : n_leads - 1) * ldz;
        acc[t] = 0.0;
    }
    for (int64_t j = (int64_t)blockIdx.x * ECG_BLOCK + threadIdx.x; j < n; j += (int64_t)gridDim.x * ECG_BLOCK) {
        const double vj = v[j];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] += row[t][j] * vj;
    }
    block_sum_store<T>(acc, ws + (int64_t)blockIdx.x * n_leads + i0, n_leads - i0);
}

// out[k] = factor · (((ws[0][k] + ws[1][k]) + ws[2][k]) + …): the workgroups strictly in index order.  One wave per output: its lanes fetch 64
// consecutive partial sums with one load (the next 64 are requested before the current ones are added), and the running sum takes them lane by lane
// through scalar registers (v_readlane) — the order of a one-lane loop without its 2 048 dependent memory round trips.  Lanes behind the last
// workgroup hold +0.0.
__global__ void __launch_bounds__(64)
k_ecg_fold(int64_t n_groups, int64_t n_out, const double *__restrict__ ws, double factor, double *__restrict__ out)
{
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x;
    double s = 0.0;
    double v = lane < n_groups ? ws[(int64_t)lane * n_out + k] : 0.0;
    for (int64_t base = 0; base < n_groups; base += 64) {
        const int64_t gn = base + 64 + lane;
        const double vn = gn < n_groups ? ws[gn * n_out + k] : 0.0;
#pragma unroll
        for (int i = 0; i < 64; ++i) s += __shfl(v, i, 64);
        v = vn;
    }
    if (lane == 0) out[k] = factor * s;
}

__global__ void __launch_bounds__(ECG_BLOCK) k_scrub_scale(int64_t n, double alpha, double *__restrict__ x)
{
    const int64_t i = (int64_t)blockIdx.x * ECG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    x[i] = alpha * (v != v ? 0.0 : v);
}

// ---- host side ----
static unsigned ecg_grid(const tb_device *dev, int64_t n)
{
    const int64_t nb = (n + ECG_BLOCK - 1) / ECG_BLOCK, cap = (int64_t)std::max(dev->n_cu, 1) * 8;
    return (unsigned)std::max<int64_t>(1, std::min(nb, cap));
}

static int ecg_workspace(tb_device *dev, const char *who, size_t doubles, double **out)
{
    if (doubles > dev->ecg_ws_doubles) {
        if (dev->capturing) {
            set_error("%s: the reduction workspace would have to grow (%zu doubles, %zu held) while a graph capture is open - make the call once with these "
                      "sizes before tb_graph_begin", who, doubles, dev->ecg_ws_doubles);
            return TB_ERR_BAD_ARG;
        }
        TB_HIP(hipSetDevice(dev->id));
        TB_HIP(hipStreamSynchronize(dev->stream)); // a reduction enqueued earlier may still use the old block
        (void)hipFree(dev->d_ecg_ws);
        dev->d_ecg_ws = nullptr; dev->ecg_ws_doubles = 0;
        hipError_t e = hipMalloc((void **)&dev->d_ecg_ws, doubles * sizeof(double));
        if (e != hipSuccess) { (void)hipGetLastError(); set_error("%s: reduction workspace (%zu B): %s", who, doubles * sizeof(double), hipGetErrorString(e)); return TB_ERR_NOMEM; }
        dev->ecg_ws_doubles = doubles;
    }
    *out = dev->d_ecg_ws;
    return TB_OK;
}

static int ecg_tile()
{
#ifdef TB_ABLATION
    if (const char *s = tune_env("TB_ECG_TILE")) { const int t = atoi(s); if (t == 4 || t == 8 || t == 16) return t; }
#endif
    return ECG_TILE;
}

static void free_ecg(tb_ecg *e)
{
    if (!e) return;
    (void)hipFree(e->d_geo); (void)hipFree(e->d_flux);
    delete e;
}

template <int KIND>
static int build_geometry(tb_ecg *e)
{
    tb_mesh *m = e->mesh;
    tb_device *dev = m->dev;
    unsigned long long *d_bad = nullptr;
    TB_HIP(hipMalloc((void **)&d_bad, sizeof(unsigned long long)));
    std::unique_ptr<unsigned long long, void (*)(unsigned long long *)> hold(d_bad, [](unsigned long long *p) { (void)hipFree(p); });
    TB_HIP(hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), dev->stream));
    TB_HIP(hipMemsetAsync(e->d_flux, 0, (size_t)e->n_points * 3 * sizeof(double), dev->stream));
    hipLaunchKernelGGL((k_ecg_geometry<KIND>), dim3((unsigned)((e->n_points + ECG_BLOCK - 1) / ECG_BLOCK)), dim3(ECG_BLOCK), 0, dev->stream, e->n_points, m->d_xyz,
                       m->d_conn, e->d_geo, d_bad);
    TB_HIP(hipGetLastError());
    unsigned long long bad = 0;
    static_assert(sizeof(unsigned long long) == sizeof(double), "read_back moves 8-byte words");
    TB_TRY(read_back(dev, (double *)&bad, (const double *)d_bad, 1));
    if (bad) {
        set_error("detJ <= 0 in cell %lld (0-based)", (long long)bad - 1);
        return TB_ERR_NEG_DETJ;
    }
    return TB_OK;
}

template <int KIND>
static void enqueue_update(tb_ecg *e, const double *d_phi)
{
    tb_mesh *m = e->mesh;
    EcgTensor dt;
    for (int i = 0; i < 9; ++i) dt.D[i] = e->form->Dconst[i];
    dt.dtab = e->form->d_dtab;
    const dim3 grid((unsigned)((e->n_points + ECG_BLOCK - 1) / ECG_BLOCK)), block(ECG_BLOCK);
    if (e->form->field)
        hipLaunchKernelGGL((k_ecg_update<KIND, true>), grid, block, 0, m->dev->stream, e->n_points, m->d_xyz, m->d_conn, m->d_cell_dofs, dt, d_phi, e->d_flux);
    else
        hipLaunchKernelGGL((k_ecg_update<KIND, false>), grid, block, 0, m->dev->stream, e->n_points, m->d_xyz, m->d_conn, m->d_cell_dofs, dt, d_phi, e->d_flux);
}

} // namespace tb

using namespace tb;

extern "C" {

int tb_ecg_create(tb_form *diffusion, tb_ecg **out)
{
    TB_REQUIRE(diffusion && out, "tb_ecg_create: NULL argument");
    *out = nullptr;
    TB_REQUIRE(diffusion->kind == TB_FORM_DIFFUSION, "tb_ecg_create: form kind %d is not TB_FORM_DIFFUSION (the cache takes D and the quadrature of a diffusion form)",
               diffusion->kind);
    tb_mesh *m = diffusion->mesh;
    const bool hex = m->geom_kind == TB_HEX8 && m->field_kind == TB_HEX8, tet = m->geom_kind == TB_TET4 && m->field_kind == TB_TET4;
    if (!(hex || tet) || m->ncomp != 1 || diffusion->qorder != 2 || diffusion->has_cellset) {
        set_error("tb_ecg_create: geometry kind %d, field kind %d, %d component(s), quadrature order %d%s - the pseudo-ECG is built for scalar first-order fields on "
                  "TB_HEX8 and TB_TET4 meshes with the 2-point rule, over all cells", m->geom_kind, m->field_kind, m->ncomp, diffusion->qorder,
                  diffusion->has_cellset ? ", cell set" : "");
        return TB_ERR_UNSUPPORTED;
    }
    tb_device *dev = m->dev;
    TB_NO_CAPTURE(dev); // allocates, tabulates D on first use and reads the detJ flag back
    TB_HIP(hipSetDevice(dev->id));
    if (diffusion->field && !diffusion->d_dtab) TB_TRY(hex ? tabulate_diffusion_field(diffusion) : tabulate_diffusion_field_tet4(diffusion));
    std::unique_ptr<tb_ecg, void (*)(tb_ecg *)> e(new tb_ecg, free_ecg);
    e->form = diffusion;
    e->mesh = m;
    e->n_points = m->n_cells * (hex ? 8 : 4);
    TB_REQUIRE(e->n_points > 0, "tb_ecg_create: the mesh has no cells");
    TB_HIP(hipMalloc((void **)&e->d_geo, (size_t)e->n_points * 4 * sizeof(double)));
    TB_HIP(hipMalloc((void **)&e->d_flux, (size_t)e->n_points * 3 * sizeof(double)));
    TB_TRY(hex ? build_geometry<TB_HEX8>(e.get()) : build_geometry<TB_TET4>(e.get()));
    *out = e.release();
    return TB_OK;
}

int tb_ecg_destroy(tb_ecg *ecg)
{
    free_ecg(ecg);
    return TB_OK;
}

int64_t tb_ecg_npoints(const tb_ecg *ecg) { return ecg ? ecg->n_points : -1; }
const double *tb_ecg_fluxes_device(const tb_ecg *ecg) { return ecg ? ecg->d_flux : nullptr; }

int tb_ecg_update(tb_ecg *ecg, const double *d_phi)
{
    TB_REQUIRE(ecg && d_phi, "tb_ecg_update: NULL argument");
    if (ecg->mesh->geom_kind == TB_HEX8) enqueue_update<TB_HEX8>(ecg, d_phi);
    else enqueue_update<TB_TET4>(ecg, d_phi);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_ecg_evaluate(tb_ecg *ecg, int64_t n_electrodes, const double *d_x, double kappa_t, double *d_out)
{
    TB_REQUIRE(ecg && (n_electrodes == 0 || (d_x && d_out)), "tb_ecg_evaluate: NULL argument");
    TB_REQUIRE(n_electrodes >= 0, "tb_ecg_evaluate: negative electrode count");
    if (n_electrodes == 0) return TB_OK;
    tb_device *dev = ecg->mesh->dev;
    const int T = ecg_tile();
    TB_REQUIRE(n_electrodes <= (int64_t)65535 * T, "tb_ecg_evaluate: %lld electrodes (at most %d per call)", (long long)n_electrodes, 65535 * T);
    const unsigned gx = ecg_grid(dev, ecg->n_points);
    double *ws = nullptr;
    TB_TRY(ecg_workspace(dev, "tb_ecg_evaluate", (size_t)gx * (size_t)n_electrodes, &ws));
    const dim3 grid(gx, (unsigned)((n_electrodes + T - 1) / T)), block(ECG_BLOCK);
#ifdef TB_ABLATION
    if (T == 4) hipLaunchKernelGGL((k_ecg_evaluate<4>), grid, block, 0, dev->stream, ecg->n_points, ecg->d_flux, ecg->d_geo, n_electrodes, d_x, ws);
    else if (T == 8) hipLaunchKernelGGL((k_ecg_evaluate<8>), grid, block, 0, dev->stream, ecg->n_points, ecg->d_flux, ecg->d_geo, n_electrodes, d_x, ws);
    else
#endif
    hipLaunchKernelGGL((k_ecg_evaluate<ECG_TILE>), grid, block, 0, dev->stream, ecg->n_points, ecg->d_flux, ecg->d_geo, n_electrodes, d_x, ws);
    hipLaunchKernelGGL(k_ecg_fold, dim3((unsigned)n_electrodes), dim3(64), 0, dev->stream, (int64_t)gx, n_electrodes, ws,
                       -1.0 / (4.0 * 3.141592653589793 * kappa_t), d_out); // ecg.jl:97
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_ecg_leads(tb_device *dev, int64_t n_leads, int64_t n, const double *d_Z, int64_t ldz, const double *d_v, double alpha, double *d_out)
{
    TB_REQUIRE(dev && (n_leads == 0 || d_out) && (n_leads == 0 || n == 0 || (d_Z && d_v)), "tb_ecg_leads: NULL argument");
    TB_REQUIRE(n_leads >= 0 && n >= 0 && ldz >= n, "tb_ecg_leads: n_leads = %lld, n = %lld, ldz = %lld (needs ldz >= n >= 0)", (long long)n_leads, (long long)n, (long long)ldz);
    if (n_leads == 0) return TB_OK;
    const int T = ecg_tile();
    TB_REQUIRE(n_leads <= (int64_t)65535 * T, "tb_ecg_leads: %lld leads (at most %d per call)", (long long)n_leads, 65535 * T);
    const unsigned gx = ecg_grid(dev, n);
    double *ws = nullptr;
    TB_TRY(ecg_workspace(dev, "tb_ecg_leads", (size_t)gx * (size_t)n_leads, &ws));
    const dim3 grid(gx, (unsigned)((n_leads + T - 1) / T)), block(ECG_BLOCK);
#ifdef TB_ABLATION
    if (T == 4) hipLaunchKernelGGL((k_ecg_leads<4>), grid, block, 0, dev->stream, n, n_leads, d_Z, ldz, d_v, ws);
    else if (T == 8) hipLaunchKernelGGL((k_ecg_leads<8>), grid, block, 0, dev->stream, n, n_leads, d_Z, ldz, d_v, ws);
    else
#endif
    hipLaunchKernelGGL((k_ecg_leads<ECG_TILE>), grid, block, 0, dev->stream, n, n_leads, d_Z, ldz, d_v, ws);
    hipLaunchKernelGGL(k_ecg_fold, dim3((unsigned)n_leads), dim3(64), 0, dev->stream, (int64_t)gx, n_leads, ws, alpha, d_out);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int tb_scrub_scale(tb_device *dev, int64_t n, double alpha, double *d_x)
{
    TB_REQUIRE(dev && (d_x || n == 0), "tb_scrub_scale: NULL argument");
    TB_REQUIRE(n >= 0, "tb_scrub_scale: negative length");
    if (n == 0) return TB_OK;
    hipLaunchKernelGGL(k_scrub_scale, dim3((unsigned)((n + ECG_BLOCK - 1) / ECG_BLOCK)), dim3(ECG_BLOCK), 0, dev->stream, n, alpha, d_x);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

} // extern "C"

// tb_assembly.hip — scalar forms on first-order elements (trilinear hexahedra, linear tetrahedra, bilinear quadrilaterals) and the two
// dispatchers of scalar assembly, launch_assemble_matrix and launch_assemble_vector.
//  * element_matrix / element_source: Mₑ, Kₑ, bₑ of one cell by ONE THREAD, reference-element values as compile-time immediates (tb_elem.hpp);
//    k_tabulate_*: a nodal coefficient field evaluated once at the quadrature points.
//  * k_matrix_direct / k_vector_direct: atomic and per-colour scatter through the (cell, i, j) → nz map of ensure_emap; k_ea_gather: the
//    element strategy of vectors.
//  * k_matrix_patch / k_vector_patch: the GENERAL patch kernels — a workgroup owns the cells of one patch of the mesh's patch plan
//    (tb_plans.cpp) and the rows first touched by it, re-integrates the halo cells, sums every owned row in LDS (ds_add_f64) and stores each
//    nz / dof once.  They serve what the specialised patch kernels do not take.
//  * k_vector_hex8_patch: the source vector on trilinear hexahedra over the vector patch plan (the linear form bench.py times).
// Elsewhere: the sum-factorised hexahedron patch kernels (tb_patch_fused.hip), the tetrahedron patch kernel (tb_assembly_tet4.hip) and the
// forms on the triquadratic field (tb_assembly_q2.hip); the dispatchers below choose among them.
//
// Arithmetic restated from (paths relative to the Thunderbolt.jl v0.0.4 tree):
//   src/modeling/core/mass.jl:28-43, src/modeling/core/diffusion.jl:28-50 (+ src/utils.jl:409-410),
//   src/modeling/core/analytical_coefficient.jl:80-101, src/modeling/core/coefficients.jl:85-99,152-162,279-292,
//   src/modeling/microstructure.jl:136-138,176-187, src/utils.jl:131-139.
// The cell loop / scatter replaced here is FerriteOperators' (third party); its in-tree model is
// src/modeling/core/coordinate_systems.jl:145-171.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "tb_assembly_dev.hpp"
#include "tb_elem.hpp"
#include "tb_hex8_sumfac.hpp"
#include "tb_internal.h"

namespace tb {
using namespace tbk;

template <int NB> __host__ __device__ constexpr int sym_idx(int i, int j)
{
    return i <= j ? i * NB - (i * (i - 1)) / 2 + (j - i) : j * NB - (j * (j - 1)) / 2 + (i - j);
}

template <class E>
__device__ __forceinline__ void load_coords(const MeshView &m, int64_t cell, double (&x)[E::NV][3])
{
    int32_t nodes[E::NV];
    const int32_t *c = m.conn + cell * E::NV;
#pragma unroll
    for (int a = 0; a < E::NV; ++a) nodes[a] = c[a];
#pragma unroll
    for (int a = 0; a < E::NV; ++a) {
        const double *p = m.xyz + 3 * (int64_t)nodes[a];
        x[a][0] = p[0]; x[a][1] = p[1]; x[a][2] = p[2];
    }
}

// orthogonalize_system(f,s,n): normalise, then Gram–Schmidt (src/utils.jl:131-139)
__device__ __forceinline__ void orthonormal_frame(double (&f)[3], double (&s)[3], double (&n)[3])
{
    const double rf = 1.0 / sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    const double rs = 1.0 / sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    const double rn = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
    for (int d = 0; d < 3; ++d) { f[d] *= rf; s[d] *= rs; n[d] *= rn; }
    const double fs = f[0] * s[0] + f[1] * s[1] + f[2] * s[2];
#pragma unroll
    for (int d = 0; d < 3; ++d) s[d] -= fs * f[d];
    const double fn = f[0] * n[0] + f[1] * n[1] + f[2] * n[2];
    const double sn = s[0] * n[0] + s[1] * n[1] + s[2] * n[2];
#pragma unroll
    for (int d = 0; d < 3; ++d) n[d] = n[d] - fn * f[d] - sn * s[d];
}

// Kₑ / Mₑ of one cell.  SYM: upper triangle packed (requires symmetric D), else full row-major.
// Diffusion is evaluated in reference coordinates: with G = −dΩ·J⁻¹·D·J⁻ᵀ (3×3, per point),
//   Kₑ[i,j] += ∂Nⱼ/∂ξ · G · ∂Nᵢ/∂ξ   ( = −(∇Nⱼ·D·∇Nᵢ) dΩ with ∇N = ∂N/∂ξ·J⁻¹, diffusion.jl:44 / PR883.jl:287-290 ),
// so the mapped gradients are never materialised and ∂N/∂ξ stays a scalar-register operand.
template <class E, int FORM, bool FIELD, bool SYM>
__device__ __forceinline__ bool element_matrix(const double (&x)[E::NV][3], const FormArgs &fa, int64_t cell,
                                               double (&Ke)[SYM ? E::NB *(E::NB + 1) / 2 : E::NB * E::NB])
{
    constexpr int NB = E::NB;
    const Tables<E> &tb = g_tables<E>;
    GeoCoeffs<E> gc;
    geo_prepare(x, gc);
    bool ok = true;
#pragma unroll 1
    for (int q = 0; q < E::NQ; ++q) {
        Geom g;
        geometry_rt<E>(tb, q, gc, g);
        ok = ok && (g.dOmega > 0.0);
        if constexpr (FORM == TB_FORM_MASS) {
            double r = fa.rho;
            if constexpr (FIELD) {
                r = 0.0;
#pragma unroll
                for (int a = 0; a < NB; ++a) r += tb.N[q][a] * fa.field[cell * NB + a];
            }
            const double rw = r * g.dOmega;
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = SYM ? i : 0; j < NB; ++j)
                    Ke[SYM ? sym_idx<NB>(i, j) : i * NB + j] += rw * tb.NN[q][sym_idx<NB>(i, j)];
        } else {
            double D[3][3];
            if constexpr (FIELD) { // tabulated once by k_tabulate_spectral (below): 6 loads instead of 72 per point
                const double *dq = fa.dtab + (cell * E::NQ + q) * 6;
                D[0][0] = dq[0]; D[0][1] = D[1][0] = dq[1]; D[0][2] = D[2][0] = dq[2];
                D[1][1] = dq[3]; D[1][2] = D[2][1] = dq[4]; D[2][2] = dq[5];
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) D[i][j] = fa.D[3 * i + j];
            }
            // H = J⁻¹·D ;  G[m][n] = −dΩ · Σₗ H[m][l]·J⁻¹[n][l]
            double H[3][3], G[3][3];
            const double mw = -g.dOmega;
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int l = 0; l < 3; ++l) H[m][l] = g.Jinv[m][0] * D[0][l] + g.Jinv[m][1] * D[1][l] + g.Jinv[m][2] * D[2][l];
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int n = (SYM ? m : 0); n < 3; ++n)
                    G[m][n] = mw * (H[m][0] * g.Jinv[n][0] + H[m][1] * g.Jinv[n][1] + H[m][2] * g.Jinv[n][2]);
            if constexpr (SYM) { G[1][0] = G[0][1]; G[2][0] = G[0][2]; G[2][1] = G[1][2]; }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                double T[3]; // T = G · ∂Nᵢ/∂ξ
#pragma unroll
                for (int m = 0; m < 3; ++m) T[m] = G[m][0] * tb.dN[q][i][0] + G[m][1] * tb.dN[q][i][1] + G[m][2] * tb.dN[q][i][2];
#pragma unroll
                for (int j = SYM ? i : 0; j < NB; ++j) {
                    // three FMAs chained straight into the accumulator (a summed product would cost mul + 2 fma + add)
                    double &k = Ke[SYM ? sym_idx<NB>(i, j) : i * NB + j];
                    k += tb.dN[q][j][0] * T[0];
                    k += tb.dN[q][j][1] * T[1];
                    k += tb.dN[q][j][2] * T[2];
                }
            }
        }
    }
    return ok;
}

// evaluate_coefficient of a SpectralTensorCoefficient over an OrthotropicMicrostructureModel of nodal fields at every
// quadrature point of every cell (coefficients.jl:85-99,479-488; microstructure.jl:36-38,176-187; utils.jl:131-139):
// interpolate f, s, n, normalise, Gram–Schmidt, D = (λ₁ f⊗f + λ₂ s⊗s + λ₃ n⊗n)·scale.  The microstructure is data of the
// form (fixed at tb_form_create), so the table is built once; the assembly kernels then read 48 doubles per cell instead
// of 72 per quadrature point (the per-point gather made the fibre-field assembly 4× slower than the constant-tensor one).
template <class E>
__global__ void __launch_bounds__(256)
k_tabulate_spectral(const double *__restrict__ field, int64_t n_cells, double l0, double l1, double l2, double scale, double *__restrict__ dtab)
{
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_cells) return;
    constexpr int NB = E::NB;
    const Tables<E> &tb = g_tables<E>;
    double fc[NB * 9];
#pragma unroll
    for (int k = 0; k < NB * 9; ++k) fc[k] = field[cell * (NB * 9) + k];
#pragma unroll 1
    for (int q = 0; q < E::NQ; ++q) {
        double f[3] = {0, 0, 0}, s[3] = {0, 0, 0}, n[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < NB; ++a) {
            const double Na = tb.N[q][a];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                f[d] += Na * fc[9 * a + d];
                s[d] += Na * fc[9 * a + 3 + d];
                n[d] += Na * fc[9 * a + 6 + d];
            }
        }
        orthonormal_frame(f, s, n);
        double *o = dtab + (cell * E::NQ + q) * 6;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) o[k++] = (l0 * f[i] * f[j] + l1 * s[i] * s[j] + l2 * n[i] * n[j]) * scale;
    }
}

// same table for an isotropic heterogeneous conductivity κ(x)·I given as first-order nodal data per cell (FieldCoefficient)
template <class E>
__global__ void __launch_bounds__(256)
k_tabulate_isotropic(const double *__restrict__ field, int64_t n_cells, double scale, double *__restrict__ dtab)
{
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_cells) return;
    constexpr int NB = E::NB;
    const Tables<E> &tb = g_tables<E>;
    double fc[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) fc[k] = field[cell * NB + k];
    for (int q = 0; q < E::NQ; ++q) {
        double v = 0.0;
#pragma unroll
        for (int a = 0; a < NB; ++a) v += tb.N[q][a] * fc[a];
        v *= scale;
        double *o = dtab + (cell * E::NQ + q) * 6;
        o[0] = v; o[1] = 0.0; o[2] = 0.0; o[3] = v; o[4] = 0.0; o[5] = v;
    }
}

// bₑ[j] += f(x_q,t)·Nⱼ·dΩ  (analytical_coefficient.jl:89-99)
template <class E>
__device__ __forceinline__ bool element_source(const double (&x)[E::NV][3], const FormArgs &fa, int64_t cell, double (&be)[E::NB])
{
    const Tables<E> &tb = g_tables<E>;
    GeoCoeffs<E> gc;
    geo_prepare(x, gc);
    bool ok = true;
#pragma unroll 1
    for (int q = 0; q < E::NQ; ++q) {
        Geom g;
        geometry_rt<E>(tb, q, gc, g);
        ok = ok && (g.dOmega > 0.0);
        double xq[3];
        geo_position(gc, tb, q, xq);
        const double fw = eval_source(fa, xq, cell, q, E::NQ) * g.dOmega;
#pragma unroll
        for (int j = 0; j < E::NB; ++j) be[j] += fw * tb.N[q][j];
    }
    return ok;
}

// ------------------------------------------------------------------------------------------------
// scatter-map construction: emap[(i*ndpc+j)*n_cells + cell] = nz index of (dofs[i], dofs[j])
// ------------------------------------------------------------------------------------------------
template <class MapT>
__global__ void k_build_emap(const int32_t *__restrict__ cell_dofs, int64_t n_cells, int ndpc,
                             const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, MapT *__restrict__ emap,
                             Status *st)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_cells * ndpc) return;
    // lane ↔ cell (coalesced emap writes), i is the slow index
    const int64_t cell = tid % n_cells;
    const int i = (int)(tid / n_cells);
    const int32_t *d = cell_dofs + cell * ndpc;
    const int32_t row = d[i];
    const int64_t lo0 = rowptr[row], hi0 = rowptr[row + 1];
    for (int j = 0; j < ndpc; ++j) {
        const int32_t c = d[j];
        int64_t lo = lo0, hi = hi0;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (colidx[mid] < c) lo = mid + 1; else hi = mid;
        }
        if (lo >= hi0 || colidx[lo] != c) { st->pattern_missing = 1; st->cell = cell; lo = lo0; }
        emap[(int64_t)(i * ndpc + j) * n_cells + cell] = (MapT)lo;
    }
}

// ------------------------------------------------------------------------------------------------
// direct strategies (atomic / per-colour): one thread per cell
// ------------------------------------------------------------------------------------------------
template <class E, int FORM, bool FIELD, bool SYM, class MapT>
__global__ void __launch_bounds__(128)
k_matrix_direct(MeshView m, FormArgs fa, const MapT *__restrict__ emap, const int32_t *__restrict__ list, int64_t n,
                double *__restrict__ nz, int atomic, Status *st)
{
    constexpr int NB = E::NB;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n) return;
    const int64_t cell = list ? list[tid] : tid;
    double x[E::NV][3];
    load_coords<E>(m, cell, x);
    double Ke[SYM ? NB * (NB + 1) / 2 : NB * NB];
#pragma unroll
    for (int k = 0; k < (SYM ? NB * (NB + 1) / 2 : NB * NB); ++k) Ke[k] = 0.0;
    if (!element_matrix<E, FORM, FIELD, SYM>(x, fa, cell, Ke)) flag_neg_detj(st, cell);
    const MapT *mp = emap + cell;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const double v = Ke[SYM ? sym_idx<NB>(i, j) : i * NB + j];
            const int64_t k = (int64_t)mp[(int64_t)(i * NB + j) * m.n_cells];
            if (atomic) unsafeAtomicAdd(nz + k, v); else nz[k] += v;
        }
}

template <class E>
__global__ void __launch_bounds__(256)
k_vector_direct(MeshView m, FormArgs fa, const int32_t *__restrict__ list, int64_t n, double *__restrict__ b,
                double *__restrict__ ea, int mode /*0 atomic, 1 rmw, 2 store to ea*/, Status *st)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n) return;
    const int64_t cell = list ? list[tid] : tid;
    double x[E::NV][3];
    load_coords<E>(m, cell, x);
    double be[E::NB];
#pragma unroll
    for (int j = 0; j < E::NB; ++j) be[j] = 0.0;
    if (!element_source<E>(x, fa, cell, be)) flag_neg_detj(st, cell);
    const int32_t *d = m.cell_dofs + cell * E::NB;
#pragma unroll
    for (int j = 0; j < E::NB; ++j) {
        if (mode == 2) ea[cell * E::NB + j] = be[j];
        else if (mode == 0) unsafeAtomicAdd(b + d[j], be[j]);
        else b[d[j]] += be[j];
    }
}

// element-assembly gather: b[d] = Σ (in cell order) bₑ slots of dof d
__global__ void k_ea_gather(const int64_t *__restrict__ ptr, const int32_t *__restrict__ src, const double *__restrict__ ea,
                            int64_t ndofs, double *__restrict__ b)
{
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= ndofs) return;
    double s = 0.0;
    for (int64_t k = ptr[d]; k < ptr[d + 1]; ++k) s += ea[src[k]];
    b[d] = s;
}

// ------------------------------------------------------------------------------------------------
// PATCH strategy
// ------------------------------------------------------------------------------------------------
struct PatchView {
    const int64_t *elem_ptr, *row_ptr;
    const int32_t *elem_cell;
    const uint16_t *elem_lrow;
    const int32_t *row_dof;
    // matrix
    const RowDesc *row_desc;
    const uint16_t *elem_rowoff;
    const void *colpos;
    int lds_entries, max_rows;
};

constexpr int PATCH_MAX_THREADS = 512;
__device__ __forceinline__ double Ke_sink() { return 0.0; }

// One workgroup per patch, (about) one thread per element instance.
//   phase 0  zero the patch's row accumulators in LDS
//   phase 1  every thread integrates one cell and adds Kₑ into the owned rows (ds_add_f64); all scatter
//            metadata of a cell is one 16-B rowoff load + the colpos bytes, issued before the arithmetic
//   phase 2  each wave streams 64 rows: descriptors are loaded coalesced, broadcast with v_readlane, and
//            every row leaves as one contiguous store — each nz is written exactly once, no zero-fill pass
template <class E, int FORM, bool FIELD, bool SYM, class PosT>
__global__ void __launch_bounds__(PATCH_MAX_THREADS, 2)
k_matrix_patch(MeshView m, FormArgs fa, PatchView pv, double *__restrict__ nz, Status *st)
{
    constexpr int NB = E::NB;
    extern __shared__ double acc[];
    const int T = blockDim.x;
    const int64_t p = blockIdx.x;
    const int64_t e0 = pv.elem_ptr[p], e1 = pv.elem_ptr[p + 1];
    const int64_t r0 = pv.row_ptr[p], r1 = pv.row_ptr[p + 1];
    const int nrows = (int)(r1 - r0);
    const RowDesc last = pv.row_desc[r1 - 1];
    const int nacc = (int)(last.off + last.len);
    // first cell's connectivity / coordinates are requested before the LDS set-up so their latency hides behind it
    int64_t e = e0 + threadIdx.x;
    int64_t cell = 0;
    double x[E::NV][3];
    if (e < e1) { cell = pv.elem_cell[e]; load_coords<E>(m, cell, x); }
    // row descriptors live behind the accumulators: nz0[max_rows] (int64) then {off,len}[max_rows]
    int64_t *dnz = (int64_t *)(acc + pv.lds_entries);
    uint2 *dol = (uint2 *)(dnz + pv.max_rows);
    for (int k = threadIdx.x; k < nacc; k += T) acc[k] = 0.0;
    for (int s = threadIdx.x; s < nrows; s += T) {
        const RowDesc d = pv.row_desc[r0 + s];
        dnz[s] = d.nz0;
        dol[s] = make_uint2(d.off, d.len);
    }
    __syncthreads();

    while (e < e1) {
        // software pipeline: the next cell's coordinates travel while this one is integrated
        const int64_t en = e + T;
        const bool more = en < e1;
        int64_t celln = 0;
        double xn[E::NV][3];
        if (more) { celln = pv.elem_cell[en]; load_coords<E>(m, celln, xn); }
        // scatter metadata: independent of the arithmetic, so its latency hides behind it too
        uint16_t ro[NB];
        PosT cp[NB * NB];
        {
            const uint16_t *rp = pv.elem_rowoff + e * NB;
#pragma unroll
            for (int i = 0; i < NB; ++i) ro[i] = rp[i];
            const PosT *cpp = (const PosT *)pv.colpos + e * (NB * NB);
#pragma unroll
            for (int k = 0; k < NB * NB; ++k) cp[k] = cpp[k];
        }
        double Ke[SYM ? NB * (NB + 1) / 2 : NB * NB];
#pragma unroll
        for (int k = 0; k < (SYM ? NB * (NB + 1) / 2 : NB * NB); ++k) Ke[k] = 0.0;
#ifdef TB_ABLATION
        if (fa.debug & 4) Ke[0] = x[0][0] + x[E::NV - 1][2]; else
#endif
        if (!element_matrix<E, FORM, FIELD, SYM>(x, fa, cell, Ke)) flag_neg_detj(st, cell);
#ifdef TB_ABLATION
        if (!(fa.debug & 1))
#endif
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (ro[i] == 0xFFFF) continue;
            double *row = acc + ro[i];
#pragma unroll
            for (int j = 0; j < NB; ++j) unsafeAtomicAdd(row + cp[i * NB + j], Ke[SYM ? sym_idx<NB>(i, j) : i * NB + j]);
        }
        if (!more) break;
        e = en; cell = celln;
#pragma unroll
        for (int a_ = 0; a_ < E::NV; ++a_) { x[a_][0] = xn[a_][0]; x[a_][1] = xn[a_][1]; x[a_][2] = xn[a_][2]; }
    }
    __syncthreads();

#ifdef TB_ABLATION
    if (fa.debug & 1) { if (threadIdx.x == 0) nz[p] = acc[0] + Ke_sink(); }
    if (fa.debug & 2) return;
#endif
    // write-out: one row per half-wave, descriptors from LDS, several rows in flight per wave
    const int half = threadIdx.x >> 5, hl = threadIdx.x & 31, nhalves = T >> 5;
#pragma unroll 4
    for (int s = half; s < nrows; s += nhalves) {
        const int64_t g0 = dnz[s];
        const uint2 ol = dol[s];
        double *dst = nz + g0;
        for (uint32_t k = hl; k < ol.y; k += 32) dst[k] = acc[ol.x + k];
    }
}

template <class E>
__global__ void __launch_bounds__(PATCH_MAX_THREADS)
k_vector_patch(MeshView m, FormArgs fa, PatchView pv, double *__restrict__ b, Status *st)
{
    extern __shared__ double acc[];
    const int T = blockDim.x;
    const int64_t p = blockIdx.x;
    const int64_t e0 = pv.elem_ptr[p], e1 = pv.elem_ptr[p + 1];
    const int64_t r0 = pv.row_ptr[p], r1 = pv.row_ptr[p + 1];
    const int nrows = (int)(r1 - r0);
    int64_t e = e0 + threadIdx.x;
    int64_t cell = 0;
    double x[E::NV][3];
    if (e < e1) { cell = pv.elem_cell[e]; load_coords<E>(m, cell, x); }
    for (int k = threadIdx.x; k < nrows; k += T) acc[k] = 0.0;
    __syncthreads();
    while (e < e1) {
        const int64_t en = e + T;
        const bool more = en < e1;
        int64_t celln = 0;
        double xn[E::NV][3];
        if (more) { celln = pv.elem_cell[en]; load_coords<E>(m, celln, xn); }
        uint16_t lr[E::NB];
        const uint16_t *lp = pv.elem_lrow + e * E::NB;
#pragma unroll
        for (int j = 0; j < E::NB; ++j) lr[j] = lp[j];
        double be[E::NB];
#pragma unroll
        for (int j = 0; j < E::NB; ++j) be[j] = 0.0;
        if (!element_source<E>(x, fa, cell, be)) flag_neg_detj(st, cell);
#pragma unroll
        for (int j = 0; j < E::NB; ++j)
            if (lr[j] != 0xFFFF) unsafeAtomicAdd(&acc[lr[j]], be[j]);
        if (!more) break;
        e = en; cell = celln;
#pragma unroll
        for (int a_ = 0; a_ < E::NV; ++a_) { x[a_][0] = xn[a_][0]; x[a_][1] = xn[a_][1]; x[a_][2] = xn[a_][2]; }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < nrows; s += T) b[pv.row_dof[r0 + s]] = acc[s];
}

// ------------------------------------------------------------------------------------------------
// Linear form on trilinear hexahedra through the vector patch plan (tb_plans.cpp: ensure_vec_patch_plan): one workgroup per patch of up to
// 8×8×8 cells.  The patch's vertex coordinates arrive pre-gathered and coalesced, instances carry 8 patch-local node indices (16 B), bₑ comes
// from the sum-factorised routine, and the per-node sums are formed in LDS.  HALO: rows owned by the patch are complete (halo cells
// re-integrated) and stored once — deterministic, no zero-fill pass.  !HALO: own cells only, every touched node is added to the zeroed vector
// with one global atomic (1.4 per cell instead of the 8 of the one-thread-per-cell scatter, whose 3.4× HBM traffic this replaces).
// ------------------------------------------------------------------------------------------------
struct VecPatchView {
    const uint4 *hdr;
    const uint16_t *elem_ln;
    const int32_t *elem_cell;
    const double *pcoord;
    const int32_t *pdof;
    int max_nodes;
};

// KIND: the source kind (TB_SRC_*) is a template parameter — one closed form per instance, no branch per Gauss point — and the kind's time value is
// read once in front of the cell loop.  All eight instances fit four waves per SIMD (≤ 128 registers) without scratch memory: DESIGN.md §4.2.
template <bool HALO, int KIND>
__global__ void __launch_bounds__(256, 4)
k_vector_hex8_patch(FormArgs fa, VecPatchView pv, double *__restrict__ b, Status *st)
{
    extern __shared__ double lds[];
    // the patch's coordinates are requested before anything waits: NX values per thread (8×8×8 tiles: ≤ 1043 nodes); larger patches fetch their
    // surplus in place.  Nothing else is carried across the cell loop: an instance's node indices are read when its trip starts and again for its
    // scatter (16 B from the cache), the dof ids at the flush — at four waves per SIMD (128 registers) the integration has none to spare for them.
    constexpr int T = 256, NX = 13;
    const int tid = threadIdx.x;
    const uint4 h = pv.hdr[blockIdx.x];
    const int64_t e0 = h.x, n0 = h.y;
    const int nrows = (int)(h.z & 0xffff), nnodes = (int)(h.z >> 16), ne = (int)h.w;
    double *acc = lds;                 // one sum per patch node
    double *xs = lds + pv.max_nodes;   // 3 per patch node
    const uint4 *eln = (const uint4 *)pv.elem_ln + e0;
    const double *pc = pv.pcoord + 3 * n0;
    double xc[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) xc[j] = tid + j * T < 3 * nnodes ? pc[tid + j * T] : 0.0;
    const int32_t *pd = pv.pdof + n0;
    for (int k = tid; k < nnodes; k += T) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < NX; ++j) if (tid + j * T < 3 * nnodes) xs[tid + j * T] = xc[j];
    for (int k = tid + NX * T; k < 3 * nnodes; k += T) xs[k] = pc[k];
    const double tv = source_time<KIND>(fa);
    __syncthreads();
    // HALO: every wave makes every trip (base < ne is uniform) and the waves add their cells' contributions in turn, a barrier between two turns: the
    // sum of a node is then taken in one order — trip, wave, the LDS unit's own order inside one instruction — and two launches give the same bits.
    // !HALO ends in global atomics, whose order is free anyway: its waves run unordered.
#pragma unroll 1
    for (int ei = tid; HALO ? ei - tid < ne : ei < ne; ei += T) {
        const bool on = !HALO || ei < ne;
        double be[8];
        if (on) {
            const uint4 l4 = eln[ei];
            const uint32_t ln[8] = {l4.x & 0xffffu, l4.x >> 16, l4.y & 0xffffu, l4.y >> 16, l4.z & 0xffffu, l4.z >> 16, l4.w & 0xffffu, l4.w >> 16};
            double x[8][3];
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const double *px = xs + 3 * ln[a];
                x[a][0] = px[0]; x[a][1] = px[1]; x[a][2] = px[2];
            }
            int64_t cell = 0;
            if constexpr (KIND == TB_SRC_TABULATED) cell = pv.elem_cell[e0 + ei];
            if (!hex8_sf_source(x, [&](int q, const double(&xq)[3]) { return eval_source_k<KIND>(fa, tv, xq, cell, q, 8); }, be)) flag_neg_detj(st, pv.elem_cell[e0 + ei]);
        }
        auto scatter = [&]() {
            // second read of the indices (the index is made opaque, or the compiler keeps the first read's four registers alive through the integration)
            int es = ei;
            asm volatile("" : "+v"(es));
            const uint4 s4 = eln[es];
            const uint32_t sn[8] = {s4.x & 0xffffu, s4.x >> 16, s4.y & 0xffffu, s4.y >> 16, s4.z & 0xffffu, s4.z >> 16, s4.w & 0xffffu, s4.w >> 16};
#pragma unroll
            for (int a = 0; a < 8; ++a)
                if (!HALO || sn[a] < (uint32_t)nrows) unsafeAtomicAdd(acc + sn[a], be[a]);
        };
        if constexpr (HALO) {
#pragma unroll 1
            for (int w = 0; w < T / 64; ++w) {
                if (on && (tid >> 6) == w) scatter();
                __syncthreads();
            }
        } else {
            scatter();
        }
    }
    if constexpr (!HALO) __syncthreads(); // (HALO: the last turn ended with one)
    for (int k = tid; k < nrows; k += T) {
        if (HALO) b[pd[k]] = acc[k];
        else unsafeAtomicAdd(b + pd[k], acc[k]);
    }
}

// (Round 6: a persistent, ticket-dealt streaming form of this kernel — next patch's inputs requested at the start of a patch's flush — was built and
// measured: 0.333 against 0.334–0.339 ms at 216³, 0.077 against 0.059 ms on the 27-layer slab, where its 768 long-lived workgroups balance worse than
// 2 460 short ones.  Removed; profiles/r06_v1/ab_stream_source_cpu16.log, ab_slab27_persistent_kernels.log.)

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
int ensure_emap(tb_pattern *p)
{
    if (p->d_emap) return TB_OK;
    tb_mesh *m = p->mesh;
    tb_device *dev = m->dev;
    const int64_t n = m->n_cells * m->ndpc;
    p->map64 = p->nnz >= (int64_t)0x7fffffff;
    const size_t bytes = (size_t)m->n_cells * m->ndpc * m->ndpc * (p->map64 ? 8 : 4);
    TB_HIP(hipMalloc(&p->d_emap, bytes));
    int rc = reset_status(dev);
    if (rc) return rc;
    if (p->map64)
        hipLaunchKernelGGL(k_build_emap<int64_t>, dim3(nblocks(n, 256)), dim3(256), 0, dev->stream, m->d_cell_dofs, m->n_cells,
                           m->ndpc, p->d_rowptr, p->d_colidx, (int64_t *)p->d_emap, dev->d_status);
    else
        hipLaunchKernelGGL(k_build_emap<int32_t>, dim3(nblocks(n, 256)), dim3(256), 0, dev->stream, m->d_cell_dofs, m->n_cells,
                           m->ndpc, p->d_rowptr, p->d_colidx, (int32_t *)p->d_emap, dev->d_status);
    TB_HIP(hipGetLastError());
    return check_status(dev);
}

static PatchView make_patch_view(const tb_mesh *m, const tb_pattern *p)
{
    const PatchPlan *pp = m->patches.get();
    PatchView v{};
    v.elem_ptr = pp->d_elem_ptr; v.row_ptr = pp->d_row_ptr; v.elem_cell = pp->d_elem_cell;
    v.elem_lrow = pp->d_elem_lrow; v.row_dof = pp->d_row_dof;
    if (p) {
        const PatchMatPlan *pm = p->patch_mat.get();
        v.row_desc = pm->d_row_desc;
        v.elem_rowoff = pm->d_elem_rowoff;
        v.colpos = pm->d_colpos8 ? (const void *)pm->d_colpos8 : (const void *)pm->d_colpos16;
        v.lds_entries = pm->max_lds_entries;
        v.max_rows = pp->max_rows;
    }
    return v;
}

template <class E, int FORM, bool FIELD, bool SYM>
static int run_matrix(tb_form *f, tb_pattern *p, int strategy, double t, double *d_nz)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    const MeshView mv = make_view(m);
    const FormArgs fa = make_args(f, t);
    if (strategy == TB_STRATEGY_PATCH) {
        { int rc = ensure_patch_plans(m, p); if (rc) return rc; }
        const PatchView pv = make_patch_view(m, p);
        const size_t lds = (size_t)p->patch_mat->max_lds_entries * sizeof(double) + (size_t)m->patches->max_rows * 16;
        const int T = m->patches->threads;
        auto launch = [&](auto k) -> int {
            TB_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k, dim3((unsigned)m->patches->n_patches), dim3(T), lds, dev->stream, mv, fa, pv, d_nz, dev->d_status);
            return TB_OK;
        };
        int rc;
        if (p->patch_mat->d_colpos8) rc = launch(k_matrix_patch<E, FORM, FIELD, SYM, uint8_t>);
        else rc = launch(k_matrix_patch<E, FORM, FIELD, SYM, uint16_t>);
        if (rc) return rc;
        TB_HIP(hipGetLastError());
        return TB_OK;
    }
    { int rc = ensure_emap(p); if (rc) return rc; }
    TB_HIP(hipMemsetAsync(d_nz, 0, (size_t)p->nnz * sizeof(double), dev->stream));
    auto go = [&](const int32_t *list, int64_t n, int atomic) -> int {
        if (n == 0) return TB_OK;
        if (p->map64)
            hipLaunchKernelGGL((k_matrix_direct<E, FORM, FIELD, SYM, int64_t>), dim3(nblocks(n, 128)), dim3(128), 0, dev->stream, mv, fa,
                               (const int64_t *)p->d_emap, list, n, d_nz, atomic, dev->d_status);
        else
            hipLaunchKernelGGL((k_matrix_direct<E, FORM, FIELD, SYM, int32_t>), dim3(nblocks(n, 128)), dim3(128), 0, dev->stream, mv, fa,
                               (const int32_t *)p->d_emap, list, n, d_nz, atomic, dev->d_status);
        TB_HIP(hipGetLastError());
        return TB_OK;
    };
    if (strategy == TB_STRATEGY_ATOMIC) return go(nullptr, m->n_cells, 1);
    if (strategy == TB_STRATEGY_PER_COLOR) {
        if (!m->colors) { int rc = build_color_plan(m); if (rc) return rc; }
        for (int c = 0; c < m->colors->ncolors; ++c) {
            int rc = go(m->colors->d_cells + m->colors->offsets[c], m->colors->offsets[c + 1] - m->colors->offsets[c], 0);
            if (rc) return rc;
        }
        return TB_OK;
    }
    set_error("matrix assembly: strategy %d not supported (use ATOMIC, PER_COLOR or PATCH)", strategy);
    return TB_ERR_UNSUPPORTED;
}

// first assembly of a diffusion form with a nodal coefficient field: tabulate the tensor at the quadrature points (the microstructure
// is data of the form, fixed at tb_form_create) and drop the nodal frames (5.8 GB at 10 M cells)
template <class E>
static int tabulate_diffusion_field_t(tb_form *f)
{
    tb_mesh *m = f->mesh;
    const size_t bytes = sizeof(double) * (size_t)m->n_cells * E::NQ * 6;
    hipError_t e = hipMalloc((void **)&f->d_dtab, bytes);
    if (e != hipSuccess) { set_error("diffusion tensor table (%zu B): %s", bytes, hipGetErrorString(e)); return TB_ERR_NOMEM; }
    const double sc = f->coef.wrap ? 1.0 / (f->coef.Cm * f->coef.chi) : 1.0;
    if (f->coef.kind == TB_COEF_FIELD_SCALAR)
        hipLaunchKernelGGL((k_tabulate_isotropic<E>), dim3(nblocks(m->n_cells, 256)), dim3(256), 0, m->dev->stream, f->d_field, m->n_cells, sc, f->d_dtab);
    else
        hipLaunchKernelGGL((k_tabulate_spectral<E>), dim3(nblocks(m->n_cells, 256)), dim3(256), 0, m->dev->stream, f->d_field, m->n_cells, f->coef.p[0],
                           f->coef.p[1], f->coef.p[2], sc, f->d_dtab);
    TB_HIP(hipGetLastError());
    TB_SYNC_STREAM(m->dev);
    (void)hipFree(f->d_field); f->d_field = nullptr;
    return TB_OK;
}
int tabulate_diffusion_field(tb_form *f) { return tabulate_diffusion_field_t<Hex8<2>>(f); } // for tb_patch_fused.hip, tb_ecg.hip
int tabulate_diffusion_field_tet4(tb_form *f) { return tabulate_diffusion_field_t<Tet4<2>>(f); } // for tb_ecg.hip
int tabulate_diffusion_field_q2(tb_form *f) { return tabulate_diffusion_field_t<Hex8<3>>(f); } // for tb_assembly_q2.hip: first-order nodal data at the 27 points

template <class E, int FORM>
static int run_matrix_coef(tb_form *f, tb_pattern *p, int strategy, double t, double *d_nz)
{
    if (f->field && FORM == TB_FORM_DIFFUSION && !f->d_dtab) { int rc = tabulate_diffusion_field_t<E>(f); if (rc) return rc; }
    if (f->field) return run_matrix<E, FORM, true, true>(f, p, strategy, t, d_nz);
    if (FORM == TB_FORM_DIFFUSION && !f->symmetric) return run_matrix<E, FORM, false, false>(f, p, strategy, t, d_nz);
    return run_matrix<E, FORM, false, true>(f, p, strategy, t, d_nz);
}

template <class E>
static int run_matrix_form(tb_form *f, tb_pattern *p, int strategy, double t, double *d_nz)
{
    if (f->kind == TB_FORM_MASS) return run_matrix_coef<E, TB_FORM_MASS>(f, p, strategy, t, d_nz);
    return run_matrix_coef<E, TB_FORM_DIFFUSION>(f, p, strategy, t, d_nz);
}

// vertex coordinates per cell, cell-major: one coalesced load for the workgroup-per-cell kernels (tb_assembly_q2.hip, the mechanics units)
__global__ void k_cell_xyz(const int32_t *__restrict__ conn, const double *__restrict__ xyz, int64_t n, int nverts, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; // (cell, vertex, component)
    if (i < n * nverts * 3) out[i] = xyz[3 * (int64_t)conn[i / 3] + i % 3];
}

int ensure_cell_xyz(tb_mesh *m)
{
    if (m->d_cell_xyz) return TB_OK;
    const int64_t n = m->n_cells * m->nverts * 3;
    TB_HIP(hipMalloc((void **)&m->d_cell_xyz, sizeof(double) * n));
    hipLaunchKernelGGL(k_cell_xyz, dim3(nblocks(n, 256)), dim3(256), 0, m->dev->stream, m->d_conn, m->d_xyz, m->n_cells, m->nverts, m->d_cell_xyz);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int launch_assemble_matrix(tb_form *f, tb_pattern *p, int strategy, double t, double *d_nz)
{
    tb_mesh *m = f->mesh;
    int rc = reset_status(m->dev);
    if (rc) return rc;
    // ElementAssemblyStrategy on first-order fields: what the reference's strategy guarantees for a matrix is element contributions summed in a
    // fixed order, no atomics, bit-reproducible (src/Thunderbolt.jl:22-32; FerriteOperators' element assembly).  The patch kernels do not give
    // that (their LDS row accumulators take the ≤ 8 contributions of a non-zero with ds_add_f64 from four waves: the order follows the wave
    // scheduling), the per-colour kernels do: cells of one colour share no dof, so every non-zero receives at most one plain read-modify-write per
    // colour and the colours run in sequence on the stream — the sum of a non-zero is taken in colour order, every time.
    if (strategy == TB_STRATEGY_ELEMENT && m->field_kind != TB_HEX27) strategy = TB_STRATEGY_PER_COLOR;
    if (strategy == TB_STRATEGY_PATCH && hex8_patch_applicable(f, p)) {
        rc = f->kind == TB_FORM_DIFFUSION ? launch_assemble_hex8_patch(f, nullptr, p, t, d_nz, nullptr) : launch_assemble_hex8_patch(nullptr, f, p, t, nullptr, d_nz);
        if (rc != TB_ERR_UNSUPPORTED) return rc; // e.g. rows longer than 255 entries: the general patch kernel below
        rc = reset_status(m->dev);
        if (rc) return rc;
    }
    if (strategy == TB_STRATEGY_PATCH && tet4_patch_applicable(f, p)) {
        rc = f->kind == TB_FORM_DIFFUSION ? launch_assemble_tet4_patch(f, nullptr, p, t, d_nz, nullptr) : launch_assemble_tet4_patch(nullptr, f, p, t, nullptr, d_nz);
        if (rc != TB_ERR_UNSUPPORTED) return rc;
        rc = reset_status(m->dev);
        if (rc) return rc;
    }
    if (m->field_kind == TB_HEX8 && f->qorder == 2) rc = run_matrix_form<Hex8<2>>(f, p, strategy, t, d_nz);
    else if (m->field_kind == TB_TET4 && f->qorder == 2) rc = run_matrix_form<Tet4<2>>(f, p, strategy, t, d_nz);
    else if (m->field_kind == TB_QUAD4 && f->qorder == 2) rc = run_matrix_form<Quad4<2>>(f, p, strategy, t, d_nz);
    else if (m->field_kind == TB_HEX27 && f->qorder == 3) rc = launch_q2_matrix(f, p, strategy, t, d_nz);
    else {
        set_error("matrix assembly: field kind %d with quadrature order %d not implemented", m->field_kind, f->qorder);
        return TB_ERR_UNSUPPORTED;
    }
    if (rc) return rc;
    return check_status(m->dev);
}

// One instance of the hexahedron source kernel per (HALO, kind).  Its dynamic LDS is 32 B per patch node, which the plan bounds by a third of a CU's
// 160 KiB (ensure_vec_patch_plan) — below the 64 KiB a kernel may ask for without raising its limit, so no attribute call sits on the launch path.
template <bool HALO, int KIND>
static int launch_vector_hex8_patch_inst(int64_t n_patches, size_t lds, tb_device *dev, const FormArgs &fa, const VecPatchView &pv, double *d_b)
{
    hipLaunchKernelGGL((k_vector_hex8_patch<HALO, KIND>), dim3((unsigned)n_patches), dim3(256), lds, dev->stream, fa, pv, d_b, dev->d_status);
    TB_HIP(hipGetLastError());
    return TB_OK;
}
template <int KIND>
static int launch_vector_hex8_patch(bool halo, int64_t n_patches, size_t lds, tb_device *dev, const FormArgs &fa, const VecPatchView &pv, double *d_b)
{
    return halo ? launch_vector_hex8_patch_inst<true, KIND>(n_patches, lds, dev, fa, pv, d_b) : launch_vector_hex8_patch_inst<false, KIND>(n_patches, lds, dev, fa, pv, d_b);
}

template <class E>
static int run_vector(tb_form *f, int strategy, double t, double *d_b)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    const MeshView mv = make_view(m);
    const FormArgs fa = make_args(f, t);
    static const bool legacy_vec = tune_env("TB_VECTOR_KERNEL") && !strcmp(tune_env("TB_VECTOR_KERNEL"), "legacy");
    if constexpr (std::is_same<E, Hex8<2>>::value) {
        if (!legacy_vec && !f->has_cellset && (strategy == TB_STRATEGY_PATCH || strategy == TB_STRATEGY_ATOMIC)) {
            const bool halo = strategy == TB_STRATEGY_PATCH;
            int rc = ensure_vec_patch_plan(m, halo);
            if (rc == TB_OK) {
                const VecPatchPlan *vp = m->vpatches[halo].get();
                const VecPatchView pv{(const uint4 *)vp->d_hdr, vp->d_elem_ln, vp->d_elem_cell, vp->d_pcoord, vp->d_pdof, vp->max_nodes};
                const size_t lds = (size_t)vp->max_nodes * 4 * sizeof(double);
                if (!halo) TB_HIP(hipMemsetAsync(d_b, 0, (size_t)m->ndofs * sizeof(double), dev->stream));
                rc = fa.src_kind == TB_SRC_CONST         ? launch_vector_hex8_patch<TB_SRC_CONST>(halo, vp->n_patches, lds, dev, fa, pv, d_b)
                     : fa.src_kind == TB_SRC_NORM_PLUS_T ? launch_vector_hex8_patch<TB_SRC_NORM_PLUS_T>(halo, vp->n_patches, lds, dev, fa, pv, d_b)
                     : fa.src_kind == TB_SRC_COS_EXP     ? launch_vector_hex8_patch<TB_SRC_COS_EXP>(halo, vp->n_patches, lds, dev, fa, pv, d_b)
                     : fa.src_kind == TB_SRC_TABULATED   ? launch_vector_hex8_patch<TB_SRC_TABULATED>(halo, vp->n_patches, lds, dev, fa, pv, d_b)
                                                         : TB_ERR_BAD_ARG;
                if (rc == TB_ERR_BAD_ARG) set_error("vector assembly: unknown source kind %d", fa.src_kind);
                return rc;
            }
            if (rc != TB_ERR_UNSUPPORTED) return rc; // unsupported layouts: the general kernels below
        }
    }
    if (strategy == TB_STRATEGY_PATCH) {
        { int rc = ensure_patch_plans(m, nullptr); if (rc) return rc; }
        const PatchView pv = make_patch_view(m, nullptr);
        const int T = m->patches->threads;
        hipLaunchKernelGGL((k_vector_patch<E>), dim3((unsigned)m->patches->n_patches), dim3(T),
                           (size_t)m->patches->max_rows * sizeof(double), dev->stream, mv, fa, pv, d_b, dev->d_status);
        TB_HIP(hipGetLastError());
        return TB_OK;
    }
    if (strategy == TB_STRATEGY_ELEMENT) {
        if (!m->ea) { int rc = build_ea_plan(m); if (rc) return rc; }
        hipLaunchKernelGGL((k_vector_direct<E>), dim3(nblocks(m->n_cells, 256)), dim3(256), 0, dev->stream, mv, fa,
                           (const int32_t *)nullptr, m->n_cells, d_b, m->ea->d_ea, 2, dev->d_status);
        TB_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ea_gather, dim3(nblocks(m->ndofs, 256)), dim3(256), 0, dev->stream, m->ea->d_ptr, m->ea->d_src,
                           m->ea->d_ea, m->ndofs, d_b);
        TB_HIP(hipGetLastError());
        return TB_OK;
    }
    TB_HIP(hipMemsetAsync(d_b, 0, (size_t)m->ndofs * sizeof(double), dev->stream));
    if (strategy == TB_STRATEGY_ATOMIC) {
        hipLaunchKernelGGL((k_vector_direct<E>), dim3(nblocks(m->n_cells, 256)), dim3(256), 0, dev->stream, mv, fa,
                           (const int32_t *)nullptr, m->n_cells, d_b, (double *)nullptr, 0, dev->d_status);
        TB_HIP(hipGetLastError());
        return TB_OK;
    }
    if (strategy == TB_STRATEGY_PER_COLOR) {
        if (!m->colors) { int rc = build_color_plan(m); if (rc) return rc; }
        for (int c = 0; c < m->colors->ncolors; ++c) {
            const int64_t n = m->colors->offsets[c + 1] - m->colors->offsets[c];
            if (!n) continue;
            hipLaunchKernelGGL((k_vector_direct<E>), dim3(nblocks(n, 256)), dim3(256), 0, dev->stream, mv, fa,
                               (const int32_t *)(m->colors->d_cells + m->colors->offsets[c]), n, d_b, (double *)nullptr, 1, dev->d_status);
            TB_HIP(hipGetLastError());
        }
        return TB_OK;
    }
    set_error("vector assembly: unknown strategy %d", strategy);
    return TB_ERR_UNSUPPORTED;
}

int launch_assemble_vector(tb_form *f, int strategy, double t, double *d_b)
{
    tb_mesh *m = f->mesh;
    int rc = reset_status(m->dev);
    if (rc) return rc;
    if (m->ncomp != 1) { set_error("source assembly needs a scalar field"); return TB_ERR_UNSUPPORTED; }
    if (m->field_kind == TB_HEX8 && f->qorder == 2) rc = run_vector<Hex8<2>>(f, strategy, t, d_b);
    else if (m->field_kind == TB_HEX8 && f->qorder == 3) rc = run_vector<Hex8<3>>(f, strategy, t, d_b);
    else if (m->field_kind == TB_TET4 && f->qorder == 2) rc = run_vector<Tet4<2>>(f, strategy, t, d_b);
    else if (m->field_kind == TB_QUAD4 && f->qorder == 2) rc = run_vector<Quad4<2>>(f, strategy, t, d_b);
    else if (m->field_kind == TB_HEX27 && f->qorder == 3) rc = launch_q2_vector(f, strategy, t, d_b);
    else {
        set_error("vector assembly: field kind %d with quadrature order %d not implemented", m->field_kind, f->qorder);
        return TB_ERR_UNSUPPORTED;
    }
    if (rc) return rc;
    return check_status(m->dev);
}

} // namespace tb

// tb_assembly.hip — gfx950 element-integration kernels: mass / diffusion matrices scattered into CSR and
// the analytical-source vector, in four scatter strategies (atomic, per-colour, element-assembly, patch).
//
// Arithmetic restated from (paths relative to the Thunderbolt.jl v0.0.4 tree):
//   src/modeling/core/mass.jl:28-43, src/modeling/core/diffusion.jl:28-50 (+ src/utils.jl:409-410),
//   src/modeling/core/analytical_coefficient.jl:80-101, src/modeling/core/coefficients.jl:85-99,152-162,279-292,
//   src/modeling/microstructure.jl:136-138,176-187, src/utils.jl:131-139.
// The cell loop / scatter replaced here is FerriteOperators' (third party); its in-tree model is
// src/modeling/core/coordinate_systems.jl:145-171.
//
// Design notes:
//  * one THREAD per cell, Kₑ kept symmetric-packed in registers; all reference-element values are
//    compile-time immediates (tb_elem.hpp), so the only global reads are connectivity, coordinates and
//    the scatter metadata.  FP64 MFMA runs at the FP64 vector rate on CDNA4, so the Kₑ contraction stays
//    on the VALU.
//  * PATCH strategy: a workgroup owns a Morton-compact patch of cells and the rows first touched by it;
//    it recomputes the halo cells, accumulates every owned row in LDS (ds_add_f64) and writes each
//    nz / dof exactly once with row-contiguous stores — no global atomics, no zero-fill pass.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>

#include "tb_elem.hpp"
#include "tb_forms.hpp"
#include "tb_hex8_sumfac.hpp"
#include "tb_internal.h"
#include "tb_math.hpp"

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

// The four source kinds, the kind known at compile time: the one definition of each closed form.  tv is the kind's time value — t for
// norm_plus_t, cos(2πt) for cos_exp (source_time below), unused by the other two.
template <int KIND>
__device__ __forceinline__ double eval_source_k(const FormArgs &fa, double tv, const double (&xq)[3], int64_t cell, int q, int nq)
{
    static_assert(KIND == TB_SRC_CONST || KIND == TB_SRC_NORM_PLUS_T || KIND == TB_SRC_COS_EXP || KIND == TB_SRC_TABULATED, "unknown source kind");
    if constexpr (KIND == TB_SRC_CONST) return fa.p0;
    else if constexpr (KIND == TB_SRC_NORM_PLUS_T) return sqrt(xq[0] * xq[0] + xq[1] * xq[1] + xq[2] * xq[2]) + tv;
    else if constexpr (KIND == TB_SRC_COS_EXP) // cos(2πt)·exp(−‖x‖²) (benchmarks-cuda-linear-form.jl:15-18); ct = cos(2πt) is uniform in space: evaluated once on the host.
        // ‖x‖² is formed directly (the square of a square root differs from it by ≤ 2 ulp) and the exponential is the bounded-argument one.
        return tv * exp_b(-(xq[0] * xq[0] + xq[1] * xq[1] + xq[2] * xq[2]));
    else return fa.table[cell * nq + q];
}

// time value of a kind: from the device slot when replayed from a graph, else the launch's own scalars
template <int KIND>
__device__ __forceinline__ double source_time(const FormArgs &fa)
{
    if constexpr (KIND == TB_SRC_NORM_PLUS_T) return fa.tslot ? fa.tslot[0] : fa.t;
    else if constexpr (KIND == TB_SRC_COS_EXP) return fa.tslot ? fa.tslot[1] : fa.ct;
    else return 0.0;
}

// run-time kind: a switch over the compile-time forms (kernels that serve every kind with one instance)
__device__ __forceinline__ double eval_source(const FormArgs &fa, const double (&xq)[3], int64_t cell, int q, int nq)
{
    switch (fa.src_kind) {
    case TB_SRC_CONST: return eval_source_k<TB_SRC_CONST>(fa, 0.0, xq, cell, q, nq);
    case TB_SRC_NORM_PLUS_T: return eval_source_k<TB_SRC_NORM_PLUS_T>(fa, source_time<TB_SRC_NORM_PLUS_T>(fa), xq, cell, q, nq);
    case TB_SRC_COS_EXP: return eval_source_k<TB_SRC_COS_EXP>(fa, source_time<TB_SRC_COS_EXP>(fa), xq, cell, q, nq);
    case TB_SRC_TABULATED: return eval_source_k<TB_SRC_TABULATED>(fa, 0.0, xq, cell, q, nq);
    }
    return 0.0;
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

__device__ __forceinline__ void flag_neg_detj(Status *st, int64_t cell)
{
    st->neg_detj = 1;
    st->cell = cell;
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
template <class E, int FORM, bool FIELD, bool SYM, class PosT, int W>
__global__ void __launch_bounds__(PATCH_MAX_THREADS, W)
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
static inline unsigned nblocks(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

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
        if (p->patch_mat->d_colpos8) rc = launch(k_matrix_patch<E, FORM, FIELD, SYM, uint8_t, 2>);
        else rc = launch(k_matrix_patch<E, FORM, FIELD, SYM, uint16_t, 2>);
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

// ------------------------------------------------------------------------------------------------
// Scalar forms on the triquadratic field (Lagrange order 2 on hexahedra, 27 dofs and 27 Gauss points per cell): Mₑ, Kₑ are 27×27 —
// too large for the one-thread-per-cell register kernels above, so a workgroup integrates a cell at a time on the matrix cores (k_matrix_q2 below)
// and the entries reach the CSR arrays through a per-cell table of row positions (k_build_q2pos) — gathered per row, scattered atomically or
// per colour.  Constant and first-order nodal coefficients (the reference's mass.jl:28-43 / diffusion.jl:28-50); sources: k_vector_q2.
// ------------------------------------------------------------------------------------------------
// position of column dof(j) inside row dof(i), per cell and pair (cell-major: one coalesced 729-entry read per workgroup)
// TL: the table in the order of the stored element matrices of the element strategy (k_matrix_q2_sf: entry 27·(i₀ + 3 i₁ + 9 i₂) + 9 j₂ + 3 j₀ + j₁)
__device__ __constant__ uint8_t g_q2_node_b[27] = {0, 8, 1, 11, 20, 9, 3, 10, 2, 16, 21, 17, 24, 26, 22, 19, 23, 18, 4, 12, 5, 15, 25, 13, 7, 14, 6}; // (= g_q2_node below)
template <bool TL>
__global__ void k_build_q2pos(const int32_t *__restrict__ cell_dofs, int64_t n_cells, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                              uint16_t *__restrict__ pos, Status *st)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_cells * 729) return;
    const int64_t cell = tid / 729;
    int i = (int)(tid % 729) / 27, j = (int)(tid % 27);
    if (TL) { i = g_q2_node_b[i]; j = g_q2_node_b[(j / 3) % 3 + 3 * (j % 3) + 9 * (j / 9)]; }
    const int32_t *d = cell_dofs + cell * 27;
    const int32_t row = d[i], col = d[j];
    const int64_t lo0 = rowptr[row], hi0 = rowptr[row + 1];
    int64_t lo = lo0, hi = hi0;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (colidx[mid] < col) lo = mid + 1; else hi = mid;
    }
    if (lo >= hi0 || colidx[lo] != col || lo - lo0 > 0xFFFF) { st->pattern_missing = 1; st->cell = cell; lo = lo0; }
    pos[tid] = (uint16_t)(lo - lo0);
}

// Element matrices of the quadratic field on the matrix cores.  Both forms are one small GEMM per cell,
//   Kₑ[i][j] = −Σ_(q,k) T[(q,k)][i]·G[(q,k)][j]   (T = dΩ·D·∇N, G = ∇N: 27 × 27 × 81)      Mₑ[i][j] = Σ_q (ρ dΩ N)[q][i]·N[q][j]   (27 × 27 × 27),
// i.e. 2 × 2 tiles of v_mfma_f64_16x16x4_f64 with 21 / 7 k-steps.  The previous form (every lane summing its entries over the points out of LDS) was
// bound by LDS bandwidth — six doubles read per three FMAs, 0.95 MB of LDS traffic per cell; an MFMA reads two doubles per lane for sixteen FMAs.
// The four waves split the k-steps (each runs its share on every tile) and the partial tiles are summed through LDS in a fixed order, so the lower-left
// tile of a symmetric form is never computed (SYM: 3 tiles instead of 4) and the stores of the element strategy are 729 consecutive doubles.
// Reference-element values are formed from the 1-D factors in registers (no table loads); geometry per point: q2_point_geometry.
typedef double q2_d4 __attribute__((ext_vector_type(4)));
__constant__ uint8_t g_q2_tix[27] = {
    0 | 0 << 2 | 0 << 4, 2 | 0 << 2 | 0 << 4, 2 | 2 << 2 | 0 << 4, 0 | 2 << 2 | 0 << 4, 0 | 0 << 2 | 2 << 4, 2 | 0 << 2 | 2 << 4, 2 | 2 << 2 | 2 << 4,
    0 | 2 << 2 | 2 << 4, 1 | 0 << 2 | 0 << 4, 2 | 1 << 2 | 0 << 4, 1 | 2 << 2 | 0 << 4, 0 | 1 << 2 | 0 << 4, 1 | 0 << 2 | 2 << 4, 2 | 1 << 2 | 2 << 4,
    1 | 2 << 2 | 2 << 4, 0 | 1 << 2 | 2 << 4, 0 | 0 << 2 | 1 << 4, 2 | 0 << 2 | 1 << 4, 2 | 2 << 2 | 1 << 4, 0 | 2 << 2 | 1 << 4, 1 | 1 << 2 | 0 << 4,
    1 | 0 << 2 | 1 << 4, 2 | 1 << 2 | 1 << 4, 1 | 2 << 2 | 1 << 4, 0 | 1 << 2 | 1 << 4, 1 | 1 << 2 | 2 << 4, 1 | 1 << 2 | 1 << 4};

// inverse of g_q2_tix: tensor index t₀ + 3 t₁ + 9 t₂ → Ferrite node
__constant__ uint8_t g_q2_node[27] = {0, 8, 1, 11, 20, 9, 3, 10, 2, 16, 21, 17, 24, 26, 22, 19, 23, 18, 4, 12, 5, 15, 25, 13, 7, 14, 6};

// 1-D quadratic Lagrange factor t ∈ {0: ξ = −1, 1: ξ = 0, 2: ξ = +1} and its derivative at x (tb_elem.hpp Hex27::q1 / dq1)
__device__ __forceinline__ double q2_l(int t, double x) { return t == 0 ? 0.5 * x * (x - 1.0) : t == 1 ? (1.0 - x * x) : 0.5 * x * (x + 1.0); }
__device__ __forceinline__ double q2_dl(int t, double x) { return t == 0 ? x - 0.5 : t == 1 ? -2.0 * x : x + 0.5; }

// geometry of point q = lane of the cell whose vertex coordinates sit in sx: J = Σ xₐ ⊗ ∂Mₐ/∂ξ of the trilinear map (tensor rule, first coordinate
// fastest).  Mass: out[0] = ρ·detJ·w.  Diffusion: out[0..8] = S = −dΩ · J⁻¹ D J⁻ᵀ, the coefficient pulled back to the reference cell, so that
// Kₑ[i][j] = Σ_q ∂Nᵢ/∂ξ · S_q · ∂Nⱼ/∂ξ with Kₑ[i,j] −= (∇Nⱼ·D·∇Nᵢ)·dΩ  (diffusion.jl:38-49; argument order of _inner_product_helper, utils.jl:409-410).
template <bool DIFF, bool MASS_FIELD>
__device__ __forceinline__ void q2_point_geometry(const double *sx, int q, double *out, double rho_c, const double *rho_nodes, const double *D, int64_t cell, Status *st)
{
    constexpr double GX = 0.7745966692414834, W0 = 0.5555555555555556, W1 = 0.8888888888888888;
    const int q0 = q % 3, q1 = (q / 3) % 3, q2 = q / 9;
    const double xi[3] = {GX * (q0 - 1), GX * (q1 - 1), GX * (q2 - 1)};
    const double wq = (q0 == 1 ? W1 : W0) * (q1 == 1 ? W1 : W0) * (q2 == 1 ? W1 : W0);
    double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, rho = 0.0;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const double f0 = 1.0 + Hex8<3>::sgn(a, 0) * xi[0], f1 = 1.0 + Hex8<3>::sgn(a, 1) * xi[1], f2 = 1.0 + Hex8<3>::sgn(a, 2) * xi[2];
        const double d[3] = {0.125 * Hex8<3>::sgn(a, 0) * f1 * f2, 0.125 * f0 * Hex8<3>::sgn(a, 1) * f2, 0.125 * f0 * f1 * Hex8<3>::sgn(a, 2)};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) J[i][k] += sx[3 * a + i] * d[k];
        if constexpr (MASS_FIELD) rho += 0.125 * f0 * f1 * f2 * rho_nodes[a];
    }
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1], c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2], c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    const double dO = det * wq;
    if (!(dO > 0.0)) { st->neg_detj = 1; st->cell = cell; }
    if constexpr (!DIFF) { out[0] = dO * (MASS_FIELD ? rho : rho_c); return; }
    const double id = 1.0 / det;
    // ji[m][k] = ∂ξ_m/∂x_k
    const double ji[3][3] = {{c00 * id, (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id, (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id},
                             {c01 * id, (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id, (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id},
                             {c02 * id, (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id, (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id}};
    // ∇Nₐ[k] = Σ_m ∂Nₐ/∂ξ_m · ji[m][k];  S[m][n] = −dΩ Σ_kl ji[n][k] D[k][l] ji[m][l]   (m pairs with Nᵢ, n with Nⱼ: −∇Nⱼ·D·∇Nᵢ)
    double E[3][3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int k = 0; k < 3; ++k) E[m][k] = -dO * (D[3 * k] * ji[m][0] + D[3 * k + 1] * ji[m][1] + D[3 * k + 2] * ji[m][2]); // −dΩ (D ∇ξ_m)[k]
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int n = 0; n < 3; ++n) out[3 * m + n] = E[m][0] * ji[n][0] + E[m][1] * ji[n][1] + E[m][2] * ji[n][2];
}

// The workgroup is persistent (cells blockIdx.x, + gridDim.x, …) and pipelined over two barriers per cell: while waves 0–2 run the tiles of cell c
// (tile 0: i, j < 16; tile 1: i < 16 ≤ j; tile 2: i, j ≥ 16; the lower-left tile of a symmetric form is the mirror of tile 1 and is stored from it),
// wave 3 computes the point geometry of cell c + 1 and requests the vertex coordinates of cell c + 2, so neither the two dependent loads
// (connectivity → coordinates) nor the 27-lane geometry phase sit on the critical path.  Non-symmetric tensors (SYM = false): wave 3 runs the
// fourth tile before the geometry.  With the coefficient pulled back (S_q above) the B operand — reference gradients ∂Nⱼ/∂ξ (mass: Nⱼ) at the
// points — is the same for every cell: each lane keeps its 21 (7) values in registers, as it keeps the reference gradients of the three
// (point, node) pairs whose A entries  A[(q,n)][i] = Σ_m ∂Nᵢ/∂ξ_m S_q[m][n]  (mass: ρ dΩ_q Nᵢ) it forms per cell: 9 FMAs per pair and one LDS
// operand buffer.  Tiles leave from the accumulator registers: 16 lanes store 16 consecutive doubles of an element-matrix row.
template <int FORM, bool FIELD, bool SYM>
__global__ void __launch_bounds__(256, 3)
k_matrix_q2(MeshView m, FormArgs fa, const double *__restrict__ cell_xyz, const int32_t *__restrict__ list, int64_t n_list, const int64_t *__restrict__ rowptr,
            const uint16_t *__restrict__ pos, double *__restrict__ nz, int atomic /*0 rmw, 1 atomic, 2 store Kₑ*/, double *__restrict__ ke, Status *st)
{
    constexpr bool DIFF = FORM == TB_FORM_DIFFUSION;
    constexpr int KD = DIFF ? 81 : 27, KS = (KD + 3) / 4, LD = 27, NS = DIFF ? 9 : 1;
    constexpr double GX = 0.7745966692414834;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, g = lane >> 4; // wave = role (re-labelling the roles per workgroup, by block index or by hardware SIMD id, changes nothing: DESIGN §8)
    __shared__ double s_x[2][24], s_rho[2][8], s_S[2][27][NS], sA[KD * LD], s_out[729];
    __shared__ int32_t s_dof[27];
    auto cell_of = [&](int64_t it) -> int64_t { return list ? (int64_t)list[it] : it; };
    int64_t it = blockIdx.x;
    if (it >= n_list) return;
    // reference values at (point q, node a): N and ∂N/∂ξ from the 1-D factors (tb_elem.hpp Hex27)
    auto ref = [&](int q, int a, double &n, double (&d)[3]) {
        const int tx = g_q2_tix[a], t0 = tx & 3, t1 = (tx >> 2) & 3, t2 = tx >> 4;
        const double x0 = GX * (q % 3 - 1), x1 = GX * ((q / 3) % 3 - 1), x2 = GX * (q / 9 - 1);
        const double l0 = q2_l(t0, x0), l1 = q2_l(t1, x1), l2 = q2_l(t2, x2);
        n = l0 * l1 * l2;
        d[0] = q2_dl(t0, x0) * l1 * l2; d[1] = l0 * q2_dl(t1, x1) * l2; d[2] = l0 * l1 * q2_dl(t2, x2);
    };
    // the (q, a) pairs this lane forms A entries for: the operand phase runs on the tile waves only (192 lanes of a symmetric form: wave 3 is the
    // producer of the next cell's geometry and shares no registers with the tile code path)
    constexpr int NC = SYM ? 192 : 256, NR = (729 + NC - 1) / NC;
    double rn[NR], rd[NR][3];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int idx = tid + NC * r < 729 ? tid + NC * r : 728;
        ref(idx / 27, idx % 27, rn[r], rd[r]);
    }
    // this lane's B operand: B[kk = 4s + g][j = 16·tj + lr];  kk = 3q + n (mass: kk = q) — the table goes through the (still unused) operand buffer once
    const int ti = wv == 0 || wv == 1 ? 0 : 1, tj = wv == 1 || wv == 2 ? 1 : 0;
    const int ra = 16 * ti + lr < 27 ? 16 * ti + lr : 26, cb = 16 * tj + lr < 27 ? 16 * tj + lr : 26;
    if (tid < NC) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int idx = tid + NC * r;
            if (idx < 729) {
                const int q = idx / 27, a = idx - 27 * q;
                if constexpr (!DIFF) sA[q * LD + a] = rn[r];
                else {
#pragma unroll
                    for (int n = 0; n < 3; ++n) sA[(3 * q + n) * LD + a] = rd[r][n];
                }
            }
        }
    }
    __syncthreads();
    double Bv[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int kk = 4 * s + g;
        Bv[s] = sA[(kk < KD ? kk : KD - 1) * LD + cb];
    }
    // producer: inputs of later cells in flight (lane < 24: a vertex coordinate; 32..39: nodal density; lane = point: the tensor there).  Two sets,
    // used alternately: a set is requested two iterations before it is parked, so the load latency never sits on the critical path
    struct Pre { double x = 0.0, r = 0.0, d[6] = {0, 0, 0, 0, 0, 0}; };
    Pre PA, PB;
    auto request = [&](Pre &P, int64_t itn) {
        if (itn >= n_list) return;
        const int64_t c = cell_of(itn);
        if (lane < 24) P.x = cell_xyz[c * 24 + lane];
        if constexpr (!DIFF && FIELD) if (lane >= 32 && lane < 40) P.r = fa.field[c * 8 + lane - 32];
        if constexpr (DIFF && FIELD) if (lane < 27) { // tensor tabulated at the 27 points of the cell (k_tabulate_spectral / _isotropic over Hex8<3>: same point order)
#pragma unroll
            for (int e = 0; e < 6; ++e) P.d[e] = fa.dtab[(c * 27 + lane) * 6 + e];
        }
    };
    double Dq[6] = {0, 0, 0, 0, 0, 0};
    auto park = [&](const Pre &P, int b) { // coordinates / densities to LDS; the tensor stays in this lane's registers
        if (lane < 24) s_x[b][lane] = P.x;
        if constexpr (!DIFF && FIELD) if (lane >= 32 && lane < 40) s_rho[b][lane - 32] = P.r;
        if constexpr (DIFF && FIELD) {
#pragma unroll
            for (int e = 0; e < 6; ++e) Dq[e] = P.d[e];
        }
    };
    auto geometry = [&](int b, int64_t itn) {
        double D[9];
        if constexpr (DIFF && FIELD) { D[0] = Dq[0]; D[1] = D[3] = Dq[1]; D[2] = D[6] = Dq[2]; D[4] = Dq[3]; D[5] = D[7] = Dq[4]; D[8] = Dq[5]; }
        else {
#pragma unroll
            for (int e = 0; e < 9; ++e) D[e] = DIFF ? fa.D[e] : 0.0;
        }
        if (lane < 27) q2_point_geometry<DIFF, !DIFF && FIELD>(s_x[b], lane, s_S[b][lane], fa.rho, s_rho[b], D, cell_of(itn), st);
    };
    const int64_t G = gridDim.x;
    if (wv == 3) { // prologue: geometry of the first cell; sets A and B hold the inputs of the second and third
        request(PA, it);
        park(PA, 0);
        __builtin_amdgcn_wave_barrier();
        geometry(0, it);
        request(PA, it + G);
        request(PB, it + 2 * G);
    }
    // one cell; PROD: this wave parks / requests / computes the next geometry, TILE: it forms operands and runs its tile
    auto iteration = [&](auto prod, auto tile, int buf, Pre &P) __attribute__((always_inline)) {
        constexpr bool PROD = decltype(prod)::value, TILE = decltype(tile)::value;
        const int64_t cell = cell_of(it);
        lds_barrier(); // S of this cell is in s_S[buf]; the operand buffer is free
        if constexpr (TILE) {
            if (tid < 27 && atomic != 2) s_dof[tid] = m.cell_dofs[cell * 27 + tid];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const int idx = tid + NC * r;
                if (idx < 729) {
                    const int q = idx / 27, a = idx - 27 * q;
                    const double *S = s_S[buf][q];
                    if constexpr (!DIFF) sA[q * LD + a] = S[0] * rn[r];          // Mₑ[i,j] += ρ·Nᵢ·Nⱼ·dΩ  (mass.jl:32-42)
                    else {
#pragma unroll
                        for (int n = 0; n < 3; ++n) sA[(3 * q + n) * LD + a] = rd[r][0] * S[n] + rd[r][1] * S[3 + n] + rd[r][2] * S[6 + n];
                    }
                }
            }
        }
        if constexpr (PROD) { park(P, buf ^ 1); request(P, it + 3 * G); } // next cell's inputs (requested two iterations ago) → LDS; the set is free again
        lds_barrier(); // operands complete
        if constexpr (TILE) {
            // lane (lr, g) feeds A[row lr][k g] and B[k g][col lr]; rows / columns ≥ 27 are clamped (never stored); the k-padding vanishes through A
            q2_d4 acc = q2_d4{0, 0, 0, 0};
            double av[KS]; // all A reads in flight before the first product
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int kk = 4 * s + g;
                av[s] = sA[(kk < KD ? kk : KD - 1) * LD + ra];
            }
            if (4 * (KS - 1) + g >= KD) av[KS - 1] = 0.0;
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], Bv[s], acc, 0, 0, 0);
            // D[row g + 4·reg][col lr]: the element strategy stores its tile straight into the contiguous Kₑ (gathered per row by k_gather_rows_q2); the
            // scattering strategies pass it through LDS so that the position table is read, and the row pointers are looked up, in entry order
            const int64_t pbase = cell * 729;
            const int j = 16 * tj + lr;
            if (j < 27) {
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int i = 16 * ti + g + 4 * rg;
                    if (i >= 27) continue;
                    if (atomic == 2) {
                        ke[pbase + 27 * i + j] = acc[rg];
                        if (SYM && wv == 1) ke[pbase + 27 * j + i] = acc[rg];
                    } else {
                        s_out[27 * i + j] = acc[rg];
                        if (SYM && wv == 1) s_out[27 * j + i] = acc[rg];
                    }
                }
            }
        }
        if (atomic != 2) { // uniform over the workgroup
            lds_barrier();
            if constexpr (TILE) {
                const int64_t pbase = cell * 729;
                for (int e = tid; e < 729; e += NC) {
                    const int64_t k = rowptr[s_dof[e / 27]] + pos[pbase + e];
                    if (atomic) unsafeAtomicAdd(nz + k, s_out[e]); else nz[k] += s_out[e];
                }
            }
        }
        if constexpr (PROD) if (it + G < n_list) geometry(buf ^ 1, it + G);
    };
    auto run = [&](auto prod, auto tile) __attribute__((always_inline)) {
        for (;;) {
            iteration(prod, tile, 0, PA);
            it += G;
            if (it >= n_list) break;
            iteration(prod, tile, 1, PB);
            it += G;
            if (it >= n_list) break;
        }
    };
    if (wv == 3) run(std::true_type{}, std::integral_constant<bool, !SYM>{});
    else run(std::false_type{}, std::true_type{});
}

// Sum-factorised form of the same element matrices (default; the matrix-core kernel above stays as the TB_Q2_KERNEL=mfma comparison).  With the
// coefficient pulled back to the reference cell (S_q above) the sum over the 27 Gauss points is three one-dimensional contractions, because node
// i ↔ (i₀, i₁, i₂), point q ↔ (q₀, q₁, q₂) and ∂̂ₘNᵢ(ξ_q) = Π_dim ψ(dim == m)_{i_dim}(q_dim), ψ(false) = φ, ψ(true) = φ′:
//   stage 1  Z1[m][n][q₁][q₂][i₀][j₀] = Σ_q₀ ψ(m==0)_{i₀}(q₀) ψ(n==0)_{j₀}(q₀) S_q[m][n]                     (81 lane-tasks per cell: 36 multiply-adds)
//   stages 2 + 3 in registers, task (i₀, j₀, i₁, j₁): contract q₁ — after which only "m is 2 or not" matters — then q₂ → the nine entries (i₂, j₂)
//                                                                                                              (81 tasks: 171 multiply-adds, 81 LDS reads)
// ≈ 1.7·10⁴ multiply-adds per cell for the stiffness matrix instead of 5.9·10⁴ (mass: 9 + 81 small tasks), on the vector ALUs.  A workgroup takes
// THREE cells per pass so that the 81-task stages fill 243 of its 256 lanes; 24 KB of LDS, persistent, the vertex coordinates of the next triple
// requested one pass ahead.  Measured at 64³ (stiffness integration alone): 0.64 ms against 1.07 ms for the matrix-core kernel; a build forced
// to three waves per SIMD spilled 200 B and took 1.19 ms; a wave-per-cell form without workgroup barriers (81 tasks in two rounds of 64 lanes,
// geometry on 27 lanes) 0.85 ms — the half-empty second rounds cost more than the barriers.  Same sums as mass.jl:28-43 / diffusion.jl:28-50 in
// another order (≲ 1e-15 relative); no symmetry assumed, so non-symmetric constant tensors need no variant of their own.
// (Round 6: the element matrices of a triple sent through LDS and stored as one run of 3 × 729 doubles — every wave store 512 contiguous bytes instead of
// seven 72-byte pieces — was built and measured at 64³: mass 1.02 against 1.04 ms, diffusion 1.29 against 1.22 ms for integration + gather: the stores were
// not what the diffusion kernel waits for, the extra barrier and 17 KB of LDS traffic per pass cost more.  Removed; profiles/r06_v1/ab_q2_element_matrices_through_lds.log.)
template <int FORM, bool FIELD>
__global__ void __launch_bounds__(256, 2)
k_matrix_q2_sf(MeshView m, FormArgs fa, const double *__restrict__ cell_xyz, const int32_t *__restrict__ list, int64_t cell0, int64_t n_list, const int64_t *__restrict__ rowptr,
               const uint16_t *__restrict__ pos, double *__restrict__ nz, int atomic /*0 rmw, 1 atomic, 2 store Kₑ*/, double *__restrict__ ke, Status *st)
{
    constexpr bool DIFF = FORM == TB_FORM_DIFFUSION;
    constexpr int NS = DIFF ? 9 : 1, NZ1 = DIFF ? 729 : 81;
    constexpr double GX = 0.7745966692414834;
    __shared__ double s_x[3][24], s_rho[3][8], s_S[3][27][NS], s_Z1[3][NZ1];
    const int tid = threadIdx.x;
    auto PH = [](int i, int q) constexpr { return i == 0 ? 0.5 * (GX * (q - 1)) * (GX * (q - 1) - 1.0) : i == 1 ? 1.0 - (GX * (q - 1)) * (GX * (q - 1)) : 0.5 * (GX * (q - 1)) * (GX * (q - 1) + 1.0); };
    auto DP = [](int i, int q) constexpr { return i == 0 ? GX * (q - 1) - 0.5 : i == 1 ? -2.0 * (GX * (q - 1)) : GX * (q - 1) + 0.5; };
    auto cell_of = [&](int64_t k) -> int64_t { return list ? (int64_t)list[k] : cell0 + k; }; // (cell0: first cell of a chunk of the chunked element assembly)
    const int64_t ntrip = (n_list + 2) / 3;
    // task of stages 2 + 3: cell kc of the triple, (j₁, j₀, i₁, i₀) — fixed for the life of the workgroup
    const int kc = tid / 81, t81 = tid - 81 * kc;
    const int tj1 = t81 % 3, tj0 = (t81 / 3) % 3, ti1 = (t81 / 9) % 3, ti0 = t81 / 27;
    double c2[2][2][3]; // ψ(m==1)_{i₁}(q₁)·ψ(n==1)_{j₁}(q₁)
#pragma unroll
    for (int q1 = 0; q1 < 3; ++q1) {
        const double pa = ti1 == 0 ? PH(0, q1) : ti1 == 1 ? PH(1, q1) : PH(2, q1), da = ti1 == 0 ? DP(0, q1) : ti1 == 1 ? DP(1, q1) : DP(2, q1);
        const double pb = tj1 == 0 ? PH(0, q1) : tj1 == 1 ? PH(1, q1) : PH(2, q1), db = tj1 == 0 ? DP(0, q1) : tj1 == 1 ? DP(1, q1) : DP(2, q1);
        c2[0][0][q1] = pa * pb; c2[0][1][q1] = pa * db; c2[1][0][q1] = da * pb; c2[1][1][q1] = da * db;
    }
    int rowi[3], colj[3]; // Ferrite nodes of (i₀, i₁, ·), (j₀, j₁, ·)
#pragma unroll
    for (int k = 0; k < 3; ++k) { rowi[k] = g_q2_node[ti0 + 3 * ti1 + 9 * k]; colj[k] = g_q2_node[tj0 + 3 * tj1 + 9 * k]; }
    // inputs of a triple: lanes 0–71 one vertex coordinate each, lanes 96–119 one nodal density each
    auto request = [&](int64_t trip, double &px, double &pr) {
        px = 0.0; pr = 0.0;
        if (tid < 72) { const int64_t k = 3 * trip + tid / 24; if (k < n_list) px = cell_xyz[cell_of(k) * 24 + tid % 24]; }
        if constexpr (!DIFF && FIELD) if (tid >= 96 && tid < 120) { const int64_t k = 3 * trip + (tid - 96) / 8; if (k < n_list) pr = fa.field[cell_of(k) * 8 + (tid - 96) % 8]; }
    };
    double px, pr;
    int64_t trip = blockIdx.x;
    if (trip >= ntrip) return;
    request(trip, px, pr);
    for (; trip < ntrip; trip += gridDim.x) {
        if (tid < 72) s_x[tid / 24][tid % 24] = px;
        if constexpr (!DIFF && FIELD) if (tid >= 96 && tid < 120) s_rho[(tid - 96) / 8][(tid - 96) % 8] = pr;
        lds_barrier();
        if (trip + gridDim.x < ntrip) request(trip + gridDim.x, px, pr); // next triple's inputs travel during this one's arithmetic
        const int64_t kcell = 3 * trip + kc;
        const bool live = tid < 243 && kcell < n_list;
        const int64_t cell = live ? cell_of(kcell) : 0;
        // geometry of the 27 points of each cell: lane = (cell of the triple, point)
        if (tid < 81) {
            const int k = tid / 27, q = tid - 27 * k;
            const int64_t kk = 3 * trip + k;
            if (kk < n_list) {
                const int64_t c = cell_of(kk);
                double D[9];
                if constexpr (DIFF && FIELD) {
                    const double *dp = fa.dtab + (c * 27 + q) * 6; // tensor tabulated at the 27 points (k_tabulate_spectral / _isotropic over Hex8<3>: same point order)
                    D[0] = dp[0]; D[1] = D[3] = dp[1]; D[2] = D[6] = dp[2]; D[4] = dp[3]; D[5] = D[7] = dp[4]; D[8] = dp[5];
                } else {
#pragma unroll
                    for (int e = 0; e < 9; ++e) D[e] = DIFF ? fa.D[e] : 0.0;
                }
                q2_point_geometry<DIFF, !DIFF && FIELD>(s_x[k], q, s_S[k][q], fa.rho, s_rho[k], D, c, st);
            }
        }
        lds_barrier();
        // stage 1
        if constexpr (DIFF) {
            if (tid < 243) { // task (m, n, q₁, q₂) of cell kc
                int t = t81;
                const int q2 = t % 3; t /= 3;
                const int q1 = t % 3; t /= 3;
                const int n_ = t % 3;
                const int m_ = t / 3;
                double in[3], tb0[3][3];
#pragma unroll
                for (int q0 = 0; q0 < 3; ++q0) in[q0] = s_S[kc][q0 + 3 * q1 + 9 * q2][3 * m_ + n_];
#pragma unroll
                for (int j0 = 0; j0 < 3; ++j0)
#pragma unroll
                    for (int q0 = 0; q0 < 3; ++q0) tb0[j0][q0] = (n_ == 0 ? DP(j0, q0) : PH(j0, q0)) * in[q0];
#pragma unroll
                for (int i0 = 0; i0 < 3; ++i0)
#pragma unroll
                    for (int j0 = 0; j0 < 3; ++j0) {
                        double v = 0.0;
#pragma unroll
                        for (int q0 = 0; q0 < 3; ++q0) v += (m_ == 0 ? DP(i0, q0) : PH(i0, q0)) * tb0[j0][q0];
                        s_Z1[kc][9 * t81 + 3 * i0 + j0] = v;
                    }
            }
        } else {
            if (tid < 27) { // task (q₁, q₂) of cell tid / 9
                const int k = tid / 9, t = tid - 9 * k, q2 = t % 3, q1 = t / 3;
                double in[3];
#pragma unroll
                for (int q0 = 0; q0 < 3; ++q0) in[q0] = s_S[k][q0 + 3 * q1 + 9 * q2][0];
#pragma unroll
                for (int i0 = 0; i0 < 3; ++i0)
#pragma unroll
                    for (int j0 = 0; j0 < 3; ++j0) {
                        double v = 0.0;
#pragma unroll
                        for (int q0 = 0; q0 < 3; ++q0) v += PH(i0, q0) * PH(j0, q0) * in[q0];
                        s_Z1[k][9 * t + 3 * i0 + j0] = v;
                    }
            }
        }
        lds_barrier();
        // stages 2 + 3
        if (live) {
            double out[3][3];
            if constexpr (DIFF) {
                double z[2][2][3];
#pragma unroll
                for (int e = 0; e < 12; ++e) (&z[0][0][0])[e] = 0.0;
#pragma unroll
                for (int m_ = 0; m_ < 3; ++m_)
#pragma unroll
                    for (int n_ = 0; n_ < 3; ++n_)
#pragma unroll
                        for (int q1 = 0; q1 < 3; ++q1) {
                            const double cf = c2[m_ == 1][n_ == 1][q1];
                            const double *zp = &s_Z1[kc][9 * (((m_ * 3 + n_) * 3 + q1) * 3) + 3 * ti0 + tj0];
#pragma unroll
                            for (int q2 = 0; q2 < 3; ++q2) z[m_ == 2][n_ == 2][q2] += cf * zp[9 * q2];
                        }
                double w[2][3][3];
#pragma unroll
                for (int mu = 0; mu < 2; ++mu)
#pragma unroll
                    for (int j2 = 0; j2 < 3; ++j2)
#pragma unroll
                        for (int q2 = 0; q2 < 3; ++q2) w[mu][j2][q2] = PH(j2, q2) * z[mu][0][q2] + DP(j2, q2) * z[mu][1][q2];
#pragma unroll
                for (int i2 = 0; i2 < 3; ++i2)
#pragma unroll
                    for (int j2 = 0; j2 < 3; ++j2) {
                        double v = 0.0;
#pragma unroll
                        for (int q2 = 0; q2 < 3; ++q2) v += PH(i2, q2) * w[0][j2][q2] + DP(i2, q2) * w[1][j2][q2];
                        out[i2][j2] = v;
                    }
            } else {
                double z[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int q1 = 0; q1 < 3; ++q1) {
                    const double *zp = &s_Z1[kc][9 * (q1 * 3) + 3 * ti0 + tj0];
#pragma unroll
                    for (int q2 = 0; q2 < 3; ++q2) z[q2] += c2[0][0][q1] * zp[9 * q2];
                }
#pragma unroll
                for (int i2 = 0; i2 < 3; ++i2)
#pragma unroll
                    for (int j2 = 0; j2 < 3; ++j2) {
                        double v = 0.0;
#pragma unroll
                        for (int q2 = 0; q2 < 3; ++q2) v += PH(i2, q2) * PH(j2, q2) * z[q2];
                        out[i2][j2] = v;
                    }
            }
            const int64_t pbase = cell * 729;
            // stored element matrices (atomic == 2) in TENSOR order: row i₀ + 3 i₁ + 9 i₂, column 9 j₂ + 3 j₀ + j₁, so that the nine lanes (j₀, j₁) of a
            // row store nine consecutive doubles and the three stores j₂ = 0, 1, 2 complete its 216 bytes (in Ferrite's node order the 64 lanes of a
            // store hit 64 separate 8-byte pieces of the 5.8 KB block: the mass kernel, whose arithmetic is a fifth of the diffusion kernel's, took 0.49
            // of that one's 0.61 ms — bound by the store path); k_gather_rows_q2<true> reads the rows in this order
            const int etl = 27 * (ti0 + 3 * ti1) + 3 * tj0 + tj1;
#pragma unroll
            for (int i2 = 0; i2 < 3; ++i2)
#pragma unroll
                for (int j2 = 0; j2 < 3; ++j2) {
                    const int e = 27 * rowi[i2] + colj[j2];
                    if (atomic == 2) ke[pbase + etl + 243 * i2 + 9 * j2] = out[i2][j2];
                    else {
                        const int64_t k = rowptr[m.cell_dofs[cell * 27 + rowi[i2]]] + pos[pbase + e];
                        if (atomic) unsafeAtomicAdd(nz + k, out[i2][j2]); else nz[k] += out[i2][j2];
                    }
                }
        }
        lds_barrier(); // the staging arrays are rewritten by the next pass
    }
}

// ElementAssemblyStrategy for the quadratic scalar field, second pass: a half-wave per row sums the rows of the element matrices that touch its dof
// (27 lanes, an LDS copy of the CSR row, cells in ascending order: bit-reproducible) and stores the CSR row once.  The contributing (cell, local row)
// slots come from a fixed-width table (W per row, −1 padded: one load, no pointer chase) and the index and value loads of eight cells are all in
// flight before the first addition.
// The element matrices of k_matrix_q2_sf are stored in tensor order (row i₀ + 3 i₁ + 9 i₂, column 9 j₂ + 3 j₀ + j₁); the element strategy then hands this
// kernel the slot table and the position table in the same order (tb_mesh ea->d_ell_t, tb_pattern::d_q2pos_t), so the loads below stay one contiguous
// run per row.  (Permuting inside this kernel instead — a row look-up between the slot load and the value load, the positions as scattered 2-byte
// reads — was measured: 0.69 → 0.86 ms.)
__global__ void __launch_bounds__(256)
k_gather_rows_q2(int64_t row0, int64_t n_rows, const int32_t *__restrict__ ell, int W, const double *__restrict__ ke, const uint16_t *__restrict__ pos,
                 const int64_t *__restrict__ rowptr, double *__restrict__ nz, int max_row)
{
    extern __shared__ double s_rows[];
    const int hw = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int64_t r = row0 + (int64_t)blockIdx.x * (blockDim.x >> 5) + hw; // rows [row0, n_rows)
    if (r >= n_rows) return;
    double *row = s_rows + (size_t)hw * max_row;
    const int64_t g0 = rowptr[r];
    const int len = (int)(rowptr[r + 1] - g0);
    for (int p = l; p < len; p += 32) row[p] = 0.0;
    for (int kb = 0; kb < W; kb += 8) {
        int slot[8], pp[8];
        double vv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) slot[k] = ell[r * W + kb + k]; // cell · 27 + local row
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool on = slot[k] >= 0 && l < 27;
            pp[k] = on ? pos[(int64_t)slot[k] * 27 + l] : -1;
            vv[k] = on ? ke[(int64_t)slot[k] * 27 + l] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (pp[k] >= 0) row[pp[k]] += vv[k];
    }
    for (int p = l; p < len; p += 32) nz[g0 + p] = row[p];
}

__global__ void __launch_bounds__(64)
k_vector_q2(MeshView m, FormArgs fa, const double *__restrict__ cell_xyz, const int32_t *__restrict__ list, double *__restrict__ b, int atomic, Status *st)
{
    // one wave per cell: lane q < 27 evaluates f(x_q, t)·dΩ_q, lane j < 27 then sums its dof's row.  Geometry and shape values come from the 1-D
    // factors in registers (the first version loaded 72 + 27 table entries per lane with lane-varying addresses and inverted J it never used),
    // vertex coordinates from the cell-major array (one load instead of connectivity → coordinate)
    constexpr double GX = 0.7745966692414834, W0 = 0.5555555555555556, W1 = 0.8888888888888888;
    const int64_t cell = list ? list[blockIdx.x] : blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ double s_x[24], s_fw[27];
    if (tid < 24) s_x[tid] = cell_xyz[cell * 24 + tid];
    __syncthreads();
    if (tid < 27) {
        const int q0 = tid % 3, q1 = (tid / 3) % 3, q2 = tid / 9;
        const double xi[3] = {GX * (q0 - 1), GX * (q1 - 1), GX * (q2 - 1)};
        double J[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, xq[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const double f0 = 1.0 + Hex8<3>::sgn(a, 0) * xi[0], f1 = 1.0 + Hex8<3>::sgn(a, 1) * xi[1], f2 = 1.0 + Hex8<3>::sgn(a, 2) * xi[2];
            const double d[3] = {0.125 * Hex8<3>::sgn(a, 0) * f1 * f2, 0.125 * f0 * Hex8<3>::sgn(a, 1) * f2, 0.125 * f0 * f1 * Hex8<3>::sgn(a, 2)};
            const double Ma = 0.125 * f0 * f1 * f2;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                xq[i] += Ma * s_x[3 * a + i];
#pragma unroll
                for (int k = 0; k < 3; ++k) J[i][k] += s_x[3 * a + i] * d[k];
            }
        }
        const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) + J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2]) +
                           J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
        const double dO = det * (q0 == 1 ? W1 : W0) * (q1 == 1 ? W1 : W0) * (q2 == 1 ? W1 : W0);
        if (!(dO > 0.0)) { st->neg_detj = 1; st->cell = cell; }
        s_fw[tid] = eval_source(fa, xq, cell, tid, 27) * dO;
    }
    __syncthreads();
    if (tid < 27) { // bₑ[j] += f(x_q,t)·Nⱼ·dΩ  (analytical_coefficient.jl:89-99)
        const int tx = g_q2_tix[tid], t0 = tx & 3, t1 = (tx >> 2) & 3, t2 = tx >> 4;
        double L0[3], L1[3], L2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { const double x = GX * (k - 1); L0[k] = q2_l(t0, x); L1[k] = q2_l(t1, x); L2[k] = q2_l(t2, x); }
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 27; ++q) v += s_fw[q] * (L0[q % 3] * L1[(q / 3) % 3] * L2[q / 9]);
        const int32_t d = m.cell_dofs[cell * 27 + tid];
        if (atomic) unsafeAtomicAdd(b + d, v); else b[d] += v;
    }
}

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

static int ensure_q2pos(tb_pattern *p)
{
    if (p->d_q2pos) return TB_OK;
    tb_mesh *m = p->mesh;
    const int64_t n = m->n_cells * 729;
    TB_HIP(hipMalloc((void **)&p->d_q2pos, sizeof(uint16_t) * n));
    int rc = reset_status(m->dev);
    if (rc) return rc;
    hipLaunchKernelGGL(k_build_q2pos<false>, dim3(nblocks(n, 256)), dim3(256), 0, m->dev->stream, m->d_cell_dofs, m->n_cells, p->d_rowptr, p->d_colidx, p->d_q2pos,
                       m->dev->d_status);
    TB_HIP(hipGetLastError());
    return check_status(m->dev);
}
// the same table in the order of the stored element matrices (element strategy)
static int ensure_q2pos_t(tb_pattern *p)
{
    if (p->d_q2pos_t) return TB_OK;
    tb_mesh *m = p->mesh;
    const int64_t n = m->n_cells * 729;
    TB_HIP(hipMalloc((void **)&p->d_q2pos_t, sizeof(uint16_t) * n));
    int rc = reset_status(m->dev);
    if (rc) return rc;
    hipLaunchKernelGGL(k_build_q2pos<true>, dim3(nblocks(n, 256)), dim3(256), 0, m->dev->stream, m->d_cell_dofs, m->n_cells, p->d_rowptr, p->d_colidx, p->d_q2pos_t,
                       m->dev->d_status);
    TB_HIP(hipGetLastError());
    return check_status(m->dev);
}

static int run_q2(tb_form *f, tb_pattern *p, int strategy, double t, double *d_nz, double *d_b)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    if (f->field && f->kind == TB_FORM_DIFFUSION && !f->d_dtab) { // first assembly: tabulate the tensor at the 27 points from the first-order nodal data
        const size_t bytes = sizeof(double) * (size_t)m->n_cells * 27 * 6;
        hipError_t e = hipMalloc((void **)&f->d_dtab, bytes);
        if (e != hipSuccess) { set_error("diffusion tensor table (%zu B): %s", bytes, hipGetErrorString(e)); return TB_ERR_NOMEM; }
        const double sc = f->coef.wrap ? 1.0 / (f->coef.Cm * f->coef.chi) : 1.0;
        if (f->coef.kind == TB_COEF_FIELD_SCALAR)
            hipLaunchKernelGGL((k_tabulate_isotropic<Hex8<3>>), dim3(nblocks(m->n_cells, 256)), dim3(256), 0, dev->stream, f->d_field, m->n_cells, sc, f->d_dtab);
        else
            hipLaunchKernelGGL((k_tabulate_spectral<Hex8<3>>), dim3(nblocks(m->n_cells, 256)), dim3(256), 0, dev->stream, f->d_field, m->n_cells, f->coef.p[0],
                               f->coef.p[1], f->coef.p[2], sc, f->d_dtab);
        TB_HIP(hipGetLastError());
        TB_SYNC_STREAM(dev);
        (void)hipFree(f->d_field); f->d_field = nullptr;
    }
    const MeshView mv = make_view(m);
    const FormArgs fa = make_args(f, t);
    const bool ea = d_nz && (strategy == TB_STRATEGY_ELEMENT);
    if (d_nz) { int rc = ensure_q2pos(p); if (rc) return rc; rc = ensure_cell_xyz(m); if (rc) return rc; if (!ea) TB_HIP(hipMemsetAsync(d_nz, 0, (size_t)p->nnz * sizeof(double), dev->stream)); }
    else { int rc = ensure_cell_xyz(m); if (rc) return rc; TB_HIP(hipMemsetAsync(d_b, 0, (size_t)m->ndofs * sizeof(double), dev->stream)); }
    double *kebuf = nullptr;
    if (ea) {
        if (!m->ea) { int rc = build_ea_plan(m); if (rc) return rc; }
        if (!p->d_kebuf) {
            hipError_t e = hipMalloc((void **)&p->d_kebuf, sizeof(double) * (size_t)m->n_cells * 729);
            if (e != hipSuccess) { set_error("element-matrix buffer (%zu B): %s", sizeof(double) * (size_t)m->n_cells * 729, hipGetErrorString(e)); return TB_ERR_NOMEM; }
        }
        kebuf = p->d_kebuf;
    }
    int64_t cell0 = 0; // first cell of the launch (chunked element assembly below)
    auto go = [&](const int32_t *list, int64_t n, int atomic) -> int {
        if (n == 0) return TB_OK;
        static const bool q2_mfma = tune_env("TB_Q2_KERNEL") && !strcmp(tune_env("TB_Q2_KERNEL"), "mfma"); // the matrix-core kernel (comparison)
        if (d_nz && !q2_mfma && atomic == 2) { // sum-factorised element matrices: three cells per pass, persistent (the scattering strategies keep the matrix-core kernel: it hands its entries over in entry order)
            const unsigned wg3 = (unsigned)std::min<int64_t>((n + 2) / 3, (int64_t)dev->n_cu * 6);
#define TB_Q2S(FORM, FIELD) hipLaunchKernelGGL((k_matrix_q2_sf<FORM, FIELD>), dim3(wg3), dim3(256), 0, dev->stream, mv, fa, m->d_cell_xyz, list, cell0, n, p->d_rowptr, p->d_q2pos, d_nz, atomic, kebuf, dev->d_status)
            if (f->kind == TB_FORM_MASS) { if (f->field) TB_Q2S(TB_FORM_MASS, true); else TB_Q2S(TB_FORM_MASS, false); }
            else { if (f->field) TB_Q2S(TB_FORM_DIFFUSION, true); else TB_Q2S(TB_FORM_DIFFUSION, false); }
#undef TB_Q2S
            TB_HIP(hipGetLastError());
            return TB_OK;
        }
        // persistent workgroups: three per CU (≤ 168 VGPRs)
        const unsigned wgs = (unsigned)std::min<int64_t>(n, (int64_t)dev->n_cu * 3);
#define TB_Q2(FORM, FIELD, SYM) hipLaunchKernelGGL((k_matrix_q2<FORM, FIELD, SYM>), dim3(wgs), dim3(256), 0, dev->stream, mv, fa, m->d_cell_xyz, list, n, p->d_rowptr, p->d_q2pos, d_nz, atomic, kebuf, dev->d_status)
        if (d_nz && f->kind == TB_FORM_MASS) { if (f->field) TB_Q2(TB_FORM_MASS, true, true); else TB_Q2(TB_FORM_MASS, false, true); }
        else if (d_nz) {
            // a non-symmetric constant tensor gives a non-symmetric Kₑ: all four tiles
            const bool sym = f->field || (fa.D[1] == fa.D[3] && fa.D[2] == fa.D[6] && fa.D[5] == fa.D[7]);
            if (f->field) TB_Q2(TB_FORM_DIFFUSION, true, true); else if (sym) TB_Q2(TB_FORM_DIFFUSION, false, true); else TB_Q2(TB_FORM_DIFFUSION, false, false);
        }
#undef TB_Q2
        else hipLaunchKernelGGL(k_vector_q2, dim3((unsigned)n), dim3(64), 0, dev->stream, mv, fa, m->d_cell_xyz, list, d_b, atomic, dev->d_status);
        TB_HIP(hipGetLastError());
        return TB_OK;
    };
    if (ea) {
        if (!p->max_row_len) for (int64_t r = 0; r < p->n_rows; ++r) p->max_row_len = std::max<int64_t>(p->max_row_len, p->h_rowptr[r + 1] - p->h_rowptr[r]);
        const int max_row = (int)p->max_row_len;
        int rc = ensure_ea_ell(m);
        if (rc) return rc;
        static const bool q2_mfma_g = tune_env("TB_Q2_KERNEL") && !strcmp(tune_env("TB_Q2_KERNEL"), "mfma"); // (the matrix-core kernel stores Ferrite's order)
        const int32_t *ell = m->ea->d_ell;
        const uint16_t *posg = p->d_q2pos;
        if (!q2_mfma_g) {
            rc = ensure_q2pos_t(p);
            if (rc) return rc;
            rc = ensure_ea_ell_q2t(m);
            if (rc) return rc;
            ell = m->ea->d_ell_t; posg = p->d_q2pos_t;
        }
        auto gather = [&](hipStream_t st, int64_t r0, int64_t r1) {
            if (r1 > r0)
                hipLaunchKernelGGL(k_gather_rows_q2, dim3((unsigned)((r1 - r0 + 7) / 8)), dim3(256), sizeof(double) * 8 * (size_t)max_row, st, r0, r1, ell, m->ea->ell_w, kebuf,
                                   posg, p->d_rowptr, d_nz, max_row);
        };
        // (a chunked form — gather of a chunk's rows on a second queue beside the integration of the next chunk, the scheme of the mechanics linearisation —
        // was built, bit-identical and slower: 1.43 / 1.53 / 1.64 ms in 4 / 8 / 16 chunks against 1.31 ms at 64³; removed in round 5, docs/rounds/r04.md)
        rc = go(nullptr, m->n_cells, 2);
        if (rc) return rc;
        gather(dev->stream, 0, m->ndofs);
        TB_HIP(hipGetLastError());
        return TB_OK;
    }
    if (strategy == TB_STRATEGY_ATOMIC || (strategy == TB_STRATEGY_ELEMENT && !d_nz)) return go(nullptr, m->n_cells, 1);
    if (strategy == TB_STRATEGY_PER_COLOR) {
        if (!m->colors) { int rc = build_color_plan(m); if (rc) return rc; }
        for (int c = 0; c < m->colors->ncolors; ++c) {
            int rc = go(m->colors->d_cells + m->colors->offsets[c], m->colors->offsets[c + 1] - m->colors->offsets[c], 0);
            if (rc) return rc;
        }
        return TB_OK;
    }
    set_error("Q2 scalar forms: strategy %d not supported (use TB_STRATEGY_ELEMENT, TB_STRATEGY_ATOMIC or TB_STRATEGY_PER_COLOR)", strategy);
    return TB_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------
// Patch strategy for linear tetrahedra on the staged layout of the hexahedron kernel (tb_patch_fused.hip): one 16-byte header per patch, the
// coordinates of the patch's nodes pre-gathered and contiguous, 8 bytes of patch-local node indices and a 4-byte index into the de-duplicated
// table of 16-byte position signatures per instance.  A tetrahedron carries a 4 × 4 element matrix — 40 B of algorithmic traffic per cell —
// so the general patch kernel (per instance: cell id, connectivity, coordinate gather, 16 row slots, 16 positions) moved mostly metadata.
// Mass and stiffness in one pass share geometry and metadata.  Instances are walked 256 at a time (a 5×5×5 tile holds 750 tetrahedra plus halo).
// The affine geometry is formed once per instance (the generic element routine re-derives it at each of the four points).
// ------------------------------------------------------------------------------------------------
struct TetPatchView {
    const uint16_t *elem_ln;
    const uint32_t *elem_sig;
    const uint8_t *sigtab;
    const RowDesc *row_desc;
    const int32_t *elem_cell;
    int kcap, max_rows, max_nodes;
};

template <bool WK, bool WM, bool FM>
__global__ void __launch_bounds__(256)
k_patch_tet4(FormArgs faK, FormArgs faM, TetPatchView pv, const uint4 *__restrict__ hdrs, const double *__restrict__ pcoord, double *__restrict__ nzK,
             double *__restrict__ nzM, Status *st)
{
    extern __shared__ double lds[];
    constexpr int T = 256;
    const int tid = threadIdx.x;
    uint4 h = hdrs[blockIdx.x];
    h.x = __builtin_amdgcn_readfirstlane(h.x); h.y = __builtin_amdgcn_readfirstlane(h.y); h.z = __builtin_amdgcn_readfirstlane(h.z); h.w = __builtin_amdgcn_readfirstlane(h.w);
    const int64_t e0 = h.x, r0 = h.y, n0 = h.z;
    const int nrows = (int)(h.w & 0x3ff), nnodes = (int)((h.w >> 10) & 0x7ff), ne = (int)(h.w >> 21);
    if (nrows == 0) return; // a patch whose dofs all belong to earlier patches writes nothing
    constexpr int NREG = (WK && WM) ? 2 : 1;
    double *accK = lds, *accM = lds + (NREG - 1) * pv.kcap;
    uint4 *desc = (uint4 *)(lds + NREG * pv.kcap); // RowDesc: nz0 (x, y), off (z), len (w)
    double *xs = (double *)(desc + pv.max_rows);
    {
        const uint4 *gd = (const uint4 *)pv.row_desc + r0;
        for (int s = tid; s < nrows; s += T) desc[s] = gd[s];
        const double *gc = pcoord + 3 * n0;
        for (int k = tid; k < 3 * nnodes; k += T) xs[k] = gc[k];
        double2 *z = (double2 *)lds;
        for (int k = tid; k < (NREG * pv.kcap) >> 1; k += T) z[k] = make_double2(0.0, 0.0);
    }
    // instance metadata runs two passes ahead of the arithmetic (node indices / signature index / cell id), the signature itself one pass ahead: no pass
    // waits for a load issued less than a pass ago
    struct Meta { uint2 l2; uint32_t sig; int32_t cell; };
    auto fetch = [&](int e) { Meta M{make_uint2(0, 0), 0u, 0}; if (e < ne) { M.l2 = ((const uint2 *)pv.elem_ln)[e0 + e]; M.sig = pv.elem_sig[e0 + e]; M.cell = pv.elem_cell[e0 + e]; } return M; };
    Meta cur = fetch(tid), nxt = fetch(tid + T);
    uint4 cpc = ((const uint4 *)pv.sigtab)[cur.sig]; // byte 4i + j: position of column j in row i
    __syncthreads();
    for (int e = tid; e < ne; e += T) {
        const uint4 cpn = ((const uint4 *)pv.sigtab)[nxt.sig];
        const Meta nn = fetch(e + 2 * T);
        const uint2 l2 = cur.l2;
        const uint4 cp = cpc;
        const int64_t cell = cur.cell;
        cur = nxt; nxt = nn; cpc = cpn;
        const uint32_t ln[4] = {l2.x & 0xffffu, l2.x >> 16, l2.y & 0xffffu, l2.y >> 16};
        const uint32_t cpw[4] = {cp.x, cp.y, cp.z, cp.w};
        double x[4][3];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double *px = xs + 3 * ln[a];
            x[a][0] = px[0]; x[a][1] = px[1]; x[a][2] = px[2];
        }
        uint32_t ro[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) ro[i] = ln[i] < (uint32_t)nrows ? desc[ln[i]].z : 0xFFFFFFFFu;
        // geometry of the affine cell, once: J = [x₁−x₀ | x₂−x₀ | x₃−x₀], ∇N₁,₂,₃ = rows of J⁻¹, ∇N₀ = −(∇N₁ + ∇N₂ + ∇N₃); the four points of the
        // rule share it (the generic element routine of the other strategies re-derives it per point: same numbers to rounding)
        double gN[4][3], det;
        {
            double e[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int i = 0; i < 3; ++i) e[k][i] = x[k + 1][i] - x[0][i];
            const double c0[3] = {e[1][1] * e[2][2] - e[1][2] * e[2][1], e[1][2] * e[2][0] - e[1][0] * e[2][2], e[1][0] * e[2][1] - e[1][1] * e[2][0]}; // e₂ × e₃
            const double c1[3] = {e[2][1] * e[0][2] - e[2][2] * e[0][1], e[2][2] * e[0][0] - e[2][0] * e[0][2], e[2][0] * e[0][1] - e[2][1] * e[0][0]}; // e₃ × e₁
            const double c2[3] = {e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0]}; // e₁ × e₂
            det = e[0][0] * c0[0] + e[0][1] * c0[1] + e[0][2] * c0[2];
            if (!(det > 0.0)) flag_neg_detj(st, cell);
            const double id = 1.0 / det;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                gN[1][i] = c0[i] * id; gN[2][i] = c1[i] * id; gN[3][i] = c2[i] * id;
                gN[0][i] = -(gN[1][i] + gN[2][i] + gN[3][i]);
            }
        }
        if constexpr (WK) {
            // Kₑ[i,j] −= (∇Nⱼ·D·∇Nᵢ)·dΩ  (diffusion.jl:38-49), Σ_q dΩ_q = det/6
            double Ke[16], Dg[4][3];
            const double mv = -det * (1.0 / 6.0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) Dg[i][k] = mv * (faK.D[3 * k] * gN[i][0] + faK.D[3 * k + 1] * gN[i][1] + faK.D[3 * k + 2] * gN[i][2]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) Ke[4 * i + j] = gN[j][0] * Dg[i][0] + gN[j][1] * Dg[i][1] + gN[j][2] * Dg[i][2];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (ro[i] != 0xFFFFFFFFu) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) unsafeAtomicAdd(accK + (ro[i] + ((cpw[i] >> (8 * j)) & 0xffu)), Ke[4 * i + j]);
                }
        }
        if constexpr (WM) {
            // Mₑ[i,j] += ρ(x_q)·Nᵢ·Nⱼ·dΩ_q over the four points  (mass.jl:32-42); dΩ_q = det·w
            double Me[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) Me[k] = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double r = faM.rho;
                if constexpr (FM) {
                    r = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; ++a) r += Tet4<2>::N(q, a) * faM.field[cell * 4 + a];
                }
                const double rw = r * det * Tet4<2>::w(q);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) Me[4 * i + j] += rw * (Tet4<2>::N(q, i) * Tet4<2>::N(q, j));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (ro[i] != 0xFFFFFFFFu) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) unsafeAtomicAdd(accM + (ro[i] + ((cpw[i] >> (8 * j)) & 0xffu)), Me[4 * i + j]);
                }
        }
    }
    __syncthreads();
    // write-out: one row per QUARTER-wave (rows of a tetrahedral mesh hold ≈ 15 entries: a half-wave per row left 17 of its 32 lanes idle — round 6),
    // each matrix's row as one contiguous run
    const int quarter = tid >> 4, ql = tid & 15;
    for (int s = quarter; s < nrows; s += T / 16) {
        const uint4 d = desc[s];
        const int64_t g0 = (int64_t)(((uint64_t)d.y << 32) | d.x);
        for (uint32_t k = ql; k < d.w; k += 16) {
            if constexpr (WK) nzK[g0 + k] = accK[d.z + k];
            if constexpr (WM) nzM[g0 + k] = accM[d.z + k];
        }
    }
}

bool tet4_patch_applicable(const tb_form *f, const tb_pattern *)
{
    static const bool legacy = getenv("TB_PATCH_KERNEL") && !strcmp(getenv("TB_PATCH_KERNEL"), "legacy");
    if (legacy) return false;
    const tb_mesh *m = f->mesh;
    if (m->field_kind != TB_TET4 || m->geom_kind != TB_TET4 || m->ncomp != 1 || f->qorder != 2 || f->has_cellset) return false;
    if (f->kind == TB_FORM_DIFFUSION) return !f->field; // tensor fields stay on the general kernel (their table is built there)
    return f->kind == TB_FORM_MASS;
}

int launch_assemble_tet4_patch(tb_form *fK, tb_form *fM, tb_pattern *p, double t, double *d_nzK, double *d_nzM)
{
    tb_form *any = fK ? fK : fM;
    tb_mesh *m = any->mesh;
    tb_device *dev = m->dev;
    int rc = reset_status(dev);
    if (rc) return rc;
    const int nreg = fK && fM ? 2 : 1;
    rc = ensure_patch_fused(m, p, nreg);
    if (rc) return rc;
    const PatchPlan *pp = m->patches.get();
    const PatchFusedPlan *pf = p->patch_fused.get();
    if (!pf->d_hdr) { set_error("tetrahedron patch kernel: a patch exceeds the packed header (1023 rows / 2047 nodes / 2047 instances)"); return TB_ERR_UNSUPPORTED; }
    TetPatchView pv{pf->d_elem_ln, pf->d_elem_sig, pf->d_sigtab, pf->d_row_desc, pp->d_elem_cell, pf->max_lds_entries, pp->max_rows, pf->max_nodes};
    const size_t lds = (size_t)nreg * pv.kcap * sizeof(double) + (size_t)pv.max_rows * sizeof(RowDesc) + (size_t)pv.max_nodes * 3 * sizeof(double);
    const FormArgs aK = fK ? make_args(fK, t) : FormArgs{}, aM = fM ? make_args(fM, t) : FormArgs{};
    const bool fm = fM && fM->field;
    auto launch = [&](auto k) -> int {
        TB_HIP(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3((unsigned)pp->n_patches), dim3(256), lds, dev->stream, aK, aM, pv, (const uint4 *)pf->d_hdr, pf->d_pcoord, d_nzK, d_nzM, dev->d_status);
        return TB_OK;
    };
    if (fK && fM) rc = fm ? launch(k_patch_tet4<true, true, true>) : launch(k_patch_tet4<true, true, false>);
    else if (fK) rc = launch(k_patch_tet4<true, false, false>);
    else rc = fm ? launch(k_patch_tet4<false, true, true>) : launch(k_patch_tet4<false, true, false>);
    if (rc) return rc;
    TB_HIP(hipGetLastError());
    return check_status(dev);
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
    else if (m->field_kind == TB_HEX27 && f->qorder == 3) rc = run_q2(f, p, strategy, t, d_nz, nullptr);
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
    else if (m->field_kind == TB_HEX27 && f->qorder == 3) rc = run_q2(f, nullptr, strategy, t, nullptr, d_b);
    else {
        set_error("vector assembly: field kind %d with quadrature order %d not implemented", m->field_kind, f->qorder);
        return TB_ERR_UNSUPPORTED;
    }
    if (rc) return rc;
    return check_status(m->dev);
}

} // namespace tb

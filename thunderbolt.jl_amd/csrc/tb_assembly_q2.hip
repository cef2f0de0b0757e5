// tb_assembly_q2.hip — scalar forms on the triquadratic field (Lagrange order 2 on hexahedra, 27 dofs and 27 Gauss points per cell): mass and
// diffusion matrices (launch_q2_matrix) and the analytical-source vector (launch_q2_vector).  Mₑ, Kₑ are 27×27 — too large for the
// one-thread-per-cell register kernels of tb_assembly.hip, so workgroups integrate the cells and the entries reach the CSR arrays through a
// per-cell table of row positions (k_build_q2pos):
//  * ELEMENT strategy: k_matrix_q2_sf (sum-factorised, three cells per pass) stores every Kₑ in tensor order, k_gather_rows_q2 sums the CSR rows from
//    them in ascending cell order — no atomics, bit-reproducible;
//  * ATOMIC and PER_COLOR: k_matrix_q2 (matrix cores, one cell per pass) hands its entries over in entry order and scatters them itself;
//  * sources: k_vector_q2, one wave per cell.
// Constant and first-order nodal coefficients (the reference's mass.jl:28-43 / diffusion.jl:28-50, analytical_coefficient.jl:89-99).  Each position
// table is built when the first strategy that reads it runs (ensure_q2pos), so a user of one strategy does not pay for the other's table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "tb_assembly_dev.hpp"
#include "tb_elem.hpp"
#include "tb_internal.h"

namespace tb {
using namespace tbk;

// Ferrite node a → its tensor index, two bits per direction: t₀ | t₁ << 2 | t₂ << 4
__constant__ uint8_t g_q2_tix[27] = {
    0 | 0 << 2 | 0 << 4, 2 | 0 << 2 | 0 << 4, 2 | 2 << 2 | 0 << 4, 0 | 2 << 2 | 0 << 4, 0 | 0 << 2 | 2 << 4, 2 | 0 << 2 | 2 << 4, 2 | 2 << 2 | 2 << 4,
    0 | 2 << 2 | 2 << 4, 1 | 0 << 2 | 0 << 4, 2 | 1 << 2 | 0 << 4, 1 | 2 << 2 | 0 << 4, 0 | 1 << 2 | 0 << 4, 1 | 0 << 2 | 2 << 4, 2 | 1 << 2 | 2 << 4,
    1 | 2 << 2 | 2 << 4, 0 | 1 << 2 | 2 << 4, 0 | 0 << 2 | 1 << 4, 2 | 0 << 2 | 1 << 4, 2 | 2 << 2 | 1 << 4, 0 | 2 << 2 | 1 << 4, 1 | 1 << 2 | 0 << 4,
    1 | 0 << 2 | 1 << 4, 2 | 1 << 2 | 1 << 4, 1 | 2 << 2 | 1 << 4, 0 | 1 << 2 | 1 << 4, 1 | 1 << 2 | 2 << 4, 1 | 1 << 2 | 1 << 4};

// its inverse: tensor index t₀ + 3 t₁ + 9 t₂ → Ferrite node
__constant__ uint8_t g_q2_node[27] = {0, 8, 1, 11, 20, 9, 3, 10, 2, 16, 21, 17, 24, 26, 22, 19, 23, 18, 4, 12, 5, 15, 25, 13, 7, 14, 6};

// position of column dof(j) inside row dof(i), per cell and pair (cell-major: one coalesced 729-entry read per workgroup)
// TL: the table in the order of the stored element matrices of the element strategy (k_matrix_q2_sf: entry 27·(i₀ + 3 i₁ + 9 i₂) + 9 j₂ + 3 j₀ + j₁)
template <bool TL>
__global__ void k_build_q2pos(const int32_t *__restrict__ cell_dofs, int64_t n_cells, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                              uint16_t *__restrict__ pos, Status *st)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= n_cells * 729) return;
    const int64_t cell = tid / 729;
    int i = (int)(tid % 729) / 27, j = (int)(tid % 27);
    if (TL) { i = g_q2_node[i]; j = g_q2_node[(j / 3) % 3 + 3 * (j % 3) + 9 * (j / 9)]; }
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
// tile of a symmetric form is never computed (SYM: 3 tiles instead of 4).
// Reference-element values are formed from the 1-D factors in registers (no table loads); geometry per point: q2_point_geometry.
typedef double q2_d4 __attribute__((ext_vector_type(4)));

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
// operand buffer.  Tiles leave the accumulator registers for an LDS copy of Kₑ, from which the tile waves scatter the 729 entries in entry order.
template <int FORM, bool FIELD, bool SYM>
__global__ void __launch_bounds__(256, 3)
k_matrix_q2(MeshView m, FormArgs fa, const double *__restrict__ cell_xyz, const int32_t *__restrict__ list, int64_t n_list, const int64_t *__restrict__ rowptr,
            const uint16_t *__restrict__ pos, double *__restrict__ nz, int atomic /*0 rmw (per colour), 1 atomic*/, Status *st)
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
            if (tid < 27) s_dof[tid] = m.cell_dofs[cell * 27 + tid];
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
            // D[row g + 4·reg][col lr]: the tile goes through LDS so that the position table is read, and the row pointers are looked up, in entry order
            const int j = 16 * tj + lr;
            if (j < 27) {
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int i = 16 * ti + g + 4 * rg;
                    if (i >= 27) continue;
                    s_out[27 * i + j] = acc[rg];
                    if (SYM && wv == 1) s_out[27 * j + i] = acc[rg];
                }
            }
        }
        lds_barrier();
        if constexpr (TILE) {
            const int64_t pbase = cell * 729;
            for (int e = tid; e < 729; e += NC) {
                const int64_t k = rowptr[s_dof[e / 27]] + pos[pbase + e];
                if (atomic) unsafeAtomicAdd(nz + k, s_out[e]); else nz[k] += s_out[e];
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

// Sum-factorised form of the same element matrices: the kernel of the ELEMENT strategy, which stores every Kₑ for k_gather_rows_q2 (the matrix-core
// kernel above is the kernel of the scattering strategies: it hands its entries over in entry order).  With the
// coefficient pulled back to the reference cell (S_q above) the sum over the 27 Gauss points is three one-dimensional contractions, because node
// i ↔ (i₀, i₁, i₂), point q ↔ (q₀, q₁, q₂) and ∂̂ₘNᵢ(ξ_q) = Π_dim ψ(dim == m)_{i_dim}(q_dim), ψ(false) = φ, ψ(true) = φ′:
//   stage 1  Z1[m][n][q₁][q₂][i₀][j₀] = Σ_q₀ ψ(m==0)_{i₀}(q₀) ψ(n==0)_{j₀}(q₀) S_q[m][n]                     (81 lane-tasks per cell: 36 multiply-adds)
//   stages 2 + 3 in registers, task (i₀, j₀, i₁, j₁): contract q₁ — after which only "m is 2 or not" matters — then q₂ → the nine entries (i₂, j₂)
//                                                                                                              (81 tasks: 171 multiply-adds, 81 LDS reads)
// ≈ 1.7·10⁴ multiply-adds per cell for the stiffness matrix instead of 5.9·10⁴ (mass: 9 + 81 small tasks), on the vector ALUs.  A workgroup takes
// THREE cells per pass so that the 81-task stages fill 243 of its 256 lanes; 24 KB of LDS, persistent, the vertex coordinates of the next triple
// requested one pass ahead.  History (docs/rounds/): with the matrix-core kernel storing its Kₑ the stiffness integration alone took 1.07 ms at
// 64³ against 0.64 ms here, which is why that kernel no longer has a store path; a build of this kernel forced
// to three waves per SIMD spilled 200 B and took 1.19 ms; a wave-per-cell form without workgroup barriers (81 tasks in two rounds of 64 lanes,
// geometry on 27 lanes) 0.85 ms — the half-empty second rounds cost more than the barriers.  Same sums as mass.jl:28-43 / diffusion.jl:28-50 in
// another order (≲ 1e-15 relative); no symmetry assumed, so non-symmetric constant tensors need no variant of their own.
// (Round 6: the element matrices of a triple sent through LDS and stored as one run of 3 × 729 doubles — every wave store 512 contiguous bytes instead of
// seven 72-byte pieces — was built and measured at 64³: mass 1.02 against 1.04 ms, diffusion 1.29 against 1.22 ms for integration + gather: the stores were
// not what the diffusion kernel waits for, the extra barrier and 17 KB of LDS traffic per pass cost more.  Removed; profiles/r06_v1/ab_q2_element_matrices_through_lds.log.)
template <int FORM, bool FIELD>
__global__ void __launch_bounds__(256, 2)
k_matrix_q2_sf(MeshView m, FormArgs fa, const double *__restrict__ cell_xyz, int64_t n_cells, double *__restrict__ ke, Status *st)
{
    constexpr bool DIFF = FORM == TB_FORM_DIFFUSION;
    constexpr int NS = DIFF ? 9 : 1, NZ1 = DIFF ? 729 : 81;
    constexpr double GX = 0.7745966692414834;
    __shared__ double s_x[3][24], s_rho[3][8], s_S[3][27][NS], s_Z1[3][NZ1];
    const int tid = threadIdx.x;
    auto PH = [](int i, int q) constexpr { return i == 0 ? 0.5 * (GX * (q - 1)) * (GX * (q - 1) - 1.0) : i == 1 ? 1.0 - (GX * (q - 1)) * (GX * (q - 1)) : 0.5 * (GX * (q - 1)) * (GX * (q - 1) + 1.0); };
    auto DP = [](int i, int q) constexpr { return i == 0 ? GX * (q - 1) - 0.5 : i == 1 ? -2.0 * (GX * (q - 1)) : GX * (q - 1) + 0.5; };
    const int64_t ntrip = (n_cells + 2) / 3; // a pass takes cells 3·trip, + 1, + 2; the last triple may be ragged
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
    // inputs of a triple: lanes 0–71 one vertex coordinate each, lanes 96–119 one nodal density each
    auto request = [&](int64_t trip, double &px, double &pr) {
        px = 0.0; pr = 0.0;
        if (tid < 72) { const int64_t k = 3 * trip + tid / 24; if (k < n_cells) px = cell_xyz[k * 24 + tid % 24]; }
        if constexpr (!DIFF && FIELD) if (tid >= 96 && tid < 120) { const int64_t k = 3 * trip + (tid - 96) / 8; if (k < n_cells) pr = fa.field[k * 8 + (tid - 96) % 8]; }
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
        const int64_t cell = 3 * trip + kc;
        const bool live = tid < 243 && cell < n_cells;
        // geometry of the 27 points of each cell: lane = (cell of the triple, point)
        if (tid < 81) {
            const int k = tid / 27, q = tid - 27 * k;
            const int64_t c = 3 * trip + k;
            if (c < n_cells) {
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
            // the element matrices are stored in TENSOR order: row i₀ + 3 i₁ + 9 i₂, column 9 j₂ + 3 j₀ + j₁, so that the nine lanes (j₀, j₁) of a
            // row store nine consecutive doubles and the three stores j₂ = 0, 1, 2 complete its 216 bytes (in Ferrite's node order the 64 lanes of a
            // store hit 64 separate 8-byte pieces of the 5.8 KB block: the mass kernel, whose arithmetic is a fifth of the diffusion kernel's, took 0.49
            // of that one's 0.61 ms — bound by the store path); k_gather_rows_q2 reads the rows in this order
            const int etl = 27 * (ti0 + 3 * ti1) + 3 * tj0 + tj1;
#pragma unroll
            for (int i2 = 0; i2 < 3; ++i2)
#pragma unroll
                for (int j2 = 0; j2 < 3; ++j2) ke[pbase + etl + 243 * i2 + 9 * j2] = out[i2][j2];
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

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
// the position table in Ferrite's order (tb_pattern::d_q2pos: the scattering strategies) or in the order of the stored element matrices
// (d_q2pos_t: the element strategy), built when the first strategy that reads it runs
static int ensure_q2pos(tb_pattern *p, bool tensor_order)
{
    uint16_t *&tab = tensor_order ? p->d_q2pos_t : p->d_q2pos;
    if (tab) return TB_OK;
    tb_mesh *m = p->mesh;
    const int64_t n = m->n_cells * 729;
    TB_HIP(hipMalloc((void **)&tab, sizeof(uint16_t) * n));
    TB_TRY(reset_status(m->dev));
    auto build = tensor_order ? k_build_q2pos<true> : k_build_q2pos<false>;
    hipLaunchKernelGGL(build, dim3(nblocks(n, 256)), dim3(256), 0, m->dev->stream, m->d_cell_dofs, m->n_cells, p->d_rowptr, p->d_colidx, tab, m->dev->d_status);
    TB_HIP(hipGetLastError());
    return check_status(m->dev);
}

// ElementAssemblyStrategy: every Kₑ stored by the sum-factorised kernel (three cells per pass, persistent: six workgroups per CU), then one gather over
// all rows.  (A chunked form — gather of a chunk's rows on a second queue beside the integration of the next chunk, the scheme of the mechanics
// linearisation — was built, bit-identical and slower: 1.43 / 1.53 / 1.64 ms in 4 / 8 / 16 chunks against 1.31 ms at 64³; removed in round 5,
// docs/rounds/r04.md)
static int q2_matrix_element(tb_form *f, tb_pattern *p, const MeshView &mv, const FormArgs &fa, double *d_nz)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    if (!m->ea) TB_TRY(build_ea_plan(m));
    TB_TRY(ensure_buffer(p->d_kebuf, p->kebuf_bytes, sizeof(double) * (size_t)m->n_cells * 729, "element-matrix buffer"));
    ensure_max_row_len(p);
    const int max_row = (int)p->max_row_len;
    TB_TRY(ensure_ea_ell(m));
    TB_TRY(ensure_q2pos(p, true));
    TB_TRY(ensure_ea_ell_q2t(m));
    const unsigned wg3 = (unsigned)std::min<int64_t>((m->n_cells + 2) / 3, (int64_t)dev->n_cu * 6);
#define TB_Q2S(FORM, FIELD) hipLaunchKernelGGL((k_matrix_q2_sf<FORM, FIELD>), dim3(wg3), dim3(256), 0, dev->stream, mv, fa, m->d_cell_xyz, m->n_cells, p->d_kebuf, dev->d_status)
    if (f->kind == TB_FORM_MASS) { if (f->field) TB_Q2S(TB_FORM_MASS, true); else TB_Q2S(TB_FORM_MASS, false); }
    else { if (f->field) TB_Q2S(TB_FORM_DIFFUSION, true); else TB_Q2S(TB_FORM_DIFFUSION, false); }
#undef TB_Q2S
    TB_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gather_rows_q2, dim3((unsigned)((m->ndofs + 7) / 8)), dim3(256), sizeof(double) * 8 * (size_t)max_row, dev->stream, (int64_t)0, m->ndofs, m->ea->d_ell_t,
                       m->ea->ell_w, p->d_kebuf, p->d_q2pos_t, p->d_rowptr, d_nz, max_row);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int launch_q2_matrix(tb_form *f, tb_pattern *p, int strategy, double t, double *d_nz)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    if (strategy != TB_STRATEGY_ELEMENT && strategy != TB_STRATEGY_ATOMIC && strategy != TB_STRATEGY_PER_COLOR) {
        set_error("Q2 scalar forms: strategy %d not supported (use TB_STRATEGY_ELEMENT, TB_STRATEGY_ATOMIC or TB_STRATEGY_PER_COLOR)", strategy);
        return TB_ERR_UNSUPPORTED;
    }
    // first assembly with a nodal coefficient field: tabulate the tensor at the 27 points from the first-order nodal data
    if (f->field && f->kind == TB_FORM_DIFFUSION && !f->d_dtab) TB_TRY(tabulate_diffusion_field_q2(f));
    TB_TRY(ensure_cell_xyz(m));
    const MeshView mv = make_view(m);
    const FormArgs fa = make_args(f, t);
    if (strategy == TB_STRATEGY_ELEMENT) return q2_matrix_element(f, p, mv, fa, d_nz);
    TB_TRY(ensure_q2pos(p, false));
    TB_HIP(hipMemsetAsync(d_nz, 0, (size_t)p->nnz * sizeof(double), dev->stream));
    auto scatter = [&](const int32_t *list, int64_t n, int atomic) -> int {
        if (n == 0) return TB_OK;
        const unsigned wgs = (unsigned)std::min<int64_t>(n, (int64_t)dev->n_cu * 3); // persistent workgroups: three per CU (≤ 168 VGPRs)
#define TB_Q2(FORM, FIELD, SYM) hipLaunchKernelGGL((k_matrix_q2<FORM, FIELD, SYM>), dim3(wgs), dim3(256), 0, dev->stream, mv, fa, m->d_cell_xyz, list, n, p->d_rowptr, p->d_q2pos, d_nz, atomic, dev->d_status)
        if (f->kind == TB_FORM_MASS) { if (f->field) TB_Q2(TB_FORM_MASS, true, true); else TB_Q2(TB_FORM_MASS, false, true); }
        else {
            // a non-symmetric constant tensor gives a non-symmetric Kₑ: all four tiles
            const bool sym = f->field || (fa.D[1] == fa.D[3] && fa.D[2] == fa.D[6] && fa.D[5] == fa.D[7]);
            if (f->field) TB_Q2(TB_FORM_DIFFUSION, true, true); else if (sym) TB_Q2(TB_FORM_DIFFUSION, false, true); else TB_Q2(TB_FORM_DIFFUSION, false, false);
        }
#undef TB_Q2
        TB_HIP(hipGetLastError());
        return TB_OK;
    };
    if (strategy == TB_STRATEGY_ATOMIC) return scatter(nullptr, m->n_cells, 1);
    if (!m->colors) TB_TRY(build_color_plan(m));
    for (int c = 0; c < m->colors->ncolors; ++c) TB_TRY(scatter(m->colors->d_cells + m->colors->offsets[c], m->colors->offsets[c + 1] - m->colors->offsets[c], 0));
    return TB_OK;
}

int launch_q2_vector(tb_form *f, int strategy, double t, double *d_b)
{
    tb_mesh *m = f->mesh;
    tb_device *dev = m->dev;
    if (strategy != TB_STRATEGY_ELEMENT && strategy != TB_STRATEGY_ATOMIC && strategy != TB_STRATEGY_PER_COLOR) {
        set_error("Q2 scalar forms: strategy %d not supported (use TB_STRATEGY_ELEMENT, TB_STRATEGY_ATOMIC or TB_STRATEGY_PER_COLOR)", strategy);
        return TB_ERR_UNSUPPORTED;
    }
    TB_TRY(ensure_cell_xyz(m));
    const MeshView mv = make_view(m);
    const FormArgs fa = make_args(f, t);
    TB_HIP(hipMemsetAsync(d_b, 0, (size_t)m->ndofs * sizeof(double), dev->stream));
    auto scatter = [&](const int32_t *list, int64_t n, int atomic) -> int {
        if (n == 0) return TB_OK;
        hipLaunchKernelGGL(k_vector_q2, dim3((unsigned)n), dim3(64), 0, dev->stream, mv, fa, m->d_cell_xyz, list, d_b, atomic, dev->d_status);
        TB_HIP(hipGetLastError());
        return TB_OK;
    };
    if (strategy != TB_STRATEGY_PER_COLOR) return scatter(nullptr, m->n_cells, 1); // the element strategy of a vector: atomic adds
    if (!m->colors) TB_TRY(build_color_plan(m));
    for (int c = 0; c < m->colors->ncolors; ++c) TB_TRY(scatter(m->colors->d_cells + m->colors->offsets[c], m->colors->offsets[c + 1] - m->colors->offsets[c], 0));
    return TB_OK;
}

} // namespace tb

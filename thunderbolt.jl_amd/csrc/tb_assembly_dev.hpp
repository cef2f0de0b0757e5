// tb_assembly_dev.hpp — what the assembly units (tb_assembly.hip, tb_assembly_q2.hip, tb_assembly_tet4.hip) share besides the argument views of
// tb_forms.hpp: the closed forms of the analytical sources, the negative-Jacobian flag and the grid-size helper of the launchers.
#pragma once
#include "tb_forms.hpp"
#include "tb_math.hpp"

namespace tb {

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

__device__ __forceinline__ void flag_neg_detj(Status *st, int64_t cell)
{
    st->neg_detj = 1;
    st->cell = cell;
}

static inline unsigned nblocks(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

} // namespace tb

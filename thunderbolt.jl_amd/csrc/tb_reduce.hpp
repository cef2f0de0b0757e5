// tb_reduce.hpp — sums and maxima over the workgroups of a launch, shared by the units that end a kernel in one (tb_spmv.hip, tb_krylov.hip, tb_algebra.hip,
// tb_reaction.hip): the workgroup sums (device, inline), the slot groups they leave through, the NaN-keeping maximum and its atomicMax key, and the grids
// of the kernels that use them (host, inline).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "tb_internal.h"

namespace tb {

// grid of a kernel of 1 024-thread workgroups that ends in a workgroup sum (block_sum_to): two per CU
static inline unsigned grid_red(tb_device *dev, int64_t n)
{
    const int64_t nb = (n + 1023) / 1024, cap = (int64_t)dev->n_cu * 2;
    return (unsigned)std::max<int64_t>(1, nb > cap ? cap : nb);
}
static inline unsigned grid_for(tb_device *dev, int64_t n, int bs)
{
    int64_t nb = (n + bs - 1) / bs;
    const int64_t cap = (int64_t)dev->n_cu * 8;
    return (unsigned)(nb > cap ? cap : nb);
}
// grid of a kernel that gives every work item its own thread: ⌈n / bs⌉ workgroups, at least one
static inline unsigned blocks_of(int64_t n, int bs) { return (unsigned)std::max<int64_t>(1, (n + bs - 1) / bs); }

// ---- one maximum ----
// max(a, b) that keeps a NaN of either operand (fmax returns the other one): the `max` of Julia's `maximum`, which the reaction-tangent controller
// reads (src/solver/time/rtc.jl:57-73) — a point that has blown up has to reach the host.  One compare more than fmax.
__device__ __forceinline__ double max_nan(double a, double b) { return (b > a || b != b) ? b : a; }
// Order-preserving map double → uint64, so atomicMax works on signed values: a total order of the finite values and ±∞ with key(−∞) > 0 (0 = "no
// element yet").  EVERY NaN, whatever its sign or payload, maps to the largest key, above key(+∞): by its bits alone a negative-sign NaN (0xfff8…, what
// x86 produces for 0/0) would sort below −∞ and lose.  decode_ordered_key (tb_algebra.hip) turns that key back into a quiet NaN.
__device__ __forceinline__ unsigned long long ordered_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return v != v ? ~0ull : (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// ---- one scalar ----
// *out += the sum of v over the workgroup (4 … 16 waves).  ONE atomic per workgroup on one address: 12.2 ns each, serialised ("reduction slots" below) —
// the kernels that end this way and run once per solver iteration are launched as 1 024-thread workgroups, two per CU (grid_red): a quarter of the
// atomics of 256-thread workgroups at the same number of threads in flight.
__device__ __forceinline__ void block_sum_to(double v, double *out)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __shared__ double sm[16];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sm[0] + sm[1] + sm[2] + sm[3];
        for (int k = 4; k < (int)(blockDim.x >> 6); ++k) t += sm[k];
        unsafeAtomicAdd(out, t);
    }
}

// two sums of a 256-thread block with one barrier: out[0] += Σ a, out[1] += Σ c (the two atomics leave from different waves)
__device__ __forceinline__ void block_sum2_to(double a, double c, double *out)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
    __shared__ double sm2[8];
    if ((threadIdx.x & 63) == 0) { sm2[threadIdx.x >> 6] = a; sm2[4 + (threadIdx.x >> 6)] = c; }
    __syncthreads();
    if (threadIdx.x == 0) unsafeAtomicAdd(out, sm2[0] + sm2[1] + sm2[2] + sm2[3]);
    if (threadIdx.x == 64) unsafeAtomicAdd(out + 1, sm2[4] + sm2[5] + sm2[6] + sm2[7]);
}

// ---- reduction slots ----
// A sum over the workgroups of a launch that ends in one atomic per workgroup on ONE address costs 12.2 ns per workgroup on MI355X — same-address (and
// same-128-byte-line) atomics serialise in L2, FP64 and integer alike (scripts/microbench/tail_atomics.hip: 2 048 co-resident workgroups, two scalars of
// one line: 51 µs; the CG update kernel on a 27-layer slab spent 23 of its 37 µs there).  The partial of workgroup b goes to slot b mod 64 of a GROUP of 64
// slots 128 B apart instead (3 µs for the same 2 048), and whoever needs the sum adds the 64 slots: the next kernel of a fused sequence (read_slots: the
// same xor tree in every wave, so every workgroup sees the same bits), or k_fold_slots (one wave) into a caller-owned scalar for the public one-kernel
// entries.  Groups live in tb_device::d_slots and are zero between uses; launches of one device are stream-ordered.  RED_SLOTS, RED_STRIDE and
// RED_GROUP are in tb_internal.h (tb_chamber.hip folds its volume through group 0 as well); k_fold_slots and its launcher fold_slots are in tb_algebra.hip.
__device__ __forceinline__ void block_sum_slots(double v, double *group)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __shared__ double sms[4];
    if ((threadIdx.x & 63) == 0) sms[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) unsafeAtomicAdd(group + RED_STRIDE * (blockIdx.x & (RED_SLOTS - 1)), sms[0] + sms[1] + sms[2] + sms[3]);
}
__device__ __forceinline__ void block_sum2_slots(double a, double c, double *ga, double *gc)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
    __shared__ double sms2[8];
    if ((threadIdx.x & 63) == 0) { sms2[threadIdx.x >> 6] = a; sms2[4 + (threadIdx.x >> 6)] = c; }
    __syncthreads();
    if (threadIdx.x == 0) unsafeAtomicAdd(ga + RED_STRIDE * (blockIdx.x & (RED_SLOTS - 1)), sms2[0] + sms2[1] + sms2[2] + sms2[3]);
    if (threadIdx.x == 64) unsafeAtomicAdd(gc + RED_STRIDE * (blockIdx.x & (RED_SLOTS - 1)), sms2[4] + sms2[5] + sms2[6] + sms2[7]);
}
// the sum of a group, in every lane (call with all 64 lanes of the wave active)
__device__ __forceinline__ double read_slots(const double *group)
{
    double v = group[RED_STRIDE * (threadIdx.x & 63)];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// group k of the device
static inline double *red_group(tb_device *dev, int k) { return dev->d_slots + (size_t)k * RED_GROUP; }

} // namespace tb

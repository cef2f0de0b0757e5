// tb_algebra.hip — the vector and entry-wise algebra around the assembled operators (all HBM-bound streams); products are in tb_spmv.hip, solvers in tb_krylov.hip:
//   Anz = Mnz − Δt·Knz                src/solver/time/euler.jl:110-116
//   y += a·x                          add!(b, source), euler.jl:90
//   max |x[i·stride]|, max x[i·stride] RTC controller input, src/solver/time/rtc.jl:64-73
//   a·b                               tb_dot
//   apply_zero!, meandiag             Dirichlet rows and columns of a device CSR matrix (Ferrite)
//   gather / scatter by index lists   halo pack and unpack of the multi-GPU path
//   k_fold_slots                      a slot group of tb_reduce.hpp into a caller-owned scalar
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "tb_internal.h"
#include "tb_reduce.hpp"

namespace tb {

__global__ void __launch_bounds__(256)
k_heat_matrix(int64_t n, const double *__restrict__ M, const double *__restrict__ K, double dt, double *__restrict__ A)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n2 = n >> 1;
    const double2 *M2 = (const double2 *)M;
    const double2 *K2 = (const double2 *)K;
    double2 *A2 = (double2 *)A;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        const double2 m = M2[i], k = K2[i];
        A2[i] = make_double2(m.x - dt * k.x, m.y - dt * k.y);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) A[n - 1] = M[n - 1] - dt * K[n - 1];
}

__global__ void __launch_bounds__(256) k_axpy(int64_t n, double a, const double *__restrict__ x, double *__restrict__ y)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) y[i] += a * x[i];
}

// Both maxima keep a NaN (max_nan, tb_reduce.hpp): any NaN in the addressed slice makes the result NaN, as Julia's `maximum` does.
__global__ void __launch_bounds__(256)
k_absmax(int64_t n, const double *__restrict__ x, int64_t stride_x, unsigned long long *__restrict__ out)
{
    double m = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) m = max_nan(m, fabs(x[i * stride_x]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max_nan(m, __shfl_xor(m, o, 64));
    __shared__ double sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max_nan(max_nan(sm[0], sm[1]), max_nan(sm[2], sm[3]));
        // non-negative doubles order like their bit patterns, and a NaN of positive sign lies above +∞ in that order: it wins the atomicMax
        // (m is +0 or an operand that went through fabs above, so its sign bit is clear)
        atomicMax(out, (unsigned long long)__double_as_longlong(m));
    }
}

__global__ void __launch_bounds__(256)
k_max(int64_t n, const double *__restrict__ x, int64_t stride_x, unsigned long long *__restrict__ out)
{
    double m = -__builtin_huge_val();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) m = max_nan(m, x[i * stride_x]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max_nan(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out, ordered_key(m)); // (NaN: the largest key)
}

int launch_heat_matrix(tb_device *dev, int64_t nnz, const double *M, const double *K, double dt, double *A)
{
    hipLaunchKernelGGL(k_heat_matrix, dim3(grid_for(dev, (nnz + 1) / 2, 256)), dim3(256), 0, dev->stream, nnz, M, K, dt, A);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int launch_axpy(tb_device *dev, int64_t n, double a, const double *x, double *y)
{
    hipLaunchKernelGGL(k_axpy, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, a, x, y);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int launch_absmax(tb_device *dev, int64_t n, const double *x, int64_t stride, double *result)
{
    TB_NO_CAPTURE(dev); // the result goes to the host
    unsigned long long *d_out = (unsigned long long *)dev->d_readback;
    TB_HIP(hipMemsetAsync(d_out, 0, sizeof(unsigned long long), dev->stream));
    hipLaunchKernelGGL(k_absmax, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, x, stride, d_out);
    TB_HIP(hipGetLastError());
    return read_back(dev, result, dev->d_readback, 1); // the key of a non-negative double is its bit pattern
}

double decode_ordered_key(unsigned long long k)
{
    if (k == ~0ull) return __builtin_nan(""); // the key of every NaN (ordered_key, tb_reduce.hpp)
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &b, sizeof v);
    return v;
}

int launch_max(tb_device *dev, int64_t n, const double *x, int64_t stride, double *result)
{
    TB_NO_CAPTURE(dev); // the result goes to the host
    unsigned long long *d_out = (unsigned long long *)dev->d_readback;
    TB_HIP(hipMemsetAsync(d_out, 0, sizeof(unsigned long long), dev->stream)); // key 0 < key(−∞)
    if (n > 0) {
        hipLaunchKernelGGL(k_max, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, x, stride, d_out);
        TB_HIP(hipGetLastError());
    }
    double key = 0.0;
    TB_TRY(read_back(dev, &key, dev->d_readback, 1));
    unsigned long long bits;
    memcpy(&bits, &key, sizeof bits);
    *result = bits ? decode_ordered_key(bits) : -__builtin_huge_val();
    return TB_OK;
}

// out[k] += sum of group k, the groups back to zero (k < ngroups ≤ 4; one wave per group)
__global__ void __launch_bounds__(256) k_fold_slots(double *__restrict__ groups, double *__restrict__ out, int ngroups)
{
    const int k = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (k >= ngroups) return;
    double *g = groups + (size_t)k * RED_GROUP;
    const double v = read_slots(g);
    g[RED_STRIDE * l] = 0.0;
    if (l == 0) out[k] += v;
}
void fold_slots(tb_device *dev, int first_group, double *d_out, int ngroups)
{
    hipLaunchKernelGGL(k_fold_slots, dim3(1), dim3(256), 0, dev->stream, red_group(dev, first_group), d_out, ngroups);
}

__global__ void __launch_bounds__(1024) k_dot(int64_t n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ out)
{
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) s += a[i] * b[i];
    block_sum_to(s, out);
}

// *d_out += a·b, enqueued only (what the solvers of tb_krylov.hip put between their other kernels)
void enqueue_dot(tb_device *dev, int64_t n, const double *a, const double *b, double *d_out)
{
    hipLaunchKernelGGL(k_dot, dim3(grid_red(dev, n)), dim3(1024), 0, dev->stream, n, a, b, d_out);
}

int launch_dot(tb_device *dev, int64_t n, const double *a, const double *b, double *result)
{
    TB_NO_CAPTURE(dev); // the result goes to the host
    double *scal = dev->d_readback;
    TB_HIP(hipMemsetAsync(scal, 0, sizeof(double), dev->stream));
    if (n > 0) {
        enqueue_dot(dev, n, a, b, scal);
        TB_HIP(hipGetLastError());
    }
    return read_back(dev, result, scal, 1);
}

// apply_zero!(K, f, ch) on device CSR (Ferrite.apply_zero!; CSR method src/utils.jl:263-278, call sites
// src/solver/nonlinear/nlsolve_common.jl:12-26): rows and columns of prescribed dofs are zeroed, their diagonal entry is set
// to `diag` (Ferrite uses the mean diagonal so the conditioning survives), f is zeroed there.  8 lanes per row.
__global__ void __launch_bounds__(256)
k_apply_zero_csr(int64_t nrows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const uint8_t *__restrict__ flags,
                 double diag, double *__restrict__ nz, double *__restrict__ f)
{
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    const int sub = threadIdx.x & 7;
    if (r >= nrows) return;
    const bool pr = flags[r];
    if (nz)
        for (int64_t k = rowptr[r] + sub; k < rowptr[r + 1]; k += 8) {
            const int32_t c = colidx[k];
            if (pr) nz[k] = c == r ? diag : 0.0;
            else if (flags[c]) nz[k] = 0.0;
        }
    if (f && pr && sub == 0) f[r] = 0.0;
}

// Σ |diag| / n (Ferrite.meandiag)
__global__ void __launch_bounds__(256)
k_sum_absdiag(int64_t nrows, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ nz, double *__restrict__ out)
{
    double s = 0.0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrows; r += stride)
        for (int64_t k = rowptr[r]; k < rowptr[r + 1]; ++k)
            if (colidx[k] == r) { s += fabs(nz[k]); break; }
    block_sum_to(s, out);
}

int launch_apply_zero(tb_pattern *pat, double *nz, double *f, const uint8_t *flags, double diag)
{
    tb_device *dev = pat->mesh->dev;
    const int64_t n = pat->n_rows;
    if (!n) return TB_OK;
    hipLaunchKernelGGL(k_apply_zero_csr, dim3((unsigned)((n * 8 + 255) / 256)), dim3(256), 0, dev->stream, n, pat->d_rowptr, pat->d_colidx, flags, diag, nz, f);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

int launch_meandiag(tb_pattern *pat, const double *nz, double *result)
{
    tb_device *dev = pat->mesh->dev;
    TB_NO_CAPTURE(dev); // the result goes to the host
    const int64_t n = pat->n_rows;
    *result = 0.0;
    if (!n) return TB_OK;
    double *scal = dev->d_readback;
    TB_HIP(hipMemsetAsync(scal, 0, 2 * sizeof(double), dev->stream));
    hipLaunchKernelGGL(k_sum_absdiag, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, pat->d_rowptr, pat->d_colidx, nz, scal);
    TB_HIP(hipGetLastError());
    double h = 0.0;
    TB_TRY(read_back(dev, &h, scal, 1));
    *result = h / (double)n;
    return TB_OK;
}

// ---- halo pack / unpack and the packed interface rows of a product (multi-GPU path) ----
__global__ void __launch_bounds__(256) k_gather_indexed(int64_t n, const double *__restrict__ vec, const int32_t *__restrict__ idx, double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = vec[idx[i]];
}

__global__ void __launch_bounds__(256) k_scatter_add_indexed(int64_t n, const double *__restrict__ in, const int32_t *__restrict__ idx, double *__restrict__ vec)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) vec[idx[i]] += in[i]; // indices of one call are distinct
}

__global__ void __launch_bounds__(256) k_scatter_indexed(int64_t n, const double *__restrict__ in, const int32_t *__restrict__ idx, double *__restrict__ vec)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) vec[idx[i]] = in[i];
}

int launch_gather_indexed(tb_device *dev, int64_t n, const double *vec, const int32_t *idx, double *out)
{
    if (n > 0) hipLaunchKernelGGL(k_gather_indexed, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, vec, idx, out);
    TB_HIP(hipGetLastError());
    return TB_OK;
}
int launch_scatter_add_indexed(tb_device *dev, int64_t n, const double *in, const int32_t *idx, double *vec)
{
    if (n > 0) hipLaunchKernelGGL(k_scatter_add_indexed, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, in, idx, vec);
    TB_HIP(hipGetLastError());
    return TB_OK;
}
int launch_scatter_indexed(tb_device *dev, int64_t n, const double *in, const int32_t *idx, double *vec)
{
    if (n > 0) hipLaunchKernelGGL(k_scatter_indexed, dim3(grid_for(dev, n, 256)), dim3(256), 0, dev->stream, n, in, idx, vec);
    TB_HIP(hipGetLastError());
    return TB_OK;
}

} // namespace tb

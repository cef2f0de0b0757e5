// Device build of thunderbolt.jl_amd/csrc/tb_math.hpp for tests/test_tt06_derived_constants.py (test only: not part of libtbhip.so).  One kernel per function,
// y[i] = f(x[i]), compiled by the test with the library's own flags, so that the values are the ones the reaction kernels get from v_rcp_f64 / v_rsq_f64,
// the Newton steps and the polynomials under -O3 -ffp-contract=fast.  The test compares them with the host build (tests/tb_math_host.cpp) and long double.
#include <hip/hip_runtime.h>

#include "tb_math.hpp"

namespace {

__global__ void __launch_bounds__(256) k_exp_b(const double *__restrict__ x, double *__restrict__ y, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = tb::exp_b(x[i]);
}

__global__ void __launch_bounds__(256) k_rcp_b(const double *__restrict__ x, double *__restrict__ y, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = tb::rcp_b(x[i]);
}

// y2: the form rsqrt_b replaced (an IEEE division by an IEEE square root), from the same kernel on the same arguments
__global__ void __launch_bounds__(256) k_rsqrt_b(const double *__restrict__ x, double *__restrict__ y, double *__restrict__ y2, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        y[i] = tb::rsqrt_b(x[i]);
        y2[i] = 1.0 / sqrt(x[i]);
    }
}

__global__ void __launch_bounds__(256) k_log_b(const double *__restrict__ x, double *__restrict__ y, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = tb::log_b(x[i]);
}

__global__ void __launch_bounds__(256) k_expm1_b(const double *__restrict__ x, double *__restrict__ y, long n)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = tb::expm1_b(x[i]);
}

} // namespace

enum { F_EXP_B = 0, F_RCP_B = 1, F_RSQRT_B = 2, F_LOG_B = 3, F_EXPM1_B = 4 };

// y[i] = f(x[i]) for host arrays of n doubles; y2 is written by F_RSQRT_B only (1/sqrt(x[i]), required there) and may be null otherwise.  Returns the status
// of the first HIP call that failed (hipSuccess = 0), −1 for a bad argument; the device buffers are freed either way.
extern "C" int tb_math_device_eval(int which, const double *x, long n, double *y, double *y2)
{
    if (which < F_EXP_B || which > F_EXPM1_B || n < 0 || (n > 0 && (!x || !y)) || (which == F_RSQRT_B && n > 0 && !y2)) return -1;
    if (n == 0) return 0;
    const size_t bytes = (size_t)n * sizeof(double);
    double *dx = nullptr, *dy = nullptr, *dy2 = nullptr;
    hipError_t rc = hipMalloc((void **)&dx, bytes);
    if (rc == hipSuccess) rc = hipMalloc((void **)&dy, bytes);
    if (rc == hipSuccess && which == F_RSQRT_B) rc = hipMalloc((void **)&dy2, bytes);
    if (rc == hipSuccess) rc = hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice);
    if (rc == hipSuccess) {
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        switch (which) {
        case F_EXP_B: hipLaunchKernelGGL(k_exp_b, grid, block, 0, 0, dx, dy, n); break;
        case F_RCP_B: hipLaunchKernelGGL(k_rcp_b, grid, block, 0, 0, dx, dy, n); break;
        case F_RSQRT_B: hipLaunchKernelGGL(k_rsqrt_b, grid, block, 0, 0, dx, dy, dy2, n); break;
        case F_LOG_B: hipLaunchKernelGGL(k_log_b, grid, block, 0, 0, dx, dy, n); break;
        default: hipLaunchKernelGGL(k_expm1_b, grid, block, 0, 0, dx, dy, n); break;
        }
        rc = hipGetLastError();
    }
    if (rc == hipSuccess) rc = hipDeviceSynchronize();
    if (rc == hipSuccess) rc = hipMemcpy(y, dy, bytes, hipMemcpyDeviceToHost);
    if (rc == hipSuccess && which == F_RSQRT_B) rc = hipMemcpy(y2, dy2, bytes, hipMemcpyDeviceToHost);
    const hipError_t f1 = dx ? hipFree(dx) : hipSuccess, f2 = dy ? hipFree(dy) : hipSuccess, f3 = dy2 ? hipFree(dy2) : hipSuccess;
    if (rc == hipSuccess) rc = f1 != hipSuccess ? f1 : f2 != hipSuccess ? f2 : f3;
    return (int)rc;
}

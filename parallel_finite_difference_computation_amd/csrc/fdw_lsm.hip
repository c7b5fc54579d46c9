// fdw_lsm.hip -- the kernels of least-squares migration (fdwave.h, "Least-squares migration"; launchers in fdw_lsm.h).  All of them are
// pointwise or streaming with z-contiguous (gathers: ix-contiguous) access.  Every fp32 update is a product and a sum rounded separately
// (the build has -ffp-contract=off); every sum is in the order S of fdwave.h, which one wave of 64 lanes performs as it stands.
#include "fdw_lsm.h"

namespace fdw {

// the fold of S: s_l = s_l + s_{l+d} for l < d, d = 32 .. 1; lane 0 ends with the result (lanes >= d compute words nobody reads)
__device__ __forceinline__ double lsm_wave_sum(double s)
{
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_down(s, d, 64);
    return s;
}

// one wave per row: blockIdx.x = the row
__global__ __launch_bounds__(64) void fdw_lsm_dot_rows_kernel(const float* a, const float* b, double* rows, int ld, int r0, int c0, int c1)
{
    const size_t base = (size_t)(r0 + (int)blockIdx.x) * ld;
    double s = 0.0;
#pragma unroll 4
    for (int z = c0 + (int)threadIdx.x; z < c1; z += 64) s = s + (double)a[base + z] * (double)b[base + z];      // the product of two floats is exact
    s = lsm_wave_sum(s);
    if (threadIdx.x == 0) rows[blockIdx.x] = s;
}

__global__ __launch_bounds__(64) void fdw_lsm_finish_kernel(const double* rows, int n, double* out)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) s = s + rows[i];
    s = lsm_wave_sum(s);
    if (threadIdx.x == 0) *out = s;
}

// one wave per time row of the gather: blockIdx.x = it
__global__ __launch_bounds__(64) void fdw_lsm_gather_kernel(const float* q, const float* dobs, const float* v2, float* w_out, float* ws, double* rows, int nx,
                                                            int pitch, int nxb, int gz)
{
    const size_t base = (size_t)blockIdx.x * nx;
    double s = 0.0;
    for (int ix = threadIdx.x; ix < nx; ix += 64) {
        const float qv = q[base + ix];
        const float w = dobs ? dobs[base + ix] - qv : qv;
        s = s + (double)w * (double)w;
        if (w_out) w_out[base + ix] = w;
        ws[base + ix] = w * v2[(size_t)(nxb + ix) * pitch + gz];
    }
    s = lsm_wave_sum(s);
    if (threadIdx.x == 0) rows[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void fdw_lsm_stack_kernel(float* h, const float* img, const float* v2, const float* mask, int pitch, int x0, int z0, int z1)
{
    const int z = z0 + blockIdx.x * 256 + threadIdx.x;
    if (z >= z1) return;
    const size_t k = (size_t)(x0 + blockIdx.y) * pitch + z;
    // the correctly rounded fp32 quotient through the fp64 one (fdw_lsm.h).  The empty asm keeps the compiler from narrowing it back to the
    // fp32 expansion, whose fused multiply-adds the library keeps to the kernels listed for them (tests/test_value_domain.py).
    double qd = (double)img[k] / (double)v2[k];
    asm volatile("" : "+v"(qd));
    const float t = (float)qd;
    h[k] = h[k] + (mask ? mask[k] * t : t);
}

// one wave per row of C: blockIdx.x = x - x0
__global__ __launch_bounds__(64) void fdw_lsm_update_kernel(float* m, float* g, const float* p, const float* h, const double* alpha, double* rows, int pitch,
                                                            int x0, int z0, int z1)
{
    const float af = (float)*alpha;
    const size_t base = (size_t)(x0 + (int)blockIdx.x) * pitch;
    double s = 0.0;
    for (int z = z0 + (int)threadIdx.x; z < z1; z += 64) {
        const size_t k = base + z;
        m[k] = m[k] + af * p[k];
        const float gv = g[k] - af * h[k];
        g[k] = gv;
        s = s + (double)gv * (double)gv;
    }
    s = lsm_wave_sum(s);
    if (threadIdx.x == 0) rows[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void fdw_lsm_direction_kernel(float* p, const float* g, const double* beta, int pitch, int x0, int z0, int z1)
{
    const int z = z0 + blockIdx.x * 256 + threadIdx.x;
    if (z >= z1) return;
    const size_t k = (size_t)(x0 + blockIdx.y) * pitch + z;
    p[k] = g[k] + (float)*beta * p[k];
}

__global__ __launch_bounds__(64) void fdw_lsm_scalar_kernel(double* sc, const double* n2, int nshots, double* hist, int k, int stage)
{
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int s = 0; s < nshots; s++) t = t + n2[s];
    if (stage == LSM_START) {
        hist[0] = 0.5 * t;
        sc[LSM_GAMMA] = sc[LSM_GG];
    } else if (stage == LSM_STEP) {
        sc[LSM_DELTA] = t;
        sc[LSM_ALPHA] = t == 0.0 ? 0.0 : sc[LSM_GAMMA] / t;
    } else if (stage == LSM_TURN) {
        const double gamma = sc[LSM_GAMMA], gg = sc[LSM_GG];
        sc[LSM_BETA] = gamma == 0.0 ? 0.0 : gg / gamma;
        hist[k + 1] = hist[k] - 0.5 * (sc[LSM_ALPHA] * gamma);
        sc[LSM_GAMMA] = gg;
    } else {
        hist[k] = 0.5 * t;
    }
}

hipError_t launch_lsm_dot_rows(const float* a, const float* b, double* rows, int ld, int r0, int nrows, int c0, int c1, hipStream_t s)
{
    if (nrows <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_lsm_dot_rows_kernel, dim3(nrows), dim3(64), 0, s, a, b, rows, ld, r0, c0, c1);
    return hipGetLastError();
}

hipError_t launch_lsm_finish(const double* rows, int n, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(fdw_lsm_finish_kernel, dim3(1), dim3(64), 0, s, rows, n > 0 ? n : 0, out);
    return hipGetLastError();
}

hipError_t launch_lsm_gather(const float* q, const float* dobs, const float* v2, float* w_out, float* ws, double* rows, int nt, int nx, int pitch, int nxb,
                             int gz, hipStream_t s)
{
    if (nt <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_lsm_gather_kernel, dim3(nt), dim3(64), 0, s, q, dobs, v2, w_out, ws, rows, nx, pitch, nxb, gz);
    return hipGetLastError();
}

hipError_t launch_lsm_stack(float* h, const float* img, const float* v2, const float* mask, int pitch, int x0, int x1, int z0, int z1, hipStream_t s)
{
    if (x1 <= x0 || z1 <= z0) return hipSuccess;
    hipLaunchKernelGGL(fdw_lsm_stack_kernel, dim3((z1 - z0 + 255) / 256, x1 - x0), dim3(256), 0, s, h, img, v2, mask, pitch, x0, z0, z1);
    return hipGetLastError();
}

hipError_t launch_lsm_update(float* m, float* g, const float* p, const float* h, const double* alpha, double* rows, int pitch, int x0, int x1, int z0, int z1,
                             hipStream_t s)
{
    if (x1 <= x0) return hipSuccess;
    hipLaunchKernelGGL(fdw_lsm_update_kernel, dim3(x1 - x0), dim3(64), 0, s, m, g, p, h, alpha, rows, pitch, x0, z0, z1);
    return hipGetLastError();
}

hipError_t launch_lsm_direction(float* p, const float* g, const double* beta, int pitch, int x0, int x1, int z0, int z1, hipStream_t s)
{
    if (x1 <= x0 || z1 <= z0) return hipSuccess;
    hipLaunchKernelGGL(fdw_lsm_direction_kernel, dim3((z1 - z0 + 255) / 256, x1 - x0), dim3(256), 0, s, p, g, beta, pitch, x0, z0, z1);
    return hipGetLastError();
}

hipError_t launch_lsm_scalars(double* sc, const double* n2, int nshots, double* hist, int k, int stage, hipStream_t s)
{
    hipLaunchKernelGGL(fdw_lsm_scalar_kernel, dim3(1), dim3(64), 0, s, sc, n2, nshots, hist, k, stage);
    return hipGetLastError();
}

}  // namespace fdw

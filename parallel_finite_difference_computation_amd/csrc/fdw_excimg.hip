// fdw_excimg.hip -- the image of excitation-amplitude imaging formed on the device (include/fdwave.h: fdw_dev_image_excitation,
// fdw_shot_excitation_batch), and the time-reversed transposition of the data gathers that the pick loop reads as its line source.
//
// Three small kernels, none on a time-stepping path.  They restate fdw_image_excitation (fdw_api.cpp) cell by cell:
//     m = max |amp| over the interior, from 0.0f with >        fdw_exc_peak_kernel
//     s = eps * m;  where |amp| > s: img = img + exc / amp      fdw_exc_stack_kernel, shots in order
// Built with -ffp-contract=off like every kernel of the library: eps * m and the add are rounded separately.
#include <hip/hip_runtime.h>

#include "fdw_excimg.h"

namespace fdw {

constexpr unsigned kAbsMask = 0x7fffffffu, kInfWord = 0x7f800000u;

// The peak as an unsigned maximum: for non-negative floats the bit pattern is monotonic, so max over the words |amp| <= +inf is the word of
// max |amp|; words above +inf are NaNs and never count (the host's `a > m` is false for them).  One block walks the rows blockIdx.y,
// blockIdx.y + gridDim.y, ... of shot blockIdx.z; each wave folds its lanes and issues one atomic maximum.  The maximum does not depend on
// the order, so the result is deterministic.
__global__ __launch_bounds__(256) void fdw_exc_peak_kernel(const float* __restrict__ amp, unsigned* __restrict__ peak, ExcImgGeom g)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    const unsigned* a = reinterpret_cast<const unsigned*>(amp) + (long long)blockIdx.z * g.bstride;
    unsigned m = 0u;
    if (col < g.nz)
        for (int row = blockIdx.y; row < g.nx; row += gridDim.y) {
            const unsigned w = a[(size_t)(g.x0 + row) * g.pitch + g.z0 + col] & kAbsMask;
            if (w <= kInfWord && w > m) m = w;
        }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, d, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m > 0u) atomicMax(peak + blockIdx.z, m);
}

// The update, one thread per interior cell, shots b = 0 .. nshots-1 in shot order.  The quotient is formed in double and rounded once:
// for fp32 operands that is the correctly rounded fp32 quotient (fp64 carries 53 >= 2 * 24 + 2 significand bits, so the second rounding
// cannot move the result), subnormal quotients included.  The double stays opaque to the optimiser, which would otherwise narrow
// fptrunc(fdiv(fpext, fpext)) back to an fp32 division.  img is stored only where a shot was selected, so every other word of it keeps its
// bits; stack (may be NULL) takes the running image after every shot, and may be exc itself: the thread has read exc_b at its cell before
// it writes there.
__global__ __launch_bounds__(256) void fdw_exc_stack_kernel(const float* exc, const float* __restrict__ amp, const unsigned* __restrict__ peak,
                                                            float eps, float* __restrict__ img, float* stack, ExcImgGeom g, int nshots)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= g.nz) return;
    for (int row = blockIdx.y; row < g.nx; row += gridDim.y) {
        const size_t k = (size_t)(g.x0 + row) * g.pitch + g.z0 + col;
        float v = img[k];
        bool changed = false;
        for (int b = 0; b < nshots; b++) {
            const size_t kb = k + (size_t)((long long)b * g.bstride);
            const float s = eps * __uint_as_float(peak[b]);
            const float a = amp[kb];
            if (__builtin_fabsf(a) > s) {
                double q = (double)exc[kb] / (double)a;
                asm volatile("" : "+v"(q));
                v = v + (float)q;
                changed = true;
            }
            if (stack) stack[kb] = v;
        }
        if (changed) img[k] = v;
    }
}

// fdw_gather_transpose_kernel (fdw_border.hip) with the time axis reversed on the way: in [shot][rows][cols] -> out [shot][cols][rows],
// out row k = in column cols-1-k.  32 x 32 tiles through LDS.
__global__ __launch_bounds__(256) void fdw_gather_transpose_rev_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols)
{
    __shared__ float tile[32][33];
    const size_t shot = (size_t)blockIdx.z * rows * cols;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8)
        if (r0 + j < rows && c0 + tx < cols) tile[j][tx] = in[shot + (size_t)(r0 + j) * cols + c0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
        if (c0 + j < cols && r0 + tx < rows) out[shot + (size_t)(cols - 1 - (c0 + j)) * rows + r0 + tx] = tile[tx][j];
}

static dim3 interior_grid(const ExcImgGeom& g, int rows_max, int z)
{
    return dim3((g.nz + 255) / 256, g.nx < rows_max ? g.nx : rows_max, z);
}

hipError_t launch_exc_peak(const float* d_amp, unsigned* d_peak, const ExcImgGeom& g, int nshots, hipStream_t s)
{
    if (g.nx <= 0 || g.nz <= 0 || nshots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_exc_peak_kernel, interior_grid(g, 256, nshots), dim3(256), 0, s, d_amp, d_peak, g);
    return hipGetLastError();
}

hipError_t launch_exc_stack(const float* d_exc, const float* d_amp, const unsigned* d_peak, float eps, float* d_img, float* d_stack,
                            const ExcImgGeom& g, int nshots, hipStream_t s)
{
    if (g.nx <= 0 || g.nz <= 0 || nshots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_exc_stack_kernel, interior_grid(g, 32768, 1), dim3(256), 0, s, d_exc, d_amp, d_peak, eps, d_img, d_stack, g, nshots);
    return hipGetLastError();
}

hipError_t launch_gather_transpose_rev(const float* d_in, float* d_out, int nx, int nt, int nshots, hipStream_t s)
{
    if (nx <= 0 || nt <= 0 || nshots <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_gather_transpose_rev_kernel, dim3((nt + 31) / 32, (nx + 31) / 32, nshots), dim3(256), 0, s, d_in, d_out, nx, nt);
    return hipGetLastError();
}

}  // namespace fdw

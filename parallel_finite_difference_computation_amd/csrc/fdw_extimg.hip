// fdw_extimg.hip -- one term of the subsurface-offset extended image (include/fdwave.h, "Extended imaging": fdw_dev_ext_image, fdw_shot_ext):
//     for h = -H .. H:   E[h+H][x][z] = E[h+H][x][z] (+) f[x-h][z] (*) r[x+h][z]      on the cells of C whose rows x-h, x+h lie in C
// A streaming kernel: two reads, then 2H+1 read-modify-writes per point, (2 + 2(2H+1)) * 4 B.  Built with -ffp-contract=off like every
// kernel of the library: the product and the sum are rounded separately.
//
// fdw_ext_image_kernel<H, V, 0>   the march.  Lanes run along z, V words each (4 where the three arrays are 16-byte aligned, else 1); a wave
//     marches one chunk of rows along x and keeps the rows x-H .. x+H of f and of r in two register rings of 2H+1 slots.  The march is unrolled
//     over one turn of the ring, so every slot index is static.  Every f and r word is loaded once per chunk (plus 2H run-in rows), every plane
//     row is loaded and stored once.  The planes of a row are all loaded before the first is stored, so their latencies overlap.  Whether a
//     row is loaded and whether a plane gets its term are the same in every lane (ext_chunk, ext_reach: fdw_extimg.h); columns outside
//     [z0, z1) in a lane's group of four are loaded (they lie inside the row) and never stored.  No LDS, no scratch, no atomics.
// fdw_ext_image_point_kernel   the ablation: one thread per cell of C, its 2(2H+1) operands through the caches.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fdw_extimg.h"
#include "fdw_internal.h"

namespace fdw {

typedef float ext_f4 __attribute__((ext_vector_type(4)));
template <int V> struct ExtVec;
template <> struct ExtVec<1> { using type = float; };
template <> struct ExtVec<4> { using type = ext_f4; };

struct ExtImgArgs {
    int pitch, x0, x1, z0, z1, xchunk;
    size_t plane;
};

template <int V>
__device__ __forceinline__ void ext_store(float* p, typename ExtVec<V>::type v, unsigned mask)
{
    if constexpr (V == 1) {
        *p = v;
    } else {
        if (mask == 0xfu) {
            *reinterpret_cast<ext_f4*>(p) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (mask >> k & 1u) p[k] = v[k];
        }
    }
}

// NUM: the numerics, last as in every kernel template of the library; the term has one arithmetic, so 0 (EXACT) is the only instantiation
template <int H, int V, int NUM>
__global__ __launch_bounds__(256) void fdw_ext_image_kernel(const float* __restrict__ f, const float* __restrict__ r, float* __restrict__ e, ExtImgArgs a)
{
    using Vec = typename ExtVec<V>::type;
    constexpr int R = 2 * H + 1;
    const int t = blockIdx.y * 256 + threadIdx.x;
    const int zc = V == 1 ? a.z0 + t : (a.z0 & ~3) + 4 * t;      // the lane's first column
    if (zc >= a.z1) return;
    unsigned mask = 0xfu;
    if constexpr (V == 4) {
        mask = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (zc + k >= a.z0 && zc + k < a.z1) mask |= 1u << k;
    }
    const ExtChunk c = ext_chunk(a.x0, a.x1, H, a.xchunk, blockIdx.x);
    auto row_of = [&](const float* p, int row) { return *reinterpret_cast<const Vec*>(p + (size_t)row * a.pitch + zc); };

    // ring slot of row c0 - H + i: i mod R
    Vec fr[R], rr[R];
#pragma unroll
    for (int i = 0; i < R; i++) {
        fr[i] = Vec(0.0f);
        rr[i] = Vec(0.0f);
    }
#pragma unroll
    for (int i = 0; i < 2 * H; i++) {
        const int row = c.c0 - H + i;
        if (row >= c.rd0 && row < c.rd1) {
            fr[i] = row_of(f, row);
            rr[i] = row_of(r, row);
        }
    }
    for (int xb = c.c0; xb < c.c1; xb += R) {
#pragma unroll
        for (int j = 0; j < R; j++) {
            const int x = xb + j;
            if (x < c.c1) {
                if (x + H < c.rd1) {
                    fr[(j + 2 * H) % R] = row_of(f, x + H);
                    rr[(j + 2 * H) % R] = row_of(r, x + H);
                }
                const int reach = ext_reach(a.x0, a.x1, x);
                float* const erow = e + (size_t)x * a.pitch;
                Vec acc[R];
#pragma unroll
                for (int q = 0; q < R; q++) {
                    const int ah = q < H ? H - q : q - H;
                    if (ah <= reach) acc[q] = *reinterpret_cast<const Vec*>(erow + (size_t)q * a.plane + zc);
                }
#pragma unroll
                for (int q = 0; q < R; q++) {
                    const int ah = q < H ? H - q : q - H;      // plane q: h = q - H, f row x - h (slot j + 2H - q), r row x + h (slot j + q)
                    if (ah <= reach) {
                        const Vec prod = fr[(j + 2 * H - q) % R] * rr[(j + q) % R];
                        acc[q] = acc[q] + prod;
                    }
                }
#pragma unroll
                for (int q = 0; q < R; q++) {
                    const int ah = q < H ? H - q : q - H;
                    if (ah <= reach) ext_store<V>(erow + (size_t)q * a.plane + zc, acc[q], mask);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void fdw_ext_image_point_kernel(const float* __restrict__ f, const float* __restrict__ r, float* __restrict__ e, ExtImgArgs a,
                                                                  int H)
{
    const int z = a.z0 + blockIdx.y * 256 + threadIdx.x;
    const int x = a.x0 + blockIdx.x;
    if (z >= a.z1) return;
    int reach = ext_reach(a.x0, a.x1, x);
    reach = reach < H ? reach : H;
    for (int h = -reach; h <= reach; h++) {
        float* const p = e + (size_t)(h + H) * a.plane + (size_t)x * a.pitch + z;
        const float prod = f[(size_t)(x - h) * a.pitch + z] * r[(size_t)(x + h) * a.pitch + z];
        *p = *p + prod;
    }
}

template <int H>
static void launch_march(const float* f, const float* r, float* e, const ExtImgArgs& a, int nchunks, bool wide, hipStream_t s)
{
    if (wide) {
        const int lanes = (a.z1 - (a.z0 & ~3) + 3) / 4;
        hipLaunchKernelGGL((fdw_ext_image_kernel<H, 4, 0>), dim3(nchunks, (lanes + 255) / 256), dim3(256), 0, s, f, r, e, a);
    } else {
        hipLaunchKernelGGL((fdw_ext_image_kernel<H, 1, 0>), dim3(nchunks, (a.z1 - a.z0 + 255) / 256), dim3(256), 0, s, f, r, e, a);
    }
}

hipError_t launch_ext_image(const float* d_f, const float* d_r, float* d_e, int H, int pitch, size_t plane, int x0, int x1, int z0, int z1, int xchunk,
                            bool pointwise, hipStream_t s)
{
    if (x1 <= x0 || z1 <= z0) return hipSuccess;
    if (H < 0 || H > FDW_EXT_HMAX) return hipErrorInvalidValue;
    ExtImgArgs a{pitch, x0, x1, z0, z1, 0, plane};
    if (pointwise) {
        hipLaunchKernelGGL(fdw_ext_image_point_kernel, dim3(x1 - x0, (z1 - z0 + 255) / 256), dim3(256), 0, s, d_f, d_r, d_e, a, H);
        return hipGetLastError();
    }
    const int nchunks = fdw_plan_ext_image(x0, x1, z1 - z0, H, xchunk, &a.xchunk, nullptr, 0);
    if (nchunks <= 0) return hipErrorInvalidValue;
    // four words per lane where every row of the three arrays and every plane starts on a 16-byte boundary
    const bool wide = ((reinterpret_cast<uintptr_t>(d_f) | reinterpret_cast<uintptr_t>(d_r) | reinterpret_cast<uintptr_t>(d_e)) & 15u) == 0 && pitch % 4 == 0 &&
                      plane % 4 == 0;
    switch (H) {
    case 0: launch_march<0>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    case 1: launch_march<1>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    case 2: launch_march<2>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    case 3: launch_march<3>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    case 4: launch_march<4>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    case 5: launch_march<5>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    case 6: launch_march<6>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    case 7: launch_march<7>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    default: launch_march<8>(d_f, d_r, d_e, a, nchunks, wide, s); break;
    }
    return hipGetLastError();
}

}  // namespace fdw

// The row plan of one term (fdwave.h, "Extended imaging"); pure host code, no context, no device.
extern "C" int fdw_plan_ext_image(int x0, int x1, int nz, int H, int xchunk, int* xchunk_out, fdw_ext_chunk* chunks, int cap)
{
    if (x0 < 0 || x1 < x0 || nz < 0 || H < 0 || H > FDW_EXT_HMAX || xchunk < 0 || (chunks && cap < 0))
        return fdw_fail(FDW_EINVAL, "extended image plan: rows [%d,%d) nz=%d H=%d (0..%d) xchunk=%d", x0, x1, nz, H, FDW_EXT_HMAX, xchunk);
    const int rows = x1 - x0;
    if (xchunk == 0) {
        // about 8192 waves of 256 columns where the grid has them; a chunk re-reads 2H run-in rows of f and r, so never shorter than H rows
        const long strip_rows = (long)rows * ((nz + 255) / 256);
        const long lo = H > 2 ? H : 2;
        xchunk = (int)(strip_rows / 8192 < lo ? lo : (strip_rows / 8192 > 64 ? 64 : strip_rows / 8192));
    }
    if (xchunk_out) *xchunk_out = xchunk;
    const int n = (rows + xchunk - 1) / xchunk;
    if (!chunks) return n;
    if (cap < n) return fdw_fail(FDW_EINVAL, "extended image plan: %d chunks, room for %d", n, cap);
    for (int i = 0; i < n; i++) {
        const fdw::ExtChunk k = fdw::ext_chunk(x0, x1, H, xchunk, i);
        fdw_ext_chunk* o = chunks + i;
        o->c0 = k.c0; o->c1 = k.c1; o->rd0 = k.rd0; o->rd1 = k.rd1;
        for (int j = 0; j < 2 * FDW_EXT_HMAX + 1; j++) {
            o->w0[j] = o->w1[j] = 0;
            if (j > 2 * H) continue;
            // plane j, h = j - H: the rows of the chunk at which ext_reach admits |h|
            const int ah = j < H ? H - j : j - H;
            int first = k.c1, last = k.c0;
            for (int x = k.c0; x < k.c1; x++)
                if (ah <= fdw::ext_reach(x0, x1, x)) {
                    if (x < first) first = x;
                    last = x + 1;
                }
            if (first < last) { o->w0[j] = first; o->w1[j] = last; }
        }
    }
    return n;
}

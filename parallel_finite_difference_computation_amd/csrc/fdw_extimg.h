// fdw_extimg.h -- subsurface-offset image gathers (fdwave.h, "Extended imaging"): the row plan of one term, stated once for the host
// (fdw_plan_ext_image) and the kernels (fdw_extimg.hip), and the launcher.  A header of its own, as fdw_born.h and fdw_dtt.h are:
// fdw_kernels.h and fdw_device.h stay what the traffic profiles were taken on.
#pragma once
#include <hip/hip_runtime.h>

#include "fdwave.h"

namespace fdw {

// Chunk i of the rows [x0, x1) of C, xchunk rows each (the last one shorter): the rows [c0, c1) whose cells it accumulates into, and the rows
// [rd0, rd1) of f and r it loads -- its own and H run-in rows on either side, cut to [x0, x1).  The one place a shifted row index is formed.
struct ExtChunk {
    int c0, c1, rd0, rd1;
};
__host__ __device__ inline ExtChunk ext_chunk(int x0, int x1, int H, int xchunk, int i)
{
    ExtChunk k;
    k.c0 = x0 + i * xchunk;
    k.c1 = k.c0 + xchunk < x1 ? k.c0 + xchunk : x1;
    k.rd0 = k.c0 - H > x0 ? k.c0 - H : x0;
    k.rd1 = k.c1 + H < x1 ? k.c1 + H : x1;
    return k;
}
// The largest |h| whose plane has a term at row x of [x0, x1): both x - |h| and x + |h| lie in [x0, x1)
__host__ __device__ inline int ext_reach(int x0, int x1, int x)
{
    const int lo = x - x0, hi = x1 - 1 - x;
    return lo < hi ? lo : hi;
}

// One term on C = rows [x0, x1) x columns [z0, z1): for h = -H .. H, plane j = h + H (`plane` words apart from d_e on),
//     e_j[x][z] = e_j[x][z] (+) f[x-h][z] (*) r[x+h][z]      wherever x - h and x + h lie in [x0, x1)
// through the chunks of fdw_plan_ext_image(x0, x1, z1 - z0, H, xchunk) (xchunk 0: automatic).  pointwise: one thread per cell reading its
// operands through the caches (the ablation: fdw_ext_image_point_kernel) instead of the march.
hipError_t launch_ext_image(const float* d_f, const float* d_r, float* d_e, int H, int pitch, size_t plane, int x0, int x1, int z0, int z1, int xchunk,
                            bool pointwise, hipStream_t s);

}  // namespace fdw

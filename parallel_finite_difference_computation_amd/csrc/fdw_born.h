// fdw_born.h -- Born modelling (fdwave.h, "Born modelling"): the launcher mode and the launchers of its kernels.  A header of its own, as
// fdw_excimg.h is: fdw_kernels.h and fdw_device.h stay what the traffic profiles were taken on.
#pragma once
#include "fdw_kernels.h"

namespace fdw {

// One more mode of the one-step ring family's table (launch_step_fast; fdw_step_born_kernel): FWD on (p, pp) + the same step without a source on
// the scattered pair + the scatter du_new += m (*) q on the interior cells + the trace rows of both new fields (fdw_dev_born_steps).  One shot, or a batch (below).
// What the launch reads from StepArgs on top of a FWD launch, in fields the forward modes leave unused, so that the struct -- and with it the
// kernel arguments of every other launch -- stays as it is:
//   psrc / fpp   the scattered pair: du_p (read only), du_pp (overwritten with the new scattered field)
//   img          the reflectivity m [nxl][pitch] (only read)
//   rec / texc   this step's trace row of the scattered field / of the background (texc as float words); either may be NULL
//   rec_z, rec_x0, rec_n   always set: the receiver column; the scatter covers rows [rec_x0, rec_x0 + rec_n) of the launch
//   img_z1       one past the last interior column of the scatter
//   exc_key      born_key(kind, z0): the kind (0 q = the new field, 1 q = its second time difference) and the first interior column
constexpr int FDW_MODE_BORN = 19;
// ... and the same launch driven by a line source (fdw_step_line_born_kernel, fdw_dev_born_line_steps): inj / inj_x / inj_n / inj_z as a
// FWD_LINE launch sets them.
// A batch of shots (gridDim.y = nbatch; fdw_born_shot_batch, fdw_born_shot_line_batch), both modes: the four fields of shot b lie b * bstride
// further on, its model b * v2_bstride, its scattered trace row rec + b * rec_bstride and its background trace row texc + b * rec_bstride
// (float words); the reflectivity img is ONE field, read unshifted by every shot.  With one shot every offset is zero.
constexpr int FDW_MODE_BORN_LINE = 20;
__host__ __device__ __forceinline__ int born_key(int kind, int z0) { return (z0 << 1) | (kind & 1); }
__host__ __device__ __forceinline__ int born_key_kind(int key) { return key & 1; }
__host__ __device__ __forceinline__ int born_key_z0(int key) { return key >> 1; }

// Born modelling behind step kernels that do not scatter themselves (orders above 8, forced generic, FDW_NO_BORN_FUSED): w = a (-) b on the
// interior cells C = rows [x0, x1) x columns [z0, z1) (fdw_born_diff_kernel), and d = d (+) m (*) q on C with q = u (kind 0) or
// (u (-) a) (-) w (kind 1), then the trace samples rec[r - x0] = d(r, gz), rec0[r - x0] = u(r, gz) of rows [x0, x1) (fdw_born_scatter_kernel)
hipError_t launch_born_diff(const float* a, const float* b, float* w, int pitch, int x0, int x1, int z0, int z1, hipStream_t s);
hipError_t launch_born_scatter(const float* u, const float* a, const float* w, const float* m, float* d, int kind, int pitch, int x0, int x1, int z0,
                               int z1, int zcols, int gz, float* rec, float* rec0, hipStream_t s);

}  // namespace fdw

// fdw_dtt.h -- second-time-difference imaging (fdwave.h, "DTT imaging"): the launcher mode and the launcher of its kernels.  A header of its own,
// as fdw_born.h is: fdw_kernels.h and fdw_device.h stay what the traffic profiles were taken on.
#pragma once
#include "fdw_born.h"

namespace fdw {

// One more mode of the one-step ring family's table (launch_step_fast; fdw_step_back_dtt_kernel): FDW_MODE_BACK with the DTT value of its
// imaging epilogue.  What the launch reads from StepArgs on top of a BACK launch, in fields BACK leaves unused:
//   rec_x0, rec_n   the rows of the cell set C: [rec_x0, rec_x0 + rec_n)
//   exc_key         born_key(0, z0): the first column of C
//   img_z1          one past the last column of C
// A batch of shots: as BACK (fields, models, gathers and images strided per shot).
constexpr int FDW_MODE_BACK_DTT = 21;

// One term on C = rows [x0, x1) x columns [z0, z1) (fdw_dtt_image_kernel): img = img (+) ((a (-) b) (-) (b (-) c)) (*) r; pre != 0: a already
// holds a (-) b (launch_born_diff took it before a step overwrote an operand).  nbatch > 1: that many shots, bstride words apart in every array.
hipError_t launch_dtt_image(const float* a, const float* b, const float* c, const float* r, float* img, int pre, int pitch, int x0, int x1, int z0, int z1,
                            int nbatch, long long bstride, hipStream_t s);

}  // namespace fdw

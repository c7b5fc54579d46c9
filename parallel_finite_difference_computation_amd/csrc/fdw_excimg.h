// fdw_excimg.h -- launchers of the excitation-amplitude image kernels (fdw_excimg.hip): the peak of |amp| over the interior, the image
// update img += exc / amp in shot order, and the time-reversed gather transposition.  Definitions in include/fdwave.h
// (fdw_dev_image_excitation, fdw_shot_excitation_batch).
#pragma once
#include <hip/hip_runtime.h>

namespace fdw {

// The interior of a field-shaped array [nxl][pitch] (rows x0 .. x0+nx-1, columns z0 .. z0+nz-1) and the stride between the arrays of
// consecutive shots, in elements.
struct ExcImgGeom {
    int pitch, x0, nx, z0, nz;
    long long bstride;
};

// peak[b] = the bit pattern of max |amp_b| over the interior, from 0 (a NaN never counts); peak[0 .. nshots) must have been zeroed on `s`
hipError_t launch_exc_peak(const float* d_amp, unsigned* d_peak, const ExcImgGeom& g, int nshots, hipStream_t s);
// for b = 0 .. nshots-1 in order, per interior cell: where |amp_b| > eps * peak_b, img = img + exc_b / amp_b; d_stack (may be NULL, may be
// d_exc): the running image after shot b into the interior of array b
hipError_t launch_exc_stack(const float* d_exc, const float* d_amp, const unsigned* d_peak, float eps, float* d_img, float* d_stack,
                            const ExcImgGeom& g, int nshots, hipStream_t s);
// gathers [shot][nx][nt] -> [shot][nt][nx] with the time axis reversed: out[shot][k][ix] = in[shot][ix][nt-1-k]
hipError_t launch_gather_transpose_rev(const float* d_in, float* d_out, int nx, int nt, int nshots, hipStream_t s);

}  // namespace fdw

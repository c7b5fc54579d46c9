// fdw_lsm.h -- least-squares migration (fdwave.h, "Least-squares migration"): the launchers of the kernels that carry a conjugate-gradient
// solve between and around the Born loop and the DTT backward loop.  A header of its own, as fdw_born.h and fdw_dtt.h are.
#pragma once
#include <hip/hip_runtime.h>

namespace fdw {

// The sum order S of fdwave.h is what ONE wave does: lane l adds x_l, x_{l+64}, ... onto +0.0 in ascending order, then the 64 partials are
// folded with s_l = s_l + s_{l+d}, d = 32 .. 1.  Every reduction below is one wave per row and one wave over the row sums, so no number
// depends on a launch geometry; nothing is added atomically.

// rows[r] = S over z in [c0, c1) of (double)a[(r0 + r) * ld + z] * (double)b[...], r in [0, nrows) (fdw_lsm_dot_rows_kernel).  The cell set C of
// a field: ld = pitch, r0 = x0, [c0, c1) = [z0, z1); a gather [nt][nx]: ld = nx, r0 = 0, [c0, c1) = [0, nx).
hipError_t launch_lsm_dot_rows(const float* a, const float* b, double* rows, int ld, int r0, int nrows, int c0, int c1, hipStream_t s);
// *out = S(rows[0 .. n)) (fdw_lsm_finish_kernel); n = 0: +0.0
hipError_t launch_lsm_finish(const double* rows, int n, double* out, hipStream_t s);
// One pass over a gather [nt][nx] (fdw_lsm_gather_kernel): w = dobs ? dobs (-) q : q; rows[it] = S of (double)w * (double)w over the row;
// w_out (NULL ok) = w; ws = w (*) v2[(nxb + ix) * pitch + gz].  w_out may be q; ws may be dobs or q (the batched visit weights the scattered
// gathers in place): every word is read before it is written, by the one thread that writes it.
hipError_t launch_lsm_gather(const float* q, const float* dobs, const float* v2, float* w_out, float* ws, double* rows, int nt, int nx, int pitch, int nxb,
                             int gz, hipStream_t s);
// On C = rows [x0, x1) x columns [z0, z1) (fdw_lsm_stack_kernel): h = h (+) mask (*) (img (/) v2), mask == NULL: h = h (+) (img (/) v2).  The
// quotient is the correctly rounded fp32 one, formed as the fp64 quotient of the two floats rounded to fp32 (53 >= 2 * 24 + 2 bits: the
// second rounding cannot change the result).
hipError_t launch_lsm_stack(float* h, const float* img, const float* v2, const float* mask, int pitch, int x0, int x1, int z0, int z1, hipStream_t s);
// On C, af = (float)*alpha (fdw_lsm_update_kernel): m = m (+) af (*) p; g = g (-) af (*) h; rows[x - x0] = S of (double)g * (double)g of the new g.
hipError_t launch_lsm_update(float* m, float* g, const float* p, const float* h, const double* alpha, double* rows, int pitch, int x0, int x1, int z0, int z1,
                             hipStream_t s);
// On C, bf = (float)*beta (fdw_lsm_direction_kernel): p = g (+) bf (*) p.
hipError_t launch_lsm_direction(float* p, const float* g, const double* beta, int pitch, int x0, int x1, int z0, int z1, hipStream_t s);

// The scalars of a solve in device memory (fdw_lsm_scalar_kernel, one wave, lane 0 works): sc[LSM_GAMMA .. LSM_GG], the shots' n2[nshots],
// the misfit history hist[].  t = n2[0] + n2[1] + ... onto +0.0 in shot order.
//   LSM_START   hist[0] = 0.5 * t; gamma = gg
//   LSM_STEP    delta = t; alpha = delta == 0 ? 0 : gamma / delta
//   LSM_TURN    beta = gamma == 0 ? 0 : gg / gamma; hist[k + 1] = hist[k] - 0.5 * (alpha * gamma); gamma = gg
//   LSM_VERIFY  hist[k] = 0.5 * t
enum { LSM_GAMMA = 0, LSM_DELTA = 1, LSM_ALPHA = 2, LSM_BETA = 3, LSM_GG = 4, LSM_NSCALARS = 5 };
enum { LSM_START = 0, LSM_STEP = 1, LSM_TURN = 2, LSM_VERIFY = 3 };
hipError_t launch_lsm_scalars(double* sc, const double* n2, int nshots, double* hist, int k, int stage, hipStream_t s);

}  // namespace fdw

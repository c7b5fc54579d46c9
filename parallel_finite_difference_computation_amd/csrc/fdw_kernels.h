// fdw_kernels.h -- internal interface between the C-ABI layer (fdw_api.cpp) and the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>

namespace fdw {

enum {
    FDW_MODE_FWD = 0,    // taper + Laplacian + leap-frog + point source   (fd_forward body, R:264-267)
    FDW_MODE_PLAIN = 1,  // Laplacian + leap-frog only                     (fd_back source field, R:317-318)
    FDW_MODE_RECV = 2,   // taper + Laplacian + leap-frog + receivers + imaging (R:325-329)
    FDW_MODE_LAP = 3,    // Laplacian only, written to `pp`                (stencil_code, S:325)
    FDW_MODE_MOD = 4,    // forward-modelling step of the CPU-serial sibling (mod_main: fd_step + ptsrc + taper_apply + trace sample)
    FDW_MODE_DD_FWD = 5, // its stored-wavefield RTM, source pass (rtm_main.cpp:165-184: fd_step + one-cell source + taper_apply2)
    FDW_MODE_BACK = 7,   // one whole backward iteration of fd_back in a single pass: source-field step + receiver step + imaging (R:317-329)
    FDW_MODE_BACK4 = 9,  // wave-pipeline kernel only: four whole iterations of fd_back in one pass of an eight-wave workgroup (source + receiver fields)
    FDW_MODE_PLAIN_ALL = 8, // wave-pipeline kernel only: PLAIN with all four time levels stored (source field of the backward loop)
    FDW_MODE_FWD_REC = 10, // launchers only: FWD + the trace sample of every step on the receiver line (fdw_dev_record_steps; StepArgs / Step2Args rec*)
    FDW_MODE_FWD_ILLUM = 11, // launchers only: FWD + the source illumination, illum += new field (*) new field over the update extents (fdw_dev_illum_steps; the accumulator travels in `img`)
    FDW_MODE_FWD_REC_ILLUM = 12, // launchers only: FWD + the trace samples + the source illumination in one launch (fdw_dev_record_illum_steps, fdw_shot_residual)
    FDW_MODE_FWD_LINE = 13, // launchers only: FWD with a LINE source in place of the point source: inj_n samples on column inj_z of rows [inj_x, inj_x+inj_n)
                            // (fdw_dev_line_steps; multi-step kernels: level k takes inj + k * inj_stride)
    FDW_MODE_FWD_LINE_REC = 14,   // ... + the trace samples, written after the injection
    FDW_MODE_FWD_LINE_ILLUM = 15, // ... + the source illumination, accumulated after the injection
    FDW_MODE_FWD_LINE_REC_ILLUM = 16, // ... + both in one launch (fdw_dev_line_record_illum_steps, fdw_shot_line_residual with an accumulator)
    FDW_MODE_FWD_EXC = 17,       // launchers only: FWD + the excitation maps (fdw_dev_excite_steps): amp travels in `img`, the time map in `texc`, exc_key = it + 1
    FDW_MODE_FWD_LINE_PICK = 18, // launchers only: FWD_LINE + the excitation pick (fdw_dev_line_pick_steps): exc travels in `img`, exc_key = top - it
    FDW_MODE_DD_RECV = 6 // its receiver pass (rtm_main.cpp:197-220) + img += stored source field * CURRENT receiver field (rtm_main.cpp:224-230)
};

constexpr int kMaxFastHalfOrder = 4;   // register-window kernel is instantiated for order 2,4,6,8
constexpr int kMaxPipeSteps = 4;       // time levels of one pass of the wave-pipeline kernel

// Everything one launch needs, passed by value (lives in SGPRs / the scalar cache).
// All row indices are LOCAL rows of this device's slab; the host translates global extents.
struct StepArgs {
    const float* p;        // [nxl][pitch] newest field (read only in this launch)
    float* pp;             // [nxl][pitch] older field, overwritten with the new one (or Laplacian out)
    float* out;            // NULL, or where the new field goes INSTEAD of over pp (pp is then only read: stored-wavefield loops keep every field)
    const float* v2;       // [nxl][pitch] squared velocity
    const float* psrc;     // IMG: source wavefield to correlate with; BACK: F_{k-1}, the newer source field (read only)
    float* fpp;            // BACK: F_{k-2}, overwritten with the reconstructed F_k
    int img_z1;            // IMG: columns >= img_z1 lie outside kernel_img's launch extent (R:133-144) and keep their image value
    float* img;            // IMG: image accumulator on the extended grid; FWD_ILLUM: the illumination accumulator
    const float* taperz;   // [ztap] z damping factors
    const float* txfac;    // [nxl] per-row x damping factor (1.0f where none applies)
    const float* inj;      // INJ=1: one source sample; INJ=2: inj_n receiver samples of this step
    const float* gcx;      // generic kernel: device copies of the scaled coefficients
    const float* gcz;
    int pitch, nxl;
    int r0, r1;            // rows updated by this launch (already clipped to rows < upd_x1)
    int lap_x0, lap_x1;    // rows / columns where the Laplacian is evaluated (0 elsewhere)
    int lap_z0, lap_z1;
    int upd_z1;            // columns >= upd_z1 keep their old value (reference launch extent)
    int ztap, tz_x1;       // damped strip: z < ztap; rows < tz_x1 get the z factor
    int xt_lo, xt_hi;      // rows in [xt_lo, xt_hi) have txfac == 1 and get the z factor (the common case)
    int pp_twice;          // pp owes the previous step's T() (all steps but the first after an upload)
    int inj_x, inj_z, inj_n;
    int xchunk, wz, nzblk, nblk, nper;  // launch geometry (fast kernel)
    float dt2;
    float cx[2 * kMaxFastHalfOrder + 1], cz[2 * kMaxFastHalfOrder + 1];
    float c0;              // FAST numerics: cz[H] + cx[H], the weight of the centre point (formed on the host in fp32)
    int numerics;          // 0 EXACT (the reference's operations), 1 FAST (symmetric sums + fma; fdw_device.h): picks the instantiation
    // FDW_MODE_MOD only: cz holds the UNSCALED weights, the spacings come separately (fd.c:24-36 scales per term)
    float dx2inv, dz2inv;
    float gw[4][4];        // expf(-(i*i + j*j)): the 7x7 Gaussian point source of ptsrc.c:49-55
    float* rec;            // this step's trace samples [rec_n]: rec[r - rec_x0] = p(r, rec_z)   (mod_main.cpp:155-157); FWD_REC: the NEW field
    int rec_z, rec_x0, rec_n;
    // batch of independent shots on one geometry (gridDim.y = shots; 0 / 1 = a single shot): shot b works on field pointers + b * bstride,
    // samples inj + b * inj_bstride, source row inj_x + b * inj_dx
    // (v2 + b * v2_bstride: one model per shot in the RTM loop, one for all in the modelling loop; rec + b * rec_bstride)
    long long bstride, inj_bstride, v2_bstride, rec_bstride;
    int inj_dx, nbatch;
    // FDW_MODE_FWD_EXC / FWD_LINE_PICK (one shot, no batch stride): the excitation-time map [nxl][pitch] and the level this launch writes / picks
    int* texc;
    int exc_key;
};

// Two-steps-per-pass kernel (temporal blocking, order 8, forward mode): see fdw_step2_kernel.
struct Step2Args {
    const float* p;        // u^n
    const float* pp;       // u^{n-1}
    const float* v2;
    float* out1;           // u^{n+1}
    float* out2;           // u^{n+2}
    const float* taperz;
    const float* txfac;
    const float* inj;      // FWD: two source samples srce[it], srce[it+1]; RECV: receiver samples of iteration it (step 1)
    const float* inj2;     // RECV: receiver samples of iteration it+1 (step 2)
    const float* psrc_a;   // RECV: source wavefield of iteration it   (imaged against u^{n+1})
    const float* psrc_b;   // RECV: source wavefield of iteration it+1 (imaged against u^{n+2})
    float* img;            // RECV: image accumulator on the extended grid (in place, owned cells only); FWD_ILLUM: the illumination accumulator
    int img_z1;            // RECV: columns >= img_z1 lie outside kernel_img's launch extent and keep their image value
    int pitch, nxl;
    int r0, r1;            // rows whose u^{n+1}, u^{n+2} this launch produces
    int r0b, r1b, chunks_a; // pipeline kernel only: optional second row range (chunks >= chunks_a walk [r0b, r1b))
    int lap_x0, lap_x1, lap_z0, lap_z1;
    int upd_x1, upd_z1;
    int ztap, tz_x1, xt_lo, xt_hi;
    int zt_lo, zt_hi;      // pipeline kernel: columns [zt_lo, zt_hi) carry no damping factor (zt_hi < 0: no x factor outside the damped strip either)
    int pp_twice;
    int inj_x, inj_z, inj_n;
    int xchunk, nstrip, nzblk, nblk, nper;
    float dt2;
    float cx[2 * kMaxFastHalfOrder + 1], cz[2 * kMaxFastHalfOrder + 1];
    float c0;              // FAST numerics: cz[H] + cx[H]
    int numerics;          // 0 EXACT, 1 FAST (see StepArgs)
    // pipeline kernel in FDW_MODE_MOD only (see StepArgs): unscaled weights in cz, spacings, Gaussian source weights, trace samples
    float dx2inv, dz2inv;
    float gw[4][4];
    float* rec;            // [steps of the pass][rec_n]: wave k writes row k (MOD: its p field; FWD_REC, also the two-step kernel: its new row)
    int rec_z, rec_x0, rec_n;
    // pipeline kernel, backward loop (fd_back, R:302-339), two passes per kPipeSteps iterations:
    //   FDW_MODE_PLAIN_ALL  the source field: like PLAIN, but EVERY wave stores its time level (wave 0 -> lvl0, wave 1 -> lvl1, then out1, out2),
    //                       because the imaging condition of iteration it+k needs F_{it+k} at every point
    //   FDW_MODE_RECV       the receiver field: wave k adds the trace samples of iteration it+k (inj + k * inj_stride) on column inj_z of rows
    //                       [inj_x, inj_x+inj_n) and multiplies its new row with the same row of plev[k] = F_{it+k}; the four products are
    //                       added to the image row in iteration order as it travels from wave to wave through an LDS FIFO
    float *lvl0, *lvl1;
    const float* plev[kMaxPipeSteps];
    int inj_stride;
    //   FDW_MODE_BACK4      both in one pass (fdw_back4_kernel): p / pp / out1 / out2 are the source field's, these the receiver field's
    const float *rp, *rpp;
    float *rout1, *rout2;
    // pipeline kernel, FDW_MODE_FWD_EXC / FWD_LINE_PICK: the excitation-time map and the key of the pass's FIRST step (it + 1 / top - it); amp / exc in img
    int* texc;
    int exc_key;
};
hipError_t launch_step2(const Step2Args& a, int half_order, int mode, hipStream_t s);

// kPipeSteps time steps per pass (wave pipeline through LDS, order 8, FWD / PLAIN): see fdw_stepn_kernel.  Uses Step2Args with
// out1 = u^{n+kPipeSteps-1}, out2 = u^{n+kPipeSteps}, inj -> kPipeSteps source samples, nstrip = strips of 64-2*kPipeSteps cells,
// nblk = nstrip * chunks workgroups of kPipeSteps waves.
// (a pipeline of two waves was measured and dropped: DESIGN.md section 3c)
constexpr int kPipeSteps = 4;
hipError_t launch_stepn(const Step2Args& a, int half_order, int mode, hipStream_t s);

// May a tile (strip of cells from cs, rows [xa, xe)) of a pipeline pass run the lean body?  Every row it touches -- stencil taps, look-ahead
// loads (PF + ring rows beyond the chunk) -- lies inside the rows where the Laplacian and the update are unmasked, its columns likewise, it is
// outside the damped strip, and neither a source nor (modelling, REC) the receiver line is in it.  By the template values of the instantiation
// that runs the tile; stated once for the kernels (workgroup-uniform, fdw_stepn.hip) and the host (fdw_debug_step4_plan: tile counts).
template <int H, int NS, bool TAPER, int INJ, bool DD = false, bool REC = false>
__host__ __device__ __forceinline__ bool pipe_tile_lean(const Step2Args& a, int cs, int xa, int xe)
{
    const int lo = xa - (NS - 1) * H - H - NS * (H + 1), hi = xe + (NS - 1) * (2 * H + 1) + 2 * H + 16;
    const int c0 = cs * 4, c1 = cs * 4 + 256;
    bool ok = (c0 >= a.lap_z0) && (c1 <= min(a.lap_z1, a.upd_z1)) && (lo >= max(a.lap_x0, 0)) && (hi <= min(min(a.lap_x1, a.upd_x1), a.nxl));
    if (TAPER) {
        ok = ok && (c0 >= a.zt_lo);
        if (a.zt_hi >= 0) ok = ok && (c1 <= a.zt_hi) && (lo >= a.xt_lo) && (hi <= a.xt_hi);      // four-sided damping (taper_apply)
    }
    if (INJ == 3) ok = ok && !((a.inj_z + 3 >= c0) && (a.inj_z - 3 < c1) && (a.inj_x + 3 >= xa - NS * H) && (a.inj_x - 3 < xe + NS * H));
    if (INJ == 2) ok = ok && !((a.inj_z >= c0) && (a.inj_z < c1) && (a.inj_x < xe + NS * H) && (a.inj_x + a.inj_n > xa - NS * H));
    if (INJ == 1) ok = ok && !((a.inj_z >= c0) && (a.inj_z < c1) && (a.inj_x >= xa - NS * H) && (a.inj_x < xe + NS * H));
    if (DD) ok = ok && !((a.rec != nullptr) && (a.rec_z >= c0) && (a.rec_z < c1));                  // trace recording
    if (REC) ok = ok && !((a.rec_z >= c0 + 4 * NS) && (a.rec_z < c1 - 4 * NS));                      // ... the strip whose owned lanes record it
    return ok;
}

// Which tile of a pipeline pass is logical block L (L = chunk row * nstrip + strip)?  Declares the strip `zb` and the rows [`xa`, `xe`) of the
// chunk (and `xb`, `second`): chunks from chunks_a on walk the second row range of the launch (the two boundary strips of a slab).  A macro
// because the kernels expand it (FDW_PIPE_TILE, fdw_stepn.hip, where the reason is written down) and the host must agree with them tile for
// tile (tile_classes, fdw_api.cpp).  FDW_PIPE_TILE_CELL: the first cell of strip zb's wave, NS halo lanes before the 64 - 2 NS cells it owns.
#define FDW_PIPE_TILE_ROWS(a, L, zb, xa, xe)                                             \
    const int zb = (L) % a.nstrip;                                                       \
    const int xb = (L) / a.nstrip;                                                       \
    const bool second = xb >= a.chunks_a;                                                \
    const int xa = second ? a.r0b + (xb - a.chunks_a) * a.xchunk : a.r0 + xb * a.xchunk; \
    const int xe = min(xa + a.xchunk, second ? a.r1b : a.r1);
#define FDW_PIPE_TILE_CELL(zb, NS) ((zb) * (64 - 2 * (NS)) - (NS))

hipError_t launch_step_fast(const StepArgs& a, int half_order, int mode, int prefetch, hipStream_t s);
hipError_t launch_step_generic(const StepArgs& a, int half_order, int mode, hipStream_t s);
hipError_t launch_taper_finalize(float* f, const float* taperz, const float* txfac, int pitch, int nxl, int ztap,
                                 int tz_x1, hipStream_t s);
// source illumination of the orders without a register-ring kernel: illum += f (*) f on rows [r0, r1), columns < z1 (fdw_illum_add_kernel)
hipError_t launch_illum_add(const float* f, float* illum, int pitch, int r0, int r1, int z1, hipStream_t s);
// excitation maps / pick of the orders without a register-ring kernel, on rows [r0, r1), columns < z1 of the field f the step just stored
// (fdw_exc_select_kernel, fdw_exc_pick_kernel)
hipError_t launch_exc_select(const float* f, float* amp, int* texc, int pitch, int r0, int r1, int z1, int key, hipStream_t s);
hipError_t launch_exc_pick(const float* f, const int* texc, float* exc, int pitch, int r0, int r1, int z1, int key, hipStream_t s);
hipError_t launch_selftest(const float* src, float* out, hipStream_t s);
// one field [.][pitch] cropped to the cells (x0 + a dec, z0 + b dec), a < nxs, b < nzs, as one dense frame [nxs][nzs] (fdw_snapshot_kernel)
hipError_t launch_snapshot(const float* f, float* frame, int pitch, int x0, int z0, int dec, int nxs, int nzs, hipStream_t s);
// receiver rows the reference injects and images but never time-steps (truncated launch extents with a narrow x border): see fdw_static_rows_kernel
// trace samples of receiver rows the loop never time-steps: see fdw_record_static_kernel
hipError_t launch_record_static(const float* p0, const float* pp0, float* rec, int pitch, int row0, int nrows, int gz, int rec_x0, int rec_n, int nsteps,
                               int nbatch, long long bstride, long long rec_bstride, hipStream_t s);
hipError_t launch_static_rows(float* pp, const float* psrc, float* img, const float* samples, int pitch, int row0, int nrows, int gz,
                              int img_z0, int img_z1, hipStream_t s);
hipError_t launch_image_laplacian(const float* d_img, float* d_out, int nx, int nz, float dx, float dz, hipStream_t s);
// d_part: 3 * nblocks doubles of scratch; d_out: {sum (a-b)^2, sum b^2, max |b|} carried in double and, with `serial`, [3], [4] = the two
// sums as the reference tool forms them (one term after the other into fp32 sums)
hipError_t launch_image_compare(const float* a, const float* b, size_t n, float* diff, double* d_part, int nblocks, double* d_out, int serial, hipStream_t s);

// ---- random-border velocity model on the device (fdw_border.hip) ----
constexpr int kRandLag = 31;          // glibc TYPE_3: y[t] = y[t-31] + y[t-3]
struct RandWindow {                   // (y[K-31] .. y[K-1]) for a stream position K
    unsigned w[kRandLag];
};
struct BorderArgs {
    const float* vp;                  // interior model [nx][nz]
    const int* draws;                 // the rand() values one extendvel_linear call consumes, in its order
    float* vel;                       // extended model [nxe][pitch] (may be null)
    float* vel2;                      // its square [nxe][pitch]
    int nx, nz, nxb, nzb, pitch;
};
struct RandBase {                     // y[K-31] .. y[K+29]: the window at the position of draw 0 and the next 30 words
    unsigned y[2 * kRandLag - 1];
};
// d_tab: x^(31 l) mod P for l < 64 as [31][64] (coefficient-major), then x^(31 64 h) mod P for block h as [blocks][31];
// P = x^31 - x^28 - 1 is the characteristic polynomial of the generator.  d_out[i] = draw number i counted from the base.
hipError_t launch_rand_stream(const RandBase& base, const unsigned* d_tab, long long n, int* d_out, hipStream_t s);
hipError_t launch_extendvel(const BorderArgs& a, hipStream_t s);
// d_in [nshots][nx][nt] -> d_out [nshots][nt][nx]
hipError_t launch_gather_transpose(const float* d_in, float* d_out, int nx, int nt, int nshots, hipStream_t s);
// d_out[i] = d_a[i] - d_b[i] for i < n, one fp32 subtraction each; d_out may be d_a (fdw_gather_residual_kernel)
hipError_t launch_gather_residual(const float* d_a, const float* d_b, float* d_out, size_t n, hipStream_t s);
// encoded data gather (fdw_encode_gathers_kernel): d_out[ix][it] = the fold over s ascending, 0 <= it - lag[s] < nt, of acc + w[s] * d_in[s][ix][it - lag[s]]
hipError_t launch_encode_gathers(const float* d_in, const int* d_lag, const float* d_w, float* d_out, int nshots, int nx, int nt, hipStream_t s);
// the same fold for nplanes encodings of one resident data set (fdw_encode_gathers_multi_kernel): d_lag, d_w [nplanes][nshots], d_out [nplanes][nx][nt]
hipError_t launch_encode_gathers_multi(const float* d_in, const int* d_lag, const float* d_w, float* d_out, int nshots, int nplanes, int nx, int nt,
                                       hipStream_t s);

}  // namespace fdw

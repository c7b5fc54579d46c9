/*
 * fdwave.h -- C ABI of libfdwave.so: the MI355X (gfx950) implementation of the 2-D acoustic
 * finite-difference hot path of FernandoSchett/parallel_finite_difference_computation.
 *
 * Plain C: pointers, ints, floats.  No HIP or torch types cross this boundary (a stream is a void*
 * that is really a hipStream_t; NULL = the context's own stream).  Every function returns 0 on
 * success or a negative FDW_E* code, with a human-readable message in fdw_last_error().  There is
 * NO CPU fallback: without a usable HIP device fdw_create() fails with FDW_ENODEVICE.
 *
 * Each entry point cites the reference interface it replaces.  File tags:
 *   S = cuda_reference_stencil_computation/fd-source-code.cu
 *   R = cuda_reference_RTM/src/fd-code.cu
 *   H = cuda_reference_RTM/lib/include/functions.h
 *   F = cuda_reference_RTM/lib/src/functions.c
 *
 * Array conventions are the reference's: a field is float[nxe][nze], x slow, z contiguous
 * (idx = ix*nze + iz, R:58), fp32 little endian, nxe = nx + 2*nxb, nze = nz + 2*nzb (R:410-411).
 * "Host" arrays are dense with that layout.  "Device" arrays (fdw_dev_*) are pitched:
 * float[nxl][pitch] with pitch = fdw_pitch(ctx) >= nze, padding columns must be zero.
 */
#ifndef FDWAVE_H
#define FDWAVE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDW_VERSION 2
#define FDW_MAX_ORDER 32

/* error codes */
#define FDW_OK 0
#define FDW_EINVAL (-1)    /* bad argument (message says which) */
#define FDW_ENODEVICE (-2) /* no HIP device / wrong architecture / HIP runtime failure at create */
#define FDW_EHIP (-3)      /* a HIP call failed later */
#define FDW_ENOMEM (-4)
#define FDW_ESTATE (-5)    /* call sequence error (e.g. back() before forward() in a device-resident shot) */
#define FDW_ECOMM (-6)     /* librccl missing, an RCCL call failed, or the ranks of an exchange disagree */

typedef struct fdw_ctx fdw_ctx;

/* The arguments of the reference's fd_init (R:200, H:15; stencil variant S:241) plus the switches
 * that the reference fixes at build time. */
typedef struct fdw_params {
    int order;      /* even, 2..FDW_MAX_ORDER (R:374 default 8).  2/4/6/8 use the register-window kernel */
    int nxe, nze;   /* extended grid (R:410-411) */
    int nxb, nzb;   /* absorbing border widths (R:375-376); 0 allowed (stencil program does not use them) */
    int nt;         /* time steps per propagation (R:351) */
    float dx, dz, dt;
    float fac;      /* taper strength F (R:377), in (0,1] */
    int compat;     /* 1: reproduce the reference's truncated RTM launch extents, gridx = floor(nxe/8)
                       etc. (R:185-195) -- required for parity with rtm_code output;
                       0: update the whole array */
    int coef_cxx;   /* 1: generic-order weights with float cosf/powf as in the stencil program (S:184-216
                       is compiled as C++); 0: double libm as in libsource.a (F:160-192).  Irrelevant
                       for order 2/4/6/8 */
    int dialect;    /* 0 (FDW_DIALECT_RTM): the CUDA programs' arithmetic and one-sided taper (everything above);
                       1 (FDW_DIALECT_MOD): the CPU-serial sibling's forward modelling -- dpct_gpu_rtm_domain_division/src:
                       fd_step's single accumulator (timestep/fd.c:24-46), four-sided taper_apply with taper = exp(-(F*(nb-i))^2)
                       (boundary/taper.c:26-66), whole-grid update; order <= 8; only fdw_model_shot and the host helpers use it */
    int numerics;   /* 0 (FDW_NUMERICS_EXACT, the default of a zeroed struct): the reference's arithmetic operation for operation (nvcc
                       --fmad=false: every product and every sum of the Laplacian rounded, R:66-72) -- results identical to the no-FMA
                       CUDA build bit for bit;
                       1 (FDW_NUMERICS_FAST): the same stencil with the symmetric taps summed first and fused multiply-adds,
                       lap = c0 p + sum_k [cz_k (p(j-k) + p(j+k)) + cx_k (p(i-k) + p(i+k))] (csrc/fdw_device.h), about half the vector
                       instructions; the fp64 leap-frog (R:89), the taper, the launch extents and every other quirk are unchanged.
                       Results agree with EXACT to rounding: <= 1e-5 max-norm-relative over the 1 700 steps of the reference's new_mod
                       deck (tests), the size of the reference's own FMA / no-FMA difference.  Dialects 1 and 2 take the same formula
                       with the spacings folded into the weights (c_k * d?2inv once instead of inside every term): the sibling's committed
                       3lay_mod gather is met to 2.2e-6 in the max norm (1.3e-5 in the L2 norm) over its 1 001 steps.
                       Against the float64 statement of the RTM loop (tests/rtm_restatement.py) the FAST image of a whole shot is
                       within 1.9e-6 max-norm-relative on two decks but 1.23e-5 on a third (70 x 53, dx = 8, dz = 12.5, order 8,
                       400 steps), where EXACT is within 1.6e-6: FAST is held to 2e-5 there (tests/test_backward_pins.py). */
} fdw_params;
enum { FDW_NUMERICS_EXACT = 0, FDW_NUMERICS_FAST = 1 };
enum { FDW_DIALECT_RTM = 0, FDW_DIALECT_MOD = 1, FDW_DIALECT_RTM_STORED = 2 };
/* 2 (FDW_DIALECT_RTM_STORED): the same sibling's stored-wavefield RTM (src/rtm_main.cpp): fd_step arithmetic as dialect 1, one-cell
 * source, taper_apply2 (top strip only, taper.c:68-83) with the taper table of dialect 1; only fdw_rtm_stored_shot uses it. */

/* A slab of the global grid owned by one device (domain decomposition along x, the slow axis).
 * The reference has no multi-GPU path; slab 0..nxe is the single-GPU case. */
typedef struct fdw_slab {
    int x_off; /* global row index of local row 0 (may include ghost rows) */
    int nxl;   /* local rows held on this device, ghost rows included */
} fdw_slab;

const char *fdw_last_error(void);
int fdw_version(void);

/* ---- life cycle ------------------------------------------------------------------------------
 * fdw_create       replaces fd_init + fd_init_cuda (R:146-224, S:218-262): derived constants
 *                  (d?2inv, dt2, scaled coefficients, taper tables), device buffers, launch
 *                  geometry.  device = HIP ordinal.
 * fdw_create_slab  same for one x-slab of a decomposed grid; slab rows must hold order/2 ghost
 *                  rows (or more) towards every neighbouring slab.
 * fdw_destroy      replaces the cudaFree block R:569-582 / S:264-275. */
int fdw_create(const fdw_params *prm, int device, fdw_ctx **out);
/* fdw_device_count   HIP devices visible to this process (0 when there is none or HIP cannot start).
 * fdw_device_usable  0 if `device` exists, is a gfx950 and can be selected -- what a rank of a multi-GPU job checks ALONE before it enters
 *                    a collective call (rtm_code slabs=N). */
int fdw_device_count(void);
int fdw_device_usable(int device);
int fdw_create_slab(const fdw_params *prm, const fdw_slab *slab, int device, fdw_ctx **out);
void fdw_destroy(fdw_ctx *ctx);

/* ---- host-array entry points (the reference's L2 seam; synchronous like the reference) ---------
 *
 * fdw_laplacian   S:320-333: H2D(p), kernel_lap, D2H(lap).  lap border cells are written as 0
 *                 (the committed golden has zeros there).  Uses coef_cxx weights.
 *
 * fdw_forward     fd_forward R:247-288.  p,pp in/out (the reference uploads them R:230-231 and
 *                 downloads d_p,d_pp R:285-286); v2 = squared velocity; sx,sz = source position on
 *                 the extended grid (R:406,408); srce[nsteps]; nsteps normally = nt.
 *
 * fdw_back        fd_back R:290-341.  snap0 = P and snap1 = PP of the forward pass (R:502-507),
 *                 d_obs = one shot gather [nx][nt] (R:426-435), gz on the extended grid (R:409),
 *                 imloc[nx][nz] in/out (uploaded R:243, downloaded R:340).
 *
 * fdw_shot        forward + back for one shot with everything device-resident (no snapshot round
 *                 trip): what main does per shot R:496-518 minus the host memsets.  Results are
 *                 identical to fdw_forward followed by fdw_back.  P/PP may be NULL.
 */
int fdw_laplacian(fdw_ctx *ctx, const float *p, float *lap);
int fdw_forward(fdw_ctx *ctx, float *p, float *pp, const float *v2, int sx, int sz, const float *srce, int nsteps);
int fdw_back(fdw_ctx *ctx, const float *v2, const float *snap0, const float *snap1, const float *d_obs, int gz,
             float *imloc, int nsteps);
int fdw_shot(fdw_ctx *ctx, const float *v2, int sx, int sz, int gz, const float *srce, const float *d_obs,
             float *imloc, float *P, float *PP);

/* ---- device-array entry points (benchmarks, multi-GPU drivers; asynchronous on `stream`) -------
 * Buffers are caller-owned device memory laid out [nxl][fdw_pitch()] (e.g. a torch tensor).
 *
 * THE STREAM CONTRACT of every entry point that takes a `stream` (pinned by tests/test_stream_contract.py):
 *   stream == NULL  the context's own stream, created with hipStreamNonBlocking.  It has NO implicit ordering against any stream of the
 *                   caller's, the legacy default stream included: what filled the buffers must have COMPLETED before the call (the caller
 *                   synchronised, or waited for an event on the host), and the results are complete only once the device (or, for the
 *                   host-array entry points, the call itself) has synchronised.  A fill queued on a torch stream and not waited for races
 *                   with the kernels here.
 *   stream != NULL  a hipStream_t of the caller's.  EVERY kernel launch, device copy and memset of the call is issued on that stream, in
 *                   order, and the call returns without synchronising: it sees whatever was queued on the stream before it -- a producer that
 *                   has not run yet included -- and work queued on the stream after it sees its results.  Nothing is issued on the context's
 *                   own stream, and no other stream or event is involved.  Chained calls on one stream need no host synchronisation in between.
 *                   The ONE exception is fdw_dev_check_field, which issues its check on the stream and then synchronises it to return the count.
 *                   ONE amendment: fdw_dev_steps2 with a pass-band depth above 1 or the moving cut (fdw_set_pass_bands, fdw_set_pass_cut, below) forks part of its passes onto side
 *                   streams of the context behind an event of the caller's stream and joins them into it before it returns; towards the
 *                   caller the ordering above holds unchanged.
 *   Host arguments (pointers to ip / ipp, role[], scalars) are read and written before the call returns.
 *
 * PRECONDITION of every entry point that takes wavefields (host or device) on a context with compat = 1 and nxe not a multiple of 8:
 * inside the damped strip (columns < 8*floor(nzb/8)) the rows the reference never time-steps (>= 8*floor(nxe/8)) must be ZERO.  The
 * reference damps those rows with taperx every step although nothing ever rewrites them (R:94-117 with the grids of R:185-195); the kernels
 * here damp on load instead of in place (csrc/fdw_device.h, "lazy taper") and cannot reproduce that for rows they never store.  Every call
 * site of the reference satisfies it (fields start at zero, R:496-497, R:511-514, and snapshots come from such runs).  The host-array entry
 * points check it and return FDW_EINVAL; the fdw_dev_* ones do not look at the data (it is on the device, and they are asynchronous) -- a
 * caller that violates it gets values in those few rows of the strip that differ from the reference's.  fdw_dev_check_field(ctx, d_field,
 * stream) runs the same check ON the device for such a caller (synchronises `stream`; FDW_EINVAL with the count of offending cells).
 * A source row in those rows is refused (FDW_EINVAL) by every path.
 *
 * fdw_dev_step    one fused time step on rows [r0,r1) of the slab:
 *                   mode 0 FWD   taper + Laplacian + leap-frog + point source  (R:264-267)
 *                   mode 1 PLAIN Laplacian + leap-frog                          (R:317-318)
 *                   mode 2 RECV  taper + Laplacian + leap-frog + receivers + imaging (R:325-329)
 *                 d_p is read, d_pp is read and overwritten with the new field (the caller swaps
 *                 roles afterwards, R:260-262).  pp_twice: 0 on the first step after fresh data,
 *                 1 afterwards (see csrc/fdw_device.h "lazy taper").  d_inj: FWD: device pointer to
 *                 the source sample of this step, inj_x/inj_z its GLOBAL position (inj_x < 0: no
 *                 source); RECV: device pointer to nx receiver samples of this step (row-contiguous,
 *                 i.e. d_obs transposed to [it][ix]), inj_z = gz.  d_psrc/d_img: RECV only.
 * fdw_dev_taper_finalize  applies the one taper pass the lazy scheme still owes to a field that was
 *                 last used as d_p (needed before it is exported or used untapered).
 * fdw_dev_laplacian  mode 3: d_lap = Laplacian(d_p), zero outside the interior.
 * fdw_dev_step2   TWO forward iterations in one pass (temporal blocking, order 8, full slab): reads d_p = newest
 *                 field u^n (the reference's d_p AFTER its swap), d_pp = u^{n-1}, writes u^{n+1} to d_out1 and
 *                 u^{n+2} to d_out2 (no aliasing allowed), d_srce_it -> {srce[it], srce[it+1]}.  10 B/point/step
 *                 instead of 16; results are bit-identical to two fdw_dev_step calls.
 * fdw_dev_steps2  nsteps iterations over FOUR rotating buffers, in pairs through fdw_dev_step2 (odd remainder:
 *                 one-step kernel).  ip and ipp index the reference's (d_p, d_pp) before the first swap on entry
 *                 and after the loop on return.
 * fdw_dev_step4   FOUR forward iterations in one pass of the wave-pipeline kernel (order 8, fields < 2 GiB): d_p = u^n,
 *                 d_pp = u^{n-1} -> d_out1 = u^{n+3}, d_out2 = u^{n+4} on local rows [r0, r1) and, optionally, [r0b, r1b)
 *                 (r1 < 0: every row the reference time-steps); rows within 16 of a range end are read from d_p / d_pp, so
 *                 a slab driver shrinks the range by 16 rows per pass between two halo exchanges (decomp.py).
 *                 d_srce_it -> srce[it .. it+3]; xchunk 0 = automatic.  Bit-identical to four fdw_dev_step calls.  Rows of a range that
 *                 the reference never time-steps (compat extents, rows >= xlim; with r1 < 0 all of them) receive the inputs' rows, which
 *                 are static -- also where a range holds such rows only and nothing is launched for it; no row outside the ranges is
 *                 written, the rows of a gap between the two ranges included (tests/test_dev_footprint.py) -- fdw_dev_back4 alike.
 * fdw_dev_steps_shrink  like fdw_dev_steps for one slab of a decomposed grid between two halo exchanges:
 *                 step j = j0.. of the cycle updates rows [h*j, nxl - h*j) on the sides that have a
 *                 neighbour (shrink_lo / shrink_hi), see decomp.py.
 * fdw_dev_back_iter  ONE iteration of fd_back's loop (R:302-339) on local rows [r0, r1) of a slab (or of the whole grid): with
 *                 step_source = 1 the source field is reconstructed one step back in time first, F_k = leap-frog(d_f1 = F_{k-1},
 *                 d_f0 = F_{k-2}) written over d_f0 (R:317-318: no taper, no source); with step_source = 0 (iterations 0 and 1, whose
 *                 source fields are the two snapshots, R:304-314) d_f1 is used as it stands and d_f0 is ignored.  Then the receiver
 *                 step (taper + Laplacian + leap-frog, d_pr read, d_ppr overwritten, R:325-327), the injection of d_samples[0..nx)
 *                 = d_obs[.][nt-1-it] on column gz of the interior rows (R:328) and img += F_k * new receiver field (R:329), where
 *                 d_img is [nxl][pitch] on the extended grid; its INTERIOR cells are what kernel_img defines (R:133-144) -- the imaging
 *                 epilogues also accumulate in border cells inside their launch extents, which no entry point reports.
 *                 The caller swaps (d_f1, d_f0) when step_source and (d_pr, d_ppr) always.
 *                 Rows of different calls of one iteration must be disjoint; pp_twice as for fdw_dev_step.  One launch where the fused
 *                 backward kernel exists (order <= 8), two otherwise.
 * fdw_dev_back4   FOUR iterations of that loop (no snapshot iterations among them) as two passes of the wave-pipeline kernel (order 8, fields
 *                 < 2 GiB, no receiver rows beyond the time-stepped rows; fdw_back_pipe_active says whether fdw_back itself takes this path on this
 *                 grid): pass 1 reconstructs F_it .. F_{it+3} from d_f1 = F_{it-1}, d_f0 = F_{it-2} into d_lvl0, d_lvl1, d_fo1, d_fo2; pass 2
 *                 advances the receiver field four times (d_pr = r^it, d_ppr = r^{it-1} -> d_ro1 = r^{it+3}, d_ro2 = r^{it+4}), injecting
 *                 d_samples + j * sample_stride at iteration it + j, and adds the four imaging products to d_img in iteration order.  Local
 *                 rows [r0, r1) and [r0b, r1b) (r1 < 0: all); rows within 16 of a range end are read from the inputs, so a slab driver
 *                 shrinks the range by 16 rows per call between two halo exchanges.  No buffer may alias another.  Bit-identical to four
 *                 fdw_dev_back_iter calls.  d_lvl0 / d_lvl1 receive F_it / F_{it+1} only in the two-pass form (FDW_NO_BACK_FUSED); the fused
 *                 pass keeps those two levels on the chip and leaves the two buffers untouched (they must still be valid memory).
 * fdw_dev_steps   nsteps FWD steps with internal role swapping; *d_srce is srce[] on the device
 *                 (may be NULL = no source).  Every step swaps the two roles first and then writes the new field
 *                 over d_pp (R:260-267): after an odd number of steps the newest field is in the buffer passed
 *                 as d_p, after an even number in the one passed as d_pp (as in the reference loop).
 */
int fdw_pitch(const fdw_ctx *ctx);           /* floats per row of a device array */
size_t fdw_field_bytes(const fdw_ctx *ctx);  /* nxl * pitch * 4 */
int fdw_dev_step(fdw_ctx *ctx, int mode, const float *d_p, float *d_pp, const float *d_v2, int r0, int r1,
                 int pp_twice, const float *d_inj, int inj_x, int inj_z, const float *d_psrc, float *d_img,
                 void *stream);
int fdw_dev_back_iter(fdw_ctx *ctx, int step_source, const float *d_f1, float *d_f0, const float *d_pr, float *d_ppr, const float *d_v2,
                      int r0, int r1, int pp_twice, const float *d_samples, int gz, float *d_img, void *stream);
int fdw_dev_back4(fdw_ctx *ctx, const float *d_f1, const float *d_f0, float *d_fo1, float *d_fo2, float *d_lvl0, float *d_lvl1, const float *d_pr,
                  const float *d_ppr, float *d_ro1, float *d_ro2, const float *d_v2, const float *d_samples, int sample_stride, int gz, float *d_img,
                  int pp_twice, int r0, int r1, int r0b, int r1b, int xchunk, void *stream);
int fdw_back_pipe_active(const fdw_ctx *ctx);
int fdw_dev_steps(fdw_ctx *ctx, float *d_p, float *d_pp, const float *d_v2, const float *d_srce, int sx, int sz,
                  int it0, int nsteps, int first_pp_twice, void *stream);
int fdw_dev_steps_shrink(fdw_ctx *ctx, float *d_p, float *d_pp, const float *d_v2, const float *d_srce, int sx, int sz,
                         int it0, int nsteps, int first_pp_twice, int j0, int shrink_lo, int shrink_hi, void *stream);
int fdw_dev_step2(fdw_ctx *ctx, const float *d_p, const float *d_pp, const float *d_v2, float *d_out1, float *d_out2, int pp_twice,
                  const float *d_srce_it, int sx, int sz, void *stream);
int fdw_dev_step4(fdw_ctx *ctx, const float *d_p, const float *d_pp, const float *d_v2, float *d_out1, float *d_out2, int pp_twice,
                  const float *d_srce_it, int sx, int sz, int r0, int r1, int r0b, int r1b, int xchunk, void *stream);
int fdw_dev_steps2(fdw_ctx *ctx, float *const *d_buf, const float *d_v2, const float *d_srce, int sx, int sz, int it0, int nsteps,
                   int first_pp_twice, int *ip, int *ipp, void *stream);
int fdw_dev_taper_finalize(fdw_ctx *ctx, float *d_f, void *stream);
int fdw_dev_check_field(fdw_ctx *ctx, const float *d_f, void *stream);
int fdw_dev_laplacian(fdw_ctx *ctx, const float *d_p, float *d_lap, void *stream);

/* ---- forward-modelling producer -------------------------------------------------------
 * fdw_model_shot  one shot of mod_main's loop (dpct_gpu_rtm_domain_division/src/mod_main.cpp:140-174) on a context created with
 *                 dialect = FDW_DIALECT_MOD: P = PP = 0; nt x { fd_step; ptsrc (7x7 Gaussian around (sx, sz), source/ptsrc.c:12-58);
 *                 taper_apply(PP); taper_apply(P); data[ix][it] = P[ix+nxb][gz] }.  vel2[nxe][nze] is the extended squared
 *                 velocity (after fdw_mod_extendvel), srce[nt], data[nx][nt].  Device resident, one launch per step.
 * fdw_mod_extendvel       taper.c:7-23: replicate the edge values outwards (in place, [nxe][nze])
 * fdw_mod_ricker_wavelet  ptsrc.c:88-99: Ricker delayed by 1/fpeak, zero after 2/fpeak
 * fdw_mod_taper_tables    taper.c:26-44 */
int fdw_model_shot(fdw_ctx *ctx, const float *vel2, int sx, int sz, int gz, const float *srce, int nt, float *data);
/* the same loop on caller-owned device arrays (d_p / d_pp = mod_main's P / PP, swapped every step; d_rec[it][nx] or NULL) */
int fdw_dev_model_steps(fdw_ctx *ctx, float *d_p, float *d_pp, const float *d_v2, const float *d_srce, int sx, int sz, int gz,
                        float *d_rec, int it0, int nsteps, void *stream);
void fdw_mod_extendvel(int nx, int nz, int nxb, int nzb, float *vel);
void fdw_mod_ricker_wavelet(int nt, float dt, float fpeak, float *srce);
void fdw_mod_taper_tables(int nxb, int nzb, float fac, float *taper_x, float *taper_z);

/* ---- stored-wavefield RTM of the CPU-serial sibling ----------------------------------------
 * fdw_rtm_stored_shot  one shot of rtm_main's loop (dpct_gpu_rtm_domain_division/src/rtm_main.cpp:158-240) on a context created with
 *                 dialect = FDW_DIALECT_RTM_STORED: the source pass keeps the field of every step on the device (nt fields: fails with
 *                 FDW_ENOMEM when they do not fit), the receiver pass injects sample nt-it of every trace of shot `is` -- read from the
 *                 WHOLE gather dobs[ns][nx][nt] of n_floats floats exactly as the reference indexes it, i.e. one sample past the trace at
 *                 it = 0 (a sample past the end of the file counts as 0) and with its nzb row offset (rtm_main.cpp:203) -- and the image
 *                 accumulates swf[nt-it-1] * rwf[it] in iteration order (same sums as rtm_main.cpp:224-230).  imloc[nx][nz] is overwritten.
 *                 When the nt fields do not fit -- the budget of fdw_set_store_budget (or FDW_STORE_BUDGET_MB), else what hipMalloc grants --
 *                 the source pass CHECKPOINTS: it keeps the pair of fields every m-th step starts from, and the receiver pass recomputes
 *                 one segment of m fields at a time from its pair (2 ceil(nt/m) + m + 1 fields, least near m = sqrt(2 nt); one more forward
 *                 pass of launches).  The recomputation repeats the same launches on the same inputs: the image is bit-identical to the
 *                 unconstrained run.  FDW_ENOMEM only when not even that fits.
 * fdw_set_store_budget  bytes the stored source fields may occupy (0 = no limit of our own); fdw_store_segments: how many segments the last
 *                 fdw_rtm_stored_shot was cut into (1 = every field was kept). */
int fdw_rtm_stored_shot(fdw_ctx *ctx, const float *vel2, int sx, int sz, int gz, const float *srce, int nt, const float *dobs,
                        size_t n_floats, int is, float *imloc);
int fdw_set_store_budget(fdw_ctx *ctx, size_t bytes);
int fdw_store_segments(const fdw_ctx *ctx);

/* ---- image post-processing -----------------------------------------------------------------
 * fdw_image_laplacian  the reference's offline filter models/3lay_mod/laplace.f90:25-29 (dir.image -> dir.imalap): second-order
 *                 Laplacian of img[nx][nz] with the frame left at zero, on `device`. */
int fdw_image_laplacian(int device, const float *img, int nx, int nz, float dx, float dz, float *out);
/* fdw_image_compare  the reference's image comparer models/marmousi/psnr ("./psnr file1 file2"; it ships as an ELF without source, so its
 *                 behaviour is restated from its output): stats = {MSE = mean (a-b)^2, RMSE, SNR = 10 log10(sum b^2 / sum (a-b)^2) dB,
 *                 PSNR = 20 log10(max |b| / RMSE) dB}; diff (may be NULL) = a - b, what the tool writes to ./dir.output.  On `device`.
 *                 exact_sums = 0: the tool's own arithmetic -- the squares added one after the other into fp32 sums (a serial recurrence: one
 *                 lane walks the arrays, ~10 ns per element), fp32 quotient and root -- so the values are the tool's, digit for digit;
 *                 exact_sums = 1: a parallel reduction carrying the same terms in double (fast; differs from the tool's figures by the
 *                 rounding the tool accumulates, up to a few 1e-5 relative on the reference's own images). */
int fdw_image_compare(int device, const float *a, const float *b, size_t n, float *diff, double stats[4], int exact_sums);

/* host <-> pitched device copies (dense [rows][nze] on the host side), synchronous */
int fdw_upload_field(fdw_ctx *ctx, float *d_dst, const float *h_src);
int fdw_download_field(fdw_ctx *ctx, float *h_dst, const float *d_src);

/* ---- random-border model generated on the device ---------------------
 * The reference rebuilds its extended velocity model on the host for every shot (extendvel_linear, F:336-394, called at
 * R:486; vel2 = vpe * vpe at R:488-494) and uploads it (R:205).  Here the interior model is uploaded once and each
 * shot's border is generated in HBM from the same unseeded glibc rand() stream, addressed by position: shot s of a
 * fresh process consumes draws [s T, (s+1) T), T = fdw_border_draws(...).  Cells the reference's loops never write
 * (bottom corners when nxb > nzb) are zero, as in the reference's calloc'ed array.
 * fdw_border_draws          rand() calls one extendvel_linear consumes: nx nzb + 2 nz nxb + 2 nzb (nzb + 1)
 * fdw_model_resident        uploads the interior velocity vp[nx][nz] (not squared); RTM dialect, full-grid context
 * fdw_dev_extendvel_linear  fills the context's resident vel2 (and vel_out[nxe][nze] on the host if not NULL) from
 *                           draws [draw_offset, draw_offset + T) of the seed-1 stream
 * fdw_shot_resident         fdw_shot (R:496-520) on the resident vel2; FDW_ESTATE if a host model was uploaded since
 * fdw_rand_stream           out[i] = draw number draw_offset + i of that stream, produced by the device generator (tests)
 * fdw_shot_batch            `nshots` consecutive shots of the reference's loop (R:480-520) through ONE launch per time step: shot b has
 *                           source row sx0 + b dsx (R:405-407), gather d_obs + b nx nt, image imloc + b nx nz (accumulated into, as
 *                           fdw_shot does), model v2_all + b nxe nze or, v2_all == NULL, the border model of draws
 *                           [draw_offset + b T, ...) drawn on the device.  Results are those of the shots run one by one, bit for bit;
 *                           contexts whose regime the batched launches do not cover (large grids, orders above 8, receiver rows
 *                           outside the truncated extents) run them one by one.
 * fdw_shot_batch_max        batch size that fills the chip for this geometry (1: batching gains nothing), at most what the batch budget
 *                           holds of fdw_shot_batch's eleven fields per shot
 * fdw_set_batch_budget      bytes the buffers of a batch may take; 0 = the default.  The budget in force is, in this order: the value set
 *                           here if non-zero, else the environment variable FDW_BATCH_BUDGET_BYTES (a decimal byte count, read at every
 *                           call; unset, empty, zero or unparsable: ignored), else 6 GiB.  So the call wins over the environment (unlike
 *                           FDW_STORE_BUDGET_MB, which overrides fdw_set_store_budget).  Only this call writes the context's value.
 *                           NULL context: FDW_EINVAL.  It bounds fdw_shot_batch_max and the parts below; results never depend on it.
 * fdw_batch_parts           how many batched launch sequences the last batched call on this context went through: 0 = its shots ran one
 *                           by one (nshots == 1, a regime the batched launches do not cover, or no room on the device), 1 = the whole
 *                           batch at once, k = k parts (a last part of a single shot counts).  Written by every batched call.
 * Who splits.  fdw_shot_batch_illum, fdw_shot_batch_residual, fdw_shot_line_batch, fdw_shot_line_batch_residual and fdw_shot_excitation_batch hold more per shot than
 * the eleven fields fdw_shot_batch_max counts and cut a batch that exceeds the budget into parts themselves.  fdw_shot_batch,
 * fdw_record_shot_batch, fdw_record_shot_line_batch and fdw_model_shot_batch have NO part loop: they take `nshots` whole, whatever the
 * budget says (fdw_batch_parts 1 or 0); their callers walk the shots in groups of at most fdw_shot_batch_max.
 * fdw_born_shot_batch and fdw_born_shot_line_batch split too: per shot they hold the eleven fields and 1 + [data0 != NULL] + [line]
 * gathers [nt][nx] (the scattered traces, the background traces, the line gathers); see "Born modelling driven by a line source, and
 * batches of Born shots".
 */
long long fdw_border_draws(int nx, int nz, int nxb, int nzb);
int fdw_shot_batch(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                   const float *srce, const float *d_obs, float *imloc);
int fdw_shot_batch_max(const fdw_ctx *ctx);
int fdw_set_batch_budget(fdw_ctx *ctx, size_t bytes);
int fdw_batch_parts(const fdw_ctx *ctx);
/* mod_main's shot loop (mod_main.cpp:140-174) for `nshots` consecutive shots (source rows sx0 + b dsx, M:99-101) on its one velocity
 * model, one launch per time step for all of them; data[nshots][nx][nt].  Same results as fdw_model_shot per shot, bit for bit. */
int fdw_model_shot_batch(fdw_ctx *ctx, int nshots, const float *vel2, int sx0, int dsx, int sz, int gz, const float *srce, int nt, float *data);
int fdw_model_resident(fdw_ctx *ctx, const float *vp);
int fdw_dev_extendvel_linear(fdw_ctx *ctx, unsigned long long draw_offset, float *vel_out);

/* ---- recorded shot gathers of the RTM dialect (the data rtm_code migrates, R:420-424) ------------------------------------------
 * Definition: data[ix][it] (ix < nx, it < nt) is what the reference's d_pp holds at row nxb + ix, column gz at the END of iteration it of
 * fd_forward's loop (R:259-267), i.e. after kernel_src (R:267): the new field u^{it+1}, undamped (the taper of R:264 reaches it only at
 * the start of the next iteration), a source on the receiver cell included.  Backward iteration k of fd_back injects sample nt-1-k
 * (R:328) into r^{k+1} and images it against F_k = u^{nt-k}, so sample j meets u^{j+1}, the level it was recorded from: migrating such a
 * gather correlates equal time levels.  (The sibling's mod_main records the CURRENT field instead, mod_main.cpp:155-157.)  Receiver
 * rows the loop never time-steps (compat extents: rows >= xlim) record what d_pp holds there; gz must lie in [0, zlim), the columns the
 * loop time-steps (fdw_get_extents), else FDW_EINVAL.  RTM dialect only (FDW_ESTATE otherwise); EXACT and FAST numerics alike.
 * fdw_dev_record_steps   fdw_dev_steps2 (R:259-267, same buffers, indices and kernel family per pass, bit-identical fields) that also writes
 *                        the samples of iteration it to d_rec + it * nx (d_rec [>= it0+nsteps][nx] on the device, absolute row it, as
 *                        fdw_dev_model_steps does)
 * fdw_record_shot        one shot from rest (R:496-497, nt = the context's steps) on v2[nxe][nze]: data[nx][nt]; P / PP (may be NULL) are
 *                        fdw_forward's, P damped as R:285 downloads it.  Full-grid contexts.
 * fdw_record_shot_batch  `nshots` of them with source rows sx0 + b dsx (R:405-407) and models as fdw_shot_batch takes them (v2_all
 *                        [nshots][nxe][nze], or NULL: the border models of draws [draw_offset + b T, ...) on the resident model): one launch
 *                        per time step for the whole batch where fdw_shot_batch batches, the shots one by one otherwise; data
 *                        [nshots][nx][nt] equals fdw_record_shot shot by shot, bit for bit. */
int fdw_dev_record_steps(fdw_ctx *ctx, float *const *d_buf, const float *d_v2, const float *d_srce, int sx, int sz, int gz, float *d_rec,
                         int it0, int nsteps, int first_pp_twice, int *ip, int *ipp, void *stream);
int fdw_record_shot(fdw_ctx *ctx, const float *v2, int sx, int sz, int gz, const float *srce, float *data, float *P, float *PP);
int fdw_record_shot_batch(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                          const float *srce, float *data);
int fdw_shot_resident(fdw_ctx *ctx, int sx, int sz, int gz, const float *srce, const float *d_obs, float *imloc, float *P, float *PP);
int fdw_rand_stream(fdw_ctx *ctx, unsigned long long draw_offset, long long n, int *out);

/* ---- source illumination of the forward loop; illumination-compensated image ------------------------------------------------
 * Definition.  RTM dialect, full-grid contexts.  For every extended-grid cell (x, z) with x < xlim, z < zlim (fdw_get_extents)
 *     for it = 0 .. nsteps-1 (increasing):   I(x,z) = I(x,z) (+) ( u(x,z) (*) u(x,z) )
 * with u = what the reference's d_pp holds at the END of iteration it of fd_forward's loop (R:259-267, after kernel_src): the value the
 * kernels store as the new field, source sample included, undamped -- the level the recording definition above samples.  (*) and (+)
 * are fp32 round-to-nearest operations rounded separately (no fused multiply-add), in EXACT and in FAST numerics alike (FAST changes the
 * Laplacian only).  Cells outside the update extents keep their value; I is read-modify-write and starts from what the caller put there.
 * Dividing the cross-correlation image sum_t F_t R_t by I = sum_t F_t^2 takes out the strong shallow energy around each shot.  The
 * accumulation rides the forward loop's own passes (the four-step pipeline stores only two of its four levels, so no caller can form I
 * from outside without giving up temporal blocking): +8 B/point per pass.  Slab contexts and the sibling's dialects: FDW_ESTATE.
 * fdw_dev_illum_steps      fdw_dev_steps2 (same buffers, indices and kernel family per pass, bit-identical fields) that also accumulates
 *                          into d_illum [nxl][pitch] (a field-sized device array; its padding columns stay as they are).  d_illum == NULL:
 *                          FDW_EINVAL.  Orders above 8 and forced generic: the generic step followed by a plain add kernel.
 * fdw_shot_illum           fdw_shot whose forward loop goes through the illumination kernels: illum[nx][nz] (interior, like imloc) is
 *                          accumulated into; imloc, P, PP equal fdw_shot's bit for bit.  The accumulator field is allocated on first use.
 * fdw_shot_resident_illum  the same on the resident vel2 (fdw_shot_resident).
 * fdw_shot_batch_illum     fdw_shot_batch (same arguments, same batched launches where it batches) whose forward loop also accumulates
 *                          every shot's illumination: illum[nshots][nx][nz] is accumulated into per shot, through a per-shot accumulator
 *                          field on the device (one more batch buffer of [nshots] fields).  imloc equals fdw_shot_batch's bit for bit, illum
 *                          equals `nshots` calls of fdw_shot_illum / fdw_shot_resident_illum bit for bit.  Contexts whose regime the
 *                          batched launches do not cover, or a device without room for the accumulators, run the shots one by one --
 *                          the same bytes.  fdw_shot_batch_max counts the eleven fields per shot of fdw_shot_batch; a larger batch than
 *                          twelve fields per shot allow in the same budget is split into parts of that size inside the call.
 * fdw_image_compensate     pure host C, usable without a device:  m = max_i illum[i] (from 0.0f with '>' comparisons, so a NaN never
 *                          wins), s = eps (*) m, d_i = illum[i] (+) s, out_i = d_i > 0 ? img[i] (/) d_i : 0.0f (IEEE fp32 division; out may
 *                          alias img).  eps finite and >= 0, else FDW_EINVAL.  O(n) once per job. */
int fdw_dev_illum_steps(fdw_ctx *ctx, float *const *d_buf, const float *d_v2, const float *d_srce, int sx, int sz, float *d_illum, int it0,
                        int nsteps, int first_pp_twice, int *ip, int *ipp, void *stream);
int fdw_shot_illum(fdw_ctx *ctx, const float *v2, int sx, int sz, int gz, const float *srce, const float *d_obs, float *imloc, float *illum,
                   float *P, float *PP);
int fdw_shot_resident_illum(fdw_ctx *ctx, int sx, int sz, int gz, const float *srce, const float *d_obs, float *imloc, float *illum,
                            float *P, float *PP);
int fdw_shot_batch_illum(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                         const float *srce, const float *d_obs, float *imloc, float *illum);
int fdw_image_compensate(const float *img, const float *illum, size_t n, float eps, float *out);

/* ---- residual migration: image d_obs minus the gather the forward loop itself models --------------------------------------------
 * Definitions.  RTM dialect, full-grid contexts, EXACT and FAST numerics alike.
 *   d_mod[ix][it]   what fdw_record_shot returns for the same context, model, source, sz and gz (the recording definition above), bit for bit:
 *                   the recording kernels write it inside the forward loop the shot runs anyway.
 *   resid[ix][it]   d_obs[ix][it] (-) d_mod[ix][it]: one fp32 subtraction, round to nearest even, subnormals kept, nothing fused.
 *   sign            with d_obs from the true model and a reflector-free migration model the residual is the reflection data.
 *   image           the one fdw_shot forms when handed `resid` as its d_obs, bit for bit; P and PP are fdw_shot's.  With an accumulator,
 *                   illum is fdw_shot_illum's, bit for bit (the forward loop then records and accumulates in one launch per pass).
 *   gz              must lie in [0, zlim) as for recording, else FDW_EINVAL before anything is enqueued.
 *   consequence     a gather modelled by fdw_record_shot / rtm_model in the model it is migrated with gives a residual whose every word is
 *                   0x00000000, and the image then equals its entry values.
 *   misfit          0.5 * sum_i resid[i]^2 on the host: each square and the sum carried in double, the squares added one after the other in
 *                   memory order (a defined, bit-checkable number; O(nx nt) per shot).
 * The same difference is the data residual of full-waveform inversion: its migrated image is the gradient, and that image divided by the
 * illumination the gradient with the pseudo-Hessian preconditioner.  No weighting or time differentiation is applied.
 * Slab contexts and the sibling's dialects: FDW_ESTATE.
 * fdw_dev_gather_residual     d_out[i] = d_a[i] (-) d_b[i] for i < n on device arrays, asynchronous on `stream`; d_out may be d_a.
 * fdw_dev_record_illum_steps  fdw_dev_steps2 (same buffers and indices, bit-identical fields) that writes the trace rows of
 *                             fdw_dev_record_steps AND accumulates as fdw_dev_illum_steps does, each pass one launch (orders above 8 and
 *                             forced generic: the generic recording step followed by the add kernel; where fdw_dev_steps2 runs a pair of
 *                             steps through the two-step kernel: two single steps that land in the same buffers).  The refusals of both; d_rec or
 *                             d_illum NULL: FDW_EINVAL (the existing entry points are the ones to call).
 * fdw_shot_residual           fdw_shot (v2 == NULL: on the resident squared model) whose forward loop records d_mod on the device, then
 *                             d_obs (-) d_mod in place on the device, then the backward loop on the difference.  illum: NULL, or accumulated
 *                             into as by fdw_shot_illum.  resid: NULL, or [nx][nt], the residual as the backward loop read it.
 * fdw_shot_batch_residual     `nshots` of them as fdw_shot_batch takes shots and models: one launch per time step for the whole batch where
 *                             fdw_shot_batch batches, one residual launch over the batch; the shots one by one otherwise -- the same bytes.
 *                             imloc [nshots][nx][nz]; illum (NULL ok) [nshots][nx][nz]; resid (NULL ok) [nshots][nx][nt].  One more batch
 *                             buffer of [nshots][nt][nx] floats (and, with illum, fdw_shot_batch_illum's accumulators); batches larger
 *                             than the memory budget allows go through in parts.
 * fdw_gather_misfit           *misfit = 0.5 * sum resid[i]^2 as defined above; pure host C.  n == 0: 0.0.  A NaN propagates. */
int fdw_dev_gather_residual(fdw_ctx *ctx, const float *d_a, const float *d_b, float *d_out, size_t n, void *stream);
int fdw_dev_record_illum_steps(fdw_ctx *ctx, float *const *d_buf, const float *d_v2, const float *d_srce, int sx, int sz, int gz, float *d_rec,
                               float *d_illum, int it0, int nsteps, int first_pp_twice, int *ip, int *ipp, void *stream);
int fdw_shot_residual(fdw_ctx *ctx, const float *v2, int sx, int sz, int gz, const float *srce, const float *d_obs, float *imloc, float *illum,
                      float *resid, float *P, float *PP);
int fdw_shot_batch_residual(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                            const float *srce, const float *d_obs, float *imloc, float *illum, float *resid);
int fdw_gather_misfit(const float *resid, size_t n, double *misfit);

/* ---- wavefield snapshots from both loops of a shot (rtm_code's dir.snaps, dir.snaps_rec, dir.snapr) --------------------------------
 * The reference opens the three files and leaves them empty (R:465-470; its deck key iss, "save snaps of this source", R:368, is read and
 * dropped).  Definitions, for the parameters every = K >= 1 and dec = D >= 1, RTM dialect, full-grid contexts, EXACT and FAST numerics alike:
 *   levels     frames are taken at the time levels L = K, 2K, ... <= nt: nframes = nt / K (integer division, may be 0); frame j is level
 *              (j+1) K in all three sets, in ascending time.
 *   snaps      u^L: what d_pp holds at the end of forward iteration it = L-1, after kernel_src (R:267) -- the level the recorded gathers
 *              and the illumination sample: raw, undamped, source sample included.
 *   snaps_rec  F_k with k = nt - L: the source field backward iteration k images (d_p after the swap of R:321-323).  k = 0 is u^nt, k = 1
 *              the handed-over P, damped once (R:285); k >= 2 are reconstructed by the undamped leap-frog of R:317-318.
 *   snapr      r^{k+1} of the same iteration: d_ppr after kernel_sism (R:328), the field multiplied into the image at R:329.
 *   frame      the interior cells (nxb + a D, nzb + b D): nxs = ceil(nx / D) by nzs = ceil(nz / D) floats laid out [nxs][nzs], z fastest,
 *              like dir.image.  Cells the loops never time-step (compat extents) carry what the device arrays hold, as the reference's do.
 * So imloc = sum over k of snaps_rec(level nt-k) (*) snapr(level nt-k) on the cells kernel_img covers, added in iteration order, and
 * snaps_rec against snaps measures how well the reconstruction from the last two fields reproduces the forward run.
 * Frames stay in a device store per requested set ([nframes][nxs][nzs]) and each set is downloaded once at the end of the shot.  The forward
 * loop runs in segments that end on the levels; in the backward loop no pass of several iterations reaches across iteration nt - L, so a K
 * that is no multiple of four (two) leaves single iterations around every stop where the loop would otherwise run four (two) per pass:
 * measured on one MI355X at 8192^2, 500 steps, D = 8: K = 100 adds 1.8 % to the plain shot's 180 ms, K = 50 adds 5.8 % -- visibly more: prefer a multiple of four.
 * Every family of passes equals the one-step iteration bit for bit: imloc, P, PP and illum are fdw_shot's / fdw_shot_illum's.
 * fdw_snap_dims     the frame count and shape for a geometry; needs no device.  every < 1 or dec < 1: FDW_EINVAL.
 * fdw_dev_snapshot  one frame of the caller-owned device field d_field [nxl][pitch] into d_frame [nxs][nzs] (device), asynchronous on `stream`:
 *                   a crop-and-decimate copy without arithmetic (NaN payloads, -0 and subnormals survive).  Slab contexts: FDW_ESTATE.
 * fdw_shot_snaps    fdw_shot (v2 == NULL: fdw_shot_resident on the resident model) with an optional illum (NULL, or as fdw_shot_illum) that
 *                   also fills the host arrays of `snaps` ([nframes][nxs][nzs] each; any may be NULL, all three NULL: FDW_EINVAL).  Slab
 *                   contexts, the sibling's dialects, a context inside a batch: FDW_ESTATE, as for fdw_shot_illum.  Frame stores that do not
 *                   fit on the device: FDW_ENOMEM with the byte counts, before anything is enqueued. */
typedef struct fdw_snaps {
    int every, dec;                      /* K, D */
    float *snaps, *snaps_rec, *snapr;    /* host, [nframes][nxs][nzs]; NULL = not wanted */
} fdw_snaps;
int fdw_snap_dims(int nx, int nz, int nt, int every, int dec, int *nframes, int *nxs, int *nzs);
int fdw_dev_snapshot(fdw_ctx *ctx, const float *d_field, int dec, float *d_frame, void *stream);
int fdw_shot_snaps(fdw_ctx *ctx, const float *v2, int sx, int sz, int gz, const float *srce, const float *d_obs, float *imloc, float *illum,
                   float *P, float *PP, const fdw_snaps *snaps);

/* ---- multi-GPU: communicators and the slab-decomposed loops (csrc/fdw_comm.cpp, csrc/fdw_slabs.cpp) ------------------------
 * The reference has no multi-GPU path.  The grid is decomposed along x, the slow axis, into one band of rows per
 * rank; a rank is one GPU, driven by one process (RCCL backend) or by one host thread of a process (RCCL or local backend).
 *
 * fdw_comm_get_unique_id  ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to the other ranks (a file, an environment
 *                         variable, torch.distributed ...).  librccl.so.1 is opened on first use (dlopen); FDW_ECOMM if it is missing.
 * fdw_comm_init_rank      ncclCommInitRank on `device`: the RCCL backend, one rank per GPU.  Halo blocks travel as ncclSend / ncclRecv
 *                         pairs inside one ncclGroupStart / ncclGroupEnd on the slab driver's communication stream (neighbours only).
 * fdw_comm_init_local     `world` ranks inside ONE process, out[r] for the host thread that drives rank r on devices[r] (NULL: all on
 *                         device 0).  A halo transfer is a device copy on the receiver's stream ordered by events after the sender's
 *                         stream.  Ranks may share a device (tests and rehearsals on a one-GPU box, where RCCL refuses duplicate
 *                         devices) or sit on different GPUs (peer copies over xGMI).  Every rank must be destroyed.
 * fdw_comm_init_stub      rank `rank` of a world whose other ranks do not exist: exchanges move nothing.  TIMING EXPERIMENTS ONLY (what
 *                         one rank of an N-way decomposition costs without its links: scripts/probe_slabs_c.py); results are wrong.
 * fdw_comm_init_shm       one rank per PROCESS without RCCL: halo blocks are staged through the POSIX shared-memory segment `name` ("/..."; rank
 *                         0 creates it, it is unlinked as soon as all ranks hold it), box_bytes = the largest message of one exchange
 *                         (fields x ghost rows x pitch x 4).  A TEST TRANSPORT (ranks may share one GPU, which RCCL refuses): the ranks'
 *                         streams are tied together by nothing but the arrival of a block, as under RCCL.  Collective.
 * fdw_comm_kind           FDW_COMM_RCCL / FDW_COMM_LOCAL / FDW_COMM_SHM, 0 for a stub or NULL
 * fdw_comm_allreduce      one double per rank, summed (op_max = 0) or the maximum (op_max = 1); blocks the host.
 * fdw_comm_selftest       one block sent to the OWN rank through the backend's send / receive path on a stream, and compared.
 *
 * fdw_slabs_create        this rank's share of the decomposition: its band of rows plus order/2 * ksteps ghost rows towards each
 *                         neighbour (ksteps = time steps per halo exchange; 0 = chosen from the band size, the same on every rank), a
 *                         slab context (fdw_create_slab), three streams.  Collective: every rank of `comm` calls it.  comm == NULL: one
 *                         rank holding the whole grid on `device`.
 * fdw_slabs_geometry      x_off = global row of local row 0, nxl = local rows (ghosts included), [own0, own1) = owned global rows,
 *                         nbuf = field buffers fdw_slabs_dev_forward rotates over (4 where it runs four time steps per pass, else 2).
 * fdw_slabs_dev_forward   fd_forward's loop (R:259-267) on caller-owned device arrays [nxl][fdw_pitch(fdw_slabs_ctx())]: buf[*ip], buf[*ipp]
 *                         are the reference's (d_p, d_pp) before its first swap on entry and after the loop on return.  Halo exchanges
 *                         included, overlapped with the interior rows; asynchronous (fdw_slabs_synchronize; fdw_slabs_stream is the
 *                         compute stream, for events).
 *                         STREAMS of fdw_slabs_dev_forward, fdw_slabs_dev_record_forward and fdw_slabs_dev_back (they take no stream argument):
 *                         each rank owns three hipStreamNonBlocking streams -- compute (fdw_slabs_stream), communication and side -- none of
 *                         them ordered against the caller's streams.  Inputs: what fills the buffers must be ordered BEFORE the call on
 *                         fdw_slabs_stream -- an event recorded behind the producer that fdw_slabs_stream waits for
 *                         (hipStreamWaitEvent), or a completed fill; the communication and side streams start every piece of their work
 *                         behind the compute stream, so behind that event too, and neighbouring ranks whose inputs arrive at different times
 *                         are ordered by the communicator's own events.  Outputs: when a call returns, every launch and transfer it issued on
 *                         the communication and side streams has already been joined into the compute stream (the last cycle of a call never
 *                         splits, and every cycle begins by waiting for the exchange before it), so a consumer needs to wait on
 *                         fdw_slabs_stream ALONE -- an event recorded on it after the call -- to read the owned rows, the owned receivers'
 *                         trace rows and the image; calls chain on it without a host synchronisation.  fdw_slabs_synchronize (all three
 *                         streams) is what a caller uses who reads on the host or is about to free the buffers.
 * fdw_slabs_dev_back      fd_back's loop (R:302-339) on caller-owned device arrays: f[role[0]], f[role[1]] = (F_{k-1}, F_{k-2}) -- before iteration 2
 *                         the (P, PP) of the forward pass, P damped (fdw_dev_taper_finalize) --, r[role[2]], r[role[3]] = (r^k, r^{k-1}), zero
 *                         before iteration 0; role[] is updated on return.  f holds nfb buffers and r nrb (fdw_slabs_back_buffers: 6 and 4
 *                         where the slab runs four iterations per pair of pipeline passes, else 2 and 2).  d_samples[nt][nx] with row it =
 *                         d_obs[.][nt-1-it], d_img [nxl][pitch] (owned rows meaningful).
 * fdw_slabs_shot          one shot of rtm_code's loop (R:496-520) on host arrays: every rank passes the GLOBAL v2[nxe][nze], srce[nt],
 *                         d_obs[nx][nt]; imloc[nx][nz] (global; accumulated into) and the optional P, PP [nxe][nze] receive this rank's
 *                         OWNED rows only.  Bit-identical to fdw_shot on the whole grid.
 * fdw_slabs_dev_record_forward
 *                         fdw_slabs_dev_forward (same fields, buffer indices, launches and exchanges) that also writes the trace samples
 *                         of iteration it (fdw_dev_record_steps' definition, receiver column gz) to d_rec + it * nx.  d_rec is THIS RANK'S OWN
 *                         device array [>= it0+nsteps][nx], indexed by the GLOBAL receiver (interior row) number.  On return (after
 *                         fdw_slabs_synchronize) the entries of the rank's OWNED interior rows are defined; entries of its ghost rows may
 *                         hold valid duplicates of a neighbour's samples or what they held before, entries of other rows are untouched:
 *                         neither is to be reported.  Receiver rows the loop never time-steps (compat extents, rows >= xlim) are written
 *                         once per call from the entry fields by the rank that owns them.  gz outside [0, zlim): FDW_EINVAL on every
 *                         rank alike, before anything is enqueued.
 * fdw_slabs_record_shot   fdw_record_shot on the decomposed grid: one shot from rest, every rank passes the GLOBAL v2[nxe][nze] and srce[nt];
 *                         data[nx][nt] (global) and the optional P, PP [nxe][nze] receive this rank's OWNED (interior) rows only, as imloc
 *                         does in fdw_slabs_shot.  Assembled over the ranks the gather is bit-identical to fdw_record_shot on the whole
 *                         grid, in EXACT and FAST numerics.  Refusals (receiver depth, dialect) as fdw_record_shot's, taken by every rank
 *                         alike before anything is enqueued.
 * fdw_slabs_set_stub      on = 1: this rank's halo exchanges move nothing from now on (the cycles keep their launches and stream hand-overs).
 *                         MEASUREMENT ONLY: bench.py times the same window with and without the transfers to report the exposed
 *                         communication fraction; results computed while it is on are wrong.  Every rank must switch together. */
typedef struct fdw_comm fdw_comm;
typedef struct fdw_slabs fdw_slabs;
#define FDW_COMM_ID_BYTES 128
int fdw_comm_get_unique_id(char id[FDW_COMM_ID_BYTES]);
int fdw_comm_init_rank(const char id[FDW_COMM_ID_BYTES], int rank, int world, int device, fdw_comm **out);
int fdw_comm_init_local(int world, const int *devices, fdw_comm **out /* [world] */);
int fdw_comm_init_stub(int rank, int world, int device, fdw_comm **out);
int fdw_comm_init_shm(const char *name, int rank, int world, int device, size_t box_bytes, fdw_comm **out);
enum { FDW_COMM_RCCL = 1, FDW_COMM_LOCAL = 2, FDW_COMM_SHM = 3 };
int fdw_comm_kind(const fdw_comm *comm);
void fdw_comm_destroy(fdw_comm *comm);
int fdw_comm_rank(const fdw_comm *comm);
int fdw_comm_world(const fdw_comm *comm);
int fdw_comm_device(const fdw_comm *comm);
int fdw_comm_is_local(const fdw_comm *comm);
int fdw_comm_allreduce(fdw_comm *comm, double *value, int op_max);
int fdw_comm_barrier(fdw_comm *comm);
int fdw_comm_selftest(fdw_comm *comm);
int fdw_slabs_create(const fdw_params *prm, fdw_comm *comm, int device, int ksteps, fdw_slabs **out);
void fdw_slabs_destroy(fdw_slabs *s);
fdw_ctx *fdw_slabs_ctx(fdw_slabs *s);
int fdw_slabs_geometry(const fdw_slabs *s, int *x_off, int *nxl, int *own0, int *own1, int *ksteps, int *nbuf);
void *fdw_slabs_stream(fdw_slabs *s);
int fdw_slabs_synchronize(fdw_slabs *s);
int fdw_slabs_dev_forward(fdw_slabs *s, float *const *buf, const float *d_v2, const float *d_srce, int sx, int sz, int it0, int nsteps,
                          int first_pp_twice, int *ip, int *ipp);
int fdw_slabs_dev_record_forward(fdw_slabs *s, float *const *buf, const float *d_v2, const float *d_srce, int sx, int sz, int gz, float *d_rec,
                                 int it0, int nsteps, int first_pp_twice, int *ip, int *ipp);
int fdw_slabs_record_shot(fdw_slabs *s, const float *v2, int sx, int sz, int gz, const float *srce, float *data, float *P, float *PP);
int fdw_slabs_back_buffers(const fdw_slabs *s, int *nfb, int *nrb);
int fdw_slabs_dev_back(fdw_slabs *s, float *const *f, float *const *r, const float *d_v2, const float *d_samples, int gz, float *d_img, int it0,
                       int nsteps, int role[4]);
int fdw_slabs_shot(fdw_slabs *s, const float *v2, int sx, int sz, int gz, const float *srce, const float *d_obs, float *imloc, float *P, float *PP);
int fdw_slabs_set_stub(fdw_slabs *s, int on);

/* ---- line sources in the forward loop: plane-wave and encoded-shot migration -------------------------
 * The RTM dialect on full-grid contexts, EXACT and FAST numerics alike.  Slab contexts, the sibling's dialects and a context inside a
 * batch of shots return FDW_ESTATE.
 *
 * Line source.  nsrc = min(nx, xlim - nxb): the interior rows the loop time-steps (fdw_get_extents).  Iteration it of fd_forward's loop
 * (R:259-267) runs unchanged except that kernel_src (R:267) is replaced: for ix = 0 .. nsrc-1, d_pp[nxb+ix][sz] = d_pp[nxb+ix][sz] (+) w[it][ix],
 * one fp32 add per row applied after the leap-frog, exactly as kernel_sism (R:124-131) adds its samples.  Samples of rows ix >= nsrc are
 * ignored: the line ends before the rows the reference never time-steps (a point source there is refused, a full-width line is not).
 * sz outside [0, zlim): FDW_EINVAL before anything is enqueued.  Recording, illumination, P / PP and the backward loop keep their
 * definitions: the recorded and the squared value is the stored new field, line samples included; the backward loop is fd_back as it
 * stands and reconstructs the source field from (P, PP) without a source (R:317-318), as it does for a point source.  fdw_dev_line_steps takes
 * at most one of d_rec and d_illum (both non-NULL is FDW_EINVAL); both together go through fdw_dev_line_record_illum_steps.
 *
 * fdw_dev_line_steps    fdw_dev_steps2 / fdw_dev_record_steps / fdw_dev_illum_steps driven by the line: d_wav [>= it0+nsteps][nx] on the
 *                       device (row it = the samples of iteration it), d_rec (NULL ok) the trace rows [it][nx] at gz, d_illum (NULL ok) the
 *                       accumulator [nxl][pitch].  The same kernel family per pass, buffer rotation and static-row recording.
 * fdw_shot_line         fdw_shot (v2 == NULL: fdw_shot_resident) whose forward loop is driven by wav[nx][nt] (the gather layout: wav[ix][it])
 *                       at depth sz; illum (NULL ok) as fdw_shot_illum.
 * fdw_record_shot_line  fdw_record_shot driven by wav[nx][nt].
 * fdw_debug_step4_plan_line  fdw_debug_step4_plan for a four-step pass of fdw_dev_line_steps (plain) with the line at depth sz.
 *
 * Encoding.  All arithmetic fp32, round to nearest, nothing fused; sums run in ascending shot order from +0.0f.
 * fdw_planewave_lags      in double, l_s = lround(p * (src_ix[s] - src_ix[0]) * dx / dt); lag[s] = l_s - min l_s >= 0.  p: ray parameter, s/m.
 * fdw_encode_line_source  wav[nx][nt] starts at zero; for s ascending and it >= lag[s]: wav[src_ix[s]][it] (+)= weight[s] (*) srce[it - lag[s]].
 *                         A src_ix outside [0, nx) or a negative lag: FDW_EINVAL.  Pure host C.
 * fdw_encode_gathers      out[ix][it] = the fold, over the s with 0 <= it - lag[s] < nt, of acc (+) weight[s] (*) d_obs_all[s][ix][it - lag[s]];
 *                         runs on `device` (fdw_encode_gathers_kernel). */
int fdw_dev_line_steps(fdw_ctx *ctx, float *const *d_buf /* [4] */, const float *d_v2, const float *d_wav, int sz, int gz, float *d_rec,
                       float *d_illum, int it0, int nsteps, int first_pp_twice, int *ip, int *ipp, void *stream);
int fdw_shot_line(fdw_ctx *ctx, const float *v2, int sz, int gz, const float *wav, const float *d_obs, float *imloc, float *illum, float *P,
                  float *PP);
int fdw_record_shot_line(fdw_ctx *ctx, const float *v2, int sz, int gz, const float *wav, float *data, float *P, float *PP);
int fdw_debug_step4_plan_line(fdw_ctx *ctx, int sz, int r0, int r1, int r0b, int r1b, int xchunk, int *nblk, int *nstrip, unsigned char *cls,
                              int cls_cap);
int fdw_planewave_lags(int nshots, const int *src_ix, float dx, float dt, double p, int *lag);
int fdw_encode_line_source(int nshots, const int *src_ix, const int *lag, const float *weight, const float *srce, int nt, int nx, float *wav);
int fdw_encode_gathers(int device, int nshots, const int *lag, const float *weight, const float *d_obs_all, int nx, int nt, float *out);

/* ---- line sources: recording with illumination, residual migration, batches, one-pass encoding -----
 * Same contexts and refusals as above (FDW_ESTATE elsewhere; sz, and gz where traces are recorded, outside [0, zlim): FDW_EINVAL before
 * anything is enqueued).  Every result is defined by single calls of the entry points above and equals them bit for bit.
 *
 * fdw_dev_line_record_illum_steps  fdw_dev_line_steps that writes the trace rows AND accumulates, every pass one launch of its family's
 *                                  combined line-source kernel (orders above 8 and the forced generic kernel: the generic recording step, then
 *                                  the accumulation).  d_rec or d_illum NULL: FDW_EINVAL.  Fields, trace rows and accumulator equal two runs
 *                                  of fdw_dev_line_steps, one with d_rec, one with d_illum.
 * fdw_shot_line_residual           fdw_shot_line that migrates resid = d_obs (-) d_mod (one fp32 subtraction per sample, fdw_dev_gather_residual),
 *                                  d_mod the gather its own forward loop records: fdw_record_shot_line's for the same context, model, wav, sz,
 *                                  gz.  imloc is fdw_shot_line's handed resid as d_obs; illum, P, PP are fdw_shot_line's.  resid (NULL ok)
 *                                  [nx][nt].  Data modelled by fdw_record_shot_line in the migration model: resid is all-zero words and imloc
 *                                  keeps its entry values.
 * fdw_shot_line_batch              `nshots` calls of fdw_shot_line, shot b with wav_all[b], d_obs[b] (both [nshots][nx][nt]), imloc[b] and
 *                                  illum[b] (NULL ok; [nshots][nx][nz]) and the model v2_all[b], or with v2_all == NULL the border model of
 *                                  draws draw_offset + b T on the resident interior model (T = fdw_border_draws), as fdw_shot_batch takes them.
 *                                  Where fdw_shot_batch batches, the whole batch advances through one launch per time step (one more batch
 *                                  buffer, [nshots][nt][nx], holds the line gathers); otherwise, and on a device without room for the
 *                                  buffers, the shots run one by one.  Batches larger than the budget of fdw_shot_batch_max allows with these
 *                                  buffers counted go through in parts.  The bytes are the same in every case.
 * fdw_shot_line_batch_residual     the same for fdw_shot_line_residual; resid (NULL ok) [nshots][nx][nt].
 * fdw_record_shot_line_batch       the same for fdw_record_shot_line; data [nshots][nx][nt].
 * fdw_encode_gathers_multi         `nplanes` calls of fdw_encode_gathers on one data set: lag, weight [nplanes][nshots], out [nplanes][nx][nt].
 *                                  One upload of d_obs_all, one launch (fdw_encode_gathers_multi_kernel), one download.  nplanes outside
 *                                  [1, 65535], a negative lag or a NULL argument: FDW_EINVAL before a device is opened. */
int fdw_dev_line_record_illum_steps(fdw_ctx *ctx, float *const *d_buf /* [4] */, const float *d_v2, const float *d_wav, int sz, int gz, float *d_rec,
                                    float *d_illum, int it0, int nsteps, int first_pp_twice, int *ip, int *ipp, void *stream);
int fdw_shot_line_residual(fdw_ctx *ctx, const float *v2, int sz, int gz, const float *wav, const float *d_obs, float *imloc, float *illum,
                           float *resid, float *P, float *PP);
int fdw_shot_line_batch(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sz, int gz, const float *wav_all,
                        const float *d_obs, float *imloc, float *illum);
int fdw_shot_line_batch_residual(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sz, int gz, const float *wav_all,
                                 const float *d_obs, float *imloc, float *illum, float *resid);
int fdw_record_shot_line_batch(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sz, int gz, const float *wav_all,
                               float *data);
int fdw_encode_gathers_multi(int device, int nshots, int nplanes, const int *lag, const float *weight, const float *d_obs_all, int nx, int nt,
                             float *out);

/* ---- excitation-amplitude imaging: a receiver-only backward loop ---------------------------------------------------------------
 * The other standard RTM imaging condition.  The forward loop remembers, per cell, the peak of the source field and the time level at which
 * it occurred (the excitation time); the backward loop propagates the receiver field ALONE, and every cell takes one sample of it, at its
 * excitation time, divided by the peak.  No source field is reconstructed, no product is accumulated, and the image is source-normalised as
 * it comes.  The RTM dialect on full-grid contexts, EXACT and FAST numerics alike (FAST changes the Laplacian only).  Slab contexts, the
 * sibling's dialects and (but for fdw_shot_excitation_batch itself) a context inside a batch: FDW_ESTATE.  A NULL required pointer, it0 < 0, a depth outside [0, zlim) (as for line
 * sources), a source row the loop never time-steps: FDW_EINVAL.  Every refusal happens before anything is enqueued.
 *
 * Excitation maps.  Two field-shaped device arrays [nxl][pitch], d_amp (float) and d_texc (int32).  Over every extended-grid cell with
 * x < xlim, z < zlim (fdw_get_extents), for it = it0 .. it0+nsteps-1 in ascending order, with u the value stored as the new field at the end
 * of iteration it -- after kernel_src, raw and undamped, the level recording, illumination and snapshots sample:
 *         if (fabsf(u) > fabsf(amp)) { amp = u; texc = it + 1; }
 * The compare is strict (the first of equal peaks wins), a NaN u never wins and a NaN already in amp stays, +-0 never replaces anything, an
 * infinity wins once, amp keeps the SIGNED winner.  Both arrays are read-modify-write and start from what the caller put there (a fresh shot:
 * all-zero words).  Cells outside the extents and the padding columns keep their words.  No arithmetic is involved: the maps are exact.
 *
 * Excitation pick.  The line-source loop of fdw_dev_line_steps (d_wav [>= it0+nsteps][nx], row it = the samples of iteration it at depth sz,
 * rows >= nsrc ignored, same damping, same static rows) with one epilogue: after the injection of iteration it, over the same cells,
 *         if (texc == top - it) exc = r;        r: the stored new field, injected sample included, raw
 * d_texc is only read.  d_exc (float [nxl][pitch]) changes only where a pick happens; every other word keeps its entry value, padding columns
 * and cells outside the extents included.  The test is int32 equality: a cell whose texc is not in (top - it0 - nsteps, top - it0] is never
 * picked.
 *
 * fdw_dev_excite_steps      fdw_dev_steps2's loop with the maps.  The same buffers, indices and fields, bit for bit; everything on the
 *                           caller's stream, nothing synchronised, no pass bands.  d_srce NULL or sx < 0: no source.
 * fdw_dev_line_pick_steps   fdw_dev_line_steps' plain loop with the pick; the same contract.
 *   Kernels: the one-step register-ring family (orders 2-8, prefetch 1 / 2 / 3) and the four-step wave pipeline have fused kernels for both,
 *   EXACT and FAST; orders above 8 and the forced generic kernel run the generic step followed by a small compare-and-select / pick
 *   kernel.  In the pipeline the amp (exc) row rides the 16-slot LDS FIFO as the illumination accumulator does, with a dword of 4-bit
 *   tags per lane and row beside it that says which level of the pass won (picks) each cell: 52 KiB of LDS, three workgroups per CU.  The
 *   two-step family has NO excitation kernel: on a context whose plain loop runs pairs, a pair becomes two single steps that land in the
 *   buffers the pair would have used (each on a copy of the field it overwrites), so fields, indices and static rows still equal the
 *   plain loop's.  Traffic: +16 B/point per forward pass (amp and texc, in and out), +12 B/point per pick pass (texc and exc in, exc out).
 *   Measured on one MI355X at 8192^2, order 8 (profiles/excitation.json): the forward loop with the maps 142.5 us
 *   per step against 96.6 plain and 123.1 with illumination (FAST 135.8 / 86.8 / 115.4); the line loop with the pick 129.8 against 97.0
 *   (FAST 123.8 / 86.6): the two device loops are 0.85 of fdw_shot's.  A whole fdw_shot_excitation of 500 steps with imloc alone takes
 *   177.8 ms against fdw_shot's 185.6 ms (FAST 173.7 / 169.0; DESIGN.md section 6r, profiles/excitation.json key image_on_device): level with
 *   the cross-correlation shot since the image is formed on the device and ONE array comes back, where it took 255.4 ms (FAST 252.0) with
 *   three downloads and the image formed on the host; a caller that asks for exc, amp and texc still pays for those downloads (251.9 ms).
 *   On a 415 x 295 deck (nt 1700) the shot takes 19.5 ms against fdw_shot's 19.3 (FAST 19.6 / 18.8).
 * fdw_shot_excitation       One shot from rest: the forward loop of fdw_shot for nt steps with the maps; the receiver fields zeroed; nt
 *                           iterations of the pick loop with top = nt, row k of the line gather = d_obs[.][nt-1-k], at depth gz.  Iteration
 *                           k meets the cells whose excitation level is nt - k: sample j pairs with level u^{j+1}, as in the recording
 *                           section.  Receiver rows the loop never time-steps (ix >= nsrc) are NOT injected -- the line-source rule, which
 *                           differs from fd_back on ragged compat grids.  v2 NULL: the resident model.  P / PP: fdw_shot's.  exc, amp,
 *                           texc: the interiors [nx][nz]; imloc is updated as fdw_image_excitation would, bit for bit, but on the device
 *                           (fdw_dev_image_excitation on the context's image accumulator) and comes back as ONE array; exc, amp and texc
 *                           are downloaded only where asked for.  Each of the four may be NULL, all four NULL is FDW_EINVAL.  The line
 *                           gather is reversed in time on the device.  The work arrays are allocated on first use.
 * fdw_image_excitation      Pure host C, no device.  m = max_i fabsf(amp[i]) taken from 0.0f with > (a NaN never wins); s = eps * m; for each
 *                           i with fabsf(amp[i]) > s: img[i] = img[i] + exc[i] / amp[i], one fp32 division and one fp32 add.  Every other
 *                           img[i] is left untouched (no + 0.0f: -0.0 survives).  eps not finite or < 0: FDW_EINVAL.  Shots stack by calling
 *                           it per shot into one img.
 * fdw_dev_image_excitation  fdw_image_excitation on device arrays.  d_exc, d_amp, d_img: field-shaped [nxl][pitch].  On the interior cells (rows
 *                           nxb .. nxb+nx-1, columns nzb .. nzb+nz-1) the result is fdw_image_excitation's on the interiors, bit for bit:
 *                           m = max |amp| over the INTERIOR only, from 0.0f with > (a NaN never wins; border cells and padding columns do not
 *                           count, although the maps are written over the whole update extents), s = eps * m (one fp32 product), where
 *                           fabsf(amp) > s: img = img + exc / amp.  The quotient is formed in double and rounded once, which for fp32
 *                           operands is the correctly rounded fp32 quotient (fp64 has 53 >= 2 * 24 + 2 significand bits).  Every other word
 *                           of d_img keeps its bits: unselected interior cells (-0.0 stays -0.0), the border, the padding.  d_exc and d_amp
 *                           are only read.  Two launches behind a memset of one word: the peak as an unsigned maximum of the words |amp|
 *                           (order-independent, so deterministic), then the update.  stream == NULL: the context's stream; everything goes
 *                           on the given stream, nothing is synchronised, nothing is allocated.  The context holds ONE peak word: calls on
 *                           different streams must not overlap.  eps not finite or < 0, a NULL pointer: FDW_EINVAL; a slab context,
 *                           another dialect, a context inside a batch: FDW_ESTATE -- before anything is enqueued.
 * fdw_shot_excitation_batch `nshots` excitation shots stacked into one image.  Shot b: source row sx0 + b dsx, gather d_obs + b nx nt, model
 *                           v2_all + b nxe nze or (v2_all == NULL) the border model of draws [draw_offset + b T, ...) on the resident model --
 *                           what fdw_shot_batch takes.  imloc [nx][nz]: the running image, in and out.  stack (may be NULL) [nshots][nx][nz]:
 *                           the running image after each shot.  exc, amp, texc (each may be NULL) [nshots][nx][nz]: the per-shot interiors.
 *                           Every output equals, bit for bit, the sequence for b = 0 .. nshots-1: fdw_shot_excitation of shot b, then
 *                           fdw_image_excitation into the one running image.  On the RTM dialect's full-grid contexts of order <= 8 in the
 *                           one-step regime (neither the pipeline nor the two-step family pays; no forced generic kernel) the forward loop
 *                           with the maps and the line loop with the pick are ONE launch per time step for all shots, followed by the peak
 *                           and the update kernel over all shots in shot order; elsewhere, and where the device has no room, the shots run
 *                           one by one through fdw_shot_excitation's own code.  Ragged compat grids batch too: the pick loop injects only
 *                           the receiver rows the loop time-steps, in a batch as alone.  fdw_batch_parts reports as for the other batched
 *                           calls (0 one by one, 1 the whole batch, k parts).  Memory: the call works in fdw_shot_batch's buffers, so per
 *                           shot it holds that call's ELEVEN fields (it uses eight: two source fields, two receiver fields, v2, amp, texc and
 *                           exc, the last of which then takes the running images) and ONE gather [nt][nx]; a batch over the batch budget
 *                           (fdw_set_batch_budget) is cut by the call itself into parts of budget / (11 fields + 1 gather) shots, run in
 *                           shot order with the running image carried from part to part; under a budget below ONE shot's share the call
 *                           takes no batch buffers and runs the shots one by one (fdw_batch_parts 0).  A NULL required pointer (srce, d_obs, imloc),
 *                           nshots < 1, a source row outside the time-stepped rows, a depth outside [0, zlim), a bad eps: FDW_EINVAL; no
 *                           model, a slab context, another dialect: FDW_ESTATE -- before anything is enqueued.
 *   Measured on one MI355X (profiles/excitation_batch.json), 415 x 295 interior, nt 1700, 32 shots: 4.67 ms per shot
 *   against 18.98 ms one by one (FAST 4.81 / 18.92), beside fdw_shot_batch's 3.99 ms (FAST 3.87).
 * Out of scope: slabs, maps under a line source, a combined recording + maps kernel, a two-step excitation kernel, batches in the pipeline
 * and generic-order families. */
int fdw_dev_excite_steps(fdw_ctx *ctx, float *const *d_buf /* [4] */, const float *d_v2, const float *d_srce, int sx, int sz, float *d_amp,
                         int *d_texc, int it0, int nsteps, int first_pp_twice, int *ip, int *ipp, void *stream);
int fdw_dev_line_pick_steps(fdw_ctx *ctx, float *const *d_buf /* [4] */, const float *d_v2, const float *d_wav, int sz, const int *d_texc, int top,
                            float *d_exc, int it0, int nsteps, int first_pp_twice, int *ip, int *ipp, void *stream);
int fdw_shot_excitation(fdw_ctx *ctx, const float *v2 /* NULL: the resident model */, int sx, int sz, int gz, const float *srce, const float *d_obs,
                        float eps, float *imloc, float *exc, float *amp, int *texc, float *P, float *PP);
int fdw_image_excitation(const float *exc, const float *amp, size_t n, float eps, float *img);
int fdw_dev_image_excitation(fdw_ctx *ctx, const float *d_exc, const float *d_amp, float eps, float *d_img, void *stream);
int fdw_shot_excitation_batch(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                              const float *srce, const float *d_obs, float eps, float *imloc, float *stack, float *exc, float *amp, int *texc);

/* ---- Born modelling: scattered-field gathers from a reflectivity model -------------------------------------------------------------
 * The other direction of migration: a reflectivity model goes back to data (demigration), the second half of least-squares migration and
 * of any linearised inversion.  The RTM dialect on full-grid contexts, EXACT and FAST numerics alike (FAST changes the Laplacian only).
 *
 * Two field pairs, the background pair (u_p, u_pp) and the scattered pair (du_p, du_pp), caller-owned, [nxl][pitch], each rotated as
 * fdw_dev_steps rotates its two buffers (swap first, then the new field is written over pp).  One squared-velocity model d_v2 and one
 * reflectivity d_m, field-shaped [nxl][pitch], of which only the words on the cell set C below are ever used: its border and padding words
 * influence no output.  Iteration it = it0 .. it0+nsteps-1 runs, in this order:
 *   1. Background step: iteration it of fd_forward's loop (R:259-267) as fdw_dev_steps runs it -- swap, taper, Laplacian, leap-frog,
 *      kernel_src with srce[it] at (sx, sz).  U: the stored new field, raw, source sample included (the level recording, illumination,
 *      snapshots and the excitation maps sample).  A, B: the words the two background buffers held on entry to the iteration (levels it, it-1).
 *   2. Scattered step: the same iteration without a source on (du_p, du_pp), same d_v2, taper and extents.  D: its stored new field.
 *   3. Scatter, on C = { (x, z) : nxb <= x < min(nxb+nx, xlim), nzb <= z < min(nzb+nz, zlim) } (fdw_get_extents):
 *          D = D (+) ( m (*) q )        product and sum rounded separately in fp32, round to nearest, nothing fused, in both numerics
 *        kind FDW_BORN_FIELD (0): q = U.  The transpose of the cross-correlation imaging condition as this library pairs levels (sample j
 *                                 meets u^{j+1}).
 *        kind FDW_BORN_DTT (1):   q = (U (-) A) (-) (A (-) B), three fp32 subtractions: the second time difference, the linearisation of
 *                                 the modelling in v2 -> v2 (1 + m).
 *      No cell of C is ever damped (z >= nzb >= ztap), so A and B are the raw words.  Cells outside C receive nothing (no + 0.0f: -0.0
 *      survives).
 *   4. Record: d_rec[it][ix] = D[nxb+ix][gz] for ix < nx (after the scatter); rows >= xlim, which no loop time-steps, follow the rule of
 *      fdw_dev_record_steps applied to the scattered pair.  d_rec0[it][ix] = U[nxb+ix][gz]: fdw_dev_record_steps' gather of the
 *      background, bit for bit.  Either pointer may be NULL.
 * Consequences: the background pair equals fdw_dev_steps on it bit for bit; m all zero words, from rest, gives du and d_rec all zero words;
 * d_rec0 equals fdw_record_shot.
 *
 * fdw_dev_born_steps  the loop above on device arrays.  Everything goes on the given stream (NULL: the context's), nothing is synchronised.
 *                     first_pp_twice applies to both pairs; after an odd or even nsteps the newest fields sit where fdw_dev_steps leaves
 *                     them.  FDW_EINVAL before anything is enqueued: gz or sz outside [0, zlim), a source row outside the time-stepped
 *                     rows [0, xlim), a NULL required pointer (the four fields, d_v2, d_m, d_srce), it0 < 0, nsteps < 0, kind outside
 *                     {0, 1}.  FDW_ESTATE: slab contexts, the sibling's dialects, a context inside a batch.
 *   Kernels: the one-step register-ring family (orders 2-8, prefetch 1 / 2 / 3 at order 8, EXACT and FAST) has a fused kernel,
 *   fdw_step_born_kernel: the scattered field rides a second register ring, v2 is read once for both fields, the m row is streamed, and the
 *   scatter and the trace samples happen in registers before the two stores: 36 B/point/step (six reads, two writes) against 32 for two
 *   plain steps.  Orders above 8 and the forced generic kernel (and FDW_NO_BORN_FUSED=1 in the environment at fdw_create, for benchmarks and
 *   tests) run the existing step on each pair and a small scatter kernel behind them; for FDW_BORN_DTT that arrangement keeps (A - B) in a
 *   context-owned scratch field, allocated by the first call that needs it (the one allocation this entry point can make).  There is no Born
 *   kernel in the two-step and four-step families: contexts whose plain loop runs them run Born with one-step launches, as fdw_dev_steps does.
 *   Measured on one MI355X (profiles/born.json; order 8, FDW_BORN_DTT, us per step): 8192^2 fused 413.2, unfused 880.9,
 *   two plain one-step loops on the parent's build 372.2 (ratio 1.110; FAST 426.7 / 887.0 / 370.3, 1.152); 2048^2 35.0 / 61.2 / 29.9 (1.170;
 *   FAST 31.7 / 60.7 / 29.6, 1.072).  Order 8, prefetch 2: 208 VGPRs, two waves per SIMD, no scratch.
 * fdw_born_shot       one shot from rest for the context's nt: m [nx][nz] is embedded into a zeroed field, the gathers are recorded on the
 *                     device and downloaded transposed to [nx][nt] as fdw_record_shot does (data: scattered; data0, may be NULL: background).
 *                     v2 NULL: the resident model (FDW_ESTATE without one).  Work arrays are allocated on first use, freed by fdw_destroy.
 * Out of scope: Born kernels in the two-step and four-step families, slabs and several GPUs (the DTT-adjoint imaging condition: "DTT
 * imaging" below; the solver that iterates on the two: "Least-squares migration"). */
enum { FDW_BORN_FIELD = 0, FDW_BORN_DTT = 1 };
int fdw_dev_born_steps(fdw_ctx *ctx, float *d_u_p, float *d_u_pp, float *d_du_p, float *d_du_pp, const float *d_v2, const float *d_m, int kind,
                       const float *d_srce, int sx, int sz, int gz, float *d_rec, float *d_rec0, int it0, int nsteps, int first_pp_twice, void *stream);
int fdw_born_shot(fdw_ctx *ctx, const float *v2 /* NULL: the resident model */, const float *m /* [nx][nz] */, int kind, int sx, int sz, int gz,
                  const float *srce, float *data /* [nx][nt] scattered */, float *data0 /* NULL ok: [nx][nt] background */);

/* ---- Born modelling driven by a line source, and batches of Born shots -------------------------------------------------------------------
 * The two further forms every migration path here has: a line source (the forward operator of plane-wave and encoded-shot least-squares
 * migration, whose gradient is fdw_shot_line_residual) and batches of small shots through one launch per time step.  Same dialect, contexts
 * and numerics as above; C, the kinds and the rounding as defined above.
 *
 * Line source.  Iteration it of fdw_dev_born_steps with step 1 replaced by the line-source iteration of fdw_dev_line_steps: after the
 * leap-frog, for ix < nsrc = min(nx, xlim - nxb): U[nxb+ix][sz] = U[nxb+ix][sz] (+) w[it][ix] (d_wav [>= it0+nsteps][nx]; samples of rows
 * ix >= nsrc are ignored).  Steps 2-4 are unchanged: the scattered pair takes no injection.  U, line samples included, is what q and d_rec0
 * see; A and B are the entry words of the background buffers.
 * Consequences: the background pair and d_rec0 equal fdw_dev_line_steps with d_rec, bit for bit; fdw_born_shot_line's data0 equals
 * fdw_record_shot_line; an all-zero m from rest gives all-zero words.
 * fdw_dev_born_line_steps  the loop on device arrays, on the given stream (NULL: the context's), nothing synchronised.  FDW_EINVAL before
 *                     anything is enqueued: sz or gz outside [0, zlim), a NULL required pointer (the four fields, d_v2, d_m, d_wav), it0 < 0,
 *                     nsteps < 0, kind outside {0, 1}.  FDW_ESTATE: slab contexts, the sibling's dialects, a context inside a batch.
 *   Kernels: fdw_step_line_born_kernel, the fused kernel above with the line injection of fdw_step_line_kernel (one sample load per row
 *   more), instantiated wherever fdw_step_born_kernel is; no scratch (DESIGN.md section 6u has the registers).  Orders above 8, the forced
 *   generic kernel and FDW_NO_BORN_FUSED=1 run the existing steps with the line source on the background pair and the scatter kernel.
 * fdw_born_shot_line  fdw_born_shot with the gather wav [nx][nt] (uploaded and transposed as fdw_record_shot_line does) in place of the
 *                     wavelet and its source row.
 *
 * Batches.  Shot b of fdw_born_shot_batch is fdw_born_shot with source row sx0 + b dsx, shot b of fdw_born_shot_line_batch is
 * fdw_born_shot_line with wav_all[b]; the model is v2_all[b] or, with v2_all == NULL, the border model of draws draw_offset + b T on the
 * resident model: shots and models as fdw_shot_batch takes them.  ONE reflectivity m [nx][nz] for all shots.  data (and data0, may be NULL)
 * [nshots][nx][nt].  Every output equals the single-shot calls bit for bit; data0 equals fdw_record_shot_batch / fdw_record_shot_line_batch.
 * Where fdw_record_shot_batch batches and the fused Born kernel runs, the whole batch is one launch per time step (gridDim.y = nshots);
 * elsewhere (orders above 8, forced generic, FDW_NO_BORN_FUSED=1, static receiver rows, the two-step and pipeline regimes), and without
 * room on the device, the shots run one by one through the single-shot code and produce the same bytes.
 * Who splits.  Both calls work in fdw_shot_batch's batch buffers (of its eleven fields per shot they use two pairs and v2; its gather buffer
 * takes the scattered traces), plus a background-gather buffer of their own when data0 is asked for, plus the line gathers of a line batch;
 * one device copy of m.  The per-shot share is therefore 11 fields + (1 + [data0 != NULL] + [line]) gathers [nt][nx], and a batch over the
 * budget (fdw_set_batch_budget) is cut into parts of what that share allows by the call itself: the shots are independent, nothing is
 * carried between parts.  Under a budget below one shot's share the shots run one by one.  fdw_batch_parts: 0 / 1 / k as for the other
 * batched calls.
 * Refusals, before anything is enqueued: those of fdw_born_shot (for the line form: of fdw_born_shot_line) plus nshots < 1 and source rows
 * outside the time-stepped rows (FDW_EINVAL); no model -- v2_all == NULL without fdw_model_resident -- is FDW_ESTATE.
 * Measured on one MI355X (profiles/born_batch.json; 415 x 295 interior, nt 1700, order 8, FDW_BORN_DTT, 32 shots, ms
 * per shot): fdw_born_shot_batch 2.857 against fdw_born_shot one by one on the parent's build 12.477 (4.37 x; FAST 2.667 / 11.426, 4.28 x);
 * the yardstick in the same run, fdw_record_shot_batch 1.410 against fdw_record_shot one by one 8.405 (5.96 x; FAST 1.345 / 8.358, 6.21 x).
 * The line loop against the parent's point-source loop, us per step: 8192^2 418.70 / 418.21 (windows spread 2.07), 2048^2 33.71 / 34.51
 * (spread 0.26). */
int fdw_dev_born_line_steps(fdw_ctx *ctx, float *d_u_p, float *d_u_pp, float *d_du_p, float *d_du_pp, const float *d_v2, const float *d_m, int kind,
                            const float *d_wav /* [>= it0+nsteps][nx] */, int sz, int gz, float *d_rec, float *d_rec0, int it0, int nsteps,
                            int first_pp_twice, void *stream);
int fdw_born_shot_line(fdw_ctx *ctx, const float *v2 /* NULL: resident */, const float *m, int kind, int sz, int gz, const float *wav /* [nx][nt] */,
                       float *data, float *data0 /* NULL ok */);
int fdw_born_shot_batch(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, const float *m /* [nx][nz], ONE for all shots */,
                        int kind, int sx0, int dsx, int sz, int gz, const float *srce, float *data /* [nshots][nx][nt] */, float *data0 /* NULL ok */);
int fdw_born_shot_line_batch(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, const float *m, int kind, int sz, int gz,
                             const float *wav_all /* [nshots][nx][nt] */, float *data, float *data0);

/* ---- DTT imaging: the second-time-difference imaging condition, the adjoint of FDW_BORN_DTT --------------------------------------------
 * fdw_shot and every form built on it image with the cross-correlation img += F_k (*) r^{k+1}: the transpose of FDW_BORN_FIELD.  This is the
 * matching transpose of FDW_BORN_DTT, the piece a linearised inversion loop (Born, residual, gradient) needs for the gradient of its own
 * misfit.  The RTM dialect on full-grid contexts, EXACT and FAST numerics alike (FAST changes the Laplacian only).
 *
 * C is the cell set of the Born section.  F_k is the source field iteration k of fd_back images and r^{k+1} the receiver field that
 * iteration stores, raw, injected sample included, both as fdw_dev_back_iter defines them today.  For k = 0 .. nsteps-1
 *          q_k = (F_k (-) F_{k+1}) (-) (F_{k+1} (-) F_{k+2})        three fp32 subtractions, round to nearest, nothing fused
 * -- the Born section's q with U = F_k, A = F_{k+1}, B = F_{k+2}: the levels u^{j+1}, u^j, u^{j-1} FDW_BORN_DTT used at forward iteration
 * j = nt-1-k -- and on C, for k ascending,
 *          img = img (+) ( q_k (*) r^{k+1} )                        product and sum rounded separately
 * Every other word of d_img keeps its bits: border, padding columns, cells outside the extents, and the border cells inside the launch
 * extents that the cross-correlation epilogue does touch.  No cell of C is ever damped: every operand is the raw word the buffers hold.
 *
 * The lag.  q_k needs F_{k+1} and F_{k+2}, which the backward loop reconstructs one and two iterations later, so the loop runs two behind:
 *   iterations 0, 1   the source fields are the two snapshots; the receiver step and its injection exactly as
 *                     fdw_dev_back_iter(step_source = 0) runs them; d_img is not touched.
 *   iteration i >= 2  fdw_dev_back_iter(step_source = 1) with the term k = i-2, q_{i-2} (*) r^{i-1}, in place of the cross-correlation:
 *                     F_{i-2} = the entry words of d_f0, F_{i-1} = d_f1, F_i = the new source field, r^{i-1} = the entry words of d_ppr.
 *   tail              after the last iteration two source-only reconstructions F_nsteps, F_{nsteps+1} (the plain leap-frog of R:317-318,
 *                     mode 1, no receiver step) supply the terms k = nsteps-2 and k = nsteps-1, paired with r^{nsteps-1} and r^{nsteps},
 *                     added in that order.  nsteps < 2: the same rule with fewer terms.
 * Consequences: the source pair and the receiver pair (static receiver rows of ragged compat grids included) equal fdw_dev_back_iter's bit
 * for bit, only the image differs; an all-zero gather leaves every word of the image as it came.
 *
 * Exact adjointness.  The backward loop steps with T = 2 + V K (V = diag(v2 dt2), K the Laplacian), which is not the transpose of the
 * forward T, but V^-1 T V = T^T.  Hence
 *          < Born_DTT(m), w > = < m, (1/v2) (.) Image_DTT( v2_rec (.) w ) >,    v2_rec[ix] = v2[nxb+ix][gz], 1/v2 per image cell,
 * up to fp32 rounding, provided that no field reaches a damped column, that the source is silent on the levels the image uses (fd_back
 * reconstructs without a source: the reference's convention, kept) and that m vanishes where the reconstruction is therefore wrong.  With a
 * constant v2 the two weights cancel.  The two weights, one fp32 operation per word, pure host code (no device), out may be the input:
 *   fdw_gather_scale_v2    out[ix][it] = g[ix][it] (*) v2[nxb+ix][gz]
 *   fdw_image_unscale_v2   out[ix][iz] = img[ix][iz] (/) v2[nxb+ix][nzb+iz]
 *
 * fdw_dev_back_iter_dtt  one iteration as defined above on caller-owned device arrays, rows [r0, r1) = [0, nxl) (the whole grid; anything
 *                     else is FDW_EINVAL).  step_source = 0: iterations 0 and 1 (d_f0 may be NULL, d_img is not touched).  Everything goes
 *                     on the given stream (NULL: the context's), nothing is synchronised.  FDW_EINVAL before anything is enqueued: a NULL
 *                     buffer, aliased arrays, gz outside the grid.  FDW_ESTATE: slab contexts, the sibling's dialects, a context inside a batch.
 * fdw_dev_dtt_image   one term on C: d_img = d_img (+) ((d_fa (-) d_fb) (-) (d_fb (-) d_fc)) (*) d_r.  A device caller's tail is
 *                     fdw_dev_step(mode 1) into a copy of the older level, then this.  Same stream contract and refusals.
 *   Kernels: the one-step register-ring family (orders 2-8, prefetch 1 / 2 / 3 at order 8, EXACT and FAST) has fdw_step_back_dtt_kernel,
 *   the fused backward iteration with one more value of its imaging epilogue: every operand is already in registers, so it adds three
 *   subtractions and one live mask and no memory traffic (36 B/point, as the cross-correlation iteration); no scratch.  Iterations 0 and 1
 *   run the receiver step as the line-source step on the receiver rows (fdw_step_line_kernel: the same damping, leap-frog and injection,
 *   no image).  Orders above 8, the forced generic kernel and FDW_NO_FUSED_BACK=1 run four launches: F_{i-2} (-) F_{i-1} on C into a
 *   context-owned scratch field (allocated by the first call that needs it), the plain source step, fdw_dtt_image_kernel while d_ppr still
 *   holds r^{i-1}, the receiver step without imaging.  The two-step and four-step families have no DTT kernel: a DTT backward loop runs
 *   one-step iterations on every context, as Born does; the forward loop keeps its family.
 *
 * Shots.  fdw_shot_dtt / fdw_shot_line_dtt are fdw_shot / fdw_shot_line with this backward loop (single iterations, then the tail into the
 * two spare source buffers); illum (NULL ok) as fdw_shot_illum, residual = 1 as fdw_shot_residual (resid NULL ok; resid with residual = 0
 * is FDW_EINVAL), v2 NULL: the resident model.  Every output other than imloc equals the cross-correlation call's bit for bit.
 * residual = 1 makes imloc the gradient of the DTT Born misfit (up to the two weights above).  The batches are fdw_shot_batch_residual's
 * and fdw_shot_line_batch_residual's: the same parts under the same budget, fdw_batch_parts 0 / 1 / k as there, batched imloc equal to the
 * single-shot calls bit for bit.  Snapshots (fdw_shot_snaps), slab contexts, the sibling's dialects and excitation imaging do not combine
 * with DTT imaging: FDW_ESTATE where a context of that kind is handed in; there is no DTT form of fdw_shot_snaps or fdw_shot_excitation.
 * Out of scope: DTT kernels in the two-step and pipeline backward families, slabs and several GPUs, snapshots (the conjugate-gradient
 * driver on Born modelling and this imaging condition: "Least-squares migration" below). */
int fdw_dev_back_iter_dtt(fdw_ctx *ctx, int step_source, const float *d_f1, float *d_f0, const float *d_pr, float *d_ppr, const float *d_v2, int r0,
                          int r1, int pp_twice, const float *d_samples, int gz, float *d_img, void *stream);
int fdw_dev_dtt_image(fdw_ctx *ctx, const float *d_fa, const float *d_fb, const float *d_fc, const float *d_r, float *d_img, void *stream);
int fdw_gather_scale_v2(const float *v2, int nxe, int nze, int nxb, int gz, int nx, int nt, const float *g /* [nx][nt] */, float *out);
int fdw_image_unscale_v2(const float *v2, int nxe, int nze, int nxb, int nzb, int nx, int nz, const float *img /* [nx][nz] */, float *out);
int fdw_shot_dtt(fdw_ctx *ctx, const float *v2 /* NULL: resident */, int sx, int sz, int gz, const float *srce, const float *d_obs, float *imloc,
                 float *illum /* NULL ok */, int residual /* 0 | 1 */, float *resid /* NULL ok */, float *P, float *PP);
int fdw_shot_line_dtt(fdw_ctx *ctx, const float *v2, int sz, int gz, const float *wav, const float *d_obs, float *imloc, float *illum, int residual,
                      float *resid, float *P, float *PP);
int fdw_shot_batch_dtt(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                       const float *srce, const float *d_obs, float *imloc, float *illum, int residual, float *resid);
int fdw_shot_line_batch_dtt(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sz, int gz, const float *wav_all,
                            const float *d_obs, float *imloc, float *illum, int residual, float *resid);

/* ---- Extended imaging: subsurface-offset image gathers ------------------------------------------------------------------------------
 * Every imaging condition above needs a migration velocity that is already right.  The extended image over subsurface offset says whether it
 * is:   I(x, z, h) = sum_t F(x - h, z, t) (*) R(x + h, z, t).   With the right velocity the energy sits at h = 0, a velocity error spreads it
 * over h.  The RTM dialect on full-grid contexts, EXACT and FAST numerics alike (FAST changes the Laplacian only).  C is the Born cell set,
 * rows [x0, x1) x columns [z0, z1).
 *
 * For a half-width H, 0 <= H <= FDW_EXT_HMAX, the extended image is 2H+1 field-shaped planes, plane j = h + H; on the device they are
 * contiguous, one fdw_field_bytes apart.  One term, for two fields f and r: for every h = -H .. H and every cell of C whose rows x - h and
 * x + h both lie in [x0, x1)
 *          E[h+H][x][z] = E[h+H][x][z] (+) ( f[x-h][z] (*) r[x+h][z] )          product and sum rounded separately in fp32, round to
 * nearest, nothing fused, in both numerics.  Every other word of every plane keeps its bits: border, padding columns, cells outside the
 * extents, and the |h| rows at either end of C.  No + 0.0f is applied, so a -0.0 survives.  No cell of C is ever damped: every operand is
 * the raw word the buffers hold.
 *
 * The loop: the backward loop of fdw_shot, run as single fdw_dev_back_iter iterations on every context (as DTT imaging does; the forward
 * loop keeps its family).  After iteration k = 0 .. nt-1 the term is added with f = F_k, the source field that iteration images (k < 2: the
 * two snapshots), and r = r^{k+1}, the receiver field it stores, injected sample included; terms in ascending k.  Consequences: the plane
 * h = 0 equals fdw_shot's imloc on the interior cells of C; imloc, P and PP equal fdw_shot's; all-zero data leave every plane as it came;
 * swapping f and r mirrors the planes (the fp32 product commutes): E_{f,r}[h] == E_{r,f}[-h] bit for bit from equal entry planes.
 *
 * fdw_plan_ext_image  the row plan of one term; pure host code, no context, no device.  Rows [x0, x1) of nz columns in chunks of xchunk rows
 *                     (0: automatic -- about 8192 waves of 256 columns where the grid has them, never below max(H, 2) nor above 64 rows;
 *                     the length used goes to *xchunk_out).  Returns the number of chunks and fills chunks[0 .. n) (NULL: counts only; cap
 *                     < n: FDW_EINVAL).  Per chunk: [c0, c1) the rows whose cells it accumulates into, [rd0, rd1) the rows of f and r it
 *                     loads ([c0 - H, c1 + H) cut to [x0, x1): 2H run-in rows), and per plane j the rows it writes, [w0[j], w1[j]) (none:
 *                     0, 0).  The launcher and the kernel form their rows with the same two inline functions (csrc/fdw_extimg.h): a
 *                     shifted row index is the one way this kernel can read outside its arrays, and it is settled here, on the CPU.
 * fdw_dev_ext_image   one term on caller-owned device arrays: d_f, d_r fields, d_eimg 2H+1 planes.  Everything goes on the given stream
 *                     (NULL: the context's), nothing is synchronised, nothing is allocated.  FDW_EINVAL before anything is enqueued: a NULL
 *                     pointer, H outside [0, FDW_EXT_HMAX], d_eimg overlapping an input (d_f may be d_r).  FDW_ESTATE: slab contexts, the
 *                     sibling's dialects, a context inside a batch.  The chunk length follows fdw_set_tuning's xchunk when non-zero.
 * fdw_shot_ext        one shot as defined above.  eimg [2H+1][nx][nz] is accumulated into, as imloc is (imloc NULL: not wanted), so a caller
 *                     stacks shots by passing the same array.  The planes live on the device for the whole shot: allocated on first use,
 *                     sized for the largest H seen, freed by fdw_destroy; without room the call fails with FDW_ENOMEM before the forward
 *                     loop starts.  v2 NULL: the resident model.
 *   Kernels (csrc/fdw_extimg.hip): fdw_ext_image_kernel<H, V, 0>, one instantiation per H and per lane width V (4 words where the arrays are
 *   16-byte aligned, else 1).  Lanes run along z; a wave marches a chunk of rows along x with the last 2H+1 rows of f and of r in two
 *   register rings with static indices, so every f and r word is read once per chunk and every plane row read and written once:
 *   (2 + 2(2H+1)) * 4 B per point.  No LDS, no scratch, no atomics.  FDW_EXT_POINTWISE=1 (read when a context is created; benchmarks and
 *   tests) runs the obvious alternative, one thread per cell reading its 2(2H+1) operands through the caches; the same bytes in every plane.
 *   Measured on one MI355X (profiles/ext_image.json), 8192^2, H = 0 / 1 / 4 / 8: 224 / 436 / 1223 / 2132 us per term
 *   (4.8 / 4.9 / 4.4 / 4.5 TB/s of the byte model; the one-step backward iteration reaches 5.3 TB/s there), the pointwise form 1.16 to
 *   1.27 times that; 2048^2: 10 / 25 / 59 / 107 us.  fdw_shot_ext at 8192^2, nt 500, H = 4: 1.20 s (fdw_shot_dtt: 0.32 s).
 * Out of scope: fusing the term into the backward kernels; the two-step and pipeline backward families; batched, line-source, residual and
 * DTT forms; slabs and several GPUs; time-shift gathers; the offset-to-angle transform; an extended Born operator. */
#define FDW_EXT_HMAX 8
typedef struct fdw_ext_chunk {
    int c0, c1;                          /* rows accumulated into */
    int rd0, rd1;                        /* rows of f and r loaded */
    int w0[2 * FDW_EXT_HMAX + 1];        /* plane j = h + H: rows written, [w0[j], w1[j]) */
    int w1[2 * FDW_EXT_HMAX + 1];
} fdw_ext_chunk;
int fdw_plan_ext_image(int x0, int x1, int nz, int H, int xchunk, int *xchunk_out, fdw_ext_chunk *chunks, int cap);
int fdw_dev_ext_image(fdw_ctx *ctx, const float *d_f, const float *d_r, int H, float *d_eimg, void *stream);
int fdw_shot_ext(fdw_ctx *ctx, const float *v2 /* NULL: resident */, int sx, int sz, int gz, const float *srce, const float *d_obs, int H,
                 float *imloc /* NULL ok */, float *eimg /* [2H+1][nx][nz], in/out */, float *P, float *PP);

/* ---- Least-squares migration: conjugate gradients on Born modelling and DTT imaging ---------------------------------------------------
 * The layer that iterates: a device-resident conjugate-gradient solver for min_m 1/2 sum_s |L_s m - d_s|^2, L_s = FDW_BORN_DTT modelling of
 * shot s, L_s^T = DTT imaging with the two v2 weights.  Same dialect, contexts and numerics as the Born section (RTM dialect, full-grid
 * contexts, EXACT and FAST: FAST changes the Laplacian only).  C is the Born cell set.  Model-space vectors are field-shaped device arrays
 * [nxl][pitch] of which only the words on C are ever read or written: every other word keeps its bits.
 *
 * Sum order S(x_0 .. x_{n-1}) of doubles: 64 partials s_l = x_l + x_{l+64} + ..., each ascending onto +0.0; then for d = 32, 16, .., 1:
 * s_l = s_l + s_{l+d} for l < d; the result is s_0 (n = 0: +0.0).  A dot product over C: the terms of row x are (double)a * (double)b (exact
 * for two floats) in column order, the row sum is S of the row's terms, the total S of the row sums in row order.  A gather [nt][nx]: the
 * same with the time rows as rows.  Totals of several shots are added in shot order onto +0.0.  No number depends on launch geometry or
 * tuning: one wave of 64 lanes performs S as it stands, nothing is added atomically.
 *
 * Visit of shot s with direction p, V_s(p, d_obs):
 *   1. the Born loop of fdw_born_shot (kind FDW_BORN_DTT) from rest with m = p; q [nt][nx] = its scattered gather, on the device;
 *   2. w = q when d_obs == NULL, else w = d_obs (-) q; n2 = <w, w> in the order above (before the weight);
 *   3. ws[it][ix] = w[it][ix] (*) v2[nxb+ix][gz]: fdw_gather_scale_v2 on the device layout;
 *   4. the DTT backward loop of fdw_shot_dtt (single iterations and the tail) onto a zeroed image with ws as the receiver data; its two
 *      snapshots are the background pair the Born loop just left (the older one damped once, fdw_dev_taper_finalize, as fdw_shot's forward
 *      loop leaves it): no second forward loop runs, and the image is the one fdw_shot_dtt(residual = 0, d_obs = ws) forms, bit for bit;
 *   5. on C: h = h (+) mask (*) (img (/) v2), quotient, product and sum rounded separately; mask == NULL: h = h (+) (img (/) v2).
 * Solve.  All scalars are doubles that live on the device; every fp32 update is a separately rounded product and sum in both numerics.
 *   start   g = 0; for each shot in order V_s(m, d_s) stacks into g.  misfit_0 = 1/2 sum_s n2_s, gamma = <g, g>, p = g.
 *   k = 0 .. niter-1:  h = 0; the visits V_s(p, NULL) stack into h.  delta = sum_s n2_s, alpha = gamma / delta (0 when delta == 0),
 *           af = (float)alpha.  m = m (+) af (*) p, g = g (-) af (*) h.  gamma' = <g, g>, beta = gamma' / gamma (0 when gamma == 0),
 *           p = g (+) (float)beta (*) p.  misfit_{k+1} = misfit_k - 1/2 (alpha gamma), gamma = gamma'.
 *   verify  one more pass of visits V_s(m, d_s) into a scratch image: the recomputed misfit 1/2 sum_s n2_s and the residual gathers w.
 *
 * Device arrays; everything goes on the given stream (NULL: the context's), nothing is synchronised or allocated.  d_rows receives the
 * row sums, d_sum / d_n2 / d_gg (one double) their S:
 *   fdw_dev_dot_cells    <a, b> over C; d_rows [x1 - x0] (the rows of C, fdw_get_extents).
 *   fdw_dev_dot_gather   <a, b> of two gathers [nt][nx]; d_rows [nt].
 *   fdw_dev_lsm_gather   steps 2 and 3 in one pass over [nt][nx]: d_w (NULL ok; may be d_q) = w, d_ws (may be d_obs, or d_q) = ws, d_rows
 *                        [nt], d_n2.  Every word is read before it is written, by the one thread that writes it.
 *   fdw_dev_lsm_stack    step 5.
 *   fdw_dev_lsm_update   m = m (+) af (*) p, g = g (-) af (*) h on C with af = (float)*d_alpha read on the device; d_rows [x1 - x0] and
 *                        d_gg = <g, g> of the new g, formed in the same pass.
 *   fdw_dev_lsm_direction  p = g (+) (float)*d_beta (*) p on C.
 *   FDW_EINVAL before anything is enqueued: a NULL required pointer, gz outside [0, zlim).  FDW_ESTATE: slab contexts, the sibling's
 *   dialects, a context inside a batch.
 *   Kernels (csrc/fdw_lsm.hip): fdw_lsm_dot_rows_kernel, fdw_lsm_gather_kernel and fdw_lsm_update_kernel run one wave per row (coalesced
 *   along z, or along ix of a gather), fdw_lsm_finish_kernel one wave over the row sums, fdw_lsm_stack_kernel and fdw_lsm_direction_kernel
 *   are pointwise, fdw_lsm_scalar_kernel is one wave that turns gamma, delta, gamma' into alpha, beta and the misfit history in device
 *   memory.  The fp32 quotient of step 5 is the fp64 quotient of the two floats rounded once more (53 >= 2 * 24 + 2 bits: correctly rounded).
 *
 * fdw_lsm_visit   one visit on host arrays: p, mask (NULL ok), h (in/out) [nx][nz]; d_obs (NULL ok), data (NULL ok: receives w) [nx][nt];
 *                 *n2 = <w, w>.  v2 NULL: the resident model (FDW_ESTATE without one).  Synchronous.
 * fdw_lsm_visit_batch  the visits V_b(p, d_obs[b]) of nshots shots on ONE direction p, stacked into h in shot order; shots and models as
 *                 fdw_born_shot_batch takes them (v2_all / draw_offset, sx0, dsx); d_obs (NULL ok) and data (NULL ok) [nshots][nx][nt],
 *                 n2 [nshots].  Groups, parts and fdw_batch_parts as fdw_lsm_solve's passes (below); the bytes are those of fdw_lsm_visit
 *                 on each shot.  Synchronous.
 * fdw_lsm_solve   the solve above; shots and models as fdw_shot_batch takes them (v2_all [nshots][nxe][nze], or NULL: the border models of
 *                 draws draw_offset + b T on the resident model; source rows sx0 + b dsx), d_obs [nshots][nx][nt], mask [nx][nz] (NULL
 *                 ok), m [nx][nz] in/out.  misfit receives niter + 1 doubles, one more (the recomputed misfit) with verify = 1; resid
 *                 (NULL ok, verify = 1 only) [nshots][nx][nt] the residual gathers of the verify pass.  m, g, p, h, the mask and every
 *                 gather stay on the device for the whole solve; the host reads no scalar back per iteration, the history comes down
 *                 once at the end.  Where fdw_born_shot_batch and fdw_shot_batch_dtt both batch, the visits of a pass run one launch per
 *                 time step in both loops inside fdw_shot_batch's buffers (the scattered pairs become the spare source buffers; no new
 *                 field buffers), in groups of what the budget (fdw_set_batch_budget) holds of eleven fields and one gather per shot;
 *                 the gather pass and the stack run shot by shot in shot order.  Elsewhere, under a budget below one shot's share and
 *                 without room on the device the shots run one by one.  The same bytes come out either way.  fdw_batch_parts: the
 *                 groups of one pass, 0 / 1 / k as for the other batched calls.  Synchronous; work arrays are allocated on first use
 *                 and freed by fdw_destroy.
 *   Refusals, before anything is enqueued: those of fdw_born_shot / fdw_born_shot_batch (FDW_EINVAL: a NULL required pointer, nshots < 1,
 *   sz, gz or a source row outside the time-stepped cells; FDW_ESTATE: no model), niter < 0, verify outside {0, 1}, resid without verify
 *   (FDW_EINVAL); slab contexts, the sibling's dialects and a context inside a batch: FDW_ESTATE.
 * Measured on one MI355X (profiles/lsm.json; order 8, seconds per shot and iteration): 8192^2, nt 500: 0.4523 against
 * 0.5364 for fdw_born_shot followed by fdw_shot_dtt on the parent's build (ratio 0.843; FAST 0.4461 / 0.5239, 0.851); 415 x 295 interior,
 * nt 1700, 32 shots batched: 0.005030 against 0.006378 for fdw_born_shot_batch followed by fdw_shot_batch_dtt (0.789; FAST 0.796).
 * rtm_code: the deck key lsm=N (with lsm_mute=K) runs fdw_lsm_solve on the deck's shots (csrc/rtm_code.c).
 * Out of scope: line-source, plane-wave and encoded forms, slabs and several GPUs, illumination or Hessian preconditioning,
 * regularisation. */
int fdw_dev_dot_cells(fdw_ctx *ctx, const float *d_a, const float *d_b, double *d_rows, double *d_sum, void *stream);
int fdw_dev_dot_gather(fdw_ctx *ctx, const float *d_a, const float *d_b, double *d_rows /* [nt] */, double *d_sum, void *stream);
int fdw_dev_lsm_gather(fdw_ctx *ctx, const float *d_q, const float *d_obs /* NULL ok */, const float *d_v2, int gz, float *d_w /* NULL ok */, float *d_ws,
                       double *d_rows /* [nt] */, double *d_n2, void *stream);
int fdw_dev_lsm_stack(fdw_ctx *ctx, float *d_h, const float *d_img, const float *d_v2, const float *d_mask /* NULL ok */, void *stream);
int fdw_dev_lsm_update(fdw_ctx *ctx, float *d_m, float *d_g, const float *d_p, const float *d_h, const double *d_alpha, double *d_rows, double *d_gg,
                       void *stream);
int fdw_dev_lsm_direction(fdw_ctx *ctx, float *d_p, const float *d_g, const double *d_beta, void *stream);
int fdw_lsm_visit(fdw_ctx *ctx, const float *v2 /* NULL: resident */, const float *p, int sx, int sz, int gz, const float *srce,
                  const float *d_obs /* NULL ok */, const float *mask /* NULL ok */, float *h, double *n2, float *data /* NULL ok */);
int fdw_lsm_visit_batch(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, const float *p /* ONE for all shots */, int sx0,
                        int dsx, int sz, int gz, const float *srce, const float *d_obs /* NULL ok */, const float *mask /* NULL ok */, float *h,
                        double *n2 /* [nshots] */, float *data /* NULL ok */);
int fdw_lsm_solve(fdw_ctx *ctx, int nshots, const float *v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz, const float *srce,
                  const float *d_obs, const float *mask /* NULL ok */, int niter, float *m, double *misfit, int verify, float *resid /* NULL ok */);

/* ---- tuning / introspection --------------------------------------------------------------------
 * fdw_set_tuning  xchunk = rows marched per wave (0 = auto), wz = waves of a block laid along z
 *                 (1,2,4; 0 = auto), use_generic = force the generic-order kernel (tests),
 *                 prefetch = software prefetch distance in rows (0 = default; 1..3, order 8 only),
 *                 two_step = temporal blocking in the forward loops: 0 auto (by grid size), 1 two steps per pass always,
 *                 4 the four-steps-per-pass wave pipeline always, -1 never.
 * fdw_get_tables  copies of the derived host tables (any pointer may be NULL):
 *                 coefs_x/z[order+1] (R:214-217), taper_x[nxb], taper_z[nzb] (R:159-166).
 * fdw_get_extents xlim/zlim = rows/columns the time update covers, ztap = damped columns (R:185-195).
 * fdw_selftest    checks on the device the two hardware behaviours the kernels rely on (one-lane
 *                 __shfl_up/down, range-predicated buffer stores); 0 if they are as assumed.
 */
int fdw_set_tuning(fdw_ctx *ctx, int xchunk, int wz, int use_generic, int prefetch, int two_step);
int fdw_get_tables(const fdw_ctx *ctx, float *coefs_x, float *coefs_z, float *taper_x, float *taper_z);
int fdw_get_extents(const fdw_ctx *ctx, int *xlim, int *zlim, int *ztap);
/* Tests and probes (nothing is launched).
 * fdw_debug_step4_plan  what fdw_dev_step4 would launch on these row ranges (forward = 1: FWD with the source at (sx, sz), sx < 0 none;
 *                       0: the PLAIN pass): tiles, strips and, for tile L = chunk row * nstrip + strip, cls[L] = 0 if it runs the lean body
 *                       (no masks, clamps, damping or source code), 1 if the full body; at most cls_cap entries are written (cls may be NULL).
 */
int fdw_debug_step4_plan(fdw_ctx *ctx, int forward, int sx, int sz, int r0, int r1, int r0b, int r1b, int xchunk, int *nblk, int *nstrip,
                         unsigned char *cls, int cls_cap);
int fdw_two_step_active(const fdw_ctx *ctx); /* 1 if the forward loops of this context use the two-step kernel */
int fdw_steps_per_pass(const fdw_ctx *ctx);  /* time steps one launch of the forward loops advances: 4 (wave pipeline), 2 or 1 */
int fdw_selftest(fdw_ctx *ctx);
/* 1 if the host loops emit roctx ranges (forward loop, backward loop, halo exchange, shot): they do when a marker library
 * (librocprofiler-sdk-roctx / libroctx64) is already in the process -- rocprofv3 --marker-trace -- or FDW_ROCTX=1 asks for it. */
int fdw_trace_active(void);

/* ---- consecutive four-step forward passes as row bands on side streams -------------------------
 * Two launches in one stream never overlap, so every pass of fdw_dev_steps2 fills and drains the chip on its own.  A pass cut into G
 * bands of whole chunk rows can overlap the next one: pass n+1 on a band needs pass n on that band and its two neighbours only.  The
 * tiles are the same tiles (bands are cut on chunk boundaries with the pass's own chunk length), so every result is unchanged bit for bit.
 *
 * fdw_plan_pass_bands  the schedule; pure host C, no context, no device.  nxl rows, of which [0, upd_x1) are time-stepped; xchunk = the
 *                      pass's chunk length; bands / depth = the wanted G / D (depth 1..FDW_PASS_DEPTH_MAX); npasses >= 1.
 *                      Launch units are numbered pass-major, band-minor: unit i = n * G + g is pass n on band g.  Bands are whole chunk
 *                      rows counted from row 0, as equal as possible (the first ones take the extra chunk row); the last band ends at
 *                      nxl: it owns the static rows [upd_x1, nxl) that every pass copies.  Unit i runs on stream i mod D (stream 0 is the
 *                      caller's) and first waits for the events of units i-D-1 .. i-2D+1 (D-1 of them; those below 0 do not exist).  With
 *                      stream order (unit i-D) every unit up to i-D is then complete, and unit i overlaps at most the D-1 units before
 *                      it.  That is safe if and only if every band holds at least 16 time-stepped rows (four steps of half order 4: a
 *                      pass on a band then reads rows of the adjacent bands only, and overwrites only what pass n-1 read there) and
 *                      G >= D+1 (the adjacent bands of pass n-1 lie at or below i-D).  A request that is not -- or G = 1 -- comes back
 *                      as ONE band [0, nxl) of depth 1: the plain loop.  *bands_out / *depth_out = what the plan uses; units (may be
 *                      NULL) receives min(cap, G * npasses) entries.  Returns G * npasses, or FDW_EINVAL.
 * fdw_set_pass_bands   the policy of fdw_dev_steps2 on this context: bands = depth = 0 automatic (below); depth 1: the bands run one after
 *                      the other on the caller's stream, no event involved.  bands < 0, depth outside [0, FDW_PASS_DEPTH_MAX] or only one of
 *                      the two zero: FDW_EINVAL.  While the policy is automatic the environment variable FDW_PASS_BANDS="G,D" (read
 *                      at every call; experiments) takes its place.
 * fdw_pass_bands       what the last fdw_dev_steps2 call on this context used (1, 1: the plain loop; 0, 0 before the first call).
 *
 * Where the schedule is used: fdw_dev_steps2 only (not inside a batch), for the passes of the four-step kernel; the steps left over
 * (nsteps mod 4) and every other entry point -- the recording, illumination and line-source loops, fdw_forward and the shots, the slab
 * drivers -- run as before.  Automatic policy (where the moving cut below does not apply: 12288^2 and larger since round 21), from the
 * measurement on one MI355X: 3 bands, depth 2
 * where a pass has at least 1776 tiles (8192^2 and larger: +3.2 % at 8192^2, +3.1 % at 12288^2, +1.7 % at 16384^2 in EXACT numerics,
 * +7.6 % at 8192^2 and +4.2 % at 16384^2 in FAST) and the call holds at least 8 passes; one band otherwise (4096^2: -16 %; 6144^2: not
 * separable from one band; a call of one pass only pays for the cut).  THE GAIN NEEDS A HARDWARE QUEUE FOR THE SIDE STREAM: a process has four, and where more streams than that are alive two
 * streams may share one; a side stream that shares the caller's queue runs behind it and the schedule costs up to a quarter of the
 * loop's time.  A process with many streams of its own sets one band (fdw_set_pass_bands(ctx, 1, 1)), as fdw_slabs_create does.
 * STREAMS (the one amendment to the stream contract above): with depth D > 1 the units of streams 1 .. D-1 run on side streams the context
 * owns (hipStreamNonBlocking, created on first use).  Every side stream first waits for an event recorded on the caller's stream at
 * entry, so a producer queued there is respected; the caller's stream waits for the last unit of every side stream before the left-over
 * steps and before the call returns -- also when a launch fails part-way.  The call stays asynchronous and ordered on the stream it was
 * given: what is queued behind it sees its results.  At most FDW_PASS_DEPTH_MAX = 3 streams, the caller's included. */
#define FDW_PASS_DEPTH_MAX 3
typedef struct fdw_band_unit {
    int pass, band;     /* n, g (fdw_plan_pass_cut: 0 lower, 1 upper, 2 the middle of a turn) */
    int r0, r1;         /* rows the unit produces (r1 = nxl for the last band: its launch ends at upd_x1 and copies the static rows) */
    int stream;         /* i mod D */
    int nwait;          /* 0 .. FDW_PASS_DEPTH_MAX - 1 */
    int wait[FDW_PASS_DEPTH_MAX - 1];   /* unit numbers, descending */
} fdw_band_unit;
int fdw_plan_pass_bands(int nxl, int upd_x1, int xchunk, int bands, int depth, int npasses, int *bands_out, int *depth_out,
                        fdw_band_unit *units, int cap);
int fdw_set_pass_bands(fdw_ctx *ctx, int bands, int depth);
int fdw_pass_bands(const fdw_ctx *ctx, int *bands, int *depth);

/* ---- two bands with a moving cut ---------------------------------------------------------------------
 * Fixed bands need three of them to run two deep (G >= D+1).  Two suffice when the cut between them MOVES by one chunk row per pass:
 * pass n is cut at chunk row c_n into a lower unit [0, c_n * xchunk) and an upper unit [c_n * xchunk, nxl).  While the cut moves down,
 * the lower unit of pass n+1 reads only rows the lower unit of pass n produced (xchunk >= 16 = the reach of a pass), so it may overlap
 * the upper unit of pass n; moving up, the same holds for the upper units.  The cut bounces between cut_lo and cut_hi.  Same tiles, same
 * results bit for bit, two launches per pass instead of three and two larger units resident.
 *
 * fdw_plan_pass_cut   the schedule; pure host C, no context, no device.  nxl, upd_x1, xchunk, npasses as for fdw_plan_pass_bands; the cut
 *                     of pass 0 is chunk row cut_hi and moves down; at cut_lo it turns and moves up, at cut_hi it turns again.  Two units
 *                     per pass, band 0 = lower, band 1 = upper (ends at nxl, owns the static rows); a pass whose cut moved down (and pass
 *                     0) issues the lower unit first, one whose cut moved up the upper unit first.  Unit i runs on stream i mod 2 and
 *                     waits for unit i-3; with stream order (i-2) everything up to i-2 is complete, so unit i can overlap unit i-1 only.
 *                     THE TURN.  A range at least four chunk rows wide turns through a pass of THREE units, none of which needs the
 *                     unit before it: after the pass cut at cut_lo+1, the lower unit [0, cut_lo X), the upper unit [(cut_lo+2) X, nxl)
 *                     and last the middle (band 2) between them; the next pass is cut at cut_lo+3 and issues its upper unit first.  At
 *                     the top the mirror image: after the pass cut at cut_hi-1, the upper unit [cut_hi X, nxl), the lower unit
 *                     [0, (cut_hi-2) X), the middle; the next pass is cut at cut_hi-3.  A narrower range turns on the spot (cut_lo,
 *                     cut_lo+1, ...), and there -- nowhere else -- the first unit of the pass after the turn touches rows of the unit
 *                     before it and waits for i-1 as well (wait[] descending: i-1, i-3).  Measured: a wait
 *                     for i-1 starts both streams' units at the same moment, and units in step run a quarter slower for several passes.
 *                     Thin requests come back as ONE unit
 *                     per pass ([0, nxl), stream 0, no waits: the plain loop) with *lo_out = *hi_out = 0: xchunk below 16, fewer than
 *                     three chunk rows, cut_lo = cut_hi, or a unit that can hold fewer than 16 time-stepped rows (cut_lo = 0;
 *                     upd_x1 - cut_hi * xchunk < 16).  Otherwise *lo_out / *hi_out = cut_lo / cut_hi.  units (may be NULL) receives
 *                     min(cap, count) entries.  Returns the unit count (2 per pass plus 1 per three-unit turn); FDW_EINVAL for
 *                     nxl < 1, upd_x1 outside [0, nxl], xchunk < 1, cut_lo < 0, cut_hi < cut_lo, npasses < 1 or cap < 0.
 * fdw_set_pass_cut    the policy of fdw_dev_steps2 on this context: 0, 0 automatic (below); -1, -1 off (the band policy alone decides);
 *                     1 <= lo <= hi: that cut range (a thin one runs the plain loop).  Anything else: FDW_EINVAL.  While it is automatic
 *                     the environment variable FDW_PASS_CUT="lo,hi" (read at every call; experiments) takes its place.  An explicit
 *                     fdw_set_pass_bands (anything but 0, 0) and FDW_PASS_BANDS take precedence over all of this.
 *                     Automatic, from the measurement on one MI355X: the moving cut over the middle
 *                     third of the chunk rows, [nch/3, nch - nch/3], where a pass has 60 000 to 500 000 strip rows (rows x strips of 56
 *                     columns of 4 cells: 4096^2 to 8192^2; +5.9 % at 4096^2, +10.6 % at 6144^2, +2.2 % at 8192^2 with 213-row chunks
 *                     instead of 173, EXACT numerics) and the call holds at least 8 passes; elsewhere the band policy above decides.
 * fdw_pass_cut        what the last fdw_dev_steps2 call used: the cut range and the number of turns (passes of three units, or units that
 *                     waited for the unit just before them); -1, -1, 0 when the moving cut did not run.  fdw_pass_bands reports 2, 2
 *                     when it did.
 *
 * Streams: the caller's and the one side stream of the band schedule, forked and joined in the same way (STREAMS above). */
int fdw_plan_pass_cut(int nxl, int upd_x1, int xchunk, int cut_lo, int cut_hi, int npasses, int *lo_out, int *hi_out, fdw_band_unit *units,
                      int cap);
int fdw_set_pass_cut(fdw_ctx *ctx, int lo, int hi);
int fdw_pass_cut(const fdw_ctx *ctx, int *lo, int *hi, int *turns);

/* ---- host formulas of libsource.a restated (pure C, usable without a device) --------------------
 * fdw_calc_coefs        calc_coefs + makeo2, F:113-192 / S:137-216 (cxx selects the float variant)
 * fdw_ricker_wavelet    ricker_wavelet, F:302-334
 * fdw_taper_tables      taper tables of fd_init_cuda, R:159-166
 * fdw_extendvel_linear  extendvel_linear, F:336-394; vel is [nxe][nze] contiguous; draws the stream
 *                       glibc rand() yields (the reference never seeds it, R:486) from a PRIVATE restatement
 *                       of that generator, so nothing else in the process can perturb the border model
 * fdw_srand             reseeds that private generator like srand(); a fresh process behaves as fdw_srand(1)
 */
int fdw_calc_coefs(int order, int cxx, float *coef /* [order+1] */);
void fdw_ricker_wavelet(int nt, float dt, float fpeak, float *s);
void fdw_taper_tables(int nxb, int nzb, float fac, float *taper_x, float *taper_z);
void fdw_extendvel_linear(int nx, int nz, int nxb, int nzb, float *vel);
void fdw_srand(unsigned seed);

#ifdef __cplusplus
}
#endif
#endif /* FDWAVE_H */

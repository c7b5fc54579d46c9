/* rtm_code -- drop-in for cuda_reference_RTM/rtm_code (src/fd-code.cu = R):
 *     ./rtm_code ./models/<model>/input.dat
 * Same deck keys and defaults (R:343-378), same input binaries (vpfile [nx][nz], datfile
 * [ns][nx][nt], optional vel_ext_file [ns][nxe][nze]), same outputs: <tmpdir>/dir.image (stacked image
 * [nx][nz]), <tmpdir>/dir.image_lap (zeros, R:477,542), empty dir.snaps / dir.snaps_rec / dir.snapr
 * (R:465-470; filled by the key `snap`, below), ./image.num text dump (R:522-528), and the stdout banners.  The per-shot propagation
 * (fd_forward + fd_back, R:499-518) is one device-resident fdw_shot() call; launch extents are the
 * reference's (compat = 1), so the image equals the reference's.  Shots run side by side on up to FDW_SHOT_WORKERS (default 4) host
 * threads / streams; models are drawn and images stacked in shot order, so every output is what the serial loop writes.
 * Not reproduced: the `file-teste` debug dump at it == 750 (R:268-281) and the in-loop progress lines.
 *
 * Several GPUs (no counterpart in the reference, which drives one): the deck key `slabs=N` (or FDW_SLABS=N in the environment) runs every
 * shot on N GPUs, the grid cut into N bands of rows with halo exchange over RCCL / xGMI inside libfdwave.so (fdw_slabs_shot), one host
 * thread per GPU; FDW_SLABS_LOCAL=1 keeps all N ranks on GPU 0 with device copies instead of RCCL (tests on a one-GPU box).  `gpus=N` (or
 * FDW_GPUS=N) deals whole shots to N GPUs instead.  Every output file is byte for byte the one-GPU program's.
 *
 * Source illumination (no counterpart in the reference): the deck key `illum=1` makes every shot's forward loop accumulate sum_t F_t^2
 * (fdw_shot_illum; per shot from zero, stacked on the host in shot order like the image) and adds two outputs, <tmpdir>/dir.illum (the
 * stack, [nx][nz]) and <tmpdir>/dir.image_illum = fdw_image_compensate(image, illumination, illum_eps), `illum_eps` defaulting to 1e-3.
 * dir.image, dir.image_lap and image.num are what they are without the key.  Small decks still advance a batch of shots through one
 * launch per time step (fdw_shot_batch_illum: one accumulator field per shot); together with slabs > 1 the key is refused.
 *
 * Wavefield snapshots (the reference opens the three files, reads the deck key `iss` -- "save snaps of this source", R:368 -- and writes
 * nothing): the deck key `snap=K` (absent, -1 or 0: the three files stay empty, every byte of every output as before) runs shot `iss`
 * through fdw_shot_snaps and writes its frames at the time levels K, 2K, ... <= nt (fdwave.h): dir.snaps the forward field, dir.snaps_rec
 * the source field the backward loop images at that level, dir.snapr the receiver field it is multiplied with -- each
 * [nt / K][ceil(nx / D)][ceil(nz / D)] floats, D = `snap_dec` (default 1) the decimation along both axes.  On decks that batch their shots,
 * shot `iss` leaves its batch and runs alone; among workers (and GPUs) the one that owns the shot takes the frames.  dir.image,
 * dir.image_lap, image.num and dir.illum* stay byte for byte what they are without the key.  iss >= ns, snap_dec < 1 and snap > 0 together
 * with slabs > 1 are refused before anything is opened.
 *
 * Residual migration (no counterpart in the reference): the deck key `resid=1` (absent or 0: the same files and the same bytes as without
 * it) sends every shot through fdw_shot_residual / fdw_shot_batch_residual: the forward loop models the shot's gather in the migration
 * model, and the backward loop migrates datfile's gather minus that one (fdwave.h) -- the direct arrival leaves the data on the device, and
 * the image is the gradient of the least-squares misfit.  Shots batch where the program batches, `gpus=N` workers take their own shots,
 * the host stacks in shot order as always.  With `illum=1` too, dir.illum and dir.image_illum are written as before and now describe the
 * residual image.  Two more outputs: <tmpdir>/dir.resid ([ns][nx][nt] floats, the layout of datfile, each shot at its offset) and
 * <tmpdir>/dir.misfit (ns doubles, 0.5 sum resid^2 per shot, fdw_gather_misfit); the total is printed after the shots.  resid=1 together
 * with slabs > 1 or with snap > 0 is refused before anything is opened.
 *
 * Plane-wave migration (no counterpart in the reference): the deck key `pw=NP` (>= 1; absent: nothing changes) migrates NP plane-wave
 * gathers instead of the ns shots.  Plane wave j has the ray parameter p_j = NP == 1 ? 0 : -P + 2 P j / (NP - 1) s/m, P = `pw_pmax`
 * (>= 0; absent or 0: NP must be 1).  Its lags come from the deck's shot rows fsx + is ds (fdw_planewave_lags), its source gather from the
 * Ricker wavelet with weights of 1 (fdw_encode_line_source), its data gather from the ns gathers of datfile (fdw_encode_gathers); the
 * model is the next draw of the border stream (R:486) or vel_ext_file's model j mod ns (R:484); fdw_shot_line migrates it.  The images
 * are stacked in the order j into dir.image, image.num has one section per plane wave, illum=1 and image_lap=1 work as for shots.  One
 * plane wave after the other; pw together with slabs > 1, gpus > 1, resid=1 or snap > 0 is refused before anything is opened.
 *
 * Excitation-amplitude imaging (no counterpart in the reference): the deck key `exc=1` (absent or 0: nothing changes) sends the shots, in
 * groups of fdw_shot_batch_max, through fdw_shot_excitation_batch (a group of one, or FDW_NO_SHOT_BATCH=1: fdw_shot_excitation): the forward loop keeps the peak of the source field and its time level per cell, the backward loop
 * propagates the receiver field alone and every cell takes its sample at that level.  dir.image is the stack in shot order of exc / amp
 * where |amp| > exc_eps max |amp| (fdw_image_excitation; `exc_eps` defaults to 1e-3), image.num has one section per shot.  exc together
 * with illum=1, resid=1, pw, snap > 0, slabs > 1 or gpus > 1 (deck or environment) is refused before anything is opened.
 *
 * Least-squares migration (no counterpart in the reference): the deck key `lsm=N` (absent or 0: nothing changes) makes dir.image the model
 * after N conjugate-gradient iterations of fdw_lsm_solve on the deck's shots, from zero; `lsm_mute=K` (default 0) zeroes the mask on the
 * interior columns iz < K.  <tmpdir>/dir.lsm_misfit holds N + 2 doubles: the misfit history and last the recomputed misfit; the history is
 * printed.  lsm together with exc, snap, slabs, pw, gpus, illum, resid or dtt is refused before anything is opened.
 *
 * DTT imaging (no counterpart in the reference): the deck key `dtt=1` (absent or 0: nothing changes) images every shot with the second time
 * difference of the source field instead of the cross-correlation (fdwave.h, "DTT imaging": fdw_shot_dtt, fdw_shot_batch_dtt, with pw
 * fdw_shot_line_dtt / fdw_shot_line_batch_dtt).  It composes with resid=1 (dir.image is then the gradient of the DTT Born misfit, up to the
 * two v2 weights of fdwave.h), illum=1, pw=NP, batching and gpus=N; every output other than the images keeps its bytes.  dtt=1 together
 * with exc=1, snap > 0 or slabs > 1 (deck or environment) is refused before anything is opened.
 *
 * Extended imaging (no counterpart in the reference): the deck key `ext=H`, 1 <= H <= 8 (absent or 0: nothing changes), also writes
 * <tmpdir>/dir.image_ext, the subsurface-offset extended image [2H+1][nx][nz] stacked in shot order (fdwave.h, "Extended imaging":
 * fdw_shot_ext, the shots one by one on one context, all into the same planes).  dir.image, dir.image_lap and image.num are byte for byte
 * what the run without the key writes.  ext together with exc, dtt, lsm, pw, slabs, gpus, snap, resid or illum is refused before anything
 * is opened. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <sys/time.h>

#include "fdw_config.h"
#include "fdwave.h"

static float *read_floats(const char *path, size_t n, const char *what)
{
    FILE *f = path ? fopen(path, "rb") : NULL;
    if (!f) {
        fprintf(stderr, "cannot open %s '%s'\n", what, path ? path : "(null)");
        return NULL;
    }
    float *a = (float *)calloc(n ? n : 1, sizeof(float)); /* R:414,421,438 memset to 0 then fread */
    const size_t got = a ? fread(a, sizeof(float), n, f) : 0;
    fclose(f);
    if (got != n) fprintf(stderr, "warning: %s '%s' holds %zu of %zu floats (rest stays zero)\n", what, path, got, n);
    return a;
}

static FILE *open_out(const char *dir, const char *name)
{
    char path[4096];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    FILE *f = fopen(path, "w");
    if (!f) fprintf(stderr, "cannot create '%s'\n", path);
    return f;
}

/* one batch of shots shared out to host threads: worker w takes shots w, w + nw, ... of the batch */
typedef struct {
    const fdw_params *prm;
    int ns, nworkers, is0, nb, nx, nt, sz, gz;
    const int *sx;
    const float *srce, *d_obs, *vel2_all;
    const float *vp;      /* dev_border: the interior model every worker keeps resident in HBM */
    long long draws;      /* rand() calls one extendvel_linear consumes */
    int dev_border;
    float *imloc_all;
    float *illoc_all;     /* illum=1: the shots' source illumination [nb][nx][nz], else NULL */
    int resid;            /* resid=1: every shot through fdw_shot_residual */
    int dtt;              /* dtt=1: every shot through fdw_shot_dtt (with resid: its residual form) */
    float *resloc_all;    /* ... the shots' residual gathers [nb][nx][nt] */
    int snap_is;          /* snap=K: the shot whose wavefield frames are taken, else -1 */
    const fdw_snaps *snaps;
    size_t ne, ni;
    int gpus;             /* workers are dealt to GPUs 0 .. gpus-1 */
    volatile int failed;
} shot_job;
typedef struct {
    shot_job *job;
    int w, nw;
} shot_worker_arg;

static void *shot_worker(void *p)
{
    shot_worker_arg *a = (shot_worker_arg *)p;
    shot_job *j = a->job;
    fdw_ctx *ctx = NULL;
    if (fdw_create(j->prm, a->w % (j->gpus > 0 ? j->gpus : 1), &ctx) != FDW_OK) { /* fd_init, R:452 (one context = one stream + its own device buffers per worker) */
        fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
        j->failed = 1;
        return NULL;
    }
    if (j->dev_border && fdw_model_resident(ctx, j->vp) != FDW_OK) {
        fprintf(stderr, "fdw_model_resident: %s\n", fdw_last_error());
        j->failed = 1;
    }
    for (int b = a->w; b < j->nb && !j->failed; b += a->nw) {
        const int is = j->is0 + b;
        const float *d_obs = j->d_obs + (size_t)is * j->nx * j->nt;
        float *imloc = j->imloc_all + (size_t)b * j->ni;
        float *illoc = j->illoc_all ? j->illoc_all + (size_t)b * j->ni : NULL;
        int rc;
        if (j->dtt) {                /* the DTT imaging condition (illoc may be NULL; with resid the residual gather comes back too; never with snap) */
            rc = j->dev_border ? fdw_dev_extendvel_linear(ctx, (unsigned long long)is * (unsigned long long)j->draws, NULL) : FDW_OK;
            if (rc == FDW_OK)
                rc = fdw_shot_dtt(ctx, j->dev_border ? NULL : j->vel2_all + (size_t)b * j->ne, j->sx[is], j->sz, j->gz, j->srce, d_obs, imloc, illoc, j->resid,
                                  j->resid ? j->resloc_all + (size_t)b * j->nx * j->nt : NULL, NULL, NULL);
        } else if (j->resid) {       /* d_obs minus the gather the forward loop models (illoc may be NULL; never together with snap) */
            rc = j->dev_border ? fdw_dev_extendvel_linear(ctx, (unsigned long long)is * (unsigned long long)j->draws, NULL) : FDW_OK;
            if (rc == FDW_OK)
                rc = fdw_shot_residual(ctx, j->dev_border ? NULL : j->vel2_all + (size_t)b * j->ne, j->sx[is], j->sz, j->gz, j->srce, d_obs, imloc, illoc,
                                       j->resloc_all + (size_t)b * j->nx * j->nt, NULL, NULL);
        } else if (is == j->snap_is) {      /* the worker that owns shot iss takes its frames (illoc may be NULL) */
            rc = j->dev_border ? fdw_dev_extendvel_linear(ctx, (unsigned long long)is * (unsigned long long)j->draws, NULL) : FDW_OK;
            if (rc == FDW_OK)
                rc = fdw_shot_snaps(ctx, j->dev_border ? NULL : j->vel2_all + (size_t)b * j->ne, j->sx[is], j->sz, j->gz, j->srce, d_obs, imloc, illoc,
                                    NULL, NULL, j->snaps);
        } else if (j->dev_border) {
            /* R:486-494 in HBM: shot `is` of the serial program consumes draws [is T, (is + 1) T) of the unseeded rand() stream */
            rc = fdw_dev_extendvel_linear(ctx, (unsigned long long)is * (unsigned long long)j->draws, NULL);
            if (rc == FDW_OK && illoc) rc = fdw_shot_resident_illum(ctx, j->sx[is], j->sz, j->gz, j->srce, d_obs, imloc, illoc, NULL, NULL);
            else if (rc == FDW_OK) rc = fdw_shot_resident(ctx, j->sx[is], j->sz, j->gz, j->srce, d_obs, imloc, NULL, NULL);
        } else if (illoc) {
            rc = fdw_shot_illum(ctx, j->vel2_all + (size_t)b * j->ne, j->sx[is], j->sz, j->gz, j->srce, d_obs, imloc, illoc, NULL, NULL);
        } else {
            rc = fdw_shot(ctx, j->vel2_all + (size_t)b * j->ne, j->sx[is], j->sz, j->gz, j->srce, d_obs, imloc, NULL, NULL);
        }
        if (rc != FDW_OK) {
            fprintf(stderr, "fdw_shot: %s\n", fdw_last_error());
            j->failed = 1;
        }
    }
    fdw_destroy(ctx);
    return NULL;
}

/* ---- slabs=N: every shot decomposed over N ranks (host threads, one GPU each) ---------------------------------------------- */
typedef struct {
    const fdw_params *prm;
    int world, local, ns, nx, nt, sz, gz;
    const int *sx;
    const float *srce, *d_obs;
    const float *v2;         /* the current shot's squared model [nxe][nze], built by rank 0 between the barriers */
    float *imloc;            /* the current shot's image [nx][nz]: every rank writes its own rows */
    char uid[FDW_COMM_ID_BYTES];
    fdw_comm **local_comms;
    pthread_barrier_t *bar;
    volatile int failed;
} slab_job;
typedef struct {
    slab_job *job;
    int rank;
    fdw_comm *comm;
    fdw_slabs *slabs;
} slab_rank;

/* Opening a rank is collective from ncclCommInitRank on (RCCL has no timeout: a rank that never arrives leaves the others waiting for
 * ever, holding their GPUs), so it goes in two phases with a barrier in between: first everything a rank can check ALONE -- its device
 * exists, is a gfx950 and can be selected --, then, only if no rank failed, the collective calls.  Every rank (the main thread included)
 * calls this exactly once and reaches both barriers. */
static int slab_rank_open(slab_rank *r)
{
    slab_job *j = r->job;
    int rc = j->local ? FDW_OK : fdw_device_usable(r->rank);                         /* rank r drives GPU r */
    if (rc != FDW_OK) {
        fprintf(stderr, "rank %d: %s\n", r->rank, fdw_last_error());
        j->failed = 1;
    }
    pthread_barrier_wait(j->bar);       /* O1: every rank has checked its device */
    if (!j->failed) {
        if (j->local) r->comm = j->local_comms[r->rank];
        else rc = fdw_comm_init_rank(j->uid, r->rank, j->world, r->rank, &r->comm);
        if (rc == FDW_OK) rc = fdw_slabs_create(j->prm, r->comm, 0, 0, &r->slabs);
        if (rc != FDW_OK) {
            fprintf(stderr, "rank %d: %s\n", r->rank, fdw_last_error());
            j->failed = 1;
        }
    }
    pthread_barrier_wait(j->bar);       /* O2: every rank is open (or the job has failed) */
    return j->failed ? FDW_ECOMM : FDW_OK;
}
static void slab_rank_shot(slab_rank *r, int is)
{
    slab_job *j = r->job;
    if (j->failed || !r->slabs) return;
    if (fdw_slabs_shot(r->slabs, j->v2, j->sx[is], j->sz, j->gz, j->srce, j->d_obs + (size_t)is * j->nx * j->nt, j->imloc, NULL, NULL) != FDW_OK) {
        fprintf(stderr, "rank %d, shot %d: %s\n", r->rank, is, fdw_last_error());
        j->failed = 1;
    }
}
static void *slab_rank_thread(void *p)      /* ranks 1 .. N-1; rank 0 is the main thread */
{
    slab_rank *r = (slab_rank *)p;
    slab_job *j = r->job;
    slab_rank_open(r);
    for (int is = 0; is < j->ns; is++) {
        pthread_barrier_wait(j->bar);       /* A: the shot's model is ready */
        slab_rank_shot(r, is);
        pthread_barrier_wait(j->bar);       /* B: every rank's rows of the image are in place */
    }
    if (r->slabs) fdw_slabs_destroy(r->slabs);
    if (r->comm) fdw_comm_destroy(r->comm);
    return NULL;
}

/* illum=1: dir.illum (the stacked illumination) and dir.image_illum (the compensated image) next to the outputs the key leaves untouched */
static int write_illum_outputs(const char *tmpdir, const float *img, const float *ill, size_t ni, float illum_eps)
{
    float *comp = (float *)malloc((ni ? ni : 1) * sizeof(float));
    FILE *fill = open_out(tmpdir, "dir.illum"), *fcomp = open_out(tmpdir, "dir.image_illum");
    if (!comp || !fill || !fcomp) return -1;
    if (fdw_image_compensate(img, ill, ni, illum_eps, comp) != FDW_OK) {
        fprintf(stderr, "fdw_image_compensate refused illum_eps=%g\n", (double)illum_eps);
        return -1;
    }
    fwrite(ill, sizeof(float), ni, fill);
    fwrite(comp, sizeof(float), ni, fcomp);
    fclose(fill);
    fclose(fcomp);
    free(comp);
    return 0;
}

/* pw=NP: the ray parameter of plane wave j, and its image stacked into img (and ill) and printed, exactly as the shot loop does per shot */
static double pw_ray(int pw, float pw_pmax, int j)
{
    return pw == 1 ? 0.0 : -(double)pw_pmax + 2.0 * (double)pw_pmax * (double)j / (double)(pw - 1);
}
static void pw_stack(FILE *fnum, int j, double p, int depth, int nx, int nz, float *img, const float *imloc, float *ill, const float *illoc)
{
    fprintf(stdout, "** plane wave %d, p = %g s/m, depth %d \n\n** backward propagation %d \n\n", j + 1, p, depth, j + 1);
    fprintf(fnum, "======== %i ========\n", j);
    for (int iz = 0; iz < nz; iz++)
        for (int ix = 0; ix < nx; ix++) {
            img[(size_t)ix * nz + iz] += imloc[(size_t)ix * nz + iz];
            fprintf(fnum, " %f \n", img[(size_t)ix * nz + iz]);
            if (ill) ill[(size_t)ix * nz + iz] += illoc[(size_t)ix * nz + iz];
        }
}

static double now_s(void)
{
    struct timeval t;
    gettimeofday(&t, NULL);
    return t.tv_sec + t.tv_usec * 1e-6;
}

int main(int argc, char **argv)
{
    struct timeval start, end;
    gettimeofday(&start, NULL);
    const int timing = getenv("FDW_TIMING") != NULL;   /* phase times on stderr */
    double t_shots = 0.0, t_stack = 0.0;
    const double t_begin = now_s();
    if (argc < 2) {
        fprintf(stderr, "usage: %s <input.dat>\n", argv[0]);
        return EXIT_FAILURE;
    }
    fdw_deck *deck = fdw_deck_read(argv[1]);
    if (!deck) return EXIT_FAILURE; /* F:51-52 */

    /* init_args, R:343-378 */
    const char *tmpdir = fdw_deck_str(deck, "tmpdir"), *vpfile = fdw_deck_str(deck, "vpfile");
    const char *datfile = fdw_deck_str(deck, "datfile"), *vel_ext_file = fdw_deck_str(deck, "vel_ext_file");
    const int nz = fdw_deck_int(deck, "nz"), nx = fdw_deck_int(deck, "nx"), nt = fdw_deck_int(deck, "nt");
    int ns = fdw_deck_int(deck, "ns"), sz = fdw_deck_int(deck, "sz"), fsx = fdw_deck_int(deck, "fsx");
    int ds = fdw_deck_int(deck, "ds"), gz = fdw_deck_int(deck, "gz"), order = fdw_deck_int(deck, "order");
    int nzb = fdw_deck_int(deck, "nzb"), nxb = fdw_deck_int(deck, "nxb"), iss = fdw_deck_int(deck, "iss");
    const int rnd = fdw_deck_int(deck, "rnd");
    const float dz = fdw_deck_float(deck, "dz"), dx = fdw_deck_float(deck, "dx"), dt = fdw_deck_float(deck, "dt");
    const float fpeak = fdw_deck_float(deck, "fpeak");
    float fac = fdw_deck_float(deck, "fac");
    const int vel_ext_flag = vel_ext_file != NULL;
    if (iss == -1) iss = 0;
    if (ns == -1) ns = 1;
    if (sz == -1) sz = 0;
    if (fsx == -1) fsx = 0;
    if (ds == -1) ds = 1;
    if (gz == -1) gz = 0;
    if (order == -1) order = 8;
    if (nzb == -1) nzb = 40;
    if (nxb == -1) nxb = 40;
    if (fac == -1.0f) fac = 0.7f;
    /* our extension (absent, -1 or 0: nothing changes): wavefield frames of shot iss every `snap` time levels, decimated by `snap_dec`.
     * Refused here, before any file, thread, communicator or device is touched */
    const int snap = fdw_deck_int(deck, "snap") > 0 ? fdw_deck_int(deck, "snap") : 0;
    const int snap_dec = fdw_deck_has(deck, "snap_dec") ? fdw_deck_int(deck, "snap_dec") : 1;
    if (snap_dec < 1) {
        fprintf(stderr, "snap_dec=%d: the decimation must be >= 1\n", snap_dec);
        return EXIT_FAILURE;
    }
    if (snap > 0) {
        int sl = fdw_deck_int(deck, "slabs");
        if (getenv("FDW_SLABS")) sl = atoi(getenv("FDW_SLABS"));
        if (sl > 1) {
            fprintf(stderr, "snap=%d cannot be combined with slabs=%d: slab-decomposed shots take no wavefield snapshots\n", snap, sl);
            return EXIT_FAILURE;
        }
        if (iss < 0 || iss >= ns) {
            fprintf(stderr, "snap=%d: iss=%d is not one of the %d shots\n", snap, iss, ns);
            return EXIT_FAILURE;
        }
    }
    /* our extension (absent or 0: nothing changes): source illumination and the compensated image.  Slab-decomposed shots do not
     * accumulate it: refused here, before any file, thread, communicator or device is touched */
    const int illum = fdw_deck_int(deck, "illum") == 1;
    float illum_eps = fdw_deck_float(deck, "illum_eps");
    if (illum_eps == -1.0f) illum_eps = 1.0e-3f;
    if (illum) {
        int sl = fdw_deck_int(deck, "slabs");
        if (getenv("FDW_SLABS")) sl = atoi(getenv("FDW_SLABS"));
        if (sl > 1) {
            fprintf(stderr, "illum=1 cannot be combined with slabs=%d: slab-decomposed shots do not accumulate the source illumination\n", sl);
            return EXIT_FAILURE;
        }
        if (!(illum_eps >= 0.0f) || illum_eps > 3.0e38f) {
            fprintf(stderr, "illum_eps=%g: must be finite and >= 0\n", (double)illum_eps);
            return EXIT_FAILURE;
        }
    }

    /* our extension (absent or 0: nothing changes): residual migration.  Slab-decomposed shots and the snapshot path do not cover it:
     * refused here, before any file, thread, communicator or device is touched */
    const int resid = fdw_deck_int(deck, "resid") == 1;
    if (resid) {
        int sl = fdw_deck_int(deck, "slabs");
        if (getenv("FDW_SLABS")) sl = atoi(getenv("FDW_SLABS"));
        if (sl > 1) {
            fprintf(stderr, "resid=1 cannot be combined with slabs=%d: slab-decomposed shots do not migrate data residuals\n", sl);
            return EXIT_FAILURE;
        }
        if (snap > 0) {
            fprintf(stderr, "resid=1 cannot be combined with snap=%d: the snapshot shot does not migrate a data residual\n", snap);
            return EXIT_FAILURE;
        }
    }

    /* our extension (absent: nothing changes): pw=NP plane-wave gathers migrated with a line source each instead of the ns shots.  One
     * context, one plane wave after the other: refused with the keys that deal shots out or change what a shot is, before any file, thread,
     * communicator or device is touched */
    const int pw = fdw_deck_has(deck, "pw") ? fdw_deck_int(deck, "pw") : 0;
    const float pw_pmax = fdw_deck_has(deck, "pw_pmax") ? fdw_deck_float(deck, "pw_pmax") : 0.0f;
    if (fdw_deck_has(deck, "pw")) {
        int sl = fdw_deck_int(deck, "slabs"), gp = fdw_deck_int(deck, "gpus");
        if (getenv("FDW_SLABS")) sl = atoi(getenv("FDW_SLABS"));
        if (getenv("FDW_GPUS")) gp = atoi(getenv("FDW_GPUS"));
        if (pw < 1) {
            fprintf(stderr, "pw=%d: the number of plane waves must be >= 1\n", pw);
            return EXIT_FAILURE;
        }
        if (!(pw_pmax >= 0.0f) || pw_pmax > 3.0e38f) {
            fprintf(stderr, "pw_pmax=%g: the largest ray parameter (s/m) must be finite and >= 0\n", (double)pw_pmax);
            return EXIT_FAILURE;
        }
        if (pw > 1 && pw_pmax == 0.0f) {
            fprintf(stderr, "pw=%d needs pw_pmax > 0: without it there is one plane wave (p = 0) only\n", pw);
            return EXIT_FAILURE;
        }
        if (sl > 1) {
            fprintf(stderr, "pw=%d cannot be combined with slabs=%d: slab-decomposed shots take no line source\n", pw, sl);
            return EXIT_FAILURE;
        }
        if (gp > 1) {
            fprintf(stderr, "pw=%d cannot be combined with gpus=%d: plane waves run one after another on one GPU\n", pw, gp);
            return EXIT_FAILURE;
        }
        if (resid) {
            fprintf(stderr, "pw=%d cannot be combined with resid=1: residual migration with a line source is not built\n", pw);
            return EXIT_FAILURE;
        }
        if (snap > 0) {
            fprintf(stderr, "pw=%d cannot be combined with snap=%d: the snapshot shot takes a point source\n", pw, snap);
            return EXIT_FAILURE;
        }
    }

    /* our extension (absent or 0: nothing changes): the excitation-amplitude imaging condition.  The shots in groups through
     * fdw_shot_excitation_batch / fdw_shot_excitation on one context: refused with every key that deals shots out or changes what a shot is, before any file, thread,
     * communicator or device is touched */
    const int exc = fdw_deck_int(deck, "exc") == 1;
    float exc_eps = fdw_deck_has(deck, "exc_eps") ? fdw_deck_float(deck, "exc_eps") : 1.0e-3f;
    if (exc) {
        int sl = fdw_deck_int(deck, "slabs"), gp = fdw_deck_int(deck, "gpus");
        if (getenv("FDW_SLABS")) sl = atoi(getenv("FDW_SLABS"));
        if (getenv("FDW_GPUS")) gp = atoi(getenv("FDW_GPUS"));
        const char *with = illum ? "illum=1" : (resid ? "resid=1" : (pw > 0 ? "pw" : (snap > 0 ? "snap" : (sl > 1 ? "slabs" : (gp > 1 ? "gpus" : NULL)))));
        if (with) {
            fprintf(stderr, "exc=1 cannot be combined with %s: the excitation-amplitude shot is a single point-source shot on one full-grid context\n", with);
            return EXIT_FAILURE;
        }
        if (!(exc_eps >= 0.0f) || exc_eps > 3.0e38f) {
            fprintf(stderr, "exc_eps=%g: must be finite and >= 0\n", (double)exc_eps);
            return EXIT_FAILURE;
        }
    }

    /* our extension (absent or 0: nothing changes): the DTT imaging condition.  The snapshot shot, the excitation shot and slab-decomposed
     * shots have no DTT form: refused before any file, thread, communicator or device is touched */
    const int dtt = fdw_deck_int(deck, "dtt") == 1;
    if (dtt) {
        int sl = fdw_deck_int(deck, "slabs");
        if (getenv("FDW_SLABS")) sl = atoi(getenv("FDW_SLABS"));
        const char *with = exc ? "exc=1" : (snap > 0 ? "snap" : (sl > 1 ? "slabs" : NULL));
        if (with) {
            fprintf(stderr, "dtt=1 cannot be combined with %s: DTT imaging is built for point- and line-source shots on one full-grid context, without snapshots\n",
                    with);
            return EXIT_FAILURE;
        }
    }

    /* our extension (absent or 0: nothing changes): least-squares migration, lsm=N conjugate-gradient iterations of fdw_lsm_solve on the
     * deck's shots (fdwave.h, "Least-squares migration").  The solve is one call on one full-grid context with point sources: refused with
     * every key that deals shots out, changes what a shot is or asks for another image, before any file, thread, communicator or device is
     * touched */
    const int lsm = fdw_deck_int(deck, "lsm") > 0 ? fdw_deck_int(deck, "lsm") : 0;
    const int lsm_mute = fdw_deck_has(deck, "lsm_mute") ? fdw_deck_int(deck, "lsm_mute") : 0;
    if (lsm > 0) {
        int sl = fdw_deck_int(deck, "slabs"), gp = fdw_deck_int(deck, "gpus");
        if (getenv("FDW_SLABS")) sl = atoi(getenv("FDW_SLABS"));
        if (getenv("FDW_GPUS")) gp = atoi(getenv("FDW_GPUS"));
        const char *with = exc ? "exc=1" : (snap > 0 ? "snap" : (sl > 1 ? "slabs" : (pw > 0 ? "pw" : (gp > 1 ? "gpus" : (illum ? "illum=1" : (resid ? "resid=1" : (dtt ? "dtt=1" : NULL)))))));
        if (with) {
            fprintf(stderr, "lsm=%d cannot be combined with %s: the least-squares solve runs point-source shots on one full-grid context and forms its own residuals and "
                            "DTT images; it has no snapshots, illumination, excitation image or slab / multi-GPU form\n", lsm, with);
            return EXIT_FAILURE;
        }
        if (lsm_mute < 0) {
            fprintf(stderr, "lsm_mute=%d: the number of muted interior columns must be >= 0\n", lsm_mute);
            return EXIT_FAILURE;
        }
    }

    /* our extension (absent or 0: nothing changes): ext=H, the subsurface-offset extended image of half-width H (fdwave.h, "Extended
     * imaging").  The shots go one by one through fdw_shot_ext on one full-grid context: refused with every key that deals shots out,
     * changes what a shot is or asks for another image, before any file, thread, communicator or device is touched */
    const int ext = fdw_deck_int(deck, "ext") > 0 ? fdw_deck_int(deck, "ext") : 0;
    if (ext > 0) {
        int sl = fdw_deck_int(deck, "slabs"), gp = fdw_deck_int(deck, "gpus");
        if (getenv("FDW_SLABS")) sl = atoi(getenv("FDW_SLABS"));
        if (getenv("FDW_GPUS")) gp = atoi(getenv("FDW_GPUS"));
        const char *with = exc ? "exc=1" : (dtt ? "dtt=1" : (lsm > 0 ? "lsm" : (pw > 0 ? "pw" : (sl > 1 ? "slabs" : (gp > 1 ? "gpus" : (snap > 0 ? "snap" : (resid ? "resid=1" : (illum ? "illum=1" : NULL))))))));
        if (with) {
            fprintf(stderr, "ext=%d cannot be combined with %s: the extended image is accumulated by single point-source cross-correlation shots on one full-grid "
                            "context; it has no batched, line-source, residual, DTT, excitation, snapshot, illumination or slab / multi-GPU form\n", ext, with);
            return EXIT_FAILURE;
        }
        if (ext > FDW_EXT_HMAX) {
            fprintf(stderr, "ext=%d: the half-width must lie in [0, %d]\n", ext, FDW_EXT_HMAX);
            return EXIT_FAILURE;
        }
    }

    printf("## vp = %s, d_obs = %s, vel_ext_file = %s, vel_ext_flag = %d \n", vpfile, datfile, vel_ext_file, vel_ext_flag);
    printf("## nz = %d, nx = %d, nt = %d \n", nz, nx, nt);
    printf("## dz = %f, dx = %f, dt = %f \n", dz, dx, dt);
    printf("## ns = %d, sz = %d, fsx = %d, ds = %d, gz = %d \n", ns, sz, fsx, ds, gz);
    printf("## order = %d, nzb = %d, nxb = %d, F = %f, rnd = %d \n", order, nzb, nxb, fac, rnd);
    int snap_nf = 0, snap_nxs = 0, snap_nzs = 0;
    if (snap > 0) {
        fdw_snap_dims(nx > 0 ? nx : 0, nz > 0 ? nz : 0, nt > 0 ? nt : 0, snap, snap_dec, &snap_nf, &snap_nxs, &snap_nzs);
        printf("## snap = %d, snap_dec = %d, iss = %d: %d frames of %d x %d in dir.snaps, dir.snaps_rec, dir.snapr \n", snap, snap_dec, iss, snap_nf,
               snap_nxs, snap_nzs);
    }
    if (dtt) printf("## dtt = 1: the image is formed with the second time difference of the source field (the adjoint of DTT Born modelling) \n");
    if (resid) printf("## resid = 1: every shot migrates d_obs minus the gather modelled in the migration model; dir.resid, dir.misfit \n");
    if (nz <= 0 || nx <= 0 || nt <= 0 || !tmpdir || !vpfile || !datfile) {
        fprintf(stderr, "input deck is missing one of tmpdir/vpfile/datfile/nz/nx/nt\n");
        return EXIT_FAILURE;
    }

    /* R:402-411 */
    float *srce = (float *)malloc((size_t)nt * sizeof(float));
    fdw_ricker_wavelet(nt, dt, fpeak, srce);
    int *sx = (int *)malloc((size_t)ns * sizeof(int));
    for (int is = 0; is < ns; is++) sx[is] = fsx + is * ds + nxb;
    sz += nzb;
    gz += nzb;
    const int nze = nz + 2 * nzb, nxe = nx + 2 * nxb;
    const size_t ne = (size_t)nxe * nze, ni = (size_t)nx * nz;

    float *vel_ext_rnd = NULL;
    if (vel_ext_flag && !(vel_ext_rnd = read_floats(vel_ext_file, ne * ns, "vel_ext_file"))) return EXIT_FAILURE; /* R:412-418 */
    float *d_obs = read_floats(datfile, (size_t)ns * nx * nt, "datfile");                                        /* R:420-424 */
    float *vp = read_floats(vpfile, ni, "vpfile");                                                               /* R:437-441 */
    if (!d_obs || !vp) return EXIT_FAILURE;
    float *vpe = (float *)calloc(ne, sizeof(float)); /* the reference leaves the border uninitialised (malloc) until extendvel */
    for (int ix = 0; ix < nx; ix++)
        for (int iz = 0; iz < nz; iz++) vpe[(size_t)(ix + nxb) * nze + iz + nzb] = vp[(size_t)ix * nz + iz]; /* R:445-449 */

    fdw_params prm;
    memset(&prm, 0, sizeof prm);
    prm.order = order; prm.nxe = nxe; prm.nze = nze; prm.nxb = nxb; prm.nzb = nzb; prm.nt = nt;
    prm.dx = dx; prm.dz = dz; prm.dt = dt; prm.fac = fac;
    prm.compat = 1;   /* the reference's launch extents, R:185-195 */
    prm.coef_cxx = 0; /* libsource.a is C, F:160-192 */
    {                 /* our extension, absent = the reference's arithmetic: numerics=1 (or FDW_NUMERICS=1) selects FAST numerics (fdwave.h) */
        int numerics = fdw_deck_int(deck, "numerics");
        if (getenv("FDW_NUMERICS")) numerics = atoi(getenv("FDW_NUMERICS"));
        prm.numerics = numerics == 1 ? FDW_NUMERICS_FAST : FDW_NUMERICS_EXACT;
        if (prm.numerics) printf("## numerics = FAST (symmetric sums + fused multiply-adds in the Laplacian; within 1e-5 of the reference's arithmetic)\n");
    }

    float *img = (float *)calloc(ni, sizeof(float)), *img_lap = (float *)calloc(ni, sizeof(float));
    FILE *fsns = open_out(tmpdir, "dir.snaps"), *fsns2 = open_out(tmpdir, "dir.snaps_rec"), *fsnr = open_out(tmpdir, "dir.snapr");
    FILE *fimg = open_out(tmpdir, "dir.image"), *fimg_lap = open_out(tmpdir, "dir.image_lap"); /* R:464-474 */
    FILE *fnum = fopen("image.num", "w");                                                       /* R:478-479 */
    if (!fimg || !fimg_lap || !fnum) return EXIT_FAILURE;
    FILE *fres = resid ? open_out(tmpdir, "dir.resid") : NULL, *fmis = resid ? open_out(tmpdir, "dir.misfit") : NULL;
    double *misfit = resid ? (double *)calloc((size_t)ns, sizeof(double)) : NULL;
    if (resid && (!fres || !fmis || !misfit)) return EXIT_FAILURE;

    /* Shots are independent (R:480-529 only couples them through the running image sum), and a shot of a deck this size fills a
     * few percent of an MI355X: up to FDW_SHOT_WORKERS (default 4) host threads, each with its own context and stream, propagate
     * shots side by side.  What must stay serial does: the border model draws from ONE rand() stream in shot order (R:486), so all
     * squared-velocity models are built first, and the images are stacked (and image.num written) in shot order afterwards. */
    /* The border model itself is generated on the device from the resident interior model (fdw_dev_extendvel_linear: the rand() stream is
     * addressed by position, so no worker waits for another's draws); FDW_HOST_BORDER=1 or a geometry the device path refuses (a one-cell
     * border) keeps the host loop below. */
    int slabs = fdw_deck_int(deck, "slabs"), gpus = fdw_deck_int(deck, "gpus");      /* our extensions; absent = -1 */
    if (getenv("FDW_SLABS")) slabs = atoi(getenv("FDW_SLABS"));
    if (getenv("FDW_GPUS")) gpus = atoi(getenv("FDW_GPUS"));
    if (slabs > 64 || gpus > 64) {
        fprintf(stderr, "slabs / gpus: at most 64\n");
        return EXIT_FAILURE;
    }
    int shots_per_launch = 1;      /* FDW_TIMING: how many shots advance through one launch per time step */
    if (pw > 0) {
        /* ---- pw=NP: NP encoded gathers, each migrated with a delayed line of sources (fdw_shot_line).  On decks where shots batch
         * (fdw_shot_batch_max > 1) the plane waves do too: all data gathers encoded in one pass (fdw_encode_gathers_multi), the line gathers
         * and the models built in the order j, then fdw_shot_batch_max plane waves per launch sequence (fdw_shot_line_batch); stacked
         * and printed in the order j either way.  FDW_NO_SHOT_BATCH=1 keeps one plane wave after the other. ---- */
        const int dev_models = !vel_ext_flag && !getenv("FDW_HOST_BORDER") && nxb != 1 && nzb != 1 && nzb <= nxe;      /* as dev_border below */
        const long long draws = fdw_border_draws(nx, nz, nxb, nzb);
        const size_t ng = (size_t)nx * nt;
        fdw_ctx *ctx = NULL;
        int *src_ix = (int *)malloc((size_t)ns * sizeof(int));
        float *ill = illum ? (float *)calloc(ni, sizeof(float)) : NULL;
        if (!src_ix || (illum && !ill)) {
            fprintf(stderr, "out of host memory\n");
            return EXIT_FAILURE;
        }
        for (int is = 0; is < ns; is++) src_ix[is] = fsx + is * ds;
        if (fdw_create(&prm, 0, &ctx) != FDW_OK || (dev_models && fdw_model_resident(ctx, vp) != FDW_OK)) {
            fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
            return EXIT_FAILURE;
        }
        int pw_bmax = (pw > 1 && !getenv("FDW_NO_SHOT_BATCH")) ? fdw_shot_batch_max(ctx) : 1;
        if (pw_bmax > pw) pw_bmax = pw;
        shots_per_launch = pw_bmax;
        const int nb = pw_bmax > 1 ? pw : 1;      /* plane waves held on the host at a time */
        int *lag = (int *)malloc((size_t)nb * ns * sizeof(int));
        float *weight = (float *)malloc((size_t)nb * ns * sizeof(float)), *wav = (float *)malloc((size_t)nb * ng * sizeof(float));
        float *enc = (float *)malloc((size_t)nb * ng * sizeof(float)), *imloc = (float *)calloc((size_t)nb * ni, sizeof(float));
        float *v2 = (float *)malloc((dev_models ? 1 : (size_t)nb) * ne * sizeof(float)), *illoc = illum ? (float *)calloc((size_t)nb * ni, sizeof(float)) : NULL;
        if (!lag || !weight || !wav || !enc || !v2 || !imloc || (illum && !illoc)) {
            fprintf(stderr, "out of host memory\n");
            return EXIT_FAILURE;
        }
        for (size_t k = 0; k < (size_t)nb * ns; k++) weight[k] = 1.0f;
        const double t0 = now_s();
        for (int j = 0; j < pw; j++) {
            const int slot = pw_bmax > 1 ? j : 0;
            const double p = pw_ray(pw, pw_pmax, j);
            if (fdw_planewave_lags(ns, src_ix, dx, dt, p, lag + (size_t)slot * ns) != FDW_OK ||
                fdw_encode_line_source(ns, src_ix, lag + (size_t)slot * ns, weight, srce, nt, nx, wav + (size_t)slot * ng) != FDW_OK) {
                fprintf(stderr, "plane wave %d (p = %g s/m): the shot rows fsx + is ds must lie in [0, nx) and the lags p (row - first row) dx / dt must be finite\n",
                        j + 1, p);
                return EXIT_FAILURE;
            }
            const float *model = NULL;      /* NULL: the squared model drawn in HBM */
            if (!dev_models) {
                const float *v = vpe;
                float *dst = v2 + (size_t)slot * ne;
                if (vel_ext_flag) v = vel_ext_rnd + (size_t)(j % ns) * ne;      /* R:484 */
                else fdw_extendvel_linear(nx, nz, nxb, nzb, vpe);               /* R:486: the next draws of the one stream, in the order j */
                for (size_t k = 0; k < ne; k++) dst[k] = v[k] * v[k];            /* R:490-494 */
                model = dst;
            }
            if (pw_bmax > 1) continue;      /* batched: migrated below */
            int rc = fdw_encode_gathers(0, ns, lag, weight, d_obs, nx, nt, enc);
            if (rc == FDW_OK && dev_models)
                rc = fdw_dev_extendvel_linear(ctx, (unsigned long long)j * (unsigned long long)draws, NULL);      /* R:486: the next draw of the stream */
            memset(imloc, 0, ni * sizeof(float));                                /* R:515 */
            if (illum) memset(illoc, 0, ni * sizeof(float));
            if (rc == FDW_OK)
                rc = dtt ? fdw_shot_line_dtt(ctx, model, sz, gz, wav, enc, imloc, illoc, 0, NULL, NULL, NULL)
                         : fdw_shot_line(ctx, model, sz, gz, wav, enc, imloc, illoc, NULL, NULL);
            if (rc != FDW_OK) {
                fprintf(stderr, "plane wave %d: %s\n", j + 1, fdw_last_error());
                return EXIT_FAILURE;
            }
            pw_stack(fnum, j, p, sz - nzb, nx, nz, img, imloc, ill, illoc);
        }
        if (pw_bmax > 1) {
            int rc = fdw_encode_gathers_multi(0, ns, pw, lag, weight, d_obs, nx, nt, enc);
            for (int j0 = 0; rc == FDW_OK && j0 < pw; j0 += pw_bmax) {
                const int n = pw - j0 < pw_bmax ? pw - j0 : pw_bmax;
                const float *models = dev_models ? NULL : v2 + (size_t)j0 * ne;
                const unsigned long long draw0 = (unsigned long long)j0 * (unsigned long long)draws;
                float *il = illum ? illoc + (size_t)j0 * ni : NULL;
                rc = dtt ? fdw_shot_line_batch_dtt(ctx, n, models, draw0, sz, gz, wav + (size_t)j0 * ng, enc + (size_t)j0 * ng, imloc + (size_t)j0 * ni, il, 0, NULL)
                         : fdw_shot_line_batch(ctx, n, models, draw0, sz, gz, wav + (size_t)j0 * ng, enc + (size_t)j0 * ng, imloc + (size_t)j0 * ni, il);
            }
            if (rc != FDW_OK) {
                fprintf(stderr, "fdw_shot_line_batch: %s\n", fdw_last_error());
                return EXIT_FAILURE;
            }
            for (int j = 0; j < pw; j++)
                pw_stack(fnum, j, pw_ray(pw, pw_pmax, j), sz - nzb, nx, nz, img, imloc + (size_t)j * ni, ill, illum ? illoc + (size_t)j * ni : NULL);
        }
        t_shots = now_s() - t0;
        fdw_destroy(ctx);
        if (illum && write_illum_outputs(tmpdir, img, ill, ni, illum_eps) != 0) return EXIT_FAILURE;
        free(src_ix); free(lag); free(weight); free(wav); free(enc); free(v2); free(imloc); free(illoc); free(ill);
        goto outputs;
    }
    if (lsm > 0) {
        /* ---- lsm=N: dir.image = the model after N conjugate-gradient iterations from zero (fdw_lsm_solve with the verify pass); the mask is
         * zero on the interior columns iz < lsm_mute.  <tmpdir>/dir.lsm_misfit: N + 2 doubles, the misfit history and last the recomputed
         * misfit.  Border models as everywhere: drawn on the device per shot, or built here in shot order. ---- */
        const int dev_models = !vel_ext_flag && !getenv("FDW_HOST_BORDER") && nxb != 1 && nzb != 1 && nzb <= nxe;      /* as dev_border below */
        fdw_ctx *ctx = NULL;
        if (fdw_create(&prm, 0, &ctx) != FDW_OK || (dev_models && fdw_model_resident(ctx, vp) != FDW_OK)) {
            fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
            return EXIT_FAILURE;
        }
        float *v2 = dev_models ? NULL : (float *)malloc((size_t)ns * ne * sizeof(float)), *mask = lsm_mute > 0 ? (float *)malloc(ni * sizeof(float)) : NULL;
        double *hist = (double *)calloc((size_t)lsm + 2, sizeof(double));
        FILE *fh = open_out(tmpdir, "dir.lsm_misfit");
        if ((!dev_models && !v2) || (lsm_mute > 0 && !mask) || !hist || !fh) {
            fprintf(stderr, "out of host memory, or cannot open dir.lsm_misfit\n");
            return EXIT_FAILURE;
        }
        for (int is = 0; is < ns && !dev_models; is++) {
            const float *v = vpe;
            if (vel_ext_flag) v = vel_ext_rnd + (size_t)is * ne;      /* R:484 */
            else fdw_extendvel_linear(nx, nz, nxb, nzb, vpe);        /* R:486: the next draws of the one stream, in shot order */
            for (size_t k = 0; k < ne; k++) v2[(size_t)is * ne + k] = v[k] * v[k];      /* R:490-494 */
        }
        for (int ix = 0; ix < nx && mask; ix++)
            for (int iz = 0; iz < nz; iz++) mask[(size_t)ix * nz + iz] = iz < lsm_mute ? 0.0f : 1.0f;
        printf("## lsm = %d, lsm_mute = %d: least-squares migration, conjugate gradients on DTT Born modelling and DTT imaging; dir.lsm_misfit \n", lsm, lsm_mute);
        const double t0 = now_s();
        if (fdw_lsm_solve(ctx, ns, v2, 0, sx[0], ds, sz, gz, srce, d_obs, mask, lsm, img, hist, 1, NULL) != FDW_OK) {
            fprintf(stderr, "fdw_lsm_solve: %s\n", fdw_last_error());
            return EXIT_FAILURE;
        }
        t_shots = now_s() - t0;
        shots_per_launch = fdw_batch_parts(ctx) > 0 ? (ns + fdw_batch_parts(ctx) - 1) / fdw_batch_parts(ctx) : 1;
        for (int k = 0; k <= lsm; k++) printf("## lsm: misfit after %d iterations = %.9e \n", k, hist[k]);
        printf("## lsm: recomputed misfit = %.9e \n", hist[lsm + 1]);
        fprintf(fnum, "======== %i ========\n", 0);
        for (int iz = 0; iz < nz; iz++)
            for (int ix = 0; ix < nx; ix++) fprintf(fnum, " %f \n", img[(size_t)ix * nz + iz]);
        if (fwrite(hist, sizeof(double), (size_t)lsm + 2, fh) != (size_t)lsm + 2 || fclose(fh) != 0) {
            fprintf(stderr, "cannot write dir.lsm_misfit\n");
            return EXIT_FAILURE;
        }
        fdw_destroy(ctx);
        free(v2); free(mask); free(hist);
        goto outputs;
    }
    if (ext > 0) {
        /* ---- ext=H: the shots one by one through fdw_shot_ext on one context, every shot accumulating into the same 2H+1 planes;
         * <tmpdir>/dir.image_ext is [2H+1][nx][nz], the shots stacked in shot order.  dir.image, dir.image_lap and image.num are what the
         * run without the key writes: each shot's image from zero, added to the running sum on the host.  Border models as everywhere. ---- */
        const int dev_models = !vel_ext_flag && !getenv("FDW_HOST_BORDER") && nxb != 1 && nzb != 1 && nzb <= nxe;      /* as dev_border below */
        const long long draws = fdw_border_draws(nx, nz, nxb, nzb);
        const size_t np = (size_t)(2 * ext + 1) * ni;
        fdw_ctx *ctx = NULL;
        if (fdw_create(&prm, 0, &ctx) != FDW_OK || (dev_models && fdw_model_resident(ctx, vp) != FDW_OK)) {
            fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
            return EXIT_FAILURE;
        }
        float *v2 = dev_models ? NULL : (float *)malloc(ne * sizeof(float)), *imloc = (float *)malloc(ni * sizeof(float));
        float *eimg = (float *)calloc(np, sizeof(float));
        FILE *fext = open_out(tmpdir, "dir.image_ext");
        if ((!dev_models && !v2) || !imloc || !eimg || !fext) {
            fprintf(stderr, "out of host memory, or cannot open dir.image_ext\n");
            return EXIT_FAILURE;
        }
        printf("## ext = %d: subsurface-offset extended image, %d planes of %d x %d in dir.image_ext \n", ext, 2 * ext + 1, nx, nz);
        const double t0 = now_s();
        for (int is = 0; is < ns; is++) {
            int rc = FDW_OK;
            if (dev_models) {
                rc = fdw_dev_extendvel_linear(ctx, (unsigned long long)is * (unsigned long long)draws, NULL);      /* R:486: the next draw of the stream */
            } else {
                const float *v = vpe;
                if (vel_ext_flag) v = vel_ext_rnd + (size_t)is * ne;      /* R:484 */
                else fdw_extendvel_linear(nx, nz, nxb, nzb, vpe);        /* R:486: the next draws of the one stream, in shot order */
                for (size_t k = 0; k < ne; k++) v2[k] = v[k] * v[k];      /* R:490-494 */
            }
            memset(imloc, 0, ni * sizeof(float));                        /* R:515 */
            if (rc == FDW_OK) rc = fdw_shot_ext(ctx, v2, sx[is], sz, gz, srce, d_obs + (size_t)is * nx * nt, ext, imloc, eimg, NULL, NULL);
            if (rc != FDW_OK) {
                fprintf(stderr, "shot %d: %s\n", is + 1, fdw_last_error());
                return EXIT_FAILURE;
            }
            fprintf(stdout, "** source %d, at (%d,%d) \n", is + 1, sx[is] - nxb, sz - nzb);
            fprintf(stdout, "\n");
            fprintf(stdout, "** backward propagation %d, at (%d,%d) \n", is + 1, sx[is] - nxb, sz - nzb);
            fprintf(stdout, "\n");
            fprintf(fnum, "======== %i ========\n", is); /* R:522-528: iz outer, ix inner, running sum */
            for (int iz = 0; iz < nz; iz++)
                for (int ix = 0; ix < nx; ix++) {
                    img[(size_t)ix * nz + iz] += imloc[(size_t)ix * nz + iz];
                    fprintf(fnum, " %f \n", img[(size_t)ix * nz + iz]);
                }
        }
        t_shots = now_s() - t0;
        if (fwrite(eimg, sizeof(float), np, fext) != np || fclose(fext) != 0) {
            fprintf(stderr, "cannot write dir.image_ext\n");
            return EXIT_FAILURE;
        }
        fdw_destroy(ctx);
        free(v2); free(imloc); free(eimg);
        goto outputs;
    }
    if (exc) {
        /* ---- exc=1: the shots in groups of fdw_shot_batch_max on one context.  A group of several shots goes through
         * fdw_shot_excitation_batch (one launch per time step for all of them; the running image after each shot comes back in `stack`), a
         * group of one through fdw_shot_excitation; either way the image of each shot is added to img in shot order on the device and
         * image.num has one section per shot as always.  FDW_NO_SHOT_BATCH=1 keeps one shot per launch sequence. ---- */
        const int dev_models = !vel_ext_flag && !getenv("FDW_HOST_BORDER") && nxb != 1 && nzb != 1 && nzb <= nxe;      /* as dev_border below */
        const long long draws = fdw_border_draws(nx, nz, nxb, nzb);
        fdw_ctx *ctx = NULL;
        if (fdw_create(&prm, 0, &ctx) != FDW_OK || (dev_models && fdw_model_resident(ctx, vp) != FDW_OK)) {
            fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
            return EXIT_FAILURE;
        }
        int bmax = (ns > 1 && !getenv("FDW_NO_SHOT_BATCH")) ? fdw_shot_batch_max(ctx) : 1;
        if (bmax > ns) bmax = ns;
        shots_per_launch = bmax;
        float *v2 = (float *)malloc((size_t)bmax * ne * sizeof(float)), *stack = (float *)malloc((size_t)bmax * ni * sizeof(float));
        if (!v2 || !stack) {
            fprintf(stderr, "out of host memory\n");
            return EXIT_FAILURE;
        }
        printf("## exc = 1, exc_eps = %g: excitation-amplitude imaging, image += exc / amp per shot \n", (double)exc_eps);
        printf("## exc: up to %d shots per launch sequence (%s) \n", bmax, bmax > 1 ? "fdw_shot_excitation_batch" : "fdw_shot_excitation, one by one");
        const double t0 = now_s();
        for (int is0 = 0; is0 < ns; is0 += bmax) {
            const int nb = is0 + bmax <= ns ? bmax : ns - is0;
            int rc = FDW_OK;
            for (int b = 0; b < nb && !dev_models; b++) {
                const float *v = vpe;
                if (vel_ext_flag) v = vel_ext_rnd + (size_t)(is0 + b) * ne;      /* R:484 */
                else fdw_extendvel_linear(nx, nz, nxb, nzb, vpe);               /* R:486: the next draws of the one stream, in shot order */
                for (size_t k = 0; k < ne; k++) v2[(size_t)b * ne + k] = v[k] * v[k];      /* R:490-494 */
            }
            const unsigned long long draw0 = (unsigned long long)is0 * (unsigned long long)draws;
            const float *gathers = d_obs + (size_t)is0 * nx * nt;
            if (nb > 1) {
                rc = fdw_shot_excitation_batch(ctx, nb, dev_models ? NULL : v2, draw0, sx[is0], ds, sz, gz, srce, gathers, exc_eps, img, stack, NULL, NULL,
                                               NULL);
            } else {
                if (dev_models) rc = fdw_dev_extendvel_linear(ctx, draw0, NULL);      /* the squared model drawn in HBM */
                if (rc == FDW_OK) rc = fdw_shot_excitation(ctx, dev_models ? NULL : v2, sx[is0], sz, gz, srce, gathers, exc_eps, img, NULL, NULL, NULL, NULL, NULL);
            }
            if (rc != FDW_OK) {
                fprintf(stderr, "shots %d..%d: %s\n", is0 + 1, is0 + nb, fdw_last_error());
                return EXIT_FAILURE;
            }
            for (int b = 0; b < nb; b++) {
                const int is = is0 + b;
                const float *run = nb > 1 ? stack + (size_t)b * ni : img;      /* the running image after shot is */
                fprintf(stdout, "** source %d, at (%d,%d) \n\n** backward propagation %d, at (%d,%d) \n\n", is + 1, sx[is] - nxb, sz - nzb, is + 1, sx[is] - nxb,
                        sz - nzb);
                fprintf(fnum, "======== %i ========\n", is);
                for (int iz = 0; iz < nz; iz++)
                    for (int ix = 0; ix < nx; ix++) fprintf(fnum, " %f \n", run[(size_t)ix * nz + iz]);
            }
        }
        free(stack);
        t_shots = now_s() - t0;
        fdw_destroy(ctx);
        free(v2);
        goto outputs;
    }
    if (slabs > 1) {
        /* ---- every shot on `slabs` GPUs: bands of rows, halo exchange inside the library ---- */
        slab_job sj;
        memset(&sj, 0, sizeof sj);
        sj.local = getenv("FDW_SLABS_LOCAL") != NULL;
        const int ndev = fdw_device_count();
        if (ndev < 1 || (!sj.local && slabs > ndev)) {      /* before any thread or communicator exists: RCCL would wait for the missing ranks for ever */
            fprintf(stderr, "slabs=%d needs %d GPUs, one rank each; %d visible%s\n", slabs, slabs, ndev < 0 ? 0 : ndev,
                    ndev >= 1 ? " (FDW_SLABS_LOCAL=1 runs the ranks as threads sharing GPU 0: rehearsals only)" : "");
            return EXIT_FAILURE;
        }
        sj.prm = &prm; sj.world = slabs; sj.ns = ns; sj.nx = nx; sj.nt = nt; sj.sz = sz; sj.gz = gz;
        sj.sx = sx; sj.srce = srce; sj.d_obs = d_obs;
        float *v2 = (float *)malloc(ne * sizeof(float)), *imloc = (float *)calloc(ni, sizeof(float));
        fdw_comm *lc[64];
        pthread_barrier_t bar;
        pthread_t th[64];
        slab_rank rk[64];
        if (!v2 || !imloc || pthread_barrier_init(&bar, NULL, (unsigned)slabs) != 0) return EXIT_FAILURE;
        sj.imloc = imloc; sj.v2 = v2; sj.bar = &bar; sj.local_comms = lc;
        if ((sj.local ? fdw_comm_init_local(slabs, NULL, lc) : fdw_comm_get_unique_id(sj.uid)) != FDW_OK) {
            fprintf(stderr, "communicator: %s\n", fdw_last_error());
            return EXIT_FAILURE;
        }
        for (int r = 0; r < slabs; r++) {
            memset(&rk[r], 0, sizeof rk[r]);
            rk[r].job = &sj; rk[r].rank = r;
            if (r > 0 && pthread_create(&th[r], NULL, slab_rank_thread, &rk[r]) != 0) return EXIT_FAILURE;
        }
        slab_rank_open(&rk[0]);
        for (int is = 0; is < ns; is++) {
            const float *v = vpe;
            if (vel_ext_flag) v = vel_ext_rnd + (size_t)is * ne;      /* R:484 */
            else fdw_extendvel_linear(nx, nz, nxb, nzb, vpe);         /* R:486 */
            for (size_t k = 0; k < ne; k++) v2[k] = v[k] * v[k];      /* R:490-494 */
            memset(imloc, 0, ni * sizeof(float));                     /* R:515 */
            pthread_barrier_wait(&bar);
            slab_rank_shot(&rk[0], is);
            pthread_barrier_wait(&bar);
            fprintf(stdout, "** source %d, at (%d,%d) \n\n** backward propagation %d, at (%d,%d) \n\n", is + 1, sx[is] - nxb, sz - nzb, is + 1, sx[is] - nxb, sz - nzb);
            fprintf(fnum, "======== %i ========\n", is);
            for (int iz = 0; iz < nz; iz++)
                for (int ix = 0; ix < nx; ix++) {
                    img[(size_t)ix * nz + iz] += imloc[(size_t)ix * nz + iz];
                    fprintf(fnum, " %f \n", img[(size_t)ix * nz + iz]);
                }
        }
        for (int r = 1; r < slabs; r++) pthread_join(th[r], NULL);
        if (rk[0].slabs) fdw_slabs_destroy(rk[0].slabs);
        if (rk[0].comm) fdw_comm_destroy(rk[0].comm);
        pthread_barrier_destroy(&bar);
        free(v2); free(imloc);
        if (sj.failed) return EXIT_FAILURE;
        goto outputs;
    }
    const int dev_border = !vel_ext_flag && !getenv("FDW_HOST_BORDER") && nxb != 1 && nzb != 1 && nzb <= nxe;
    int nworkers = 4;
    if (getenv("FDW_SHOT_WORKERS")) nworkers = atoi(getenv("FDW_SHOT_WORKERS"));
    if (nworkers < 1) nworkers = 1;
    if (gpus > 1 && nworkers < gpus) nworkers = gpus;      /* at least one worker per GPU */
    if (nworkers > ns) nworkers = ns;
    if (nworkers > 64) nworkers = 64;
    while (nworkers > 1 && (size_t)ns * (ne + ni) * sizeof(float) > ((size_t)8 << 30)) nworkers = 1;   /* big decks: one shot fills the GPU anyway */
    /* Small decks: a whole batch of shots advances through ONE launch per time step (fdw_shot_batch; the library says how many shots fill
     * the chip for this geometry, 1 = the grid is big enough by itself).  FDW_NO_SHOT_BATCH=1 keeps one shot per launch sequence. */
    fdw_ctx *bctx = NULL;
    int bmax = 1;
    if (ns > 1 && !getenv("FDW_NO_SHOT_BATCH") && gpus <= 1) {      /* (shots dealt to several GPUs go one context per worker instead) */
        if (fdw_create(&prm, 0, &bctx) != FDW_OK) {
            fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
            return EXIT_FAILURE;
        }
        bmax = fdw_shot_batch_max(bctx);
        if (bmax > ns) bmax = ns;
        if (bmax > 1 && dev_border && fdw_model_resident(bctx, vp) != FDW_OK) {
            fprintf(stderr, "fdw_model_resident: %s\n", fdw_last_error());
            return EXIT_FAILURE;
        }
        if (bmax <= 1) {
            fdw_destroy(bctx);
            bctx = NULL;
        }
    }
    const int batch = bctx ? bmax : (nworkers > 1 ? ns : 1);      /* shots whose model and image are held at once */
    if (bctx) shots_per_launch = bmax;
    float *vel2_all = (float *)malloc((size_t)batch * ne * sizeof(float)), *imloc_all = (float *)calloc((size_t)batch * ni, sizeof(float));
    float *illoc_all = illum ? (float *)calloc((size_t)batch * ni, sizeof(float)) : NULL, *ill = illum ? (float *)calloc(ni, sizeof(float)) : NULL;
    const size_t ng = (size_t)nx * nt;
    float *resloc_all = resid ? (float *)calloc((size_t)batch * ng, sizeof(float)) : NULL;
    if (!vel2_all || !imloc_all || (illum && (!illoc_all || !ill)) || (resid && !resloc_all)) {
        fprintf(stderr, "out of host memory\n");
        return EXIT_FAILURE;
    }
    shot_job job;
    job.prm = &prm; job.ns = ns; job.nworkers = nworkers; job.sx = sx; job.sz = sz; job.gz = gz; job.srce = srce; job.d_obs = d_obs;
    job.nx = nx; job.nt = nt; job.ne = ne; job.ni = ni; job.vel2_all = vel2_all; job.imloc_all = imloc_all; job.illoc_all = illoc_all; job.failed = 0;
    job.resid = resid; job.resloc_all = resloc_all; job.dtt = dtt;
    job.vp = vp; job.draws = fdw_border_draws(nx, nz, nxb, nzb); job.dev_border = dev_border; job.gpus = gpus;
    if (gpus > 1) {      /* more GPUs asked for than visible: the workers share the visible ones, as in rtm_model (the bytes do not depend on where a shot runs) */
        const int ndev = fdw_device_count();
        if (ndev >= 1 && gpus > ndev) {
            fprintf(stderr, "gpus=%d: %d visible; the %d workers share %s\n", gpus, ndev, nworkers, ndev == 1 ? "it" : "them");
            job.gpus = ndev;
        }
    }
    /* snap=K: the three frame sets of shot iss, on the host until they are written */
    const size_t snap_n = (size_t)snap_nf * snap_nxs * snap_nzs;
    fdw_snaps sn;
    memset(&sn, 0, sizeof sn);
    sn.every = snap; sn.dec = snap_dec;
    if (snap > 0) {
        sn.snaps = (float *)calloc(snap_n ? snap_n : 1, sizeof(float));
        sn.snaps_rec = (float *)calloc(snap_n ? snap_n : 1, sizeof(float));
        sn.snapr = (float *)calloc(snap_n ? snap_n : 1, sizeof(float));
        if (!sn.snaps || !sn.snaps_rec || !sn.snapr) {
            fprintf(stderr, "out of host memory\n");
            return EXIT_FAILURE;
        }
    }
    job.snap_is = snap > 0 ? iss : -1; job.snaps = &sn;

    for (int is0 = 0; is0 < ns; is0 += batch) {
        const int nb = is0 + batch <= ns ? batch : ns - is0;
        for (int b = 0; b < nb && !dev_border; b++) { /* models in shot order: the rand() stream is sequential */
            const int is = is0 + b;
            const float *v = vpe;
            if (vel_ext_flag)
                v = vel_ext_rnd + (size_t)is * ne; /* R:484 */
            else
                fdw_extendvel_linear(nx, nz, nxb, nzb, vpe); /* R:486: glibc rand(), never seeded */
            float *v2 = vel2_all + (size_t)b * ne;
            for (size_t k = 0; k < ne; k++) v2[k] = v[k] * v[k]; /* R:490-494 */
        }
        const double t0 = now_s();
        job.is0 = is0; job.nb = nb;
        memset(imloc_all, 0, (size_t)nb * ni * sizeof(float));                                 /* R:515 */
        if (illum) memset(illoc_all, 0, (size_t)nb * ni * sizeof(float));                      /* per shot from zero */
        if (bctx) {
            /* shots is0 .. is0 + nb - 1: source rows sx[is0] + b ds (R:405-407), border models from draws [(is0 + b) T, ...) of the stream */
            /* models: drawn on the device, or the host-built ones of this batch (vel_ext_file decks, FDW_HOST_BORDER=1) */
            /* snap=K: shot iss leaves the batch and runs alone through fdw_shot_snaps; the shots before and after it batch as they did */
            for (int b0 = 0; b0 < nb;) {
                const int isb = is0 + b0;
                const int n = isb == job.snap_is ? 1 : (job.snap_is > isb && job.snap_is < is0 + nb ? job.snap_is - isb : nb - b0);
                const unsigned long long draw0 = (unsigned long long)isb * (unsigned long long)job.draws;
                const float *models = dev_border ? NULL : vel2_all + (size_t)b0 * ne, *gathers = d_obs + (size_t)isb * nx * nt;
                float *im = imloc_all + (size_t)b0 * ni, *il = illum ? illoc_all + (size_t)b0 * ni : NULL;
                int rc;
                if (dtt) {
                    rc = fdw_shot_batch_dtt(bctx, n, models, draw0, sx[isb], ds, sz, gz, srce, gathers, im, il, resid, resid ? resloc_all + (size_t)b0 * ng : NULL);
                } else if (resid) {
                    rc = fdw_shot_batch_residual(bctx, n, models, draw0, sx[isb], ds, sz, gz, srce, gathers, im, il, resloc_all + (size_t)b0 * ng);
                } else if (isb == job.snap_is) {
                    rc = dev_border ? fdw_dev_extendvel_linear(bctx, draw0, NULL) : FDW_OK;
                    if (rc == FDW_OK) rc = fdw_shot_snaps(bctx, models, sx[isb], sz, gz, srce, gathers, im, il, NULL, NULL, &sn);
                } else {
                    rc = illum ? fdw_shot_batch_illum(bctx, n, models, draw0, sx[isb], ds, sz, gz, srce, gathers, im, il)
                               : fdw_shot_batch(bctx, n, models, draw0, sx[isb], ds, sz, gz, srce, gathers, im);
                }
                if (rc != FDW_OK) {
                    fprintf(stderr, "fdw_shot_batch: %s\n", fdw_last_error());
                    return EXIT_FAILURE;
                }
                b0 += n;
            }
        } else {
            const int nw = nb < nworkers ? nb : nworkers;
            pthread_t th[64];
            shot_worker_arg wa[64];
            for (int w = 0; w < nw; w++) {
                wa[w].job = &job; wa[w].w = w; wa[w].nw = nw;
                if (w > 0 && pthread_create(&th[w], NULL, shot_worker, &wa[w]) != 0) {
                    fprintf(stderr, "pthread_create failed\n");
                    return EXIT_FAILURE;
                }
            }
            shot_worker(&wa[0]);
            for (int w = 1; w < nw; w++) pthread_join(th[w], NULL);
            if (job.failed) return EXIT_FAILURE;
        }
        const double t1 = now_s();
        t_shots += t1 - t0;
        for (int b = 0; b < nb; b++) {               /* R:480-529 in shot order */
            const int is = is0 + b;
            const float *imloc = imloc_all + (size_t)b * ni;
            fprintf(stdout, "** source %d, at (%d,%d) \n", is + 1, sx[is] - nxb, sz - nzb);
            fprintf(stdout, "\n");
            fprintf(stdout, "** backward propagation %d, at (%d,%d) \n", is + 1, sx[is] - nxb, sz - nzb);
            fprintf(stdout, "\n");
            fprintf(fnum, "======== %i ========\n", is); /* R:522-528: iz outer, ix inner, running sum */
            for (int iz = 0; iz < nz; iz++)
                for (int ix = 0; ix < nx; ix++) {
                    img[(size_t)ix * nz + iz] += imloc[(size_t)ix * nz + iz];
                    fprintf(fnum, " %f \n", img[(size_t)ix * nz + iz]);
                }
            if (resid) {                             /* dir.resid in shot order: every shot at its offset; its misfit */
                const float *resloc = resloc_all + (size_t)b * ng;
                if (fwrite(resloc, sizeof(float), ng, fres) != ng || fdw_gather_misfit(resloc, ng, &misfit[is]) != FDW_OK) {
                    fprintf(stderr, "cannot write dir.resid\n");
                    return EXIT_FAILURE;
                }
            }
            if (illum) {                             /* stacked like the image, in shot order: independent of the number of workers */
                const float *illoc = illoc_all + (size_t)b * ni;
                for (int iz = 0; iz < nz; iz++)
                    for (int ix = 0; ix < nx; ix++) ill[(size_t)ix * nz + iz] += illoc[(size_t)ix * nz + iz];
            }
        }
        t_stack += now_s() - t1;
    }
    if (bctx) fdw_destroy(bctx);
    free(vel2_all);
    free(imloc_all);
    if (illum) {      /* dir.illum and dir.image_illum, next to the outputs the key leaves untouched */
        if (write_illum_outputs(tmpdir, img, ill, ni, illum_eps) != 0) return EXIT_FAILURE;
        free(illoc_all);
        free(ill);
    }
    if (resid) {      /* dir.misfit: ns doubles; the total added in shot order */
        double total = 0.0;
        for (int is = 0; is < ns; is++) total = total + misfit[is];
        fwrite(misfit, sizeof(double), (size_t)ns, fmis);
        fclose(fres);
        fclose(fmis);
        printf("## misfit = %.9e (0.5 sum resid^2 over %d shots) \n", total, ns);
        free(misfit);
        free(resloc_all);
    }
    if (snap > 0) {      /* dir.snaps, dir.snaps_rec, dir.snapr: shot iss, [frames][ceil(nx / D)][ceil(nz / D)] each */
        if (!fsns || !fsns2 || !fsnr) return EXIT_FAILURE;
        fwrite(sn.snaps, sizeof(float), snap_n, fsns);
        fwrite(sn.snaps_rec, sizeof(float), snap_n, fsns2);
        fwrite(sn.snapr, sizeof(float), snap_n, fsnr);
        free(sn.snaps); free(sn.snaps_rec); free(sn.snapr);
    }
outputs:
    if (timing)
        fprintf(stderr, "[timing] shots per launch sequence: up to %d (%s)\n", shots_per_launch,
                shots_per_launch > 1 ? (lsm > 0 ? "fdw_lsm_solve" : exc ? "fdw_shot_excitation_batch" : pw > 0 ? "fdw_shot_line_batch" : (resid ? "fdw_shot_batch_residual" : (illum ? "fdw_shot_batch_illum" : "fdw_shot_batch")))
                                     : (resid ? "one by one, fdw_shot_residual" : "one by one"));
    if (timing)
        fprintf(stderr, "[timing] total %.3f s: shots (contexts, border models, propagation) %.3f s, stacking + image.num %.3f s, rest (deck, inputs) %.3f s\n",
                now_s() - t_begin, t_shots, t_stack, now_s() - t_begin - t_shots - t_stack);
    /* opt-in extension (deck key image_lap=1): fill dir.image_lap with the reference's own offline filter (models/3lay_mod/laplace.f90)
     * of the stacked image instead of the zeros the reference writes (R:477, R:542) */
    if (fdw_deck_int(deck, "image_lap") == 1 && fdw_image_laplacian(0, img, nx, nz, dx, dz, img_lap) != FDW_OK) {
        fprintf(stderr, "fdw_image_laplacian: %s\n", fdw_last_error());
        return EXIT_FAILURE;
    }
    gettimeofday(&end, NULL);
    /* the reference divides integers (whole seconds, R:536); we print the real value */
    const double exec = ((end.tv_sec - start.tv_sec) * 1000000.0 + (end.tv_usec - start.tv_usec)) / 1000000.0;
    printf("> Exec time = %.2f (s)\n", exec);

    fwrite(img, sizeof(float), ni, fimg);         /* R:540 */
    fwrite(img_lap, sizeof(float), ni, fimg_lap); /* R:542 */
    if (fsns) fclose(fsns);
    if (fsns2) fclose(fsns2);
    if (fsnr) fclose(fsnr);
    fclose(fimg);
    fclose(fimg_lap);
    fclose(fnum);
    free(srce); free(sx); free(vel_ext_rnd); free(d_obs); free(vp); free(vpe);
    free(img); free(img_lap);
    fdw_deck_free(deck);
    return 0;
}

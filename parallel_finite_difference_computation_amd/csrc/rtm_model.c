/* rtm_model -- models the shot gathers that rtm_code migrates:
 *     ./rtm_model ./models/<model>/input.dat
 * Reads the same deck as rtm_code (keys and defaults of R:343-378, numerics= included) and writes the deck's datfile as [ns][nx][nt] fp32,
 * the layout rtm_code reads (R:420-424).  Shot `is` has its source at (fsx + is ds + nxb, sz + nzb), the Ricker wavelet of
 * fdw_ricker_wavelet (R:402-411), and the model rtm_code migrates that shot with: vel_ext_file's shot `is` if the deck names one (R:484),
 * otherwise the border model of draws [is T, (is+1) T) of the unseeded rand() stream (R:486).  Sample (ix, it) is the field fd_forward's
 * d_pp holds at (ix + nxb, gz + nzb) at the end of iteration it (fdw_record_shot, fdwave.h), so rtm_code on the written file correlates
 * equal time levels.  Shots go through fdw_record_shot_batch in batches of fdw_shot_batch_max.  The gathers are written to a temporary file
 * beside datfile and renamed at the end: a run that fails leaves an existing datfile as it was.
 *
 * Several GPUs, with the keys, environment variables and refusals of rtm_code: `gpus=N` (FDW_GPUS=N) deals whole shots to worker threads on
 * N GPUs, each with its own context (FDW_SHOT_WORKERS=W: that many workers, at least one per GPU; set above 1 without gpus= it runs W
 * workers on GPU 0; more GPUs asked for than visible: the workers share the visible ones, with a note on stderr); every worker writes the
 * gathers of its shots at their offsets in the temporary file.  `slabs=N` (FDW_SLABS=N) models
 * every shot on N GPUs through fdw_slabs_record_shot, one host thread per rank (FDW_SLABS_LOCAL=1: all ranks on GPU 0); the ranks share
 * one host-built model per shot (the border drawn by the host's extendvel_linear in shot order, the same values the device draws), each
 * writes its own receiver rows of the shot's gather.  In every mode the datfile is byte for byte the one-GPU program's.
 *
 * Born modelling (fdwave.h, "Born modelling"): with `bornfile=<path>` (fp32 [nx][nz] reflectivity; `born_kind=0|1`, default 1 = the second
 * time difference) the datfile holds the SCATTERED gathers [ns][nx][nt] of fdw_born_shot in the models and border draws the program uses
 * without the key, on one GPU, in groups of fdw_shot_batch_max shots through fdw_born_shot_batch (one launch per time step for the group where
 * the library batches; FDW_NO_SHOT_BATCH=1 keeps one shot after the other; the files are byte for byte the same either way);
 * `born_bg=<path>` also writes the background gathers, which are the plain program's datfile.
 * bornfile together with slabs / gpus (deck key or environment), a born_kind outside {0, 1} and a short or missing reflectivity file are
 * refused before any file, thread or device is touched. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <unistd.h>

#include "fdw_config.h"
#include "fdwave.h"

static float *read_floats(const char *path, size_t n, const char *what)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s '%s'\n", what, path);
        return NULL;
    }
    float *a = (float *)calloc(n ? n : 1, sizeof(float));
    const size_t got = a ? fread(a, sizeof(float), n, f) : 0;
    fclose(f);
    if (got != n) fprintf(stderr, "warning: %s '%s' holds %zu of %zu floats (rest stays zero)\n", what, path, got, n);
    return a;
}

/* ---- gpus=N / FDW_SHOT_WORKERS: worker w models shots w, w + nw, ... on GPU w % gpus and writes each gather at its offset ---- */
typedef struct {
    const fdw_params *prm;
    int ns, nx, nt, sz, gz, sx0, ds, gpus, dev_border, fd;
    const float *srce, *vp, *v2_all;      /* v2_all: every shot's host-built squared model [ns][nxe][nze], or NULL (dev_border) */
    unsigned long long draws;
    size_t ne, ng;
    volatile int failed;
} model_job;
typedef struct {
    model_job *job;
    int w, nw;
} model_worker_arg;

static int write_at(int fd, const float *a, size_t n, size_t float_off)
{
    const char *p = (const char *)a;
    size_t left = n * sizeof(float);
    off_t off = (off_t)(float_off * sizeof(float));
    while (left > 0) {
        const ssize_t k = pwrite(fd, p, left, off);
        if (k <= 0) return -1;
        p += k; off += k; left -= (size_t)k;
    }
    return 0;
}

static void *model_worker(void *p)
{
    model_worker_arg *a = (model_worker_arg *)p;
    model_job *j = a->job;
    fdw_ctx *ctx = NULL;
    float *data = (float *)malloc(j->ng * sizeof(float));
    if (!data || fdw_create(j->prm, a->w % (j->gpus > 0 ? j->gpus : 1), &ctx) != FDW_OK) {
        fprintf(stderr, "worker %d: %s\n", a->w, data ? fdw_last_error() : "out of host memory");
        j->failed = 1;
        free(data);
        return NULL;
    }
    if (j->dev_border && fdw_model_resident(ctx, j->vp) != FDW_OK) {
        fprintf(stderr, "fdw_model_resident: %s\n", fdw_last_error());
        j->failed = 1;
    }
    for (int is = a->w; is < j->ns && !j->failed; is += a->nw) {
        /* one shot with the one-GPU program's model: draws [is T, (is + 1) T) of the stream, or its host-built model */
        if (fdw_record_shot_batch(ctx, 1, j->v2_all ? j->v2_all + (size_t)is * j->ne : NULL, (unsigned long long)is * j->draws, j->sx0 + is * j->ds, j->ds,
                                  j->sz, j->gz, j->srce, data) != FDW_OK) {
            fprintf(stderr, "shot %d: %s\n", is, fdw_last_error());
            j->failed = 1;
        } else if (write_at(j->fd, data, j->ng, (size_t)is * j->ng) != 0) {
            fprintf(stderr, "shot %d: write failed\n", is);
            j->failed = 1;
        }
    }
    fdw_destroy(ctx);
    free(data);
    return NULL;
}

/* ---- slabs=N: every shot decomposed over N ranks (host threads, one GPU each), as rtm_code's slab mode ---- */
typedef struct {
    const fdw_params *prm;
    int world, local, ns, sz, gz, sx0, ds;
    const float *srce;
    const float *v2;         /* the current shot's squared model [nxe][nze], built by rank 0 between the barriers */
    float *data;             /* the current shot's gather [nx][nt]: every rank writes its own rows */
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

/* two phases with a barrier in between (rtm_code.c, slab_rank_open): what a rank can check alone, then the collective calls */
static void slab_rank_open(slab_rank *r)
{
    slab_job *j = r->job;
    int rc = j->local ? FDW_OK : fdw_device_usable(r->rank);
    if (rc != FDW_OK) {
        fprintf(stderr, "rank %d: %s\n", r->rank, fdw_last_error());
        j->failed = 1;
    }
    pthread_barrier_wait(j->bar);
    if (!j->failed) {
        if (j->local) r->comm = j->local_comms[r->rank];
        else rc = fdw_comm_init_rank(j->uid, r->rank, j->world, r->rank, &r->comm);
        if (rc == FDW_OK) rc = fdw_slabs_create(j->prm, r->comm, 0, 0, &r->slabs);
        if (rc != FDW_OK) {
            fprintf(stderr, "rank %d: %s\n", r->rank, fdw_last_error());
            j->failed = 1;
        }
    }
    pthread_barrier_wait(j->bar);
}
static void slab_rank_shot(slab_rank *r, int is)
{
    slab_job *j = r->job;
    if (j->failed || !r->slabs) return;
    if (fdw_slabs_record_shot(r->slabs, j->v2, j->sx0 + is * j->ds, j->sz, j->gz, j->srce, j->data, NULL, NULL) != FDW_OK) {
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
        pthread_barrier_wait(j->bar);       /* B: every rank's rows of the gather are in place */
    }
    if (r->slabs) fdw_slabs_destroy(r->slabs);
    if (r->comm) fdw_comm_destroy(r->comm);
    return NULL;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s <input.dat>\n", argv[0]);
        return EXIT_FAILURE;
    }
    fdw_deck *deck = fdw_deck_read(argv[1]);
    if (!deck) return EXIT_FAILURE;

    /* init_args, R:343-378 (as rtm_code) */
    const char *vpfile = fdw_deck_str(deck, "vpfile"), *datfile = fdw_deck_str(deck, "datfile"), *vel_ext_file = fdw_deck_str(deck, "vel_ext_file");
    const int nz = fdw_deck_int(deck, "nz"), nx = fdw_deck_int(deck, "nx"), nt = fdw_deck_int(deck, "nt");
    int ns = fdw_deck_int(deck, "ns"), sz = fdw_deck_int(deck, "sz"), fsx = fdw_deck_int(deck, "fsx");
    int ds = fdw_deck_int(deck, "ds"), gz = fdw_deck_int(deck, "gz"), order = fdw_deck_int(deck, "order");
    int nzb = fdw_deck_int(deck, "nzb"), nxb = fdw_deck_int(deck, "nxb");
    const int rnd = fdw_deck_int(deck, "rnd");
    const float dz = fdw_deck_float(deck, "dz"), dx = fdw_deck_float(deck, "dx"), dt = fdw_deck_float(deck, "dt");
    const float fpeak = fdw_deck_float(deck, "fpeak");
    float fac = fdw_deck_float(deck, "fac");
    const int vel_ext_flag = vel_ext_file != NULL;
    if (ns == -1) ns = 1;
    if (sz == -1) sz = 0;
    if (fsx == -1) fsx = 0;
    if (ds == -1) ds = 1;
    if (gz == -1) gz = 0;
    if (order == -1) order = 8;
    if (nzb == -1) nzb = 40;
    if (nxb == -1) nxb = 40;
    if (fac == -1.0f) fac = 0.7f;

    printf("## vp = %s, d_obs = %s, vel_ext_file = %s, vel_ext_flag = %d \n", vpfile, datfile, vel_ext_file, vel_ext_flag);
    printf("## nz = %d, nx = %d, nt = %d \n", nz, nx, nt);
    printf("## dz = %f, dx = %f, dt = %f \n", dz, dx, dt);
    printf("## ns = %d, sz = %d, fsx = %d, ds = %d, gz = %d \n", ns, sz, fsx, ds, gz);
    printf("## order = %d, nzb = %d, nxb = %d, F = %f, rnd = %d \n", order, nzb, nxb, fac, rnd);
    if (nz <= 0 || nx <= 0 || nt <= 0 || ns <= 0 || !vpfile || !datfile) {
        fprintf(stderr, "input deck is missing one of vpfile/datfile/nz/nx/nt (or ns <= 0)\n");
        return EXIT_FAILURE;
    }
    /* several GPUs, as rtm_code: refused here, before any file, thread, communicator or device is touched */
    int slabs = fdw_deck_int(deck, "slabs"), gpus = fdw_deck_int(deck, "gpus");
    if (getenv("FDW_SLABS")) slabs = atoi(getenv("FDW_SLABS"));
    if (getenv("FDW_GPUS")) gpus = atoi(getenv("FDW_GPUS"));
    if (slabs > 64 || gpus > 64) {
        fprintf(stderr, "slabs / gpus: at most 64\n");
        return EXIT_FAILURE;
    }
    /* Born modelling: one GPU, shot by shot; everything that cannot run is refused here */
    const char *bornfile = fdw_deck_str(deck, "bornfile"), *born_bg = fdw_deck_str(deck, "born_bg");
    int born_kind = fdw_deck_int(deck, "born_kind");
    if (born_kind == -1) born_kind = FDW_BORN_DTT;
    if (!bornfile && born_bg) {
        fprintf(stderr, "born_bg needs bornfile\n");
        return EXIT_FAILURE;
    }
    if (bornfile) {
        if (slabs > 1 || gpus > 1) {
            fprintf(stderr, "bornfile: Born modelling runs on one GPU, shot by shot: %s is refused\n", slabs > 1 ? "slabs" : "gpus");
            return EXIT_FAILURE;
        }
        if (born_kind != FDW_BORN_FIELD && born_kind != FDW_BORN_DTT) {
            fprintf(stderr, "bornfile: born_kind = %d is neither 0 (the field) nor 1 (its second time difference)\n", born_kind);
            return EXIT_FAILURE;
        }
        FILE *bf = fopen(bornfile, "rb");
        long have = -1;
        if (bf && fseek(bf, 0, SEEK_END) == 0) have = ftell(bf);
        if (bf) fclose(bf);
        if (have < 0 || (size_t)have < (size_t)nx * (size_t)nz * sizeof(float)) {
            fprintf(stderr, "bornfile '%s' is missing or holds fewer than nx * nz = %zu floats\n", bornfile, (size_t)nx * (size_t)nz);
            return EXIT_FAILURE;
        }
    }
    const int slabs_local = getenv("FDW_SLABS_LOCAL") != NULL;
    if (slabs > 1) {
        const int ndev = fdw_device_count();
        if (ndev < 1 || (!slabs_local && slabs > ndev)) {      /* RCCL would wait for the missing ranks for ever */
            fprintf(stderr, "slabs=%d needs %d GPUs, one rank each; %d visible%s\n", slabs, slabs, ndev < 0 ? 0 : ndev,
                    ndev >= 1 ? " (FDW_SLABS_LOCAL=1 runs the ranks as threads sharing GPU 0: rehearsals only)" : "");
            return EXIT_FAILURE;
        }
    }
    int nworkers = getenv("FDW_SHOT_WORKERS") ? atoi(getenv("FDW_SHOT_WORKERS")) : (gpus > 1 ? 4 : 1);
    if (nworkers < 1) nworkers = 1;
    if (gpus > 1 && nworkers < gpus) nworkers = gpus;      /* at least one worker per GPU */
    if (nworkers > ns) nworkers = ns;
    if (nworkers > 64) nworkers = 64;
    const int nze = nz + 2 * nzb, nxe = nx + 2 * nxb;
    sz += nzb;
    gz += nzb;
    if (gz < 0 || gz >= nze) {
        fprintf(stderr, "receiver depth gz = %d lies outside the grid (%d rows with the borders)\n", gz - nzb, nze);
        return EXIT_FAILURE;
    }
    const size_t ne = (size_t)nxe * nze, ni = (size_t)nx * nz, ng = (size_t)nx * nt;

    fdw_params prm;
    memset(&prm, 0, sizeof prm);
    prm.order = order; prm.nxe = nxe; prm.nze = nze; prm.nxb = nxb; prm.nzb = nzb; prm.nt = nt;
    prm.dx = dx; prm.dz = dz; prm.dt = dt; prm.fac = fac;
    prm.compat = 1;   /* the reference's launch extents, R:185-195 */
    prm.coef_cxx = 0;
    prm.numerics = fdw_deck_int(deck, "numerics") == 1 ? FDW_NUMERICS_FAST : FDW_NUMERICS_EXACT;
    if (prm.numerics) printf("## numerics = FAST (symmetric sums + fused multiply-adds in the Laplacian; within 1e-5 of the reference's arithmetic)\n");

    float *srce = (float *)malloc((size_t)nt * sizeof(float));      /* R:402-404 */
    float *vp = read_floats(vpfile, ni, "vpfile");
    float *vel_ext = vel_ext_flag ? read_floats(vel_ext_file, ne * ns, "vel_ext_file") : NULL;
    if (!srce || !vp || (vel_ext_flag && !vel_ext)) return EXIT_FAILURE;
    fdw_ricker_wavelet(nt, dt, fpeak, srce);

    /* border models: drawn on the device where the library can (as rtm_code does), else built on the host in shot order (R:486) */
    const int dev_border = !vel_ext_flag && nxb != 1 && nzb != 1 && nzb <= nxe;
    const unsigned long long draws = (unsigned long long)fdw_border_draws(nx, nz, nxb, nzb);
    const int sx0 = fsx + nxb;
    float *vpe = vel_ext_flag ? NULL : (float *)calloc(ne, sizeof(float));      /* the interior model in its extended array (host-built borders) */
    if (!vel_ext_flag && !vpe) {
        fprintf(stderr, "out of host memory\n");
        return EXIT_FAILURE;
    }
    if (vpe)
        for (int ix = 0; ix < nx; ix++)
            for (int iz = 0; iz < nz; iz++) vpe[(size_t)(ix + nxb) * nze + iz + nzb] = vp[(size_t)ix * nz + iz];      /* R:445-449 */
    /* shot `is` of the host loop: its model squared into v2 (vel_ext_file's, or the next border of the sequential rand() stream) */
#define HOST_MODEL(is, v2)                                                                                                    \
    do {                                                                                                                      \
        const float *v_ = vel_ext_flag ? vel_ext + (size_t)(is) * ne : vpe;                          /* R:484 */               \
        if (!vel_ext_flag) fdw_extendvel_linear(nx, nz, nxb, nzb, vpe);                              /* R:486 */               \
        for (size_t k_ = 0; k_ < ne; k_++) (v2)[k_] = v_[k_] * v_[k_];                               /* R:490-494 */           \
    } while (0)

    char *tmp = (char *)malloc(strlen(datfile) + 16);
    sprintf(tmp, "%s.XXXXXX", datfile);
    const int fd = mkstemp(tmp);
    FILE *out = fd >= 0 ? fdopen(fd, "wb") : NULL;
    if (!out) {
        fprintf(stderr, "cannot create a temporary file beside '%s'\n", datfile);
        return EXIT_FAILURE;
    }
    int ok = 1;
    if (slabs > 1) {
        /* ---- every shot on `slabs` GPUs ---- */
        slab_job sj;
        memset(&sj, 0, sizeof sj);
        sj.local = slabs_local;
        sj.prm = &prm; sj.world = slabs; sj.ns = ns; sj.sz = sz; sj.gz = gz; sj.sx0 = sx0; sj.ds = ds; sj.srce = srce;
        float *v2 = (float *)malloc(ne * sizeof(float)), *data = (float *)calloc(ng, sizeof(float));
        fdw_comm *lc[64];
        pthread_barrier_t bar;
        pthread_t th[64];
        slab_rank rk[64];
        int nth = 0;
        if (!v2 || !data || pthread_barrier_init(&bar, NULL, (unsigned)slabs) != 0) ok = 0;
        sj.v2 = v2; sj.data = data; sj.bar = &bar; sj.local_comms = lc;
        if (ok && (sj.local ? fdw_comm_init_local(slabs, NULL, lc) : fdw_comm_get_unique_id(sj.uid)) != FDW_OK) {
            fprintf(stderr, "communicator: %s\n", fdw_last_error());
            ok = 0;
        }
        if (ok) {
            for (int r = 0; r < slabs; r++) {
                memset(&rk[r], 0, sizeof rk[r]);
                rk[r].job = &sj; rk[r].rank = r;
            }
            for (int r = 1; r < slabs; r++) {
                if (pthread_create(&th[r], NULL, slab_rank_thread, &rk[r]) != 0) {      /* the others would wait at the barrier for ever */
                    fprintf(stderr, "pthread_create failed\n");
                    unlink(tmp);
                    _exit(EXIT_FAILURE);
                }
                nth = r;
            }
            slab_rank_open(&rk[0]);
            for (int is = 0; is < ns; is++) {
                if (!sj.failed) HOST_MODEL(is, v2);
                pthread_barrier_wait(&bar);
                slab_rank_shot(&rk[0], is);
                pthread_barrier_wait(&bar);
                if (!sj.failed && fwrite(data, sizeof(float), ng, out) != ng) {
                    fprintf(stderr, "write to '%s' failed\n", tmp);
                    sj.failed = 1;
                }
                if (!sj.failed)
                    printf("** shot %d, source at (%d,%d): %d receivers at depth %d, %d samples\n", is + 1, fsx + is * ds, sz - nzb, nx, gz - nzb, nt);
            }
            for (int r = 1; r <= nth; r++) pthread_join(th[r], NULL);
            if (rk[0].slabs) fdw_slabs_destroy(rk[0].slabs);
            if (rk[0].comm) fdw_comm_destroy(rk[0].comm);
            pthread_barrier_destroy(&bar);
            if (sj.failed) ok = 0;
        }
        free(v2); free(data);
    } else if (bornfile) {
        /* ---- Born modelling: one GPU, groups of fdw_shot_batch_max shots through fdw_born_shot_batch, each shot in the model the plain
         * program gives it.  FDW_NO_SHOT_BATCH=1: groups of one, which the library runs as fdw_born_shot. ---- */
        fdw_ctx *ctx = NULL;
        float *m = read_floats(bornfile, ni, "bornfile");
        char *tmpbg = born_bg ? (char *)malloc(strlen(born_bg) + 16) : NULL;
        FILE *bg = NULL;
        if (!m || (born_bg && !tmpbg)) {
            fprintf(stderr, "out of host memory\n");
            ok = 0;
        }
        if (ok && born_bg) {
            sprintf(tmpbg, "%s.XXXXXX", born_bg);
            const int fdb = mkstemp(tmpbg);
            bg = fdb >= 0 ? fdopen(fdb, "wb") : NULL;
            if (!bg) {
                fprintf(stderr, "cannot create a temporary file beside '%s'\n", born_bg);
                ok = 0;
            }
        }
        if (ok && fdw_create(&prm, 0, &ctx) != FDW_OK) {
            fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
            ok = 0;
        }
        if (ok && dev_border && fdw_model_resident(ctx, vp) != FDW_OK) {
            fprintf(stderr, "fdw_model_resident: %s\n", fdw_last_error());
            ok = 0;
        }
        int batch = (ok && ns > 1 && !getenv("FDW_NO_SHOT_BATCH")) ? fdw_shot_batch_max(ctx) : 1;
        if (batch > ns) batch = ns;
        if (batch < 1) batch = 1;
        float *data = (float *)malloc((size_t)batch * ng * sizeof(float)), *data0 = born_bg ? (float *)malloc((size_t)batch * ng * sizeof(float)) : NULL;
        float *v2 = dev_border ? NULL : (float *)malloc((size_t)batch * ne * sizeof(float));
        if (ok && (!data || (born_bg && !data0) || (!dev_border && !v2))) {
            fprintf(stderr, "out of host memory\n");
            ok = 0;
        }
        for (int is0 = 0; is0 < ns && ok; is0 += batch) {
            const int nb = is0 + batch <= ns ? batch : ns - is0;
            for (int b = 0; b < nb && !dev_border; b++) HOST_MODEL(is0 + b, v2 + (size_t)b * ne);
            if (fdw_born_shot_batch(ctx, nb, v2, (unsigned long long)is0 * draws, m, born_kind, sx0 + is0 * ds, ds, sz, gz, srce, data, data0) != FDW_OK) {
                fprintf(stderr, "shots %d..%d: %s\n", is0, is0 + nb - 1, fdw_last_error());
                ok = 0;
                break;
            }
            if (is0 == 0 && getenv("FDW_TIMING"))      /* which path the first group took (a group of one, or a regime the library does not batch: one by one) */
                fprintf(stderr, "[timing] shots per launch sequence: up to %d (%s)\n", batch, fdw_batch_parts(ctx) > 0 ? "fdw_born_shot_batch" : "one by one");
            if (fwrite(data, sizeof(float), (size_t)nb * ng, out) != (size_t)nb * ng || (bg && fwrite(data0, sizeof(float), (size_t)nb * ng, bg) != (size_t)nb * ng)) {
                fprintf(stderr, "write failed\n");
                ok = 0;
                break;
            }
            for (int b = 0; b < nb; b++)
                printf("** shot %d, source at (%d,%d): %d receivers at depth %d, %d samples (scattered field, kind %d)\n", is0 + b + 1, fsx + (is0 + b) * ds,
                       sz - nzb, nx, gz - nzb, nt, born_kind);
        }
        if (ctx) fdw_destroy(ctx);
        if (bg && fclose(bg) != 0) ok = 0;
        if (bg && ok && rename(tmpbg, born_bg) != 0) {
            fprintf(stderr, "cannot rename '%s' to '%s'\n", tmpbg, born_bg);
            ok = 0;
        }
        if (bg && !ok) unlink(tmpbg);
        free(m); free(data); free(data0); free(v2); free(tmpbg);
    } else if (nworkers > 1) {
        /* ---- whole shots dealt to worker threads / GPUs ---- */
        model_job job;
        memset(&job, 0, sizeof job);
        float *v2_all = dev_border ? NULL : (float *)malloc((size_t)ns * ne * sizeof(float));
        if (!dev_border && !v2_all) {
            fprintf(stderr, "out of host memory\n");
            ok = 0;
        }
        for (int is = 0; is < ns && ok && !dev_border; is++) HOST_MODEL(is, v2_all + (size_t)is * ne);      /* in shot order: the rand() stream is sequential */
        /* more GPUs asked for than visible: the workers share the visible ones (the bytes do not depend on where a shot runs) */
        const int ndev = fdw_device_count();
        if (gpus > 1 && ndev >= 1 && gpus > ndev) {
            fprintf(stderr, "gpus=%d: %d visible; the %d workers share %s\n", gpus, ndev, nworkers, ndev == 1 ? "it" : "them");
            gpus = ndev;
        }
        job.prm = &prm; job.ns = ns; job.nx = nx; job.nt = nt; job.sz = sz; job.gz = gz; job.sx0 = sx0; job.ds = ds; job.gpus = gpus;
        job.dev_border = dev_border; job.fd = fd; job.srce = srce; job.vp = vp; job.v2_all = v2_all; job.draws = draws; job.ne = ne; job.ng = ng;
        pthread_t th[64];
        model_worker_arg wa[64];
        int nth = 0;
        for (int w = 0; w < nworkers && ok; w++) {
            wa[w].job = &job; wa[w].w = w; wa[w].nw = nworkers;
            if (w > 0) {
                if (pthread_create(&th[w], NULL, model_worker, &wa[w]) != 0) {
                    fprintf(stderr, "pthread_create failed\n");
                    job.failed = 1;
                    break;
                }
                nth = w;
            }
        }
        if (ok) model_worker(&wa[0]);
        for (int w = 1; w <= nth; w++) pthread_join(th[w], NULL);
        if (job.failed) ok = 0;
        for (int is = 0; is < ns && ok; is++)
            printf("** shot %d, source at (%d,%d): %d receivers at depth %d, %d samples\n", is + 1, fsx + is * ds, sz - nzb, nx, gz - nzb, nt);
        free(v2_all);
    } else {
        /* ---- one GPU: batches of fdw_shot_batch_max shots through one launch per time step ---- */
        fdw_ctx *ctx = NULL;
        if (fdw_create(&prm, 0, &ctx) != FDW_OK) {
            fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
            ok = 0;
        }
        if (ok && dev_border && fdw_model_resident(ctx, vp) != FDW_OK) {
            fprintf(stderr, "fdw_model_resident: %s\n", fdw_last_error());
            ok = 0;
        }
        int batch = ok ? fdw_shot_batch_max(ctx) : 1;
        if (batch > ns) batch = ns;
        if (ok && getenv("FDW_TIMING"))      /* as rtm_code says it: how many shots advance through one launch per time step */
            fprintf(stderr, "[timing] shots per launch sequence: up to %d (%s)\n", batch, batch > 1 ? "fdw_record_shot_batch" : "one by one");
        float *data = (float *)malloc((size_t)batch * ng * sizeof(float));
        float *v2_all = dev_border ? NULL : (float *)malloc((size_t)batch * ne * sizeof(float));
        if (ok && (!data || (!dev_border && !v2_all))) {
            fprintf(stderr, "out of host memory\n");
            ok = 0;
        }
        for (int is0 = 0; is0 < ns && ok; is0 += batch) {
            const int nb = is0 + batch <= ns ? batch : ns - is0;
            for (int b = 0; b < nb && !dev_border; b++) HOST_MODEL(is0 + b, v2_all + (size_t)b * ne);
            if (fdw_record_shot_batch(ctx, nb, v2_all, (unsigned long long)is0 * draws, sx0 + is0 * ds, ds, sz, gz, srce, data) != FDW_OK) {
                fprintf(stderr, "fdw_record_shot_batch: %s\n", fdw_last_error());
                ok = 0;
                break;
            }
            if (fwrite(data, sizeof(float), (size_t)nb * ng, out) != (size_t)nb * ng) {
                fprintf(stderr, "write to '%s' failed\n", tmp);
                ok = 0;
                break;
            }
            for (int b = 0; b < nb; b++)
                printf("** shot %d, source at (%d,%d): %d receivers at depth %d, %d samples\n", is0 + b + 1, fsx + (is0 + b) * ds, sz - nzb, nx, gz - nzb, nt);
        }
        if (ctx) fdw_destroy(ctx);
        free(data); free(v2_all);
    }
#undef HOST_MODEL
    if (fclose(out) != 0) ok = 0;
    if (ok && rename(tmp, datfile) != 0) {
        fprintf(stderr, "cannot rename '%s' to '%s'\n", tmp, datfile);
        ok = 0;
    }
    if (!ok) unlink(tmp);
    free(tmp); free(vpe); free(vel_ext); free(vp); free(srce);
    fdw_deck_free(deck);
    return ok ? 0 : EXIT_FAILURE;
}

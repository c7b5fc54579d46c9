/* rtm_model -- models the shot gathers that rtm_code migrates:
 *     ./rtm_model ./models/<model>/input.dat
 * Reads the same deck as rtm_code (keys and defaults of R:343-378, numerics= included) and writes the deck's datfile as [ns][nx][nt] fp32,
 * the layout rtm_code reads (R:420-424).  Shot `is` has its source at (fsx + is ds + nxb, sz + nzb), the Ricker wavelet of
 * fdw_ricker_wavelet (R:402-411), and the model rtm_code migrates that shot with: vel_ext_file's shot `is` if the deck names one (R:484),
 * otherwise the border model of draws [is T, (is+1) T) of the unseeded rand() stream (R:486).  Sample (ix, it) is the field fd_forward's
 * d_pp holds at (ix + nxb, gz + nzb) at the end of iteration it (fdw_record_shot, fdwave.h), so rtm_code on the written file correlates
 * equal time levels.  Shots go through fdw_record_shot_batch in batches of fdw_shot_batch_max.  The gathers are written to a temporary file
 * beside datfile and renamed at the end: a run that fails leaves an existing datfile as it was. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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
    if (fdw_deck_int(deck, "slabs") > 1 || fdw_deck_int(deck, "gpus") > 1) {
        fprintf(stderr, "rtm_model runs on one GPU: slabs= and gpus= greater than 1 are not supported\n");
        return EXIT_FAILURE;
    }
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

    fdw_ctx *ctx = NULL;
    if (fdw_create(&prm, 0, &ctx) != FDW_OK) {
        fprintf(stderr, "fdw_create: %s\n", fdw_last_error());
        return EXIT_FAILURE;
    }
    /* border models: drawn on the device where the library can (as rtm_code does), else built on the host in shot order (R:486) */
    const int dev_border = !vel_ext_flag && nxb != 1 && nzb != 1 && nzb <= nxe;
    if (dev_border && fdw_model_resident(ctx, vp) != FDW_OK) {
        fprintf(stderr, "fdw_model_resident: %s\n", fdw_last_error());
        return EXIT_FAILURE;
    }
    int batch = fdw_shot_batch_max(ctx);
    if (batch > ns) batch = ns;
    float *data = (float *)malloc((size_t)batch * ng * sizeof(float));
    float *v2_all = dev_border ? NULL : (float *)malloc((size_t)batch * ne * sizeof(float));
    float *vpe = dev_border || vel_ext_flag ? NULL : (float *)calloc(ne, sizeof(float));
    if (!data || (!dev_border && !v2_all) || (!dev_border && !vel_ext_flag && !vpe)) {
        fprintf(stderr, "out of host memory\n");
        return EXIT_FAILURE;
    }
    if (vpe)
        for (int ix = 0; ix < nx; ix++)
            for (int iz = 0; iz < nz; iz++) vpe[(size_t)(ix + nxb) * nze + iz + nzb] = vp[(size_t)ix * nz + iz];      /* R:445-449 */

    char *tmp = (char *)malloc(strlen(datfile) + 16);
    sprintf(tmp, "%s.XXXXXX", datfile);
    const int fd = mkstemp(tmp);
    FILE *out = fd >= 0 ? fdopen(fd, "wb") : NULL;
    if (!out) {
        fprintf(stderr, "cannot create a temporary file beside '%s'\n", datfile);
        return EXIT_FAILURE;
    }
    const unsigned long long draws = (unsigned long long)fdw_border_draws(nx, nz, nxb, nzb);
    int ok = 1;
    for (int is0 = 0; is0 < ns && ok; is0 += batch) {
        const int nb = is0 + batch <= ns ? batch : ns - is0;
        for (int b = 0; b < nb && !dev_border; b++) {
            const float *v = vel_ext_flag ? vel_ext + (size_t)(is0 + b) * ne : vpe;      /* R:484 */
            if (!vel_ext_flag) fdw_extendvel_linear(nx, nz, nxb, nzb, vpe);             /* R:486: glibc rand(), never seeded */
            float *v2 = v2_all + (size_t)b * ne;
            for (size_t k = 0; k < ne; k++) v2[k] = v[k] * v[k];                       /* R:490-494 */
        }
        if (fdw_record_shot_batch(ctx, nb, v2_all, (unsigned long long)is0 * draws, fsx + is0 * ds + nxb, ds, sz, gz, srce, data) != FDW_OK) {
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
    if (fclose(out) != 0) ok = 0;
    if (ok && rename(tmp, datfile) != 0) {
        fprintf(stderr, "cannot rename '%s' to '%s'\n", tmp, datfile);
        ok = 0;
    }
    if (!ok) unlink(tmp);
    fdw_destroy(ctx);
    free(tmp); free(data); free(v2_all); free(vpe); free(vel_ext); free(vp); free(srce);
    fdw_deck_free(deck);
    return ok ? 0 : EXIT_FAILURE;
}

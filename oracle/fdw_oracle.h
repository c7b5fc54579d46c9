/*
 * fdw_oracle.h -- TEST INFRASTRUCTURE ONLY, private to oracle/: what fdw_oracle.c and fdw_oracle_mod.c share.
 */
#ifndef FDW_ORACLE_H
#define FDW_ORACLE_H

#include <math.h>
#include <stddef.h>

/* F:113-158 == S:137-182 (fdw_oracle.c) */
void orc_calc_coefs(int order, int cxx, float *coef);

/* FAST numerics (see the header of fdw_oracle.c): lap = c0 p + sum_k [cz_k (p(j-k) + p(j+k)) + cx_k (p(i-k) + p(i+k))], c0 = cz_0 + cx_0 in
 * fp32, one chain: acc = c0 * p; per k = 1..h: acc = fma(z sum, cz_k, acc); acc = fma(x sum, cx_k, acc).  p points at the centre, sx = floats
 * between rows; the weights carry their spacing. */
static inline float orc_lap_fast(const float *p, size_t sx, int h, const float *coefsx, const float *coefsz)
{
    float c0 = coefsz[h] + coefsx[h];
    float acc = c0 * p[0];
    int k;
    for (k = 1; k <= h; k++) {
        float sz = p[-k] + p[k];
        float sxs = p[-(long)(k * sx)] + p[k * sx];
        acc = fmaf(sz, coefsz[h - k], acc);
        acc = fmaf(sxs, coefsx[h - k], acc);
    }
    return acc;
}

#endif

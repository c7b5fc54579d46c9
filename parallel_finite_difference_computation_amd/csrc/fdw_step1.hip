// fdw_step1.hip -- one time step per pass: the fused register-ring kernel (all modes and dialects), the generic-order kernel, the
// small utility kernels and their launchers.  Design notes: fdw_device.h.
//
// This file is compiled three times (csrc/Makefile) so that its ~70 instantiations build side by side:
//   FDW_TU 0 (fdw_step1.o)       the RTM dialect with the reference's exact arithmetic, the generic-order kernel, the utility kernels
//   FDW_TU 1 (fdw_step1_dd.o)    the dialects of the CPU-serial sibling (MOD, DD_FWD, DD_RECV)
//   FDW_TU 2 (fdw_step1_fast.o)  the RTM dialect with FAST numerics (fdw_device.h)
#include "fdw_device.h"
#include "fdw_born.h"
#include "fdw_dtt.h"

#pragma clang fp contract(off)

#ifndef FDW_TU
#define FDW_TU 0
#endif

namespace fdw {

// ------------------------------------------------------------------------------------------------
// fused step kernel
//   H       half order (1..4)
//   TAPER   apply the lazy top-strip damping to p / pp
//   INJ     0 none, 1 point source (kernel_src), 2 receiver row (kernel_sism), 3 7x7 Gaussian point source (ptsrc.c of the CPU-serial sibling)
//   IMG     img += psrc * pp_new epilogue (kernel_img)
//   LAPONLY store the Laplacian itself into a.pp (stencil_code path, S:110-135); no update
//   DD      arithmetic of the CPU-serial sibling's fd_step (single accumulator, per-term scaling) + one trace sample per row
//   PF      software prefetch distance in rows
//   REC     trace recording of the RTM dialect's forward loop: the new field at column rec_z of every receiver row (fdw_step_rec_kernel)
//   ILL     source illumination of the forward loop: sv.img += new field (*) new field on the updated cells, product and sum rounded
//           separately (fdw_step_illum_kernel); the row of the accumulator rides the image queue
//   EXC     excitation-amplitude imaging (fdwave.h, "excitation amplitude"), the RTM dialect's forward loops; batched like the fields:
//           1  the excitation maps: where |new field| > |amp| strictly, amp = the new field (signed) and texc = a.exc_key (= it + 1);
//              the amp row rides the image queue (a.img), the texc row a queue of its own (fdw_step_exc_kernel)
//           2  the excitation pick: where texc == a.exc_key (= top - it), exc = the new field; texc is only read, the exc row (a.img) is
//              stored back whole, unpicked words with the bits they came with (fdw_step_line_pick_kernel)
//           Compares and selects only: texc travels as 32-bit words in float registers and meets no arithmetic.
//   BORN    Born modelling (fdwave.h, "Born modelling"; fdw_step_born_kernel): the second register ring of BACK carries the SCATTERED field
//           (sv.psrc = du_p read only, sv.fpp = du_pp overwritten), which gets the damping and no injection; the row of the reflectivity m
//           (a.img, only read) rides the pointwise queue; on the interior cells du_new = du_new (+) m (*) q, with q the background's new
//           value (kind 0, fdw_born.h) or its second time difference (1) from the registers the leap-frog just used; then the trace samples
//   DTT     second-time-difference imaging (fdwave.h, "DTT imaging"; fdw_step_back_dtt_kernel), a value of the IMG epilogue of BACK: on the
//           cells C img += ((F_old (-) F_cur) (-) (F_cur (-) F_new)) (*) the receiver field the launch OVERWRITES (its entry words), from
//           registers the two leap-frogs already hold; every other word of the image row is stored back with the bits it came with
// block = 256 threads = 4 independent waves (no LDS, no barrier).
//
// ONE code path for every tile.  Every global load of the march is unconditional (addresses are
// clamped into the slab instead of being predicated), so the compiler's s_waitcnt bookkeeping stays
// exact and the look-ahead loads really stay in flight.  Whatever a clamped load brings in only ever
// reaches outputs that the column / row masks zero: rows outside the slab are taps of rows whose
// Laplacian is masked (lap_x0 >= H, lap_x1 <= nxl-H), columns outside the grid are taps of columns
// >= nze-H.  Edge handling (masks, damping, injection) is wave-uniform branches around VALU / scalar
// loads only.
// ------------------------------------------------------------------------------------------------
// the field pointers, sample pointer and source row of the shot a block works on (shot 0: the launch arguments themselves)
struct ShotView {
    const float* p;
    float* pp;
    float* out;            // where the new field is stored: pp itself unless StepArgs::out names another array
    const float* v2;
    const float* psrc;
    float* fpp;
    float* img;
    const float* inj;
    int inj_x;
    float* rec;
};

template <int H, bool TAPER, int INJ, bool IMG, bool LAPONLY, int PF, bool DD = false, bool BACK = false, int NUM = 0, bool REC = false, bool ILL = false,
          int EXC = 0, bool BORN = false, bool DTT = false>
__device__ __forceinline__ void march(const StepArgs& a, const ShotView& sv, const int lane, const int zs, const int xa, const int xe)
{
    // BACK: one whole backward iteration of fd_back (R:317-329) in a single pass: the source field is reconstructed in a second
    // register ring (sv.psrc = F_{k-1} read only, sv.fpp = F_{k-2} overwritten with F_k: kernel_lap + kernel_time without damping,
    // R:317-318) next to the receiver step, v2 is read once for both and F_k meets the new receiver row in registers for the imaging
    // condition instead of travelling through memory.
    using G = RingGeom<H, PF>;
    constexpr int R = G::R, LOOK = G::LOOK;
    const size_t pitch = (size_t)a.pitch;
    const int z0 = zs + lane * 4;
    const bool partial = (zs + 256 > a.pitch);              // wave-uniform: last strip of a ragged row
    const bool act = z0 < a.pitch;                          // pitch % 4 == 0: a float4 never straddles a row end
    const unsigned voff = (unsigned)min(z0, a.pitch - 4) * 4u;
    // strip halo in ONE load by all lanes: lane 0 fetches the 4 columns left of the strip, every other
    // lane the 4 columns right of it (a single 16-B piece; only lane 63 consumes it).
    const unsigned hoff = (unsigned)((lane == 0) ? max(zs - 4, 0) : min(zs + 256, a.pitch - 4)) * 4u;
    const bool lane_first = (lane == 0), lane_last = (lane == 63);
    const int rowmax = min(a.nxl, xe + H) - 1;              // last row of p this wave can need

    // wave-uniform classification of the tile
    const bool zedge = (zs < a.lap_z0) || (zs + 256 > a.lap_z1) || (!LAPONLY && zs + 256 > a.upd_z1);
    const bool xedge = (xa < a.lap_x0) || (xe > a.lap_x1);
    const bool wave_tap = TAPER && (zs - 4 < a.ztap);
    const bool xtap = wave_tap && ((xa - H < a.xt_lo) || (xe + H > a.xt_hi));   // rows with an x factor / no z factor
    bool inj_here = false;
    if (INJ == 1) inj_here = (sv.inj_x >= xa) && (sv.inj_x < xe) && (a.inj_z >= zs) && (a.inj_z < zs + 256);
    if (INJ == 2) inj_here = (a.inj_z >= zs) && (a.inj_z < zs + 256) && (sv.inj_x < xe) && (sv.inj_x + a.inj_n > xa);
    if (INJ == 3) inj_here = (a.inj_z + 3 >= zs) && (a.inj_z - 3 < zs + 256) && (sv.inj_x + 3 >= xa) && (sv.inj_x - 3 < xe);   // 7x7 blob
    const float inj_src = ((INJ == 1 || INJ == 3) && inj_here) ? sload(sv.inj, 0) : 0.0f;
    const bool rec_here = DD && (a.rec != nullptr) && (a.rec_z >= zs) && (a.rec_z < zs + 256);
    const CoefPairs<H> cpk = coef_pairs<H>(a.cx, a.cz);
    const v2f c0p = v2f{a.c0, a.c0};                          // FAST numerics: weight of the centre point
    // REC: the lane whose float4 holds column rec_z records element rec_z & 3 of its new row (strips do not overlap: one lane in the grid)
    const bool rec_lane = (REC || BORN) && (z0 >> 2) == (a.rec_z >> 2);
    constexpr bool TWO = BACK || BORN;                      // a second field is stepped side by side in a ring of its own
    const bool born_here = (BORN || DTT) && (zs < a.img_z1) && (zs + 256 > born_key_z0(a.exc_key));      // wave-uniform: the strip holds interior columns

    // per-lane column masks and damping factors
    bool mlap[4], mupd[4], znc[4], znh[4], ihit[4];
    [[maybe_unused]] bool mborn[4];                         // BORN: the interior columns (the scatter's); DTT: the imaged columns
    float tzc[4], tzh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int z = z0 + e;
        mlap[e] = (z >= a.lap_z0) && (z < a.lap_z1);
        mupd[e] = z < a.upd_z1;
        ihit[e] = (z == a.inj_z);
        if constexpr (BORN || DTT) mborn[e] = (z >= born_key_z0(a.exc_key)) && (z < a.img_z1);
        znc[e] = znh[e] = false;
        tzc[e] = tzh[e] = 1.0f;
    }
    if (wave_tap) {
        const int hz = (lane == 0) ? zs - 4 : zs + 256;     // true (unclamped) column of this lane's halo piece
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int zc = z0 + e, zh = hz + e;
            znc[e] = zc < a.ztap;
            znh[e] = (zh >= 0) && (zh < a.ztap);
            if (znc[e]) tzc[e] = a.taperz[zc];
            if (znh[e]) tzh[e] = a.taperz[zh];
        }
    }
    // one application of the reference's damping to a row held in registers (R:103-114)
    auto taper_row = [&](f4& v, const float* tz, const bool* zone, int row) {
        if (!xtap) {   // common case: no x factor on these rows, every row gets the z factor; *1.0f is exact
#pragma unroll
            for (int e = 0; e < 4; ++e) v.v[e] = v.v[e] * tz[e];
        } else {
            const int rc = min(max(row, 0), a.nxl - 1);
            const float txr = sload(a.txfac, rc);
            const bool rowtz = row < a.tz_x1;
#pragma unroll
            for (int e = 0; e < 4; ++e) v.v[e] = taper1(v.v[e], tz[e], zone[e], rowtz, txr);
        }
    };

    // ---- loaders: unconditional, clamped --------------------------------------------------------
    auto load_p = [&](int row) -> f4 { return f4_load(sv.p + (size_t)min(max(row, 0), rowmax) * pitch, voff); };
    auto load_halo = [&](int row) -> f4 { return f4_load(sv.p + (size_t)row * pitch, hoff); };
    auto load_plain = [&](const float* base, int row) -> f4 { return f4_load_stream(base + (size_t)row * pitch, voff); };
    auto load_f = [&](int row) -> f4 { return f4_load(sv.psrc + (size_t)min(max(row, 0), rowmax) * pitch, voff); };
    auto load_fhalo = [&](int row) -> f4 { return f4_load(sv.psrc + (size_t)row * pitch, hoff); };

    // ---- prologue: ring rows xa-H .. xa-H+R-1; pointwise rows xa .. xa+PF-1 --------------------
    // Issue order matters: the loop-header s_waitcnt is the stricter of (prologue state, end-of-turn
    // state).  Issuing the look-ahead loads in the order the steady state would have issued them
    // ("virtual steps" -LOOK..-1) makes the two states agree, so no turn starts with a pipeline drain.
    f4 ring[R];
    f4 qhal[PF], qpp[PF], qv2[PF], qps[PF], qim[PF];
    f4 qtx[EXC ? PF : 1];                                   // EXC: the texc row, as words
    [[maybe_unused]] float* texc_w = nullptr;               // EXC: the time map of this block's shot (a batch: a.texc + shot * a.bstride)
    if constexpr (EXC != 0) texc_w = reinterpret_cast<float*>(a.texc) + (long long)blockIdx.y * a.bstride;
    f4 fring[TWO ? R : 1], fqhal[TWO ? PF : 1], fqpp[TWO ? PF : 1];      // the source field's (BORN: the scattered field's) ring and pointwise queues
    f4 qm[BORN ? PF : 1];                                   // BORN: the reflectivity row
    [[maybe_unused]] const float* rec0_w = nullptr;         // BORN: this step's background trace row of this block's shot (a.texc + shot * a.rec_bstride)
    if constexpr (BORN) rec0_w = reinterpret_cast<const float*>(a.texc) + (long long)blockIdx.y * a.rec_bstride;
    constexpr int NV = LOOK > PF ? LOOK : PF;
    static_for<2 * H>([&](auto K) {
        constexpr int k = decltype(K)::value;
        ring[k] = load_p(xa - H + k);
        if constexpr (TWO) fring[k] = load_f(xa - H + k);
        __builtin_amdgcn_sched_barrier(0);
    });
    static_for<NV>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value - NV;   // virtual step -NV .. -1
        if constexpr (j >= -LOOK) {
            ring[j + 2 * H + LOOK] = load_p(xa + j + H + LOOK);
            if constexpr (TWO) fring[j + 2 * H + LOOK] = load_f(xa + j + H + LOOK);
        }
        if constexpr (j >= -PF) {
            constexpr int m = j + PF;
            const int row = min(xa + m, xe - 1);
            qhal[m] = load_halo(row);
            if constexpr (!LAPONLY) {
                qpp[m] = load_plain(sv.pp, row);
                qv2[m] = load_plain(sv.v2, row);
            }
            if constexpr (IMG) {
                if constexpr (!BACK) qps[m] = load_plain(sv.psrc, row);
                qim[m] = load_plain(sv.img, row);
            }
            if constexpr (ILL) qim[m] = load_plain(sv.img, row);
            if constexpr (EXC != 0) {
                qim[m] = load_plain(sv.img, row);
                qtx[m] = load_plain(texc_w, row);
            }
            if constexpr (TWO) {
                fqhal[m] = load_fhalo(row);
                fqpp[m] = load_plain(sv.fpp, row);
            }
            if constexpr (BORN) qm[m] = load_plain(a.img, row);
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    if (wave_tap) {   // the first 2H window rows never "enter" the window during the march: damp them here
        static_for<2 * H>([&](auto K) {
            constexpr int k = decltype(K)::value;
            taper_row(ring[k], tzc, znc, xa - H + k);
            if constexpr (BORN) taper_row(fring[k], tzc, znc, xa - H + k);
        });
    }

    // One row of the march.  GUARD=false: the row is known to exist; GUARD=true: wave-uniform test.
    auto row_step = [&](const int rb, auto UU, auto GG) {
        constexpr int U = decltype(UU)::value;
        constexpr bool GUARD = decltype(GG)::value;
        constexpr int Q = U % PF;          // pointwise queue slot of this row (R % PF == 0)
        const int r = rb + U;
        if (!GUARD || r < xe) {
            // ---- damping of what enters the computation this step -----------------------------
            f4 hal = qhal[Q];
            f4 ppt = qpp[Q];
            if (wave_tap) {
                taper_row(ring[(U + 2 * H) % R], tzc, znc, r + H);   // row r+H enters the window
                taper_row(hal, tzh, znh, r);
                if constexpr (!LAPONLY) {
                    taper_row(ppt, tzc, znc, r);
                    if (a.pp_twice) taper_row(ppt, tzc, znc, r);
                }
            }
            // ---- z neighbours from the adjacent lanes (DPP lane shifts), strip halo at the ends ----
            const f4 c = ring[(U + H) % R];
            f4 lft, rgt;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float up = lane_up(c.v[e]), dn = lane_down(c.v[e]);
                lft.v[e] = lane_first ? hal.v[e] : up;
                rgt.v[e] = lane_last ? hal.v[e] : dn;
            }
            const bool rowok = (r >= a.lap_x0) && (r < a.lap_x1);
            f4 res, imr;
            if constexpr (DD) {
                if (rec_here && r >= a.rec_x0 && r < a.rec_x0 + a.rec_n) {      // the trace sample of this step: the current field at depth rec_z
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        // mod_main's iteration is fd_step, ptsrc, taper_apply(PP), taper_apply(P), and only then data = P (mod_main.cpp:147-157): the
                        // sample is P after this iteration's taper_apply.  The device array holds P one pass short of the field fd_step reads; the
                        // window row c got that pass on load, so it is fd_step's P, and this iteration's own pass -- which the array will only
                        // see on the next load -- is applied here: the column's z factor (1.0f, exact, between the strips; receiver rows are
                        // interior rows and carry no x factor).  Two passes from the array, as two taper_apply calls lie between it and the sample.
                        if (z0 + e == a.rec_z) sv.rec[r - a.rec_x0] = c.v[e] * tzc[e];
                }
            }
            if constexpr (DD && NUM == 0) {
                // the sibling's own arithmetic: one accumulator, every term scaled by its spacing (laplacian_dd_pt)
                float W[12];
#pragma unroll
                for (int e = 0; e < 4; ++e) { W[e] = lft.v[e]; W[4 + e] = c.v[e]; W[8 + e] = rgt.v[e]; }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float col[2 * H + 1];
#pragma unroll
                    for (int io = 0; io <= 2 * H; ++io) col[io] = ring[(U + io) % R].v[e];
                    float lap = laplacian_dd_pt<H>(W, e, col, a.cz, a.dx2inv, a.dz2inv);
                    if (zedge || xedge) lap = (rowok && mlap[e]) ? lap : 0.0f;
                    const float upd = leapfrog_prod(c.v[e], ppt.v[e], (qv2[Q].v[e] * a.dt2) * lap);
                    res.v[e] = zedge ? (mupd[e] ? upd : ppt.v[e]) : upd;
                }
            } else {
                // packed pairs: same products and sums in the same order as laplacian_pt (see laplacian_pair); FAST numerics (NUM 1, any
                // dialect: the host hands over weights that carry their spacing): one chain of symmetric sums and fused multiply-adds
                const ZPairs zp = zpairs(lft, c, rgt);
                static_for<2>([&](auto PP) {
                    constexpr int P = decltype(PP)::value;
                    v2f lap2 = lap_pair<NUM, H, P>(zp, [&](auto IO) { return f4_pair(ring[(U + decltype(IO)::value) % R], P); }, cpk, c0p);
                    if (zedge || xedge) lap2 = v2f{(rowok && mlap[2 * P]) ? lap2.x : 0.0f, (rowok && mlap[2 * P + 1]) ? lap2.y : 0.0f};
                    if constexpr (LAPONLY) {
                        res.v[2 * P] = lap2.x;
                        res.v[2 * P + 1] = lap2.y;
                    } else {
                        const v2f prod2 = (f4_pair(qv2[Q], P) * a.dt2) * lap2;
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const int e = 2 * P + q;
                            const float upd = leapfrog_prod(c.v[e], ppt.v[e], q ? prod2.y : prod2.x);
                            res.v[e] = zedge ? (mupd[e] ? upd : ppt.v[e]) : upd;
                        }
                    }
                });
            }
            if constexpr (INJ != 0) {
                if (inj_here) {   // wave-uniform, rare
                    const bool injrow = (INJ == 1) ? (r == sv.inj_x) : ((r >= sv.inj_x) && (r < sv.inj_x + a.inj_n));
                    if (injrow) {
                        const float injv = (INJ == 1) ? inj_src : sload(sv.inj, r - sv.inj_x);
#pragma unroll
                        for (int e = 0; e < 4; ++e) res.v[e] = ihit[e] ? res.v[e] + injv : res.v[e];
                    }
                }
            }
            if constexpr (INJ == 3) {
                if (inj_here && r >= sv.inj_x - 3 && r <= sv.inj_x + 3) {   // ptsrc.c:49-55: s += ts * exp(-xn*xn - zn*zn), all float
                    const int dxa = r > sv.inj_x ? r - sv.inj_x : sv.inj_x - r;
                    const float g0 = a.gw[dxa][0], g1 = a.gw[dxa][1], g2 = a.gw[dxa][2], g3 = a.gw[dxa][3];   // wave-uniform kernarg reads
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int dz = z0 + e - a.inj_z, dza = dz < 0 ? -dz : dz;
                        const float g = dza == 0 ? g0 : (dza == 1 ? g1 : (dza == 2 ? g2 : g3));
                        if (dza <= 3 && mupd[e]) res.v[e] = res.v[e] + inj_src * g;      // ptsrc.c leaves out the cells beyond the grid edge: none lands in a padding column
                    }
                }
            }
            if constexpr (ILL) {
                // the value squared is the one stored below, source sample included and undamped; cells outside the update extents keep theirs
#pragma unroll
                for (int e = 0; e < 4; ++e) imr.v[e] = qim[Q].v[e] + res.v[e] * res.v[e];
                if (zedge) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) imr.v[e] = mupd[e] ? imr.v[e] : qim[Q].v[e];
                }
            }
            f4 txr;
            if constexpr (EXC == 1) {
                // the value compared and kept is the one stored below, source sample included and undamped; a NaN on either side compares
                // false, so it never wins and is never replaced; cells outside the update extents keep both words
                const float key = __int_as_float(a.exc_key);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool win = (__builtin_fabsf(res.v[e]) > __builtin_fabsf(qim[Q].v[e])) && (!zedge || mupd[e]);
                    imr.v[e] = win ? res.v[e] : qim[Q].v[e];
                    txr.v[e] = win ? key : qtx[Q].v[e];
                }
            }
            if constexpr (EXC == 2) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool pick = (__float_as_int(qtx[Q].v[e]) == a.exc_key) && (!zedge || mupd[e]);
                    imr.v[e] = pick ? res.v[e] : qim[Q].v[e];
                }
            }
            f4 fres;
            [[maybe_unused]] f4 fc_dtt;                             // DTT: the centre row of the source ring (F_{k+1})
            if constexpr (TWO) {
                // ---- the source field's own step on the same row: kernel_lap + kernel_time, no damping, no injection (R:317-318) ----
                // BORN: the scattered field's, with the damping of the forward step (what enters the computation this step) and no injection
                f4 fhal = fqhal[Q];
                if constexpr (BORN) {
                    if (wave_tap) {
                        taper_row(fring[(U + 2 * H) % R], tzc, znc, r + H);
                        taper_row(fhal, tzh, znh, r);
                        taper_row(fqpp[Q], tzc, znc, r);
                        if (a.pp_twice) taper_row(fqpp[Q], tzc, znc, r);
                    }
                }
                const f4 fc = fring[(U + H) % R];
                if constexpr (DTT) fc_dtt = fc;
                f4 flft, frgt;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float up = lane_up(fc.v[e]), dn = lane_down(fc.v[e]);
                    flft.v[e] = lane_first ? fhal.v[e] : up;
                    frgt.v[e] = lane_last ? fhal.v[e] : dn;
                }
                const ZPairs fzp = zpairs(flft, fc, frgt);
                static_for<2>([&](auto PP) {
                    constexpr int P = decltype(PP)::value;
                    v2f lap2 = lap_pair<NUM, H, P>(fzp, [&](auto IO) { return f4_pair(fring[(U + decltype(IO)::value) % R], P); }, cpk, c0p);
                    if (zedge || xedge) lap2 = v2f{(rowok && mlap[2 * P]) ? lap2.x : 0.0f, (rowok && mlap[2 * P + 1]) ? lap2.y : 0.0f};
                    const v2f prod2 = (f4_pair(qv2[Q], P) * a.dt2) * lap2;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const int e = 2 * P + q;
                        const float upd = leapfrog_prod(fc.v[e], fqpp[Q].v[e], q ? prod2.y : prod2.x);
                        fres.v[e] = zedge ? (mupd[e] ? upd : fqpp[Q].v[e]) : upd;
                    }
                });
            }
            if constexpr (BORN) {
                // ---- the scatter on the interior cells: no cell of them is damped (z >= nzb >= ztap), so c and ppt are the words the two
                // background buffers held; product and sum rounded separately; every other cell keeps its word (a select, no + 0.0f) ----
                if (born_here && (unsigned)(r - a.rec_x0) < (unsigned)a.rec_n) {
                    const bool born_kind = born_key_kind(a.exc_key) != 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float q = born_kind ? (res.v[e] - c.v[e]) - (c.v[e] - ppt.v[e]) : res.v[e];
                        const float sc = fres.v[e] + qm[Q].v[e] * q;
                        fres.v[e] = mborn[e] ? sc : fres.v[e];
                    }
                }
            }
            if constexpr (IMG && DTT) {
                // the second time difference of the source field meets r^{k+1}, the word this launch overwrites: no cell of C is damped, so
                // ppt is that word (a damping factor there is exactly 1.0f); three subtractions, product and sum rounded one by one; a select
                // elsewhere, so that the border cells of the launch extents keep their bits
                const bool dtt_row = born_here && (unsigned)(r - a.rec_x0) < (unsigned)a.rec_n;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float q = (fqpp[Q].v[e] - fc_dtt.v[e]) - (fc_dtt.v[e] - fres.v[e]);
                    const float im = qim[Q].v[e] + q * ppt.v[e];
                    imr.v[e] = (dtt_row && mborn[e]) ? im : qim[Q].v[e];
                }
            } else if constexpr (IMG) {
                // kernel_img (R:133-144) correlates with the NEW receiver field; the sibling's rtm_main stores the CURRENT one
                // (rwf[it] = P, rtm_main.cpp:211-215), an interior point of which carries damping factors of exactly 1.0f
#pragma unroll
                for (int e = 0; e < 4; ++e) imr.v[e] = qim[Q].v[e] + (BACK ? fres.v[e] : qps[Q].v[e]) * (DD ? c.v[e] : res.v[e]);
                if (zedge) {      // kernel_img's launch covers interior columns j < zlim only (R:133-144)
#pragma unroll
                    for (int e = 0; e < 4; ++e) imr.v[e] = (z0 + e < a.img_z1) ? imr.v[e] : qim[Q].v[e];
                }
            }
            if (!partial) {
                f4_store(sv.out + (size_t)r * pitch, voff, res);
                if constexpr (IMG) f4_store(sv.img + (size_t)r * pitch, voff, imr);
                if constexpr (ILL) f4_store(sv.img + (size_t)r * pitch, voff, imr);
                if constexpr (EXC != 0) f4_store(sv.img + (size_t)r * pitch, voff, imr);
                if constexpr (EXC == 1) f4_store(texc_w + (size_t)r * pitch, voff, txr);
                if constexpr (TWO) f4_store(sv.fpp + (size_t)r * pitch, voff, fres);
            } else if (act) {
                f4_store(sv.out + (size_t)r * pitch, voff, res);
                if constexpr (IMG) f4_store(sv.img + (size_t)r * pitch, voff, imr);
                if constexpr (ILL) f4_store(sv.img + (size_t)r * pitch, voff, imr);
                if constexpr (EXC != 0) f4_store(sv.img + (size_t)r * pitch, voff, imr);
                if constexpr (EXC == 1) f4_store(texc_w + (size_t)r * pitch, voff, txr);
                if constexpr (TWO) f4_store(sv.fpp + (size_t)r * pitch, voff, fres);
            }
            if constexpr (BORN) {      // the trace samples of both new fields (either gather may be absent: wave-uniform)
                if (a.rec) f1_store_arr(array_rsrc(sv.rec, (unsigned)a.rec_n * 4u), rec_offset(rec_lane, r, a.rec_x0, a.rec_n), f4_pick(fres, a.rec_z & 3));
                if (a.texc) f1_store_arr(array_rsrc(rec0_w, (unsigned)a.rec_n * 4u), rec_offset(rec_lane, r, a.rec_x0, a.rec_n), f4_pick(res, a.rec_z & 3));
            }
            if constexpr (REC) f1_store_arr(array_rsrc(sv.rec, (unsigned)a.rec_n * 4u), rec_offset(rec_lane, r, a.rec_x0, a.rec_n), f4_pick(res, a.rec_z & 3));

            // ---- refill the slots this row just freed (look-ahead loads) ----------------------
            ring[U] = load_p(r - H + R);
            {
                const int nr = min(r + PF, xe - 1);
                qhal[Q] = load_halo(nr);
                if constexpr (!LAPONLY) {
                    qpp[Q] = load_plain(sv.pp, nr);
                    qv2[Q] = load_plain(sv.v2, nr);
                }
                if constexpr (IMG) {
                    if constexpr (!BACK) qps[Q] = load_plain(sv.psrc, nr);
                    qim[Q] = load_plain(sv.img, nr);
                }
                if constexpr (ILL) qim[Q] = load_plain(sv.img, nr);
                if constexpr (EXC != 0) {
                    qim[Q] = load_plain(sv.img, nr);
                    qtx[Q] = load_plain(texc_w, nr);
                }
                if constexpr (TWO) {
                    fqhal[Q] = load_fhalo(nr);
                    fqpp[Q] = load_plain(sv.fpp, nr);
                }
                if constexpr (BORN) qm[Q] = load_plain(a.img, nr);
            }
            if constexpr (TWO) fring[U] = load_f(r - H + R);
        }
        // keep the look-ahead loads where they were issued: without this the machine scheduler
        // sinks each load to one row before its first use to save registers, which turns the
        // software prefetch into a load-use stall every row
        __builtin_amdgcn_sched_barrier(0);
    };

    int rb = xa;
    // bulk: whole turns of the ring, no tests, exact s_waitcnt bookkeeping
    for (; rb + R <= xe; rb += R)
        static_for<R>([&](auto UU) { row_step(rb, UU, std::false_type{}); });
    // remaining rows (< R)
    if (rb < xe)
        static_for<R>([&](auto UU) { row_step(rb, UU, std::true_type{}); });
}

// Tile placement of the one-step kernels: the shot a block works on and the strip and rows of each of its four waves.  Declares the ShotView
// `sv` of shot blockIdx.y (a batch of independent shots of one geometry fills the chip where one small grid cannot), `lane`, the first column
// `zs` of the wave's strip and its rows [`xa`, `xe`), and leaves the kernel where the wave has no tile (no barrier follows).
// XCD-aware block remap: blocks b and b + 8 share an XCD (round-robin dispatch), so each XCD gets a contiguous run of logical blocks = a
// contiguous band of x rows whose chunk halos it re-reads from its own L2.  Placement only changes speed, never results.  a.wz = waves of a
// block laid along z (1, 2 or 4); the others take consecutive chunks.  A macro for the reason written down at FDW_PIPE_TILE (fdw_stepn.hip).
#define FDW_STEP_TILE(a, sv, lane, zs, xa, xe)                                                                           \
    const int shot = blockIdx.y;                                                                                         \
    const long long o = shot * a.bstride;                                                                                \
    const ShotView sv{a.p + o, a.pp + o, (a.out ? a.out : a.pp) + o, a.v2 + shot * a.v2_bstride, a.psrc + o, a.fpp + o,  \
                      a.img + o, a.inj + shot * a.inj_bstride, a.inj_x + shot * a.inj_dx, a.rec + shot * a.rec_bstride}; \
    const int lane = threadIdx.x & 63;                                                                                   \
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                                      \
    const int bid = blockIdx.x;                                                                                          \
    const int L = (bid & 7) * a.nper + (bid >> 3);                                                                       \
    if (L >= a.nblk) return;                                                                                             \
    const int zb = L % a.nzblk;                                                                                          \
    const int xb = L / a.nzblk;                                                                                          \
    const int wz = a.wz;                                                                                                 \
    const int strip = zb * wz + (w & (wz - 1));                                                                          \
    const int chunk = xb * (4 / wz) + (w / wz);                                                                          \
    const int zs = strip * 256;                                                                                          \
    if (zs >= a.pitch) return;                                                                                           \
    const int xa = a.r0 + chunk * a.xchunk;                                                                              \
    const int xe = min(xa + a.xchunk, a.r1);                                                                             \
    if (xa >= xe) return;

template <int H, bool TAPER, int INJ, bool IMG, bool LAPONLY, int PF, bool DD = false, bool BACK = false, int NUM = 0>
__global__ __launch_bounds__(256) void fdw_step_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, TAPER, INJ, IMG, LAPONLY, PF, DD, BACK, NUM>(a, sv, lane, zs, xa, xe);
}

// the forward step (FDW_MODE_FWD) that also records its trace samples (FDW_MODE_FWD_REC; batched like the others: rec + shot * rec_bstride).
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_rec_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 1, false, false, PF, false, false, NUM, true>(a, sv, lane, zs, xa, xe);
}

// the forward step (FDW_MODE_FWD) that also accumulates the source illumination (FDW_MODE_FWD_ILLUM: a.img is the accumulator, +8 B/point/step).
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_illum_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 1, false, false, PF, false, false, NUM, false, true>(a, sv, lane, zs, xa, xe);
}

// the forward step that records its trace samples AND accumulates the source illumination (FDW_MODE_FWD_REC_ILLUM: the forward loop of
// fdw_shot_residual with an accumulator): the sample is fdw_step_rec_kernel's single 32-bit store, the accumulator row rides the pointwise
// queue as in fdw_step_illum_kernel.
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_rec_illum_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 1, false, false, PF, false, false, NUM, true, true>(a, sv, lane, zs, xa, xe);
}

// the forward step driven by a LINE source instead of the point source (FDW_MODE_FWD_LINE*: fdw_dev_line_steps): TAPER + INJ = 2 without imaging,
// one sample per row of [inj_x, inj_x + inj_n) added on column inj_z after the leap-frog, exactly as the receiver pass adds its trace samples.
// REC: the trace row of the new field, line sample included; ILL: its square into the accumulator (a.img).
template <int H, int PF, bool REC, bool ILL, int NUM>
__global__ __launch_bounds__(256) void fdw_step_line_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 2, false, false, PF, false, false, NUM, REC, ILL>(a, sv, lane, zs, xa, xe);
}

// the line-source step that records its trace samples AND accumulates the source illumination (FDW_MODE_FWD_LINE_REC_ILLUM: the forward loop of
// fdw_shot_line_residual with an accumulator, fdw_dev_line_record_illum_steps): fdw_step_rec_illum_kernel with INJ = 2 -- sample and square are
// the stored new field, line sample included.  A kernel of its own name, as the point source's combined kernel is.
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_line_rec_illum_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 2, false, false, PF, false, false, NUM, true, true>(a, sv, lane, zs, xa, xe);
}

// the forward step (FDW_MODE_FWD) that also keeps the excitation maps (FDW_MODE_FWD_EXC, fdw_dev_excite_steps): a.img is amp, a.texc the time
// map, both read and written once per cell, +16 B/point/step.  A batch: amp travels as sv.img, the map of shot b is a.texc + b * a.bstride.
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_exc_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 1, false, false, PF, false, false, NUM, false, false, 1>(a, sv, lane, zs, xa, xe);
}

// the line-source step that also takes the excitation pick (FDW_MODE_FWD_LINE_PICK, fdw_dev_line_pick_steps): fdw_step_line_kernel's step, then
// exc = the new field, line sample included, where texc equals a.exc_key.  a.img is exc.
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_line_pick_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 2, false, false, PF, false, false, NUM, false, false, 2>(a, sv, lane, zs, xa, xe);
}

// Born modelling (FDW_MODE_BORN, fdw_dev_born_steps): the forward step on the background pair, the same step without a source on the scattered
// pair in a second register ring, v2 read once for both, and the scatter and the trace samples in registers before the two stores.  Six reads
// (p, pp, du_p, du_pp, v2, m) and two writes: 36 B/point/step against the 32 of two plain steps.  The kind is a launch argument (fdw_born.h): the second
// difference costs three subtractions on registers the leap-frog already holds.
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_born_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 1, false, false, PF, false, false, NUM, false, false, 0, true>(a, sv, lane, zs, xa, xe);
}

// Born modelling driven by a LINE source (FDW_MODE_BORN_LINE, fdw_dev_born_line_steps): fdw_step_born_kernel with INJ = 2 -- the background's new
// field takes one sample per row of [inj_x, inj_x + inj_n) on column inj_z after the leap-frog, and that field, line samples included, is what
// the scatter and the background trace row see.  The scattered pair takes no injection.  One sample load per row more than the point source.
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_line_born_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 2, false, false, PF, false, false, NUM, false, false, 0, true>(a, sv, lane, zs, xa, xe);
}

// Second-time-difference imaging (FDW_MODE_BACK_DTT, fdw_dev_back_iter_dtt): the fused backward iteration (BACK) with the DTT value of its
// imaging epilogue.  The loads and stores are BACK's, 36 B/point; three subtractions and one more live mask on top of it.
template <int H, int PF, int NUM>
__global__ __launch_bounds__(256) void fdw_step_back_dtt_kernel(const StepArgs a)
{
    FDW_STEP_TILE(a, sv, lane, zs, xa, xe)
    march<H, true, 2, true, false, PF, false, true, NUM, false, false, 0, false, true>(a, sv, lane, zs, xa, xe);
}

#if FDW_TU == 0
// ------------------------------------------------------------------------------------------------
// generic-order kernel: any even order up to FDW_MAX_ORDER, one thread per point, every tap from
// global memory (L1/L2 absorb the reuse).  Same arithmetic, same lazy-taper rules; used for orders
// the register-ring kernel is not instantiated for, and as an independent cross-check of it.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float generic_p(const StepArgs& a, int row, int z, bool taper)
{
    float v = a.p[(size_t)row * a.pitch + z];
    if (taper && z < a.ztap) v = taper1(v, a.taperz[z], true, row < a.tz_x1, a.txfac[row]);
    return v;
}

template <bool REC>
__device__ __forceinline__ void generic_point(const StepArgs& a, int h, int taper, int injmode, int img, int laponly)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    const int r = a.r0 + blockIdx.y;
    if (z >= a.pitch || r >= a.r1) return;
    const size_t k = (size_t)r * a.pitch + z;
    float lap = 0.0f;
    if (r >= a.lap_x0 && r < a.lap_x1 && z >= a.lap_z0 && z < a.lap_z1) {
        if (a.numerics) {      // FAST: one chain of symmetric sums and fused multiply-adds (fdw_device.h)
            lap = a.c0 * generic_p(a, r, z, taper);
            for (int k = 1; k <= h; ++k)
                lap = laplacian_fast_tap(lap, generic_p(a, r, z - k, taper), generic_p(a, r, z + k, taper), generic_p(a, r - k, z, taper),
                                         generic_p(a, r + k, z, taper), a.gcz[h - k], a.gcx[h - k]);
        } else {
            float acmz = 0.0f, acmx = 0.0f;
            for (int io = 0; io <= 2 * h; ++io) {
                acmz = acmz + generic_p(a, r, z + io - h, taper) * a.gcz[io];
                acmx = acmx + generic_p(a, r + io - h, z, taper) * a.gcx[io];
            }
            lap = acmz + acmx;
        }
    }
    float out;
    if (laponly) {
        out = lap;
    } else {
        const float pc = generic_p(a, r, z, taper);
        float ppv = a.pp[k];
        if (taper && z < a.ztap) {
            const bool rowtz = r < a.tz_x1;
            const float txr = a.txfac[r], tz = a.taperz[z];
            ppv = taper1(ppv, tz, true, rowtz, txr);
            if (a.pp_twice) ppv = taper1(ppv, tz, true, rowtz, txr);
        }
        const float upd = leapfrog_pt(pc, ppv, a.v2[k], a.dt2, lap);
        out = (z < a.upd_z1) ? upd : ppv;
        if (injmode == 1) {
            if (r == a.inj_x && z == a.inj_z) out = out + a.inj[0];
        } else if (injmode == 2) {
            if (r >= a.inj_x && r < a.inj_x + a.inj_n && z == a.inj_z) out = out + a.inj[r - a.inj_x];
        }
    }
    a.pp[k] = out;
    if (REC && z == a.rec_z && (unsigned)(r - a.rec_x0) < (unsigned)a.rec_n) a.rec[r - a.rec_x0] = out;      // this step's trace sample
    if (img) a.img[k] = a.img[k] + a.psrc[k] * out;
}

__global__ __launch_bounds__(256) void fdw_generic_kernel(const StepArgs a, int h, int taper, int injmode,
                                                          int img, int laponly)
{
    generic_point<false>(a, h, taper, injmode, img, laponly);
}
// FDW_MODE_FWD_REC / FWD_LINE_REC: the forward step (injmode 1 point source, 2 line source) and its trace sample (one thread per point: no
// march loop to keep free of branches)
__global__ __launch_bounds__(256) void fdw_generic_rec_kernel(const StepArgs a, int h, int injmode)
{
    generic_point<true>(a, h, 1, injmode, 0, 0);
}

// Source illumination behind the generic-order kernel (orders above 8, forced generic): illum += f (*) f with f the field the step just
// stored, on the cells the step updated.  Product and sum are rounded separately (the file is built with -ffp-contract=off).
__global__ __launch_bounds__(256) void fdw_illum_add_kernel(const float* f, float* illum, int pitch, int r0, int z1)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z >= z1) return;
    const size_t k = (size_t)(r0 + blockIdx.y) * pitch + z;
    const float u = f[k];
    illum[k] = illum[k] + u * u;
}

// The excitation maps behind the generic-order kernel: f is the field the step just stored; where |f| > |amp| strictly, amp = f and
// texc = key (= it + 1), on the cells the step updated.  A NaN on either side compares false.
__global__ __launch_bounds__(256) void fdw_exc_select_kernel(const float* f, float* amp, int* texc, int pitch, int r0, int z1, int key)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z >= z1) return;
    const size_t k = (size_t)(r0 + blockIdx.y) * pitch + z;
    const float u = f[k];
    if (__builtin_fabsf(u) > __builtin_fabsf(amp[k])) {
        amp[k] = u;
        texc[k] = key;
    }
}

// The excitation pick behind the generic-order kernel: exc = f where texc == key (= top - it), on the cells the step updated.
__global__ __launch_bounds__(256) void fdw_exc_pick_kernel(const float* f, const int* texc, float* exc, int pitch, int r0, int z1, int key)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z >= z1) return;
    const size_t k = (size_t)(r0 + blockIdx.y) * pitch + z;
    if (texc[k] == key) reinterpret_cast<unsigned*>(exc)[k] = reinterpret_cast<const unsigned*>(f)[k];
}

// Born modelling behind step kernels that do not scatter themselves (orders above 8, forced generic, FDW_NO_BORN_FUSED=1).  The background
// step overwrites B (the older level) with U, so the second difference needs (A - B) kept: w = a (-) b on the interior cells, before that step.
__global__ __launch_bounds__(256) void fdw_born_diff_kernel(const float* a, const float* b, float* w, int pitch, int x0, int z0, int z1)
{
    const int z = z0 + blockIdx.x * 256 + threadIdx.x;
    if (z >= z1) return;
    const size_t k = (size_t)(x0 + blockIdx.y) * pitch + z;
    w[k] = a[k] - b[k];
}

// ... and after both steps: d = d (+) m (*) q on the interior cells [z0, z1) of rows x0 + blockIdx.y, q = u (kind 0) or (u (-) a) (-) w (kind 1),
// product and sum rounded separately, every other cell left alone; then this step's trace samples of the row at column gz (rec: the scattered
// field after the scatter, rec0: the background; either may be NULL).  Threads cover columns [0, zcols) because gz may lie outside [z0, z1).
__global__ __launch_bounds__(256) void fdw_born_scatter_kernel(const float* u, const float* a, const float* w, const float* m, float* d, int kind, int pitch,
                                                               int x0, int z0, int z1, int zcols, int gz, float* rec, float* rec0)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    if (z >= zcols) return;
    const size_t k = (size_t)(x0 + blockIdx.y) * pitch + z;
    const bool in = (z >= z0) && (z < z1);
    if (!in && z != gz) return;
    const float uv = u[k];
    float dv = d[k];
    if (in) {
        const float q = kind ? (uv - a[k]) - w[k] : uv;
        dv = dv + m[k] * q;
        d[k] = dv;
    }
    if (z == gz) {
        if (rec) rec[blockIdx.y] = dv;
        if (rec0) rec0[blockIdx.y] = uv;
    }
}

// One term of second-time-difference imaging on the cells C = rows [x0, x0 + gridDim.y) x columns [z0, z1) (fdwave.h, "DTT imaging"):
// img = img (+) ((a (-) b) (-) (b (-) c)) (*) r, every operation rounded on its own; pre: a already holds the first difference (a (-) b taken
// by fdw_born_diff_kernel before the step that overwrote its operand).  blockIdx.z = shot of a batch (every array bstride words further on).
// Behind the tail of the DTT backward loop and behind step kernels without the fused epilogue (orders above 8, forced generic,
// FDW_NO_FUSED_BACK=1).
__global__ __launch_bounds__(256) void fdw_dtt_image_kernel(const float* a, const float* b, const float* c, const float* r, float* img, int pre, int pitch,
                                                            int x0, int z0, int z1, long long bstride)
{
    const int z = z0 + blockIdx.x * 256 + threadIdx.x;
    if (z >= z1) return;
    const size_t k = (size_t)((long long)blockIdx.z * bstride) + (size_t)(x0 + blockIdx.y) * pitch + z;
    const float bv = b[k];
    const float d1 = pre ? a[k] : a[k] - bv;
    const float q = d1 - (bv - c[k]);
    img[k] = img[k] + q * r[k];
}

// ------------------------------------------------------------------------------------------------
// the one T() the lazy scheme owes d_p before it leaves the device (fd_forward's D2H of d_p, R:285)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fdw_taper_finalize_kernel(float* f, const float* taperz, const float* txfac,
                                                                 int pitch, int nxl, int ztap, int tz_x1)
{
    const int z = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (z >= ztap || z >= pitch || r >= nxl) return;
    const size_t k = (size_t)r * pitch + z;
    f[k] = taper1(f[k], taperz[z], true, r < tz_x1, txfac[r]);
}

// ------------------------------------------------------------------------------------------------
// device self test of the two hardware behaviours the kernels rely on:
//   out[0..63]    = lane_up(src)     (lane i takes lane i-1's value; lane 0's result is unspecified)
//   out[64..127]  = lane_down(src)   (lane i takes lane i+1's value; lane 63's result is unspecified)
//   out[128..383] = a 64 x float4 row written with the range-predicated buffer store: lanes 2..61 store at
//                   their own offset, the others at 0xFFFFFFF0 and must be dropped by the descriptor check
// ------------------------------------------------------------------------------------------------
// Image post-processing: the second-order Laplacian filter of laplace.f90:25-29 on a dense [nx][nz] image, in the
// order the Fortran expression spells, frame left at zero.  HBM bound and tiny (one read, one write per point).
__global__ __launch_bounds__(256) void fdw_image_lap_kernel(const float* img, float* out, int nx, int nz, float dx, float dz)
{
    const int iz = blockIdx.x * 256 + threadIdx.x, ix = blockIdx.y;
    if (iz >= nz) return;
    const size_t k = (size_t)ix * nz + iz;
    float r = 0.0f;
    if (ix >= 1 && ix < nx - 1 && iz >= 1 && iz < nz - 1) {
        const float c = img[k];
        r = ((img[k + 1] - 2.0f * c) + img[k - 1]) / (dz * dz) + ((img[k + nz] - 2.0f * c) + img[k - nz]) / (dx * dx);
    }
    out[k] = r;
}

// Receiver rows the reference injects (kernel_sism, R:124-131) and images (kernel_img, R:133-144) although its truncated launch
// extents never time-step them: rows [xlim, nxb + min(nx, xlim)), which exist only when the x border is narrower than nxe - xlim
// (decks with nxb < 7).  Their field values are static apart from this injection, but the neighbouring time-stepped row reads them.
// One thread per cell of those rows: pp(row, gz) += sample; img(row, z) += psrc(row, z) * pp(row, z) for the imaged columns.
__global__ __launch_bounds__(256) void fdw_static_rows_kernel(float* pp, const float* psrc, float* img, const float* samples, int pitch, int row0,
                                                              int gz, int img_z0, int img_z1)
{
    const int z = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (z >= pitch) return;
    const size_t k = (size_t)(row0 + i) * pitch + z;
    float v = pp[k];
    if (z == gz) {
        v = v + samples[i];
        pp[k] = v;
    }
    if (z >= img_z0 && z < img_z1) img[k] = img[k] + psrc[k] * v;
}

// Trace samples of receiver rows the loop never time-steps (compat extents, rows >= xlim): the reference's d_pp there holds, at the end of
// iteration it0 + k, what its d_p held before the loop for even k and what its d_pp held for odd k (the pointers swap every iteration,
// R:260-262, and no kernel writes those rows).  rec -> the row of iteration it0; blockIdx.y = shot of a batch.
__global__ __launch_bounds__(256) void fdw_record_static_kernel(const float* p0, const float* pp0, float* rec, int pitch, int row0, int nrows, int gz,
                                                                int rec_x0, int rec_n, int nsteps, long long bstride, long long rec_bstride)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nrows * nsteps) return;
    const int k = t / nrows, row = row0 + t % nrows;
    const long long b = blockIdx.y;
    rec[b * rec_bstride + (long long)k * rec_n + (row - rec_x0)] = ((k & 1) ? pp0 : p0)[b * bstride + (long long)row * pitch + gz];
}

// Wavefield snapshot (fdw_dev_snapshot, fdw_shot_snaps): frame[a][b] = f(x0 + a dec, z0 + b dec) for a < nxs, b < nzs -- the interior of one
// field cropped and decimated into one dense frame, z fastest like dir.image.  Lanes run along z: the stores are coalesced, the loads too
// when dec = 1.  No arithmetic: the values travel as 32-bit words, so NaN payloads, -0 and subnormals arrive as they are.  blockIdx.y strides
// over the frame rows (a grid holds 65 535 of them at most).
__global__ __launch_bounds__(256) void fdw_snapshot_kernel(const float* f, float* frame, int pitch, int x0, int z0, int dec, int nxs, int nzs)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nzs) return;
    const unsigned* src = reinterpret_cast<const unsigned*>(f);
    unsigned* dst = reinterpret_cast<unsigned*>(frame);
    const size_t col = (size_t)z0 + (size_t)b * (size_t)dec;
    for (int a = blockIdx.y; a < nxs; a += gridDim.y)
        dst[(size_t)a * (size_t)nzs + (size_t)b] = src[((size_t)x0 + (size_t)a * (size_t)dec) * (size_t)pitch + col];
}

__global__ void fdw_selftest_kernel(const float* src, float* out)
{
    const int t = threadIdx.x;
    out[t] = lane_up(src[t]);
    out[64 + t] = lane_down(src[t]);
    f4 v;
    v.v[0] = v.v[1] = v.v[2] = v.v[3] = src[t];
    const unsigned off = (t >= 2 && t <= 61) ? (unsigned)t * 16u : 0xFFFFFFF0u;
    f4_store_rsrc(out + 128, 64u * 16u, off, v);
}

#endif   // FDW_TU == 0

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// the mode table of the RTM dialect: exact arithmetic in FDW_TU 0, FAST numerics in FDW_TU 2 (NUM = 1: prefetch distance 2 only, the tuning knob
// exists for the exact order-8 kernels)
#if FDW_TU == 0 || FDW_TU == 2
template <int H, int PF, int NUM>
static hipError_t launch_rtm_hp(const StepArgs& a, int mode, hipStream_t s)
{
    const dim3 grid(8 * a.nper, a.nbatch > 1 ? a.nbatch : 1), block(256);
    switch (mode) {
    case FDW_MODE_FWD:   hipLaunchKernelGGL((fdw_step_kernel<H, true, 1, false, false, PF, false, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_PLAIN: hipLaunchKernelGGL((fdw_step_kernel<H, false, 0, false, false, PF, false, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_RECV:  hipLaunchKernelGGL((fdw_step_kernel<H, true, 2, true, false, PF, false, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_LAP:   hipLaunchKernelGGL((fdw_step_kernel<H, false, 0, false, true, PF, false, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_BACK:  hipLaunchKernelGGL((fdw_step_kernel<H, true, 2, true, false, PF, false, true, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_REC: hipLaunchKernelGGL((fdw_step_rec_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_ILLUM: hipLaunchKernelGGL((fdw_step_illum_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_REC_ILLUM: hipLaunchKernelGGL((fdw_step_rec_illum_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE: hipLaunchKernelGGL((fdw_step_line_kernel<H, PF, false, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE_REC: hipLaunchKernelGGL((fdw_step_line_kernel<H, PF, true, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE_ILLUM: hipLaunchKernelGGL((fdw_step_line_kernel<H, PF, false, true, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE_REC_ILLUM: hipLaunchKernelGGL((fdw_step_line_rec_illum_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_EXC: hipLaunchKernelGGL((fdw_step_exc_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE_PICK: hipLaunchKernelGGL((fdw_step_line_pick_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_BORN: hipLaunchKernelGGL((fdw_step_born_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_BORN_LINE: hipLaunchKernelGGL((fdw_step_line_born_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_BACK_DTT: hipLaunchKernelGGL((fdw_step_back_dtt_kernel<H, PF, NUM>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
#endif

#if FDW_TU == 0
hipError_t launch_step_dd(const StepArgs& a, int h, int mode, int pf, hipStream_t s);        // fdw_step1_dd.o
hipError_t launch_step_fastnum(const StepArgs& a, int h, int mode, hipStream_t s);           // fdw_step1_fast.o

hipError_t launch_step_fast(const StepArgs& a, int h, int mode, int pf, hipStream_t s)
{
    if (a.nper <= 0) return hipSuccess;
    if (mode == FDW_MODE_MOD || mode == FDW_MODE_DD_FWD || mode == FDW_MODE_DD_RECV) return launch_step_dd(a, h, mode, pf, s);
    if (a.numerics) return launch_step_fastnum(a, h, mode, s);
    if (h == 4) {
        switch (pf) {
        case 1: return launch_rtm_hp<4, 1, 0>(a, mode, s);
        case 3: return launch_rtm_hp<4, 3, 0>(a, mode, s);
        default: return launch_rtm_hp<4, 2, 0>(a, mode, s);
        }
    }
    switch (h) {
    case 1: return launch_rtm_hp<1, 2, 0>(a, mode, s);
    case 2: return launch_rtm_hp<2, 2, 0>(a, mode, s);
    case 3: return launch_rtm_hp<3, 2, 0>(a, mode, s);
    default: return hipErrorInvalidValue;
    }
}
#elif FDW_TU == 1
// the sibling's dialects; FAST numerics (NUM = 1, prefetch distance 2): the RTM dialect's symmetric-sum / fma chain on weights that carry their spacing
template <int H, int PF, int NUM>
static hipError_t launch_dd_hp(const StepArgs& a, int mode, hipStream_t s)
{
    const dim3 grid(8 * a.nper, a.nbatch > 1 ? a.nbatch : 1), block(256);
    switch (mode) {
    case FDW_MODE_MOD:     hipLaunchKernelGGL((fdw_step_kernel<H, true, 3, false, false, PF, true, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_DD_FWD:  hipLaunchKernelGGL((fdw_step_kernel<H, true, 1, false, false, PF, true, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_DD_RECV: hipLaunchKernelGGL((fdw_step_kernel<H, true, 2, true, false, PF, true, false, NUM>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
hipError_t launch_step_dd(const StepArgs& a, int h, int mode, int pf, hipStream_t s)
{
    if (a.numerics) {
        switch (h) {
        case 1: return launch_dd_hp<1, 2, 1>(a, mode, s);
        case 2: return launch_dd_hp<2, 2, 1>(a, mode, s);
        case 3: return launch_dd_hp<3, 2, 1>(a, mode, s);
        case 4: return launch_dd_hp<4, 2, 1>(a, mode, s);
        default: return hipErrorInvalidValue;
        }
    }
    if (h == 4) {
        switch (pf) {
        case 1: return launch_dd_hp<4, 1, 0>(a, mode, s);
        case 3: return launch_dd_hp<4, 3, 0>(a, mode, s);
        default: return launch_dd_hp<4, 2, 0>(a, mode, s);
        }
    }
    switch (h) {
    case 1: return launch_dd_hp<1, 2, 0>(a, mode, s);
    case 2: return launch_dd_hp<2, 2, 0>(a, mode, s);
    case 3: return launch_dd_hp<3, 2, 0>(a, mode, s);
    default: return hipErrorInvalidValue;
    }
}
#elif FDW_TU == 2
hipError_t launch_step_fastnum(const StepArgs& a, int h, int mode, hipStream_t s)
{
    switch (h) {
    case 1: return launch_rtm_hp<1, 2, 1>(a, mode, s);
    case 2: return launch_rtm_hp<2, 2, 1>(a, mode, s);
    case 3: return launch_rtm_hp<3, 2, 1>(a, mode, s);
    case 4: return launch_rtm_hp<4, 2, 1>(a, mode, s);
    default: return hipErrorInvalidValue;
    }
}
#endif

#if FDW_TU == 0
hipError_t launch_step_generic(const StepArgs& a, int h, int mode, hipStream_t s)
{
    if (a.r1 <= a.r0) return hipSuccess;
    const dim3 grid((a.pitch + 255) / 256, a.r1 - a.r0), block(256);
    if (mode == FDW_MODE_FWD_REC || mode == FDW_MODE_FWD_LINE_REC) {
        hipLaunchKernelGGL(fdw_generic_rec_kernel, grid, block, 0, s, a, h, mode == FDW_MODE_FWD_REC ? 1 : 2);
        return hipGetLastError();
    }
    const int taper = (mode == FDW_MODE_FWD || mode == FDW_MODE_RECV || mode == FDW_MODE_FWD_LINE);
    const int inj = (mode == FDW_MODE_FWD) ? 1 : ((mode == FDW_MODE_RECV || mode == FDW_MODE_FWD_LINE) ? 2 : 0);
    hipLaunchKernelGGL(fdw_generic_kernel, grid, block, 0, s, a, h, taper, inj, mode == FDW_MODE_RECV ? 1 : 0,
                       mode == FDW_MODE_LAP ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_illum_add(const float* f, float* illum, int pitch, int r0, int r1, int z1, hipStream_t s)
{
    const int zc = z1 < pitch ? z1 : pitch;
    if (r1 <= r0 || zc <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_illum_add_kernel, dim3((zc + 255) / 256, r1 - r0), dim3(256), 0, s, f, illum, pitch, r0, zc);
    return hipGetLastError();
}

hipError_t launch_exc_select(const float* f, float* amp, int* texc, int pitch, int r0, int r1, int z1, int key, hipStream_t s)
{
    const int zc = z1 < pitch ? z1 : pitch;
    if (r1 <= r0 || zc <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_exc_select_kernel, dim3((zc + 255) / 256, r1 - r0), dim3(256), 0, s, f, amp, texc, pitch, r0, zc, key);
    return hipGetLastError();
}

hipError_t launch_exc_pick(const float* f, const int* texc, float* exc, int pitch, int r0, int r1, int z1, int key, hipStream_t s)
{
    const int zc = z1 < pitch ? z1 : pitch;
    if (r1 <= r0 || zc <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_exc_pick_kernel, dim3((zc + 255) / 256, r1 - r0), dim3(256), 0, s, f, texc, exc, pitch, r0, zc, key);
    return hipGetLastError();
}

hipError_t launch_born_diff(const float* a, const float* b, float* w, int pitch, int x0, int x1, int z0, int z1, hipStream_t s)
{
    if (x1 <= x0 || z1 <= z0) return hipSuccess;
    hipLaunchKernelGGL(fdw_born_diff_kernel, dim3((z1 - z0 + 255) / 256, x1 - x0), dim3(256), 0, s, a, b, w, pitch, x0, z0, z1);
    return hipGetLastError();
}

hipError_t launch_born_scatter(const float* u, const float* a, const float* w, const float* m, float* d, int kind, int pitch, int x0, int x1, int z0,
                               int z1, int zcols, int gz, float* rec, float* rec0, hipStream_t s)
{
    if (x1 <= x0 || zcols <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_born_scatter_kernel, dim3((zcols + 255) / 256, x1 - x0), dim3(256), 0, s, u, a, w, m, d, kind, pitch, x0, z0, z1, zcols, gz, rec,
                       rec0);
    return hipGetLastError();
}

hipError_t launch_dtt_image(const float* a, const float* b, const float* c, const float* r, float* img, int pre, int pitch, int x0, int x1, int z0, int z1,
                            int nbatch, long long bstride, hipStream_t s)
{
    if (x1 <= x0 || z1 <= z0) return hipSuccess;
    hipLaunchKernelGGL(fdw_dtt_image_kernel, dim3((z1 - z0 + 255) / 256, x1 - x0, nbatch > 1 ? nbatch : 1), dim3(256), 0, s, a, b, c, r, img, pre, pitch, x0,
                       z0, z1, bstride);
    return hipGetLastError();
}

hipError_t launch_taper_finalize(float* f, const float* taperz, const float* txfac, int pitch, int nxl, int ztap,
                                 int tz_x1, hipStream_t s)
{
    if (ztap <= 0 || nxl <= 0) return hipSuccess;
    const dim3 grid((ztap + 255) / 256, nxl), block(256);
    hipLaunchKernelGGL(fdw_taper_finalize_kernel, grid, block, 0, s, f, taperz, txfac, pitch, nxl, ztap, tz_x1);
    return hipGetLastError();
}

// ---- image comparison (the reference's offline tool models/marmousi/psnr: "./psnr file1 file2") ----------------------------------------
// diff = a - b (fp32, as the tool writes it to dir.output); per block: sums of the squares (a-b)^2 and b^2 in double, max |b|.
// The tool itself adds the squares one after the other into fp32 sums; a parallel reduction cannot reproduce that order, so the sums here are
// those of the same terms carried in double (they differ from the tool's in the 6th-7th digit, where the tool carries its rounding).
__global__ __launch_bounds__(256) void fdw_image_compare_kernel(const float* a, const float* b, size_t n, float* diff, double* part)
{
    __shared__ double sh[3][256];
    double sd = 0.0, sb = 0.0, mx = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float x = a[i], y = b[i];
        const float d = x - y;
        if (diff) diff[i] = d;
        sd += (double)d * (double)d;
        sb += (double)y * (double)y;
        mx = fmax(mx, (double)fabsf(y));
    }
    sh[0][threadIdx.x] = sd; sh[1][threadIdx.x] = sb; sh[2][threadIdx.x] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
            sh[2][threadIdx.x] = fmax(sh[2][threadIdx.x], sh[2][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x * 3 + 0] = sh[0][0];
        part[blockIdx.x * 3 + 1] = sh[1][0];
        part[blockIdx.x * 3 + 2] = sh[2][0];
    }
}
__global__ __launch_bounds__(256) void fdw_image_compare_final_kernel(const double* part, int nblocks, double* out)
{
    __shared__ double sh[3][256];
    double sd = 0.0, sb = 0.0, mx = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        sd += part[i * 3];
        sb += part[i * 3 + 1];
        mx = fmax(mx, part[i * 3 + 2]);
    }
    sh[0][threadIdx.x] = sd; sh[1][threadIdx.x] = sb; sh[2][threadIdx.x] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + w];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + w];
            sh[2][threadIdx.x] = fmax(sh[2][threadIdx.x], sh[2][threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out[0] = sh[0][0]; out[1] = sh[1][0]; out[2] = sh[2][0]; }
}
// The tool's own arithmetic: the squares (formed in double) added one after the other into fp32 sums -- a serial recurrence, so ONE lane walks
// the arrays (an offline tool: ~10 ns per element).  out[3] = sum (a-b)^2, out[4] = sum b^2 as the tool holds them.
__global__ void fdw_image_compare_serial_kernel(const float* a, const float* b, size_t n, double* out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float sd = 0.0f, sb = 0.0f;
    for (size_t i = 0; i < n; i++) {
        const float y = b[i];
        const float d = a[i] - y;
        sd = (float)((double)sd + (double)d * (double)d);
        sb = (float)((double)sb + (double)y * (double)y);
    }
    out[3] = (double)sd;
    out[4] = (double)sb;
}
hipError_t launch_image_compare(const float* a, const float* b, size_t n, float* diff, double* d_part, int nblocks, double* d_out, int serial, hipStream_t s)
{
    hipLaunchKernelGGL(fdw_image_compare_kernel, dim3(nblocks), dim3(256), 0, s, a, b, n, diff, d_part);
    hipLaunchKernelGGL(fdw_image_compare_final_kernel, dim3(1), dim3(256), 0, s, d_part, nblocks, d_out);
    if (serial) hipLaunchKernelGGL(fdw_image_compare_serial_kernel, dim3(1), dim3(64), 0, s, a, b, n, d_out);
    return hipGetLastError();
}

hipError_t launch_image_laplacian(const float* d_img, float* d_out, int nx, int nz, float dx, float dz, hipStream_t s)
{
    hipLaunchKernelGGL(fdw_image_lap_kernel, dim3((nz + 255) / 256, nx), dim3(256), 0, s, d_img, d_out, nx, nz, dx, dz);
    return hipGetLastError();
}

hipError_t launch_static_rows(float* pp, const float* psrc, float* img, const float* samples, int pitch, int row0, int nrows, int gz,
                              int img_z0, int img_z1, hipStream_t s)
{
    if (nrows <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_static_rows_kernel, dim3((pitch + 255) / 256, nrows), dim3(256), 0, s, pp, psrc, img, samples, pitch, row0, gz, img_z0, img_z1);
    return hipGetLastError();
}

hipError_t launch_record_static(const float* p0, const float* pp0, float* rec, int pitch, int row0, int nrows, int gz, int rec_x0, int rec_n, int nsteps,
                               int nbatch, long long bstride, long long rec_bstride, hipStream_t s)
{
    if (nrows <= 0 || nsteps <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_record_static_kernel, dim3((nrows * nsteps + 255) / 256, nbatch > 1 ? nbatch : 1), dim3(256), 0, s, p0, pp0, rec, pitch, row0, nrows,
                       gz, rec_x0, rec_n, nsteps, bstride, rec_bstride);
    return hipGetLastError();
}

hipError_t launch_snapshot(const float* f, float* frame, int pitch, int x0, int z0, int dec, int nxs, int nzs, hipStream_t s)
{
    if (nxs <= 0 || nzs <= 0) return hipSuccess;
    hipLaunchKernelGGL(fdw_snapshot_kernel, dim3((nzs + 255) / 256, nxs < 65535 ? nxs : 65535), dim3(256), 0, s, f, frame, pitch, x0, z0, dec, nxs, nzs);
    return hipGetLastError();
}

hipError_t launch_selftest(const float* src, float* out, hipStream_t s)
{
    hipLaunchKernelGGL(fdw_selftest_kernel, dim3(1), dim3(64), 0, s, src, out);
    return hipGetLastError();
}
#endif   // FDW_TU == 0

}  // namespace fdw

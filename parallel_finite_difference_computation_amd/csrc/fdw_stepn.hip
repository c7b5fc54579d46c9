// fdw_stepn.hip -- four time steps per pass: a pipeline of waves through LDS.  Shared helpers and design notes: fdw_device.h.
#include "fdw_device.h"

#pragma clang fp contract(off)

namespace fdw {

// ------------------------------------------------------------------------------------------------
// NS time steps per pass: a pipeline of NS waves per workgroup, one wave per time level, rows handed from
// wave to wave through LDS.  Wave k (k = 0..NS-1) computes u^{n+k+1}; only wave 0 reads global memory
// (u^n, u^{n-1}, v2) and only the last two waves write it (u^{n+NS-1} -> out1, u^{n+NS} -> out2), so a
// pass moves 12 B in + 8 B out per point for NS steps instead of per step.
//
// Every wave is the one-step march on a register ring of 2H+1 rows of "its" p field.  At march step m wave k
// works on row r_k(m) = xa - (NS-1)H - k(H+1) + m: a skew of H+1 rows per stage, so that what wave k-1
// produced during step m-1 (its result row r_{k-1}(m-1) = r_k(m)+H, which enters wave k's window, and the
// row its own window dropped, r_{k-1}(m-1)-H = r_k(m), which is wave k's "pp") is consumed during step m;
// one workgroup barrier per march step separates producer and consumer, link buffers alternate by the parity
// of m.  v2 dt2 rows (formed once, by wave 0) ride a 16-row LDS FIFO.  Where all waves run ONE body (WK 0: the modelling dialect, the receiver
// field, the recording and illumination full bodies) the global loads of waves k > 0 are sent out of range through the buffer descriptor
// (no memory request, zeros returned) and the stores of waves < NS-2 likewise, so the s_waitcnt counting stays exact and nothing diverges.
// Workgroups away from the frame of the grid, the damped strip and the sources -- nine in ten on a large grid -- run the LEAN body instead
// (pipe_lean: no masks, clamps, damping or injection code).  The lean body and the forward kernel's full body are compiled once for wave 0
// and once for the other waves (WK 1 / 2: no selects between "from memory" and "from LDS", no switched-off loads); there the forward kernels
// issue no switched-off store either: wave 0's body holds none, and in the other waves' body, which issues no global loads whose count a
// branch could split, the store sits behind a scalar branch on k that wave 1 skips.
// Validity: wave k's rows are good from march step k(2H+1) on (its window then holds only good rows of wave
// k-1); in z every step costs H = one lane per side, so NS lanes per side of a wave are halo and 64-2NS owned.
// Per point and step the arithmetic is the one-step kernel's (packed pairs as in the two-step kernel).
// ------------------------------------------------------------------------------------------------
// v2 FIFO depth: the last wave reads row m - (NS-1)(H+1) while wave 0 writes row m, so (NS-1)(H+1)+1 rows, rounded up to 8 or 16
constexpr int kFusedFifoRows = 20;      // fused backward kernel: a v2 row is 1 + 3 (H + 1) = 16 march steps under way from the first wave to the last
constexpr int pipe_fifo_rows(int ns, int h) { return (ns - 1) * (h + 1) + 1 <= 8 ? 8 : 16; }
template <int FD>
__device__ __forceinline__ int pipe_fifo_slot(int m)
{
    if constexpr ((FD & (FD - 1)) == 0) return m & (FD - 1);
    else return ((m % FD) + FD) % FD;
}

// BK: 0 forward / modelling loops; 1 source field of the backward loop (every wave stores its level); 2 receiver field of the backward
// loop (INJ = 2: trace samples per level, imaging against plev[k], image rows chained through imf);
// 3 / 4: the two roles of the FUSED backward kernel (fdw_back4_kernel: eight waves, four per field): 3 = source field (PLAIN arithmetic,
// wave 0 fills the shared v2 FIFO, every wave's new row also serves the receiver wave of its level), 4 = receiver field (one march step
// behind: its rows, windows and FIFO slots are those of role 3 shifted by D = 1, so that the source-field row it images against was
// written to the link buffers during the step before; v2 for all four waves from the FIFO; image as in BK 2)
// LEAN: the body for workgroups that touch neither the frame of the grid (no Laplacian / update masks, no row clamps), nor the damped strip,
// nor the source (instantiate with TAPER = false, INJ = 0): the kernel picks it per workgroup (pipe_lean)
// WK: 0 = the wave finds out at run time whether it is wave 0; 1 / 2 = compiled for wave 0 / for the other waves (both bodies of the forward kernel)
// NUM: 0 = the reference's exact arithmetic, 1 = FAST numerics (symmetric sums + fused multiply-adds, fdw_device.h)
// REC: forward loop with trace recording (FDW_MODE_FWD_REC): wave k records its new row u^{n+k+1} at column rec_z into rec + k rec_n, from owned
// lanes and the tile's own rows [xa, xe) only (the conditions of the field stores), so every sample is written once
// ILL: forward loop with source illumination (FDW_MODE_FWD_ILLUM): a.img += u^{n+k+1} (*) u^{n+k+1} for k = 0 .. NS-1 in that order on the updated
// cells.  The accumulator row travels like the image row of BK 2: in at wave 0 from memory, through the imf FIFO from wave to wave, each wave
// adding the square of the row it has just formed (raw, source sample included), out from the last wave -- owned lanes, the tile's own rows
// EXC: excitation-amplitude imaging (fdwave.h), the RTM dialect's forward passes.  Two arrays per epilogue, ONE f4 row in the imf FIFO: beside it
// travels a dword per lane and row (tgf, 4 KiB) with a 4-bit tag per cell.
//   1  the maps (FDW_MODE_FWD_EXC): the amp row (a.img) goes in at wave 0, wave k keeps u^{n+k+1} where it beats the row strictly in magnitude and
//      tags the cell k + 1, the last wave stores amp and turns the tags into a.exc_key + tag - 1 (= it + 1 of the winning level) over the texc row,
//      which it alone loads (its own rows, owned lanes, PF steps ahead); untagged cells keep their word
//   2  the pick (FDW_MODE_FWD_LINE_PICK): wave 0 loads the texc row and forms the tags once, tag d + 1 where texc == a.exc_key - d (= top - it
//      of level d) for d < NS; the exc row (a.img) goes in at wave 0, wave k puts u^{n+k+1} (sample included) into the cells tagged k + 1, the last
//      wave stores it; no other wave loads anything
// Compares, selects and integer adds only: texc meets no float arithmetic.  Masks as ILL: none in the lean body, the update masks in the full one.
template <int H, int NS, bool TAPER, int INJ, int PF, bool DD = false, int BK = 0, bool LEAN = false, int WK = 0, int NUM = 0, bool REC = false, bool ILL = false,
          int EXC = 0>
__device__ __forceinline__ void marchn(const Step2Args& a, const int lane, const int k, const int cs, const int xa, const int xe,
                                       f4 (*link)[2][2][64], f4 (*fifo)[64], f4 (*imf)[64] = nullptr, f4 (*linkx)[2][2][64] = nullptr,
                                       unsigned (*tgf)[64] = nullptr)
{
    static_assert(!LEAN || (!TAPER && INJ == 0), "the lean body has no damping, no injection (and records no trace)");
    constexpr bool IMG = (BK == 2 || BK == 4);
    constexpr bool ACC = IMG || ILL || (EXC != 0);            // a row of an accumulator (image, illumination, amp, exc) rides along
    static_assert(EXC == 0 || (BK == 0 && !DD && !ILL && !REC), "the excitation epilogues belong to the RTM dialect's plain forward passes");
    static_assert(!ILL || (BK == 0 && !DD), "illumination belongs to the RTM dialect's forward pass");
    constexpr int D = (BK == 4) ? 1 : 0;                      // this role runs D march steps behind
    constexpr int DL = (BK >= 3) ? 1 : 0;                     // ... so both roles of the fused kernel loop one step longer
    // one march step per workgroup barrier (two measured slower: DESIGN.md section 3c): a wave consumes what its predecessor produced
    // during the previous step, so consecutive waves work H + 1 rows apart
    constexpr int R = ((2 * H + PF + PF - 1) / PF) * PF;
    constexpr int LOOK = R - 2 * H;
    constexpr int SK = H + 1;
    constexpr int FD = BK >= 3 ? kFusedFifoRows : pipe_fifo_rows(NS, H);
    static_assert((NS - 1) * SK + 1 <= FD, "the v2 FIFO holds every row from wave 0's to the last wave's");
    const bool first = WK == 1 ? true : (WK == 2 ? false : (k == 0));      // WK 1 / 2: the body compiled for wave 0 / for the other waves
    const int cell = cs + lane;
    const int z0 = cell * 4;
    const unsigned voff = (unsigned)min(max(z0, 0), a.pitch - 4) * 4u;
    const bool own = (lane >= NS) && (lane <= 63 - NS) && (z0 >= 0) && (z0 < a.pitch);
    const unsigned soff = (own && (BK == 1 || k >= NS - 2)) ? voff : kLaneOff;      // only the last two waves store (BK 1: all four levels are kept)
    const unsigned loff = first ? voff : kLaneOff;                        // only wave 0 loads
    const unsigned row_bytes = (unsigned)a.pitch * 4u;
    const int rowmax = a.nxl - 1;
    const unsigned arr_bytes = (unsigned)a.nxl * row_bytes;               // < 2 GiB (checked by the host)
    const float *gp = BK == 4 ? a.rp : a.p, *gpp = BK == 4 ? a.rpp : a.pp;      // the fused kernel's receiver role has its own pair of fields
    float *go1 = BK == 4 ? a.rout1 : a.out1, *go2 = BK == 4 ? a.rout2 : a.out2;
    const __amdgpu_buffer_rsrc_t rs_p = array_rsrc(gp, arr_bytes), rs_pp = array_rsrc(gpp, arr_bytes), rs_v2 = array_rsrc(a.v2, arr_bytes);
    const __amdgpu_buffer_rsrc_t rs_out = array_rsrc((k == NS - 1) ? go2 : ((BK == 1 && k < NS - 2) ? (k == 0 ? a.lvl0 : a.lvl1) : go1), arr_bytes);
    // BK 2: this wave's source-field level and, for wave 0 / the last wave, the image
    const __amdgpu_buffer_rsrc_t rs_lev = array_rsrc(BK == 2 ? a.plev[k] : gp, arr_bytes), rs_img = array_rsrc(ACC ? a.img : go1, arr_bytes);
    const unsigned ioff = (ACC && own) ? voff : kLaneOff;                 // imaging: owned lanes only

    const bool wave_tap = TAPER && (cs * 4 < a.ztap);
    const bool xtap = wave_tap && ((xa - NS * H < a.xt_lo) || (xe + NS * H > a.xt_hi));
    const CoefPairs<H> cpk = (DD && NUM == 0) ? coef_pairs<H>(a.cz, a.cz) : coef_pairs<H>(a.cx, a.cz);      // DD, exact: the unscaled weights (the spacings enter per term)
    const v2f ddinv = v2f{a.dz2inv, a.dx2inv};
    const v2f c0p = v2f{a.c0, a.c0};                                      // FAST numerics: weight of the centre point
    const int blob = (INJ == 3) ? 3 : 0;                                  // INJ 3: 7x7 Gaussian source of the CPU-serial sibling (ptsrc.c:49-55)
    const bool inj_here = (INJ == 2) ? ((a.inj_z >= cs * 4) && (a.inj_z < cs * 4 + 256) && (a.inj_x < xe + NS * H) && (a.inj_x + a.inj_n > xa - NS * H))
                                     : ((INJ != 0) && (a.inj_z + blob >= cs * 4) && (a.inj_z - blob < cs * 4 + 256) && (a.inj_x + blob >= xa - NS * H) && (a.inj_x - blob < xe + NS * H));
    const float injv = (INJ != 2 && inj_here) ? sload(a.inj, k) : 0.0f;    // source sample of this wave's time step (R:119-122)
    const float* injk = a.inj + (INJ == 2 ? k * a.inj_stride : 0);        // INJ 2: the trace samples of iteration it + k (R:124-131)
    const bool rec_here = DD && !LEAN && (a.rec != nullptr) && (a.rec_z >= cs * 4) && (a.rec_z < cs * 4 + 256);
    static_assert(!REC || (!LEAN && !DD && BK == 0), "trace recording belongs to the full body of the RTM dialect's forward pass");
    const bool rec_lane = REC && own && (cell == (a.rec_z >> 2));

    bool mlap[4], mupd[4], znc[4], ihit[4];
    float tzc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int z = z0 + e;
        mlap[e] = (z >= a.lap_z0) && (z < a.lap_z1);
        mupd[e] = (z >= 0) && (z < a.upd_z1);
        ihit[e] = (z == a.inj_z);
        znc[e] = (z >= 0) && (z < a.ztap);
        tzc[e] = 1.0f;
    }
    if (wave_tap) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (znc[e]) tzc[e] = a.taperz[z0 + e];
    }
    auto taper_row = [&](f4& v, int row) {
        if (!xtap) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v.v[e] = v.v[e] * tzc[e];
        } else {
            const int rc = min(max(row, 0), a.nxl - 1);
            const float txr = sload(a.txfac, rc);
            const bool rowtz = row < a.tz_x1;
#pragma unroll
            for (int e = 0; e < 4; ++e) v.v[e] = taper1(v.v[e], tzc[e], znc[e], rowtz, txr);
        }
    };
    auto rowoff = [&](int row) -> unsigned { return LEAN ? (unsigned)row * row_bytes : (unsigned)min(max(row, 0), rowmax) * row_bytes; };
    // cache policy (fdw_device.h): p rows are re-read by the neighbouring chunk, the pointwise streams are read once
    auto load_p = [&](int row) -> f4 { return f4_load_arr(rs_p, loff, rowoff(row), false); };
    auto load_pw = [&](__amdgpu_buffer_rsrc_t rs, int row) -> f4 { return f4_load_arr(rs, loff, rowoff(row), true); };

    // rows: wave 0's centre row at march step m is s0 + m (what the global loads follow); this wave's is rk + m
    const int s0 = xa - (NS - 1) * H - D, b0 = s0 - H;
    const int rk = s0 - k * SK;
    const int M = (xe - xa) + (NS - 1) * (2 * H + 1) + DL;
    const int kp = max(k - 1, 0);
    f4 ring[R];
    f4 qpp[PF], qv2[PF];
    f4 qlv[BK == 2 ? PF : 1], qim[ACC ? PF : 1];                        // BK 2: this wave's source-field rows; BK 2, 4: (wave 0) the image rows, PF steps ahead
    const unsigned imoff = (ACC && first) ? ioff : kLaneOff;              // only wave 0 reads the image
    bool zim[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) zim[e] = (z0 + e >= 0) && (z0 + e < a.img_z1);
    // EXC: the time map.  1: read and written by the last wave; 2: read by wave 0
    const __amdgpu_buffer_rsrc_t rs_tx = array_rsrc(EXC != 0 ? reinterpret_cast<const float*>(a.texc) : gp, arr_bytes);
    const unsigned txoff = EXC == 1 ? ((own && k == NS - 1) ? voff : kLaneOff) : imoff;
    f4 qtx[EXC != 0 ? PF : 1];
    constexpr int NV = LOOK > PF ? LOOK : PF;
    static_for<2 * H>([&](auto K) {
        constexpr int kk = decltype(K)::value;
        ring[kk] = load_p(b0 + kk);
        __builtin_amdgcn_sched_barrier(0);
    });
    static_for<NV>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value - NV;
        if constexpr (j >= -LOOK) ring[j + 2 * H + LOOK] = load_p(b0 + j + 2 * H + LOOK);
        if constexpr (j >= -PF) {
            constexpr int mm = j + PF;
            qpp[mm] = load_pw(rs_pp, s0 + mm);
            if constexpr (BK != 4) qv2[mm] = load_pw(rs_v2, s0 + mm);
            if constexpr (BK == 2) qlv[mm] = f4_load_arr(rs_lev, ioff, rowoff(rk + mm), true);
            if constexpr (IMG) qim[mm] = f4_load_arr(rs_img, imoff, rowoff(rk + mm), true);
            if constexpr (ILL && WK != 2) qim[mm] = f4_load_arr(rs_img, imoff, rowoff(rk + mm), true);
            if constexpr (EXC != 0 && WK != 2) qim[mm] = f4_load_arr(rs_img, imoff, rowoff(rk + mm), true);
            if constexpr ((EXC == 1 && WK != 1) || (EXC == 2 && WK != 2)) qtx[mm] = f4_load_arr(rs_tx, txoff, rowoff(rk + mm), true);
        }
        __builtin_amdgcn_sched_barrier(0);
    });
    if (wave_tap) {
        static_for<2 * H>([&](auto K) {
            constexpr int kk = decltype(K)::value;
            taper_row(ring[kk], b0 + kk);
        });
    }

    // A wave has nothing useful to compute before its window holds good rows of its predecessor (march steps < k (2H + 1); during the
    // last 2H of them it only collects the rows entering its window) nor after the last row a later level needs from it: outside
    // [m_lo, m_hi) it keeps the barriers and its memory instructions, which are predicated off through the buffer descriptor so that
    // the s_waitcnt counting stays exact.  That frees a fifth of the issue slots of a 43-row chunk (7 % at 173 rows) for the other
    // workgroups of the CU.  The modelling dialect (DD) runs every step: skipping measured 5 % slower there, its scalar Laplacian
    // leaves no slack.
    const int m_lo = k * (2 * H + 1) + D, m_hi = (xe - xa) + 2 * (NS - 1) * H + k + D;

    auto row_step = [&](const int mb, auto UU) {
        constexpr int U = decltype(UU)::value;
        constexpr int Q = U % PF;
        constexpr int E = (U + 2 * H) % R;                      // slot of the row entering the window this step
        const int m = mb + U;
        const int r = rk + m;
        const int par = m & 1;                                   // link buffers alternate per march step
        const bool act = DD || ((m >= m_lo) && (m < m_hi));
        const bool fill = DD || ((m >= m_lo - 2 * H) && (m < m_hi));                   // collecting the rows that enter the window
        // ---- what the previous wave handed over during march step m-1: the row entering this wave's window ----
        if (fill) {
            if (!first) ring[E] = link[kp][par ^ 1][0][lane];
            if (wave_tap) taper_row(ring[E], r + H);            // damped once as "p" of this step
        }
        f4 u;
        float im0, im1, im2, im3;                               // the image row (BK 2, 4), as scalars: defined on every path without an instruction
        if constexpr (ACC) asm volatile("" : "=v"(im0), "=v"(im1), "=v"(im2), "=v"(im3));
        unsigned tgv;                                           // EXC: the row's tags
        if constexpr (EXC != 0) asm volatile("" : "=v"(tgv));
        if (act) {
        // pp and v2 of this row live in the look-ahead queue's registers: wave 0 finds them there (loaded PF steps ago), the other waves
        // read theirs from LDS into the same registers (their own look-ahead loads are switched off and return nothing they need)
        f4 &ppt = qpp[Q], &v2t = qv2[Q];                        // v2t: v2 dt2 once past the block below
        if (first) {
            if constexpr (BK == 4) {
                v2t = fifo[pipe_fifo_slot<FD>(m - D)][lane];     // the source-field role's wave 0 parked it one step ago
            } else {
                // v2 dt2 (R:89's first product) is formed once, here, and travels through the FIFO in place of v2
                const v2f w01 = v2f{qv2[Q].v[0], qv2[Q].v[1]} * a.dt2, w23 = v2f{qv2[Q].v[2], qv2[Q].v[3]} * a.dt2;
                qv2[Q].v[0] = w01.x; qv2[Q].v[1] = w01.y; qv2[Q].v[2] = w23.x; qv2[Q].v[3] = w23.y;
                fifo[pipe_fifo_slot<FD>(m)][lane] = qv2[Q];
            }
        } else {
            ppt = link[kp][par ^ 1][1][lane];
            v2t = fifo[pipe_fifo_slot<FD>(m - D - k * SK)][lane];
        }
        if (wave_tap) {
            taper_row(ppt, r);                                  // "pp": from memory once (+ once owed), from LDS once more
            if (first && a.pp_twice) taper_row(ppt, r);
        }
        const f4 c1 = ring[(U + H) % R];
        const bool rowok = LEAN || ((r >= a.lap_x0) && (r < a.lap_x1));
        const bool rowupd = LEAN || ((r >= 0) && (r < a.upd_x1));
        if constexpr (DD) {
            // this wave's p field is P of iteration it0 + k: its trace sample (mod_main.cpp:155-157); owned lanes and rows only
            if (rec_here && own && r >= xa && r < xe && r >= a.rec_x0 && r < a.rec_x0 + a.rec_n) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (z0 + e == a.rec_z) a.rec[k * a.rec_n + (r - a.rec_x0)] = c1.v[e] * tzc[e];      // after this step's taper_apply, as the one-step kernel
            }
        }
        auto row = [&](auto IO) -> const f4& { return ring[(U + decltype(IO)::value) % R]; };
        v2f lapq[2];
        // DD exact: the sibling's single-accumulator Laplacian, two cells per instruction; DD FAST: the weights carry their spacing
        if constexpr (DD && NUM == 0) laplacian_dd_quad<H>(lane_window(c1), row, cpk, ddinv, lapq[0], lapq[1]);
        else lap_quad<NUM, H>(c1, row, cpk, c0p, lapq[0], lapq[1]);
        // (the masks behind a per-workgroup branch, taken only where a tile touches the frame, measured 1.5 % slower: DESIGN.md section 3c)
        static_for<2>([&](auto PP) {
            constexpr int P = decltype(PP)::value;
            v2f lap2 = lapq[P];
            if constexpr (!LEAN) lap2 = v2f{(rowok && mlap[2 * P]) ? lap2.x : 0.0f, (rowok && mlap[2 * P + 1]) ? lap2.y : 0.0f};
            const v2f prod2 = f4_pair(v2t, P) * lap2;          // v2t holds v2 dt2 (see above)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = 2 * P + q;
                const float upd = leapfrog_prod(c1.v[e], ppt.v[e], q ? prod2.y : prod2.x);
                u.v[e] = (LEAN || (rowupd && mupd[e])) ? upd : ppt.v[e];
            }
        });
        if constexpr (INJ == 1) {
            if (inj_here && r == a.inj_x) {
#pragma unroll
                for (int e = 0; e < 4; ++e) u.v[e] = ihit[e] ? u.v[e] + injv : u.v[e];
            }
        }
        if constexpr (INJ == 2) {
            if (inj_here && r >= a.inj_x && r < a.inj_x + a.inj_n) {      // kernel_sism: one add per receiver row (R:124-131)
                const float v = sload(injk, r - a.inj_x);
#pragma unroll
                for (int e = 0; e < 4; ++e) u.v[e] = ihit[e] ? u.v[e] + v : u.v[e];
            }
        }
        if constexpr (IMG) {
            // kernel_img (R:133-144) for iteration it + k: img += F_{it+k} * (the receiver field just formed).  The image row enters at wave 0
            // from memory, collects the four products in iteration order on its way through the LDS FIFO and leaves from the last wave.
            f4 im;
            if (first) im = qim[Q];
            else im = imf[r & 15][lane];
            if (r >= xa && r < xe) {
                f4 lv;
                if constexpr (BK == 4) lv = linkx[k][par ^ 1][0][lane];      // F_{it+k}(r): the source-field wave of this level formed it one step ago
                else lv = qlv[Q];
#pragma unroll
                for (int e = 0; e < 4; ++e) im.v[e] = zim[e] ? im.v[e] + lv.v[e] * u.v[e] : im.v[e];
            }
            if (k < NS - 1) imf[r & 15][lane] = im;
            im0 = im.v[0]; im1 = im.v[1]; im2 = im.v[2]; im3 = im.v[3];
        }
        if constexpr (ILL) {
            // the square of the row as it is stored and handed on (the window rows are damped copies); product and sum rounded separately
            f4 il;
            if (first) il = qim[Q];
            else il = imf[r & 15][lane];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sq = u.v[e] * u.v[e];
                il.v[e] = (LEAN || (rowupd && mupd[e])) ? il.v[e] + sq : il.v[e];
            }
            if (k < NS - 1) imf[r & 15][lane] = il;
            im0 = il.v[0]; im1 = il.v[1]; im2 = il.v[2]; im3 = il.v[3];
        }
        if constexpr (EXC == 1) {
            // the row compared and kept is the one stored and handed on (raw, source sample included); a NaN on either side compares false
            f4 am;
            unsigned tg;
            if (first) { am = qim[Q]; tg = 0u; }
            else { am = imf[r & 15][lane]; tg = tgf[r & 15][lane]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool win = (__builtin_fabsf(u.v[e]) > __builtin_fabsf(am.v[e])) && (LEAN || (rowupd && mupd[e]));
                am.v[e] = win ? u.v[e] : am.v[e];
                tg = win ? ((tg & ~(15u << (4 * e))) | ((unsigned)(k + 1) << (4 * e))) : tg;
            }
            if (k < NS - 1) { imf[r & 15][lane] = am; tgf[r & 15][lane] = tg; }
            im0 = am.v[0]; im1 = am.v[1]; im2 = am.v[2]; im3 = am.v[3];
            tgv = tg;
        }
        if constexpr (EXC == 2) {
            f4 ex;
            unsigned tg;
            if (first) {
                ex = qim[Q];
                tg = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned d = (unsigned)a.exc_key - (unsigned)__float_as_int(qtx[Q].v[e]);      // level d of the pass picks this cell
                    tg |= (d < (unsigned)NS ? d + 1u : 0u) << (4 * e);
                }
            } else { ex = imf[r & 15][lane]; tg = tgf[r & 15][lane]; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool pick = (((tg >> (4 * e)) & 15u) == (unsigned)(k + 1)) && (LEAN || (rowupd && mupd[e]));
                ex.v[e] = pick ? u.v[e] : ex.v[e];
            }
            if (k < NS - 1) { imf[r & 15][lane] = ex; tgf[r & 15][lane] = tg; }
            im0 = ex.v[0]; im1 = ex.v[1]; im2 = ex.v[2]; im3 = ex.v[3];
        }
        if constexpr (INJ == 3) {
            if (inj_here && r >= a.inj_x - 3 && r <= a.inj_x + 3) {
                const int dxa = r > a.inj_x ? r - a.inj_x : a.inj_x - r;
                const float g0 = a.gw[dxa][0], g1 = a.gw[dxa][1], g2 = a.gw[dxa][2], g3 = a.gw[dxa][3];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int dz = z0 + e - a.inj_z, dza = dz < 0 ? -dz : dz;
                    const float g = dza == 0 ? g0 : (dza == 1 ? g1 : (dza == 2 ? g2 : g3));
                    if (dza <= 3 && mupd[e]) u.v[e] = u.v[e] + injv * g;      // ptsrc.c leaves out the cells beyond the grid edge: none lands in a padding column
                }
            }
        }
        // ---- hand over to the next wave: the new row (raw) and the row leaving this window (damped once) ----
        link[k][par][0][lane] = u;
        link[k][par][1][lane] = ring[U];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) asm volatile("" : "=v"(u.v[e]));      // defined (no instruction) on the path that skips the row
        }
        // The field store.  Forward kernels (BK 0) keep the last two levels only: the body compiled for wave 0 holds no store at all, the
        // body of the other waves holds it behind a scalar branch that wave 1 skips (k is wave-uniform; this body issues no global loads,
        // so no load count crosses the branch).  Everywhere else every wave issues it and switches its lanes off through the offset.
        if constexpr (!(BK == 0 && WK == 1 && NS > 2)) {
            if (!(BK == 0 && WK == 2) || k >= NS - 2) {
                const unsigned so = (act && (r >= xa) && (r < xe) && (m < M)) ? soff : kLaneOff;
                f4_store_arr(rs_out, so, rowoff(r), u);
            }
        }
        if constexpr (REC)
            f1_store_arr(array_rsrc(a.rec + (size_t)k * a.rec_n, (unsigned)a.rec_n * 4u),
                         rec_offset(rec_lane && act && (r >= xa) && (r < xe) && (m < M), r, a.rec_x0, a.rec_n), f4_pick(u, a.rec_z & 3));
        if constexpr (ACC) {
            const unsigned sim = (k == NS - 1 && act && (r >= xa) && (r < xe)) ? ioff : kLaneOff;
            f4 im;
            im.v[0] = im0; im.v[1] = im1; im.v[2] = im2; im.v[3] = im3;
            f4_store_arr(rs_img, sim, rowoff(r), im);
            if constexpr (EXC == 1 && WK != 1) {      // the time map of the last wave's row: the winning level's it + 1 where a level of this pass won
                f4 tx;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned w = (tgv >> (4 * e)) & 15u;
                    tx.v[e] = w ? __int_as_float(a.exc_key + (int)w - 1) : qtx[Q].v[e];
                }
                f4_store_arr(rs_tx, sim, rowoff(r), tx);
            }
        }
        // ---- look-ahead loads of wave 0 into the slots this step freed ----
        if constexpr (WK != 2) ring[U] = load_p(b0 + m + R);
        qpp[Q] = load_pw(rs_pp, s0 + m + PF);
        if constexpr (BK != 4) qv2[Q] = load_pw(rs_v2, s0 + m + PF);
        if constexpr (BK == 2) qlv[Q] = f4_load_arr(rs_lev, ioff, rowoff(r + PF), true);
        if constexpr (IMG) qim[Q] = f4_load_arr(rs_img, imoff, rowoff(r + PF), true);
        if constexpr (ILL && WK != 2) qim[Q] = f4_load_arr(rs_img, imoff, rowoff(r + PF), true);
        if constexpr (EXC != 0 && WK != 2) qim[Q] = f4_load_arr(rs_img, imoff, rowoff(r + PF), true);
        if constexpr ((EXC == 1 && WK != 1) || (EXC == 2 && WK != 2)) qtx[Q] = f4_load_arr(rs_tx, txoff, rowoff(r + PF), true);
        __syncthreads();
    };

    for (int mb = 0; mb < M; mb += R)
        static_for<R>([&](auto UU) { row_step(mb, UU); });
}

// Workgroup-uniform: may this tile run the lean body?  (pipe_tile_lean, fdw_kernels.h: the host counts the tiles by the same predicate)
template <int H, int NS, bool TAPER, int INJ, bool DD = false, bool REC = false>
__device__ __forceinline__ bool pipe_lean(const Step2Args& a, int cs, int xa, int xe)
{
    return pipe_tile_lean<H, NS, TAPER, INJ, DD, REC>(a, cs, xa, xe);
}

// workgroups per CU the launch bounds hold the kernels to: 5 x 4 waves = 96 VGPRs (forward, source field); 4 for the modelling dialect;
// 3 for the receiver field (BK 2)
constexpr int kPipeWG = 5;
constexpr int kDDWG = 4;
constexpr int kPipePF = 2;      // rows of global look-ahead of wave 0

// Tile placement of the pipeline kernels: which strip and rows a workgroup works on, and which wave of it this is.  Declares `lane`, the wave
// index `k` (wave-uniform), the first cell `cs` of the strip and the rows [`xa`, `xe`) of the chunk; leaves the kernel where the workgroup
// has no tile.  Blocks b and b + 8 share an XCD (round-robin dispatch), so XCD x takes the logical blocks [x nper, (x + 1) nper): a contiguous
// band of chunks whose halo rows it re-reads from its own L2.  Whole workgroups return (L and the tile are workgroup-uniform), so every barrier
// of the march is reached by all its waves.  From L on the text is the host's too (FDW_PIPE_TILE_ROWS, fdw_kernels.h).
// A macro and not a function, on evidence: as a __forceinline__ function that returns the six values in a struct, 0 of the 30 kernels of this
// file (and 2 of 56 of the FAST one-step unit) keep their instruction text -- scalar register numbering and scheduling move; as a function that
// takes the kernel's body as a lambda, 0 of 4 sampled kernels keep it; expanded as a macro, every kernel is byte-identical to the hand-written
// copies it replaces (scripts/kernel_diff.py, profiles/r16_resource_report.txt).  The same holds for FDW_STEP_TILE and FDW_STEP2_TILE.
// For the same reason the pair `if (k == 0) marchn<..., WK 1, ...>(...); else marchn<..., WK 2, ...>(...);` stays written out at its 15 sites:
// behind one __forceinline__ function template over the remaining arguments, 24 of the 30 kernels change their text (2 their SGPR spills).
#define FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)                                   \
    const int lane = threadIdx.x & 63;                                              \
    const int k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                 \
    const int bid = blockIdx.x;                                                     \
    const int L = (bid & 7) * a.nper + (bid >> 3);                                  \
    if (L >= a.nblk) return;                                                        \
    FDW_PIPE_TILE_ROWS(a, L, zb, xa, xe)                                            \
    if (xa >= xe) return;                                                           \
    const int cs = FDW_PIPE_TILE_CELL(zb, NS);

template <int H, int NS, bool TAPER, int INJ, int PF, bool DD = false, int BK = 0, int NUM = 0>
__global__ __launch_bounds__(64 * NS, BK == 2 ? 3 : (DD ? kDDWG : kPipeWG)) void fdw_stepn_kernel(const Step2Args a)
{
    FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)
    __shared__ f4 link[NS][2][2][64];                      // [producer wave][parity][0 new row | 1 row leaving the window][lane]
    __shared__ f4 fifo[pipe_fifo_rows(NS, H)][64];
    if constexpr (BK == 2) {
        __shared__ f4 imf[16][64];                         // image rows on their way from wave to wave (a row is 3 (H + 1) = 15 steps under way)
        marchn<H, NS, TAPER, INJ, PF, DD, BK, false, 0, NUM>(a, lane, k, cs, xa, xe, link, fifo, imf);
    } else if constexpr (BK == 0) {
        // nine workgroups in ten of a large grid touch neither the frame, nor the damped strip, nor the source: they take the lean body,
        // compiled once for wave 0 and once for the other waves (the modelling dialect: one body for all four)
        if (pipe_lean<H, NS, TAPER, INJ, DD>(a, cs, xa, xe)) {
            if constexpr (!DD) {
                if (k == 0) marchn<H, NS, false, 0, PF, DD, 0, true, 1, NUM>(a, lane, k, cs, xa, xe, link, fifo);
                else marchn<H, NS, false, 0, PF, DD, 0, true, 2, NUM>(a, lane, k, cs, xa, xe, link, fifo);
            } else {
                marchn<H, NS, false, 0, PF, DD, 0, true, 0, NUM>(a, lane, k, cs, xa, xe, link, fifo);
            }
        }
        // ... and so is the full body of the others (not the modelling dialect): no selects between "from memory" and "from LDS", no switched-off
        // look-ahead loads with their waits in waves 1 .. NS-1
        else if constexpr (DD) marchn<H, NS, TAPER, INJ, PF, DD, BK, false, 0, NUM>(a, lane, k, cs, xa, xe, link, fifo);
        else {
            if (k == 0) marchn<H, NS, TAPER, INJ, PF, false, 0, false, 1, NUM>(a, lane, k, cs, xa, xe, link, fifo);
            else marchn<H, NS, TAPER, INJ, PF, false, 0, false, 2, NUM>(a, lane, k, cs, xa, xe, link, fifo);
        }
    } else {
        marchn<H, NS, TAPER, INJ, PF, DD, BK, false, 0, NUM>(a, lane, k, cs, xa, xe, link, fifo);
    }
}

// FDW_MODE_FWD_REC: the forward pass that also records the trace samples of its kPipeSteps steps.  The tiles whose owned lanes hold the
// receiver column run the full body with recording, the others fdw_stepn_kernel's lean bodies.  Four workgroups per CU, not
// kPipeWG: at 96 VGPRs the recording full body spills one VGPR to scratch (its SGPRs, at the limit of 106, spill into VGPR lanes); DESIGN.md 6f.
template <int NUM>
__global__ __launch_bounds__(64 * kPipeSteps, kDDWG) void fdw_stepn_rec_kernel(const Step2Args a)
{
    constexpr int H = 4, NS = kPipeSteps, PF = kPipePF;
    FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)
    __shared__ f4 link[NS][2][2][64];
    __shared__ f4 fifo[pipe_fifo_rows(NS, H)][64];
    if (pipe_lean<H, NS, true, 1, false, true>(a, cs, xa, xe)) {
        if (k == 0) marchn<H, NS, false, 0, PF, false, 0, true, 1, NUM>(a, lane, k, cs, xa, xe, link, fifo);
        else marchn<H, NS, false, 0, PF, false, 0, true, 2, NUM>(a, lane, k, cs, xa, xe, link, fifo);
    }
    else marchn<H, NS, true, 1, PF, false, 0, false, 0, NUM, true>(a, lane, k, cs, xa, xe, link, fifo);
}

// FDW_MODE_FWD_ILLUM: the forward pass that also accumulates the source illumination of its kPipeSteps steps (a.img).  Every tile carries the
// accumulator row: the lean tiles add the squares without masks, the tiles on the frame, the damped strip or the source with the update masks
// of the full body.  16 KiB of LDS more than fdw_stepn_kernel (48 KiB): three workgroups per CU, so up to 168 VGPRs.
template <int NUM>
__global__ __launch_bounds__(64 * kPipeSteps, 3) void fdw_stepn_illum_kernel(const Step2Args a)
{
    constexpr int H = 4, NS = kPipeSteps, PF = kPipePF;
    FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)
    __shared__ f4 link[NS][2][2][64];
    __shared__ f4 fifo[pipe_fifo_rows(NS, H)][64];
    __shared__ f4 ilf[16][64];                             // accumulator rows on their way from wave to wave (3 (H + 1) = 15 steps under way)
    if (pipe_lean<H, NS, true, 1>(a, cs, xa, xe)) {
        if (k == 0) marchn<H, NS, false, 0, PF, false, 0, true, 1, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
        else marchn<H, NS, false, 0, PF, false, 0, true, 2, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
    }
    else marchn<H, NS, true, 1, PF, false, 0, false, 0, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
}

// FDW_MODE_FWD_REC_ILLUM: the forward pass that records the trace samples of its kPipeSteps steps AND accumulates their source illumination
// (the forward loop of fdw_shot_residual with an accumulator).  Every tile carries the accumulator row through the 16-slot LDS FIFO as in
// fdw_stepn_illum_kernel (48 KiB of LDS, three workgroups per CU, the square taken before the hand-over); the tiles whose owned lanes hold the
// receiver column run the full body, in which wave k also records row k of the pass as in fdw_stepn_rec_kernel; all others run
// fdw_stepn_illum_kernel's bodies, lean where the tile allows.
template <int NUM>
__global__ __launch_bounds__(64 * kPipeSteps, 3) void fdw_stepn_rec_illum_kernel(const Step2Args a)
{
    constexpr int H = 4, NS = kPipeSteps, PF = kPipePF;
    FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)
    __shared__ f4 link[NS][2][2][64];
    __shared__ f4 fifo[pipe_fifo_rows(NS, H)][64];
    __shared__ f4 ilf[16][64];
    if (pipe_lean<H, NS, true, 1, false, true>(a, cs, xa, xe)) {
        if (k == 0) marchn<H, NS, false, 0, PF, false, 0, true, 1, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
        else marchn<H, NS, false, 0, PF, false, 0, true, 2, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
    }
    else marchn<H, NS, true, 1, PF, false, 0, false, 0, NUM, true, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
}

// FDW_MODE_FWD_LINE*: the forward pass driven by a LINE source (fdw_dev_line_steps): wave k adds the samples inj + k inj_stride on column inj_z
// of rows [inj_x, inj_x + inj_n) to its new row, as the receiver pass of the backward loop does (INJ = 2), here without imaging.  Only the
// tiles of the strip that holds the line (and those on the frame and in the damped strip) run the full body; the others keep the lean bodies
// of fdw_stepn_kernel (plain, REC) or of fdw_stepn_illum_kernel (ILL).  REC: wave k records row k of the pass after the injection, full body
// where the owned lanes hold the receiver column; ILL: the accumulator row rides the 16-slot LDS FIFO, the square taken after the injection.
// Workgroups per CU as the point-source kernels of the same variant.
template <bool REC, bool ILL, int NUM>
__global__ __launch_bounds__(64 * kPipeSteps, ILL ? 3 : (REC ? kDDWG : kPipeWG)) void fdw_stepn_line_kernel(const Step2Args a)
{
    static_assert(!(REC && ILL), "recording and illumination together are not built for the line source");
    constexpr int H = 4, NS = kPipeSteps, PF = kPipePF;
    FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)
    __shared__ f4 link[NS][2][2][64];
    __shared__ f4 fifo[pipe_fifo_rows(NS, H)][64];
    const bool lean = pipe_lean<H, NS, true, 2, false, REC>(a, cs, xa, xe);
    if constexpr (ILL) {
        __shared__ f4 ilf[16][64];
        if (lean) {
            if (k == 0) marchn<H, NS, false, 0, PF, false, 0, true, 1, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
            else marchn<H, NS, false, 0, PF, false, 0, true, 2, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
        }
        else marchn<H, NS, true, 2, PF, false, 0, false, 0, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
    } else {
        if (lean) {
            if (k == 0) marchn<H, NS, false, 0, PF, false, 0, true, 1, NUM>(a, lane, k, cs, xa, xe, link, fifo);
            else marchn<H, NS, false, 0, PF, false, 0, true, 2, NUM>(a, lane, k, cs, xa, xe, link, fifo);
        }
        else if constexpr (REC) marchn<H, NS, true, 2, PF, false, 0, false, 0, NUM, true>(a, lane, k, cs, xa, xe, link, fifo);
        else {
            if (k == 0) marchn<H, NS, true, 2, PF, false, 0, false, 1, NUM>(a, lane, k, cs, xa, xe, link, fifo);
            else marchn<H, NS, true, 2, PF, false, 0, false, 2, NUM>(a, lane, k, cs, xa, xe, link, fifo);
        }
    }
}

// FDW_MODE_FWD_LINE_REC_ILLUM: the line-source pass that records the trace samples of its kPipeSteps steps AND accumulates their illumination
// (fdw_dev_line_record_illum_steps, fdw_shot_line_residual with an accumulator): fdw_stepn_rec_illum_kernel with INJ = 2.  The tiles of the
// strip that holds the line, of the strip whose owned lanes hold the receiver column, on the frame and in the damped strip run the full body,
// in which wave k injects, records row k of the pass and squares, in that order; all others run fdw_stepn_illum_kernel's lean bodies.  48 KiB
// of LDS, three workgroups per CU.  A kernel of its own name, as the point source's combined kernel is.
template <int NUM>
__global__ __launch_bounds__(64 * kPipeSteps, 3) void fdw_stepn_line_rec_illum_kernel(const Step2Args a)
{
    constexpr int H = 4, NS = kPipeSteps, PF = kPipePF;
    FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)
    __shared__ f4 link[NS][2][2][64];
    __shared__ f4 fifo[pipe_fifo_rows(NS, H)][64];
    __shared__ f4 ilf[16][64];
    if (pipe_lean<H, NS, true, 2, false, true>(a, cs, xa, xe)) {
        if (k == 0) marchn<H, NS, false, 0, PF, false, 0, true, 1, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
        else marchn<H, NS, false, 0, PF, false, 0, true, 2, NUM, false, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
    }
    else marchn<H, NS, true, 2, PF, false, 0, false, 0, NUM, true, true>(a, lane, k, cs, xa, xe, link, fifo, ilf);
}

// FDW_MODE_FWD_EXC: the forward pass that also keeps the excitation maps of its kPipeSteps steps (a.img = amp, a.texc; marchn, EXC 1).  Every
// tile carries the amp row through the 16-slot LDS FIFO as fdw_stepn_illum_kernel carries its accumulator, and beside it a dword of tags per
// lane and row: 16 + 16 + 16 + 4 = 52 KiB of LDS, three workgroups per CU (156 of the CU's 160 KiB).  Lean tiles compare without masks, the
// tiles on the frame, the damped strip or the source with the update masks of the full body.
template <int NUM>
__global__ __launch_bounds__(64 * kPipeSteps, 3) void fdw_stepn_exc_kernel(const Step2Args a)
{
    constexpr int H = 4, NS = kPipeSteps, PF = kPipePF;
    FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)
    __shared__ f4 link[NS][2][2][64];
    __shared__ f4 fifo[pipe_fifo_rows(NS, H)][64];
    __shared__ f4 amf[16][64];                             // amp rows on their way from wave to wave (3 (H + 1) = 15 steps under way)
    __shared__ unsigned tgf[16][64];                       // ... and their tags
    if (pipe_lean<H, NS, true, 1>(a, cs, xa, xe)) {
        if (k == 0) marchn<H, NS, false, 0, PF, false, 0, true, 1, NUM, false, false, 1>(a, lane, k, cs, xa, xe, link, fifo, amf, nullptr, tgf);
        else marchn<H, NS, false, 0, PF, false, 0, true, 2, NUM, false, false, 1>(a, lane, k, cs, xa, xe, link, fifo, amf, nullptr, tgf);
    }
    // the full body too is compiled once for wave 0 and once for the other waves, as the plain forward kernel's: with one body for all four waves
    // the compiler keeps the amp look-ahead queue in scratch memory
    else if (k == 0) marchn<H, NS, true, 1, PF, false, 0, false, 1, NUM, false, false, 1>(a, lane, k, cs, xa, xe, link, fifo, amf, nullptr, tgf);
    else marchn<H, NS, true, 1, PF, false, 0, false, 2, NUM, false, false, 1>(a, lane, k, cs, xa, xe, link, fifo, amf, nullptr, tgf);
}

// FDW_MODE_FWD_LINE_PICK: the line-source pass that also takes the excitation pick of its kPipeSteps steps (a.img = exc, a.texc read only;
// marchn, EXC 2): fdw_stepn_line_kernel's tiles (full body in the strip that holds the line, on the frame and in the damped strip, lean
// elsewhere), every tile carrying the exc row and the tags wave 0 formed.  52 KiB of LDS, three workgroups per CU.
template <int NUM>
__global__ __launch_bounds__(64 * kPipeSteps, 3) void fdw_stepn_line_pick_kernel(const Step2Args a)
{
    constexpr int H = 4, NS = kPipeSteps, PF = kPipePF;
    FDW_PIPE_TILE(a, NS, lane, k, cs, xa, xe)
    __shared__ f4 link[NS][2][2][64];
    __shared__ f4 fifo[pipe_fifo_rows(NS, H)][64];
    __shared__ f4 exf[16][64];
    __shared__ unsigned tgf[16][64];
    if (pipe_lean<H, NS, true, 2>(a, cs, xa, xe)) {
        if (k == 0) marchn<H, NS, false, 0, PF, false, 0, true, 1, NUM, false, false, 2>(a, lane, k, cs, xa, xe, link, fifo, exf, nullptr, tgf);
        else marchn<H, NS, false, 0, PF, false, 0, true, 2, NUM, false, false, 2>(a, lane, k, cs, xa, xe, link, fifo, exf, nullptr, tgf);
    }
    else if (k == 0) marchn<H, NS, true, 2, PF, false, 0, false, 1, NUM, false, false, 2>(a, lane, k, cs, xa, xe, link, fifo, exf, nullptr, tgf);
    else marchn<H, NS, true, 2, PF, false, 0, false, 2, NUM, false, false, 2>(a, lane, k, cs, xa, xe, link, fifo, exf, nullptr, tgf);
}

// Four iterations of the backward loop in ONE pass: a workgroup of eight waves, waves 0-3 the pipeline of the source field (role 3), waves 4-7
// the pipeline of the receiver field one march step behind (role 4).  The source-field levels never leave the chip: the receiver wave of
// level k reads F_{it+k}(row) from the link buffer the source-field wave k wrote it to for its own successor.  6 fields in + 5 out per
// four iterations = 44 B/point (the two-pass form moves 92).  Both roles run the same number of march steps and reach one barrier per step.
template <int H, int NS, int PF, int NUM = 0>
__global__ __launch_bounds__(128 * NS, 2) void fdw_back4_kernel(const Step2Args a)
{
    FDW_PIPE_TILE(a, NS, lane, k8, cs, xa, xe)
    __shared__ f4 linkF[NS][2][2][64];
    __shared__ f4 linkR[NS][2][2][64];
    __shared__ f4 fifo[kFusedFifoRows][64];
    __shared__ f4 imf[16][64];
    // each role runs the lean body (compiled once for its wave 0 and once for its other waves) where its tile allows
    if (k8 < NS) {
        if (pipe_lean<H, NS, false, 0>(a, cs, xa, xe)) {
            if (k8 == 0) marchn<H, NS, false, 0, PF, false, 3, true, 1, NUM>(a, lane, k8, cs, xa, xe, linkF, fifo);
            else marchn<H, NS, false, 0, PF, false, 3, true, 2, NUM>(a, lane, k8, cs, xa, xe, linkF, fifo);
        } else {
            marchn<H, NS, false, 0, PF, false, 3, false, 0, NUM>(a, lane, k8, cs, xa, xe, linkF, fifo);
        }
    } else {
        // receiver role: lean where the tile holds neither the damped strip nor the receiver line
        if (pipe_lean<H, NS, true, 2>(a, cs, xa, xe)) {
            if (k8 == NS) marchn<H, NS, false, 0, PF, false, 4, true, 1, NUM>(a, lane, 0, cs, xa, xe, linkR, fifo, imf, linkF);
            else marchn<H, NS, false, 0, PF, false, 4, true, 2, NUM>(a, lane, k8 - NS, cs, xa, xe, linkR, fifo, imf, linkF);
        } else {
            marchn<H, NS, true, 2, PF, false, 4, false, 0, NUM>(a, lane, k8 - NS, cs, xa, xe, linkR, fifo, imf, linkF);
        }
    }
}

template <int NUM>
static hipError_t launch_stepn_num(const Step2Args& a, int mode, hipStream_t s)
{
    const dim3 grid(8 * a.nper), block(64 * kPipeSteps);
    switch (mode) {
    case FDW_MODE_FWD:   hipLaunchKernelGGL((fdw_stepn_kernel<4, kPipeSteps, true, 1, kPipePF, false, 0, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_REC: hipLaunchKernelGGL((fdw_stepn_rec_kernel<NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_ILLUM: hipLaunchKernelGGL((fdw_stepn_illum_kernel<NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_REC_ILLUM: hipLaunchKernelGGL((fdw_stepn_rec_illum_kernel<NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE: hipLaunchKernelGGL((fdw_stepn_line_kernel<false, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE_REC: hipLaunchKernelGGL((fdw_stepn_line_kernel<true, false, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE_ILLUM: hipLaunchKernelGGL((fdw_stepn_line_kernel<false, true, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE_REC_ILLUM: hipLaunchKernelGGL((fdw_stepn_line_rec_illum_kernel<NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_EXC: hipLaunchKernelGGL((fdw_stepn_exc_kernel<NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_FWD_LINE_PICK: hipLaunchKernelGGL((fdw_stepn_line_pick_kernel<NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_PLAIN: hipLaunchKernelGGL((fdw_stepn_kernel<4, kPipeSteps, false, 0, kPipePF, false, 0, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_MOD:   hipLaunchKernelGGL((fdw_stepn_kernel<4, kPipeSteps, true, 3, kPipePF, true, 0, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_PLAIN_ALL: hipLaunchKernelGGL((fdw_stepn_kernel<4, kPipeSteps, false, 0, kPipePF, false, 1, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_RECV:  hipLaunchKernelGGL((fdw_stepn_kernel<4, kPipeSteps, true, 2, kPipePF, false, 2, NUM>), grid, block, 0, s, a); break;
    case FDW_MODE_BACK4: hipLaunchKernelGGL((fdw_back4_kernel<4, kPipeSteps, kPipePF, NUM>), grid, dim3(128 * kPipeSteps), 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_stepn(const Step2Args& a, int h, int mode, hipStream_t s)
{
    if (a.nper <= 0) return hipSuccess;
    if (h != 4) return hipErrorInvalidValue;
    return a.numerics ? launch_stepn_num<1>(a, mode, s) : launch_stepn_num<0>(a, mode, s);      // FAST numerics (fdw_device.h): the same kernels with NUM = 1
}

}  // namespace fdw

// fdw_api.cpp -- the C ABI of libfdwave.so (include/fdwave.h) on top of the gfx950 kernels.
//
// Replaces the reference's L2 seam: fd_init / fd_init_cuda / write_buffers / fd_forward / fd_back of
// cuda_reference_RTM/src/fd-code.cu (R) and fd_init / the single launch of
// cuda_reference_stencil_computation/fd-source-code.cu (S).  There is no CPU compute path in this
// library: if HIP cannot be initialised on a gfx950 device fdw_create fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "fdw_born.h"
#include "fdw_dtt.h"
#include "fdw_extimg.h"
#include "fdw_lsm.h"
#include "fdw_excimg.h"
#include "fdw_internal.h"
#include "fdw_kernels.h"
#include "fdwave.h"

using namespace fdw;

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int fdw_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
#define fail fdw_fail

extern "C" const char* fdw_last_error(void) { return g_err; }
extern "C" int fdw_version(void) { return FDW_VERSION; }

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
// events of the launch units of unit_passes: unit i records slot i % kBandRing, and the last unit that waits for it (i + 2D - 1 in the band
// plan, i + 3 in the cut plan) is issued before unit i + kBandRing records the slot again
constexpr int kBandRing = 8;
static_assert(kBandRing >= 2 * FDW_PASS_DEPTH_MAX, "a slot must not be recorded again before its last waiter is issued");

struct fdw_ctx {
    fdw_params prm{};
    fdw_slab slab{};
    int device = 0;
    int h = 0, pitch = 0, nxl = 0;
    int nx = 0, nz = 0;            // interior size of the GLOBAL grid
    int xlim = 0, zlim = 0, ztap = 0;  // global launch extents (R:185-195)
    // local-row translations
    int lap_x0 = 0, lap_x1 = 0, lap_z0 = 0, lap_z1 = 0;     // RTM modes
    int slap_x0 = 0, slap_x1 = 0, slap_z0 = 0, slap_z1 = 0; // stencil program (full interior)
    int upd_x1 = 0, upd_z1 = 0, tz_x1 = 0, xt_lo = 0, xt_hi = 0;
    float dt2 = 0.f, dx2inv = 0.f, dz2inv = 0.f;
    float c0 = 0.f;                // FAST numerics: cz[h] + cx[h]
    float fcx[FDW_MAX_ORDER + 1]{}, fcz[FDW_MAX_ORDER + 1]{};  // FAST numerics of dialects 1, 2: the weights with their spacing folded in (fp32 products)
    float cx[FDW_MAX_ORDER + 1]{}, cz[FDW_MAX_ORDER + 1]{};    // RTM weights (C libm variant unless coef_cxx); dialect MOD: unscaled
    float* d_rec = nullptr;     // dialect MOD: trace samples [nt][nx] of one shot
    size_t rec_cap = 0;
    std::vector<float> taper_x, taper_z, txfac;
    // device tables
    float *d_taperz = nullptr, *d_txfac = nullptr, *d_gcx = nullptr, *d_gcz = nullptr;
    hipStream_t stream = nullptr;
    // lazily allocated work buffers of the host-array API
    float* fld[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // 8, 9: source-field levels of a backward pipeline pass
    float *d_v2 = nullptr, *d_img = nullptr, *d_srce = nullptr, *d_dobs = nullptr;
    float* d_illum = nullptr;   // source illumination of one shot on the extended grid (fdw_shot_illum); allocated on first use
    float* d_amp = nullptr;     // excitation maps and picked samples of one shot on the extended grid (fdw_shot_excitation); allocated on first use
    int* d_texc = nullptr;
    float* d_exc = nullptr;
    unsigned* d_peak = nullptr;   // max |amp| per shot as a word (fdw_dev_image_excitation, fdw_shot_excitation_batch); one word from creation on
    int peak_cap = 0;
    float* d_snap[3] = {nullptr, nullptr, nullptr};   // frame stores of fdw_shot_snaps (snaps, snaps_rec, snapr): [nframes][nxs][nzs] each
    size_t snap_cap[3] = {0, 0, 0};
    size_t srce_cap = 0, dobs_cap = 0;
    // tuning
    int xchunk = 0, wz = 0, use_generic = 0, prefetch = 0, force_edge = 0, xchunk2 = 0;
    int tb = 0;   // two-steps-per-pass kernel: 0 auto (large grids), 1 always, -1 never
    // random-border model generated on the device (row f4): interior model, one call's draws, jump tables, the extended model
    float *d_vp = nullptr, *d_vpe = nullptr;
    int* d_draws = nullptr;
    long long draws_cap = 0;
    unsigned* d_jump = nullptr;   // the generator's jump table (fdw_border.hip), sized for njump blocks of 64 threads
    int njump = 0;
    bool model_resident = false, v2_resident = false;
    // a batch of shots through one launch per time step (fdw_shot_batch): per-shot copies of the eight fields, v2, image, gather
    int nbatch = 1, batch_dsx = 0, batch_cap = 0, batch_nt = 0;
    bool batch_all = false;      // the batch buffers hold the RTM loop's full set (else: the modelling loop's two fields + gathers)
    float* bfld[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float *b_v2 = nullptr, *b_img = nullptr, *b_dobs = nullptr;
    float* b_illum = nullptr;    // the shots' source illuminations, [shots] fields (fdw_shot_batch_illum); allocated on first use
    int b_illum_cap = 0;         // ... shots it holds
    bool batch_illum = false;    // inside fdw_shot_batch_illum's forward loop: the one place a batched launch accumulates illumination
    float* b_rec = nullptr;      // the shots' modelled gathers [shots][nt][nx] (fdw_shot_batch_residual); allocated on first use
    size_t b_rec_cap = 0;
    float* d_wav = nullptr;      // the line-source gather of fdw_shot_line / fdw_record_shot_line, [nt][nx] (one step's samples contiguous)
    size_t wav_cap = 0;
    float* b_wav = nullptr;      // the shots' line-source gathers [shots][nt][nx] (fdw_shot_line_batch and its kin); allocated on first use
    size_t b_wav_cap = 0;
    float* d_raw = nullptr;      // gathers as the caller holds them ([shot][nx][nt]) before the transposition on the device
    size_t raw_cap = 0;
    int no_fused_back = 0;   // experiments / tests: backward iterations as two launches (source step, receiver step) -- FDW_NO_FUSED_BACK=1
    int no_back_pipe = 0;    // experiments / tests: no wave-pipeline passes in the backward loop -- FDW_NO_BACK_PIPE=1
    int no_back_fused = 0;   // experiments / tests: the backward pipeline as two passes (source field, receiver field) instead of the fused kernel -- FDW_NO_BACK_FUSED=1
    int no_born_fused = 0;   // benchmarks / tests: Born modelling as two step launches and a scatter kernel at orders <= 8 too -- FDW_NO_BORN_FUSED=1
    float* d_born_m = nullptr;     // fdw_born_shot: the reflectivity embedded into a zeroed field; allocated on first use
    float* d_born_rec0 = nullptr;  // ... the background gather [nt][nx] beside d_rec
    size_t born_rec0_cap = 0;
    float* d_dtt_w = nullptr;      // DTT imaging without the fused kernel: F_{i-2} (-) F_{i-1} on C, taken before the source step overwrites F_{i-2}
    float* d_born_w = nullptr;     // Born modelling without the fused kernel, FDW_BORN_DTT: (A - B) of the background on the interior cells
    float* d_eimg = nullptr;       // fdw_shot_ext: the planes of the extended image, eimg_planes fields; allocated on first use, sized for the largest H seen
    int eimg_planes = 0;
    int ext_pointwise = 0;         // benchmarks / tests: the extended-image term one thread per cell instead of the march -- FDW_EXT_POINTWISE=1
    float* b_born_rec0 = nullptr;  // fdw_born_shot_batch with data0: the shots' background gathers [shots][nt][nx]; allocated on first use
    size_t b_born_rec0_cap = 0;
    // least-squares migration (fdw_lsm_visit, fdw_lsm_solve); allocated on first use
    float* d_lsm_f[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // m, g, p, h, the mask, the verify pass's scratch image
    float* d_lsm_dobs = nullptr;   // the shots' data gathers [shots][nt][nx]
    float* d_lsm_res = nullptr;    // the verify pass's residual gathers [shots][nt][nx]
    float* d_lsm_d = nullptr;      // doubles: row sums, the solver's scalars, the shots' n2, the misfit history (LsmDoubles)
    size_t lsm_dobs_cap = 0, lsm_res_cap = 0, lsm_d_cap = 0;
    size_t store_budget = 0; // fdw_rtm_stored_shot: bytes the stored source fields may take (0: whatever the device grants); fdw_set_store_budget
    int store_segments = 0;  // ... segments the last such shot was cut into (1: every field kept)
    size_t batch_budget = 0; // bytes a batch of shots may take (0: FDW_BATCH_BUDGET_BYTES, else 6 GiB); written by fdw_set_batch_budget alone
    int batch_parts = 0;     // batched launch sequences of the last batched call (0: its shots ran one by one); fdw_batch_parts
    bool batch_single = false;      // inside a batched call: a part of more than one shot ran its shots one by one
    // consecutive four-step forward passes as row bands on side streams (fdw_set_pass_bands; band_passes)
    int pb_bands = 0, pb_depth = 0;             // the policy; 0, 0: automatic
    int pb_used_bands = 0, pb_used_depth = 0;   // what the last forward loop used (fdw_pass_bands)
    int pc_lo = 0, pc_hi = 0;                   // two bands with a moving cut (fdw_set_pass_cut): the policy; 0, 0: automatic, -1, -1: off
    int pc_used_lo = -1, pc_used_hi = -1, pc_used_turns = 0;      // what the last forward loop used (fdw_pass_cut)
    hipStream_t pb_side[FDW_PASS_DEPTH_MAX - 1] = {};      // created on first use
    hipEvent_t pb_fork = nullptr, pb_join[FDW_PASS_DEPTH_MAX - 1] = {}, pb_ring[kBandRing] = {};
};

static size_t field_elems(const fdw_ctx* c) { return (size_t)c->nxl * (size_t)c->pitch; }

extern "C" int fdw_pitch(const fdw_ctx* c) { return c ? c->pitch : 0; }
extern "C" size_t fdw_field_bytes(const fdw_ctx* c) { return c ? field_elems(c) * sizeof(float) : 0; }

static int is_full_grid(const fdw_ctx* c) { return c->slab.x_off == 0 && c->nxl == c->prm.nxe; }

static hipStream_t pick_stream(fdw_ctx* c, void* s) { return s ? (hipStream_t)s : c->stream; }

static int alloc_zero(float** p, size_t elems)
{
    if (*p) return FDW_OK;
    hipError_t e = hipMalloc((void**)p, elems * sizeof(float));
    if (e != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc(%zu bytes) failed: %s", elems * sizeof(float), hipGetErrorString(e));
    HIP_TRY(hipMemset(*p, 0, elems * sizeof(float)));
    HIP_TRY(hipDeviceSynchronize());   // the context stream is non-blocking: do not let it overtake the memset
    return FDW_OK;
}

static int ensure_work_buffers(fdw_ctx* c, int nfields, bool need_img)
{
    for (int i = 0; i < nfields; i++) {
        int rc = alloc_zero(&c->fld[i], field_elems(c));
        if (rc) return rc;
    }
    int rc = alloc_zero(&c->d_v2, field_elems(c));
    if (rc) return rc;
    if (need_img) {
        rc = alloc_zero(&c->d_img, field_elems(c));
        if (rc) return rc;
    }
    return FDW_OK;
}

static int ensure_cap(float** p, size_t* cap, size_t elems)
{
    if (*cap >= elems && *p) return FDW_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc((void**)p, std::max<size_t>(elems, 1) * sizeof(float));
    if (e != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    *cap = elems;
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// create / destroy
// ------------------------------------------------------------------------------------------------
static int validate(const fdw_params* p, const fdw_slab* s)
{
    if (!p) return fail(FDW_EINVAL, "params is NULL");
    if (p->order < 2 || p->order > FDW_MAX_ORDER || (p->order & 1))
        return fail(FDW_EINVAL, "order=%d must be even and in [2,%d]", p->order, FDW_MAX_ORDER);
    if (p->nxe <= p->order || p->nze <= p->order)
        return fail(FDW_EINVAL, "grid %dx%d too small for order %d", p->nxe, p->nze, p->order);
    if (p->nxb < 0 || p->nzb < 0 || 2 * p->nxb >= p->nxe || 2 * p->nzb >= p->nze)
        return fail(FDW_EINVAL, "borders nxb=%d nzb=%d do not leave an interior in %dx%d", p->nxb, p->nzb, p->nxe, p->nze);
    if ((p->nxb > 0 || p->nzb > 0) && !(p->fac > 0.0f && p->fac <= 1.0f))
        return fail(FDW_EINVAL, "fac=%g must be in (0,1]", (double)p->fac);
    if (!(p->dx > 0.0f) || !(p->dz > 0.0f)) return fail(FDW_EINVAL, "dx, dz must be positive");
    if (p->nt < 0) return fail(FDW_EINVAL, "nt=%d is negative", p->nt);
    if (p->dialect < FDW_DIALECT_RTM || p->dialect > FDW_DIALECT_RTM_STORED) return fail(FDW_EINVAL, "dialect=%d is unknown", p->dialect);
    if (p->dialect != FDW_DIALECT_RTM && p->order > 2 * kMaxFastHalfOrder)
        return fail(FDW_EINVAL, "dialects 1 and 2 are built for orders 2..%d", 2 * kMaxFastHalfOrder);
    if (p->numerics != FDW_NUMERICS_EXACT && p->numerics != FDW_NUMERICS_FAST) return fail(FDW_EINVAL, "numerics=%d is unknown", p->numerics);
    if (s->nxl <= p->order || s->x_off < 0 || s->x_off + s->nxl > p->nxe)
        return fail(FDW_EINVAL, "slab [%d,%d) does not fit the grid (nxe=%d) or is thinner than the stencil",
                    s->x_off, s->x_off + s->nxl, p->nxe);
    return FDW_OK;
}

extern "C" int fdw_create_slab(const fdw_params* prm, const fdw_slab* slab, int device, fdw_ctx** out)
{
    if (!out) return fail(FDW_EINVAL, "out is NULL");
    *out = nullptr;
    if (!slab) return fail(FDW_EINVAL, "slab is NULL");
    int rc = validate(prm, slab);
    if (rc) return rc;

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(FDW_ENODEVICE, "no HIP device available (%s); libfdwave has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device < 0 || device >= ndev) return fail(FDW_ENODEVICE, "device %d out of range (have %d)", device, ndev);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return fail(FDW_ENODEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(FDW_ENODEVICE, "device %d is %s; libfdwave is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    if ((e = hipSetDevice(device)) != hipSuccess) return fail(FDW_ENODEVICE, "hipSetDevice: %s", hipGetErrorString(e));

    fdw_ctx* c = new (std::nothrow) fdw_ctx();
    if (!c) return fail(FDW_ENOMEM, "out of host memory");
    c->prm = *prm;
    c->slab = *slab;
    c->device = device;
    c->h = prm->order / 2;
    c->nxl = slab->nxl;
    c->nx = prm->nxe - 2 * prm->nxb;
    c->nz = prm->nze - 2 * prm->nzb;
    c->pitch = ((prm->nze + 63) / 64) * 64;  // 256-B aligned rows: every lane's float4 is aligned
    if (const char* nf = getenv("FDW_NO_FUSED_BACK")) c->no_fused_back = atoi(nf);
    if (const char* nf = getenv("FDW_NO_BACK_PIPE")) c->no_back_pipe = atoi(nf);
    if (const char* nf = getenv("FDW_NO_BORN_FUSED")) c->no_born_fused = atoi(nf);
    if (const char* nf = getenv("FDW_NO_BACK_FUSED")) c->no_back_fused = atoi(nf);
    if (const char* nf = getenv("FDW_EXT_POINTWISE")) c->ext_pointwise = atoi(nf);
    if (const char* pad = getenv("FDW_PITCH_PAD")) {   // experiment knob: extra floats per row (multiple of 4)
        const int extra = atoi(pad);
        if (extra > 0 && extra % 4 == 0) c->pitch += extra;
    }

    // launch extents, R:185-195 (the int assignment truncates before ceil)
    const bool mod = prm->dialect != FDW_DIALECT_RTM;              // the CPU-serial sibling's arithmetic (fd.c)
    const bool four_sided = prm->dialect == FDW_DIALECT_MOD;       // taper_apply (mod_main) vs taper_apply2 (rtm_main)
    if (mod) {                    // fd.c:24-46 and taper.c walk the whole array; taper_apply's z table spans the whole row
        c->xlim = prm->nxe;
        c->zlim = prm->nze;
        c->ztap = four_sided ? prm->nze : prm->nzb;
    } else if (prm->compat) {
        c->xlim = 8 * (prm->nxe / 8);
        c->zlim = 8 * (prm->nze / 8);
        c->ztap = 8 * (prm->nzb / 8);
    } else {
        c->xlim = prm->nxe;
        c->zlim = prm->nze;
        c->ztap = prm->nzb;
    }
    const int h = c->h, xo = slab->x_off;
    // kernel_lap covers i = h + t, t < xlim threads, and i < nxe - h (R:56-64)
    const int glx0 = h, glx1 = std::min(prm->nxe - h, h + c->xlim);
    c->lap_x0 = std::max(h, glx0 - xo);
    c->lap_x1 = std::min(c->nxl - h, glx1 - xo);
    c->lap_z0 = h;
    c->lap_z1 = std::min(prm->nze - h, h + c->zlim);
    // the stencil program rounds its grid up to 32 (S:231-238): whole interior
    c->slap_x0 = std::max(h, h - xo);
    c->slap_x1 = std::min(c->nxl - h, prm->nxe - h - xo);
    c->slap_z0 = h;
    c->slap_z1 = prm->nze - h;
    c->upd_x1 = std::max(0, std::min(c->nxl, c->xlim - xo));
    c->upd_z1 = c->zlim;
    c->tz_x1 = c->upd_x1;
    // rows outside [xt_lo, xt_hi) carry an x damping factor or miss the z factor (corner tiles)
    c->xt_lo = std::max(0, std::min(c->nxl, prm->nxb - xo));
    c->xt_hi = std::max(c->xt_lo, std::min(c->nxl, std::min(prm->nxe - prm->nxb, c->xlim) - xo));

    // derived constants, R:203-217 (double quotient narrowed to float; float*float scaling)
    const float dx2inv = (1. / prm->dx) * (1. / prm->dx);
    const float dz2inv = (1. / prm->dz) * (1. / prm->dz);
    c->dt2 = prm->dt * prm->dt;
    c->dx2inv = dx2inv;
    c->dz2inv = dz2inv;
    float w[FDW_MAX_ORDER + 1];
    fdw_calc_coefs(prm->order, mod ? 1 : prm->coef_cxx, w);
    for (int io = 0; io <= prm->order; io++) {
        c->cz[io] = mod ? w[io] : dz2inv * w[io];      // fd.c:33-34 scales inside every term
        c->cx[io] = mod ? w[io] : dx2inv * w[io];
    }
    for (int io = 0; io <= prm->order; io++) {      // FAST numerics of the sibling's dialects: c_k * d?2inv once, instead of inside every term
        c->fcz[io] = mod ? w[io] * dz2inv : c->cz[io];
        c->fcx[io] = mod ? w[io] * dx2inv : c->cx[io];
    }
    c->c0 = c->fcz[c->h] + c->fcx[c->h];    // FAST numerics: the centre point's weight (one fp32 add, part of that mode's definition)
    c->taper_x.assign(std::max(prm->nxb, 1), 1.0f);
    c->taper_z.assign(std::max(prm->nzb, 1), 1.0f);
    if (mod) {
        fdw_mod_taper_tables(prm->nxb, prm->nzb, prm->fac, c->taper_x.data(), c->taper_z.data());
        if (four_sided) {         // taper.c:50-56 as ONE factor per column: top strip, 1.0f, mirrored bottom strip
            std::vector<float> full(prm->nze, 1.0f);
            for (int i = 0; i < prm->nzb; i++) {
                full[i] = c->taper_z[i];
                full[prm->nze - 1 - i] = c->taper_z[i];
            }
            c->taper_z.swap(full);
        }                         // taper_apply2 (taper.c:68-83) has the CUDA path's shape: z factors on the top strip, x factors inside it only
    } else {
        if (prm->nxb > 0) fdw_taper_tables(prm->nxb, 0, prm->fac, c->taper_x.data(), nullptr);
        if (prm->nzb > 0) fdw_taper_tables(0, prm->nzb, prm->fac, nullptr, c->taper_z.data());
    }
    // per-row x factor: thread i < nxb (and < xlim) scales columns i and nxe-1-i by taperx[i] (R:108-115)
    c->txfac.assign(c->nxl, 1.0f);
    for (int l = 0; l < c->nxl; l++) {
        const int g = xo + l, gm = prm->nxe - 1 - g;
        if (g < prm->nxb && g < c->xlim) c->txfac[l] = c->taper_x[g];
        else if (gm < prm->nxb && gm < c->xlim) c->txfac[l] = c->taper_x[gm];
    }

#define CREATE_TRY(call)                                                                                  \
    do {                                                                                                  \
        hipError_t e2_ = (call);                                                                          \
        if (e2_ != hipSuccess) {                                                                          \
            fail(FDW_EHIP, "%s failed: %s", #call, hipGetErrorString(e2_));                               \
            fdw_destroy(c);                                                                               \
            return FDW_EHIP;                                                                              \
        }                                                                                                 \
    } while (0)
    CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const size_t ntz = std::max(c->ztap, 1);
    CREATE_TRY(hipMalloc((void**)&c->d_taperz, ntz * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&c->d_txfac, c->nxl * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&c->d_gcx, (FDW_MAX_ORDER + 1) * sizeof(float)));
    CREATE_TRY(hipMalloc((void**)&c->d_gcz, (FDW_MAX_ORDER + 1) * sizeof(float)));
    CREATE_TRY(hipMemcpy(c->d_taperz, c->taper_z.data(), std::min<size_t>(ntz, c->taper_z.size()) * sizeof(float), hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(c->d_txfac, c->txfac.data(), c->nxl * sizeof(float), hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(c->d_gcx, c->cx, (FDW_MAX_ORDER + 1) * sizeof(float), hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(c->d_gcz, c->cz, (FDW_MAX_ORDER + 1) * sizeof(float), hipMemcpyHostToDevice));
    CREATE_TRY(hipMalloc((void**)&c->d_peak, sizeof(unsigned)));      // so that fdw_dev_image_excitation never allocates
    c->peak_cap = 1;
#undef CREATE_TRY
    *out = c;
    return FDW_OK;
}

extern "C" int fdw_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

extern "C" int fdw_device_usable(int device)
{
    const int n = fdw_device_count();
    if (device < 0 || device >= n) return fail(FDW_ENODEVICE, "device %d does not exist (%d visible)", device, n);
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return fail(FDW_ENODEVICE, "hipGetDeviceProperties(%d): %s", device, hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(FDW_ENODEVICE, "device %d is %s; libfdwave is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    if ((e = hipSetDevice(device)) != hipSuccess) return fail(FDW_ENODEVICE, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    return FDW_OK;
}

extern "C" int fdw_create(const fdw_params* prm, int device, fdw_ctx** out)
{
    if (!prm) return fail(FDW_EINVAL, "params is NULL");
    fdw_slab s{0, prm->nxe};
    return fdw_create_slab(prm, &s, device, out);
}

extern "C" void fdw_destroy(fdw_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipStream_t side : c->pb_side)
        if (side) {
            (void)hipStreamSynchronize(side);
            (void)hipStreamDestroy(side);
        }
    for (hipEvent_t e : c->pb_join)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->pb_ring)
        if (e) (void)hipEventDestroy(e);
    if (c->pb_fork) (void)hipEventDestroy(c->pb_fork);
    float* bufs[] = {c->d_taperz, c->d_txfac, c->d_gcx, c->d_gcz, c->fld[0], c->fld[1], c->fld[2], c->fld[3],
                     c->fld[4], c->fld[5], c->fld[6], c->fld[7], c->fld[8], c->fld[9], c->d_v2, c->d_img, c->d_illum, c->d_srce, c->d_dobs, c->d_rec,
                     c->d_vp, c->d_vpe, (float*)c->d_draws, (float*)c->d_jump, c->bfld[0], c->bfld[1], c->bfld[2], c->bfld[3],
                     c->bfld[4], c->bfld[5], c->bfld[6], c->bfld[7], c->b_v2, c->b_img, c->b_dobs, c->b_illum, c->b_rec, c->b_wav, c->d_raw, c->d_wav, c->d_snap[0], c->d_snap[1], c->d_snap[2], c->d_amp, (float*)c->d_texc, c->d_exc, (float*)c->d_peak,
                     c->d_born_m, c->d_born_rec0, c->d_born_w, c->b_born_rec0, c->d_dtt_w, c->d_eimg,
                     c->d_lsm_f[0], c->d_lsm_f[1], c->d_lsm_f[2], c->d_lsm_f[3], c->d_lsm_f[4], c->d_lsm_f[5], c->d_lsm_dobs, c->d_lsm_res, c->d_lsm_d};
    for (float* b : bufs)
        if (b) (void)hipFree(b);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// ------------------------------------------------------------------------------------------------
// launch geometry + one step
// ------------------------------------------------------------------------------------------------
// ring size of the register-ring kernel for (half order, prefetch) -- must match RingGeom in fdw_device.h
static int ring_rows(int h, int pf) { return ((2 * h + pf + pf - 1) / pf) * pf; }
static int effective_prefetch(const fdw_ctx* c) { return (c->h == 4 && c->prefetch >= 1 && c->prefetch <= 3) ? c->prefetch : 2; }

static void fill_geometry(const fdw_ctx* c, StepArgs& a, int rows, int batch = 1)
{
    const int nstrips = (c->pitch + 255) / 256;
    int wz = c->wz;
    if (wz != 1 && wz != 2 && wz != 4) wz = nstrips >= 4 ? 4 : (nstrips >= 2 ? 2 : 1);
    int xchunk = c->xchunk;
    if (xchunk <= 0) {
        // Measured on MI355X (scripts/probe_step.py, order 8): once every tile runs the same
        // branch-free body the step time is flat in the chunk length to within run-to-run noise,
        // with a shallow optimum at short chunks (many waves per CU slot = good balance; the 2H
        // halo rows a neighbouring chunk re-reads come from L2 / Infinity Cache, not HBM).
        //   HBM-resident grids (>= 8192^2): one ring turn (10 rows at prefetch 2)
        //   Infinity-Cache-resident grids (4096^2): 24 rows
        //   small decks (new_mod 415x295 ... 2048^2): as many waves as the grid gives, down to ONE row per
        //   wave -- a launch is a latency chain (prologue + rows), 5.1 us/step at 1 row vs 12.7 at 8 on new_mod
        const long strip_rows = (long)rows * nstrips * batch;   // a batch of shots counts as one grid of that many rows
        if (strip_rows >= 200000) xchunk = ring_rows(c->h, effective_prefetch(c));
        else if (strip_rows >= 60000) xchunk = 24;   // 4096^2 class (Infinity-Cache resident)
        else xchunk = (int)std::min<long>(std::max<long>((strip_rows + 4095) / 4096, 1), 10);   // >= ~4096 waves, down to 1 row each;
                                                                                                  // a 1056 x 8192 slab (N = 8) lands on 9: 293 Gpt/s vs 268 at 24
    }
    a.xchunk = xchunk;
    a.wz = wz;
    a.nzblk = (nstrips + wz - 1) / wz;
    const int chunks = (rows + xchunk - 1) / xchunk;
    const int wpx = 4 / wz;
    const int nxblk = (chunks + wpx - 1) / wpx;
    a.nblk = a.nzblk * nxblk;
    a.nper = (a.nblk + 7) / 8;
}

// ---- launch arguments: what the one-step, two-step and wave-pipeline kernels share ----------------------
// inj_x of a launch without a point source.  It matches no row, also after a batch's shift inj_x + b * inj_dx (|b * inj_dx| < nxl), and lies
// far outside the halo rows the multi-step kernels look at for a source (inj_x >= xa - H).
constexpr int kNoRow = -1000000;

// field pointers, geometry, numerics and the coefficient table (EXACT or FAST weights; taps beyond the order are 0)
template <class A>
static void fill_common(const fdw_ctx* c, A& a, const float* d_p, decltype(A::pp) d_pp, const float* d_v2, int pp_twice)
{
    a.p = d_p; a.pp = d_pp; a.v2 = d_v2;
    a.taperz = c->d_taperz; a.txfac = c->d_txfac;
    a.pitch = c->pitch; a.nxl = c->nxl;
    a.lap_x0 = c->lap_x0; a.lap_x1 = c->lap_x1; a.lap_z0 = c->lap_z0; a.lap_z1 = c->lap_z1;
    if constexpr (std::is_same_v<A, Step2Args>) a.upd_x1 = c->upd_x1;
    a.upd_z1 = c->upd_z1;
    a.ztap = c->ztap; a.tz_x1 = c->tz_x1; a.xt_lo = c->xt_lo; a.xt_hi = c->xt_hi;
    a.pp_twice = pp_twice ? 1 : 0;
    a.img_z1 = c->prm.nzb + std::min(c->nz, c->zlim);      // kernel_img: interior columns j < zlim && j < nz (R:133-144)
    a.dt2 = c->dt2;
    a.c0 = c->c0;
    a.numerics = c->prm.numerics;
    a.dx2inv = c->dx2inv; a.dz2inv = c->dz2inv;            // read by the instantiations of the sibling's dialects only
    const bool fastw = c->prm.numerics == FDW_NUMERICS_FAST;      // (for the RTM dialect fcx / fcz are cx / cz)
    for (int io = 0; io <= 2 * kMaxFastHalfOrder; io++) {
        a.cx[io] = io <= c->prm.order ? (fastw ? c->fcx[io] : c->cx[io]) : 0.0f;
        a.cz[io] = io <= c->prm.order ? (fastw ? c->fcz[io] : c->cz[io]) : 0.0f;
    }
}

// this step's trace row on the receiver line (interior rows nxb .. nxb+nx-1, R:126-129): rec[r - rec_x0] = a field at (r, rec_z)
template <class A>
static void fill_rec(const fdw_ctx* c, A& a, float* d_rec, int rec_z)
{
    a.rec = d_rec; a.rec_z = rec_z;
    a.rec_x0 = c->prm.nxb - c->slab.x_off; a.rec_n = c->nx;
}

// the modelling dialect (mod_main): the weights of the 7x7 Gaussian source and this step's trace row, rec[r - rec_x0] = p(r, rec_z)
template <class A>
static int fill_mod(const fdw_ctx* c, A& a, const char* who, float* d_rec, int rec_z)
{
    if (d_rec && (rec_z < 0 || rec_z >= c->prm.nze)) return fail(FDW_EINVAL, "%s: receiver depth %d outside the grid", who, rec_z);
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) a.gw[i][j] = expf(-(float)(i * i) - (float)(j * j));   // ptsrc.c:53 with exp(float) as g++ resolves it
    fill_rec(c, a, d_rec, rec_z);
    return FDW_OK;
}

// where a launch injects, in local rows: from row x (kNoRow: nowhere), n receiver rows (0 for a point source); the sample of row x sits at
// `shift` in the caller's sample row
struct Injection {
    int x = kNoRow, n = 0;
    ptrdiff_t shift = 0;
};

// The point source of a FWD / DD_FWD / MOD launch at global (sx, sz).  None without samples, nor at sx < 0 outside the modelling dialect
// (the callers' "no source").  A row outside this slab matches no row of the launch.
static int place_source(const fdw_ctx* c, const char* who, bool mod, const float* d_inj, int sx, int sz, Injection* in)
{
    if (!d_inj || (!mod && sx < 0)) return FDW_OK;
    if (sz < 0 || sz >= c->prm.nze || sx < 0 || sx >= c->prm.nxe) return fail(FDW_EINVAL, "%s: source (%d,%d) outside the grid", who, sx, sz);
    in->x = sx - c->slab.x_off;
    if (in->x >= c->upd_x1 && in->x < c->nxl)
        return fail(FDW_EINVAL, "%s: source row %d lies in rows the reference never time-steps (>= %d)", who, sx, c->xlim);
    return FDW_OK;
}

// Receivers at depth gz on the interior rows off .. off+nx-1 (R:126-129: off = nxb) below xlim, clipped to this slab.  The sibling's rtm_main
// offsets them by nzb instead (PP[ix+nzb][gz], rtm_main.cpp:203) -- the same thing only when both borders are equally wide; kept as is.
static int place_receivers(const fdw_ctx* c, const char* who, int off, int gz, Injection* in)
{
    if (gz < 0 || gz >= c->prm.nze) return fail(FDW_EINVAL, "%s: receiver depth %d outside the grid", who, gz);
    if (off + c->nx > c->prm.nxe) return fail(FDW_EINVAL, "%s: receiver rows [%d,%d) leave the grid", who, off, off + c->nx);
    const int l0 = std::max(off - c->slab.x_off, 0), l1 = std::min(off + std::min(c->nx, c->xlim) - c->slab.x_off, c->nxl);
    in->x = l0;
    in->n = std::max(0, l1 - l0);
    in->shift = l0 + c->slab.x_off - off;
    return FDW_OK;
}

// The line source of a forward launch (fdwave.h, "line sources"): one sample per interior row the loop time-steps, rows nxb .. nxb+nsrc-1 with
// nsrc = min(nx, xlim - nxb), on column sz.  Full-grid contexts only (the callers check): local rows are global rows.
static int place_line(const fdw_ctx* c, const char* who, int sz, Injection* in)
{
    if (sz < 0 || sz >= c->zlim) return fail(FDW_EINVAL, "%s: line-source depth %d outside the time-stepped columns [0,%d)", who, sz, c->zlim);
    in->x = c->prm.nxb;
    in->n = std::max(0, std::min(c->nx, c->xlim - c->prm.nxb));
    return FDW_OK;
}

// ---- what a forward pass does besides stepping ------------------------------------------------------------------------------------------
// excitation-amplitude imaging (fdwave.h): what one forward step does on top of its update.  Maps: exc_arr = amp, where the new field beats
// it strictly in magnitude amp takes it and texc takes the key (= it + 1).  Pick: exc_arr = exc, which takes the new field where
// texc == key (= top - it); texc is only read.
enum class Exc { none, maps, pick };

// The description of a forward loop, filled where the loop is asked for: its arrays hold all iterations.  The launch builders take a
// FwdView, which only view_at() makes: the launch whose first step is iteration `it`.
struct Forward {
    const float* samples = nullptr;   // the wavelet [nt] of a point source at (sx, sz) -- NULL, or sx < 0 outside the modelling dialect: none --
    int sx = -1, sz = 0;
    bool line = false;                // ... or the line-source gather [nt][nx] on column sz (sx unused)
    float* rec = nullptr;             // recording: the trace rows [nt][nx] at depth gz
    int gz = 0;
    float* illum = nullptr;           // the source illumination accumulator
    Exc exc = Exc::none;              // the excitation maps of a point-source pass / the pick of a line-source pass
    float* exc_arr = nullptr;         // amp (maps) or exc (pick)
    int* texc = nullptr;
    int top = 0;                      // pick: iteration it takes the cells with texc == top - it
    bool may_band = false;            // fdw_dev_steps2: the loop's pipeline passes may run as row bands (steps_loop)
    Forward recording(float* d_rec, int rec_z) const { Forward v = *this; v.rec = d_rec; v.gz = rec_z; return v; }      // (NULL: none)
    Forward illuminating(float* d_illum) const { Forward v = *this; v.illum = d_illum; return v; }
    Forward exciting(Exc what, float* arr, int* map, int pick_top) const { Forward v = *this; v.exc = what; v.exc_arr = arr; v.texc = map; v.top = pick_top; return v; }
};
struct FwdView : Forward {
    int exc_key = 0;                  // the excitation key of the launch's first step
    float* out = nullptr;             // DD_FWD: the new field goes here instead of over pp
};
// The strides, stated once: a line source advances nx samples per step and a point source one, a trace row is nx samples, the maps' key
// is it + 1 and the pick's top - it.
static FwdView view_at(const Forward& f, int it, int nx)
{
    FwdView v;
    static_cast<Forward&>(v) = f;
    if (f.samples) v.samples = f.samples + (size_t)it * (f.line ? (size_t)nx : 1);
    if (f.rec) v.rec = f.rec + (size_t)it * (size_t)nx;
    v.exc_key = f.exc == Exc::pick ? f.top - it : it + 1;
    return v;
}
// a point source at (sx, sz) with the samples d_srce (NULL: no source) / a line source on column sz with the gather d_wav
static Forward point_source(const float* d_srce, int sx, int sz) { Forward f; f.samples = d_srce; f.sx = d_srce ? sx : -1; f.sz = sz; return f; }
static Forward line_source(const float* d_wav, int sz) { Forward f; f.samples = d_wav; f.sz = sz; f.line = true; return f; }
// what a backward launch injects: its first iteration's receiver samples [nx], at depth gz
static FwdView receiver_samples(const float* d_samples, int gz) { return view_at(point_source(d_samples, -1, gz), 0, 0); }

// The forward variants the launchers are built for: (line?, records?, illuminates?, excitation) <-> launcher mode, and what each kernel
// family does with it.  The one-step ring family and the pipeline have a kernel for every row.  two_step: the two-step family has one (a
// pair of such steps is two single steps on copies otherwise).  generic: what the generic-order family launches for it; where that is
// another mode, the illumination / excitation follows the plain step as an add kernel.  A new variant is one row here.
static const struct FwdVariant {
    int kmode;
    bool line, rec, illum;
    Exc exc;
    bool two_step;
    int generic;
} kFwdVariants[] = {
    // kmode, line, rec, illum, exc, two_step, generic
    {FDW_MODE_FWD, false, false, false, Exc::none, true, FDW_MODE_FWD},
    {FDW_MODE_FWD_REC, false, true, false, Exc::none, true, FDW_MODE_FWD_REC},
    {FDW_MODE_FWD_ILLUM, false, false, true, Exc::none, true, FDW_MODE_FWD},
    {FDW_MODE_FWD_REC_ILLUM, false, true, true, Exc::none, false, FDW_MODE_FWD_REC},
    {FDW_MODE_FWD_LINE, true, false, false, Exc::none, true, FDW_MODE_FWD_LINE},
    {FDW_MODE_FWD_LINE_REC, true, true, false, Exc::none, true, FDW_MODE_FWD_LINE_REC},
    {FDW_MODE_FWD_LINE_ILLUM, true, false, true, Exc::none, true, FDW_MODE_FWD_LINE},
    {FDW_MODE_FWD_LINE_REC_ILLUM, true, true, true, Exc::none, true, FDW_MODE_FWD_LINE_REC},
    {FDW_MODE_FWD_EXC, false, false, false, Exc::maps, false, FDW_MODE_FWD},
    {FDW_MODE_FWD_LINE_PICK, true, false, false, Exc::pick, false, FDW_MODE_FWD_LINE},
};
// The row of a launch of base mode `mode` with these extras.  Only FWD has variants: the other modes (PLAIN, RECV, MOD ...) are served as
// they are by every family that takes them.  kmode -1: no kernel is built for the combination.
static FwdVariant fwd_variant(int mode, const Forward& f)
{
    for (const FwdVariant& v : kFwdVariants)
        if (mode == FDW_MODE_FWD && v.line == f.line && v.rec == (f.rec != nullptr) && v.illum == (f.illum != nullptr) && v.exc == f.exc) return v;
    return FwdVariant{mode == FDW_MODE_FWD ? -1 : mode, false, false, false, Exc::none, true, mode};
}
// whether the family of `steps` steps per pass (1: ring or generic order, 2: two-step, kPipeSteps: pipeline) serves it in one pass
static bool family_serves(int steps, const FwdVariant& v) { return steps != 2 || v.two_step; }

// rec*, img, texc and exc_key of a forward launch from its view
template <class A>
static void fill_forward(const fdw_ctx* c, A& a, const FwdVariant& v, const FwdView& f)
{
    if (v.rec) fill_rec(c, a, f.rec, f.gz);
    if (v.illum) a.img = f.illum;      // the accumulator travels in `img`
    if (f.exc != Exc::none) {
        a.img = f.exc_arr; a.texc = f.texc; a.exc_key = f.exc_key;
    }
}

// Where a launch of `mode` injects f.samples: the line or the point of a forward launch (a line's samples: [steps][nx] at depth f.sz), or
// the receiver rows of a backward launch (receiver_samples).
static int place_injection(const fdw_ctx* c, const char* who, int mode, const FwdView& f, Injection* in)
{
    if (f.line) {
        if (mode != FDW_MODE_FWD || !f.samples) return fail(FDW_EINVAL, "%s: a line source drives a forward launch", who);
        return place_line(c, who, f.sz, in);
    }
    if (mode == FDW_MODE_FWD || mode == FDW_MODE_DD_FWD || mode == FDW_MODE_MOD) return place_source(c, who, mode == FDW_MODE_MOD, f.samples, f.sx, f.sz, in);
    if (mode == FDW_MODE_RECV || mode == FDW_MODE_DD_RECV || mode == FDW_MODE_BACK || mode == FDW_MODE_BACK4)
        return place_receivers(c, who, mode == FDW_MODE_DD_RECV ? c->prm.nzb : c->prm.nxb, f.sz, in);
    return FDW_OK;
}

// Receiver rows [x, x+n) from upd_x1 up to r1 lie beyond the time-stepped rows (narrow x border + truncated extents): the reference still
// injects into them and images them.  `samples` holds row x's sample.
static int static_receiver_rows(fdw_ctx* c, int x, int n, int r1, float* field, const float* samples, const float* psrc, float* img, int gz,
                                int img_z1, hipStream_t s)
{
    const int s0 = std::max(x, c->upd_x1), s1 = std::min(x + n, r1);
    if (s1 <= s0) return FDW_OK;
    hipError_t e = launch_static_rows(field, psrc, img, samples + (s0 - x), c->pitch, s0, s1 - s0, gz, c->prm.nzb, img_z1, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "static-row launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

// the cell set C of the Born scatter and of DTT imaging on a full-grid context: rows [x0, x1), columns [z0, z1)
struct BornCells {
    int x0, x1, z0, z1;
};
static BornCells born_cells(const fdw_ctx* c)
{
    return BornCells{c->prm.nxb, std::min(c->prm.nxb + c->nx, c->xlim), c->prm.nzb, std::min(c->prm.nzb + c->nz, c->zlim)};
}

struct BackExtra {           // what the receiver / imaging variants of the one-step and two-step kernels need on top of the forward ones
    const float* inj2 = nullptr;      // two-step: the receiver samples of iteration it+1
    const float* psrc_a = nullptr;    // the source field the new receiver field is imaged against (two-step: iteration it's)
    const float* psrc_b = nullptr;    // two-step: iteration it+1's
    float* img = nullptr;
    float* fpp = nullptr;             // BACK: the older source field, stepped in place by the same launch
    // second-time-difference imaging (fdwave.h, "DTT imaging"):
    bool no_img = false;              // RECV: the receiver step and its injection alone -- the image is neither read nor written
    bool dtt = false;                 // BACK: the DTT value of the imaging epilogue (FDW_MODE_BACK_DTT)
};

// One launch of the one-step kernels on rows [r0, r1).  f (a view): the source, trace row and accumulators of a FWD / DD_FWD / MOD step, the
// receiver samples of a RECV / DD_RECV / BACK step; bk: the source field and image of the latter.
static int step_impl(fdw_ctx* c, int mode, const float* d_p, float* d_pp, const float* d_v2, int r0, int r1, int pp_twice, const FwdView& f,
                     const BackExtra& bk, hipStream_t s)
{
    const bool lap = (mode == FDW_MODE_LAP);
    if (!d_p || !d_pp) return fail(FDW_EINVAL, "step: field pointer is NULL");
    if (!lap && !d_v2) return fail(FDW_EINVAL, "step: v2 is NULL");
    if ((mode == FDW_MODE_RECV || mode == FDW_MODE_DD_RECV || mode == FDW_MODE_BACK) && !(bk.no_img && mode == FDW_MODE_RECV) && (!bk.psrc_a || !bk.img || !f.samples))
        return fail(FDW_EINVAL, "step: RECV needs d_inj, d_psrc and d_img");
    if (bk.no_img && (mode != FDW_MODE_RECV || !f.samples)) return fail(FDW_EINVAL, "step: the receiver step without imaging is a RECV step with d_inj");
    if (bk.dtt && mode != FDW_MODE_BACK) return fail(FDW_EINVAL, "step: the DTT epilogue belongs to a BACK step");
    if (mode == FDW_MODE_BACK && (!bk.fpp || bk.fpp == d_pp || bk.fpp == d_p || bk.psrc_a == d_pp || c->h > kMaxFastHalfOrder || c->use_generic))
        return fail(FDW_EINVAL, "step: BACK needs the older source field as a fourth, distinct buffer and an order <= 8");
    if (mode < FDW_MODE_FWD || mode > FDW_MODE_BACK) return fail(FDW_EINVAL, "step: unknown mode %d", mode);
    const int mode_dialect = mode == FDW_MODE_MOD ? FDW_DIALECT_MOD : ((mode == FDW_MODE_DD_FWD || mode == FDW_MODE_DD_RECV) ? FDW_DIALECT_RTM_STORED : FDW_DIALECT_RTM);
    if (mode_dialect != c->prm.dialect)
        return fail(FDW_ESTATE, "step: mode %d does not belong to this context's dialect %d", mode, c->prm.dialect);
    if (r0 < 0 || r1 > c->nxl || r0 > r1) return fail(FDW_EINVAL, "step: rows [%d,%d) outside the slab (%d rows)", r0, r1, c->nxl);
    // f.out (the new field stored somewhere else than over pp) is honoured by the register-ring kernel's DD_FWD instantiation only -- the one
    // caller, fdw_rtm_stored_shot, whose store slots are zero-filled so that cells the kernel never stores equal what an in-place update
    // would have left there.  Anything else would silently update in place: refuse.
    if (f.out && (mode != FDW_MODE_DD_FWD || c->h > kMaxFastHalfOrder || c->use_generic || f.out == d_p || f.out == d_pp))
        return fail(FDW_EINVAL, "step: a separate output array is supported by the DD_FWD register-ring kernel only, and must not alias the inputs");

    StepArgs a{};
    fill_common(c, a, d_p, d_pp, d_v2, pp_twice);
    a.psrc = bk.psrc_a; a.img = bk.img; a.fpp = bk.fpp;
    a.out = f.out;            // NULL: in place over pp
    a.gcx = c->d_gcx; a.gcz = c->d_gcz;
    a.r0 = r0;
    a.r1 = lap ? r1 : std::min(r1, c->upd_x1);   // rows >= xlim are never time-stepped (R:83-87)
    if (lap) {                // the stencil program rounds its grid up to 32 (S:231-238): whole interior
        a.lap_x0 = c->slap_x0; a.lap_x1 = c->slap_x1; a.lap_z0 = c->slap_z0; a.lap_z1 = c->slap_z1;
    }
    Injection in;
    FDW_TRY(place_injection(c, "step", mode, f, &in));
    if (mode == FDW_MODE_MOD) FDW_TRY(fill_mod(c, a, "step", f.rec, f.gz));
    // (a batch accumulates per shot, illum + shot * field, inside fdw_shot_batch_illum only)
    if (f.illum && (mode != FDW_MODE_FWD || (c->nbatch > 1 && !c->batch_illum)))
        return fail(FDW_EINVAL, "step: illumination belongs to a forward step of one shot");
    // the maps ride a point-source step, the pick a line-source step; neither is built together with recording or illumination.  A batch
    // (fdw_shot_excitation_batch): the one-step ring kernels only, amp / exc and the time map [shot] fields like the others
    const FwdVariant v = fwd_variant(mode, f);
    if (f.exc != Exc::none && (v.kmode < 0 || mode != FDW_MODE_FWD || !f.exc_arr || !f.texc || (c->nbatch > 1 && (c->h > kMaxFastHalfOrder || c->use_generic))))
        return fail(FDW_EINVAL, "step: the excitation maps belong to a plain forward step, the pick to a plain line-source step (a batch: orders <= 8)");
    // the RTM forward step that records its trace row, that accumulates the source illumination, or both
    fill_forward(c, a, v, f);
    a.inj = f.samples + in.shift; a.inj_x = in.x; a.inj_z = f.sz; a.inj_n = in.n;
    if (a.r1 <= a.r0) return FDW_OK;
    if (c->nbatch > 1) {      // fdw_shot_batch: shot b = these pointers + b fields, its own gather, its own source row
        a.nbatch = c->nbatch;
        a.bstride = (long long)field_elems(c);
        // the wavelet is shared, its row moves; receivers and line sources (fdw_shot_line_batch): a gather each, the rows the same
        const bool one_source = (mode == FDW_MODE_FWD && !f.line) || mode == FDW_MODE_MOD;
        a.inj_bstride = one_source ? 0 : (long long)c->nx * (f.line ? c->batch_nt : c->prm.nt);
        a.inj_dx = one_source ? c->batch_dsx : 0;
        a.v2_bstride = mode == FDW_MODE_MOD ? 0 : a.bstride;                       // mod_main models every shot on one velocity model (M:140-174)
        a.rec_bstride = (long long)c->nx * c->batch_nt;
    }
    // DTT imaging: a receiver step that leaves the image alone is the line-source step on the receiver rows (damping, leap-frog, one sample
    // per row after it: the same instantiation, the same bytes in pp); the fused iteration has a mode of its own, which images on C only
    const int kmode = bk.no_img ? FDW_MODE_FWD_LINE : (bk.dtt ? FDW_MODE_BACK_DTT : v.kmode);
    if (bk.dtt) {
        const BornCells C = born_cells(c);
        a.rec_x0 = C.x0; a.rec_n = std::max(0, C.x1 - C.x0);
        a.img_z1 = C.z1; a.exc_key = born_key(0, C.z0);
    }
    hipError_t e;
    if (c->h <= kMaxFastHalfOrder && !c->use_generic) {
        fill_geometry(c, a, a.r1 - a.r0, std::max(c->nbatch, 1));
        e = launch_step_fast(a, c->h, kmode, effective_prefetch(c), s);
    } else {
        if (mode >= FDW_MODE_MOD) return fail(FDW_EINVAL, "step: mode %d has no generic-order kernel", mode);
        // no generic-order illumination kernel: the plain step, then illum += pp (*) pp over the cells it updated
        // (recording too: the generic recording step, then the same add)
        e = launch_step_generic(a, c->h, bk.no_img ? FDW_MODE_FWD_LINE : v.generic, s);
        if (e == hipSuccess && v.illum) e = launch_illum_add(d_pp, f.illum, c->pitch, a.r0, a.r1, c->upd_z1, s);
        // no generic-order excitation kernel either: the plain step, then the compare-and-select / the pick over the cells it updated
        if (e == hipSuccess && f.exc != Exc::none)
            e = f.exc == Exc::pick ? launch_exc_pick(d_pp, f.texc, f.exc_arr, c->pitch, a.r0, a.r1, c->upd_z1, f.exc_key, s)
                                   : launch_exc_select(d_pp, f.exc_arr, f.texc, c->pitch, a.r0, a.r1, c->upd_z1, f.exc_key, s);
    }
    if (e != hipSuccess) return fail(FDW_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    if ((mode == FDW_MODE_RECV || mode == FDW_MODE_BACK) && r1 > c->upd_x1)      // (DTT imaging: no static row lies in C -- the injection alone, an empty column range)
        return static_receiver_rows(c, a.inj_x, a.inj_n, std::min(r1, c->nxl), d_pp, a.inj, mode == FDW_MODE_BACK ? bk.fpp : bk.psrc_a, bk.img, f.sz,
                                    (bk.no_img || bk.dtt) ? c->prm.nzb : a.img_z1, s);
    return FDW_OK;
}

extern "C" int fdw_dev_step(fdw_ctx* c, int mode, const float* d_p, float* d_pp, const float* d_v2, int r0, int r1,
                            int pp_twice, const float* d_inj, int inj_x, int inj_z, const float* d_psrc, float* d_img,
                            void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (mode == FDW_MODE_LAP) return fail(FDW_EINVAL, "use fdw_dev_laplacian for mode 3");
    const Forward f = point_source(d_inj, inj_x, inj_z);      // d_inj is the source's sample in the forward modes, the receivers' in the others
    BackExtra bk;
    bk.psrc_a = d_psrc; bk.img = d_img;
    return step_impl(c, mode, d_p, d_pp, d_v2, r0, r1, pp_twice, view_at(f, 0, c->nx), bk, pick_stream(c, stream));
}

// One iteration of fd_back's loop (R:302-339) on rows [r0, r1) of the slab, on caller-owned device arrays.
static int back_iter(fdw_ctx* c, int step_source, const float* d_f1, float* d_f0, const float* d_pr, float* d_ppr, const float* d_v2, int r0, int r1,
                     int pp_twice, const float* d_samples, int gz, float* d_img, hipStream_t s)
{
    const FwdView rs = receiver_samples(d_samples, gz);
    BackExtra bk;
    bk.psrc_a = d_f1; bk.img = d_img;
    if (!step_source)      // iterations 0 and 1: the source field is a snapshot as it stands (R:304-314)
        return step_impl(c, FDW_MODE_RECV, d_pr, d_ppr, d_v2, r0, r1, pp_twice, rs, bk, s);
    // the whole iteration in ONE pass: the source field is stepped in place (F_k overwrites F_{k-2}) in the same kernel that steps the
    // receiver field, and meets the new receiver row in registers for the imaging condition
    if (c->h <= kMaxFastHalfOrder && !c->use_generic && !c->no_fused_back) {
        bk.fpp = d_f0;
        return step_impl(c, FDW_MODE_BACK, d_pr, d_ppr, d_v2, r0, r1, pp_twice, rs, bk, s);
    }
    FDW_TRY(step_impl(c, FDW_MODE_PLAIN, d_f1, d_f0, d_v2, r0, r1, 0, FwdView{}, BackExtra{}, s));      // F_k overwrites F_{k-2} (R:317-318)
    bk.psrc_a = d_f0;
    return step_impl(c, FDW_MODE_RECV, d_pr, d_ppr, d_v2, r0, r1, pp_twice, rs, bk, s);
}

extern "C" int fdw_dev_back_iter(fdw_ctx* c, int step_source, const float* d_f1, float* d_f0, const float* d_pr, float* d_ppr, const float* d_v2,
                                 int r0, int r1, int pp_twice, const float* d_samples, int gz, float* d_img, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (c->prm.dialect != FDW_DIALECT_RTM) return fail(FDW_ESTATE, "fdw_dev_back_iter belongs to the RTM dialect");
    if (!d_f1 || !d_pr || !d_ppr || !d_v2 || !d_samples || !d_img || (step_source && !d_f0)) return fail(FDW_EINVAL, "back_iter: NULL buffer");
    return back_iter(c, step_source, d_f1, d_f0, d_pr, d_ppr, d_v2, r0, r1, pp_twice, d_samples, gz, d_img, pick_stream(c, stream));
}

// ---- second-time-difference imaging (definitions in fdwave.h, "DTT imaging") ----
static bool dtt_fused(const fdw_ctx* c) { return c->h <= kMaxFastHalfOrder && !c->use_generic && !c->no_fused_back; }

// one term on C: img = img (+) ((a (-) b) (-) (b (-) c)) (*) r; pre: a holds a (-) b already.  Inside a batch: every shot.
static int dtt_image(fdw_ctx* c, const float* d_a, const float* d_b, const float* d_c, const float* d_r, float* d_img, int pre, hipStream_t s)
{
    const BornCells C = born_cells(c);
    hipError_t e = launch_dtt_image(d_a, d_b, d_c, d_r, d_img, pre, c->pitch, C.x0, C.x1, C.z0, C.z1, c->nbatch, (long long)field_elems(c), s);
    if (e != hipSuccess) return fail(FDW_EHIP, "DTT image launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

// the scratch field of the unfused arrangement: every word read is written first (no memset, nothing to wait for)
static int ensure_dtt_scratch(fdw_ctx* c)
{
    if (dtt_fused(c) || c->d_dtt_w) return FDW_OK;
    hipError_t e = hipMalloc((void**)&c->d_dtt_w, field_elems(c) * sizeof(float));
    if (e != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc(%zu bytes) failed: %s", field_elems(c) * sizeof(float), hipGetErrorString(e));
    return FDW_OK;
}

// One iteration of the DTT backward loop: back_iter's fields, the image term q_{i-2} (*) r^{i-1} in place of the cross-correlation
// (step_source != 0), no image at all in iterations 0 and 1.
static int back_iter_dtt(fdw_ctx* c, int step_source, const float* d_f1, float* d_f0, const float* d_pr, float* d_ppr, const float* d_v2, int r0, int r1,
                         int pp_twice, const float* d_samples, int gz, float* d_img, hipStream_t s)
{
    const FwdView rs = receiver_samples(d_samples, gz);
    BackExtra bk;
    if (!step_source) {
        bk.no_img = true;
        return step_impl(c, FDW_MODE_RECV, d_pr, d_ppr, d_v2, r0, r1, pp_twice, rs, bk, s);
    }
    if (dtt_fused(c)) {
        bk.psrc_a = d_f1; bk.img = d_img; bk.fpp = d_f0; bk.dtt = true;
        return step_impl(c, FDW_MODE_BACK, d_pr, d_ppr, d_v2, r0, r1, pp_twice, rs, bk, s);
    }
    // in four launches: the first difference while F_{i-2} still stands, the source step over it, the term while d_ppr still holds r^{i-1},
    // the receiver step
    FDW_TRY(ensure_dtt_scratch(c));
    const BornCells C = born_cells(c);
    hipError_t e = launch_born_diff(d_f0, d_f1, c->d_dtt_w, c->pitch, C.x0, C.x1, C.z0, C.z1, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "DTT difference launch failed: %s", hipGetErrorString(e));
    FDW_TRY(step_impl(c, FDW_MODE_PLAIN, d_f1, d_f0, d_v2, r0, r1, 0, FwdView{}, BackExtra{}, s));
    FDW_TRY(dtt_image(c, c->d_dtt_w, d_f1, d_f0, d_ppr, d_img, 1, s));
    bk.no_img = true;
    return step_impl(c, FDW_MODE_RECV, d_pr, d_ppr, d_v2, r0, r1, pp_twice, rs, bk, s);
}

// what the two device entry points refuse before anything is enqueued
static int check_dtt_ctx(const fdw_ctx* c, const char* who)
{
    if (c->prm.dialect != FDW_DIALECT_RTM) return fail(FDW_ESTATE, "%s: DTT imaging belongs to the RTM dialect (the sibling's dialects do not combine with it)", who);
    if (!is_full_grid(c)) return fail(FDW_ESTATE, "%s: DTT imaging: full-grid contexts only (slab contexts do not combine with it)", who);
    if (c->nbatch > 1) return fail(FDW_ESTATE, "%s: not inside a batch of shots", who);
    return FDW_OK;
}

extern "C" int fdw_dev_back_iter_dtt(fdw_ctx* c, int step_source, const float* d_f1, float* d_f0, const float* d_pr, float* d_ppr, const float* d_v2,
                                     int r0, int r1, int pp_twice, const float* d_samples, int gz, float* d_img, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_dtt_ctx(c, "fdw_dev_back_iter_dtt"));
    if (!d_f1 || !d_pr || !d_ppr || !d_v2 || !d_samples || !d_img || (step_source && !d_f0)) return fail(FDW_EINVAL, "fdw_dev_back_iter_dtt: NULL buffer");
    if (step_source && (d_f0 == d_f1 || d_f0 == d_pr || d_f0 == d_ppr || d_f1 == d_ppr || d_img == d_f0 || d_img == d_ppr))
        return fail(FDW_EINVAL, "fdw_dev_back_iter_dtt: the source pair, the receiver pair and the image are distinct arrays");
    if (r0 != 0 || r1 != c->nxl) return fail(FDW_EINVAL, "fdw_dev_back_iter_dtt: rows [%d,%d) are not the whole grid [0,%d)", r0, r1, c->nxl);
    if (gz < 0 || gz >= c->prm.nze) return fail(FDW_EINVAL, "fdw_dev_back_iter_dtt: receiver depth %d outside the grid", gz);
    HIP_TRY(hipSetDevice(c->device));
    if (step_source) FDW_TRY(ensure_dtt_scratch(c));
    return back_iter_dtt(c, step_source, d_f1, d_f0, d_pr, d_ppr, d_v2, r0, r1, pp_twice, d_samples, gz, d_img, pick_stream(c, stream));
}

extern "C" int fdw_dev_dtt_image(fdw_ctx* c, const float* d_fa, const float* d_fb, const float* d_fc, const float* d_r, float* d_img, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_dtt_ctx(c, "fdw_dev_dtt_image"));
    if (!d_fa || !d_fb || !d_fc || !d_r || !d_img) return fail(FDW_EINVAL, "fdw_dev_dtt_image: NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    return dtt_image(c, d_fa, d_fb, d_fc, d_r, d_img, 0, pick_stream(c, stream));
}

// ---- subsurface-offset image gathers (definitions in fdwave.h, "Extended imaging") ----
// one term on C: plane h + H of d_eimg += f[x-h] (*) r[x+h], h = -H .. H
static int ext_image(fdw_ctx* c, const float* d_f, const float* d_r, int H, float* d_eimg, hipStream_t s)
{
    const BornCells C = born_cells(c);
    hipError_t e = launch_ext_image(d_f, d_r, d_eimg, H, c->pitch, field_elems(c), C.x0, C.x1, C.z0, C.z1, c->xchunk, c->ext_pointwise != 0, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "extended image launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

static int check_ext_ctx(const fdw_ctx* c, const char* who, int H)
{
    if (c->prm.dialect != FDW_DIALECT_RTM) return fail(FDW_ESTATE, "%s: extended imaging belongs to the RTM dialect (the sibling's dialects do not combine with it)", who);
    if (!is_full_grid(c)) return fail(FDW_ESTATE, "%s: extended imaging: full-grid contexts only (slab contexts do not combine with it)", who);
    if (c->nbatch > 1) return fail(FDW_ESTATE, "%s: not inside a batch of shots", who);
    if (H < 0 || H > FDW_EXT_HMAX) return fail(FDW_EINVAL, "%s: H=%d outside [0,%d]", who, H, FDW_EXT_HMAX);
    return FDW_OK;
}

extern "C" int fdw_dev_ext_image(fdw_ctx* c, const float* d_f, const float* d_r, int H, float* d_eimg, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_ext_ctx(c, "fdw_dev_ext_image", H));
    if (!d_f || !d_r || !d_eimg) return fail(FDW_EINVAL, "fdw_dev_ext_image: NULL buffer");
    const uintptr_t fb = fdw_field_bytes(c), e0 = (uintptr_t)d_eimg, e1 = e0 + (uintptr_t)(2 * H + 1) * fb;
    for (const float* in : {d_f, d_r})
        if ((uintptr_t)in < e1 && (uintptr_t)in + fb > e0) return fail(FDW_EINVAL, "fdw_dev_ext_image: the planes of d_eimg overlap an input field");
    HIP_TRY(hipSetDevice(c->device));
    return ext_image(c, d_f, d_r, H, d_eimg, pick_stream(c, stream));
}

extern "C" int fdw_dev_laplacian(fdw_ctx* c, const float* d_p, float* d_lap, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    return step_impl(c, FDW_MODE_LAP, d_p, d_lap, nullptr, 0, c->nxl, 0, FwdView{}, BackExtra{}, pick_stream(c, stream));
}

// ---- two time steps per pass (temporal blocking) --------------------------------------------------
// The two-step kernel wins where a launch is bandwidth bound (>= 8192^2: +18 %, 16384^2: +47 %); on small decks a
// launch is a latency chain and the longer march loses (new_mod: 12 vs 5 us/step), so the one-step kernel stays.
// Auto-selection threshold of the wave-pipeline kernel, in strip rows (rows x strips of 56 cells).  Measured (scripts/probe_sizes.py,
// probe_slabsize.py): 2048^2 (20k) one-step 280 vs pipeline 253 Gpt/s; 1056x8192 (39k) 312 vs 371; 4096^2 (78k) 337 (two-step 360) vs 452.
constexpr long kPipeAutoStripRows = 30000;
static bool two_step_pays(const fdw_ctx* c)
{
    if (c->h != kMaxFastHalfOrder || c->use_generic || c->tb < 0 || c->prm.dialect != FDW_DIALECT_RTM) return false;
    if (c->tb > 0) return true;
    return (long)c->upd_x1 * ((c->pitch / 4 + 59) / 60) >= 200000;
}

// The end of a pass of an even number of steps (step2_impl, stepn_impl).  Rows the reference never time-steps (compat, nxe not a multiple
// of 8) are static in both fields, which swap roles every step: out1 now carries pp's rows, out2 p's; so do the levels in between
// (PLAIN_ALL: level 0 pp's, level 1 p's) and the receiver field of BACK4.  Receiver rows among them (two-step RECV): iteration it injects
// into (and images) what is now out1, iteration it+1 what is now out2.
// rr: the rows the call was asked for.  A pass on row ranges copies the static rows AMONG them and no others -- none of a gap between the
// two ranges, and those of a range that holds no time-stepped row at all.
struct RowRanges {      // rows the pass produces: [r0, r1) and optionally [r0b, r1b); r1 < 0 = all rows the reference time-steps
    int r0 = 0, r1 = -1, r0b = 0, r1b = 0, xchunk = 0;
};
static int even_steps_tail(fdw_ctx* c, int mode, const Step2Args& a, const RowRanges& rr, hipStream_t s)
{
    const bool whole = rr.r1 < 0;
    const int span[2][2] = {{whole ? 0 : rr.r0, whole ? INT_MAX : rr.r1}, {whole ? 0 : rr.r0b, whole ? 0 : rr.r1b}};
    for (const auto& sp : span) {
        const int x0 = std::max(sp[0], c->upd_x1), x1 = std::min(sp[1], c->nxl);
        if (x1 <= x0) continue;
        const size_t off = (size_t)x0 * c->pitch, n = (size_t)(x1 - x0) * c->pitch * sizeof(float);
        auto pair = [&](float* o1, float* o2, const float* p, const float* pp) -> int {
            HIP_TRY(hipMemcpyAsync(o1 + off, pp + off, n, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(o2 + off, p + off, n, hipMemcpyDeviceToDevice, s));
            return FDW_OK;
        };
        FDW_TRY(pair(a.out1, a.out2, a.p, a.pp));
        if (mode == FDW_MODE_PLAIN_ALL) FDW_TRY(pair(a.lvl0, a.lvl1, a.p, a.pp));
        if (mode == FDW_MODE_BACK4) FDW_TRY(pair(a.rout1, a.rout2, a.rp, a.rpp));
    }
    // (the pipeline's receiver passes, inj2 = NULL, run only where every receiver row is time-stepped: fdw_receivers_stepped)
    if (mode != FDW_MODE_RECV || !a.inj2) return FDW_OK;
    FDW_TRY(static_receiver_rows(c, a.inj_x, a.inj_n, c->nxl, a.out1, a.inj, a.psrc_a, a.img, a.inj_z, a.img_z1, s));
    return static_receiver_rows(c, a.inj_x, a.inj_n, c->nxl, a.out2, a.inj2, a.psrc_b, a.img, a.inj_z, a.img_z1, s);
}


// mode FWD: f (a view) -> f.samples = {srce[it], srce[it+1]} at (f.sx, f.sz) (f.sx < 0: none), or the line samples of both steps; f.rec: the
//   trace rows of both steps, rec and rec + nx; f.illum: their squares added to the illumination
// mode PLAIN: no taper, no injection
// mode RECV: f.samples / ex.inj2 -> receiver samples of iterations it / it+1 (nx each), f.sz = gz, imaging with ex.psrc_a/b
static int step2_impl(fdw_ctx* c, int mode, const float* d_p, const float* d_pp, const float* d_v2, float* d_out1, float* d_out2, int pp_twice,
                      const FwdView& f, const BackExtra& ex, hipStream_t s)
{
    if (c->h != kMaxFastHalfOrder) return fail(FDW_EINVAL, "step2: the two-step kernel is built for order 8 only");
    if (!d_p || !d_pp || !d_v2 || !d_out1 || !d_out2) return fail(FDW_EINVAL, "step2: NULL buffer");
    if (d_out1 == d_p || d_out1 == d_pp || d_out2 == d_p || d_out2 == d_pp || d_out1 == d_out2)
        return fail(FDW_EINVAL, "step2: outputs must not alias the inputs (tiles re-read each other's input rows)");
    Step2Args a{};
    fill_common(c, a, d_p, d_pp, d_v2, pp_twice);
    a.out1 = d_out1; a.out2 = d_out2;
    a.psrc_a = ex.psrc_a; a.psrc_b = ex.psrc_b; a.img = ex.img;
    a.r0 = 0; a.r1 = c->upd_x1;
    if (mode == FDW_MODE_RECV && (!f.samples || !ex.inj2 || !ex.psrc_a || !ex.psrc_b || !ex.img))
        return fail(FDW_EINVAL, "step2: RECV needs both sample rows, both source fields and the image");
    Injection in;
    FDW_TRY(place_injection(c, "step2", mode, f, &in));
    a.inj = f.samples + in.shift; a.inj2 = f.line ? f.samples + c->nx : ex.inj2 + in.shift; a.inj_x = in.x; a.inj_z = f.sz; a.inj_n = in.n;
    const int ncells = c->pitch / 4;
    a.nstrip = (ncells + 59) / 60;
    a.nzblk = (a.nstrip + 3) / 4;
    const int rows = a.r1 - a.r0;
    if (rows <= 0) return FDW_OK;
    // whole ring turns only (the march is branch-free, a partial turn still costs a full one): xchunk + 2H = 10k.
    // Measured (scripts/probe_tb.py / probe_slabsize.py, noise-filled fields, same-box A/B; +-5 % between boxes): 16384^2 449 Gpt/s
    // at 42 (443 at 22, 444 at 72); 8192^2 442 at 32 (435 at 22, 408 at 42); 4128x8192 416-423 at 32; 2080x8192 375 at 32;
    // 1056x8192 301 at 22 (267 at 32: too few waves).
    const long strip_rows = (long)rows * a.nstrip;
    int xchunk = c->xchunk2 > 0 ? c->xchunk2 : (strip_rows >= 1000000 ? 42 : (strip_rows >= 70000 ? 32 : (strip_rows >= 16384 ? 22 : 2)));
    a.xchunk = xchunk;
    const int chunks = (rows + xchunk - 1) / xchunk;
    a.nblk = a.nzblk * chunks;
    a.nper = (a.nblk + 7) / 8;
    const FwdVariant v = fwd_variant(mode, f);
    if ((f.illum && mode != FDW_MODE_FWD) || v.kmode < 0 || !family_serves(2, v))
        return fail(FDW_EINVAL, "step2: illumination belongs to a forward pass, and no two-step kernel is built for this combination of extras");
    fill_forward(c, a, v, f);
    hipError_t e = launch_step2(a, c->h, v.kmode, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "step2 launch failed: %s", hipGetErrorString(e));
    return even_steps_tail(c, mode, a, RowRanges{}, s);
}

// ---- kPipeSteps time steps per pass (wave pipeline through LDS) -------------------------------------
static bool pipe_pays(const fdw_ctx* c)
{
    if (c->h != kMaxFastHalfOrder || c->use_generic || c->tb < 0 || c->prm.dialect == FDW_DIALECT_RTM_STORED) return false;
    if ((size_t)c->nxl * c->pitch * sizeof(float) >= (1ull << 31)) return false;   // the kernel addresses a field through one 2 GiB buffer descriptor
    if (c->tb == kPipeSteps) return true;
    if (c->tb > 0) return false;                                   // two-step forced
    return (long)c->upd_x1 * ((c->pitch / 4 + 55) / 56) >= kPipeAutoStripRows;
}

// FWD: f.samples -> kPipeSteps source samples srce[it .. it+kPipeSteps-1]; PLAIN: no taper, no injection.
// d_out1 = u^{n+kPipeSteps-1}, d_out2 = u^{n+kPipeSteps}.
struct StepnBack {      // the passes of the backward loop (Step2Args: lvl0, lvl1, plev, img, inj_stride, rp ...)
    float *lvl0 = nullptr, *lvl1 = nullptr;       // PLAIN_ALL: where waves 0 and 1 store their levels
    const float* plev[kPipeSteps] = {};           // RECV: the source field of iterations it .. it+3
    float* img = nullptr;
    int inj_stride = 0;                           // RECV, BACK4: floats between the sample rows of consecutive iterations
    const float *rp = nullptr, *rpp = nullptr;    // BACK4: the receiver pair (the positional arguments are the source field's)
    float *rout1 = nullptr, *rout2 = nullptr;
};
// cls[L] of every tile of a FWD / PLAIN launch of fdw_stepn_kernel, in the tile order L = chunk row * nstrip + strip: 0 = it runs the lean body,
// 1 = the full body, by the placement the kernels expand and the predicate they pick the body with (FDW_PIPE_TILE_ROWS, pipe_tile_lean: fdw_kernels.h)
static void tile_classes(const Step2Args& a, const FwdVariant& v, std::vector<unsigned char>& cls)
{
    constexpr int H = kMaxFastHalfOrder, NS = kPipeSteps;
    cls.resize((size_t)a.nblk);
    for (int L = 0; L < a.nblk; L++) {
        FDW_PIPE_TILE_ROWS(a, L, zb, xa, xe)
        const int cs = FDW_PIPE_TILE_CELL(zb, NS);
        const bool lean = v.kmode == FDW_MODE_PLAIN ? pipe_tile_lean<H, NS, false, 0>(a, cs, xa, xe)
                          : (v.line && v.rec)       ? pipe_tile_lean<H, NS, true, 2, false, true>(a, cs, xa, xe)
                          : v.line                  ? pipe_tile_lean<H, NS, true, 2>(a, cs, xa, xe)
                                                    : pipe_tile_lean<H, NS, true, 1>(a, cs, xa, xe);
        cls[(size_t)L] = lean ? 0 : 1;
    }
}

// strips of a pipeline pass (each owns 64 - 2 kPipeSteps columns of 4 cells) and the chunk length of its forward passes on `strip_rows` =
// rows x strips (the measurements are in stepn_impl)
static int pipe_strips(const fdw_ctx* c)
{
    const int ncells = c->pitch / 4, own = 64 - 2 * kPipeSteps;
    return (ncells + own - 1) / own;
}
// `moving_cut`: the passes run as two bands with a moving cut (steps_loop).  Its two resident units together are one whole pass, so the
// 8192^2 class need not keep its pass above the 1280 workgroup slots and takes a longer chunk, 213 rows for 27 rows of run-in (8192^2,
// Gpoints/s, profiles/r21_ab_bench.txt, session 3: 173 rows 737 - 747, 213 rows 751 - 755, 253 rows 750 - 752; session 4, FAST: 213 rows
// 877 - 879, 253 rows 853 - 857); the classes below it keep their chunk lengths (4096^2 and 6144^2 were measured at those; 6144^2 at 173
// rows 698 - 699 against 706 - 709 at 143).
static int pipe_fwd_xchunk(const fdw_ctx* c, long strip_rows, bool moving_cut = false)
{
    const bool fastnum = c->prm.numerics == FDW_NUMERICS_FAST;
    if (c->xchunk2 <= 0) {
        if (const char* e = getenv("FDW_FWD_XCHUNK")) if (atoi(e) > 0) return atoi(e);      // experiments
        if (moving_cut && strip_rows >= 250000 && strip_rows < 1000000) return 213;
    }
    return c->xchunk2 > 0 ? c->xchunk2 : (strip_rows >= 1000000 ? 253 : (strip_rows >= 250000 ? 173 : (strip_rows >= 120000 ? (fastnum ? 173 : 143) : (strip_rows >= 60000 ? 83 : 43))));
}

struct StepnPlan {
    int nblk = 0, nstrip = 0;
    std::vector<unsigned char> cls;
};
static thread_local StepnPlan* g_plan = nullptr;

static int stepn_impl(fdw_ctx* c, int mode, const float* d_p, const float* d_pp, const float* d_v2, float* d_out1, float* d_out2, int pp_twice,
                      const FwdView& f, const StepnBack& bk, const RowRanges& rr, hipStream_t s)
{
    const bool recv = mode == FDW_MODE_RECV || mode == FDW_MODE_BACK4;
    if (c->h != kMaxFastHalfOrder) return fail(FDW_EINVAL, "stepn: the pipelined kernel is built for order 8 only");
    if (mode != FDW_MODE_FWD && mode != FDW_MODE_PLAIN && mode != FDW_MODE_MOD && mode != FDW_MODE_PLAIN_ALL && mode != FDW_MODE_RECV && mode != FDW_MODE_BACK4)
        return fail(FDW_EINVAL, "stepn: FWD, PLAIN, PLAIN_ALL, RECV, BACK4 or MOD only");
    if (mode == FDW_MODE_BACK4) {
        if (!bk.img || !f.samples || !bk.rp || !bk.rpp || !bk.rout1 || !bk.rout2) return fail(FDW_EINVAL, "stepn: BACK4 needs the receiver pair, its outputs, samples and image");
        const float* all[8] = {d_p, d_pp, d_out1, d_out2, bk.rp, bk.rpp, bk.rout1, bk.rout2};
        for (int i = 0; i < 8; i++)
            for (int j = i + 1; j < 8; j++)
                if (all[i] == all[j]) return fail(FDW_EINVAL, "stepn: BACK4 buffers must not alias");
    }
    if ((mode == FDW_MODE_PLAIN_ALL && (!bk.lvl0 || !bk.lvl1)) ||
        (mode == FDW_MODE_RECV && (!bk.img || !f.samples || !bk.plev[0] || !bk.plev[1] || !bk.plev[2] || !bk.plev[3])))
        return fail(FDW_EINVAL, "stepn: the backward passes need their level buffers / source fields, samples and image");
    if ((mode == FDW_MODE_MOD) != (c->prm.dialect == FDW_DIALECT_MOD)) return fail(FDW_ESTATE, "stepn: mode %d does not belong to dialect %d", mode, c->prm.dialect);
    if (!d_p || !d_pp || !d_v2 || !d_out1 || !d_out2) return fail(FDW_EINVAL, "stepn: NULL buffer");
    if (d_out1 == d_p || d_out1 == d_pp || d_out2 == d_p || d_out2 == d_pp || d_out1 == d_out2)
        return fail(FDW_EINVAL, "stepn: outputs must not alias the inputs (tiles re-read each other's input rows)");
    Step2Args a{};
    fill_common(c, a, d_p, d_pp, d_v2, pp_twice);
    a.out1 = d_out1; a.out2 = d_out2;
    const bool whole = rr.r1 < 0;
    if (!whole && (rr.r0 < 0 || rr.r1 > c->nxl || rr.r0b < 0 || rr.r1b > c->nxl || (rr.r1b > rr.r0b && rr.r0b < rr.r1)))
        return fail(FDW_EINVAL, "stepn: row ranges [%d,%d) [%d,%d) outside the slab or overlapping", rr.r0, rr.r1, rr.r0b, rr.r1b);
    a.r0 = whole ? 0 : rr.r0; a.r1 = std::min(whole ? c->upd_x1 : rr.r1, c->upd_x1);
    a.r0b = whole ? 0 : rr.r0b; a.r1b = whole ? 0 : std::min(rr.r1b, c->upd_x1);
    {   // columns without a damping factor (taper_apply's table is 1.0f between the two strips; the RTM dialects damp the top strip only)
        const bool four_sided = c->prm.dialect == FDW_DIALECT_MOD;
        a.zt_lo = four_sided ? c->prm.nzb : c->ztap;
        a.zt_hi = four_sided ? c->prm.nze - c->prm.nzb : -1;
    }
    Injection in;
    FDW_TRY(place_injection(c, "stepn", mode, f, &in));
    if (f.line) a.inj_stride = c->nx;
    if (mode == FDW_MODE_PLAIN_ALL) {
        a.lvl0 = bk.lvl0; a.lvl1 = bk.lvl1;
        for (float* o : {d_out1, d_out2}) if (bk.lvl0 == o || bk.lvl1 == o || bk.lvl0 == bk.lvl1 || bk.lvl0 == d_p || bk.lvl0 == d_pp || bk.lvl1 == d_p || bk.lvl1 == d_pp)
            return fail(FDW_EINVAL, "stepn: level buffers must not alias the inputs or outputs");
    }
    if (mode == FDW_MODE_BACK4) {
        a.rp = bk.rp; a.rpp = bk.rpp; a.rout1 = bk.rout1; a.rout2 = bk.rout2;
    }
    if (recv) {
        a.inj_stride = bk.inj_stride;
        a.img = bk.img;
        for (int i = 0; i < kPipeSteps; i++) a.plev[i] = bk.plev[i];
    }
    if (mode == FDW_MODE_MOD) FDW_TRY(fill_mod(c, a, "stepn", f.rec, f.gz));
    if (f.illum && mode != FDW_MODE_FWD) return fail(FDW_EINVAL, "stepn: illumination belongs to a forward pass");
    // the excitation maps of a point-source pass / the pick of a line-source pass; f.exc_key belongs to the pass's first step
    const FwdVariant v = fwd_variant(mode, f);
    if (f.exc != Exc::none && (v.kmode < 0 || mode != FDW_MODE_FWD || !f.exc_arr || !f.texc))
        return fail(FDW_EINVAL, "stepn: the excitation maps belong to a plain forward pass, the pick to a plain line-source pass");
    // FWD with f.rec: the trace rows of the pass's four steps; with f.illum: their squares added to the illumination; with both: both
    fill_forward(c, a, v, f);
    a.inj = f.samples + in.shift; a.inj_x = in.x; a.inj_z = f.sz; a.inj_n = in.n;
    const int ncells = c->pitch / 4, own = 64 - 2 * kPipeSteps;
    a.nstrip = (ncells + own - 1) / own;
    a.nzblk = a.nstrip;
    const int rows_a = std::max(a.r1 - a.r0, 0), rows_b = std::max(a.r1b - a.r0b, 0), rows = rows_a + rows_b;
    static_assert(kPipeSteps % 2 == 0, "static-row bookkeeping assumes an even number of steps per pass");
    // (even_steps_tail: the static rows among the rows asked for)
    if (rows <= 0) return g_plan ? FDW_OK : even_steps_tail(c, mode, a, rr, s);      // no time-stepped row among them: nothing to launch
    // whole ring turns: xchunk + (NS-1)(2H+1) = 10k  ->  xchunk = 10k - 27 (13, 23, ... 83, 93, ...)
    const long strip_rows = (long)rows * a.nstrip;
    // measured: 16384^2 579 Gpt/s at 253 (560 at 173); 8192^2 566 at 173 (509 at 83, 553 at 253); 4096^2 452 at 83 (382 at 43, 388 at 173);
    // 1056x8192 371 at 43 (355 at 63, 340 at 33)
    // end of round 2 (scripts/probe_pipe.py, PIPE_SHAPE): 4128x8192 (half of the bench grid) 584 at 83, 592 at 123, 609 at 143, 601 at 173;
    // 2144x8192 538 at 83 (499 at 53, 521 at 103)
    // end of round 3 (same probe, FAST numerics): 4128x8192 677 at 143, 710 at 173, 700 at 83 -- the memory-bound FAST kernel prefers the longer chunk there
    int xchunk = pipe_fwd_xchunk(c, strip_rows);
    if (mode == FDW_MODE_BACK4 && c->xchunk2 <= 0) {
        // the eight-wave kernel holds two workgroups per CU (512 at a time): longer chunks than the forward kernel's at the same grid size
        // (scripts/probe_slabs_c.py, us per iteration by chunk length 43 / 83 / 123 / 173: 8192 rows 363 / 309 / 289 / 277; 4160 rows 192 / 172 / 157 / 162;
        //  2176 rows 109 / 94 / 102 / 93; 1152 rows 61 / 64 / 69 / 80)
        // end of round 2 (lean bodies, scripts/probe_back.py, 8192 rows, us per iteration): 93: 240, 103: 233, 123: 228, 133: 230, 143: 234, 153: 226,
        //  163: 234, 173: 234, 193: 233, 213: 225, 223: 231 -- 54 chunks x 37 strips fill the 512 workgroup slots 3.9 times over
        xchunk = strip_rows >= 250000 ? 153 : (strip_rows >= 120000 ? 123 : (strip_rows >= 60000 ? 83 : 43));
        if (const char* e = getenv("FDW_BACK4_XCHUNK")) xchunk = atoi(e) > 0 ? atoi(e) : xchunk;      // experiments
    }
    if (rr.xchunk > 0) xchunk = rr.xchunk;
    a.xchunk = xchunk;
    a.chunks_a = (rows_a + xchunk - 1) / xchunk;
    const int chunks = a.chunks_a + (rows_b + xchunk - 1) / xchunk;
    a.nblk = a.nstrip * chunks;
    a.nper = (a.nblk + 7) / 8;
    if (g_plan) {      // fdw_debug_step4_plan: the tiles of this launch and which of them run the lean body; nothing launched
        g_plan->nblk = a.nblk; g_plan->nstrip = a.nstrip;
        tile_classes(a, v, g_plan->cls);
        return FDW_OK;
    }
    hipError_t e = launch_stepn(a, c->h, v.kmode, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "stepn launch failed: %s", hipGetErrorString(e));
    return even_steps_tail(c, mode, a, rr, s);
}

int fdw_receivers_stepped(const fdw_ctx* c) { return c->prm.nxb + c->nx <= c->xlim; }

// FOUR iterations of fd_back's loop (R:317-329) through the wave pipeline on row ranges of the slab: source field f1, f0 -> fo1, fo2, receiver
// field pr, ppr -> ro1, ro2.  Fused (one pass of the eight-wave kernel, the levels in between never leave the chip) unless FDW_NO_BACK_FUSED:
// then PLAIN_ALL reconstructs F_it .. F_{it+3} into lvl0, lvl1, fo1, fo2 and a RECV pass advances the receiver field four times, injects each
// iteration's samples (rows sample_stride apart) and adds the four products F_{it+j} r^{it+j+1} to the image in iteration order.
static int back4(fdw_ctx* c, const float* d_f1, const float* d_f0, float* d_fo1, float* d_fo2, float* d_lvl0, float* d_lvl1, const float* d_pr,
                 const float* d_ppr, float* d_ro1, float* d_ro2, const float* d_v2, const float* d_samples, int sample_stride, int gz, float* d_img,
                 int pp_twice, const RowRanges& rr, hipStream_t s)
{
    if (!c->no_back_fused) {
        StepnBack b4;
        b4.rp = d_pr; b4.rpp = d_ppr; b4.rout1 = d_ro1; b4.rout2 = d_ro2; b4.img = d_img;
        b4.inj_stride = sample_stride;
        return stepn_impl(c, FDW_MODE_BACK4, d_f1, d_f0, d_v2, d_fo1, d_fo2, pp_twice, receiver_samples(d_samples, gz), b4, rr, s);
    }
    StepnBack fb;
    fb.lvl0 = d_lvl0; fb.lvl1 = d_lvl1;
    FDW_TRY(stepn_impl(c, FDW_MODE_PLAIN_ALL, d_f1, d_f0, d_v2, d_fo1, d_fo2, 0, FwdView{}, fb, rr, s));
    StepnBack rb;
    rb.plev[0] = d_lvl0; rb.plev[1] = d_lvl1; rb.plev[2] = d_fo1; rb.plev[3] = d_fo2;
    rb.img = d_img;
    rb.inj_stride = sample_stride;
    return stepn_impl(c, FDW_MODE_RECV, d_pr, d_ppr, d_v2, d_ro1, d_ro2, pp_twice, receiver_samples(d_samples, gz), rb, rr, s);
}

extern "C" int fdw_dev_back4(fdw_ctx* c, const float* d_f1, const float* d_f0, float* d_fo1, float* d_fo2, float* d_lvl0, float* d_lvl1, const float* d_pr,
                             const float* d_ppr, float* d_ro1, float* d_ro2, const float* d_v2, const float* d_samples, int sample_stride, int gz,
                             float* d_img, int pp_twice, int r0, int r1, int r0b, int r1b, int xchunk, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (c->prm.dialect != FDW_DIALECT_RTM || c->h != kMaxFastHalfOrder || (size_t)c->nxl * c->pitch * sizeof(float) >= (1ull << 31))
        return fail(FDW_EINVAL, "back4: needs the RTM dialect, order 8 and fields below 2 GiB");
    if (!fdw_receivers_stepped(c)) return fail(FDW_EINVAL, "back4: receiver rows beyond the time-stepped rows are not covered by the pipelined passes");
    return back4(c, d_f1, d_f0, d_fo1, d_fo2, d_lvl0, d_lvl1, d_pr, d_ppr, d_ro1, d_ro2, d_v2, d_samples, sample_stride, gz, d_img, pp_twice,
                 RowRanges{r0, r1, r0b, r1b, xchunk}, pick_stream(c, stream));
}

// the backward loop's tier (back_loop; fdw_slabs_create asks the same of every rank)
extern "C" int fdw_back_pipe_active(const fdw_ctx* c)
{
    return c && pipe_pays(c) && c->prm.dialect == FDW_DIALECT_RTM && fdw_receivers_stepped(c) && !c->no_back_pipe ? 1 : 0;
}

extern "C" int fdw_two_step_active(const fdw_ctx* c) { return c && two_step_pays(c) ? 1 : 0; }
extern "C" int fdw_steps_per_pass(const fdw_ctx* c) { return !c ? 0 : (pipe_pays(c) ? kPipeSteps : (two_step_pays(c) ? 2 : 1)); }

extern "C" int fdw_dev_step2(fdw_ctx* c, const float* d_p, const float* d_pp, const float* d_v2, float* d_out1, float* d_out2, int pp_twice,
                             const float* d_srce_it, int sx, int sz, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    return step2_impl(c, FDW_MODE_FWD, d_p, d_pp, d_v2, d_out1, d_out2, pp_twice, view_at(point_source(d_srce_it, sx, sz), 0, c->nx), BackExtra{}, pick_stream(c, stream));
}

// kPipeSteps (4) forward iterations in one pass of the wave-pipeline kernel on the given row ranges of a slab
extern "C" int fdw_dev_step4(fdw_ctx* c, const float* d_p, const float* d_pp, const float* d_v2, float* d_out1, float* d_out2, int pp_twice,
                             const float* d_srce_it, int sx, int sz, int r0, int r1, int r0b, int r1b, int xchunk, void* stream)
{
    // (fdw_dev_step4_rec without a gather is exactly this launch)
    return fdw_dev_step4_rec(c, d_p, d_pp, d_v2, d_out1, d_out2, pp_twice, d_srce_it, sx, sz, r0, r1, r0b, r1b, xchunk, nullptr, 0, (hipStream_t)stream);
}

// The tiles a pipeline pass on the rows rr would launch and their classes, through stepn_impl's plan hook.  Nothing is launched.
static float* const kPlanFake = reinterpret_cast<float*>(uintptr_t(1) << 20);      // never dereferenced: the plan hook returns before the launch
static int step4_plan(fdw_ctx* c, int mode, const Forward& f, const RowRanges& rr, int* nblk, int* nstrip, unsigned char* cls, int cls_cap)
{
    StepnPlan plan;
    g_plan = &plan;
    const int rc = stepn_impl(c, mode, kPlanFake, kPlanFake + 1, kPlanFake + 2, kPlanFake + 3, kPlanFake + 4, 1, view_at(f, 0, c->nx), StepnBack{}, rr, nullptr);
    g_plan = nullptr;
    if (rc != FDW_OK) return rc;
    *nblk = plan.nblk; *nstrip = plan.nstrip;
    if (cls) std::copy(plan.cls.begin(), plan.cls.begin() + std::min<size_t>(plan.cls.size(), (size_t)std::max(cls_cap, 0)), cls);
    return FDW_OK;
}

// Tests and probes: what fdw_dev_step4 (forward = 1: FWD with the source at (sx, sz), sx < 0 none; 0: PLAIN) would launch on these row ranges --
// tiles, strips and, per tile of the order L = chunk row * nstrip + strip, its class (0 lean, 1 full).  Launches nothing.
extern "C" int fdw_debug_step4_plan(fdw_ctx* c, int forward, int sx, int sz, int r0, int r1, int r0b, int r1b, int xchunk, int* nblk, int* nstrip,
                                    unsigned char* cls, int cls_cap)
{
    if (!c || !nblk || !nstrip) return fail(FDW_EINVAL, "NULL argument");
    if (c->h != kMaxFastHalfOrder) return fail(FDW_EINVAL, "step4: needs order 8");
    const Forward f = point_source(forward && sx >= 0 ? kPlanFake + 5 : nullptr, sx, sz);      // (no samples: no source)
    return step4_plan(c, forward ? FDW_MODE_FWD : FDW_MODE_PLAIN, f, RowRanges{r0, r1, r0b, r1b, xchunk}, nblk, nstrip, cls, cls_cap);
}

// The same for a pass of fdw_dev_line_steps (plain) with the line at depth sz: the tiles of the strip that holds the line run the full body.
extern "C" int fdw_debug_step4_plan_line(fdw_ctx* c, int sz, int r0, int r1, int r0b, int r1b, int xchunk, int* nblk, int* nstrip, unsigned char* cls,
                                         int cls_cap)
{
    if (!c || !nblk || !nstrip) return fail(FDW_EINVAL, "NULL argument");
    if (c->prm.dialect != FDW_DIALECT_RTM || !is_full_grid(c)) return fail(FDW_ESTATE, "step4 plan: line sources need a full-grid context of the RTM dialect");
    if (c->h != kMaxFastHalfOrder) return fail(FDW_EINVAL, "step4: needs order 8");
    return step4_plan(c, FDW_MODE_FWD, line_source(kPlanFake + 5, sz), RowRanges{r0, r1, r0b, r1b, xchunk}, nblk, nstrip, cls, cls_cap);
}

// Trace samples of iterations it0 .. it0+nsteps-1 on the receiver rows the loop never time-steps (rows >= xlim of this slab): what the
// reference's d_pp holds there, from the fields (d_p, d_pp) before the first swap
static int record_static(fdw_ctx* c, const float* d_p, const float* d_pp, int gz, float* d_rec, int it0, int nsteps, hipStream_t s)
{
    if (nsteps <= 0) return FDW_OK;
    const size_t nxs = (size_t)c->nx;
    const int rec_x0 = c->prm.nxb - c->slab.x_off, r0 = std::max({rec_x0, c->upd_x1, 0}), r1 = std::min(rec_x0 + c->nx, c->nxl);
    const long long rec_bstride = c->nbatch > 1 ? (long long)nxs * c->batch_nt : 0;
    hipError_t e = launch_record_static(d_p, d_pp, d_rec + (size_t)it0 * nxs, c->pitch, r0, r1 - r0, gz, rec_x0, c->nx, nsteps, c->nbatch,
                                        (long long)field_elems(c), rec_bstride, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "static receiver rows: launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

// ---- consecutive pipeline passes as row bands on side streams (fdwave.h: fdw_plan_pass_bands) -----------------------------------------
// The schedule.  Pure host arithmetic: no context, no HIP call.
extern "C" int fdw_plan_pass_bands(int nxl, int upd_x1, int xchunk, int bands, int depth, int npasses, int* bands_out, int* depth_out,
                                   fdw_band_unit* units, int cap)
{
    if (nxl <= 0 || upd_x1 < 0 || upd_x1 > nxl || xchunk <= 0 || bands < 1 || depth < 1 || depth > FDW_PASS_DEPTH_MAX || npasses < 1 || (units && cap < 0))
        return fail(FDW_EINVAL, "pass bands: nxl=%d upd_x1=%d xchunk=%d bands=%d depth=%d (1..%d) npasses=%d", nxl, upd_x1, xchunk, bands, depth,
                    FDW_PASS_DEPTH_MAX, npasses);
    constexpr int reach = kPipeSteps * kMaxFastHalfOrder;      // rows beyond its own that a pass reads on either side
    const int nchunks = (upd_x1 + xchunk - 1) / xchunk;
    int G = bands, D = depth;
    // the first nchunks % G bands hold one chunk row more than the others; the thinnest band is the last (it also has the ragged chunk)
    const int base = nchunks / G, extra = nchunks % G;
    auto first_chunk = [&](int g) { return g * base + std::min(g, extra); };
    const bool safe = G >= 2 && G >= D + 1 && base >= 1 && (long)base * xchunk >= reach && upd_x1 - first_chunk(G - 1) * xchunk >= reach;
    if (!safe) G = D = 1;
    if (npasses > INT_MAX / G) return fail(FDW_EINVAL, "pass bands: %d passes of %d bands", npasses, G);
    if (bands_out) *bands_out = G;
    if (depth_out) *depth_out = D;
    const int total = G * npasses;
    for (int i = 0; units && i < std::min(cap, total); i++) {
        fdw_band_unit& u = units[i];
        u.pass = i / G; u.band = i % G;
        u.r0 = G == 1 ? 0 : first_chunk(u.band) * xchunk;
        u.r1 = u.band == G - 1 ? nxl : first_chunk(u.band + 1) * xchunk;
        u.stream = i % D;
        u.nwait = 0;
        for (int k = 0; k < FDW_PASS_DEPTH_MAX - 1; k++) u.wait[k] = -1;
        for (int j = i - D - 1; j >= i - 2 * D + 1 && j >= 0; j--) u.wait[u.nwait++] = j;
    }
    return total;
}

extern "C" int fdw_set_pass_bands(fdw_ctx* c, int bands, int depth)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (bands < 0 || depth < 0 || depth > FDW_PASS_DEPTH_MAX || (bands == 0) != (depth == 0))
        return fail(FDW_EINVAL, "pass bands: bands=%d depth=%d (0, 0 = automatic; depth 1..%d)", bands, depth, FDW_PASS_DEPTH_MAX);
    c->pb_bands = bands; c->pb_depth = depth;
    return FDW_OK;
}

extern "C" int fdw_pass_bands(const fdw_ctx* c, int* bands, int* depth)
{
    if (!c || !bands || !depth) return fail(FDW_EINVAL, "NULL argument");
    *bands = c->pb_used_bands; *depth = c->pb_used_depth;
    return FDW_OK;
}

// ---- two bands with a moving cut (fdwave.h: fdw_plan_pass_cut) -----------------------------------------------------------------------
// The schedule.  Pure host arithmetic: no context, no HIP call.
extern "C" int fdw_plan_pass_cut(int nxl, int upd_x1, int xchunk, int cut_lo, int cut_hi, int npasses, int* lo_out, int* hi_out,
                                 fdw_band_unit* units, int cap)
{
    if (nxl <= 0 || upd_x1 < 0 || upd_x1 > nxl || xchunk <= 0 || cut_lo < 0 || cut_hi < cut_lo || npasses < 1 || (units && cap < 0))
        return fail(FDW_EINVAL, "pass cut: nxl=%d upd_x1=%d xchunk=%d cut=[%d,%d] npasses=%d", nxl, upd_x1, xchunk, cut_lo, cut_hi, npasses);
    constexpr int reach = kPipeSteps * kMaxFastHalfOrder;      // rows beyond its own that a pass reads on either side
    const int nchunks = (upd_x1 + xchunk - 1) / xchunk;
    // the lower unit is thinnest at cut_lo, the upper one at cut_hi; a cut that moves by one chunk row moves by at least the reach
    const bool safe = xchunk >= reach && nchunks >= 3 && cut_lo < cut_hi && cut_lo >= 1 && cut_hi < nchunks && upd_x1 - (long)cut_hi * xchunk >= reach;
    if (npasses > INT_MAX / 3) return fail(FDW_EINVAL, "pass cut: %d passes", npasses);
    if (lo_out) *lo_out = safe ? cut_lo : 0;
    if (hi_out) *hi_out = safe ? cut_hi : 0;
    auto clear_waits = [](fdw_band_unit& u) {
        u.nwait = 0;
        for (int k = 0; k < FDW_PASS_DEPTH_MAX - 1; k++) u.wait[k] = -1;
    };
    if (!safe) {
        for (int i = 0; units && i < std::min(cap, npasses); i++) {
            fdw_band_unit& u = units[i];
            u.pass = i; u.band = 0; u.r0 = 0; u.r1 = nxl; u.stream = 0;
            clear_waits(u);
        }
        return npasses;
    }
    auto meet = [](int a0, int a1, int b0, int b1) { return a0 < b1 && b0 < a1; };      // rows [a0, a1) against rows [b0, b1)
    int total = 0;
    fdw_band_unit prev{};
    auto emit = [&](int pass, int band, int r0, int r1) {
        const int i = total++;
        fdw_band_unit u{};
        u.pass = pass; u.band = band; u.r0 = r0; u.r1 = r1;
        u.stream = i % 2;
        clear_waits(u);
        if (i >= 1 && prev.pass != pass) {
            // the unit before belongs to the pass before: it wrote the buffers this unit reads and read the buffers this unit writes
            const int rd0 = std::max(r0 - reach, 0), rd1 = std::min(r1 + reach, nxl);
            const int prd0 = std::max(prev.r0 - reach, 0), prd1 = std::min(prev.r1 + reach, nxl);
            if (meet(prev.r0, prev.r1, rd0, rd1) || meet(r0, r1, prd0, prd1)) u.wait[u.nwait++] = i - 1;
        }
        if (i >= 3) u.wait[u.nwait++] = i - 3;
        if (units && i < cap) units[i] = u;
        prev = u;
    };
    // a range at least four chunk rows wide turns through a pass of three units, which needs no wait for the unit before; a narrower
    // one turns on the spot and its first unit after the turn waits
    const bool three = cut_hi - cut_lo >= 4;
    const int X = xchunk;
    int cut = cut_hi, dir = -1;      // the cut of the pass and the way it moved to get there
    for (int n = 0; n < npasses; n++) {
        if (n > 0 && three && dir < 0 && cut == cut_lo + 1) {
            // the lower unit needs the lower unit before it alone, the upper unit the upper one alone; the middle comes last, so that the
            // upper unit of the next pass, [(cut_lo + 3) X, nxl), shares no row with the unit before it
            emit(n, 0, 0, cut_lo * X);
            emit(n, 1, (cut_lo + 2) * X, nxl);
            emit(n, 2, cut_lo * X, (cut_lo + 2) * X);
            cut = cut_lo + 2; dir = 1;
            continue;
        }
        if (n > 0 && three && dir > 0 && cut == cut_hi - 1) {
            emit(n, 1, cut_hi * X, nxl);
            emit(n, 0, 0, (cut_hi - 2) * X);
            emit(n, 2, (cut_hi - 2) * X, cut_hi * X);
            cut = cut_hi - 2; dir = -1;
            continue;
        }
        if (n > 0) {
            if (!three && (cut + dir < cut_lo || cut + dir > cut_hi)) dir = -dir;
            cut += dir;
        }
        for (int k = 0; k < 2; k++) {
            if ((k == 0) == (dir < 0)) emit(n, 0, 0, cut * X);      // the cut moved down: lower unit first; up: upper unit first
            else emit(n, 1, cut * X, nxl);
        }
    }
    return total;
}

extern "C" int fdw_set_pass_cut(fdw_ctx* c, int lo, int hi)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (!((lo == 0 && hi == 0) || (lo == -1 && hi == -1) || (lo >= 1 && hi >= lo)))
        return fail(FDW_EINVAL, "pass cut: lo=%d hi=%d (0, 0 = automatic; -1, -1 = off; else 1 <= lo <= hi)", lo, hi);
    c->pc_lo = lo; c->pc_hi = hi;
    return FDW_OK;
}

extern "C" int fdw_pass_cut(const fdw_ctx* c, int* lo, int* hi, int* turns)
{
    if (!c || !lo || !hi || !turns) return fail(FDW_EINVAL, "NULL argument");
    *lo = c->pc_used_lo; *hi = c->pc_used_hi; *turns = c->pc_used_turns;
    return FDW_OK;
}

// The wanted bands / depth of the forward loop's pipeline passes of `tiles` tiles each: the knob, else FDW_PASS_BANDS="G,D" (experiments),
// else the automatic policy, which is the measurement on one MI355X and nothing else (DESIGN.md section 3c, round 13;
// profiles/r13_band_probe.txt, python bench.py against the parent commit, Gpoints/s):
//   tiles   grid            3/2      other settings
//    950    4096^2          -16 %    (4/2 -30 %)
//   1204    6144^2          +1.6 % in one session, +0.9 % with overlapping ranges in the next; FAST -0.2 %: not separable
//   1776    8192^2          +3.4 %   (4/2 -4 %, every D = 3 -25 % and worse, 3/1 -24 %: cutting alone costs);  FAST numerics +7.6 %
//   3960    12288^2         +3.1 %   (4/2 +3.0 %, 6/2 +0.4 %)
//   4810    16384^2         +1.8 %   (4/2, 5/2 +1.7 %, 6/2 +1.2 %, 7/2 -0.2 %, 8/2 -1.4 %, 9/2 -2.8 %);  FAST numerics +4.2 %
// Three bands two deep wherever it was measured to gain: the fewest bands the schedule allows, so the price of cutting is least and two
// resident units together are the largest.  All of these are calls of 100 passes and more.  The units overlap only inside one call (it
// joins before it returns), so a call of a single pass pays for the cut and gets nothing back: below kBandAutoPasses the automatic policy
// stays at one band (a bound from that reasoning, not from a measurement).
// The gain needs the side stream on a hardware queue of its own.  A process holds four; where more streams are alive than that the
// runtime lets streams share a queue, and a side stream that shares the caller's runs behind it: the schedule then costs what 3/1 costs.
// Seen on the slab driver's context (one rank, three more streams: a whole 8192^2 shot 586 against 650 Gpoints/s), which therefore sets
// one band for its context (fdw_slabs_create), and on every depth-3 setting above (two of the three streams on one queue,
// profiles/r13_band_probe.txt).  A caller with many streams of its own does the same: fdw_set_pass_bands(ctx, 1, 1).
constexpr int kBandAutoTiles = 1776, kBandAutoPasses = 8;      // 1776: the smallest pass measured to gain, every run above the parent's
static void wanted_pass_bands(const fdw_ctx* c, long tiles, int npasses, int* bands, int* depth)
{
    *bands = *depth = 1;
    if (c->pb_bands > 0) {
        *bands = c->pb_bands; *depth = c->pb_depth;
    } else if (const char* e = getenv("FDW_PASS_BANDS")) {
        int g = 0, d = 0;
        if (sscanf(e, "%d,%d", &g, &d) == 2 && g >= 1 && d >= 1 && d <= FDW_PASS_DEPTH_MAX) { *bands = g; *depth = d; }
    } else if (tiles >= kBandAutoTiles && npasses >= kBandAutoPasses) {
        *bands = 3; *depth = 2;
    }
}

// Whether the forward loop's passes run as two bands with a moving cut, asked only while the band policy above is automatic: the knob, else
// FDW_PASS_CUT="lo,hi" (experiments; anything unreadable: off), else the automatic policy.  `nchunks`: chunk rows of a pass at the chunk
// length this schedule would use.
// Automatic, from the measurement on one MI355X (profiles/r21_ab_bench.txt; python bench.py, the moving
// cut over the middle third of the chunk rows against what the tree did before, Gpoints/s):
//   strip rows   grid       before                  moving cut
//     78 k       4096^2     one band, 83 rows       +5.9 % (FAST +2.0 %)
//    172 k       6144^2     one band, 143 rows      +10.6 % (FAST, 173 rows, +1.5 %)
//    303 k       8192^2     3/2, 173 rows           173 rows +0.7 %; 213 rows +2.2 % (FAST +2.2 %); 253 rows +1.0 %
//    676 k       12288^2    3/2, 173 rows           173 rows -1.7 %, 253 rows +0.5 .. 1.3 %: stays with the three bands
//   1212 k       16384^2    3/2, 253 rows           -1.4 %: stays with the three bands
// Narrower ranges lose (8192^2, 213 rows: [16,23] -0.6 %, [17,22] -2.2 % against [13,26]): every turn costs a small launch that holds its
// queue for a tile's time; so do wide ones ([2,37] -6 %): a small unit beside a large one leaves the large one's start and end uncovered.
constexpr long kCutAutoMinStripRows = 60000, kCutAutoMaxStripRows = 500000;
static bool wanted_pass_cut(const fdw_ctx* c, long strip_rows, int nchunks, int npasses, int* lo, int* hi)
{
    if (c->pc_lo >= 1) { *lo = c->pc_lo; *hi = c->pc_hi; return true; }
    if (c->pc_lo < 0) return false;
    if (const char* e = getenv("FDW_PASS_CUT")) {
        int a = 0, b = 0;
        if (sscanf(e, "%d,%d", &a, &b) != 2 || a < 1 || b < a) return false;
        *lo = a; *hi = b;
        return true;
    }
    if (strip_rows < kCutAutoMinStripRows || strip_rows >= kCutAutoMaxStripRows || npasses < kBandAutoPasses) return false;
    *lo = nchunks / 3; *hi = nchunks - nchunks / 3;      // the middle third: both units stay above a third of the pass
    return true;
}

static int ensure_band_streams(fdw_ctx* c, int depth)
{
    if (!c->pb_fork) HIP_TRY(hipEventCreateWithFlags(&c->pb_fork, hipEventDisableTiming));
    for (hipEvent_t& e : c->pb_ring)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (int j = 0; j < depth - 1; j++) {
        if (!c->pb_side[j]) HIP_TRY(hipStreamCreateWithFlags(&c->pb_side[j], hipStreamNonBlocking));
        if (!c->pb_join[j]) HIP_TRY(hipEventCreateWithFlags(&c->pb_join[j], hipEventDisableTiming));
    }
    return FDW_OK;
}

// Plain forward passes of the pipeline kernel (what steps_loop's first branch issues one after the other on s) as the launch units of
// fdw_plan_pass_bands or fdw_plan_pass_cut, whole passes one after the other: every unit on the stream its plan names (D of them) behind the
// events of the units the plan names.  Fork: every side stream starts behind an event recorded on s here.  Join: s waits for the last unit of every
// side stream, whatever happened in between.  *ip, *ipp advance over the passes issued.
static int unit_passes(fdw_ctx* c, float* const* buf, const float* d_v2, const Forward& f, int it0, int first_pp_twice, int* ip, int* ipp, hipStream_t s,
                       const std::vector<fdw_band_unit>& units, int D, int xchunk)
{
    const int total = (int)units.size();
    std::vector<char> awaited((size_t)total, 0);      // units whose event someone waits for
    for (int i = 0; i < total; i++) {
        const fdw_band_unit& u = units[(size_t)i];
        if (u.stream < 0 || u.stream >= D || u.nwait < 0 || u.nwait > FDW_PASS_DEPTH_MAX - 1) return fail(FDW_ESTATE, "pass units: unit %d is malformed", i);
        for (int w = 0; w < u.nwait; w++) {
            if (u.wait[w] < 0 || u.wait[w] >= i || i - u.wait[w] >= kBandRing) return fail(FDW_ESTATE, "pass units: unit %d waits for unit %d", i, u.wait[w]);
            awaited[(size_t)u.wait[w]] = 1;
        }
    }
    hipStream_t st[FDW_PASS_DEPTH_MAX] = {s};
    if (D > 1) {
        FDW_TRY(ensure_band_streams(c, D));
        HIP_TRY(hipEventRecord(c->pb_fork, s));
        for (int j = 1; j < D; j++) {
            st[j] = c->pb_side[j - 1];
            HIP_TRY(hipStreamWaitEvent(st[j], c->pb_fork, 0));
        }
    }
    auto issue = [&]() -> int {
        int o1 = 0, o2 = 0;
        for (int i = 0; i < total; i++) {
            const fdw_band_unit& u = units[(size_t)i];
            if (i == 0 || units[(size_t)i - 1].pass != u.pass) spare_pair(*ip, *ipp, &o1, &o2);      // the first unit of its pass
            const int k = u.pass * kPipeSteps;
            for (int w = 0; w < u.nwait; w++) HIP_TRY(hipStreamWaitEvent(st[u.stream], c->pb_ring[u.wait[w] % kBandRing], 0));
            FDW_TRY(stepn_impl(c, FDW_MODE_FWD, buf[*ipp], buf[*ip], d_v2, buf[o1], buf[o2], (k > 0) || first_pp_twice, view_at(f, it0 + k, c->nx), StepnBack{},
                                RowRanges{u.r0, u.r1, 0, 0, xchunk}, st[u.stream]));
            if (D > 1 && awaited[(size_t)i]) HIP_TRY(hipEventRecord(c->pb_ring[i % kBandRing], st[u.stream]));
            if (i + 1 == total || units[(size_t)i + 1].pass != u.pass) { *ip = o1; *ipp = o2; }      // the last: d_p = u^{n+kPipeSteps-1}, d_pp = u^{n+kPipeSteps}
        }
        return FDW_OK;
    };
    const int rc = issue();
    char msg[sizeof g_err];
    if (rc != FDW_OK) memcpy(msg, g_err, sizeof msg);
    int jrc = FDW_OK;
    for (int j = 1; j < D; j++) {
        hipError_t e = hipEventRecord(c->pb_join[j - 1], st[j]);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, c->pb_join[j - 1], 0);
        if (e != hipSuccess && jrc == FDW_OK) jrc = fail(FDW_EHIP, "pass bands: joining side stream %d failed: %s", j, hipGetErrorString(e));
    }
    if (rc != FDW_OK) memcpy(g_err, msg, sizeof msg);      // the first error is the one to report
    return rc != FDW_OK ? rc : jrc;
}

// `npasses` passes as G fixed bands D deep
static int band_passes(fdw_ctx* c, float* const* buf, const float* d_v2, const Forward& f, int it0, int npasses, int first_pp_twice, int* ip, int* ipp,
                       hipStream_t s, int G, int D, int xchunk)
{
    std::vector<fdw_band_unit> units((size_t)G * npasses);
    int g_ = 0, d_ = 0;
    const int total = fdw_plan_pass_bands(c->nxl, c->upd_x1, xchunk, G, D, npasses, &g_, &d_, units.data(), (int)units.size());
    if (total < 0) return total;
    if (g_ != G || d_ != D || total != (int)units.size()) return fail(FDW_ESTATE, "pass bands: the plan changed between two calls");
    return unit_passes(c, buf, d_v2, f, it0, first_pp_twice, ip, ipp, s, units, D, xchunk);
}

// `npasses` passes as two bands whose cut moves between chunk rows lo and hi; *turns: the passes of three units and the units that wait for the
// unit just before them
static int cut_passes(fdw_ctx* c, float* const* buf, const float* d_v2, const Forward& f, int it0, int npasses, int first_pp_twice, int* ip, int* ipp,
                      hipStream_t s, int lo, int hi, int xchunk, int* turns)
{
    int lo_ = 0, hi_ = 0;
    const int total = fdw_plan_pass_cut(c->nxl, c->upd_x1, xchunk, lo, hi, npasses, &lo_, &hi_, nullptr, 0);
    if (total < 0) return total;
    std::vector<fdw_band_unit> units((size_t)total);
    if (lo_ != lo || hi_ != hi || fdw_plan_pass_cut(c->nxl, c->upd_x1, xchunk, lo, hi, npasses, &lo_, &hi_, units.data(), total) != total)
        return fail(FDW_ESTATE, "pass cut: the plan changed between two calls");
    *turns = 0;
    for (int i = 1; i < total; i++) *turns += units[(size_t)i].band == 2 || (units[(size_t)i].nwait > 0 && units[(size_t)i].wait[0] == i - 1);
    return unit_passes(c, buf, d_v2, f, it0, first_pp_twice, ip, ipp, s, units, 2, xchunk);
}

// A pass of m steps whose family has no kernel for the loop's extras (the two-step family: point-source recording + illumination, the
// excitation maps and the pick) becomes m single steps that land where the pass would: u^{n+1} in buf[o1], u^{n+2} in buf[o2], the current
// pair left as it is, each on a copy of the field it overwrites -- the same fields in all four buffers, the same indices and static rows
// as the plain loop.  `it`: the iteration of the first step.
static int single_steps_on_copies(fdw_ctx* c, float* const* buf, const float* d_v2, const Forward& f, int it, int m, int twice, int ip, int ipp, int o1,
                                  int o2, hipStream_t s)
{
    const size_t bytes = field_elems(c) * sizeof(float) * (size_t)std::max(c->nbatch, 1);
    const float* newest = buf[ipp];
    for (int j = 0; j < m; j++) {
        float* dst = buf[(j & 1) ? o2 : o1];
        if (j < 2) HIP_TRY(hipMemcpyAsync(dst, buf[j == 0 ? ip : ipp], bytes, hipMemcpyDeviceToDevice, s));
        FDW_TRY(step_impl(c, FDW_MODE_FWD, newest, dst, d_v2, 0, c->nxl, twice || j > 0, view_at(f, it + j, c->nx), BackExtra{}, s));
        newest = dst;
    }
    return FDW_OK;
}

// nsteps reference iterations (R:259-267) over four rotating buffers: kPipeSteps per pass through the wave pipeline, pairs of steps through
// the two-step kernel, single steps through the one-step kernel, whichever pays.  On entry buf[*ip], buf[*ipp] are the reference's (d_p, d_pp)
// BEFORE the first swap; on return they index (d_p, d_pp) after the loop.  Whatever the loop does besides stepping (Forward: recording,
// illumination, a line source, the excitation maps or pick): the same family per pass, the same rotation, the same static rows, each pass
// through its kernel's variant (kFwdVariants), and every family equals the one-step iteration bit for bit.  Inside a batch (c->nbatch > 1,
// one-step passes only) a line source's samples are the batch's [shot][nt][nx] and step_impl strides them per shot.
static int steps_loop(fdw_ctx* c, float* const* buf, const float* d_v2, const Forward& f, int it0, int nsteps, int first_pp_twice, int* ip, int* ipp,
                      hipStream_t s)
{
    if (!c || !buf || !ip || !ipp) return fail(FDW_EINVAL, "NULL argument");
    if (*ip < 0 || *ip > 3 || *ipp < 0 || *ipp > 3 || *ip == *ipp) return fail(FDW_EINVAL, "steps2: bad buffer indices");
    const FwdVariant var = fwd_variant(FDW_MODE_FWD, f);
    if (var.kmode < 0) return fail(FDW_EINVAL, "steps: no kernel is built for this combination of a line source, recording, illumination and excitation");
    if (f.rec) FDW_TRY(record_static(c, buf[*ip], buf[*ipp], f.gz, f.rec, it0, nsteps, s));
    int k = 0;
    c->pb_used_bands = c->pb_used_depth = 1;
    c->pc_used_lo = c->pc_used_hi = -1; c->pc_used_turns = 0;
    if (f.may_band && var.kmode == FDW_MODE_FWD && c->nbatch <= 1 && nsteps >= kPipeSteps && pipe_pays(c)) {
        // fdw_dev_steps2, the plain forward loop on caller-owned buffers: its pipeline passes may run as row bands (whole chunk rows of the pass's own chunk length: the same tiles)
        const int nstrip = pipe_strips(c), npasses = nsteps / kPipeSteps;
        const long strip_rows = (long)c->upd_x1 * nstrip;
        const int xchunk = pipe_fwd_xchunk(c, strip_rows), xcut = pipe_fwd_xchunk(c, strip_rows, true);
        int G = 1, D = 1, lo = 0, hi = 0;
        // a band policy that is set, by the knob or the environment, is kept; else the moving cut where it is wanted; else the automatic bands
        const bool bands_set = c->pb_bands > 0 || getenv("FDW_PASS_BANDS");
        if (!bands_set && wanted_pass_cut(c, strip_rows, (c->upd_x1 + xcut - 1) / xcut, npasses, &lo, &hi)) {
            if (fdw_plan_pass_cut(c->nxl, c->upd_x1, xcut, lo, hi, npasses, &lo, &hi, nullptr, 0) < 0) return FDW_EINVAL;
            if (lo > 0) {      // else too thin: the plain loop below
                c->pb_used_bands = c->pb_used_depth = 2;
                c->pc_used_lo = lo; c->pc_used_hi = hi;
                FDW_TRY(cut_passes(c, buf, d_v2, f, it0, npasses, first_pp_twice, ip, ipp, s, lo, hi, xcut, &c->pc_used_turns));
                k = npasses * kPipeSteps;
            }
        } else {
            wanted_pass_bands(c, (long)nstrip * ((c->upd_x1 + xchunk - 1) / xchunk), npasses, &G, &D);
            if (G > 1 && fdw_plan_pass_bands(c->nxl, c->upd_x1, xchunk, G, D, npasses, &G, &D, nullptr, 0) < 0) return FDW_EINVAL;
        }
        if (G > 1) {
            c->pb_used_bands = G; c->pb_used_depth = D;
            FDW_TRY(band_passes(c, buf, d_v2, f, it0, npasses, first_pp_twice, ip, ipp, s, G, D, xchunk));
            k = npasses * kPipeSteps;
        }
    }
    while (k < nsteps) {
        const int twice = (k > 0) || first_pp_twice;
        const FwdView v = view_at(f, it0 + k, c->nx);
        // the steps of this pass: the family that pays among those the steps left allow
        const int m = (nsteps - k >= kPipeSteps && pipe_pays(c)) ? kPipeSteps : ((nsteps - k >= 2 && two_step_pays(c)) ? 2 : 1);
        if (m == 1) {
            std::swap(*ip, *ipp);
            FDW_TRY(step_impl(c, FDW_MODE_FWD, buf[*ip], buf[*ipp], d_v2, 0, c->nxl, twice, v, BackExtra{}, s));
            k += 1;
            continue;
        }
        int o1, o2;   // the two buffers not holding the current pair
        spare_pair(*ip, *ipp, &o1, &o2);
        // after the swap the kernel's p is the old d_pp (newest field), its pp the old d_p
        if (!family_serves(m, var))
            FDW_TRY(single_steps_on_copies(c, buf, d_v2, f, it0 + k, m, twice, *ip, *ipp, o1, o2, s));
        else if (m == kPipeSteps)
            FDW_TRY(stepn_impl(c, FDW_MODE_FWD, buf[*ipp], buf[*ip], d_v2, buf[o1], buf[o2], twice, v, StepnBack{}, RowRanges{}, s));
        else
            FDW_TRY(step2_impl(c, FDW_MODE_FWD, buf[*ipp], buf[*ip], d_v2, buf[o1], buf[o2], twice, v, BackExtra{}, s));
        *ip = o1; *ipp = o2;   // d_p = u^{n+m-1}, d_pp = u^{n+m}
        k += m;
    }
    return FDW_OK;
}

extern "C" int fdw_dev_steps2(fdw_ctx* c, float* const* buf, const float* d_v2, const float* d_srce, int sx, int sz, int it0, int nsteps,
                              int first_pp_twice, int* ip, int* ipp, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "NULL argument");
    Forward f = point_source(d_srce, sx, sz);
    f.may_band = true;
    return steps_loop(c, buf, d_v2, f, it0, nsteps, first_pp_twice, ip, ipp, pick_stream(c, stream));
}

// the receiver column of a recorded gather: one the forward loop time-steps (R:83-87: j < zlim)
static int check_record_depth(const fdw_ctx* c, int gz)
{
    if (c->prm.dialect != FDW_DIALECT_RTM) return fail(FDW_ESTATE, "trace recording belongs to the RTM dialect (the sibling's has fdw_model_shot)");
    if (gz < 0 || gz >= c->zlim) return fail(FDW_EINVAL, "receiver depth %d outside the time-stepped columns [0,%d)", gz, c->zlim);
    return FDW_OK;
}

extern "C" int fdw_dev_record_steps(fdw_ctx* c, float* const* d_buf, const float* d_v2, const float* d_srce, int sx, int sz, int gz, float* d_rec,
                                    int it0, int nsteps, int first_pp_twice, int* ip, int* ipp, void* stream)
{
    if (!c || !d_rec) return fail(FDW_EINVAL, "NULL argument");
    if (it0 < 0) return fail(FDW_EINVAL, "it0=%d", it0);
    FDW_TRY(check_record_depth(c, gz));
    const Forward f = point_source(d_srce, sx, sz).recording(d_rec, gz);
    return steps_loop(c, d_buf, d_v2, f, it0, nsteps, first_pp_twice, ip, ipp, pick_stream(c, stream));
}

// ---- what the slab driver's recording loop (fdw_slabs_dev_record_forward) launches: fdw_dev_step / fdw_dev_step4 on row ranges of the slab
// that also write their trace rows (d_rec_row: this step's [nx]; d_rec: the pass's four), and the static receiver rows of a whole call.
// d_rec* == NULL: exactly the plain launch.
int fdw_check_record_depth(const fdw_ctx* c, int gz) { return c ? check_record_depth(c, gz) : fail(FDW_EINVAL, "ctx is NULL"); }

int fdw_dev_step_rec(fdw_ctx* c, const float* d_p, float* d_pp, const float* d_v2, int r0, int r1, int pp_twice, const float* d_srce_it, int sx, int sz,
                     float* d_rec_row, int gz, hipStream_t s)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    return step_impl(c, FDW_MODE_FWD, d_p, d_pp, d_v2, r0, r1, pp_twice, view_at(point_source(d_srce_it, sx, sz).recording(d_rec_row, gz), 0, c->nx), BackExtra{},
                     pick_stream(c, s));
}

int fdw_dev_step4_rec(fdw_ctx* c, const float* d_p, const float* d_pp, const float* d_v2, float* d_out1, float* d_out2, int pp_twice, const float* d_srce_it,
                      int sx, int sz, int r0, int r1, int r0b, int r1b, int xchunk, float* d_rec, int gz, hipStream_t s)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (c->h != kMaxFastHalfOrder || (size_t)c->nxl * c->pitch * sizeof(float) >= (1ull << 31))
        return fail(FDW_EINVAL, "step4: needs order 8 and fields below 2 GiB");
    return stepn_impl(c, FDW_MODE_FWD, d_p, d_pp, d_v2, d_out1, d_out2, pp_twice, view_at(point_source(d_srce_it, sx, sz).recording(d_rec, gz), 0, c->nx), StepnBack{},
                      RowRanges{r0, r1, r0b, r1b, xchunk}, pick_stream(c, s));
}

int fdw_dev_record_static(fdw_ctx* c, const float* d_p, const float* d_pp, int gz, float* d_rec, int it0, int nsteps, hipStream_t s)
{
    if (!c || !d_p || !d_pp || !d_rec) return fail(FDW_EINVAL, "NULL argument");
    return record_static(c, d_p, d_pp, gz, d_rec, it0, nsteps, pick_stream(c, s));
}

// What source illumination, line sources, excitation-amplitude imaging, wavefield snapshots and residual migration (`what`) ask of the
// context: the RTM dialect on the whole grid, one shot at a time
static int check_single_shot_ctx(const fdw_ctx* c, const char* what, const char* who)
{
    if (c->prm.dialect != FDW_DIALECT_RTM) return fail(FDW_ESTATE, "%s: %s: RTM dialect only", who, what);
    if (!is_full_grid(c)) return fail(FDW_ESTATE, "%s: %s: full-grid contexts only (slab-decomposed shots are not covered)", who, what);
    if (c->nbatch > 1) return fail(FDW_ESTATE, "%s: not inside a batch of shots", who);
    return FDW_OK;
}

extern "C" int fdw_dev_illum_steps(fdw_ctx* c, float* const* d_buf, const float* d_v2, const float* d_srce, int sx, int sz, float* d_illum, int it0,
                                   int nsteps, int first_pp_twice, int* ip, int* ipp, void* stream)
{
    if (!c || !d_illum) return fail(FDW_EINVAL, "NULL argument");
    if (it0 < 0) return fail(FDW_EINVAL, "it0=%d", it0);
    FDW_TRY(check_single_shot_ctx(c, "source illumination", "fdw_dev_illum_steps"));
    const Forward f = point_source(d_srce, sx, sz).illuminating(d_illum);
    return steps_loop(c, d_buf, d_v2, f, it0, nsteps, first_pp_twice, ip, ipp, pick_stream(c, stream));
}

// the forward loop that records and accumulates in one launch per pass (the forward loop of fdw_shot_residual with an accumulator)
extern "C" int fdw_dev_record_illum_steps(fdw_ctx* c, float* const* d_buf, const float* d_v2, const float* d_srce, int sx, int sz, int gz, float* d_rec,
                                          float* d_illum, int it0, int nsteps, int first_pp_twice, int* ip, int* ipp, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "NULL argument");
    if (!d_rec || !d_illum)
        return fail(FDW_EINVAL, "fdw_dev_record_illum_steps needs both d_rec and d_illum (one alone: fdw_dev_record_steps / fdw_dev_illum_steps)");
    if (it0 < 0) return fail(FDW_EINVAL, "it0=%d", it0);
    FDW_TRY(check_single_shot_ctx(c, "source illumination", "fdw_dev_record_illum_steps"));
    FDW_TRY(check_record_depth(c, gz));
    const Forward f = point_source(d_srce, sx, sz).recording(d_rec, gz).illuminating(d_illum);
    return steps_loop(c, d_buf, d_v2, f, it0, nsteps, first_pp_twice, ip, ipp, pick_stream(c, stream));
}

// ---- line sources (definitions in fdwave.h) ----
// the depth of the line, and recording and illumination together only where the caller runs the combined kernels
static int check_line_args(const fdw_ctx* c, const char* who, int sz, int gz, bool rec, bool illum, bool both_built = false)
{
    if (rec && illum && !both_built) return fail(FDW_EINVAL, "%s: trace recording and illumination together are not built for a line source", who);
    if (sz < 0 || sz >= c->zlim) return fail(FDW_EINVAL, "%s: line-source depth %d outside the time-stepped columns [0,%d)", who, sz, c->zlim);
    if (rec) FDW_TRY(check_record_depth(c, gz));
    return FDW_OK;
}

extern "C" int fdw_dev_line_steps(fdw_ctx* c, float* const* d_buf, const float* d_v2, const float* d_wav, int sz, int gz, float* d_rec, float* d_illum,
                                  int it0, int nsteps, int first_pp_twice, int* ip, int* ipp, void* stream)
{
    if (!c || !d_wav) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "line sources", "fdw_dev_line_steps"));
    if (it0 < 0) return fail(FDW_EINVAL, "it0=%d", it0);
    FDW_TRY(check_line_args(c, "fdw_dev_line_steps", sz, gz, d_rec != nullptr, d_illum != nullptr));
    const Forward f = line_source(d_wav, sz).recording(d_rec, gz).illuminating(d_illum);
    return steps_loop(c, d_buf, d_v2, f, it0, nsteps, first_pp_twice, ip, ipp, pick_stream(c, stream));
}

// fdw_dev_line_steps that writes the trace rows and accumulates, one launch per pass: every family's combined line-source kernel
extern "C" int fdw_dev_line_record_illum_steps(fdw_ctx* c, float* const* d_buf, const float* d_v2, const float* d_wav, int sz, int gz, float* d_rec,
                                               float* d_illum, int it0, int nsteps, int first_pp_twice, int* ip, int* ipp, void* stream)
{
    if (!c || !d_wav) return fail(FDW_EINVAL, "NULL argument");
    if (!d_rec || !d_illum)
        return fail(FDW_EINVAL, "fdw_dev_line_record_illum_steps needs both d_rec and d_illum (one alone or neither: fdw_dev_line_steps)");
    FDW_TRY(check_single_shot_ctx(c, "line sources", "fdw_dev_line_record_illum_steps"));
    if (it0 < 0) return fail(FDW_EINVAL, "it0=%d", it0);
    FDW_TRY(check_line_args(c, "fdw_dev_line_record_illum_steps", sz, gz, true, true, true));
    const Forward f = line_source(d_wav, sz).recording(d_rec, gz).illuminating(d_illum);
    return steps_loop(c, d_buf, d_v2, f, it0, nsteps, first_pp_twice, ip, ipp, pick_stream(c, stream));
}

// ---- excitation-amplitude imaging (definitions in fdwave.h) ----
// a point source the maps' forward loop can inject: a cell the loop time-steps
static int check_exc_source(const fdw_ctx* c, const char* who, int sx, int sz)
{
    if (sz < 0 || sz >= c->zlim) return fail(FDW_EINVAL, "%s: source depth %d outside the time-stepped columns [0,%d)", who, sz, c->zlim);
    if (sx >= c->upd_x1) return fail(FDW_EINVAL, "%s: source row %d outside the time-stepped rows [0,%d)", who, sx, c->upd_x1);
    return FDW_OK;
}

extern "C" int fdw_dev_excite_steps(fdw_ctx* c, float* const* d_buf, const float* d_v2, const float* d_srce, int sx, int sz, float* d_amp, int* d_texc,
                                    int it0, int nsteps, int first_pp_twice, int* ip, int* ipp, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "excitation-amplitude imaging", "fdw_dev_excite_steps"));
    if (!d_buf || !d_buf[0] || !d_buf[1] || !d_buf[2] || !d_buf[3] || !d_v2 || !d_amp || !d_texc || !ip || !ipp) return fail(FDW_EINVAL, "NULL argument");
    if (it0 < 0) return fail(FDW_EINVAL, "it0=%d", it0);
    if (d_srce && sx >= 0) FDW_TRY(check_exc_source(c, "fdw_dev_excite_steps", sx, sz));
    const Forward f = point_source(d_srce, sx, sz).exciting(Exc::maps, d_amp, d_texc, 0);
    return steps_loop(c, d_buf, d_v2, f, it0, nsteps, first_pp_twice, ip, ipp, pick_stream(c, stream));
}

extern "C" int fdw_dev_line_pick_steps(fdw_ctx* c, float* const* d_buf, const float* d_v2, const float* d_wav, int sz, const int* d_texc, int top,
                                       float* d_exc, int it0, int nsteps, int first_pp_twice, int* ip, int* ipp, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "excitation-amplitude imaging", "fdw_dev_line_pick_steps"));
    if (!d_buf || !d_buf[0] || !d_buf[1] || !d_buf[2] || !d_buf[3] || !d_v2 || !d_wav || !d_texc || !d_exc || !ip || !ipp) return fail(FDW_EINVAL, "NULL argument");
    if (it0 < 0) return fail(FDW_EINVAL, "it0=%d", it0);
    FDW_TRY(check_line_args(c, "fdw_dev_line_pick_steps", sz, 0, false, false));
    const Forward f = line_source(d_wav, sz).exciting(Exc::pick, d_exc, const_cast<int*>(d_texc), top);      // the pick only reads the map
    return steps_loop(c, d_buf, d_v2, f, it0, nsteps, first_pp_twice, ip, ipp, pick_stream(c, stream));
}

// The image of `nshots` excitation shots on the device (fdw_excimg.hip), everything on s: the per-shot peak words zeroed, the peaks of |amp|
// over the interior, then img = img + exc / amp in shot order where |amp| > eps * peak.  d_exc, d_amp (and d_stack, if any): [nshots] fields,
// d_img one field; c->d_peak holds at least nshots words.
static int exc_image(fdw_ctx* c, const float* d_exc, const float* d_amp, float eps, float* d_img, float* d_stack, int nshots, hipStream_t s)
{
    const ExcImgGeom g{c->pitch, c->prm.nxb, c->nx, c->prm.nzb, c->nz, (long long)field_elems(c)};
    HIP_TRY(hipMemsetAsync(c->d_peak, 0, (size_t)nshots * sizeof(unsigned), s));
    hipError_t e = launch_exc_peak(d_amp, c->d_peak, g, nshots, s);
    if (e == hipSuccess) e = launch_exc_stack(d_exc, d_amp, c->d_peak, eps, d_img, d_stack, g, nshots, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "excitation image launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

static int check_exc_eps(const char* who, float eps)
{
    if (!(eps >= 0.0f) || std::isinf(eps)) return fail(FDW_EINVAL, "%s: eps must be finite and >= 0", who);
    return FDW_OK;
}

extern "C" int fdw_dev_image_excitation(fdw_ctx* c, const float* d_exc, const float* d_amp, float eps, float* d_img, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "excitation-amplitude imaging", "fdw_dev_image_excitation"));
    if (!d_exc || !d_amp || !d_img) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_exc_eps("fdw_dev_image_excitation", eps));
    return exc_image(c, d_exc, d_amp, eps, d_img, nullptr, 1, pick_stream(c, stream));
}

// d_out[i] = d_a[i] - d_b[i] (fdw_gather_residual_kernel); d_out may be d_a
static int gather_residual(const float* d_a, const float* d_b, float* d_out, size_t n, hipStream_t s)
{
    hipError_t e = launch_gather_residual(d_a, d_b, d_out, n, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "gather residual launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

extern "C" int fdw_dev_gather_residual(fdw_ctx* c, const float* d_a, const float* d_b, float* d_out, size_t n, void* stream)
{
    if (!c || (n > 0 && (!d_a || !d_b || !d_out))) return fail(FDW_EINVAL, "NULL argument");
    return gather_residual(d_a, d_b, d_out, n, pick_stream(c, stream));
}

// ksteps-cycle of the slab decomposition in one call: step j (1-based, j = j0 .. j0+nsteps-1) updates the
// rows still valid on the interior sides, [h*j, nxl - h*j) (decomp.py "deep halos").
extern "C" int fdw_dev_steps_shrink(fdw_ctx* c, float* d_p, float* d_pp, const float* d_v2, const float* d_srce, int sx, int sz,
                                    int it0, int nsteps, int first_pp_twice, int j0, int shrink_lo, int shrink_hi, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    hipStream_t s = pick_stream(c, stream);
    const Forward f = point_source(d_srce, sx, sz);
    for (int k = 0; k < nsteps; k++) {
        std::swap(d_p, d_pp);  // R:260-262
        const int j = j0 + k;
        const int r0 = shrink_lo ? c->h * j : 0;
        const int r1 = c->nxl - (shrink_hi ? c->h * j : 0);
        if (r1 <= r0) return fail(FDW_EINVAL, "steps_shrink: slab exhausted at cycle step %d", j);
        int rc = step_impl(c, FDW_MODE_FWD, d_p, d_pp, d_v2, r0, r1, (k > 0) || first_pp_twice, view_at(f, it0 + k, c->nx), BackExtra{}, s);
        if (rc) return rc;
    }
    return FDW_OK;
}

extern "C" int fdw_dev_steps(fdw_ctx* c, float* d_p, float* d_pp, const float* d_v2, const float* d_srce, int sx, int sz,
                             int it0, int nsteps, int first_pp_twice, void* stream)
{
    return fdw_dev_steps_shrink(c, d_p, d_pp, d_v2, d_srce, sx, sz, it0, nsteps, first_pp_twice, 0, 0, 0, stream);
}

extern "C" int fdw_dev_taper_finalize(fdw_ctx* c, float* d_f, void* stream)
{
    if (!c || !d_f) return fail(FDW_EINVAL, "ctx or field is NULL");
    hipError_t e = launch_taper_finalize(d_f, c->d_taperz, c->d_txfac, c->pitch, c->nxl, c->ztap, c->tz_x1, pick_stream(c, stream));
    if (e != hipSuccess) return fail(FDW_EHIP, "taper finalize launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// host <-> device transfers
// ------------------------------------------------------------------------------------------------
static int upload_rows(fdw_ctx* c, float* d_dst, const float* h_src, hipStream_t s)
{
    if (d_dst == c->d_v2) c->v2_resident = false;
    HIP_TRY(hipMemcpy2DAsync(d_dst, (size_t)c->pitch * sizeof(float), h_src, (size_t)c->prm.nze * sizeof(float),
                             (size_t)c->prm.nze * sizeof(float), c->nxl, hipMemcpyHostToDevice, s));
    return FDW_OK;
}
static int download_rows(fdw_ctx* c, float* h_dst, const float* d_src, hipStream_t s)
{
    HIP_TRY(hipMemcpy2DAsync(h_dst, (size_t)c->prm.nze * sizeof(float), d_src, (size_t)c->pitch * sizeof(float),
                             (size_t)c->prm.nze * sizeof(float), c->nxl, hipMemcpyDeviceToHost, s));
    return FDW_OK;
}

extern "C" int fdw_upload_field(fdw_ctx* c, float* d_dst, const float* h_src)
{
    if (!c || !d_dst || !h_src) return fail(FDW_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = upload_rows(c, d_dst, h_src, c->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}
extern "C" int fdw_download_field(fdw_ctx* c, float* h_dst, const float* d_src)
{
    if (!c || !h_dst || !d_src) return fail(FDW_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = download_rows(c, h_dst, d_src, c->stream);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

// The reference damps rows >= xlim of the top strip with taperx only, every step, in place; the lazy
// scheme cannot reproduce that for rows that are never rewritten.  Those cells are zero at every call
// site of the reference (R:496-497, R:511-514 and snapshots of such runs), so we require it.
static int check_static_taper_rows(const fdw_ctx* c, const float* f, const char* name)
{
    if (c->xlim >= c->prm.nxe || c->ztap <= 0) return FDW_OK;
    for (int i = c->xlim; i < c->prm.nxe; i++)
        for (int j = 0; j < c->ztap; j++)
            if (f[(size_t)i * c->prm.nze + j] != 0.0f)
                return fail(FDW_EINVAL, "%s[%d][%d] != 0: in compat mode rows >= %d of the damped strip must be zero "
                                        "(they are never time-stepped by the reference, R:185-195)", name, i, j, c->xlim);
    return FDW_OK;
}

// the same precondition for a DEVICE array (fdw_border.hip; declared here rather than in fdw_kernels.h, whose text is part of the kernel-source hash of bench.py)
namespace fdw {
hipError_t launch_static_strip_check(const float* f, int pitch, int row0, int nrows, int ztap, unsigned* flag, hipStream_t s);
}
extern "C" int fdw_dev_check_field(fdw_ctx* c, const float* d_f, void* stream)
{
    if (!c || !d_f) return fail(FDW_EINVAL, "ctx or field is NULL");
    const int row0 = std::max(c->xlim - c->slab.x_off, 0);              // local rows the reference never time-steps
    if (row0 >= c->nxl || c->ztap <= 0) return FDW_OK;                  // nothing to check on this grid / slab
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = pick_stream(c, stream);
    unsigned* d_flag = nullptr;
    HIP_TRY(hipMalloc((void**)&d_flag, sizeof(unsigned)));
    unsigned bad = 0;
    hipError_t e = hipMemsetAsync(d_flag, 0, sizeof(unsigned), s);
    if (e == hipSuccess) e = launch_static_strip_check(d_f, c->pitch, row0, c->nxl - row0, c->ztap, d_flag, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d_flag);
    if (e != hipSuccess) return fail(FDW_EHIP, "fdw_dev_check_field: %s", hipGetErrorString(e));
    if (bad)
        return fail(FDW_EINVAL, "%u cells of the damped strip (columns < %d) are non-zero on rows the reference never time-steps (global rows >= %d): "
                                "in compat mode they must be zero (R:185-195; include/fdwave.h, PRECONDITION)", bad, c->ztap, c->xlim);
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// host-array entry points
// ------------------------------------------------------------------------------------------------
extern "C" int fdw_laplacian(fdw_ctx* c, const float* p, float* lap)
{
    if (!c || !p || !lap) return fail(FDW_EINVAL, "NULL argument");
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_laplacian needs a full-grid context");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_work_buffers(c, 2, false);
    if (rc) return rc;
    if ((rc = upload_rows(c, c->fld[0], p, c->stream))) return rc;
    if ((rc = step_impl(c, FDW_MODE_LAP, c->fld[0], c->fld[1], nullptr, 0, c->nxl, 0, FwdView{}, BackExtra{}, c->stream))) return rc;
    if ((rc = download_rows(c, lap, c->fld[1], c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

// ---- wavefield snapshots (fdw_snap_dims, fdw_dev_snapshot, fdw_shot_snaps; definitions in fdwave.h) ----
static int snap_extent(int n, int dec) { return (n + dec - 1) / dec; }

struct SnapPlan {        // one shot's snapshots: the frame geometry and the device frame stores of the requested sets
    int every = 1, dec = 1, nframes = 0, nxs = 0, nzs = 0;
    float* store[3] = {nullptr, nullptr, nullptr};      // snaps, snaps_rec, snapr: [nframes][nxs][nzs]; NULL = not requested
    size_t frame_elems() const { return (size_t)nxs * (size_t)nzs; }
};

// the interior cells (nxb + a dec, nzb + b dec) of one field as one dense frame [ceil(nx/dec)][ceil(nz/dec)]
static int snapshot(fdw_ctx* c, const float* d_field, int dec, float* d_frame, hipStream_t s)
{
    hipError_t e = launch_snapshot(d_field, d_frame, c->pitch, c->prm.nxb, c->prm.nzb, dec, snap_extent(c->nx, dec), snap_extent(c->nz, dec), s);
    if (e != hipSuccess) return fail(FDW_EHIP, "snapshot launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

static int upload_source(fdw_ctx* c, const float* srce, int n)
{
    int rc = ensure_cap(&c->d_srce, &c->srce_cap, (size_t)std::max(n, 1));
    if (rc) return rc;
    if (n > 0) HIP_TRY(hipMemcpyAsync(c->d_srce, srce, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return FDW_OK;
}

// fd_forward's loop body R:259-267 for nsteps iterations over the context's four field buffers (pairs of steps go through the two-step kernel
// where it pays); *ip / *ipp index (d_p, d_pp) before the loop and after it.  f: the loop's source and extras.  sn (fdw_shot_snaps;
// SnapPlan{}: none): the loop runs in segments that end on the snapshot levels L = every, 2 every, ... (a loop cut at any iteration equals the
// uncut one bit for bit: it0 and the owed-taper flag carry over), and after each the frame of d_pp = u^L goes into the frame store.
static int forward_loop(fdw_ctx* c, int* ip, int* ipp, const Forward& f, int nsteps, const SnapPlan& sn)
{
    FDW_RANGE("fdw: forward loop (fd_forward)");
    int it = 0;
    for (int j = 0; sn.store[0] && j < sn.nframes; j++) {
        const int level = (j + 1) * sn.every;
        FDW_TRY(steps_loop(c, c->fld, c->d_v2, f, it, level - it, it > 0, ip, ipp, c->stream));
        FDW_TRY(snapshot(c, c->fld[*ipp], sn.dec, sn.store[0] + (size_t)j * sn.frame_elems(), c->stream));
        it = level;
    }
    int rc = steps_loop(c, c->fld, c->d_v2, f, it, nsteps - it, it > 0, ip, ipp, c->stream);
    if (rc) return rc;
    if (nsteps > 0) return fdw_dev_taper_finalize(c, c->fld[*ip], c->stream);   // the T() d_p still owes (R:285 downloads the damped d_p)
    return FDW_OK;
}

extern "C" int fdw_forward(fdw_ctx* c, float* p, float* pp, const float* v2, int sx, int sz, const float* srce, int nsteps)
{
    if (!c || !p || !pp || !v2 || (!srce && nsteps > 0)) return fail(FDW_EINVAL, "NULL argument");
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_forward needs a full-grid context");
    if (nsteps < 0) return fail(FDW_EINVAL, "nsteps=%d", nsteps);
    int rc;
    if ((rc = check_static_taper_rows(c, p, "p")) || (rc = check_static_taper_rows(c, pp, "pp"))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ensure_work_buffers(c, 4, false))) return rc;
    int ip = 0, ipp = 1;
    if ((rc = upload_rows(c, c->fld[0], p, c->stream)) || (rc = upload_rows(c, c->fld[1], pp, c->stream)) ||
        (rc = upload_rows(c, c->d_v2, v2, c->stream)) || (rc = upload_source(c, srce, nsteps)))
        return rc;
    if ((rc = forward_loop(c, &ip, &ipp, point_source(c->d_srce, sx, sz), nsteps, SnapPlan{}))) return rc;
    if ((rc = download_rows(c, p, c->fld[ip], c->stream)) || (rc = download_rows(c, pp, c->fld[ipp], c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

// d_obs [nx][nt] (R:426-435) -> device [nt][nx] so that one step's samples are contiguous
static int gathers_to_device(fdw_ctx* c, const float* d_obs, float* d_dst, int nshots)
{
    const size_t n = (size_t)c->nx * c->prm.nt * nshots;
    int rc = ensure_cap(&c->d_raw, &c->raw_cap, n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_raw, d_obs, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipError_t e = launch_gather_transpose(c->d_raw, d_dst, c->nx, c->prm.nt, nshots, c->stream);
    if (e != hipSuccess) return fail(FDW_EHIP, "gather transposition launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}
static int upload_gather(fdw_ctx* c, const float* d_obs)
{
    int rc = ensure_cap(&c->d_dobs, &c->dobs_cap, (size_t)c->nx * c->prm.nt);
    if (rc) return rc;
    return gathers_to_device(c, d_obs, c->d_dobs, 1);
}

// the line-source gather wav [nx][nt] -> c->d_wav [nt][nx] (transposed on the device, like a data gather)
static int upload_line_source(fdw_ctx* c, const float* wav)
{
    int rc = ensure_cap(&c->d_wav, &c->wav_cap, (size_t)c->nx * c->prm.nt);
    if (rc) return rc;
    return gathers_to_device(c, wav, c->d_wav, 1);
}

static int image_to_device(fdw_ctx* c, const float* imloc, float* d_dst)
{
    HIP_TRY(hipMemsetAsync(d_dst, 0, field_elems(c) * sizeof(float), c->stream));
    float* dst = d_dst + (size_t)c->prm.nxb * c->pitch + c->prm.nzb;
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)c->pitch * sizeof(float), imloc, (size_t)c->nz * sizeof(float),
                             (size_t)c->nz * sizeof(float), c->nx, hipMemcpyHostToDevice, c->stream));
    return FDW_OK;
}
static int image_to_host(fdw_ctx* c, float* imloc, const float* d_src)
{
    const float* src = d_src + (size_t)c->prm.nxb * c->pitch + c->prm.nzb;
    HIP_TRY(hipMemcpy2DAsync(imloc, (size_t)c->nz * sizeof(float), src, (size_t)c->pitch * sizeof(float),
                             (size_t)c->nz * sizeof(float), c->nx, hipMemcpyDeviceToHost, c->stream));
    return FDW_OK;
}

// fd_back's loop R:302-339 on device buffers.
//   F_k  = source wavefield of iteration k:  F_0 = snap1 (u^nt), F_1 = snap0 (u^{nt-1}, R:304-314),
//          F_k = leap-frog(F_{k-1}, F_{k-2}) for k >= 2 (no taper, no source, R:317-318)
//   r^k  = receiver field: r^{k+1} = damped leap-frog(r^k, r^{k-1}) + d_obs[.][nt-1-k] on row gz (R:325-328)
//   img += F_k * r^{k+1}  (R:329)
// Iterations go four at a time through the wave pipeline where it pays (back4), in PAIRS through the two-step kernel where that pays (one
// pass reconstructs F_k, F_{k+1}; one pass advances the receiver field twice and applies both imaging conditions), singly through the
// one-step kernels otherwise (back_iter).  src[0..3] / rcv[0..3]: rotating buffers; on entry src[0] = snap0, src[1] = snap1, the receivers
// are zero.
// sn (fdw_shot_snaps; SnapPlan{}: none): iterations k = nt - L of the snapshot levels L are STOPS: no pass of several iterations reaches across one (the
// family is chosen by the iterations left until the next stop; every family equals the one-step iteration bit for bit, so the image
// does not change), and after iteration k the frames of F_k and r^{k+1} go into the frame stores at index L / every - 1.
// dtt (fdw_shot_dtt and its kin): single iterations of back_iter_dtt -- no pairs, no pipeline -- and the tail of two source-only
// reconstructions into the spare source buffers with their two image terms (fdwave.h, "DTT imaging").
// ext_H >= 0 (fdw_shot_ext): single iterations of back_iter too, and after iteration k the term F_k, r^{k+1} of the extended image into the
// planes d_eimg (fdwave.h, "Extended imaging").
static int back_loop(fdw_ctx* c, float* const src[4], float* const rcv[4], int gz, int nsteps, const SnapPlan& sn, bool dtt = false, int ext_H = -1,
                     float* d_eimg = nullptr)
{
    FDW_RANGE("fdw: backward loop + imaging (fd_back)");
    const int nt = c->prm.nt;
    const size_t nxs = (size_t)c->nx;
    auto samples = [&](int it) { return c->d_dobs + (size_t)(nt - 1 - it) * nxs; };
    int f1 = 0, f0 = 1;          // indices into src of F_{k-1} (newer) and F_{k-2}: before iteration 2 these are snap0, snap1
    int rn = 0, ro = 1;          // indices into rcv of r^k (d_pr) and r^{k-1} (d_ppr)
    int it = 0;
    const bool single = dtt || ext_H >= 0;
    const bool pairs = two_step_pays(c) && !single;
    const bool pipe = fdw_back_pipe_active(c) && c->nbatch <= 1 && !single;
    if (dtt) FDW_TRY(ensure_dtt_scratch(c));
    std::vector<int> stops;      // ascending iterations after which frames are taken
    if (sn.store[1] || sn.store[2])
        for (int j = sn.nframes - 1; j >= 0; j--)
            if (nt - (j + 1) * sn.every < nsteps) stops.push_back(nt - (j + 1) * sn.every);
    size_t next = 0;             // stops[next] = the first stop not yet passed
    if (pipe && c->no_back_fused && nsteps >= 2 + kPipeSteps) {      // the two-pass form keeps two levels in memory
        FDW_TRY(alloc_zero(&c->fld[8], field_elems(c)));
        FDW_TRY(alloc_zero(&c->fld[9], field_elems(c)));
    }
    while (it < nsteps) {
        const int left = (next < stops.size() ? stops[next] + 1 : nsteps) - it;      // iterations until the next stop (or the end)
        if (pipe && it >= 2 && left >= kPipeSteps) {
            int o1, o2, q1, q2;
            spare_pair(f1, f0, &o1, &o2);
            spare_pair(rn, ro, &q1, &q2);
            // iteration it+1 reads the sample row before (time-reversed traces, R:328)
            FDW_TRY(back4(c, src[f1], src[f0], src[o1], src[o2], c->fld[8], c->fld[9], rcv[rn], rcv[ro], rcv[q1], rcv[q2], c->d_v2, samples(it),
                          -(int)nxs, gz, c->d_img, it > 0, RowRanges{}, c->stream));
            f0 = o1; f1 = o2;
            ro = q1; rn = q2;
            it += kPipeSteps;
        } else if (pairs && left >= 2 && it != 1) {      // (it = 1 only after a stop at iteration 0: F_1 is still a snapshot, a pair would reconstruct it)
            const float *Fa, *Fb;   // source fields of iterations it, it+1
            if (it == 0) {
                Fa = src[1]; Fb = src[0];                      // u^nt, u^{nt-1}
            } else {
                int o1, o2;
                spare_pair(f1, f0, &o1, &o2);
                FDW_TRY(step2_impl(c, FDW_MODE_PLAIN, src[f1], src[f0], c->d_v2, src[o1], src[o2], 0, FwdView{}, BackExtra{}, c->stream));
                Fa = src[o1]; Fb = src[o2];
                f0 = o1; f1 = o2;
            }
            int q1, q2;
            spare_pair(rn, ro, &q1, &q2);
            BackExtra ex;
            ex.inj2 = samples(it + 1); ex.psrc_a = Fa; ex.psrc_b = Fb; ex.img = c->d_img;
            FDW_TRY(step2_impl(c, FDW_MODE_RECV, rcv[rn], rcv[ro], c->d_v2, rcv[q1], rcv[q2], it > 0, receiver_samples(samples(it), gz), ex, c->stream));
            ro = q1; rn = q2;
            it += 2;
        } else {
            // iteration 0 images u^nt, iteration 1 u^{nt-1}; from iteration 2 on F_k overwrites F_{k-2}
            FDW_TRY((dtt ? back_iter_dtt : back_iter)(c, it >= 2, it == 0 ? src[f0] : src[f1], src[f0], rcv[rn], rcv[ro], c->d_v2, 0, c->nxl, it > 0, samples(it), gz,
                                                      c->d_img, c->stream));
            if (it >= 2) std::swap(f1, f0);
            std::swap(rn, ro);
            // F_k: u^nt (src[1]) at k = 0, then the newer of the source pair; r^{k+1}: the newer receiver field
            if (ext_H >= 0) FDW_TRY(ext_image(c, it == 0 ? src[1] : src[f1], rcv[rn], ext_H, d_eimg, c->stream));
            it += 1;
        }
        if (next < stops.size() && it == stops[next] + 1) {
            // F_k: u^nt (src[1]) at k = 0, then the newer of the source pair (k = 1: the handed-over P in src[0]); r^{k+1}: the newer receiver field
            const int k = stops[next++];
            const size_t off = (size_t)((nt - k) / sn.every - 1) * sn.frame_elems();
            if (sn.store[1]) FDW_TRY(snapshot(c, k == 0 ? src[1] : src[f1], sn.dec, sn.store[1] + off, c->stream));
            if (sn.store[2]) FDW_TRY(snapshot(c, rcv[rn], sn.dec, sn.store[2] + off, c->stream));
        }
    }
    if (dtt && nsteps >= 1) {
        // the tail: terms k = nsteps-2 (with r^{nsteps-1}) and k = nsteps-1 (with r^{nsteps}), in that order; nsteps = 1: term 0 alone.  Each
        // needs one more level of the source field: the plain leap-frog (R:317-318) into a spare buffer, the three levels kept side by side.
        int o[2];
        spare_pair(f1, f0, &o[0], &o[1]);
        const size_t bytes = field_elems(c) * (size_t)std::max(c->nbatch, 1) * sizeof(float);
        const float* lvl[4] = {src[f0], src[f1], nullptr, nullptr};      // F_{nsteps-2}, F_{nsteps-1} (nsteps = 1: the snapshots F_0, F_1)
        const float* r[2] = {rcv[ro], rcv[rn]};
        const int nterms = nsteps >= 2 ? 2 : 1;
        for (int t = 0; t < nterms; t++) {
            HIP_TRY(hipMemcpyAsync(src[o[t]], lvl[t], bytes, hipMemcpyDeviceToDevice, c->stream));
            FDW_TRY(step_impl(c, FDW_MODE_PLAIN, lvl[t + 1], src[o[t]], c->d_v2, 0, c->nxl, 0, FwdView{}, BackExtra{}, c->stream));
            lvl[t + 2] = src[o[t]];
            FDW_TRY(dtt_image(c, lvl[t], lvl[t + 1], lvl[t + 2], r[nterms == 2 ? t : 1], c->d_img, 0, c->stream));
        }
    }
    return FDW_OK;
}

static int zero_fields(fdw_ctx* c, float* const f[], int n)
{
    for (int i = 0; i < n; i++) HIP_TRY(hipMemsetAsync(f[i], 0, field_elems(c) * sizeof(float), c->stream));
    return FDW_OK;
}

// the backward loop's source-field buffers after the forward loop: the snapshots where it left them (fld[ip], fld[ipp]), then the other two
// of the first four
static void source_buffers(const fdw_ctx* c, int ip, int ipp, float* src[4])
{
    int o1, o2;
    spare_pair(ip, ipp, &o1, &o2);
    src[0] = c->fld[ip]; src[1] = c->fld[ipp]; src[2] = c->fld[o1]; src[3] = c->fld[o2];
}

extern "C" int fdw_back(fdw_ctx* c, const float* v2, const float* snap0, const float* snap1, const float* d_obs, int gz,
                        float* imloc, int nsteps)
{
    if (!c || !v2 || !snap0 || !snap1 || !d_obs || !imloc) return fail(FDW_EINVAL, "NULL argument");
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_back needs a full-grid context");
    if (nsteps < 0 || nsteps > c->prm.nt) return fail(FDW_EINVAL, "nsteps=%d outside [0,nt=%d]", nsteps, c->prm.nt);
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "no interior to image");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_work_buffers(c, 8, true))) return rc;
    if ((rc = upload_rows(c, c->d_v2, v2, c->stream)) || (rc = upload_gather(c, d_obs)) || (rc = image_to_device(c, imloc, c->d_img))) return rc;
    // the reference uploads the two snapshots into d_pp at it = 0 and 1 (R:304-314); having both on the device up front is the same
    if ((rc = upload_rows(c, c->fld[0], snap0, c->stream)) || (rc = upload_rows(c, c->fld[1], snap1, c->stream))) return rc;
    if ((rc = zero_fields(c, c->fld + 4, 2))) return rc;             // R:513-514
    if ((rc = back_loop(c, c->fld, c->fld + 4, gz, nsteps, SnapPlan{}))) return rc;
    if ((rc = image_to_host(c, imloc, c->d_img))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

static int gathers_to_host(fdw_ctx* c, const float* d_rec, int nshots, float* data);

// The squared model of a call is the caller's v2 or (v2 == NULL) the resident one (fdw_dev_extendvel_linear); a caller's v2 ends the residency
// once the entry point has accepted its arguments.
static int has_model(const fdw_ctx* c, const float* v2) { return v2 || c->v2_resident ? FDW_OK : fail(FDW_ESTATE, "no resident squared model: call fdw_dev_extendvel_linear first"); }
static void end_residency(fdw_ctx* c, const float* v2) { if (v2) c->v2_resident = false; }

struct ShotExtras {      // what a shot does beyond fdw_shot's; of a batch every array is [nshots][...]
    bool line = false;         // fdw_shot_line: `samples` is the line-source gather [nx][nt] on column sz in place of the wavelet [nt]; sx is unused
    float* illum = nullptr;    // the interior illumination [nx][nz] the forward loop accumulates into (fdw_shot_illum)
    SnapPlan snaps;            // one shot: the snapshot plan of fdw_shot_snaps (frame stores already allocated)
    bool residual = false;     // fdw_shot_residual: the forward loop records the modelled gather (c->d_rec; a batch: b_rec [shot][nt][nx]), which turns
    float* resid = nullptr;    // the data gather into d_obs - d_mod in place before the backward loop reads it; resid: NULL, or [nx][nt] that difference
    bool dtt = false;          // fdw_shot_dtt and its kin: the backward loop images with the second time difference of the source field (back_loop)
    int ext_H = -1;            // fdw_shot_ext: >= 0, the half-width of the extended image the backward loop accumulates into c->d_eimg; imloc may be NULL
    ShotExtras of_shot(size_t b, size_t ni, size_t ng) const { ShotExtras x = *this; if (illum) x.illum += b * ni; if (resid) x.resid += b * ng; return x; }
};
// the uploaded source as the forward loop takes it: the wavelet in c->d_srce, or (line) the gathers transposed to [shot][nt][nx] in d_wav
static Forward device_source(const fdw_ctx* c, bool line, int sx, int sz, const float* d_wav) { return line ? line_source(d_wav, sz) : point_source(c->d_srce, sx, sz); }

// v2 == nullptr: the squared model already resident in c->d_v2
static int shot_impl(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* samples, const float* d_obs, float* imloc, float* P, float* PP,
                     const ShotExtras& x)
{
    if (!c || !samples || !d_obs || (!imloc && x.ext_H < 0)) return fail(FDW_EINVAL, "NULL argument");
    if (x.residual) FDW_TRY(check_record_depth(c, gz));
    FDW_RANGE("fdw: shot (uploads, forward, backward, image download)");
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_shot needs a full-grid context");
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "no interior to image");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    const int nt = c->prm.nt;
    if ((rc = ensure_work_buffers(c, 8, true))) return rc;
    int ip = 0, ipp = 1;
    HIP_TRY(hipMemsetAsync(c->fld[0], 0, field_elems(c) * sizeof(float), c->stream));    // R:496-497
    HIP_TRY(hipMemsetAsync(c->fld[1], 0, field_elems(c) * sizeof(float), c->stream));
    if ((v2 && (rc = upload_rows(c, c->d_v2, v2, c->stream))) || (rc = x.line ? upload_line_source(c, samples) : upload_source(c, samples, nt)) ||
        (rc = upload_gather(c, d_obs)) || (rc = imloc ? image_to_device(c, imloc, c->d_img) : zero_fields(c, &c->d_img, 1)))
        return rc;
    if (x.illum && ((rc = alloc_zero(&c->d_illum, field_elems(c))) || (rc = image_to_device(c, x.illum, c->d_illum)))) return rc;
    if (x.residual && (rc = ensure_cap(&c->d_rec, &c->rec_cap, (size_t)c->nx * nt))) return rc;
    const Forward f = device_source(c, x.line, sx, sz, c->d_wav).recording(x.residual ? c->d_rec : nullptr, gz).illuminating(x.illum ? c->d_illum : nullptr);
    if ((rc = forward_loop(c, &ip, &ipp, f, nt, x.snaps))) return rc;
    if (x.residual) {      // both [nt][nx] in forward time: the backward loop's sample indexing stays as it is
        if ((rc = gather_residual(c->d_dobs, c->d_rec, c->d_dobs, (size_t)c->nx * nt, c->stream))) return rc;
        if (x.resid && (rc = gathers_to_host(c, c->d_dobs, 1, x.resid))) return rc;
    }
    if (x.illum && (rc = image_to_host(c, x.illum, c->d_illum))) return rc;
    if (P && (rc = download_rows(c, P, c->fld[ip], c->stream))) return rc;
    if (PP && (rc = download_rows(c, PP, c->fld[ipp], c->stream))) return rc;
    float* src[4];
    source_buffers(c, ip, ipp, src);
    if ((rc = zero_fields(c, c->fld + 4, 2))) return rc;
    if ((rc = back_loop(c, src, c->fld + 4, gz, nt, x.snaps, x.dtt, x.ext_H, c->d_eimg))) return rc;
    if (imloc && (rc = image_to_host(c, imloc, c->d_img))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

extern "C" int fdw_shot(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, const float* d_obs,
                        float* imloc, float* P, float* PP)
{
    if (!v2) return fail(FDW_EINVAL, "NULL argument");
    if (c) c->v2_resident = false;
    return shot_impl(c, v2, sx, sz, gz, srce, d_obs, imloc, P, PP, ShotExtras{});
}

extern "C" int fdw_shot_illum(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, const float* d_obs, float* imloc,
                              float* illum, float* P, float* PP)
{
    if (!c || !v2 || !illum) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "source illumination", "fdw_shot_illum"));
    c->v2_resident = false;
    ShotExtras x;
    x.illum = illum;
    return shot_impl(c, v2, sx, sz, gz, srce, d_obs, imloc, P, PP, x);
}

// ---- wavefield snapshots ----
extern "C" int fdw_snap_dims(int nx, int nz, int nt, int every, int dec, int* nframes, int* nxs, int* nzs)
{
    if (every < 1 || dec < 1) return fail(FDW_EINVAL, "snapshots: every=%d and dec=%d must both be >= 1", every, dec);
    if (nx < 0 || nz < 0 || nt < 0) return fail(FDW_EINVAL, "snapshots: nx=%d nz=%d nt=%d", nx, nz, nt);
    if (nframes) *nframes = nt / every;
    if (nxs) *nxs = snap_extent(nx, dec);
    if (nzs) *nzs = snap_extent(nz, dec);
    return FDW_OK;
}

extern "C" int fdw_dev_snapshot(fdw_ctx* c, const float* d_field, int dec, float* d_frame, void* stream)
{
    if (!c || !d_field || !d_frame) return fail(FDW_EINVAL, "NULL argument");
    if (dec < 1) return fail(FDW_EINVAL, "snapshot: dec=%d must be >= 1", dec);
    FDW_TRY(check_single_shot_ctx(c, "wavefield snapshots", "fdw_dev_snapshot"));
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "no interior to take a frame of");
    return snapshot(c, d_field, dec, d_frame, pick_stream(c, stream));
}

extern "C" int fdw_shot_snaps(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, const float* d_obs, float* imloc, float* illum,
                              float* P, float* PP, const fdw_snaps* snaps)
{
    if (!c || !snaps) return fail(FDW_EINVAL, "NULL argument");
    float* const host[3] = {snaps->snaps, snaps->snaps_rec, snaps->snapr};
    if (!host[0] && !host[1] && !host[2]) return fail(FDW_EINVAL, "fdw_shot_snaps: none of snaps, snaps_rec, snapr is requested");
    SnapPlan plan;
    plan.every = snaps->every; plan.dec = snaps->dec;
    FDW_TRY(fdw_snap_dims(c->nx, c->nz, c->prm.nt, snaps->every, snaps->dec, &plan.nframes, &plan.nxs, &plan.nzs));
    FDW_TRY(check_single_shot_ctx(c, "wavefield snapshots", "fdw_shot_snaps"));
    FDW_TRY(has_model(c, v2));
    if (!srce || !d_obs || !imloc) return fail(FDW_EINVAL, "NULL argument");
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "no interior to image");
    HIP_TRY(hipSetDevice(c->device));
    // the frame stores, before anything is enqueued
    const size_t set_elems = (size_t)plan.nframes * plan.frame_elems();
    int nsets = 0;
    for (int i = 0; i < 3; i++) nsets += host[i] != nullptr;
    FDW_TRY(ensure_work_buffers(c, 8, true));
    for (int i = 0; i < 3 && set_elems > 0; i++) {
        if (!host[i]) continue;
        if (ensure_cap(&c->d_snap[i], &c->snap_cap[i], set_elems) != FDW_OK) {
            size_t free_b = 0, total_b = 0;
            (void)hipMemGetInfo(&free_b, &total_b);
            return fail(FDW_ENOMEM, "fdw_shot_snaps: the frame stores do not fit: %d sets x %d frames x %zu bytes = %zu bytes, %zu bytes free on the device",
                        nsets, plan.nframes, plan.frame_elems() * sizeof(float), (size_t)nsets * set_elems * sizeof(float), free_b);
        }
        plan.store[i] = c->d_snap[i];
    }
    end_residency(c, v2);
    ShotExtras x;
    x.illum = illum; x.snaps = plan;
    FDW_TRY(shot_impl(c, v2, sx, sz, gz, srce, d_obs, imloc, P, PP, x));
    // one download per set (shot_impl has synchronised: the copies below are the only work left on the stream)
    for (int i = 0; i < 3; i++)
        if (plan.store[i]) HIP_TRY(hipMemcpyAsync(host[i], plan.store[i], set_elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// recorded shot gathers of the RTM dialect (the data rtm_code migrates, R:420-424)
// ------------------------------------------------------------------------------------------------
// d_rec [nshots][nt][nx] -> data [nshots][nx][nt] (the layout of rtm_code's datfile; fd_back reads d_obs[ix][nt-1-it], R:328)
static int gathers_to_host(fdw_ctx* c, const float* d_rec, int nshots, float* data)
{
    const size_t n = (size_t)c->nx * c->prm.nt * nshots;
    if (n == 0) return FDW_OK;
    FDW_TRY(ensure_cap(&c->d_raw, &c->raw_cap, n));
    hipError_t e = launch_gather_transpose(d_rec, c->d_raw, c->prm.nt, c->nx, nshots, c->stream);
    if (e != hipSuccess) return fail(FDW_EHIP, "gather transposition launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(data, c->d_raw, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return FDW_OK;
}

// fd_forward from rest (R:496-497, R:259-267) recording data[ix][it] = d_pp(nxb + ix, gz) at the end of iteration it.  v2 == nullptr: the
// squared model already resident in c->d_v2 (fdw_dev_extendvel_linear).
static int record_impl(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* samples, float* data, float* P, float* PP, bool line)
{
    if (!c || !samples || !data) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_record_depth(c, gz));
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_record_shot needs a full-grid context");
    if (c->nx <= 0) return fail(FDW_EINVAL, "no receiver rows");
    HIP_TRY(hipSetDevice(c->device));
    const int nt = c->prm.nt;
    FDW_TRY(ensure_work_buffers(c, 4, false));
    FDW_TRY(ensure_cap(&c->d_rec, &c->rec_cap, (size_t)c->nx * nt));
    HIP_TRY(hipMemsetAsync(c->fld[0], 0, field_elems(c) * sizeof(float), c->stream));
    HIP_TRY(hipMemsetAsync(c->fld[1], 0, field_elems(c) * sizeof(float), c->stream));
    if (v2) FDW_TRY(upload_rows(c, c->d_v2, v2, c->stream));
    FDW_TRY(line ? upload_line_source(c, samples) : upload_source(c, samples, nt));
    int ip = 0, ipp = 1;
    FDW_TRY(forward_loop(c, &ip, &ipp, device_source(c, line, sx, sz, c->d_wav).recording(c->d_rec, gz), nt, SnapPlan{}));
    FDW_TRY(gathers_to_host(c, c->d_rec, 1, data));
    if (P) FDW_TRY(download_rows(c, P, c->fld[ip], c->stream));
    if (PP) FDW_TRY(download_rows(c, PP, c->fld[ipp], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

extern "C" int fdw_record_shot(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, float* data, float* P, float* PP)
{
    if (!v2) return fail(FDW_EINVAL, "NULL argument");
    if (c) c->v2_resident = false;
    return record_impl(c, v2, sx, sz, gz, srce, data, P, PP, false);
}

// ------------------------------------------------------------------------------------------------
// Born modelling (definitions in fdwave.h)
// ------------------------------------------------------------------------------------------------
static bool born_fused(const fdw_ctx* c) { return c->h <= kMaxFastHalfOrder && !c->use_generic && !c->no_born_fused; }

// what fdw_dev_born_steps and fdw_born_shot ask of their arguments beyond the pointers
static int check_born_args(const fdw_ctx* c, const char* who, int kind, int sx, int sz, int gz)
{
    if (kind != FDW_BORN_FIELD && kind != FDW_BORN_DTT) return fail(FDW_EINVAL, "%s: kind=%d is neither FDW_BORN_FIELD nor FDW_BORN_DTT", who, kind);
    if (sz < 0 || sz >= c->zlim) return fail(FDW_EINVAL, "%s: source depth %d outside the time-stepped columns [0,%d)", who, sz, c->zlim);
    if (sx < 0 || sx >= c->upd_x1) return fail(FDW_EINVAL, "%s: source row %d outside the time-stepped rows [0,%d)", who, sx, c->upd_x1);
    if (gz < 0 || gz >= c->zlim) return fail(FDW_EINVAL, "%s: receiver depth %d outside the time-stepped columns [0,%d)", who, gz, c->zlim);
    return FDW_OK;
}

// One iteration in ONE launch of the register-ring family (FDW_MODE_BORN; a line source: FDW_MODE_BORN_LINE): the pairs as the swap left
// them, f the source's view at this iteration, rec / rec0 this iteration's trace rows (either may be NULL).  Inside a batch the launch covers
// every shot: fields, models, sources and trace rows strided as step_impl strides them, the reflectivity shared.
static int born_step_fused(fdw_ctx* c, const float* d_u_p, float* d_u_pp, const float* d_du_p, float* d_du_pp, const float* d_v2, const float* d_m, int kind,
                           const FwdView& f, int gz, float* rec, float* rec0, int pp_twice, hipStream_t s)
{
    StepArgs a{};
    fill_common(c, a, d_u_p, d_u_pp, d_v2, pp_twice);
    a.psrc = d_du_p; a.fpp = d_du_pp;
    a.img = const_cast<float*>(d_m);      // only read
    a.r0 = 0;
    a.r1 = std::min(c->nxl, c->upd_x1);
    Injection in;
    FDW_TRY(place_injection(c, "Born modelling", FDW_MODE_FWD, f, &in));
    a.inj = f.samples + in.shift; a.inj_x = in.x; a.inj_z = f.sz; a.inj_n = in.n;
    fill_rec(c, a, rec, gz);
    a.texc = reinterpret_cast<int*>(rec0);      // the background's trace row travels where the excitation modes carry their map
    const BornCells C = born_cells(c);
    a.img_z1 = C.z1; a.exc_key = born_key(kind, C.z0);      // the rows of C: the receiver rows the launch covers
    if (a.r1 <= a.r0) return FDW_OK;
    if (c->nbatch > 1) {      // fdw_born_shot_batch / fdw_born_shot_line_batch: step_impl's strides; both trace rows advance by rec_bstride
        a.nbatch = c->nbatch;
        a.bstride = a.v2_bstride = (long long)field_elems(c);
        a.inj_bstride = f.line ? (long long)c->nx * c->batch_nt : 0;
        a.inj_dx = f.line ? 0 : c->batch_dsx;
        a.rec_bstride = (long long)c->nx * c->batch_nt;
    }
    fill_geometry(c, a, a.r1 - a.r0, std::max(c->nbatch, 1));
    hipError_t e = launch_step_fast(a, c->h, f.line ? FDW_MODE_BORN_LINE : FDW_MODE_BORN, effective_prefetch(c), s);
    if (e != hipSuccess) return fail(FDW_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

// The loop of fdw_dev_born_steps / fdw_dev_born_line_steps behind its checks; src: the point or the line source of the background pair.
// Without the fused kernel: the scattered pair's step, (A - B) of the background into the scratch field (FDW_BORN_DTT: the background step
// overwrites B), the background step, the scatter kernel with the trace samples.
static int born_loop(fdw_ctx* c, float* d_u_p, float* d_u_pp, float* d_du_p, float* d_du_pp, const float* d_v2, const float* d_m, int kind,
                     const Forward& src, int gz, float* d_rec, float* d_rec0, int it0, int nsteps, int first_pp_twice, hipStream_t s)
{
    const int sz = src.sz;
    const bool fused = born_fused(c);
    if (!fused && kind == FDW_BORN_DTT && !c->d_born_w) {      // every word read is written first: no memset, nothing to wait for
        hipError_t e = hipMalloc((void**)&c->d_born_w, field_elems(c) * sizeof(float));
        if (e != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc(%zu bytes) failed: %s", field_elems(c) * sizeof(float), hipGetErrorString(e));
    }
    if (d_rec) FDW_TRY(record_static(c, d_du_p, d_du_pp, gz, d_rec, it0, nsteps, s));
    if (d_rec0) FDW_TRY(record_static(c, d_u_p, d_u_pp, gz, d_rec0, it0, nsteps, s));
    const BornCells C = born_cells(c);
    const size_t nx = (size_t)c->nx;
    for (int k = 0; k < nsteps; k++) {
        std::swap(d_u_p, d_u_pp);      // R:260-262, both pairs
        std::swap(d_du_p, d_du_pp);
        const int twice = (k > 0) || first_pp_twice;
        const FwdView f = view_at(src, it0 + k, c->nx);
        float* rec = d_rec ? d_rec + (size_t)(it0 + k) * nx : nullptr;
        float* rec0 = d_rec0 ? d_rec0 + (size_t)(it0 + k) * nx : nullptr;
        if (fused) {
            FDW_TRY(born_step_fused(c, d_u_p, d_u_pp, d_du_p, d_du_pp, d_v2, d_m, kind, f, gz, rec, rec0, twice, s));
            continue;
        }
        FDW_TRY(step_impl(c, FDW_MODE_FWD, d_du_p, d_du_pp, d_v2, 0, c->nxl, twice, view_at(point_source(nullptr, -1, sz), 0, c->nx), BackExtra{}, s));
        hipError_t e = hipSuccess;
        if (kind == FDW_BORN_DTT) e = launch_born_diff(d_u_p, d_u_pp, c->d_born_w, c->pitch, C.x0, C.x1, C.z0, C.z1, s);
        if (e != hipSuccess) return fail(FDW_EHIP, "Born difference launch failed: %s", hipGetErrorString(e));
        FDW_TRY(step_impl(c, FDW_MODE_FWD, d_u_p, d_u_pp, d_v2, 0, c->nxl, twice, f, BackExtra{}, s));
        e = launch_born_scatter(d_u_pp, d_u_p, c->d_born_w, d_m, d_du_pp, kind, c->pitch, C.x0, C.x1, C.z0, C.z1, c->upd_z1, gz, rec, rec0, s);
        if (e != hipSuccess) return fail(FDW_EHIP, "Born scatter launch failed: %s", hipGetErrorString(e));
    }
    return FDW_OK;
}

extern "C" int fdw_dev_born_steps(fdw_ctx* c, float* d_u_p, float* d_u_pp, float* d_du_p, float* d_du_pp, const float* d_v2, const float* d_m, int kind,
                                  const float* d_srce, int sx, int sz, int gz, float* d_rec, float* d_rec0, int it0, int nsteps, int first_pp_twice,
                                  void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_single_shot_ctx(c, "Born modelling", "fdw_dev_born_steps"));
    if (!d_u_p || !d_u_pp || !d_du_p || !d_du_pp || !d_v2 || !d_m || !d_srce) return fail(FDW_EINVAL, "fdw_dev_born_steps: NULL argument");
    if (it0 < 0 || nsteps < 0) return fail(FDW_EINVAL, "fdw_dev_born_steps: it0=%d nsteps=%d", it0, nsteps);
    FDW_TRY(check_born_args(c, "fdw_dev_born_steps", kind, sx, sz, gz));
    return born_loop(c, d_u_p, d_u_pp, d_du_p, d_du_pp, d_v2, d_m, kind, point_source(d_srce, sx, sz), gz, d_rec, d_rec0, it0, nsteps, first_pp_twice,
                     pick_stream(c, stream));
}

extern "C" int fdw_dev_born_line_steps(fdw_ctx* c, float* d_u_p, float* d_u_pp, float* d_du_p, float* d_du_pp, const float* d_v2, const float* d_m, int kind,
                                       const float* d_wav, int sz, int gz, float* d_rec, float* d_rec0, int it0, int nsteps, int first_pp_twice, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_single_shot_ctx(c, "Born modelling", "fdw_dev_born_line_steps"));
    if (!d_u_p || !d_u_pp || !d_du_p || !d_du_pp || !d_v2 || !d_m || !d_wav) return fail(FDW_EINVAL, "fdw_dev_born_line_steps: NULL argument");
    if (it0 < 0 || nsteps < 0) return fail(FDW_EINVAL, "fdw_dev_born_line_steps: it0=%d nsteps=%d", it0, nsteps);
    FDW_TRY(check_born_args(c, "fdw_dev_born_line_steps", kind, 0, sz, gz));      // a line has no source row
    return born_loop(c, d_u_p, d_u_pp, d_du_p, d_du_pp, d_v2, d_m, kind, line_source(d_wav, sz), gz, d_rec, d_rec0, it0, nsteps, first_pp_twice,
                     pick_stream(c, stream));
}

// fdw_born_shot (samples: the wavelet [nt]) / fdw_born_shot_line (line: the gather [nx][nt], sx unused)
static int born_shot_impl(fdw_ctx* c, const char* who, const float* v2, const float* m, int kind, int sx, int sz, int gz, const float* samples, float* data,
                          float* data0, bool line)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_single_shot_ctx(c, "Born modelling", who));
    if (!m || !samples || !data) return fail(FDW_EINVAL, "%s: NULL argument", who);
    FDW_TRY(has_model(c, v2));
    FDW_TRY(check_born_args(c, who, kind, line ? 0 : sx, sz, gz));
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "%s: no interior", who);
    HIP_TRY(hipSetDevice(c->device));
    const int nt = c->prm.nt;
    FDW_TRY(ensure_work_buffers(c, 4, false));
    FDW_TRY(alloc_zero(&c->d_born_m, field_elems(c)));
    FDW_TRY(ensure_cap(&c->d_rec, &c->rec_cap, (size_t)c->nx * nt));
    if (data0) FDW_TRY(ensure_cap(&c->d_born_rec0, &c->born_rec0_cap, (size_t)c->nx * nt));
    FDW_TRY(zero_fields(c, c->fld, 4));
    end_residency(c, v2);
    if (v2) FDW_TRY(upload_rows(c, c->d_v2, v2, c->stream));
    FDW_TRY(line ? upload_line_source(c, samples) : upload_source(c, samples, nt));
    FDW_TRY(image_to_device(c, m, c->d_born_m));
    FDW_TRY(born_loop(c, c->fld[0], c->fld[1], c->fld[2], c->fld[3], c->d_v2, c->d_born_m, kind, device_source(c, line, sx, sz, c->d_wav), gz, c->d_rec,
                      data0 ? c->d_born_rec0 : nullptr, 0, nt, 0, c->stream));
    FDW_TRY(gathers_to_host(c, c->d_rec, 1, data));
    if (data0) FDW_TRY(gathers_to_host(c, c->d_born_rec0, 1, data0));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

extern "C" int fdw_born_shot(fdw_ctx* c, const float* v2, const float* m, int kind, int sx, int sz, int gz, const float* srce, float* data, float* data0)
{
    return born_shot_impl(c, "fdw_born_shot", v2, m, kind, sx, sz, gz, srce, data, data0, false);
}

extern "C" int fdw_born_shot_line(fdw_ctx* c, const float* v2, const float* m, int kind, int sz, int gz, const float* wav, float* data, float* data0)
{
    return born_shot_impl(c, "fdw_born_shot_line", v2, m, kind, -1, sz, gz, wav, data, data0, true);
}

// ---- shots driven by a line source (definitions in fdwave.h) ----
extern "C" int fdw_shot_line(fdw_ctx* c, const float* v2, int sz, int gz, const float* wav, const float* d_obs, float* imloc, float* illum, float* P,
                             float* PP)
{
    if (!c || !wav) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "line sources", "fdw_shot_line"));
    FDW_TRY(has_model(c, v2));
    FDW_TRY(check_line_args(c, "fdw_shot_line", sz, gz, false, illum != nullptr));
    end_residency(c, v2);
    ShotExtras x;
    x.line = true; x.illum = illum;
    return shot_impl(c, v2, -1, sz, gz, wav, d_obs, imloc, P, PP, x);
}

extern "C" int fdw_record_shot_line(fdw_ctx* c, const float* v2, int sz, int gz, const float* wav, float* data, float* P, float* PP)
{
    if (!c || !wav) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "line sources", "fdw_record_shot_line"));
    FDW_TRY(has_model(c, v2));
    FDW_TRY(check_line_args(c, "fdw_record_shot_line", sz, gz, true, false));
    end_residency(c, v2);
    return record_impl(c, v2, -1, sz, gz, wav, data, P, PP, true);
}

// fdw_shot_line that migrates d_obs - d_mod, d_mod the gather its own forward loop records (fdw_record_shot_line's, bit for bit); with illum
// the forward loop runs the combined line-source kernels
extern "C" int fdw_shot_line_residual(fdw_ctx* c, const float* v2, int sz, int gz, const float* wav, const float* d_obs, float* imloc, float* illum,
                                      float* resid, float* P, float* PP)
{
    if (!c || !wav) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "line sources", "fdw_shot_line_residual"));
    FDW_TRY(has_model(c, v2));
    FDW_TRY(check_line_args(c, "fdw_shot_line_residual", sz, gz, true, illum != nullptr, true));
    end_residency(c, v2);
    ShotExtras x;
    x.line = true; x.illum = illum; x.residual = true; x.resid = resid;
    return shot_impl(c, v2, -1, sz, gz, wav, d_obs, imloc, P, PP, x);
}

// The encoded data gather on the device (fdw_encode_gathers_kernel): every output element folds its shots in ascending order.
extern "C" int fdw_encode_gathers(int device, int nshots, const int* lag, const float* weight, const float* d_obs_all, int nx, int nt, float* out)
{
    if (nshots < 0 || nx < 1 || nt < 1 || nx > 65535 || !out || (nshots > 0 && (!lag || !weight || !d_obs_all))) return fail(FDW_EINVAL, "encode_gathers: bad argument");
    for (int s = 0; s < nshots; s++)
        if (lag[s] < 0) return fail(FDW_EINVAL, "encode_gathers: lag[%d]=%d is negative", s, lag[s]);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || device < 0 || device >= ndev)
        return fail(FDW_ENODEVICE, "encode_gathers: no HIP device %d (%s); libfdwave has no CPU path", device, e != hipSuccess ? hipGetErrorString(e) : "out of range");
    HIP_TRY(hipSetDevice(device));
    const size_t gather = (size_t)nx * nt * sizeof(float), all = gather * (size_t)std::max(nshots, 1), tab = (size_t)std::max(nshots, 1) * sizeof(int);
    float *d_in = nullptr, *d_out = nullptr, *d_w = nullptr;
    int* d_lag = nullptr;
    int rc = FDW_OK;
    if (hipMalloc((void**)&d_in, all) != hipSuccess || hipMalloc((void**)&d_out, gather) != hipSuccess || hipMalloc((void**)&d_w, tab) != hipSuccess ||
        hipMalloc((void**)&d_lag, tab) != hipSuccess)
        rc = fail(FDW_ENOMEM, "encode_gathers: hipMalloc(%zu) failed", all + gather);
    else if ((nshots > 0 && ((e = hipMemcpy(d_in, d_obs_all, all, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(d_w, weight, tab, hipMemcpyHostToDevice)) != hipSuccess ||
                             (e = hipMemcpy(d_lag, lag, tab, hipMemcpyHostToDevice)) != hipSuccess)) ||
             (e = launch_encode_gathers(d_in, d_lag, d_w, d_out, nshots, nx, nt, nullptr)) != hipSuccess || (e = hipMemcpy(out, d_out, gather, hipMemcpyDeviceToHost)) != hipSuccess)
        rc = fail(FDW_EHIP, "encode_gathers: %s", hipGetErrorString(e));
    for (void* b : {(void*)d_in, (void*)d_out, (void*)d_w, (void*)d_lag})
        if (b) (void)hipFree(b);
    return rc;
}

// nplanes encodings of one data set: one upload of d_obs_all, one launch (fdw_encode_gathers_multi_kernel, blockIdx.y = the plane wave), one
// download.  Every refusal comes before a device is opened.
extern "C" int fdw_encode_gathers_multi(int device, int nshots, int nplanes, const int* lag, const float* weight, const float* d_obs_all, int nx, int nt,
                                        float* out)
{
    if (nshots < 0 || nplanes < 1 || nplanes > 65535 || nx < 1 || nt < 1 || nx > 65535 || !out || (nshots > 0 && (!lag || !weight || !d_obs_all)))
        return fail(FDW_EINVAL, "encode_gathers_multi: bad argument");
    for (size_t i = 0; i < (size_t)nplanes * (size_t)nshots; i++)
        if (lag[i] < 0) return fail(FDW_EINVAL, "encode_gathers_multi: lag[%zu][%zu]=%d is negative", i / (size_t)nshots, i % (size_t)nshots, lag[i]);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || device < 0 || device >= ndev)
        return fail(FDW_ENODEVICE, "encode_gathers_multi: no HIP device %d (%s); libfdwave has no CPU path", device,
                    e != hipSuccess ? hipGetErrorString(e) : "out of range");
    HIP_TRY(hipSetDevice(device));
    const size_t gather = (size_t)nx * nt * sizeof(float), all = gather * (size_t)std::max(nshots, 1), outb = gather * (size_t)nplanes;
    const size_t tab = (size_t)nplanes * (size_t)std::max(nshots, 1) * sizeof(int), used = (size_t)nplanes * (size_t)nshots * sizeof(int);
    float *d_in = nullptr, *d_out = nullptr, *d_w = nullptr;
    int* d_lag = nullptr;
    int rc = FDW_OK;
    if (hipMalloc((void**)&d_in, all) != hipSuccess || hipMalloc((void**)&d_out, outb) != hipSuccess || hipMalloc((void**)&d_w, tab) != hipSuccess ||
        hipMalloc((void**)&d_lag, tab) != hipSuccess)
        rc = fail(FDW_ENOMEM, "encode_gathers_multi: hipMalloc(%zu) failed", all + outb);
    else if ((nshots > 0 && ((e = hipMemcpy(d_in, d_obs_all, all, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(d_w, weight, used, hipMemcpyHostToDevice)) != hipSuccess ||
                             (e = hipMemcpy(d_lag, lag, used, hipMemcpyHostToDevice)) != hipSuccess)) ||
             (e = launch_encode_gathers_multi(d_in, d_lag, d_w, d_out, nshots, nplanes, nx, nt, nullptr)) != hipSuccess ||
             (e = hipMemcpy(out, d_out, outb, hipMemcpyDeviceToHost)) != hipSuccess)
        rc = fail(FDW_EHIP, "encode_gathers_multi: %s", hipGetErrorString(e));
    for (void* b : {(void*)d_in, (void*)d_out, (void*)d_w, (void*)d_lag})
        if (b) (void)hipFree(b);
    return rc;
}

// ------------------------------------------------------------------------------------------------
// tuning / introspection
// ------------------------------------------------------------------------------------------------
extern "C" int fdw_set_store_budget(fdw_ctx* c, size_t bytes)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    c->store_budget = bytes;
    return FDW_OK;
}
extern "C" int fdw_store_segments(const fdw_ctx* c) { return c ? c->store_segments : 0; }

extern "C" int fdw_set_batch_budget(fdw_ctx* c, size_t bytes)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    c->batch_budget = bytes;
    return FDW_OK;
}
extern "C" int fdw_batch_parts(const fdw_ctx* c) { return c ? c->batch_parts : 0; }

// The bytes a batch of shots may take: the context's own value (fdw_set_batch_budget) if non-zero, else FDW_BATCH_BUDGET_BYTES (a decimal
// byte count read at every call; empty, zero or anything else counts as unset), else 6 GiB.
static size_t batch_budget(const fdw_ctx* c)
{
    if (c->batch_budget) return c->batch_budget;
    if (const char* e = getenv("FDW_BATCH_BUDGET_BYTES")) {
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (*e >= '0' && *e <= '9' && *end == '\0' && v > 0) return (size_t)v;
    }
    return (size_t)6 << 30;
}

// fdw_batch_parts' bookkeeping.  Every batched entry point brackets its parts with batch_begin / batch_end; every part says how it ran
// (batch_part_ran): a part that could not go through the batched launches although it holds more than one shot (!batch_ok, no room)
// makes the call count as "one by one".  A part of a single shot inside a larger batch is a launch sequence like any other.
static void batch_begin(fdw_ctx* c) { c->batch_parts = 0; c->batch_single = false; }
static void batch_part_ran(fdw_ctx* c, bool batched_path) { c->batch_parts++; c->batch_single = c->batch_single || !batched_path; }
static int batch_end(fdw_ctx* c, int nshots, int rc)
{
    if (nshots <= 1 || c->batch_single) c->batch_parts = 0;
    c->batch_single = false;
    return rc;
}

extern "C" int fdw_set_tuning(fdw_ctx* c, int xchunk, int wz, int use_generic, int prefetch, int two_step)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (xchunk < 0 || (wz != 0 && wz != 1 && wz != 2 && wz != 4) || prefetch < 0 || prefetch > 3)
        return fail(FDW_EINVAL, "bad tuning xchunk=%d wz=%d prefetch=%d", xchunk, wz, prefetch);
    c->xchunk = xchunk;
    c->wz = wz;
    c->use_generic = use_generic ? 1 : 0;
    c->prefetch = prefetch;
    c->tb = two_step < 0 ? -1 : (two_step == kPipeSteps ? kPipeSteps : (two_step > 0 ? 1 : 0));   // kPipeSteps: force the wave-pipeline kernel
    c->xchunk2 = xchunk;   // the two-step kernel shares the knob (0 = its own default)
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// forward-modelling producer (dialect MOD): mod_main.cpp:140-174
// ------------------------------------------------------------------------------------------------
// nsteps iterations of M:147-164 on caller-owned device arrays: d_p / d_pp are M's P / PP (roles swap every step, as there),
// d_rec [>= (it0+nsteps)][nx] receives the trace samples of iteration it at row it (NULL: not recorded).
extern "C" int fdw_dev_model_steps(fdw_ctx* c, float* d_p, float* d_pp, const float* d_v2, const float* d_srce, int sx, int sz, int gz,
                                   float* d_rec, int it0, int nsteps, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (c->prm.dialect != FDW_DIALECT_MOD) return fail(FDW_ESTATE, "fdw_dev_model_steps needs a context created with dialect = FDW_DIALECT_MOD");
    hipStream_t s = pick_stream(c, stream);
    const Forward f = point_source(d_srce, sx, sz).recording(d_rec, gz);
    int k = 0;
    if (pipe_pays(c) && nsteps >= kPipeSteps) {
        // four steps per pass, out of place: the caller's two buffers plus two of the context's rotate.  In M's convention P is
        // the current field; a pass reads (p = P, pp = PP) and leaves PP' = u^{n+3} in out1, P' = u^{n+4} in out2.
        int rc = ensure_work_buffers(c, 4, false);
        if (rc) return rc;
        float* B[4] = {d_p, d_pp, c->fld[2], c->fld[3]};
        int iP = 0, iPP = 1;
        for (; nsteps - k >= kPipeSteps; k += kPipeSteps) {
            int o1, o2;
            spare_pair(iP, iPP, &o1, &o2);
            rc = stepn_impl(c, FDW_MODE_MOD, B[iP], B[iPP], d_v2, B[o1], B[o2], 1, view_at(f, it0 + k, c->nx), StepnBack{}, RowRanges{}, s);
            if (rc) return rc;
            iPP = o1; iP = o2;
        }
        // hand the state back in the caller's buffers: an even number of M's swaps leaves P in d_p and PP in d_pp
        const size_t bytes = field_elems(c) * sizeof(float);
        auto move = [&](int dst, int src) { return hipMemcpyAsync(B[dst], B[src], bytes, hipMemcpyDeviceToDevice, s); };
        if (iP == 1 && iPP == 0) {            // crossed: go through a context buffer (both are free here)
            HIP_TRY(move(2, 0)); HIP_TRY(move(0, 1)); HIP_TRY(move(1, 2));
        } else if (iPP == 0) {                // PP sits where P must go: B[1] is free, clear B[0] first
            HIP_TRY(move(1, 0));
            HIP_TRY(move(0, iP));
        } else {                              // B[0] is free or already holds P
            if (iP != 0) HIP_TRY(move(0, iP));
            if (iPP != 1) HIP_TRY(move(1, iPP));
        }
    }
    for (; k < nsteps; k++) {
        int rc = step_impl(c, FDW_MODE_MOD, d_p, d_pp, d_v2, 0, c->nxl, 1, view_at(f, it0 + k, c->nx), BackExtra{}, s);
        if (rc) return rc;
        std::swap(d_p, d_pp);
    }
    return FDW_OK;
}

extern "C" int fdw_model_shot(fdw_ctx* c, const float* vel2, int sx, int sz, int gz, const float* srce, int nt, float* data)
{
    if (!c || !vel2 || !data || (!srce && nt > 0)) return fail(FDW_EINVAL, "NULL argument");
    if (c->prm.dialect != FDW_DIALECT_MOD) return fail(FDW_ESTATE, "fdw_model_shot needs a context created with dialect = FDW_DIALECT_MOD");
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_model_shot needs a full-grid context");
    if (nt < 0) return fail(FDW_EINVAL, "nt=%d", nt);
    if (gz < c->prm.nzb || gz >= c->prm.nzb + c->nz)
        return fail(FDW_EINVAL, "receiver depth %d is not an interior column [%d,%d)", gz, c->prm.nzb, c->prm.nzb + c->nz);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_work_buffers(c, 2, false))) return rc;
    const size_t nx = c->nx, nrec = nx * (size_t)nt;
    if ((rc = ensure_cap(&c->d_rec, &c->rec_cap, nrec))) return rc;
    if ((rc = upload_rows(c, c->d_v2, vel2, c->stream)) || (rc = upload_source(c, srce, nt))) return rc;
    HIP_TRY(hipMemsetAsync(c->fld[0], 0, field_elems(c) * sizeof(float), c->stream));   // M:144-145
    HIP_TRY(hipMemsetAsync(c->fld[1], 0, field_elems(c) * sizeof(float), c->stream));
    // lazy damping: memory holds raw fields; as "p" a field owes one taper_apply, as "pp" two (it was damped once as the new
    // field and once more as P, M:151-152).  At it = 0 both are zero, so the count does not matter.
    if ((rc = fdw_dev_model_steps(c, c->fld[0], c->fld[1], c->d_v2, c->d_srce, sx, sz, gz, c->d_rec, 0, nt, c->stream))) return rc;
    std::vector<float> t(nrec);
    HIP_TRY(hipMemcpyAsync(t.data(), c->d_rec, nrec * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t ix = 0; ix < nx; ix++)            // device [it][ix] -> data[ix][it] (M:156)
        for (size_t it = 0; it < (size_t)nt; it++) data[ix * nt + it] = t[it * nx + ix];
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// stored-wavefield RTM (dialect RTM_STORED): rtm_main.cpp:158-240
// ------------------------------------------------------------------------------------------------
extern "C" int fdw_rtm_stored_shot(fdw_ctx* c, const float* vel2, int sx, int sz, int gz, const float* srce, int nt, const float* dobs,
                                   size_t n_floats, int is, float* imloc)
{
    if (!c || !vel2 || !imloc || !dobs || (!srce && nt > 0)) return fail(FDW_EINVAL, "NULL argument");
    if (c->prm.dialect != FDW_DIALECT_RTM_STORED) return fail(FDW_ESTATE, "fdw_rtm_stored_shot needs a context created with dialect = FDW_DIALECT_RTM_STORED");
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_rtm_stored_shot needs a full-grid context");
    if (nt < 0 || is < 0) return fail(FDW_EINVAL, "nt=%d is=%d", nt, is);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_work_buffers(c, 2, true))) return rc;
    const size_t nx = c->nx, fe = field_elems(c);
    // receiver samples as the reference indexes them: step it reads dobs[is][ix][nt - it]
    std::vector<float> rows(std::max<size_t>(nx * (size_t)nt, 1));
    for (int it = 0; it < nt; it++)
        for (size_t ix = 0; ix < nx; ix++) {
            const size_t k = ((size_t)is * nx + ix) * (size_t)nt + (size_t)(nt - it);
            rows[(size_t)it * nx + ix] = k < n_floats ? dobs[k] : 0.0f;
        }
    if ((rc = ensure_cap(&c->d_dobs, &c->dobs_cap, rows.size()))) return rc;
    HIP_TRY(hipMemcpy(c->d_dobs, rows.data(), rows.size() * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = upload_rows(c, c->d_v2, vel2, c->stream)) || (rc = upload_source(c, srce, nt))) return rc;
    float *d_p = c->fld[0], *d_pp = c->fld[1];
    // The source wavefield of every step (rtm_main.cpp:177-181 keeps the interior; whole pitched fields here so that the imaging epilogue of
    // the step kernel can read them like any other field): swf[it] = P of step it, it = 0 .. nt-1, swf[0] = 0.  The receiver pass consumes
    // them LAST FIRST (iteration it images against swf[nt-it-1], rtm_main.cpp:224-230).
    //   * They fit the store budget (fdw_set_store_budget; default: whatever hipMalloc grants): all nt fields are kept, one segment.
    //   * They do not: CHECKPOINTING.  The steps are cut into S segments of m; the forward pass keeps, per segment, only the pair of fields it
    //     starts from (2 S fields) and runs through ONE segment buffer of m + 1 fields; the receiver pass takes the segments last first and
    //     recomputes each from its pair into that buffer before consuming it.  The recomputation is the same launches on the same inputs, so
    //     every stored field -- and with it the image -- is bit-identical to the unconstrained run; the price is one more forward pass
    //     (2 nt + nt launches instead of nt + nt).  Memory 2 S + m + 1 fields, least at m ~ sqrt(2 nt): 1 001 steps fit in 92 fields.
    const size_t fbytes = fe * sizeof(float);
    size_t budget_fields = c->store_budget ? c->store_budget / fbytes : (size_t)-1;
    if (const char* e = getenv("FDW_STORE_BUDGET_MB")) budget_fields = (size_t)atoll(e) * ((size_t)1 << 20) / fbytes;
    int m = std::max(nt, 1), S = 1;                       // segment length, segments
    float *d_seg = nullptr, *d_ck = nullptr;
    struct Free { float*& p; ~Free() { if (p) (void)hipFree(p); } } g1{d_seg}, g2{d_ck};
    bool whole = (size_t)nt + 1 <= budget_fields;
    const int forced_m = getenv("FDW_STORE_SEGMENT") ? atoi(getenv("FDW_STORE_SEGMENT")) : 0;      // tests: checkpoint with this segment length whatever fits
    if (forced_m > 0 && forced_m < nt) whole = false;
    if (whole && nt > 0 && hipMalloc((void**)&d_seg, fbytes * ((size_t)nt + 1)) != hipSuccess) {      // no budget given and the device says no: checkpoint into what is free
        (void)hipGetLastError();
        d_seg = nullptr;
        whole = false;
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        budget_fields = (size_t)(0.9 * (double)fr) / fbytes;
    }
    if (!whole && nt > 0) {
        // the longest segment that fits: fewest restarts, same recomputation cost (one forward pass) whatever m is
        int best = 0;
        for (int mm = nt; mm >= 1; mm--)
            if (2 * (size_t)((nt + mm - 1) / mm) + (size_t)mm + 1 <= budget_fields) { best = mm; break; }
        if (forced_m > 0 && forced_m < nt) best = forced_m;
        if (best == 0)
            return fail(FDW_ENOMEM, "the stored source fields of %d steps need at least %d fields of %zu bytes with checkpointing (%d + 1 without); the store budget holds %zu",
                        nt, (int)(2 * std::ceil(std::sqrt(nt / 2.0)) + std::ceil(std::sqrt(2.0 * nt)) + 1), fbytes, nt, budget_fields);
        m = best;
        S = (nt + m - 1) / m;
        hipError_t e1 = hipMalloc((void**)&d_seg, fbytes * ((size_t)m + 1));
        hipError_t e2 = e1 == hipSuccess ? hipMalloc((void**)&d_ck, fbytes * 2 * (size_t)S) : e1;
        if (e1 != hipSuccess || e2 != hipSuccess) return fail(FDW_ENOMEM, "checkpointed store (%d segments of %d steps, %zu bytes per field): %s", S, m, fbytes, hipGetErrorString(e2));
    }
    c->store_segments = S;
    auto seg = [&](int j) { return d_seg + (size_t)j * fe; };
    auto ck = [&](int s, int which) { return d_ck + ((size_t)2 * s + which) * fe; };      // which 0: swf[s m - 1], 1: swf[s m]
    // one segment of the forward loop: fields swf[s0 .. s0+len] into seg[0 .. len]; prev = swf[s0 - 1], seg[0] must hold swf[s0].
    // Step it reads p = swf[it], pp = swf[it-1] and writes the new field straight into the next slot -- no copy per step.  (Cells a launch
    // never stores -- the padding columns -- are zero in every slot from the memset below and stay so.)
    auto run_segment = [&](int s0, int len, const float* prev) -> int {
        for (int j = 0; j < len; j++) {
            const int it = s0 + j;
            float* pp_in = j > 0 ? seg(j - 1) : const_cast<float*>(prev);                  // only read (out is given)
            FwdView f = view_at(point_source(c->d_srce, sx, sz), it, c->nx);
            f.out = seg(j + 1);
            int r = step_impl(c, FDW_MODE_DD_FWD, seg(j), pp_in, c->d_v2, 0, c->nxl, 1, f, BackExtra{}, c->stream);
            if (r) return r;
        }
        return FDW_OK;
    };
    if (nt > 0) {
        HIP_TRY(hipMemsetAsync(d_seg, 0, fbytes * ((size_t)m + 1), c->stream));          // swf[0] = 0 (rtm_main.cpp:161-162) and every padding column
        HIP_TRY(hipMemsetAsync(d_pp, 0, fbytes, c->stream));                              // the field before step 0
        if (d_ck) HIP_TRY(hipMemsetAsync(d_ck, 0, fbytes * 2 * (size_t)S, c->stream));
        for (int s = 0; s < S; s++) {
            const int s0 = s * m, len = std::min(m, nt - s0);
            if (s > 0) HIP_TRY(hipMemcpyAsync(seg(0), ck(s, 1), fbytes, hipMemcpyDeviceToDevice, c->stream));
            if ((rc = run_segment(s0, len, s > 0 ? ck(s, 0) : d_pp))) return rc;
            if (s + 1 < S) {                              // what the next segment starts from: swf[s0 + m - 1], swf[s0 + m]
                HIP_TRY(hipMemcpyAsync(ck(s + 1, 0), seg(m - 1), fbytes, hipMemcpyDeviceToDevice, c->stream));
                HIP_TRY(hipMemcpyAsync(ck(s + 1, 1), seg(m), fbytes, hipMemcpyDeviceToDevice, c->stream));
            }
        }
    }
    HIP_TRY(hipMemsetAsync(d_p, 0, fbytes, c->stream));     // rtm_main.cpp:187-189
    HIP_TRY(hipMemsetAsync(d_pp, 0, fbytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_img, 0, fbytes, c->stream));
    float* d_zero = nullptr;                                // checkpointing: the zero field before step 0 (d_pp is a receiver field from here on)
    struct Free g3{d_zero};
    if (S > 1) {
        if (hipMalloc((void**)&d_zero, fbytes) != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc(%zu) failed", fbytes);
        HIP_TRY(hipMemsetAsync(d_zero, 0, fbytes, c->stream));
    }
    int it = 0;
    for (int s = S - 1; s >= 0 && nt > 0; s--) {
        const int s0 = s * m, len = std::min(m, nt - s0);
        if (s < S - 1) {                                    // (the last segment is still in the buffer from the forward pass)
            HIP_TRY(hipMemcpyAsync(seg(0), s > 0 ? ck(s, 1) : d_zero, fbytes, hipMemcpyDeviceToDevice, c->stream));
            if ((rc = run_segment(s0, len, s > 0 ? ck(s, 0) : d_zero))) return rc;
        }
        for (int j = len - 1; j >= 0; j--, it++) {          // receiver iteration `it` images against swf[nt - it - 1] = swf[s0 + j]
            BackExtra bk;
            bk.psrc_a = seg(j); bk.img = c->d_img;
            rc = step_impl(c, FDW_MODE_DD_RECV, d_p, d_pp, c->d_v2, 0, c->nxl, 1, receiver_samples(c->d_dobs + (size_t)it * nx, gz), bk, c->stream);
            if (rc) return rc;
            std::swap(d_p, d_pp);
        }
    }
    if ((rc = image_to_host(c, imloc, c->d_img))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// image post-processing (row f3): laplace.f90
// ------------------------------------------------------------------------------------------------
extern "C" int fdw_image_laplacian(int device, const float* img, int nx, int nz, float dx, float dz, float* out)
{
    if (!img || !out || nx < 1 || nz < 1 || !(dx > 0.0f) || !(dz > 0.0f)) return fail(FDW_EINVAL, "image_laplacian: bad argument");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || device < 0 || device >= ndev)
        return fail(FDW_ENODEVICE, "image_laplacian: no HIP device %d (%s); libfdwave has no CPU path", device, e != hipSuccess ? hipGetErrorString(e) : "out of range");
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)nx * nz * sizeof(float);
    float *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc((void**)&d_in, bytes) != hipSuccess || hipMalloc((void**)&d_out, bytes) != hipSuccess) {
        if (d_in) (void)hipFree(d_in);
        return fail(FDW_ENOMEM, "image_laplacian: hipMalloc(%zu) failed", bytes);
    }
    int rc = FDW_OK;
    if ((e = hipMemcpy(d_in, img, bytes, hipMemcpyHostToDevice)) != hipSuccess || (e = launch_image_laplacian(d_in, d_out, nx, nz, dx, dz, nullptr)) != hipSuccess ||
        (e = hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost)) != hipSuccess)
        rc = fail(FDW_EHIP, "image_laplacian: %s", hipGetErrorString(e));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

// The reference's image comparer models/marmousi/psnr (an ELF without source; behaviour read off its output: MSE = mean (a-b)^2, RMSE, SNR =
// 10 log10(sum b^2 / sum (a-b)^2), PSNR = 20 log10(max |b| / RMSE), the difference a - b written out) on the device.
extern "C" int fdw_image_compare(int device, const float* a, const float* b, size_t n, float* diff, double stats[4], int exact_sums)
{
    if (!a || !b || !stats || n == 0) return fail(FDW_EINVAL, "image_compare: bad argument");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || device < 0 || device >= ndev)
        return fail(FDW_ENODEVICE, "image_compare: no HIP device %d (%s); libfdwave has no CPU path", device, e != hipSuccess ? hipGetErrorString(e) : "out of range");
    HIP_TRY(hipSetDevice(device));
    const int nblocks = (int)std::min<size_t>(1024, (n + 255) / 256);
    float *d_a = nullptr, *d_b = nullptr, *d_d = nullptr;
    double* d_w = nullptr;
    const size_t bytes = n * sizeof(float);
    int rc = FDW_OK;
    if (hipMalloc((void**)&d_a, bytes) != hipSuccess || hipMalloc((void**)&d_b, bytes) != hipSuccess || (diff && hipMalloc((void**)&d_d, bytes) != hipSuccess) ||
        hipMalloc((void**)&d_w, (3 * (size_t)nblocks + 8) * sizeof(double)) != hipSuccess)
        rc = fail(FDW_ENOMEM, "image_compare: hipMalloc failed");
    double h[5] = {0, 0, 0, 0, 0};
    if (rc == FDW_OK) {
        if ((e = hipMemcpy(d_a, a, bytes, hipMemcpyHostToDevice)) != hipSuccess || (e = hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice)) != hipSuccess ||
            (e = launch_image_compare(d_a, d_b, n, d_d, d_w + 8, nblocks, d_w, exact_sums ? 0 : 1, nullptr)) != hipSuccess ||
            (e = hipMemcpy(h, d_w, sizeof h, hipMemcpyDeviceToHost)) != hipSuccess || (diff && (e = hipMemcpy(diff, d_d, bytes, hipMemcpyDeviceToHost)) != hipSuccess))
            rc = fail(FDW_EHIP, "image_compare: %s", hipGetErrorString(e));
    }
    for (void* p : {(void*)d_a, (void*)d_b, (void*)d_d, (void*)d_w})
        if (p) (void)hipFree(p);
    if (rc != FDW_OK) return rc;
    if (exact_sums) {
        const double mse = h[0] / (double)n, rmse = std::sqrt(mse);
        stats[0] = mse;
        stats[1] = rmse;
        stats[2] = 10.0 * std::log10(h[1] / h[0]);
        stats[3] = 20.0 * std::log10(h[2] / rmse);
    } else {      // the tool's own arithmetic (pinned to its output by the oracle's restatement): fp32 sums, fp32 quotient and root, PSNR kept in fp32
        const float sd = (float)h[3], sb = (float)h[4], mx = (float)h[2];
        const float mse = sd / (float)n, rmse = sqrtf(mse);
        stats[0] = mse;
        stats[1] = rmse;
        stats[2] = 10.0 * std::log10((double)(sb / sd));
        stats[3] = (float)(20.0 * std::log10((double)(mx / rmse)));
    }
    return FDW_OK;
}

extern "C" int fdw_get_tables(const fdw_ctx* c, float* coefs_x, float* coefs_z, float* taper_x, float* taper_z)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (coefs_x) memcpy(coefs_x, c->cx, (c->prm.order + 1) * sizeof(float));
    if (coefs_z) memcpy(coefs_z, c->cz, (c->prm.order + 1) * sizeof(float));
    if (taper_x && c->prm.nxb > 0) memcpy(taper_x, c->taper_x.data(), c->prm.nxb * sizeof(float));
    if (taper_z && c->prm.nzb > 0) memcpy(taper_z, c->taper_z.data(), c->prm.nzb * sizeof(float));
    return FDW_OK;
}

extern "C" int fdw_get_extents(const fdw_ctx* c, int* xlim, int* zlim, int* ztap)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (xlim) *xlim = c->xlim;
    if (zlim) *zlim = c->zlim;
    if (ztap) *ztap = c->ztap;
    return FDW_OK;
}

extern "C" int fdw_selftest(fdw_ctx* c)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    float h_src[64], h_out[384];
    for (int i = 0; i < 64; i++) h_src[i] = 100.0f + i;
    for (int i = 0; i < 384; i++) h_out[i] = -7.0f;
    float* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, (64 + 384) * sizeof(float)));
    hipError_t e = hipMemcpy(d, h_src, sizeof h_src, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 64, h_out, sizeof h_out, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_selftest(d, d + 64, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(h_out, d + 64, sizeof h_out, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(FDW_EHIP, "selftest: %s", hipGetErrorString(e));
    for (int i = 0; i < 64; i++) {
        // lane 0 (63) has no neighbour to take from: the kernels never use what it receives (a halo lane / replaced by the strip halo)
        const float up = i == 0 ? h_out[0] : h_src[i - 1], dn = i == 63 ? h_out[127] : h_src[i + 1];
        if (h_out[i] != up || h_out[64 + i] != dn)
            return fail(FDW_EHIP, "selftest: lane exchange mismatch at lane %d (up %g want %g, down %g want %g)", i,
                        (double)h_out[i], (double)up, (double)h_out[64 + i], (double)dn);
        for (int k = 0; k < 4; k++) {
            const float want = (i >= 2 && i <= 61) ? h_src[i] : -7.0f;   // out-of-range lanes must leave memory alone
            if (h_out[128 + 4 * i + k] != want)
                return fail(FDW_EHIP, "selftest: range-predicated buffer store wrote %g at cell %d (want %g)",
                            (double)h_out[128 + 4 * i + k], i, (double)want);
        }
    }
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// random-border velocity model generated on the device
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int L = fdw::kRandLag;
using Mat = std::vector<unsigned>;     // 31 x 31 over Z/2^32, row-major

Mat mat_mul(const Mat& a, const Mat& b)
{
    Mat r((size_t)L * L, 0u);
    for (int i = 0; i < L; i++)
        for (int k = 0; k < L; k++) {
            const unsigned aik = a[(size_t)i * L + k];
            if (!aik) continue;
            for (int j = 0; j < L; j++) r[(size_t)i * L + j] += aik * b[(size_t)k * L + j];
        }
    return r;
}

struct RandTables {
    Mat pow2[64];        // M^(2^j): one stream position per application
    unsigned glo[65][L]; // x^(31 l) mod P, l = 0..64, P = x^31 - x^28 - 1 (the generator's characteristic polynomial)
    unsigned w0[L];      // window before the first step of a seed-1 generator (before glibc's 310 discarded outputs)
};

// The window W = (y[K-31] .. y[K-1]) advances by  W' = (w1 .. w30, w0 + w28)  (y[K] = y[K-31] + y[K-3]).
const RandTables& rand_tables()
{
    static RandTables t;
    static std::once_flag once;
    std::call_once(once, [] {
        Mat m((size_t)L * L, 0u);
        for (int i = 0; i + 1 < L; i++) m[(size_t)i * L + i + 1] = 1;
        m[(size_t)(L - 1) * L + 0] = 1;
        m[(size_t)(L - 1) * L + 28] = 1;
        t.pow2[0] = m;
        for (int j = 1; j < 64; j++) t.pow2[j] = mat_mul(t.pow2[j - 1], t.pow2[j - 1]);
        std::memset(t.glo, 0, sizeof t.glo);
        t.glo[0][0] = 1u;
        for (int l = 0; l < 64; l++) {
            unsigned g[L];
            std::memcpy(g, t.glo[l], sizeof g);
            for (int k = 0; k < L; k++) {                      // times x: the x^31 term folds into x^28 + 1
                const unsigned top = g[L - 1];
                for (int i = L - 1; i > 0; i--) g[i] = g[i - 1];
                g[0] = top;
                g[28] += top;
            }
            std::memcpy(t.glo[l + 1], g, sizeof g);
        }
        // glibc srandom_r(1): r[0] = seed, r[i] = 16807 r[i-1] mod (2^31 - 1) by Schrage's method; front pointer at r[3], rear at r[0]
        unsigned r[L];
        int word = 1;
        r[0] = 1u;
        for (int k = 1; k < L; k++) {
            const long hi = word / 127773, lo = word % 127773;
            long v = 16807 * lo - 2836 * hi;
            if (v < 0) v += 2147483647;
            word = (int)v;
            r[k] = (unsigned)word;
        }
        // step t adds slot t mod 31 into slot (t + 3) mod 31, i.e. y[t] = y[t-31] + y[t-3] with y[s] = r[(s + 34) mod 31] for s in [-31, 0)
        for (int s = 0; s < L; s++) t.w0[s] = r[(s + 3) % L];
    });
    return t;
}

fdw::RandWindow window_at(unsigned long long k)
{
    const RandTables& t = rand_tables();
    unsigned w[L], v[L];
    std::memcpy(w, t.w0, sizeof w);
    for (int j = 0; j < 64; j++)
        if ((k >> j) & 1) {
            const Mat& m = t.pow2[j];
            for (int i = 0; i < L; i++) {
                unsigned acc = 0;
                for (int c = 0; c < L; c++) acc += m[(size_t)i * L + c] * w[c];
                v[i] = acc;
            }
            std::memcpy(w, v, sizeof w);
        }
    fdw::RandWindow out;
    std::memcpy(out.w, w, sizeof w);
    return out;
}

constexpr unsigned long long kGlibcDiscard = 310;     // outputs srandom_r() throws away

// a * b mod P
void poly_mul(const unsigned* a, const unsigned* b, unsigned* out)
{
    unsigned c[2 * L - 1] = {0};
    for (int i = 0; i < L; i++)
        for (int j = 0; j < L; j++) c[i + j] += a[i] * b[j];
    for (int k = 2 * L - 2; k >= L; k--) {                    // x^k = x^(k-3) + x^(k-31)
        c[k - 3] += c[k];
        c[k - L] += c[k];
    }
    std::memcpy(out, c, L * sizeof(unsigned));
}

fdw::RandBase base_at(unsigned long long k)
{
    const fdw::RandWindow w = window_at(k);
    fdw::RandBase b;
    std::memcpy(b.y, w.w, sizeof w.w);
    for (int s = 0; s < L - 1; s++) b.y[L + s] = b.y[s] + b.y[s + 28];     // y[K+s] = y[K+s-31] + y[K+s-3]
    return b;
}

// device table for up to ndraws draws per launch: [31][64] lane factors, then one block factor per 64 threads
int ensure_rand_tables(fdw_ctx* c, long long ndraws)
{
    const long long threads = (ndraws + L - 1) / L;
    const int need = (int)std::max<long long>((threads + 63) / 64, 1);
    if (c->d_jump && c->njump >= need) return FDW_OK;
    if (c->d_jump) (void)hipFree(c->d_jump);
    c->d_jump = nullptr;
    const RandTables& t = rand_tables();
    std::vector<unsigned> flat((size_t)L * 64 + (size_t)need * L);
    for (int i = 0; i < L; i++)
        for (int l = 0; l < 64; l++) flat[(size_t)i * 64 + l] = t.glo[l][i];
    unsigned* hi = &flat[(size_t)L * 64];
    std::memset(hi, 0, L * sizeof(unsigned));
    hi[0] = 1u;
    for (int h = 1; h < need; h++) poly_mul(hi + (size_t)(h - 1) * L, t.glo[64], hi + (size_t)h * L);
    hipError_t e = hipMalloc((void**)&c->d_jump, flat.size() * sizeof(unsigned));
    if (e != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpy(c->d_jump, flat.data(), flat.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    c->njump = need;
    return FDW_OK;
}
}  // namespace

static int ensure_draws(fdw_ctx* c, long long n)
{
    n = std::max<long long>(n, 1);
    int rc = ensure_rand_tables(c, n);
    if (rc || c->draws_cap >= n) return rc;
    if (c->d_draws) (void)hipFree(c->d_draws);
    c->d_draws = nullptr;
    c->draws_cap = 0;
    hipError_t e = hipMalloc((void**)&c->d_draws, (size_t)n * sizeof(int));
    if (e != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    c->draws_cap = n;
    return FDW_OK;
}

extern "C" long long fdw_border_draws(int nx, int nz, int nxb, int nzb)
{
    if (nx < 0 || nz < 0 || nxb < 0 || nzb < 0) return -1;
    return (long long)nx * nzb + 2ll * nz * nxb + 2ll * nzb * (nzb + 1);
}

extern "C" int fdw_rand_stream(fdw_ctx* c, unsigned long long draw_offset, long long n, int* out)
{
    if (!c || (!out && n > 0) || n < 0) return fail(FDW_EINVAL, "bad argument");
    if (n == 0) return FDW_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_rand_tables(c, n);
    if (rc) return rc;
    int* d = nullptr;
    hipError_t e = hipMalloc((void**)&d, (size_t)n * sizeof(int));
    if (e != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    e = launch_rand_stream(base_at(kGlibcDiscard + draw_offset), c->d_jump, n, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(FDW_EHIP, "rand_stream: %s", hipGetErrorString(e));
    return FDW_OK;
}

extern "C" int fdw_model_resident(fdw_ctx* c, const float* vp)
{
    if (!c || !vp) return fail(FDW_EINVAL, "NULL argument");
    if (c->prm.dialect != FDW_DIALECT_RTM) return fail(FDW_ESTATE, "the random-border model belongs to the RTM dialect");
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_model_resident needs a full-grid context");
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "no interior");
    const int nxb = c->prm.nxb, nzb = c->prm.nzb;
    if (nxb == 1 || nzb == 1) return fail(FDW_EINVAL, "a border of one cell divides by zero in the reference's ramp (nb - 1)");
    if (nzb > c->prm.nxe) return fail(FDW_EINVAL, "nzb=%d > nxe=%d: the reference's corner loops leave the array", nzb, c->prm.nxe);
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_work_buffers(c, 0, false);
    if (rc) return rc;
    const size_t n = (size_t)c->nx * c->nz;
    if (!c->d_vp) {
        hipError_t e = hipMalloc((void**)&c->d_vp, n * sizeof(float));
        if (e != hipSuccess) return fail(FDW_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    if ((rc = ensure_draws(c, fdw_border_draws(c->nx, c->nz, nxb, nzb)))) return rc;
    if ((rc = alloc_zero(&c->d_vpe, field_elems(c)))) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_vp, vp, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->model_resident = true;
    c->v2_resident = false;
    return FDW_OK;
}

extern "C" int fdw_dev_extendvel_linear(fdw_ctx* c, unsigned long long draw_offset, float* vel_out)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    if (!c->model_resident) return fail(FDW_ESTATE, "no resident model: call fdw_model_resident first");
    HIP_TRY(hipSetDevice(c->device));
    const long long n = fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    hipError_t e = launch_rand_stream(base_at(kGlibcDiscard + draw_offset), c->d_jump, n, c->d_draws, c->stream);
    if (e != hipSuccess) return fail(FDW_EHIP, "rand_stream launch failed: %s", hipGetErrorString(e));
    BorderArgs a{c->d_vp, c->d_draws, c->d_vpe, c->d_v2, c->nx, c->nz, c->prm.nxb, c->prm.nzb, c->pitch};
    e = launch_extendvel(a, c->stream);
    if (e != hipSuccess) return fail(FDW_EHIP, "extendvel launch failed: %s", hipGetErrorString(e));
    c->v2_resident = true;
    if (vel_out) {
        int rc = download_rows(c, vel_out, c->d_vpe, c->stream);
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return FDW_OK;
}

extern "C" int fdw_shot_resident(fdw_ctx* c, int sx, int sz, int gz, const float* srce, const float* d_obs, float* imloc, float* P, float* PP)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(has_model(c, nullptr));
    return shot_impl(c, nullptr, sx, sz, gz, srce, d_obs, imloc, P, PP, ShotExtras{});
}

extern "C" int fdw_shot_resident_illum(fdw_ctx* c, int sx, int sz, int gz, const float* srce, const float* d_obs, float* imloc, float* illum,
                                       float* P, float* PP)
{
    if (!c || !illum) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "source illumination", "fdw_shot_resident_illum"));
    FDW_TRY(has_model(c, nullptr));
    ShotExtras x;
    x.illum = illum;
    return shot_impl(c, nullptr, sx, sz, gz, srce, d_obs, imloc, P, PP, x);
}

// ---- the excitation-amplitude shot (definitions in fdwave.h) ----
extern "C" int fdw_image_excitation(const float* exc, const float* amp, size_t n, float eps, float* img)
{
    if (!(eps >= 0.0f) || std::isinf(eps)) return fail(FDW_EINVAL, "fdw_image_excitation: eps must be finite and >= 0");
    if (n > 0 && (!exc || !amp || !img)) return fail(FDW_EINVAL, "NULL argument");
    float m = 0.0f;
    for (size_t i = 0; i < n; i++) {
        const float a = fabsf(amp[i]);
        if (a > m) m = a;
    }
    const float s = eps * m;
    for (size_t i = 0; i < n; i++)
        if (fabsf(amp[i]) > s) img[i] = img[i] + exc[i] / amp[i];
    return FDW_OK;
}

// the data gathers d_obs [nshots][nx][nt] as the pick loop's line gathers d_dst [nshots][nt][nx]: row k = d_obs[.][nt-1-k], reversed on the device
static int reversed_gathers_to_device(fdw_ctx* c, const float* d_obs, float* d_dst, int nshots)
{
    const size_t n = (size_t)c->nx * c->prm.nt * nshots;
    if (n == 0) return FDW_OK;
    int rc = ensure_cap(&c->d_raw, &c->raw_cap, n);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->d_raw, d_obs, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipError_t e = launch_gather_transpose_rev(c->d_raw, d_dst, c->nx, c->prm.nt, nshots, c->stream);
    if (e != hipSuccess) return fail(FDW_EHIP, "gather transposition launch failed: %s", hipGetErrorString(e));
    return FDW_OK;
}

// what every excitation shot asks of its arguments beyond the pointers (a batch: of its first and last source row)
static int check_exc_shot(const fdw_ctx* c, const char* who, int sx, int sz, int gz, float eps)
{
    FDW_TRY(check_exc_eps(who, eps));
    if (sx < 0) return fail(FDW_EINVAL, "%s: source row %d", who, sx);
    FDW_TRY(check_exc_source(c, who, sx, sz));
    FDW_TRY(check_line_args(c, who, gz, 0, false, false));
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "no interior to image");
    return FDW_OK;
}

// fdw_shot_excitation behind its checks.  The image is formed on the device (exc_image, one shot) and comes back as ONE interior array;
// exc, amp and texc come back only where the caller asked for them.
static int shot_excitation_impl(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, const float* d_obs, float eps, float* imloc,
                                float* exc, float* amp, int* texc, float* P, float* PP)
{
    FDW_RANGE("fdw: excitation-amplitude shot (uploads, forward + maps, receiver loop + pick, image, downloads)");
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    const int nt = c->prm.nt, nx = c->nx;
    const size_t fe = field_elems(c);
    if ((rc = ensure_work_buffers(c, 8, imloc != nullptr)) || (rc = alloc_zero(&c->d_amp, fe)) || (rc = alloc_zero((float**)&c->d_texc, fe)) ||
        (rc = alloc_zero(&c->d_exc, fe)) || (rc = ensure_cap(&c->d_wav, &c->wav_cap, (size_t)nx * nt)))
        return rc;
    float* const maps[3] = {c->d_amp, (float*)c->d_texc, c->d_exc};
    if ((rc = zero_fields(c, c->fld, 2)) || (rc = zero_fields(c, maps, 3))) return rc;
    end_residency(c, v2);
    if ((v2 && (rc = upload_rows(c, c->d_v2, v2, c->stream))) || (rc = upload_source(c, srce, nt))) return rc;
    if ((rc = reversed_gathers_to_device(c, d_obs, c->d_wav, 1))) return rc;
    if (imloc && (rc = image_to_device(c, imloc, c->d_img))) return rc;
    int ip = 0, ipp = 1;
    const Forward fwd = point_source(c->d_srce, sx, sz).exciting(Exc::maps, c->d_amp, c->d_texc, 0);
    if ((rc = steps_loop(c, c->fld, c->d_v2, fwd, 0, nt, 0, &ip, &ipp, c->stream))) return rc;
    if (nt > 0 && (rc = fdw_dev_taper_finalize(c, c->fld[ip], c->stream))) return rc;      // as fdw_shot's forward loop leaves d_p
    if (P && (rc = download_rows(c, P, c->fld[ip], c->stream))) return rc;
    if (PP && (rc = download_rows(c, PP, c->fld[ipp], c->stream))) return rc;
    if ((rc = zero_fields(c, c->fld + 4, 2))) return rc;
    int rp = 0, rpp = 1;
    const Forward bwd = line_source(c->d_wav, gz).exciting(Exc::pick, c->d_exc, c->d_texc, nt);
    if ((rc = steps_loop(c, c->fld + 4, c->d_v2, bwd, 0, nt, 0, &rp, &rpp, c->stream))) return rc;
    if (imloc && ((rc = exc_image(c, c->d_exc, c->d_amp, eps, c->d_img, nullptr, 1, c->stream)) || (rc = image_to_host(c, imloc, c->d_img)))) return rc;
    if (exc && (rc = image_to_host(c, exc, c->d_exc))) return rc;
    if (amp && (rc = image_to_host(c, amp, c->d_amp))) return rc;
    if (texc && (rc = image_to_host(c, (float*)texc, (const float*)c->d_texc))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

extern "C" int fdw_shot_excitation(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, const float* d_obs, float eps, float* imloc,
                                   float* exc, float* amp, int* texc, float* P, float* PP)
{
    if (!c) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "excitation-amplitude imaging", "fdw_shot_excitation"));
    if (!srce || !d_obs || (!imloc && !exc && !amp && !texc)) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_exc_eps("fdw_shot_excitation", eps));
    FDW_TRY(has_model(c, v2));
    FDW_TRY(check_exc_shot(c, "fdw_shot_excitation", sx, sz, gz, eps));
    return shot_excitation_impl(c, v2, sx, sz, gz, srce, d_obs, eps, imloc, exc, amp, texc, P, PP);
}

// ---- residual migration (definitions in fdwave.h) ----
extern "C" int fdw_shot_residual(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, const float* d_obs, float* imloc, float* illum,
                                 float* resid, float* P, float* PP)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_single_shot_ctx(c, "residual migration", "fdw_shot_residual"));
    FDW_TRY(has_model(c, v2));
    end_residency(c, v2);
    ShotExtras x;
    x.illum = illum; x.residual = true; x.resid = resid;
    return shot_impl(c, v2, sx, sz, gz, srce, d_obs, imloc, P, PP, x);
}

// ------------------------------------------------------------------------------------------------
// a batch of shots through ONE launch per time step
// ------------------------------------------------------------------------------------------------
// A shot of a deck of the reference's size (new_mod: 495 x 375 extended) is 3400 dependent launches of kernels that fill a few percent
// of the chip and last 3.5-7 us each: latency, not bandwidth.  Shots are independent (R:480-529 couples them only through the image sum),
// so `nshots` of them on one geometry go through the same launches side by side: gridDim.y = shot, every field pointer offset by
// shot * field, the gather by shot * nx * nt, the source row by shot * dsx (the reference's sx = fsx + is * ds, R:405-407).
static bool batch_ok(const fdw_ctx* c)
{
    if (c->prm.dialect == FDW_DIALECT_MOD) return c->h <= kMaxFastHalfOrder && !c->use_generic && !pipe_pays(c);
    return c->prm.dialect == FDW_DIALECT_RTM && c->h <= kMaxFastHalfOrder && !c->use_generic && !c->no_fused_back && !two_step_pays(c) &&
           !pipe_pays(c) && fdw_receivers_stepped(c);
}

extern "C" int fdw_shot_batch_max(const fdw_ctx* c)
{
    if (!c || !is_full_grid(c) || !batch_ok(c)) return 1;
    const long waves = (long)c->nxl * ((c->pitch + 255) / 256);        // one-row-per-wave regime: waves one shot launches
    const long by_fill = 32768 / std::max<long>(waves, 1);            // measured on new_mod-sized shots: 18.6 ms per shot alone, 5.6 at 8, 4.4 at 16, 3.7 at 32
    const long by_mem = (long)(batch_budget(c) / (11 * field_elems(c) * sizeof(float)));
    return (int)std::max<long>(1, std::min<long>({by_fill, by_mem, 64}));
}

// Per-shot copies of what a batch needs: the RTM loop (need_all) its eight fields, v2, image and gathers; the modelling loop only two
// fields and the gathers.  On an allocation failure whatever was allocated is released again (the callers then run the shots one by one).
static int ensure_batch_buffers(fdw_ctx* c, int n, bool need_all)
{
    const size_t nx = c->nx, nt = std::max(c->prm.nt, 1);
    if (c->batch_cap >= n && (c->batch_all || !need_all)) return FDW_OK;
    float** all[] = {&c->bfld[0], &c->bfld[1], &c->bfld[2], &c->bfld[3], &c->bfld[4], &c->bfld[5], &c->bfld[6], &c->bfld[7], &c->b_v2, &c->b_img, &c->b_dobs};
    auto release = [&] {
        for (float** q : all) {
            if (*q) (void)hipFree(*q);
            *q = nullptr;
        }
        c->batch_cap = 0;
        c->batch_all = false;
    };
    release();
    for (float** q : all) {
        const bool wanted = need_all || q == &c->bfld[0] || q == &c->bfld[1] || q == &c->b_dobs;
        if (!wanted) continue;
        const size_t elems = (q == &c->b_dobs ? nx * nt : field_elems(c)) * (size_t)n;
        hipError_t e = hipMalloc((void**)q, elems * sizeof(float));
        if (e == hipSuccess) e = hipMemset(*q, 0, elems * sizeof(float));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            release();
            return fail(FDW_ENOMEM, "batch of %d shots: hipMalloc / hipMemset(%zu bytes) failed: %s", n, elems * sizeof(float), hipGetErrorString(e));
        }
    }
    HIP_TRY(hipDeviceSynchronize());
    c->batch_cap = n;
    c->batch_all = need_all;
    return FDW_OK;
}

namespace {
struct BatchScope {      // the context's single-shot buffers step aside for the batch ones while a batch runs
    fdw_ctx* c;
    BatchScope(fdw_ctx* ctx, int n, int dsx, bool illum) : c(ctx)
    {
        swap();
        c->nbatch = n; c->batch_dsx = dsx; c->batch_nt = c->prm.nt; c->batch_illum = illum;
    }
    ~BatchScope() { swap(); c->nbatch = 1; c->batch_dsx = 0; c->batch_illum = false; }
    void swap()
    {
        for (int i = 0; i < 8; i++) std::swap(c->fld[i], c->bfld[i]);
        std::swap(c->d_v2, c->b_v2);
        std::swap(c->d_img, c->b_img);
        std::swap(c->d_dobs, c->b_dobs);
    }
};
}  // namespace

// the batch's squared models into b_v2: host-given (v2_all [nshots][nxe][nze]) or the border models of draws [draw_offset + b T, ...) on the
// resident interior model (the shots' draws are consecutive in the stream: one launch generates them all)
static int batch_models(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset)
{
    hipStream_t s = c->stream;
    const long long draws = fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    const size_t ne = (size_t)c->prm.nxe * c->prm.nze, fe = field_elems(c);
    if (!v2_all) {
        HIP_TRY(hipStreamSynchronize(s));                     // a larger draw buffer replaces one the stream may still be reading
        FDW_TRY(ensure_draws(c, draws * nshots));
        hipError_t e = launch_rand_stream(base_at(kGlibcDiscard + draw_offset), c->d_jump, draws * nshots, c->d_draws, s);
        if (e != hipSuccess) return fail(FDW_EHIP, "rand_stream launch failed: %s", hipGetErrorString(e));
    }
    for (int b = 0; b < nshots; b++) {
        if (v2_all) {
            HIP_TRY(hipMemcpy2DAsync(c->b_v2 + b * fe, (size_t)c->pitch * sizeof(float), v2_all + b * ne, (size_t)c->prm.nze * sizeof(float),
                                     (size_t)c->prm.nze * sizeof(float), c->nxl, hipMemcpyHostToDevice, s));
        } else {
            BorderArgs ba{c->d_vp, c->d_draws + (size_t)b * draws, nullptr, c->b_v2 + b * fe, c->nx, c->nz, c->prm.nxb, c->prm.nzb, c->pitch};
            hipError_t e = launch_extendvel(ba, s);
            if (e != hipSuccess) return fail(FDW_EHIP, "border model launch failed: %s", hipGetErrorString(e));
        }
    }
    return FDW_OK;
}

// the per-shot accumulator fields of a batch with illumination: one more batch buffer, kept apart from the others so that fdw_shot_batch's
// own allocation stays what it is
static int ensure_batch_illum(fdw_ctx* c, int n)
{
    if (c->b_illum && c->b_illum_cap >= n) return FDW_OK;
    if (c->b_illum) (void)hipFree(c->b_illum);
    c->b_illum = nullptr;
    c->b_illum_cap = 0;
    const size_t bytes = field_elems(c) * (size_t)n * sizeof(float);
    hipError_t e = hipMalloc((void**)&c->b_illum, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c->b_illum = nullptr;
        return fail(FDW_ENOMEM, "batch of %d shots: hipMalloc(%zu bytes) for the illumination failed: %s", n, bytes, hipGetErrorString(e));
    }
    c->b_illum_cap = n;
    return FDW_OK;
}

// the interiors of `nshots` host arrays [nx][nz] into / out of the batch's fields (b_img, b_illum)
static int batch_interiors_to_device(fdw_ctx* c, float* d_dst, const float* h_src, int nshots)
{
    const size_t ni = (size_t)c->nx * c->nz, fe = field_elems(c);
    HIP_TRY(hipMemsetAsync(d_dst, 0, fe * nshots * sizeof(float), c->stream));
    for (int b = 0; b < nshots; b++)
        HIP_TRY(hipMemcpy2DAsync(d_dst + b * fe + (size_t)c->prm.nxb * c->pitch + c->prm.nzb, (size_t)c->pitch * sizeof(float), h_src + b * ni,
                                 (size_t)c->nz * sizeof(float), (size_t)c->nz * sizeof(float), c->nx, hipMemcpyHostToDevice, c->stream));
    return FDW_OK;
}
static int batch_interiors_to_host(fdw_ctx* c, float* h_dst, const float* d_src, int nshots)
{
    const size_t ni = (size_t)c->nx * c->nz, fe = field_elems(c);
    for (int b = 0; b < nshots; b++)
        HIP_TRY(hipMemcpy2DAsync(h_dst + b * ni, (size_t)c->nz * sizeof(float), d_src + b * fe + (size_t)c->prm.nxb * c->pitch + c->prm.nzb,
                                 (size_t)c->pitch * sizeof(float), (size_t)c->nz * sizeof(float), c->nx, hipMemcpyDeviceToHost, c->stream));
    return FDW_OK;
}

// the source rows of a batch of point-source shots: rows the forward loop time-steps
static int check_batch_source_rows(const fdw_ctx* c, int nshots, int sx0, int dsx)
{
    const int sx_last = sx0 + (nshots - 1) * dsx;
    if (std::min(sx0, sx_last) < 0 || std::max(sx0, sx_last) >= c->prm.nxe || std::max(sx0, sx_last) >= c->upd_x1)
        return fail(FDW_EINVAL, "source rows %d..%d leave the rows the reference time-steps (< %d)", sx0, sx_last, c->upd_x1);
    return FDW_OK;
}

// fdw_shot_batch, with x.illum fdw_shot_batch_illum, with x.residual fdw_shot_batch_residual.  x.line (fdw_shot_line_batch and its kin):
// `samples` holds the shots' line-source gathers [nshots][nx][nt] in place of the wavelet and (sx0, dsx): one more batch buffer, b_wav
// [shot][nt][nx], from which every forward launch takes a row per shot.
static int shot_batch_impl(fdw_ctx* c, const char* who, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                           const float* samples, const float* d_obs, float* imloc, const ShotExtras& x)
{
    if (!c || !samples || !d_obs || !imloc) return fail(FDW_EINVAL, "NULL argument");
    if (nshots < 1) return fail(FDW_EINVAL, "nshots=%d", nshots);
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "%s needs a full-grid context", who);
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "no interior to image");
    if (!v2_all && !c->model_resident) return fail(FDW_ESTATE, "no model: pass v2_all or call fdw_model_resident first");
    const int nt = c->prm.nt;
    const size_t ni = (size_t)c->nx * c->nz, ne = (size_t)c->prm.nxe * c->prm.nze, ng = (size_t)c->nx * nt, fe = field_elems(c);
    if (!x.line) FDW_TRY(check_batch_source_rows(c, nshots, sx0, dsx));
    HIP_TRY(hipSetDevice(c->device));
    const long long draws = fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    auto one_by_one = [&] {
        for (int b = 0; b < nshots; b++) {
            if (!v2_all) FDW_TRY(fdw_dev_extendvel_linear(c, draw_offset + (unsigned long long)b * draws, nullptr));
            FDW_TRY(shot_impl(c, v2_all ? v2_all + b * ne : nullptr, sx0 + b * dsx, sz, gz, x.line ? samples + b * ng : samples, d_obs + b * ng, imloc + b * ni,
                              nullptr, nullptr, x.of_shot(b, ni, ng)));
        }
        return (int)FDW_OK;
    };
    auto fallback = [&] { batch_part_ran(c, false); return one_by_one(); };
    if (!batch_ok(c)) return fallback();      // a regime the batched launches do not cover
    if (nshots == 1) { batch_part_ran(c, true); return one_by_one(); }      // nothing to gain
    int rc;
    if ((rc = ensure_work_buffers(c, 8, true))) return rc;
    if ((rc = ensure_batch_buffers(c, nshots, true)) == FDW_ENOMEM) return fallback();      // no room for the batch
    if (!rc && x.illum && (rc = ensure_batch_illum(c, nshots)) == FDW_ENOMEM) return fallback();      // ... or for its accumulators
    if (!rc && x.residual && (rc = ensure_cap(&c->b_rec, &c->b_rec_cap, ng * nshots)) == FDW_ENOMEM) return fallback();      // ... or its modelled gathers
    if (!rc && x.line && (rc = ensure_cap(&c->b_wav, &c->b_wav_cap, ng * nshots)) == FDW_ENOMEM) return fallback();      // ... or its line-source gathers
    if (!rc) batch_part_ran(c, true);
    if (rc || (rc = x.line ? gathers_to_device(c, samples, c->b_wav, nshots) : upload_source(c, samples, nt))) return rc;
    hipStream_t s = c->stream;
    if ((rc = gathers_to_device(c, d_obs, c->b_dobs, nshots))) return rc;      // [shot][nx][nt] -> [shot][nt][nx]
    if ((rc = batch_models(c, nshots, v2_all, draw_offset))) return rc;
    for (int i = 0; i < 8; i++) HIP_TRY(hipMemsetAsync(c->bfld[i], 0, fe * nshots * sizeof(float), s));    // R:496-497, R:511-514
    if ((rc = batch_interiors_to_device(c, c->b_img, imloc, nshots))) return rc;
    if (x.illum && (rc = batch_interiors_to_device(c, c->b_illum, x.illum, nshots))) return rc;
    {
        BatchScope scope(c, nshots, dsx, x.illum != nullptr);
        int ip = 0, ipp = 1;
        const Forward f = device_source(c, x.line, sx0, sz, c->b_wav).recording(x.residual ? c->b_rec : nullptr, gz).illuminating(x.illum ? c->b_illum : nullptr);
        if ((rc = steps_loop(c, c->fld, c->d_v2, f, 0, nt, 0, &ip, &ipp, s))) return rc;
        if (x.residual && (rc = gather_residual(c->d_dobs, c->b_rec, c->d_dobs, ng * nshots, s))) return rc;      // d_dobs: the batch's [shot][nt][nx]
        for (int b = 0; b < nshots && nt > 0; b++)
            if ((rc = fdw_dev_taper_finalize(c, c->fld[ip] + b * fe, s))) return rc;
        float* src[4];
        source_buffers(c, ip, ipp, src);
        if ((rc = back_loop(c, src, c->fld + 4, gz, nt, SnapPlan{}, x.dtt))) return rc;
    }
    if (x.resid && (rc = gathers_to_host(c, c->b_dobs, nshots, x.resid))) return rc;
    if (x.illum && (rc = batch_interiors_to_host(c, x.illum, c->b_illum, nshots))) return rc;
    if ((rc = batch_interiors_to_host(c, imloc, c->b_img, nshots))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return FDW_OK;
}

extern "C" int fdw_shot_batch(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                              const float* srce, const float* d_obs, float* imloc)
{
    if (!c) return fail(FDW_EINVAL, "NULL argument");
    batch_begin(c);
    return batch_end(c, nshots, shot_batch_impl(c, "fdw_shot_batch", nshots, v2_all, draw_offset, sx0, dsx, sz, gz, srce, d_obs, imloc, ShotExtras{}));
}

// How many shots of a batch go through at once: what the budget fdw_shot_batch_max counts with (batch_budget) holds of `fields` fields and `gathers`
// gathers [nt][nx] per shot.  A larger batch goes through in parts of that size: the parts are independent, the bytes the same.
static int batch_part(const fdw_ctx* c, int nshots, int fields, int gathers)
{
    const size_t ng = (size_t)c->nx * c->prm.nt;
    const long by_mem = (long)(batch_budget(c) / (((size_t)fields * field_elems(c) + (size_t)gathers * ng) * sizeof(float)));
    return (int)std::max<long>(1, std::min<long>(by_mem, nshots));
}
// shot_batch_impl in parts of what batch_part allows for `fields` fields and `gathers` gathers per shot
static int shot_batch_in_parts(fdw_ctx* c, const char* who, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                               const float* samples, const float* d_obs, float* imloc, const ShotExtras& x, int fields, int gathers)
{
    const int part = batch_part(c, nshots, fields, gathers);
    const size_t ni = (size_t)c->nx * c->nz, ne = (size_t)c->prm.nxe * c->prm.nze, ng = (size_t)c->nx * c->prm.nt;
    const unsigned long long draws = (unsigned long long)fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    batch_begin(c);
    for (int b0 = 0; b0 < nshots; b0 += part) {
        const int nb = std::min(part, nshots - b0);
        FDW_TRY(shot_batch_impl(c, who, nb, v2_all ? v2_all + b0 * ne : nullptr, draw_offset + b0 * draws, sx0 + b0 * dsx, dsx, sz, gz,
                                x.line && samples ? samples + b0 * ng : samples, d_obs ? d_obs + b0 * ng : nullptr, imloc ? imloc + b0 * ni : nullptr,
                                x.of_shot(b0, ni, ng)));
    }
    return batch_end(c, nshots, FDW_OK);
}

// ---- a batch of excitation shots (definitions in fdwave.h) ----
// The regime of its batched launches: fdw_shot_batch's (the one-step ring family: orders <= 8, neither the pipeline nor the two-step regime)
// without its conditions on the backward loop -- the pick loop is a line-source forward loop, which injects only the receiver rows the loop
// time-steps, so ragged compat grids batch too.
static bool excitation_batch_ok(const fdw_ctx* c)
{
    return c->prm.dialect == FDW_DIALECT_RTM && c->h <= kMaxFastHalfOrder && !c->use_generic && !two_step_pays(c) && !pipe_pays(c);
}

static int ensure_peaks(fdw_ctx* c, int n)
{
    if (c->peak_cap >= n) return FDW_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned* p = nullptr;
    hipError_t e = hipMalloc((void**)&p, (size_t)n * sizeof(unsigned));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FDW_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    (void)hipFree(c->d_peak);
    c->d_peak = p;
    c->peak_cap = n;
    return FDW_OK;
}

// One part of fdw_shot_excitation_batch: `nshots` shots whose images are added to imloc in shot order.  Batched, it works in
// fdw_shot_batch's buffers: bfld[0..1] the source fields, bfld[2..3] the receiver fields, bfld[4] amp, bfld[5] texc, bfld[6] exc (which the
// stack kernel then overwrites with the running images), b_dobs the time-reversed gathers [shot][nt][nx]; the running image is c->d_img.
static int excitation_batch_part(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                                 const float* srce, const float* d_obs, float eps, float* imloc, float* stack, float* exc, float* amp, int* texc, bool room)
{
    const int nt = c->prm.nt;
    const size_t ni = (size_t)c->nx * c->nz, ne = (size_t)c->prm.nxe * c->prm.nze, ng = (size_t)c->nx * nt, fe = field_elems(c);
    const long long draws = fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    auto one_by_one = [&] {
        for (int b = 0; b < nshots; b++) {
            if (!v2_all) FDW_TRY(fdw_dev_extendvel_linear(c, draw_offset + (unsigned long long)b * draws, nullptr));
            FDW_TRY(shot_excitation_impl(c, v2_all ? v2_all + b * ne : nullptr, sx0 + b * dsx, sz, gz, srce, d_obs + b * ng, eps, imloc, exc ? exc + b * ni : nullptr,
                                         amp ? amp + b * ni : nullptr, texc ? texc + b * ni : nullptr, nullptr, nullptr));
            if (stack) memcpy(stack + b * ni, imloc, ni * sizeof(float));
        }
        return (int)FDW_OK;
    };
    auto fallback = [&] { batch_part_ran(c, false); return one_by_one(); };
    if (!excitation_batch_ok(c) || !room) return fallback();      // a regime the batched launches do not cover, or a budget below one shot
    if (nshots == 1) { batch_part_ran(c, true); return one_by_one(); }      // nothing to gain
    int rc;
    if ((rc = ensure_work_buffers(c, 8, true))) return rc;
    if ((rc = ensure_batch_buffers(c, nshots, true)) == FDW_ENOMEM) return fallback();      // no room for the batch
    if (!rc && (rc = ensure_peaks(c, nshots)) == FDW_ENOMEM) return fallback();
    if (!rc) batch_part_ran(c, true);
    if (rc || (rc = upload_source(c, srce, nt))) return rc;
    hipStream_t s = c->stream;
    if ((rc = reversed_gathers_to_device(c, d_obs, c->b_dobs, nshots))) return rc;
    if ((rc = batch_models(c, nshots, v2_all, draw_offset))) return rc;
    for (int i = 0; i < 7; i++) HIP_TRY(hipMemsetAsync(c->bfld[i], 0, fe * nshots * sizeof(float), s));
    if ((rc = image_to_device(c, imloc, c->d_img))) return rc;
    {
        BatchScope scope(c, nshots, dsx, false);
        int ip = 0, ipp = 1, rp = 0, rpp = 1;
        // batch_ok: one-step passes only, so each loop stays in the first two of the four buffers it is handed
        const Forward fwd = point_source(c->d_srce, sx0, sz).exciting(Exc::maps, c->fld[4], (int*)c->fld[5], 0);
        if ((rc = steps_loop(c, c->fld, c->d_v2, fwd, 0, nt, 0, &ip, &ipp, s))) return rc;
        const Forward bwd = line_source(c->d_dobs, gz).exciting(Exc::pick, c->fld[6], (int*)c->fld[5], nt);
        if ((rc = steps_loop(c, c->fld + 2, c->d_v2, bwd, 0, nt, 0, &rp, &rpp, s))) return rc;
    }
    if (exc && (rc = batch_interiors_to_host(c, exc, c->bfld[6], nshots))) return rc;      // before the running images take its place
    if (amp && (rc = batch_interiors_to_host(c, amp, c->bfld[4], nshots))) return rc;
    if (texc && (rc = batch_interiors_to_host(c, (float*)texc, c->bfld[5], nshots))) return rc;
    if ((rc = exc_image(c, c->bfld[6], c->bfld[4], eps, c->d_img, stack ? c->bfld[6] : nullptr, nshots, s))) return rc;
    if (stack && (rc = batch_interiors_to_host(c, stack, c->bfld[6], nshots))) return rc;
    if ((rc = image_to_host(c, imloc, c->d_img))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return FDW_OK;
}

extern "C" int fdw_shot_excitation_batch(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                                         const float* srce, const float* d_obs, float eps, float* imloc, float* stack, float* exc, float* amp, int* texc)
{
    if (!c) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "excitation-amplitude imaging", "fdw_shot_excitation_batch"));
    if (!srce || !d_obs || !imloc) return fail(FDW_EINVAL, "NULL argument");
    if (nshots < 1) return fail(FDW_EINVAL, "nshots=%d", nshots);
    if (!v2_all && !c->model_resident) return fail(FDW_ESTATE, "no model: pass v2_all or call fdw_model_resident first");
    FDW_TRY(check_batch_source_rows(c, nshots, sx0, dsx));
    FDW_TRY(check_exc_shot(c, "fdw_shot_excitation_batch", sx0, sz, gz, eps));
    HIP_TRY(hipSetDevice(c->device));
    if (v2_all) c->v2_resident = false;
    // per shot the batch holds fdw_shot_batch's eleven fields (of which it uses two source and two receiver fields, v2, amp, texc and exc)
    // and one gather [nt][nx]
    const size_t ni = (size_t)c->nx * c->nz, ne = (size_t)c->prm.nxe * c->prm.nze, ng = (size_t)c->nx * c->prm.nt;
    const bool room = batch_budget(c) >= (11 * field_elems(c) + ng) * sizeof(float);      // a budget below ONE shot: no batch buffers at all
    const int part = room ? batch_part(c, nshots, 11, 1) : nshots;
    const unsigned long long draws = (unsigned long long)fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    batch_begin(c);
    for (int b0 = 0; b0 < nshots; b0 += part) {      // in shot order: imloc is carried from part to part
        const int nb = std::min(part, nshots - b0);
        FDW_TRY(excitation_batch_part(c, nb, v2_all ? v2_all + b0 * ne : nullptr, draw_offset + b0 * draws, sx0 + b0 * dsx, dsx, sz, gz, srce, d_obs + b0 * ng, eps,
                                      imloc, stack ? stack + b0 * ni : nullptr, exc ? exc + b0 * ni : nullptr, amp ? amp + b0 * ni : nullptr,
                                      texc ? texc + b0 * ni : nullptr, room));
    }
    return batch_end(c, nshots, FDW_OK);
}

// fdw_shot_batch whose forward loop also accumulates every shot's source illumination.  The batch holds one field more per shot than
// fdw_shot_batch_max counts (11), so a batch larger than twelve fields per shot allow within the same budget goes through in parts of that
// size: the parts are independent, the bytes the same.
extern "C" int fdw_shot_batch_illum(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                                    const float* srce, const float* d_obs, float* imloc, float* illum)
{
    if (!c || !illum) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "source illumination", "fdw_shot_batch_illum"));
    if (nshots < 1) return fail(FDW_EINVAL, "nshots=%d", nshots);
    ShotExtras x;
    x.illum = illum;
    return shot_batch_in_parts(c, "fdw_shot_batch_illum", nshots, v2_all, draw_offset, sx0, dsx, sz, gz, srce, d_obs, imloc, x, 12, 0);
}

// fdw_shot_batch whose forward loop also records every shot's modelled gather (and, with illum, accumulates its illumination in the same
// launch), migrating d_obs - d_mod.  The batch holds the modelled gathers and, with illum, one field more per shot than fdw_shot_batch_max
// counts: a batch larger than the same budget allows goes through in parts -- independent, the bytes the same.
extern "C" int fdw_shot_batch_residual(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                                       const float* srce, const float* d_obs, float* imloc, float* illum, float* resid)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_single_shot_ctx(c, "residual migration", "fdw_shot_batch_residual"));
    FDW_TRY(check_record_depth(c, gz));
    if (nshots < 1) return fail(FDW_EINVAL, "nshots=%d", nshots);
    ShotExtras x;
    x.illum = illum; x.residual = true; x.resid = resid;
    return shot_batch_in_parts(c, "fdw_shot_batch_residual", nshots, v2_all, draw_offset, sx0, dsx, sz, gz, srce, d_obs, imloc, x, illum ? 12 : 11, 1);
}

// ---- batches of line-source shots (definitions in fdwave.h) ----
// fdw_shot_line (illum == NULL or not) / fdw_shot_line_residual for `nshots` shots: shot_batch_impl with the shots' line gathers in place of the
// moving point source.  On top of fdw_shot_batch's eleven fields per shot the batch holds the line gathers, with illum the accumulators and
// with residual the modelled gathers: parts by batch_part.
static int shot_line_batch(fdw_ctx* c, const char* who, int nshots, const float* v2_all, unsigned long long draw_offset, int sz, int gz,
                           const float* wav_all, const float* d_obs, float* imloc, float* illum, bool residual, float* resid)
{
    if (!c || !wav_all) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "line sources", who));
    FDW_TRY(check_line_args(c, who, sz, gz, residual, illum != nullptr, true));
    if (nshots < 1) return fail(FDW_EINVAL, "nshots=%d", nshots);
    ShotExtras x;
    x.line = true; x.illum = illum; x.residual = residual; x.resid = resid;
    return shot_batch_in_parts(c, who, nshots, v2_all, draw_offset, -1, 0, sz, gz, wav_all, d_obs, imloc, x, illum ? 12 : 11, residual ? 2 : 1);
}

extern "C" int fdw_shot_line_batch(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sz, int gz, const float* wav_all,
                                   const float* d_obs, float* imloc, float* illum)
{
    return shot_line_batch(c, "fdw_shot_line_batch", nshots, v2_all, draw_offset, sz, gz, wav_all, d_obs, imloc, illum, false, nullptr);
}

extern "C" int fdw_shot_line_batch_residual(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sz, int gz,
                                            const float* wav_all, const float* d_obs, float* imloc, float* illum, float* resid)
{
    return shot_line_batch(c, "fdw_shot_line_batch_residual", nshots, v2_all, draw_offset, sz, gz, wav_all, d_obs, imloc, illum, true, resid);
}

// `nshots` recorded gathers (fdw_record_shot) through one launch per time step for the whole batch where batch_ok holds, one shot after the
// other otherwise; models as fdw_shot_batch takes them.  data [nshots][nx][nt].
// line (fdw_record_shot_line_batch): `samples` holds the shots' line-source gathers [nshots][nx][nt] in place of the wavelet and (sx0, dsx)
static int record_batch_impl(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                             const float* samples, float* data, bool line)
{
    if (!c || !samples || !data) return fail(FDW_EINVAL, "NULL argument");
    if (nshots < 1) return fail(FDW_EINVAL, "nshots=%d", nshots);
    FDW_TRY(check_record_depth(c, gz));
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_record_shot_batch needs a full-grid context");
    if (c->nx <= 0) return fail(FDW_EINVAL, "no receiver rows");
    if (!v2_all && !c->model_resident) return fail(FDW_ESTATE, "no model: pass v2_all or call fdw_model_resident first");
    const int nt = c->prm.nt;
    const size_t ne = (size_t)c->prm.nxe * c->prm.nze, ng = (size_t)c->nx * nt, fe = field_elems(c);
    if (!line) FDW_TRY(check_batch_source_rows(c, nshots, sx0, dsx));
    HIP_TRY(hipSetDevice(c->device));
    const long long draws = fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    auto one_by_one = [&] {
        for (int b = 0; b < nshots; b++) {
            if (!v2_all) FDW_TRY(fdw_dev_extendvel_linear(c, draw_offset + (unsigned long long)b * draws, nullptr));
            FDW_TRY(record_impl(c, v2_all ? v2_all + b * ne : nullptr, sx0 + b * dsx, sz, gz, line ? samples + b * ng : samples, data + b * ng, nullptr, nullptr, line));
        }
        return (int)FDW_OK;
    };
    batch_begin(c);
    if (nshots == 1 || !batch_ok(c)) return one_by_one();
    int rc;
    if ((rc = ensure_batch_buffers(c, nshots, true)) == FDW_ENOMEM) return one_by_one();
    if (!rc && line && (rc = ensure_cap(&c->b_wav, &c->b_wav_cap, ng * nshots)) == FDW_ENOMEM) return one_by_one();
    if (!rc) batch_part_ran(c, true);      // no part loop here: the whole batch or, above, the shots one by one (fdw_batch_parts 1 or 0)
    if (rc || (rc = line ? gathers_to_device(c, samples, c->b_wav, nshots) : upload_source(c, samples, nt)) || (rc = batch_models(c, nshots, v2_all, draw_offset)))
        return rc;
    hipStream_t s = c->stream;
    for (int i = 0; i < 2; i++) HIP_TRY(hipMemsetAsync(c->bfld[i], 0, fe * nshots * sizeof(float), s));    // R:496-497
    {
        BatchScope scope(c, nshots, dsx, false);
        int ip = 0, ipp = 1;
        const Forward f = device_source(c, line, sx0, sz, c->b_wav).recording(c->d_dobs, gz);      // d_dobs: the batch's [shot][nt][nx]
        if ((rc = steps_loop(c, c->fld, c->d_v2, f, 0, nt, 0, &ip, &ipp, s))) return rc;
    }
    if ((rc = gathers_to_host(c, c->b_dobs, nshots, data))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return FDW_OK;
}

extern "C" int fdw_record_shot_batch(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                                     const float* srce, float* data)
{
    if (!srce) return fail(FDW_EINVAL, "NULL argument");
    return record_batch_impl(c, nshots, v2_all, draw_offset, sx0, dsx, sz, gz, srce, data, false);
}

extern "C" int fdw_record_shot_line_batch(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sz, int gz, const float* wav_all,
                                          float* data)
{
    if (!c || !wav_all) return fail(FDW_EINVAL, "NULL argument");
    FDW_TRY(check_single_shot_ctx(c, "line sources", "fdw_record_shot_line_batch"));
    FDW_TRY(check_line_args(c, "fdw_record_shot_line_batch", sz, gz, true, false));
    return record_batch_impl(c, nshots, v2_all, draw_offset, -1, 0, sz, gz, wav_all, data, true);
}

// ---- batches of Born shots (definitions in fdwave.h) ----
// The regime of the batched launches: fdw_record_shot_batch's, where the fused Born kernel runs
static bool born_batch_ok(const fdw_ctx* c) { return batch_ok(c) && born_fused(c); }

// One part of fdw_born_shot_batch / fdw_born_shot_line_batch: `nshots` independent shots.  Batched, it works in fdw_shot_batch's buffers:
// bfld[0..1] the background pairs, bfld[2..3] the scattered pairs, b_v2 the models, b_dobs the scattered trace rows [shot][nt][nx], b_wav the
// line gathers; b_born_rec0 the background trace rows when data0 is asked for; ONE reflectivity, c->d_born_m, for all shots.
static int born_batch_part(fdw_ctx* c, const char* who, int nshots, const float* v2_all, unsigned long long draw_offset, const float* m, int kind, int sx0,
                           int dsx, int sz, int gz, const float* samples, float* data, float* data0, bool line, bool room)
{
    const int nt = c->prm.nt;
    const size_t ne = (size_t)c->prm.nxe * c->prm.nze, ng = (size_t)c->nx * nt, fe = field_elems(c);
    const long long draws = fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    auto one_by_one = [&] {
        for (int b = 0; b < nshots; b++) {
            if (!v2_all) FDW_TRY(fdw_dev_extendvel_linear(c, draw_offset + (unsigned long long)b * draws, nullptr));
            FDW_TRY(born_shot_impl(c, who, v2_all ? v2_all + b * ne : nullptr, m, kind, sx0 + b * dsx, sz, gz, line ? samples + b * ng : samples, data + b * ng,
                                   data0 ? data0 + b * ng : nullptr, line));
        }
        return (int)FDW_OK;
    };
    auto fallback = [&] { batch_part_ran(c, false); return one_by_one(); };
    if (!born_batch_ok(c) || !room) return fallback();      // a regime the batched launches do not cover, or a budget below one shot
    if (nshots == 1) { batch_part_ran(c, true); return one_by_one(); }      // nothing to gain
    int rc;
    if ((rc = alloc_zero(&c->d_born_m, fe))) return rc;
    if ((rc = ensure_batch_buffers(c, nshots, true)) == FDW_ENOMEM) return fallback();      // no room for the batch
    if (!rc && data0 && (rc = ensure_cap(&c->b_born_rec0, &c->b_born_rec0_cap, ng * nshots)) == FDW_ENOMEM) return fallback();      // ... or its background gathers
    if (!rc && line && (rc = ensure_cap(&c->b_wav, &c->b_wav_cap, ng * nshots)) == FDW_ENOMEM) return fallback();      // ... or its line-source gathers
    if (!rc) batch_part_ran(c, true);
    if (rc || (rc = line ? gathers_to_device(c, samples, c->b_wav, nshots) : upload_source(c, samples, nt)) || (rc = batch_models(c, nshots, v2_all, draw_offset)))
        return rc;
    hipStream_t s = c->stream;
    for (int i = 0; i < 4; i++) HIP_TRY(hipMemsetAsync(c->bfld[i], 0, fe * nshots * sizeof(float), s));
    if ((rc = image_to_device(c, m, c->d_born_m))) return rc;
    {
        BatchScope scope(c, nshots, dsx, false);
        // d_dobs: the batch's [shot][nt][nx]
        if ((rc = born_loop(c, c->fld[0], c->fld[1], c->fld[2], c->fld[3], c->d_v2, c->d_born_m, kind, device_source(c, line, sx0, sz, c->b_wav), gz, c->d_dobs,
                            data0 ? c->b_born_rec0 : nullptr, 0, nt, 0, s)))
            return rc;
    }
    if ((rc = gathers_to_host(c, c->b_dobs, nshots, data))) return rc;
    if (data0 && (rc = gathers_to_host(c, c->b_born_rec0, nshots, data0))) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return FDW_OK;
}

// the checks of both batched Born calls, then the parts.  Per shot the batch holds fdw_shot_batch's eleven fields (of which it uses the two
// pairs and v2) and the scattered gather [nt][nx], with data0 the background gather, of a line batch the line gather: parts by batch_part.
static int born_batch_impl(fdw_ctx* c, const char* who, int nshots, const float* v2_all, unsigned long long draw_offset, const float* m, int kind, int sx0,
                           int dsx, int sz, int gz, const float* samples, float* data, float* data0, bool line)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_single_shot_ctx(c, "Born modelling", who));
    if (!m || !samples || !data) return fail(FDW_EINVAL, "%s: NULL argument", who);
    if (nshots < 1) return fail(FDW_EINVAL, "%s: nshots=%d", who, nshots);
    if (!v2_all && !c->model_resident) return fail(FDW_ESTATE, "%s: no model: pass v2_all or call fdw_model_resident first", who);
    FDW_TRY(check_born_args(c, who, kind, line ? 0 : sx0, sz, gz));
    if (!line) FDW_TRY(check_batch_source_rows(c, nshots, sx0, dsx));
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "%s: no interior", who);
    HIP_TRY(hipSetDevice(c->device));
    if (v2_all) c->v2_resident = false;
    const size_t ne = (size_t)c->prm.nxe * c->prm.nze, ng = (size_t)c->nx * c->prm.nt;
    const int gathers = 1 + (data0 ? 1 : 0) + (line ? 1 : 0);
    const bool room = batch_budget(c) >= (11 * field_elems(c) + (size_t)gathers * ng) * sizeof(float);      // a budget below ONE shot: no batch buffers at all
    const int part = room ? batch_part(c, nshots, 11, gathers) : nshots;
    const unsigned long long draws = (unsigned long long)fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    batch_begin(c);
    for (int b0 = 0; b0 < nshots; b0 += part) {      // independent shots: nothing is carried from part to part
        const int nb = std::min(part, nshots - b0);
        FDW_TRY(born_batch_part(c, who, nb, v2_all ? v2_all + b0 * ne : nullptr, draw_offset + b0 * draws, m, kind, sx0 + b0 * dsx, dsx, sz, gz,
                                line ? samples + b0 * ng : samples, data + b0 * ng, data0 ? data0 + b0 * ng : nullptr, line, room));
    }
    return batch_end(c, nshots, FDW_OK);
}

extern "C" int fdw_born_shot_batch(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, const float* m, int kind, int sx0, int dsx,
                                   int sz, int gz, const float* srce, float* data, float* data0)
{
    return born_batch_impl(c, "fdw_born_shot_batch", nshots, v2_all, draw_offset, m, kind, sx0, dsx, sz, gz, srce, data, data0, false);
}

extern "C" int fdw_born_shot_line_batch(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, const float* m, int kind, int sz, int gz,
                                        const float* wav_all, float* data, float* data0)
{
    return born_batch_impl(c, "fdw_born_shot_line_batch", nshots, v2_all, draw_offset, m, kind, -1, 0, sz, gz, wav_all, data, data0, true);
}

// mod_main's shot loop (M:140-174) for `nshots` consecutive shots on its one velocity model, one launch per time step for all of them
extern "C" int fdw_model_shot_batch(fdw_ctx* c, int nshots, const float* vel2, int sx0, int dsx, int sz, int gz, const float* srce, int nt, float* data)
{
    if (!c || !vel2 || !data || (!srce && nt > 0)) return fail(FDW_EINVAL, "NULL argument");
    if (c->prm.dialect != FDW_DIALECT_MOD) return fail(FDW_ESTATE, "fdw_model_shot_batch needs a context created with dialect = FDW_DIALECT_MOD");
    if (!is_full_grid(c)) return fail(FDW_EINVAL, "fdw_model_shot_batch needs a full-grid context");
    if (nshots < 1 || nt < 0) return fail(FDW_EINVAL, "nshots=%d nt=%d", nshots, nt);
    if (gz < c->prm.nzb || gz >= c->prm.nzb + c->nz)
        return fail(FDW_EINVAL, "receiver depth %d is not an interior column [%d,%d)", gz, c->prm.nzb, c->prm.nzb + c->nz);
    const int sx_last = sx0 + (nshots - 1) * dsx;
    if (std::min(sx0, sx_last) < 0 || std::max(sx0, sx_last) >= c->prm.nxe) return fail(FDW_EINVAL, "source rows %d..%d leave the grid", sx0, sx_last);
    const size_t nx = c->nx, ng = nx * (size_t)nt, fe = field_elems(c);
    auto one_by_one = [&] {
        for (int b = 0; b < nshots; b++) FDW_TRY(fdw_model_shot(c, vel2, sx0 + b * dsx, sz, gz, srce, nt, data + b * ng));
        return (int)FDW_OK;
    };
    batch_begin(c);
    if (nshots == 1 || nt == 0 || nt > c->prm.nt || !batch_ok(c)) return one_by_one();
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_work_buffers(c, 2, false))) return rc;
    if ((rc = ensure_batch_buffers(c, nshots, false)) == FDW_ENOMEM) return one_by_one();      // no room for the batch: the shots one after the other
    if (!rc) batch_part_ran(c, true);      // no part loop here either
    if (rc || (rc = upload_source(c, srce, nt))) return rc;
    if ((rc = ensure_cap(&c->d_raw, &c->raw_cap, ng * nshots))) return rc;
    hipStream_t s = c->stream;
    if ((rc = upload_rows(c, c->d_v2, vel2, s))) return rc;
    HIP_TRY(hipMemsetAsync(c->bfld[0], 0, fe * nshots * sizeof(float), s));   // M:144-145
    HIP_TRY(hipMemsetAsync(c->bfld[1], 0, fe * nshots * sizeof(float), s));
    c->nbatch = nshots; c->batch_dsx = dsx; c->batch_nt = nt;
    rc = fdw_dev_model_steps(c, c->bfld[0], c->bfld[1], c->d_v2, c->d_srce, sx0, sz, gz, c->b_dobs, 0, nt, s);
    c->nbatch = 1; c->batch_dsx = 0;
    if (rc) return rc;
    // device [shot][it][ix] -> data[shot][ix][it] (M:156)
    hipError_t e = launch_gather_transpose(c->b_dobs, c->d_raw, nt, (int)nx, nshots, s);
    if (e != hipSuccess) return fail(FDW_EHIP, "gather transposition launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(data, c->d_raw, ng * nshots * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// shots that image with the second time difference of the source field (definitions in fdwave.h, "DTT imaging")
// ------------------------------------------------------------------------------------------------
// what every DTT shot entry point refuses before anything is enqueued; the ShotExtras of the call
static int dtt_shot_extras(fdw_ctx* c, const char* who, float* illum, int residual, float* resid, int gz, ShotExtras* x)
{
    FDW_TRY(check_dtt_ctx(c, who));
    if (residual != 0 && residual != 1) return fail(FDW_EINVAL, "%s: residual=%d is neither 0 nor 1", who, residual);
    if (resid && !residual) return fail(FDW_EINVAL, "%s: resid is the output of residual=1", who);
    if (residual) FDW_TRY(check_record_depth(c, gz));
    x->dtt = true; x->illum = illum; x->residual = residual != 0; x->resid = resid;
    return FDW_OK;
}

extern "C" int fdw_shot_dtt(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, const float* d_obs, float* imloc, float* illum,
                            int residual, float* resid, float* P, float* PP)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    ShotExtras x;
    FDW_TRY(dtt_shot_extras(c, "fdw_shot_dtt", illum, residual, resid, gz, &x));
    FDW_TRY(has_model(c, v2));
    if (!srce || !d_obs || !imloc) return fail(FDW_EINVAL, "fdw_shot_dtt: NULL argument");
    end_residency(c, v2);
    return shot_impl(c, v2, sx, sz, gz, srce, d_obs, imloc, P, PP, x);
}

extern "C" int fdw_shot_line_dtt(fdw_ctx* c, const float* v2, int sz, int gz, const float* wav, const float* d_obs, float* imloc, float* illum, int residual,
                                 float* resid, float* P, float* PP)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    ShotExtras x;
    FDW_TRY(dtt_shot_extras(c, "fdw_shot_line_dtt", illum, residual, resid, gz, &x));
    FDW_TRY(has_model(c, v2));
    if (!wav || !d_obs || !imloc) return fail(FDW_EINVAL, "fdw_shot_line_dtt: NULL argument");
    FDW_TRY(check_line_args(c, "fdw_shot_line_dtt", sz, gz, residual != 0, illum != nullptr, residual != 0));
    end_residency(c, v2);
    x.line = true;
    return shot_impl(c, v2, -1, sz, gz, wav, d_obs, imloc, P, PP, x);
}

// the batches: fdw_shot_batch_residual's parts (eleven fields per shot, one more with illum; one gather more with residual, one more for a line)
extern "C" int fdw_shot_batch_dtt(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz,
                                  const float* srce, const float* d_obs, float* imloc, float* illum, int residual, float* resid)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    ShotExtras x;
    FDW_TRY(dtt_shot_extras(c, "fdw_shot_batch_dtt", illum, residual, resid, gz, &x));
    if (!srce || !d_obs || !imloc) return fail(FDW_EINVAL, "fdw_shot_batch_dtt: NULL argument");
    if (nshots < 1) return fail(FDW_EINVAL, "nshots=%d", nshots);
    return shot_batch_in_parts(c, "fdw_shot_batch_dtt", nshots, v2_all, draw_offset, sx0, dsx, sz, gz, srce, d_obs, imloc, x, illum ? 12 : 11, residual ? 1 : 0);
}

extern "C" int fdw_shot_line_batch_dtt(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sz, int gz, const float* wav_all,
                                       const float* d_obs, float* imloc, float* illum, int residual, float* resid)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    ShotExtras x;
    FDW_TRY(dtt_shot_extras(c, "fdw_shot_line_batch_dtt", illum, residual, resid, gz, &x));
    if (!wav_all || !d_obs || !imloc) return fail(FDW_EINVAL, "fdw_shot_line_batch_dtt: NULL argument");
    FDW_TRY(check_line_args(c, "fdw_shot_line_batch_dtt", sz, gz, residual != 0, illum != nullptr, true));
    if (nshots < 1) return fail(FDW_EINVAL, "nshots=%d", nshots);
    x.line = true;
    return shot_batch_in_parts(c, "fdw_shot_line_batch_dtt", nshots, v2_all, draw_offset, -1, 0, sz, gz, wav_all, d_obs, imloc, x, illum ? 12 : 11,
                               residual ? 2 : 1);
}

// ------------------------------------------------------------------------------------------------
// the shot that accumulates the subsurface-offset extended image (definitions in fdwave.h, "Extended imaging")
// ------------------------------------------------------------------------------------------------
extern "C" int fdw_shot_ext(fdw_ctx* c, const float* v2, int sx, int sz, int gz, const float* srce, const float* d_obs, int H, float* imloc, float* eimg,
                            float* P, float* PP)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_ext_ctx(c, "fdw_shot_ext", H));
    FDW_TRY(has_model(c, v2));
    if (!srce || !d_obs || !eimg) return fail(FDW_EINVAL, "fdw_shot_ext: NULL argument");
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "no interior to image");
    HIP_TRY(hipSetDevice(c->device));
    const int planes = 2 * H + 1;
    const size_t fe = field_elems(c);
    if (c->eimg_planes < planes) {      // the planes of the largest H seen, before anything is enqueued
        if (c->d_eimg) (void)hipFree(c->d_eimg);
        c->d_eimg = nullptr;
        c->eimg_planes = 0;
        hipError_t e = hipMalloc((void**)&c->d_eimg, (size_t)planes * fe * sizeof(float));
        if (e != hipSuccess) {
            c->d_eimg = nullptr;
            size_t free_b = 0, total_b = 0;
            (void)hipMemGetInfo(&free_b, &total_b);
            return fail(FDW_ENOMEM, "fdw_shot_ext: the planes do not fit: %d planes x %zu bytes = %zu bytes, %zu bytes free on the device", planes,
                        fe * sizeof(float), (size_t)planes * fe * sizeof(float), free_b);
        }
        c->eimg_planes = planes;
    }
    FDW_TRY(ensure_work_buffers(c, 8, true));
    end_residency(c, v2);
    const size_t ni = (size_t)c->nx * c->nz;
    for (int j = 0; j < planes; j++) FDW_TRY(image_to_device(c, eimg + j * ni, c->d_eimg + j * fe));
    ShotExtras x;
    x.ext_H = H;
    FDW_TRY(shot_impl(c, v2, sx, sz, gz, srce, d_obs, imloc, P, PP, x));
    // (shot_impl has synchronised: the copies below are the only work left on the stream)
    for (int j = 0; j < planes; j++) FDW_TRY(image_to_host(c, eimg + j * ni, c->d_eimg + j * fe));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

// ------------------------------------------------------------------------------------------------
// least-squares migration: conjugate gradients on Born modelling and DTT imaging (definitions in fdwave.h, "Least-squares migration")
// ------------------------------------------------------------------------------------------------
static int check_lsm_ctx(const fdw_ctx* c, const char* who)
{
    FDW_TRY(check_dtt_ctx(c, who));
    if (c->nbatch > 1) return fail(FDW_ESTATE, "%s: not inside a batch of shots", who);
    return FDW_OK;
}

static int lsm_launched(hipError_t e, const char* what)
{
    return e == hipSuccess ? (int)FDW_OK : fail(FDW_EHIP, "least-squares migration: %s launch failed: %s", what, hipGetErrorString(e));
}

extern "C" int fdw_dev_dot_cells(fdw_ctx* c, const float* d_a, const float* d_b, double* d_rows, double* d_sum, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_dev_dot_cells"));
    if (!d_a || !d_b || !d_rows || !d_sum) return fail(FDW_EINVAL, "fdw_dev_dot_cells: NULL buffer");
    const BornCells C = born_cells(c);
    const int rows = std::max(C.x1 - C.x0, 0);
    hipStream_t s = pick_stream(c, stream);
    FDW_TRY(lsm_launched(launch_lsm_dot_rows(d_a, d_b, d_rows, c->pitch, C.x0, rows, C.z0, C.z1, s), "row sums"));
    return lsm_launched(launch_lsm_finish(d_rows, rows, d_sum, s), "total");
}

extern "C" int fdw_dev_dot_gather(fdw_ctx* c, const float* d_a, const float* d_b, double* d_rows, double* d_sum, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_dev_dot_gather"));
    if (!d_a || !d_b || !d_rows || !d_sum) return fail(FDW_EINVAL, "fdw_dev_dot_gather: NULL buffer");
    hipStream_t s = pick_stream(c, stream);
    FDW_TRY(lsm_launched(launch_lsm_dot_rows(d_a, d_b, d_rows, c->nx, 0, c->prm.nt, 0, c->nx, s), "row sums"));
    return lsm_launched(launch_lsm_finish(d_rows, c->prm.nt, d_sum, s), "total");
}

// steps 2 and 3 of a visit behind their checks
static int lsm_gather(fdw_ctx* c, const float* d_q, const float* d_obs, const float* d_v2, int gz, float* d_w, float* d_ws, double* d_rows, double* d_n2,
                      hipStream_t s)
{
    FDW_TRY(lsm_launched(launch_lsm_gather(d_q, d_obs, d_v2, d_w, d_ws, d_rows, c->prm.nt, c->nx, c->pitch, c->prm.nxb, gz, s), "gather"));
    return lsm_launched(launch_lsm_finish(d_rows, c->prm.nt, d_n2, s), "total");
}

extern "C" int fdw_dev_lsm_gather(fdw_ctx* c, const float* d_q, const float* d_obs, const float* d_v2, int gz, float* d_w, float* d_ws, double* d_rows,
                                  double* d_n2, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_dev_lsm_gather"));
    if (!d_q || !d_v2 || !d_ws || !d_rows || !d_n2) return fail(FDW_EINVAL, "fdw_dev_lsm_gather: NULL buffer");
    if (gz < 0 || gz >= c->zlim) return fail(FDW_EINVAL, "fdw_dev_lsm_gather: receiver depth %d outside the time-stepped columns [0,%d)", gz, c->zlim);
    return lsm_gather(c, d_q, d_obs, d_v2, gz, d_w, d_ws, d_rows, d_n2, pick_stream(c, stream));
}

extern "C" int fdw_dev_lsm_stack(fdw_ctx* c, float* d_h, const float* d_img, const float* d_v2, const float* d_mask, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_dev_lsm_stack"));
    if (!d_h || !d_img || !d_v2) return fail(FDW_EINVAL, "fdw_dev_lsm_stack: NULL buffer");
    const BornCells C = born_cells(c);
    return lsm_launched(launch_lsm_stack(d_h, d_img, d_v2, d_mask, c->pitch, C.x0, C.x1, C.z0, C.z1, pick_stream(c, stream)), "stack");
}

extern "C" int fdw_dev_lsm_update(fdw_ctx* c, float* d_m, float* d_g, const float* d_p, const float* d_h, const double* d_alpha, double* d_rows, double* d_gg,
                                  void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_dev_lsm_update"));
    if (!d_m || !d_g || !d_p || !d_h || !d_alpha || !d_rows || !d_gg) return fail(FDW_EINVAL, "fdw_dev_lsm_update: NULL buffer");
    const BornCells C = born_cells(c);
    hipStream_t s = pick_stream(c, stream);
    FDW_TRY(lsm_launched(launch_lsm_update(d_m, d_g, d_p, d_h, d_alpha, d_rows, c->pitch, C.x0, C.x1, C.z0, C.z1, s), "update"));
    return lsm_launched(launch_lsm_finish(d_rows, std::max(C.x1 - C.x0, 0), d_gg, s), "total");
}

extern "C" int fdw_dev_lsm_direction(fdw_ctx* c, float* d_p, const float* d_g, const double* d_beta, void* stream)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_dev_lsm_direction"));
    if (!d_p || !d_g || !d_beta) return fail(FDW_EINVAL, "fdw_dev_lsm_direction: NULL buffer");
    const BornCells C = born_cells(c);
    return lsm_launched(launch_lsm_direction(d_p, d_g, d_beta, c->pitch, C.x0, C.x1, C.z0, C.z1, pick_stream(c, stream)), "direction");
}

// the doubles of a visit or a solve inside c->d_lsm_d
struct LsmDoubles {
    double *rows, *sc, *n2, *hist;
};
static int lsm_doubles(fdw_ctx* c, int nshots, int nhist, LsmDoubles* d)
{
    const size_t nrows = (size_t)std::max(c->prm.nt, c->nxl);
    FDW_TRY(ensure_cap(&c->d_lsm_d, &c->lsm_d_cap, 2 * (nrows + LSM_NSCALARS + (size_t)nshots + (size_t)nhist)));
    d->rows = reinterpret_cast<double*>(c->d_lsm_d);
    d->sc = d->rows + nrows;
    d->n2 = d->sc + LSM_NSCALARS;
    d->hist = d->n2 + nshots;
    return FDW_OK;
}

// the buffers every visit works in: the Born loop's four fields and the backward loop's receiver pair, v2, the image, both gathers
static int lsm_work_buffers(fdw_ctx* c)
{
    FDW_TRY(ensure_work_buffers(c, 8, true));
    FDW_TRY(ensure_cap(&c->d_rec, &c->rec_cap, (size_t)c->nx * c->prm.nt));
    return ensure_cap(&c->d_dobs, &c->dobs_cap, (size_t)c->nx * c->prm.nt);
}

// One visit on the context's stream with the model in c->d_v2 and the wavelet in c->d_srce: d_p the direction, d_obs NULL or the shot's data
// [nt][nx] (may be c->d_dobs), d_mask NULL or the mask, d_h the stack, d_w NULL or where w goes (may be c->d_rec).  The Born loop leaves the
// background pair in fld[0..1], the newest level where an odd or even nt puts it; the scattered pair fld[2..3] becomes the two spare
// source buffers of the backward loop.
static int lsm_visit_dev(fdw_ctx* c, const float* d_p, int sx, int sz, int gz, const float* d_obs, const float* d_mask, float* d_h, double* d_rows,
                         double* d_n2, float* d_w)
{
    const int nt = c->prm.nt;
    hipStream_t s = c->stream;
    FDW_TRY(zero_fields(c, c->fld, 4));
    FDW_TRY(born_loop(c, c->fld[0], c->fld[1], c->fld[2], c->fld[3], c->d_v2, d_p, FDW_BORN_DTT, point_source(c->d_srce, sx, sz), gz, c->d_rec, nullptr, 0, nt,
                      0, s));
    const int inew = nt % 2 ? 0 : 1, iold = 1 - inew;
    if (nt > 0) FDW_TRY(fdw_dev_taper_finalize(c, c->fld[iold], s));      // as fdw_shot's forward loop leaves d_p
    FDW_TRY(lsm_gather(c, c->d_rec, d_obs, c->d_v2, gz, d_w, c->d_dobs, d_rows, d_n2, s));
    float* src[4] = {c->fld[iold], c->fld[inew], c->fld[2], c->fld[3]};
    FDW_TRY(zero_fields(c, c->fld + 4, 2));
    HIP_TRY(hipMemsetAsync(c->d_img, 0, field_elems(c) * sizeof(float), s));
    FDW_TRY(back_loop(c, src, c->fld + 4, gz, nt, SnapPlan{}, true));
    const BornCells C = born_cells(c);
    return lsm_launched(launch_lsm_stack(d_h, c->d_img, c->d_v2, d_mask, c->pitch, C.x0, C.x1, C.z0, C.z1, s), "stack");
}

// The visits of `nb` consecutive shots (source rows sx0 + b dsx) through ONE launch per time step in both loops, inside fdw_shot_batch's
// buffers: bfld[0..1] the background pairs, bfld[2..3] the scattered pairs and then the spare source buffers, bfld[4..5] the receiver pairs,
// b_v2 the models, b_img the images, b_dobs the scattered gathers and, in place, the weighted receiver data.  ONE direction d_p for all
// shots.  d_obs NULL or [nb][nt][nx], d_w NULL or [nb][nt][nx], d_n2 [nb].  The gather pass and the stack run shot by shot, in shot order:
// the bytes are those of lsm_visit_dev on each shot.
static int lsm_visit_group(fdw_ctx* c, int nb, const float* v2_part, unsigned long long draw_offset, const float* d_p, int sx0, int dsx, int sz, int gz,
                           const float* d_obs, const float* d_mask, float* d_h, double* d_rows, double* d_n2, float* d_w)
{
    const int nt = c->prm.nt;
    const size_t fe = field_elems(c), ng = (size_t)c->nx * nt;
    hipStream_t s = c->stream;
    FDW_TRY(batch_models(c, nb, v2_part, draw_offset));
    for (int i = 0; i < 6; i++) HIP_TRY(hipMemsetAsync(c->bfld[i], 0, fe * nb * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(c->b_img, 0, fe * nb * sizeof(float), s));
    BatchScope scope(c, nb, dsx, false);
    FDW_TRY(born_loop(c, c->fld[0], c->fld[1], c->fld[2], c->fld[3], c->d_v2, d_p, FDW_BORN_DTT, point_source(c->d_srce, sx0, sz), gz, c->d_dobs, nullptr, 0,
                      nt, 0, s));
    const int inew = nt % 2 ? 0 : 1, iold = 1 - inew;
    for (int b = 0; b < nb && nt > 0; b++) FDW_TRY(fdw_dev_taper_finalize(c, c->fld[iold] + b * fe, s));
    for (int b = 0; b < nb; b++)
        FDW_TRY(lsm_gather(c, c->d_dobs + b * ng, d_obs ? d_obs + b * ng : nullptr, c->d_v2 + b * fe, gz, d_w ? d_w + b * ng : nullptr, c->d_dobs + b * ng,
                           d_rows, d_n2 + b, s));
    float* src[4] = {c->fld[iold], c->fld[inew], c->fld[2], c->fld[3]};
    FDW_TRY(back_loop(c, src, c->fld + 4, gz, nt, SnapPlan{}, true));
    const BornCells C = born_cells(c);
    for (int b = 0; b < nb; b++)
        FDW_TRY(lsm_launched(launch_lsm_stack(d_h, c->d_img + b * fe, c->d_v2 + b * fe, d_mask, c->pitch, C.x0, C.x1, C.z0, C.z1, s), "stack"));
    return FDW_OK;
}

extern "C" int fdw_lsm_visit(fdw_ctx* c, const float* v2, const float* p, int sx, int sz, int gz, const float* srce, const float* d_obs, const float* mask,
                             float* h, double* n2, float* data)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_lsm_visit"));
    if (!p || !srce || !h || !n2) return fail(FDW_EINVAL, "fdw_lsm_visit: NULL argument");
    FDW_TRY(has_model(c, v2));
    FDW_TRY(check_born_args(c, "fdw_lsm_visit", FDW_BORN_DTT, sx, sz, gz));
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "fdw_lsm_visit: no interior");
    HIP_TRY(hipSetDevice(c->device));
    FDW_TRY(lsm_work_buffers(c));
    FDW_TRY(alloc_zero(&c->d_born_m, field_elems(c)));
    FDW_TRY(alloc_zero(&c->d_lsm_f[3], field_elems(c)));
    if (mask) FDW_TRY(alloc_zero(&c->d_lsm_f[4], field_elems(c)));
    LsmDoubles d;
    FDW_TRY(lsm_doubles(c, 1, 0, &d));
    end_residency(c, v2);
    if (v2) FDW_TRY(upload_rows(c, c->d_v2, v2, c->stream));
    FDW_TRY(upload_source(c, srce, c->prm.nt));
    FDW_TRY(image_to_device(c, p, c->d_born_m));
    FDW_TRY(image_to_device(c, h, c->d_lsm_f[3]));
    if (mask) FDW_TRY(image_to_device(c, mask, c->d_lsm_f[4]));
    if (d_obs) FDW_TRY(gathers_to_device(c, d_obs, c->d_dobs, 1));
    FDW_TRY(lsm_visit_dev(c, c->d_born_m, sx, sz, gz, d_obs ? c->d_dobs : nullptr, mask ? c->d_lsm_f[4] : nullptr, c->d_lsm_f[3], d.rows, d.n2,
                          data ? c->d_rec : nullptr));
    FDW_TRY(image_to_host(c, h, c->d_lsm_f[3]));
    HIP_TRY(hipMemcpyAsync(n2, d.n2, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (data) FDW_TRY(gathers_to_host(c, c->d_rec, 1, data));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

// The shots of a pass of visits and how they go through: where fdw_born_shot_batch and fdw_shot_batch_dtt both batch, in groups of what the
// budget holds of eleven fields and one gather per shot (the caller's own arrays are not the batch's); elsewhere, under a budget below one
// shot's share and without room on the device, one by one (part = 1).
struct LsmShots {
    int nshots;
    const float* v2_all;
    unsigned long long draw_offset;
    int sx0, dsx, sz, gz;
    int part = 1;
    bool model_set = false;      // one shot: its model stays where the first visit put it
};
// decides the groups, allocates their buffers and sets fdw_batch_parts: the groups of ONE pass (every pass runs the same groups)
static int lsm_plan(fdw_ctx* c, LsmShots* S)
{
    const size_t ng = (size_t)c->nx * c->prm.nt;
    const bool room = batch_budget(c) >= (11 * field_elems(c) + ng) * sizeof(float);
    bool batched = S->nshots > 1 && born_batch_ok(c) && room;
    S->part = batched ? batch_part(c, S->nshots, 11, 1) : 1;
    if (S->part > 1) {
        const int rc = ensure_batch_buffers(c, S->part, true);
        if (rc == FDW_ENOMEM) { S->part = 1; batched = false; }      // no room on the device: one by one
        else if (rc) return rc;
    }
    batch_begin(c);
    for (int b0 = 0; b0 < S->nshots; b0 += S->part) batch_part_ran(c, batched);
    (void)batch_end(c, S->nshots, FDW_OK);
    if (S->v2_all) c->v2_resident = false;
    return FDW_OK;
}
// One pass: V_b(d_dir, d_obs ? d_obs[b] : NULL) for every shot in order, stacked into d_stack; the shots' n2 into d.n2, w into d_w (NULL ok).
// d_obs, d_w: device [nshots][nt][nx].  A group of one shot runs the single-shot code.
static int lsm_pass(fdw_ctx* c, LsmShots* S, const float* d_dir, const float* d_obs, const float* d_mask, float* d_stack, const LsmDoubles& d, float* d_w)
{
    const size_t ne = (size_t)c->prm.nxe * c->prm.nze, ng = (size_t)c->nx * c->prm.nt;
    const unsigned long long draws = (unsigned long long)fdw_border_draws(c->nx, c->nz, c->prm.nxb, c->prm.nzb);
    for (int b0 = 0; b0 < S->nshots; b0 += S->part) {
        const int nb = std::min(S->part, S->nshots - b0);
        const float* obs = d_obs ? d_obs + b0 * ng : nullptr;
        float* w = d_w ? d_w + b0 * ng : nullptr;
        const unsigned long long draw0 = S->draw_offset + (unsigned long long)b0 * draws;
        if (nb > 1) {
            FDW_TRY(lsm_visit_group(c, nb, S->v2_all ? S->v2_all + b0 * ne : nullptr, draw0, d_dir, S->sx0 + b0 * S->dsx, S->dsx, S->sz, S->gz, obs, d_mask,
                                    d_stack, d.rows, d.n2 + b0, w));
            continue;
        }
        if (S->nshots > 1 || !S->model_set)
            FDW_TRY(S->v2_all ? upload_rows(c, c->d_v2, S->v2_all + b0 * ne, c->stream) : fdw_dev_extendvel_linear(c, draw0, nullptr));
        S->model_set = true;
        FDW_TRY(lsm_visit_dev(c, d_dir, S->sx0 + b0 * S->dsx, S->sz, S->gz, obs, d_mask, d_stack, d.rows, d.n2 + b0, w));
    }
    return FDW_OK;
}

// what fdw_lsm_visit_batch and fdw_lsm_solve refuse of their shots and models
static int check_lsm_shots(fdw_ctx* c, const char* who, int nshots, const float* v2_all, int sx0, int dsx, int sz, int gz)
{
    if (nshots < 1) return fail(FDW_EINVAL, "%s: nshots=%d", who, nshots);
    if (!v2_all && !c->model_resident) return fail(FDW_ESTATE, "%s: no model: pass v2_all or call fdw_model_resident first", who);
    FDW_TRY(check_born_args(c, who, FDW_BORN_DTT, sx0, sz, gz));
    FDW_TRY(check_batch_source_rows(c, nshots, sx0, dsx));
    if (c->nx <= 0 || c->nz <= 0) return fail(FDW_EINVAL, "%s: no interior", who);
    return FDW_OK;
}

extern "C" int fdw_lsm_visit_batch(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, const float* p, int sx0, int dsx, int sz, int gz,
                                   const float* srce, const float* d_obs, const float* mask, float* h, double* n2, float* data)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_lsm_visit_batch"));
    if (!p || !srce || !h || !n2) return fail(FDW_EINVAL, "fdw_lsm_visit_batch: NULL argument");
    FDW_TRY(check_lsm_shots(c, "fdw_lsm_visit_batch", nshots, v2_all, sx0, dsx, sz, gz));
    HIP_TRY(hipSetDevice(c->device));
    const size_t ng = (size_t)c->nx * c->prm.nt;
    FDW_TRY(lsm_work_buffers(c));
    FDW_TRY(alloc_zero(&c->d_born_m, field_elems(c)));
    FDW_TRY(alloc_zero(&c->d_lsm_f[3], field_elems(c)));
    if (mask) FDW_TRY(alloc_zero(&c->d_lsm_f[4], field_elems(c)));
    if (d_obs) FDW_TRY(ensure_cap(&c->d_lsm_dobs, &c->lsm_dobs_cap, ng * nshots));
    if (data) FDW_TRY(ensure_cap(&c->d_lsm_res, &c->lsm_res_cap, ng * nshots));
    LsmDoubles d;
    FDW_TRY(lsm_doubles(c, nshots, 0, &d));
    LsmShots S{nshots, v2_all, draw_offset, sx0, dsx, sz, gz};
    FDW_TRY(lsm_plan(c, &S));
    FDW_TRY(upload_source(c, srce, c->prm.nt));
    FDW_TRY(image_to_device(c, p, c->d_born_m));
    FDW_TRY(image_to_device(c, h, c->d_lsm_f[3]));
    if (mask) FDW_TRY(image_to_device(c, mask, c->d_lsm_f[4]));
    if (d_obs) FDW_TRY(gathers_to_device(c, d_obs, c->d_lsm_dobs, nshots));
    FDW_TRY(lsm_pass(c, &S, c->d_born_m, d_obs ? c->d_lsm_dobs : nullptr, mask ? c->d_lsm_f[4] : nullptr, c->d_lsm_f[3], d, data ? c->d_lsm_res : nullptr));
    FDW_TRY(image_to_host(c, h, c->d_lsm_f[3]));
    HIP_TRY(hipMemcpyAsync(n2, d.n2, (size_t)nshots * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (data) FDW_TRY(gathers_to_host(c, c->d_lsm_res, nshots, data));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FDW_OK;
}

extern "C" int fdw_lsm_solve(fdw_ctx* c, int nshots, const float* v2_all, unsigned long long draw_offset, int sx0, int dsx, int sz, int gz, const float* srce,
                             const float* d_obs, const float* mask, int niter, float* m, double* misfit, int verify, float* resid)
{
    if (!c) return fail(FDW_EINVAL, "ctx is NULL");
    FDW_TRY(check_lsm_ctx(c, "fdw_lsm_solve"));
    if (!srce || !d_obs || !m || !misfit) return fail(FDW_EINVAL, "fdw_lsm_solve: NULL argument");
    if (niter < 0) return fail(FDW_EINVAL, "fdw_lsm_solve: niter=%d", niter);
    if (verify != 0 && verify != 1) return fail(FDW_EINVAL, "fdw_lsm_solve: verify=%d is neither 0 nor 1", verify);
    if (resid && !verify) return fail(FDW_EINVAL, "fdw_lsm_solve: resid is the output of verify=1");
    FDW_TRY(check_lsm_shots(c, "fdw_lsm_solve", nshots, v2_all, sx0, dsx, sz, gz));
    HIP_TRY(hipSetDevice(c->device));
    const int nt = c->prm.nt;
    const size_t ng = (size_t)c->nx * nt, fbytes = field_elems(c) * sizeof(float);
    FDW_TRY(lsm_work_buffers(c));
    for (int i = 0; i < 6; i++)
        if (i != 4 || mask) FDW_TRY(alloc_zero(&c->d_lsm_f[i], field_elems(c)));
    FDW_TRY(ensure_cap(&c->d_lsm_dobs, &c->lsm_dobs_cap, ng * nshots));
    if (resid) FDW_TRY(ensure_cap(&c->d_lsm_res, &c->lsm_res_cap, ng * nshots));
    LsmDoubles d;
    FDW_TRY(lsm_doubles(c, nshots, niter + 2, &d));
    LsmShots S{nshots, v2_all, draw_offset, sx0, dsx, sz, gz};
    FDW_TRY(lsm_plan(c, &S));
    float *d_m = c->d_lsm_f[0], *d_g = c->d_lsm_f[1], *d_p = c->d_lsm_f[2], *d_h = c->d_lsm_f[3], *d_mask = mask ? c->d_lsm_f[4] : nullptr, *d_scr = c->d_lsm_f[5];
    hipStream_t s = c->stream;
    const BornCells C = born_cells(c);
    const int crows = std::max(C.x1 - C.x0, 0);
    FDW_TRY(upload_source(c, srce, nt));
    FDW_TRY(image_to_device(c, m, d_m));
    if (mask) FDW_TRY(image_to_device(c, mask, d_mask));
    FDW_TRY(gathers_to_device(c, d_obs, c->d_lsm_dobs, nshots));
    auto pass = [&](const float* d_dir, bool data, float* d_stack, float* d_w) { return lsm_pass(c, &S, d_dir, data ? c->d_lsm_dobs : nullptr, d_mask, d_stack, d, d_w); };
    HIP_TRY(hipMemsetAsync(d_g, 0, fbytes, s));
    FDW_TRY(pass(d_m, true, d_g, nullptr));
    FDW_TRY(lsm_launched(launch_lsm_dot_rows(d_g, d_g, d.rows, c->pitch, C.x0, crows, C.z0, C.z1, s), "row sums"));
    FDW_TRY(lsm_launched(launch_lsm_finish(d.rows, crows, d.sc + LSM_GG, s), "total"));
    FDW_TRY(lsm_launched(launch_lsm_scalars(d.sc, d.n2, nshots, d.hist, 0, LSM_START, s), "scalars"));
    HIP_TRY(hipMemcpyAsync(d_p, d_g, fbytes, hipMemcpyDeviceToDevice, s));
    for (int k = 0; k < niter; k++) {
        HIP_TRY(hipMemsetAsync(d_h, 0, fbytes, s));
        FDW_TRY(pass(d_p, false, d_h, nullptr));
        FDW_TRY(lsm_launched(launch_lsm_scalars(d.sc, d.n2, nshots, d.hist, k, LSM_STEP, s), "scalars"));
        FDW_TRY(lsm_launched(launch_lsm_update(d_m, d_g, d_p, d_h, d.sc + LSM_ALPHA, d.rows, c->pitch, C.x0, C.x1, C.z0, C.z1, s), "update"));
        FDW_TRY(lsm_launched(launch_lsm_finish(d.rows, crows, d.sc + LSM_GG, s), "total"));
        FDW_TRY(lsm_launched(launch_lsm_scalars(d.sc, d.n2, nshots, d.hist, k, LSM_TURN, s), "scalars"));
        FDW_TRY(lsm_launched(launch_lsm_direction(d_p, d_g, d.sc + LSM_BETA, c->pitch, C.x0, C.x1, C.z0, C.z1, s), "direction"));
    }
    if (verify) {
        HIP_TRY(hipMemsetAsync(d_scr, 0, fbytes, s));
        FDW_TRY(pass(d_m, true, d_scr, resid ? c->d_lsm_res : nullptr));
        FDW_TRY(lsm_launched(launch_lsm_scalars(d.sc, d.n2, nshots, d.hist, niter + 1, LSM_VERIFY, s), "scalars"));
        if (resid) FDW_TRY(gathers_to_host(c, c->d_lsm_res, nshots, resid));
    }
    FDW_TRY(image_to_host(c, m, d_m));
    HIP_TRY(hipMemcpyAsync(misfit, d.hist, (size_t)(niter + 1 + verify) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FDW_OK;
}

"""Host-side mirror of the reference's propagation API on top of libfdwave.so.

The reference (cuda_reference_RTM/src/fd-code.cu) exposes fd_init / fd_forward / fd_back as C
functions over file-scope globals; `FDWave` is that state as an object and keeps the reference's
argument meaning (extended-grid sizes, nz-before-nx order of the raw arrays, sx/sz/gz on the
extended grid).  All arrays are numpy float32 [nxe][nze] (x slow, z contiguous, fd-code.cu:58).
"""
import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import Params, Slab, Snaps, check, lib


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


# ---- host formulas (functions.c restated in csrc/fdw_host.c) --------------------------------------
def calc_coefs(order, cxx=False):
    """calc_coefs (functions.c:113-158); cxx=True = the stencil program's float-overload variant."""
    c = np.zeros(order + 1, np.float32)
    check(lib().fdw_calc_coefs(order, int(cxx), c))
    return c


def ricker_wavelet(nt, dt, fpeak):
    """ricker_wavelet (functions.c:328-334)."""
    s = np.zeros(nt, np.float32)
    lib().fdw_ricker_wavelet(nt, dt, fpeak, s)
    return s


def taper_tables(nxb, nzb, fac):
    """taper_x / taper_z of fd_init_cuda (fd-code.cu:159-166)."""
    tx = np.zeros(max(nxb, 1), np.float32)
    tz = np.zeros(max(nzb, 1), np.float32)
    lib().fdw_taper_tables(nxb, nzb, fac, tx.ctypes.data, tz.ctypes.data)
    return tx[:nxb], tz[:nzb]


def srand(seed):
    """Reseed the private restatement of glibc rand() behind extendvel_linear (fresh process == srand(1))."""
    lib().fdw_srand(seed)


def extendvel_linear(vpe, nx, nz, nxb, nzb):
    """extendvel_linear (functions.c:336-394), in place; draws glibc's rand() stream (private generator)."""
    if vpe.shape != (nx + 2 * nxb, nz + 2 * nzb) or vpe.dtype != np.float32 or not vpe.flags.c_contiguous:
        raise ValueError("vpe must be C-contiguous float32 [nx+2nxb][nz+2nzb]")
    lib().fdw_extendvel_linear(nx, nz, nxb, nzb, vpe)
    return vpe


def mod_extendvel(vel, nx, nz, nxb, nzb):
    """taper.c:7-23 of the CPU-serial sibling: replicate the edge values outwards, in place on [nxe][nze]."""
    vel = _f32(vel, (nx + 2 * nxb, nz + 2 * nzb))
    lib().fdw_mod_extendvel(nx, nz, nxb, nzb, vel)
    return vel


def mod_ricker_wavelet(nt, dt, fpeak):
    s = np.zeros(nt, np.float32)
    lib().fdw_mod_ricker_wavelet(nt, dt, fpeak, s)
    return s


def mod_taper_tables(nxb, nzb, fac):
    tx, tz = np.ones(max(nxb, 1), np.float32), np.ones(max(nzb, 1), np.float32)
    lib().fdw_mod_taper_tables(nxb, nzb, fac, tx, tz)
    return tx[:nxb], tz[:nzb]


def image_laplacian(img, dx, dz, device=0):
    """The reference's offline image filter (models/3lay_mod/laplace.f90:25-29) on img[nx][nz]; runs on the GPU."""
    img = np.ascontiguousarray(img, np.float32)
    out = np.zeros_like(img)
    check(lib().fdw_image_laplacian(device, img, img.shape[0], img.shape[1], dx, dz, out))
    return out


def image_compare(a, b, device=0, want_diff=False, exact_sums=False):
    """The reference's `./psnr file1 file2` (models/marmousi/psnr) on the GPU: dict(mse, rmse, snr, psnr) and, if asked, the difference a - b.
    exact_sums=False: the tool's own (serial fp32) sums, its figures digit for digit; True: a parallel reduction in double."""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    if a.size != b.size:
        raise ValueError("sizes differ")
    st = (C.c_double * 4)()
    diff = np.zeros_like(a) if want_diff else None
    check(lib().fdw_image_compare(device, a, b, a.size, diff.ctypes.data if want_diff else None, st, int(exact_sums)))
    out = dict(mse=st[0], rmse=st[1], snr=st[2], psnr=st[3])
    return (out, diff) if want_diff else out


def image_compensate(img, illum, eps=1e-3):
    """The image divided by the source illumination (fdwave.h, fdw_image_compensate): img / (illum + eps * max illum) in fp32, 0 where the
    denominator is not positive.  Host arithmetic; eps is a parameter of the method (finite, >= 0)."""
    img = np.ascontiguousarray(img, np.float32)
    illum = _f32(illum, img.shape)
    out = np.empty_like(img)
    check(lib().fdw_image_compensate(img.ctypes.data, illum.ctypes.data, img.size, eps, out.ctypes.data))
    return out


def image_excitation(exc, amp, eps=1e-3, img=None):
    """The excitation-amplitude image of one shot added to img (fdwave.h, fdw_image_excitation): img += exc / amp in fp32 where
    |amp| > eps * max |amp|, every other cell left as it is.  img=None starts from zeros; shots stack by passing the same img again.  Host
    arithmetic; eps is a parameter of the method (finite, >= 0).  Returns img (a copy of the one passed in)."""
    exc = np.ascontiguousarray(exc, np.float32)
    amp = _f32(amp, exc.shape)
    img = np.zeros(exc.shape, np.float32) if img is None else np.array(_f32(img, exc.shape), order="C")
    check(lib().fdw_image_excitation(exc.ctypes.data, amp.ctypes.data, exc.size, eps, img.ctypes.data))
    return img


def gather_misfit(resid):
    """0.5 * sum resid^2 of a data residual (fdwave.h, fdw_gather_misfit): each square and the sum carried in double, added one after the
    other in memory order.  Host arithmetic."""
    resid = np.ascontiguousarray(resid, np.float32)
    m = C.c_double()
    check(lib().fdw_gather_misfit(resid.ctypes.data if resid.size else None, resid.size, C.byref(m)))
    return m.value


def gather_scale_v2(v2, nxb, gz, g):
    """fdw_gather_scale_v2: out[ix][it] = g[ix][it] * v2[nxb+ix][gz], the data-side weight of the exact adjoint of BORN_DTT (fdwave.h, "DTT
    imaging").  One fp32 product per word.  No device."""
    v2, g = np.ascontiguousarray(v2, np.float32), np.ascontiguousarray(g, np.float32)
    out = np.empty_like(g)
    check(lib().fdw_gather_scale_v2(v2, v2.shape[0], v2.shape[1], int(nxb), int(gz), g.shape[0], g.shape[1], g, out))
    return out


def image_unscale_v2(v2, nxb, nzb, img):
    """fdw_image_unscale_v2: out = img / v2 on the interior, the model-side weight of the exact adjoint of BORN_DTT.  No device."""
    v2, img = np.ascontiguousarray(v2, np.float32), np.ascontiguousarray(img, np.float32)
    out = np.empty_like(img)
    check(lib().fdw_image_unscale_v2(v2, v2.shape[0], v2.shape[1], int(nxb), int(nzb), img.shape[0], img.shape[1], img, out))
    return out


def snap_dims(nx, nz, nt, every, dec=1):
    """fdw_snap_dims: (nframes, nxs, nzs) = (nt // every, ceil(nx / dec), ceil(nz / dec)); every < 1 or dec < 1 is refused.  No device."""
    a, b, c = C.c_int(), C.c_int(), C.c_int()
    check(lib().fdw_snap_dims(nx, nz, nt, int(every), int(dec), C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def plan_pass_bands(nxl, upd_x1, xchunk, bands, depth, npasses):
    """fdw_plan_pass_bands (fdwave.h): (bands, depth, units) of the schedule dev_steps2 follows; units[i] = dict(pass_, band, r0, r1, stream,
    wait).  A request the planner finds unsafe comes back as one band of depth 1.  No device."""
    g, d = C.c_int(), C.c_int()
    n = lib().fdw_plan_pass_bands(nxl, upd_x1, xchunk, bands, depth, npasses, C.byref(g), C.byref(d), None, 0)
    check(min(n, 0))
    units = (_lib.BandUnit * n)()
    check(min(lib().fdw_plan_pass_bands(nxl, upd_x1, xchunk, bands, depth, npasses, C.byref(g), C.byref(d), units, n), 0))
    return g.value, d.value, [dict(pass_=u.pass_, band=u.band, r0=u.r0, r1=u.r1, stream=u.stream, wait=[u.wait[k] for k in range(u.nwait)])
                              for u in units]


def plan_pass_cut(nxl, upd_x1, xchunk, cut_lo, cut_hi, npasses):
    """fdw_plan_pass_cut (fdwave.h): (lo, hi, units) of the two-band schedule whose cut moves between chunk rows cut_lo and cut_hi; units as
    plan_pass_bands gives them (band 0: lower, 1: upper).  A thin request comes back as one unit per pass with lo = hi = 0.  No device."""
    lo, hi = C.c_int(), C.c_int()
    n = lib().fdw_plan_pass_cut(nxl, upd_x1, xchunk, cut_lo, cut_hi, npasses, C.byref(lo), C.byref(hi), None, 0)
    check(min(n, 0))
    units = (_lib.BandUnit * n)()
    check(min(lib().fdw_plan_pass_cut(nxl, upd_x1, xchunk, cut_lo, cut_hi, npasses, C.byref(lo), C.byref(hi), units, n), 0))
    return lo.value, hi.value, [dict(pass_=u.pass_, band=u.band, r0=u.r0, r1=u.r1, stream=u.stream, wait=[u.wait[k] for k in range(u.nwait)])
                                for u in units]


def plan_ext_image(x0, x1, nz, H, xchunk=0):
    """fdw_plan_ext_image (fdwave.h): (xchunk used, chunks) of one extended-image term on rows [x0, x1) of nz columns; chunks[i] =
    dict(c0, c1, rd0, rd1, writes) with writes[j] = (w0, w1), the rows of plane j = h + H that chunk writes (w0 == w1: none).  No device."""
    used = C.c_int()
    n = lib().fdw_plan_ext_image(x0, x1, nz, H, xchunk, C.byref(used), None, 0)
    check(min(n, 0))
    chunks = (_lib.ExtChunk * max(n, 1))()
    check(min(lib().fdw_plan_ext_image(x0, x1, nz, H, xchunk, C.byref(used), chunks, n), 0))
    return used.value, [dict(c0=k.c0, c1=k.c1, rd0=k.rd0, rd1=k.rd1, writes=[(k.w0[j], k.w1[j]) for j in range(2 * H + 1)]) for k in chunks[:n]]


def planewave_lags(src_ix, dx, dt, p):
    """fdw_planewave_lags (fdwave.h): lag[s] = lround(p (src_ix[s] - src_ix[0]) dx / dt) - the smallest of them, in double; p in s/m."""
    src_ix = _i32(src_ix)
    lag = np.zeros(src_ix.size, np.int32)
    check(lib().fdw_planewave_lags(src_ix.size, src_ix.ctypes.data, dx, dt, float(p), lag.ctypes.data))
    return lag


def encode_line_source(src_ix, lag, weight, srce, nx):
    """fdw_encode_line_source (fdwave.h): wav[nx][nt], wav[src_ix[s]][it] += weight[s] * srce[it - lag[s]] for s ascending.  Host arithmetic."""
    src_ix, lag, weight, srce = _i32(src_ix), _i32(lag), _f32(weight).reshape(-1), _f32(srce).reshape(-1)
    if not (src_ix.size == lag.size == weight.size):
        raise ValueError("src_ix, lag and weight must have one entry per shot")
    wav = np.zeros((nx, srce.size), np.float32)
    check(lib().fdw_encode_line_source(src_ix.size, src_ix.ctypes.data, lag.ctypes.data, weight.ctypes.data, srce.ctypes.data, srce.size, nx,
                                       wav.ctypes.data))
    return wav


def encode_gathers(lag, weight, d_obs_all, device=0):
    """fdw_encode_gathers (fdwave.h): out[ix][it] = sum over s ascending, 0 <= it - lag[s] < nt, of weight[s] * d_obs_all[s][ix][it - lag[s]],
    every element folded in shot order on the GPU."""
    lag, weight = _i32(lag), _f32(weight).reshape(-1)
    d_obs_all = np.ascontiguousarray(d_obs_all, np.float32)
    if d_obs_all.ndim != 3 or not (d_obs_all.shape[0] == lag.size == weight.size):
        raise ValueError("d_obs_all must be [nshots][nx][nt] with one lag and one weight per shot")
    _, nx, nt = d_obs_all.shape
    out = np.zeros((nx, nt), np.float32)
    check(lib().fdw_encode_gathers(device, lag.size, lag.ctypes.data, weight.ctypes.data, d_obs_all.ctypes.data, nx, nt, out.ctypes.data))
    return out


def encode_gathers_multi(lag, weight, d_obs_all, device=0):
    """fdw_encode_gathers_multi (fdwave.h): encode_gathers for `nplanes` encodings of one data set in one upload and one launch.
    lag, weight [nplanes][nshots]; returns out[nplanes][nx][nt], plane j equal to encode_gathers(lag[j], weight[j], d_obs_all) bit for bit."""
    lag, weight = np.ascontiguousarray(lag, np.int32), _f32(weight)
    d_obs_all = np.ascontiguousarray(d_obs_all, np.float32)
    if d_obs_all.ndim != 3 or lag.ndim != 2 or lag.shape != weight.shape or lag.shape[1] != d_obs_all.shape[0]:
        raise ValueError("d_obs_all must be [nshots][nx][nt], lag and weight [nplanes][nshots]")
    _, nx, nt = d_obs_all.shape
    out = np.zeros((lag.shape[0], nx, nt), np.float32)
    check(lib().fdw_encode_gathers_multi(device, lag.shape[1], lag.shape[0], lag.ctypes.data, weight.ctypes.data, d_obs_all.ctypes.data, nx, nt,
                                         out.ctypes.data))
    return out


class FDWave:
    """One fd_init (fd-code.cu:200-224 / fd-source-code.cu:241-262) worth of state on one MI355X."""

    def __init__(self, order, nxe, nze, nxb=0, nzb=0, nt=0, fac=1.0, dx=1.0, dz=1.0, dt=0.0, *, compat=True,
                 coef_cxx=False, device=0, slab=None, dialect=0, numerics=0):
        """dialect 0: the CUDA programs (stencil_code / rtm_code); 1: the forward-modelling producer of the CPU-serial sibling
        (mod_main: model_shot only); 2: its stored-wavefield RTM (rtm_main: rtm_stored_shot only).
        numerics 0: the reference's arithmetic operation for operation (bit-exact); 1: FAST -- symmetric taps summed first + fused
        multiply-adds in the Laplacian (fdwave.h), within 1e-5 of the former, RTM dialect only."""
        self.params = Params(order, nxe, nze, nxb, nzb, nt, dx, dz, dt, fac, int(compat), int(coef_cxx), int(dialect), int(numerics))
        self._h = C.c_void_p()
        if slab is None:
            check(lib().fdw_create(C.byref(self.params), device, C.byref(self._h)))
            self.x_off, self.nxl = 0, nxe
        else:
            self.x_off, self.nxl = slab
            s = Slab(self.x_off, self.nxl)
            check(lib().fdw_create_slab(C.byref(self.params), C.byref(s), device, C.byref(self._h)))
        self.order, self.nxe, self.nze, self.nxb, self.nzb, self.nt = order, nxe, nze, nxb, nzb, nt
        self.nx, self.nz = nxe - 2 * nxb, nze - 2 * nzb
        self.device = device
        self.pitch = lib().fdw_pitch(self._h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().fdw_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        if sys.is_finalizing():      # interpreter shutdown: the HIP runtime may already be gone, and the process frees everything anyway
            return
        try:
            self.close()
        except Exception:
            pass

    # ---- introspection --------------------------------------------------------------------------
    def tables(self):
        cx = np.zeros(self.order + 1, np.float32)
        cz = np.zeros(self.order + 1, np.float32)
        tx = np.zeros(max(self.nxb, 1), np.float32)
        tz = np.zeros(max(self.nzb, 1), np.float32)
        check(lib().fdw_get_tables(self._h, cx.ctypes.data, cz.ctypes.data, tx.ctypes.data, tz.ctypes.data))
        return cx, cz, tx[:self.nxb], tz[:self.nzb]

    def extents(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        check(lib().fdw_get_extents(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_tuning(self, xchunk=0, wz=0, use_generic=False, prefetch=0, two_step=0, force_edge=False):
        """two_step: 0 auto, 1 two steps per pass, 4 the four-wave pipeline, -1 never (temporal blocking in forward loops).  force_edge is obsolete and ignored."""
        check(lib().fdw_set_tuning(self._h, xchunk, wz, int(use_generic), prefetch, int(two_step)))

    def two_step_active(self):
        return bool(lib().fdw_two_step_active(self._h))

    def steps_per_pass(self):
        """Time steps one launch of the forward loops advances on this grid: 4 (wave pipeline), 2 (two-step kernel) or 1."""
        return int(lib().fdw_steps_per_pass(self._h))

    def set_pass_bands(self, bands=0, depth=0):
        """How dev_steps2 issues the passes of the four-step kernel (fdwave.h): `bands` row bands per pass, units `depth` deep on the caller's
        stream and depth - 1 side streams.  0, 0: automatic; depth 1: the bands one after the other on the caller's stream.  Results never
        depend on it."""
        check(lib().fdw_set_pass_bands(self._h, int(bands), int(depth)))

    def pass_bands(self):
        """(bands, depth) the last dev_steps2 call used; (1, 1) is the plain loop."""
        a, b = C.c_int(), C.c_int()
        check(lib().fdw_pass_bands(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_pass_cut(self, lo=0, hi=0):
        """dev_steps2's passes as two row bands whose cut moves between chunk rows lo and hi (fdwave.h: fdw_set_pass_cut).  0, 0: automatic;
        -1, -1: off.  An explicit set_pass_bands takes precedence.  Results never depend on it."""
        check(lib().fdw_set_pass_cut(self._h, int(lo), int(hi)))

    def pass_cut(self):
        """(lo, hi, turns) of the moving cut in the last dev_steps2 call; (-1, -1, 0) when it did not run."""
        a, b, t = C.c_int(), C.c_int(), C.c_int()
        check(lib().fdw_pass_cut(self._h, C.byref(a), C.byref(b), C.byref(t)))
        return a.value, b.value, t.value

    def selftest(self):
        check(lib().fdw_selftest(self._h))

    # ---- host-array API (the reference's L2 seam) -----------------------------------------------
    def laplacian(self, p):
        """stencil_code's single kernel_lap launch (fd-source-code.cu:320-333)."""
        p = _f32(p, (self.nxe, self.nze))
        out = np.empty_like(p)
        check(lib().fdw_laplacian(self._h, p, out))
        return out

    def forward(self, v2, sx, sz, srce, p=None, pp=None, nsteps=None):
        """fd_forward (fd-code.cu:247-288): returns (P, PP) = (d_p, d_pp) after the loop."""
        shape = (self.nxe, self.nze)
        p = np.zeros(shape, np.float32) if p is None else np.array(p, np.float32, order="C")
        pp = np.zeros(shape, np.float32) if pp is None else np.array(pp, np.float32, order="C")
        srce = _f32(srce)
        nsteps = len(srce) if nsteps is None else nsteps
        if nsteps > len(srce):
            raise ValueError("srce shorter than nsteps")
        check(lib().fdw_forward(self._h, p, pp, _f32(v2, shape), sx, sz, srce, nsteps))
        return p, pp

    def back(self, v2, snap0, snap1, d_obs, gz, imloc=None, nsteps=None):
        """fd_back (fd-code.cu:290-341): d_obs [nx][nt]; returns imloc [nx][nz]."""
        shape = (self.nxe, self.nze)
        imloc = np.zeros((self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")
        nsteps = self.nt if nsteps is None else nsteps
        check(lib().fdw_back(self._h, _f32(v2, shape), _f32(snap0, shape), _f32(snap1, shape),
                             _f32(d_obs, (self.nx, self.nt)), gz, imloc, nsteps))
        return imloc

    def shot(self, v2, sx, sz, gz, srce, d_obs, imloc=None, want_fields=False, want_illum=False, illum=None):
        """One shot of rtm_code's loop (fd-code.cu:496-518), device resident.  want_illum: the forward loop also accumulates the source
        illumination illum[nx][nz] (from zero, or into `illum`; fdwave.h), appended to what is returned."""
        shape = (self.nxe, self.nze)
        imloc = np.zeros((self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")
        P = np.zeros(shape, np.float32) if want_fields else None
        PP = np.zeros(shape, np.float32) if want_fields else None
        fields = (P.ctypes.data if want_fields else None, PP.ctypes.data if want_fields else None)
        if want_illum:
            illum = np.zeros((self.nx, self.nz), np.float32) if illum is None else np.array(_f32(illum, (self.nx, self.nz)), order="C")
            check(lib().fdw_shot_illum(self._h, _f32(v2, shape), sx, sz, gz, _f32(srce, (self.nt,)), _f32(d_obs, (self.nx, self.nt)), imloc, illum,
                                       *fields))
            return (imloc, P, PP, illum) if want_fields else (imloc, illum)
        check(lib().fdw_shot(self._h, _f32(v2, shape), sx, sz, gz, _f32(srce, (self.nt,)),
                             _f32(d_obs, (self.nx, self.nt)), imloc, *fields))
        return (imloc, P, PP) if want_fields else imloc

    # ---- wavefield snapshots (fdwave.h: dir.snaps, dir.snaps_rec, dir.snapr) ----
    def snap_dims(self, every, dec=1):
        """(nframes, nxs, nzs) of this geometry's snapshots every `every` time levels, decimated by `dec`: frames at levels every, 2 every, ...
        <= nt of ceil(nx / dec) x ceil(nz / dec) interior cells.  Needs no device."""
        return snap_dims(self.nx, self.nz, self.nt, every, dec)

    def dev_snapshot(self, d_field, dec, d_frame, stream=None):
        """One frame of the device field d_field [nxl][pitch] into the device array d_frame [nxs][nzs]: a bit-exact crop-and-decimate copy.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_snapshot(self._h, d_field, int(dec), d_frame, stream))

    def shot_snaps(self, v2, sx, sz, gz, srce, d_obs, every, dec=1, sets=("snaps", "snaps_rec", "snapr"), imloc=None, want_fields=False,
                   want_illum=False, illum=None):
        """shot() (v2=None: shot_resident()) that also takes wavefield frames at the levels every, 2 every, ... (fdwave.h): `snaps` the forward
        field u^L, `snaps_rec` the source field the backward loop images at that level, `snapr` the receiver field it is multiplied with.
        Returns a dict: image, the requested sets as [nframes][nxs][nzs], and P, PP / illum if asked."""
        nframes, nxs, nzs = self.snap_dims(every, dec)
        unknown = set(sets) - {"snaps", "snaps_rec", "snapr"}
        if unknown:
            raise ValueError(f"unknown frame sets {sorted(unknown)}")
        shape = (self.nxe, self.nze)
        out = {name: np.zeros((nframes, nxs, nzs), np.float32) for name in sets}
        out["image"] = np.zeros((self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")
        if want_fields:
            out["P"], out["PP"] = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        if want_illum:
            out["illum"] = np.zeros((self.nx, self.nz), np.float32) if illum is None else np.array(_f32(illum, (self.nx, self.nz)), order="C")

        def ptr(name):
            return out[name].ctypes.data if name in out else None

        sn = Snaps(int(every), int(dec), ptr("snaps"), ptr("snaps_rec"), ptr("snapr"))
        check(lib().fdw_shot_snaps(self._h, None if v2 is None else _f32(v2, shape).ctypes.data, sx, sz, gz, _f32(srce, (self.nt,)),
                                   _f32(d_obs, (self.nx, self.nt)), out["image"], ptr("illum"), ptr("P"), ptr("PP"), C.byref(sn)))
        return out

    # ---- random-border model generated on the device ----
    def border_draws(self):
        """rand() calls one extendvel_linear (functions.c:336-394) consumes on this geometry."""
        return int(lib().fdw_border_draws(self.nx, self.nz, self.nxb, self.nzb))

    def model_resident(self, vp):
        """Upload the interior velocity model vp[nx][nz] (not squared) once; the per-shot borders are then drawn on the device."""
        check(lib().fdw_model_resident(self._h, _f32(vp, (self.nx, self.nz))))

    def dev_extendvel_linear(self, draw_offset, want_vel=False):
        """extendvel_linear + vel2 = vpe * vpe (fd-code.cu:486-494) in HBM, from draws [draw_offset, draw_offset + border_draws()) of the
        unseeded glibc rand() stream.  want_vel: also return the extended model [nxe][nze]."""
        vel = np.zeros((self.nxe, self.nze), np.float32) if want_vel else None
        check(lib().fdw_dev_extendvel_linear(self._h, int(draw_offset), vel.ctypes.data if want_vel else None))
        return vel

    def shot_resident(self, sx, sz, gz, srce, d_obs, imloc=None, want_fields=False, want_illum=False, illum=None):
        """shot() on the squared model dev_extendvel_linear left in HBM."""
        shape = (self.nxe, self.nze)
        imloc = np.zeros((self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")
        P = np.zeros(shape, np.float32) if want_fields else None
        PP = np.zeros(shape, np.float32) if want_fields else None
        if want_illum:
            illum = np.zeros((self.nx, self.nz), np.float32) if illum is None else np.array(_f32(illum, (self.nx, self.nz)), order="C")
            check(lib().fdw_shot_resident_illum(self._h, sx, sz, gz, _f32(srce, (self.nt,)), _f32(d_obs, (self.nx, self.nt)), imloc, illum,
                                                P.ctypes.data if want_fields else None, PP.ctypes.data if want_fields else None))
            return (imloc, P, PP, illum) if want_fields else (imloc, illum)
        check(lib().fdw_shot_resident(self._h, sx, sz, gz, _f32(srce, (self.nt,)), _f32(d_obs, (self.nx, self.nt)), imloc,
                                      P.ctypes.data if want_fields else None, PP.ctypes.data if want_fields else None))
        return (imloc, P, PP) if want_fields else imloc

    def shot_batch(self, nshots, sx0, dsx, sz, gz, srce, d_obs, v2_all=None, draw_offset=0, imloc=None, want_illum=False, illum=None):
        """`nshots` consecutive shots of rtm_code's loop (fd-code.cu:480-520) through one launch per time step.  d_obs[nshots][nx][nt];
        v2_all[nshots][nxe][nze], or None = border models drawn on the device from the resident interior model at draws
        draw_offset + b * border_draws().  Returns imloc[nshots][nx][nz].  want_illum: the forward loop also accumulates every shot's
        source illumination illum[nshots][nx][nz] (from zero, or into `illum`); returns (imloc, illum)."""
        imloc = np.zeros((nshots, self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")
        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        if want_illum:
            shape = (nshots, self.nx, self.nz)
            illum = np.zeros(shape, np.float32) if illum is None else np.array(_f32(illum, shape), order="C")
            check(lib().fdw_shot_batch_illum(self._h, nshots, v2p, int(draw_offset), sx0, dsx, sz, gz, _f32(srce, (self.nt,)),
                                             _f32(d_obs, (nshots, self.nx, self.nt)), imloc, illum))
            return imloc, illum
        check(lib().fdw_shot_batch(self._h, nshots, v2p, int(draw_offset), sx0, dsx, sz, gz, _f32(srce, (self.nt,)),
                                   _f32(d_obs, (nshots, self.nx, self.nt)), imloc))
        return imloc

    def shot_residual(self, v2, sx, sz, gz, srce, d_obs, imloc=None, want_resid=True, want_fields=False, want_illum=False, illum=None):
        """Residual migration of one shot (fdwave.h, fdw_shot_residual): shot() (v2=None: shot_resident()) whose forward loop also models the
        gather d_mod of the migration model at gz, and whose backward loop migrates d_obs - d_mod instead of d_obs.  Returns a dict: image,
        and resid [nx][nt] / illum / P, PP as asked."""
        shape = (self.nxe, self.nze)
        out = {"image": np.zeros((self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")}
        if want_resid:
            out["resid"] = np.zeros((self.nx, self.nt), np.float32)
        if want_fields:
            out["P"], out["PP"] = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        if want_illum:
            out["illum"] = np.zeros((self.nx, self.nz), np.float32) if illum is None else np.array(_f32(illum, (self.nx, self.nz)), order="C")

        def ptr(name):
            return out[name].ctypes.data if name in out else None

        check(lib().fdw_shot_residual(self._h, None if v2 is None else _f32(v2, shape).ctypes.data, sx, sz, gz, _f32(srce, (self.nt,)),
                                      _f32(d_obs, (self.nx, self.nt)), out["image"], ptr("illum"), ptr("resid"), ptr("P"), ptr("PP")))
        return out

    def shot_batch_residual(self, nshots, sx0, dsx, sz, gz, srce, d_obs, v2_all=None, draw_offset=0, imloc=None, want_resid=True,
                            want_illum=False, illum=None):
        """`nshots` residual migrations, shots and models as shot_batch takes them (one launch per time step where shot_batch batches).
        Returns a dict: image [nshots][nx][nz], and resid [nshots][nx][nt] / illum [nshots][nx][nz] as asked."""
        out = {"image": np.zeros((nshots, self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")}
        if want_resid:
            out["resid"] = np.zeros((nshots, self.nx, self.nt), np.float32)
        if want_illum:
            shape = (nshots, self.nx, self.nz)
            out["illum"] = np.zeros(shape, np.float32) if illum is None else np.array(_f32(illum, shape), order="C")
        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        check(lib().fdw_shot_batch_residual(self._h, nshots, v2p, int(draw_offset), sx0, dsx, sz, gz, _f32(srce, (self.nt,)),
                                            _f32(d_obs, (nshots, self.nx, self.nt)), out["image"],
                                            out["illum"].ctypes.data if want_illum else None, out["resid"].ctypes.data if want_resid else None))
        return out

    def record_shot(self, v2, sx, sz, gz, srce, want_fields=False):
        """fd_forward from rest (fd-code.cu:496-497, 259-267) recording the gather data[nx][nt]: data[ix][it] = d_pp(nxb + ix, gz) at the end
        of iteration it (fdwave.h, fdw_record_shot), the layout rtm_code's datfile holds per shot.  want_fields: also (P, PP) as forward()."""
        shape = (self.nxe, self.nze)
        data = np.zeros((self.nx, self.nt), np.float32)
        P = np.zeros(shape, np.float32) if want_fields else None
        PP = np.zeros(shape, np.float32) if want_fields else None
        check(lib().fdw_record_shot(self._h, _f32(v2, shape), sx, sz, gz, _f32(srce, (self.nt,)), data,
                                    P.ctypes.data if want_fields else None, PP.ctypes.data if want_fields else None))
        return (data, P, PP) if want_fields else data

    # ---- Born modelling (fdwave.h: scattered-field gathers from a reflectivity model) ----
    def born_shot(self, v2, m, sx, sz, gz, srce, kind=_lib.BORN_DTT, want_background=False):
        """One Born shot from rest (fdwave.h, fdw_born_shot): the scattered gather data[nx][nt] of the reflectivity m[nx][nz] in the background
        v2 (None: the resident model); kind: BORN_FIELD or BORN_DTT.  want_background: also the background gather, which is record_shot()'s."""
        data = np.zeros((self.nx, self.nt), np.float32)
        data0 = np.zeros((self.nx, self.nt), np.float32) if want_background else None
        check(lib().fdw_born_shot(self._h, None if v2 is None else _f32(v2, (self.nxe, self.nze)).ctypes.data, _f32(m, (self.nx, self.nz)), int(kind),
                                  sx, sz, gz, _f32(srce, (self.nt,)), data, data0.ctypes.data if want_background else None))
        return (data, data0) if want_background else data

    def dev_born_steps(self, d_u_p, d_u_pp, d_du_p, d_du_pp, d_v2, d_m, kind, d_srce, sx, sz, gz, d_rec, d_rec0, it0, nsteps, first_pp_twice=False,
                       stream=None):
        """nsteps Born iterations on the background pair (d_u_p, d_u_pp) and the scattered pair (d_du_p, d_du_pp), each rotated as dev_steps rotates
        its two buffers; d_m: the reflectivity, field-shaped; d_rec / d_rec0 (device [it][nx], either may be None): the scattered and the
        background gather (fdwave.h, fdw_dev_born_steps).  stream=None: the context's own non-blocking stream, unordered against the caller's
        streams (the legacy default stream included); a caller's stream: every launch of the call is issued on it and the call does not
        synchronise (fdwave.h)."""
        check(lib().fdw_dev_born_steps(self._h, d_u_p, d_u_pp, d_du_p, d_du_pp, d_v2, d_m, int(kind), d_srce, sx, sz, gz, d_rec, d_rec0, it0, nsteps,
                                       int(first_pp_twice), stream))

    def dev_born_line_steps(self, d_u_p, d_u_pp, d_du_p, d_du_pp, d_v2, d_m, kind, d_wav, sz, gz, d_rec, d_rec0, it0, nsteps, first_pp_twice=False,
                            stream=None):
        """dev_born_steps whose background pair is driven by the line source d_wav (device [>= it0+nsteps][nx]) on column sz instead of a point
        source (fdwave.h, fdw_dev_born_line_steps).  stream as dev_born_steps takes it."""
        check(lib().fdw_dev_born_line_steps(self._h, d_u_p, d_u_pp, d_du_p, d_du_pp, d_v2, d_m, int(kind), d_wav, sz, gz, d_rec, d_rec0, it0, nsteps,
                                            int(first_pp_twice), stream))

    def born_shot_line(self, v2, m, sz, gz, wav, kind=_lib.BORN_DTT, want_background=False):
        """born_shot() driven by the line source wav[nx][nt] at depth sz (fdwave.h, fdw_born_shot_line); the background gather is
        record_shot_line()'s."""
        data = np.zeros((self.nx, self.nt), np.float32)
        data0 = np.zeros((self.nx, self.nt), np.float32) if want_background else None
        v2, m, wav = None if v2 is None else _f32(v2, (self.nxe, self.nze)), _f32(m, (self.nx, self.nz)), _f32(wav, (self.nx, self.nt))
        check(lib().fdw_born_shot_line(self._h, None if v2 is None else v2.ctypes.data, m.ctypes.data, int(kind), sz, gz, wav.ctypes.data, data.ctypes.data,
                                       data0.ctypes.data if want_background else None))
        return (data, data0) if want_background else data

    def born_shot_batch(self, nshots, m, sx0, dsx, sz, gz, srce, kind=_lib.BORN_DTT, v2_all=None, draw_offset=0, want_background=False):
        """`nshots` Born shots of ONE reflectivity m[nx][nz], source rows sx0 + b dsx, models as shot_batch takes them (fdwave.h,
        fdw_born_shot_batch): data[nshots][nx][nt], with want_background (data, data0).  One launch per time step where record_shot_batch
        batches and the fused Born kernel runs; batch_parts() says how the call went."""
        data = np.zeros((nshots, self.nx, self.nt), np.float32)
        data0 = np.zeros((nshots, self.nx, self.nt), np.float32) if want_background else None
        v2_all, m, srce = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)), _f32(m, (self.nx, self.nz)), _f32(srce, (self.nt,))
        check(lib().fdw_born_shot_batch(self._h, nshots, None if v2_all is None else v2_all.ctypes.data, int(draw_offset), m.ctypes.data, int(kind), sx0, dsx,
                                        sz, gz, srce.ctypes.data, data.ctypes.data, data0.ctypes.data if want_background else None))
        return (data, data0) if want_background else data

    def born_shot_line_batch(self, nshots, m, sz, gz, wav_all, kind=_lib.BORN_DTT, v2_all=None, draw_offset=0, want_background=False):
        """born_shot_batch() with the shots' line sources wav_all[nshots][nx][nt] at depth sz (fdwave.h, fdw_born_shot_line_batch)."""
        data = np.zeros((nshots, self.nx, self.nt), np.float32)
        data0 = np.zeros((nshots, self.nx, self.nt), np.float32) if want_background else None
        v2_all, m = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)), _f32(m, (self.nx, self.nz))
        wav_all = _f32(wav_all, (nshots, self.nx, self.nt))
        check(lib().fdw_born_shot_line_batch(self._h, nshots, None if v2_all is None else v2_all.ctypes.data, int(draw_offset), m.ctypes.data, int(kind), sz, gz,
                                             wav_all.ctypes.data, data.ctypes.data, data0.ctypes.data if want_background else None))
        return (data, data0) if want_background else data

    # ---- DTT imaging (fdwave.h: the second-time-difference imaging condition, the adjoint of BORN_DTT) ----
    def _dtt_out(self, lead, imloc, residual, want_resid, want_fields, want_illum, illum):
        out = {"image": np.zeros(lead + (self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")}
        if residual and want_resid:
            out["resid"] = np.zeros(lead + (self.nx, self.nt), np.float32)
        if want_fields:
            out["P"], out["PP"] = np.zeros((self.nxe, self.nze), np.float32), np.zeros((self.nxe, self.nze), np.float32)
        if want_illum:
            shape = lead + (self.nx, self.nz)
            out["illum"] = np.zeros(shape, np.float32) if illum is None else np.array(_f32(illum, shape), order="C")
        return out, (lambda name: out[name].ctypes.data if name in out else None)

    def shot_dtt(self, v2, sx, sz, gz, srce, d_obs, imloc=None, residual=False, want_resid=True, want_fields=False, want_illum=False, illum=None):
        """shot() (v2=None: the resident model) whose backward loop images with the second time difference of the source field (fdwave.h,
        fdw_shot_dtt); residual: migrate d_obs - d_mod as shot_residual() does -- the image is then the gradient of the BORN_DTT misfit.
        Returns a dict: image, and resid / illum / P, PP as asked; all but the image equal the cross-correlation calls' bit for bit."""
        out, ptr = self._dtt_out((), imloc, residual, want_resid, want_fields, want_illum, illum)
        check(lib().fdw_shot_dtt(self._h, None if v2 is None else _f32(v2, (self.nxe, self.nze)).ctypes.data, sx, sz, gz, _f32(srce, (self.nt,)),
                                 _f32(d_obs, (self.nx, self.nt)), out["image"], ptr("illum"), int(bool(residual)), ptr("resid"), ptr("P"), ptr("PP")))
        return out

    def shot_line_dtt(self, v2, sz, gz, wav, d_obs, imloc=None, residual=False, want_resid=True, want_fields=False, want_illum=False, illum=None):
        """shot_dtt() driven by the line source wav[nx][nt] at depth sz (fdwave.h, fdw_shot_line_dtt)."""
        out, ptr = self._dtt_out((), imloc, residual, want_resid, want_fields, want_illum, illum)
        check(lib().fdw_shot_line_dtt(self._h, None if v2 is None else _f32(v2, (self.nxe, self.nze)).ctypes.data, sz, gz, _f32(wav, (self.nx, self.nt)),
                                      _f32(d_obs, (self.nx, self.nt)), out["image"], ptr("illum"), int(bool(residual)), ptr("resid"), ptr("P"), ptr("PP")))
        return out

    def shot_batch_dtt(self, nshots, sx0, dsx, sz, gz, srce, d_obs, v2_all=None, draw_offset=0, imloc=None, residual=False, want_resid=True,
                       want_illum=False, illum=None):
        """`nshots` shot_dtt() shots, shots and models as shot_batch takes them (fdwave.h, fdw_shot_batch_dtt); batch_parts() says how the call
        went.  Returns a dict: image [nshots][nx][nz], and resid / illum as asked."""
        out, ptr = self._dtt_out((nshots,), imloc, residual, want_resid, False, want_illum, illum)
        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        check(lib().fdw_shot_batch_dtt(self._h, nshots, v2p, int(draw_offset), sx0, dsx, sz, gz, _f32(srce, (self.nt,)),
                                       _f32(d_obs, (nshots, self.nx, self.nt)), out["image"], ptr("illum"), int(bool(residual)), ptr("resid")))
        return out

    def shot_line_batch_dtt(self, nshots, sz, gz, wav_all, d_obs, v2_all=None, draw_offset=0, imloc=None, residual=False, want_resid=True,
                            want_illum=False, illum=None):
        """shot_batch_dtt() with the shots' line sources wav_all[nshots][nx][nt] at depth sz (fdwave.h, fdw_shot_line_batch_dtt)."""
        out, ptr = self._dtt_out((nshots,), imloc, residual, want_resid, False, want_illum, illum)
        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        check(lib().fdw_shot_line_batch_dtt(self._h, nshots, v2p, int(draw_offset), sz, gz, _f32(wav_all, (nshots, self.nx, self.nt)),
                                            _f32(d_obs, (nshots, self.nx, self.nt)), out["image"], ptr("illum"), int(bool(residual)), ptr("resid")))
        return out

    def dev_back_iter_dtt(self, step_source, d_f1, d_f0, d_pr, d_ppr, d_v2, r0, r1, pp_twice, d_samples, gz, d_img, stream=None):
        """dev_back_iter() with the DTT image term in place of the cross-correlation; step_source=0 (iterations 0 and 1) leaves d_img alone
        (fdwave.h, fdw_dev_back_iter_dtt).  stream as dev_back_iter takes it."""
        check(lib().fdw_dev_back_iter_dtt(self._h, int(step_source), d_f1, d_f0, d_pr, d_ppr, d_v2, r0, r1, int(pp_twice), d_samples, gz, d_img, stream))

    def dev_dtt_image(self, d_fa, d_fb, d_fc, d_r, d_img, stream=None):
        """One DTT image term on the interior cells: d_img += ((d_fa - d_fb) - (d_fb - d_fc)) * d_r (fdwave.h, fdw_dev_dtt_image): the tail of
        a device caller's loop, behind dev_step(MODE_PLAIN).  stream as dev_back_iter takes it."""
        check(lib().fdw_dev_dtt_image(self._h, d_fa, d_fb, d_fc, d_r, d_img, stream))

    # ---- subsurface-offset image gathers (fdwave.h: "Extended imaging") ----
    def dev_ext_image(self, d_f, d_r, H, d_eimg, stream=None):
        """One term of the extended image on the Born cell set: plane h + H of d_eimg (2H+1 field-shaped planes, one field apart) +=
        d_f[x-h] * d_r[x+h] wherever both rows lie in the cell set (fdwave.h, fdw_dev_ext_image).  stream as dev_back_iter takes it."""
        check(lib().fdw_dev_ext_image(self._h, d_f, d_r, int(H), d_eimg, stream))

    def shot_ext(self, v2, sx, sz, gz, srce, d_obs, H, eimg=None, imloc=None, want_image=True, want_fields=False):
        """shot() (v2=None: the resident model) whose backward loop also accumulates the subsurface-offset extended image eimg[2H+1][nx][nz]
        (from zero, or into `eimg`; fdwave.h, fdw_shot_ext).  Returns a dict: eimg, image (want_image) and P, PP (want_fields); image, P and PP
        equal shot()'s bit for bit, and plane H of eimg equals the image on the interior cells of the Born cell set."""
        shape = (2 * max(int(H), 0) + 1, self.nx, self.nz)      # (a negative H is the library's to refuse)
        out = dict(eimg=np.zeros(shape, np.float32) if eimg is None else np.array(_f32(eimg, shape), order="C"))
        if want_image:
            out["image"] = np.zeros((self.nx, self.nz), np.float32) if imloc is None else np.array(_f32(imloc, (self.nx, self.nz)), order="C")
        if want_fields:
            out["P"], out["PP"] = np.zeros((self.nxe, self.nze), np.float32), np.zeros((self.nxe, self.nze), np.float32)
        ptr = lambda k: out[k].ctypes.data if k in out else None      # noqa: E731
        check(lib().fdw_shot_ext(self._h, None if v2 is None else _f32(v2, (self.nxe, self.nze)).ctypes.data, sx, sz, gz, _f32(srce, (self.nt,)),
                                 _f32(d_obs, (self.nx, self.nt)), int(H), ptr("image"), ptr("eimg"), ptr("P"), ptr("PP")))
        return out

    # ---- least-squares migration (fdwave.h: conjugate gradients on BORN_DTT modelling and DTT imaging) ----
    def dev_dot_cells(self, d_a, d_b, d_rows, d_sum, stream=None):
        """<a, b> over the Born cell set of two field-shaped device arrays, in the sum order of fdwave.h: d_rows (device doubles, one per
        row of the cell set) the row sums, d_sum (one device double) the total (fdw_dev_dot_cells).  stream as dev_born_steps takes it."""
        check(lib().fdw_dev_dot_cells(self._h, d_a, d_b, d_rows, d_sum, stream))

    def dev_dot_gather(self, d_a, d_b, d_rows, d_sum, stream=None):
        """<a, b> of two device gathers [nt][nx]; d_rows [nt] device doubles, d_sum one (fdw_dev_dot_gather)."""
        check(lib().fdw_dev_dot_gather(self._h, d_a, d_b, d_rows, d_sum, stream))

    def dev_lsm_gather(self, d_q, d_obs, d_v2, gz, d_w, d_ws, d_rows, d_n2, stream=None):
        """One pass over a device gather [nt][nx]: w = d_obs - q (d_obs None: q), d_n2 = <w, w>, d_w (None ok) = w, d_ws = w * v2[nxb+ix][gz]
        (fdw_dev_lsm_gather)."""
        check(lib().fdw_dev_lsm_gather(self._h, d_q, d_obs, d_v2, gz, d_w, d_ws, d_rows, d_n2, stream))

    def dev_lsm_stack(self, d_h, d_img, d_v2, d_mask, stream=None):
        """h = h + mask * (img / v2) on the Born cell set, d_mask None: h = h + img / v2 (fdw_dev_lsm_stack)."""
        check(lib().fdw_dev_lsm_stack(self._h, d_h, d_img, d_v2, d_mask, stream))

    def dev_lsm_update(self, d_m, d_g, d_p, d_h, d_alpha, d_rows, d_gg, stream=None):
        """m = m + af * p, g = g - af * h on the Born cell set with af = float32 of the device double d_alpha; d_gg = <g, g> of the new g
        (fdw_dev_lsm_update)."""
        check(lib().fdw_dev_lsm_update(self._h, d_m, d_g, d_p, d_h, d_alpha, d_rows, d_gg, stream))

    def dev_lsm_direction(self, d_p, d_g, d_beta, stream=None):
        """p = g + float32(beta) * p on the Born cell set, beta a device double (fdw_dev_lsm_direction)."""
        check(lib().fdw_dev_lsm_direction(self._h, d_p, d_g, d_beta, stream))

    def lsm_visit(self, v2, p, sx, sz, gz, srce, d_obs=None, mask=None, h=None, want_data=False):
        """One visit of a least-squares migration (fdwave.h, fdw_lsm_visit): Born modelling of the direction p[nx][nz], the residual d_obs - q
        (d_obs None: q), its weighted DTT image stacked onto h (None: zeros) through the mask (None: none).  v2 None: the resident model.
        Returns a dict: h, n2 = <w, w>, and data = w [nx][nt] with want_data."""
        out = {"h": np.zeros((self.nx, self.nz), np.float32) if h is None else np.array(_f32(h, (self.nx, self.nz)), order="C")}
        if want_data:
            out["data"] = np.zeros((self.nx, self.nt), np.float32)
        n2 = C.c_double(0.0)
        d_obs = None if d_obs is None else _f32(d_obs, (self.nx, self.nt))
        mask = None if mask is None else _f32(mask, (self.nx, self.nz))
        check(lib().fdw_lsm_visit(self._h, None if v2 is None else _f32(v2, (self.nxe, self.nze)).ctypes.data, _f32(p, (self.nx, self.nz)), sx, sz, gz,
                                  _f32(srce, (self.nt,)), None if d_obs is None else d_obs.ctypes.data, None if mask is None else mask.ctypes.data,
                                  out["h"], C.byref(n2), out["data"].ctypes.data if want_data else None))
        out["n2"] = n2.value
        return out

    def lsm_visit_batch(self, nshots, p, sx0, dsx, sz, gz, srce, d_obs=None, mask=None, h=None, v2_all=None, draw_offset=0, want_data=False):
        """The visits of `nshots` shots on ONE direction p, stacked into h in shot order (fdwave.h, fdw_lsm_visit_batch); shots and models as
        born_shot_batch takes them, d_obs[nshots][nx][nt] or None.  One launch per time step in both loops where born_shot_batch and
        shot_batch_dtt batch; batch_parts() says how the call went.  Returns a dict: h, n2[nshots], and data[nshots][nx][nt] with want_data."""
        out = {"h": np.zeros((self.nx, self.nz), np.float32) if h is None else np.array(_f32(h, (self.nx, self.nz)), order="C"),
               "n2": np.zeros(max(nshots, 1), np.float64)}
        if want_data:
            out["data"] = np.zeros((nshots, self.nx, self.nt), np.float32)
        v2_all = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze))
        d_obs = None if d_obs is None else _f32(d_obs, (nshots, self.nx, self.nt))
        mask = None if mask is None else _f32(mask, (self.nx, self.nz))
        check(lib().fdw_lsm_visit_batch(self._h, nshots, None if v2_all is None else v2_all.ctypes.data, int(draw_offset), _f32(p, (self.nx, self.nz)), sx0, dsx,
                                        sz, gz, _f32(srce, (self.nt,)), None if d_obs is None else d_obs.ctypes.data,
                                        None if mask is None else mask.ctypes.data, out["h"], out["n2"].ctypes.data,
                                        out["data"].ctypes.data if want_data else None))
        return out

    def lsm_solve(self, nshots, sx0, dsx, sz, gz, srce, d_obs, niter, m=None, mask=None, v2_all=None, draw_offset=0, verify=False, want_resid=False):
        """`niter` conjugate-gradient iterations on min_m 1/2 sum_s |Born_DTT_s m - d_s|^2 (fdwave.h, fdw_lsm_solve); shots and models as
        shot_batch takes them, d_obs[nshots][nx][nt], m the start model (None: zeros), mask[nx][nz] or None.  Returns a dict: m, misfit
        (niter + 1 float64 values, one more -- the recomputed misfit -- with verify) and, with verify and want_resid, resid[nshots][nx][nt]."""
        out = {"m": np.zeros((self.nx, self.nz), np.float32) if m is None else np.array(_f32(m, (self.nx, self.nz)), order="C"),
               "misfit": np.zeros(niter + 1 + int(bool(verify)) if niter >= 0 else 1, np.float64)}
        if want_resid:
            out["resid"] = np.zeros((nshots, self.nx, self.nt), np.float32)
        v2_all = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze))
        mask = None if mask is None else _f32(mask, (self.nx, self.nz))
        check(lib().fdw_lsm_solve(self._h, nshots, None if v2_all is None else v2_all.ctypes.data, int(draw_offset), sx0, dsx, sz, gz, _f32(srce, (self.nt,)),
                                  _f32(d_obs, (nshots, self.nx, self.nt)), None if mask is None else mask.ctypes.data, niter, out["m"],
                                  out["misfit"].ctypes.data, int(bool(verify)), out["resid"].ctypes.data if want_resid else None))
        return out

    # ---- line sources (fdwave.h: plane-wave and encoded-shot migration) ----
    def shot_line(self, v2, sz, gz, wav, d_obs, imloc=None, want_fields=False, want_illum=False, illum=None):
        """shot() (v2=None: shot_resident()) whose forward loop is driven by the line source wav[nx][nt] at depth sz instead of a point source
        (fdwave.h, fdw_shot_line).  Returns what shot() returns."""
        shape = (self.nxe, self.nze)
        imloc = np.zeros((self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")
        P = np.zeros(shape, np.float32) if want_fields else None
        PP = np.zeros(shape, np.float32) if want_fields else None
        if want_illum:
            illum = np.zeros((self.nx, self.nz), np.float32) if illum is None else np.array(_f32(illum, (self.nx, self.nz)), order="C")
        check(lib().fdw_shot_line(self._h, None if v2 is None else _f32(v2, shape).ctypes.data, sz, gz, _f32(wav, (self.nx, self.nt)),
                                  _f32(d_obs, (self.nx, self.nt)), imloc, illum.ctypes.data if want_illum else None,
                                  P.ctypes.data if want_fields else None, PP.ctypes.data if want_fields else None))
        out = (imloc, P, PP) if want_fields else (imloc,)
        out = out + (illum,) if want_illum else out
        return out if len(out) > 1 else imloc

    def record_shot_line(self, v2, sz, gz, wav, want_fields=False):
        """record_shot() driven by the line source wav[nx][nt] at depth sz (fdwave.h, fdw_record_shot_line); v2=None: the resident model."""
        shape = (self.nxe, self.nze)
        data = np.zeros((self.nx, self.nt), np.float32)
        P = np.zeros(shape, np.float32) if want_fields else None
        PP = np.zeros(shape, np.float32) if want_fields else None
        check(lib().fdw_record_shot_line(self._h, None if v2 is None else _f32(v2, shape).ctypes.data, sz, gz, _f32(wav, (self.nx, self.nt)), data,
                                         P.ctypes.data if want_fields else None, PP.ctypes.data if want_fields else None))
        return (data, P, PP) if want_fields else data

    def dev_line_steps(self, bufs, d_v2, d_wav, sz, it0, nsteps, gz=0, d_rec=None, d_illum=None, first_pp_twice=False, ip=0, ipp=1, stream=None):
        """dev_steps2 / dev_record_steps / dev_illum_steps driven by the line source d_wav (device [it][nx]) at depth sz (fdwave.h).
        Returns (ip, ipp) as dev_steps2 does.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        arr = (C.c_void_p * 4)(*bufs)
        a, b = C.c_int(ip), C.c_int(ipp)
        check(lib().fdw_dev_line_steps(self._h, arr, d_v2, d_wav, sz, gz, d_rec, d_illum, it0, nsteps, int(first_pp_twice), C.byref(a), C.byref(b),
                                       stream))
        return a.value, b.value

    def dev_line_record_illum_steps(self, bufs, d_v2, d_wav, sz, gz, d_rec, d_illum, it0, nsteps, first_pp_twice=False, ip=0, ipp=1, stream=None):
        """dev_line_steps that writes the trace rows AND accumulates the illumination, one launch per pass (fdwave.h).  Returns (ip, ipp).
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        arr = (C.c_void_p * 4)(*bufs)
        a, b = C.c_int(ip), C.c_int(ipp)
        check(lib().fdw_dev_line_record_illum_steps(self._h, arr, d_v2, d_wav, sz, gz, d_rec, d_illum, it0, nsteps, int(first_pp_twice), C.byref(a),
                                                    C.byref(b), stream))
        return a.value, b.value

    # ---- excitation-amplitude imaging (fdwave.h: a receiver-only backward loop) ----
    def dev_excite_steps(self, bufs, d_v2, d_srce, sx, sz, d_amp, d_texc, it0, nsteps, first_pp_twice=False, ip=0, ipp=1, stream=None):
        """dev_steps2 that also keeps the excitation maps d_amp (float) / d_texc (int32), device [nxl][pitch] (fdwave.h).  Returns (ip, ipp).
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        arr = (C.c_void_p * 4)(*bufs)
        a, b = C.c_int(ip), C.c_int(ipp)
        check(lib().fdw_dev_excite_steps(self._h, arr, d_v2, d_srce, sx, sz, d_amp, d_texc, it0, nsteps, int(first_pp_twice), C.byref(a), C.byref(b),
                                         stream))
        return a.value, b.value

    def dev_line_pick_steps(self, bufs, d_v2, d_wav, sz, d_texc, top, d_exc, it0, nsteps, first_pp_twice=False, ip=0, ipp=1, stream=None):
        """dev_line_steps (plain) that also takes the excitation pick: d_exc = the new field where d_texc == top - it (fdwave.h).  Returns
        (ip, ipp).
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        arr = (C.c_void_p * 4)(*bufs)
        a, b = C.c_int(ip), C.c_int(ipp)
        check(lib().fdw_dev_line_pick_steps(self._h, arr, d_v2, d_wav, sz, d_texc, top, d_exc, it0, nsteps, int(first_pp_twice), C.byref(a),
                                            C.byref(b), stream))
        return a.value, b.value

    def dev_image_excitation(self, d_exc, d_amp, eps, d_img, stream=None):
        """The excitation-amplitude image of one shot on device arrays [nxl][pitch] (fdwave.h, fdw_dev_image_excitation): on the interior,
        d_img += d_exc / d_amp where |d_amp| > eps * max |d_amp|; every other word of d_img keeps its bits.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_image_excitation(self._h, d_exc, d_amp, eps, d_img, stream))

    def shot_excitation_batch(self, nshots, sx0, dsx, sz, gz, srce, d_obs, eps=1e-3, v2_all=None, draw_offset=0, imloc=None, want_stack=True,
                              want_maps=True):
        """`nshots` excitation-amplitude shots stacked into one image in shot order, through one launch per time step where shot_batch()
        batches (fdwave.h, fdw_shot_excitation_batch).  d_obs[nshots][nx][nt]; models as shot_batch() takes them.  Returns a dict: image
        [nx][nz] (a copy of imloc, zeros if None, with every shot's image added), and as asked stack [nshots][nx][nz] (the running image after
        each shot) and exc, amp, texc [nshots][nx][nz]."""
        inner = (self.nx, self.nz)
        out = {"image": np.zeros(inner, np.float32) if imloc is None else np.array(_f32(imloc, inner), order="C")}
        if want_stack:
            out["stack"] = np.zeros((nshots,) + inner, np.float32)
        if want_maps:
            out["exc"], out["amp"], out["texc"] = (np.zeros((nshots,) + inner, t) for t in (np.float32, np.float32, np.int32))

        def ptr(name):
            return out[name].ctypes.data if name in out else None

        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        srce = _f32(srce, (self.nt,))
        d_obs = _f32(d_obs, (nshots, self.nx, self.nt))
        check(lib().fdw_shot_excitation_batch(self._h, nshots, v2p, int(draw_offset), sx0, dsx, sz, gz, srce.ctypes.data, d_obs.ctypes.data, eps,
                                              ptr("image"), ptr("stack"), ptr("exc"), ptr("amp"), ptr("texc")))
        return out

    def shot_excitation(self, v2, sx, sz, gz, srce, d_obs, eps=1e-3, imloc=None, want_fields=False, want_maps=True):
        """One shot under the excitation-amplitude imaging condition (fdwave.h, fdw_shot_excitation); v2=None: the resident model.  Returns
        (imloc, exc, amp, texc), the interiors [nx][nz] (texc int32), and with want_fields also P, PP as shot() returns them.  imloc (a copy of
        the one passed in, zeros if None) has the shot's image added to it.  want_maps=False: only the image comes back (one download);
        exc, amp and texc are None."""
        shape = (self.nxe, self.nze)
        inner = (self.nx, self.nz)
        imloc = np.zeros(inner, np.float32) if imloc is None else np.array(_f32(imloc, inner), order="C")
        if not want_maps:
            srce, d_obs = _f32(srce, (self.nt,)), _f32(d_obs, inner[:1] + (self.nt,))
            check(lib().fdw_shot_excitation(self._h, None if v2 is None else _f32(v2, shape).ctypes.data, sx, sz, gz, srce.ctypes.data, d_obs.ctypes.data,
                                            eps, imloc.ctypes.data, None, None, None, None, None))
            return imloc, None, None, None
        exc, amp, texc = np.zeros(inner, np.float32), np.zeros(inner, np.float32), np.zeros(inner, np.int32)
        P = np.zeros(shape, np.float32) if want_fields else None
        PP = np.zeros(shape, np.float32) if want_fields else None
        srce = _f32(srce, (self.nt,))
        d_obs = _f32(d_obs, inner[:1] + (self.nt,))
        check(lib().fdw_shot_excitation(self._h, None if v2 is None else _f32(v2, shape).ctypes.data, sx, sz, gz, srce.ctypes.data, d_obs.ctypes.data,
                                        eps, imloc.ctypes.data, exc.ctypes.data, amp.ctypes.data, texc.ctypes.data,
                                        P.ctypes.data if want_fields else None, PP.ctypes.data if want_fields else None))
        out = (imloc, exc, amp, texc)
        return out + (P, PP) if want_fields else out

    def shot_line_residual(self, v2, sz, gz, wav, d_obs, imloc=None, want_resid=True, want_fields=False, want_illum=False, illum=None):
        """Residual migration with a line source (fdwave.h, fdw_shot_line_residual): shot_line() whose forward loop also models the gather d_mod
        of record_shot_line() and whose backward loop migrates d_obs - d_mod.  Returns a dict as shot_residual() does."""
        shape = (self.nxe, self.nze)
        out = {"image": np.zeros((self.nx, self.nz), np.float32) if imloc is None else np.array(imloc, np.float32, order="C")}
        if want_resid:
            out["resid"] = np.zeros((self.nx, self.nt), np.float32)
        if want_fields:
            out["P"], out["PP"] = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        if want_illum:
            out["illum"] = np.zeros((self.nx, self.nz), np.float32) if illum is None else np.array(_f32(illum, (self.nx, self.nz)), order="C")

        def ptr(name):
            return out[name].ctypes.data if name in out else None

        check(lib().fdw_shot_line_residual(self._h, None if v2 is None else _f32(v2, shape).ctypes.data, sz, gz, _f32(wav, (self.nx, self.nt)),
                                           _f32(d_obs, (self.nx, self.nt)), out["image"], ptr("illum"), ptr("resid"), ptr("P"), ptr("PP")))
        return out

    def shot_line_batch(self, nshots, sz, gz, wav_all, d_obs, v2_all=None, draw_offset=0, imloc=None, want_illum=False, illum=None):
        """`nshots` line-source shots (shot_line) through one launch per time step where shot_batch batches: wav_all, d_obs [nshots][nx][nt],
        models as shot_batch takes them.  Returns imloc[nshots][nx][nz], or (imloc, illum) with want_illum."""
        shape = (nshots, self.nx, self.nz)
        imloc = np.zeros(shape, np.float32) if imloc is None else np.array(_f32(imloc, shape), order="C")
        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        if want_illum:
            illum = np.zeros(shape, np.float32) if illum is None else np.array(_f32(illum, shape), order="C")
        check(lib().fdw_shot_line_batch(self._h, nshots, v2p, int(draw_offset), sz, gz, _f32(wav_all, (nshots, self.nx, self.nt)),
                                        _f32(d_obs, (nshots, self.nx, self.nt)), imloc, illum.ctypes.data if want_illum else None))
        return (imloc, illum) if want_illum else imloc

    def shot_line_batch_residual(self, nshots, sz, gz, wav_all, d_obs, v2_all=None, draw_offset=0, imloc=None, want_resid=True, want_illum=False,
                                 illum=None):
        """`nshots` residual migrations with line sources (shot_line_residual), batched as shot_line_batch.  Returns a dict: image
        [nshots][nx][nz], and resid [nshots][nx][nt] / illum [nshots][nx][nz] as asked."""
        shape = (nshots, self.nx, self.nz)
        out = {"image": np.zeros(shape, np.float32) if imloc is None else np.array(_f32(imloc, shape), order="C")}
        if want_resid:
            out["resid"] = np.zeros((nshots, self.nx, self.nt), np.float32)
        if want_illum:
            out["illum"] = np.zeros(shape, np.float32) if illum is None else np.array(_f32(illum, shape), order="C")
        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        check(lib().fdw_shot_line_batch_residual(self._h, nshots, v2p, int(draw_offset), sz, gz, _f32(wav_all, (nshots, self.nx, self.nt)),
                                                 _f32(d_obs, (nshots, self.nx, self.nt)), out["image"],
                                                 out["illum"].ctypes.data if want_illum else None, out["resid"].ctypes.data if want_resid else None))
        return out

    def record_shot_line_batch(self, nshots, sz, gz, wav_all, v2_all=None, draw_offset=0):
        """`nshots` gathers recorded with line sources (record_shot_line), batched as shot_line_batch: data[nshots][nx][nt]."""
        data = np.zeros((nshots, self.nx, self.nt), np.float32)
        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        check(lib().fdw_record_shot_line_batch(self._h, nshots, v2p, int(draw_offset), sz, gz, _f32(wav_all, (nshots, self.nx, self.nt)), data))
        return data

    def debug_step4_plan_line(self, sz, r0=0, r1=-1, r0b=0, r1b=0, xchunk=0):
        """(nblk, nstrip, cls) of a four-step pass of dev_line_steps with the line at depth sz: cls[chunk row * nstrip + strip] = 0 lean, 1 full."""
        nblk, nstrip = C.c_int(), C.c_int()
        check(lib().fdw_debug_step4_plan_line(self._h, sz, r0, r1, r0b, r1b, xchunk, C.byref(nblk), C.byref(nstrip), None, 0))
        cls = np.zeros(nblk.value, np.uint8)
        check(lib().fdw_debug_step4_plan_line(self._h, sz, r0, r1, r0b, r1b, xchunk, C.byref(nblk), C.byref(nstrip), cls.ctypes.data, cls.size))
        return nblk.value, nstrip.value, cls

    def record_shot_batch(self, nshots, sx0, dsx, sz, gz, srce, v2_all=None, draw_offset=0):
        """`nshots` recorded gathers, source rows sx0 + b dsx, models as shot_batch takes them: data[nshots][nx][nt]."""
        data = np.zeros((nshots, self.nx, self.nt), np.float32)
        v2p = None if v2_all is None else _f32(v2_all, (nshots, self.nxe, self.nze)).ctypes.data
        check(lib().fdw_record_shot_batch(self._h, nshots, v2p, int(draw_offset), sx0, dsx, sz, gz, _f32(srce, (self.nt,)), data))
        return data

    def shot_batch_max(self):
        return int(lib().fdw_shot_batch_max(self._h))

    def rand_stream(self, draw_offset, n):
        """Draws [draw_offset, draw_offset + n) of the unseeded glibc rand() stream as the device generator produces them."""
        out = np.zeros(n, np.int32)
        check(lib().fdw_rand_stream(self._h, int(draw_offset), n, out.ctypes.data))
        return out

    def model_shot(self, vel2, sx, sz, gz, srce):
        """One shot of mod_main's loop (dpct_gpu_rtm_domain_division/src/mod_main.cpp:140-174): the gather data[nx][nt]."""
        srce = _f32(srce)
        data = np.zeros((self.nx, srce.size), np.float32)
        check(lib().fdw_model_shot(self._h, _f32(vel2, (self.nxe, self.nze)), sx, sz, gz, srce, srce.size, data))
        return data

    def model_shot_batch(self, nshots, vel2, sx0, dsx, sz, gz, srce):
        """`nshots` consecutive shots of mod_main's loop through one launch per time step: data[nshots][nx][nt]."""
        srce = _f32(srce)
        data = np.zeros((nshots, self.nx, srce.size), np.float32)
        check(lib().fdw_model_shot_batch(self._h, nshots, _f32(vel2, (self.nxe, self.nze)), sx0, dsx, sz, gz, srce, srce.size, data))
        return data

    def rtm_stored_shot(self, vel2, sx, sz, gz, srce, dobs, shot=0):
        """One shot of the sibling's stored-wavefield RTM (dpct_gpu_rtm_domain_division/src/rtm_main.cpp:158-240); dobs is the WHOLE
        gather [ns][nx][nt] (the reference reads one sample past each trace, see fdwave.h).  Returns imloc[nx][nz]."""
        srce = _f32(srce)
        dobs = np.ascontiguousarray(dobs, np.float32).ravel()
        imloc = np.zeros((self.nx, self.nz), np.float32)
        check(lib().fdw_rtm_stored_shot(self._h, _f32(vel2, (self.nxe, self.nze)), sx, sz, gz, srce, srce.size, dobs, dobs.size, shot, imloc))
        return imloc

    def dev_check_field(self, d_f, stream=None):
        """The precondition of the lazy damping checked on a DEVICE array (compat extents: the damped strip must be zero on the rows the
        reference never time-steps; fdwave.h).  Raises FdwError if it is violated; synchronises the stream.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: the check is issued on it -- and, the one exception among the dev_* methods, this call SYNCHRONISES it (fdwave.h)."""
        check(lib().fdw_dev_check_field(self._h, d_f, stream))

    def set_store_budget(self, nbytes):
        """Bytes the stored source fields of rtm_stored_shot may occupy (0: no limit of our own).  Below nt + 1 fields the shot checkpoints and
        recomputes (fdwave.h); the image stays bit-identical."""
        check(lib().fdw_set_store_budget(self._h, int(nbytes)))

    def store_segments(self):
        """Segments the last rtm_stored_shot was cut into (1: every field was kept)."""
        return int(lib().fdw_store_segments(self._h))

    def set_batch_budget(self, nbytes):
        """Bytes the buffers of a batch of shots may take (0: FDW_BATCH_BUDGET_BYTES if set, else 6 GiB; a non-zero value wins over the
        environment).  It bounds shot_batch_max() and the parts the batched calls cut a batch into (fdwave.h); results never depend on it."""
        check(lib().fdw_set_batch_budget(self._h, int(nbytes)))

    def batch_parts(self):
        """Batched launch sequences of the last batched call (0: its shots ran one by one, 1: the whole batch at once, k: k parts)."""
        return int(lib().fdw_batch_parts(self._h))

    def field_bytes(self):
        return int(lib().fdw_field_bytes(self._h))

    def dev_model_steps(self, d_p, d_pp, d_v2, d_srce, sx, sz, gz, d_rec, it0, nsteps, stream=None):
        """stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_model_steps(self._h, d_p, d_pp, d_v2, d_srce, sx, sz, gz, d_rec, it0, nsteps, stream))

    # ---- device-array API (raw pointers; see device.py for torch helpers) -----------------------
    # THE STREAM CONTRACT of every dev_* method (fdwave.h, pinned by tests/test_stream_contract.py):
    #   stream=None   the context's own hipStreamNonBlocking stream.  It has NO implicit ordering against the caller's streams, the legacy
    #                 default stream included: whatever filled the buffers must have completed (torch.cuda.synchronize(), or an event the
    #                 caller has waited for on the host) before the call, and the results are ready only after the device was synchronised.
    #   stream=S      (a hipStream_t as an int, e.g. torch.cuda.Stream().cuda_stream) every launch, copy and memset of the call is issued on
    #                 S and the call returns without synchronising: work queued on S before the call is seen by it, work queued on S after
    #                 it sees its results.  The one exception is dev_check_field, which synchronises S to return its count.
    def dev_step(self, mode, d_p, d_pp, d_v2, r0=0, r1=None, pp_twice=True, d_inj=None, inj_x=-1, inj_z=0,
                 d_psrc=None, d_img=None, stream=None):
        """One fused time step (fdwave.h, fdw_dev_step; mode 3 is dev_laplacian's).  stream: the contract above -- None is the context's own
        non-blocking stream, unordered against the caller's; a caller's stream carries every launch of the call."""
        r1 = self.nxl if r1 is None else r1
        check(lib().fdw_dev_step(self._h, mode, d_p, d_pp, d_v2, r0, r1, int(pp_twice), d_inj, inj_x, inj_z,
                                 d_psrc, d_img, stream))

    def dev_back_iter(self, step_source, d_f1, d_f0, d_pr, d_ppr, d_v2, r0, r1, pp_twice, d_samples, gz, d_img, stream=None):
        """One iteration of fd_back's loop (fd-code.cu:302-339) on local rows [r0, r1): see fdwave.h.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_back_iter(self._h, int(step_source), d_f1, d_f0, d_pr, d_ppr, d_v2, r0, r1, int(pp_twice), d_samples, gz, d_img, stream))

    def dev_back4(self, d_f1, d_f0, d_fo1, d_fo2, d_lvl0, d_lvl1, d_pr, d_ppr, d_ro1, d_ro2, d_v2, d_samples, sample_stride, gz, d_img, pp_twice=True,
                  r0=0, r1=-1, r0b=0, r1b=0, xchunk=0, stream=None):
        """Four iterations of fd_back's loop as two passes of the wave pipeline on local rows [r0, r1) (+ [r0b, r1b)); r1 < 0 = all rows: see
        fdwave.h.  stream: the contract above -- None is the context's own non-blocking stream, unordered against the caller's; a caller's
        stream carries every launch and copy of the call, which does not synchronise."""
        check(lib().fdw_dev_back4(self._h, d_f1, d_f0, d_fo1, d_fo2, d_lvl0, d_lvl1, d_pr, d_ppr, d_ro1, d_ro2, d_v2, d_samples, int(sample_stride), gz,
                                  d_img, int(pp_twice), r0, r1, r0b, r1b, xchunk, stream))

    def dev_steps(self, d_p, d_pp, d_v2, d_srce, sx, sz, it0, nsteps, first_pp_twice=False, stream=None):
        """nsteps forward iterations on two buffers (one-step kernel; fdwave.h, fdw_dev_steps).
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_steps(self._h, d_p, d_pp, d_v2, d_srce, sx, sz, it0, nsteps, int(first_pp_twice), stream))

    def dev_steps_shrink(self, d_p, d_pp, d_v2, d_srce, sx, sz, it0, nsteps, first_pp_twice, j0, shrink_lo, shrink_hi, stream=None):
        """stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_steps_shrink(self._h, d_p, d_pp, d_v2, d_srce, sx, sz, it0, nsteps, int(first_pp_twice), j0,
                                         int(shrink_lo), int(shrink_hi), stream))

    def dev_step2(self, d_p, d_pp, d_v2, d_out1, d_out2, pp_twice=True, d_srce_it=None, sx=-1, sz=0, stream=None):
        """Two forward iterations in one pass (temporal blocking); d_p is the NEWEST field.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_step2(self._h, d_p, d_pp, d_v2, d_out1, d_out2, int(pp_twice), d_srce_it, sx, sz, stream))

    def dev_step4(self, d_p, d_pp, d_v2, d_out1, d_out2, pp_twice=True, d_srce_it=None, sx=-1, sz=0, r0=0, r1=-1, r0b=0, r1b=0, xchunk=0, stream=None):
        """Four forward iterations in one pass (wave pipeline) on local rows [r0, r1) (+ [r0b, r1b)); r1 < 0 = all rows.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_step4(self._h, d_p, d_pp, d_v2, d_out1, d_out2, int(pp_twice), d_srce_it, sx, sz, r0, r1, r0b, r1b, xchunk, stream))

    def dev_steps2(self, bufs, d_v2, d_srce, sx, sz, it0, nsteps, first_pp_twice=False, ip=0, ipp=1, stream=None):
        """nsteps iterations over four rotating device buffers (pairs via the two-step kernel).
        Returns the indices (ip, ipp) of the reference's (d_p, d_pp) after the loop.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h).  On large grids the
        four-step passes run as row bands, part of them on a side stream of the context that starts behind `stream` and is joined into it
        before the call returns (set_pass_bands; fdwave.h): towards the caller the ordering is the same."""
        arr = (C.c_void_p * 4)(*bufs)
        a, b = C.c_int(ip), C.c_int(ipp)
        check(lib().fdw_dev_steps2(self._h, arr, d_v2, d_srce, sx, sz, it0, nsteps, int(first_pp_twice), C.byref(a), C.byref(b), stream))
        return a.value, b.value

    def dev_record_steps(self, bufs, d_v2, d_srce, sx, sz, gz, d_rec, it0, nsteps, first_pp_twice=False, ip=0, ipp=1, stream=None):
        """dev_steps2 that also writes the trace samples of iteration it to d_rec + it * nx (device [it][nx]; fdwave.h).
        Returns (ip, ipp) as dev_steps2 does.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        arr = (C.c_void_p * 4)(*bufs)
        a, b = C.c_int(ip), C.c_int(ipp)
        check(lib().fdw_dev_record_steps(self._h, arr, d_v2, d_srce, sx, sz, gz, d_rec, it0, nsteps, int(first_pp_twice), C.byref(a), C.byref(b), stream))
        return a.value, b.value

    def dev_illum_steps(self, bufs, d_v2, d_srce, sx, sz, d_illum, it0, nsteps, first_pp_twice=False, ip=0, ipp=1, stream=None):
        """dev_steps2 that also adds the square of every step's new field to d_illum (device [nxl][pitch]; fdwave.h).
        Returns (ip, ipp) as dev_steps2 does.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        arr = (C.c_void_p * 4)(*bufs)
        a, b = C.c_int(ip), C.c_int(ipp)
        check(lib().fdw_dev_illum_steps(self._h, arr, d_v2, d_srce, sx, sz, d_illum, it0, nsteps, int(first_pp_twice), C.byref(a), C.byref(b), stream))
        return a.value, b.value

    def dev_record_illum_steps(self, bufs, d_v2, d_srce, sx, sz, gz, d_rec, d_illum, it0, nsteps, first_pp_twice=False, ip=0, ipp=1, stream=None):
        """dev_steps2 that writes the trace rows of dev_record_steps and accumulates as dev_illum_steps does, one launch per pass (fdwave.h).
        Returns (ip, ipp) as dev_steps2 does.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        arr = (C.c_void_p * 4)(*bufs)
        a, b = C.c_int(ip), C.c_int(ipp)
        check(lib().fdw_dev_record_illum_steps(self._h, arr, d_v2, d_srce, sx, sz, gz, d_rec, d_illum, it0, nsteps, int(first_pp_twice), C.byref(a),
                                               C.byref(b), stream))
        return a.value, b.value

    def dev_gather_residual(self, d_a, d_b, d_out, n, stream=None):
        """d_out[i] = d_a[i] - d_b[i] for i < n on device arrays of floats (one fp32 subtraction each); d_out may be d_a.
        stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_gather_residual(self._h, d_a, d_b, d_out, int(n), stream))

    def dev_taper_finalize(self, d_f, stream=None):
        """stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_taper_finalize(self._h, d_f, stream))

    def dev_laplacian(self, d_p, d_lap, stream=None):
        """stream=None: the context's own non-blocking stream, unordered against the caller's streams (the legacy default stream included); a caller's
        stream: every launch, copy and memset of the call is issued on it and the call does not synchronise (fdwave.h)."""
        check(lib().fdw_dev_laplacian(self._h, d_p, d_lap, stream))

    def upload(self, d_dst, h_src):
        check(lib().fdw_upload_field(self._h, d_dst, _f32(h_src, (self.nxl, self.nze))))

    def download(self, d_src):
        out = np.empty((self.nxl, self.nze), np.float32)
        check(lib().fdw_download_field(self._h, out, d_src))
        return out


# ---- literal reference names --------------------------------------------------------------------
_state = {"ctx": None}


def fd_init(order, nxe, nze, nxb, nzb, nt, ns, fac, dx, dz, dt):
    """fd_init (fd-code.cu:200): creates the process-global propagation state like the reference."""
    if _state["ctx"] is not None:
        _state["ctx"].close()
    _state["ctx"] = FDWave(order, nxe, nze, nxb, nzb, nt, fac, dx, dz, dt, compat=True)
    return _state["ctx"]


def fd_forward(order, p, pp, v2, nz, nx, nt, is_, sz, sx, srce, propag=0):
    """fd_forward (fd-code.cu:247): note the reference's nz-before-nx order; p/pp are updated in place."""
    ctx = _state["ctx"]
    if ctx is None:
        raise _lib.FdwError(_lib.FDW_ESTATE, "fd_init has not been called")
    P, PP = ctx.forward(v2, int(sx[is_]), sz, srce, p, pp, nt)
    p[...] = P
    pp[...] = PP


def fd_back(order, p, pp, pr, ppr, v2, nz, nx, nt, is_, sz, gz, snaps, imloc, d_obs):
    """fd_back (fd-code.cu:290): d_obs[is] is the [nx][nt] gather; imloc is accumulated in place."""
    ctx = _state["ctx"]
    if ctx is None:
        raise _lib.FdwError(_lib.FDW_ESTATE, "fd_init has not been called")
    imloc[...] = ctx.back(v2, snaps[0], snaps[1], np.asarray(d_obs[is_]).reshape(ctx.nx, ctx.nt), gz, imloc, nt)

"""TEST HELPER (not a conftest): a second statement of the reference's backward loop, written from R alone, for tests/test_backward_pins.py.

R = cuda_reference_RTM/src/fd-code.cu.  The CPU oracle (oracle/fdw_oracle.c) and the HIP kernels were written by the same hand, so a
shared misreading of fd_back (R:290-341) -- a trace index, the order of the two snapshots, an offset, which field is imaged or damped --
would pass every test that holds one to the other.  This module states the same loop again, as whole-array NumPy passes, and owes the
oracle nothing but the host tables that are pinned on their own (taper, scaled weights, Ricker: tests/test_oracle_golden.py).

Two statements of the loop share one body, `_Loop`:
  * zero velocity, fp32 (`forward_zero_velocity`, `back_zero_velocity`, `shot_zero_velocity`): with v2 == 0 the leap-frog of
    kernel_time (R:89) is pp = 2p - pp with the v2*dt2*lap term a signed zero, so no Laplacian is needed; every other pass is pointwise.
    Each reference operation is rounded to fp32 where the reference rounds it, so the result is exact: the oracle and every HIP path
    must equal it bit for bit.
  * float64 with propagation (`forward_f64`, `back_f64`, `shot_f64`): the same loop with the order-N Laplacian of kernel_lap (R:53-78)
    over its own launch extents, carried in float64.  The fp32 kernels are held to it within a tolerance.

`mutation=` applies one named misreading of fd_back (MUTATIONS_ZERO_VELOCITY, MUTATIONS_F64) so that the tests can show that the
pins catch what they are meant to catch.

Two of the reference's kernels race, and nothing here is evidence about how they resolve on the reference's hardware:
  * kernel_tapper (R:94-117): on the right-hand x strip, thread i scales column nx-1-i by taperx[i] while that column's own thread
    scales it by taperz[j].  The taper is applied as (p * taperz) * taperx on both sides.
  * kernel_sism (R:124-131): it is launched with 8 x 8 blocks, so the 8 threadIdx.y replicas of a receiver all add the same sample to
    one address.  One add per receiver is applied.
Both are conventions, the same ones the oracle takes (fdw_oracle.c orc_kernel_tapper, orc_kernel_sism); a test against this module
cannot tell whether they are the reference's behaviour.
"""
import numpy as np

from oracle import oracle as O

SIZEBLOCK = 8          # the reference's block edge (lib/include/functions.h `sizeblock`), dimBlock(sizeblock, sizeblock) at R:255, R:298

# every misreading below changes the image at zero velocity; the last three only show once waves propagate (the damped strip z < nzb
# never meets the imaged interior otherwise, and the receiver Laplacian is multiplied by v2 = 0)
MUTATIONS_ZERO_VELOCITY = (
    "snapshots_swapped",         # it == 0 takes snaps[0] instead of snaps[1] (R:310 reads snaps[1-it])
    "trace_nt_minus_it",         # sample nt-it instead of nt-1-it (R:129)
    "trace_it",                  # the trace read forwards in time
    "gz_plus_1",                 # receivers one row deeper
    "receiver_x_plus_1",         # receivers one column to the right of i+nxb
    "image_before_injection",    # kernel_img launched before kernel_sism (R:328-329)
    "image_source_pp",           # the image reads d_pp instead of d_p (R:329)
    "image_receiver_pr",         # the image reads d_pr instead of d_ppr (R:329)
)
MUTATIONS_F64 = MUTATIONS_ZERO_VELOCITY + (
    "damp_source",               # kernel_tapper also on the reconstructed source field (R:317-323 has none)
    "undamped_receiver",         # no kernel_tapper on the receiver field (R:325)
    "receiver_lap_of_source",    # the receiver step's kernel_lap reads d_p instead of d_pr (R:326)
)


def launch_extents(nxe, nze, nzb, compat=True):
    """(xlim, zlim, ztap): threads launched along x, along z, and along z for kernel_tapper.

    R:185-195 assigns the float quotient to `int div_x` before ceil() sees it, so gridx = floor(nxe / 8) and the launch covers
    8 * floor(nxe / 8) rows; likewise gridz for nze and gridBorder_z for nzb (dimGridTaper = (gridx, gridBorder_z), R:250, R:295).
    compat=False is the product's option of covering the whole array."""
    if not compat:
        return nxe, nze, nzb
    gridx, gridz, grid_bz = int(float(nxe) / SIZEBLOCK), int(float(nze) / SIZEBLOCK), int(float(nzb) / SIZEBLOCK)
    return SIZEBLOCK * gridx, SIZEBLOCK * gridz, SIZEBLOCK * grid_bz


class _Loop:
    """The passes of fd_forward / fd_back on one deck in one precision (np.float32: rounded as the reference rounds; np.float64)."""

    def __init__(self, deck, dtype, v2=None, mutation=None):
        self.d, self.dt = deck, dtype
        self.nxe, self.nze, self.nxb, self.nzb, self.nt = deck["nxe"], deck["nze"], deck["nxb"], deck["nzb"], deck["nt"]
        self.nx, self.nz = self.nxe - 2 * self.nxb, self.nze - 2 * self.nzb
        assert self.nx > 0 and self.nz > 0
        self.h = deck["order"] // 2
        self.xlim, self.zlim, self.ztap = launch_extents(self.nxe, self.nze, self.nzb, deck.get("compat", True))
        tx, tz = O.taper_tables(self.nxb, self.nzb, deck["fac"])                       # R:159-166 (pinned host table)
        self.tx, self.tz = tx.astype(dtype), tz.astype(dtype)
        known = MUTATIONS_F64 if v2 is not None else MUTATIONS_ZERO_VELOCITY
        assert mutation is None or mutation in known, mutation
        self.mut = mutation
        if v2 is None:                       # zero velocity: kernel_lap's result only ever meets v2 = 0
            self.v2dt2 = None
        else:
            cx, cz = O.scaled_coefs(deck["order"], deck["dx"], deck["dz"])            # R:203-217 (pinned host table)
            self.cx, self.cz = cx.astype(np.float64), cz.astype(np.float64)
            dt2 = np.float32(deck["dt"]) * np.float32(deck["dt"])                        # R:205
            self.v2dt2 = np.asarray(v2, np.float64).reshape(self.nxe, self.nze) * np.float64(dt2)

    def zeros(self):
        return np.zeros((self.nxe, self.nze), self.dt)

    def field(self, a):
        return np.array(np.asarray(a, np.float32).reshape(self.nxe, self.nze), self.dt)

    def taper(self, p, pp):
        """kernel_tapper (R:94-117) on dimGridTaper: threads i < xlim, j < ztap; taperz where i < nx (= nxe), then the taperx pair where
        i < nxb on column i and its mirror nxe-1-i (the race convention of the module docstring)."""
        zt = min(self.ztap, self.nzb)
        xs = min(self.xlim, self.nxe)
        nl = min(self.xlim, self.nxb)
        assert self.nxe - nl >= nl                                                     # mirror columns never meet the left ones
        for f in (p, pp):
            f[:xs, :zt] *= self.tz[:zt]
            f[:nl, :zt] *= self.tx[:nl, None]
            f[self.nxe - 1 - np.arange(nl), :zt] *= self.tx[:nl, None]

    def lap(self, p):
        """kernel_lap (R:53-78): thread (ti, tj) works on i = h + ti < nxe - h, j = h + tj < nze - h with ti < xlim, tj < zlim; the
        rest of the shared d_laplace buffer is never written (zero: cudaMalloc'ed scratch only ever written on these extents)."""
        h = self.h
        i1, j1 = min(self.nxe - h, h + self.xlim), min(self.nze - h, h + self.zlim)
        out = np.zeros((self.nxe, self.nze), np.float64)
        if i1 <= h or j1 <= h:
            return out
        acc = np.zeros((i1 - h, j1 - h), np.float64)
        for io in range(2 * h + 1):
            a = io - h
            acc += p[h:i1, h + a:j1 + a] * self.cz[io] + p[h + a:i1 + a, h:j1] * self.cx[io]
        out[h:i1, h:j1] = acc
        return out

    def time(self, p, pp, lap_of):
        """kernel_lap + kernel_time (R:80-92) on threads i < xlim, j < zlim: pp = 2.*p - pp + v2*dt2*lap.  The literal 2. makes the sum a
        double; at zero velocity the v2*dt2*lap term is a signed zero and adds nothing, and the one rounding to fp32 is the store."""
        xl, zl = min(self.xlim, self.nxe), min(self.zlim, self.nze)
        u = 2.0 * p[:xl, :zl].astype(np.float64) - pp[:xl, :zl]
        if self.v2dt2 is not None:
            u += self.v2dt2[:xl, :zl] * self.lap(lap_of)[:xl, :zl]
        pp[:xl, :zl] = u

    def forward(self, sx, sz, srce, p, pp, nsteps):
        """fd_forward's loop (R:259-267): swap, taper, Laplacian + leap-frog, source add into d_pp.  Returns (d_p, d_pp)."""
        srce = np.asarray(srce, np.float32).astype(self.dt)
        for it in range(nsteps):
            p, pp = pp, p
            self.taper(p, pp)
            self.time(p, pp, p)
            pp[sx, sz] += srce[it]                                                       # kernel_src (R:119-122): one add
        return p, pp

    def _inject(self, ppr, d_obs, it, gz):
        """kernel_sism (R:124-131) on dimGridUpb: receiver i < nx - 2 nxb with i < xlim adds d_obs[i*nt + (nt-1-it)] at (i+nxb, gz)."""
        nt, n = self.nt, min(self.nx, self.xlim)
        k = {"trace_nt_minus_it": nt - it, "trace_it": it}.get(self.mut, nt - 1 - it)
        flat = np.concatenate([d_obs.ravel(), np.zeros(1, d_obs.dtype)])               # nt - it at it = 0 runs one sample past a trace
        samples = flat[np.minimum(np.arange(n) * nt + k, flat.size - 1)]
        x0 = self.nxb + (self.mut == "receiver_x_plus_1")
        ppr[x0:x0 + n, gz + (self.mut == "gz_plus_1")] += samples

    def _image(self, img, p, ppr):
        """kernel_img (R:133-144) on dimGrid: i < nx - 2 nxb, j < nz - 2 nzb, both within the launch."""
        ni, nj = min(self.nx, self.xlim), min(self.nz, self.zlim)
        img[:ni, :nj] += p[self.nxb:self.nxb + ni, self.nzb:self.nzb + nj] * ppr[self.nxb:self.nxb + ni, self.nzb:self.nzb + nj]

    def back(self, snap0, snap1, d_obs, gz, img, nsteps):
        """fd_back's loop (R:302-339) from four zero fields (R:511-514); snap0 = P, snap1 = PP of the forward pass (R:502-507)."""
        d_obs = np.asarray(d_obs, np.float32).reshape(self.nx, self.nt).astype(self.dt)
        snaps = (self.field(snap0), self.field(snap1))
        if self.mut == "snapshots_swapped":
            snaps = snaps[::-1]
        p, pp, pr, ppr = self.zeros(), self.zeros(), self.zeros(), self.zeros()
        for it in range(nsteps):
            if it < 2:
                pp = snaps[1 - it].copy()                                                # R:304-314: pp[ix][iz] = snaps[1-it][ix][iz]
            else:
                self.time(p, pp, p)                                                      # R:317-318: no taper on the source field
            p, pp = pp, p                                                                # R:321-323
            if self.mut == "damp_source":
                self.taper(p, pp)
            if self.mut != "undamped_receiver":
                self.taper(pr, ppr)                                                      # R:325
            self.time(pr, ppr, p if self.mut == "receiver_lap_of_source" else pr)      # R:326-327
            src = pp if self.mut == "image_source_pp" else p
            rec = pr if self.mut == "image_receiver_pr" else ppr
            if self.mut == "image_before_injection":
                self._image(img, src, rec)
                self._inject(ppr, d_obs, it, gz)
            else:
                self._inject(ppr, d_obs, it, gz)                                         # R:328
                self._image(img, src, rec)                                               # R:329
            pr, ppr = ppr, pr                                                            # R:331-333
        return img


def _start_image(loop, imloc):
    return np.zeros((loop.nx, loop.nz), loop.dt) if imloc is None else np.array(np.asarray(imloc, np.float32).reshape(loop.nx, loop.nz), loop.dt)


def _forward(deck, dtype, v2, sx, sz, srce, p, pp, nsteps):
    L = _Loop(deck, dtype, v2)
    p = L.zeros() if p is None else L.field(p)
    pp = L.zeros() if pp is None else L.field(pp)
    return L.forward(sx, sz, srce, p, pp, len(srce) if nsteps is None else nsteps)


def _back(deck, dtype, v2, snap0, snap1, d_obs, gz, imloc, nsteps, mutation):
    L = _Loop(deck, dtype, v2, mutation)
    return L.back(snap0, snap1, d_obs, gz, _start_image(L, imloc), L.nt if nsteps is None else nsteps)


def _shot(deck, dtype, v2, sx, sz, gz, srce, d_obs, imloc, mutation):
    """One shot of main()'s loop (R:496-518): fd_forward from zero fields, P / PP handed over as snaps[0] / snaps[1], fd_back."""
    P, PP = _forward(deck, dtype, v2, sx, sz, srce, None, None, deck["nt"])
    return _back(deck, dtype, v2, P, PP, d_obs, gz, imloc, None, mutation)


# ---- zero velocity, fp32, exact ---------------------------------------------------------------------------------------------------------
def forward_zero_velocity(deck, sx, sz, srce, p=None, pp=None, nsteps=None):
    """fd_forward at v2 == 0 in fp32: (d_p, d_pp)."""
    return _forward(deck, np.float32, None, sx, sz, srce, p, pp, nsteps)


def back_zero_velocity(deck, snap0, snap1, d_obs, gz, imloc=None, nsteps=None, mutation=None):
    """fd_back at v2 == 0 in fp32: imloc [nx][nz], accumulated onto imloc (R:243 uploads it)."""
    return _back(deck, np.float32, None, snap0, snap1, d_obs, gz, imloc, nsteps, mutation)


def shot_zero_velocity(deck, sx, sz, gz, srce, d_obs, imloc=None, mutation=None):
    """fd_forward + fd_back at v2 == 0 in fp32.  The source never leaves (sx, sz), so the image is zero unless sz == gz."""
    return _shot(deck, np.float32, None, sx, sz, gz, srce, d_obs, imloc, mutation)


# ---- float64 with propagation -----------------------------------------------------------------------------------------------------------
def forward_f64(deck, v2, sx, sz, srce, p=None, pp=None, nsteps=None):
    return _forward(deck, np.float64, v2, sx, sz, srce, p, pp, nsteps)


def back_f64(deck, v2, snap0, snap1, d_obs, gz, imloc=None, nsteps=None, mutation=None):
    return _back(deck, np.float64, v2, snap0, snap1, d_obs, gz, imloc, nsteps, mutation)


def shot_f64(deck, v2, sx, sz, gz, srce, d_obs, imloc=None, mutation=None):
    return _shot(deck, np.float64, v2, sx, sz, gz, srce, d_obs, imloc, mutation)

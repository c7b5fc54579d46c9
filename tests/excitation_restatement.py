"""TEST HELPER (not a conftest): the CPU restatements of excitation-amplitude imaging (fdwave.h, "excitation-amplitude imaging"), shared by
tests/test_excitation.py, tests/test_excitation_batch.py and the excitation cases of tests/stream_cases.py.  They use existing oracle calls
only; tests/test_excitation.py::test_restatement_guards pins them to Oracle.forward and line_restatement.
  Maps: the chain of tests/test_illum.py::illum_restatement (Oracle.forward, one iteration per call, PP after the call is the level u) with
        `win = |u| > |amp|; amp[win] = u[win]; texc[win] = it + 1` inside the update extents.
  Pick: the chain of tests/test_line_source.py::line_restatement (swap, Oracle.slab_step, the line add) with
        `hit = texc == top - it; exc[hit] = PP[hit]` inside the update extents.
  Image: fdw_image_excitation spelled in np.float32.
No arithmetic touches the maps, so every comparison is bit for bit (NaNs by position where the fields hold any)."""
import numpy as np

from test_line_source import extents_of


def maps_restatement(orc, v2, sx, sz, srce, xlim, zlim, p0=None, pp0=None, amp0=None, texc0=None, it0=0, maps=True):
    """(amp, texc, P, PP) after len(srce) iterations it0, it0 + 1, ... of the oracle's fd_forward chained one per call; compare and select
    only, inside the update extents only.  maps=False: the chain alone (its guard)."""
    P, PP = p0, pp0
    amp = np.zeros(orc.shape, np.float32) if amp0 is None else np.array(amp0, np.float32)
    texc = np.zeros(orc.shape, np.int32) if texc0 is None else np.array(texc0, np.int32)
    with np.errstate(all="ignore"):
        for k in range(len(srce)):
            P, PP = orc.forward(v2, sx, sz, srce[k:k + 1], P, PP)
            if maps:
                u, a, t = PP[:xlim, :zlim], amp[:xlim, :zlim], texc[:xlim, :zlim]
                win = np.abs(u) > np.abs(a)                      # strict; False wherever either side is a NaN
                a[win] = u[win]
                t[win] = it0 + k + 1
    return amp, texc, P, PP


def pick_restatement(orc, d, v2, w, sz, texc, top, exc0, p0=None, pp0=None, it0=0, nsteps=None):
    """dict(P, PP, exc, npicked) after iterations it0 .. it0 + nsteps - 1 of line_restatement's chain with the pick after the line add."""
    nxe, nze, nxb = d["nxe"], d["nze"], d["nxb"]
    nx = nxe - 2 * nxb
    xlim, zlim, _ = extents_of(d)
    nsrc = min(nx, xlim - nxb)
    P = np.zeros((nxe, nze), np.float32) if p0 is None else np.array(p0, np.float32, order="C")
    PP = np.zeros((nxe, nze), np.float32) if pp0 is None else np.array(pp0, np.float32, order="C")
    v2 = np.ascontiguousarray(v2, np.float32)
    exc = np.array(exc0, np.float32)
    nsteps = len(w) - it0 if nsteps is None else nsteps
    picked = np.zeros((nxe, nze), bool)
    iters = set()
    with np.errstate(all="ignore"):
        for it in range(it0, it0 + nsteps):
            P, PP = PP, P
            orc.slab_step(0, P, PP, v2, 0, nxe, -1, 0, 0.0)
            PP[nxb:nxb + nsrc, sz] = (PP[nxb:nxb + nsrc, sz] + np.asarray(w[it][:nsrc], np.float32)).astype(np.float32)
            if texc is not None:
                hit = np.asarray(texc)[:xlim, :zlim] == top - it
                exc[:xlim, :zlim][hit] = PP[:xlim, :zlim][hit]
                picked[:xlim, :zlim] |= hit
                if (hit & (PP[:xlim, :zlim] != 0)).any():
                    iters.add(it)
    return dict(P=P, PP=PP, exc=exc, picked=picked, iters=iters)


def image_selection(amp, eps):
    """The cells fdw_image_excitation updates: |amp| > eps (*) max |amp|, the max taken from 0.0f with > (a NaN never wins)."""
    amp = np.asarray(amp, np.float32).ravel()
    m = np.float32(0.0)
    with np.errstate(all="ignore"):
        for a in np.abs(amp):
            if a > m:
                m = a
        return np.abs(amp) > np.float32(eps) * m


def image_formula(exc, amp, eps, img):
    """fdw_image_excitation spelled in np.float32 (fdwave.h)."""
    exc, amp = np.asarray(exc, np.float32).ravel(), np.asarray(amp, np.float32).ravel()
    out = np.array(img, np.float32).ravel()
    sel = image_selection(amp, eps)
    with np.errstate(all="ignore"):
        out[sel] = (out[sel] + (exc[sel] / amp[sel]).astype(np.float32)).astype(np.float32)
    return out.reshape(np.shape(img))


def shot_restatement(orc, d, v2, sx, sz, gz, srce, d_obs):
    """fdw_shot_excitation from rest: (exc, amp, texc, P, PP, iterations with a non-zero pick) on the extended grid."""
    xlim, zlim, _ = extents_of(d)
    nt = len(srce)
    amp, texc, P, PP = maps_restatement(orc, v2, sx, sz, srce, xlim, zlim)
    w = np.ascontiguousarray(d_obs[:, ::-1].T)                 # row k = d_obs[.][nt-1-k]
    r = pick_restatement(orc, d, v2, w, gz, texc, nt, np.zeros(orc.shape, np.float32))
    return r["exc"], amp, texc, P, PP, r["iters"]

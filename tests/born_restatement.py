"""TEST HELPER (not a conftest): the CPU restatement of Born modelling (fdwave.h, "Born modelling"), shared by tests/test_born.py.  Existing
oracle calls only.  Per iteration, as fdwave.h numbers the steps:
  1. the background pair: swap; Oracle.slab_step(0, P, PP, v2, 0, nxe, -1, 0, 0.0); the point add at (sx, sz) -- the chain
     tests/test_line_source.py::line_restatement(point=...) guards against Oracle.forward;
  2. the same chain without the add on the scattered pair;
  3. the scatter on C in np.float32, product and sum rounded separately: D = D + m * q, q = U or (U - A) - (A - B), A and B the words the
     background pair held on C before the swap (no cell of C is damped, so the oracle's eagerly damped arrays hold the raw words there);
  4. the trace rows of both new fields.
Like the oracle's own arrays, the returned older fields (U_P, DU_P) have had the damping pass the device arrays still owe
(fdw_dev_taper_finalize); the newest (U_PP, DU_PP) are raw."""
import numpy as np

from test_line_source import extents_of

FIELD, DTT = 0, 1


def born_cells(d):
    """C as (x0, x1, z0, z1): rows [x0, x1), columns [z0, z1)."""
    nxe, nze, nxb, nzb = d["nxe"], d["nze"], d["nxb"], d["nzb"]
    xlim, zlim, _ = extents_of(d)
    return nxb, min(nxe - nxb, xlim), nzb, min(nze - nzb, zlim)


def embed_m(d, m_int, outside=0.0):
    """The interior reflectivity [nx][nz] as a field [nxe][nze]; `outside` fills every word that is not an interior cell."""
    nxe, nze, nxb, nzb = d["nxe"], d["nze"], d["nxb"], d["nzb"]
    f = np.full((nxe, nze), outside, np.float32)
    f[nxb:nxe - nxb, nzb:nze - nzb] = m_int
    return f


def born_restatement(orc, d, v2, m, kind, sx, sz, gz, srce, u0=None, u1=None, du0=None, du1=None, it0=0, nsteps=None, nt=None, scatter=True):
    """dict(U_P, U_PP, DU_P, DU_PP, rec[nt][nx], rec0[nt][nx]) after iterations it0 .. it0 + nsteps - 1 from the pairs (u0, u1) and (du0, du1)
    (None: rest).  m: field-shaped [nxe][nze], read on C only.  Rows of rec / rec0 outside the iterations run stay zero.  scatter=False: the two
    chains alone (the guard)."""
    f32 = np.float32
    nxe, nze, nxb = d["nxe"], d["nze"], d["nxb"]
    nx = nxe - 2 * nxb
    x0, x1, z0, z1 = born_cells(d)
    C = (slice(x0, x1), slice(z0, z1))
    new = lambda a: np.zeros((nxe, nze), f32) if a is None else np.array(a, f32, order="C")      # noqa: E731
    P, PP, DP, DPP = new(u0), new(u1), new(du0), new(du1)
    v2 = np.ascontiguousarray(v2, f32)
    m = np.asarray(m, f32)
    nsteps = len(srce) - it0 if nsteps is None else nsteps
    nt = max(len(srce), it0 + nsteps) if nt is None else nt
    rec, rec0 = np.zeros((nt, nx), f32), np.zeros((nt, nx), f32)
    with np.errstate(all="ignore"):
        for it in range(it0, it0 + nsteps):
            A, B = PP[C].copy(), P[C].copy()
            P, PP = PP, P
            orc.slab_step(0, P, PP, v2, 0, nxe, -1, 0, 0.0)
            PP[sx, sz] = f32(PP[sx, sz] + f32(srce[it]))
            DP, DPP = DPP, DP
            orc.slab_step(0, DP, DPP, v2, 0, nxe, -1, 0, 0.0)
            if scatter:
                U = PP[C]
                q = U if kind == FIELD else ((U - A).astype(f32) - (A - B).astype(f32)).astype(f32)
                DPP[C] = (DPP[C] + (m[C] * q).astype(f32)).astype(f32)
            rec[it] = DPP[nxb:nxb + nx, gz]
            rec0[it] = PP[nxb:nxb + nx, gz]
    return dict(U_P=P, U_PP=PP, DU_P=DP, DU_PP=DPP, rec=rec, rec0=rec0)

"""TEST HELPER (not a conftest): the CPU restatement of line-source Born modelling (fdwave.h, "Born modelling driven by a line source"),
shared by tests/test_born_batch.py.  It is tests/born_restatement.py::born_restatement with the point add of step 1 replaced by the line add
on rows nxb .. nxb+nsrc-1, nsrc = min(nx, xlim - nxb): the chain tests/test_line_source.py::line_restatement runs on the background pair.
Existing oracle calls only; steps 2-4 as born_restatement spells them."""
import numpy as np

from born_restatement import FIELD, born_cells
from test_line_source import extents_of


def born_line_restatement(orc, d, v2, m, kind, sz, gz, w, u0=None, u1=None, du0=None, du1=None, it0=0, nsteps=None, nt=None, scatter=True):
    """dict(U_P, U_PP, DU_P, DU_PP, rec[nt][nx], rec0[nt][nx]) after iterations it0 .. it0 + nsteps - 1.  w[it][ix]: the line samples (nx per
    iteration; those of rows ix >= nsrc are ignored).  Everything else as born_restatement."""
    f32 = np.float32
    nxe, nze, nxb = d["nxe"], d["nze"], d["nxb"]
    nx = nxe - 2 * nxb
    xlim, _, _ = extents_of(d)
    nsrc = min(nx, xlim - nxb)
    x0, x1, z0, z1 = born_cells(d)
    C = (slice(x0, x1), slice(z0, z1))
    new = lambda a: np.zeros((nxe, nze), f32) if a is None else np.array(a, f32, order="C")      # noqa: E731
    P, PP, DP, DPP = new(u0), new(u1), new(du0), new(du1)
    v2 = np.ascontiguousarray(v2, f32)
    m = np.asarray(m, f32)
    nsteps = len(w) - it0 if nsteps is None else nsteps
    nt = max(len(w), it0 + nsteps) if nt is None else nt
    rec, rec0 = np.zeros((nt, nx), f32), np.zeros((nt, nx), f32)
    with np.errstate(all="ignore"):
        for it in range(it0, it0 + nsteps):
            A, B = PP[C].copy(), P[C].copy()
            P, PP = PP, P
            orc.slab_step(0, P, PP, v2, 0, nxe, -1, 0, 0.0)
            PP[nxb:nxb + nsrc, sz] = (PP[nxb:nxb + nsrc, sz] + np.asarray(w[it][:nsrc], f32)).astype(f32)
            DP, DPP = DPP, DP
            orc.slab_step(0, DP, DPP, v2, 0, nxe, -1, 0, 0.0)
            if scatter:
                U = PP[C]
                q = U if kind == FIELD else ((U - A).astype(f32) - (A - B).astype(f32)).astype(f32)
                DPP[C] = (DPP[C] + (m[C] * q).astype(f32)).astype(f32)
            rec[it] = DPP[nxb:nxb + nx, gz]
            rec0[it] = PP[nxb:nxb + nx, gz]
    return dict(U_P=P, U_PP=PP, DU_P=DP, DU_PP=DPP, rec=rec, rec0=rec0)

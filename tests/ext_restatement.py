"""TEST HELPER (not a conftest): the CPU restatement of the subsurface-offset extended image (fdwave.h, "Extended imaging"), shared by
tests/test_ext_image.py.  numpy on top of tests/dtt_restatement.py's F and R, every operation rounded on its own:
  term    for h = -H .. H, on the cells of C whose rows x - h and x + h lie in C:   E[h+H][x][z] = E[h+H][x][z] + f[x-h][z] * r[x+h][z]
          (np.float32 product, then np.float32 sum); every other word of every plane as it came.
  loop    dtt_back_restatement's chain (Oracle.slab_back_iter with a throwaway image): after iteration k the term with f = F_k and
          r = r^{k+1}, k ascending."""
import numpy as np

from born_restatement import born_cells
from dtt_restatement import dtt_back_restatement

f32 = np.float32


def ext_term(E, f, r, H, cells):
    """One term added IN PLACE to the planes E [2H+1][rows][cols]; f, r arrays of the same [rows][cols]; cells = (x0, x1, z0, z1) in their
    coordinates."""
    x0, x1, z0, z1 = cells
    assert E.shape[0] == 2 * H + 1 and E.dtype == f32
    f, r = np.asarray(f, f32), np.asarray(r, f32)
    with np.errstate(all="ignore"):
        for h in range(-H, H + 1):
            a, b = x0 + abs(h), x1 - abs(h)
            if b <= a:
                continue
            prod = (f[a - h:b - h, z0:z1] * r[a + h:b + h, z0:z1]).astype(f32)
            E[h + H, a:b, z0:z1] = (E[h + H, a:b, z0:z1] + prod).astype(f32)
    return E


def ext_term_fields(d, E0, f, r, H):
    """One term on field-shaped arrays [nxe][nze] of deck d: a new array of planes."""
    return ext_term(np.array(E0, f32, order="C"), f, r, H, born_cells(d))


def ext_back_restatement(orc, d, v2, F1, F0, samples, gz, H, E0=None, nsteps=None):
    """The backward loop from the snapshots F1 = F_1, F0 = F_0 and receivers at rest, accumulating the extended image.  E0: the entry planes
    as fields [2H+1][nxe][nze] (None: zeros).  Returns dict(E: the planes as fields, xcorr: the cross-correlation image of the same chain as a
    field, F, R: {level: words on C})."""
    nxe, nze = d["nxe"], d["nze"]
    x0, x1, z0, z1 = born_cells(d)
    r = dtt_back_restatement(orc, d, v2, F1, F0, samples, gz, nsteps=nsteps)
    nsteps = len(samples) if nsteps is None else nsteps
    E = np.zeros((2 * H + 1, nxe, nze), f32) if E0 is None else np.array(E0, f32, order="C")
    onC = np.ascontiguousarray(E[:, x0:x1, z0:z1])
    for k in range(nsteps):
        ext_term(onC, r["F"][k], r["R"][k + 1], H, (0, x1 - x0, 0, z1 - z0))
    E[:, x0:x1, z0:z1] = onC
    return dict(E=E, xcorr=r["xcorr"], F=r["F"], R=r["R"])

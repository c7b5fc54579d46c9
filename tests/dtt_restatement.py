"""TEST HELPER (not a conftest): the CPU restatement of second-time-difference imaging (fdwave.h, "DTT imaging"), shared by tests/test_dtt.py.
Existing oracle calls only.
  fields  Oracle.slab_back_iter on the whole grid, one call per iteration, with a THROWAWAY image: a copy of the snapshot with
          step_source = 0 for k < 2, step_source = 1 from then on, F_k overwriting F_{k-2} (the chain tests/test_snaps.py guards against
          Oracle.back; test_dtt.py guards this copy of it too).  On the cell set C the oracle's eagerly damped arrays hold the raw words: no
          cell of C is ever damped.
  tail    two Oracle.slab_step(..., sx = -1, taper_rows = (0, 0)) calls on the source pair: the plain leap-frog of R:317-318 (test_dtt.py
          guards, on a damped deck, that this equals the source half of two more slab_back_iter(step_source = 1) calls).
  image   in np.float32 on C, every operation rounded on its own:
              q_k = (F_k - F_{k+1}) - (F_{k+1} - F_{k+2});   img = img + q_k * r^{k+1}      for k = 0 .. nsteps-1, ascending
          pairing = 0 pairs q_k with r^k instead (the off-by-one control of the dot-product test)."""
import numpy as np

from born_restatement import born_cells

f32 = np.float32


def dtt_back_restatement(orc, d, v2, F1, F0, samples, gz, img0=None, pr=None, ppr=None, nsteps=None, pairing=1, accumulate=None):
    """The DTT backward loop from the snapshots F1 = F_1 (fd_forward's handed-over P) and F0 = F_0 (u^nt) and the receiver pair (pr, ppr)
    (None: rest).  samples[k]: the nx receiver samples iteration k injects.  img0: the entry image as a field [nxe][nze] (None: zeros).
    Returns dict(img: the field, every word outside C as it came; xcorr: the throwaway cross-correlation image of the same chain;
    f_new, f_old: the source pair as fdw_dev_back_iter leaves it after nsteps iterations; r_new, r_old: the receiver pair (r_old damped as the
    oracle holds it); F, R: {level: words on C}).  accumulate: a dtype (np.float64) for the image sum of the dot-product test; None: fp32."""
    nxe, nze = d["nxe"], d["nze"]
    x0, x1, z0, z1 = born_cells(d)
    C = (slice(x0, x1), slice(z0, z1))
    v2 = np.ascontiguousarray(v2, f32)
    nsteps = len(samples) if nsteps is None else nsteps
    new = lambda a: np.zeros((nxe, nze), f32) if a is None else np.array(a, f32, order="C")      # noqa: E731
    f1, f0, pr, ppr, img = new(F1), new(F0), new(pr), new(ppr), new(img0)
    throw = np.zeros((nxe, nze), f32)
    unused = np.zeros((nxe, nze), f32)
    F = {0: f0[C].copy(), 1: f1[C].copy()}
    R = {0: pr[C].copy()}
    with np.errstate(all="ignore"):
        for k in range(nsteps):
            s = np.ascontiguousarray(samples[k], f32)
            if k < 2:
                orc.slab_back_iter(0, 0, (f0 if k == 0 else f1).copy(), unused, pr, ppr, v2, 0, nxe, s, gz, throw)
            else:
                orc.slab_back_iter(0, 1, f1, f0, pr, ppr, v2, 0, nxe, s, gz, throw)
                F[k] = f0[C].copy()
                f1, f0 = f0, f1
            R[k + 1] = ppr[C].copy()
            pr, ppr = ppr, pr
        # the tail: F_nsteps and F_{nsteps+1} (nsteps = 1: F_2 alone); f1 is the newest level the loop holds (F_1 while nsteps < 3)
        newer, older = f1, f0
        for lvl in range(max(nsteps, 2), nsteps + 2 if nsteps >= 1 else 0):
            nxt = np.array(older, f32, order="C")
            orc.slab_step(0, newer, nxt, v2, 0, nxe, -1, 0, 0.0, taper_rows=(0, 0))
            F[lvl] = nxt[C].copy()
            newer, older = nxt, newer
        acc = img[C].astype(accumulate) if accumulate else img[C].copy()
        for k in range(nsteps):
            q = ((F[k] - F[k + 1]).astype(f32) - (F[k + 1] - F[k + 2]).astype(f32)).astype(f32)
            r = R[k + 1] if pairing else R[k]
            acc = acc + (q.astype(accumulate) * r.astype(accumulate)) if accumulate else (acc + (q * r).astype(f32)).astype(f32)
    out_img = img.astype(accumulate) if accumulate else img
    out_img[C] = acc
    return dict(img=out_img, xcorr=throw, f_new=f1, f_old=f0, r_new=pr, r_old=ppr, F=F, R=R)

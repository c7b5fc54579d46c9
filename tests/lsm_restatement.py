"""TEST HELPER (not a conftest): the CPU restatement of least-squares migration (fdwave.h, "Least-squares migration"), shared by
tests/test_lsm.py.  The two loops are tests/born_restatement.py and tests/dtt_restatement.py; everything around them is numpy:
  sums      the order S of fdwave.h, written twice: sum_loop (a Python loop over one vector, the definition as it reads) and sum_rows (the
            same order for many rows at once).  Terms are float64 products of float32 values, which are exact.
  visit     Born loop, w = d_obs - q (or q), n2 = <w, w>, ws = w * v2[nxb+ix][gz], the DTT backward loop from the background pair the Born
            restatement returns (its older field already damped once, as the device's is after fdw_dev_taper_finalize) onto a zero image,
            h = h + mask * (img / v2) on C -- every fp32 operation rounded on its own.
  solve     the conjugate-gradient recurrences with float64 scalars and np.float32 updates.
Model-space vectors are fields [nxe][nze]; only the words on C are read or written.  Gathers are [nt][nx]."""
import numpy as np

from born_restatement import DTT, born_cells, born_restatement
from dtt_restatement import dtt_back_restatement

f32, f64 = np.float32, np.float64


def sum_loop(x):
    """S(x_0 .. x_{n-1}) as fdwave.h states it."""
    x = np.asarray(x, f64)
    s = [0.0] * 64
    for lane in range(64):
        for i in range(lane, len(x), 64):
            s[lane] = s[lane] + float(x[i])
    d = 32
    while d >= 1:
        for lane in range(d):
            s[lane] = s[lane] + s[lane + d]
        d //= 2
    return s[0]


def sum_rows(t):
    """S along the last axis of t [..., n] (float64), vectorised: padding a row with +0.0 adds +0.0 to partials that are never -0.0."""
    t = np.asarray(t, f64)
    lead, n = t.shape[:-1], t.shape[-1]
    k = -(-n // 64)
    pad = np.zeros(lead + (k * 64,), f64)
    pad[..., :n] = t
    pad = pad.reshape(lead + (k, 64))
    s = np.zeros(lead + (64,), f64)
    for j in range(k):
        s = s + pad[..., j, :]
    d = 32
    while d >= 1:
        s[..., :d] = s[..., :d] + s[..., d:2 * d]
        d //= 2
    return s[..., 0]


def dot_rows(a, b):
    """(row sums, total) of <a, b> for two float32 arrays [rows][n]."""
    rows = sum_rows(np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64))
    return rows, float(sum_rows(rows))


def cells(d):
    x0, x1, z0, z1 = born_cells(d)
    return slice(x0, x1), slice(z0, z1)


def dot_cells(d, a, b):
    C = cells(d)
    return dot_rows(a[C], b[C])


def gather_step(d, v2, q, d_obs, gz):
    """Steps 2 and 3: (w, ws, row sums of <w, w>, n2)."""
    nxb, nx = d["nxb"], d["nxe"] - 2 * d["nxb"]
    with np.errstate(all="ignore"):
        w = np.array(q, f32) if d_obs is None else (np.asarray(d_obs, f32) - np.asarray(q, f32)).astype(f32)
        rows, n2 = dot_rows(w, w)
        ws = (w * np.asarray(v2, f32)[nxb:nxb + nx, gz][None, :]).astype(f32)
    return w, ws, rows, n2


def stack_step(d, v2, h, img, mask):
    """Step 5 onto a copy of h."""
    C = cells(d)
    out = np.array(h, f32)
    with np.errstate(all="ignore"):
        t = (np.asarray(img, f32)[C] / np.asarray(v2, f32)[C]).astype(f32)
        if mask is not None:
            t = (np.asarray(mask, f32)[C] * t).astype(f32)
        out[C] = (out[C] + t).astype(f32)
    return out


def update_step(d, m, g, p, h, alpha):
    """(m, g, row sums of <g, g>, <g, g>) after m = m + af p, g = g - af h on C."""
    C = cells(d)
    af = f32(alpha)
    m, g = np.array(m, f32), np.array(g, f32)
    with np.errstate(all="ignore"):
        m[C] = (m[C] + (af * p[C]).astype(f32)).astype(f32)
        g[C] = (g[C] - (af * h[C]).astype(f32)).astype(f32)
    rows, gg = dot_cells(d, g, g)
    return m, g, rows, gg


def direction_step(d, p, g, beta):
    C = cells(d)
    p = np.array(p, f32)
    with np.errstate(all="ignore"):
        p[C] = (g[C] + (f32(beta) * p[C]).astype(f32)).astype(f32)
    return p


def visit(orc, d, v2, p, sx, sz, gz, srce, d_obs=None, mask=None, h=None):
    """V(p, d_obs) of one shot: dict(h: the stack (a copy), n2, w, ws, q, img: the field-shaped DTT image of ws)."""
    v2 = np.ascontiguousarray(v2, f32)
    h = np.zeros((d["nxe"], d["nze"]), f32) if h is None else h
    b = born_restatement(orc, d, v2, p, DTT, sx, sz, gz, srce)
    w, ws, _, n2 = gather_step(d, v2, b["rec"], d_obs, gz)
    img = dtt_back_restatement(orc, d, v2, b["U_P"], b["U_PP"], np.ascontiguousarray(ws[::-1]), gz)["img"]
    return dict(h=stack_step(d, v2, h, img, mask), n2=n2, w=w, ws=ws, q=b["rec"], img=img)


def solve(orc, d, v2s, sxs, sz, gz, srce, d_obs, niter, m0=None, mask=None, verify=False):
    """dict(m, misfit [niter + 1 (+ 1)], resid [shots][nt][nx] with verify, g, p, alphas, betas).  v2s, sxs, d_obs: one entry per shot."""
    shape = (d["nxe"], d["nze"])
    ns = len(sxs)
    m = np.zeros(shape, f32) if m0 is None else np.array(m0, f32)

    def visits(vec, data, stack):
        t, ws = 0.0, []
        for s in range(ns):
            r = visit(orc, d, v2s[s], vec, sxs[s], sz, gz, srce, d_obs[s] if data else None, mask, stack)
            stack = r["h"]
            t = t + r["n2"]
            ws.append(r["w"])
        return stack, t, ws

    g, t, _ = visits(m, True, np.zeros(shape, f32))
    hist = [0.5 * t]
    gamma = dot_cells(d, g, g)[1]
    p = g.copy()
    alphas, betas = [], []
    for k in range(niter):
        h, delta, _ = visits(p, False, np.zeros(shape, f32))
        alpha = 0.0 if delta == 0.0 else gamma / delta
        m, g, _, gg = update_step(d, m, g, p, h, alpha)
        beta = 0.0 if gamma == 0.0 else gg / gamma
        p = direction_step(d, p, g, beta)
        hist.append(hist[k] - 0.5 * (alpha * gamma))
        gamma = gg
        alphas.append(alpha)
        betas.append(beta)
    out = dict(m=m, g=g, p=p, alphas=alphas, betas=betas)
    if verify:
        _, t, ws = visits(m, True, np.zeros(shape, f32))
        hist.append(0.5 * t)
        out["resid"] = np.stack(ws)
    out["misfit"] = np.array(hist, f64)
    return out

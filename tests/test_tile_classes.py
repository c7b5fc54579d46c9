"""GPU: the lean and the full body of the four-step forward pass, each compiled for wave 0 and for the other waves, against the CPU oracle bit
for bit.

The deck is the smallest at which every body occurs in one launch: 180 x 500 at 13-row chunks is 14 chunk rows x 3 strips of columns.  Strip 0
holds the damped columns, strip 2 and the outer chunk rows touch the frame of the grid (full body, with and without damping at work); chunk
rows 4 .. 8 of strip 1 touch nothing (lean body) except around the source, which sits in the middle of them (full body with the injection at
work).  Outputs are pre-filled with sentinels, so a tile that is not run shows.  The kernels that share the tile predicate (modelling dialect,
receiver / fused backward passes) run once each on the same deck."""
import ctypes as C

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from conftest import assert_bit_equal, make_deck, random_fields
from oracle import oracle as O
from parallel_finite_difference_computation_amd import _lib

pytestmark = pytest.mark.gpu

XCHUNK = 13
SX, SZ = 84, 300          # chunk row 6 (rows 78 .. 90), strip 1 (columns 224 .. 447 are its own)
LEAN, FULL = 0, 1


def mk(d, **kw):
    ctx = F.FDWave(d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"], compat=False, **kw)
    ctx.set_tuning(two_step=4, xchunk=XCHUNK)
    assert ctx.steps_per_pass() == 4
    return ctx


def mko(d, **kw):
    return O.Oracle(d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"], compat=False, **kw)


def plan(ctx, forward=1, sx=SX, sz=SZ, r0=0, r1=-1, r0b=0, r1b=0, xchunk=XCHUNK):
    """The classes, as [chunk row][strip], of the tiles fdw_dev_step4 would launch (the host's copy of the kernel's predicate)."""
    nblk, nstrip = C.c_int(), C.c_int()
    cls = (C.c_ubyte * 4096)()
    _lib.check(_lib.lib().fdw_debug_step4_plan(ctx._h, forward, sx, sz, r0, r1, r0b, r1b, xchunk, C.byref(nblk), C.byref(nstrip),
                                               C.cast(cls, C.c_void_p), len(cls)))
    return np.array(cls[:nblk.value], np.uint8).reshape(-1, nstrip.value)


@pytest.fixture(scope="module")
def deck():
    d = make_deck(180, 500, 12, 14, 8, seed=21, compat=False)
    d["sx"], d["sz"] = SX, SZ
    d["srce"] = O.ricker_wavelet(8, d["dt"], 30.0)
    d["p0"], d["pp0"] = random_fields(d, seed=5, amp=0.1)
    d["want"] = {}
    for numerics in (0, 1):
        orc = mko(d, numerics=numerics)
        for nsteps in (4, 8):
            d["want"][numerics, nsteps] = orc.forward(d["v2"], SX, SZ, d["srce"], d["p0"], d["pp0"], nsteps=nsteps)      # (P = u^{n+k-1}, PP = u^{n+k})
    for a in (d["p0"], d["pp0"], d["v2"], d["srce"]) + tuple(x for w in d["want"].values() for x in w):
        a.setflags(write=False)
    return d


def dev_field(ctx, h, torch):
    t = torch.zeros((h.shape[0], ctx.pitch), device="cuda:0")
    t[:, :h.shape[1]] = torch.from_numpy(np.array(h)).to("cuda:0")
    return t


def test_the_deck_holds_every_class(deck):
    ctx = mk(deck)
    cls = plan(ctx)
    assert cls.shape == (14, 3)
    assert (cls[:, 0] == FULL).all(), "strip 0 holds the damped columns"
    assert (cls[:, 2] == FULL).all() and (cls[:4, 1] == FULL).all() and (cls[9:, 1] == FULL).all(), "the frame of the grid"
    assert list(cls[4:9, 1]) == [LEAN, FULL, FULL, FULL, LEAN], "the source at row 84 reaches 16 rows into the chunks on either side"
    cls_p = plan(ctx, forward=0)                                                        # PLAIN: nothing damped, no source
    assert (cls_p[4:9, 1] == LEAN).all() and (cls_p == LEAN).sum() == 5
    one = plan(ctx, r0=52, r1=65)                                                       # one chunk: three tiles for eight XCDs
    assert one.shape == (1, 3) and list(one[0]) == [FULL, LEAN, FULL]


@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
def test_forward_loop_and_single_passes_vs_oracle(deck, numerics):
    """fdw_dev_steps2 for 4 and 8 steps and fdw_dev_step4 on the whole grid, on one chunk and on two row ranges: the oracle's fields (FAST: its
    restatement of the FAST formula) bit for bit inside the rows asked for, the sentinels outside."""
    import torch
    d = deck
    nxe, nze = d["nxe"], d["nze"]
    ctx = mk(d, numerics=numerics)
    srce, v2 = torch.from_numpy(np.array(d["srce"])).to("cuda:0"), dev_field(ctx, d["v2"], torch)
    for nsteps in (4, 8):
        oP, oPP = d["want"][numerics, nsteps]
        bufs = [dev_field(ctx, d["p0"], torch), dev_field(ctx, d["pp0"], torch), torch.full((nxe, ctx.pitch), 7.0, device="cuda:0"),
                torch.full((nxe, ctx.pitch), -7.0, device="cuda:0")]
        for b in bufs[2:]:
            b[:, nze:] = 0
        torch.cuda.synchronize()
        ip, ipp = ctx.dev_steps2([b.data_ptr() for b in bufs], v2.data_ptr(), srce.data_ptr(), SX, SZ, 0, nsteps, first_pp_twice=False, ip=0, ipp=1)
        ctx.dev_taper_finalize(bufs[ip].data_ptr())
        torch.cuda.synchronize()
        assert_bit_equal(bufs[ipp][:, :nze].cpu().numpy(), oPP, f"PP after {nsteps} steps, numerics {numerics}")
        assert_bit_equal(bufs[ip][:, :nze].cpu().numpy(), oP, f"P after {nsteps} steps, numerics {numerics}")
    oP, oPP = d["want"][numerics, 4]
    newest, older = dev_field(ctx, d["pp0"], torch), dev_field(ctx, d["p0"], torch)      # forward()'s convention: the kernel's p is pp0
    for ranges in (dict(r0=0, r1=-1), dict(r0=52, r1=65), dict(r0=16, r1=50, r0b=120, r1b=164), dict(r0=0, r1=33, r0b=150, r1b=180)):
        out1 = torch.full((nxe, ctx.pitch), 7.0, device="cuda:0")
        out2 = torch.full((nxe, ctx.pitch), -7.0, device="cuda:0")
        torch.cuda.synchronize()
        ctx.dev_step4(newest.data_ptr(), older.data_ptr(), v2.data_ptr(), out1.data_ptr(), out2.data_ptr(), pp_twice=False, d_srce_it=srce.data_ptr(),
                      sx=SX, sz=SZ, xchunk=XCHUNK, **ranges)
        ctx.dev_taper_finalize(out1.data_ptr())
        torch.cuda.synchronize()
        rows = np.zeros(nxe, bool)
        if ranges["r1"] < 0:
            rows[:] = True
        else:
            rows[ranges["r0"]:ranges["r1"]] = True
            rows[ranges.get("r0b", 0):ranges.get("r1b", 0)] = True
        h1, h2 = out1[:, :nze].cpu().numpy(), out2[:, :nze].cpu().numpy()
        assert_bit_equal(h2[rows], oPP[rows], f"u^(n+4) on {ranges}, numerics {numerics}")
        assert_bit_equal(h1[rows], oP[rows], f"u^(n+3) on {ranges}, numerics {numerics}")
        assert (h2[~rows] == -7.0).all() and (h1[~rows][:, d["nzb"]:] == 7.0).all(), f"rows outside {ranges} were written"


def test_source_sweep_across_the_class_borders(deck):
    """Four steps with the source on either side of every border between lean, frame and damped tiles: rows 51 | 52 and 116 | 117 (chunk rows
    3 | 4 and 8 | 9), 16 rows further in and out (where the source stops reaching the neighbouring chunk), and the first / last columns the
    strips read (208, 432, 464) and own (224, 448)."""
    d = deck
    ctx, orc = mk(d), mko(d)
    seen = set()
    for sx in (35, 36, 51, 52, 68, 116, 117, 133):
        for sz in (14, 207, 208, 223, 224, 431, 432, 447, 448, 463, 464, 485):
            seen.add(int((plan(ctx, sx=sx, sz=sz) == LEAN).sum()))
            P, PP = ctx.forward(d["v2"], sx, sz, d["srce"][:4], d["p0"], d["pp0"], nsteps=4)
            oP, oPP = orc.forward(d["v2"], sx, sz, d["srce"][:4], d["p0"], d["pp0"], nsteps=4)
            assert_bit_equal(PP, oPP, f"PP source at ({sx},{sz})")
            assert_bit_equal(P, oP, f"P source at ({sx},{sz})")
    assert len(seen) >= 2, seen      # the sweep moved tiles between the classes


def test_modelling_loop_and_shot_share_the_predicate(deck):
    """fdw_dev_model_steps (modelling dialect) and fdw_shot (receiver field / fused backward pass) on the same grid: these kernels pick their
    bodies by the same predicate, with their own template values."""
    import torch
    d = deck
    nxe, nze, nxb, nzb, fac, nsteps = d["nxe"], d["nze"], d["nxb"], d["nzb"], 0.02, 8
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    rng = np.random.default_rng(3)
    srce = (1e-2 * rng.standard_normal(nsteps)).astype(np.float32)
    P0, PP0 = (1e-3 * np.array(d["p0"])).astype(np.float32), (1e-3 * np.array(d["pp0"])).astype(np.float32)
    v2 = np.array(d["v2"])
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nsteps, fac, 10.0, 12.5, 0.001, dialect=1)
    ctx.set_tuning(two_step=4, xchunk=XCHUNK)
    assert ctx.steps_per_pass() == 4
    p, pp, dv2, dsr = dev_field(ctx, P0, torch), dev_field(ctx, PP0, torch), dev_field(ctx, v2, torch), torch.from_numpy(srce).to("cuda:0")
    rec = torch.zeros((nsteps, nx), device="cuda:0")
    torch.cuda.synchronize()
    sx, sz, gz = SX, SZ, SZ - 10
    ctx.dev_model_steps(p.data_ptr(), pp.data_ptr(), dv2.data_ptr(), dsr.data_ptr(), sx, sz, gz, rec.data_ptr(), 0, nsteps)
    torch.cuda.synchronize()
    wP, wPP, wdata = O.mod_steps(8, nx, nz, nxb, nzb, 10.0, 12.5, 0.001, fac, v2, sx, sz, gz, srce,
                                 O.mod_taper_apply(P0, nx, nz, nxb, nzb, fac, 1), O.mod_taper_apply(PP0, nx, nz, nxb, nzb, fac, 2))
    assert_bit_equal(rec.cpu().numpy().T, wdata, "modelling gather")
    assert_bit_equal(O.mod_taper_apply(p[:, :nze].cpu().numpy(), nx, nz, nxb, nzb, fac, 1), wP, "modelling P")
    assert_bit_equal(O.mod_taper_apply(pp[:, :nze].cpu().numpy(), nx, nz, nxb, nzb, fac, 2), wPP, "modelling PP")
    # one shot: forward loop, then the backward loop four iterations per pass
    sctx, orc = mk(d), mko(d)
    d_obs = rng.standard_normal((nx, d["nt"])).astype(np.float32)
    img = sctx.shot(v2, SX, d["nzb"] + 2, d["nzb"] + 1, d["srce"], d_obs)
    oP, oPP = orc.forward(v2, SX, d["nzb"] + 2, d["srce"])
    assert_bit_equal(img, orc.back(v2, oP, oPP, d_obs, d["nzb"] + 1), "image of one shot")
    assert np.abs(img).max() > 0

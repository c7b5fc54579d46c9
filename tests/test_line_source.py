"""Line sources in the RTM forward loop (fdwave.h, "line sources"): fdw_dev_line_steps, fdw_shot_line, fdw_record_shot_line, the encoders
fdw_planewave_lags / fdw_encode_line_source / fdw_encode_gathers, and rtm_code's pw= decks.

The restatement uses existing oracle calls only.  Per iteration: swap (P, PP); Oracle.slab_step(0, P, PP, v2, 0, nxe, -1, 0, 0.0) -- the
whole-grid step without a source --; then PP[nxb:nxb+nsrc, sz] = PP[...] + w[it, :nsrc] in np.float32, nsrc = min(nx, xlim - nxb); then
the trace row PP[nxb:nxb+nx, gz] is read, or u * u is added to the illumination inside the update extents, as tests/test_record.py and
tests/test_illum.py do.  Run with a point source instead of the line the same chain equals Oracle.forward bit for bit (first test)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from conftest import ROOT, assert_bit_equal, make_deck, random_fields
from oracle import oracle as O
from test_record import interface_hits, two_layer_case
from test_stepn_isa_budget import isa  # noqa: F401  (a fixture)
from value_classes import assert_same_nonfinite

BIN = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin")
LEAN, FULL = 0, 1
EINVAL, ESTATE = -1, -5


def args_of(d):
    return (d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"])


def extents_of(d):
    return O.extents(d["nxe"], d["nze"], d["nzb"], d.get("compat", True)) if d.get("compat", True) else (d["nxe"], d["nze"], d["nzb"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def line_restatement(orc, d, v2, w, sz, gz=None, p0=None, pp0=None, il0=None, point=None):
    """dict(P, PP, data[nx][nt], illum) after len(w) iterations of the chain in the module docstring.  w[it][ix]: the line samples (nx per
    iteration, those of rows >= nsrc ignored).  point = (sx, srce): a point source in place of the line (the guard of the chain itself)."""
    nxe, nze, nxb = d["nxe"], d["nze"], d["nxb"]
    nx = nxe - 2 * nxb
    xlim, zlim, _ = extents_of(d)
    nsrc = min(nx, xlim - nxb)
    P = np.zeros((nxe, nze), np.float32) if p0 is None else np.array(p0, np.float32, order="C")
    PP = np.zeros((nxe, nze), np.float32) if pp0 is None else np.array(pp0, np.float32, order="C")
    v2 = np.ascontiguousarray(v2, np.float32)
    nt = len(point[1]) if point else len(w)
    data = np.zeros((nx, nt), np.float32)
    il = np.zeros((nxe, nze), np.float32) if il0 is None else np.array(il0, np.float32)
    with np.errstate(all="ignore"):
        for it in range(nt):
            P, PP = PP, P
            orc.slab_step(0, P, PP, v2, 0, nxe, -1, 0, 0.0)
            if point:
                PP[point[0], sz] = np.float32(PP[point[0], sz] + np.float32(point[1][it]))
            else:
                PP[nxb:nxb + nsrc, sz] = (PP[nxb:nxb + nsrc, sz] + np.asarray(w[it][:nsrc], np.float32)).astype(np.float32)
            if gz is not None:
                data[:, it] = PP[nxb:nxb + nx, gz]
            u = PP[:xlim, :zlim]
            il[:xlim, :zlim] = (il[:xlim, :zlim] + (u * u).astype(np.float32)).astype(np.float32)
    return dict(P=P, PP=PP, data=data, illum=il)


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("grid", [(87, 70, 12, 10), (87, 70, 3, 10)], ids=["87x70", "ragged"])
def test_restatement_with_a_point_source_is_the_oracle_forward(grid, numerics):
    nt = 11
    d = make_deck(*grid, nt, seed=4)
    p0, pp0 = random_fields(d, 6, amp=0.1)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0 + np.float32(3.0)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    for a, b in ((None, None), (p0, pp0)):
        got = line_restatement(orc, d, d["v2"], None, d["sz"], p0=a, pp0=b, point=(d["sx"], srce))
        oP, oPP = orc.forward(d["v2"], d["sx"], d["sz"], srce, a, b)
        assert_bit_equal(got["PP"], oPP, "PP of the chain")
        assert_bit_equal(got["P"], oP, "P of the chain")
        assert np.count_nonzero(oPP) > 100


def lags_formula(src_ix, dx, dt, p):
    src_ix = np.asarray(src_ix, np.int64)
    l = np.array([int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)                        # lround: halves away from zero
                  for v in (float(p) * (src_ix - src_ix[0]).astype(np.float64) * float(np.float32(dx)) / float(np.float32(dt)))], np.int64)
    return (l - l.min()).astype(np.int32)


def line_source_formula(src_ix, lag, weight, srce, nx):
    nt = len(srce)
    wav = np.zeros((nx, nt), np.float32)
    for s in range(len(src_ix)):
        for it in range(int(lag[s]), nt):
            prod = np.float32(np.float32(weight[s]) * np.float32(srce[it - lag[s]]))
            wav[src_ix[s], it] = np.float32(wav[src_ix[s], it] + prod)
    return wav


def gathers_formula(lag, weight, d_obs_all):
    ns, nx, nt = d_obs_all.shape
    out = np.zeros((nx, nt), np.float32)
    with np.errstate(all="ignore"):
        for s in range(ns):
            L = int(lag[s])
            if L < nt:
                prod = (np.float32(weight[s]) * d_obs_all[s][:, :nt - L]).astype(np.float32)
                out[:, L:] = (out[:, L:] + prod).astype(np.float32)
    return out


@pytest.mark.parametrize("p", [0.0, 2.5e-4, -2.5e-4, -1.3e-3, 7.77e-5])
def test_planewave_lags_match_the_formula(p):
    for src_ix in ([5, 10, 15, 20, 60], [40, 7, 7, 90, 0], [3]):
        got = F.planewave_lags(src_ix, 10.0, 0.001, p)
        assert_bit_equal(got.view(np.float32), lags_formula(src_ix, 10.0, 0.001, p).view(np.float32), f"lags p={p} {src_ix}")
        assert got.min() == 0
    if p < 0:
        assert F.planewave_lags([0, 10], 10.0, 0.001, p)[0] > 0          # negative p: the first shot fires last


def test_encode_line_source_matches_the_formula_and_refuses():
    nt, nx = 37, 29
    rng = np.random.default_rng(2)
    srce = rng.standard_normal(nt).astype(np.float32)
    src_ix = np.array([3, 11, 11, 28, 0, 17], np.int32)                   # two shots on one row
    lag = np.array([0, 5, 2, nt - 1, nt, 3 * nt], np.int32)              # lags >= nt contribute nothing
    weight = np.array([1.0, -1.0, 1.0, -1.0, 1.0, 0.3721], np.float32)
    want = line_source_formula(src_ix, lag, weight, srce, nx)
    got = F.encode_line_source(src_ix, lag, weight, srce, nx)
    assert_bit_equal(got, want, "encoded source gather")
    assert np.count_nonzero(got[11]) > nt - 6 and not got[0].any() and not got[17].any() and np.count_nonzero(got[28]) == 1
    one = F.encode_line_source(src_ix[5:], [4], weight[5:], srce, nx)
    assert_bit_equal(one[17, 4:], (np.float32(0.3721) * srce[:nt - 4]).astype(np.float32), "a non-trivial weight")
    for bad_ix, bad_lag in (([3, nx], [0, 0]), ([-1, 3], [0, 0]), ([3, 4], [0, -1])):
        with pytest.raises(F.FdwError) as e:
            F.encode_line_source(bad_ix, bad_lag, [1.0, 1.0], srce, nx)
        assert e.value.code == EINVAL
    with pytest.raises(F.FdwError):
        F.planewave_lags([1, 2], 10.0, 0.0, 1e-4)
    with pytest.raises(F.FdwError):
        F.planewave_lags([1, 2], 10.0, 0.001, float("nan"))


def test_line_source_superposes_point_sources():
    """On the restatement alone: the gather of a line source built from shifted, weighted point sources agrees with the float64 sum of the
    shifted, weighted point-source gathers of the oracle to 1e-5 of the largest sample (the project's fp32 tolerance; the propagator is linear)."""
    nxe, nze, nb, nt = 81, 65, 10, 40
    d = make_deck(nxe, nze, nb, nb, nt, seed=1, order=8)
    nx = nxe - 2 * nb
    srce = O.ricker_wavelet(nt, 0.001, 30.0)
    orc = O.Oracle(*args_of(d), compat=True)
    sz, gz = nb + 2, nb + 1
    src_ix = np.arange(0, nx, 5, dtype=np.int32)
    lag = (2 * np.arange(src_ix.size)).astype(np.int32)
    weight = np.where(np.arange(src_ix.size) % 2 == 0, 1.0, -1.0).astype(np.float32)
    wav = F.encode_line_source(src_ix, lag, weight, srce, nx)
    got = line_restatement(orc, d, d["v2"], wav.T, sz, gz=gz)["data"]
    want = np.zeros((nx, nt), np.float64)
    for s in range(src_ix.size):
        g = line_restatement(orc, d, d["v2"], None, sz, gz=gz, point=(nb + int(src_ix[s]), srce))["data"].astype(np.float64)
        want[:, lag[s]:] += float(weight[s]) * g[:, :nt - lag[s]]
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"superposition: max-norm-relative error {err:.3g}")
    assert np.abs(want).max() > 0 and err <= 1e-5


LINE_KERNELS = ("fdw_step_line_kernel", "fdw_step2_line_kernel", "fdw_stepn_line_kernel")


def test_line_kernels_exist_in_both_numerics_without_spills(isa):      # noqa: F811
    names = [k for k in isa if "_line_kernel" in k]
    for k in names:
        meta = isa[k][0]
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (k, meta)
    for num in (0, 1):
        for rec, ill in ((0, 0), (1, 0), (0, 1)):
            for base in LINE_KERNELS[1:]:
                assert any(f"{base}ILb{rec}ELb{ill}ELi{num}EEEv" in k for k in names), (base, num, rec, ill)
            for h in (1, 2, 3, 4):
                assert any(f"fdw_step_line_kernelILi{h}ELi2ELb{rec}ELb{ill}ELi{num}EEEv" in k for k in names), (h, num, rec, ill)
            if num == 0:
                for pf in (1, 3):
                    assert any(f"fdw_step_line_kernelILi4ELi{pf}ELb{rec}ELb{ill}ELi0EEEv" in k for k in names), (pf, rec, ill)
    assert not any("ELb1ELb1ELi" in k for k in names), "recording and illumination together are not built"
    assert any("fdw_encode_gathers_kernel" in k for k in isa)


def test_every_line_source_symbol_is_exported():
    L = F.lib()
    for name in ("fdw_dev_line_steps", "fdw_shot_line", "fdw_record_shot_line", "fdw_debug_step4_plan_line", "fdw_planewave_lags",
                 "fdw_encode_line_source", "fdw_encode_gathers"):
        assert hasattr(L, name)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_dev_line_steps
# ---------------------------------------------------------------------------------------------------------------------------------------
class Device:
    """Entry state of one forward run on the device: four field buffers (p, pp, two spares holding sentinels), v2, the line-source gather
    [nt][nx], a trace store and an accumulator pre-filled with what the caller hands over."""

    def __init__(self, ctx, d, p0, pp0, w, il0=None, nt_rec=None):
        import torch
        self.torch, self.ctx, self.nze = torch, ctx, d["nze"]
        dev = torch.device("cuda:0")
        nxe, nze = d["nxe"], d["nze"]
        self.bufs = [torch.zeros((nxe, ctx.pitch), device=dev) for _ in range(4)]
        self.bufs[0][:, :nze] = torch.from_numpy(np.array(p0)).to(dev)
        self.bufs[1][:, :nze] = torch.from_numpy(np.array(pp0)).to(dev)
        self.bufs[2][:, :nze] = 7.0
        self.bufs[3][:, :nze] = -7.0
        self.v2 = torch.zeros((nxe, ctx.pitch), device=dev)
        self.v2[:, :nze] = torch.from_numpy(np.array(d["v2"])).to(dev)
        self.il = torch.zeros((nxe, ctx.pitch), device=dev)
        if il0 is not None:
            self.il[:, :nze] = torch.from_numpy(np.array(il0)).to(dev)
        self.w = torch.from_numpy(np.array(w, np.float32, order="C")).to(dev)
        self.rec = torch.full((len(w) if nt_rec is None else nt_rec, nxe - 2 * d["nxb"]), 9.0, device=dev)
        torch.cuda.synchronize()

    def run(self, variant, sz, gz, nsteps, it0=0, first=False, ip=0, ipp=1):
        out = self.ctx.dev_line_steps([b.data_ptr() for b in self.bufs], self.v2.data_ptr(), self.w.data_ptr(), sz, it0, nsteps, gz=gz,
                                      d_rec=self.rec.data_ptr() if variant == "rec" else None,
                                      d_illum=self.il.data_ptr() if variant == "ill" else None, first_pp_twice=first, ip=ip, ipp=ipp)
        self.torch.cuda.synchronize()
        return out

    def field(self, i, finalize=False):
        if finalize:
            self.ctx.dev_taper_finalize(self.bufs[i].data_ptr())
            self.torch.cuda.synchronize()
        return self.bufs[i][:, :self.nze].cpu().numpy()

    def illum(self):
        assert not self.il[:, self.nze:].any()
        return self.il[:, :self.nze].cpu().numpy()

    def traces(self):
        return self.rec.cpu().numpy()


def check_run(dv, variant, want, ip, ipp, nsteps, il0, what, same=assert_bit_equal):
    """PP, P (after the damping the lazy scheme still owes it), and the variant's own output against the restatement; the other outputs untouched."""
    same(dv.field(ipp), want["PP"], "PP, " + what)
    same(dv.field(ip, finalize=True), want["P"], "P, " + what)
    if variant == "rec":
        same(dv.traces()[:nsteps], want["data"].T[:nsteps], "trace rows, " + what)
        assert (dv.traces()[nsteps:] == 9.0).all(), what
    else:
        assert (dv.traces() == 9.0).all(), "no trace row is written, " + what
    same(dv.illum(), want["illum"] if variant == "ill" else il0, "illumination, " + what)


NXE, NZE, NXB, NZB = 87, 70, 12, 10                      # compat: xlim 80, zlim 64, ztap 8; nx 63, every interior row time-stepped
NT = 11                                                  # two_step=4: passes of 4 + 4 + 2 + 1 steps; two_step=1: 5 pairs + 1
FAMILIES = [  # (order, tuning, numerics it applies to)
    (2, {}, (0, 1)), (4, {}, (0, 1)), (6, {}, (0, 1)), (10, {}, (0, 1)), (8, dict(use_generic=True, two_step=-1), (0, 1)),
    (8, dict(two_step=-1), (0, 1)), (8, dict(two_step=-1, prefetch=1), (0,)), (8, dict(two_step=-1, prefetch=3), (0,)),
    (8, dict(two_step=1), (0, 1)), (8, dict(two_step=4), (0, 1)),
]
FAMILY_CASES = [(o, t, n) for o, t, nums in FAMILIES for n in nums]


@functools.lru_cache(maxsize=None)
def small_case(order, numerics, grid=(NXE, NZE, NXB, NZB)):
    """Deck, entry fields, line samples and the restatement's answers for both depths (outside and inside the damped strip), shared by the
    tuning variants of one order; never modified."""
    d = make_deck(*grid, NT, seed=3, order=order, dx=10.0, dz=12.5)
    nx = d["nxe"] - 2 * d["nxb"]
    rng = np.random.default_rng(11)
    p0, pp0 = random_fields(d, 5, amp=0.1)
    il0 = (0.5 + rng.random((d["nxe"], d["nze"]))).astype(np.float32)
    w = rng.standard_normal((NT, nx)).astype(np.float32)
    xlim = extents_of(d)[0]
    w[:, max(0, xlim - d["nxb"]):] = 1e30                 # rows the loop never time-steps: their samples must have no effect
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    want = {sz: line_restatement(orc, d, d["v2"], w, sz, gz=sz, p0=p0, pp0=pp0, il0=il0) for sz in (d["nzb"] + 3, 5)}
    for a in (p0, pp0, il0, w, d["v2"]) + tuple(x for r in want.values() for x in r.values()):
        a.setflags(write=False)
    return d, p0, pp0, il0, w, want


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "rec", "ill"])
@pytest.mark.parametrize("order,tuning,numerics", FAMILY_CASES)
def test_dev_line_steps_vs_restatement(order, tuning, numerics, variant):
    """Noise-filled entry fields, a noise line at a depth outside and one inside the damped strip, the receivers ON the line (gz == sz: the
    recorded sample includes the line sample): every output equals the restatement bit for bit."""
    d, p0, pp0, il0, w, want = small_case(order, numerics)
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    if "two_step" in tuning:
        assert ctx.steps_per_pass() == {-1: 1, 1: 2, 4: 4}[tuning["two_step"]]
    for sz in want:
        what = f"order {order} {tuning} numerics {numerics} {variant} sz {sz}"
        dv = Device(ctx, d, p0, pp0, w, il0)
        ip, ipp = dv.run(variant, sz, sz, NT)
        check_run(dv, variant, want[sz], ip, ipp, NT, il0, what)
        assert np.count_nonzero(want[sz]["data"]) > 0.9 * want[sz]["data"].size


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "rec", "ill"])
@pytest.mark.parametrize("order,tuning", [(8, dict(two_step=-1)), (8, dict(two_step=1)), (8, dict(two_step=4)), (4, {}), (10, {})])
def test_ragged_grid_line_ends_before_the_static_rows(order, tuning, variant):
    """nxe = 87, nxb = 3: xlim = 80, so nsrc = 77 of nx = 81.  The samples of rows >= nsrc (1e30 here) have no effect, and the trace rows of
    the static receiver rows are what fdw_dev_record_steps defines (the entry fields' values, alternating)."""
    d, p0, pp0, il0, w, want = small_case(order, 0, (87, 70, 3, 10))
    assert extents_of(d)[0] == 80 and (w[:, 77:] == 1e30).all() and w.shape[1] == 81
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(**tuning)
    sz = d["nzb"] + 3
    dv = Device(ctx, d, p0, pp0, w, il0)
    ip, ipp = dv.run(variant, sz, sz, NT)
    check_run(dv, variant, want[sz], ip, ipp, NT, il0, f"ragged order {order} {tuning} {variant}")
    assert np.abs(want[sz]["PP"]).max() < 1e3
    assert_bit_equal(want[sz]["data"][77:, 0], p0[80:84, sz], "static rows: after the first swap d_pp holds the entry d_p there")
    assert_bit_equal(want[sz]["data"][77:, 1], pp0[80:84, sz], "static rows: ... and the entry d_pp after the second")


@pytest.mark.gpu
def test_dev_line_steps_continues_a_loop_and_refuses():
    """it0 > 0 with first_pp_twice: 5 + 6 steps equal 11; the refusals of fdwave.h."""
    d, p0, pp0, il0, w, want = small_case(8, 0)
    sz = d["nzb"] + 3
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(two_step=4)
    for variant in ("rec", "ill"):
        dv = Device(ctx, d, p0, pp0, w, il0)
        ip, ipp = dv.run(variant, sz, sz, 5)
        ip, ipp = dv.run(variant, sz, sz, NT - 5, it0=5, first=True, ip=ip, ipp=ipp)
        same = dv.traces() if variant == "rec" else dv.illum()
        assert_bit_equal(same, want[sz]["data"].T if variant == "rec" else want[sz]["illum"], f"5 + 6 steps, {variant}")
        assert_bit_equal(dv.field(ipp), want[sz]["PP"], "PP after 5 + 6 steps")
    dv = Device(ctx, d, p0, pp0, w, il0)
    ptrs = [b.data_ptr() for b in dv.bufs]
    zlim = extents_of(d)[1]

    def code(c, **kw):
        a = dict(sz=sz, it0=0, nsteps=4, gz=sz, d_rec=None, d_illum=None)
        a.update(kw)
        with pytest.raises(F.FdwError) as e:
            c.dev_line_steps(ptrs, dv.v2.data_ptr(), a.pop("d_wav", dv.w.data_ptr()), a.pop("sz"), a.pop("it0"), a.pop("nsteps"), **a)
        return e.value.code
    assert code(ctx, sz=zlim) == EINVAL and code(ctx, sz=-1) == EINVAL and code(ctx, d_wav=None) == EINVAL and code(ctx, it0=-1) == EINVAL
    assert code(ctx, d_rec=dv.rec.data_ptr(), d_illum=dv.il.data_ptr()) == EINVAL              # both together are not built
    assert code(ctx, d_rec=dv.rec.data_ptr(), gz=zlim) == EINVAL
    slab = F.FDWave(*args_of(d), compat=True, device=0, slab=(0, 40))
    mod = F.FDWave(*args_of(d), compat=True, device=0, dialect=1)
    stored = F.FDWave(*args_of(d), compat=True, device=0, dialect=2)
    for other in (slab, mod, stored):
        assert code(other) == ESTATE
    dv.torch.cuda.synchronize()
    assert_bit_equal(dv.field(0), p0, "a refused call enqueues nothing")
    assert_bit_equal(dv.field(1), pp0, "a refused call enqueues nothing")
    assert ctx.dev_line_steps(ptrs, dv.v2.data_ptr(), dv.w.data_ptr(), zlim - 1, 0, 1) == (1, 0)      # the deepest column is accepted


# ---- the pipeline deck of tests/test_tile_classes.py: lean and full tiles in one launch ----
XCHUNK = 13


@functools.lru_cache(maxsize=None)
def pipe_case(numerics):
    d = make_deck(180, 500, 12, 14, 8, seed=21, compat=False)
    nx = d["nxe"] - 2 * d["nxb"]
    rng = np.random.default_rng(7)
    p0, pp0 = random_fields(d, seed=5, amp=0.1)
    il0 = (0.5 + rng.random((d["nxe"], d["nze"]))).astype(np.float32)
    w = rng.standard_normal((8, nx)).astype(np.float32)
    orc = O.Oracle(*args_of(d), compat=False, numerics=numerics)
    want = {sz: line_restatement(orc, d, d["v2"], w, sz, gz=310, p0=p0, pp0=pp0, il0=il0) for sz in (16, 300)}
    for a in (p0, pp0, il0, w, d["v2"]) + tuple(x for r in want.values() for x in r.values()):
        a.setflags(write=False)
    return d, p0, pp0, il0, w, want


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("variant", ["plain", "rec", "ill"])
def test_pipeline_deck_lean_and_full_tiles(variant, numerics):
    """180 x 500 at 13-row chunks: 14 chunk rows x 3 strips.  Line at depth 16 (strip 0): the lean tiles of strip 1 survive; at depth 300
    (strip 1): every tile of strip 1 runs the full body with the injection at work.  8 steps from noise fields."""
    d, p0, pp0, il0, w, want = pipe_case(numerics)
    ctx = F.FDWave(*args_of(d), compat=False, device=0, numerics=numerics)
    ctx.set_tuning(two_step=4, xchunk=XCHUNK)
    assert ctx.steps_per_pass() == 4
    for sz in (16, 300):
        nblk, nstrip, cls = ctx.debug_step4_plan_line(sz, xchunk=XCHUNK)
        cls = cls.reshape(-1, nstrip)
        assert cls.shape == (14, 3) and (cls[:, 0] == FULL).all() and (cls[:, 2] == FULL).all()
        if sz == 16:
            assert list(cls[:, 1]) == [FULL] * 4 + [LEAN] * 5 + [FULL] * 5, "the line in strip 0 leaves strip 1's lean tiles lean"
        else:
            assert (cls == FULL).all(), "the line crosses every tile of strip 1"
        dv = Device(ctx, d, p0, pp0, w, il0)
        ip, ipp = dv.run(variant, sz, 310, 8)
        check_run(dv, variant, want[sz], ip, ipp, 8, il0, f"pipeline deck {variant} numerics {numerics} sz {sz}")


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", [dict(two_step=-1), dict(two_step=1), dict(two_step=4), dict(use_generic=True, two_step=-1)], ids=str)
def test_line_samples_at_the_edges_of_the_value_domain(tuning):
    """-0.0, subnormals and one infinity among the line samples: NaN positions equal, every other cell bit for bit."""
    d, p0, pp0, il0, w, _ = small_case(8, 0)
    w = np.array(w)
    w[:, 3] = -0.0
    w[:, 10:20] = np.float32(1e-41)
    w[:, 20:24] = np.float32(-3e-45)
    w[2, 40] = np.inf
    sz = d["nzb"] + 3
    orc = O.Oracle(*args_of(d), compat=True)
    zero = np.zeros_like(p0)
    for a, b in ((p0, pp0), (zero, zero)):                                  # from noise, and from rest (where -0.0 and the subnormals show)
        want = line_restatement(orc, d, d["v2"], w, sz, gz=sz, p0=a, pp0=b, il0=il0)
        assert np.isnan(want["PP"]).any() and np.isinf(want["data"]).any()
        ctx = F.FDWave(*args_of(d), compat=True, device=0)
        ctx.set_tuning(**tuning)
        for variant in ("rec", "ill"):
            dv = Device(ctx, d, a, b, w, il0)
            ip, ipp = dv.run(variant, sz, sz, NT)
            check_run(dv, variant, want, ip, ipp, NT, il0, f"value domain {tuning} {variant}", same=assert_same_nonfinite)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: whole shots
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shot_case(numerics=0):
    nxe, nze, nxb, nzb, nt = 70, 53, 9, 8, 60
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=8)
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    rng = np.random.default_rng(4)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 100.0
    src_ix = np.arange(2, nx, 7, dtype=np.int32)
    lag = F.planewave_lags(src_ix, 10.0, 0.001, 3e-4)
    wav = F.encode_line_source(src_ix, lag, np.ones(src_ix.size, np.float32), srce, nx)
    d_obs = rng.standard_normal((nx, nt)).astype(np.float32)
    sz, gz = nzb + 2, nzb + 1
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    want = line_restatement(orc, d, d["v2"], wav.T, sz, gz=gz)
    want["image"] = orc.back(d["v2"], want["P"], want["PP"], d_obs, gz)
    for a in (srce, wav, d_obs, d["v2"]) + tuple(want.values()):
        a.setflags(write=False)
    return d, nx, nz, srce, wav, d_obs, sz, gz, want


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("tuning", [dict(two_step=-1), dict(two_step=1), dict(two_step=4)], ids=str)
def test_shot_line_and_record_shot_line(tuning, numerics):
    d, nx, nz, srce, wav, d_obs, sz, gz, want = shot_case(numerics)
    nxb, nzb = d["nxb"], d["nzb"]
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    img, P, PP, il = ctx.shot_line(d["v2"], sz, gz, wav, d_obs, want_fields=True, want_illum=True)
    assert_bit_equal(PP, want["PP"], "PP")
    assert_bit_equal(P, want["P"], "P")
    assert_bit_equal(il, want["illum"][nxb:nxb + nx, nzb:nzb + nz], "illumination")
    assert_bit_equal(img, want["image"], "image vs Oracle.back fed with the restatement's (P, PP)")
    assert np.abs(img).max() > 0 and il.max() > 0
    assert_bit_equal(ctx.shot_line(d["v2"], sz, gz, wav, d_obs), img, "image without illumination")
    data, rP, rPP = ctx.record_shot_line(d["v2"], sz, gz, wav, want_fields=True)
    assert_bit_equal(data, want["data"], "gather")
    assert_bit_equal(rPP, want["PP"], "PP of the recording run")
    assert_bit_equal(rP, want["P"], "P of the recording run")
    assert np.count_nonzero(data) > 0.5 * data.size
    with pytest.raises(F.FdwError) as e:
        ctx.shot_line(d["v2"], extents_of(d)[1], gz, wav, d_obs)
    assert e.value.code == EINVAL


@pytest.mark.gpu
def test_shot_line_on_the_resident_model():
    nxe, nze, nxb, nzb, nt = 91, 77, 12, 10, 29
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    rng = np.random.default_rng(3)
    vp = (1500 + 1000 * rng.random((nx, nz))).astype(np.float32)
    wav = rng.standard_normal((nx, nt)).astype(np.float32)
    d_obs = rng.standard_normal((nx, nt)).astype(np.float32)
    sz, gz = nzb + 2, nzb + 1
    ctx.model_resident(vp)
    with pytest.raises(F.FdwError) as e:
        ctx.shot_line(None, sz, gz, wav, d_obs)                       # no squared model drawn yet
    assert e.value.code == ESTATE
    vel = ctx.dev_extendvel_linear(ctx.border_draws(), want_vel=True)
    got = ctx.shot_line(None, sz, gz, wav, d_obs, want_fields=True, want_illum=True)
    data = ctx.record_shot_line(None, sz, gz, wav)
    fresh = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    v2 = (vel * vel).astype(np.float32)
    for name, a, b in zip(("image", "P", "PP", "illum"), got, fresh.shot_line(v2, sz, gz, wav, d_obs, want_fields=True, want_illum=True)):
        assert_bit_equal(a, b, name + ": resident model vs the same model handed over")
    assert_bit_equal(data, fresh.record_shot_line(v2, sz, gz, wav), "gather: resident model vs the same model handed over")
    assert np.abs(got[0]).max() > 0


@pytest.mark.gpu
def test_one_context_through_point_and_line_shots():
    """shot -> shot_line -> record_shot -> shot_line with other samples, on one context: each answer equals a fresh context's."""
    d, nx, nz, srce, wav, d_obs, sz, gz, want = shot_case(0)
    sx = d["nxb"] + 20
    wav2 = np.array(wav[::-1] * np.float32(0.5))
    calls = [lambda c: c.shot(d["v2"], sx, sz, gz, srce, d_obs, want_fields=True),
             lambda c: c.shot_line(d["v2"], sz, gz, wav, d_obs, want_fields=True, want_illum=True),
             lambda c: (c.record_shot(d["v2"], sx, sz, gz, srce),),
             lambda c: c.shot_line(d["v2"], sz, gz, wav2, d_obs, want_fields=True)]
    for tuning in (dict(two_step=-1), dict(two_step=4)):
        one = F.FDWave(*args_of(d), compat=True, device=0)
        one.set_tuning(**tuning)
        for i, call in enumerate(calls):
            fresh = F.FDWave(*args_of(d), compat=True, device=0)
            fresh.set_tuning(**tuning)
            for j, (a, b) in enumerate(zip(call(one), call(fresh))):
                assert_bit_equal(a, b, f"call {i}, output {j}, {tuning}")
            fresh.close()
    assert_bit_equal(one.shot_line(d["v2"], sz, gz, wav, d_obs), want["image"], "and the restatement's image")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the encoded data gather
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nt", [63, 257])
@pytest.mark.parametrize("nshots", [1, 7])
def test_encode_gathers_matches_the_fold(nshots, nt):
    nx = 37
    rng = np.random.default_rng(nshots * 1000 + nt)
    d_obs_all = rng.standard_normal((nshots, nx, nt)).astype(np.float32)
    d_obs_all[0, 3, 5] = -0.0
    lag = np.array([0, nt - 1, nt, 3, 3, 2 * nt + 1, 17][:nshots], np.int32)
    weight = np.array([1.0, -1.0, 1.0, 0.3721, -1.0, 1.0, 1.0][:nshots], np.float32)
    want = gathers_formula(lag, weight, d_obs_all)
    got = F.encode_gathers(lag, weight, d_obs_all)
    assert_bit_equal(got, want, f"encoded gather, {nshots} shots, nt {nt}")
    assert np.count_nonzero(got) > 0.9 * got.size
    if nshots == 1:
        assert_bit_equal(got, d_obs_all[0] + np.float32(0.0), "weight 1, lag 0: the gather itself (+0.0f start)")
    with pytest.raises(F.FdwError) as e:
        F.encode_gathers(-lag - 1, weight, d_obs_all)
    assert e.value.code == EINVAL


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the image shows the model that made the data
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plane_wave_migration_images_the_interface():
    """Three plane waves over the two-layer case of tests/test_record.py, per-row lags 0, ix // 4 and 2 (nx - 1 - ix) // 4: the reflection data
    of each (layered minus homogeneous record) migrated with the same line source puts the image Laplacian's maximum on the interface."""
    args, nx, nz, nb, iface, v2, h2, _ = two_layer_case()
    nt = args[5]
    ctx = F.FDWave(*args, compat=True, device=0)
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    sz = gz = nb + 2
    ix = np.arange(nx, dtype=np.int32)
    for name, lag in (("flat", 0 * ix), ("dipping right", ix // 4), ("dipping left", 2 * (nx - 1 - ix) // 4)):
        wav = F.encode_line_source(ix, lag, np.ones(nx, np.float32), srce, nx)
        refl = ctx.record_shot_line(v2, sz, gz, wav) - ctx.record_shot_line(h2, sz, gz, wav)
        img = ctx.shot_line(h2, sz, gz, wav, refl)
        hits = interface_hits(F.image_laplacian(img, 10.0, 10.0), nz, nb, iface)
        print(f"plane wave {name}: interface hits {hits:.3f}")
        assert hits >= 0.9, (name, hits)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the program: rtm_code's pw= decks
# ---------------------------------------------------------------------------------------------------------------------------------------
PW_PMAX = 2.0e-4                                         # s/m: 40 time steps between neighbouring shot rows of the deck below


def _pw_deck(tmp_path, extra, with_vel_ext=False):
    """A small rtm_code job on disk, as tests/test_programs.py builds its own; returns its arrays."""
    nx, nz, nxb, nzb, nt, ns = 61, 47, 17, 13, 90, 3
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    rng = np.random.default_rng(11)
    vp = (1500 + 2500 * np.linspace(0, 1, nz, dtype=np.float32)[None, :] + 100 * rng.standard_normal((nx, nz))).astype(np.float32)
    d_obs = rng.standard_normal((ns, nx, nt)).astype(np.float32)
    (tmp_path / "models").mkdir()
    (tmp_path / "output").mkdir()
    vp.tofile(tmp_path / "models" / "vp.bin")
    d_obs.tofile(tmp_path / "models" / "dobs.bin")
    deck = ("tmpdir=./output\nvpfile=./models/vp.bin\ndatfile=./models/dobs.bin\n"
            f"nz={nz}\nnx={nx}\nnt={nt}\ndz=10\ndx=10\ndt=0.001\nfpeak=25.\nns={ns}\nsz=1\nfsx=5\nds=20\ngz=2\n"
            f"nxb={nxb}\nnzb={nzb}\nrnd=1\nfac=0.75\norder=8\n")
    vel_ext = None
    if with_vel_ext:
        vel_ext = (1500 + 2000 * rng.random((ns, nxe, nze))).astype(np.float32)
        vel_ext.tofile(tmp_path / "models" / "velext.bin")
        deck = deck.replace("vpfile=", "vel_ext_file=./models/velext.bin\nvpfile=")
    (tmp_path / "input.dat").write_text(deck + extra)
    return nx, nz, nxb, nzb, nt, ns, vp, d_obs, vel_ext


def _run_rtm_code(tmp_path, env=None):
    base = {k: v for k, v in os.environ.items() if k not in ("FDW_SLABS", "FDW_GPUS")}
    return subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=dict(base, **(env or {})))


@pytest.mark.parametrize("extra,words", [
    ("pw=3\npw_pmax=2e-4\nslabs=2\n", ("pw", "slabs")), ("pw=3\npw_pmax=2e-4\ngpus=2\n", ("pw", "gpus")),
    ("pw=3\npw_pmax=2e-4\nresid=1\n", ("pw", "resid")), ("pw=3\npw_pmax=2e-4\nsnap=10\n", ("pw", "snap")),
    ("pw=0\n", ("pw",)), ("pw=3\n", ("pw", "pw_pmax")), ("pw=3\npw_pmax=0\n", ("pw", "pw_pmax")), ("pw=2\npw_pmax=-1e-4\n", ("pw_pmax",)),
])
def test_rtm_code_refuses_pw_key_combinations(tmp_path, extra, words):
    """Before any file, thread, communicator or device is touched: runs where no GPU is."""
    _pw_deck(tmp_path, extra)
    r = _run_rtm_code(tmp_path)
    assert r.returncode != 0
    for w in words:
        assert w in r.stderr, r.stderr
    assert os.listdir(tmp_path / "output") == [] and not os.path.exists(tmp_path / "image.num")


def test_rtm_code_refuses_pw_with_the_environments_slabs_and_gpus(tmp_path):
    _pw_deck(tmp_path, "pw=1\n")
    for env, word in (({"FDW_SLABS": "2"}, "slabs"), ({"FDW_GPUS": "2"}, "gpus")):
        r = _run_rtm_code(tmp_path, env)
        assert r.returncode != 0 and "pw" in r.stderr and word in r.stderr, r.stderr
    assert os.listdir(tmp_path / "output") == []


def test_python_driver_refuses_a_pw_deck(tmp_path):
    from parallel_finite_difference_computation_amd import rtm
    _pw_deck(tmp_path, "pw=3\npw_pmax=2e-4\n")
    with pytest.raises(ValueError, match="pw"):
        rtm.read_deck(str(tmp_path / "input.dat"))


def pw_composition(nx, nz, nxb, nzb, nt, ns, vp, d_obs, vel_ext, npw):
    """(dir.image, dir.illum) of a pw= deck of _pw_deck through the Python API, one plane wave after the other, stacked in the order j."""
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    with_vel_ext = vel_ext is not None
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    srce = F.ricker_wavelet(nt, 0.001, 25.0)
    src_ix = 5 + 20 * np.arange(ns)
    P = float(np.float32(PW_PMAX))
    img, ill = np.zeros((nx, nz), np.float32), np.zeros((nx, nz), np.float32)
    if not with_vel_ext:
        ctx.model_resident(vp)
    seen = set()
    for j in range(npw):
        p = -P + 2.0 * P * j / (npw - 1)
        lag = F.planewave_lags(src_ix, 10.0, 0.001, p)
        seen.add(tuple(lag))
        wav = F.encode_line_source(src_ix, lag, np.ones(ns, np.float32), srce, nx)
        enc = F.encode_gathers(lag, np.ones(ns, np.float32), d_obs)
        if with_vel_ext:
            v2 = (vel_ext[j % ns] * vel_ext[j % ns]).astype(np.float32)
        else:
            ctx.dev_extendvel_linear(j * ctx.border_draws())
            v2 = None
        im, il = ctx.shot_line(v2, 1 + nzb, 2 + nzb, wav, enc, want_illum=True)
        img, ill = img + im, ill + il
    assert len(seen) >= 3 and np.abs(img).max() > 0
    ctx.close()
    return img, ill


@pytest.mark.gpu
@pytest.mark.parametrize("with_vel_ext,npw", [(False, 3), (True, 4)], ids=["border-stream-pw3", "vel-ext-pw4"])
def test_rtm_code_plane_waves_equal_the_python_composition(tmp_path, with_vel_ext, npw):
    """dir.image (and, with illum=1, dir.illum / dir.image_illum) of a pw= deck against the same composition through the Python API: lags,
    source gather, data gather, the model of plane wave j (the next draw of the border stream / vel_ext model j mod ns), shot_line, stacked
    in the order j."""
    nx, nz, nxb, nzb, nt, ns, vp, d_obs, vel_ext = _pw_deck(tmp_path, f"pw={npw}\npw_pmax={PW_PMAX}\n", with_vel_ext)
    img, ill = pw_composition(nx, nz, nxb, nzb, nt, ns, vp, d_obs, vel_ext, npw)
    r = _run_rtm_code(tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert f"** plane wave {npw}" in r.stdout and "> Exec time" in r.stdout
    assert_bit_equal(np.fromfile(tmp_path / "output" / "dir.image", np.float32).reshape(nx, nz), img, "dir.image")
    lines = (tmp_path / "image.num").read_text().splitlines()
    assert len(lines) == npw * (1 + nx * nz) and lines[0] == "======== 0 ========" and lines[(npw - 1) * (1 + nx * nz)] == f"======== {npw - 1} ========"
    assert not np.fromfile(tmp_path / "output" / "dir.image_lap", np.float32).any()
    assert not os.path.exists(tmp_path / "output" / "dir.illum")
    (tmp_path / "input.dat").write_text((tmp_path / "input.dat").read_text() + "illum=1\nimage_lap=1\n")
    r = _run_rtm_code(tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert_bit_equal(np.fromfile(tmp_path / "output" / "dir.image", np.float32).reshape(nx, nz), img, "dir.image with illum=1")
    assert_bit_equal(np.fromfile(tmp_path / "output" / "dir.illum", np.float32).reshape(nx, nz), ill, "dir.illum")
    assert_bit_equal(np.fromfile(tmp_path / "output" / "dir.image_illum", np.float32).reshape(nx, nz), F.image_compensate(img, ill, 1e-3), "dir.image_illum")
    assert_bit_equal(np.fromfile(tmp_path / "output" / "dir.image_lap", np.float32).reshape(nx, nz), F.image_laplacian(img, 10.0, 10.0), "dir.image_lap")
    if not with_vel_ext:      # the host border loop draws the same stream
        r = _run_rtm_code(tmp_path, {"FDW_HOST_BORDER": "1"})
        assert r.returncode == 0, r.stderr
        assert_bit_equal(np.fromfile(tmp_path / "output" / "dir.image", np.float32).reshape(nx, nz), img, "dir.image with FDW_HOST_BORDER=1")


@pytest.mark.gpu
@pytest.mark.parametrize("with_vel_ext", [False, True], ids=["border-stream", "vel-ext"])
def test_rtm_code_takes_five_plane_waves_in_groups_of_two(tmp_path, with_vel_ext):
    """pw=5 under a batch budget that lets fdw_shot_batch_max be 2: fdw_shot_line_batch takes plane waves {0, 1}, {2, 3}, {4}, each group its
    own line gathers, encoded data, models (draws from j0 T on) and image slots.  dir.image, dir.illum and dir.image_illum against the
    composition plane wave by plane wave, every file and stdout against the run with FDW_NO_SHOT_BATCH=1."""
    import batch_groups as G
    keys = f"pw=5\npw_pmax={PW_PMAX}\nillum=1\n"
    (tmp_path / "grouped").mkdir()
    (tmp_path / "single").mkdir()
    nx, nz, nxb, nzb, nt, ns, vp, d_obs, vel_ext = _pw_deck(tmp_path / "grouped", keys, with_vel_ext)
    _pw_deck(tmp_path / "single", keys, with_vel_ext)
    img, ill = pw_composition(nx, nz, nxb, nzb, nt, ns, vp, d_obs, vel_ext, 5)
    grouped, r = G.run_program("rtm_code", tmp_path / "grouped", G.group_env(nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt))
    G.assert_grouped(r.stderr, "fdw_shot_line_batch")
    assert_bit_equal(np.frombuffer(grouped["dir.image"], np.float32).reshape(nx, nz), img, "dir.image")
    assert_bit_equal(np.frombuffer(grouped["dir.illum"], np.float32).reshape(nx, nz), ill, "dir.illum")
    assert_bit_equal(np.frombuffer(grouped["dir.image_illum"], np.float32).reshape(nx, nz), F.image_compensate(img, ill, 1e-3), "dir.image_illum")
    single, r1 = G.run_program("rtm_code", tmp_path / "single", {"FDW_NO_SHOT_BATCH": "1", "FDW_TIMING": "1"})
    G.assert_grouped(r1.stderr, "one by one", 1)
    assert sorted(grouped) == sorted(single)
    for name in single:
        assert grouped[name] == single[name], name
    assert (tmp_path / "grouped" / "image.num").read_bytes() == (tmp_path / "single" / "image.num").read_bytes()
    assert G.without_exec_time(r.stdout) == G.without_exec_time(r1.stdout)

"""Line sources, second part (fdwave.h): trace recording together with illumination (fdw_dev_line_record_illum_steps), residual migration
(fdw_shot_line_residual), batches of line-source shots (fdw_shot_line_batch, fdw_shot_line_batch_residual, fdw_record_shot_line_batch), the
one-pass data encoder (fdw_encode_gathers_multi) and rtm_code's batched pw= decks.

Every comparison is bit for bit: against the restatement of tests/test_line_source.py (its module docstring spells the chain), against single
calls on fresh contexts, or against the numpy fold.  Outputs are pre-filled with sentinels."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from conftest import assert_bit_equal, make_deck
from oracle import oracle as O
from test_line_source import (FAMILY_CASES, NT, Device, _pw_deck, _run_rtm_code, args_of, extents_of, line_restatement, pipe_case, shot_case,
                              small_case)
from test_stepn_isa_budget import isa  # noqa: F401  (a fixture)

EINVAL, ENODEVICE, ESTATE = -1, -2, -5
NEW_SYMBOLS = ("fdw_dev_line_record_illum_steps", "fdw_shot_line_residual", "fdw_shot_line_batch", "fdw_shot_line_batch_residual",
               "fdw_record_shot_line_batch", "fdw_encode_gathers_multi")


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_new_symbol_is_exported_with_its_signature():
    L = F.lib()
    declared = {name: args for name, _, args in F._lib.SIGNATURES}
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and getattr(L, name).argtypes == declared[name] and getattr(L, name).restype is C.c_int, name
    for method in ("dev_line_record_illum_steps", "shot_line_residual", "shot_line_batch", "shot_line_batch_residual", "record_shot_line_batch"):
        assert callable(getattr(F.FDWave, method))
    assert callable(F.encode_gathers_multi)


def test_combined_line_kernels_exist_in_both_numerics_without_spills(isa):      # noqa: F811
    """The line-source kernels that record and accumulate in one launch, all three families: orders 2-8 at prefetch 2 in both numerics, order 8
    EXACT also at prefetch 1 and 3; no scratch, no spilled VGPR.  And the multi-plane encoder."""
    names = [k for k in isa if "_line_rec_illum_kernel" in k]
    for k in names + [k for k in isa if "fdw_encode_gathers_multi_kernel" in k]:
        meta = isa[k][0]
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (k, meta)
    for num in (0, 1):
        for base in ("fdw_step2_line_rec_illum_kernel", "fdw_stepn_line_rec_illum_kernel"):
            assert any(f"{base}ILi{num}EEEv" in k for k in names), (base, num)
        for h in (1, 2, 3, 4):
            assert any(f"fdw_step_line_rec_illum_kernelILi{h}ELi2ELi{num}EEEv" in k for k in names), (h, num)
    for pf in (1, 3):
        assert any(f"fdw_step_line_rec_illum_kernelILi4ELi{pf}ELi0EEEv" in k for k in names), pf
    assert len(names) == 14, names
    assert sum(1 for k in isa if "fdw_encode_gathers_multi_kernel" in k) == 1


def test_encode_gathers_multi_refuses_before_a_device_is_opened():
    """A negative lag, nplanes < 1 and NULL arguments are FDW_EINVAL where no GPU is; well-formed arguments get past them (to the device)."""
    L = F.lib()
    ns, npl, nx, nt = 3, 2, 5, 7
    lag = np.zeros((npl, ns), np.int32)
    w = np.ones((npl, ns), np.float32)
    d = np.zeros((ns, nx, nt), np.float32)
    out = np.full((npl, nx, nt), 9.0, np.float32)

    def call(nshots=ns, nplanes=npl, lag=lag, w=w, d=d, out=out, nx=nx, nt=nt):
        ptr = [None if a is None else a.ctypes.data for a in (lag, w, d, out)]
        return L.fdw_encode_gathers_multi(0, nshots, nplanes, ptr[0], ptr[1], ptr[2], nx, nt, ptr[3])
    bad = lag.copy()
    bad[1, 2] = -1
    assert call(lag=bad) == EINVAL and b"lag[1][2]" in L.fdw_last_error()
    for kw in (dict(nplanes=0), dict(nplanes=-3), dict(nplanes=65536), dict(lag=None), dict(w=None), dict(d=None), dict(out=None), dict(nx=0), dict(nt=0),
               dict(nshots=-1)):
        assert call(**kw) == EINVAL, kw
    assert (out == 9.0).all()
    with pytest.raises(F.FdwError) as e:
        F.encode_gathers_multi(bad, w, d)
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        F.encode_gathers_multi(lag[0], w[0], d)
    assert call() in (0, ENODEVICE)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_dev_line_record_illum_steps
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_both(dv, sz, gz, nsteps, it0=0, first=False, ip=0, ipp=1):
    out = dv.ctx.dev_line_record_illum_steps([b.data_ptr() for b in dv.bufs], dv.v2.data_ptr(), dv.w.data_ptr(), sz, gz, dv.rec.data_ptr(),
                                             dv.il.data_ptr(), it0, nsteps, first_pp_twice=first, ip=ip, ipp=ipp)
    dv.torch.cuda.synchronize()
    return out


def check_both(dv, want, ip, ipp, nsteps, what):
    """Fields, trace rows and accumulator of ONE run against the restatement (which is also what two runs of dev_line_steps give, one
    recording, one accumulating: tests/test_line_source.py)."""
    assert_bit_equal(dv.field(ipp), want["PP"], "PP, " + what)
    assert_bit_equal(dv.field(ip, finalize=True), want["P"], "P, " + what)
    assert_bit_equal(dv.traces()[:nsteps], want["data"].T[:nsteps], "trace rows, " + what)
    assert (dv.traces()[nsteps:] == 9.0).all(), what
    assert_bit_equal(dv.illum(), want["illum"], "illumination, " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("order,tuning,numerics", FAMILY_CASES)
def test_dev_line_record_illum_steps_vs_restatement(order, tuning, numerics):
    """Noise-filled entry fields and accumulator, a noise line outside and inside the damped strip, the receivers ON the line (gz == sz)."""
    d, p0, pp0, il0, w, want = small_case(order, numerics)
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    for sz in want:
        dv = Device(ctx, d, p0, pp0, w, il0, nt_rec=NT + 2)
        ip, ipp = run_both(dv, sz, sz, NT)
        check_both(dv, want[sz], ip, ipp, NT, f"order {order} {tuning} numerics {numerics} sz {sz}")


@pytest.mark.gpu
@pytest.mark.parametrize("order,tuning", [(8, dict(two_step=-1)), (8, dict(two_step=1)), (8, dict(two_step=4)), (4, {}), (10, {})])
def test_ragged_grid_records_static_rows_and_accumulates(order, tuning):
    """nxe = 87, nxb = 3: nsrc = 77 of nx = 81; the samples beyond the line are 1e30 and the trace rows of the static receiver rows are the
    entry fields' values, alternating."""
    d, p0, pp0, il0, w, want = small_case(order, 0, (87, 70, 3, 10))
    assert extents_of(d)[0] == 80 and (w[:, 77:] == 1e30).all() and w.shape[1] == 81
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(**tuning)
    sz = d["nzb"] + 3
    dv = Device(ctx, d, p0, pp0, w, il0)
    ip, ipp = run_both(dv, sz, sz, NT)
    check_both(dv, want[sz], ip, ipp, NT, f"ragged order {order} {tuning}")
    assert_bit_equal(dv.traces()[0, 77:], p0[80:84, sz], "static rows of the first trace row")
    assert np.abs(want[sz]["PP"]).max() < 1e3


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
def test_pipeline_deck_lean_and_full_tiles(numerics):
    """180 x 500 at 13-row chunks, receivers at depth 310 (strip 1): the line at depth 16 leaves lean tiles in the launch, at 300 none in strip 1."""
    d, p0, pp0, il0, w, want = pipe_case(numerics)
    ctx = F.FDWave(*args_of(d), compat=False, device=0, numerics=numerics)
    ctx.set_tuning(two_step=4, xchunk=13)
    assert ctx.steps_per_pass() == 4
    for sz in (16, 300):
        dv = Device(ctx, d, p0, pp0, w, il0)
        ip, ipp = run_both(dv, sz, 310, 8)
        check_both(dv, want[sz], ip, ipp, 8, f"pipeline deck numerics {numerics} sz {sz}")


@pytest.mark.gpu
def test_dev_line_record_illum_steps_continues_a_loop_and_refuses():
    d, p0, pp0, il0, w, want = small_case(8, 0)
    sz = d["nzb"] + 3
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(two_step=4)
    dv = Device(ctx, d, p0, pp0, w, il0)
    ip, ipp = run_both(dv, sz, sz, 5)
    ip, ipp = run_both(dv, sz, sz, NT - 5, it0=5, first=True, ip=ip, ipp=ipp)
    check_both(dv, want[sz], ip, ipp, NT, "5 + 6 steps")
    dv = Device(ctx, d, p0, pp0, w, il0)
    ptrs = [b.data_ptr() for b in dv.bufs]
    zlim = extents_of(d)[1]

    def code(c, **kw):
        a = dict(d_wav=dv.w.data_ptr(), sz=sz, gz=sz, d_rec=dv.rec.data_ptr(), d_illum=dv.il.data_ptr(), it0=0, nsteps=4)
        a.update(kw)
        with pytest.raises(F.FdwError) as e:
            c.dev_line_record_illum_steps(ptrs, dv.v2.data_ptr(), a["d_wav"], a["sz"], a["gz"], a["d_rec"], a["d_illum"], a["it0"], a["nsteps"])
        return e.value.code
    for kw in (dict(d_rec=None), dict(d_illum=None), dict(d_wav=None), dict(sz=zlim), dict(sz=-1), dict(gz=zlim), dict(gz=-1), dict(it0=-1)):
        assert code(ctx, **kw) == EINVAL, kw
    for other in (F.FDWave(*args_of(d), compat=True, device=0, slab=(0, 40)), F.FDWave(*args_of(d), compat=True, device=0, dialect=1),
                  F.FDWave(*args_of(d), compat=True, device=0, dialect=2)):
        assert code(other) == ESTATE
    with pytest.raises(F.FdwError) as e:      # the older entry point keeps refusing both together
        ctx.dev_line_steps(ptrs, dv.v2.data_ptr(), dv.w.data_ptr(), sz, 0, 4, gz=sz, d_rec=dv.rec.data_ptr(), d_illum=dv.il.data_ptr())
    assert e.value.code == EINVAL
    dv.torch.cuda.synchronize()
    assert_bit_equal(dv.field(0), p0, "a refused call enqueues nothing")
    assert_bit_equal(dv.field(1), pp0, "a refused call enqueues nothing")
    assert_bit_equal(dv.illum(), il0, "a refused call enqueues nothing")
    assert (dv.traces() == 9.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_shot_line_residual
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("tuning", [dict(two_step=-1), dict(two_step=1), dict(two_step=4)], ids=str)
def test_shot_line_residual_is_shot_line_on_the_residual(tuning, numerics):
    d, nx, nz, srce, wav, d_obs, sz, gz, want = shot_case(numerics)
    rng = np.random.default_rng(17)
    im0, il0 = rng.standard_normal((nx, nz)).astype(np.float32), rng.random((nx, nz)).astype(np.float32)
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    got = ctx.shot_line_residual(d["v2"], sz, gz, wav, d_obs, imloc=im0, want_fields=True, want_illum=True, illum=il0)
    d_mod = ctx.record_shot_line(d["v2"], sz, gz, wav)
    assert_bit_equal(d_mod, want["data"], "the modelled gather is the restatement's")
    resid = (d_obs - d_mod).astype(np.float32)
    assert_bit_equal(got["resid"], resid, "resid = d_obs (-) record_shot_line")
    img, P, PP, il = ctx.shot_line(d["v2"], sz, gz, wav, resid, imloc=im0, want_fields=True, want_illum=True, illum=il0)
    for name, a, b in (("image", got["image"], img), ("illum", got["illum"], il), ("P", got["P"], P), ("PP", got["PP"], PP)):
        assert_bit_equal(a, b, f"{name}: shot_line_residual vs shot_line(resid), {tuning} numerics {numerics}")
    assert_bit_equal(PP, want["PP"], "PP vs the restatement")
    plain = ctx.shot_line_residual(d["v2"], sz, gz, wav, d_obs, imloc=im0, want_resid=False)
    assert_bit_equal(plain["image"], img, "image without illumination and without resid")
    assert np.abs(img - im0).max() > 0 and (il - il0).max() > 0


@pytest.mark.gpu
def test_shot_line_residual_of_its_own_data_is_all_zero_words_and_on_the_resident_model():
    nxe, nze, nxb, nzb, nt = 91, 77, 12, 10, 29
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    args = (8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001)
    ctx = F.FDWave(*args, compat=True, device=0)
    rng = np.random.default_rng(3)
    vp = (1500 + 1000 * rng.random((nx, nz))).astype(np.float32)
    wav = rng.standard_normal((nx, nt)).astype(np.float32)
    d_obs = rng.standard_normal((nx, nt)).astype(np.float32)
    im0 = rng.standard_normal((nx, nz)).astype(np.float32)
    sz, gz = nzb + 2, nzb + 1
    ctx.model_resident(vp)
    with pytest.raises(F.FdwError) as e:
        ctx.shot_line_residual(None, sz, gz, wav, d_obs)
    assert e.value.code == ESTATE
    vel = ctx.dev_extendvel_linear(ctx.border_draws(), want_vel=True)
    got = ctx.shot_line_residual(None, sz, gz, wav, d_obs, imloc=im0, want_fields=True, want_illum=True)
    own = ctx.shot_line_residual(None, sz, gz, wav, ctx.record_shot_line(None, sz, gz, wav), imloc=im0)
    assert not own["resid"].view(np.uint32).any(), "data modelled in the migration model leave a residual of all-zero words"
    assert_bit_equal(own["image"], im0, "... and the image keeps its entry values")
    fresh = F.FDWave(*args, compat=True, device=0)
    ref = fresh.shot_line_residual((vel * vel).astype(np.float32), sz, gz, wav, d_obs, imloc=im0, want_fields=True, want_illum=True)
    for name in ("image", "resid", "illum", "P", "PP"):
        assert_bit_equal(got[name], ref[name], name + ": resident model vs the same model handed over")
    assert np.abs(got["image"] - im0).max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: batches
# ---------------------------------------------------------------------------------------------------------------------------------------
NB = 3


@functools.lru_cache(maxsize=None)
def batch_case(order=8, grid=(70, 53, 9, 8), nt=60):
    """Three models, line gathers and data gathers on the geometry of shot_case, and non-zero entry images and accumulators; never modified."""
    d = make_deck(*grid, nt, seed=8, order=order)
    nx, nz = d["nxe"] - 2 * d["nxb"], d["nze"] - 2 * d["nzb"]
    rng = np.random.default_rng(23)
    v2_all = np.stack([(d["v2"] * np.float32(1.0 - 0.04 * b)).astype(np.float32) for b in range(NB)])
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 100.0
    src_ix = np.arange(2, nx, 7, dtype=np.int32)
    wav_all = np.stack([F.encode_line_source(src_ix, F.planewave_lags(src_ix, 10.0, 0.001, p), np.ones(src_ix.size, np.float32), srce, nx)
                        for p in (3e-4, 0.0, -2e-4)])
    wav_all[1, 5] += rng.standard_normal(nt).astype(np.float32)
    d_obs = rng.standard_normal((NB, nx, nt)).astype(np.float32)
    im0 = rng.standard_normal((NB, nx, nz)).astype(np.float32)
    il0 = rng.random((NB, nx, nz)).astype(np.float32)
    for a in (v2_all, wav_all, d_obs, im0, il0):
        a.setflags(write=False)
    return d, nx, nz, v2_all, wav_all, d_obs, im0, il0, d["nzb"] + 2, d["nzb"] + 1


def singles(make_ctx, d, v2_all, wav_all, d_obs, im0, il0, sz, gz, n=NB):
    """What the batch entry points must return, from single calls on one fresh context."""
    c = make_ctx()
    out = dict(plain=[], image=[], illum=[], r_image=[], r_resid=[], ri_image=[], ri_illum=[], data=[])
    for b in range(n):
        out["plain"].append(c.shot_line(v2_all[b], sz, gz, wav_all[b], d_obs[b], imloc=im0[b]))
        im, il = c.shot_line(v2_all[b], sz, gz, wav_all[b], d_obs[b], imloc=im0[b], want_illum=True, illum=il0[b])
        out["image"].append(im), out["illum"].append(il)
        r = c.shot_line_residual(v2_all[b], sz, gz, wav_all[b], d_obs[b], imloc=im0[b])
        out["r_image"].append(r["image"]), out["r_resid"].append(r["resid"])
        r = c.shot_line_residual(v2_all[b], sz, gz, wav_all[b], d_obs[b], imloc=im0[b], want_illum=True, illum=il0[b])
        out["ri_image"].append(r["image"]), out["ri_illum"].append(r["illum"])
        out["data"].append(c.record_shot_line(v2_all[b], sz, gz, wav_all[b]))
    c.close()
    return {k: np.stack(v) for k, v in out.items()}


def check_batches(ctx, want, v2_all, wav_all, d_obs, im0, il0, sz, gz, what, n=NB):
    assert_bit_equal(ctx.shot_line_batch(n, sz, gz, wav_all, d_obs, v2_all=v2_all, imloc=im0), want["plain"], "shot_line_batch, " + what)
    im, il = ctx.shot_line_batch(n, sz, gz, wav_all, d_obs, v2_all=v2_all, imloc=im0, want_illum=True, illum=il0)
    assert_bit_equal(im, want["image"], "shot_line_batch with illum: image, " + what)
    assert_bit_equal(il, want["illum"], "shot_line_batch with illum: illum, " + what)
    r = ctx.shot_line_batch_residual(n, sz, gz, wav_all, d_obs, v2_all=v2_all, imloc=im0)
    assert_bit_equal(r["image"], want["r_image"], "shot_line_batch_residual: image, " + what)
    assert_bit_equal(r["resid"], want["r_resid"], "shot_line_batch_residual: resid, " + what)
    r = ctx.shot_line_batch_residual(n, sz, gz, wav_all, d_obs, v2_all=v2_all, imloc=im0, want_illum=True, illum=il0, want_resid=False)
    assert_bit_equal(r["image"], want["ri_image"], "shot_line_batch_residual with illum: image, " + what)
    assert_bit_equal(r["illum"], want["ri_illum"], "shot_line_batch_residual with illum: illum, " + what)
    assert_bit_equal(ctx.record_shot_line_batch(n, sz, gz, wav_all, v2_all=v2_all), want["data"], "record_shot_line_batch, " + what)
    assert_bit_equal(want["image"], want["plain"], "the accumulator does not touch the image")
    # guards against a trivially empty case, no bound on the code.  The restatement's gathers are non-zero in 70 to 97 % of their samples on
    # the 70 x 53 decks and in 43, 87 and 9.5 % on the short ragged one, whose delayed third line has hardly begun after 24 steps
    assert np.abs(want["plain"] - im0[:n]).max() > 0 and (want["illum"] - il0[:n]).max() > 0
    assert all(np.count_nonzero(g) > 0.05 * g.size for g in want["data"])


@pytest.mark.gpu
@pytest.mark.parametrize("order,prefetch,numerics", [(4, 0, 0), (4, 0, 1), (8, 0, 0), (8, 0, 1), (8, 1, 0), (8, 3, 0)])
def test_line_batches_equal_single_calls(order, prefetch, numerics):
    d, nx, nz, v2_all, wav_all, d_obs, im0, il0, sz, gz = batch_case(order)

    def make_ctx():
        c = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
        c.set_tuning(prefetch=prefetch)
        return c
    want = singles(make_ctx, d, v2_all, wav_all, d_obs, im0, il0, sz, gz)
    ctx = make_ctx()
    assert ctx.shot_batch_max() >= NB and ctx.steps_per_pass() == 1, "this deck batches: one launch per time step for the three shots"
    check_batches(ctx, want, v2_all, wav_all, d_obs, im0, il0, sz, gz, f"order {order} prefetch {prefetch} numerics {numerics}")
    if order == 8 and prefetch == 0:      # and directly against the restatement: gather, illumination from rest, image through Oracle.back
        orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
        nxb, nzb = d["nxb"], d["nzb"]
        im, il = ctx.shot_line_batch(NB, sz, gz, wav_all, d_obs, v2_all=v2_all, want_illum=True)
        data = ctx.record_shot_line_batch(NB, sz, gz, wav_all, v2_all=v2_all)
        for b in range(NB):
            r = line_restatement(orc, d, v2_all[b], wav_all[b].T, sz, gz=gz)
            assert_bit_equal(data[b], r["data"], f"gather of shot {b} vs the restatement")
            assert_bit_equal(il[b], r["illum"][nxb:nxb + nx, nzb:nzb + nz], f"illumination of shot {b} vs the restatement")
            assert_bit_equal(im[b], orc.back(v2_all[b], r["P"], r["PP"], d_obs[b], gz), f"image of shot {b} vs Oracle.back on the restatement's fields")


@pytest.mark.gpu
def test_line_batch_on_resident_border_models_and_a_batch_of_one():
    """v2_all = None: shot b on the border model of draws draw_offset + b T, here from draw_offset = 2 T, on the 91 x 77 deck; and nshots = 1."""
    nxe, nze, nxb, nzb, nt = 91, 77, 12, 10, 29
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    args = (8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001)
    rng = np.random.default_rng(5)
    vp = (1500 + 1000 * rng.random((nx, nz))).astype(np.float32)
    wav_all = rng.standard_normal((NB, nx, nt)).astype(np.float32)
    d_obs = rng.standard_normal((NB, nx, nt)).astype(np.float32)
    im0, il0 = rng.standard_normal((NB, nx, nz)).astype(np.float32), rng.random((NB, nx, nz)).astype(np.float32)
    sz, gz = nzb + 2, nzb + 1
    ctx = F.FDWave(*args, compat=True, device=0)
    ctx.model_resident(vp)
    T = ctx.border_draws()
    assert ctx.shot_batch_max() >= NB
    got = ctx.shot_line_batch_residual(NB, sz, gz, wav_all, d_obs, draw_offset=2 * T, imloc=im0, want_illum=True, illum=il0)
    data = ctx.record_shot_line_batch(NB, sz, gz, wav_all, draw_offset=2 * T)
    plain = ctx.shot_line_batch(NB, sz, gz, wav_all, d_obs, draw_offset=2 * T, imloc=im0)
    one = F.FDWave(*args, compat=True, device=0)
    one.model_resident(vp)
    for b in range(NB):
        one.dev_extendvel_linear((2 + b) * T)
        r = one.shot_line_residual(None, sz, gz, wav_all[b], d_obs[b], imloc=im0[b], want_illum=True, illum=il0[b])
        for name in ("image", "resid", "illum"):
            assert_bit_equal(got[name][b], r[name], f"{name} of shot {b}: draws from (2 + {b}) T")
        assert_bit_equal(data[b], one.record_shot_line(None, sz, gz, wav_all[b]), f"gather of shot {b}")
        assert_bit_equal(plain[b], one.shot_line(None, sz, gz, wav_all[b], d_obs[b], imloc=im0[b]), f"image of shot {b}")
    # nshots = 1: the single call
    one.dev_extendvel_linear(5 * T)
    r = one.shot_line_residual(None, sz, gz, wav_all[1], d_obs[1], imloc=im0[1], want_illum=True, illum=il0[1])
    g1 = ctx.shot_line_batch_residual(1, sz, gz, wav_all[1:2], d_obs[1:2], draw_offset=5 * T, imloc=im0[1:2], want_illum=True, illum=il0[1:2])
    for name in ("image", "resid", "illum"):
        assert_bit_equal(g1[name][0], r[name], name + ", a batch of one")
    im1, il1 = ctx.shot_line_batch(1, sz, gz, wav_all[1:2], d_obs[1:2], draw_offset=5 * T, imloc=im0[1:2], want_illum=True, illum=il0[1:2])
    im, il = one.shot_line(None, sz, gz, wav_all[1], d_obs[1], imloc=im0[1], want_illum=True, illum=il0[1])
    assert_bit_equal(im1[0], im, "image, a batch of one")
    assert_bit_equal(il1[0], il, "illum, a batch of one")
    assert_bit_equal(ctx.record_shot_line_batch(1, sz, gz, wav_all[1:2], draw_offset=5 * T)[0], one.record_shot_line(None, sz, gz, wav_all[1]), "gather, a batch of one")
    with pytest.raises(F.FdwError) as e:
        ctx.shot_line_batch(NB, extents_of(dict(nxe=nxe, nze=nze, nzb=nzb))[1], gz, wav_all, d_obs)
    assert e.value.code == EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("name,order,tuning,grid", [
    ("order10", 10, {}, (70, 53, 9, 8)), ("generic", 8, dict(use_generic=True), (70, 53, 9, 8)), ("pipeline", 8, dict(two_step=4), (70, 53, 9, 8)),
    ("ragged", 8, {}, (87, 70, 3, 10))])
def test_line_batch_fallbacks_give_the_same_bytes(name, order, tuning, grid):
    """Where fdw_shot_batch does not batch -- an order above 8, the forced generic kernel, a multi-step family, receiver rows the loop never
    time-steps -- the shots run one by one inside the call: the same bytes."""
    d, nx, nz, v2_all, wav_all, d_obs, im0, il0, sz, gz = batch_case(order, grid, 24)

    def make_ctx():
        c = F.FDWave(*args_of(d), compat=True, device=0)
        c.set_tuning(**tuning)
        return c
    ctx = make_ctx()
    assert ctx.shot_batch_max() == 1, name
    want = singles(make_ctx, d, v2_all, wav_all, d_obs, im0, il0, sz, gz)
    check_batches(ctx, want, v2_all, wav_all, d_obs, im0, il0, sz, gz, name)


@pytest.mark.gpu
def test_one_context_through_point_and_line_batches():
    """shot_batch -> shot_line_batch -> shot_line -> shot_line_batch_residual on one context: each answer equals a fresh context's."""
    d, nx, nz, v2_all, wav_all, d_obs, im0, il0, sz, gz = batch_case(8)
    srce = O.ricker_wavelet(d["nt"], 0.001, 30.0) * 100.0
    sx0 = d["nxb"] + 10
    calls = [lambda c: (c.shot_batch(NB, sx0, 9, sz, gz, srce, d_obs, v2_all=v2_all, imloc=im0),),
             lambda c: c.shot_line_batch(NB, sz, gz, wav_all, d_obs, v2_all=v2_all, imloc=im0, want_illum=True, illum=il0),
             lambda c: c.shot_line(v2_all[2], sz, gz, wav_all[0], d_obs[1], want_fields=True, want_illum=True),
             lambda c: tuple(c.shot_line_batch_residual(NB, sz, gz, wav_all[::-1], d_obs, v2_all=v2_all, want_illum=True).values()),
             lambda c: (c.shot_batch(NB, sx0, 9, sz, gz, srce, d_obs, v2_all=v2_all),)]
    one = F.FDWave(*args_of(d), compat=True, device=0)
    for i, call in enumerate(calls):
        fresh = F.FDWave(*args_of(d), compat=True, device=0)
        for j, (a, b) in enumerate(zip(call(one), call(fresh))):
            assert_bit_equal(a, b, f"call {i}, output {j}")
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the one-pass encoder and the program
# ---------------------------------------------------------------------------------------------------------------------------------------
def fold(lag, weight, d_obs_all):
    """out[ix][it]: shots in ascending order from +0.0f, product and sum rounded separately."""
    ns, nx, nt = d_obs_all.shape
    out = np.zeros((nx, nt), np.float32)
    for s in range(ns):
        L = int(lag[s])
        if L < nt:
            out[:, L:] = (out[:, L:] + (np.float32(weight[s]) * d_obs_all[s][:, :nt - L]).astype(np.float32)).astype(np.float32)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nplanes", [1, 4])
@pytest.mark.parametrize("nt", [63, 257])
@pytest.mark.parametrize("nshots", [1, 7])
def test_encode_gathers_multi_equals_single_encodings_and_the_fold(nshots, nt, nplanes):
    nx = 37
    rng = np.random.default_rng(nshots * 1000 + nt + nplanes)
    d_obs_all = rng.standard_normal((nshots, nx, nt)).astype(np.float32)
    d_obs_all[0, 3, 5] = -0.0
    lags = np.array([[0, nt - 1, nt, 3, 3, 2 * nt + 1, 17], [5, 0, 1, 2, nt + 3, 4, 0], [nt, nt, nt, nt, nt, nt, nt], [1, 2, 3, 4, 5, 6, 7]], np.int32)
    weights = np.array([[1.0, -1.0, 1.0, 0.3721, -1.0, 1.0, 1.0], [-1.0, 1.0, 0.3721, 1.0, 1.0, -1.0, 1.0], [1.0] * 7, [0.3721, -1, 1, -1, 1, -1, 0.3721]], np.float32)
    lag, weight = lags[:nplanes, :nshots], weights[:nplanes, :nshots]
    got = F.encode_gathers_multi(lag, weight, d_obs_all)
    assert got.shape == (nplanes, nx, nt)
    for j in range(nplanes):
        assert_bit_equal(got[j], F.encode_gathers(lag[j], weight[j], d_obs_all), f"plane {j} vs encode_gathers, {nshots} shots, nt {nt}")
        assert_bit_equal(got[j], fold(lag[j], weight[j], d_obs_all), f"plane {j} vs the fold")
    assert np.count_nonzero(got[0]) > 0.9 * got[0].size
    if nplanes == 4:
        assert not got[2].view(np.uint32).any(), "every lag >= nt: +0.0f everywhere"


@pytest.mark.gpu
@pytest.mark.parametrize("with_vel_ext", [False, True], ids=["border-stream", "vel-ext"])
def test_rtm_code_batches_its_plane_waves(tmp_path, with_vel_ext):
    """pw=4 with illum=1: the default environment (fdw_encode_gathers_multi + fdw_shot_line_batch) against FDW_NO_SHOT_BATCH=1 (one plane wave
    after the other): every output file and stdout byte for byte, and FDW_TIMING names the path."""
    outs = {}
    for sub, env, word in (("batch", {}, "fdw_shot_line_batch"), ("single", {"FDW_NO_SHOT_BATCH": "1"}, "one by one")):
        work = tmp_path / sub
        work.mkdir()
        _pw_deck(work, "pw=4\npw_pmax=2e-4\nillum=1\nimage_lap=1\n", with_vel_ext)
        r = _run_rtm_code(work, dict(env, FDW_TIMING="1"))
        assert r.returncode == 0, r.stderr + r.stdout
        line = [ln for ln in r.stderr.splitlines() if "shots per launch sequence" in ln]
        assert len(line) == 1 and word in line[0], r.stderr
        assert ("up to 4" in line[0]) == (sub == "batch"), line[0]
        files = {f: (work / "output" / f).read_bytes() for f in sorted(os.listdir(work / "output"))}
        files["image.num"] = (work / "image.num").read_bytes()
        files["stdout"] = "\n".join(ln for ln in r.stdout.splitlines() if "Exec time" not in ln).encode()
        outs[sub] = files
    assert set(outs["batch"]) == set(outs["single"]) >= {"dir.image", "dir.illum", "dir.image_illum", "dir.image_lap", "image.num", "stdout"}
    for f in outs["batch"]:
        assert outs["batch"][f] == outs["single"][f], f
    assert np.frombuffer(outs["batch"]["dir.image"], np.float32).any() and np.frombuffer(outs["batch"]["dir.illum"], np.float32).any()
    if not with_vel_ext:      # the host border loop draws its models in the order j from the one stream
        work = tmp_path / "host"
        work.mkdir()
        _pw_deck(work, "pw=4\npw_pmax=2e-4\nillum=1\nimage_lap=1\n", with_vel_ext)
        r = _run_rtm_code(work, {"FDW_HOST_BORDER": "1", "FDW_TIMING": "1"})
        assert r.returncode == 0 and "fdw_shot_line_batch" in r.stderr, r.stderr
        for f in ("dir.image", "dir.illum", "dir.image_illum"):
            assert (work / "output" / f).read_bytes() == outs["single"][f], f + " with FDW_HOST_BORDER=1"

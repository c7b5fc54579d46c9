"""Residual migration (fdwave.h): fdw_shot_residual images d_obs minus the gather its own forward loop models, fdw_dev_record_illum_steps is the
forward loop that records and accumulates the source illumination in one launch per pass, fdw_dev_gather_residual the subtraction kernel,
fdw_gather_misfit the host misfit, rtm_code's deck key resid=1 the program.

The reference throughout is the composition the feature replaces, through entry points the other modules pin to the CPU oracle:
record_shot in the migration model (tests/test_record.py), one np.float32 subtraction, then shot / shot(want_illum=True)
(tests/test_gpu_parity.py, tests/test_illum.py) -- bit for bit.  The batch is in tests/test_residual_batch.py."""
import functools
import os
import subprocess

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
import value_classes as V
from conftest import ROOT, assert_bit_equal, make_deck, random_fields
from oracle import oracle as O
from test_illum import _Device
from test_record import interface_hits, two_layer_case

BIN = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin")

# the compat deck of tests/test_record.py: nxe = 69 -> rows >= 64 are never time-stepped and nxb = 3 puts receiver rows 64, 65 (traces 61, 62)
# among them; nze = 301 -> zlim = 296, so the receiver line sits on both sides of the one-step kernel's strip border (256) and of the
# pipeline's (224); nzb = 10 -> ztap = 8; dx != dz
NXE, NZE, NXB, NZB, NT = 69, 301, 3, 10, 23
NX, NZ = NXE - 2 * NXB, NZE - 2 * NZB
LIVE = 64 - NXB                                           # traces below this one sit on time-stepped rows
SX = 58                                                   # a few rows from the static ones: their neighbours record a signal at every order


def _deck(order=8, nt=NT):
    return make_deck(NXE, NZE, NXB, NZB, nt, seed=3, order=order, dx=10.0, dz=12.5)


def _args(d):
    return (d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"])


@functools.lru_cache(maxsize=None)
def _shot_inputs():
    """Wavelet, observed gather (noise: non-zero on every trace), non-zero entry image, positive entry illumination."""
    rng = np.random.default_rng(77)
    srce = (O.ricker_wavelet(NT, 0.001, 30.0) * 1000.0).astype(np.float32)
    d_obs = rng.standard_normal((NX, NT)).astype(np.float32)
    im0 = rng.standard_normal((NX, NZ)).astype(np.float32)
    il0 = (0.5 + rng.random((NX, NZ))).astype(np.float32)
    return srce, d_obs, im0, il0


def composition(ctx, v2, sx, sz, gz, srce, d_obs, im0, il0):
    """What shot_residual replaces: (resid, image, P, PP, illum); illum is None without il0.  v2 None: the resident squared model."""
    def rec():
        if v2 is None:      # the resident model through the entry points that read it: a gather is what record_shot gives on the same model
            raise AssertionError("composition needs the model on the host")
        return ctx.record_shot(v2, sx, sz, gz, srce)
    d_mod = rec()
    resid = (d_obs - d_mod).astype(np.float32)
    if il0 is None:
        img, P, PP = ctx.shot(v2, sx, sz, gz, srce, resid, imloc=im0, want_fields=True)
        return resid, d_mod, img, P, PP, None
    img, P, PP, il = ctx.shot(v2, sx, sz, gz, srce, resid, imloc=im0, want_fields=True, want_illum=True, illum=il0)
    return resid, d_mod, img, P, PP, il


def assert_residual_not_vacuous(resid, d_obs, d_mod, what):
    """The static rows carry d_obs itself (d_mod is zero there from rest); their time-stepped neighbours carry a modelled signal and a
    non-zero difference."""
    assert_bit_equal(resid[LIVE:], d_obs[LIVE:], "static receiver rows, " + what)
    assert not d_mod[LIVE:].any(), what
    for ix in (LIVE - 1, LIVE - 2):
        assert resid[ix].any() and d_mod[ix].any() and (resid[ix] != d_obs[ix]).any(), (what, ix)
    assert np.count_nonzero(resid != d_obs) > NX, what


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: symbols, the misfit, the refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_residual_symbol_is_exported():
    L = F.lib()
    for name in ("fdw_dev_gather_residual", "fdw_dev_record_illum_steps", "fdw_shot_residual", "fdw_shot_batch_residual", "fdw_gather_misfit"):
        assert hasattr(L, name), name
    for name in ("shot_residual", "shot_batch_residual", "dev_record_illum_steps", "dev_gather_residual"):
        assert hasattr(F.FDWave, name), name
    assert callable(F.gather_misfit)


def misfit_formula(a):
    s = 0.0
    for x in np.asarray(a, np.float32).ravel().tolist():      # Python floats are doubles; a float32 converts exactly
        s = s + x * x
    return 0.5 * s


def test_gather_misfit_matches_its_formula():
    rng = np.random.default_rng(1)
    noise = rng.standard_normal(1027).astype(np.float32)
    big = np.ldexp(rng.standard_normal(64).astype(np.float32), 60).astype(np.float32)       # 2^60 values: the square overflows fp32, not double
    mixed = V.patched_1d(999, 5, classes=V.FINITE)
    for name, a in (("zeros", np.zeros(100, np.float32)), ("noise", noise), ("2^60", big), ("value classes", mixed), ("empty", np.zeros(0, np.float32))):
        got, want = F.gather_misfit(a), misfit_formula(a)
        assert np.isfinite(want), name
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (name, got, want)
    assert F.gather_misfit(np.zeros(100, np.float32)) == 0.0 and F.gather_misfit(np.zeros(0, np.float32)) == 0.0
    assert F.gather_misfit(big) > 2.0 ** 100
    with_nan = noise.copy()
    with_nan[500] = np.nan
    assert np.isnan(F.gather_misfit(with_nan))                     # one NaN propagates
    # a sum in fp32, or squares formed in fp32, would differ
    assert F.gather_misfit(noise) != 0.5 * float(np.sum(noise * noise, dtype=np.float32))
    import ctypes
    m = ctypes.c_double(7.0)
    assert F.lib().fdw_gather_misfit(None, 3, ctypes.byref(m)) != 0 and F.lib().fdw_gather_misfit(noise.ctypes.data, 3, None) != 0


def _write_min_deck(tmp_path, extra):
    np.full((20, 30), 2000.0, np.float32).tofile(tmp_path / "vp.bin")
    np.zeros(2 * 30 * 10, np.float32).tofile(tmp_path / "dobs.bin")
    (tmp_path / "out").mkdir(exist_ok=True)
    (tmp_path / "input.dat").write_text("tmpdir=./out\nvpfile=./vp.bin\ndatfile=./dobs.bin\nnz=20\nnx=30\nnt=10\ndz=10\ndx=10\ndt=0.001\nfpeak=25\n"
                                        "ns=2\nsz=1\nfsx=3\nds=5\ngz=2\nnxb=8\nnzb=8\nfac=0.75\norder=8\n" + extra)


@pytest.mark.parametrize("extra,env_extra,words", [("resid=1\nslabs=2\n", {}, ("resid", "slabs")), ("resid=1\n", {"FDW_SLABS": "2"}, ("resid", "slabs")),
                                                   ("resid=1\nsnap=5\n", {}, ("resid", "snap"))], ids=["slabs-key", "FDW_SLABS", "snap"])
def test_rtm_code_refuses_resid_with_slabs_or_snapshots(tmp_path, extra, env_extra, words):
    """Before any file, thread, communicator or device is touched: runs where no GPU is, and leaves the output directory empty."""
    _write_min_deck(tmp_path, extra)
    env = {k: v for k, v in os.environ.items() if k not in ("FDW_SLABS", "FDW_GPUS")}
    env.update(env_extra)
    r = subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode != 0
    assert all(w in r.stderr for w in words), r.stderr
    assert os.listdir(tmp_path / "out") == []
    assert not os.path.exists(tmp_path / "image.num")


def test_python_driver_refuses_a_resid_deck(tmp_path):
    from parallel_finite_difference_computation_amd import rtm
    _write_min_deck(tmp_path, "resid=1\n")
    with pytest.raises(ValueError, match="resid"):
        rtm.read_deck(str(tmp_path / "input.dat"))
    (tmp_path / "input.dat").write_text((tmp_path / "input.dat").read_text().replace("resid=1", "resid=0"))
    assert rtm.read_deck(str(tmp_path / "input.dat"))["resid"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the subtraction kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def _class_operands(n, seed):
    """a, b of n floats in runs of every value class, +-inf (inf - inf among them) and NaNs with payloads."""
    a = V.patched_1d(n, seed, classes=V.CLASSES, run=2)
    b = V.patched_1d(n, seed + 1, classes=V.CLASSES, run=3)
    rng = np.random.default_rng(seed)
    if n >= 16:
        k = rng.choice(n, size=max(4, n // 16), replace=False)
        q = len(k) // 4
        a[k[:q]] = np.inf
        b[k[:q]] = np.where(np.arange(q) % 2 == 0, np.inf, -np.inf)            # inf - inf = NaN, inf - -inf = inf
        b[k[q:2 * q]] = -np.inf
        a.view(np.uint32)[k[2 * q:3 * q]] = 0x7FC00000 | rng.integers(1, 1 << 22, len(k[2 * q:3 * q]), dtype=np.uint32)      # NaN payloads
        b.view(np.uint32)[k[3 * q:]] = 0xFF800001 + rng.integers(0, 1 << 22, len(k[3 * q:]), dtype=np.uint32)
        a[k[0]] = b[k[0]] = np.float32(1.5)                                      # exact cancellation: +0
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_dev_gather_residual_vs_float32_subtraction(n):
    """Out of place with guard words on both sides of the output (at an aligned and at an odd offset: the 16-byte path and the scalar one),
    and in place.  NaNs by position (the sign and payload of a NaN result differ between the CPU and the GPU), everything else bit for bit."""
    import torch
    dev = torch.device("cuda:0")
    ctx = F.FDWave(8, NXE, NZE, NXB, NZB, NT, 0.75, 10.0, 12.5, 0.001, compat=True, device=0)
    a, b = _class_operands(n, 40 + n)
    with np.errstate(invalid="ignore", over="ignore"):
        want = (a - b).astype(np.float32)
    if n == 1027:
        c = V.classify(want)
        assert c["subnormal"] > 0 and c["nan"] > 0 and c["inf"] > 0 and c["large"] > 0 and c["pzero"] > 0, c
        assert V.classify(a)["nan"] > 0 and V.classify(b)["nan"] > 0
        assert (np.isinf(a) & np.isinf(b) & np.isnan(want)).any()                # inf - inf
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    for lead in (4, 5):                                                          # floats before the output: 16-byte aligned or not
        out = torch.full((lead + n + 7,), 9.0, device=dev)
        torch.cuda.synchronize()
        ctx.dev_gather_residual(ta.data_ptr(), tb.data_ptr(), out.data_ptr() + 4 * lead, n)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[:lead] == 9.0).all() and (got[lead + n:] == 9.0).all(), f"guard words, n {n} lead {lead}"
        V.assert_same_nonfinite(got[lead:lead + n], want, f"out of place, n {n} lead {lead}")
    inplace = ta.clone()
    torch.cuda.synchronize()
    ctx.dev_gather_residual(inplace.data_ptr(), tb.data_ptr(), inplace.data_ptr(), n)
    torch.cuda.synchronize()
    V.assert_same_nonfinite(inplace.cpu().numpy(), want, f"in place, n {n}")
    assert_bit_equal(tb.cpu().numpy(), b, "the subtrahend is left alone")


@pytest.mark.gpu
def test_dev_gather_residual_past_two_gib():
    """One launch over 2^29 + 5 floats (just past 2^31 bytes), in place: an index that wraps at 32 bits leaves the far end unwritten or
    writes the near end twice.  Checked on the device; head, tail and the words around the 2^31-byte mark also on the host."""
    import torch
    dev = torch.device("cuda:0")
    n = (1 << 29) + 5
    ctx = F.FDWave(8, NXE, NZE, NXB, NZB, NT, 0.75, 10.0, 12.5, 0.001, compat=True, device=0)
    a = torch.arange(n, device=dev, dtype=torch.int32).remainder_(4099).to(torch.float32)      # exact small integers, a period that is no power of two
    b = torch.full((n,), 0.5, device=dev)
    b[1::2] = -1.25
    want = a - b
    torch.cuda.synchronize()
    ctx.dev_gather_residual(a.data_ptr(), b.data_ptr(), a.data_ptr(), n)
    torch.cuda.synchronize()
    assert bool(torch.equal(a, want))
    for lo, hi in ((0, 8), ((1 << 29) - 8, (1 << 29) + 5)):
        idx = np.arange(lo, hi)
        host = (idx % 4099).astype(np.float32) - np.where(idx % 2 == 0, np.float32(0.5), np.float32(-1.25))
        assert_bit_equal(a[lo:hi].cpu().numpy(), host.astype(np.float32), f"words {lo}..{hi}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: shot_residual against the composition it replaces
# ---------------------------------------------------------------------------------------------------------------------------------------
SHOT_CASES = [  # (order, tuning, gz, sz): the receiver line on both sides of each family's strip border, the source a few cells from it
    (2, {}, 255, 252), (4, {}, 256, 259), (6, {}, 255, 252), (10, {}, 256, 259),
    (8, dict(two_step=-1, prefetch=1), 255, 252), (8, dict(two_step=-1, prefetch=2), 256, 259), (8, dict(two_step=-1, prefetch=3), 255, 252),
    (8, dict(two_step=-1, prefetch=2), 255, 255),                                # sz == gz: the source sample is in the recorded cell
    (8, dict(use_generic=True, two_step=-1), 256, 259),
    (8, dict(two_step=4), 223, 220), (8, dict(two_step=4), 224, 227),
]


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("order,tuning,gz,sz", SHOT_CASES)
def test_shot_residual_vs_the_composition(order, tuning, gz, sz, numerics):
    d = _deck(order)
    srce, d_obs, im0, il0 = _shot_inputs()
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    if tuning.get("two_step") == 4:
        assert ctx.steps_per_pass() == 4
    for entry_il in (None, il0):
        what = f"order {order} {tuning} gz {gz} numerics {numerics} illum {entry_il is not None}"
        resid, d_mod, img, P, PP, il = composition(ctx, d["v2"], SX, sz, gz, srce, d_obs, im0, entry_il)
        got = ctx.shot_residual(d["v2"], SX, sz, gz, srce, d_obs, imloc=im0, want_fields=True, want_illum=entry_il is not None, illum=entry_il)
        assert_bit_equal(got["resid"], resid, "resid, " + what)
        assert_bit_equal(got["image"], img, "image, " + what)
        assert_bit_equal(got["P"], P, "P, " + what)
        assert_bit_equal(got["PP"], PP, "PP, " + what)
        if entry_il is not None:
            assert_bit_equal(got["illum"], il, "illum, " + what)
            assert (il > il0).any()
        else:
            assert "illum" not in got
        assert_residual_not_vacuous(resid, d_obs, d_mod, what)
        assert (img != im0).any(), what
        # the image does differ from the one the gather as it stands gives
        assert (img != ctx.shot(d["v2"], SX, sz, gz, srce, d_obs, imloc=im0)).any(), what
    # resid not asked for: the same image
    lean = ctx.shot_residual(d["v2"], SX, sz, gz, srce, d_obs, imloc=im0, want_resid=False)
    assert sorted(lean) == ["image"]
    assert_bit_equal(lean["image"], img, "image without the residual download")


@pytest.mark.gpu
@pytest.mark.parametrize("tuning,gz,sz", [(dict(two_step=-1), 256, 259), (dict(two_step=4), 223, 220)], ids=["one-step", "pipeline"])
def test_shot_residual_on_the_resident_model(tuning, gz, sz):
    """v2 = None: the squared model dev_extendvel_linear left in HBM, against the composition on the same model handed over by the host."""
    d = _deck(8)
    srce, d_obs, im0, il0 = _shot_inputs()
    ctx = F.FDWave(*_args(d), compat=True, device=0)
    ctx.set_tuning(**tuning)
    with pytest.raises(F.FdwError) as e:
        ctx.shot_residual(None, SX, sz, gz, srce, d_obs)
    assert e.value.code == -5                                                   # FDW_ESTATE: no resident squared model yet
    vp = (1500 + 1000 * np.random.default_rng(3).random((NX, NZ))).astype(np.float32)
    ctx.model_resident(vp)
    off = 3 * ctx.border_draws()
    vel = ctx.dev_extendvel_linear(off, want_vel=True)
    v2 = (vel * vel).astype(np.float32)
    for entry_il in (None, il0):
        resid, d_mod, img, P, PP, il = composition(ctx, v2, SX, sz, gz, srce, d_obs, im0, entry_il)
        ctx.dev_extendvel_linear(off)
        got = ctx.shot_residual(None, SX, sz, gz, srce, d_obs, imloc=im0, want_fields=True, want_illum=entry_il is not None, illum=entry_il)
        for name, want in (("resid", resid), ("image", img), ("P", P), ("PP", PP)) + ((("illum", il),) if entry_il is not None else ()):
            assert_bit_equal(got[name], want, f"{name}, resident model, {tuning}, illum {entry_il is not None}")
        assert_residual_not_vacuous(resid, d_obs, d_mod, f"resident model {tuning}")


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("tuning,gz,sz", [(dict(two_step=-1), 256, 259), (dict(two_step=4), 224, 227), (dict(two_step=0), 255, 252)],
                         ids=["one-step", "pipeline", "auto"])
def test_a_gather_modelled_in_the_migration_model_leaves_a_zero_residual(tuning, gz, sz, numerics):
    d = _deck(8)
    srce, _, im0, il0 = _shot_inputs()
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    d_obs = ctx.record_shot(d["v2"], SX, sz, gz, srce)
    assert np.count_nonzero(d_obs) > NX
    got = ctx.shot_residual(d["v2"], SX, sz, gz, srce, d_obs, imloc=im0, want_illum=True, illum=il0)
    assert not got["resid"].view(np.uint32).any()                               # every word 0x00000000: no -0, no subnormal left over
    assert_bit_equal(got["image"], im0, "the image keeps its entry values")
    assert (got["illum"] > il0).any()
    assert F.gather_misfit(got["resid"]) == 0.0


@pytest.mark.gpu
def test_shot_residual_refusals():
    d = _deck(8)
    srce, d_obs, _, _ = _shot_inputs()
    ctx = F.FDWave(*_args(d), compat=True, device=0)
    for gz in (-1, 296, NZE):                                                   # zlim = 296: the columns the forward loop time-steps
        with pytest.raises(F.FdwError) as e:
            ctx.shot_residual(d["v2"], SX, 20, gz, srce, d_obs)
        assert e.value.code == -1                                               # FDW_EINVAL
    slab = F.FDWave(*_args(d), compat=True, device=0, slab=(0, 40))
    mod = F.FDWave(*_args(d), compat=True, device=0, dialect=1)
    for other in (slab, mod):
        with pytest.raises(F.FdwError) as e:
            other.shot_residual(d["v2"], SX, 20, 20, srce, d_obs)
        assert e.value.code == -5                                               # FDW_ESTATE
        with pytest.raises(F.FdwError) as e:
            other.shot_batch_residual(2, SX, 3, 20, 20, srce, np.stack([d_obs, d_obs]), v2_all=np.stack([d["v2"], d["v2"]]))
        assert e.value.code == -5


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the combined forward loop against the three existing ones
# ---------------------------------------------------------------------------------------------------------------------------------------
STEP_FAMILIES = [  # (order, tuning, (sz, gz) pairs across the family's strip border)
    (2, {}, ((255, 256), (256, 255))), (4, {}, ((255, 256), (256, 255))), (6, {}, ((255, 256), (256, 255))), (10, {}, ((255, 256), (256, 255))),
    (8, dict(two_step=-1, prefetch=1), ((255, 256), (256, 255))), (8, dict(two_step=-1, prefetch=2), ((255, 256), (256, 255))),
    (8, dict(two_step=-1, prefetch=3), ((255, 256), (256, 255))), (8, dict(use_generic=True, two_step=-1), ((255, 256), (256, 255))),
    (8, dict(two_step=4), ((223, 224), (224, 223))),
    (8, dict(two_step=1), ((239, 240), (240, 239))),      # two-step forced: the combined loop has no such kernel and runs single steps
]


class _Run(_Device):
    """_Device plus a trace buffer [nt + 2][nx] filled with a guard value."""

    def __init__(self, ctx, d, p0, pp0, il0, srce, nt):
        super().__init__(ctx, d, p0, pp0, il0, srce)
        self.nx = d["nxe"] - 2 * d["nxb"]
        self.rec = self.torch.full((nt + 2, self.nx), 9.0, device=self.bufs[0].device)
        self.torch.cuda.synchronize()

    def traces(self):
        return self.rec.cpu().numpy()


def _three_way(ctx, d, p0, pp0, il0, srce, sx, sz, gz, nt, calls, what):
    """The combined loop over `calls` = [(it0, nsteps), ...] against dev_steps2 (fields, indices), dev_record_steps (trace rows) and
    dev_illum_steps (accumulator) over the same calls from the same entry state."""
    import torch
    runs = {}
    for kind in ("both", "plain", "rec", "ill"):
        r = _Run(ctx, d, p0, pp0, il0, srce, nt)
        ip, ipp, first = 0, 1, False
        for it0, n in calls:
            a = (r.ptrs(), r.v2.data_ptr(), r.srce.data_ptr(), sx, sz)
            if kind == "both":
                ip, ipp = ctx.dev_record_illum_steps(*a, gz, r.rec.data_ptr(), r.il.data_ptr(), it0, n, first, ip, ipp)
            elif kind == "plain":
                ip, ipp = ctx.dev_steps2(*a, it0, n, first, ip, ipp)
            elif kind == "rec":
                ip, ipp = ctx.dev_record_steps(*a, gz, r.rec.data_ptr(), it0, n, first, ip, ipp)
            else:
                ip, ipp = ctx.dev_illum_steps(*a, r.il.data_ptr(), it0, n, first, ip, ipp)
            first = True
        torch.cuda.synchronize()
        runs[kind] = (r, (ip, ipp))
    both, idx = runs["both"]
    assert idx == runs["plain"][1] == runs["rec"][1] == runs["ill"][1], what
    for i in range(4):
        assert_bit_equal(both.field(i), runs["plain"][0].field(i), f"buffer {i} vs dev_steps2, " + what)
    assert_bit_equal(both.traces(), runs["rec"][0].traces(), "trace rows vs dev_record_steps, " + what)
    assert_bit_equal(both.illum(), runs["ill"][0].illum(), "accumulator vs dev_illum_steps, " + what)
    return both


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("order,tuning,places", STEP_FAMILIES)
def test_dev_record_illum_steps_vs_the_three_loops(order, tuning, places, numerics):
    """Noise-filled entry fields (static rows included) and a positive entry illumination, 1 to 9 steps, 5 + 4 == 9."""
    nt = 9
    d = _deck(order, nt)
    p0, pp0 = random_fields(d, 5, amp=0.01)
    il0 = (0.5 + np.random.default_rng(9).random((NXE, NZE))).astype(np.float32)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0 + np.float32(3.0)
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    for sz, gz in places:
        for nsteps in range(1, 10):
            what = f"order {order} {tuning} numerics {numerics} sz {sz} gz {gz}, {nsteps} steps"
            r = _three_way(ctx, d, p0, pp0, il0, srce, SX, sz, gz, nt, [(0, nsteps)], what)
            t = r.traces()
            assert (t[nsteps:] == 9.0).all() and (t[:nsteps] != 9.0).all(), what          # exactly the rows of the steps taken
            assert (t[:nsteps, LIVE:] != 0).all()                                        # static receiver rows: the entry fields' values
            il = r.illum()
            assert (il[:64, :296] > il0[:64, :296]).mean() > 0.9 and np.array_equal(il[64:], il0[64:]) and np.array_equal(il[:, 296:], il0[:, 296:])
        nine = _three_way(ctx, d, p0, pp0, il0, srce, SX, sz, gz, nt, [(0, 9)], "9 steps")
        split = _three_way(ctx, d, p0, pp0, il0, srce, SX, sz, gz, nt, [(0, 5), (5, 4)], "5 + 4 steps")
        assert_bit_equal(split.traces(), nine.traces(), "5 + 4 vs 9: trace rows")
        assert_bit_equal(split.illum(), nine.illum(), "5 + 4 vs 9: accumulator")


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", [dict(two_step=-1), dict(two_step=4)], ids=["one-step", "pipeline"])
@pytest.mark.parametrize("exp", [-66, 60])
def test_dev_record_illum_steps_with_subnormal_and_overflowing_squares(exp, tuning):
    """Entry fields times 2^-66 (every square is subnormal or zero) and times 2^60 (every square overflows): no flush, no trap, the same
    bits as the two loops it combines."""
    nt = 9
    d = _deck(8, nt)
    p0, pp0 = random_fields(d, 5)
    p0, pp0 = np.ldexp(p0, exp).astype(np.float32), np.ldexp(pp0, exp).astype(np.float32)
    il0 = np.zeros((NXE, NZE), np.float32)
    srce = np.ldexp(O.ricker_wavelet(nt, 0.001, 30.0), exp).astype(np.float32)
    ctx = F.FDWave(*_args(d), compat=True, device=0)
    ctx.set_tuning(**tuning)
    sz, gz = (223, 224) if tuning["two_step"] == 4 else (255, 256)
    r = _three_way(ctx, d, p0, pp0, il0, srce, SX, sz, gz, nt, [(0, 9)], f"fields x 2^{exp} {tuning}")
    c = V.classify(r.illum()[:64, :296])
    if exp < 0:
        assert c["subnormal"] > 1000 and c["normal"] == 0 and c["large"] == 0, c
    else:
        assert c["inf"] > 1000, c
    assert np.count_nonzero(r.traces()[:9]) > 9 * LIVE // 2


WIDE = (150, 1300, 20, 24)      # the wide grid of tests/test_kernel_census.py: six pipeline strips, four chunks of 43 rows


def _pipe_tiles(ctx, nxe, nze, nxb, nzb, sx, sz, gz):
    """The wave-pipeline kernel's tiles on a small grid (chunks of 43 rows, strips of 56 owned cells of four columns) and, restating
    pipe_lean (csrc/fdw_stepn.hip) for the RTM forward pass with recording, which of them run the lean bodies."""
    xlim, zlim, ztap = ctx.extents()
    h, ns, pitch = 4, 4, ctx.pitch
    lap = (h, xlim - h, h, zlim - h)                      # rows / columns with a Laplacian in compat extents
    nstrip = -(-(pitch // 4) // (64 - 2 * ns))
    lean, full = [], []
    for xa in range(0, xlim, 43):
        xe = min(xa + 43, xlim)
        for zb in range(nstrip):
            c0 = (zb * (64 - 2 * ns) - ns) * 4
            c1 = c0 + 256
            lo, hi = xa - (ns - 1) * h - h - ns * (h + 1), xe + (ns - 1) * (2 * h + 1) + 2 * h + 16
            ok = c0 >= lap[2] and c1 <= min(lap[3], zlim) and lo >= lap[0] and hi <= min(lap[1], xlim, nxe) and c0 >= ztap
            ok = ok and not (c0 <= sz < c1 and xa - ns * h <= sx < xe + ns * h)
            ok = ok and not (c0 + 4 * ns <= gz < c1 - 4 * ns)
            (lean if ok else full).append((xa, zb))
    return lean, full


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
def test_dev_record_illum_steps_on_lean_and_full_pipeline_tiles(numerics):
    """A grid on which the pipeline kernel runs both bodies: the tiles that own the receiver column, hold the source, or touch the frame or
    the damped strip take the full body (recording in it), the others the lean ones (accumulating only)."""
    nxe, nze, nxb, nzb = WIDE
    nt = 9
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=5, dx=10.0, dz=12.5)
    sx, sz, gz = 56, 509, 512
    p0, pp0 = random_fields(d, 7, amp=0.01)
    il0 = (0.5 + np.random.default_rng(9).random((nxe, nze))).astype(np.float32)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0 + np.float32(3.0)
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(two_step=4)
    assert ctx.steps_per_pass() == 4
    lean, full = _pipe_tiles(ctx, nxe, nze, nxb, nzb, sx, sz, gz)
    assert len(lean) >= 2 and len(full) >= 2, (lean, full)
    gz_strip = [zb for zb in range(6) if (zb * 56 - 4) * 4 + 16 <= gz < (zb * 56 - 4) * 4 + 256 - 16]
    assert len(gz_strip) == 1 and any(zb == gz_strip[0] for _, zb in full) and any(xa == 43 and zb != gz_strip[0] for xa, zb in lean)
    xlim, zlim, _ = ctx.extents()
    for calls in ([(0, 8)], [(0, 9)], [(0, 4), (4, 5)]):
        r = _three_way(ctx, d, p0, pp0, il0, srce, sx, sz, gz, nt, calls, f"wide grid, numerics {numerics}, calls {calls}")
        il = r.illum()
        for xa, zb in lean[:2] + full[:2]:                                               # the accumulator moved under both bodies
            z0 = max((zb * 56) * 4, 0)
            assert (il[xa:xa + 43, z0:z0 + 224][:xlim - xa, :max(zlim - z0, 0)] > il0[xa:xa + 43, z0:z0 + 224][:xlim - xa, :max(zlim - z0, 0)]).mean() > 0.9
        assert (r.traces()[:sum(n for _, n in calls)] != 9.0).all()


@pytest.mark.gpu
def test_dev_record_illum_steps_refusals():
    import torch
    d = _deck(8, 9)
    p0, pp0 = random_fields(d, 5)
    srce = O.ricker_wavelet(9, 0.001, 30.0)
    ctx = F.FDWave(*_args(d), compat=True, device=0)
    r = _Run(ctx, d, p0, pp0, np.zeros((NXE, NZE), np.float32), srce, 9)
    a = (r.ptrs(), r.v2.data_ptr(), r.srce.data_ptr(), SX, 255)
    for rec, il in ((None, r.il.data_ptr()), (r.rec.data_ptr(), None)):                  # one alone: the existing entry points
        with pytest.raises(F.FdwError) as e:
            ctx.dev_record_illum_steps(*a, 256, rec, il, 0, 4)
        assert e.value.code == -1
    with pytest.raises(F.FdwError) as e:
        ctx.dev_record_illum_steps(*a, 296, r.rec.data_ptr(), r.il.data_ptr(), 0, 4)     # gz outside [0, zlim)
    assert e.value.code == -1
    for other in (F.FDWave(*_args(d), compat=True, device=0, slab=(0, 40)), F.FDWave(*_args(d), compat=True, device=0, dialect=1)):
        with pytest.raises(F.FdwError) as e:
            other.dev_record_illum_steps(*a, 256, r.rec.data_ptr(), r.il.data_ptr(), 0, 4)
        assert e.value.code == -5
    torch.cuda.synchronize()
    assert (r.traces() == 9.0).all()                                                     # refused before anything was enqueued


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the physics
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_residual_migration_images_the_interface():
    """two_layer_case() of tests/test_record.py: data recorded in the two-layer model, migrated in the homogeneous one.  shot_residual equals
    the three-loop construction (record, record, subtract, shot) bit for bit and images the interface; the misfit is positive, and exactly 0
    for data from the homogeneous model itself."""
    args, nx, nz, nb, iface, v2, h2, shots = two_layer_case()
    ctx = F.FDWave(*args, compat=True, device=0)
    nt = args[5]
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    sz = gz = nb + 2
    img = np.zeros((nx, nz), np.float32)
    want = np.zeros((nx, nz), np.float32)
    for sx in shots:
        data = ctx.record_shot(v2, sx, sz, gz, srce)
        hom = ctx.record_shot(h2, sx, sz, gz, srce)
        refl = data - hom
        got = ctx.shot_residual(h2, sx, sz, gz, srce, data)
        assert_bit_equal(got["resid"], refl, f"residual = reflection data, shot at {sx}")
        one = ctx.shot(h2, sx, sz, gz, srce, refl)
        assert_bit_equal(got["image"], one, f"image, shot at {sx}")
        img, want = img + got["image"], want + one
        assert F.gather_misfit(got["resid"]) > 0.0
        zero = ctx.shot_residual(h2, sx, sz, gz, srce, hom)
        assert F.gather_misfit(zero["resid"]) == 0.0 and not zero["image"].any()
    assert_bit_equal(img, want, "stacked image")
    assert interface_hits(F.image_laplacian(img, 10.0, 10.0), nz, nb, iface) >= 0.9


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the programs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _two_shot_deck(path, vp, extra=""):
    nx, nz = vp.shape
    (path / "models").mkdir(parents=True)
    (path / "output").mkdir()
    vp.tofile(path / "models" / "vp.bin")
    (path / "input.dat").write_text("tmpdir=./output\nvpfile=./models/vp.bin\ndatfile=./models/dobs.bin\n"
                                    f"nz={nz}\nnx={nx}\nnt=47\ndz=10\ndx=10\ndt=0.001\nfpeak=25.\nns=2\nsz=1\nfsx=5\nds=20\ngz=2\n"
                                    "nxb=10\nnzb=9\nrnd=1\nfac=0.75\norder=8\n" + extra)


def _run(exe, path, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("FDW_SHOT_WORKERS", "FDW_SLABS", "FDW_GPUS", "FDW_NO_SHOT_BATCH")}
    env.update(env_extra or {})
    r = subprocess.run([os.path.join(BIN, exe), "./input.dat"], cwd=path, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    out = path / "output"
    return {name: (out / name).read_bytes() for name in sorted(os.listdir(out))}, r


@pytest.mark.gpu
def test_rtm_model_then_rtm_code_resid(tmp_path):
    nx, nz, nxb, nzb, nt, ns, ds = 50, 37, 10, 9, 47, 2, 20
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    rng = np.random.default_rng(11)
    vp = (1500 + 2500 * np.linspace(0, 1, nz, dtype=np.float32)[None, :] + 100 * rng.standard_normal((nx, nz))).astype(np.float32)
    other = (vp * np.float32(1.1)).astype(np.float32)                                     # the "true" model of the second datfile
    plain_files = ["dir.image", "dir.image_lap", "dir.snapr", "dir.snaps", "dir.snaps_rec"]

    # 1. data modelled in the migration model itself: zero residual, zero misfit, zero image
    a = tmp_path / "same"
    _two_shot_deck(a, vp, "resid=1\n")
    _run("rtm_model", a)                                                                 # ignores the key
    dobs_same = (a / "models" / "dobs.bin").read_bytes()
    files, r = _run("rtm_code", a, {"FDW_TIMING": "1"})
    assert sorted(files) == sorted(plain_files + ["dir.resid", "dir.misfit"])
    assert len(files["dir.resid"]) == ns * nx * nt * 4 and not any(files["dir.resid"])
    assert files["dir.misfit"] == np.zeros(ns, np.float64).tobytes()
    assert len(files["dir.image"]) == nx * nz * 4 and not any(files["dir.image"])
    assert "## resid = 1" in r.stdout and "## misfit = 0.000000000e+00" in r.stdout and "residual" in r.stderr

    # 2. data from another model: dir.resid and dir.image equal the API composition on the program's own border models
    b = tmp_path / "other"
    _two_shot_deck(b, other)
    _run("rtm_model", b)
    dobs = np.fromfile(b / "models" / "dobs.bin", np.float32).reshape(ns, nx, nt)
    assert (b / "models" / "dobs.bin").read_bytes() != dobs_same
    plain, _ = _run("rtm_code", b)                                                       # without the key: today's files
    assert sorted(plain) == plain_files
    runs = {}
    for name, extra, env in (("resid", "resid=1\n", {}), ("gpus2", "resid=1\ngpus=2\n", {}), ("nobatch", "resid=1\n", {"FDW_NO_SHOT_BATCH": "1"}),
                             ("illum", "resid=1\nillum=1\n", {}), ("illum-nobatch", "resid=1\nillum=1\n", {"FDW_NO_SHOT_BATCH": "1"}), ("off", "resid=0\n", {})):
        c = tmp_path / name
        _two_shot_deck(c, vp, extra)
        (c / "models" / "dobs.bin").write_bytes(dobs.tobytes())
        runs[name], _ = _run("rtm_code", c, env)
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    ctx.model_resident(vp)
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    img, ill = np.zeros((nx, nz), np.float32), np.zeros((nx, nz), np.float32)
    resid, misfit = np.zeros((ns, nx, nt), np.float32), np.zeros(ns, np.float64)
    for s in range(ns):
        vel = ctx.dev_extendvel_linear(s * ctx.border_draws(), want_vel=True)            # shot s: draws [s T, (s + 1) T) of the unseeded stream
        v2 = (vel * vel).astype(np.float32)
        sx, sz, gz = 5 + s * ds + nxb, 1 + nzb, 2 + nzb
        resid[s] = dobs[s] - ctx.record_shot(v2, sx, sz, gz, srce)
        im, il = ctx.shot(v2, sx, sz, gz, srce, resid[s], want_illum=True)
        img, ill = img + im, ill + il
        misfit[s] = F.gather_misfit(resid[s])
    assert np.count_nonzero(resid) > ns * nx and img.any() and (misfit > 0).all()
    for name in ("resid", "gpus2", "nobatch", "illum", "illum-nobatch"):
        got = runs[name]
        assert got["dir.resid"] == resid.tobytes(), name
        assert got["dir.misfit"] == misfit.tobytes(), name
        assert got["dir.image"] == img.tobytes(), name
        for f in plain_files[1:]:
            assert got[f] == plain[f], (name, f)
    for name in ("illum", "illum-nobatch"):
        assert sorted(runs[name]) == sorted(plain_files + ["dir.resid", "dir.misfit", "dir.illum", "dir.image_illum"])
        assert runs[name]["dir.illum"] == ill.tobytes(), name
        assert runs[name]["dir.image_illum"] == F.image_compensate(img, ill, 1e-3).tobytes(), name
    # resid=0 and no key at all: the same files and the same bytes as on the same datfile without the feature
    c = tmp_path / "nokey"
    _two_shot_deck(c, vp)
    (c / "models" / "dobs.bin").write_bytes(dobs.tobytes())
    nokey, _ = _run("rtm_code", c)
    assert sorted(nokey) == sorted(runs["off"]) == plain_files
    for f in plain_files:
        assert nokey[f] == runs["off"][f], f
    assert nokey["dir.image"] != img.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("illum", [False, True], ids=["resid", "resid-illum"])
def test_rtm_code_resid_in_groups_of_two_shots(tmp_path, illum):
    """resid=1 under a batch budget that lets fdw_shot_batch_max be 2 (groups {0, 1}, {2, 3}, {4} through fdw_shot_batch_residual): dir.resid
    and dir.misfit in shot order and dir.image (with illum=1 also dir.illum, dir.image_illum) against the oracle's shot loop, every file
    against the run one shot at a time."""
    import batch_groups as G
    extra = "resid=1\n" + ("illum=1\n" if illum else "")
    nx, nz, nxb, nzb, nt, ns, vp, d_obs, _ = G.five_shot_case(tmp_path / "grouped", extra=extra)
    G.five_shot_case(tmp_path / "single", extra=extra)
    grouped, r = G.run_program("rtm_code", tmp_path / "grouped", G.group_env(nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt))
    G.assert_grouped(r.stderr, "fdw_shot_batch_residual")
    want = G.five_shot_oracle()
    img = G.stack(want["r_image"])
    assert_bit_equal(np.frombuffer(grouped["dir.resid"], np.float32).reshape(ns, nx, nt), want["resid"], "dir.resid, shot order")
    misfit = np.array([misfit_formula(want["resid"][s]) for s in range(ns)], np.float64)
    assert grouped["dir.misfit"] == misfit.tobytes() and len(set(misfit)) == ns and (misfit > 0).all()
    assert_bit_equal(np.frombuffer(grouped["dir.image"], np.float32).reshape(nx, nz), img, "dir.image")
    assert np.count_nonzero(want["resid"] != d_obs) > ns * nx
    if illum:
        ill = G.stack(want["illum"])
        assert_bit_equal(np.frombuffer(grouped["dir.illum"], np.float32).reshape(nx, nz), ill, "dir.illum")
        assert grouped["dir.image_illum"] == F.image_compensate(img, ill, 1e-3).tobytes()
    single, r1 = G.run_program("rtm_code", tmp_path / "single", {"FDW_NO_SHOT_BATCH": "1", "FDW_TIMING": "1"})
    G.assert_grouped(r1.stderr, "one by one, fdw_shot_residual", 1)
    assert sorted(grouped) == sorted(single) and ("dir.illum" in single) == illum
    for name in single:
        assert grouped[name] == single[name], name
    assert G.without_exec_time(r.stdout) == G.without_exec_time(r1.stdout)

"""Source illumination for a batch of shots (fdw_shot_batch_illum, FDWave.shot_batch(want_illum=True), rtm_code's illum=1 on small decks):
one launch per time step advances every shot and accumulates every shot's illumination into its own field.  The reference throughout is the
per-shot entry point (fdw_shot_illum / fdw_shot_resident_illum), bit for bit -- itself pinned to the chained oracle by tests/test_illum.py;
one case per numerics goes to the oracle's restatement directly."""
import os
import subprocess

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from conftest import ROOT, assert_bit_equal, make_deck
from oracle import oracle as O
from test_illum import _run_rtm_code, illum_restatement

# the compat deck of tests/test_illum.py with a wider x border: nxb = 3 puts receiver rows beyond xlim = 64, which the batched launches do
# not cover (fdw_receivers_stepped); nxb = 8 keeps them below it.  nze = 301 -> zlim = 296; nzb = 10 -> ztap = 8; dx != dz.
NXE, NZE, NXB, NZB, NT = 69, 301, 8, 10, 23
NX, NZ = NXE - 2 * NXB, NZE - 2 * NZB
SX0, SZ, GZ = 30, 223, 220      # receivers 3 cells from the sources: the image changes within NT steps


def _deck(order):
    return make_deck(NXE, NZE, NXB, NZB, NT, seed=3, order=order, dx=10.0, dz=12.5)


def _args(d):
    return (d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"])


def _inputs(ns, seed=0):
    """Per-shot models, gathers, entry images (non-zero) and entry illuminations (positive), the interior model of the resident case."""
    rng = np.random.default_rng(100 + seed)
    v2_all = np.stack([make_deck(NXE, NZE, NXB, NZB, NT, seed=20 + s, dx=10.0, dz=12.5)["v2"] for s in range(ns)])
    d_obs = rng.standard_normal((ns, NX, NT)).astype(np.float32)
    im0 = rng.standard_normal((ns, NX, NZ)).astype(np.float32)
    il0 = (0.5 + rng.random((ns, NX, NZ))).astype(np.float32)
    vp = (1500 + 1000 * rng.random((NX, NZ))).astype(np.float32)
    return v2_all, d_obs, im0, il0, vp


def _one_by_one(ctx, ns, dsx, srce, d_obs, im0, il0, v2_all=None, draw_offset=0):
    """The per-shot calls the batch must reproduce: host models through shot(), the resident model through shot_resident()."""
    imgs, ils = [], []
    for s in range(ns):
        if v2_all is not None:
            im, il = ctx.shot(v2_all[s], SX0 + s * dsx, SZ, GZ, srce, d_obs[s], imloc=im0[s], want_illum=True, illum=il0[s])
        else:
            ctx.dev_extendvel_linear(draw_offset + s * ctx.border_draws())
            im, il = ctx.shot_resident(SX0 + s * dsx, SZ, GZ, srce, d_obs[s], imloc=im0[s], want_illum=True, illum=il0[s])
        imgs.append(im)
        ils.append(il)
    return np.stack(imgs), np.stack(ils)


def test_shot_batch_illum_is_exported():
    import ctypes as C
    L = F.lib()
    assert hasattr(L, "fdw_shot_batch_illum")
    # the batch budget and the part count (tests/test_batch_parts.py), with their signatures
    assert L.fdw_set_batch_budget.argtypes == [C.c_void_p, C.c_size_t] and L.fdw_set_batch_budget.restype is C.c_int
    assert L.fdw_batch_parts.argtypes == [C.c_void_p] and L.fdw_batch_parts.restype is C.c_int


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("order", [2, 4, 6, 8])
def test_batch_illum_equals_the_shots_one_by_one(order, numerics):
    d = _deck(order)
    srce = O.ricker_wavelet(NT, 0.001, 30.0) * 1000.0
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    assert ctx.shot_batch_max() > 1                       # the batched launches really run (batch_ok holds on this geometry)
    xlim, zlim, _ = O.extents(NXE, NZE, NZB, True)
    assert ctx.extents()[:2] == (xlim, zlim) == (64, 296)
    for ns in (2, 5):
        v2_all, d_obs, im0, il0, vp = _inputs(ns, ns)
        for dsx in (3, -2):
            what = f"order {order} numerics {numerics}, {ns} shots, dsx {dsx}"
            # host models
            img, il = ctx.shot_batch(ns, SX0, dsx, SZ, GZ, srce, d_obs, v2_all=v2_all, imloc=im0, want_illum=True, illum=il0)
            want_img, want_il = _one_by_one(ctx, ns, dsx, srce, d_obs, im0, il0, v2_all=v2_all)
            assert_bit_equal(il, want_il, "illumination, host models, " + what)
            assert_bit_equal(img, want_img, "image, host models, " + what)
            assert_bit_equal(img, ctx.shot_batch(ns, SX0, dsx, SZ, GZ, srce, d_obs, v2_all=v2_all, imloc=im0), "image vs fdw_shot_batch, " + what)
            # vacuity: every shot added something of its own
            for s in range(ns):
                assert (il[s] > il0[s]).any(), what
                for t in range(s):
                    assert not np.array_equal(il[s] - il0[s], il[t] - il0[t]), what
            assert not np.array_equal(img, im0)
            if (order, ns, dsx) == (8, 2, 3):             # one case per numerics against the oracle's restatement
                orc = O.Oracle(*_args(d), compat=True, numerics=numerics)
                for s in range(ns):
                    entry = np.pad(il0[s], ((NXB, NXB), (NZB, NZB)))
                    want, _, _ = illum_restatement(orc, v2_all[s], SX0 + s * dsx, SZ, srce, xlim, zlim, il0=entry)
                    assert_bit_equal(il[s], want[NXB:NXB + NX, NZB:NZB + NZ], f"shot {s} vs the restatement, " + what)
            # the resident interior model, borders drawn on the device from draws [(7 + s) T, ...)
            ctx.model_resident(vp)
            off = 7 * ctx.border_draws()
            img, il = ctx.shot_batch(ns, SX0, dsx, SZ, GZ, srce, d_obs, draw_offset=off, imloc=im0, want_illum=True, illum=il0)
            want_img, want_il = _one_by_one(ctx, ns, dsx, srce, d_obs, im0, il0, draw_offset=off)
            assert_bit_equal(il, want_il, "illumination, resident model, " + what)
            assert_bit_equal(img, want_img, "image, resident model, " + what)
            assert (il > il0).any()
    # from zero when no accumulator is handed over
    img, il = ctx.shot_batch(2, SX0, 3, SZ, GZ, srce, d_obs[:2], v2_all=v2_all[:2], want_illum=True)
    _, want_il = _one_by_one(ctx, 2, 3, srce, d_obs[:2], np.zeros_like(im0[:2]), np.zeros_like(il0[:2]), v2_all=v2_all[:2])
    assert_bit_equal(il, want_il, "illumination from zero")


@pytest.mark.gpu
@pytest.mark.parametrize("order,tuning", [(10, {}), (8, dict(two_step=4))], ids=["order10", "forced-pipeline"])
def test_batch_illum_fallback_runs_the_shots_one_by_one(order, tuning):
    """Contexts whose regime the batched launches do not cover (orders above 8; the wave pipeline): the same bytes as the per-shot calls."""
    d = _deck(order)
    srce = O.ricker_wavelet(NT, 0.001, 30.0) * 1000.0
    ctx = F.FDWave(*_args(d), compat=True, device=0)
    ctx.set_tuning(**tuning)
    assert ctx.shot_batch_max() == 1
    ns, dsx = 3, 3
    v2_all, d_obs, im0, il0, vp = _inputs(ns, 9)
    img, il = ctx.shot_batch(ns, SX0, dsx, SZ, GZ, srce, d_obs, v2_all=v2_all, imloc=im0, want_illum=True, illum=il0)
    want_img, want_il = _one_by_one(ctx, ns, dsx, srce, d_obs, im0, il0, v2_all=v2_all)
    assert_bit_equal(il, want_il, "illumination")
    assert_bit_equal(img, want_img, "image")
    assert (il > il0).any()
    ctx.model_resident(vp)
    img, il = ctx.shot_batch(ns, SX0, dsx, SZ, GZ, srce, d_obs, draw_offset=11, imloc=im0, want_illum=True, illum=il0)
    want_img, want_il = _one_by_one(ctx, ns, dsx, srce, d_obs, im0, il0, draw_offset=11)
    assert_bit_equal(il, want_il, "illumination, resident model")
    assert_bit_equal(img, want_img, "image, resident model")


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
def test_batch_illum_at_the_edges_of_the_value_domain(numerics):
    """The wavelet times 2^60: squares overflow to +inf around the sources; times 2^-66: squares land in the subnormal range.  A batch
    shares one wavelet between its shots, so the two scales are two batches; each equals its per-shot calls bit for bit (from a zero
    illumination, so that a subnormal sum is not absorbed by the entry value)."""
    d = _deck(8)
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    assert ctx.shot_batch_max() > 1
    ns, dsx = 3, 3
    v2_all, d_obs, im0, _, _ = _inputs(ns, 4)
    il0 = np.zeros((ns, NX, NZ), np.float32)
    base = O.ricker_wavelet(NT, 0.001, 30.0) * 1000.0
    seen = {}
    for k in (60, -66):
        srce = (base * np.float32(2.0) ** np.float32(k)).astype(np.float32)
        with np.errstate(all="ignore"):
            img, il = ctx.shot_batch(ns, SX0, dsx, SZ, GZ, srce, d_obs, v2_all=v2_all, imloc=im0, want_illum=True, illum=il0)
            want_img, want_il = _one_by_one(ctx, ns, dsx, srce, d_obs, im0, il0, v2_all=v2_all)
        assert_bit_equal(il, want_il, f"illumination, wavelet x 2^{k}")
        assert_bit_equal(img, want_img, f"image, wavelet x 2^{k}")
        seen[k] = il
    for s in range(ns):      # vacuity: the per-shot results hold what the case is about, in every shot
        assert np.isposinf(seen[60][s]).any()
        sub = (np.abs(seen[-66][s]) < np.float32(2.0 ** -126)) & (seen[-66][s] != 0)
        assert sub.any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the program
# ---------------------------------------------------------------------------------------------------------------------------------------
def _four_shot_deck(tmp_path, extra=""):
    nx, nz, nxb, nzb, nt, ns, ds = 50, 37, 10, 9, 47, 4, 9
    rng = np.random.default_rng(11)
    vp = (1500 + 2500 * np.linspace(0, 1, nz, dtype=np.float32)[None, :] + 100 * rng.standard_normal((nx, nz))).astype(np.float32)
    (tmp_path / "models").mkdir(parents=True)
    (tmp_path / "output").mkdir()
    vp.tofile(tmp_path / "models" / "vp.bin")
    rng.standard_normal((ns, nx, nt)).astype(np.float32).tofile(tmp_path / "models" / "dobs.bin")
    (tmp_path / "input.dat").write_text("tmpdir=./output\nvpfile=./models/vp.bin\ndatfile=./models/dobs.bin\n"
                                        f"nz={nz}\nnx={nx}\nnt={nt}\ndz=10\ndx=10\ndt=0.001\nfpeak=25.\nns={ns}\nsz=1\nfsx=5\nds={ds}\ngz=2\n"
                                        f"nxb={nxb}\nnzb={nzb}\nrnd=1\nfac=0.75\norder=8\n" + extra)
    return nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt


@pytest.mark.gpu
def test_rtm_code_illum_through_the_batch_path(tmp_path):
    """illum=1 with the default environment (a batch of shots per launch) against FDW_NO_SHOT_BATCH=1 (one by one): the same five files."""
    nxe, nze, nxb, nzb, nt = _four_shot_deck(tmp_path / "batch", "illum=1\n")
    _four_shot_deck(tmp_path / "single", "illum=1\n")
    assert "FDW_NO_SHOT_BATCH" not in os.environ, "the default run would not batch"
    batch, num_batch = _run_rtm_code(tmp_path / "batch")
    # the default run took the batch path, the other did not: the program says so under FDW_TIMING
    exe = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin", "rtm_code")
    for sub, env, word in (("batch", {}, "fdw_shot_batch_illum"), ("single", {"FDW_NO_SHOT_BATCH": "1"}, "one by one")):
        r = subprocess.run([exe, "./input.dat"], cwd=tmp_path / sub, capture_output=True, text=True, env=dict(os.environ, FDW_TIMING="1", **env), timeout=300)
        assert r.returncode == 0, r.stderr
        line = [ln for ln in r.stderr.splitlines() if "shots per launch sequence" in ln]
        assert len(line) == 1 and word in line[0], r.stderr
        if sub == "batch":
            assert "up to 4 " in line[0], line           # all four shots of the deck in one batch
    single, num_single = _run_rtm_code(tmp_path / "single", {"FDW_NO_SHOT_BATCH": "1"})
    names = ["dir.illum", "dir.image_illum", "dir.image", "dir.image_lap"]
    for name in names:
        assert batch[name] == single[name], name
    assert num_batch == num_single
    assert np.frombuffer(batch["dir.illum"], np.float32).max() > 0 and np.abs(np.frombuffer(batch["dir.image"], np.float32)).max() > 0
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    assert ctx.shot_batch_max() > 1

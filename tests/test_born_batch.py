"""Born modelling driven by a line source, and batches of Born shots (fdwave.h, the sub-section after "Born modelling"):
fdw_dev_born_line_steps, fdw_born_shot_line, fdw_born_shot_batch, fdw_born_shot_line_batch, and rtm_model bornfile= in groups of shots.

The line restatement (tests/born_line_restatement.py) is tests/born_restatement.py with the point add replaced by the line add; the GPU is
held to both bit for bit.  Decks, reflectivities (NaN words outside C and in the padding columns) and the device harness are those of
tests/test_born.py.  In every batch the shots differ in source row or line gather AND in model, so a mixed-up shot index changes bytes; the
shots from rest are asserted to carry non-zero scattered samples on at least half of every shot's traces, so no equality is between zeros."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from born_line_restatement import born_line_restatement
from born_restatement import DTT, FIELD, born_cells, born_restatement, embed_m
from conftest import ROOT, assert_bit_equal, make_deck, random_fields
from oracle import oracle as O
from test_born import CONFIGS, DECKS, NT, PAD_NAN, Device, reflectivity
from test_line_source import args_of, extents_of, line_restatement
from test_stepn_isa_budget import isa  # noqa: F401  (a fixture)
from value_classes import assert_same_nonfinite

EINVAL, ESTATE = -1, -5
KINDS = pytest.mark.parametrize("kind", [FIELD, DTT], ids=["field", "dtt"])
NUMERICS = pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])


def nsrc_of(d):
    return min(d["nxe"] - 2 * d["nxb"], extents_of(d)[0] - d["nxb"])


@functools.lru_cache(maxsize=None)
def line_case(deck, order, numerics, kind, place=None, nsteps=NT):
    """Deck, entry fields of both pairs, m, the line gather w [NT][nx] and the restatement's answer; never modified.  Rows >= nsrc of w hold
    NaNs where the deck has any (static-rows): they are ignored, so the answer is finite."""
    nxe, nze, nxb, nzb, _ = DECKS[deck]
    d = make_deck(nxe, nze, nxb, nzb, NT, seed=3, order=order, dx=10.0, dz=12.5)
    nx = nxe - 2 * nxb
    u0, u1 = random_fields(d, 5, amp=0.1)
    du0, du1 = random_fields(d, 6, amp=0.05)
    m = reflectivity(d)
    w = np.random.default_rng(21).standard_normal((NT, nx)).astype(np.float32)
    w[:, nsrc_of(d):] = np.nan
    sz, gz = place or (d["sz"], d["gz"])
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    want = born_line_restatement(orc, d, d["v2"], m, kind, sz, gz, w, u0, u1, du0, du1, nsteps=nsteps)
    for a in (u0, u1, du0, du1, m, w, d["v2"]) + tuple(want.values()):
        a.setflags(write=False)
    return d, u0, u1, du0, du1, m, w, (sz, gz), want


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement's guards, the built library, the program's refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
@NUMERICS
@pytest.mark.parametrize("deck", ["87x70", "static-rows"])
def test_line_restatement_background_chain_is_the_line_chain(deck, numerics):
    d, u0, u1, du0, du1, m, w, (sz, gz), want = line_case(deck, 8, numerics, DTT)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    ref = line_restatement(orc, d, d["v2"], w, sz, gz, u0, u1)
    bare = born_line_restatement(orc, d, d["v2"], m, DTT, sz, gz, w, u0, u1, du0, du1, scatter=False)
    for r in (bare, want):
        assert_bit_equal(r["U_PP"], ref["PP"], "background PP")
        assert_bit_equal(r["U_P"], ref["P"], "background P")
        assert_bit_equal(r["rec0"].T, ref["data"], "background gather")
    point = born_restatement(orc, d, d["v2"], m, DTT, d["sx"], sz, gz, np.zeros(NT, np.float32), u0, u1, du0, du1, scatter=False)
    assert_bit_equal(bare["DU_PP"], point["DU_PP"], "scattered pair without the scatter: the source-free chain")
    assert np.isnan(w).any() == (deck == "static-rows")
    assert all(np.isfinite(v).all() for v in want.values()), "rows >= nsrc of the line gather are ignored"
    assert (want["DU_PP"] != bare["DU_PP"]).mean() > 0.3 and (want["rec"] != bare["rec"]).any()


@KINDS
def test_line_restatement_zero_m_from_rest_gives_zero_words(kind):
    d, w = line_case("87x70", 8, 0, kind)[0], line_case("87x70", 8, 0, kind)[6]
    r = born_line_restatement(O.Oracle(*args_of(d), compat=True), d, d["v2"], np.zeros((d["nxe"], d["nze"]), np.float32), kind, d["sz"], d["gz"], w)
    for k in ("DU_P", "DU_PP", "rec"):
        assert not r[k].view(np.uint32).any(), k
    assert r["rec0"].any() and r["U_PP"].any()


def test_the_four_symbols_are_exported_and_mirrored():
    L = F.lib()
    for name in ("fdw_dev_born_line_steps", "fdw_born_shot_line", "fdw_born_shot_batch", "fdw_born_shot_line_batch"):
        assert hasattr(L, name), name
    for name in ("dev_born_line_steps", "born_shot_line", "born_shot_batch", "born_shot_line_batch"):
        assert hasattr(F.FDWave, name), name
    header = open(os.path.join(ROOT, "include", "fdwave.h")).read()
    for name in ("fdw_dev_born_line_steps", "fdw_born_shot_line(", "fdw_born_shot_batch(", "fdw_born_shot_line_batch("):
        assert "int " + name in header, name


def test_line_born_kernels_exist_in_both_numerics_without_scratch(isa):      # noqa: F811
    names = [k for k in isa if "fdw_step_line_born_kernel" in k]
    for h in (1, 2, 3, 4):
        for num in (0, 1):
            assert any(f"fdw_step_line_born_kernelILi{h}ELi2ELi{num}EEEv" in k for k in names), (h, num, names)
    for pf in (1, 3):
        assert any(f"fdw_step_line_born_kernelILi4ELi{pf}ELi0EEEv" in k for k in names), pf
    assert len(names) == 10, names
    for k in names + [k for k in isa if "fdw_step_born_kernel" in k]:
        meta = isa[k][0]
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (k, meta)
        assert not any(mn.startswith("scratch_") for mn, _ in isa[k][1]), k


BIN = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin")
PNX, PNZ, PNT, PNB, PNS, PFSX, PDS = 30, 24, 40, 8, 5, 3, 3


def _write_deck(tmp_path, extra, m=None):
    """A five-shot deck small enough for fdw_shot_batch_max to hold all its shots."""
    vp = (1500 + 1000 * np.random.default_rng(5).random((PNX, PNZ))).astype(np.float32)
    vp.tofile(tmp_path / "vp.bin")
    if m is not None:
        np.asarray(m, np.float32).tofile(tmp_path / "m.bin")
    (tmp_path / "input.dat").write_text(f"vpfile=./vp.bin\ndatfile=./data.bin\nnz={PNZ}\nnx={PNX}\nnt={PNT}\ndz=10\ndx=10\ndt=0.001\nfpeak=60\n"
                                        f"ns={PNS}\nsz=1\nfsx={PFSX}\nds={PDS}\ngz=2\nnxb={PNB}\nnzb={PNB}\nfac=0.75\norder=8\n" + extra)
    return vp


def _run_rtm_model(tmp_path, env=None):
    base = {k: v for k, v in os.environ.items() if k not in ("FDW_SLABS", "FDW_GPUS", "FDW_SHOT_WORKERS", "FDW_NO_SHOT_BATCH", "FDW_TIMING")}
    base.update(env or {})
    return subprocess.run([os.path.join(BIN, "rtm_model"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=base)


@pytest.mark.parametrize("extra,env,word", [("slabs=2\n", {}, "slabs"), ("gpus=2\n", {}, "gpus"), ("", dict(FDW_SLABS="2"), "slabs"),
                                            ("", dict(FDW_GPUS="2"), "gpus"), ("born_kind=2\n", {}, "born_kind")])
def test_rtm_model_refusals_are_unchanged_on_a_batchable_deck(tmp_path, extra, env, word):
    _write_deck(tmp_path, "bornfile=./m.bin\nborn_bg=./bg.bin\n" + extra, m=np.zeros((PNX, PNZ)))
    before = sorted(os.listdir(tmp_path))
    r = _run_rtm_model(tmp_path, env)
    assert r.returncode != 0 and "bornfile" in r.stderr and word in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before
    _write_deck(tmp_path, "bornfile=./m.bin\n", m=np.zeros(PNX * PNZ - 1))      # a short reflectivity file
    before = sorted(os.listdir(tmp_path))
    r = _run_rtm_model(tmp_path)
    assert r.returncode != 0 and "bornfile" in r.stderr, r.stderr
    assert sorted(os.listdir(tmp_path)) == before


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_dev_born_line_steps on device arrays
# ---------------------------------------------------------------------------------------------------------------------------------------
class LineDevice(Device):
    """tests/test_born.py's device state with the line gather [NT][nx] where the wavelet was."""

    def born(self, kind, place, it0, nsteps, first=False, rec=True, rec0=True, swap=False, stream=None):
        p = {k: t.data_ptr() for k, t in self.f.items()}
        a, b, c, e = (p["u1"], p["u0"], p["du1"], p["du0"]) if swap else (p["u0"], p["u1"], p["du0"], p["du1"])
        sz, gz = place
        self.ctx.dev_born_line_steps(a, b, c, e, p["v2"], p["m"], kind, self.srce.data_ptr(), sz, gz, self.rec.data_ptr() if rec else None,
                                     self.rec0.data_ptr() if rec0 else None, it0, nsteps, first_pp_twice=first, stream=stream)


def check_line_run(ctx, c, kind, what, split=None, rec=True, rec0=True, nsteps=NT):
    """test_born.check_run for the line loop: both pairs, both gathers, m, v2, the line gather and the padding columns."""
    d, u0, u1, du0, du1, m, w, place, want = c
    dv = LineDevice(ctx, d, u0, u1, du0, du1, m, w)
    if split is None:
        dv.born(kind, place, 0, nsteps, rec=rec, rec0=rec0)
    else:
        dv.born(kind, place, 0, split, rec=rec, rec0=rec0)
        dv.born(kind, place, split, nsteps - split, first=True, rec=rec, rec0=rec0, swap=bool(split & 1))
    new, old = ("0", "1") if nsteps & 1 else ("1", "0")
    grec, grec0 = dv.gathers()
    pads = {k: dv.whole(k)[:, d["nze"]:] for k in dv.f}
    assert_bit_equal(dv.get("u" + new), want["U_PP"], "background newest, " + what)
    assert_bit_equal(dv.get("du" + new), want["DU_PP"], "scattered newest, " + what)
    assert_bit_equal(dv.get("u" + old, finalize=True), want["U_P"], "background older, " + what)
    assert_bit_equal(dv.get("du" + old, finalize=True), want["DU_P"], "scattered older, " + what)
    assert_bit_equal(grec[:nsteps], want["rec"][:nsteps] if rec else np.full_like(grec[:nsteps], 9.0), "scattered gather, " + what)
    assert_bit_equal(grec0[:nsteps], want["rec0"][:nsteps] if rec0 else np.full_like(grec0[:nsteps], -9.0), "background gather, " + what)
    assert (grec[nsteps:] == 9.0).all() and (grec0[nsteps:] == -9.0).all(), "rows outside the iterations run, " + what
    assert_same_nonfinite(dv.get("m"), m, "m is only read, " + what)
    assert_bit_equal(dv.get("v2"), d["v2"], "v2 is only read, " + what)
    assert_same_nonfinite(dv.srce.cpu().numpy(), w, "the line gather is only read, " + what)
    for k, p in pads.items():
        assert (p.view(np.uint32) == (PAD_NAN if k == "m" else 0)).all(), f"padding columns of {k}, " + what
    return dv


def assert_line_case_not_vacuous(c):
    d, _, _, _, _, m, w, _, want = c
    x0, x1, z0, z1 = born_cells(d)
    assert np.isfinite(m[x0:x1, z0:z1]).all() and np.isnan(m).sum() == m.size - (d["nxe"] - 2 * d["nxb"]) * (d["nze"] - 2 * d["nzb"])
    assert all(np.isfinite(v).all() for v in want.values()) and np.count_nonzero(want["rec"]) > 0.9 * want["rec"].size


@pytest.mark.gpu
@KINDS
@NUMERICS
@pytest.mark.parametrize("order,tuning", CONFIGS, ids=str)
def test_dev_born_line_steps_vs_restatement(order, tuning, numerics, kind):
    """Seven iterations from noise-filled pairs, in one call and as 4 + 3, on the four decks (the static-rows deck with NaNs in the rows
    >= nsrc of the line gather); the background pair also against fdw_dev_line_steps on a copy."""
    for deck, (_, _, _, _, xchunk) in DECKS.items():
        c = line_case(deck, order, numerics, kind)
        assert_line_case_not_vacuous(c)
        d, u0, u1, du0, du1, m, w, (sz, gz), want = c
        ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
        ctx.set_tuning(xchunk=xchunk, two_step=-1, **tuning)
        what = f"{deck} order {order} {tuning} numerics {numerics} kind {kind}"
        dv = check_line_run(ctx, c, kind, what)
        check_line_run(ctx, c, kind, what + ", 4 + 3", split=4)
        ref = LineDevice(ctx, d, u0, u1, du0, du1, m, w)
        ctx.dev_line_steps([ref.f["u0"].data_ptr(), ref.f["u1"].data_ptr(), None, None], ref.f["v2"].data_ptr(), ref.srce.data_ptr(), sz, 0, NT, gz=gz,
                           d_rec=ref.rec0.data_ptr())
        assert_bit_equal(dv.whole("u0"), ref.whole("u0"), "background vs fdw_dev_line_steps, " + what)
        assert_bit_equal(dv.gathers()[1], ref.gathers()[1], "background gather vs fdw_dev_line_steps, " + what)
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("two_step", [4, 1])
def test_line_loop_on_contexts_of_the_other_families(two_step):
    for kind in (FIELD, DTT):
        c = line_case("wide", 8, 0, kind)
        ctx = F.FDWave(*args_of(c[0]), compat=True, device=0)
        ctx.set_tuning(two_step=two_step)
        assert ctx.steps_per_pass() == {1: 2, 4: 4}[two_step]
        check_line_run(ctx, c, kind, f"two_step {two_step} kind {kind}")
        check_line_run(ctx, line_case("wide", 8, 0, kind, nsteps=4), kind, f"two_step {two_step} kind {kind}, an even count", nsteps=4)


@pytest.mark.gpu
@KINDS
def test_line_loop_either_gather_may_be_absent(kind):
    c = line_case("static-rows", 8, 0, kind)
    assert np.isnan(c[6][:, nsrc_of(c[0]):]).all() and nsrc_of(c[0]) == 77
    ctx = F.FDWave(*args_of(c[0]), compat=True, device=0)
    check_line_run(ctx, c, kind, "no scattered gather", rec=False)
    check_line_run(ctx, c, kind, "no background gather", rec0=False)
    check_line_run(ctx, c, kind, "no gather at all", rec=False, rec0=False)


@pytest.mark.gpu
@NUMERICS
def test_line_depths_at_their_limits(numerics):
    """The line inside the damped strip and on the last time-stepped column; gz in the interior and inside the damped strip."""
    d = line_case("static-rows", 8, numerics, DTT)[0]
    _, zlim, ztap = extents_of(d)
    z0 = born_cells(d)[2]
    assert ztap == 8 and zlim - 1 >= z0
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    for place in ((5, z0), (zlim - 1, 3), (z0 + 2, zlim - 1)):
        for kind in (FIELD, DTT):
            check_line_run(ctx, line_case("static-rows", 8, numerics, kind, place=place), kind, f"place {place} kind {kind} numerics {numerics}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: whole shots, single and batched
# ---------------------------------------------------------------------------------------------------------------------------------------
GRID = (87, 70, 12, 10)                                  # every receiver row is time-stepped: fdw_record_shot_batch batches on it
STATIC_GRID = (87, 70, 3, 10)                            # receiver rows 80..83 are not: batches fall back
SNT = 31
DSX = 13                                                 # source rows nxb + 14 + 13 b: 26, 39, 52 (65, 78 of five shots) on GRID


@functools.lru_cache(maxsize=None)
def shots(grid, order, numerics, kind, nshots=3):
    """nshots shots from rest on one reflectivity: distinct models, distinct source rows, distinct line gathers; the restatement's gathers
    [nshots][nx][nt] of the point-source and of the line-source form.  Asserted: at least half of every shot's scattered traces are non-zero."""
    nxe, nze, nxb, nzb = grid
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    decks = [make_deck(nxe, nze, nxb, nzb, SNT, seed=3 + 4 * b, order=order) for b in range(nshots)]
    d = decks[0]
    v2_all = np.stack([k["v2"] for k in decks])
    srce = (O.ricker_wavelet(SNT, 0.001, 120.0) * 1000.0).astype(np.float32)
    m = (0.3 * np.random.default_rng(8).standard_normal((nx, nz))).astype(np.float32)
    wav_all = np.random.default_rng(9).standard_normal((nshots, nx, SNT)).astype(np.float32)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    sx0 = nxb + 14
    out = dict(d=d, v2_all=v2_all, srce=srce, m=m, wav_all=wav_all, sx0=sx0, sz=d["sz"], gz=d["gz"])
    for name in ("point", "line"):
        rec, rec0 = [], []
        for b in range(nshots):
            if name == "point":
                r = born_restatement(orc, d, v2_all[b], embed_m(d, m), kind, sx0 + b * DSX, d["sz"], d["gz"], srce)
            else:
                r = born_line_restatement(orc, d, v2_all[b], embed_m(d, m), kind, d["sz"], d["gz"], np.ascontiguousarray(wav_all[b].T))
            live = (r["rec"] != 0).any(axis=0)
            assert live.sum() >= (nx + 1) // 2, f"{name} shot {b}: {live.sum()} of {nx} scattered traces are non-zero"
            rec.append(r["rec"].T.copy())
            rec0.append(r["rec0"].T.copy())
        out[name] = np.stack(rec), np.stack(rec0)
        assert all((out[name][0][a] != out[name][0][b]).any() for a in range(nshots) for b in range(a)), "the shots differ"
    for a in out.values():
        for x in (a if isinstance(a, tuple) else (a,)):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    return out


def make_ctx(s, numerics=0, **tuning):
    ctx = F.FDWave(*args_of(s["d"]), compat=True, device=0, numerics=numerics)
    if tuning:
        ctx.set_tuning(**tuning)
    return ctx


def born_batches(ctx, s, kind, nshots=3, background=True):
    """(point, line) through the batched calls, each (data, data0 or None), and fdw_batch_parts of each."""
    v2 = s["v2_all"][:nshots]
    a = ctx.born_shot_batch(nshots, s["m"], s["sx0"], DSX, s["sz"], s["gz"], s["srce"], kind=kind, v2_all=v2, want_background=background)
    pa = ctx.batch_parts()
    b = ctx.born_shot_line_batch(nshots, s["m"], s["sz"], s["gz"], s["wav_all"][:nshots], kind=kind, v2_all=v2, want_background=background)
    pb = ctx.batch_parts()
    return (a if background else (a, None)), (b if background else (b, None)), (pa, pb)


def born_singles(ctx, s, kind, nshots=3):
    """The same shots through fdw_born_shot / fdw_born_shot_line, one by one."""
    pt = [ctx.born_shot(s["v2_all"][b], s["m"], s["sx0"] + b * DSX, s["sz"], s["gz"], s["srce"], kind=kind, want_background=True) for b in range(nshots)]
    ln = [ctx.born_shot_line(s["v2_all"][b], s["m"], s["sz"], s["gz"], s["wav_all"][b], kind=kind, want_background=True) for b in range(nshots)]
    return tuple(np.stack(x) for x in zip(*pt)), tuple(np.stack(x) for x in zip(*ln))


@pytest.mark.gpu
@KINDS
@NUMERICS
@pytest.mark.parametrize("order,tuning", [(8, {}), (8, dict(two_step=4)), (12, {})], ids=str)
@pytest.mark.parametrize("grid", [STATIC_GRID, (69, 301, 8, 10)], ids=["87x70", "69x301"])
def test_born_shot_line_from_rest(grid, order, tuning, numerics, kind):
    s = shots(grid, order, numerics, kind, 1)
    d, v2, wav = s["d"], s["v2_all"][0], s["wav_all"][0]
    ctx = make_ctx(s, numerics, **tuning)
    what = f"{grid} order {order} {tuning} numerics {numerics} kind {kind}"
    data, data0 = ctx.born_shot_line(v2, s["m"], s["sz"], s["gz"], wav, kind=kind, want_background=True)
    assert_bit_equal(data, s["line"][0][0], "scattered gather, " + what)
    assert_bit_equal(data0, s["line"][1][0], "background gather, " + what)
    assert_bit_equal(data0, ctx.record_shot_line(v2, s["sz"], s["gz"], wav), "background gather vs fdw_record_shot_line, " + what)
    assert_bit_equal(ctx.born_shot_line(v2, s["m"], s["sz"], s["gz"], wav, kind=kind), data, "again, without the background gather, " + what)
    assert not ctx.born_shot_line(v2, np.zeros_like(s["m"]), s["sz"], s["gz"], wav, kind=kind).view(np.uint32).any(), "zero m: zero words, " + what


@functools.lru_cache(maxsize=None)
def resident_case():
    nxe, nze, nxb, nzb = GRID
    rng = np.random.default_rng(3)
    vp = (1500 + 1000 * rng.random((nxe - 2 * nxb, nze - 2 * nzb))).astype(np.float32)
    vp.setflags(write=False)
    return vp


@pytest.mark.gpu
def test_born_shot_line_on_the_resident_model():
    s = shots(GRID, 8, 0, DTT)
    d, wav = s["d"], s["wav_all"][1]
    ctx = make_ctx(s)
    ctx.model_resident(resident_case())
    with pytest.raises(F.FdwError) as e:
        ctx.born_shot_line(None, s["m"], s["sz"], s["gz"], wav)     # no squared model drawn yet
    assert e.value.code == ESTATE
    vel = ctx.dev_extendvel_linear(2 * ctx.border_draws(), want_vel=True)
    data, data0 = ctx.born_shot_line(None, s["m"], s["sz"], s["gz"], wav, want_background=True)
    want = born_line_restatement(O.Oracle(*args_of(d), compat=True), d, (vel * vel).astype(np.float32), embed_m(d, s["m"]), DTT, s["sz"], s["gz"],
                                 np.ascontiguousarray(wav.T))
    assert np.count_nonzero(want["rec"]) > 100
    assert_bit_equal(data, want["rec"].T, "resident model: scattered gather")
    assert_bit_equal(data0, want["rec0"].T, "resident model: background gather")
    assert_bit_equal(data0, ctx.record_shot_line(None, s["sz"], s["gz"], wav), "resident model: background vs fdw_record_shot_line")


@pytest.mark.gpu
@KINDS
@NUMERICS
@pytest.mark.parametrize("order", [2, 4, 6, 8])
def test_batches_of_three_shots(order, numerics, kind):
    """Both batched calls against the restatement per shot AND against the single-shot calls, with and without the background gathers;
    the whole batch went through one launch sequence; data0 is fdw_record_shot_batch's / fdw_record_shot_line_batch's."""
    s = shots(GRID, order, numerics, kind)
    ctx = make_ctx(s, numerics)
    what = f"order {order} numerics {numerics} kind {kind}"
    pt, ln, parts = born_batches(ctx, s, kind)
    assert parts == (1, 1), parts
    spt, sln = born_singles(ctx, s, kind)
    for name, got, single in (("point", pt, spt), ("line", ln, sln)):
        for i, g in enumerate(("scattered", "background")):
            assert_bit_equal(got[i], s[name][i], f"{name} batch vs restatement, {g}, {what}")
            assert_bit_equal(got[i], single[i], f"{name} batch vs the single-shot calls, {g}, {what}")
    npt, nln, parts = born_batches(ctx, s, kind, background=False)
    assert parts == (1, 1), parts
    assert_bit_equal(npt[0], pt[0], "point batch without data0, " + what)
    assert_bit_equal(nln[0], ln[0], "line batch without data0, " + what)
    assert_bit_equal(pt[1], ctx.record_shot_batch(3, s["sx0"], DSX, s["sz"], s["gz"], s["srce"], v2_all=s["v2_all"]), "data0 vs fdw_record_shot_batch, " + what)
    assert_bit_equal(ln[1], ctx.record_shot_line_batch(3, s["sz"], s["gz"], s["wav_all"], v2_all=s["v2_all"]), "data0 vs fdw_record_shot_line_batch, " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("offset_shots", [0, 2])
def test_batches_on_border_models_drawn_on_the_device(offset_shots):
    s = shots(GRID, 8, 0, DTT)
    ctx = make_ctx(s)
    ctx.model_resident(resident_case())
    T = ctx.border_draws()
    off = offset_shots * T
    pt = ctx.born_shot_batch(3, s["m"], s["sx0"], DSX, s["sz"], s["gz"], s["srce"], draw_offset=off, want_background=True)
    assert ctx.batch_parts() == 1
    ln = ctx.born_shot_line_batch(3, s["m"], s["sz"], s["gz"], s["wav_all"], draw_offset=off, want_background=True)
    assert ctx.batch_parts() == 1
    vels = []
    for b in range(3):
        vels.append(ctx.dev_extendvel_linear(off + b * T, want_vel=True))
        one = ctx.born_shot(None, s["m"], s["sx0"] + b * DSX, s["sz"], s["gz"], s["srce"], want_background=True)
        lone = ctx.born_shot_line(None, s["m"], s["sz"], s["gz"], s["wav_all"][b], want_background=True)
        for i in range(2):
            assert_bit_equal(pt[i][b], one[i], f"draw offset {off}: point shot {b}, gather {i}")
            assert_bit_equal(ln[i][b], lone[i], f"draw offset {off}: line shot {b}, gather {i}")
        assert np.count_nonzero(one[0]) > 100 and np.count_nonzero(lone[0]) > 100
    assert (vels[0] != vels[1]).any() and (vels[1] != vels[2]).any(), "the shots' models differ"


def share(ctx, s, gathers):
    return 11 * ctx.field_bytes() + gathers * 4 * s["m"].shape[0] * SNT


@pytest.mark.gpu
def test_a_batch_over_the_budget_goes_through_in_parts():
    """Five shots under a budget that holds two: three parts; under a budget below one shot's share: one by one.  The same bytes."""
    s = shots(GRID, 8, 0, DTT, 5)
    ctx = make_ctx(s)
    pt, ln, parts = born_batches(ctx, s, DTT, nshots=5)
    assert parts == (1, 1)
    for i in range(2):
        assert_bit_equal(pt[i], s["point"][i], f"five shots at once: point, gather {i}")
        assert_bit_equal(ln[i], s["line"][i], f"five shots at once: line, gather {i}")
    for budget_pt, budget_ln, want_parts in ((2 * share(ctx, s, 2) + 100, 2 * share(ctx, s, 3) + 100, 3), (share(ctx, s, 2) - 4, share(ctx, s, 3) - 4, 0)):
        ctx.set_batch_budget(budget_pt)
        a = ctx.born_shot_batch(5, s["m"], s["sx0"], DSX, s["sz"], s["gz"], s["srce"], v2_all=s["v2_all"], want_background=True)
        assert ctx.batch_parts() == want_parts
        ctx.set_batch_budget(budget_ln)
        b = ctx.born_shot_line_batch(5, s["m"], s["sz"], s["gz"], s["wav_all"], v2_all=s["v2_all"], want_background=True)
        assert ctx.batch_parts() == want_parts
        for i in range(2):
            assert_bit_equal(a[i], pt[i], f"parts {want_parts}: point, gather {i}")
            assert_bit_equal(b[i], ln[i], f"parts {want_parts}: line, gather {i}")
    ctx.set_batch_budget(0)


@pytest.mark.gpu
@pytest.mark.parametrize("grid,order,tuning", [(GRID, 12, {}), (GRID, 8, dict(use_generic=True)), (STATIC_GRID, 8, {})], ids=["order12", "generic", "static-rows"])
def test_fall_backs_run_one_by_one_with_the_same_bytes(grid, order, tuning):
    s = shots(grid, order, 0, DTT)
    ctx = make_ctx(s, **tuning)
    pt, ln, parts = born_batches(ctx, s, DTT)
    assert parts == (0, 0), parts
    spt, sln = born_singles(ctx, s, DTT)
    for name, got, single in (("point", pt, spt), ("line", ln, sln)):
        for i in range(2):
            assert_bit_equal(got[i], s[name][i], f"{name} fall-back vs restatement, gather {i}")
            assert_bit_equal(got[i], single[i], f"{name} fall-back vs the single-shot calls, gather {i}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: FDW_NO_BORN_FUSED=1 (read when a context is created) in a child process: the line loop and the batches' fall-back
# ---------------------------------------------------------------------------------------------------------------------------------------
def unfused_child():
    assert os.environ.get("FDW_NO_BORN_FUSED") == "1"
    for order, tuning in ((8, dict(prefetch=2)), (4, {})):
        for numerics in (0, 1):
            for kind in (FIELD, DTT):
                for deck in ("static-rows", "wide"):
                    c = line_case(deck, order, numerics, kind)
                    ctx = F.FDWave(*args_of(c[0]), compat=True, device=0, numerics=numerics)
                    ctx.set_tuning(xchunk=DECKS[deck][4], two_step=-1, **tuning)
                    check_line_run(ctx, c, kind, f"unfused {deck} order {order} numerics {numerics} kind {kind}", split=3)
                    ctx.close()
    s = shots(GRID, 8, 0, DTT)
    ctx = make_ctx(s)
    pt, ln, parts = born_batches(ctx, s, DTT)
    assert parts == (0, 0), parts
    for i in range(2):
        assert_bit_equal(pt[i], s["point"][i], f"unfused batch: point, gather {i}")
        assert_bit_equal(ln[i], s["line"][i], f"unfused batch: line, gather {i}")
    print("unfused: ok")


@pytest.mark.gpu
def test_unfused_arrangement_line_loop_and_batches():
    env = dict(os.environ, FDW_NO_BORN_FUSED="1")
    r = subprocess.run([sys.executable, "-c", "import conftest, test_born_batch; test_born_batch.unfused_child()"], cwd=os.path.join(ROOT, "tests"),
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "unfused: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: one context through a sequence of calls that share the batch buffers
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_context_in_sequence():
    s = shots(GRID, 8, 0, DTT)
    d, nx = s["d"], s["m"].shape[0]
    orc = O.Oracle(*args_of(d), compat=True)
    d_obs = np.random.default_rng(2).standard_normal((3, nx, SNT)).astype(np.float32)
    imgs = []
    for b in range(3):
        oP, oPP = orc.forward(s["v2_all"][b], s["sx0"] + b * DSX, s["sz"], s["srce"])
        imgs.append(orc.back(s["v2_all"][b], oP, oPP, d_obs[b], s["gz"]))
    ctx = make_ctx(s)
    for turn in range(2):
        pt = ctx.born_shot_batch(3, s["m"], s["sx0"], DSX, s["sz"], s["gz"], s["srce"], v2_all=s["v2_all"], want_background=True)
        assert ctx.batch_parts() == 1
        for i in range(2):
            assert_bit_equal(pt[i], s["point"][i], f"turn {turn}: fdw_born_shot_batch, gather {i}")
        got = ctx.shot_batch(3, s["sx0"], DSX, s["sz"], s["gz"], s["srce"], d_obs, v2_all=s["v2_all"])
        assert ctx.batch_parts() == 1
        assert_bit_equal(got, np.stack(imgs), f"turn {turn}: fdw_shot_batch")
        one = ctx.born_shot(s["v2_all"][1], s["m"], s["sx0"] + DSX, s["sz"], s["gz"], s["srce"], want_background=True)
        for i in range(2):
            assert_bit_equal(one[i], s["point"][i][1], f"turn {turn}: fdw_born_shot, gather {i}")
        assert_bit_equal(ctx.shot(s["v2_all"][2], s["sx0"] + 2 * DSX, s["sz"], s["gz"], s["srce"], d_obs[2]), imgs[2], f"turn {turn}: fdw_shot")
        ln = ctx.born_shot_line_batch(3, s["m"], s["sz"], s["gz"], s["wav_all"], v2_all=s["v2_all"], want_background=True)
        for i in range(2):
            assert_bit_equal(ln[i], s["line"][i], f"turn {turn}: fdw_born_shot_line_batch, gather {i}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the stream contract (a late producer) and the footprint (a guarded arena) of fdw_dev_born_line_steps
# ---------------------------------------------------------------------------------------------------------------------------------------
IT0, NSTEPS = 2, 5                                       # rows [2, 7) of the nine-row gathers


def _stream_case(kind):
    import stream_cases as S
    deck = "ragged"
    nxe, nze, nxb, nzb = S.DECKS[deck]["geom"]
    nx = nxe - 2 * nxb
    _, sz, gz = S.DECKS[deck]["place"]

    def m_of(i):
        return reflectivity(i["d"], seed=3 if i is S.inputs(deck, "true") else 11)

    def ins(i):
        return dict(u0=("field", i["p0"]), u1=("field", i["pp0"]), du0=("field", i["f1"]), du1=("field", i["f0"]), v2=("field", i["v2"]),
                    m=("field", m_of(i)), w=("flat", i["w"]))

    outs = dict(rec=("flat", (S.NT, nx), 9.0), rec0=("flat", (S.NT, nx), -7.0))

    def call(ctx, p, stream):
        ctx.dev_born_line_steps(p["u0"], p["u1"], p["du0"], p["du1"], p["v2"], p["m"], kind, p["w"], sz, gz, p["rec"], p["rec0"], IT0, NSTEPS,
                                stream=stream)
        rows = np.arange(IT0, IT0 + NSTEPS)
        return [("U_PP", "u0", None, None), ("DU_PP", "du0", None, None), ("rec", "rec", None, rows), ("rec0", "rec0", None, rows)]

    def want(v):
        i = S.inputs(deck, v)
        r = born_line_restatement(S.oracle(deck, 0), i["d"], i["v2"], m_of(i), kind, sz, gz, i["w"], i["p0"], i["pp0"], i["f1"], i["f0"], it0=IT0,
                                  nsteps=NSTEPS)
        rows = np.arange(IT0, IT0 + NSTEPS)
        return dict(U_PP=r["U_PP"], DU_PP=r["DU_PP"], rec=r["rec"][rows], rec0=r["rec0"][rows])

    return S.Case(f"born-line-kind{kind}-{deck}", deck, 0, -1, ins, outs, call, want, scratch=("u0", "u1", "du0", "du1"), pad_words=dict(m=PAD_NAN))


@pytest.mark.gpu
def test_line_loop_late_producer_on_the_callers_stream():
    import torch

    import stream_cases as S
    case_ = _stream_case(DTT)
    run = S.Run(case_, torch)
    torch.cuda.synchronize()
    delay = S.Delay(torch)
    st = torch.cuda.Stream()
    run.enqueue(st, delay, 40.0)
    busy = run.busy
    st.synchronize()
    got, want, decoy = run.results(), case_.want("true"), case_.want("decoy")
    for k in want:
        assert_bit_equal(got[k], want[k], f"late producer: {k}")
        assert (want[k] != decoy[k]).any(), k
    assert busy, "the entry point returned only after the stream had drained: it synchronised"
    run.close()


@pytest.mark.gpu
@KINDS
def test_line_loop_guarded_arena_footprint(kind):
    import torch

    import footprint_arena as A
    import stream_cases as S
    case_ = _stream_case(kind)
    arena = A.build(case_, S.inputs("ragged", "true"))
    ctx = case_.make_ctx()
    assert ctx.pitch == arena.pitch
    t = torch.from_numpy(arena.up.view(np.int32).copy()).to("cuda:0")
    labels = case_.call(ctx, arena.pointers(t.data_ptr()), None)
    torch.cuda.synchronize()
    ctx.close()
    down = t.cpu().numpy().view(np.uint32)
    bad = A.check(arena, down, labels)
    assert not bad, "\n".join(bad)
    got, want = A.results(arena, down, labels), case_.want("true")
    for k in want:
        assert_bit_equal(got[k], want[k], f"arena: {k}")
    rec = arena.bufs["rec"].values(down)
    assert (rec[:IT0] == 9.0).all() and (rec[IT0 + NSTEPS:] == 9.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def code(fn, *a, **kw):
    with pytest.raises(F.FdwError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.mark.gpu
def test_refusals_of_the_line_loop_enqueue_nothing():
    c = line_case("static-rows", 8, 0, DTT)
    d, u0, u1, du0, du1, m, w, (sz, gz), _ = c
    _, zlim, _ = extents_of(d)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    dv = LineDevice(ctx, d, u0, u1, du0, du1, m, w)
    p = {k: t.data_ptr() for k, t in dv.f.items()}
    good = [p["u0"], p["u1"], p["du0"], p["du1"], p["v2"], p["m"], DTT, dv.srce.data_ptr(), sz, gz, dv.rec.data_ptr(), dv.rec0.data_ptr(), 0, 3]
    born = ctx.dev_born_line_steps
    for k in (0, 1, 2, 3, 4, 5, 7):                                # the four fields, v2, m, the line gather
        a = list(good)
        a[k] = None
        assert code(born, *a) == EINVAL, k
    for k, vals in ((6, (-1, 2)), (8, (-1, zlim)), (9, (-1, zlim)), (12, (-1,)), (13, (-1,))):
        for v in vals:
            a = list(good)
            a[k] = v
            assert code(born, *a) == EINVAL, (k, v)
    assert F.lib().fdw_dev_born_line_steps(None, *good, 0, None) == EINVAL
    others = [F.FDWave(*args_of(d), compat=True, device=0, slab=(0, 40)), F.FDWave(*args_of(d), compat=True, device=0, dialect=1),
              F.FDWave(*args_of(d), compat=True, device=0, dialect=2)]
    for other in others:
        assert code(other.dev_born_line_steps, *good) == ESTATE
    dv.torch.cuda.synchronize()
    for k, a in (("u0", u0), ("u1", u1), ("du0", du0), ("du1", du1)):
        assert_bit_equal(dv.get(k), a, f"a refused call enqueues nothing: {k}")
    grec, grec0 = dv.gathers()
    assert (grec == 9.0).all() and (grec0 == -9.0).all()
    born(*[*good[:8], zlim - 1, zlim - 1, *good[10:]])                # the deepest column is accepted
    born(*[*good[:13], 0])                                          # no step is not an error


@pytest.mark.gpu
def test_refusals_of_the_shot_calls():
    s = shots(STATIC_GRID, 8, 0, DTT)
    d, m, srce, wav_all, v2_all = s["d"], s["m"], s["srce"], s["wav_all"], s["v2_all"]
    sx0, sz, gz = s["sx0"], s["sz"], s["gz"]
    xlim, zlim, _ = extents_of(d)
    ctx = make_ctx(s)
    line, pb, lb = ctx.born_shot_line, ctx.born_shot_batch, ctx.born_shot_line_batch
    # fdw_born_shot_line
    assert code(line, v2_all[0], m, zlim, gz, wav_all[0]) == EINVAL
    assert code(line, v2_all[0], m, -1, gz, wav_all[0]) == EINVAL
    assert code(line, v2_all[0], m, sz, zlim, wav_all[0]) == EINVAL
    assert code(line, v2_all[0], m, sz, gz, wav_all[0], kind=2) == EINVAL
    assert code(line, None, m, sz, gz, wav_all[0]) == ESTATE          # no resident model
    # the batches: fdw_born_shot's refusals, nshots < 1, the source rows
    assert code(pb, 3, m, sx0, DSX, zlim, gz, srce, v2_all=v2_all) == EINVAL
    assert code(pb, 3, m, sx0, DSX, sz, zlim, srce, v2_all=v2_all) == EINVAL
    assert code(pb, 3, m, sx0, DSX, sz, gz, srce, v2_all=v2_all, kind=-1) == EINVAL
    assert code(pb, 3, m, xlim - 2 * DSX, DSX, sz, gz, srce, v2_all=v2_all) == EINVAL       # the last source row is row xlim
    assert code(pb, 3, m, 2 * DSX - 1, -DSX, sz, gz, srce, v2_all=v2_all) == EINVAL         # ... is row -1
    assert code(pb, 3, m, sx0, DSX, sz, gz, srce) == ESTATE                                 # no model at all
    assert code(lb, 3, m, zlim, gz, wav_all, v2_all=v2_all) == EINVAL
    assert code(lb, 3, m, sz, zlim, wav_all, v2_all=v2_all) == EINVAL
    assert code(lb, 3, m, sz, gz, wav_all, v2_all=v2_all, kind=2) == EINVAL
    assert code(lb, 3, m, sz, gz, wav_all) == ESTATE
    L = F.lib()
    nx = m.shape[0]
    data = np.zeros((3, nx, SNT), np.float32)
    v2p, mp, sp, wp, dp = v2_all.ctypes.data, m.ctypes.data, srce.ctypes.data, wav_all.ctypes.data, data.ctypes.data
    assert L.fdw_born_shot_batch(ctx._h, 0, v2p, 0, mp, DTT, sx0, DSX, sz, gz, sp, dp, None) == EINVAL
    assert L.fdw_born_shot_line_batch(ctx._h, 0, v2p, 0, mp, DTT, sz, gz, wp, dp, None) == EINVAL
    assert L.fdw_born_shot_batch(None, 3, v2p, 0, mp, DTT, sx0, DSX, sz, gz, sp, dp, None) == EINVAL
    assert L.fdw_born_shot_line_batch(None, 3, v2p, 0, mp, DTT, sz, gz, wp, dp, None) == EINVAL
    assert L.fdw_born_shot_line(None, v2p, mp, DTT, sz, gz, wp, dp, None) == EINVAL
    for bad in ((None, sp, dp), (mp, None, dp), (mp, sp, None)):
        assert L.fdw_born_shot_batch(ctx._h, 3, v2p, 0, bad[0], DTT, sx0, DSX, sz, gz, bad[1], bad[2], None) == EINVAL
    for bad in ((None, wp, dp), (mp, None, dp), (mp, wp, None)):
        assert L.fdw_born_shot_line_batch(ctx._h, 3, v2p, 0, bad[0], DTT, sz, gz, bad[1], bad[2], None) == EINVAL
        assert L.fdw_born_shot_line(ctx._h, v2p, bad[0], DTT, sz, gz, bad[1], bad[2], None) == EINVAL
    assert not data.any(), "a refused call writes nothing"
    for other in (F.FDWave(*args_of(d), compat=True, device=0, slab=(0, 40)), F.FDWave(*args_of(d), compat=True, device=0, dialect=1),
                  F.FDWave(*args_of(d), compat=True, device=0, dialect=2)):
        assert code(other.born_shot_line, v2_all[0], m, sz, gz, wav_all[0]) == ESTATE
        assert code(other.born_shot_batch, 3, m, sx0, DSX, sz, gz, srce, v2_all=v2_all) == ESTATE
        assert code(other.born_shot_line_batch, 3, m, sz, gz, wav_all, v2_all=v2_all) == ESTATE
    # the context still works, and the accepted extremes are accepted
    got = pb(3, m, xlim - 1 - 2 * DSX, DSX, zlim - 1, zlim - 1, srce, v2_all=v2_all)
    assert got.shape == (3, nx, SNT)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: rtm_model bornfile= in groups of shots
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@KINDS
def test_rtm_model_bornfile_batched_equals_shot_by_shot_and_born_shot(tmp_path, kind):
    m = (0.3 * np.random.default_rng(6).standard_normal((PNX, PNZ))).astype(np.float32)
    vp = _write_deck(tmp_path, f"bornfile=./m.bin\nborn_bg=./bg.bin\nborn_kind={kind}\n", m=m)
    r = _run_rtm_model(tmp_path, dict(FDW_TIMING="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[timing] shots per launch sequence: up to 5 (fdw_born_shot_batch)" in r.stderr, r.stderr
    batched = (tmp_path / "data.bin").read_bytes(), (tmp_path / "bg.bin").read_bytes()
    os.remove(tmp_path / "data.bin")
    os.remove(tmp_path / "bg.bin")
    r = _run_rtm_model(tmp_path, dict(FDW_TIMING="1", FDW_NO_SHOT_BATCH="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "(one by one)" in r.stderr and "fdw_born_shot_batch" not in r.stderr, r.stderr
    assert batched == ((tmp_path / "data.bin").read_bytes(), (tmp_path / "bg.bin").read_bytes()), "FDW_NO_SHOT_BATCH=1 writes the same bytes"
    data = np.frombuffer(batched[0], np.float32).reshape(PNS, PNX, PNT)
    bg = np.frombuffer(batched[1], np.float32).reshape(PNS, PNX, PNT)
    ctx = F.FDWave(8, PNX + 2 * PNB, PNZ + 2 * PNB, PNB, PNB, PNT, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    ctx.model_resident(vp)
    srce = F.ricker_wavelet(PNT, 0.001, 60.0)
    for i in range(PNS):
        ctx.dev_extendvel_linear(i * ctx.border_draws())
        want, want0 = ctx.born_shot(None, m, PFSX + PDS * i + PNB, 1 + PNB, 2 + PNB, srce, kind=kind, want_background=True)
        assert np.count_nonzero(want) > 100
        assert_bit_equal(data[i], want, f"shot {i}: scattered gathers")
        assert_bit_equal(bg[i], want0, f"shot {i}: background gathers")
    assert all((data[i] != data[j]).any() for i in range(PNS) for j in range(i))

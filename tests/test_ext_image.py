"""Subsurface-offset image gathers (fdwave.h, "Extended imaging"): fdw_plan_ext_image, fdw_dev_ext_image, fdw_shot_ext, rtm_code's ext=H.

The restatement (tests/ext_restatement.py) is numpy on top of tests/dtt_restatement.py's F and R, every operation rounded on its own; the
GPU is held to it bit for bit on every word of every plane (C against the restatement, every other word as it came, sentinels in the
padding columns), NaNs by position."""
import functools
import os
import subprocess

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from born_restatement import DTT, born_cells, born_restatement, embed_m
from conftest import ROOT, assert_bit_equal, make_deck, random_fields
from ext_restatement import ext_back_restatement, ext_term, ext_term_fields
from oracle import oracle as O
from test_born import CONFIGS, DECKS
from test_line_source import args_of, extents_of
from test_stepn_isa_budget import isa  # noqa: F401  (a fixture)

EINVAL, ESTATE = -1, -5
HMAX = 8
PAD = 0x7FC0E7A1                                         # what the padding columns of the planes hold
NT = 9
f32 = np.float32


def inner(d, a):
    return a[..., d["nxb"]:d["nxe"] - d["nxb"], d["nzb"]:d["nze"] - d["nzb"]]


def mirrored(E):
    return np.ascontiguousarray(E[::-1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the built library, the restatement, the row plan, the programs' refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_ext_symbol_is_exported_declared_and_mirrored():
    L = F.lib()
    header = open(os.path.join(ROOT, "include", "fdwave.h")).read()
    for name in ("fdw_plan_ext_image", "fdw_dev_ext_image", "fdw_shot_ext"):
        assert hasattr(L, name), name
        assert name + "(" in header, name
    assert "#define FDW_EXT_HMAX 8" in header
    for name in ("dev_ext_image", "shot_ext"):
        assert hasattr(F.FDWave, name), name
    assert callable(F.plan_ext_image)


@functools.lru_cache(maxsize=None)
def chain_case(deck="static-rows", numerics=0, H=3):
    nxe, nze, nxb, nzb, _ = DECKS[deck]
    d = make_deck(nxe, nze, nxb, nzb, NT, seed=3, order=8)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    P, PP = orc.forward(d["v2"], d["sx"], d["sz"], O.ricker_wavelet(NT, 0.001, 120.0) * 1000.0)
    d_obs = np.random.default_rng(2).standard_normal((nxe - 2 * nxb, NT)).astype(f32)
    return d, orc, P, PP, d_obs, ext_back_restatement(orc, d, d["v2"], P, PP, d_obs.T[::-1], d["gz"], H)


@pytest.mark.parametrize("numerics", [0, 1])
def test_restatement_zero_offset_plane_is_the_cross_correlation_image(numerics):
    d, orc, P, PP, d_obs, r = chain_case(numerics=numerics)
    x0, x1, z0, z1 = born_cells(d)
    assert_bit_equal(r["E"][3][x0:x1, z0:z1], r["xcorr"][x0:x1, z0:z1], "plane h = 0 on C")
    assert_bit_equal(inner(d, r["xcorr"]), orc.back(d["v2"], P, PP, d_obs, d["gz"]), "the chain's cross-correlation image is Oracle.back's")
    assert all(r["E"][j][x0:x1, z0:z1].any() for j in range(7))
    out = np.ones(r["E"].shape, bool)
    out[:, x0:x1, z0:z1] = False
    assert not r["E"][out].any(), "nothing outside C"
    for h in range(1, 4):      # the |h| rows at either end of C
        for j in (3 - h, 3 + h):
            assert not r["E"][j][x0:x0 + h].any() and not r["E"][j][x1 - h:x1].any()


def test_restatement_mirror_identity_and_zero_data():
    rng = np.random.default_rng(5)
    f, r = rng.standard_normal((40, 33)).astype(f32), rng.standard_normal((40, 33)).astype(f32)
    E0 = rng.standard_normal((9, 40, 33)).astype(f32)
    cells = (3, 37, 2, 30)
    a = ext_term(E0.copy(), f, r, 4, cells)
    b = ext_term(mirrored(E0), r, f, 4, cells)
    assert_bit_equal(a, mirrored(b), "E_{f,r}[h] == E_{r,f}[-h]")
    assert (a != E0).any() and (a[0] != a[8]).any()
    assert_bit_equal(ext_term(E0.copy(), f, np.zeros_like(r), 4, cells), E0, "a zero field adds zeros: noise planes keep their bits")
    d, orc, P, PP, d_obs, _ = chain_case()
    E0 = np.random.default_rng(6).standard_normal((7, d["nxe"], d["nze"])).astype(f32)
    still = ext_back_restatement(orc, d, d["v2"], P, PP, np.zeros_like(d_obs.T), d["gz"], 3, E0=E0)      # receivers at rest: r^{k+1} = +0.0 on C
    assert_bit_equal(still["E"], E0, "all-zero data leave every plane as it came")


def test_zero_offset_plane_carries_the_largest_energy_on_a_reflector_deck():
    """96 x 88, borders 6 / 7, nt 120, srce = [1, -2, 1, 0 ...], a flat reflector m[:, 40] = 0.3 whose FDW_BORN_DTT gather is the data,
    source (the middle row) and receivers at nzb + 8, the migration velocity the one the data were modelled in: of the 13 planes at H = 6 the plane h = 0
    has strictly the largest energy.  The ratio to the next plane is printed; measured on the restatement: 1.447."""
    nt, H = 120, 6
    d = make_deck(96, 88, 6, 7, nt)
    nxb, nzb = d["nxb"], d["nzb"]
    nx, nz = d["nxe"] - 2 * nxb, d["nze"] - 2 * nzb
    sx, sz = nxb + nx // 2, nzb + 8
    srce = np.zeros(nt, f32)
    srce[:3] = 1.0, -2.0, 1.0
    m = np.zeros((nx, nz), f32)
    m[:, 40] = 0.3
    orc = O.Oracle(*args_of(d), compat=True)
    rec = born_restatement(orc, d, d["v2"], embed_m(d, m), DTT, sx, sz, sz, srce)["rec"]
    P, PP = orc.forward(d["v2"], sx, sz, srce)
    r = ext_back_restatement(orc, d, d["v2"], P, PP, np.ascontiguousarray(rec[::-1]), sz, H)
    x0, x1, z0, z1 = born_cells(d)
    assert_bit_equal(r["E"][H][x0:x1, z0:z1], r["xcorr"][x0:x1, z0:z1], "plane h = 0 on C")
    energy = (r["E"].astype(np.float64) ** 2).sum(axis=(1, 2))
    order = np.argsort(energy)[::-1]
    print("energy per plane / the largest:", np.round(energy / energy.max(), 4), "ratio to the next plane: %.3f" % (energy[order[0]] / energy[order[1]]))
    assert order[0] == H and energy[order[0]] > energy[order[1]], energy


ROW_EXTENTS = [(0, 1), (5, 6), (5, 7), (3, 64), (6, 70), (0, 200), (17, 8209)]      # x0, x1


@pytest.mark.parametrize("H", range(HMAX + 1))
def test_plan_reads_inside_C_and_tiles_every_plane_exactly_once(H):
    """Every row index the plan reads lies in [x0, x1); every row it writes for offset h in [x0 + |h|, x1 - |h|); the written rows tile that
    range exactly once; chunk lengths 1, 2H, 2H + 1 and 0 (automatic)."""
    extents = ROW_EXTENTS + [(4, 4 + n) for n in (2 * H, 2 * H + 1, 2 * H + 2) if n > 0]
    for x0, x1 in extents:
        for xchunk in sorted({1, max(2 * H, 1), 2 * H + 1, 0}):
            for nz in (1, 300, 8192):
                used, chunks = F.plan_ext_image(x0, x1, nz, H, xchunk)
                what = f"rows [{x0},{x1}) nz {nz} H {H} xchunk {xchunk} -> {used}"
                assert used == xchunk or (xchunk == 0 and max(H, 2) <= used <= 64), what
                assert len(chunks) == -(-(x1 - x0) // used), what
                times = np.zeros((2 * H + 1, x1 + H + 2), int)
                at = x0
                for c in chunks:
                    assert c["c0"] == at and c["c0"] < c["c1"] <= min(c["c0"] + used, x1), what
                    at = c["c1"]
                    assert x0 <= c["rd0"] <= c["c0"] and c["c1"] <= c["rd1"] <= x1, (what, c)
                    assert c["rd0"] == max(x0, c["c0"] - H) and c["rd1"] == min(x1, c["c1"] + H), (what, c)
                    for j, (w0, w1) in enumerate(c["writes"]):
                        h = j - H
                        if w0 == w1:
                            continue
                        assert c["c0"] <= w0 < w1 <= c["c1"], (what, c)
                        times[j, w0:w1] += 1
                        # the operands of the rows written: f[x - h], r[x + h]
                        assert c["rd0"] <= w0 - abs(h) and w1 - 1 + abs(h) < c["rd1"], (what, c, h)
                assert at == x1, what
                for j in range(2 * H + 1):
                    want = np.zeros(times.shape[1], int)
                    want[x0 + abs(j - H):max(x1 - abs(j - H), x0 + abs(j - H))] = 1
                    assert (times[j] == want).all(), (what, j)
    assert F.lib().fdw_plan_ext_image(0, 10, 5, HMAX + 1, 0, None, None, 0) == EINVAL
    assert F.lib().fdw_plan_ext_image(0, 10, 5, -1, 0, None, None, 0) == EINVAL
    assert F.lib().fdw_plan_ext_image(3, 2, 5, 0, 0, None, None, 0) == EINVAL
    assert F.plan_ext_image(7, 7, 5, H)[1] == []


def test_ext_kernels_exist_without_scratch(isa):      # noqa: F811
    names = [k for k in isa if "fdw_ext_image" in k]
    for H in range(HMAX + 1):
        for V in (1, 4):
            assert any(f"fdw_ext_image_kernelILi{H}ELi{V}ELi0EEEv" in k for k in names), (H, V, names)
    assert any("fdw_ext_image_point_kernelE" in k for k in names)
    assert len(names) == 2 * (HMAX + 1) + 1, names
    for k in names:
        meta = isa[k][0]
        print(k, {f: meta.get(f) for f in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count")})
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (k, meta)
        assert not any(mn.startswith("scratch_") or "atomic" in mn or mn.startswith("ds_") for mn, _ in isa[k][1]), k


@pytest.mark.parametrize("extra,env_extra,words", [("ext=2\nexc=1\n", {}, ("ext", "exc")), ("ext=2\ndtt=1\n", {}, ("ext", "dtt")), ("ext=2\nlsm=3\n", {}, ("ext", "lsm")),
                                                   ("ext=2\npw=3\npw_pmax=0.0001\n", {}, ("ext", "pw")), ("ext=2\nslabs=2\n", {}, ("ext", "slabs")),
                                                   ("ext=2\n", {"FDW_SLABS": "2"}, ("ext", "slabs")), ("ext=2\ngpus=2\n", {}, ("ext", "gpus")),
                                                   ("ext=2\nsnap=5\n", {}, ("ext", "snap")), ("ext=2\nresid=1\n", {}, ("ext", "resid")),
                                                   ("ext=2\nillum=1\n", {}, ("ext", "illum"))],
                         ids=["exc", "dtt", "lsm", "pw", "slabs-key", "FDW_SLABS", "gpus", "snap", "resid", "illum"])
def test_rtm_code_refuses_ext_with_the_keys_it_does_not_combine_with(tmp_path, extra, env_extra, words):
    """Before any file, thread, communicator or device is touched: runs where no GPU is, and leaves the output directory empty."""
    from test_residual import BIN, _write_min_deck
    _write_min_deck(tmp_path, extra)
    env = {k: v for k, v in os.environ.items() if k not in ("FDW_SLABS", "FDW_GPUS")}
    env.update(env_extra)
    r = subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode != 0
    assert "ext=2 cannot be combined" in r.stderr and all(w in r.stderr for w in words), r.stderr
    assert os.listdir(tmp_path / "out") == []
    assert not os.path.exists(tmp_path / "image.num")


def test_rtm_code_refuses_a_half_width_above_the_maximum(tmp_path):
    from test_residual import BIN, _write_min_deck
    _write_min_deck(tmp_path, "ext=9\n")
    r = subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode != 0 and "ext=9" in r.stderr and os.listdir(tmp_path / "out") == []


def test_python_driver_refuses_an_ext_deck(tmp_path):
    from parallel_finite_difference_computation_amd import rtm
    from test_residual import _write_min_deck
    _write_min_deck(tmp_path, "ext=2\n")
    with pytest.raises(ValueError, match="ext"):
        rtm.read_deck(str(tmp_path / "input.dat"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: one term on caller-owned arrays
# ---------------------------------------------------------------------------------------------------------------------------------------
class Planes:
    """f, r (fields, +0.0 padding) and the 2H+1 planes (PAD in the padding columns) on the device.  shift: the three arrays start that many
    words past a 256-byte boundary (1: no array is 16-byte aligned, the one-word-per-lane kernels run)."""

    def __init__(self, ctx, f, r, E0, shift=0):
        import torch
        self.torch, self.ctx, self.nze = torch, ctx, f.shape[1]
        self.t = {}
        for name, a, pad in (("f", f, 0), ("r", r, 0), ("E", E0.reshape(-1, E0.shape[-1]), PAD)):
            h = np.full((a.shape[0], ctx.pitch), pad, np.uint32)
            h[:, :self.nze] = np.ascontiguousarray(a, f32).view(np.uint32)
            flat = np.concatenate([np.zeros(shift, np.uint32), h.ravel()])
            self.t[name] = (torch.from_numpy(flat.view(np.int32)).to("cuda:0"), h.shape)
        self.shift, self.nplanes = shift, E0.shape[0]
        torch.cuda.synchronize()

    def ptr(self, name):
        return self.t[name][0].data_ptr() + 4 * self.shift

    def term(self, H, swap=False, stream=None):
        a, b = ("r", "f") if swap else ("f", "r")
        self.ctx.dev_ext_image(self.ptr(a), self.ptr(b), H, self.ptr("E"), stream=stream)

    def whole(self, name):
        self.torch.cuda.synchronize()
        t, shape = self.t[name]
        return t.cpu().numpy().view(np.uint32)[self.shift:].reshape(shape)

    def planes(self):
        """The planes [2H+1][nxe][nze] as float32, after checking the padding columns."""
        w = self.whole("E")
        assert (w[:, self.nze:] == PAD).all(), "padding columns of the planes"
        return np.ascontiguousarray(w[:, :self.nze]).view(f32).reshape(self.nplanes, -1, self.nze)


def noise_case(d, H, seed):
    rng = np.random.default_rng(seed)
    shape = (d["nxe"], d["nze"])
    return rng.standard_normal(shape).astype(f32), rng.standard_normal(shape).astype(f32), rng.standard_normal((2 * H + 1,) + shape).astype(f32)


def seam_xchunk(rows):
    """A chunk length that cuts `rows` rows into at least three chunks, the last of one row (1 where the rows are too few)."""
    for xc in range((rows - 1) // 2, 0, -1):
        if (rows - 1) % xc == 0:
            return xc
    return 1


def run_term(ctx, d, H, seed, what, shift=0, same=assert_bit_equal, case=None):
    f, r, E0 = case or noise_case(d, H, seed)
    want = ext_term_fields(d, E0, f, r, H)
    dv = Planes(ctx, f, r, E0, shift)
    dv.term(H)
    same(dv.planes(), want, "planes, " + what)
    for name, a in (("f", f), ("r", r)):
        assert_bit_equal(dv.whole(name)[:, :d["nze"]].view(f32), a, name + " is only read, " + what)
    x0, x1, z0, z1 = born_cells(d)
    changed = want.view(np.uint32) != E0.view(np.uint32)
    for j in range(2 * H + 1):
        a, b = x0 + abs(j - H), x1 - abs(j - H)
        if b > a:
            assert changed[j, a:b, z0:z1].mean() > 0.9, (what, j)
            changed[j, a:b, z0:z1] = False
    assert not changed.any(), "the restatement changes the cells of the definition only, " + what
    return dv


def plain_deck(rows, cols, nxb=5, nzb=6):
    """A whole-grid (compat = False) deck whose C is rows x cols."""
    d = make_deck(rows + 2 * nxb, cols + 2 * nzb, nxb, nzb, NT, seed=1, compat=False)
    assert born_cells(d) == (nxb, nxb + rows, nzb, nzb + cols)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("H", range(HMAX + 1))
def test_dev_ext_image_vs_restatement(H):
    """Every instantiation (H = 0 .. 8, four words per lane and one) on the four decks of tests/test_born.py -- the ragged compat grid
    ("static-rows": xlim 80 inside the interior) and the pitch == nze deck ("flush") among them --, EXACT and FAST contexts, automatic chunks
    and chunks cut so that C spans at least three with a last chunk of one row; row extents of C of 1, 2, 2H, 2H + 1, 2H + 2 and 64 rows and
    column extents of 1, 63, 64, 65, 256 and 257 columns.  The planes enter with noise and a sentinel in their padding columns."""
    seed = 100 * H
    for deck, (nxe, nze, nxb, nzb, _) in DECKS.items():
        d = make_deck(nxe, nze, nxb, nzb, NT, seed=3)
        x0, x1, z0, z1 = born_cells(d)
        for numerics in (0, 1):
            ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
            if deck == "flush":
                assert ctx.pitch == nze
            if deck == "static-rows":
                assert extents_of(d)[0] < nxe - nxb
            for xchunk in (0, seam_xchunk(x1 - x0)):
                ctx.set_tuning(xchunk=xchunk)
                if xchunk:
                    used, chunks = F.plan_ext_image(x0, x1, z1 - z0, H, xchunk)
                    assert len(chunks) >= 3 and chunks[-1]["c1"] - chunks[-1]["c0"] == 1, (deck, xchunk)
                for shift in (0, 1):
                    seed += 1
                    run_term(ctx, d, H, seed, f"{deck} numerics {numerics} H {H} xchunk {xchunk} shift {shift}", shift)
            ctx.close()
    for rows in sorted({1, 2, 2 * H, 2 * H + 1, 2 * H + 2, 64} - {0}):
        for cols, shift in ((65, 0), (63, 1)):
            d = plain_deck(rows, cols)
            ctx = F.FDWave(*args_of(d), compat=False, device=0)
            seed += 1
            case = noise_case(d, H, seed)
            got = run_term(ctx, d, H, seed, f"C of {rows} rows x {cols} H {H} shift {shift}", shift, case=case).planes()
            for j in range(2 * H + 1):      # the short ones leave the outer planes wholly untouched
                if 2 * abs(j - H) >= rows:
                    assert_bit_equal(got[j], case[2][j], f"plane {j} of a C of {rows} rows")
            ctx.close()
    for cols in (1, 63, 64, 65, 256, 257):
        for shift in (0, 1):
            d = plain_deck(2 * H + 2, cols)
            ctx = F.FDWave(*args_of(d), compat=False, device=0)
            ctx.set_tuning(xchunk=1 if cols == 257 else 0)
            seed += 1
            run_term(ctx, d, H, seed, f"C of {2 * H + 2} x {cols} columns H {H} shift {shift}", shift)
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [0, 2, 8])
def test_pointwise_form_gives_the_same_bytes(H, monkeypatch):
    """FDW_EXT_POINTWISE=1 (read when a context is created): one thread per cell."""
    monkeypatch.setenv("FDW_EXT_POINTWISE", "1")
    for deck in ("static-rows", "flush"):
        nxe, nze, nxb, nzb, _ = DECKS[deck]
        d = make_deck(nxe, nze, nxb, nzb, NT, seed=3)
        ctx = F.FDWave(*args_of(d), compat=True, device=0)
        run_term(ctx, d, H, 900 + H, f"pointwise {deck} H {H}")
        ctx.close()


@functools.lru_cache(maxsize=None)
def class_case(H):
    """f, r and the entry planes made of value classes on the "87x70" deck: subnormals, both zeros, tiny and large values (products of two
    values near 2^60 overflow), the overflowing class, planted infinities and NaNs; a block where the term is -0.0 (+) +0.0; -0.0 in the |h|
    rows at either end of C, where nothing is added."""
    import value_classes as V
    nxe, nze, nxb, nzb, _ = DECKS["87x70"]
    d = make_deck(nxe, nze, nxb, nzb, NT, seed=3)
    x0, x1, z0, z1 = born_cells(d)
    xc, zc = V.deck_cuts(d, np.random.default_rng(H), 3)
    f = V.patched((nxe, nze), 10 + H, classes=V.CLASSES, xcuts=xc, zcuts=zc)
    r = V.patched((nxe, nze), 20 + H, classes=V.CLASSES, xcuts=xc, zcuts=zc)
    E0 = np.stack([V.patched((nxe, nze), 30 + H + j, classes=V.FINITE, xcuts=xc, zcuts=zc) for j in range(2 * H + 1)])
    f[x0 + 20:x0 + 23, z0 + 5:z0 + 9] = np.inf
    r[x0 + 30:x0 + 33, z0 + 5:z0 + 9] = -np.inf
    f[x0 + 40:x0 + 42, z0 + 11:z0 + 15] = np.nan
    r[x0 + 44:x0 + 46, z0 + 21:z0 + 25] = np.nan
    blk = (slice(x0 + 24, x0 + 30), slice(z0 + 30, z0 + 38))      # -0.0 (+) (+0.0 (*) 1.0) = +0.0
    f[blk], r[blk] = 0.0, 1.0
    E0[(slice(None),) + blk] = -0.0
    E0[:, x0:x0 + max(H, 1), z0:z1] = -0.0
    E0[:, x1 - max(H, 1):x1, z0:z1] = -0.0
    want = ext_term_fields(d, E0, f, r, H)
    c = V.classify(want[:, x0:x1, z0:z1])
    assert all(c[k] > 0 for k in ("nan", "inf", "subnormal", "pzero", "nzero", "tiny", "large", "normal")), c
    assert (want[H][blk].view(np.uint32) == 0).all(), "-0.0 (+) +0.0 is +0.0"
    for j in range(2 * H + 1):
        h = abs(j - H)
        if h:
            assert (want[j, x0:x0 + h, z0:z1].view(np.uint32) == 0x80000000).all() and (want[j, x1 - h:x1, z0:z1].view(np.uint32) == 0x80000000).all()
    for a in (f, r, E0, want):
        a.setflags(write=False)
    return d, f, r, E0, want, blk


@pytest.mark.parametrize("H", [0, 3, 8])
def test_value_class_case_holds_every_class(H):
    """On the CPU: the restatement's planes of the value-class case hold every class (asserted where the case is built)."""
    want = class_case(H)[4]
    assert want.shape[0] == 2 * H + 1


@pytest.mark.gpu
@pytest.mark.parametrize("H", [0, 3, 8])
def test_value_classes_travel_as_the_restatement_says(H):
    import value_classes as V
    d, f, r, E0, want, blk = class_case(H)
    x0, x1, z0, z1 = born_cells(d)
    for shift in (0, 1):
        ctx = F.FDWave(*args_of(d), compat=True, device=0)
        ctx.set_tuning(xchunk=7)
        dv = Planes(ctx, f, r, E0, shift)
        dv.term(H)
        got = dv.planes()
        V.assert_same_nonfinite(got, want, f"value classes H {H} shift {shift}")
        assert (got[H][blk].view(np.uint32) == 0).all()
        for j in range(2 * H + 1):
            h = abs(j - H)
            if h:
                assert (got[j, x0:x0 + h, z0:z1].view(np.uint32) == 0x80000000).all(), "-0.0 survives where nothing is added"
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [1, 4, 8])
def test_swapping_the_inputs_mirrors_the_planes(H):
    nxe, nze, nxb, nzb, _ = DECKS["wide"]
    d = make_deck(nxe, nze, nxb, nzb, NT, seed=3)
    f, r, E0 = noise_case(d, H, 40 + H)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    a, b = Planes(ctx, f, r, E0), Planes(ctx, f, r, mirrored(E0))
    a.term(H)
    b.term(H, swap=True)
    ea, eb = a.planes(), b.planes()
    assert_bit_equal(ea, mirrored(eb), f"E_(f,r)[h] == E_(r,f)[-h], H {H}")
    assert (ea[0] != ea[2 * H]).any()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: whole shots
# ---------------------------------------------------------------------------------------------------------------------------------------
HS = 3


@functools.lru_cache(maxsize=None)
def shot_case(deck, order, numerics):
    """Deck, wavelet, two gathers, entry planes and the restatement's planes after one shot and after two stacked ones; never modified."""
    nxe, nze, nxb, nzb, _ = DECKS[deck]
    d = make_deck(nxe, nze, nxb, nzb, NT, seed=3, order=order, dx=10.0, dz=12.5)
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    srce = O.ricker_wavelet(NT, 0.001, 120.0) * 1000.0
    rng = np.random.default_rng(2)
    d_obs = rng.standard_normal((2, nx, NT)).astype(f32)
    entry = rng.standard_normal((2 * HS + 1, nx, nz)).astype(f32)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    P, PP = orc.forward(d["v2"], d["sx"], d["sz"], srce)
    P2, PP2 = orc.forward(d["v2"], d["sx"] + 5, d["sz"], srce)
    E0 = np.zeros((2 * HS + 1, nxe, nze), f32)
    inner(d, E0)[...] = entry
    one = ext_back_restatement(orc, d, d["v2"], P, PP, np.ascontiguousarray(d_obs[0].T[::-1]), d["gz"], HS, E0=E0)
    two = ext_back_restatement(orc, d, d["v2"], P2, PP2, np.ascontiguousarray(d_obs[1].T[::-1]), d["gz"], HS, E0=one["E"])
    zero = ext_back_restatement(orc, d, d["v2"], P, PP, np.ascontiguousarray(d_obs[0].T[::-1]), d["gz"], 0)
    want = dict(one=inner(d, one["E"]).copy(), two=inner(d, two["E"]).copy(), zero=inner(d, zero["E"]).copy())
    for a in (srce, d_obs, entry) + tuple(want.values()):
        a.setflags(write=False)
    return d, srce, d_obs, entry, want


def interior_cells(d):
    """C in interior coordinates."""
    x0, x1, z0, z1 = born_cells(d)
    return slice(x0 - d["nxb"], x1 - d["nxb"]), slice(z0 - d["nzb"], z1 - d["nzb"])


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("order,tuning", CONFIGS, ids=str)
def test_shot_ext_vs_restatement(order, tuning, numerics):
    """fdw_shot_ext on the four decks: the planes against the restatement (entry planes of noise), h = 0 against fdw_shot's imloc on the
    interior cells of C, imloc / P / PP against fdw_shot, two shots stacked into one eimg, H = 0, and a smaller H after a larger one."""
    for deck, (_, _, _, _, xchunk) in DECKS.items():
        d, srce, d_obs, entry, want = shot_case(deck, order, numerics)
        what = f"{deck} order {order} {tuning} numerics {numerics}"
        place = (d["sx"], d["sz"], d["gz"])
        ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
        ctx.set_tuning(xchunk=xchunk, **tuning)
        got = ctx.shot_ext(d["v2"], *place, srce, d_obs[0], HS, eimg=entry, want_fields=True)
        assert_bit_equal(got["eimg"], want["one"], "planes, " + what)
        img, P, PP = ctx.shot(d["v2"], *place, srce, d_obs[0], want_fields=True)
        for k, a in (("image", img), ("P", P), ("PP", PP)):
            assert_bit_equal(got[k], a, f"{k} vs fdw_shot, " + what)
        C = interior_cells(d)
        fresh = ctx.shot_ext(d["v2"], *place, srce, d_obs[0], HS)
        assert_bit_equal(fresh["eimg"][HS][C], img[C], "plane h = 0 vs fdw_shot's imloc on C, " + what)
        assert img[C].any()
        # a second shot stacked into the same planes; no image asked for
        again = ctx.shot_ext(d["v2"], place[0] + 5, place[1], place[2], srce, d_obs[1], HS, eimg=got["eimg"], want_image=False)
        assert_bit_equal(again["eimg"], want["two"], "two shots stacked, " + what)
        assert "image" not in again
        # H = 0 after H = 3: one plane, nothing of the larger call's planes leaks
        zero = ctx.shot_ext(d["v2"], *place, srce, d_obs[0], 0)
        assert_bit_equal(zero["eimg"], want["zero"], "H = 0 after H = 3, " + what)
        assert_bit_equal(zero["eimg"][0][C], img[C], "H = 0 vs fdw_shot's imloc on C, " + what)
        ctx.close()


@pytest.mark.gpu
def test_shot_ext_on_the_resident_model_and_the_other_families():
    d, srce, d_obs, entry, want = shot_case("wide", 8, 0)
    place = (d["sx"], d["sz"], d["gz"])
    for two_step in (4, 1):      # contexts whose fdw_shot runs the pipeline / pairs: the extended loop runs one-step iterations
        ctx = F.FDWave(*args_of(d), compat=True, device=0)
        ctx.set_tuning(two_step=two_step)
        got = ctx.shot_ext(d["v2"], *place, srce, d_obs[0], HS, eimg=entry)
        assert_bit_equal(got["eimg"], want["one"], f"two_step {two_step}")
        assert_bit_equal(got["image"], ctx.shot(d["v2"], *place, srce, d_obs[0]), f"image, two_step {two_step}")
        ctx.close()
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    vp = np.sqrt(inner(d, d["v2"])).astype(f32)
    ctx.model_resident(vp)
    vel = ctx.dev_extendvel_linear(0, want_vel=True)
    v2 = (vel * vel).astype(f32)
    orc = O.Oracle(*args_of(d), compat=True)
    P, PP = orc.forward(v2, place[0], place[1], srce)
    r = ext_back_restatement(orc, d, v2, P, PP, np.ascontiguousarray(d_obs[0].T[::-1]), place[2], 2)
    got = ctx.shot_ext(None, *place, srce, d_obs[0], 2)
    assert_bit_equal(got["eimg"], inner(d, r["E"]), "resident model")
    assert_bit_equal(got["image"], ctx.shot_resident(*place, srce, d_obs[0]), "image on the resident model")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the stream contract (a late producer) and the footprint (a guarded arena) of fdw_dev_ext_image, through tests/stream_cases.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def _stream_case(numerics=0, H=2):
    import stream_cases as S
    deck = "ragged"

    def planes(i):
        return np.concatenate([i[k] for k in ("img0", "lap_in", "il0", "amp_img", "exc0")][:2 * H + 1])

    def ins(i):
        return dict(FS=("field", i["f1"]), RS=("field", i["pr"]), E=("field", planes(i)))

    def call(ctx, p, stream):
        ctx.dev_ext_image(p["FS"], p["RS"], H, p["E"], stream=stream)
        return [("eimg", "E", None, None)]

    def want(v):
        i = S.inputs(deck, v)
        nxe, nze = i["d"]["nxe"], i["d"]["nze"]
        return dict(eimg=ext_term_fields(i["d"], planes(i).reshape(2 * H + 1, nxe, nze), i["f1"], i["pr"], H).reshape(-1, nze))

    return S.Case("ext_image-" + deck, deck, numerics, -1, ins, {}, call, want, pad_words=dict(E=PAD))


@pytest.mark.gpu
def test_late_producer_on_the_callers_stream():
    """Decoys in every input; behind 40 ms of delay on the caller's stream the true fields and planes are copied in, then the entry point,
    then the planes copied out: the answer is that of the true inputs, and the call returned while the stream was still busy."""
    import torch

    import stream_cases as S
    case_ = _stream_case()
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
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
def test_guarded_arena_footprint(numerics):
    """Every buffer carved from one arena with NaN guard bands: guards and padding columns intact (the planes' sentinel too), d_f and d_r
    unchanged, every plane changed on its rows of C only."""
    import torch

    import footprint_arena as A
    import stream_cases as S
    H = 2
    case_ = _stream_case(numerics, H)
    i = S.inputs("ragged", "true")
    arena = A.build(case_, i)
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
    assert_bit_equal(got["eimg"], want["eimg"], "arena: planes")
    nxe, nze = i["d"]["nxe"], i["d"]["nze"]
    x0, x1, z0, z1 = born_cells(i["d"])
    changed = (got["eimg"] != case_.ins(i)["E"][1]).reshape(2 * H + 1, nxe, nze)
    for j in range(2 * H + 1):
        h = abs(j - H)
        assert changed[j, x0 + h:x1 - h, z0:z1].mean() > 0.9
        changed[j, x0 + h:x1 - h, z0:z1] = False
    assert not changed.any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: refusals enqueue nothing
# ---------------------------------------------------------------------------------------------------------------------------------------
def refused(code, fn, *a, **k):
    with pytest.raises(F.FdwError) as e:
        fn(*a, **k)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


@pytest.mark.gpu
def test_refusals_enqueue_nothing():
    nxe, nze, nxb, nzb, _ = DECKS["87x70"]
    d = make_deck(nxe, nze, nxb, nzb, NT, seed=3)
    f, r, E0 = noise_case(d, 2, 7)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    dv = Planes(ctx, f, r, E0)
    before = {k: dv.whole(k).copy() for k in ("f", "r", "E")}
    p = dv.ptr
    fb = nxe * ctx.pitch * 4
    refused(EINVAL, ctx.dev_ext_image, None, p("r"), 2, p("E"))
    refused(EINVAL, ctx.dev_ext_image, p("f"), None, 2, p("E"))
    refused(EINVAL, ctx.dev_ext_image, p("f"), p("r"), 2, None)
    refused(EINVAL, ctx.dev_ext_image, p("f"), p("r"), -1, p("E"))
    refused(EINVAL, ctx.dev_ext_image, p("f"), p("r"), HMAX + 1, p("E"))
    assert "overlap" in refused(EINVAL, ctx.dev_ext_image, p("E") + 4 * fb, p("r"), 2, p("E"))      # an input that is the last plane
    assert "overlap" in refused(EINVAL, ctx.dev_ext_image, p("f"), p("E") + 64, 2, p("E"))
    assert "overlap" in refused(EINVAL, ctx.dev_ext_image, p("f"), p("r"), 0, p("r"))
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    srce, d_obs = np.zeros(NT, f32), np.zeros((nx, NT), f32)
    place = (d["sx"], d["sz"], d["gz"])
    refused(EINVAL, ctx.shot_ext, d["v2"], *place, srce, d_obs, HMAX + 1)
    refused(EINVAL, ctx.shot_ext, d["v2"], *place, srce, d_obs, -1)
    assert F.lib().fdw_shot_ext(ctx._h, d["v2"].ctypes.data, *place, srce, d_obs, 2, None, None, None, None) == EINVAL
    assert "resident" in refused(ESTATE, ctx.shot_ext, None, *place, srce, d_obs, 2)
    stored = F.FDWave(*args_of(d), compat=False, device=0, dialect=2)
    assert "dialect" in refused(ESTATE, stored.dev_ext_image, p("f"), p("r"), 2, p("E"))
    assert "dialect" in refused(ESTATE, stored.shot_ext, d["v2"], *place, srce, d_obs, 2)
    stored.close()
    slab = F.FDWave(*args_of(d), compat=True, device=0, slab=(0, nxe // 2 + 8))
    assert "slab" in refused(ESTATE, slab.dev_ext_image, p("f"), p("r"), 2, p("E"))
    assert "slab" in refused(ESTATE, slab.shot_ext, d["v2"], *place, srce, d_obs, 2)
    slab.close()
    for k in before:
        assert (dv.whole(k) == before[k]).all(), f"{k} after the refusals"
    # all-zero data leave every plane as it came (the receiver field stays zero; entry planes of noise)
    entry = np.random.default_rng(8).standard_normal((5, nx, nz)).astype(f32)
    got = ctx.shot_ext(d["v2"], *place, O.ricker_wavelet(NT, 0.001, 120.0) * 1000.0, d_obs, 2, eimg=entry)
    assert_bit_equal(got["eimg"], entry, "all-zero data")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the program: rtm_code's deck key ext=H
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rtm_code_ext(tmp_path):
    """ext=2 on a two-shot deck: dir.image_ext is two fdw_shot_ext calls stacked into one eimg on the program's own border models,
    dir.image what the run without the key writes; ext=0 changes nothing."""
    from test_residual import _run, _two_shot_deck
    nx, nz, nxb, nzb, nt, ns, ds = 50, 37, 10, 9, 47, 2, 20
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    rng = np.random.default_rng(11)
    vp = (1500 + 2500 * np.linspace(0, 1, nz, dtype=f32)[None, :] + 100 * rng.standard_normal((nx, nz))).astype(f32)
    dobs = rng.standard_normal((ns, nx, nt)).astype(f32)
    runs = {}
    for name, extra in (("plain", ""), ("ext", "ext=2\n"), ("off", "ext=0\n")):
        c = tmp_path / name
        _two_shot_deck(c, vp, extra)
        dobs.tofile(c / "models" / "dobs.bin")
        runs[name], r = _run("rtm_code", c)
        assert ("## ext = 2" in r.stdout) == (name == "ext"), name
        if name != "plain":
            assert (c / "image.num").read_bytes() == (tmp_path / "plain" / "image.num").read_bytes(), name
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    ctx.model_resident(vp)
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    eimg = np.zeros((5, nx, nz), f32)
    for s in range(ns):
        ctx.dev_extendvel_linear(s * ctx.border_draws())
        eimg = ctx.shot_ext(None, 5 + s * ds + nxb, 1 + nzb, 2 + nzb, srce, dobs[s], 2, eimg=eimg)["eimg"]
    ctx.close()
    assert eimg.any() and all(eimg[j].any() for j in range(5))
    assert runs["ext"]["dir.image_ext"] == eimg.tobytes()
    assert sorted(runs["ext"]) == sorted(set(runs["plain"]) | {"dir.image_ext"})
    assert sorted(runs["off"]) == sorted(runs["plain"])
    for f in runs["plain"]:
        assert runs["off"][f] == runs["plain"][f], f
        assert runs["ext"][f] == runs["plain"][f], f

"""Second-time-difference imaging (fdwave.h, "DTT imaging"): fdw_dev_back_iter_dtt, fdw_dev_dtt_image, fdw_shot_dtt and its line and batched
forms, the two host weights.

The restatement (tests/dtt_restatement.py) takes its fields from Oracle.slab_back_iter with a throwaway image and forms the image in
np.float32; the GPU is held to it bit for bit, on every word of the image (C against the restatement, every other word untouched, sentinels
in the padding columns), and the two field pairs to fdw_dev_back_iter on copies."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from born_restatement import DTT, born_cells, born_restatement, embed_m
from conftest import ROOT, assert_bit_equal, make_deck, random_fields
from dtt_restatement import dtt_back_restatement
from oracle import oracle as O
from test_born import CONFIGS, DECKS
from test_line_source import args_of, extents_of
from test_stepn_isa_budget import isa  # noqa: F401  (a fixture)

EINVAL, ESTATE = -1, -5
NIT = 7                                                  # iterations of the device-level runs; restarted after 4
PAD = 0x7FC0D77A                                         # what the padding columns of the image hold
f32 = np.float32


def inner(d, a):
    return a[d["nxb"]:d["nxe"] - d["nxb"], d["nzb"]:d["nze"] - d["nzb"]]


@functools.lru_cache(maxsize=None)
def case(deck, order, numerics, nsteps=NIT):
    """Deck, noise snapshots, a noise receiver pair, a noise image (every word of the field), a noise gather and the restatement's answer;
    never modified."""
    nxe, nze, nxb, nzb, _ = DECKS[deck]
    d = make_deck(nxe, nze, nxb, nzb, NIT, seed=3, order=order, dx=10.0, dz=12.5)
    F1, F0 = random_fields(d, 5, amp=0.1)
    R0 = random_fields(d, 6, amp=0.1)
    rng = np.random.default_rng(11)
    img0 = rng.standard_normal((nxe, nze)).astype(f32)
    samples = rng.standard_normal((NIT, nxe - 2 * nxb)).astype(f32)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    want = dtt_back_restatement(orc, d, d["v2"], F1, F0, samples, d["gz"], img0=img0, pr=R0[0], ppr=R0[1], nsteps=nsteps)
    want["R0"] = R0
    for a in (F1, F0, img0, samples, d["v2"], want["img"]) + R0:
        a.setflags(write=False)
    return d, F1, F0, img0, samples, want


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement's guards, the built library
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("deck", ["87x70", "static-rows"])
def test_restatement_chain_is_oracle_back(deck, numerics):
    """The throwaway image of the restatement's chain is Oracle.back's image; the source pair it leaves is the reconstruction."""
    nxe, nze, nxb, nzb, _ = DECKS[deck]
    nt = 9
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=3, order=8)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    P, PP = orc.forward(d["v2"], d["sx"], d["sz"], O.ricker_wavelet(nt, 0.001, 120.0) * 1000.0)
    d_obs = np.random.default_rng(2).standard_normal((nxe - 2 * nxb, nt)).astype(f32)
    r = dtt_back_restatement(orc, d, d["v2"], P, PP, d_obs.T[::-1], d["gz"])
    assert_bit_equal(inner(d, r["xcorr"]), orc.back(d["v2"], P, PP, d_obs, d["gz"]), "the chain's cross-correlation image")
    assert inner(d, r["img"]).any() and (inner(d, r["img"]) != inner(d, r["xcorr"])).any()


def test_restatement_tail_is_the_plain_step_on_a_damped_deck():
    """The tail's slab_step(sx = -1, taper_rows = (0, 0)) equals the source half of two more slab_back_iter(step_source = 1) calls."""
    d, F1, F0, img0, samples, want = case("87x70", 8, 0)
    assert extents_of(d)[2] > 0, "the deck has damped columns"
    orc = O.Oracle(*args_of(d), compat=True)
    nxe, nze = d["nxe"], d["nze"]
    f1, f0 = want["f_new"].copy(), want["f_old"].copy()
    g1, g0 = f1.copy(), f0.copy()
    z = lambda: np.zeros((nxe, nze), f32)      # noqa: E731
    x0, x1, z0, z1 = born_cells(d)
    for lvl in (NIT, NIT + 1):
        nxt = g0.copy()
        orc.slab_step(0, g1, nxt, d["v2"], 0, nxe, -1, 0, 0.0, taper_rows=(0, 0))
        g1, g0 = nxt, g1
        orc.slab_back_iter(0, 1, f1, f0, z(), z(), d["v2"], 0, nxe, np.zeros(nxe - 2 * d["nxb"], f32), d["gz"], z())
        f1, f0 = f0, f1
        assert_bit_equal(g1, f1, f"F_{lvl}")
        assert_bit_equal(g1[x0:x1, z0:z1], want["F"][lvl], f"F_{lvl} on C")


def test_zero_data_leaves_every_word_of_the_image():
    d, F1, F0, img0, samples, want = case("static-rows", 8, 0)
    orc = O.Oracle(*args_of(d), compat=True)
    r = dtt_back_restatement(orc, d, d["v2"], F1, F0, np.zeros_like(samples), d["gz"], img0=img0)      # (receivers at rest)
    assert_bit_equal(r["img"], img0, "image after an all-zero gather")
    x0, x1, z0, z1 = born_cells(d)
    changed = want["img"] != img0
    assert changed[x0:x1, z0:z1].mean() > 0.5
    changed[x0:x1, z0:z1] = False
    assert not changed.any(), "the noise gather changes C only"


def test_every_dtt_symbol_is_exported_and_mirrored():
    L = F.lib()
    for name in ("fdw_dev_back_iter_dtt", "fdw_dev_dtt_image", "fdw_shot_dtt", "fdw_shot_line_dtt", "fdw_shot_batch_dtt", "fdw_shot_line_batch_dtt",
                 "fdw_gather_scale_v2", "fdw_image_unscale_v2"):
        assert hasattr(L, name), name
        assert name + "(" in open(os.path.join(ROOT, "include", "fdwave.h")).read(), name
    for name in ("dev_back_iter_dtt", "dev_dtt_image", "shot_dtt", "shot_line_dtt", "shot_batch_dtt", "shot_line_batch_dtt"):
        assert hasattr(F.FDWave, name), name
    assert F.IMAGE_DTT == 1 and F.IMAGE_XCORR == 0


def test_host_weights_are_one_fp32_operation_per_word_and_alias():
    rng = np.random.default_rng(4)
    nxe, nze, nxb, nzb, nt = 23, 19, 3, 4, 6
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    v2 = (1e6 * (1 + rng.random((nxe, nze)))).astype(f32)
    g, img = rng.standard_normal((nx, nt)).astype(f32), rng.standard_normal((nx, nz)).astype(f32)
    assert_bit_equal(F.gather_scale_v2(v2, nxb, 5, g), g * v2[nxb:nxb + nx, 5:6], "gather weight")
    assert_bit_equal(F.image_unscale_v2(v2, nxb, nzb, img), img / v2[nxb:nxb + nx, nzb:nzb + nz], "image weight")
    a, b = g.copy(), img.copy()
    assert F.lib().fdw_gather_scale_v2(v2, nxe, nze, nxb, 5, nx, nt, a, a) == 0 and F.lib().fdw_image_unscale_v2(v2, nxe, nze, nxb, nzb, nx, nz, b, b) == 0
    assert_bit_equal(a, g * v2[nxb:nxb + nx, 5:6], "in place")
    assert_bit_equal(b, img / v2[nxb:nxb + nx, nzb:nzb + nz], "in place")
    assert F.lib().fdw_gather_scale_v2(v2, nxe, nze, nxb, nze, nx, nt, a, a) == EINVAL


def test_dtt_kernels_exist_in_both_numerics_without_scratch(isa):      # noqa: F811
    names = [k for k in isa if "fdw_step_back_dtt_kernel" in k or "fdw_dtt_image_kernel" in k]
    for h in (1, 2, 3, 4):
        for num in (0, 1):
            assert any(f"fdw_step_back_dtt_kernelILi{h}ELi2ELi{num}EEEv" in k for k in names), (h, num, names)
    for pf in (1, 3):
        assert any(f"fdw_step_back_dtt_kernelILi4ELi{pf}ELi0EEEv" in k for k in names), pf
    assert any("fdw_dtt_image_kernelE" in k for k in names)
    assert len(names) == 11, names
    for k in names:
        meta = isa[k][0]
        print(k, {f: meta.get(f) for f in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count")})
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (k, meta)
        assert not any(mn.startswith("scratch_") for mn, _ in isa[k][1]), k


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: exact adjointness (the physics of the definition, on the restatements alone)
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dot_products():
    nt = 60
    d = make_deck(96, 88, 6, 7, nt)
    assert extents_of(d)[2] == 0, "ztap 0: no damped column"
    nxe, nze, nxb, nzb = d["nxe"], d["nze"], d["nxb"], d["nzb"]
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    sx, sz = nxb + nx // 2, nzb + nz // 2
    gz = sz - 3
    srce = np.zeros(nt, f32)
    srce[:2] = 1.0, -0.5
    m = (0.3 * np.random.default_rng(3).standard_normal((nx, nz))).astype(f32)
    m[sx - nxb - 12:sx - nxb + 13, sz - nzb - 12:sz - nzb + 13] = 0
    w = np.random.default_rng(7).standard_normal((nt, nx)).astype(f32)
    orc = O.Oracle(*args_of(d), compat=True)
    v2 = d["v2"].astype(np.float64)
    rec = born_restatement(orc, d, d["v2"], embed_m(d, m), DTT, sx, sz, gz, srce)["rec"].astype(np.float64)
    lhs = float((rec * w).sum())
    scale = float(np.linalg.norm(rec) * np.linalg.norm(w.astype(np.float64)))
    ws = (w.astype(np.float64) * v2[nxb:nxb + nx, gz][None, :]).astype(f32)
    P, PP = orc.forward(d["v2"], sx, sz, srce)
    out = {}
    for name, pairing, acc in (("fp32", 1, None), ("fp64", 1, np.float64), ("off-by-one", 0, np.float64)):
        img = dtt_back_restatement(orc, d, d["v2"], P, PP, ws[::-1], gz, pairing=pairing, accumulate=acc)["img"]
        rhs = float((m.astype(np.float64) * inner(d, img).astype(np.float64) / inner(d, v2)).sum())
        out[name] = abs(lhs - rhs) / scale
        out[name + ", by |lhs|"] = abs(lhs - rhs) / abs(lhs)
    out["cos"] = abs(lhs) / scale
    return out


def test_dtt_image_is_the_exact_adjoint_of_dtt_born_modelling():
    """<Born_DTT(m), w> against <m, (1/v2) Image_DTT(v2_rec w)> on the restatements alone: 96 x 88, borders 6 / 7 (no damped column), 60 steps,
    srce = [1, -0.5, 0, ...] at the interior centre, gz three cells above it, m zero within 12 cells of the source, a white gather, the two
    weights applied in float64.
    The mismatch |lhs - rhs| is taken relative to |Born_DTT(m)| |w|, the scale the rounding error of a dot product follows: a white gather
    is nearly orthogonal to the data (here cos = |lhs| / (|d| |w|) = 1.1e-3; 3e-4 to 7e-3 over five seeds of w), so a figure relative to
    |lhs| carries that chance factor of 10^2 to 10^3.5 on top of the fp32 rounding it is meant to show, and no bound on it separates rounding
    from a wrong pairing for every w.
    Measured with this restatement (w: seed 7): 3.7e-8 with the image summed in fp32 as defined, 3.8e-8 summed in fp64; the pairing q_k
    with r^k: 7.7e-3.  (Relative to |lhs| the same three read 3.3e-5, 3.3e-5 and 6.7; over the seeds 1 to 4 of w the first is 3.2e-5,
    2.7e-4, 1.8e-6, 1.2e-4, while relative to the norms it stays between 1.3e-8 and 8.6e-8.)
    Asserted: below 1e-5 for the pairing of the definition; the pairing q_k with r^k misses the same bound.  (The test cannot see the tail:
    q_0 and q_1 live where m is zero; the bit-exact GPU tests pin it.)"""
    e = _dot_products()
    print("dot-product mismatch: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["fp32"] < 1e-5 and e["fp64"] < 1e-5, e
    assert e["off-by-one"] > 1e-5, e


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the device state of one run
# ---------------------------------------------------------------------------------------------------------------------------------------
class Device:
    """The source pair, the receiver pair (R0; None: at rest), two spare fields, v2, the image (noise, sentinels in the padding columns) and the sample
    rows on the device; `twin`: the same without the DTT image, for fdw_dev_back_iter on copies."""

    def __init__(self, ctx, d, F1, F0, img0, samples, state=None, R0=None):
        import torch
        self.torch, self.ctx, self.d, self.nze = torch, ctx, d, d["nze"]
        dev = torch.device("cuda:0")

        def field(a, pad=0):
            h = np.full((d["nxe"], ctx.pitch), pad, np.uint32)
            h[:, :self.nze] = np.ascontiguousarray(a, f32).view(np.uint32)
            return torch.from_numpy(h.view(f32)).to(dev)
        zero = np.zeros((d["nxe"], d["nze"]), f32)
        if state is None:
            R0 = (zero, zero) if R0 is None else R0
            self.f = dict(f1=field(F1), f0=field(F0), pr=field(R0[0]), ppr=field(R0[1]), s0=field(zero), s1=field(zero), v2=field(d["v2"]), img=field(img0, PAD))
        else:                                                      # a restart: the words another context's run left
            self.f = {k: torch.from_numpy(v.copy()).to(dev) for k, v in state.items()}
        self.samples = torch.from_numpy(np.array(samples, f32, order="C")).to(dev)
        self.names = dict(f1="f1", f0="f0", pr="pr", ppr="ppr")      # which buffer holds which role
        torch.cuda.synchronize()

    def ptr(self, role):
        return self.f[self.names.get(role, role)].data_ptr()

    def iterate(self, k, dtt=True, stream=None):
        """Iteration k as back_loop issues it."""
        n = self.names
        call = self.ctx.dev_back_iter_dtt if dtt else self.ctx.dev_back_iter
        first = n["f0"] if k == 0 else n["f1"]
        call(k >= 2, self.f[first].data_ptr(), self.ptr("f0"), self.ptr("pr"), self.ptr("ppr"), self.ptr("v2"), 0, self.d["nxe"], k > 0,
             self.samples[k].data_ptr(), self.d["gz"], self.ptr("img"), stream=stream)
        if k >= 2:
            n["f1"], n["f0"] = n["f0"], n["f1"]
        n["pr"], n["ppr"] = n["ppr"], n["pr"]

    def tail(self, nsteps, stream=None):
        """What fdwave.h tells a device caller: fdw_dev_step(mode 1) into a copy of the older level, then fdw_dev_dtt_image."""
        n = self.names
        lv = [n["f0"], n["f1"], "s0", "s1"]
        r = [n["ppr"], n["pr"]]
        nterms = 2 if nsteps >= 2 else (1 if nsteps == 1 else 0)
        for t in range(nterms):
            self.f[lv[t + 2]].copy_(self.f[lv[t]])
            self.torch.cuda.synchronize()
            self.ctx.dev_step(F.MODE_PLAIN, self.f[lv[t + 1]].data_ptr(), self.f[lv[t + 2]].data_ptr(), self.ptr("v2"), 0, self.d["nxe"], False, stream=stream)
            self.ctx.dev_dtt_image(self.f[lv[t]].data_ptr(), self.f[lv[t + 1]].data_ptr(), self.f[lv[t + 2]].data_ptr(),
                                   self.f[r[t if nterms == 2 else 1]].data_ptr(), self.ptr("img"), stream=stream)

    def state(self):
        self.torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.f.items()}

    def whole(self, role):
        self.torch.cuda.synchronize()
        return self.f[self.names.get(role, role)].cpu().numpy()


def check_image(dv, c, what, same=assert_bit_equal):
    """Every word of the device image: C against the restatement, the rest as it came (bit for bit), the sentinels in the padding columns.
    same: the comparison with the restatement (value_classes.assert_same_nonfinite where the deck holds NaNs)."""
    d, F1, F0, img0, samples, want = c
    got = dv.whole("img")
    assert (got[:, d["nze"]:].view(np.uint32) == PAD).all(), "padding columns of the image, " + what
    same(got[:, :d["nze"]], want["img"], "image, " + what)
    x0, x1, z0, z1 = born_cells(d)
    out = np.ones(img0.shape, bool)
    out[x0:x1, z0:z1] = False
    assert_bit_equal(got[:, :d["nze"]][out], img0[out], "image outside C, " + what)


def run_and_check(make_ctx, c, what, restart=None, nsteps=NIT, same=assert_bit_equal):
    """nsteps iterations and the tail (restart: a fresh context and fresh buffers holding the same words after that many iterations) against the
    restatement; both field pairs against fdw_dev_back_iter on copies."""
    d, F1, F0, img0, samples, want = c
    ctx = make_ctx()
    dv = Device(ctx, d, F1, F0, img0, samples, R0=want["R0"])
    tw = Device(ctx, d, F1, F0, img0, samples, R0=want["R0"])
    for k in range(nsteps):
        if restart is not None and k == restart:
            state, names = dv.state(), dict(dv.names)
            ctx2 = make_ctx()
            dv = Device(ctx2, d, F1, F0, img0, samples, state=state)
            dv.names = names
        dv.iterate(k)
        tw.iterate(k, dtt=False)
    dv.torch.cuda.synchronize()
    for role in ("f1", "f0", "pr", "ppr", "v2"):
        same(dv.whole(role), tw.whole(role), f"{role} vs fdw_dev_back_iter, " + what)
    assert (tw.whole("img") != dv.whole("img")).any()
    dv.tail(nsteps)
    check_image(dv, c, what, same)
    for role in ("f1", "f0", "pr", "ppr", "v2"):
        same(dv.whole(role), tw.whole(role), f"{role} after the tail, " + what)
    return dv


def ctx_maker(d, numerics, xchunk, tuning):
    def make():
        ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
        ctx.set_tuning(xchunk=xchunk, two_step=-1, **tuning)
        return ctx
    return make


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: every kernel, every deck
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("order,tuning", CONFIGS, ids=str)
def test_dev_back_iter_dtt_vs_restatement(order, tuning, numerics):
    """Seven iterations and the tail from noise-filled snapshots, a noise image and a noise gather, in one sequence and restarted after
    iteration 4, on the four decks."""
    for deck, (_, _, _, _, xchunk) in DECKS.items():
        c = case(deck, order, numerics)
        what = f"{deck} order {order} {tuning} numerics {numerics}"
        make = ctx_maker(c[0], numerics, xchunk, tuning)
        run_and_check(make, c, what)
        run_and_check(make, c, what + ", restarted after 4", restart=4)


@pytest.mark.gpu
@pytest.mark.parametrize("nsteps", [0, 1, 2, 3])
def test_short_loops_have_fewer_terms(nsteps):
    c = case("static-rows", 8, 0, nsteps=nsteps)
    d, F1, F0, img0, samples, want = c
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    dv = Device(ctx, d, F1, F0, img0, samples, R0=want["R0"])
    for k in range(nsteps):
        dv.iterate(k)
    if nsteps <= 2:
        assert_bit_equal(dv.whole("img")[:, :d["nze"]], img0, "iterations 0 and 1 leave the image alone")
    dv.tail(nsteps)
    check_image(dv, c, f"nsteps {nsteps}")
    assert (want["img"] != img0).any() == (nsteps > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("two_step", [4, 1])
def test_contexts_of_the_other_families_run_one_step_iterations(two_step):
    c = case("wide", 8, 0)

    def make():
        ctx = F.FDWave(*args_of(c[0]), compat=True, device=0)
        ctx.set_tuning(two_step=two_step)
        return ctx
    run_and_check(make, c, f"two_step {two_step}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: FDW_NO_FUSED_BACK=1 (read when a context is created) in a child process
# ---------------------------------------------------------------------------------------------------------------------------------------
def unfused_child():
    assert os.environ.get("FDW_NO_FUSED_BACK") == "1"
    for order, tuning in ((8, dict(prefetch=2)), (8, dict(prefetch=3)), (4, {})):
        for numerics in (0, 1):
            for deck in ("static-rows", "wide"):
                c = case(deck, order, numerics)
                run_and_check(ctx_maker(c[0], numerics, DECKS[deck][4], tuning), c, f"unfused {deck} order {order} numerics {numerics}", restart=4)
    d, srce, d_obs, v2s, want = shot_case((87, 70, 3, 10), 8, 0)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    assert_bit_equal(ctx.shot_dtt(d["v2"], d["sx"], d["sz"], d["gz"], srce, d_obs)["image"], want["image"], "unfused fdw_shot_dtt")
    print("unfused: ok")


@pytest.mark.gpu
def test_unfused_arrangement_gives_the_same_bytes():
    env = dict(os.environ, FDW_NO_FUSED_BACK="1")
    r = subprocess.run([sys.executable, "-c", "import conftest, test_dtt; test_dtt.unfused_child()"], cwd=os.path.join(ROOT, "tests"), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "unfused: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: whole shots
# ---------------------------------------------------------------------------------------------------------------------------------------
NT_SHOT = 40


def shot_restatement(orc, d, v2, forward, d_obs, gz, imloc=None):
    """The forward oracle (forward: v2 -> (P, PP)) and the restatement's backward loop: the interior image."""
    P, PP = forward(v2)
    img0 = None if imloc is None else embed_m(d, imloc)
    return inner(d, dtt_back_restatement(orc, d, v2, P, PP, np.ascontiguousarray(d_obs.T[::-1]), gz, img0=img0)["img"]).copy()


@functools.lru_cache(maxsize=None)
def shot_case(grid, order, numerics, nshots=1):
    nxe, nze, nxb, nzb = grid
    d = make_deck(nxe, nze, nxb, nzb, NT_SHOT, seed=3, order=order)
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    srce = O.ricker_wavelet(NT_SHOT, 0.001, 120.0) * 1000.0
    rng = np.random.default_rng(2)
    d_obs = rng.standard_normal((nshots, nx, NT_SHOT)).astype(f32)
    v2s = np.stack([d["v2"]] + [(d["v2"] * f32(1.0 + 0.01 * b)).astype(f32) for b in range(1, nshots)])
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    images = np.stack([shot_restatement(orc, d, v2s[b], lambda v, b=b: orc.forward(v, d["sx"] + 2 * b, d["sz"], srce), d_obs[b], d["gz"])
                       for b in range(nshots)])
    want = dict(image=images[0] if nshots == 1 else images)
    return d, srce, (d_obs[0] if nshots == 1 else d_obs), v2s, want


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("order,tuning", [(8, {}), (8, dict(two_step=4)), (12, {})], ids=str)
def test_shot_dtt_from_rest(order, tuning, numerics):
    """fdw_shot_dtt against the forward oracle plus the restatement; with illum, with residual = 1 and on the resident model every other
    output equals the cross-correlation call's."""
    d, srce, d_obs, v2s, want = shot_case((87, 70, 12, 10), order, numerics)
    v2, place = d["v2"], (d["sx"], d["sz"], d["gz"])
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    what = f"order {order} {tuning} numerics {numerics}"
    got = ctx.shot_dtt(v2, *place, srce, d_obs, want_fields=True, want_illum=True)
    assert_bit_equal(got["image"], want["image"], "fdw_shot_dtt image, " + what)
    _, P, PP, illum = ctx.shot(v2, *place, srce, d_obs, want_fields=True, want_illum=True)
    for k, a in (("P", P), ("PP", PP), ("illum", illum)):
        assert_bit_equal(got[k], a, f"{k} vs fdw_shot_illum, " + what)
    # an entry image is added to, on every cell
    entry = np.random.default_rng(9).standard_normal(want["image"].shape).astype(f32)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    again = shot_restatement(orc, d, v2, lambda v: orc.forward(v, place[0], place[1], srce), d_obs, place[2], imloc=entry)
    assert_bit_equal(ctx.shot_dtt(v2, *place, srce, d_obs, imloc=entry)["image"], again, "fdw_shot_dtt onto an entry image, " + what)
    # residual = 1: a gather modelled in the migration model leaves the image untouched; a noisy one migrates the difference
    ref = ctx.shot_residual(v2, *place, srce, d_obs, want_fields=True, want_illum=True)
    res = ctx.shot_dtt(v2, *place, srce, d_obs, residual=True, want_fields=True, want_illum=True)
    for k in ("resid", "P", "PP", "illum"):
        assert_bit_equal(res[k], ref[k], f"{k} vs fdw_shot_residual, " + what)
    assert_bit_equal(res["image"], shot_restatement(orc, d, v2, lambda v: orc.forward(v, place[0], place[1], srce), ref["resid"], place[2]),
                     "residual image, " + what)
    modelled = ctx.record_shot(v2, *place, srce)
    clean = ctx.shot_dtt(v2, *place, srce, modelled, imloc=entry, residual=True)
    assert_bit_equal(clean["image"], entry, "a gather modelled in the migration model, " + what)
    assert not clean["resid"].view(np.uint32).any()
    ctx.close()


@pytest.mark.gpu
def test_shot_dtt_on_the_resident_model_and_the_ragged_deck():
    d, srce, d_obs, v2s, want = shot_case((87, 70, 3, 10), 8, 0)
    place = (d["sx"], d["sz"], d["gz"])
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    assert_bit_equal(ctx.shot_dtt(d["v2"], *place, srce, d_obs)["image"], want["image"], "static receiver rows")
    nxb, nzb = d["nxb"], d["nzb"]
    vp = np.sqrt(inner(d, d["v2"])).astype(f32)
    ctx.model_resident(vp)
    vel = ctx.dev_extendvel_linear(0, want_vel=True)
    v2 = (vel * vel).astype(f32)
    orc = O.Oracle(*args_of(d), compat=True)
    img = shot_restatement(orc, d, v2, lambda v: orc.forward(v, place[0], place[1], srce), d_obs, place[2])
    assert_bit_equal(ctx.shot_dtt(None, *place, srce, d_obs)["image"], img, "resident model")
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
def test_shot_line_dtt(numerics):
    from test_line_source import line_restatement
    d, srce, d_obs, v2s, _ = shot_case((87, 70, 12, 10), 8, numerics)
    nx = d["nxe"] - 2 * d["nxb"]
    wav = (np.random.default_rng(5).standard_normal((nx, NT_SHOT)) * 100.0).astype(f32)
    sz, gz = d["sz"], d["gz"]
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)

    def forward(v):
        r = line_restatement(orc, d, v, np.ascontiguousarray(wav.T), sz, gz=gz)
        return r["P"], r["PP"]
    got = ctx.shot_line_dtt(d["v2"], sz, gz, wav, d_obs, want_fields=True, want_illum=True)
    assert_bit_equal(got["image"], shot_restatement(orc, d, d["v2"], forward, d_obs, gz), f"fdw_shot_line_dtt image, numerics {numerics}")
    _, P, PP, illum = ctx.shot_line(d["v2"], sz, gz, wav, d_obs, want_fields=True, want_illum=True)
    for k, a in (("P", P), ("PP", PP), ("illum", illum)):
        assert_bit_equal(got[k], a, f"{k} vs fdw_shot_line")
    ref = ctx.shot_line_residual(d["v2"], sz, gz, wav, d_obs)
    res = ctx.shot_line_dtt(d["v2"], sz, gz, wav, d_obs, residual=True)
    assert_bit_equal(res["resid"], ref["resid"], "resid vs fdw_shot_line_residual")
    assert_bit_equal(res["image"], shot_restatement(orc, d, d["v2"], forward, ref["resid"], gz), "line residual image")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: batches
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("grid,batched", [((87, 70, 12, 10), True), ((87, 70, 3, 10), False)], ids=["87x70", "static-rows"])
def test_batches_equal_the_single_shot_calls(grid, batched, numerics):
    """Five shots, a budget that forces parts of two: every output equals the single-shot calls bit for bit; fdw_batch_parts reads 0 (one
    by one: the ragged deck), 1 (the whole batch) or k."""
    n = 5
    d, srce, d_obs, v2s, _ = shot_case(grid, 8, numerics, nshots=n)
    nx = d["nxe"] - 2 * d["nxb"]
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(two_step=-1)
    wav = (np.random.default_rng(5).standard_normal((n, nx, NT_SHOT)) * 100.0).astype(f32)
    single = [ctx.shot_dtt(v2s[b], d["sx"] + 2 * b, d["sz"], d["gz"], srce, d_obs[b], residual=True, want_illum=True) for b in range(n)]
    lines = [ctx.shot_line_dtt(v2s[b], d["sz"], d["gz"], wav[b], d_obs[b], want_illum=True) for b in range(n)]
    fe, ng = d["nxe"] * ctx.pitch, nx * NT_SHOT
    for budget, parts in ((0, 1), (int(2.5 * (12 * fe + 2 * ng) * 4), 3)):
        ctx.set_batch_budget(budget)
        got = ctx.shot_batch_dtt(n, d["sx"], 2, d["sz"], d["gz"], srce, d_obs, v2_all=v2s, residual=True, want_illum=True)
        assert ctx.batch_parts() == (parts if batched else 0), (budget, ctx.batch_parts())
        for k in ("image", "resid", "illum"):
            assert_bit_equal(got[k], np.stack([s[k] for s in single]), f"batched {k}, budget {budget}")
        got = ctx.shot_line_batch_dtt(n, d["sz"], d["gz"], wav, d_obs, v2_all=v2s, want_illum=True)
        assert ctx.batch_parts() == (parts if batched else 0), (budget, ctx.batch_parts())
        for k in ("image", "illum"):
            assert_bit_equal(got[k], np.stack([s[k] for s in lines]), f"batched line {k}, budget {budget}")
    ref = ctx.shot_batch_residual(n, d["sx"], 2, d["sz"], d["gz"], srce, d_obs, v2_all=v2s, want_illum=True)
    for k in ("resid", "illum"):
        assert_bit_equal(np.stack([s[k] for s in single]), ref[k], f"{k} vs fdw_shot_batch_residual")
    assert (ref["image"] != np.stack([s["image"] for s in single])).any()
    ctx.close()


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
    c = case("87x70", 8, 0)
    d, F1, F0, img0, samples, want = c
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    dv = Device(ctx, d, F1, F0, img0, samples)
    before = dv.state()
    p = dv.ptr
    nxe, gz = d["nxe"], d["gz"]
    s = dv.samples.data_ptr()
    refused(EINVAL, ctx.dev_back_iter_dtt, 1, p("f1"), None, p("pr"), p("ppr"), p("v2"), 0, nxe, True, s, gz, p("img"))
    refused(EINVAL, ctx.dev_back_iter_dtt, 1, p("f1"), p("f0"), p("pr"), p("ppr"), p("v2"), 0, nxe, True, s, gz, None)
    refused(EINVAL, ctx.dev_back_iter_dtt, 1, p("f1"), p("f1"), p("pr"), p("ppr"), p("v2"), 0, nxe, True, s, gz, p("img"))
    refused(EINVAL, ctx.dev_back_iter_dtt, 1, p("f1"), p("f0"), p("pr"), p("ppr"), p("v2"), 0, nxe, True, s, d["nze"], p("img"))
    refused(EINVAL, ctx.dev_back_iter_dtt, 1, p("f1"), p("f0"), p("pr"), p("ppr"), p("v2"), 4, nxe - 4, True, s, gz, p("img"))
    refused(EINVAL, ctx.dev_back_iter_dtt, 0, p("f1"), None, p("pr"), p("ppr"), p("v2"), 0, nxe, True, None, gz, p("img"))
    refused(EINVAL, ctx.dev_dtt_image, p("f1"), p("f0"), None, p("pr"), p("img"))
    nx, nz = nxe - 2 * d["nxb"], d["nze"] - 2 * d["nzb"]
    srce, d_obs = np.zeros(NIT, f32), np.zeros((nx, NIT), f32)
    place = (d["sx"], d["sz"], d["gz"])
    refused(EINVAL, ctx.shot_dtt, d["v2"], d["sx"], d["sz"], d["nze"], srce, d_obs, residual=True)
    assert F.lib().fdw_shot_dtt(ctx._h, d["v2"].ctypes.data, *place, srce, d_obs, np.zeros((nx, nz), f32), None, 2, None, None, None) == EINVAL
    assert F.lib().fdw_shot_dtt(ctx._h, d["v2"].ctypes.data, *place, srce, d_obs, np.zeros((nx, nz), f32), None, 0, d_obs.ctypes.data, None, None) == EINVAL
    assert "resident" in refused(ESTATE, ctx.shot_dtt, None, *place, srce, d_obs)
    assert F.lib().fdw_shot_batch_dtt(ctx._h, 0, d["v2"].ctypes.data, 0, d["sx"], 1, d["sz"], d["gz"], srce, d_obs, np.zeros((nx, nz), f32), None, 0, None) == EINVAL
    after = dv.state()
    for k in before:
        assert_bit_equal(after[k], before[k], f"{k} after the refusals")
    # the sibling's dialect and slab contexts do not combine with DTT imaging
    stored = F.FDWave(*args_of(d), compat=False, device=0, dialect=2)
    msg = refused(ESTATE, stored.dev_back_iter_dtt, 1, p("f1"), p("f0"), p("pr"), p("ppr"), p("v2"), 0, nxe, True, s, gz, p("img"))
    assert "dialect" in msg
    assert "dialect" in refused(ESTATE, stored.shot_dtt, d["v2"], *place, srce, d_obs)
    stored.close()
    slab = F.FDWave(*args_of(d), compat=True, device=0, slab=(0, nxe // 2 + 8))
    assert "slab" in refused(ESTATE, slab.dev_dtt_image, p("f1"), p("f0"), p("s0"), p("pr"), p("img"))
    assert "slab" in refused(ESTATE, slab.shot_dtt, d["v2"], *place, srce, d_obs)
    slab.close()
    after = dv.state()
    for k in before:
        assert_bit_equal(after[k], before[k], f"{k} after the refusals")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the programs: rtm_code's deck key dtt=1
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,env_extra,words", [("dtt=1\nexc=1\n", {}, ("dtt", "exc")), ("dtt=1\nsnap=5\n", {}, ("dtt", "snap")),
                                                   ("dtt=1\nslabs=2\n", {}, ("dtt", "slabs")), ("dtt=1\n", {"FDW_SLABS": "2"}, ("dtt", "slabs"))],
                         ids=["exc", "snap", "slabs-key", "FDW_SLABS"])
def test_rtm_code_refuses_dtt_with_excitation_snapshots_or_slabs(tmp_path, extra, env_extra, words):
    """Before any file, thread, communicator or device is touched: runs where no GPU is, and leaves the output directory empty."""
    from test_residual import BIN, _write_min_deck
    _write_min_deck(tmp_path, extra)
    env = {k: v for k, v in os.environ.items() if k not in ("FDW_SLABS", "FDW_GPUS")}
    env.update(env_extra)
    r = subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode != 0
    assert "dtt=1 cannot be combined" in r.stderr and all(w in r.stderr for w in words), r.stderr
    assert os.listdir(tmp_path / "out") == []
    assert not os.path.exists(tmp_path / "image.num")


def test_python_driver_refuses_a_dtt_deck(tmp_path):
    from parallel_finite_difference_computation_amd import rtm
    from test_residual import _write_min_deck
    _write_min_deck(tmp_path, "dtt=1\n")
    with pytest.raises(ValueError, match="dtt"):
        rtm.read_deck(str(tmp_path / "input.dat"))


@pytest.mark.gpu
def test_rtm_code_dtt(tmp_path):
    """dtt=1: dir.image is the stack of fdw_shot_dtt on the program's own border models, batched, one shot at a time and on two workers;
    with resid=1 the stack of its residual form, dir.resid and dir.misfit those of resid=1 alone; with illum=1 dir.illum stays what it is."""
    from test_residual import _run, _two_shot_deck
    nx, nz, nxb, nzb, nt, ns, ds = 50, 37, 10, 9, 47, 2, 20
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    rng = np.random.default_rng(11)
    vp = (1500 + 2500 * np.linspace(0, 1, nz, dtype=f32)[None, :] + 100 * rng.standard_normal((nx, nz))).astype(f32)
    dobs = rng.standard_normal((ns, nx, nt)).astype(f32)
    runs = {}
    for name, extra, env in (("plain", "", {}), ("dtt", "dtt=1\n", {}), ("nobatch", "dtt=1\n", {"FDW_NO_SHOT_BATCH": "1"}), ("gpus2", "dtt=1\ngpus=2\n", {}),
                             ("resid", "dtt=1\nresid=1\n", {}), ("resid-nobatch", "dtt=1\nresid=1\n", {"FDW_NO_SHOT_BATCH": "1"}),
                             ("resid-only", "resid=1\n", {}), ("illum", "dtt=1\nillum=1\n", {}), ("illum-only", "illum=1\n", {}), ("off", "dtt=0\n", {})):
        c = tmp_path / name
        _two_shot_deck(c, vp, extra)
        dobs.tofile(c / "models" / "dobs.bin")
        runs[name], r = _run("rtm_code", c, env)
        assert ("## dtt = 1" in r.stdout) == ("dtt=1" in extra), name
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    ctx.model_resident(vp)
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    img, rimg = np.zeros((nx, nz), f32), np.zeros((nx, nz), f32)
    for s in range(ns):
        vel = ctx.dev_extendvel_linear(s * ctx.border_draws(), want_vel=True)
        v2 = (vel * vel).astype(f32)
        place = (5 + s * ds + nxb, 1 + nzb, 2 + nzb)
        img = img + ctx.shot_dtt(v2, *place, srce, dobs[s])["image"]
        rimg = rimg + ctx.shot_dtt(v2, *place, srce, dobs[s], residual=True)["image"]
    assert img.any() and rimg.any() and (img != rimg).any()
    for name in ("dtt", "nobatch", "gpus2", "illum"):
        assert runs[name]["dir.image"] == img.tobytes(), name
    for name in ("resid", "resid-nobatch"):
        assert runs[name]["dir.image"] == rimg.tobytes(), name
        for f in ("dir.resid", "dir.misfit"):
            assert runs[name][f] == runs["resid-only"][f], (name, f)
    assert runs["illum"]["dir.illum"] == runs["illum-only"]["dir.illum"]
    assert sorted(runs["off"]) == sorted(runs["plain"]) == sorted(runs["dtt"])
    for f in runs["plain"]:
        assert runs["off"][f] == runs["plain"][f], f
    assert runs["plain"]["dir.image"] != img.tobytes()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the stream contract (a late producer) and the footprint (a guarded arena) of the two device entry points, through the machinery of
# tests/stream_cases.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def _stream_case(numerics=0, env=None):
    """fdw_dev_back_iter_dtt(step_source = 1) from noise-filled pairs, then fdw_dev_dtt_image on the levels (F1, F_new, PR) against the new
    receiver field: two terms on C, every other word of the image as uploaded (the sentinel in its padding columns included)."""
    import stream_cases as S
    deck = "ragged"
    nxe, nze, nxb, nzb = S.DECKS[deck]["geom"]
    gz = S.DECKS[deck]["place"][2]

    def ins(i):
        return dict(F1=("field", i["f1"]), F0=("field", i["f0"]), PR=("field", i["pr"]), PPR=("field", i["ppr"]), v2=("field", i["v2"]),
                    IMG=("field", i["img0"]), SAMP=("flat", i["samples"]))

    def call(ctx, p, stream):
        ctx.dev_back_iter_dtt(1, p["F1"], p["F0"], p["PR"], p["PPR"], p["v2"], 0, nxe, False, p["SAMP"], gz, p["IMG"], stream=stream)
        ctx.dev_dtt_image(p["F1"], p["F0"], p["PR"], p["PPR"], p["IMG"], stream=stream)
        return [("r_new", "PPR", None, None), ("F0", "F0", None, None), ("img", "IMG", None, None)]

    def want(v):
        i = S.inputs(deck, v)
        c = S.back_chain(deck, numerics, v, 1, 1)
        x0, x1, z0, z1 = born_cells(i["d"])
        C = (slice(x0, x1), slice(z0, z1))
        a, b, new, pr, ppr, rn = i["f0"][C], i["f1"][C], c["F0"][C], i["pr"][C], i["ppr"][C], c["r_new"][C]
        img = np.array(i["img0"], f32)
        with np.errstate(all="ignore"):
            q = ((a - b).astype(f32) - (b - new).astype(f32)).astype(f32)
            acc = (img[C] + (q * ppr).astype(f32)).astype(f32)
            q = ((b - new).astype(f32) - (new - pr).astype(f32)).astype(f32)
            img[C] = (acc + (q * rn).astype(f32)).astype(f32)
        return dict(r_new=c["r_new"], F0=c["F0"], img=img)

    return S.Case("back_iter_dtt-" + deck + ("-unfused" if env else ""), deck, numerics, -1, ins, {}, call, want, env=env, pad_words=dict(IMG=PAD))


@pytest.mark.gpu
def test_late_producer_on_the_callers_stream():
    """Decoys in every input; behind 40 ms of delay on the caller's stream the true fields, model, image and samples are copied in, then the
    two entry points, then the outputs copied out: the answers are those of the true inputs, and the calls returned while the stream was
    still busy (nothing synchronised)."""
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
    assert busy, "the entry points returned only after the stream had drained: they synchronised"
    run.close()


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
def test_guarded_arena_footprint(numerics):
    """Every buffer carved from one arena with NaN guard bands: guards and padding columns intact (the image's sentinel too), d_f1, d_pr,
    d_v2 and the samples unchanged, the image changed on C only."""
    import torch

    import footprint_arena as A
    import stream_cases as S
    case_ = _stream_case(numerics)
    i = S.inputs("ragged", "true")
    arena = A.build(case_, i)
    ctx = case_.make_ctx()
    assert ctx.pitch == arena.pitch
    t = torch.from_numpy(arena.up.view(np.int32).copy()).to("cuda:0")
    labels = case_.call(ctx, arena.pointers(t.data_ptr()), None)
    torch.cuda.synchronize()
    ctx.close()                                                     # (fdw_destroy drains the context's stream)
    down = t.cpu().numpy().view(np.uint32)
    bad = A.check(arena, down, labels)
    assert not bad, "\n".join(bad)
    got, want = A.results(arena, down, labels), case_.want("true")
    for k in want:
        assert_bit_equal(got[k], want[k], f"arena: {k}")
    x0, x1, z0, z1 = born_cells(i["d"])
    changed = got["img"] != i["img0"]
    assert changed[x0:x1, z0:z1].mean() > 0.9
    changed[x0:x1, z0:z1] = False
    assert not changed.any()

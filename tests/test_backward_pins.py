"""The backward half (fd_back, R:290-341: time reversal, receiver injection, imaging) pinned to a statement that does not come from the oracle.

R = cuda_reference_RTM/src/fd-code.cu.  The reference's .cu cannot be built here and ships no usable image, so every other test of the
backward loop holds the HIP kernels to oracle/fdw_oracle.c's orc_fd_back, which was written by the same hand.  tests/rtm_restatement.py
states the loop again from R, and this file holds both the oracle and the kernels to it:
  * at zero velocity, where the loop has a closed form in fp32: bit for bit;
  * with propagation, against a float64 statement: within 1e-5 max-norm-relative (the project's tolerance for the reference's own
    fp32 rounding noise);
and shows that each bound catches the misreadings it is meant to catch (MUTATIONS_ZERO_VELOCITY, MUTATIONS_F64).  The two race
conventions (kernel_tapper's right-hand strip, kernel_sism's replicas) are shared with the oracle and are not pinned by this file.

CPU part: the oracle against the restatement.  GPU part (-m gpu): every backward path of the library against the restatement directly.
"""
import os
import subprocess

import numpy as np
import pytest

import rtm_restatement as R
from conftest import ROOT, assert_bit_equal, make_deck, random_fields, rel_max
from oracle import oracle as O

TOL = 1e-5          # EXACT numerics: the HIP / oracle image against the float64 restatement
TOL_FAST = 2e-5     # FAST numerics (fdwave.h): measured up to 1.23e-5 on F64_DECKS[2], see test_gpu_images_against_the_float64_restatement


def _orc(d, numerics=0):
    return O.Oracle(d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"],
                    compat=d.get("compat", True), numerics=numerics)


def _mk(d, **kw):
    import parallel_finite_difference_computation_amd as F
    return F.FDWave(d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"],
                    compat=d.get("compat", True), **kw)


def _deck(case, seed=21):
    nxe, nze, nxb, nzb, nt, order, compat, fac, dx, dz = case
    return make_deck(nxe, nze, nxb, nzb, nt, seed=seed, order=order, compat=compat, fac=fac, dx=dx, dz=dz)


def _data(d, seed):
    """A gather d_obs[nx][nt] and a non-zero start image (the loop accumulates into imloc, R:243)."""
    rng = np.random.default_rng(seed)
    nx, nz = d["nxe"] - 2 * d["nxb"], d["nze"] - 2 * d["nzb"]
    return rng.standard_normal((nx, d["nt"])).astype(np.float32), rng.standard_normal((nx, nz)).astype(np.float32)


def _srce(d):
    return (O.ricker_wavelet(d["nt"], d["dt"], 30.0) + 0.25).astype(np.float32)


# (nxe, nze, nxb, nzb, nt, order, compat, fac, dx, dz)
ZV_DECKS = [(99, 83, 17, 13, 23, 8, True, 0.75, 10.0, 10.0),       # compat, nxe / nze / nzb not multiples of 8 (xlim 96, zlim 80, ztap 8)
            (101, 90, 12, 19, 22, 4, True, 1.0, 10.0, 10.0),       # compat ragged, fac = 1 (the taper is the identity)
            (99, 83, 17, 13, 21, 8, False, 0.75, 10.0, 10.0),      # full extents
            (150, 130, 20, 24, 20, 6, False, 0.5, 25.0, 8.0)]      # full extents, dx != dz
ZV_IDS = ["compat-ragged", "compat-ragged-fac1", "full", "full-dx25-dz8"]

# with propagation; nt long enough for the waves to cross the damped strip and the receiver row many times
F64_DECKS = [(99, 83, 17, 13, 200, 8, True, 0.75, 10.0, 10.0),
             (150, 130, 20, 24, 300, 4, False, 0.75, 25.0, 8.0),
             (70, 53, 10, 10, 400, 8, True, 0.75, 8.0, 12.5)]
F64_IDS = ["99x83-o8-compat-nt200", "150x130-o4-dx25-dz8-nt300", "70x53-o8-dx8-dz12.5-nt400"]


def _f64_case(case):
    d = _deck(case, seed=5)
    d_obs, _ = _data(d, 2)
    return d, O.ricker_wavelet(d["nt"], d["dt"], 30.0), d_obs


# ==== CPU: the oracle against the restatement =============================================================================================

def test_launch_extents_derived_from_the_reference():
    """R:185-195 truncates nxe / 8 (an int assignment before ceil), so the launches cover 8 floor(n / 8) rows, columns and taper rows; the
    restatement derives that itself and the oracle agrees."""
    for nxe, nze, nzb in ((99, 83, 13), (96, 80, 16), (101, 90, 19), (3001, 3003, 40), (70, 53, 10), (8, 9, 7)):
        for compat in (True, False):
            assert R.launch_extents(nxe, nze, nzb, compat) == O.extents(nxe, nze, nzb, compat)
    assert R.launch_extents(99, 83, 13) == (96, 80, 8)
    assert R.launch_extents(99, 83, 13, compat=False) == (99, 83, 13)


@pytest.mark.parametrize("case", ZV_DECKS, ids=ZV_IDS)
def test_zero_velocity_oracle_equals_the_restatement_bit_for_bit(case):
    """v2 = 0: orc_fd_forward and orc_fd_back against the fp32 emulation, bit for bit -- forward from zero and from random fields, a whole shot
    with sz == gz (the only case where the source field meets the receivers without propagation), and fd_back from random snapshots for
    iteration counts that leave 0..3 iterations over a multiple of four, onto a non-zero start image."""
    d = _deck(case)
    z = np.zeros((d["nxe"], d["nze"]), np.float32)
    srce, (d_obs, im0) = _srce(d), _data(d, 3)
    orc, nt, sx, gz = _orc(d), d["nt"], d["sx"], d["gz"]

    for p0, pp0, n in ((None, None, nt), (*random_fields(d, 4), nt - 3)):
        P, PP = R.forward_zero_velocity(d, sx, gz, srce, p0, pp0, nsteps=n)
        oP, oPP = orc.forward(z, sx, gz, srce, p0, pp0, nsteps=n)
        assert_bit_equal(oP, P, f"forward P, {n} steps")
        assert_bit_equal(oPP, PP, f"forward PP, {n} steps")

    img = R.shot_zero_velocity(d, sx, gz, gz, srce, d_obs)
    oP, oPP = orc.forward(z, sx, gz, srce)
    assert_bit_equal(orc.back(z, oP, oPP, d_obs, gz), img, "whole shot, sz == gz")
    assert np.count_nonzero(img) > 0

    s0, s1 = random_fields(d, 5)
    for n in (nt, nt - 1, nt - 2, nt - 3, 1, 2, 3):
        want = R.back_zero_velocity(d, s0, s1, d_obs, gz, imloc=im0, nsteps=n)
        assert_bit_equal(orc.back(z, s0, s1, d_obs, gz, imloc=im0, nsteps=n), want, f"back from random snapshots, {n} iterations")
        assert np.any(want != im0)
    assert np.count_nonzero(R.back_zero_velocity(d, s0, s1, d_obs, gz)) > 0


@pytest.mark.parametrize("case", F64_DECKS, ids=F64_IDS)
def test_oracle_image_within_tolerance_of_the_float64_restatement(case):
    """With propagation: the fp32 oracle image of a whole shot against shot_f64, and fd_back from the forward snapshots for fewer iterations
    onto a non-zero image against back_f64.  Measured (max-norm-relative): 1.71e-6, 1.43e-6, 1.63e-6 for the three whole shots -- below the
    1e-5 bound by a factor of six, while the closest misreading (test_float64_mutations_move_the_image_far_past_the_tolerance) is at 1.7e-2."""
    d, srce, d_obs = _f64_case(case)
    orc = _orc(d)
    oP, oPP = orc.forward(d["v2"], d["sx"], d["sz"], srce)
    want = R.shot_f64(d, d["v2"], d["sx"], d["sz"], d["gz"], srce, d_obs)
    got = orc.back(d["v2"], oP, oPP, d_obs, d["gz"])
    assert rel_max(got, want) < TOL, rel_max(got, want)
    fP, fPP = R.forward_f64(d, d["v2"], d["sx"], d["sz"], srce)
    assert rel_max(oP, fP) < TOL and rel_max(oPP, fPP) < TOL
    _, im0 = _data(d, 6)
    im0 *= np.float32(np.abs(want).max())
    n = d["nt"] // 2 + 1
    want = R.back_f64(d, d["v2"], oP, oPP, d_obs, d["gz"], imloc=im0, nsteps=n)
    assert rel_max(orc.back(d["v2"], oP, oPP, d_obs, d["gz"], imloc=im0, nsteps=n), want) < TOL


def test_zero_velocity_mutations_change_the_image():
    """Each misreading of MUTATIONS_ZERO_VELOCITY changes the bits of the emulated image (both on a whole shot with sz == gz and from random
    snapshots): a kernel or an oracle that made it would fail the bit-for-bit pins above."""
    d = _deck(ZV_DECKS[0])
    srce, (d_obs, _) = _srce(d), _data(d, 3)
    s0, s1 = random_fields(d, 5)
    base_back = R.back_zero_velocity(d, s0, s1, d_obs, d["gz"])
    base_shot = R.shot_zero_velocity(d, d["sx"], d["gz"], d["gz"], srce, d_obs)
    for m in R.MUTATIONS_ZERO_VELOCITY:
        assert np.any(R.back_zero_velocity(d, s0, s1, d_obs, d["gz"], mutation=m) != base_back), m
        assert np.any(R.shot_zero_velocity(d, d["sx"], d["gz"], d["gz"], srce, d_obs, mutation=m) != base_shot), m


@pytest.mark.parametrize("case", F64_DECKS, ids=F64_IDS)
def test_float64_mutations_move_the_image_far_past_the_tolerance(case):
    """Each misreading of MUTATIONS_F64 -- the zero-velocity ones, the two taper ones (damping the reconstructed source field, not damping the
    receiver field) and a receiver Laplacian that reads the source field -- moves the float64 image by at least 100 x TOL.  Measured: the
    smallest is image_before_injection at 1.7e-2 (the 150 x 130 deck), the taper pair at 4.8e-2 .. 8.6e-1, the rest 0.13 .. 124."""
    d, srce, d_obs = _f64_case(case)
    base = R.shot_f64(d, d["v2"], d["sx"], d["sz"], d["gz"], srce, d_obs)
    for m in R.MUTATIONS_F64:
        dist = rel_max(R.shot_f64(d, d["v2"], d["sx"], d["sz"], d["gz"], srce, d_obs, mutation=m), base)
        assert dist >= 100 * TOL, (m, dist)


# ==== GPU: every backward path against the restatement ====================================================================================

GPU_ZV_DECKS = [(99, 83, 17, 13, 23, 8, True, 0.75, 10.0, 10.0), (150, 130, 20, 24, 22, 8, False, 0.75, 25.0, 8.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_ZV_DECKS, ids=["compat-ragged", "full-dx25-dz8"])
def test_gpu_zero_velocity_every_backward_path_bit_for_bit(case, monkeypatch):
    """v2 = 0, random snapshots (zero on the never-stepped rows of the damped strip, the lazy damping's precondition), non-zero start image:
    fdw_back through the fused one-step iteration, the two-launch form, the paired two-step iterations, the wave pipeline (fused and two-pass,
    three chunk lengths), FDW_NO_BACK_PIPE, and FAST numerics -- each equal to the fp32 emulation bit for bit for iteration counts that leave
    0..3 iterations over a multiple of four.  At v2 = 0 FAST gives EXACT's bits: fma(0, lap, x) == x and 2p - pp rounds once in both."""
    d = _deck(case)
    z = np.zeros((d["nxe"], d["nze"]), np.float32)
    d_obs, im0 = _data(d, 3)
    s0, s1 = random_fields(d, 5)
    nt, gz = d["nt"], d["gz"]
    want = {n: R.back_zero_velocity(d, s0, s1, d_obs, gz, imloc=im0, nsteps=n) for n in (nt, nt - 1, nt - 2, nt - 3, 2, 3)}
    ctx = _mk(d)
    assert ctx.extents() == R.launch_extents(d["nxe"], d["nze"], d["nzb"], d["compat"])
    ctxs = {"default": (ctx, [(0, 0)]), "one-step": (ctx, [(-1, 0)]), "two-step pairs": (ctx, [(1, 0)]),
            "pipeline": (ctx, [(4, x) for x in (0, 13, 23)])}
    for env, name, modes in (("FDW_NO_FUSED_BACK", "two launches", [(-1, 0), (0, 0)]), ("FDW_NO_BACK_FUSED", "two-pass pipeline", [(4, 0), (4, 13)]),
                             ("FDW_NO_BACK_PIPE", "no back pipeline", [(4, 0)])):
        monkeypatch.setenv(env, "1")
        ctxs[name] = (_mk(d), modes)
        monkeypatch.delenv(env)
    ctxs["FAST"] = (_mk(d, numerics=1), [(-1, 0), (0, 0), (4, 0), (4, 23)])
    for name, (c, modes) in ctxs.items():
        for two_step, xchunk in modes:
            c.set_tuning(two_step=two_step, xchunk=xchunk)
            for n, w in want.items():
                assert_bit_equal(c.back(z, s0, s1, d_obs, gz, imloc=im0, nsteps=n), w, f"{name}, two_step={two_step}, xchunk={xchunk}, {n} iterations")
    assert np.any(want[nt] != im0)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_ZV_DECKS, ids=["compat-ragged", "full-dx25-dz8"])
def test_gpu_zero_velocity_whole_shot_bit_for_bit(case):
    """fdw_shot at v2 = 0 with sz == gz (forward loop, snapshot hand-over, backward loop): P, PP and the image equal the emulation bit for
    bit, on the kernels the library picks, on the one-step kernels and through the wave pipeline, in both numerics."""
    d = _deck(case)
    z = np.zeros((d["nxe"], d["nze"]), np.float32)
    srce, (d_obs, im0) = _srce(d), _data(d, 3)
    sx, gz = d["sx"], d["gz"]
    P, PP = R.forward_zero_velocity(d, sx, gz, srce)
    want = R.shot_zero_velocity(d, sx, gz, gz, srce, d_obs, imloc=im0)
    assert np.any(want != im0)
    for numerics in (0, 1):
        ctx = _mk(d, numerics=numerics)
        for mode in (0, -1, 4):
            ctx.set_tuning(two_step=mode)
            img, gP, gPP = ctx.shot(z, sx, gz, gz, srce, d_obs, imloc=im0, want_fields=True)
            what = f"numerics={numerics}, two_step={mode}"
            assert_bit_equal(gP, P, f"shot P, {what}")
            assert_bit_equal(gPP, PP, f"shot PP, {what}")
            assert_bit_equal(img, want, f"shot image, {what}")


@pytest.mark.gpu
def test_gpu_zero_velocity_shot_batch_bit_for_bit():
    """fdw_shot_batch (one launch per time step for all shots) on an all-zero v2_all, sz == gz for every shot: each image equals the
    emulation of its own shot bit for bit."""
    d = _deck(GPU_ZV_DECKS[0])
    nshots, dsx, gz = 3, 2, d["gz"]
    srce = _srce(d)
    rng = np.random.default_rng(13)
    nx, nz = d["nxe"] - 2 * d["nxb"], d["nze"] - 2 * d["nzb"]
    d_obs = rng.standard_normal((nshots, nx, d["nt"])).astype(np.float32)
    im0 = rng.standard_normal((nshots, nx, nz)).astype(np.float32)
    ctx = _mk(d)
    assert ctx.shot_batch_max() > 1
    got = ctx.shot_batch(nshots, d["sx"], dsx, gz, gz, srce, d_obs, v2_all=np.zeros((nshots, d["nxe"], d["nze"]), np.float32), imloc=im0)
    for b in range(nshots):
        want = R.shot_zero_velocity(d, d["sx"] + b * dsx, gz, gz, srce, d_obs[b], imloc=im0[b])
        assert_bit_equal(got[b], want, f"batched shot {b}")
        assert np.any(want != im0[b])


@pytest.mark.gpu
@pytest.mark.parametrize("world,ksteps,shape,compat,pipe", [(2, 4, (400, 500), True, False), (2, 4, (333, 2500), True, True),
                                                            (3, 3, (701, 523), True, False), (3, 8, (900, 2100), False, True)],
                         ids=["2ranks-k4", "2ranks-pipeline-k4-ragged", "3ranks-k3-ragged", "3ranks-pipeline-k8"])
def test_gpu_zero_velocity_slabs_bit_for_bit(world, ksteps, shape, compat, pipe, monkeypatch):
    """fdw_slabs_shot on `world` ranks as host threads sharing this GPU (as in test_slabs_gpu.py), FDW_SLAB_PIPE 0 and 1, v2 = 0 and
    sz == gz: the image and the fields gathered from the ranks' owned rows equal the emulation bit for bit."""
    import parallel_finite_difference_computation_amd as F
    nxe, nze = shape
    nt = 2 * max(ksteps, 4) + 5
    d = make_deck(nxe, nze, 40, 40, nt, seed=3, compat=compat)
    z = np.zeros((nxe, nze), np.float32)
    srce, (d_obs, im0) = _srce(d), _data(d, 4)
    sx, gz = d["sx"], d["gz"]
    P, PP = R.forward_zero_velocity(d, sx, gz, srce)
    want = R.shot_zero_velocity(d, sx, gz, gz, srce, d_obs, imloc=im0)
    monkeypatch.setenv("FDW_SLAB_PIPE", "1" if pipe else "0")
    comms = F.Comm.local(world)

    def rank(r):
        s = F.Slabs(d["order"], nxe, nze, d["nxb"], d["nzb"], nt, d["fac"], d["dx"], d["dz"], d["dt"], comm=comms[r], compat=compat, ksteps=ksteps)
        assert (s.nbuf == 4) == pipe
        out = s.shot(z, sx, gz, gz, srce, d_obs, imloc=im0, want_fields=True)
        geo = (s.own0, s.own1, s.owned_interior_rows())
        s.close()
        return out, geo

    img, gP, gPP = np.array(im0), np.zeros_like(P), np.zeros_like(PP)
    for (im, p, pp), (o0, o1, (a, b)) in F.run_ranks(rank, world):
        img[a:b] = im[a:b]
        gP[o0:o1], gPP[o0:o1] = p[o0:o1], pp[o0:o1]
    for c in comms:
        c.close()
    assert_bit_equal(gPP, PP, "PP gathered from the ranks")
    assert_bit_equal(gP, P, "P gathered from the ranks")
    assert_bit_equal(img, want, "image gathered from the ranks")
    assert np.any(want != im0)


@pytest.mark.gpu
def test_gpu_zero_velocity_past_the_pipeline_threshold():
    """A 3001 x 3003 compat grid, where the library runs four iterations per pass by itself (steps_per_pass() == 4, no forcing): fdw_back from
    random snapshots and a whole fdw_shot with sz == gz at v2 = 0 equal the emulation bit for bit."""
    d = make_deck(3001, 3003, 40, 40, 11, seed=2, compat=True)
    z = np.zeros((d["nxe"], d["nze"]), np.float32)
    srce, (d_obs, im0) = _srce(d), _data(d, 7)
    s0, s1 = random_fields(d, 9, amp=1e-3)
    ctx = _mk(d)
    assert ctx.steps_per_pass() == 4
    assert ctx.extents() == R.launch_extents(3001, 3003, 40) == (3000, 3000, 40)
    for n in (11, 8):
        want = R.back_zero_velocity(d, s0, s1, d_obs, d["gz"], imloc=im0, nsteps=n)
        assert_bit_equal(ctx.back(z, s0, s1, d_obs, d["gz"], imloc=im0, nsteps=n), want, f"back, {n} iterations")
        assert np.any(want != im0)
    img, P, PP = ctx.shot(z, d["sx"], d["gz"], d["gz"], srce, d_obs, imloc=im0, want_fields=True)
    wP, wPP = R.forward_zero_velocity(d, d["sx"], d["gz"], srce)
    assert_bit_equal(P, wP, "shot P")
    assert_bit_equal(PP, wPP, "shot PP")
    assert_bit_equal(img, R.shot_zero_velocity(d, d["sx"], d["gz"], d["gz"], srce, d_obs, imloc=im0), "shot image")


@pytest.mark.gpu
def test_gpu_rtm_code_zero_velocity_stack(tmp_path):
    """bin/rtm_code on a two-shot deck whose vel_ext_file is all zeros (vel^2 = 0 for every shot, R:483-494) and sz == gz: dir.image equals
    the fp32 stack (R:525) of the two emulated shots bit for bit -- shots batched (the default on a small deck) and one at a time."""
    nx, nz, nxb, nzb, nt, ns, fsx, ds, szgz = 61, 47, 17, 13, 60, 2, 5, 20, 3
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    rng = np.random.default_rng(17)
    d_obs = rng.standard_normal((ns, nx, nt)).astype(np.float32)
    (tmp_path / "models").mkdir()
    (tmp_path / "output").mkdir()
    np.full((nx, nz), 2000.0, np.float32).tofile(tmp_path / "models" / "vp.bin")
    d_obs.tofile(tmp_path / "models" / "dobs.bin")
    np.zeros((ns, nxe, nze), np.float32).tofile(tmp_path / "models" / "velext.bin")
    (tmp_path / "input.dat").write_text(
        "tmpdir=./output\nvpfile=./models/vp.bin\ndatfile=./models/dobs.bin\nvel_ext_file=./models/velext.bin\n"
        f"nz={nz}\nnx={nx}\nnt={nt}\ndz=10\ndx=10\ndt=0.001\nfpeak=25.\nns={ns}\nsz={szgz}\nfsx={fsx}\nds={ds}\ngz={szgz}\n"
        f"nxb={nxb}\nnzb={nzb}\nrnd=1\nfac=0.75\norder=8\n")
    d = dict(order=8, nxe=nxe, nze=nze, nxb=nxb, nzb=nzb, nt=nt, fac=0.75, dx=10.0, dz=10.0, dt=0.001, compat=True)
    srce = O.ricker_wavelet(nt, 0.001, 25.0)                                  # R:402-403
    img = np.zeros((nx, nz), np.float32)
    for s in range(ns):                                                      # R:406-409: sx = fsx + is ds + nxb, sz / gz + nzb
        img = img + R.shot_zero_velocity(d, fsx + s * ds + nxb, szgz + nzb, szgz + nzb, srce, d_obs[s])
    assert np.count_nonzero(img) >= ns
    exe = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin", "rtm_code")
    for env in ({}, {"FDW_NO_SHOT_BATCH": "1"}):
        r = subprocess.run([exe, "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=dict(os.environ, **env), timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        assert_bit_equal(np.fromfile(tmp_path / "output" / "dir.image", np.float32).reshape(nx, nz), img, f"dir.image with {env}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", F64_DECKS, ids=F64_IDS)
def test_gpu_images_against_the_float64_restatement(case):
    """With propagation: fdw_shot's image against shot_f64 -- EXACT numerics within 1e-5 on the kernels the library picks and forced through
    the wave pipeline (1.71e-6, 1.43e-6, 1.63e-6, equal to the oracle's bits); FAST numerics within TOL_FAST on the same paths.  FAST
    measured 1.94e-6, 1.84e-6 and 1.23e-5 (the 70 x 53, dx = 8, dz = 12.5 deck over 400 iterations), recorded in fdwave.h; the closest
    misreading is at 1.7e-2."""
    d, srce, d_obs = _f64_case(case)
    want = R.shot_f64(d, d["v2"], d["sx"], d["sz"], d["gz"], srce, d_obs)
    for numerics, tol in ((0, TOL), (1, TOL_FAST)):
        ctx = _mk(d, numerics=numerics)
        for mode in (0, 4):
            ctx.set_tuning(two_step=mode)
            dist = rel_max(ctx.shot(d["v2"], d["sx"], d["sz"], d["gz"], srce, d_obs), want)
            print(f"numerics={numerics} two_step={mode}: {dist:.3g}")
            assert dist < tol, (numerics, mode, dist)

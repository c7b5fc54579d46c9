"""GPU: the one-step register-ring kernels of order 8 at EVERY prefetch distance, in every mode, against the CPU oracle bit for bit.

fdw_set_tuning(prefetch = 1 | 2 | 3) is public ABI and picks a different instantiation of fdw_step_kernel / fdw_step_rec_kernel /
fdw_step_illum_kernel for each distance: a ring of 9, 10 or 12 rows (fdw_api.cpp ring_rows), its own register allocation and wait counts.
The rest of the suite runs prefetch 1 and 3 through the forward mode only (test_gpu_parity.py::test_forward_interior_waves_vs_oracle);
this module runs the Laplacian, the backward loop fused and in two launches, trace recording, the illumination, the modelling dialect and
the stored-wavefield RTM at 1 and 3, with 2 as a control that ties the cases to ones the other modules already pass.  What ran is not
taken from the names here: scripts/kernel_census.py traces every GPU module with the profiler and profiles/kernel_census.csv records the
launches per kernel; tests/test_programs.py::test_every_compiled_kernel_runs_in_a_parity_module holds the library to it.

Every prefetch case: order 8, EXACT numerics, two_step = -1 with steps_per_pass() == 1 asserted, chunk lengths 0 (automatic), one and two
turns of the ring of that prefetch distance and 13 (neither); the source row lies where the ring has wrapped inside its chunk.  Each case
first checks on the oracle alone that what it compares is not empty.  Behind them: FAST numerics on a grid past fill_geometry's large-grid
threshold with prefetch 1 and 3, and the kernels of orders 2, 4 and 6 that the census showed without a launch in a parity module (the
two-launch backward loop and the stored-wavefield RTM, both numerics)."""
import functools

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from conftest import assert_bit_equal, make_deck, random_fields
from oracle import oracle as O
from test_illum import STEP_COUNTS, _Device, illum_restatement
from test_record import oracle_gather

pytestmark = pytest.mark.gpu

H = 4                                             # half order
PREFETCH = (1, 2, 3)                              # 2: the control
RING = {pf: ((2 * H + pf + pf - 1) // pf) * pf for pf in PREFETCH}
assert RING == {1: 9, 2: 10, 3: 12}               # fdw_api.cpp ring_rows(4, pf)
WIDE = (150, 1300, 20, 24)                        # nxe, nze, nxb, nzb: six strips of 256 columns, several chunks: most waves run the mask-free interior body
RAGGED = (69, 301, 3, 10)                         # the compat grid of test_record.py: xlim 64 (receiver rows 64, 65 never time-stepped), zlim 296, ztap 8
SX = {WIDE: 56, RAGGED: 17}                       # source rows, see ring_has_wrapped


def chunks(pf):
    return (0, RING[pf], 2 * RING[pf], 13)


def ring_has_wrapped(row, xchunk, ring):
    """A chunk loads rows -H .. of its first row on; when it computes `row` it has loaded offset + 2H + 1 rows: more than the ring holds."""
    return row % xchunk + 2 * H + 1 > ring


for _sx in SX.values():
    for _pf in PREFETCH:
        assert all(ring_has_wrapped(_sx, c, RING[_pf]) for c in chunks(_pf) if c), (_sx, _pf)


def tune(ctx, pf, xchunk):
    ctx.set_tuning(xchunk=xchunk, prefetch=pf, two_step=-1)
    assert ctx.steps_per_pass() == 1


def rtm_deck(grid, nt, seed, **kw):
    nxe, nze, nxb, nzb = grid
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=seed, **kw)
    d["sx"] = SX[grid]
    return d


def args_of(d):
    return (d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"])


def reach(nx, nz, sx, sz, gz, nt):
    """Interior cells both fields of an nt-step shot can have reached when they meet: a field spreads H cells per step along the axes, so a
    cell needs ceil(L1 distance to the source / H) steps of the source field and ceil(|z - gz| / H) of the receiver field, nt - 1 between
    them (interior coordinates)."""
    x, z = np.arange(nx)[:, None], np.arange(nz)[None, :]
    hops = -(-(np.abs(x - sx) + np.abs(z - sz)) // H) + -(-np.abs(z - gz) // H)
    return hops <= nt - 1


def assert_image_not_vacuous(delta, mask, what):
    """More than half of the cells reached by both fields carry a non-zero imaging sum (delta: the image from a zero start image)."""
    assert mask.sum() >= 100, what
    share = float(np.mean(delta[mask] != 0))
    print(f"{what}: {int(mask.sum())} cells reached by both fields, {share:.3f} of them non-zero")
    assert share > 0.5, (what, share)


# ---------------------------------------------------------------------------------------------------------------------------------------
# LAP
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pf", PREFETCH)
@pytest.mark.parametrize("shape", [(203, 777), (150, 1301)], ids=lambda s: "x".join(map(str, s)))
def test_laplacian_at_every_prefetch_distance(shape, pf):
    nxe, nze = shape
    p = np.random.default_rng(nxe + nze).standard_normal(shape).astype(np.float32)
    want = O.stencil(8, nxe, nze, 10.0, 12.5, p)
    assert np.count_nonzero(want) > 0.9 * (nxe - 2 * H) * (nze - 2 * H)
    ctx = F.FDWave(8, nxe, nze, dx=10.0, dz=12.5)
    for xchunk in chunks(pf):
        tune(ctx, pf, xchunk)
        assert_bit_equal(ctx.laplacian(p), want, f"laplacian {shape} prefetch {pf} xchunk {xchunk}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the backward loop: BACK (one launch per iteration), and PLAIN + RECV (FDW_NO_FUSED_BACK=1)
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _back_case(grid):
    nt = 12
    d = rtm_deck(grid, nt, seed=31, dx=10.0, dz=12.5 if grid == RAGGED else 10.0)
    nx, nz = d["nxe"] - 2 * d["nxb"], d["nze"] - 2 * d["nzb"]
    rng = np.random.default_rng(8)
    srce = (O.ricker_wavelet(nt, d["dt"], 30.0) * 1000.0 + 3.0).astype(np.float32)
    d_obs = rng.standard_normal((nx, nt)).astype(np.float32)
    im0 = rng.standard_normal((nx, nz)).astype(np.float32)
    s0, s1 = random_fields(d, seed=15, amp=0.1)                   # noise-filled snapshots: the source field is dense from the first iteration
    orc = O.Oracle(*args_of(d), compat=True)
    oP, oPP = orc.forward(d["v2"], d["sx"], d["sz"], srce)
    xlim = 8 * (d["nxe"] // 8)
    rows = np.arange(nx)[:, None] + d["nxb"] < xlim               # receiver rows the reference time-steps
    want = {}
    for name, a, b in (("noise snapshots", s0, s1), ("forward snapshots", oP, oPP)):
        for n in (nt, 3):
            want[name, n] = orc.back(d["v2"], a, b, d_obs, d["gz"], imloc=im0, nsteps=n)
        delta = orc.back(d["v2"], a, b, d_obs, d["gz"])
        # noise: the source field is everywhere, the receiver field within H cells per iteration of its line; from rest: both spread from a point / a line
        if name.startswith("noise"):
            mask = -(-np.abs(np.arange(nz)[None, :] - (d["gz"] - d["nzb"])) // H) <= nt - 1
        else:
            mask = reach(nx, nz, d["sx"] - d["nxb"], d["sz"] - d["nzb"], d["gz"] - d["nzb"], nt)
        assert_image_not_vacuous(delta, mask & rows, f"backward loop on {grid}, {name}")
        assert (want[name, nt] != im0).any()
    assert np.count_nonzero(oPP) > 100
    return d, srce, d_obs, im0, (s0, s1), (oP, oPP), want


@pytest.mark.parametrize("pf", PREFETCH)
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-launches"])
@pytest.mark.parametrize("grid", [WIDE, RAGGED], ids=["wide", "ragged-compat"])
def test_backward_loop_at_every_prefetch_distance(grid, fused, pf, monkeypatch):
    """fdw_back from noise-filled snapshots and from the forward run's, onto a non-zero image, all iterations and three; fdw_shot with the
    forward fields it returns.  The host API hands back no reconstructed source field: every one of them enters the image through the
    imaging product of its iteration, over the band the receiver field has reached."""
    d, srce, d_obs, im0, noise, fwd, want = _back_case(grid)
    if fused:
        monkeypatch.delenv("FDW_NO_FUSED_BACK", raising=False)
    else:
        monkeypatch.setenv("FDW_NO_FUSED_BACK", "1")
    ctx = F.FDWave(*args_of(d), compat=True)
    monkeypatch.delenv("FDW_NO_FUSED_BACK", raising=False)
    for xchunk in chunks(pf):
        tune(ctx, pf, xchunk)
        what = f"{grid} fused={fused} prefetch {pf} xchunk {xchunk}"
        for name, (a, b) in (("noise snapshots", noise), ("forward snapshots", fwd)):
            for n in (d["nt"], 3):
                got = ctx.back(d["v2"], a, b, d_obs, d["gz"], imloc=im0, nsteps=n)
                assert_bit_equal(got, want[name, n], f"image, {name}, {n} iterations, {what}")
        img, P, PP = ctx.shot(d["v2"], d["sx"], d["sz"], d["gz"], srce, d_obs, imloc=im0, want_fields=True)
        assert_bit_equal(P, fwd[0], "shot P, " + what)
        assert_bit_equal(PP, fwd[1], "shot PP, " + what)
        assert_bit_equal(img, want["forward snapshots", d["nt"]], "shot image, " + what)


# ---------------------------------------------------------------------------------------------------------------------------------------
# recording
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _record_case(grid, gz, sz):
    nxe, nze, nxb, nzb = grid
    nt = 14
    d = rtm_deck(grid, nt, seed=5, dx=10.0, dz=12.5)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0
    orc = O.Oracle(*args_of(d), compat=True)
    want, oP, oPP = oracle_gather(orc, d["v2"], d["sx"], sz, gz, srce, nxb, nxe - 2 * nxb)
    live = min(nxe - 2 * nxb, 8 * (nxe // 8) - nxb)              # receiver rows the reference time-steps
    assert np.count_nonzero(want[:live, -1]) > 0.2 * live and np.count_nonzero(want) > 2 * live
    return d, srce, want, oP, oPP


@pytest.mark.parametrize("pf", PREFETCH)
@pytest.mark.parametrize("grid,gz,sz", [(RAGGED, 255, 252), (RAGGED, 256, 259), (WIDE, 511, 509), (WIDE, 512, 514)],
                         ids=["ragged-gz255", "ragged-gz256", "wide-gz511", "wide-gz512"])
def test_record_shot_at_every_prefetch_distance(grid, gz, sz, pf):
    """The receiver line on both sides of a border of the one-step kernel's 256-column strips; the source a few cells from it."""
    d, srce, want, oP, oPP = _record_case(grid, gz, sz)
    ctx = F.FDWave(*args_of(d), compat=True)
    for xchunk in chunks(pf):
        tune(ctx, pf, xchunk)
        what = f"{grid} gz {gz} prefetch {pf} xchunk {xchunk}"
        data, P, PP = ctx.record_shot(d["v2"], d["sx"], sz, gz, srce, want_fields=True)
        assert_bit_equal(data, want, "gather, " + what)
        assert_bit_equal(P, oP, "P, " + what)
        assert_bit_equal(PP, oPP, "PP, " + what)
    if grid == RAGGED:
        assert not want[64 - grid[2]:].any()                      # receiver rows 64, 65: never time-stepped, zero from rest


# ---------------------------------------------------------------------------------------------------------------------------------------
# illumination
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _illum_case(sz, nsteps):
    nxe, nze, nxb, nzb = RAGGED
    d = rtm_deck(RAGGED, max(STEP_COUNTS), seed=3, dx=10.0, dz=12.5)
    p0, pp0 = random_fields(d, 5)
    il0 = (0.5 + np.random.default_rng(9).random((nxe, nze))).astype(np.float32)
    srce = O.ricker_wavelet(d["nt"], 0.001, 30.0) * 1000.0 + np.float32(3.0)
    xlim, zlim, _ = O.extents(nxe, nze, nzb, True)
    orc = O.Oracle(*args_of(d), compat=True)
    want, _, oPP = illum_restatement(orc, d["v2"], d["sx"], sz, srce[:nsteps], xlim, zlim, p0, pp0, il0)
    assert (want[:xlim, :zlim] > il0[:xlim, :zlim]).mean() > 0.9      # nearly every cell inside the extents has gained
    assert_bit_equal(want[xlim:], il0[xlim:], "restatement outside the extents")
    assert_bit_equal(want[:, zlim:], il0[:, zlim:], "restatement outside the extents")
    return d, p0, pp0, il0, srce, want, oPP


@pytest.mark.parametrize("pf", PREFETCH)
@pytest.mark.parametrize("sz", [255, 256])
def test_dev_illum_steps_at_every_prefetch_distance(sz, pf):
    """fdw_dev_illum_steps from noise-filled fields and a positive entry illumination against the chained restatement, for every step count
    of test_illum.py; _Device.illum() checks that the padding columns stay zero."""
    import torch
    for nsteps in STEP_COUNTS:
        d, p0, pp0, il0, srce, want, oPP = _illum_case(sz, nsteps)
        ctx = F.FDWave(*args_of(d), compat=True, device=0)
        for xchunk in chunks(pf):
            tune(ctx, pf, xchunk)
            what = f"sz {sz}, {nsteps} steps, prefetch {pf} xchunk {xchunk}"
            a = _Device(ctx, d, p0, pp0, il0, srce)
            ia = ctx.dev_illum_steps(a.ptrs(), a.v2.data_ptr(), a.srce.data_ptr(), d["sx"], sz, a.il.data_ptr(), 0, nsteps)
            torch.cuda.synchronize()
            assert_bit_equal(a.illum(), want, "illumination, " + what)
            assert_bit_equal(a.field(ia[1]), oPP, "PP, " + what)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the sibling's dialects: MOD, and DD_FWD + DD_RECV
# ---------------------------------------------------------------------------------------------------------------------------------------
DD_CASES = [  # nx, nz, nxb, nzb, nt, dx, dz, fac, (sx, sz, gz) on the extended grid
    (110, 1252, 20, 24, 12, 10.0, 10.0, 0.02, (56, 26, 27)),          # WIDE
    (61, 290, 10, 10, 14, 8.0, 12.5, 0.05, (17, 254, 257)),           # nxe = 81, nze = 310; source blob and receivers across the strip border at z = 256
    (61, 47, 17, 13, 40, 10.0, 12.5, 0.02, (17 + 18, 14, 15)),        # nxe = 95, nze = 73: one partial strip
]
for _c in DD_CASES:
    for _pf in PREFETCH:
        assert all(ring_has_wrapped(_c[8][0], c, RING[_pf]) for c in chunks(_pf) if c), _c


@functools.lru_cache(maxsize=None)
def _dd_model(i):
    nx, nz, nxb, nzb, nt, dx, dz, fac, _ = DD_CASES[i]
    rng = np.random.default_rng(nx * 31 + nz)
    vp = (1500 + 2500 * rng.random((nx, nz))).astype(np.float32)
    v2 = np.zeros((nx + 2 * nxb, nz + 2 * nzb), np.float32)
    v2[nxb:nxb + nx, nzb:nzb + nz] = vp * vp
    v2 = O.mod_extendvel(v2, nx, nz, nxb, nzb)
    srce = (O.mod_ricker_wavelet(nt, 0.001, 40.0) + 0.1 * rng.standard_normal(nt)).astype(np.float32)      # non-zero to the last step
    dobs = rng.standard_normal((2, nx, nt)).astype(np.float32)
    return v2, srce, dobs


@functools.lru_cache(maxsize=None)
def _mod_want(i):
    nx, nz, nxb, nzb, nt, dx, dz, fac, (sx, sz, gz) = DD_CASES[i]
    v2, srce, _ = _dd_model(i)
    want = O.mod_shot(8, nx, nz, nxb, nzb, dx, dz, 0.001, fac, v2, sx, sz, gz, srce)
    assert np.count_nonzero(want[:, -1]) > 0.2 * nx and np.count_nonzero(want) > 2 * nx
    return want


@pytest.mark.parametrize("pf", PREFETCH)
@pytest.mark.parametrize("i", range(len(DD_CASES)), ids=lambda i: "x".join(map(str, DD_CASES[i][:5])))
def test_model_shot_at_every_prefetch_distance(i, pf):
    nx, nz, nxb, nzb, nt, dx, dz, fac, (sx, sz, gz) = DD_CASES[i]
    v2, srce, _ = _dd_model(i)
    want = _mod_want(i)
    ctx = F.FDWave(8, nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt, fac, dx, dz, 0.001, dialect=1)
    for xchunk in chunks(pf):
        tune(ctx, pf, xchunk)
        assert_bit_equal(ctx.model_shot(v2, sx, sz, gz, srce), want, f"gather, case {i} prefetch {pf} xchunk {xchunk}")


@functools.lru_cache(maxsize=None)
def _stored_want(i, shot):
    nx, nz, nxb, nzb, nt, dx, dz, fac, (sx, sz, gz) = DD_CASES[i]
    v2, srce, dobs = _dd_model(i)
    want = O.rtm_stored_shot(8, nx, nz, nxb, nzb, dx, dz, 0.001, fac, v2, sx, sz, gz, srce, dobs, shot=shot)
    # rtm_main's receivers sit on rows ix + nzb (fdw_api.cpp place_receivers); their depth and the source's in interior coordinates
    assert_image_not_vacuous(want, reach(nx, nz, sx - nxb, sz - nzb, gz - nzb, nt), f"stored-wavefield RTM, case {i} shot {shot}")
    return want


@pytest.mark.parametrize("pf", PREFETCH)
@pytest.mark.parametrize("i", range(len(DD_CASES)), ids=lambda i: "x".join(map(str, DD_CASES[i][:5])))
def test_rtm_stored_shot_at_every_prefetch_distance(i, pf, monkeypatch):
    """Both shots of a two-shot gather (the second reads one sample past its last trace); every field kept, and once checkpointed into
    segments of seven steps (FDW_STORE_SEGMENT), which recomputes the source pass segment by segment."""
    nx, nz, nxb, nzb, nt, dx, dz, fac, (sx, sz, gz) = DD_CASES[i]
    v2, srce, dobs = _dd_model(i)
    ctx = F.FDWave(8, nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt, fac, dx, dz, 0.001, dialect=2)
    for shot in (0, 1):
        want = _stored_want(i, shot)
        for xchunk in chunks(pf):
            tune(ctx, pf, xchunk)
            for seg in (None, 7) if xchunk == RING[pf] else (None,):
                if seg:
                    monkeypatch.setenv("FDW_STORE_SEGMENT", str(seg))
                got = ctx.rtm_stored_shot(v2, sx, sz, gz, srce, dobs, shot=shot)
                monkeypatch.delenv("FDW_STORE_SEGMENT", raising=False)
                assert ctx.store_segments() == (-(-nt // seg) if seg else 1)
                assert_bit_equal(got, want, f"image, case {i} shot {shot} prefetch {pf} xchunk {xchunk} segment {seg}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# FAST numerics past fill_geometry's large-grid threshold: the chunk is sized for a ring the FAST kernels (always prefetch 2) do not have
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fast_large_case():
    nxe, nze, nb, nsteps = 6400, 8192, 16, 3
    rng = np.random.default_rng(64)
    v2 = ((1500.0 + 2000.0 * rng.random((nxe, nze), dtype=np.float32)) ** 2).astype(np.float32)
    p0 = 0.1 * rng.standard_normal((nxe, nze), dtype=np.float32)
    pp0 = 0.1 * rng.standard_normal((nxe, nze), dtype=np.float32)
    srce = (O.ricker_wavelet(nsteps, 0.001, 30.0) * 1000.0 + 3.0).astype(np.float32)
    orc = O.Oracle(8, nxe, nze, nb, nb, nsteps, 0.75, 10.0, 10.0, 0.001, compat=True, omp=True, numerics=1)
    oP, oPP = orc.forward(v2, nxe // 2 + 5, 1000, srce, p0, pp0)
    assert np.count_nonzero(oPP) > 0.99 * oPP.size
    return (nxe, nze, nb, nsteps), v2, p0, pp0, srce, oP, oPP


@pytest.mark.parametrize("pf", [1, 3])
def test_fast_numerics_with_a_chunk_sized_for_another_ring(pf):
    """rows x 256-column strips >= 200 000: with xchunk = 0 fill_geometry takes one ring turn of effective_prefetch() -- 9 or 12 rows --
    for kernels whose ring holds 10.  Three steps from noise-filled fields equal the oracle's FAST restatement bit for bit."""
    (nxe, nze, nb, nsteps), v2, p0, pp0, srce, oP, oPP = _fast_large_case()
    ctx = F.FDWave(8, nxe, nze, nb, nb, nsteps, 0.75, 10.0, 10.0, 0.001, compat=True, numerics=1)
    tune(ctx, pf, 0)
    assert ctx.extents()[0] * -(-ctx.pitch // 256) >= 200000
    P, PP = ctx.forward(v2, nxe // 2 + 5, 1000, srce, p0, pp0)
    ctx.close()
    assert_bit_equal(PP, oPP, f"FAST PP, prefetch {pf}")
    assert_bit_equal(P, oP, f"FAST P, prefetch {pf}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# orders 2, 4, 6 (prefetch 2 only), both numerics: the backward loop in both forms and the stored-wavefield RTM
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("order", [2, 4, 6])
def test_backward_loop_low_orders_fused_and_in_two_launches(order, numerics, monkeypatch):
    """BACK, and PLAIN + RECV under FDW_NO_FUSED_BACK=1, of the register-ring kernels of orders 2, 4 and 6, EXACT against the oracle and FAST
    against its FAST restatement, on the ragged compat grid with dx != dz."""
    nxe, nze, nxb, nzb = RAGGED
    nt = 12
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=order, order=order, dx=10.0, dz=12.5)
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    rng = np.random.default_rng(order)
    srce = (O.ricker_wavelet(nt, d["dt"], 30.0) * 1000.0 + 3.0).astype(np.float32)
    d_obs = rng.standard_normal((nx, nt)).astype(np.float32)
    im0 = rng.standard_normal((nx, nz)).astype(np.float32)
    s0, s1 = random_fields(d, seed=15, amp=0.1)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    oP, oPP = orc.forward(d["v2"], d["sx"], d["sz"], srce)
    hops = -(-np.abs(np.arange(nz)[None, :] - (d["gz"] - nzb)) // (order // 2))
    rows = np.arange(nx)[:, None] + nxb < 8 * (nxe // 8)
    assert_image_not_vacuous(orc.back(d["v2"], s0, s1, d_obs, d["gz"]), (hops <= nt - 1) & rows, f"order {order} numerics {numerics}")
    for fused in (True, False):
        if not fused:
            monkeypatch.setenv("FDW_NO_FUSED_BACK", "1")
        ctx = F.FDWave(*args_of(d), compat=True, numerics=numerics)
        monkeypatch.delenv("FDW_NO_FUSED_BACK", raising=False)
        ctx.set_tuning(two_step=-1)
        assert ctx.steps_per_pass() == 1
        what = f"order {order} numerics {numerics} fused={fused}"
        for n in (nt, 3):
            assert_bit_equal(ctx.back(d["v2"], s0, s1, d_obs, d["gz"], imloc=im0, nsteps=n),
                             orc.back(d["v2"], s0, s1, d_obs, d["gz"], imloc=im0, nsteps=n), f"image from noise snapshots, {n} iterations, {what}")
        img, P, PP = ctx.shot(d["v2"], d["sx"], d["sz"], d["gz"], srce, d_obs, imloc=im0, want_fields=True)
        assert_bit_equal(PP, oPP, "shot PP, " + what)
        assert_bit_equal(img, orc.back(d["v2"], oP, oPP, d_obs, d["gz"], imloc=im0), "shot image, " + what)
        ctx.close()


@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("order", [2, 4, 6])
def test_rtm_stored_shot_low_orders(order, numerics, monkeypatch):
    """DD_FWD and DD_RECV of orders 2, 4 and 6 in both numerics, every field kept and checkpointed."""
    nx, nz, nxb, nzb, nt, dx, dz, fac, (sx, sz, gz) = DD_CASES[1]
    v2, srce, dobs = _dd_model(1)
    want = O.rtm_stored_shot(order, nx, nz, nxb, nzb, dx, dz, 0.001, fac, v2, sx, sz, gz, srce, dobs, shot=1, numerics=numerics)
    assert np.count_nonzero(want) > 100
    ctx = F.FDWave(order, nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt, fac, dx, dz, 0.001, dialect=2, numerics=numerics)
    for seg in (None, 5):
        if seg:
            monkeypatch.setenv("FDW_STORE_SEGMENT", str(seg))
        got = ctx.rtm_stored_shot(v2, sx, sz, gz, srce, dobs, shot=1)
        monkeypatch.delenv("FDW_STORE_SEGMENT", raising=False)
        assert_bit_equal(got, want, f"image, order {order} numerics {numerics} segment {seg}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# the image comparer (bin/psnr's device work): the census showed its three kernels launched by test_programs only
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 65539, 300007])
def test_image_compare_vs_oracle(n):
    """fdw_image_compare on seeded arrays: 300 007 elements are more than its 1024 blocks of 256 take in one stride.  The tool's own
    arithmetic (serial fp32 sums of squares formed in double, one lane) equals the oracle's restatement in all four figures exactly, and the
    difference a - b bit for bit.  exact_sums: the squares are exact in double, so the parallel sum differs from the exact sum (math.fsum)
    by at most (n - 1) 2^-53 relative in any order -- 3.4e-11 here -- plus a rounding each for the quotient, the root and the logarithm;
    asserted at 1e-9 (relative for MSE and RMSE, absolute on the decibel figures, whose derivative 10 / ln 10 keeps that inside 1e-9)."""
    import math
    rng = np.random.default_rng(n)
    b = rng.standard_normal(n).astype(np.float32)
    b[n // 2] = -7.5                                              # the largest |b| is negative
    a = (b + np.float32(0.05) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    ost, odiff = O.image_compare(a, b, want_diff=True)
    assert np.count_nonzero(odiff) > 0.9 * n and all(np.isfinite(ost)) and ost[0] > 0
    st, diff = F.image_compare(a, b, want_diff=True)
    assert_bit_equal(diff, odiff, f"difference, n = {n}")
    for k, v in zip(("mse", "rmse", "snr", "psnr"), ost):
        assert st[k] == v, (n, k, st[k], v)
    st2, diff2 = F.image_compare(a, b, want_diff=True, exact_sums=True)
    assert_bit_equal(diff2, odiff, f"difference, exact_sums, n = {n}")
    d64, b64 = odiff.astype(np.float64), b.astype(np.float64)
    sd, sb = math.fsum(d64 * d64), math.fsum(b64 * b64)
    mse = sd / n
    want = dict(mse=mse, rmse=math.sqrt(mse), snr=10.0 * math.log10(sb / sd), psnr=20.0 * math.log10(7.5 / math.sqrt(mse)))
    assert (n - 1) * 2.0 ** -53 < 1e-10
    for k in ("mse", "rmse"):
        assert abs(st2[k] - want[k]) <= 1e-9 * want[k], (n, k, st2[k], want[k])
    for k in ("snr", "psnr"):
        assert abs(st2[k] - want[k]) <= 1e-9, (n, k, st2[k], want[k])

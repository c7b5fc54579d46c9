"""Excitation-amplitude imaging, second part (fdwave.h): the image formed on the device (fdw_dev_image_excitation), fdw_shot_excitation that
downloads one array, batches of excitation shots (fdw_shot_excitation_batch) and rtm_code's exc=1 decks in groups.

Everything is compared bit for bit.  The anchors: fdw_image_excitation / its numpy spelling image_formula for the image, and for a batch the
shots one by one (fdw_shot_excitation per shot, then image_formula in shot order), which tests/test_excitation.py pins to the CPU oracle.

Whole shots and batches also run on the three edge decks of tests/stream_cases.py (flush: pitch == nze, strips run into the next row;
onecol: the third pipeline strip owns one column; narrow: 41 rows) -- the batched kernels address shot b at b * bstride inside the library's
own buffers, so no guarded arena can hold them; what can be done is to run them where no padding column absorbs a stray store.  What these
cases CANNOT see: a shot starts from rest, so the fields near the array ends are still zero after 40 steps and a stray store of an unchanged
word there is invisible.  The arena cases of tests/test_dev_footprint.py are the ones with teeth."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
import footprint_arena as FA
import stream_cases as SC
import value_classes as V
from conftest import ROOT, assert_bit_equal, make_deck
from oracle import oracle as O
from test_excitation import SHOT_GRIDS, Device, _run_rtm_code, image_formula, image_selection, shot_case, shot_restatement
from test_line_source import args_of
from test_stepn_isa_budget import isa  # noqa: F401  (a fixture)

gpu = pytest.mark.gpu
EINVAL, ESTATE = -1, -5
NEW_KERNELS = ("fdw_exc_peak_kernel", "fdw_exc_stack_kernel", "fdw_gather_transpose_rev_kernel")


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: symbols, the division argument, the built kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_entry_points_are_exported():
    L = F.lib()
    for name in ("fdw_dev_image_excitation", "fdw_shot_excitation_batch"):
        assert hasattr(L, name)
    for name in ("dev_image_excitation", "shot_excitation_batch"):
        assert hasattr(F.FDWave, name)


def _same_quotients(a, b, what):
    """(float)((double)a / (double)b) == a / b in float32, bit for bit; NaNs by position."""
    with np.errstate(all="ignore"):
        narrow = a / b
        wide = (a.astype(np.float64) / b.astype(np.float64)).astype(np.float32)
    assert narrow.dtype == np.float32
    V.assert_same_nonfinite(wide, narrow, what)
    return narrow


def test_a_double_quotient_rounded_once_is_the_fp32_quotient():
    """The stack kernel divides in double and rounds once.  fp64 carries 53 >= 2 * 24 + 2 significand bits, so the double quotient of two fp32
    numbers never lies close enough to a rounding boundary of fp32 for the second rounding to move it -- subnormal results included, where
    fp32 keeps fewer bits still."""
    rng = np.random.default_rng(17)
    n = 1 << 20
    a, b = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(2))
    q = _same_quotients(a, b, "random operand bit patterns")
    assert np.isnan(q).any() and np.isinf(q).any() and (q == 0).any()
    # quotients forced into the subnormal range of fp32: |a| in [2^-126, 2^-100), |b| in [2, 2^41)
    a, b = V._exponent_range(rng, n, -126, -101), V._exponent_range(rng, n, 1, 40)
    q = _same_quotients(a, b, "subnormal quotients")
    sub = (q != 0) & (np.abs(q) < V.MIN_NORMAL)
    assert sub.mean() > 0.3, sub.mean()
    # the value classes of tests/test_value_domain.py and the infinities, every pair of them
    classes = {c: V.class_values(c, 4096, rng, large_exp=100) for c in V.CLASSES}
    classes["inf"] = np.where(rng.integers(0, 2, 4096) == 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    classes["nan"] = np.full(4096, np.nan, np.float32)
    for ca, va in classes.items():
        for cb, vb in classes.items():
            _same_quotients(va, rng.permutation(vb), f"{ca} / {cb}")


def test_the_image_kernels_are_built_without_scratch_or_spills(isa):      # noqa: F811
    for base in NEW_KERNELS:
        names = [k for k in isa if f"{len(base)}{base}E" in k]
        assert len(names) == 1, (base, names)
        meta, body = isa[names[0]]
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (base, meta)
    stack = [mn for mn, _ in isa[[k for k in isa if "fdw_exc_stack_kernelE" in k][0]][1]]
    assert any(mn.startswith("v_div_fmas_f64") for mn in stack) and not any(mn.startswith("v_div_fmas_f32") for mn in stack)
    peak = [mn for mn, _ in isa[[k for k in isa if "fdw_exc_peak_kernelE" in k][0]][1]]
    assert any(mn.startswith("global_atomic_umax") for mn in peak), "one vector atomic maximum per wave"


# ---------------------------------------------------------------------------------------------------------------------------------------
# the decks of the batches: shot_case's, with a gather per shot
# ---------------------------------------------------------------------------------------------------------------------------------------
NT = 23
ROWS_UP = (30, 5)          # sx0, dsx: rows 30, 35, 40, 45
ROWS_DOWN = (45, -5)
ROW_STILL = (40, 0)        # dsx = 0: the shots differ in model and gather alone
ORDERS = [(8, 1), (8, 2), (8, 3), (4, 0)]      # (order, prefetch)
# The edge decks of tests/stream_cases.py (geometry and compat from its table): (sz, gz) and the first source row of the ascending run.
# 40 steps: at 23 an order-4 shot on `narrow` picks 77 non-zero cells, short of the 100 every case asks for.  The placements are not the
# table's: onecol's puts the receiver depth in the damped border, where the pick finds nothing in the interior.  narrow has 41 rows (29
# interior): its source rows are 12, 17, 22, 27.
EDGE_NT = 40
EDGE_PLACE = {"flush": (258, 255), "narrow": (40, 38), "onecol": (436, 432)}
EDGE_ROW0 = {"flush": 30, "narrow": 12, "onecol": 30}
EDGE_ORDERS = [(8, 2), (4, 0)]


def row0_of(grid):
    return EDGE_ROW0.get(grid, 30)


def runs_of(grid):
    """BATCH_RUNS with the source rows of the grid: [((sx0, dsx), shots, eps)]."""
    shift = row0_of(grid) - 30
    return [((rows[0] + shift, rows[1]), n, eps) for rows, n, eps in BATCH_RUNS]


@functools.lru_cache(maxsize=None)
def batch_deck(grid, order):
    edge = grid in EDGE_PLACE
    nxe, nze, nxb, nzb = SC.DECKS[grid]["geom"] if edge else SHOT_GRIDS[grid]
    nt = EDGE_NT if edge else NT
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=3, order=order, compat=SC.DECKS[grid]["compat"] if edge else True)
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    srce = O.ricker_wavelet(nt, 0.001, 120.0) * 1000.0
    gathers = np.stack([np.random.default_rng(2 + b).standard_normal((nx, nt)).astype(np.float32) for b in range(4)])
    im0 = np.random.default_rng(77).standard_normal((nx, nz)).astype(np.float32)
    im0[::3, ::2] = -0.0
    for a in (srce, gathers, im0, d["v2"]):
        a.setflags(write=False)
    sz, gz = EDGE_PLACE[grid] if edge else (nzb + 30, nzb + 26)
    if edge:
        assert FA.pitch_of(nze) == {"flush": nze, "narrow": 64, "onecol": 512}[grid] and 0 <= gz < sz < O.extents(nxe, nze, nzb, d["compat"])[1]
    return d, nx, nz, srce, gathers, sz, gz, im0


def model_of(d, k):
    """Model k of a deck: v2 (*) (1 + 0.05 k)."""
    return (d["v2"] * np.float32(1.0 + 0.05 * k)).astype(np.float32) if k else d["v2"]


def shots_of(rows, n, row0=30):
    """[(source row, gather index b, model index k)] of a batch of n shots.  Every shot of every batch has a model of its own, so that a
    launch that reads another shot's model changes bytes.  Where the source moves the model belongs to the source ROW, k = (sx - 30) / 5:
    the ascending run has model b for shot b (v2 (*) (1 + 0.05 b)), the descending run meets the same four (row, model) pairs with other
    gathers; with dsx = 0 shot b has model b.  row0: the first row of the grid's ascending run (30 but on the `narrow` deck)."""
    sx0, dsx = rows
    return [(sx0 + b * dsx, b, (sx0 + b * dsx - row0) // 5 if dsx else b) for b in range(n)]


@functools.lru_cache(maxsize=None)
def restated(grid, order, numerics, sx, b, k):
    """The CPU restatement of one shot of a batch: the interiors of exc, amp, texc and the iterations with a non-zero pick."""
    d, nx, nz, srce, gathers, sz, gz, _ = batch_deck(grid, order)
    orc = O.Oracle(*args_of(d), compat=d["compat"], numerics=numerics)
    exc, amp, texc, _, _, iters = shot_restatement(orc, d, model_of(d, k), sx, sz, gz, srce, gathers[b])
    inner = (slice(d["nxb"], d["nxb"] + nx), slice(d["nzb"], d["nzb"] + nz))
    out = dict(exc=exc[inner].copy(), amp=amp[inner].copy(), texc=texc[inner].copy(), iters=frozenset(iters))
    for a in (out["exc"], out["amp"], out["texc"]):
        a.setflags(write=False)
    return out


def assert_conditions(grid, order, numerics, rows, n, eps):
    """What every batch case asks of its shots, on the restatement alone: at least 100 picked non-zero cells from at least 5 iterations per
    shot; at eps = 1e-3 at least 20 interior cells both selected and carrying a non-zero exc; consecutive running images differ.  Returns
    the restated running images [n][nx][nz]."""
    _, nx, nz, _, _, _, _, im0 = batch_deck(grid, order)
    img, stack = im0, []
    for sx, b, k in shots_of(rows, n, row0_of(grid)):
        w = restated(grid, order, numerics, sx, b, k)
        nonzero = int((w["exc"] != 0).sum())
        sel = image_selection(w["amp"], eps).reshape(nx, nz)
        both = int((sel & (w["exc"] != 0)).sum())
        print(f"{grid} order {order} numerics {numerics} sx {sx} gather {b}: {nonzero} picked non-zero cells from {len(w['iters'])} iterations, "
              f"{both} selected and non-zero at eps {eps}")
        new = image_formula(w["exc"], w["amp"], eps, img)
        assert nonzero >= 100 and len(w["iters"]) >= 5, (nonzero, sorted(w["iters"]))
        assert eps != 1e-3 or both >= 20, both
        assert (new.view(np.uint32) != np.asarray(img).view(np.uint32)).any(), "the shot does not move the running image"
        img = new
        stack.append(img)
    return np.stack(stack)


BATCH_RUNS = [(ROWS_UP, 4, 1e-3), (ROWS_DOWN, 4, 0.0), (ROW_STILL, 3, 1e-3)]


@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("order", [8, 4])
@pytest.mark.parametrize("grid", list(SHOT_GRIDS) + list(EDGE_PLACE))
def test_the_batch_decks_meet_their_conditions(grid, order, numerics):
    """The conditions of every batch case, asserted here once, on the restatement alone and without a device, for every deck, order, numerics,
    row sequence and eps the GPU cases run (which assert the same before they ask the device).  The restatement gives 106 .. 220
    picked non-zero cells from 7 .. 12 iterations and 23 .. 70 cells both selected and non-zero at eps = 1e-3.  (The count is where the
    receiver field has arrived by each cell's excitation time: it depends on the source row and the model, not on the gather.  On ONE shared
    model rows 35 and 45 of the 69 x 301 grid at order 4 would pick 99 cells; every shot has a model of its own here, see shots_of.)
    On the three edge decks, 40 steps (orders 4, 8 and, for the whole shots, 10): 194 .. 471 picked non-zero cells from 25 .. 30 iterations,
    168 .. 344 both selected and non-zero at eps = 1e-3; no source row had to be moved."""
    for rows, n, eps in runs_of(grid):
        assert_conditions(grid, order, numerics, rows, n, eps)
    assert_conditions(grid, order, numerics, runs_of(grid)[0][0], 4, 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_dev_image_excitation against image_formula / fdw_image_excitation
# ---------------------------------------------------------------------------------------------------------------------------------------
IMAGE_GRIDS = [(87, 70, 12, 10), (69, 301, 3, 10)]      # pitch 128 and 320: padding columns on both, a second 256-column strip on the second
SENTINELS = np.array([0x7FC12345, 0xFFC54321, 0x42F70000, 0x7F800000, 0x00000001, 0x80000000], np.uint32)      # NaN payloads, 123.5, inf, ...


def _words(shape, seed):
    return SENTINELS[np.random.default_rng(seed).integers(0, len(SENTINELS), shape)]


def image_inputs(grid, pitch, pattern):
    """(exc, amp, img) as uint32 words [nxe][pitch], built from the value classes.  Outside the interior all three carry sentinel words; in amp
    the border holds +inf and the padding columns 3.3e38, both above every finite interior peak."""
    nxe, nze, nxb, nzb = grid
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    inner = (slice(nxb, nxb + nx), slice(nzb, nzb + nz))
    rng = np.random.default_rng(5)
    xc, zc = V.cuts(nx, [nx // 3, nx // 2], rng, 3), V.cuts(nz, [4, 64 - nzb, 256 - nzb, nz // 2], rng, 3)
    exc, amp, img = (_words((nxe, pitch), s).copy() for s in (1, 2, 3))
    e = V.patched((nx, nz), 11, classes=V.CLASSES, xcuts=xc, zcuts=zc, large_exp=60)
    e[1::7, 2::5], e[2::7, 3::5], e[3::9, 1::6] = np.inf, -np.inf, np.nan
    a = V.patched((nx, nz), 12, classes=V.FINITE, xcuts=xc, zcuts=zc, large_exp=60)
    a[4::11, 5::7] = np.nan
    if pattern == "inf":
        a[nx // 2, nz // 2], a[3, 5] = np.inf, -np.inf
    elif pattern == "allnan":
        a[:] = np.nan
    elif pattern == "allzero":
        a[:] = 0.0
        a[::2, ::3] = -0.0
    i = np.random.default_rng(9).standard_normal((nx, nz)).astype(np.float32)
    i[::2, 1::2] = -0.0
    exc[inner], amp[inner], img[inner] = e.view(np.uint32), a.view(np.uint32), i.view(np.uint32)
    amp[0, 1] = np.float32(np.inf).view(np.uint32)                  # the border
    amp[nxb + 1, pitch - 1] = np.float32(3.3e38).view(np.uint32)    # a padding column
    assert pitch > nze
    return exc, amp, img, inner


IMAGE_CASES = [("finite", 0.0, True), ("finite", 1e-3, True), ("finite", 1.0, False), ("finite", 3e38, False), ("inf", 1e-3, False), ("inf", 0.0, False),
               ("allnan", 1e-3, False), ("allnan", 0.0, False), ("allzero", 1e-3, False), ("allzero", 0.0, False)]


@gpu
@pytest.mark.parametrize("grid", IMAGE_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_dev_image_excitation_vs_the_formula(grid):
    import torch
    nxe, nze, nxb, nzb = grid
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, NT, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    dev = torch.device("cuda:0")
    for pattern, eps, some in IMAGE_CASES:
        exc, amp, img, inner = image_inputs(grid, ctx.pitch, pattern)
        what = f"{nxe}x{nze} {pattern} eps {eps}"
        e, a, i = (x[inner].view(np.float32) for x in (exc, amp, img))
        sel = image_selection(a, eps).reshape(a.shape)
        print(f"{what}: {int(sel.sum())} of {sel.size} cells selected")
        if some:
            assert sel.any() and not sel.all() and ((~sel) & (i.view(np.uint32) == 0x80000000)).any()
        else:
            assert not sel.any()
        want = image_formula(e, a, eps, i)
        d_exc, d_amp, d_img = (torch.from_numpy(x.view(np.int32)).to(dev) for x in (exc, amp, img))
        torch.cuda.synchronize()
        ctx.dev_image_excitation(d_exc.data_ptr(), d_amp.data_ptr(), eps, d_img.data_ptr())
        torch.cuda.synchronize()
        got = d_img.cpu().numpy().view(np.uint32)
        V.assert_same_nonfinite(got[inner].view(np.float32), want, "interior vs image_formula, " + what)
        V.assert_same_nonfinite(got[inner].view(np.float32), F.image_excitation(e, a, eps, i), "interior vs fdw_image_excitation, " + what)
        assert_bit_equal(got[inner].view(np.float32)[~sel], i[~sel], "unselected interior cells keep their words, " + what)
        outside = np.ones(img.shape, bool)
        outside[inner] = False
        assert np.array_equal(got[outside], img[outside]), "words of d_img outside the interior, " + what
        assert np.array_equal(d_exc.cpu().numpy().view(np.uint32), exc) and np.array_equal(d_amp.cpu().numpy().view(np.uint32), amp), "inputs, " + what


@gpu
def test_dev_image_excitation_refusals():
    import torch
    nxe, nze, nxb, nzb = IMAGE_GRIDS[0]
    args = (8, nxe, nze, nxb, nzb, NT, 0.75, 10.0, 10.0, 0.001)
    ctx = F.FDWave(*args, compat=True, device=0)
    exc, amp, img, _ = image_inputs(IMAGE_GRIDS[0], ctx.pitch, "finite")
    d_exc, d_amp, d_img = (torch.from_numpy(x.view(np.int32)).to("cuda:0") for x in (exc, amp, img))
    torch.cuda.synchronize()
    L = F.lib()
    p = (d_exc.data_ptr(), d_amp.data_ptr(), d_img.data_ptr())
    for eps in (-1e-3, float("nan"), float("inf"), -float("inf")):
        assert L.fdw_dev_image_excitation(ctx._h, p[0], p[1], eps, p[2], None) == EINVAL
    assert L.fdw_dev_image_excitation(ctx._h, None, p[1], 1e-3, p[2], None) == EINVAL
    assert L.fdw_dev_image_excitation(ctx._h, p[0], None, 1e-3, p[2], None) == EINVAL
    assert L.fdw_dev_image_excitation(ctx._h, p[0], p[1], 1e-3, None, None) == EINVAL
    assert L.fdw_dev_image_excitation(None, p[0], p[1], 1e-3, p[2], None) == EINVAL
    slab = F.FDWave(*args, compat=True, device=0, slab=(16, 40))
    assert L.fdw_dev_image_excitation(slab._h, p[0], p[1], 1e-3, p[2], None) == ESTATE
    mod = F.FDWave(*args, device=0, dialect=1)
    assert L.fdw_dev_image_excitation(mod._h, p[0], p[1], 1e-3, p[2], None) == ESTATE
    torch.cuda.synchronize()
    for t, h in ((d_exc, exc), (d_amp, amp), (d_img, img)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), h), "a refused call touches nothing"


@gpu
@pytest.mark.parametrize("two_step", [-1, 4])
def test_both_loops_and_the_image_chained_on_one_callers_stream(two_step):
    """fdw_dev_excite_steps, fdw_dev_line_pick_steps and fdw_dev_image_excitation on one caller's stream with no synchronisation in between,
    from rest, against the restatement of the whole shot."""
    import torch
    d, nx, nz, srce, d_obs, sz, gz, want = shot_case("87x70", 8, 0)
    w = want[30]
    nt = len(srce)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(two_step=two_step)
    zero = np.zeros((d["nxe"], d["nze"]), np.float32)
    a = Device(ctx, d, zero, zero, srce)
    b = Device(ctx, d, zero, zero, np.ascontiguousarray(d_obs[:, ::-1].T))
    for k in (2, 3):      # from rest: no sentinels in the spare buffers either
        a.bufs[k].zero_()
        b.bufs[k].zero_()
    inner = (slice(d["nxb"], d["nxb"] + nx), slice(d["nzb"], d["nzb"] + nz))
    img0 = _words((d["nxe"], ctx.pitch), 4).copy()
    im = np.random.default_rng(8).standard_normal((nx, nz)).astype(np.float32)
    im[::2] = -0.0
    img0[inner] = im.view(np.uint32)
    d_img = torch.from_numpy(img0.view(np.int32)).to("cuda:0")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    a.excite(30, sz, 0, nt, stream=st.cuda_stream)
    ctx.dev_line_pick_steps(b.ptrs(), b.v2.data_ptr(), b.samples.data_ptr(), gz, a.maps["texc"].data_ptr(), nt, b.maps["exc"].data_ptr(), 0, nt,
                            stream=st.cuda_stream)
    ctx.dev_image_excitation(b.maps["exc"].data_ptr(), a.maps["amp"].data_ptr(), 1e-3, d_img.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    assert_bit_equal(a.map("amp")[inner], w["amp"], "amp")
    assert_bit_equal(b.map("exc")[inner], w["exc"], "exc")
    got = d_img.cpu().numpy().view(np.uint32)
    sel = image_selection(w["amp"], 1e-3).reshape(nx, nz)
    assert sel.any() and not sel.all()
    assert_bit_equal(got[inner].view(np.float32), image_formula(w["exc"], w["amp"], 1e-3, im), "the image of the chained calls")
    outside = np.ones(img0.shape, bool)
    outside[inner] = False
    assert np.array_equal(got[outside], img0[outside])


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_shot_excitation with one download
# ---------------------------------------------------------------------------------------------------------------------------------------
def edge_shot_case(grid, order, numerics):
    """shot_case's tuple for an edge deck: the batch deck's first gather, the source at the third row of its ascending run, 40 steps; the
    condition every whole-shot case asks for is asserted on the restatement before the device is asked."""
    d, nx, nz, srce, gathers, sz, gz, _ = batch_deck(grid, order)
    sx = row0_of(grid) + 10
    w = restated(grid, order, numerics, sx, 0, 0)
    nonzero = int((w["exc"] != 0).sum())
    print(f"{grid} order {order} numerics {numerics} sx {sx}: {nonzero} picked non-zero cells from {len(w['iters'])} iterations")
    assert nonzero >= 100 and len(w["iters"]) >= 5, (nonzero, sorted(w["iters"]))
    return d, nx, nz, srce, gathers[0], sz, gz, {sx: w}


@gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("order,tuning", [(8, dict(two_step=-1)), (8, dict(two_step=4)), (4, {}), (10, {})], ids=str)
@pytest.mark.parametrize("grid", list(SHOT_GRIDS) + list(EDGE_PLACE))
def test_shot_excitation_with_the_image_alone(grid, order, tuning, numerics):
    """On the edge decks (see the module docstring for what they cannot see): every family, pitch == nze among them."""
    d, nx, nz, srce, d_obs, sz, gz, want = (edge_shot_case if grid in EDGE_PLACE else shot_case)(grid, order, numerics)
    sx = row0_of(grid) + 10
    ctx = F.FDWave(*args_of(d), compat=d["compat"], device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    im0 = batch_deck(grid, 8)[7]
    for eps in (1e-3, 0.0):
        alone = ctx.shot_excitation(d["v2"], sx, sz, gz, srce, d_obs, eps, im0, want_maps=False)[0]
        img, exc, amp, texc = ctx.shot_excitation(d["v2"], sx, sz, gz, srce, d_obs, eps, im0)
        what = f"{grid} order {order} {tuning} numerics {numerics} eps {eps}"
        assert_bit_equal(alone, img, "imloc alone vs all four outputs, " + what)
        assert_bit_equal(img, image_formula(exc, amp, eps, im0), "imloc vs image_formula on the returned exc and amp, " + what)
        assert_bit_equal(exc, want[sx]["exc"], "exc vs the restatement, " + what)
        assert (img.view(np.uint32) != im0.view(np.uint32)).any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: batches against the shots one by one
# ---------------------------------------------------------------------------------------------------------------------------------------
def one_by_one(ctx, d, shots, srce, gathers, sz, gz, eps, im0, models=None):
    """fdw_shot_excitation per shot, then image_formula in shot order -> dict(image, stack, exc, amp, texc).  models: None = host models
    (model_of), else (draw_offset, T): the resident model's border models."""
    img, out = im0, dict(stack=[], exc=[], amp=[], texc=[])
    for sx, b, k in shots:
        if models is None:
            v2 = model_of(d, k)
        else:
            ctx.dev_extendvel_linear(models[0] + b * models[1])
            v2 = None
        _, exc, amp, texc = ctx.shot_excitation(v2, sx, sz, gz, srce, gathers[b], eps)
        img = image_formula(exc, amp, eps, img)
        for k, v in (("stack", img), ("exc", exc), ("amp", amp), ("texc", texc)):
            out[k].append(v)
    return dict(image=img, **{k: np.stack(v) for k, v in out.items()})


def assert_same_outputs(got, want, what):
    for k in ("image", "stack", "exc", "amp", "texc"):
        assert_bit_equal(got[k].view(np.float32), want[k].view(np.float32), f"{k}, {what}")


# every grid of SHOT_GRIDS with every (order, prefetch) and both numerics, as before the edge decks; the edge decks with order 8 (prefetch 2)
# and order 4.  The ids are what the stacked decorators gave: grid-order-prefetch-numerics.
BATCH_PARAMS = [(g, o, pf, num) for g, pairs in ([(g, ORDERS) for g in SHOT_GRIDS] + [(g, EDGE_ORDERS) for g in EDGE_PLACE])
                for o, pf in pairs for num in (0, 1)]


@gpu
@pytest.mark.parametrize("grid,order,prefetch,numerics", BATCH_PARAMS, ids=[f"{g}-{o}-{pf}-{('exact', 'fast')[num]}" for g, o, pf, num in BATCH_PARAMS])
def test_batches_equal_the_shots_one_by_one(grid, order, prefetch, numerics):
    """On the edge decks (see the module docstring for what they cannot see): the batched launches at pitch == nze and on 41 rows."""
    d, nx, nz, srce, gathers, sz, gz, im0 = batch_deck(grid, order)
    ctx = F.FDWave(*args_of(d), compat=d["compat"], device=0, numerics=numerics)
    ctx.set_tuning(prefetch=prefetch)
    row0 = row0_of(grid)
    for rows, nmax, eps in runs_of(grid):
        restack = assert_conditions(grid, order, numerics, rows, nmax, eps)
        ref = one_by_one(ctx, d, shots_of(rows, nmax, row0), srce, gathers, sz, gz, eps, im0)
        assert_bit_equal(ref["stack"], restack, f"the one-by-one anchor vs the restatement, {rows}")
        for n in ((1, 2, 3, 4) if rows[1] > 0 else (nmax,)):
            what = f"{grid} order {order} prefetch {prefetch} numerics {numerics} rows {rows} n {n} eps {eps}"
            v2_all = np.stack([model_of(d, k) for _, _, k in shots_of(rows, n, row0)])
            got = ctx.shot_excitation_batch(n, rows[0], rows[1], sz, gz, srce, gathers[:n], eps, v2_all=v2_all, imloc=im0)
            assert ctx.batch_parts() == (1 if n > 1 else 0), what
            want = dict(image=ref["stack"][n - 1], **{k: ref[k][:n] for k in ("stack", "exc", "amp", "texc")})
            assert_same_outputs(got, want, what)
            lean = ctx.shot_excitation_batch(n, rows[0], rows[1], sz, gz, srce, gathers[:n], eps, v2_all=v2_all, imloc=im0, want_stack=False, want_maps=False)
            assert_bit_equal(lean["image"], want["image"], "imloc alone, " + what)


@gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
def test_batch_on_the_resident_model_at_a_draw_offset(numerics):
    grid, order, n, eps = "87x70", 8, 3, 1e-3
    d, nx, nz, srce, gathers, sz, gz, im0 = batch_deck(grid, order)
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    vp = (1500 + 1000 * np.random.default_rng(3).random((nx, nz))).astype(np.float32)
    L = F.lib()
    args = (ctx._h, n, None, 0, 30, 5, sz, gz, srce.ctypes.data, gathers.ctypes.data, C.c_float(eps), np.array(im0).ctypes.data, None, None, None, None)
    assert L.fdw_shot_excitation_batch(*args) == ESTATE      # no model yet
    ctx.model_resident(vp)
    T = ctx.border_draws()
    off = 3 * T + 1
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    inner = (slice(d["nxb"], d["nxb"] + nx), slice(d["nzb"], d["nzb"] + nz))
    for b in range(n):      # the conditions, on the restatement alone, on the models the device draws
        vel = ctx.dev_extendvel_linear(off + b * T, want_vel=True)
        exc, amp, _, _, _, iters = shot_restatement(orc, d, (vel * vel).astype(np.float32), 30 + 5 * b, sz, gz, srce, gathers[b])
        assert (exc[inner] != 0).sum() >= 100 and len(iters) >= 5
        assert (image_selection(amp[inner], eps).reshape(nx, nz) & (exc[inner] != 0)).sum() >= 20
    ref = one_by_one(ctx, d, shots_of(ROWS_UP, n), srce, gathers, sz, gz, eps, im0, models=(off, T))
    got = ctx.shot_excitation_batch(n, 30, 5, sz, gz, srce, gathers[:n], eps, draw_offset=off, imloc=im0)
    assert ctx.batch_parts() == 1
    assert_same_outputs(got, ref, f"resident model, numerics {numerics}")
    for b in range(1, n):
        assert (ref["stack"][b].view(np.uint32) != ref["stack"][b - 1].view(np.uint32)).any()
        assert not np.array_equal(ref["amp"][b], ref["amp"][b - 1])
    other = ctx.shot_excitation_batch(n, 30, 5, sz, gz, srce, gathers[:n], eps, draw_offset=0, imloc=im0)
    assert not np.array_equal(other["amp"], got["amp"]), "the draw offset picks the border models"


@gpu
def test_parts_fallbacks_and_one_context_through_a_sequence():
    grid, order, eps = "87x70", 8, 1e-3
    d, nx, nz, srce, gathers, sz, gz, im0 = batch_deck(grid, order)
    assert_conditions(grid, order, 0, ROWS_UP, 4, eps)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ref = one_by_one(ctx, d, shots_of(ROWS_UP, 4), srce, gathers, sz, gz, eps, im0)
    v2_all = np.stack([model_of(d, k) for _, _, k in shots_of(ROWS_UP, 4)])
    per_shot = 11 * ctx.field_bytes() + 4 * nx * NT      # fdwave.h: eleven fields and one gather [nt][nx] per shot

    def batch(c=ctx):
        return c.shot_excitation_batch(4, 30, 5, sz, gz, srce, gathers, eps, v2_all=v2_all, imloc=im0)
    assert_same_outputs(batch(), ref, "the whole batch")
    assert ctx.batch_parts() == 1
    ctx.set_batch_budget(3 * per_shot)
    assert_same_outputs(batch(), ref, "3 + 1")
    assert ctx.batch_parts() == 2
    ctx.set_batch_budget(2 * per_shot - 1)
    assert_same_outputs(batch(), ref, "parts of one")
    assert ctx.batch_parts() == 4
    ctx.set_batch_budget(per_shot - 1)
    assert_same_outputs(batch(), ref, "a budget below one shot")
    assert ctx.batch_parts() == 0
    ctx.set_batch_budget(0)
    # one context through shot_excitation_batch, shot, shot_excitation_batch
    plain = ctx.shot(d["v2"], 30, sz, gz, srce, gathers[0])
    assert_bit_equal(plain, F.FDWave(*args_of(d), compat=True, device=0).shot(d["v2"], 30, sz, gz, srce, gathers[0]), "fdw_shot after a batch")
    assert_same_outputs(batch(), ref, "the batch after fdw_shot")
    assert ctx.batch_parts() == 1
    # a context outside the batch regime: the same bytes, one by one
    piped = F.FDWave(*args_of(d), compat=True, device=0)
    piped.set_tuning(two_step=4)
    assert_same_outputs(batch(piped), ref, "forced pipeline")
    assert piped.batch_parts() == 0


@gpu
def test_batch_refusals():
    d, nx, nz, srce, gathers, sz, gz, im0 = batch_deck("87x70", 8)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    L = F.lib()
    v2_all = np.stack([d["v2"]] * 2)
    img = np.array(im0)
    good = dict(n=2, v2=v2_all.ctypes.data, sx0=30, dsx=5, sz=sz, gz=gz, srce=srce.ctypes.data, obs=gathers.ctypes.data, eps=1e-3, img=img.ctypes.data)

    def call(c=ctx, **kw):
        a = dict(good, **kw)
        return L.fdw_shot_excitation_batch(c._h, a["n"], a["v2"], 0, a["sx0"], a["dsx"], a["sz"], a["gz"], a["srce"], a["obs"], C.c_float(a["eps"]), a["img"],
                                           None, None, None, None)
    xlim, zlim, _ = ctx.extents()
    for kw in (dict(srce=None), dict(obs=None), dict(img=None), dict(n=0), dict(sx0=xlim - 3), dict(sx0=2, dsx=-5), dict(sz=zlim), dict(gz=-1), dict(gz=zlim),
               dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf"))):
        assert call(**kw) == EINVAL, kw
    assert call(v2=None) == ESTATE                                      # no model
    args = args_of(d)
    assert call(F.FDWave(*args, compat=True, device=0, slab=(16, 40))) == ESTATE
    assert call(F.FDWave(*args, device=0, dialect=1)) == ESTATE
    assert_bit_equal(img, im0, "a refused call writes nothing")
    assert call() == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: rtm_code's exc=1 deck in groups
# ---------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_rtm_code_exc_deck_batched_equals_one_by_one_and_the_python_composition(tmp_path):
    nxe, nze, nxb, nzb = SHOT_GRIDS["87x70"]
    nx, nz, nt, ns = nxe - 2 * nxb, nze - 2 * nzb, 40, 5
    rng = np.random.default_rng(6)
    vp = (1800.0 + 600.0 * rng.random((nx, nz))).astype(np.float32)
    d_obs = rng.standard_normal((ns, nx, nt)).astype(np.float32)
    outs = {}
    for name, env in (("plain", {}), ("single", dict(FDW_NO_SHOT_BATCH="1"))):
        work = tmp_path / name
        (work / "out").mkdir(parents=True)
        vp.tofile(work / "vp.bin")
        d_obs.tofile(work / "dobs.bin")
        (work / "input.dat").write_text(f"tmpdir=./out\nvpfile=./vp.bin\ndatfile=./dobs.bin\nnz={nz}\nnx={nx}\nnt={nt}\ndz=10\ndx=10\ndt=0.001\nfpeak=25\n"
                                        f"ns={ns}\nsz=1\nfsx=5\nds=9\ngz=2\nnxb={nxb}\nnzb={nzb}\nfac=0.75\norder=8\nexc=1\nexc_eps=0.002\n")
        r = _run_rtm_code(work, env)
        assert r.returncode == 0, r.stderr
        m = re.search(r"^## exc: up to (\d+) shots per launch sequence", r.stdout, re.M)
        assert m, r.stdout
        outs[name] = ((work / "out" / "dir.image").read_bytes(), (work / "image.num").read_bytes(), int(m.group(1)),
                      [ln for ln in r.stdout.splitlines() if ln.startswith("** ")])
    assert outs["plain"][2] > 1 and outs["single"][2] == 1
    assert outs["plain"][0] == outs["single"][0], "dir.image"
    assert outs["plain"][1] == outs["single"][1], "image.num"
    assert outs["plain"][3] == outs["single"][3] and len(outs["plain"][3]) == 2 * ns
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    ctx.model_resident(vp)
    srce = F.ricker_wavelet(nt, 0.001, 25.0)
    img, sections = None, []
    for s in range(ns):
        ctx.dev_extendvel_linear(s * ctx.border_draws())
        img = ctx.shot_excitation(None, 5 + 9 * s + nxb, 1 + nzb, 2 + nzb, srce, d_obs[s], 0.002, img)[0]
        sections.append(f"======== {s} ========\n" + "".join(" %f \n" % v for v in img.T.ravel()))
    assert np.abs(img).max() > 0
    assert outs["plain"][0] == img.tobytes(), "dir.image vs the Python composition"
    assert outs["plain"][1].decode() == "".join(sections), "image.num vs the Python composition"

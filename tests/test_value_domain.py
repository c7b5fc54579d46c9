"""Every kernel family at the edges of the fp32 value domain: subnormals, signed zeros, huge values, infinities and NaNs.

The rest of the suite checks the HIP paths against the oracle at a great many shapes and in one value regime (amp * N(0, 1) fields,
velocities of 1200-4200 m/s).  A kernel whose float mode flushed subnormals, or whose masks were written as arithmetic (a 0/1 multiply,
an unconditional `+ 0.0f`), would pass all of it.  This file varies the VALUES (tests/value_classes.py: patches of subnormal, tiny,
+-0, large and overflowing numbers with their borders on the strip / lane / halo / taper borders of the kernels):

  B  static, no GPU   the float mode of every kernel descriptor of libfdwave.so and a census of its multiply-add instructions
  C  CPU              the oracle pinned on these operands independently of itself (spelled-out EXACT chain, zero-velocity restatement on
                      scaled fields, power-of-two homogeneity), the conditions under which the GPU comparisons are not vacuous, and a
                      demonstration that the comparisons reject the three errors this file exists for
  D  GPU (-m gpu)     every kernel family against the oracle, bit for bit (NaNs by position: their sign and payload legitimately differ
                      between x86 and the GPU)

Every GPU test builds its inputs and the oracle's answer through a `_want_*` function that asserts, ON THE ORACLE'S OUTPUT, that the
extreme values survived to the output (MIN_SUBNORMAL_SHARE of subnormals, both zeros, finiteness, 1-50 % non-finite); the CPU test
test_inputs_carry_their_value_classes_to_the_oracle_output runs all of them, so a deck that lost its classes fails without a GPU.
"""
import functools
import re
import subprocess
import tempfile

import numpy as np
import pytest

import rtm_restatement as R
import value_classes as V
from conftest import assert_bit_equal, make_deck, random_fields
from oracle import oracle as O
from test_backward_pins import ZV_DECKS, ZV_IDS
from test_gpu_parity import BACK_CASES
from test_stepn_isa_budget import LLVM, _code_objects, isa  # noqa: F401  (isa is a fixture)

gpu = pytest.mark.gpu
MIN_SUBNORMAL_SHARE = 0.10


# ==== B. static: float mode and instruction census of the built library ====================================================================

# How EXACT and FAST kernels are told apart: every kernel template that exists in both numerics carries the numerics as its LAST template
# argument (csrc: `int NUM`, 0 = the reference's arithmetic, 1 = FAST), so the mangled name ends `...Li0EEEv<args>` or `...Li1EEEv<args>`
# (the form EXACT_QUAD of tests/test_stepn_isa_budget.py spells out for the four-step kernels).  A kernel that is no template has one
# arithmetic only and counts as EXACT.
TEMPLATE_KERNEL = re.compile(r"^_ZN3fdw(?:12_GLOBAL__N_1)?\d+fdw_\w+?_kernelI(?:L[ib]\d+E)*Li([01])EEEv")
PLAIN_KERNEL = re.compile(r"^_ZN3fdw(?:12_GLOBAL__N_1)?\d+fdw_\w+?_kernelE")
FUSED_F32 = re.compile(r"^v_(pk_)?fma(c|mk|ak|_mix|_mixlo|_mixhi)?(_legacy)?_f32")       # v_fma_f32, v_fmac_f32, v_pk_fma_f32, ... any encoding suffix
LEGACY_F32 = re.compile(r"^v_(mad|mac|madmk|madak)(_legacy)?_f32")                       # v_mad_f32, v_mac_f32, v_mad_legacy_f32, ...
# The only fused multiply-adds an EXACT kernel may hold are those of a correctly rounded fp32 DIVISION, which the compiler expands into
# v_div_scale, v_rcp, five fused multiply-adds, v_div_fmas and v_div_fixup -- IEEE division, the same result as the host's.  The kernels that
# divide, by name (none of them is on a time-stepping path):
DIVIDING_KERNELS = ("fdw_image_lap_kernel", "fdw_extendvel_kernel")
FMA_PER_DIVISION = 5
# The generic-order kernels are no templates: they take the numerics at RUN time (StepArgs.numerics) and hold both chains, the EXACT loop
# (products and adds) and the FAST loop (one fused multiply-add per axis and tap pair).  They count as EXACT -- their EXACT path is what
# every order above 8 runs -- with exactly the FAST loop's two fused multiply-adds allowed; that the switch selects the right loop is the
# business of the GPU tests below, which run them on both numerics.
RUNTIME_NUMERICS = {"fdw_generic_kernel": 2, "fdw_generic_rec_kernel": 2}


def _allowed_fused(kernel, ndiv):
    return FMA_PER_DIVISION * ndiv + sum(n for name, n in RUNTIME_NUMERICS.items() if f"{len(name)}{name}E" in kernel)


def _split(isa_map):
    exact, fast, neither = [], [], []
    for k in isa_map:
        m = TEMPLATE_KERNEL.match(k)
        if m:
            (fast if m.group(1) == "1" else exact).append(k)
        elif PLAIN_KERNEL.match(k):
            exact.append(k)
        else:
            neither.append(k)
    return exact, fast, neither


def _count(body, rx):
    return sum(1 for mn, _ in body if rx.match(mn))


@pytest.fixture(scope="module")
def descriptors(isa):      # noqa: F811
    """{kernel symbol: {amdhsa directive: value}} from the kernel descriptors (.rodata) of every code object of the library."""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in _code_objects(td):
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-D", "-j", ".rodata", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout
            for name, block in re.findall(r"^\.amdhsa_kernel (\S+)\n(.*?)^\.end_amdhsa_kernel", text, re.M | re.S):
                out[name] = {k: int(v, 0) for k, v in re.findall(r"^\s*\.amdhsa_(\w+) (\S+)$", block, re.M)}
    return out


def test_every_kernel_keeps_subnormals_and_rounds_to_nearest_even(isa, descriptors):      # noqa: F811
    """"fp32 denormals are preserved".  Every kernel descriptor has float_denorm_mode_32 = 3 and float_denorm_mode_16_64 = 3
    (subnormals kept on input and output) and round mode 0 (to nearest even) for both; and every disassembled kernel has a descriptor."""
    assert set(descriptors) == set(isa), sorted(set(descriptors) ^ set(isa))
    assert len(descriptors) > 100
    for k, d in descriptors.items():
        mode = {n: d.get(n) for n in ("float_denorm_mode_32", "float_denorm_mode_16_64", "float_round_mode_32", "float_round_mode_16_64")}
        assert mode == {"float_denorm_mode_32": 3, "float_denorm_mode_16_64": 3, "float_round_mode_32": 0, "float_round_mode_16_64": 0}, (k, mode)
    # nothing switches the mode inside a kernel either (s_denorm_mode / s_round_mode / a write of the MODE register)
    for k, (_, body) in isa.items():
        bad = [mn for mn, ops in body if mn in ("s_denorm_mode", "s_round_mode") or (mn.startswith("s_setreg") and any("HW_REG_MODE" in o for o in ops))]
        assert not bad, (k, bad)


def test_every_kernel_is_exact_or_fast_and_only_fast_kernels_fuse(isa):      # noqa: F811
    """Every kernel symbol falls into exactly one of EXACT / FAST (a new kernel cannot go uncounted).  EXACT kernels hold no fp32 fused or
    legacy multiply-add but those of a division expansion and the FAST loop of the two run-time-switched generic-order kernels
    (RUNTIME_NUMERICS); v_fma_f64 is expected: leapfrog_prod's exact 2.0 * p - pp.  FAST kernels do hold
    fused multiply-adds -- so the census is known to see them -- and no legacy v_mad_f32 / v_mac_f32 (which do not keep subnormals)."""
    exact, fast, neither = _split(isa)
    assert not neither, f"kernels that are neither a plain function nor a template whose last argument is the numerics: {neither}"
    assert len(exact) + len(fast) == len(isa) and len(exact) > 60 and len(fast) > 30, (len(exact), len(fast))
    for k in exact:
        body = isa[k][1]
        ndiv = _count(body, re.compile(r"^v_div_fmas_f32"))
        assert _count(body, LEGACY_F32) == 0, k
        assert _count(body, FUSED_F32) == _allowed_fused(k, ndiv), (k, [mn for mn, _ in body if FUSED_F32.match(mn)])
        assert (ndiv > 0) == any(name in k for name in DIVIDING_KERNELS), (k, ndiv)
    for k in fast:
        body = isa[k][1]
        assert _count(body, FUSED_F32) > 0, f"{k}: a FAST kernel without a fused multiply-add (is its last template argument the numerics?)"
        assert _count(body, LEGACY_F32) == 0, k
        assert _count(body, re.compile(r"^v_div_fmas_f32")) == 0, k
    # every FAST kernel has its EXACT twin (same name but for the last template argument)
    twins = {re.sub(r"Li1EEEv", "Li0EEEv", k) for k in fast}
    assert twins <= set(exact), sorted(twins - set(exact))
    assert sum(1 for k in exact if _allowed_fused(k, 0)) == len(RUNTIME_NUMERICS)
    assert any(FUSED_F32.match(m) for m in ("v_fma_f32", "v_fmac_f32_e32", "v_pk_fma_f32", "v_fmac_f32_dpp", "v_fma_f32_e64_dpp", "v_fmac_f32_sdwa"))
    assert all(FUSED_F32.match(m) for m in ("v_fma_f32", "v_fmac_f32_e32", "v_pk_fma_f32", "v_fmac_f32_dpp", "v_fmac_f32_sdwa", "v_fmaak_f32"))
    assert all(LEGACY_F32.match(m) for m in ("v_mad_f32", "v_mac_f32_e32", "v_mad_legacy_f32", "v_mac_f32_dpp", "v_madmk_f32"))
    assert not any(FUSED_F32.match(m) or LEGACY_F32.match(m) for m in ("v_fma_f64", "v_mad_u64_u32", "v_mad_i64_i32", "v_mad_u32_u24", "v_div_fmas_f32"))


# ==== decks, inputs and the oracle's answers (shared by the CPU condition test and the GPU tests) ============================================

SMALL_W = ("subnormal",) * 8 + ("tiny", "pzero", "nzero", "nzero")      # SMALL with the subnormals weighted up (a tiny patch floods its neighbours)
MIXED = V.FINITE                                                                 # all finite classes side by side
REGIMES = {"small": dict(classes=SMALL_W), "mixed": dict(classes=MIXED, large_exp=40)}
V2_BIG = np.float32(1.0e8)          # (10 km/s)^2: v2 dt2 = 100


def _deck(nxe, nze, nxb, nzb, nt, compat, dx, dz, order=8, fac=0.75, seed=3):
    return make_deck(nxe, nze, nxb, nzb, nt, seed=seed, order=order, compat=compat, dx=dx, dz=dz, fac=fac)


def _patched_v2(d, seed, big=V2_BIG):
    """The deck's velocity with patches of v2 = 0 and (big) of a very large v2 next to normal ones (velocity is pointwise)."""
    xc, zc = V.deck_cuts(d, np.random.default_rng(seed), 3)
    m = _class_map(d, seed, 4, xc, zc)
    v2 = d["v2"].copy()
    v2[m == 2] = 0.0
    if big is not None:
        v2[m == 3] = big
    return v2


def _class_map(d, seed, n, xc, zc):
    """An int array [nxe][nze] of patches numbered 0 .. n-1 between the cuts."""
    return V.patched((d["nxe"], d["nze"]), seed, classes=("pzero",) * n, xcuts=xc, zcuts=zc, want_map=True)[1]


def _oracle(d, numerics=0):
    return O.Oracle(d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"], compat=d.get("compat", True),
                    numerics=numerics)


def _ctx(d, numerics=0, **kw):
    import parallel_finite_difference_computation_amd as F
    return F.FDWave(d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"], compat=d.get("compat", True),
                    numerics=numerics, **kw)


def _extents(d):
    return O.extents(d["nxe"], d["nze"], d["nzb"], d.get("compat", True))


def _need_subnormals(what, *fields):
    for i, f in enumerate(fields):
        assert V.share(f, "subnormal") >= MIN_SUBNORMAL_SHARE, f"{what}: output field {i} of the oracle holds too few subnormals: {V.shares(f)}"


def _need_one_subnormal(what, a):
    assert V.classify(a)["subnormal"] >= 1, f"{what}: no subnormal in the oracle's image / gather: {V.shares(a)}"


def _need_both_zeros(what, a):
    c = V.classify(a)
    assert c["nzero"] >= 1 and c["pzero"] >= 1, f"{what}: the time-stepped cells of the oracle's output lack a signed zero: {V.shares(a)}"


def _need_finite(what, *fields):
    for i, f in enumerate(fields):
        assert np.isfinite(f).all(), f"{what}: output field {i} of the oracle is not finite: {V.shares(f)}"


def _need_some_nonfinite(what, *fields):
    for i, f in enumerate(fields):
        s = V.share(f, "nan", "inf")
        assert 0.01 <= s <= 0.50, f"{what}: {s:.4f} of output field {i} of the oracle is non-finite (wanted 1 % .. 50 %): {V.shares(f)}"


def _need_plain(what, *fields):
    for i, f in enumerate(fields):
        c = V.classify(f)
        assert c["subnormal"] == c["nan"] == c["inf"] == 0, f"{what}: field {i} holds subnormal or non-finite values: {V.shares(f)}"


# ---- D.1 Laplacian ------------------------------------------------------------------------------------------------------------------------
LAP_SHAPE, LAP_DX, LAP_DZ = (48, 1300), 7.5, 12.5          # six 256-column strips
LAP_ORDERS = (2, 4, 8, 10, 16)
LAP_CLASSES = ("subnormal",) * 8 + MIXED          # every finite class, the subnormals weighted up: one large neighbour within order / 2 hides them


@functools.lru_cache(maxsize=None)
def _want_laplacian(order, numerics):
    nxe, nze = LAP_SHAPE
    d = dict(nxe=nxe, nze=nze, nxb=0, nzb=0, order=order, compat=False)
    xc, zc = V.deck_cuts(d, np.random.default_rng(order), 4)
    p = V.patched(LAP_SHAPE, 100 + order, classes=LAP_CLASSES, xcuts=xc, zcuts=zc)
    want = O.stencil(order, nxe, nze, LAP_DX, LAP_DZ, p, numerics=numerics)
    what = f"laplacian order {order} numerics {numerics}"
    _need_finite(what, want)
    _need_subnormals(what, want)
    if numerics:      # EXACT: both accumulators start from +0.0f and exact cancellation gives +0.0, so the reference's Laplacian is never -0.0
        _need_both_zeros(what, want)
    else:
        assert V.classify(want)["nzero"] == 0
    return p, want


# ---- D.2 forward loop -----------------------------------------------------------------------------------------------------------------------
# (nxe, nze, nxb, nzb, compat, dx, dz)
FWD_DECKS = {"99x83-compat": (99, 83, 17, 13, True, 25.0, 8.0),
             "150x1300-full": (150, 1300, 20, 24, False, 8.0, 12.5),           # six z strips
             "452x720-compat": (452, 720, 16, 16, True, 10.0, 12.5)}           # lean and full tiles of the wave pipeline
FWD_STEPS = (1, 4, 5, 13)
FWD_NT = 13


@functools.lru_cache(maxsize=None)
def _fwd_inputs(deck, regime):
    nxe, nze, nxb, nzb, compat, dx, dz = FWD_DECKS[deck]
    d = _deck(nxe, nze, nxb, nzb, FWD_NT, compat, dx, dz)
    inp = V.deck_inputs(d, seed=len(deck) * 7 + len(regime), **REGIMES[regime])
    # -0.0 / +0.0 pairs (the loop swaps first: its newer field is the `pp` argument): where pp is -0.0, p is +0.0, so that
    # 2 (-0) - (+0) = -0 meets the signed zero of v2 dt2 lap in the v2 = 0 patches
    inp["p"][inp["pp"].view(np.uint32) == 0x80000000] = 0.0
    # the small regime has no patch of (10 km/s)^2: beyond the stability limit every step multiplies the field, and thirteen of them lift
    # the subnormals out of their range; the mixed regime keeps it
    return d, _patched_v2(d, 50 + len(deck), big=None if regime == "small" else V2_BIG), inp


@functools.lru_cache(maxsize=None)
def _want_forward(deck, regime, nsteps, numerics):
    d, v2, inp = _fwd_inputs(deck, regime)
    oP, oPP = _oracle(d, numerics).forward(v2, d["sx"], d["sz"], inp["srce"], inp["p"], inp["pp"], nsteps=nsteps)
    what = f"forward {deck} {regime} {nsteps} steps numerics {numerics}"
    xlim, zlim, _ = _extents(d)
    if regime == "small":
        _need_subnormals(what, oP, oPP)
        if nsteps == 1:      # -0.0 does not outlive a second leap-frog (2 (-0) - (-0) = +0, and a sum never rounds to -0): a one-step condition
            _need_both_zeros(what, oPP[:xlim, :zlim])
    else:
        _need_finite(what, oP, oPP)
        _need_one_subnormal(what, oPP)
    return oP, oPP


# ---- D.3 backward loop and imaging ----------------------------------------------------------------------------------------------------------
BACK_DECK = (140, 610, 14, 18, True, 10.0, 12.5)
BACK_NT = 23
BACK_ITERS = (1, 3, 4, 7, BACK_NT)
# the snapshots and the start image come from the regime; the gather holds normal numbers, zeros and subnormals, so that in the small regime
# the imaging products (subnormal x normal) land in the subnormal range instead of all underflowing to zero
GATHER = {"small": dict(classes=("normal", "normal", "pzero", "nzero", "subnormal")), "mixed": dict(classes=MIXED, large_exp=10)}
BACK_REGIMES = {"small": REGIMES["small"], "mixed": dict(classes=MIXED, large_exp=20)}      # (fields x gather, summed over the iterations, stay finite)


@functools.lru_cache(maxsize=None)
def _back_inputs(regime):
    nxe, nze, nxb, nzb, compat, dx, dz = BACK_DECK
    d = _deck(nxe, nze, nxb, nzb, BACK_NT, compat, dx, dz, seed=17)
    inp = V.deck_inputs(d, seed=31 + len(regime), **BACK_REGIMES[regime])
    inp["d_obs"] = V.deck_inputs(d, seed=77, **GATHER[regime])["d_obs"]
    return d, _patched_v2(d, 61, big=None), inp


@functools.lru_cache(maxsize=None)
def _want_back(regime, n, numerics):
    d, v2, inp = _back_inputs(regime)
    want = _oracle(d, numerics).back(v2, inp["p"], inp["pp"], inp["d_obs"], d["gz"], imloc=inp["im0"], nsteps=n)
    what = f"backward {regime} {n} iterations numerics {numerics}"
    assert (want.view(np.uint32) != inp["im0"].view(np.uint32)).mean() > (0.05 if n >= 3 else 0.0), f"{what}: the image hardly changed"
    if regime == "small":
        _need_subnormals(what, want)
        _need_both_zeros(what, want)
    else:
        _need_finite(what, want)
        _need_one_subnormal(what, want)
    return want


# whole shots from rest: a wavelet whose samples run through every small class, times 2^k so that the expanding field lives in and around
# the subnormal range; gathers as above
SHOT_DECK = (59, 51, 9, 9, True, 10.0, 10.0)          # small, so that the field around the source is a tenth of the grid
SHOT_NT = 45
SHOT_K = -100


@functools.lru_cache(maxsize=None)
def _shot_inputs(regime):
    nxe, nze, nxb, nzb, compat, dx, dz = SHOT_DECK
    d = _deck(nxe, nze, nxb, nzb, SHOT_NT, compat, dx, dz, seed=7)
    nx = nxe - 2 * nxb
    ricker = (O.ricker_wavelet(SHOT_NT, d["dt"], 30.0) + 0.25).astype(np.float32)
    if regime == "small":
        srce = np.ldexp(ricker, SHOT_K).astype(np.float32)
        srce[5::7] = V.class_values("subnormal", len(srce[5::7]), np.random.default_rng(1))
        srce[6::7] = V.class_values("nzero", len(srce[6::7]), np.random.default_rng(1))
    else:
        srce = np.ldexp(ricker, 30).astype(np.float32)
    inp = V.deck_inputs(d, seed=41 + len(regime), **BACK_REGIMES[regime])
    gathers = np.stack([V.patched((nx, SHOT_NT), 90 + b, xcuts=(7, 8, 30, 31), zcuts=range(3, SHOT_NT, 3), **GATHER[regime]) for b in range(3)])
    v2_all = np.stack([_patched_v2(d, 70, big=None), d["v2"], (d["v2"] * np.float32(1.04)).astype(np.float32)])
    return d, v2_all, srce, gathers, inp["im0"]


@functools.lru_cache(maxsize=None)
def _want_shots(regime, numerics=0):
    """[(P, PP, image onto im0, image onto zero, gather recorded at gz)] for the three shots of the batch (source rows sx + 2 b)."""
    d, v2_all, srce, gathers, im0 = _shot_inputs(regime)
    orc, out = _oracle(d, numerics), []
    for b in range(3):
        P, PP = orc.forward(v2_all[b], d["sx"] + 2 * b, d["sz"], srce)
        img = orc.back(v2_all[b], P, PP, gathers[b], d["gz"], imloc=im0)
        img0 = orc.back(v2_all[b], P, PP, gathers[b], d["gz"])
        rec = np.zeros((d["nxe"] - 2 * d["nxb"], SHOT_NT), np.float32)
        for it in range(SHOT_NT):      # fdw_record_shot: data[ix][it] = d_pp(nxb + ix, gz) at the end of iteration it
            rec[:, it] = orc.forward(v2_all[b], d["sx"] + 2 * b, d["sz"], srce, nsteps=it + 1)[1][d["nxb"]:d["nxe"] - d["nxb"], d["gz"]]
        what = f"shot {b} {regime} numerics {numerics}"
        if regime == "small":
            _need_subnormals(what, P, PP)
            _need_one_subnormal(what, img)
            _need_one_subnormal(what, rec)
        else:
            _need_finite(what, P, PP, img, img0, rec)
        out.append((P, PP, img, img0, rec))
    return out


# ---- D.4 scaled whole shots -------------------------------------------------------------------------------------------------------------------
def _back_case_inputs(case):
    nxe, nze, nxb, nzb, nt, order, compat = case
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=7, order=order, compat=compat)
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    rng = np.random.default_rng(9)
    p, pp = random_fields(d, seed=11, amp=1e-3)      # amplitudes that keep fields x gather x 2^120, summed over nt iterations, below FLT_MAX
    return d, dict(p=p, pp=pp, srce=(1e-3 * (O.ricker_wavelet(nt, d["dt"], 30.0) + 0.25)).astype(np.float32),
                   d_obs=(0.1 * rng.standard_normal((nx, nt))).astype(np.float32), im0=rng.standard_normal((nx, nz)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _want_scaled(case, k):
    """BACK_CASES deck with every input times 2^k: forward from the (scaled) random fields, backward from the result onto the scaled image."""
    d, inp = _back_case_inputs(case)
    s = V.scaled(inp, k)
    orc = _oracle(d)
    oP, oPP = orc.forward(d["v2"], d["sx"], d["sz"], s["srce"], s["p"], s["pp"])
    oimg = orc.back(d["v2"], oP, oPP, s["d_obs"], d["gz"], imloc=s["im0"])
    what = f"scaled shot {case} k={k}"
    if k == -130:
        _need_subnormals(what, oP, oPP)
        _need_one_subnormal(what, oimg)
    elif k == 60:
        _need_finite(what, oP, oPP, oimg)
    else:
        _need_plain(what, oP, oPP, oimg)
    return s, oP, oPP, oimg


# ---- D.5 sibling dialects -----------------------------------------------------------------------------------------------------------------------
MOD_DECKS = {"61x47": (61, 47, 17, 13, 40, 10.0, 12.5, 0.02, (5, 1, 2)), "40x600": (40, 600, 5, 30, 20, 10.0, 10.0, 0.03, (20, 250, 255))}


def _mod_v2(nx, nz, nxb, nzb, seed):
    rng = np.random.default_rng(seed)
    vp = (1500 + 2500 * rng.random((nx, nz))).astype(np.float32)
    v2 = np.zeros((nx + 2 * nxb, nz + 2 * nzb), np.float32)
    v2[nxb:nxb + nx, nzb:nzb + nz] = vp * vp
    return O.mod_extendvel(v2, nx, nz, nxb, nzb)


def _small_wavelet(nt, k, seed):
    w = np.ldexp((O.mod_ricker_wavelet(nt, 0.001, 40.0) + 0.1 * np.random.default_rng(seed).standard_normal(nt)).astype(np.float32), k).astype(np.float32)
    w[5::7] = V.class_values("subnormal", len(w[5::7]), np.random.default_rng(seed))
    w[6::7] = V.class_values("nzero", len(w[6::7]), np.random.default_rng(seed))
    return w


@functools.lru_cache(maxsize=None)
def _want_model_shot(deck, regime, numerics=0):
    nx, nz, nxb, nzb, nt, dx, dz, fac, (sx0, sz0, gz0) = MOD_DECKS[deck]
    v2 = _mod_v2(nx, nz, nxb, nzb, nx)
    srce = _small_wavelet(nt, -118 if regime == "small" else 60, 3)
    want = O.mod_shot(8, nx, nz, nxb, nzb, dx, dz, 0.001, fac, v2, sx0 + nxb, sz0 + nzb, gz0 + nzb, srce, numerics=numerics)
    what = f"model shot {deck} {regime}"
    if regime == "small":
        _need_subnormals(what, want)
    else:
        _need_finite(what, want)
        assert V.share(want, "large") > 0.1, V.shares(want)
    return v2, srce, (sx0 + nxb, sz0 + nzb, gz0 + nzb), want


MSTEPS = dict(nx=420, nz=688, nxb=16, nzb=16, fac=0.02, dx=10.0, dz=12.5, sx=200, sz=452, gz=440)
MSTEPS_RUNS = ((8, 43), (9, 0))          # (steps, xchunk)


@functools.lru_cache(maxsize=None)
def _want_model_steps(regime, nsteps, numerics=0):
    m = MSTEPS
    nxe, nze = m["nx"] + 2 * m["nxb"], m["nz"] + 2 * m["nzb"]
    d = dict(nxe=nxe, nze=nze, nxb=m["nxb"], nzb=m["nzb"], order=8, compat=False, nt=nsteps)
    inp = V.deck_inputs(d, seed=5 + len(regime), **REGIMES[regime])
    v2 = ((1500 + 2500 * np.random.default_rng(77).random((nxe, nze))) ** 2).astype(np.float32)
    srce = inp["srce"]
    args = (8, m["nx"], m["nz"], m["nxb"], m["nzb"], m["dx"], m["dz"], 0.001, m["fac"], v2, m["sx"], m["sz"], m["gz"], srce)
    wP, wPP, wdata = O.mod_steps(*args, O.mod_taper_apply(inp["p"], m["nx"], m["nz"], m["nxb"], m["nzb"], m["fac"], 1),
                                 O.mod_taper_apply(inp["pp"], m["nx"], m["nz"], m["nxb"], m["nzb"], m["fac"], 2), numerics=numerics)
    what = f"model steps {regime} {nsteps}"
    if regime == "small":
        _need_subnormals(what, wP, wPP)
        _need_one_subnormal(what, wdata)
    else:
        _need_finite(what, wP, wPP, wdata)
    return inp["p"], inp["pp"], v2, srce, wP, wPP, wdata


STORED = (25, 21, 7, 7, 30, 10.0, 12.5, 0.02)          # small: the image of one shot lives around its source
STORED_K = -124


@functools.lru_cache(maxsize=None)
def _want_stored(regime, shot, numerics=0):
    nx, nz, nxb, nzb, nt, dx, dz, fac = STORED
    v2 = _mod_v2(nx, nz, nxb, nzb, 5)
    srce = _small_wavelet(nt, STORED_K if regime == "small" else 30, 4)
    dobs = np.stack([V.patched((nx, nt), 20 + b, xcuts=(7, 8, 16, 17), zcuts=range(3, nt, 3), **(GATHER[regime] if regime == "small" else dict(classes=MIXED, large_exp=30)))
                     for b in range(2)])
    sx, sz, gz = nxb + 8 + 6 * shot, nzb + 4, nzb + 2
    want = O.rtm_stored_shot(8, nx, nz, nxb, nzb, dx, dz, 0.001, fac, v2, sx, sz, gz, srce, dobs, shot=shot, numerics=numerics)
    what = f"stored-wavefield shot {shot} {regime}"
    if regime == "small":
        _need_subnormals(what, want)
    else:
        _need_finite(what, want)
        assert np.count_nonzero(want) > want.size // 10, V.shares(want)
    return v2, srce, dobs, (sx, sz, gz), want


@functools.lru_cache(maxsize=None)
def _want_image_laplacian():
    img = V.patched((37, 301), 2, classes=MIXED, xcuts=V.cuts(37, (1, 18, 36)), zcuts=V.cuts(301, (1, 4, 64, 150, 256, 300)))
    want = O.image_laplacian(img, 8.0, 12.5)
    _need_finite("image laplacian", want)
    _need_subnormals("image laplacian", want)
    return img, want


# ---- D.6 slabs -------------------------------------------------------------------------------------------------------------------------------
SLAB = dict(world=3, ksteps=3, shape=(152, 48), nb=8, nt=61, compat=True)
SLAB_K = -100


@functools.lru_cache(maxsize=None)
def _want_slabs(regime):
    nxe, nze = SLAB["shape"]
    d = _deck(nxe, nze, SLAB["nb"], SLAB["nb"], SLAB["nt"], SLAB["compat"], 10.0, 10.0, seed=3)
    nx, nz = nxe - 2 * SLAB["nb"], nze - 2 * SLAB["nb"]
    # class borders on and beside the slab seams (the owned bands are about nxe / 3 rows) and inside the ghost rows on either side of them
    seams = [nxe * r // 3 + o for r in (1, 2) for o in (-4 * SLAB["ksteps"], -4, 0, 4, 4 * SLAB["ksteps"])]
    xc, zc = V.cuts(nxe, seams + [d["nxb"], nxe - d["nxb"]]), V.deck_cuts(d)[1]
    m = V.patched((nxe, nze), 8, classes=("pzero",) * 4, xcuts=xc, zcuts=zc, want_map=True)[1]
    v2 = d["v2"].copy()
    v2[m == 2] = 0.0
    ricker = (O.ricker_wavelet(SLAB["nt"], d["dt"], 30.0) + 0.25).astype(np.float32)
    kw = GATHER[regime] if regime == "small" else dict(classes=MIXED, large_exp=30)
    srce = np.ldexp(ricker, SLAB_K if regime == "small" else 30).astype(np.float32)
    d_obs = V.patched((nx, SLAB["nt"]), 12, xcuts=[c - d["nxb"] for c in xc], zcuts=range(3, SLAB["nt"], 3), **kw)
    im0 = V.patched((nx, nz), 13, xcuts=[c - d["nxb"] for c in xc], zcuts=[c - d["nzb"] for c in zc], **BACK_REGIMES[regime])
    orc = _oracle(d)
    oP, oPP = orc.forward(v2, d["sx"], d["sz"], srce)
    oimg = orc.back(v2, oP, oPP, d_obs, d["gz"], imloc=im0)
    what = f"slabs {regime}"
    if regime == "small":
        _need_subnormals(what, oP, oPP, oimg)
    else:
        _need_finite(what, oP, oPP, oimg)
    return d, v2, srce, d_obs, im0, oP, oPP, oimg


# ---- D.7 non-finite data ------------------------------------------------------------------------------------------------------------------------
NONFINITE = ("normal",) * 14 + ("pzero", "overflowing")
NF_DECKS = {"99x83-compat": 2, "452x720-compat": 3}          # deck of FWD_DECKS -> steps


@functools.lru_cache(maxsize=None)
def _want_nonfinite_forward(deck):
    nxe, nze, nxb, nzb, compat, dx, dz = FWD_DECKS[deck]
    n = NF_DECKS[deck]
    d = _deck(nxe, nze, nxb, nzb, n, compat, dx, dz)
    inp = V.deck_inputs(d, seed=23, classes=NONFINITE, extra=0)
    with np.errstate(all="ignore"):
        oP, oPP = _oracle(d).forward(d["v2"], d["sx"], d["sz"], inp["srce"], inp["p"], inp["pp"], nsteps=n)
    what = f"non-finite forward {deck}"
    _need_some_nonfinite(what, oPP)
    assert V.classify(oPP)["nan"] > 0 and V.classify(oPP)["inf"] > 0, V.shares(oPP)
    # the containment the reference has: nothing outside the launch extents is ever written, whatever its neighbours hold
    xlim, zlim, _ = _extents(d)
    first, second = (inp["p"], inp["pp"]) if n % 2 == 0 else (inp["pp"], inp["p"])
    for name, out, src in (("P", oP, first), ("PP", oPP, second)):
        assert_bit_equal(out[xlim:], src[xlim:], f"{what}: rows >= xlim of {name}")
        assert_bit_equal(out[:, zlim:], src[:, zlim:], f"{what}: columns >= zlim of {name}")
        assert not np.isfinite(out[xlim - 5:xlim]).all() or not np.isfinite(out[:, zlim - 5:zlim]).all(), f"{what}: no non-finite value beside the extents"
    return d, inp, oP, oPP


@functools.lru_cache(maxsize=None)
def _want_nonfinite_back(n=3):
    nxe, nze, nxb, nzb, compat, dx, dz = BACK_DECK
    d = _deck(nxe, nze, nxb, nzb, BACK_NT, compat, dx, dz, seed=17)
    inp = V.deck_inputs(d, seed=29, classes=NONFINITE, extra=0)
    with np.errstate(all="ignore"):
        want = _oracle(d).back(d["v2"], inp["p"], inp["pp"], inp["d_obs"], d["gz"], imloc=inp["im0"], nsteps=n)
    _need_some_nonfinite("non-finite backward", want)
    return d, inp, want


def _all_wants():
    for order in LAP_ORDERS:
        for numerics in (0, 1):
            yield _want_laplacian, (order, numerics)
    for deck in FWD_DECKS:
        for regime in REGIMES:
            for n in FWD_STEPS:
                for numerics in (0, 1):
                    yield _want_forward, (deck, regime, n, numerics)
    for regime in REGIMES:
        for n in BACK_ITERS:
            yield _want_back, (regime, n, 0)
        yield _want_back, (regime, BACK_NT, 1)
        yield _want_shots, (regime,)
        for deck in MOD_DECKS:
            yield _want_model_shot, (deck, regime)
        for nsteps, _ in MSTEPS_RUNS:
            yield _want_model_steps, (regime, nsteps)
        for shot in (0, 1):
            yield _want_stored, (regime, shot)
        yield _want_slabs, (regime,)
    for case in BACK_CASES:
        for k in (-130, 60, -40, 40):
            yield _want_scaled, (case, k)
    yield _want_image_laplacian, ()
    for deck in NF_DECKS:
        yield _want_nonfinite_forward, (deck,)
    yield _want_nonfinite_back, ()


# ==== C. CPU ===================================================================================================================================

def test_inputs_carry_their_value_classes_to_the_oracle_output():
    """Every input set of section D, run through the oracle alone: each `_want_*` asserts its own condition (subnormal share, both zeros,
    finiteness, 1-50 % non-finite) on the oracle's output, so the GPU comparisons cannot pass vacuously."""
    n = 0
    for fn, args in _all_wants():
        fn(*args)
        n += 1
    assert n > 100


def test_value_class_helpers():
    rng = np.random.default_rng(0)
    sub = V.class_values("subnormal", 4000, rng)
    assert V.classify(sub)["subnormal"] == 4000 and {1, 0x80000001, 0x007FFFFF, 0x807FFFFF} <= set(sub.view(np.uint32).tolist())
    assert V.classify(V.class_values("tiny", 1000, rng))["tiny"] == 1000
    assert V.classify(V.class_values("nzero", 10, rng))["nzero"] == 10 and V.classify(V.class_values("pzero", 10, rng))["pzero"] == 10
    big = V.class_values("large", 1000, rng)
    assert V.classify(big)["large"] == 1000 and np.abs(big).max() < 2.0 ** 61 and np.abs(big).min() >= 2.0 ** 40
    ov = V.class_values("overflowing", 1000, rng)
    assert np.isfinite(ov).all() and np.abs(ov).min() >= 2.0 ** 100 and (np.abs(ov) == np.finfo(np.float32).max).any()
    d = make_deck(99, 300, 17, 13, 5, seed=1)
    xc, zc = V.deck_cuts(d)
    assert {3, 4, 5, 16, 17, 18, 95, 96, 97}.issubset(xc) and {7, 8, 9, 12, 13, 14, 63, 64, 65, 223, 224, 225, 239, 240, 241, 255, 256, 257, 295, 296, 297}.issubset(zc)
    inp = V.deck_inputs(d, 3)
    assert not inp["p"][96:, :8].any() and not inp["pp"][96:, :8].any()          # conftest.random_fields' precondition
    c = V.classify(inp["p"])
    assert all(c[k] > 0 for k in ("subnormal", "tiny", "pzero", "nzero", "normal", "large")) and c["nan"] == c["inf"] == 0
    s = V.scaled(inp, 3)
    assert_bit_equal(s["srce"], inp["srce"] * np.float32(8.0), "scaled wavelet")
    nan = np.array([1.0, np.nan, np.inf, -0.0], np.float32)
    V.assert_same_nonfinite(nan, np.array([1.0, -np.nan, np.inf, -0.0], np.float32))
    for other in ([1.0, np.nan, -np.inf, -0.0], [1.0, np.nan, np.inf, 0.0], [np.nan, np.nan, np.inf, -0.0], [1.0, 2.0, np.inf, -0.0]):
        with pytest.raises(AssertionError):
            V.assert_same_nonfinite(nan, np.array(other, np.float32))


@pytest.mark.parametrize("order", [2, 4, 8, 12])
def test_exact_chain_spelled_out(order):
    """The EXACT arithmetic stated with explicit np.float32 operations, independently of oracle/fdw_oracle.c, on a grid filled from all
    finite classes with dx != dz.  kernel_lap: two accumulators from 0.0f, the taps in `io` order, one product and one add per tap and
    axis, acmz + acmx last; kernel_time: (v2 * dt2) * lap in fp32, 2. * p - pp + that in double, one rounding at the store -- v2 = 0 cells
    and a very large v2 included.  O.stencil and one step of the oracle's forward loop equal it bit for bit."""
    f32, h = np.float32, order // 2
    nxe, nze, dx, dz = 37, 45, 7.5, 12.5
    xc, zc = V.cuts(nxe, (h, 18, nxe - h)), V.cuts(nze, (h, 4, 22, nze - h))
    p = V.patched((nxe, nze), order, classes=MIXED, xcuts=xc, zcuts=zc)

    def lap_of(field, cx, cz):
        acmz, acmx = np.zeros((nxe - 2 * h, nze - 2 * h), f32), np.zeros((nxe - 2 * h, nze - 2 * h), f32)
        for io in range(order + 1):
            a = io - h
            acmz = (acmz + (field[h:nxe - h, h + a:nze - h + a] * f32(cz[io])).astype(f32)).astype(f32)
            acmx = (acmx + (field[h + a:nxe - h + a, h:nze - h] * f32(cx[io])).astype(f32)).astype(f32)
        out = np.zeros((nxe, nze), f32)
        out[h:nxe - h, h:nze - h] = (acmz + acmx).astype(f32)
        return out

    cx, cz = O.scaled_coefs(order, dx, dz, cxx=True)
    want = lap_of(p, cx, cz)
    assert V.classify(want)["subnormal"] > 0 and np.isfinite(want).all(), V.shares(want)
    assert_bit_equal(O.stencil(order, nxe, nze, dx, dz, p), want, f"orc_stencil vs the spelled-out chain, order {order}")

    # one leap-frog step: full extents, fac = 1 (the taper is the identity), source sample +0.0 added at (sx, sz)
    d = make_deck(nxe, nze, 3, 3, 1, seed=order, order=order, compat=False, fac=1.0, dx=dx, dz=dz)
    assert all(t == 1.0 for t in np.concatenate(O.taper_tables(3, 3, 1.0)))
    older = V.patched((nxe, nze), order + 50, classes=MIXED, xcuts=xc, zcuts=zc)
    m = V.patched((nxe, nze), order + 60, classes=("pzero",) * 4, xcuts=xc, zcuts=zc, want_map=True)[1]
    v2 = d["v2"].copy()
    v2[m == 2], v2[m == 3] = 0.0, V2_BIG
    p[10:18, 12:20], older[10:18, 12:20], v2[10:18, 12:20] = -0.0, 0.0, 0.0      # 2 (-0) - (+0) + 0 * lap: -0.0 where lap < 0 (the block's rim)
    cx, cz = O.scaled_coefs(order, dx, dz)
    lap = lap_of(p, cx, cz)
    dt2 = f32(f32(d["dt"]) * f32(d["dt"]))
    term = ((v2 * dt2).astype(f32) * lap).astype(f32)
    new = (2.0 * p.astype(np.float64) - older.astype(np.float64) + term.astype(np.float64)).astype(f32)
    new[d["sx"], d["sz"]] = f32(new[d["sx"], d["sz"]] + f32(0.0))
    assert np.isfinite(new).all() and V.classify(new)["nzero"] > 0 and V.classify(new)["subnormal"] > 0, V.shares(new)
    # the oracle's loop swaps first: its d_p is the `pp` argument, its d_pp the `p` argument
    oP, oPP = _oracle(d).forward(v2, d["sx"], d["sz"], np.zeros(1, f32), older, p, nsteps=1)
    assert_bit_equal(oPP, new, f"one oracle step vs the spelled-out leap-frog, order {order}")
    assert_bit_equal(oP, p, "the newer field is handed on unchanged")


@pytest.mark.parametrize("k", [-130, 60])
@pytest.mark.parametrize("case", ZV_DECKS, ids=ZV_IDS)
def test_zero_velocity_restatement_on_scaled_fields(case, k):
    """tests/test_backward_pins.py's zero-velocity statements with fields, wavelet, gather and start image times 2^-130 (everything subnormal)
    and 2^60: oracle == restatement bit for bit.  The restatement drops the v2 dt2 lap term at zero velocity ("a signed zero adds nothing"),
    which is false where 2p - pp is -0.0; so -0.0 is kept out of the fields given to it (the few values that underflow to -0.0 when
    scaled are replaced by +0.0 below) -- the signed zeros are the business of test_exact_chain_spelled_out and of the GPU tests."""
    nxe, nze, nxb, nzb, nt, order, compat, fac, dx, dz = case
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=21, order=order, compat=compat, fac=fac, dx=dx, dz=dz)
    rng = np.random.default_rng(3)
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    amp = 1.0 if k < 0 else 1e-3      # (up: amplitudes that keep fields x gather x 2^120, summed over nt iterations, below FLT_MAX)
    p0, pp0 = random_fields(d, 4, amp=amp)
    s0, s1 = random_fields(d, 5, amp=amp)
    inp = V.scaled(dict(p=p0, pp=pp0, srce=(amp * (O.ricker_wavelet(nt, d["dt"], 30.0) + 0.25)).astype(np.float32),
                        d_obs=(rng.standard_normal((nx, nt)) * (1.0 if k < 0 else 0.1)).astype(np.float32),
                        im0=rng.standard_normal((nx, nz)).astype(np.float32)), k)
    s0, s1 = np.ldexp(s0, k).astype(np.float32), np.ldexp(s1, k).astype(np.float32)
    for a in (*inp.values(), s0, s1):
        a[a == 0] = 0.0                                  # a value that underflowed to -0.0 becomes +0.0
        assert V.classify(a)["nzero"] == 0
    z = np.zeros((nxe, nze), np.float32)
    orc, sx, gz = _oracle(d), d["sx"], d["gz"]
    P, PP = R.forward_zero_velocity(d, sx, gz, inp["srce"], inp["p"], inp["pp"], nsteps=nt - 3)
    oP, oPP = orc.forward(z, sx, gz, inp["srce"], inp["p"], inp["pp"], nsteps=nt - 3)
    if k < 0:
        _need_subnormals("zero-velocity forward", oP, oPP)
    else:
        _need_finite("zero-velocity forward", oP, oPP)
        assert V.share(oPP, "large") > 0.5
    assert_bit_equal(oP, P, "forward P")
    assert_bit_equal(oPP, PP, "forward PP")
    for n in (nt, nt - 1, nt - 2, nt - 3, 1, 2, 3):
        want = R.back_zero_velocity(d, s0, s1, inp["d_obs"], gz, imloc=inp["im0"], nsteps=n)
        assert_bit_equal(orc.back(z, s0, s1, inp["d_obs"], gz, imloc=inp["im0"], nsteps=n), want, f"back from scaled snapshots, {n} iterations")
        if k < 0:
            _need_subnormals("zero-velocity image", want)
        else:
            _need_finite("zero-velocity image", want)
            assert np.any(want != inp["im0"])


@pytest.mark.parametrize("k", [-40, 40])
def test_oracle_is_homogeneous_under_powers_of_two(k):
    """The loop is homogeneous of degree one in (p, pp, srce), the image of degree two in (fields x gather) and of degree one in the start
    image; scaling by 2^k is exact while nothing under- or overflows.  On normal-class decks: oracle(2^k inputs) == 2^k oracle(inputs) bit for
    bit -- forward fields, the gather of the modelling loop, and the image (fields and gather times 2^k, start image times 2^2k).  The proof
    that the scaled inputs of the GPU tests are sound."""
    for case in BACK_CASES[1:4]:
        d, inp = _back_case_inputs(case)
        s = V.scaled(inp, k)
        orc = _oracle(d)
        P, PP = orc.forward(d["v2"], d["sx"], d["sz"], inp["srce"], inp["p"], inp["pp"])
        sP, sPP = orc.forward(d["v2"], d["sx"], d["sz"], s["srce"], s["p"], s["pp"])
        im2 = np.ldexp(inp["im0"], 2 * k).astype(np.float32)
        img = orc.back(d["v2"], P, PP, inp["d_obs"], d["gz"], imloc=inp["im0"])
        simg = orc.back(d["v2"], sP, sPP, s["d_obs"], d["gz"], imloc=im2)
        _need_plain(f"homogeneity {case} k={k}", P, PP, img, sP, sPP, simg)
        assert_bit_equal(sP, np.ldexp(P, k), f"P {case}")
        assert_bit_equal(sPP, np.ldexp(PP, k), f"PP {case}")
        assert_bit_equal(simg, np.ldexp(img, 2 * k), f"image {case}")
    m = MSTEPS
    nx, nz, nxb, nzb = 61, 47, 17, 13
    rng = np.random.default_rng(4)
    v2 = _mod_v2(nx, nz, nxb, nzb, 9)
    P0, PP0 = rng.standard_normal((2, nx + 2 * nxb, nz + 2 * nzb)).astype(np.float32)
    srce = rng.standard_normal(12).astype(np.float32)
    args = (8, nx, nz, nxb, nzb, m["dx"], m["dz"], 0.001, m["fac"], v2, nxb + 5, nzb + 1, nzb + 2)
    a = O.mod_steps(*args, srce, P0, PP0)
    b = O.mod_steps(*args, np.ldexp(srce, k), np.ldexp(P0, k), np.ldexp(PP0, k))
    _need_plain(f"modelling homogeneity k={k}", *a, *b)
    for name, x, y in zip(("P", "PP", "gather"), a, b):
        assert_bit_equal(y, np.ldexp(x, k), f"modelling loop {name}")


def test_the_comparisons_reject_flushing_plus_zero_and_mask_multiplies():
    """Without touching the kernels: the three errors this file is about, applied to the ORACLE's own results, are each rejected by the
    comparison the GPU tests use -- so the chosen inputs carry each class to the output, and a kernel that made the error would fail.
      * flush-to-zero of subnormals, on the outputs and on the inputs (a kernel in denormal mode 0 does both);
      * x + 0.0f on every cell (what an unconditional add of a zero does to -0.0);
      * a 0/1-mask multiply instead of a select on the cells outside the launch extents of a non-finite field."""
    for deck in FWD_DECKS:
        for n in (1, 13):
            d, v2, inp = _fwd_inputs(deck, "small")
            oP, oPP = _want_forward(deck, "small", n, 0)
            with pytest.raises(AssertionError):
                assert_bit_equal(V.flush_subnormals(oPP), oPP, "flushed output")
            if n == 1:      # the signed-zero cases are the one-step runs (_want_forward)
                xlim, zlim, _ = _extents(d)
                with pytest.raises(AssertionError):
                    assert_bit_equal(V.add_plus_zero(oPP)[:xlim, :zlim], oPP[:xlim, :zlim], "x + 0.0f")
            fP, fPP = _oracle(d).forward(v2, d["sx"], d["sz"], V.flush_subnormals(inp["srce"]), V.flush_subnormals(inp["p"]), V.flush_subnormals(inp["pp"]), nsteps=n)
            with pytest.raises(AssertionError):
                assert_bit_equal(fPP, oPP, "flushed inputs")
    for regime in REGIMES:
        want = _want_back(regime, BACK_NT, 0)
        for bad in (V.flush_subnormals(want), V.add_plus_zero(want)):
            with pytest.raises(AssertionError):
                assert_bit_equal(bad, want, "image")
    for numerics, mutations in ((0, (V.flush_subnormals,)), (1, (V.flush_subnormals, V.add_plus_zero))):
        _, lap = _want_laplacian(8, numerics)
        for mutate in mutations:
            with pytest.raises(AssertionError):
                assert_bit_equal(mutate(lap), lap, "laplacian")
    for deck in NF_DECKS:
        d, inp, oP, oPP = _want_nonfinite_forward(deck)
        xlim, zlim, _ = _extents(d)
        mask = np.zeros(oPP.shape, bool)
        mask[:xlim, :zlim] = True
        with np.errstate(all="ignore"):
            upd = np.where(mask, oPP, np.float32(np.inf))            # what an unmasked lane computed from inf / NaN neighbours
        bad = V.mask_multiply(upd, oPP, mask)
        with pytest.raises(AssertionError):
            V.assert_same_nonfinite(bad, oPP, "mask multiply")
        V.assert_same_nonfinite(np.where(mask, upd, oPP), oPP, "select")


# ==== D. GPU ===================================================================================================================================

@gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("order", LAP_ORDERS)
def test_gpu_laplacian_on_value_classes(order, numerics):
    """fdw_laplacian, the register-ring kernels and the generic-order kernel, EXACT and FAST (against the oracle's FAST restatement), on a grid
    of six z strips filled from all finite classes."""
    import parallel_finite_difference_computation_amd as F
    p, want = _want_laplacian(order, numerics)
    ctx = F.FDWave(order, *LAP_SHAPE, dx=LAP_DX, dz=LAP_DZ, coef_cxx=True, numerics=numerics)
    assert_bit_equal(ctx.laplacian(p), want, f"laplacian order {order} numerics {numerics}")
    ctx.set_tuning(xchunk=13, wz=2)
    assert_bit_equal(ctx.laplacian(p), want, f"laplacian order {order} numerics {numerics}, xchunk 13 wz 2")
    ctx.set_tuning(use_generic=True)
    assert_bit_equal(ctx.laplacian(p), want, f"generic-order laplacian order {order} numerics {numerics}")


@gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("deck", list(FWD_DECKS))
def test_gpu_forward_loop_on_value_classes(deck, regime, numerics):
    """fdw_forward through the one-step, two-step and wave-pipeline kernels, two chunk lengths each, from class-patched p / pp with a
    class-patched wavelet and a velocity model with patches of v2 = 0 and of (10 km/s)^2: compat and full extents, dx != dz, 1, 4, 5 and 13
    steps; P and PP equal the oracle's (EXACT) or its FAST restatement's bit for bit."""
    d, v2, inp = _fwd_inputs(deck, regime)
    ctx = _ctx(d, numerics)
    for n in FWD_STEPS:
        oP, oPP = _want_forward(deck, regime, n, numerics)
        for mode in (-1, 1, 4):
            for xchunk in (0, 13):
                ctx.set_tuning(two_step=mode, xchunk=xchunk)
                P, PP = ctx.forward(v2, d["sx"], d["sz"], inp["srce"], inp["p"], inp["pp"], nsteps=n)
                what = f"{deck} {regime} numerics={numerics} two_step={mode} xchunk={xchunk} steps={n}"
                assert_bit_equal(PP, oPP, what + ": PP")
                assert_bit_equal(P, oP, what + ": P")
    ctx.set_tuning(use_generic=True)
    P, PP = ctx.forward(v2, d["sx"], d["sz"], inp["srce"], inp["p"], inp["pp"], nsteps=5)
    oP, oPP = _want_forward(deck, regime, 5, numerics)
    assert_bit_equal(PP, oPP, f"{deck} {regime} numerics={numerics} generic-order kernel: PP")
    assert_bit_equal(P, oP, f"{deck} {regime} numerics={numerics} generic-order kernel: P")


@gpu
@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_backward_loop_on_value_classes(regime, monkeypatch):
    """fdw_back from class-patched snapshots, gather and start image through the fused one-step iteration, the two-launch form, the paired
    iterations, the eight-wave pipeline and its two-pass form, for 1, 3, 4, 7 and nt iterations; FAST numerics for nt iterations."""
    d, v2, inp = _back_inputs(regime)
    for k in ("FDW_NO_FUSED_BACK", "FDW_NO_BACK_FUSED"):
        monkeypatch.delenv(k, raising=False)
    fused = _ctx(d)
    monkeypatch.setenv("FDW_NO_FUSED_BACK", "1")
    split = _ctx(d)
    monkeypatch.delenv("FDW_NO_FUSED_BACK")
    monkeypatch.setenv("FDW_NO_BACK_FUSED", "1")
    two_pass = _ctx(d)
    monkeypatch.delenv("FDW_NO_BACK_FUSED")
    for n in BACK_ITERS:
        want = _want_back(regime, n, 0)
        for name, c, mode, xchunk in (("fused one-step", fused, -1, 0), ("two launches", split, -1, 0), ("paired", fused, 1, 0), ("eight-wave pipeline", fused, 4, 0),
                                      ("eight-wave pipeline, xchunk 13", fused, 4, 13), ("two-pass pipeline", two_pass, 4, 0)):
            c.set_tuning(two_step=mode, xchunk=xchunk)
            got = c.back(v2, inp["p"], inp["pp"], inp["d_obs"], d["gz"], imloc=inp["im0"], nsteps=n)
            assert_bit_equal(got, want, f"{regime}: image, {name}, {n} iterations")
    want = _want_back(regime, BACK_NT, 1)
    fast = _ctx(d, 1)
    for mode in (-1, 1, 4):
        fast.set_tuning(two_step=mode)
        assert_bit_equal(fast.back(v2, inp["p"], inp["pp"], inp["d_obs"], d["gz"], imloc=inp["im0"]), want, f"{regime}: FAST image, two_step={mode}")


@gpu
@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_whole_shots_on_value_classes(regime):
    """fdw_shot, fdw_shot_batch (3 shots) and fdw_record_shot from rest: a wavelet scaled into (and holding samples of) the subnormal range,
    or by 2^40; class-patched gathers and start image; a velocity model with v2 = 0 patches for the first shot."""
    d, v2_all, srce, gathers, im0 = _shot_inputs(regime)
    want = _want_shots(regime)
    ctx = _ctx(d)
    for mode in (-1, 1, 4):
        ctx.set_tuning(two_step=mode)
        for b in range(3):
            oP, oPP, oimg, _, orec = want[b]
            img, P, PP = ctx.shot(v2_all[b], d["sx"] + 2 * b, d["sz"], d["gz"], srce, gathers[b], imloc=im0, want_fields=True)
            assert_bit_equal(PP, oPP, f"{regime} shot {b} two_step={mode}: PP")
            assert_bit_equal(P, oP, f"{regime} shot {b} two_step={mode}: P")
            assert_bit_equal(img, oimg, f"{regime} shot {b} two_step={mode}: image")
            rec, P, PP = ctx.record_shot(v2_all[b], d["sx"] + 2 * b, d["sz"], d["gz"], srce, want_fields=True)
            assert_bit_equal(rec, orec, f"{regime} recorded gather {b} two_step={mode}")
            assert_bit_equal(PP, oPP, f"{regime} record_shot {b} two_step={mode}: PP")
    ctx.set_tuning(two_step=0)
    got = ctx.shot_batch(3, d["sx"], 2, d["sz"], d["gz"], srce, gathers, v2_all=v2_all)
    for b in range(3):
        assert_bit_equal(got[b], want[b][3], f"{regime} batched shot {b}")


@gpu
@pytest.mark.parametrize("case", BACK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_gpu_scaled_whole_decks(case):
    """The decks of test_gpu_parity.BACK_CASES with every input times 2^-130 (everything subnormal) and 2^60 against the oracle, and times
    2^-40 / 2^40 against the oracle AND against 2^k times the kernels' own unscaled result."""
    d, inp = _back_case_inputs(case)
    ctx = _ctx(d)
    modes = (-1, 1, 4) if d["order"] == 8 else (-1,)
    base = {}
    for k in (0, -130, 60, -40, 40):
        for mode in modes:
            ctx.set_tuning(two_step=mode)
            if k == 0:
                P, PP = ctx.forward(d["v2"], d["sx"], d["sz"], inp["srce"], inp["p"], inp["pp"])
                base[mode] = (P, PP, ctx.back(d["v2"], P, PP, inp["d_obs"], d["gz"], imloc=inp["im0"]))
                continue
            s, oP, oPP, oimg = _want_scaled(case, k)
            P, PP = ctx.forward(d["v2"], d["sx"], d["sz"], s["srce"], s["p"], s["pp"])
            img = ctx.back(d["v2"], oP, oPP, s["d_obs"], d["gz"], imloc=s["im0"])
            what = f"{case} k={k} two_step={mode}"
            assert_bit_equal(PP, oPP, what + ": PP")
            assert_bit_equal(P, oP, what + ": P")
            assert_bit_equal(img, oimg, what + ": image")
            if abs(k) == 40:
                assert_bit_equal(P, np.ldexp(base[mode][0], k), what + ": P vs 2^k x the unscaled run")
                assert_bit_equal(PP, np.ldexp(base[mode][1], k), what + ": PP vs 2^k x the unscaled run")
                im2 = ctx.back(d["v2"], P, PP, s["d_obs"], d["gz"], imloc=np.ldexp(inp["im0"], 2 * k).astype(np.float32))
                assert_bit_equal(im2, np.ldexp(base[mode][2], 2 * k), what + ": image vs 2^2k x the unscaled run")


@gpu
@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_modelling_dialect_on_value_classes(regime):
    """fdw_model_shot (Gaussian source from rest, one-step kernel and wave pipeline) and fdw_dev_model_steps from class-patched fields
    (fields and gather) against O.mod_shot / O.mod_steps."""
    import torch

    import parallel_finite_difference_computation_amd as F
    for deck in MOD_DECKS:
        nx, nz, nxb, nzb, nt, dx, dz, fac, _ = MOD_DECKS[deck]
        v2, srce, (sx, sz, gz), want = _want_model_shot(deck, regime)
        ctx = F.FDWave(8, nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt, fac, dx, dz, 0.001, dialect=1)
        for mode, xchunk in ((-1, 0), (4, 0), (4, 7)):
            ctx.set_tuning(two_step=mode, xchunk=xchunk)
            assert_bit_equal(ctx.model_shot(v2, sx, sz, gz, srce), want, f"{regime} model shot {deck} two_step={mode} xchunk={xchunk}")
    m = MSTEPS
    nx, nz, nxb, nzb, fac = m["nx"], m["nz"], m["nxb"], m["nzb"], m["fac"]
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    dev = torch.device("cuda:0")
    for nsteps, xchunk in MSTEPS_RUNS:
        P0, PP0, v2, srce, wP, wPP, wdata = _want_model_steps(regime, nsteps)
        ctx = F.FDWave(8, nxe, nze, nxb, nzb, nsteps, fac, m["dx"], m["dz"], 0.001, dialect=1)
        ctx.set_tuning(two_step=4, xchunk=xchunk)
        assert ctx.steps_per_pass() == 4

        def up(a):
            t = torch.zeros((nxe, ctx.pitch), device=dev)
            t[:, :nze] = torch.from_numpy(a).to(dev)
            return t
        p, pp, dv2, dsr = up(P0), up(PP0), up(v2), torch.from_numpy(srce).to(dev)
        assert_bit_equal(p[:, :nze].cpu().numpy(), P0, "the upload keeps every bit")
        rec = torch.zeros((nsteps, nx), device=dev)
        torch.cuda.synchronize()
        ctx.dev_model_steps(p.data_ptr(), pp.data_ptr(), dv2.data_ptr(), dsr.data_ptr(), m["sx"], m["sz"], m["gz"], rec.data_ptr(), 0, nsteps)
        torch.cuda.synchronize()
        assert_bit_equal(rec.cpu().numpy().T, wdata, f"{regime} gather nsteps={nsteps}")
        gP, gPP = (p, pp) if nsteps % 2 == 0 else (pp, p)
        assert_bit_equal(O.mod_taper_apply(gP[:, :nze].cpu().numpy(), nx, nz, nxb, nzb, fac, 1), wP, f"{regime} P nsteps={nsteps}")
        assert_bit_equal(O.mod_taper_apply(gPP[:, :nze].cpu().numpy(), nx, nz, nxb, nzb, fac, 2), wPP, f"{regime} PP nsteps={nsteps}")


@gpu
@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_stored_wavefield_rtm_and_image_filter_on_value_classes(regime, monkeypatch):
    """fdw_rtm_stored_shot with every field kept and with checkpointing (fdw_set_store_budget, forced segment lengths) against
    O.rtm_stored_shot; fdw_image_laplacian on a class-patched image."""
    import parallel_finite_difference_computation_amd as F
    nx, nz, nxb, nzb, nt, dx, dz, fac = STORED
    ctx = F.FDWave(8, nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt, fac, dx, dz, 0.001, dialect=2)
    least = min(2 * -(-nt // s) + s + 1 for s in range(1, nt + 1))
    for shot in (0, 1):
        v2, srce, dobs, (sx, sz, gz), want = _want_stored(regime, shot)
        for budget_fields, forced in ((0, None), (least + 2, None), (0, 7), (0, 1)):
            ctx.set_store_budget(budget_fields * ctx.field_bytes())
            if forced:
                monkeypatch.setenv("FDW_STORE_SEGMENT", str(forced))
            else:
                monkeypatch.delenv("FDW_STORE_SEGMENT", raising=False)
            got = ctx.rtm_stored_shot(v2, sx, sz, gz, srce, dobs, shot=shot)
            assert_bit_equal(got, want, f"{regime} stored-wavefield image of shot {shot}, budget {budget_fields} fields, forced segment {forced}")
            assert (ctx.store_segments() == 1) == (budget_fields == 0 and forced is None)
        monkeypatch.delenv("FDW_STORE_SEGMENT", raising=False)
    img, want = _want_image_laplacian()
    assert_bit_equal(F.image_laplacian(img, 8.0, 12.5), want, "image Laplacian of a class-patched image")


@gpu
@pytest.mark.parametrize("regime", list(REGIMES))
def test_gpu_slab_driver_on_value_classes(regime, monkeypatch):
    """Three ranks as host threads on one GPU through the C slab driver (forward loop, hand-over, backward loop with imaging, every halo
    exchange): class borders of the velocity model (v2 = 0 patches), the gather and the start image on the slab seams and in the ghost rows;
    P, PP and the image gathered from the ranks' owned rows equal the ORACLE's bit for bit."""
    import parallel_finite_difference_computation_amd as F
    d, v2, srce, d_obs, im0, oP, oPP, oimg = _want_slabs(regime)
    nxe, nze = SLAB["shape"]
    monkeypatch.setenv("FDW_SLAB_PIPE", "0")
    comms = F.Comm.local(SLAB["world"])

    def rank(r):
        s = F.Slabs(d["order"], nxe, nze, d["nxb"], d["nzb"], SLAB["nt"], d["fac"], d["dx"], d["dz"], d["dt"], comm=comms[r], compat=SLAB["compat"], ksteps=SLAB["ksteps"])
        out = s.shot(v2, d["sx"], d["sz"], d["gz"], srce, d_obs, imloc=im0, want_fields=True)
        geo = (s.own0, s.own1, s.owned_interior_rows())
        s.close()
        return out, geo

    res = F.run_ranks(rank, SLAB["world"])
    img, gP, gPP, rows = np.array(im0), np.zeros_like(oP), np.zeros_like(oPP), 0
    for (im, p, pp), (o0, o1, (a, b)) in res:
        img[a:b] = im[a:b]
        gP[o0:o1], gPP[o0:o1] = p[o0:o1], pp[o0:o1]
        rows += o1 - o0
    for c in comms:
        c.close()
    assert rows == nxe
    assert_bit_equal(gPP, oPP, f"{regime}: PP gathered from the ranks")
    assert_bit_equal(gP, oP, f"{regime}: P gathered from the ranks")
    assert_bit_equal(img, oimg, f"{regime}: image gathered from the ranks")


@gpu
@pytest.mark.parametrize("deck", list(NF_DECKS))
def test_gpu_nonfinite_forward_and_containment(deck):
    """Fields with patches of values up to FLT_MAX: sums reach +-inf and inf - inf.  One-step, two-step and pipeline kernels against the
    oracle -- NaNs by position only (their sign and payload legitimately differ between x86 and the GPU), infinities and every finite cell
    bit for bit.  The oracle's output already holds the reference's containment (rows >= xlim and columns >= zlim bit-identical to the
    input, asserted in _want_nonfinite_forward), so equality with it is containment on the host arrays; on device arrays the pad columns
    [nze, pitch) stay +0.0 bit for bit.  Ordinary arithmetic on unusual numbers: nothing here can fault."""
    import torch
    d, inp, oP, oPP = _want_nonfinite_forward(deck)
    n = NF_DECKS[deck]
    nxe, nze = d["nxe"], d["nze"]
    xlim, zlim, _ = _extents(d)
    ctx = _ctx(d)
    first, second = (inp["p"], inp["pp"]) if n % 2 == 0 else (inp["pp"], inp["p"])
    for mode in (-1, 1, 4):
        for xchunk in (0, 13):
            ctx.set_tuning(two_step=mode, xchunk=xchunk)
            P, PP = ctx.forward(d["v2"], d["sx"], d["sz"], inp["srce"], inp["p"], inp["pp"], nsteps=n)
            what = f"non-finite {deck} two_step={mode} xchunk={xchunk}"
            V.assert_same_nonfinite(PP, oPP, what + ": PP")
            V.assert_same_nonfinite(P, oP, what + ": P")
            for name, out, src in (("P", P, first), ("PP", PP, second)):      # untouched cells: bit-identical, NaN-free by construction
                assert_bit_equal(out[xlim:], src[xlim:], what + f": rows >= xlim of {name}")
                assert_bit_equal(out[:, zlim:], src[:, zlim:], what + f": columns >= zlim of {name}")
    dev = torch.device("cuda:0")
    for mode in (-1, 1, 4):
        ctx.set_tuning(two_step=mode)
        bufs = [torch.zeros((nxe, ctx.pitch), device=dev) for _ in range(4)]
        bufs[0][:, :nze] = torch.from_numpy(inp["p"]).to(dev)
        bufs[1][:, :nze] = torch.from_numpy(inp["pp"]).to(dev)
        dv2 = torch.zeros((nxe, ctx.pitch), device=dev)
        dv2[:, :nze] = torch.from_numpy(d["v2"]).to(dev)
        dsr = torch.from_numpy(inp["srce"]).to(dev)
        torch.cuda.synchronize()
        ip, ipp = ctx.dev_steps2([b.data_ptr() for b in bufs], dv2.data_ptr(), dsr.data_ptr(), d["sx"], d["sz"], 0, n, False, 0, 1)
        ctx.dev_taper_finalize(bufs[ip].data_ptr())
        torch.cuda.synchronize()
        V.assert_same_nonfinite(bufs[ipp][:, :nze].cpu().numpy(), oPP, f"non-finite {deck} device arrays two_step={mode}: PP")
        V.assert_same_nonfinite(bufs[ip][:, :nze].cpu().numpy(), oP, f"non-finite {deck} device arrays two_step={mode}: P")
        if ctx.pitch > nze:
            for i, b in enumerate(bufs):
                pad = b[:, nze:].cpu().numpy()
                assert_bit_equal(pad, np.zeros_like(pad), f"non-finite {deck} two_step={mode}: pad columns of buffer {i}")


@gpu
def test_gpu_nonfinite_backward():
    """fdw_back on overflowing snapshots, gather and start image through the fused one-step iteration and the eight-wave pipeline."""
    d, inp, want = _want_nonfinite_back()
    ctx = _ctx(d)
    for mode in (-1, 1, 4):
        ctx.set_tuning(two_step=mode)
        got = ctx.back(d["v2"], inp["p"], inp["pp"], inp["d_obs"], d["gz"], imloc=inp["im0"], nsteps=3)
        V.assert_same_nonfinite(got, want, f"non-finite backward two_step={mode}")

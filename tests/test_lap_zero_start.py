"""The exact four-step Laplacian (laplacian_quad, csrc/fdw_device.h) starts its z chains from term 0 instead of 0 + term 0; its x chains keep
the leading zero.  The reference's form has the zero in both.  The two agree bit for bit because the zero only turns -0 into +0, and the half
that keeps it is then never -0, so the final add az + ax cannot see the sign of a zero az.

CPU part (no GPU): one cell's two nine-term chains and their final add restated in numpy float32, in three forms -- both chains from zero
(the reference), the z chain without (what is built), both without (wrong) -- over the value classes of tests/value_classes.py and over EVERY
sign pattern of zero on the 18 terms.  Forms one and two must agree everywhere; form three must differ on the all-(-0) input, which shows
that the comparison can see the effect.

GPU part: the four-step kernel forced on 1024 x 1024 at 61-row chunks (17 chunk rows x 5 strips: lean tiles, the damped strip, the frame and
the two tiles around the source all occur, asserted below), eight steps = two passes, from three starts built around signed zeros, against the
CPU oracle bit for bit.  "p" below is the field the first step takes the Laplacian of (the `pp` argument of forward(), which swaps first)."""
import ctypes as C

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from conftest import assert_bit_equal, bits, make_deck, random_fields
from oracle import oracle as O
from parallel_finite_difference_computation_amd import _lib
from value_classes import CLASSES, class_values

NTERM = 9
PZ, NZ = np.float32(0.0), np.float32(-0.0)


def chain(terms, leading_zero):
    """terms[..., 0] + ... + terms[..., 8] from the left, every add rounded to fp32; leading_zero: 0 + term 0 first."""
    acc = (np.zeros(terms.shape[:-1], np.float32) + terms[..., 0]) if leading_zero else terms[..., 0].copy()
    for t in range(1, NTERM):
        acc = acc + terms[..., t]
    assert acc.dtype == np.float32
    return acc


def lap_forms(tz, tx):
    """(reference, built, wrong) of az + ax for the z terms tz[n][9] and the x terms tx[n][9]."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (chain(tz, True) + chain(tx, True), chain(tz, False) + chain(tx, True), chain(tz, False) + chain(tx, False))


def zero_sign_patterns():
    """Every assignment of +0 / -0 to the 18 terms: [2^18][18]."""
    k = np.arange(1 << (2 * NTERM), dtype=np.uint32)[:, None]
    sign = (k >> np.arange(2 * NTERM, dtype=np.uint32)[None, :]) & np.uint32(1)
    return (sign << np.uint32(31)).view(np.float32)


def class_inputs():
    """Terms drawn per class pair (z terms of one class, x terms of another), all classes mixed term by term, and zeros mixed into every class."""
    rng = np.random.default_rng(12)
    n = 4096
    out = []
    for cz in CLASSES:
        for cx in CLASSES:
            out.append(np.concatenate([class_values(cz, n * NTERM, rng).reshape(n, NTERM), class_values(cx, n * NTERM, rng).reshape(n, NTERM)], axis=1))
    pool = np.concatenate([class_values(c, 8192, rng) for c in CLASSES])
    out.append(pool[rng.integers(0, pool.size, (16 * n, 2 * NTERM))])
    zeros = zero_sign_patterns()
    for c in CLASSES:                                                   # a few non-zero terms of one class among signed zeros
        t = zeros[rng.integers(0, 1 << (2 * NTERM), 4 * n)].copy()
        hit = rng.random(t.shape) < 0.15
        t[hit] = class_values(c, int(hit.sum()), rng)
        out.append(t)
    return np.concatenate(out)


def test_z_chain_without_its_zero_is_the_reference_bit_for_bit():
    for name, t in (("zero sign patterns", zero_sign_patterns()), ("value classes", class_inputs())):
        ref, built, _ = lap_forms(t[:, :NTERM], t[:, NTERM:])
        bad = np.flatnonzero(bits(ref) != bits(built))
        assert bad.size == 0, f"{name}: {bad.size} of {len(t)} inputs differ; first {t[bad[0]]!r}: {ref[bad[0]]!r} vs {built[bad[0]]!r}"
    nonfinite = ~np.isfinite(lap_forms(t[:, :NTERM], t[:, NTERM:])[0])
    assert nonfinite.any() and not nonfinite.all()                     # the class inputs reach inf and NaN and are not only that


def test_dropping_both_zeros_is_seen():
    t = np.full((1, 2 * NTERM), NZ, np.float32)
    ref, built, wrong = lap_forms(t[:, :NTERM], t[:, NTERM:])
    assert bits(ref)[0] == 0 and bits(built)[0] == 0 and bits(wrong)[0] == 0x80000000
    z = zero_sign_patterns()
    ref, _, wrong = lap_forms(z[:, :NTERM], z[:, NTERM:])
    assert (bits(ref) != bits(wrong)).sum() == 1                       # ... and that is the only zero pattern on which it shows


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
N, NB, XCHUNK, NSTEPS = 1024, 64, 61, 8
SX, SZ = 500, 500                      # chunk rows 7 | 8 (rows 427 .. 487 | 488 .. 548), strip 2 (its own columns 448 .. 671)
LEAN, FULL = 0, 1
# rows across the chunk border 182 | 183, columns across 207 | 208 and 223 | 224 (strips 0 | 1); wide enough that eight steps of four cells from
# every side leave zeros in its middle
RECT = (slice(140, 232), slice(160, 272))


def mk(d, **kw):
    ctx = F.FDWave(d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"], compat=False, **kw)
    ctx.set_tuning(two_step=4, xchunk=XCHUNK)
    assert ctx.steps_per_pass() == 4
    return ctx


def plan(ctx, sx, sz):
    nblk, nstrip = C.c_int(), C.c_int()
    cls = (C.c_ubyte * 4096)()
    _lib.check(_lib.lib().fdw_debug_step4_plan(ctx._h, 1, sx, sz, 0, -1, 0, 0, XCHUNK, C.byref(nblk), C.byref(nstrip), C.cast(cls, C.c_void_p), len(cls)))
    return np.array(cls[:nblk.value], np.uint8).reshape(-1, nstrip.value)


@pytest.fixture(scope="module")
def deck():
    d = make_deck(N, N, NB, NB, NSTEPS, seed=33, compat=False)
    shape = (N, N)
    zeros, ricker = np.zeros(NSTEPS, np.float32), O.ricker_wavelet(NSTEPS, d["dt"], 30.0)
    starts = {}
    # (a) p = -0, pp = +0 everywhere: the neighbourhood on which a Laplacian without any leading zero is -0 and the new value -0 instead of +0
    starts["a"] = (np.full(shape, NZ, np.float32), np.zeros(shape, np.float32), zeros)
    # (b) the same with one non-zero cell in a lean tile (chunk row 3, strip 1) and one in a frame tile (chunk row 0, strip 2)
    pb = np.full(shape, NZ, np.float32)
    pb[200, 300], pb[10, 600] = 1.0, -0.5
    starts["b"] = (pb, np.zeros(shape, np.float32), zeros)
    # (c) noise with a rectangle of -0 (+0 in the older field) across a strip border and a chunk border
    older, newest = random_fields(d, seed=7, amp=0.1)
    newest[RECT], older[RECT] = NZ, PZ
    starts["c"] = (newest, older, ricker)
    d["starts"] = starts
    d["want"] = {}
    for key, numerics in (("a", 0), ("b", 0), ("c", 0), ("c", 1)):
        p, pp, srce = starts[key]
        orc = O.Oracle(d["order"], N, N, NB, NB, NSTEPS, d["fac"], d["dx"], d["dz"], d["dt"], compat=False, numerics=numerics)
        d["want"][key, numerics] = orc.forward(d["v2"], SX, SZ, srce, pp, p, nsteps=NSTEPS)
    for a in [d["v2"]] + [x for s in starts.values() for x in s] + [x for w in d["want"].values() for x in w]:
        a.setflags(write=False)
    return d


@pytest.mark.gpu
def test_the_deck_holds_every_tile_class(deck):
    ctx = mk(deck)
    cls, nosrc = plan(ctx, SX, SZ), plan(ctx, -1, -1)
    assert cls.shape == (17, 5)
    inner = np.zeros(cls.shape, bool)
    inner[1:15, 1:4] = True
    assert (nosrc[inner] == LEAN).all() and (nosrc[~inner] == FULL).all(), "strip 0: the damped columns; strip 4, chunk rows 0, 15, 16: the frame"
    src = (cls != nosrc)
    assert src.sum() == 2 and src[7, 2] and src[8, 2] and (cls[src] == FULL).all(), "the source at row 500 reaches into chunk rows 7 and 8 of strip 2"
    assert (cls == LEAN).sum() == 40 and (cls == FULL).sum() == 45
    assert cls[3, 1] == LEAN and cls[0, 2] == FULL                      # the two non-zero cells of start (b)
    assert cls[2, 0] == FULL and cls[3, 0] == FULL and cls[2, 1] == LEAN and cls[3, 1] == LEAN      # the rectangle of start (c)


@pytest.mark.gpu
@pytest.mark.parametrize("start,numerics", [("a", 0), ("b", 0), ("c", 0), ("c", 1)], ids=["a-exact", "b-exact", "c-exact", "c-fast"])
def test_signed_zero_starts_vs_oracle(deck, start, numerics):
    d = deck
    p, pp, srce = d["starts"][start]
    ctx = mk(d, numerics=numerics)
    P, PP = ctx.forward(d["v2"], SX, SZ, srce, pp, p, nsteps=NSTEPS)
    oP, oPP = d["want"][start, numerics]
    if start == "a":
        assert not (np.abs(oPP) > 0).any()                              # all zeros: only their signs are at stake
    if start == "c":
        assert (bits(oPP[RECT]) << np.uint32(1) == 0).any()             # zeros survive inside the rectangle after eight steps of four cells each
    assert_bit_equal(PP, oPP, f"PP, start ({start}), numerics {numerics}")
    assert_bit_equal(P, oP, f"P, start ({start}), numerics {numerics}")

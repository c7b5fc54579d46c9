"""TEST HELPER (not a conftest): fp32 fields made of VALUE CLASSES, for tests/test_value_domain.py.

Every other test of the suite draws its data from amp * N(0, 1): normal numbers of one magnitude.  The fields made here are laid out as
rectangular patches, each filled from one class, with the patch borders ON and NEXT TO the places where the kernels change behaviour
(`deck_cuts`): the float4 border (z mod 4), the 16-lane DPP row (z mod 64), the strip borders of the three forward kernels (multiples of
224, 240 and 256 columns), the halo columns and rows (order / 2 from each edge), the damped strip (z < ztap, x < nxb and its mirror) and
the launch extents of compat mode (xlim, zlim).

Classes (CLASSES):
  normal       amp * N(0, 1), the regime the rest of the suite lives in (the control)
  subnormal    nonzero, |x| < 2^-126, both signs, the smallest (bit patterns 1, 0x80000001) and the largest (0x007fffff) among them
  tiny         2^-126 <= |x| < 2^-100: products with taper factors and v2 dt2 lap underflow INTO the subnormal range and round there
  pzero, nzero +0.0 and -0.0
  large        2^(large_exp-20) <= |x| < 2^(large_exp+1) (default large_exp = 60): every intermediate of a few time steps still finite
  overflowing  2^100 <= |x| <= FLT_MAX: sums reach +-inf and inf - inf (non-finite tests only)
"""
import numpy as np

FINITE = ("normal", "subnormal", "tiny", "pzero", "nzero", "large")
SMALL = ("subnormal", "tiny", "pzero", "nzero")             # nothing here ever leaves the neighbourhood of the subnormal range
CLASSES = FINITE + ("overflowing",)
FLT_MAX_BITS = 0x7F7FFFFF
MIN_NORMAL = np.float32(2.0 ** -126)
TINY_TOP = np.float32(2.0 ** -100)
LARGE_BOTTOM = np.float32(2.0 ** 40)


def _from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(np.float32)


def _signed(rng, mag_bits):
    return _from_bits(mag_bits.astype(np.uint32) | (rng.integers(0, 2, mag_bits.shape, dtype=np.uint32) << np.uint32(31)))


def _exponent_range(rng, n, e_lo, e_hi):
    """n values with a random sign, a random mantissa and an unbiased exponent drawn from [e_lo, e_hi]."""
    e = rng.integers(e_lo + 127, e_hi + 128, n, dtype=np.uint32)
    return _signed(rng, (e << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32))


def class_values(cls, n, rng, amp=1.0, large_exp=60):
    """n fp32 values of one class."""
    if cls == "normal":
        return (amp * rng.standard_normal(n)).astype(np.float32)
    if cls == "subnormal":
        mag = rng.integers(1, 1 << 23, n, dtype=np.uint32)
        pick = rng.integers(0, 16, n)
        mag[pick == 0] = 1                                   # the smallest subnormal (either sign)
        mag[pick == 1] = 0x007FFFFF                          # the largest
        return _signed(rng, mag)
    if cls == "tiny":
        return _exponent_range(rng, n, -126, -101)
    if cls == "pzero":
        return np.zeros(n, np.float32)
    if cls == "nzero":
        return _from_bits(np.full(n, 0x80000000, np.uint32)).copy()
    if cls == "large":
        return _exponent_range(rng, n, large_exp - 20, large_exp)
    if cls == "overflowing":
        v = _exponent_range(rng, n, 100, 127)
        b = v.view(np.uint32)
        top = rng.integers(0, 16, n) == 0
        b[top] = (b[top] & np.uint32(0x80000000)) | np.uint32(FLT_MAX_BITS)     # +-FLT_MAX itself
        return v
    raise ValueError(cls)


def cuts(n, specials, rng=None, extra=0):
    """Sorted cut positions in (0, n): every special position and its two neighbours, plus `extra` random ones."""
    c = set()
    for s in specials:
        c.update(k for k in (s - 1, s, s + 1) if 0 < k < n)
    if rng is not None and extra:
        c.update(int(k) for k in rng.integers(1, n, extra))
    return sorted(c)


def deck_cuts(deck, rng=None, extra=3):
    """(xcuts, zcuts) of a deck (conftest.make_deck): the places named in the module docstring."""
    nxe, nze, nxb, nzb, h = deck["nxe"], deck["nze"], deck["nxb"], deck["nzb"], deck["order"] // 2
    compat = deck.get("compat", True)
    xlim, zlim, ztap = (8 * (nxe // 8), 8 * (nze // 8), 8 * (nzb // 8)) if compat else (nxe, nze, nzb)
    zs = [h, nze - h, nzb, nze - nzb, ztap, zlim]
    for strip in (64, 224, 240, 256):
        zs += list(range(strip, nze, strip))
    zs += [4 * ((nze // 3) // 4), 4 * ((2 * nze // 3) // 4) + 2]      # a float4 border and the middle of a float4 away from everything else
    xs = [h, nxe - h, nxb, nxe - nxb, xlim, nxe // 2]
    return cuts(nxe, xs, rng, extra), cuts(nze, zs, rng, extra)


def patched(shape, seed, classes=FINITE, xcuts=(), zcuts=(), amp=1.0, large_exp=60, want_map=False):
    """An fp32 array [nxe][nze] of rectangular patches between the cut positions, each patch filled from one class drawn from `classes`
    (every class is used at least once when there are enough patches).  want_map: also the int array of class indices into `classes`."""
    nxe, nze = shape
    rng = np.random.default_rng(seed)
    xe, ze = [0] + [c for c in xcuts if 0 < c < nxe] + [nxe], [0] + [c for c in zcuts if 0 < c < nze] + [nze]
    npatch = (len(xe) - 1) * (len(ze) - 1)
    which = rng.integers(0, len(classes), npatch)
    if npatch >= len(classes):
        which[rng.permutation(npatch)[:len(classes)]] = np.arange(len(classes))
    out = np.zeros(shape, np.float32)
    cmap = np.zeros(shape, np.int8)
    k = 0
    for a, b in zip(xe[:-1], xe[1:]):
        for c, d in zip(ze[:-1], ze[1:]):
            cls = classes[which[k]]
            out[a:b, c:d] = class_values(cls, (b - a) * (d - c), rng, amp, large_exp).reshape(b - a, d - c)
            cmap[a:b, c:d] = which[k]
            k += 1
    return (out, cmap) if want_map else out


def patched_1d(n, seed, classes=FINITE, amp=1.0, large_exp=60, run=3):
    """n values in runs of `run` samples of one class each (wavelets, traces)."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, np.float32)
    for a in range(0, n, run):
        m = min(run, n - a)
        out[a:a + m] = class_values(classes[int(rng.integers(0, len(classes)))], m, rng, amp, large_exp)
    return out


def compat_precondition(deck, *fields):
    """conftest.random_fields' zeroing: in compat mode the rows >= xlim of the damped strip z < ztap are never stepped and must be zero."""
    if deck.get("compat", True):
        xlim, ztap = 8 * (deck["nxe"] // 8), 8 * (deck["nzb"] // 8)
        for f in fields:
            f[xlim:, :ztap] = 0
    return fields


def deck_inputs(deck, seed, classes=FINITE, amp=1.0, large_exp=60, extra=3):
    """Class-patched p, pp, wavelet, gather d_obs[nx][nt] and start image im0[nx][nz] of a deck, as a dict."""
    nxe, nze, nxb, nzb, nt = deck["nxe"], deck["nze"], deck["nxb"], deck["nzb"], deck["nt"]
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    rng = np.random.default_rng(seed)
    xc, zc = deck_cuts(deck, rng, extra)
    kw = dict(classes=classes, amp=amp, large_exp=large_exp)
    p, pp = patched((nxe, nze), seed + 1, xcuts=xc, zcuts=zc, **kw), patched((nxe, nze), seed + 2, xcuts=xc, zcuts=zc, **kw)
    compat_precondition(deck, p, pp)
    im0 = patched((nx, nz), seed + 3, xcuts=[c - nxb for c in xc], zcuts=[c - nzb for c in zc], **kw)
    d_obs = patched((nx, nt), seed + 4, xcuts=[c - nxb for c in xc], zcuts=range(3, nt, 3), **kw)
    return dict(p=p, pp=pp, srce=patched_1d(nt, seed + 5, **kw), d_obs=d_obs, im0=im0)


def scaled(inputs, k):
    """The inputs (dict of p, pp, srce, d_obs, im0, any subset) times 2^k: exact unless a value leaves the normal range, where it is rounded
    once (to a subnormal) or overflows."""
    return {name: (np.ldexp(a, k).astype(np.float32) if name in ("p", "pp", "srce", "d_obs", "im0") and a is not None else a)
            for name, a in inputs.items()}


def classify(a):
    """Counts per class of an fp32 array: nan, inf, pzero, nzero, subnormal, tiny (2^-126 <= |x| < 2^-100), normal, large (|x| >= 2^40)."""
    a = np.ascontiguousarray(a, np.float32).ravel()
    b = a.view(np.uint32)
    mag = np.abs(a)
    fin = np.isfinite(a)
    out = dict(nan=int(np.isnan(a).sum()), inf=int(np.isinf(a).sum()), pzero=int((b == 0).sum()), nzero=int((b == 0x80000000).sum()),
               subnormal=int(((mag > 0) & (mag < MIN_NORMAL)).sum()), tiny=int(((mag >= MIN_NORMAL) & (mag < TINY_TOP)).sum()),
               normal=int((fin & (mag >= TINY_TOP) & (mag < LARGE_BOTTOM)).sum()), large=int((fin & (mag >= LARGE_BOTTOM)).sum()))
    assert sum(out.values()) == a.size
    return out


def share(a, *names):
    """Fraction of the cells of `a` in the named classes of `classify`."""
    c = classify(a)
    return sum(c[n] for n in names) / max(1, np.size(a))


def shares(a):
    """classify as fractions, rounded, for assertion messages."""
    n = max(1, np.size(a))
    return {k: round(v / n, 4) for k, v in classify(a).items() if v}


def assert_same_nonfinite(a, b, what=""):
    """Same NaN positions (NaN sign and payload legitimately differ between the CPU and the GPU); every other cell, infinities included,
    equal bit for bit."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    na, nb = np.isnan(a), np.isnan(b)
    bad = np.flatnonzero((na != nb).ravel())
    if bad.size:
        k = bad[0]
        raise AssertionError(f"{what}: NaN in {bad.size} cells of one side only; first at coords {np.unravel_index(k, a.shape)}: "
                             f"{a.ravel()[k]!r} vs {b.ravel()[k]!r}")
    bad = np.flatnonzero(((a.view(np.uint32) != b.view(np.uint32)) & ~na).ravel())
    if bad.size:
        k = bad[0]
        raise AssertionError(f"{what}: {bad.size} of {a.size} non-NaN values differ bitwise; first at coords {np.unravel_index(k, a.shape)}: "
                             f"{a.ravel()[k]!r} vs {b.ravel()[k]!r}")


# ---- the three errors the value-domain tests exist to catch, applied to an array (tests/test_value_domain.py shows that each is caught) ----
def flush_subnormals(a):
    """What a kernel built with fp32 denormal mode 0 makes of a value: subnormals become zeros of the same sign."""
    a = np.array(a, np.float32)
    b = a.view(np.uint32)
    b[(b & np.uint32(0x7F800000)) == 0] &= np.uint32(0x80000000)
    return a


def add_plus_zero(a):
    """x + 0.0f on every cell: the identity but for -0.0, which becomes +0.0."""
    return (np.asarray(a, np.float32) + np.float32(0.0)).astype(np.float32)


def mask_multiply(new, old, mask):
    """`mask * new + (1 - mask) * old` in fp32 instead of `mask ? new : old`."""
    m = mask.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (m * np.asarray(new, np.float32) + (np.float32(1.0) - m) * np.asarray(old, np.float32)).astype(np.float32)

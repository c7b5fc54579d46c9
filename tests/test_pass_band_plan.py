"""fdw_plan_pass_bands (fdwave.h): the schedule that lets consecutive four-step forward passes overlap as row bands on side streams.

The planner is pure host arithmetic, so everything here runs without a device.  For every plan the test rebuilds HAPPENS-BEFORE from what
the plan states -- stream order (a unit follows the previous unit of its stream) plus the waits, transitively closed -- and requires, for
EVERY pair of units, that the two are ordered whenever one writes rows of a buffer that the other reads or writes.  What a unit touches:

    pass n reads the two input fields of the pass on rows [r0 - 16, r1 + 16) (four steps of half order 4), clipped to the grid,
    and writes its two output fields on rows [r0, r1); the last band's range ends at nxl, the static rows [upd_x1, nxl) included;
    the four buffers rotate: the outputs of pass n are the inputs of pass n + 1, whose outputs are the inputs of pass n again.

So with the buffers as two pairs, pass n reads pair n mod 2 and writes the other one.

Besides: the bands tile [0, nxl) exactly once on chunk boundaries and are as equal as possible; the numbering is pass-major; unit i runs
on stream i mod D and everything up to unit i - D happens before it; a request that is too thin (a band below 16 time-stepped rows, fewer
bands than D + 1) comes back as one band of depth 1 and a sound request comes back as asked -- the expectation is restated here.

The check is not vacuous: test_a_dropped_wait_is_caught removes single waits from sound plans and the pair rule reports a race."""
import ctypes as C
import functools

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from parallel_finite_difference_computation_amd._lib import PASS_DEPTH_MAX, BandUnit

REACH = 16
XCHUNKS = (13, 16, 23, 43)
NXLS = sorted(set(range(16, 401, 7)) | {16, 31, 32, 33, 69, 224, 230, 399, 400})
PASSES = 5


def plan(nxl, upd, xchunk, bands, depth, npasses):
    g, d, units = F.plan_pass_bands(nxl, upd, xchunk, bands, depth, npasses)
    assert len(units) == g * npasses
    return g, d, units


def expected(nxl, upd, xchunk, bands, depth):
    """(G, D, band edges) restated: whole chunk rows from row 0, the first nchunks % G bands one chunk row longer."""
    nchunks = -(-upd // xchunk)
    if bands >= 2 and bands >= depth + 1 and bands <= nchunks:
        base, extra = divmod(nchunks, bands)
        first = [g * base + min(g, extra) for g in range(bands + 1)]
        heights = [min(first[g + 1] * xchunk, upd) - first[g] * xchunk for g in range(bands)]
        if min(heights) >= REACH:
            return bands, depth, [f * xchunk for f in first[:-1]] + [nxl]
    return 1, 1, [0, nxl]


@functools.lru_cache(maxsize=None)
def happens_before(order):
    """order: per unit (stream, waits).  hb[i, j]: unit j is complete before unit i starts."""
    n = len(order)
    reach, last = [0] * n, {}
    for i, (stream, waits) in enumerate(order):
        preds = list(waits) + ([last[stream]] if stream in last else [])
        for p in preds:
            assert 0 <= p < i, f"unit {i} is ordered behind unit {p}"
            reach[i] |= reach[p] | (1 << p)
        last[stream] = i
    return np.array([[(reach[i] >> j) & 1 for j in range(n)] for i in range(n)], bool).reshape(n, n)


def races(units, nxl, order=None):
    """Pairs (i, j), i < j, that touch the same rows of a buffer, one of them writing, without being ordered."""
    order = order or tuple((u["stream"], tuple(u["wait"])) for u in units)
    hb = happens_before(order)
    r0 = np.array([u["r0"] for u in units])
    r1 = np.array([u["r1"] for u in units])
    rd = np.array([u["pass_"] % 2 for u in units])
    wr = 1 - rd
    a0, a1 = np.maximum(r0 - REACH, 0), np.minimum(r1 + REACH, nxl)

    def meet(lo, hi, lo2, hi2):
        return (lo[:, None] < hi2[None, :]) & (lo2[None, :] < hi[:, None])

    write_read = (wr[:, None] == rd[None, :]) & meet(r0, r1, a0, a1)          # i writes what j reads
    write_write = (wr[:, None] == wr[None, :]) & meet(r0, r1, r0, r1)
    conflict = write_read | write_read.T | write_write
    np.fill_diagonal(conflict, False)
    bad = conflict & ~(hb | hb.T)
    return [(int(i), int(j)) for i, j in zip(*np.nonzero(np.triu(bad)))]


def check_plan(nxl, upd, xchunk, bands, depth):
    what = f"nxl={nxl} upd_x1={upd} xchunk={xchunk} bands={bands} depth={depth}"
    g, d, units = plan(nxl, upd, xchunk, bands, depth, PASSES)
    eg, ed, edges = expected(nxl, upd, xchunk, bands, depth)
    assert (g, d) == (eg, ed), what
    for i, u in enumerate(units):
        assert (u["pass_"], u["band"], u["stream"]) == (i // g, i % g, i % d), (what, i)
        assert (u["r0"], u["r1"]) == (edges[u["band"]], edges[u["band"] + 1]), (what, i)      # tiles [0, nxl) once, the same in every pass
        assert u["r0"] % xchunk == 0 and (u["r1"] % xchunk == 0 or u["r1"] == nxl), (what, i)
        assert u["wait"] == [j for j in range(i - d - 1, i - 2 * d, -1) if j >= 0], (what, i)
    assert races(units, nxl) == [], what
    hb = happens_before(tuple((u["stream"], tuple(u["wait"])) for u in units))
    for i in range(len(units)):
        assert hb[i, :max(i - d + 1, 0)].all(), f"{what}: unit {i} may overlap a unit before {i - d + 1}"
    return g, d, units


@pytest.mark.parametrize("xchunk", XCHUNKS)
def test_every_plan_orders_every_conflicting_pair(xchunk):
    banded = 0
    for nxl in NXLS:
        for upd in sorted({nxl, 8 * (nxl // 8), max(nxl - 21, 1)}):
            for bands in range(1, 13):
                for depth in range(1, PASS_DEPTH_MAX + 1):
                    g, d, _ = check_plan(nxl, upd, xchunk, bands, depth)
                    banded += g > 1
    assert banded > 500          # the sweep is not all fall-backs


@pytest.mark.parametrize("npasses", [1, 2, 3, 4])
def test_fewer_passes_are_a_prefix(npasses):
    for nxl, upd, xchunk, bands, depth in ((230, 230, 23, 10, 3), (230, 224, 23, 5, 3), (400, 400, 43, 3, 2), (400, 393, 16, 12, 3), (100, 100, 13, 3, 1)):
        g, d, units = plan(nxl, upd, xchunk, bands, depth, PASSES)
        g2, d2, short = plan(nxl, upd, xchunk, bands, depth, npasses)
        assert (g2, d2) == (g, d) and g > 1 and short == units[:g * npasses]
        assert races(short, nxl) == []


def test_thin_requests_come_back_as_one_band():
    for args in ((230, 230, 13, 10, 2),      # bands of one 13-row chunk
                 (230, 230, 23, 3, 3),       # G < D + 1
                 (230, 230, 23, 2, 2),
                 (230, 217, 23, 10, 2),      # the last band holds 217 - 207 = 10 time-stepped rows
                 (230, 230, 23, 11, 2),      # more bands than chunk rows
                 (230, 230, 23, 1, 1)):
        g, d, units = plan(*args, 3)
        assert (g, d) == (1, 1) and [(u["r0"], u["r1"], u["stream"], u["wait"]) for u in units] == [(0, 230, 0, [])] * 3, args
    assert plan(230, 224, 23, 10, 3, 1)[:2] == (10, 3)      # 224 - 207 = 17 rows: enough
    assert plan(230, 230, 23, 2, 1, 1)[:2] == (2, 1)


def test_bad_arguments_are_refused():
    L = F.lib()
    g, d = C.c_int(), C.c_int()
    for args in ((0, 0, 23, 3, 2, 1), (230, 231, 23, 3, 2, 1), (230, 230, 0, 3, 2, 1), (230, 230, 23, 0, 2, 1), (230, 230, 23, 3, 0, 1),
                 (230, 230, 23, 3, PASS_DEPTH_MAX + 1, 1), (230, 230, 23, 3, 2, 0)):
        assert L.fdw_plan_pass_bands(*args, C.byref(g), C.byref(d), None, 0) == -1, args
    units = (BandUnit * 4)()
    assert L.fdw_plan_pass_bands(230, 230, 23, 3, 2, 5, C.byref(g), C.byref(d), units, 4) == 15      # the count, whatever the capacity
    assert [u.r0 for u in units] == [0, 92, 161, 0]
    assert L.fdw_set_pass_bands(None, 0, 0) == -1 and L.fdw_pass_bands(None, C.byref(g), C.byref(d)) == -1


def test_a_dropped_wait_is_caught():
    """The pair rule sees a missing wait: in the tightest sound plans (G = D + 1) every wait for the previous pass on the same or a
    neighbouring band is needed.  (With D = 3 band 0 also waits for the last band of the pass before the previous one, which the uniform
    rule i - 2D + 1 names although the two share no rows: that one wait may go.)"""
    for nxl, xchunk, bands, depth in ((230, 23, 3, 2), (230, 23, 4, 3), (400, 43, 4, 3)):
        g, d, units = plan(nxl, nxl, xchunk, bands, depth, PASSES)
        assert (g, d) == (bands, depth)
        order = [(u["stream"], tuple(u["wait"])) for u in units]
        dropped = 0
        for i, (stream, waits) in enumerate(order):
            for w in waits:
                if units[w]["pass_"] != units[i]["pass_"] - 1 or abs(units[w]["band"] - units[i]["band"]) > 1:
                    continue
                cut = list(order)
                cut[i] = (stream, tuple(x for x in waits if x != w))
                assert races(units, nxl, tuple(cut)), f"bands={bands} depth={depth}: unit {i} without its wait for {w} races with nothing"
                dropped += 1
        assert dropped >= PASSES

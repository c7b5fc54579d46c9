#!/usr/bin/env python3
"""Cost of a full tile of the four-step pass against a lean one (development tool; FDW_LIB selects a variant build).

Times fdw_dev_step4 on the bench grid (8192^2, source in the middle) with HIP events around N back-to-back launches, median of R
repeats, EXACT and FAST, on the rows [173, 8131) -- 46 whole chunk rows of 173, lean except the strips 0 and 36 and the source tile --
and on the whole grid.  Run it on the build as it is and on one whose tile predicate sends every tile to the full body
(profiles/README.md has the one-line patch): both interior launches are uniform in the chunk length, so the two times give
w = c_full / c_lean, and the whole-grid time against (c_lean N_lean + c_full N_full) / slots gives what placement costs.

TILE_XCHUNK=173,143,... sweeps the chunk length of the whole-grid launch (the interior rows go with the first); TILE_NUMERICS=0 EXACT only."""
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

import parallel_finite_difference_computation_amd as F
from parallel_finite_difference_computation_amd import _lib

N_LAUNCH = int(os.environ.get("TILE_N", "40"))
REPEATS = int(os.environ.get("TILE_R", "7"))
n = int(os.environ.get("TILE_SIZE", "8192"))
chunks = [int(v) for v in os.environ.get("TILE_XCHUNK", "173").split(",")]
dev = torch.device("cuda:0")
ts = torch.cuda.Stream()
torch.cuda.set_stream(ts)
s = ts.cuda_stream


def plan(ctx, sx, sz, r0, r1, xchunk):
    """(tiles, lean, full) as the host classifies them, or None on a build without the export."""
    fn = getattr(_lib.lib(), "fdw_debug_step4_plan", None)
    if fn is None:
        return None
    nblk, nstrip = C.c_int(), C.c_int()
    cls = (C.c_ubyte * 65536)()
    _lib.check(fn(ctx._h, 1, sx, sz, r0, r1, 0, 0, xchunk, C.byref(nblk), C.byref(nstrip), C.cast(cls, C.c_void_p), len(cls)))
    c = list(cls[:nblk.value])
    return nblk.value, c.count(0), c.count(1)


def time_launches(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(N_LAUNCH):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / N_LAUNCH)
    return statistics.median(out), min(out), max(out)


for numerics in [int(v) for v in os.environ.get("TILE_NUMERICS", "0,1").split(",")]:
    ctx = F.FDWave(8, n, n, 64, 64, 100, 0.75, 10.0, 10.0, 0.001, compat=False, numerics=numerics)
    ctx.set_tuning(two_step=4)
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED0001)
    bufs = [torch.zeros((n, ctx.pitch), device=dev) for _ in range(4)]
    for b in bufs[:2]:
        b[:, :n] = 1e-3 * torch.randn((n, n), device=dev, generator=g)
    v2 = torch.zeros((n, ctx.pitch), device=dev)
    v2[:, :n] = (1500.0 + 2500.0 * torch.rand((n, n), device=dev, generator=g)) ** 2
    srce = torch.from_numpy(F.ricker_wavelet(100, 0.001, 20.0)).to(dev)
    sx = sz = n // 2
    for xchunk in chunks:
        ranges = [("whole", 0, -1)]
        if xchunk == chunks[0]:
            ranges.insert(0, ("interior", xchunk, xchunk * (n // xchunk)))      # chunk rows 1 .. the last whole one but one
        for name, r0, r1 in ranges:
            def go():
                ctx.dev_step4(bufs[0].data_ptr(), bufs[1].data_ptr(), v2.data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), True, srce.data_ptr() + 4 * 50,
                              sx, sz, r0=r0, r1=r1, xchunk=xchunk, stream=s)
            med, lo, hi = time_launches(go)
            pl = plan(ctx, sx, sz, r0, r1, xchunk)
            tiles = "tiles n/a (no fdw_debug_step4_plan in this build)" if pl is None else \
                f"tiles {pl[0]} lean {pl[1]} full {pl[2]}"
            print(f"{os.path.basename(F.LIB_PATH):28s} {'FAST ' if numerics else 'EXACT'} {n}^2 xchunk={xchunk:3d} {name:8s} rows [{r0},{r1}): "
                  f"median {med:8.2f} us/launch (min {lo:.2f} max {hi:.2f}, {REPEATS} x {N_LAUNCH} launches)  {tiles}", flush=True)
    del bufs, v2, ctx

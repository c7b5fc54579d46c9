#!/usr/bin/env python3
"""The cost of a line source in the forward loop, and what plane-wave migration saves on a small deck.

    python3 scripts/bench_line_source.py [--size 8192] [--steps 200] [--warmup 50] [--repeats 5] [--out profiles/line_source_8192.json]

Part 1, per numerics (EXACT, FAST): order 8 on a size^2 grid, noise-filled fields.  The point-source forward loop (fdw_dev_steps2) and the
line-source loop (fdw_dev_line_steps, plain, a full-width line at depth nzb + 2) run in the same process on the same buffers, alternating;
each window is `steps` steps after `warmup`, timed with events; the median of `repeats` windows is reported, with the ratio and the tile
classes of one four-step pass of each loop (fdw_debug_step4_plan / fdw_debug_step4_plan_line): the line makes every tile of the strip
that holds it run the full body.

Part 2: a deck of the size of new_mod (315 x 195 interior, borders 50, nt 1700, six shots, synthetic model and data) migrated as six
shots one by one (fdw_shot), as one batch (fdw_shot_batch: what rtm_code does on such a deck) and as NP = 3 plane waves (encoding +
fdw_shot_line each): wall time of each.

--batch (profiles/line_batch.json) measures instead: the forward loop that records and accumulates, point source
(fdw_dev_record_illum_steps) against line source (fdw_dev_line_record_illum_steps), alternating as in part 1; and the same deck with NP = 6
plane waves through the one-by-one path (fdw_encode_gathers + fdw_shot_line per plane wave) and the batched path (fdw_encode_gathers_multi +
fdw_shot_line_batch), alternating in one process, median of three, beside the six point shots one by one and as one fdw_shot_batch.
Development tool, not part of the suite."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import parallel_finite_difference_computation_amd as F  # noqa: E402
from parallel_finite_difference_computation_amd import _lib  # noqa: E402


def plan_point(ctx, sx, sz):
    nblk, nstrip = C.c_int(), C.c_int()
    _lib.check(_lib.lib().fdw_debug_step4_plan(ctx._h, 1, sx, sz, 0, -1, 0, 0, 0, C.byref(nblk), C.byref(nstrip), None, 0))
    cls = (C.c_ubyte * nblk.value)()
    _lib.check(_lib.lib().fdw_debug_step4_plan(ctx._h, 1, sx, sz, 0, -1, 0, 0, 0, C.byref(nblk), C.byref(nstrip), C.cast(cls, C.c_void_p), nblk.value))
    return nblk.value, nstrip.value, int(sum(cls))


def forward_loops(size, steps, warmup, repeats, numerics):
    nb = 64
    dev = torch.device("cuda:0")
    ctx = F.FDWave(8, size, size, nb, nb, steps + warmup, 0.75, 10.0, 10.0, 0.001, compat=False, numerics=numerics)
    nx = size - 2 * nb
    sz = nb + 2
    gen = torch.Generator(device=dev).manual_seed(1)
    bufs = [torch.randn((size, ctx.pitch), device=dev, generator=gen) * 1e-3 for _ in range(4)]
    for b in bufs:
        b[:, size:] = 0
    v2 = torch.zeros((size, ctx.pitch), device=dev)
    v2[:, :size] = (1500.0 + 2500.0 * torch.rand((size, size), device=dev, generator=gen)) ** 2
    srce = torch.randn(steps + warmup, device=dev, generator=gen) * 1e-3
    wav = torch.randn((steps + warmup, nx), device=dev, generator=gen) * 1e-3
    ptrs = [b.data_ptr() for b in bufs]
    st = {"ip": 0, "ipp": 1}
    ts = torch.cuda.Stream()                                # the loops and the timing events on one stream
    torch.cuda.set_stream(ts)
    s = ts.cuda_stream

    def point(it0, n):
        st["ip"], st["ipp"] = ctx.dev_steps2(ptrs, v2.data_ptr(), srce.data_ptr(), size // 2, sz, it0, n, True, st["ip"], st["ipp"], stream=s)

    def line(it0, n):
        st["ip"], st["ipp"] = ctx.dev_line_steps(ptrs, v2.data_ptr(), wav.data_ptr(), sz, it0, n, first_pp_twice=True, ip=st["ip"], ipp=st["ipp"], stream=s)

    def window(fn):
        fn(0, warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warmup, steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3          # us per step

    t = {"point": [], "line": []}
    for _ in range(repeats):                                # alternating: drift of the clocks hits both alike
        t["point"].append(window(point))
        t["line"].append(window(line))
    nblk, nstrip, full_point = plan_point(ctx, size // 2, sz)
    nblk_l, nstrip_l, cls = ctx.debug_step4_plan_line(sz)
    assert (nblk, nstrip) == (nblk_l, nstrip_l)
    torch.cuda.set_stream(torch.cuda.default_stream())
    tp, tl = statistics.median(t["point"]), statistics.median(t["line"])
    out = dict(numerics="fast" if numerics else "exact", steps_per_pass=ctx.steps_per_pass(), point_us_per_step=round(tp, 2), line_us_per_step=round(tl, 2),
               ratio_line_over_point=round(tl / tp, 4), point_windows_us=[round(x, 2) for x in t["point"]], line_windows_us=[round(x, 2) for x in t["line"]],
               tiles=nblk, strips=nstrip, full_tiles_point=full_point, full_tiles_line=int(cls.sum()),
               extra_full_tiles=int(cls.sum()) - full_point, extra_full_tile_share=round((int(cls.sum()) - full_point) / nblk, 4))
    print(json.dumps(out), flush=True)
    return out


def record_illum_loops(size, steps, warmup, repeats, numerics):
    """us per step of the forward loop that writes its trace rows and accumulates the illumination: point source against line source."""
    nb = 64
    dev = torch.device("cuda:0")
    nt = steps + warmup
    ctx = F.FDWave(8, size, size, nb, nb, nt, 0.75, 10.0, 10.0, 0.001, compat=False, numerics=numerics)
    nx = size - 2 * nb
    sz, gz = nb + 2, nb + 1
    gen = torch.Generator(device=dev).manual_seed(1)
    bufs = [torch.randn((size, ctx.pitch), device=dev, generator=gen) * 1e-3 for _ in range(4)]
    for b in bufs:
        b[:, size:] = 0
    v2 = torch.zeros((size, ctx.pitch), device=dev)
    v2[:, :size] = (1500.0 + 2500.0 * torch.rand((size, size), device=dev, generator=gen)) ** 2
    srce = torch.randn(nt, device=dev, generator=gen) * 1e-3
    wav = torch.randn((nt, nx), device=dev, generator=gen) * 1e-3
    rec = torch.zeros((nt, nx), device=dev)
    il = torch.zeros((size, ctx.pitch), device=dev)
    ptrs = [b.data_ptr() for b in bufs]
    st = {"ip": 0, "ipp": 1}
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    s = ts.cuda_stream

    def point(it0, n):
        st["ip"], st["ipp"] = ctx.dev_record_illum_steps(ptrs, v2.data_ptr(), srce.data_ptr(), size // 2, sz, gz, rec.data_ptr(), il.data_ptr(), it0, n, True,
                                                         st["ip"], st["ipp"], stream=s)

    def line(it0, n):
        st["ip"], st["ipp"] = ctx.dev_line_record_illum_steps(ptrs, v2.data_ptr(), wav.data_ptr(), sz, gz, rec.data_ptr(), il.data_ptr(), it0, n, True,
                                                              st["ip"], st["ipp"], stream=s)

    def window(fn):
        fn(0, warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warmup, steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3

    t = {"point": [], "line": []}
    for _ in range(repeats):
        t["point"].append(window(point))
        t["line"].append(window(line))
    torch.cuda.set_stream(torch.cuda.default_stream())
    tp, tl = statistics.median(t["point"]), statistics.median(t["line"])
    out = dict(numerics="fast" if numerics else "exact", steps_per_pass=ctx.steps_per_pass(), point_us_per_step=round(tp, 2), line_us_per_step=round(tl, 2),
               ratio_line_over_point=round(tl / tp, 4), point_windows_us=[round(x, 2) for x in t["point"]], line_windows_us=[round(x, 2) for x in t["line"]])
    print(json.dumps(out), flush=True)
    return out


def whole_job_batched(npw=6):
    """The deck of whole_job with NP plane waves: the one-by-one path against the batched path, alternating; the six point shots beside them."""
    nx, nz, nb, nt, ns, fsx, ds = 315, 195, 50, 1700, 6, 7, 60
    nxe, nze = nx + 2 * nb, nz + 2 * nb
    rng = np.random.default_rng(0)
    vp = (1500 + 2500 * np.linspace(0, 1, nz, dtype=np.float32)[None, :] + 50 * rng.standard_normal((nx, nz))).astype(np.float32)
    d_obs = rng.standard_normal((ns, nx, nt)).astype(np.float32)
    srce = F.ricker_wavelet(nt, 0.001, 20.0)
    sz = gz = nb
    src_ix = fsx + ds * np.arange(ns)
    ones = np.ones(ns, np.float32)
    pmax = 2.0e-4
    ctx = F.FDWave(8, nxe, nze, nb, nb, nt, 0.75, 10.0, 10.0, 0.001, compat=True)
    ctx.model_resident(vp)
    draws = ctx.border_draws()
    bmax = max(1, min(npw, ctx.shot_batch_max()))
    last = {}

    def rays():
        return [-pmax + 2 * pmax * j / (npw - 1) for j in range(npw)]

    def one_by_one():
        imgs = []
        for j, p in enumerate(rays()):
            lag = F.planewave_lags(src_ix, 10.0, 0.001, p)
            wav = F.encode_line_source(src_ix, lag, ones, srce, nx)
            enc = F.encode_gathers(lag, ones, d_obs)
            ctx.dev_extendvel_linear(j * draws)
            imgs.append(ctx.shot_line(None, sz, gz, wav, enc))
        last["one"] = np.stack(imgs)

    def batched():
        lags = np.stack([F.planewave_lags(src_ix, 10.0, 0.001, p) for p in rays()])
        wavs = np.stack([F.encode_line_source(src_ix, lag, ones, srce, nx) for lag in lags])
        encs = F.encode_gathers_multi(lags, np.ones((npw, ns), np.float32), d_obs)
        imgs = [ctx.shot_line_batch(min(bmax, npw - j0), sz, gz, wavs[j0:j0 + bmax], encs[j0:j0 + bmax], draw_offset=j0 * draws) for j0 in range(0, npw, bmax)]
        last["batch"] = np.concatenate(imgs)

    def shots():
        for s in range(ns):
            ctx.dev_extendvel_linear(s * draws)
            ctx.shot_resident(int(src_ix[s]) + nb, sz, gz, srce, d_obs[s])

    def shot_batch():
        ctx.shot_batch(ns, int(src_ix[0]) + nb, ds, sz, gz, srce, d_obs)

    walls = {"plane_waves_one_by_one_s": [], "plane_waves_batched_s": [], "six_shots_one_by_one_s": [], "six_shots_one_batch_s": []}
    fns = dict(zip(walls, (one_by_one, batched, shots, shot_batch)))
    for fn in fns.values():
        fn()                                                # allocations, first launches
    assert np.array_equal(last["one"].view(np.uint32), last["batch"].view(np.uint32)), "the batched plane waves are not the one-by-one images"
    for _ in range(3):                                      # alternating
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            walls[name].append(time.perf_counter() - t0)
    out = {k: round(statistics.median(v), 4) for k, v in walls.items()}
    out.update({k[:-2] + "_windows_s": [round(x, 4) for x in v] for k, v in walls.items()})
    out["plane_waves_per_batch"] = bmax
    out["images_bit_identical"] = True
    out["deck"] = f"{nx} x {nz} interior, borders {nb}, nt {nt}, ns {ns}, NP {npw}"
    print(json.dumps(out), flush=True)
    return out


def whole_job(npw=3):
    nx, nz, nb, nt, ns, fsx, ds = 315, 195, 50, 1700, 6, 7, 60
    nxe, nze = nx + 2 * nb, nz + 2 * nb
    rng = np.random.default_rng(0)
    vp = (1500 + 2500 * np.linspace(0, 1, nz, dtype=np.float32)[None, :] + 50 * rng.standard_normal((nx, nz))).astype(np.float32)
    d_obs = rng.standard_normal((ns, nx, nt)).astype(np.float32)
    srce = F.ricker_wavelet(nt, 0.001, 20.0)
    sz = gz = nb
    src_ix = fsx + ds * np.arange(ns)
    ctx = F.FDWave(8, nxe, nze, nb, nb, nt, 0.75, 10.0, 10.0, 0.001, compat=True)
    ctx.model_resident(vp)
    draws = ctx.border_draws()

    def shots():
        for s in range(ns):
            ctx.dev_extendvel_linear(s * draws)
            ctx.shot_resident(int(src_ix[s]) + nb, sz, gz, srce, d_obs[s])

    bmax = max(1, min(ns, ctx.shot_batch_max()))

    def batch():
        for s0 in range(0, ns, bmax):
            n = min(bmax, ns - s0)
            ctx.shot_batch(n, int(src_ix[s0]) + nb, ds, sz, gz, srce, d_obs[s0:s0 + n], draw_offset=s0 * draws)

    def planes():
        pmax = 2.0e-4
        for j in range(npw):
            lag = F.planewave_lags(src_ix, 10.0, 0.001, -pmax + 2 * pmax * j / (npw - 1))
            wav = F.encode_line_source(src_ix, lag, np.ones(ns, np.float32), srce, nx)
            enc = F.encode_gathers(lag, np.ones(ns, np.float32), d_obs)
            ctx.dev_extendvel_linear(j * draws)
            ctx.shot_line(None, sz, gz, wav, enc)

    out = {}
    for name, fn in (("six_shots_one_by_one_s", shots), ("six_shots_one_batch_s", batch), ("three_plane_waves_s", planes)):
        fn()                                                # allocations, first launches
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            walls.append(time.perf_counter() - t0)
        out[name] = round(statistics.median(walls), 4)
    out["shots_per_batch"] = bmax
    out["deck"] = f"{nx} x {nz} interior, borders {nb}, nt {nt}, ns {ns}, NP {npw}"
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", action="store_true", help="the measurements of DESIGN.md section 6m instead (profiles/line_batch.json)")
    a = ap.parse_args()
    if a.batch:
        res = dict(size=a.size, order=8, steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0),
                   whole_job=whole_job_batched(), record_illum_forward=[record_illum_loops(a.size, a.steps, a.warmup, a.repeats, n) for n in (0, 1)])
    else:
        res = dict(size=a.size, order=8, steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0),
                   forward=[forward_loops(a.size, a.steps, a.warmup, a.repeats, n) for n in (0, 1)], whole_job=whole_job())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

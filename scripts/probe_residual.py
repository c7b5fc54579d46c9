#!/usr/bin/env python3
"""The cost of residual migration on one MI355X.

    python3 scripts/probe_residual.py shots [--tree DIR] [--reps N] [--out FILE]
        whole 8192^2 shots of 500 steps (order 8, 64-cell borders, full extents: the setting of scripts/probe_snaps.py), alternating in one
        process: fdw_shot, fdw_shot_illum, the composition residual migration replaces (fdw_record_shot + host subtraction + fdw_shot, and the
        same with fdw_shot_illum) and, where the library has it, fdw_shot_residual without and with an accumulator.  --tree: a built checkout
        (its own package and library; the parent commit's has only the compositions).  Results are compared bitwise before anything is timed.
    python3 scripts/probe_residual.py batch [--reps N] [--out FILE]
        new_mod's size (415 x 295 with its borders of 50, nt = 1700, order 8, host models): ms per shot of fdw_shot_batch_residual at 6 shots and
        at fdw_shot_batch_max(), without and with illumination, against fdw_shot_residual one by one (the method of scripts/probe_batch_illum.py)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/probe_residual.py kernel
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- python3 scripts/probe_residual.py kernel        (then WRITE_SIZE, a run of its own)
        40 steps of fdw_dev_illum_steps, then 40 of fdw_dev_record_illum_steps, at 8192^2 through the wave pipeline
    python3 scripts/probe_residual.py parse TRACE_DIR FETCH_DIR WRITE_DIR [--out FILE]
        per pass: kernel time and HBM-side bytes per point and step of fdw_stepn_illum_kernel and fdw_stepn_rec_illum_kernel"""
import argparse
import collections
import csv
import glob
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NB, NT = 8192, 64, 500


def shots(tree, reps, out):
    sys.path.insert(0, tree)
    import numpy as np
    import parallel_finite_difference_computation_amd as F
    ctx = F.FDWave(8, N, N, NB, NB, NT, 0.75, 10.0, 10.0, 1.0e-3, compat=False, device=0)
    nx = N - 2 * NB
    vel = (1500.0 + 2000.0 * np.arange(N, dtype=np.float32)[None, :] / (N - 1) + np.zeros((N, 1), np.float32)).astype(np.float32)
    v2 = np.ascontiguousarray(vel * vel)
    srce = F.ricker_wavelet(NT, 1.0e-3, 20.0)
    d_obs = np.random.default_rng(1).standard_normal((nx, NT)).astype(np.float32)
    sx, sz, gz = N // 2, NB + 2, NB + 3
    have = hasattr(F.FDWave, "shot_residual")
    print("tree", tree, "steps per pass", ctx.steps_per_pass(), "fdw_shot_residual", have, flush=True)

    def compose(illum):
        resid = d_obs - ctx.record_shot(v2, sx, sz, gz, srce)
        r = ctx.shot(v2, sx, sz, gz, srce, resid, want_illum=illum)
        return (resid,) + (tuple(r) if illum else (r,))

    variants = collections.OrderedDict([
        ("shot", lambda: ctx.shot(v2, sx, sz, gz, srce, d_obs)),
        ("shot_illum", lambda: ctx.shot(v2, sx, sz, gz, srce, d_obs, want_illum=True)),
        ("composition", lambda: compose(False)),
        ("composition_illum", lambda: compose(True)),
    ])
    if have:
        variants["residual"] = lambda: ctx.shot_residual(v2, sx, sz, gz, srce, d_obs)
        variants["residual_illum"] = lambda: ctx.shot_residual(v2, sx, sz, gz, srce, d_obs, want_illum=True)
    first = {k: fn() for k, fn in variants.items()}                   # allocations, first launches; and the results
    if have:
        for comp, res in (("composition", "residual"), ("composition_illum", "residual_illum")):
            assert np.array_equal(first[comp][0].view(np.uint32), first[res]["resid"].view(np.uint32)), res
            assert np.array_equal(first[comp][1].view(np.uint32), first[res]["image"].view(np.uint32)), res
        assert np.array_equal(first["composition_illum"][2].view(np.uint32), first["residual_illum"]["illum"].view(np.uint32))
        print("resid, image, illum identical to the composition's", flush=True)
    del first
    T = {k: [] for k in variants}
    for r in range(reps):
        for k, fn in variants.items():
            t = time.perf_counter()
            fn()
            T[k].append(time.perf_counter() - t)
        print("round", r, {k: round(v[-1] * 1e3, 1) for k, v in T.items()}, flush=True)
    res = dict(tree=tree, n=N, nt=NT, reps=reps, ms={k: [round(x * 1e3, 2) for x in v] for k, v in T.items()},
               median_ms={k: round(statistics.median(v) * 1e3, 2) for k, v in T.items()},
               min_max_ms={k: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for k, v in T.items()})
    print(json.dumps(res))
    if out:
        json.dump(res, open(out, "w"), indent=1)


def batch(reps, out):
    sys.path.insert(0, HERE)
    import numpy as np
    import parallel_finite_difference_computation_amd as F
    nxe, nze, nb, nt = 415, 295, 50, 1700
    nx = nxe - 2 * nb
    ctx = F.FDWave(8, nxe, nze, nb, nb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    bmax = ctx.shot_batch_max()
    rng = np.random.default_rng(1)
    srce = F.ricker_wavelet(nt, 0.001, 20.0)
    v2 = ((1500 + 2500 * rng.random((bmax, nxe, nze))) ** 2).astype(np.float32)
    d_obs = rng.standard_normal((bmax, nx, nt)).astype(np.float32)
    sx0, ds, sz, gz = nb + 7, 300 // max(bmax, 6), nb, nb
    T = collections.defaultdict(list)
    for n in (6, bmax):
        variants = [(f"one_by_one@{n}", lambda il: [ctx.shot_residual(v2[s], sx0 + s * ds, sz, gz, srce, d_obs[s], want_illum=il) for s in range(n)]),
                    (f"batch@{n}", lambda il: ctx.shot_batch_residual(n, sx0, ds, sz, gz, srce, d_obs[:n], v2_all=v2[:n], want_illum=il))]
        for il in (False, True):
            for name, fn in variants:
                fn(il)
            for r in range(reps):
                for name, fn in variants:
                    t = time.perf_counter()
                    fn(il)
                    T[name + ("+illum" if il else "")].append((time.perf_counter() - t) * 1e3 / n)
    res = dict(batch_max=bmax, reps=reps, ms_per_shot={k: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for k, v in T.items()})
    print(json.dumps(res))
    if out:
        json.dump(res, open(out, "w"), indent=1)


def kernel():
    sys.path.insert(0, HERE)
    import torch
    import parallel_finite_difference_computation_amd as F
    ctx = F.FDWave(8, N, N, NB, NB, 40, 0.75, 10.0, 10.0, 1.0e-3, compat=False, device=0)
    assert ctx.steps_per_pass() == 4
    dev = torch.device("cuda:0")
    bufs = [0.01 * torch.randn((N, ctx.pitch), device=dev) for _ in range(4)]
    v2 = torch.full((N, ctx.pitch), 2000.0 ** 2, device=dev)
    il = torch.zeros((N, ctx.pitch), device=dev)
    rec = torch.zeros((40, N - 2 * NB), device=dev)
    srce = torch.zeros(40, device=dev)
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() for b in bufs]
    ip, ipp = ctx.dev_illum_steps(ptrs, v2.data_ptr(), srce.data_ptr(), N // 2, NB + 2, il.data_ptr(), 0, 40)
    torch.cuda.synchronize()
    ctx.dev_record_illum_steps(ptrs, v2.data_ptr(), srce.data_ptr(), N // 2, NB + 2, NB + 3, rec.data_ptr(), il.data_ptr(), 0, 40, True, ip, ipp)
    torch.cuda.synchronize()


def parse(dirs, out):
    res = {}
    for f in glob.glob(os.path.join(dirs[0], "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f, newline="")):
            for k in ("fdw_stepn_illum_kernel", "fdw_stepn_rec_illum_kernel"):
                if k + "<" in r["Name"] or k + "I" in r["Name"]:
                    res.setdefault(k, {}).update(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2), min_us=round(float(r["MinNs"]) / 1e3, 2),
                                                 max_us=round(float(r["MaxNs"]) / 1e3, 2))
    for d, ctr, scale in ((dirs[1], "FETCH_SIZE", 2048.0), (dirs[2], "WRITE_SIZE", 1024.0)):      # KiB; a 128-B read request is tallied as 64 B on gfx950
        acc = collections.defaultdict(list)
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(f, newline="")):
                if r["Counter_Name"] == ctr:
                    for k in ("fdw_stepn_illum_kernel", "fdw_stepn_rec_illum_kernel"):
                        if k + "<" in r["Kernel_Name"] or k + "I" in r["Kernel_Name"]:
                            acc[k].append(float(r["Counter_Value"]) * scale)
        for k, v in acc.items():
            res.setdefault(k, {})[ctr + "_bytes_per_point_step"] = round(statistics.mean(v) / (N * N * 4.0), 3)
            res[k][ctr + "_dispatches"] = len(v)
    for k, v in res.items():
        if "FETCH_SIZE_bytes_per_point_step" in v and "WRITE_SIZE_bytes_per_point_step" in v:
            v["bytes_per_point_step"] = round(v["FETCH_SIZE_bytes_per_point_step"] + v["WRITE_SIZE_bytes_per_point_step"], 3)
    print(json.dumps(res))
    if out:
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("what", choices=("shots", "batch", "kernel", "parse"))
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.what == "shots":
        shots(os.path.abspath(a.tree), a.reps, a.out)
    elif a.what == "batch":
        batch(a.reps, a.out)
    elif a.what == "kernel":
        kernel()
    else:
        parse(a.dirs, a.out)

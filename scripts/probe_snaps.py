#!/usr/bin/env python3
"""The cost of wavefield snapshots on one MI355X.

    python3 scripts/probe_snaps.py shots [--out FILE]
        whole 8192^2 shots of 500 steps (order 8, 64-cell borders, full extents: the setting of bench.py --workload rtm-slab) through fdw_shot
        and fdw_shot_snaps, same build, alternating windows, D = 8, K = 100 and K = 50; the images are compared bitwise first
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 scripts/probe_snaps.py kernel
        50 launches of fdw_snapshot_kernel at 8192^2 with D = 1, then 50 with D = 8 (a profiler run of its own: kernel tracing only)
    python3 scripts/probe_snaps.py parse DIR [--out FILE]
        the per-frame kernel times of that trace beside the bytes the kernel moves"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, NB, NT, DEC = 8192, 64, 500, 8


def shots(out):
    import numpy as np
    import parallel_finite_difference_computation_amd as F
    ctx = F.FDWave(8, N, N, NB, NB, NT, 0.75, 10.0, 10.0, 1.0e-3, compat=False, device=0)
    nx = N - 2 * NB
    vel = (1500.0 + 2000.0 * np.arange(N, dtype=np.float32)[None, :] / (N - 1) + np.zeros((N, 1), np.float32)).astype(np.float32)
    v2 = np.ascontiguousarray(vel * vel)
    srce = F.ricker_wavelet(NT, 1.0e-3, 20.0)
    d_obs = np.random.default_rng(1).standard_normal((nx, NT)).astype(np.float32)
    sx, sz, gz = N // 2, NB + 2, NB + 3
    print("steps per pass", ctx.steps_per_pass(), "backward pipeline", F.lib().fdw_back_pipe_active(ctx._h), flush=True)

    def plain():
        t = time.perf_counter()
        img = ctx.shot(v2, sx, sz, gz, srce, d_obs)
        return time.perf_counter() - t, img

    def snaps(K):
        t = time.perf_counter()
        got = ctx.shot_snaps(v2, sx, sz, gz, srce, d_obs, K, DEC)
        return time.perf_counter() - t, got

    _, img0 = plain()
    for K in (100, 50):
        _, got = snaps(K)
        assert np.array_equal(got["image"].view(np.uint32), img0.view(np.uint32)), K
        print("K", K, "frames", got["snaps"].shape, "image identical", flush=True)
    T = {"plain": [], "K100": [], "K50": []}
    for r in range(5):
        T["plain"].append(plain()[0])
        T["K100"].append(snaps(100)[0])
        T["plain"].append(plain()[0])
        T["K50"].append(snaps(50)[0])
        print("round", r, {k: round(v[-1] * 1e3, 2) for k, v in T.items()}, flush=True)
    med = {k: statistics.median(v) for k, v in T.items()}
    res = dict(n=N, nt=NT, dec=DEC, ms={k: [round(x * 1e3, 3) for x in v] for k, v in T.items()}, median_ms={k: round(v * 1e3, 3) for k, v in med.items()},
               plain_spread_pct=round(100 * (max(T["plain"]) - min(T["plain"])) / med["plain"], 2),
               overhead_pct={k: round(100 * (med[k] / med["plain"] - 1), 2) for k in ("K100", "K50")})
    print(json.dumps(res))
    if out:
        json.dump(res, open(out, "w"), indent=1)


def kernel():
    import torch
    import parallel_finite_difference_computation_amd as F
    ctx = F.FDWave(8, N, N, NB, NB, 1, 0.75, 10.0, 10.0, 1.0e-3, compat=False, device=0)
    field = torch.randn((N, ctx.pitch), device="cuda:0")
    frame = torch.zeros((N - 2 * NB) ** 2, device="cuda:0")
    torch.cuda.synchronize()
    for dec in (1, 8):
        for _ in range(50):
            ctx.dev_snapshot(field.data_ptr(), dec, frame.data_ptr())
        torch.cuda.synchronize()


def parse(trace_dir, out):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f, newline="")):
            if "fdw_snapshot_kernel" in r.get("Kernel_Name", ""):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    if len(rows) != 100:
        sys.exit(f"expected the 100 launches of `probe_snaps.py kernel`, found {len(rows)}")
    us = [(e - s) / 1e3 for s, e in rows]
    nx = N - 2 * NB
    res = {}
    for name, part, dec in (("D1", us[:50], 1), ("D8", us[50:], 8)):
        nxs = -(-nx // dec)
        med = statistics.median(part)
        res[name] = dict(median_us=round(med, 2), min_us=round(min(part), 2), max_us=round(max(part), 2), frame_bytes=nxs * nxs * 4,
                         read_bytes_requested=nxs * nxs * 4, rows_touched_bytes=nxs * nx * 4, GBps_requested=round(2 * nxs * nxs * 4 / med / 1e3, 1))
    print(json.dumps(res))
    if out:
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("what", choices=("shots", "kernel", "parse"))
    ap.add_argument("trace_dir", nargs="?")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.what == "shots":
        shots(a.out)
    elif a.what == "kernel":
        kernel()
    else:
        parse(a.trace_dir or ".", a.out)

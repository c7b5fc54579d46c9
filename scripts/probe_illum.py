#!/usr/bin/env python3
"""Cost of the source illumination.  Every GPU step is a child process under its own `timeout`; the first one that
fails ends the probe.

    python3 scripts/probe_illum.py [--parent-tree DIR] [--quick] [--profile | --profile-only] [--out DIR]        one JSON line per measurement on stdout

  * bench.py of the parent commit (--parent-tree: a built checkout of it; its own bench.py, package and library) and of this tree,
    alternating: with illumination off the headline must sit inside the parent's own run-to-run spread;
  * 8192^2 x 1000 steps and 16384^2 x 200 steps, EXACT and FAST, medians of repeated event-timed windows, the variants alternating in one
    process: fdw_dev_steps2 through the pipeline and one step per launch (what a user of the parent has to run to see every time level),
    fdw_dev_illum_steps through the pipeline, the two-step and the one-step illumination kernels;
  * --profile: one rocprofv3 --kernel-trace --stats run of the illumination loop at 8192^2 and two counter runs of their own (FETCH_SIZE,
    then WRITE_SIZE: together they exceed what one pass can collect; HBM bytes per point and step), written under DIR/prof_illum8192/ (--out DIR; default: the system's temporary directory).

    python3 scripts/probe_illum.py --child N NSTEPS NUMERICS WINDOWS [illum-only]      (what the children run)"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def child(n, nsteps, numerics, windows, illum_only):
    import torch

    import parallel_finite_difference_computation_amd as F
    dev = torch.device("cuda:0")
    ts = torch.cuda.Stream()          # a real stream: a NULL handle would send the launches to the context's own stream
    torch.cuda.set_stream(ts)
    nb = 40
    ctx = F.FDWave(8, n, n, nb, nb, nsteps, 0.75, 10.0, 10.0, 0.001, compat=True, device=0, numerics=numerics)
    pitch = ctx.pitch
    g = torch.Generator(device=dev).manual_seed(1)
    bufs = [torch.zeros((n, pitch), device=dev) for _ in range(4)]
    bufs[0][:, nb:n - nb] = 1e-3 * torch.randn((n, n - 2 * nb), device=dev, generator=g)
    v2 = torch.zeros((n, pitch), device=dev)
    v2[:, :n] = (1500.0 + 2500.0 * torch.rand((n, n), device=dev, generator=g)) ** 2
    srce = torch.zeros(nsteps, device=dev)
    il = torch.zeros((n, pitch), device=dev)
    ptrs, stream = [b.data_ptr() for b in bufs], ts.cuda_stream
    plain = lambda: ctx.dev_steps2(ptrs, v2.data_ptr(), srce.data_ptr(), n // 2, nb + 5, 0, nsteps, True, 0, 1, stream=stream)
    illum = lambda: ctx.dev_illum_steps(ptrs, v2.data_ptr(), srce.data_ptr(), n // 2, nb + 5, il.data_ptr(), 0, nsteps, True, 0, 1, stream=stream)

    def window(fn, two_step):
        ctx.set_tuning(two_step=two_step)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    variants = [("illum_pipeline", illum, 0)] if illum_only else [
        ("steps2_pipeline", plain, 0), ("steps2_one_step", plain, -1), ("illum_pipeline", illum, 0), ("illum_two_step", illum, 1), ("illum_one_step", illum, -1)]
    torch.cuda.synchronize()
    for _, fn, tb in variants:
        window(fn, tb)
    t = {name: [] for name, _, _ in variants}
    for _ in range(windows):
        for name, fn, tb in variants:
            t[name].append(window(fn, tb))
    pts = float(n) * n * nsteps
    out = dict(case=f"{n}^2 x {nsteps} steps", numerics="FAST" if numerics else "EXACT", windows=windows)
    for name in t:
        m = statistics.median(t[name])
        out[name] = dict(us_per_step=round(m * 1e3 / nsteps, 2), gpts=round(pts / m / 1e6, 1), min_ms=round(min(t[name]), 2), max_ms=round(max(t[name]), 2))
    if not illum_only:
        out["illum_pipeline_vs_steps2_pipeline"] = round(out["illum_pipeline"]["us_per_step"] / out["steps2_pipeline"]["us_per_step"], 3)
        out["illum_pipeline_vs_parent_one_step_loop"] = round(out["illum_pipeline"]["us_per_step"] / out["steps2_one_step"]["us_per_step"], 3)
    print(json.dumps(out), flush=True)


def run(cmd, limit, env=None, cwd=None, log=None):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env, cwd=cwd)
    if log:
        open(log, "w").write(r.stdout + r.stderr)
    if r.returncode != 0:
        sys.exit(f"[probe_illum] {' '.join(cmd)} failed (rc {r.returncode}); nothing more is started\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return r.stdout


def main():
    quick, me = "--quick" in sys.argv, os.path.abspath(__file__)
    parent = sys.argv[sys.argv.index("--parent-tree") + 1] if "--parent-tree" in sys.argv else None
    if parent and "--profile-only" not in sys.argv:
        tail = ["--gpus", "1"] + (["--steps", "200", "--warmup", "20"] if quick else [])
        vals = {"parent": [], "this": []}
        for _ in range(1 if quick else 2):
            for who in ("parent", "this"):
                env = {k: v for k, v in os.environ.items() if k not in ("FDW_LIB", "PYTHONPATH")}
                tree = os.path.abspath(parent) if who == "parent" else ROOT
                line = [ln for ln in run(["python3", os.path.join(tree, "bench.py")] + tail, 600, env=env, cwd=tree).splitlines() if ln.startswith("{") and '"metric"' in ln][-1]
                d = json.loads(line)
                vals[who].append(d["value"])
                print(json.dumps(dict(bench=who, value=d["value"], unit=d["unit"], ms_per_step=d["ms_per_step"], steps=d["steps"])), flush=True)
        print(json.dumps(dict(bench_summary=vals, parent_spread=[min(vals["parent"]), max(vals["parent"])], this_spread=[min(vals["this"]), max(vals["this"])])), flush=True)
    windows = "3" if quick else "7"
    for n, nsteps in ((8192, 1000), (16384, 200)) if "--profile-only" not in sys.argv else ():
        for numerics in (0, 1):
            sys.stdout.write(run(["python3", me, "--child", str(n), str(nsteps), str(numerics), windows], 300))
            sys.stdout.flush()
    if "--profile" in sys.argv or "--profile-only" in sys.argv:
        base = os.path.abspath(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else tempfile.gettempdir()
        out, tmp = os.path.join(base, "prof_illum8192"), tempfile.gettempdir()
        os.makedirs(out, exist_ok=True)
        tail = ["--", "python3", me, "--child", "8192", "200", "0", "2", "illum-only"]
        fmt = ["--output-format", "csv"]
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.join(out, "trace")] + fmt + tail, 300, cwd=tmp, log=os.path.join(out, "trace.log"))
        for i, ctr in enumerate(("FETCH_SIZE", "WRITE_SIZE")):      # one counter group per pass
            run(["rocprofv3", "--pmc", ctr, "-d", os.path.join(out, f"pmc{i}")] + fmt + tail, 300, cwd=tmp, log=os.path.join(out, f"pmc{i}.log"))
        stats = glob.glob(os.path.join(out, "trace", "**", "*kernel_stats.csv"), recursive=True)
        if stats:
            open(os.path.join(out, "kernel_stats.csv"), "w").write(open(stats[0]).read())
        agg = {}
        for f in glob.glob(os.path.join(out, "pmc[01]", "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if "illum" in row["Kernel_Name"]:
                    a = agg.setdefault(row["Kernel_Name"].split("(")[0], {}).setdefault(row["Counter_Name"], [0.0, 0])
                    a[0] += float(row["Counter_Value"])
                    a[1] += 1
        for k, c in agg.items():
            rd = c.get("FETCH_SIZE", [0, 1])[0] / max(c.get("FETCH_SIZE", [0, 1])[1], 1) * 1024 * 2      # KiB; x 2 on gfx950 (scripts/profile_bench.py)
            wr = c.get("WRITE_SIZE", [0, 1])[0] / max(c.get("WRITE_SIZE", [0, 1])[1], 1) * 1024
            print(json.dumps(dict(kernel=k, dispatches=c.get("FETCH_SIZE", [0, 0])[1], read_MB_per_launch=round(rd / 1e6, 1), write_MB_per_launch=round(wr / 1e6, 1),
                                  hbm_bytes_per_point_and_step=round((rd + wr) / (8192.0 * 8192.0 * 4), 2))), flush=True)


if __name__ == "__main__":
    if "--child" in sys.argv:
        a = sys.argv[sys.argv.index("--child") + 1:]
        child(int(a[0]), int(a[1]), int(a[2]), int(a[3]), len(a) > 4)
    else:
        main()

#!/usr/bin/env python3
"""Born modelling (fdwave.h, "Born modelling"): microseconds per step of the fused loop, of the unfused arrangement and of two plain loops.

    python3 scripts/bench_born.py --parent-root DIR [--sizes 8192,2048] [--steps 200] [--warmup 20] [--repeats 5] [--out profiles/born.json]

Order 8, EXACT and FAST, FDW_BORN_DTT, two_step = -1, from noise-filled fields with the source in the interior.  Per size and numerics:
  fused     fdw_dev_born_steps (fdw_step_born_kernel: 36 B/point/step -- u p and pp, du p and pp, v2, m in; u and du out);
  unfused   the same call in a process started with FDW_NO_BORN_FUSED=1: the scattered step, (A - B) into the scratch field, the
            background step, the scatter kernel (16 + 12 + 16 + 24 = 68 B/point/step on the interior: two steps, the difference's two reads
            and one write, the scatter's five reads and one write);
  two_plain fdw_dev_steps on one pair and then on another, two_step = -1 (32 B/point/step), taken from a BUILD OF THE PARENT COMMIT
            (--parent-root: a checkout of it with its library built), not from the tree under test.
Each figure: a worker process per build and arrangement, in it `repeats` windows of `steps` steps after `warmup` steps, timed with two
events on the stream the loops run on, the median of the windows.  The byte model expects fused = 36/32 = 1.125 x two_plain.  Out of scope
here as in the library: Born kernels in the two-step and four-step families, slabs (batches and line sources: --batch, below).

Measured on one MI355X: see profiles/born.json and DESIGN.md section 6t.

    python3 scripts/bench_born.py --batch --parent-root DIR [--shots 32] [--sizes 2048,8192] [--out profiles/born_batch.json]

Batches and line sources (fdwave.h, the sub-section after "Born modelling").  Two measurements:
  batch     the reference's own deck size (415 x 295 interior, borders of 40, nt 1700), order 8, FDW_BORN_DTT, border models drawn on the
            device, `shots` shots: ms per shot (host wall clock around the synchronous call, median of `repeats` windows after one warm-up
            window) through fdw_born_shot_batch on this tree against fdw_born_shot one by one on the BUILD OF THE PARENT COMMIT; beside it,
            taken in the same run on this tree, the yardstick: fdw_record_shot_batch against fdw_record_shot one by one.
  line      us per step of fdw_dev_born_line_steps on this tree against fdw_dev_born_steps on the parent's build, at --sizes, as above;
            the difference is reported against the spread of the windows."""
import argparse
import json
import os
import statistics
import subprocess
import sys

NB = 16


def worker(args):
    sys.path.insert(0, args.root)
    import numpy as np
    import torch

    import parallel_finite_difference_computation_amd as F
    assert os.path.abspath(os.path.dirname(F.__file__)).startswith(os.path.abspath(args.root)), F.__file__
    dev = torch.device("cuda:0")
    for size in args.size_list:
        for numerics in (0, 1):
            nt = args.steps + args.warmup
            ctx = F.FDWave(8, size, size, NB, NB, nt, 0.75, 10.0, 10.0, 0.001, compat=False, numerics=numerics)
            ctx.set_tuning(two_step=-1)
            g = torch.Generator(device=dev).manual_seed(1)
            f = [0.01 * torch.randn((size, ctx.pitch), device=dev, generator=g) for _ in range(4)]
            v2 = (1500.0 + 1500.0 * torch.rand((size, ctx.pitch), device=dev, generator=g)) ** 2
            m = 0.1 * torch.randn((size, ctx.pitch), device=dev, generator=g)
            srce = torch.from_numpy(np.asarray(F.ricker_wavelet(nt, 0.001, 20.0)) * 10.0).to(dev)
            rec = torch.zeros((nt, size - 2 * NB), device=dev)
            ts = torch.cuda.Stream()
            torch.cuda.set_stream(ts)
            s = ts.cuda_stream
            sx, sz, gz = size // 2, size // 2, NB + 1
            p = [t.data_ptr() for t in f]

            def born(it0, n):
                ctx.dev_born_steps(p[0], p[1], p[2], p[3], v2.data_ptr(), m.data_ptr(), 1, srce.data_ptr(), sx, sz, gz, rec.data_ptr(), None, it0, n,
                                   first_pp_twice=True, stream=s)

            wav = torch.randn((nt, size - 2 * NB), device=dev, generator=g) if args.worker == "line" else None

            def line(it0, n):
                ctx.dev_born_line_steps(p[0], p[1], p[2], p[3], v2.data_ptr(), m.data_ptr(), 1, wav.data_ptr(), sz, gz, rec.data_ptr(), None, it0, n,
                                        first_pp_twice=True, stream=s)

            def two_plain(it0, n):
                ctx.dev_steps(p[0], p[1], v2.data_ptr(), srce.data_ptr(), sx, sz, it0, n, first_pp_twice=True, stream=s)
                ctx.dev_steps(p[2], p[3], v2.data_ptr(), srce.data_ptr(), sx, sz, it0, n, first_pp_twice=True, stream=s)
            fn = two_plain if args.worker == "two_plain" else (line if args.worker == "line" else born)
            w = []
            for _ in range(args.repeats):
                fn(0, args.warmup)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(args.warmup, args.steps)
                e1.record()
                torch.cuda.synchronize()
                w.append(e0.elapsed_time(e1) / args.steps * 1e3)
            torch.cuda.set_stream(torch.cuda.default_stream())
            print(json.dumps(dict(what=args.worker, size=size, numerics="fast" if numerics else "exact", us_per_step=round(statistics.median(w), 2),
                                  windows_us=[round(x, 2) for x in w])), flush=True)
            ctx.close()
            del f, v2, m, rec
            torch.cuda.empty_cache()


BATCH_DECK = (415, 295, 40, 40, 1700)      # nx, nz, nxb, nzb, nt: the reference's new_mod deck


def batch_worker(args):
    """batch_new (this tree): fdw_born_shot_batch, fdw_record_shot_batch, fdw_record_shot one by one; batch_parent: fdw_born_shot one by one."""
    import time

    sys.path.insert(0, args.root)
    import numpy as np

    import parallel_finite_difference_computation_amd as F
    assert os.path.abspath(os.path.dirname(F.__file__)).startswith(os.path.abspath(args.root)), F.__file__
    nx, nz, nxb, nzb, nt = BATCH_DECK
    n = args.shots
    rng = np.random.default_rng(1)
    vp = (1500.0 + 2000.0 * np.linspace(0, 1, nz, dtype=np.float32)[None, :] + 100.0 * rng.standard_normal((nx, nz))).astype(np.float32)
    m = (0.1 * rng.standard_normal((nx, nz))).astype(np.float32)
    srce = F.ricker_wavelet(nt, 0.001, 20.0)
    sx0, dsx, sz, gz = nxb + 20, (nx - 40) // max(n, 1), nzb + 2, nzb + 1
    for numerics in (0, 1):
        ctx = F.FDWave(8, nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, numerics=numerics)
        ctx.model_resident(vp)
        T = ctx.border_draws()

        def born_single():
            for b in range(n):
                ctx.dev_extendvel_linear(b * T)
                ctx.born_shot(None, m, sx0 + b * dsx, sz, gz, srce, kind=1)

        def record_single():
            for b in range(n):      # a batch of one: the border model of its draws, then fdw_record_shot's own code
                ctx.record_shot_batch(1, sx0 + b * dsx, dsx, sz, gz, srce, draw_offset=b * T)

        def born_batch():
            ctx.born_shot_batch(n, m, sx0, dsx, sz, gz, srce, kind=1)
            assert ctx.batch_parts() == 1, ctx.batch_parts()

        def record_batch():
            ctx.record_shot_batch(n, sx0, dsx, sz, gz, srce)
            assert ctx.batch_parts() == 1, ctx.batch_parts()

        todo = dict(born_single=born_single) if args.worker == "batch_parent" else dict(born_batch=born_batch, record_batch=record_batch, record_single=record_single)
        for name, fn in todo.items():
            w = []
            for k in range(args.repeats + 1):
                t0 = time.perf_counter()
                fn()
                if k:
                    w.append((time.perf_counter() - t0) / n * 1e3)
            print(json.dumps(dict(what=name, numerics="fast" if numerics else "exact", ms_per_shot=round(statistics.median(w), 3),
                                  windows_ms=[round(x, 3) for x in w], shots=n, batch_max=ctx.shot_batch_max())), flush=True)
        ctx.close()


def run_worker(here, which, root, args, extra, limit=300):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, here, "--worker", which, "--root", root, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--repeats", str(args.repeats)] + extra
    e = {k: v for k, v in os.environ.items() if k not in ("FDW_NO_BORN_FUSED", "FDW_NO_SHOT_BATCH", "FDW_BATCH_BUDGET_BYTES")}
    r = subprocess.run(cmd, capture_output=True, text=True, env=e)
    if r.returncode != 0:
        raise SystemExit(f"worker {which} ({root}) failed with status {r.returncode}: nothing more is started\n{r.stdout}\n{r.stderr}")
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def batch_main(here, this_root, args):
    parent = os.path.abspath(args.parent_root)
    rows = {}
    for which, root in (("batch_parent", parent), ("batch_new", this_root)):
        for d in run_worker(here, which, root, args, ["--shots", str(args.shots)]):
            rows.setdefault(d["numerics"], {})[d["what"]] = d
    batch = {}
    for num, d in rows.items():
        ms = {k: d[k]["ms_per_shot"] for k in ("born_batch", "born_single", "record_batch", "record_single")}
        batch[num] = dict(ms_per_shot=ms, windows_ms={k: d[k]["windows_ms"] for k in ms}, born_single_over_batch=round(ms["born_single"] / ms["born_batch"], 3),
                          record_single_over_batch=round(ms["record_single"] / ms["record_batch"], 3), born_batch_is_faster=ms["born_batch"] < ms["born_single"],
                          batch_max=d["born_batch"]["batch_max"])
    lines = {}
    for which, root in (("fused", parent), ("line", this_root)):
        for d in run_worker(here, which, root, args, ["--sizes", args.sizes]):
            lines.setdefault(f"{d['size']}^2 {d['numerics']}", {})["point_parent" if which == "fused" else "line"] = d
    line = {}
    for key, d in lines.items():
        a, b = d["line"], d["point_parent"]
        spread = max(max(x["windows_us"]) - min(x["windows_us"]) for x in (a, b))
        line[key] = dict(us_per_step=dict(line=a["us_per_step"], point_parent=b["us_per_step"]), windows_us=dict(line=a["windows_us"], point_parent=b["windows_us"]),
                         difference_us=round(a["us_per_step"] - b["us_per_step"], 2), window_spread_us=round(spread, 2))
    nx, nz, nxb, nzb, nt = BATCH_DECK
    res = dict(method=f"batch: {nx} x {nz} interior, borders {nxb} / {nzb}, nt {nt}, order 8, FDW_BORN_DTT, {args.shots} shots on device-drawn border models, host wall "
                      f"clock per call, median of {args.repeats} windows after one warm-up window; born_single on a build of the parent commit, the other three on "
                      f"this tree in one process.  line: order 8, FDW_BORN_DTT, two_step = -1, {args.steps} steps after {args.warmup} of warm-up per window, median of "
                      f"{args.repeats} windows; point_parent = fdw_dev_born_steps on the parent's build",
               batch=batch, line=line)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(batch={k: (v["ms_per_shot"], v["born_single_over_batch"], v["record_single_over_batch"]) for k, v in batch.items()},
                          line={k: (v["us_per_step"], v["difference_us"], v["window_spread_us"]) for k, v in line.items()}), indent=1), flush=True)


def main():
    here = os.path.abspath(__file__)
    this_root = os.path.abspath(os.path.join(os.path.dirname(here), ".."))
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="8192,2048")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None, help="default: profiles/born.json, with --batch profiles/born_batch.json")
    ap.add_argument("--batch", action="store_true", help="batches of shots and the line loop (profiles/born_batch.json) instead of the fused / unfused table")
    ap.add_argument("--shots", type=int, default=32)
    ap.add_argument("--worker", choices=["fused", "unfused", "two_plain", "line", "batch_parent", "batch_new"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=this_root, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.size_list = [int(x) for x in args.sizes.split(",") if x]
    if args.worker:
        return batch_worker(args) if args.worker.startswith("batch_") else worker(args)
    if not args.parent_root:
        ap.error("--parent-root is needed: the two plain loops (--batch: the one-by-one Born shots) are timed on a build of the parent commit")
    if args.out is None:
        args.out = os.path.join(this_root, "profiles", "born_batch.json" if args.batch else "born.json")
    if args.batch:
        return batch_main(here, this_root, args)
    rows = {}
    for which, root, env in (("two_plain", os.path.abspath(args.parent_root), {}), ("fused", this_root, {}), ("unfused", this_root, dict(FDW_NO_BORN_FUSED="1"))):
        cmd = ["timeout", "-k", "10", "300", sys.executable, here, "--worker", which, "--root", root, "--sizes", args.sizes, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
        e = {k: v for k, v in os.environ.items() if k != "FDW_NO_BORN_FUSED"}
        e.update(env)
        r = subprocess.run(cmd, capture_output=True, text=True, env=e)
        if r.returncode != 0:
            raise SystemExit(f"worker {which} ({root}) failed with status {r.returncode}: nothing more is started\n{r.stdout}\n{r.stderr}")
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                rows.setdefault(f"{d['size']}^2 {d['numerics']}", {})[which] = d
    table = {}
    for key, d in rows.items():
        us = {k: d[k]["us_per_step"] for k in ("fused", "unfused", "two_plain")}
        table[key] = dict(us_per_step=us, windows_us={k: d[k]["windows_us"] for k in us}, fused_over_two_plain=round(us["fused"] / us["two_plain"], 4),
                          unfused_over_two_plain=round(us["unfused"] / us["two_plain"], 4), fused_beats_unfused=us["fused"] < us["unfused"])
    res = dict(method=f"order 8, FDW_BORN_DTT, two_step = -1; {args.steps} steps after {args.warmup} of warm-up per window, median of {args.repeats} windows, "
                      "one worker process per arrangement; two_plain on a build of the parent commit", byte_model=dict(fused=36, two_plain=32, unfused=68),
               results=table)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["us_per_step"], v["fused_over_two_plain"]) for k, v in table.items()}, indent=1), flush=True)


if __name__ == "__main__":
    main()

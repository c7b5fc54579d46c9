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
here as in the library: Born kernels in the two-step and four-step families, batches, line sources, slabs.

Measured on one MI355X: see profiles/born.json and DESIGN.md section 6t."""
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

            def two_plain(it0, n):
                ctx.dev_steps(p[0], p[1], v2.data_ptr(), srce.data_ptr(), sx, sz, it0, n, first_pp_twice=True, stream=s)
                ctx.dev_steps(p[2], p[3], v2.data_ptr(), srce.data_ptr(), sx, sz, it0, n, first_pp_twice=True, stream=s)
            fn = two_plain if args.worker == "two_plain" else born
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


def main():
    here = os.path.abspath(__file__)
    this_root = os.path.abspath(os.path.join(os.path.dirname(here), ".."))
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="8192,2048")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(this_root, "profiles", "born.json"))
    ap.add_argument("--worker", choices=["fused", "unfused", "two_plain"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=this_root, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.size_list = [int(x) for x in args.sizes.split(",") if x]
    if args.worker:
        return worker(args)
    if not args.parent_root:
        ap.error("--parent-root is needed: the two plain loops are timed on a build of the parent commit")
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

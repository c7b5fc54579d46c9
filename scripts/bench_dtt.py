#!/usr/bin/env python3
"""DTT imaging (fdwave.h, "DTT imaging"): the one-step backward loop with the DTT epilogue against the cross-correlation loop of the parent.

    python3 scripts/bench_dtt.py --parent-root DIR [--sizes 8192,2048] [--steps 100] [--warmup 10] [--repeats 3] [--rounds 3] [--out profiles/dtt.json]

Order 8, EXACT and FAST, two_step = -1, noise-filled source and receiver pairs, iterations with step_source = 1.  Per size and numerics:
  parent   fdw_dev_back_iter on a BUILD OF THE PARENT COMMIT (--parent-root: a checkout of it with its library built): the yardstick;
  dtt      fdw_dev_back_iter_dtt on this tree (fdw_step_back_dtt_kernel); both move 36 B/point (r p and pp, F p and pp, v2, img in; r, F, img out);
  xcorr    fdw_dev_back_iter on this tree (the kernel the parent runs, rebuilt): what the rebuild alone changes.
A worker process per build and round, the builds interleaved round by round in one session; in a worker `repeats` windows of `steps`
iterations after `warmup`, timed with two events on the stream the loop runs on.  Per figure the median over all windows of all rounds; the
spread is max - min of the parent's own windows.  Acceptance (the issue): dtt / parent within that spread plus 5 %.

Whole shots (this tree, one process): a 500-step fdw_shot_dtt against fdw_shot at the first of --sizes (fdw_shot's backward loop runs the
four-step pipeline there; the DTT loop runs one-step iterations), host wall clock around the synchronous call; and the reference's deck size
(415 x 295 interior, borders 40, nt 1700), `shots` shots on device-drawn border models, fdw_shot_batch_dtt against fdw_shot_batch, ms per
shot.  Measured on one MI355X: profiles/dtt.json and DESIGN.md section 6v."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

NB = 16
BATCH_DECK = (415, 295, 40, 40, 1700)      # nx, nz, nxb, nzb, nt: the reference's new_mod deck


def iter_worker(args):
    sys.path.insert(0, args.root)
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
            img = torch.zeros((size, ctx.pitch), device=dev)
            samples = torch.randn((nt, size - 2 * NB), device=dev, generator=g)
            ts = torch.cuda.Stream()
            torch.cuda.set_stream(ts)
            s = ts.cuda_stream
            call = ctx.dev_back_iter_dtt if args.worker == "dtt" else ctx.dev_back_iter
            p = [t.data_ptr() for t in f]
            state = dict(k=0)

            def loop(n):
                for _ in range(n):
                    k = state["k"]
                    a, b = (p[0], p[1]) if k % 2 == 0 else (p[1], p[0])
                    c, d = (p[2], p[3]) if k % 2 == 0 else (p[3], p[2])
                    call(1, a, b, c, d, v2.data_ptr(), 0, size, True, samples[k % nt].data_ptr(), NB + 1, img.data_ptr(), stream=s)
                    state["k"] = k + 1
            w = []
            for _ in range(args.repeats):
                loop(args.warmup)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loop(args.steps)
                e1.record()
                torch.cuda.synchronize()
                w.append(e0.elapsed_time(e1) / args.steps * 1e3)
            torch.cuda.set_stream(torch.cuda.default_stream())
            print(json.dumps(dict(what=args.worker, size=size, numerics="fast" if numerics else "exact", windows_us=[round(x, 2) for x in w])), flush=True)
            ctx.close()
            del f, v2, img, samples
            torch.cuda.empty_cache()


def shot_worker(args):
    sys.path.insert(0, args.root)
    import numpy as np

    import parallel_finite_difference_computation_amd as F
    size, nt = args.size_list[0], 500
    rng = np.random.default_rng(1)
    for numerics in (0, 1):
        ctx = F.FDWave(8, size, size, NB, NB, nt, 0.75, 10.0, 10.0, 0.001, compat=False, numerics=numerics)
        v2 = ((1500.0 + 1500.0 * rng.random((size, size), dtype=np.float32)) ** 2).astype(np.float32)
        srce = F.ricker_wavelet(nt, 0.001, 20.0)
        d_obs = rng.standard_normal((size - 2 * NB, nt), dtype=np.float32)
        place = (size // 2, NB + 2, NB + 1)
        out = {}
        for name, fn in (("shot", lambda: ctx.shot(v2, *place, srce, d_obs)), ("shot_dtt", lambda: ctx.shot_dtt(v2, *place, srce, d_obs))):
            w = []
            for k in range(args.repeats + 1):
                t0 = time.perf_counter()
                fn()
                if k:
                    w.append(time.perf_counter() - t0)
            out[name] = dict(s_per_shot=round(statistics.median(w), 4), windows_s=[round(x, 4) for x in w])
        print(json.dumps(dict(what="shot", size=size, nt=nt, numerics="fast" if numerics else "exact", back_pipe=ctx.back_pipe_active() if hasattr(ctx, "back_pipe_active") else None,
                              **out)), flush=True)
        ctx.close()
    nx, nz, nxb, nzb, nt = BATCH_DECK
    n = args.shots
    vp = (1500.0 + 2000.0 * np.linspace(0, 1, nz, dtype=np.float32)[None, :] + 100.0 * rng.standard_normal((nx, nz))).astype(np.float32)
    srce = F.ricker_wavelet(nt, 0.001, 20.0)
    d_obs = rng.standard_normal((n, nx, nt), dtype=np.float32)
    sx0, dsx, sz, gz = nxb + 20, (nx - 40) // max(n, 1), nzb + 2, nzb + 1
    for numerics in (0, 1):
        ctx = F.FDWave(8, nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, numerics=numerics)
        ctx.model_resident(vp)
        out = {}
        for name, fn in (("shot_batch", lambda: ctx.shot_batch(n, sx0, dsx, sz, gz, srce, d_obs)), ("shot_batch_dtt", lambda: ctx.shot_batch_dtt(n, sx0, dsx, sz, gz, srce, d_obs))):
            w = []
            for k in range(args.repeats + 1):
                t0 = time.perf_counter()
                fn()
                assert ctx.batch_parts() == 1, ctx.batch_parts()
                if k:
                    w.append((time.perf_counter() - t0) / n * 1e3)
            out[name] = dict(ms_per_shot=round(statistics.median(w), 3), windows_ms=[round(x, 3) for x in w])
        print(json.dumps(dict(what="batch", shots=n, numerics="fast" if numerics else "exact", **out)), flush=True)
        ctx.close()


def run_worker(here, which, root, args, limit=300):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, here, "--worker", which, "--root", root, "--sizes", args.sizes, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--shots", str(args.shots)]
    e = {k: v for k, v in os.environ.items() if k not in ("FDW_NO_FUSED_BACK", "FDW_NO_SHOT_BATCH", "FDW_BATCH_BUDGET_BYTES")}
    r = subprocess.run(cmd, capture_output=True, text=True, env=e)
    if r.returncode != 0:
        raise SystemExit(f"worker {which} ({root}) failed with status {r.returncode}: nothing more is started\n{r.stdout}\n{r.stderr}")
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    here = os.path.abspath(__file__)
    this_root = os.path.abspath(os.path.join(os.path.dirname(here), ".."))
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", default="8192,2048")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shots", type=int, default=32)
    ap.add_argument("--no-shots", action="store_true", help="the iteration table alone")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(this_root, "profiles", "dtt.json"))
    ap.add_argument("--worker", choices=["parent", "dtt", "xcorr", "shots"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=this_root, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.size_list = [int(x) for x in args.sizes.split(",") if x]
    if args.worker:
        return shot_worker(args) if args.worker == "shots" else iter_worker(args)
    if not args.parent_root:
        ap.error("--parent-root is needed: the yardstick is timed on a build of the parent commit")
    windows = {}
    for _ in range(args.rounds):      # the builds interleaved, round by round
        for which, root in (("parent", os.path.abspath(args.parent_root)), ("dtt", this_root), ("xcorr", this_root)):
            for d in run_worker(here, which, root, args):
                windows.setdefault(f"{d['size']}^2 {d['numerics']}", {}).setdefault(which, []).extend(d["windows_us"])
    table = {}
    for key, w in windows.items():
        us = {k: round(statistics.median(v), 2) for k, v in w.items()}
        spread = (max(w["parent"]) - min(w["parent"])) / us["parent"]
        ratio = us["dtt"] / us["parent"]
        table[key] = dict(us_per_iteration=us, windows_us=w, dtt_over_parent=round(ratio, 4), xcorr_over_parent=round(us["xcorr"] / us["parent"], 4),
                          parent_window_spread=round(spread, 4), bound=round(1.0 + spread + 0.05, 4), within_bound=ratio <= 1.0 + spread + 0.05)
    res = dict(method=f"order 8, two_step = -1, step_source = 1; {args.steps} iterations after {args.warmup} of warm-up per window, {args.repeats} windows per worker, "
                      f"{args.rounds} rounds of (parent, dtt, xcorr) workers interleaved in one session; medians over all windows; parent = fdw_dev_back_iter on a build "
                      "of the parent commit; bound = 1 + the parent's window spread + 0.05", byte_model=dict(dtt=36, parent=36), iterations=table)
    if not args.no_shots:
        rows = run_worker(here, "shots", this_root, args, limit=900)
        res["shots"] = [d for d in rows if d["what"] == "shot"]
        res["batches"] = [d for d in rows if d["what"] == "batch"]
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["us_per_iteration"], v["dtt_over_parent"], v["bound"], v["within_bound"]) for k, v in table.items()}, indent=1), flush=True)
    for d in res.get("shots", []) + res.get("batches", []):
        print(json.dumps(d), flush=True)


if __name__ == "__main__":
    main()

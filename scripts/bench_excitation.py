#!/usr/bin/env python3
"""What excitation-amplitude imaging costs against the cross-correlation shot.

    python3 scripts/bench_excitation.py [--size 8192] [--steps 500] [--warmup 20] [--repeats 5] [--shot-repeats 3] [--out profiles/excitation.json]

Per numerics (EXACT, FAST), order 8 on a size^2 grid, one process, nothing else on the GPU:

  0. a check before anything is timed: over 8 steps from noise fields the automatic path (on a large grid the four-step pipeline kernels)
     equals the one-step family (two_step=-1) bit for bit on amp, texc and exc;
  1. the forward loop plain (fdw_dev_steps2, one band: the excitation loops use no pass bands), with illumination (fdw_dev_illum_steps) and
     with the excitation maps (fdw_dev_excite_steps); the line loop plain (fdw_dev_line_steps) and with the pick (fdw_dev_line_pick_steps).
     The variants alternate on the same buffers; a window is `steps` steps after `warmup`, timed with events on one stream; the median of
     `repeats` windows is reported in us per step, with the bytes per point and step the loop must move at least;
  2. whole shots of `steps` time steps: fdw_shot against fdw_shot_excitation, wall time, alternating, median of `shot-repeats`;
  3. the same shot comparison on the new_mod deck size (415 x 295 extended, nt 1700).

    python3 scripts/bench_excitation.py --image-on-device --parent-root DIR [--size 8192] [--steps 500] [--rounds 3]

The whole shot since the image is formed on the device, against the build of the PARENT commit in the same sitting: DIR
is a checkout of the parent with its library built.  The check of step 0 runs first; then worker processes alternate, parent build and this
build, `rounds` times each; a worker warms up, then times fdw_shot, fdw_shot_excitation with all four outputs and (this build)
fdw_shot_excitation with imloc alone, on size^2 and on the new_mod deck size, EXACT and FAST; the medians over the rounds go under the key
"image_on_device" of --out, with a breakdown of this build's imloc-only shot at size^2: the two device loops and the image kernels timed
with events on device arrays, the rest being uploads and the one download.
Development tool, not part of the suite."""
import argparse
import json
import os
import statistics
import sys
import time

# --root DIR (the workers of --image-on-device): the tree whose package and library this process loads
ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import parallel_finite_difference_computation_amd as F  # noqa: E402

NB = 64


def make_state(ctx, size, nt, seed=1):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(seed)
    bufs = [torch.randn((size, ctx.pitch), device=dev, generator=gen) * 1e-3 for _ in range(4)]
    for b in bufs:
        b[:, size:] = 0
    v2 = torch.zeros((size, ctx.pitch), device=dev)
    v2[:, :size] = (1500.0 + 2500.0 * torch.rand((size, size), device=dev, generator=gen)) ** 2
    srce = torch.randn(nt, device=dev, generator=gen) * 1e-3
    wav = torch.randn((nt, size - 2 * NB), device=dev, generator=gen) * 1e-3
    return bufs, v2, srce, wav


def check_paths(size, numerics):
    """amp, texc and exc of the automatic path against the one-step family over 8 steps; raises if a word differs."""
    dev = torch.device("cuda:0")
    nsteps = 8
    out = {}
    for name, tuning in (("auto", {}), ("one-step", dict(two_step=-1))):
        ctx = F.FDWave(8, size, size, NB, NB, nsteps, 0.75, 10.0, 10.0, 0.001, compat=False, numerics=numerics)
        ctx.set_tuning(**tuning)
        bufs, v2, srce, wav = make_state(ctx, size, nsteps)
        gen = torch.Generator(device=dev).manual_seed(7)
        amp = torch.randn((size, ctx.pitch), device=dev, generator=gen) * 1e-5
        texc = torch.randint(-1, nsteps + 3, (size, ctx.pitch), device=dev, generator=gen, dtype=torch.int32)
        exc = torch.randn((size, ctx.pitch), device=dev, generator=gen)
        ptrs = [b.data_ptr() for b in bufs]
        torch.cuda.synchronize()                              # the loops run on the context's own stream, unordered against torch's
        ctx.dev_excite_steps(ptrs, v2.data_ptr(), srce.data_ptr(), size // 2, NB + 2, amp.data_ptr(), texc.data_ptr(), 0, nsteps)
        torch.cuda.synchronize()
        texc_maps = texc.clone()
        texc.copy_(torch.randint(-1, nsteps + 3, (size, ctx.pitch), device=dev, generator=gen, dtype=torch.int32))
        torch.cuda.synchronize()
        ip, ipp = ctx.dev_line_pick_steps(ptrs, v2.data_ptr(), wav.data_ptr(), NB + 2, texc.data_ptr(), nsteps, exc.data_ptr(), 0, nsteps)
        torch.cuda.synchronize()
        out[name] = (amp.view(torch.int32), texc_maps, exc.view(torch.int32), bufs[ipp].view(torch.int32), ctx.steps_per_pass())
    for i, what in enumerate(("amp", "texc", "exc", "the newest field")):
        if not torch.equal(out["auto"][i], out["one-step"][i]):
            raise SystemExit(f"numerics {numerics}: {what} of the automatic path differs from the one-step family")
    return out["auto"][4]


def loops(size, steps, warmup, repeats, numerics):
    dev = torch.device("cuda:0")
    nt = steps + warmup
    ctx = F.FDWave(8, size, size, NB, NB, nt, 0.75, 10.0, 10.0, 0.001, compat=False, numerics=numerics)
    ctx.set_pass_bands(1, 1)                                # the plain loop as the other loops run it: no row bands
    bufs, v2, srce, wav = make_state(ctx, size, nt)
    acc = torch.zeros((size, ctx.pitch), device=dev)
    amp = torch.zeros((size, ctx.pitch), device=dev)
    texc = torch.zeros((size, ctx.pitch), device=dev, dtype=torch.int32)
    exc = torch.zeros((size, ctx.pitch), device=dev)
    ptrs = [b.data_ptr() for b in bufs]
    st = {"ip": 0, "ipp": 1}
    ts = torch.cuda.Stream()
    torch.cuda.set_stream(ts)
    s = ts.cuda_stream
    sx, sz = size // 2, NB + 2

    def keep(r):
        st["ip"], st["ipp"] = r
    fns = {
        "forward_plain": lambda it0, n: keep(ctx.dev_steps2(ptrs, v2.data_ptr(), srce.data_ptr(), sx, sz, it0, n, True, st["ip"], st["ipp"], stream=s)),
        "forward_illum": lambda it0, n: keep(ctx.dev_illum_steps(ptrs, v2.data_ptr(), srce.data_ptr(), sx, sz, acc.data_ptr(), it0, n, True, st["ip"],
                                                                   st["ipp"], stream=s)),
        "forward_maps": lambda it0, n: keep(ctx.dev_excite_steps(ptrs, v2.data_ptr(), srce.data_ptr(), sx, sz, amp.data_ptr(), texc.data_ptr(), it0, n, True,
                                                                   st["ip"], st["ipp"], stream=s)),
        "line_plain": lambda it0, n: keep(ctx.dev_line_steps(ptrs, v2.data_ptr(), wav.data_ptr(), sz, it0, n, first_pp_twice=True, ip=st["ip"], ipp=st["ipp"],
                                                              stream=s)),
        "line_pick": lambda it0, n: keep(ctx.dev_line_pick_steps(ptrs, v2.data_ptr(), wav.data_ptr(), sz, texc.data_ptr(), nt, exc.data_ptr(), it0, n, True,
                                                                  st["ip"], st["ipp"], stream=s)),
    }

    def window(fn):
        fn(0, warmup)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(warmup, steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3          # us per step

    t = {k: [] for k in fns}
    for _ in range(repeats):                                # alternating: drift of the clocks hits all alike
        for k, fn in fns.items():
            t[k].append(window(fn))
    torch.cuda.set_stream(torch.cuda.default_stream())
    spp = ctx.steps_per_pass()
    # bytes per point and step a loop moves at least: a pass reads p, pp, v2 and writes its last two levels (20 B per pass of spp steps;
    # the one-step kernel 16 B per step); illumination + 8 B, the maps + 16 B (amp and texc, in and out), the pick + 12 B (texc and exc in,
    # exc out), each per pass
    base = 20.0 / spp if spp > 1 else 16.0
    model = dict(forward_plain=base, line_plain=base, forward_illum=base + 8.0 / spp, forward_maps=base + 16.0 / spp, line_pick=base + 12.0 / spp)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(numerics="fast" if numerics else "exact", size=size, steps=steps, steps_per_pass=spp,
               us_per_step={k: round(v, 2) for k, v in med.items()}, windows_us={k: [round(x, 2) for x in v] for k, v in t.items()},
               min_bytes_per_point_step={k: round(v, 2) for k, v in model.items()},
               effective_GBps={k: round(model[k] * size * size / (med[k] * 1e-6) / 1e9, 1) for k in med},
               ratio_maps_over_plain=round(med["forward_maps"] / med["forward_plain"], 4),
               ratio_maps_over_illum=round(med["forward_maps"] / med["forward_illum"], 4),
               ratio_pick_over_line=round(med["line_pick"] / med["line_plain"], 4))
    print(json.dumps(out), flush=True)
    return out


def shots(nxe, nze, nb, nt, repeats, numerics, what, image_alone=False):
    rng = np.random.default_rng(3)
    ctx = F.FDWave(8, nxe, nze, nb, nb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, numerics=numerics)
    nx = nxe - 2 * nb
    v2 = ((1500.0 + 2500.0 * rng.random((nxe, nze))) ** 2).astype(np.float32)
    srce = F.ricker_wavelet(nt, 0.001, 25.0)
    d_obs = (1e-3 * rng.standard_normal((nx, nt))).astype(np.float32)
    sx, sz, gz = nxe // 2, nb + 2, nb + 1

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def xcorr():
        ctx.shot(v2, sx, sz, gz, srce, d_obs)

    def excitation():
        ctx.shot_excitation(v2, sx, sz, gz, srce, d_obs)

    def image_only():
        ctx.shot_excitation(v2, sx, sz, gz, srce, d_obs, want_maps=False)
    fns = {"fdw_shot": xcorr, "fdw_shot_excitation": excitation}
    if image_alone:
        fns["fdw_shot_excitation_imloc_only"] = image_only
    for fn in fns.values():                                # warm-up: allocations, first launches
        fn()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(what=what, numerics="fast" if numerics else "exact", grid=[nxe, nze], nt=nt, steps_per_pass=ctx.steps_per_pass(),
               ms={k: round(v, 2) for k, v in med.items()}, runs_ms={k: [round(x, 2) for x in v] for k, v in t.items()},
               ratio_excitation_over_shot=round(med["fdw_shot_excitation"] / med["fdw_shot"], 4))
    print(json.dumps(out), flush=True)
    return out


def breakdown(size, steps, numerics):
    """This build's imloc-only shot at size^2 in parts: the forward loop with the maps and the line loop with the pick over `steps` steps from
    rest, and fdw_dev_image_excitation, each timed with events on device arrays (ms)."""
    dev = torch.device("cuda:0")
    ctx = F.FDWave(8, size, size, NB, NB, steps, 0.75, 10.0, 10.0, 0.001, compat=True, numerics=numerics)
    bufs, v2, srce, wav = make_state(ctx, size, steps)
    amp = torch.zeros((size, ctx.pitch), device=dev)
    texc = torch.zeros((size, ctx.pitch), device=dev, dtype=torch.int32)
    exc = torch.zeros((size, ctx.pitch), device=dev)
    img = torch.zeros((size, ctx.pitch), device=dev)
    ptrs = [b.data_ptr() for b in bufs]
    ts = torch.cuda.Stream()
    s = ts.cuda_stream

    def timed(fn):
        torch.cuda.synchronize()
        with torch.cuda.stream(ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    out = {}
    for _ in range(2):                                      # the second pass is the one reported
        out["forward_maps_ms"] = timed(lambda: ctx.dev_excite_steps(ptrs, v2.data_ptr(), srce.data_ptr(), size // 2, NB + 2, amp.data_ptr(), texc.data_ptr(), 0,
                                                                   steps, stream=s))
        out["line_pick_ms"] = timed(lambda: ctx.dev_line_pick_steps(ptrs, v2.data_ptr(), wav.data_ptr(), NB + 1, texc.data_ptr(), steps, exc.data_ptr(), 0, steps,
                                                                   stream=s))
        out["image_kernels_ms"] = timed(lambda: ctx.dev_image_excitation(exc.data_ptr(), amp.data_ptr(), 1e-3, img.data_ptr(), stream=s))
    out = dict(what=f"{size}^2 breakdown", numerics="fast" if numerics else "exact", **{k: round(v, 2) for k, v in out.items()})
    print(json.dumps(out), flush=True)
    return out


def worker(args):
    """One process of --image-on-device: JSON lines on stdout."""
    if args.worker == "check":
        for numerics in (0, 1):
            print(json.dumps(dict(check=True, numerics=numerics, steps_per_pass_auto=check_paths(args.size, numerics))), flush=True)
        return
    this = args.worker == "this"
    for numerics in (0, 1):
        shots(args.size, args.size, NB, args.steps, 1, numerics, f"{args.size}^2", image_alone=this)
        shots(415, 295, 50, 1700, 3, numerics, "new_mod deck size", image_alone=this)
    if this and args.with_breakdown:
        for numerics in (0, 1):
            breakdown(args.size, args.steps, numerics)


def image_on_device(args):
    import subprocess
    here = os.path.abspath(__file__)
    this_root = os.path.abspath(os.path.join(os.path.dirname(here), ".."))

    def run(which, root, extra=()):
        cmd = ["timeout", "-k", "10", "300", sys.executable, here, "--worker", which, "--root", root, "--size", str(args.size), "--steps", str(args.steps)] + list(extra)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"worker {which} ({root}) failed with status {r.returncode}: nothing more is started\n{r.stdout}\n{r.stderr}")
        return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    checks = run("check", this_root)
    print(json.dumps(checks), flush=True)
    rows = {}
    parts = []
    for r in range(args.rounds):
        for which, root in (("parent", os.path.abspath(args.parent_root)), ("this", this_root)):
            for line in run(which, root, ["--with-breakdown"] if r == args.rounds - 1 else []):
                if "ms" in line:
                    for k, v in line["ms"].items():
                        rows.setdefault((line["what"], line["numerics"], which + ":" + k), []).append(v)
                else:
                    parts.append(line)
    table = {}
    for (what, numerics, k), v in sorted(rows.items()):
        table.setdefault(what, {}).setdefault(numerics, {})[k] = dict(median_ms=round(statistics.median(v), 2), runs_ms=v)
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    res["image_on_device"] = dict(method=f"worker processes alternating between the parent's build and this build, {args.rounds} rounds; median of the rounds; "
                                         f"{args.steps} steps at {args.size}^2, 1700 steps on the new_mod deck size (a worker's own median of 3 there)",
                                  checks=checks, ms=table, breakdown_this_build=parts)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["image_on_device"]["ms"], indent=1), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shot-repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "excitation.json"))
    ap.add_argument("--image-on-device", action="store_true", help="the whole shot of this build against the parent's build (see the module docstring)")
    ap.add_argument("--parent-root", default=None, help="--image-on-device: a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--worker", choices=["check", "parent", "this"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--with-breakdown", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.image_on_device:
        if not args.parent_root:
            ap.error("--image-on-device needs --parent-root")
        return image_on_device(args)
    res = dict(device=torch.cuda.get_device_name(0), checks=[], loops=[], shots=[])
    for numerics in (0, 1):
        spp = check_paths(args.size, numerics)
        res["checks"].append(dict(numerics="fast" if numerics else "exact", steps=8, steps_per_pass_auto=spp,
                                  auto_equals_one_step_on=["amp", "texc", "exc", "newest field"]))
        print(json.dumps(res["checks"][-1]), flush=True)
    for numerics in (0, 1):
        res["loops"].append(loops(args.size, args.steps, args.warmup, args.repeats, numerics))
    for numerics in (0, 1):
        res["shots"].append(shots(args.size, args.size, NB, args.steps, args.shot_repeats, numerics, f"{args.size}^2"))
    for numerics in (0, 1):
        res["shots"].append(shots(415, 295, 50, 1700, args.shot_repeats, numerics, "new_mod deck size"))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

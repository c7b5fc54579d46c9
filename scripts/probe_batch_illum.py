#!/usr/bin/env python3
"""Cost of the illumination in a batch of shots and of trace recording on a slab (section 6f).  Every GPU step is a
child process under its own `timeout`; the first one that fails ends the probe.

    python3 scripts/probe_batch_illum.py [--parent-tree DIR] [--reps N] [--only batch|slabs]        one JSON line per measurement on stdout

  * new_mod's size (415 x 295 with its borders of 50, nt = 1700, order 8, EXACT, host models as its vel_ext_file deck gives them): ms per
    shot of fdw_shot_batch_illum and of plain fdw_shot_batch at nshots = 6 and at fdw_shot_batch_max(), against fdw_shot_illum one by one --
    the only way of the parent commit (--parent-tree: a built checkout of it; its own package and library), measured there and here in
    alternating child processes.  Medians over the repetitions, minimum and maximum stated;
  * one rank of an N-way decomposition of the 8192^2 grid with the links stubbed (scripts/probe_slabs_c.py), N = 2 and 8: us per step of
    fdw_slabs_dev_forward against fdw_slabs_dev_record_forward, alternating in one process; the plain figure also on the parent tree.

    python3 scripts/probe_batch_illum.py --child-batch TREE | --child-slabs TREE REPS      (what the children run)"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def child_batch(tree):
    sys.path.insert(0, tree)
    import numpy as np

    import parallel_finite_difference_computation_amd as F
    nxe, nze, nb, nt = 415, 295, 50, 1700
    nx, nz = nxe - 2 * nb, nze - 2 * nb
    ctx = F.FDWave(8, nxe, nze, nb, nb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    bmax = ctx.shot_batch_max()
    rng = np.random.default_rng(1)
    srce = F.ricker_wavelet(nt, 0.001, 20.0)
    v2 = ((1500 + 2500 * rng.random((bmax, nxe, nze))) ** 2).astype(np.float32)
    d_obs = rng.standard_normal((bmax, nx, nt)).astype(np.float32)
    have_batch_illum = hasattr(F.lib(), "fdw_shot_batch_illum")
    sx0, ds, sz, gz = nb + 7, 300 // max(bmax, 6), nb, nb

    def one_by_one(n):
        for s in range(n):
            ctx.shot(v2[s], sx0 + s * ds, sz, gz, srce, d_obs[s], want_illum=True)

    def batch(n, illum):
        if illum:
            ctx.shot_batch(n, sx0, ds, sz, gz, srce, d_obs[:n], v2_all=v2[:n], want_illum=True)
        else:
            ctx.shot_batch(n, sx0, ds, sz, gz, srce, d_obs[:n], v2_all=v2[:n])

    out = dict(tree=tree, batch_max=bmax)
    for n in (6, bmax):
        variants = [("one_by_one_illum", lambda: one_by_one(n)), ("batch_plain", lambda: batch(n, False))]
        if have_batch_illum:
            variants.append(("batch_illum", lambda: batch(n, True)))
        for name, fn in variants:
            fn()                                          # allocations, first launches
            t0 = time.perf_counter()
            fn()
            out[f"{name}@{n}"] = (time.perf_counter() - t0) * 1e3 / n      # ms per shot, uploads and downloads included
    print(json.dumps(out), flush=True)


def child_slabs(tree, reps):
    sys.path.insert(0, tree)
    import torch

    import parallel_finite_difference_computation_amd as F
    dev = torch.device("cuda:0")
    n, K, NB = 8192, 320, 64
    out = dict(tree=tree)
    for world in (2, 8):
        comm = F.Comm.stub(world // 2, world)
        sl = F.Slabs(8, n, n, NB, NB, K, 0.75, 10.0, 10.0, 1e-3, comm=comm, compat=False, ksteps=0)
        fl = [1e-3 * torch.randn((sl.nxl, sl.pitch), device=dev) for _ in range(sl.nbuf)]
        for f in fl:
            f[:, n:] = 0
        v2 = torch.zeros((sl.nxl, sl.pitch), device=dev)
        v2[:, :n] = 2500.0 ** 2
        srce = torch.zeros(K, device=dev)
        rec = torch.zeros((K, n - 2 * NB), device=dev)
        ptrs = [f.data_ptr() for f in fl]
        torch.cuda.synchronize()
        variants = [("forward", lambda: sl.dev_forward(ptrs, v2.data_ptr(), srce.data_ptr(), n // 2, n // 2, 0, K, True, 0, 1))]
        if hasattr(sl, "dev_record_forward"):
            variants.append(("record_forward", lambda: sl.dev_record_forward(ptrs, v2.data_ptr(), srce.data_ptr(), n // 2, n // 2, NB + 3, rec.data_ptr(), 0, K, True, 0, 1)))
        t = {name: [] for name, _ in variants}
        for rep in range(reps + 1):
            for name, fn in variants:
                t0 = time.perf_counter()
                fn()
                sl.synchronize()
                if rep > 0:                               # repetition 0 warms up
                    t[name].append((time.perf_counter() - t0) / K * 1e6)
        for name in t:
            out[f"{name}@N={world}"] = dict(us_per_step=round(statistics.median(t[name]), 2), min=round(min(t[name]), 2), max=round(max(t[name]), 2),
                                            rows=sl.own1 - sl.own0, ksteps=sl.ksteps, nbuf=sl.nbuf)
        sl.close()
        comm.close()
    print(json.dumps(out), flush=True)


def run(cmd, limit):
    env = {k: v for k, v in os.environ.items() if k not in ("FDW_LIB", "PYTHONPATH")}
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.exit(f"[probe_batch_illum] {' '.join(cmd)} failed (rc {r.returncode}); nothing more is started\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    me = os.path.abspath(__file__)
    parent = os.path.abspath(sys.argv[sys.argv.index("--parent-tree") + 1]) if "--parent-tree" in sys.argv else None
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    trees = ([("parent", parent)] if parent else []) + [("this", ROOT)]
    if only in (None, "batch"):
        samples = {}
        for _ in range(reps):
            for who, tree in trees:                       # alternating
                d = run(["python3", me, "--child-batch", tree], 300)
                for k, v in d.items():
                    if "@" in k:
                        samples.setdefault((who, k), []).append(v)
                bmax = d["batch_max"]
        for (who, k), v in sorted(samples.items()):
            print(json.dumps(dict(tree=who, variant=k, ms_per_shot=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), reps=len(v))), flush=True)
        base = "parent" if parent else "this"
        for n in (6, bmax):
            ref, got = samples[(base, f"one_by_one_illum@{n}")], samples[("this", f"batch_illum@{n}")]
            spread = max(max(ref) - min(ref), max(got) - min(got))
            print(json.dumps(dict(nshots=n, one_by_one_tree=base, one_by_one_ms_per_shot=round(statistics.median(ref), 3),
                                  batch_illum_ms_per_shot=round(statistics.median(got), 3), spread_ms=round(spread, 3),
                                  batch_wins_by_more_than_the_spread=statistics.median(ref) - statistics.median(got) > spread,
                                  batch_plain_ms_per_shot=round(statistics.median(samples[("this", f"batch_plain@{n}")]), 3))), flush=True)
    if only in (None, "slabs"):
        for who, tree in trees:
            d = run(["python3", me, "--child-slabs", tree, str(reps)], 600)
            d["tree"] = who
            print(json.dumps(d), flush=True)


if __name__ == "__main__":
    if "--child-batch" in sys.argv:
        child_batch(sys.argv[sys.argv.index("--child-batch") + 1])
    elif "--child-slabs" in sys.argv:
        i = sys.argv.index("--child-slabs")
        child_slabs(sys.argv[i + 1], int(sys.argv[i + 2]))
    else:
        main()

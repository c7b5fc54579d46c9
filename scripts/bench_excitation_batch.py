#!/usr/bin/env python3
"""What a batch of excitation-amplitude shots gains on a small deck.

    python3 scripts/bench_excitation_batch.py [--nx 415] [--nz 295] [--nb 50] [--nt 1700] [--shots 32] [--repeats 3] [--out profiles/excitation_batch.json]

One process, order 8, EXACT and FAST, a deck of the new_mod size (nx x nz interior, borders nb), `shots` shots on one host model with a gather
each.  Four ways through the same shots, alternating, wall time, median of `repeats`, in ms per shot:

    fdw_shot one by one            fdw_shot_batch (one launch per time step for all shots)
    fdw_shot_excitation one by one (imloc alone: one download per shot)
    fdw_shot_excitation_batch      (with the running images, as rtm_code takes them)

Before anything is timed the batch's image and running images are compared bit for bit with the shots one by one, and fdw_batch_parts is
asserted to be 1 for both batched calls.  Development tool, not part of the suite."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402

import parallel_finite_difference_computation_amd as F  # noqa: E402


def run(nx, nz, nb, nt, ns, repeats, numerics):
    nxe, nze = nx + 2 * nb, nz + 2 * nb
    rng = np.random.default_rng(3)
    ctx = F.FDWave(8, nxe, nze, nb, nb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, numerics=numerics)
    v2 = ((1500.0 + 2500.0 * rng.random((nxe, nze))) ** 2).astype(np.float32)
    v2_all = np.broadcast_to(v2, (ns, nxe, nze)).copy()
    srce = F.ricker_wavelet(nt, 0.001, 25.0)
    d_obs = (1e-3 * rng.standard_normal((ns, nx, nt))).astype(np.float32)
    sx0, dsx, sz, gz = nb + 20, max(1, (nx - 40) // ns), nb + 2, nb + 1

    def shot_one_by_one():
        for b in range(ns):
            ctx.shot(v2, sx0 + b * dsx, sz, gz, srce, d_obs[b])

    def shot_batch():
        ctx.shot_batch(ns, sx0, dsx, sz, gz, srce, d_obs, v2_all=v2_all)

    def excitation_one_by_one():
        img, stack = None, []
        for b in range(ns):
            img = ctx.shot_excitation(v2, sx0 + b * dsx, sz, gz, srce, d_obs[b], 1e-3, img, want_maps=False)[0]
            stack.append(img)
        return img, np.stack(stack)

    def excitation_batch():
        r = ctx.shot_excitation_batch(ns, sx0, dsx, sz, gz, srce, d_obs, 1e-3, v2_all=v2_all, want_maps=False)
        return r["image"], r["stack"]
    fns = {"fdw_shot": shot_one_by_one, "fdw_shot_batch": shot_batch, "fdw_shot_excitation": excitation_one_by_one,
           "fdw_shot_excitation_batch": excitation_batch}
    # warm-up and the check: the same bytes
    shot_one_by_one()
    shot_batch()
    parts = {"fdw_shot_batch": ctx.batch_parts()}
    a, b = excitation_one_by_one(), excitation_batch()
    parts["fdw_shot_excitation_batch"] = ctx.batch_parts()
    if not (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))):
        raise SystemExit(f"numerics {numerics}: the batch differs from the shots one by one")
    if parts != {"fdw_shot_batch": 1, "fdw_shot_excitation_batch": 1}:
        raise SystemExit(f"the batched calls did not take the batch whole: {parts}")
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3 / ns)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(numerics="fast" if numerics else "exact", interior=[nx, nz], border=nb, nt=nt, shots=ns, batch_equals_one_by_one=True, batch_parts=parts,
               shot_batch_max=ctx.shot_batch_max(), ms_per_shot={k: round(v, 3) for k, v in med.items()},
               runs_ms_per_shot={k: [round(x, 3) for x in v] for k, v in t.items()},
               ratio_excitation_batch_over_one_by_one=round(med["fdw_shot_excitation_batch"] / med["fdw_shot_excitation"], 4),
               ratio_excitation_batch_over_shot_batch=round(med["fdw_shot_excitation_batch"] / med["fdw_shot_batch"], 4))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--nx", type=int, default=415)
    ap.add_argument("--nz", type=int, default=295)
    ap.add_argument("--nb", type=int, default=50)
    ap.add_argument("--nt", type=int, default=1700)
    ap.add_argument("--shots", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "excitation_batch.json"))
    args = ap.parse_args()
    res = dict(runs=[run(args.nx, args.nz, args.nb, args.nt, args.shots, args.repeats, numerics) for numerics in (0, 1)])
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of trace recording: fdw_dev_steps2 against fdw_dev_record_steps on the same buffers, alternating, each the median of repeated
event-timed windows (8192^2 x 1000 steps, 16384^2 x 200 steps, EXACT; 8192^2 FAST); then bin/rtm_model and bin/rtm_code on the reference's
new_mod deck (six shots; fixtures from tests/golden), wall time, and fdw_record_shot_batch of those six shots in process.

    python3 scripts/probe_record.py [--quick]          one JSON line per case on stdout"""
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import parallel_finite_difference_computation_amd as F  # noqa: E402

dev = torch.device("cuda:0")
ts = torch.cuda.Stream()          # a real stream: a NULL stream handle would send the library's launches to its context's own stream
torch.cuda.set_stream(ts)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def steps_case(n, nsteps, windows, numerics=0):
    nb = 40
    ctx = F.FDWave(8, n, n, nb, nb, nsteps, 0.75, 10.0, 10.0, 0.001, compat=True, device=0, numerics=numerics)
    pitch = ctx.pitch
    g = torch.Generator(device=dev).manual_seed(1)
    bufs = [torch.zeros((n, pitch), device=dev) for _ in range(4)]
    bufs[0][:, nb:n - nb] = 1e-3 * torch.randn((n, n - 2 * nb), device=dev, generator=g)
    v2 = torch.zeros((n, pitch), device=dev)
    v2[:, :n] = (1500.0 + 2500.0 * torch.rand((n, n), device=dev, generator=g)) ** 2
    srce = torch.zeros(nsteps, device=dev)
    rec = torch.zeros((nsteps, n - 2 * nb), device=dev)
    ptrs = [b.data_ptr() for b in bufs]
    stream = ts.cuda_stream
    plain = lambda: ctx.dev_steps2(ptrs, v2.data_ptr(), srce.data_ptr(), n // 2, nb + 5, 0, nsteps, True, 0, 1, stream=stream)
    recd = lambda: ctx.dev_record_steps(ptrs, v2.data_ptr(), srce.data_ptr(), n // 2, nb + 5, nb + 10, rec.data_ptr(), 0, nsteps, True, 0, 1, stream=stream)
    torch.cuda.synchronize()
    window(plain)
    window(recd)
    a, b = [], []
    for _ in range(windows):
        a.append(window(plain))
        b.append(window(recd))
    ma, mb = statistics.median(a), statistics.median(b)
    out = dict(case=f"{n}^2 x {nsteps} steps", numerics="FAST" if numerics else "EXACT", steps_per_pass=ctx.steps_per_pass(), windows=windows,
               dev_steps2_ms=round(ma, 3), dev_record_steps_ms=round(mb, 3), us_per_step=[round(1e3 * ma / nsteps, 2), round(1e3 * mb / nsteps, 2)],
               overhead_pct=round(100.0 * (mb - ma) / ma, 2), spread_pct=[round(100.0 * (max(a) - min(a)) / ma, 1), round(100.0 * (max(b) - min(b)) / mb, 1)])
    del bufs, v2, rec, ctx
    torch.cuda.empty_cache()
    return out


def new_mod_case(runs):
    golden = os.path.join(ROOT, "tests", "golden")
    bin_dir = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin")
    vel = np.load(os.path.join(golden, "new_mod_vel_ext_rnd6.npz"))["vel"]
    walls = {"rtm_model": [], "rtm_code": []}
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "models", "new_mod")
        os.makedirs(d)
        os.makedirs(os.path.join(tmp, "output"))
        shutil.copy(os.path.join(golden, "decks", "new_mod.dat"), os.path.join(d, "input.dat"))
        shutil.copy(os.path.join(golden, "new_mod_vel_koslov.f32"), os.path.join(d, "vel-koslov.1"))
        vel.tofile(os.path.join(d, "vel_ext_rnd.6"))
        for _ in range(runs):
            for exe in ("rtm_model", "rtm_code"):
                t0 = time.perf_counter()
                r = subprocess.run([os.path.join(bin_dir, exe), "./models/new_mod/input.dat"], cwd=tmp, capture_output=True, text=True, timeout=300)
                walls[exe].append(time.perf_counter() - t0)
                assert r.returncode == 0, r.stderr
    ctx = F.FDWave(8, 415, 295, 50, 50, 1700, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    srce = F.ricker_wavelet(1700, 0.001, 20.0)
    v2 = (vel * vel).astype(np.float32)
    ctx.record_shot_batch(6, 57, 60, 50, 50, srce, v2_all=v2)
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ctx.record_shot_batch(6, 57, 60, 50, 50, srce, v2_all=v2)
        t.append(time.perf_counter() - t0)
    return dict(case="new_mod deck, 6 shots x 1700 steps", runs=runs, rtm_model_wall_s=round(statistics.median(walls["rtm_model"]), 3),
                rtm_code_wall_s=round(statistics.median(walls["rtm_code"]), 3), record_shot_batch_s=round(statistics.median(t), 4),
                batch=ctx.shot_batch_max())


if __name__ == "__main__":
    quick = "--quick" in sys.argv
    for n, nsteps, w, num in [(8192, 1000, 3 if quick else 9, 0), (16384, 200, 3 if quick else 9, 0), (8192, 1000, 3 if quick else 5, 1)]:
        print(json.dumps(steps_case(n, nsteps, w, num)), flush=True)
    print(json.dumps(new_mod_case(2 if quick else 3)), flush=True)

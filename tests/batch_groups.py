"""What the program tests of GROUPED shots share.  rtm_code, rtm_model and mod_main walk their shots in groups of fdw_shot_batch_max; on every
test deck that is 32 to 64, so each loop runs once.  FDW_BATCH_BUDGET_BYTES (fdwave.h, fdw_set_batch_budget) brings it down to 2: five shots
then go through as groups {0, 1}, {2, 3}, {4}, and under FDW_TIMING the programs say on stderr how many shots a launch sequence takes."""
import functools
import os
import subprocess
import tempfile
from pathlib import Path

import numpy as np

import parallel_finite_difference_computation_amd as F
from conftest import ROOT
from oracle import oracle as O

BIN = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin")
NS, DS, FSX, SZ, GZ = 5, 11, 5, 1, 2      # the five-shot deck: source rows 5, 16, .. 49 of 61, depths as tests/test_programs.py has them
GROUP_FIELDS = 30      # fdw_shot_batch_max = 30 / 11 = 2; the parts inside the library (up to 12.5 fields per shot) come out at 2 as well


def group_env(nxe, nze, nxb, nzb, nt, fac=0.75, dialect=0):
    """The environment under which the programs take this geometry's shots two at a time; the library confirms the arithmetic."""
    kw = dict(compat=True) if dialect == 0 else dict(dialect=dialect)
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, fac, 10.0, 10.0, 0.001, device=0, **kw)
    budget = GROUP_FIELDS * ctx.field_bytes()
    assert ctx.shot_batch_max() > 2, "without a budget the program would take the deck's shots as one group"
    ctx.set_batch_budget(budget)
    assert ctx.shot_batch_max() == 2
    ctx.close()
    return {"FDW_BATCH_BUDGET_BYTES": str(budget), "FDW_TIMING": "1"}


def assert_grouped(stderr, entry, n=2):
    """The program's own word that it grouped: `[timing] shots per launch sequence: up to 2 (<entry point>)`."""
    line = [ln for ln in stderr.splitlines() if "shots per launch sequence" in ln]
    assert len(line) == 1 and f"shots per launch sequence: up to {n} ({entry})" in line[0], stderr


def without_exec_time(stdout):
    return "\n".join(ln for ln in stdout.splitlines() if "Exec time" not in ln)


def five_shot_case(path, with_vel_ext=False, extra=""):
    """The 95 x 73 deck of tests/test_programs.py with five shots in `path`; returns (nx, nz, nxb, nzb, nt, ns, vp, d_obs, vel_ext)."""
    from test_programs import _small_rtm_case
    path.mkdir(parents=True, exist_ok=True)
    case = _small_rtm_case(path, with_vel_ext, ns=NS, ds=DS)
    with open(path / "input.dat", "a") as f:
        f.write(extra)
    return case


def run_program(exe, path, env=None, arg="./input.dat"):
    """One run of a program in `path` -> (the files of ./output as bytes, the completed process)."""
    base = {k: v for k, v in os.environ.items() if k not in ("FDW_SHOT_WORKERS", "FDW_SLABS", "FDW_GPUS", "FDW_NO_SHOT_BATCH", "FDW_HOST_BORDER",
                                                             "FDW_BATCH_BUDGET_BYTES", "FDW_TIMING")}
    r = subprocess.run([os.path.join(BIN, exe), arg], cwd=path, capture_output=True, text=True, env=dict(base, **(env or {})), timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    out = path / "output"
    return {name: (out / name).read_bytes() for name in sorted(os.listdir(out))}, r


@functools.lru_cache(maxsize=None)
def five_shot_oracle(with_vel_ext=False):
    """oracle_shots() of the five-shot deck, computed once."""
    with tempfile.TemporaryDirectory() as tmp:
        nx, nz, nxb, nzb, nt, ns, vp, d_obs, vel_ext = five_shot_case(Path(tmp) / "deck", with_vel_ext)
    out = oracle_shots(nx, nz, nxb, nzb, nt, ns, FSX, DS, SZ, GZ, vp, d_obs, vel_ext)
    for a in out.values():
        a.setflags(write=False)
    return out


def oracle_shots(nx, nz, nxb, nzb, nt, ns, fsx, ds, sz, gz, vp, d_obs, vel_ext=None, fpeak=25.0):
    """rtm_code's shot loop (R:480-529) on the oracle, shot by shot in the order of the one rand() stream: per shot the squared model, the
    gather the forward loop models (data), the illumination from zero (illum), the image of d_obs (image), resid = d_obs (-) data and its
    image (r_image); d_obs None: models, gathers and illuminations only.  sz, gz, fsx as the deck gives them (interior coordinates)."""
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    orc = O.Oracle(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True)
    xlim, zlim, _ = O.extents(nxe, nze, nzb, True)
    srce = O.ricker_wavelet(nt, 0.001, fpeak)
    vpe = np.zeros((nxe, nze), np.float32)
    vpe[nxb:nxb + nx, nzb:nzb + nz] = vp
    out = dict(v2=[], data=[], illum=[], image=[], resid=[], r_image=[])
    for s in range(ns):
        if vel_ext is not None:
            v = vel_ext[s]
        else:
            O.extendvel_linear(vpe, nx, nz, nxb, nzb, seed=1 if s == 0 else None)      # the reference never seeds rand()
            v = vpe
        v2 = (v * v).astype(np.float32)
        P = PP = None
        data = np.zeros((nx, nt), np.float32)
        il = np.zeros((nxe, nze), np.float32)
        for it in range(nt):
            P, PP = orc.forward(v2, fsx + s * ds + nxb, sz + nzb, srce[it:it + 1], P, PP)
            data[:, it] = PP[nxb:nxb + nx, gz + nzb]
            u = PP[:xlim, :zlim]
            il[:xlim, :zlim] = (il[:xlim, :zlim] + (u * u).astype(np.float32)).astype(np.float32)
        out["v2"].append(v2)
        out["data"].append(data)
        out["illum"].append(il[nxb:nxb + nx, nzb:nzb + nz].copy())
        if d_obs is not None:
            out["image"].append(orc.back(v2, P, PP, d_obs[s], gz + nzb))
            resid = (d_obs[s] - data).astype(np.float32)
            out["resid"].append(resid)
            out["r_image"].append(orc.back(v2, P, PP, resid, gz + nzb))
    return {k: np.stack(v) for k, v in out.items() if v}


def stack(per_shot):
    """The running sum in shot order (R:522-528), one rounded fp32 addition per shot."""
    total = np.zeros(per_shot.shape[1:], np.float32)
    for a in per_shot:
        total = (total + a).astype(np.float32)
    return total

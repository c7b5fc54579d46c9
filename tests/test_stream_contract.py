"""The stream contract of fdwave.h: every fdw_dev_* entry point issues every launch, copy and memset on the stream it is given and does
not synchronise (fdw_dev_check_field excepted, which is documented to); the slab drivers are ordered through fdw_slabs_stream alone.

Method: a LATE PRODUCER on the caller's stream only.  Every device input holds a DECOY -- a second, valid argument
set -- when the device is synchronised for the last time.  Then, on one torch stream S: a delay, device copies of the TRUE inputs over the
decoys, the entry point with stream = S, copies of every output.  Right after the entry point returns S.query() must be False (the call
did not synchronise, and the delay still held the inputs back when everything had been issued); after S.synchronize() the outputs must
equal the CPU oracle's answer to the TRUE inputs bit for bit.  A launch, copy or memset that lands on any other stream runs during the
delay: it reads decoys, or writes before the producer does, and the comparison fails.  The cases and their oracle answers are in
tests/stream_cases.py (CASES, the catalogue of 100, and EXC_CASES, the excitation entry points: DESIGN.md section 6s); the unmarked test below shows on the CPU that the decoys matter (the oracle's two answers differ in more than half
of the cells of every output, and no answer holds a sentinel).

The delay: torch.cuda._sleep, calibrated per module with two events.  Measured on one MI355X on the parent commit: the longest host wall
time from the first enqueue on S to the return of the entry point, over all cases, is 6.08 ms (the first case of the module; the median
is 0.07 ms) -- MEASURED_WALL_MS below; the delay is ten times that (and at least 20 ms): 60.8 ms, (r + 1) times that for rank r of a slab case.

Controls: the same construction with the producer on S and the entry point on a second stream T.  Where T completes while S is still
held by the delay -- the streams overlapped -- the outputs must DIFFER from the oracle's answer: the method sees what it looks for."""
import functools
import threading
import time

import numpy as np
import pytest

import stream_cases as SC
from conftest import assert_bit_equal, random_fields
from oracle import oracle as O
from test_line_source import args_of, line_restatement

MEASURED_WALL_MS = 6.08     # see the docstring and DESIGN.md section 6n
DELAY_MS = max(20.0, 10.0 * MEASURED_WALL_MS)
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the decoys matter
# ---------------------------------------------------------------------------------------------------------------------------------------
def _adequate(true, decoy, what, cells=None):
    """cells: {label: (rows, columns)} where a call may write only part of a label's array (Case.cells): the share is counted there."""
    assert sorted(true) == sorted(decoy), what
    for label, a in true.items():
        b = decoy[label]
        assert a.shape == b.shape and a.size > 0, (what, label)
        assert np.isfinite(a).all() and np.isfinite(b).all(), (what, label)
        where = (cells or {}).get(label, (slice(None),) * a.ndim)
        share = float((a.view(np.uint32) != b.view(np.uint32))[where].mean())
        assert share > 0.5, f"{what}: {label} of the decoys equals the true answer in {1 - share:.0%} of the cells"
        for s in SC.SENTINELS:
            assert not (a == s).any(), f"{what}: {label} holds the sentinel {s}"


ALL_CASES = SC.CASES + SC.EXC_CASES      # the 100 cases of the catalogue, then the excitation entry points


@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_the_decoys_matter(case):
    """A call that read decoys, or an output still holding its sentinel, cannot pass for the answer to the true inputs.  Where a call may
    write only part of an array (the excitation maps: the update extents; the image: the interior) the answers differ in more than half of
    THOSE cells -- the rest holds entry words, which differ between the two sets anyway."""
    _adequate(case.want("true"), case.want("decoy"), case.name, case.cells)


def test_the_check_field_plant_is_three_cells():
    i = SC.inputs("ragged", "true")
    assert np.count_nonzero(i["planted"] != i["clean"]) == 3 and not i["clean"][64:, :8].any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: single contexts
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_delay():
    import torch
    d = SC.Delay(torch)
    yield torch, d
    if SC.WALLS:
        worst = max(SC.WALLS, key=SC.WALLS.get)
        print(f"\n[stream contract] delay {DELAY_MS} ms ({'_sleep' if d.scratch is None else 'passes'}, {d.per_ms:.0f} per ms); longest host wall from "
              f"the first enqueue to the return of the entry point: {SC.WALLS[worst]:.3f} ms ({worst}); median {np.median(list(SC.WALLS.values())):.3f} ms")


def _check(run, what):
    want = run.case.want("true")
    got = run.results()
    assert sorted(got) == sorted(want), what
    for label in sorted(want):
        assert_bit_equal(got[label], want[label], f"{label}, {what}")


@gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_late_producer(case, torch_delay):
    torch, delay = torch_delay
    run = SC.Run(case, torch)
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    run.enqueue(S, delay, DELAY_MS)
    assert run.busy, f"{case.name}: the stream was idle when the entry point returned after {run.wall_ms:.2f} ms: the call synchronised, or outlasted the delay"
    S.synchronize()
    _check(run, case.name)
    run.close()


@gpu
def test_check_field_synchronises_and_counts_the_late_cells(torch_delay):
    """fdw_dev_check_field behind a late producer that plants three violating cells in a clean field: FDW_EINVAL with that count, and --
    the one documented exception -- the stream is idle afterwards."""
    import parallel_finite_difference_computation_amd as F
    torch, delay = torch_delay
    i = SC.inputs("ragged", "true")
    ctx = F.FDWave(*args_of(i["d"]), compat=True, device=0)
    nze = i["d"]["nze"]
    fld = torch.zeros((i["d"]["nxe"], ctx.pitch), device="cuda:0")
    stage = torch.zeros_like(fld)
    fld[:, :nze] = torch.from_numpy(np.array(i["clean"])).to("cuda:0")
    stage[:, :nze] = torch.from_numpy(np.array(i["planted"])).to("cuda:0")
    ctx.dev_check_field(fld.data_ptr())                 # clean: accepted (and the kernel is loaded)
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        delay(DELAY_MS)
        fld.copy_(stage, non_blocking=True)
        with pytest.raises(F.FdwError) as ei:
            ctx.dev_check_field(fld.data_ptr(), stream=S.cuda_stream)
        idle = S.query()
    assert ei.value.code == SC.EINVAL and "3 cells" in str(ei.value), str(ei.value)
    assert idle is True
    ctx.close()


@gpu
def test_two_contexts_on_two_streams(torch_delay):
    """Two contexts at once, each behind its own late producer with its own delay: each gives its own oracle answer."""
    torch, delay = torch_delay
    runs = [SC.Run(SC.BY_NAME[n], torch) for n in ("steps2-stepped-pipeline", "record-ragged-one-step", "line_rec_ill-ragged-two-step-fast")]
    streams = [torch.cuda.Stream() for _ in runs]
    torch.cuda.synchronize()
    for k, (run, S) in enumerate(zip(runs, streams)):
        run.enqueue(S, delay, DELAY_MS * (len(runs) - k))      # the first stream is released last
    assert all(r.busy for r in runs)
    for S in reversed(streams):
        S.synchronize()
    for run in runs:
        _check(run, run.case.name + ", beside two other contexts")
        run.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: controls -- the entry point on ANOTHER stream than the producer must be caught
# ---------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["steps2-ragged-one-step", "steps2-ragged-two-step", "steps2-stepped-pipeline"])
def test_control_a_call_on_another_stream_is_caught(name, torch_delay):
    """Which hardware queue serves a stream is the runtime's choice, and it depends on what the tests before this one created: with the
    excitation cases in front of it the first pair this test draws came to share a queue (T's work finished the moment S's delay ended),
    while the pairs drawn next did not.  So up to three pairs are tried, each with a fresh context and buffers, before the test skips."""
    torch, delay = torch_delay
    for attempt in range(3):
        run = SC.Run(SC.BY_NAME[name], torch)
        S, T = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        run.enqueue(S, delay, DELAY_MS, entry=T, collect=False)
        t0 = time.perf_counter()
        while not T.query() and time.perf_counter() - t0 < 0.5e-3 * DELAY_MS:
            pass
        overlapped = T.query() and not S.query()
        S.wait_stream(T)
        run.collect(S)
        S.synchronize()
        T.synchronize()
        if overlapped:
            break
        run.close()
    if not overlapped:
        pytest.skip("the two streams share a hardware queue: T did not run while the delay held S")
    want, got = run.case.want("true"), run.results()
    for label in want:
        assert (got[label].view(np.uint32) != want[label].view(np.uint32)).any(), f"{name}: {label} equals the true answer although the call ran ahead of the producer"
    run.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# slab drivers: ranks as threads, each behind its own late producer; the consumer waits on fdw_slabs_stream alone
# ---------------------------------------------------------------------------------------------------------------------------------------
SLAB_DECKS = {"2ranks-k4": (2, 4, (400, 500), False), "3ranks-pipeline-k8-split": (3, 8, (900, 2100), True)}
SLAB_NT = 9


def _slab_place(name):
    from test_slabs_record import _edge
    world, ksteps, (nxe, nze), pipe = SLAB_DECKS[name]
    gz = 224 if pipe else 256
    return _edge(nxe, world, 1) + 3, gz + 3, gz


@functools.lru_cache(maxsize=None)
def slab_inputs(name, v):
    from test_slabs_gpu import _case
    from test_slabs_record import NB
    world, ksteps, (nxe, nze), pipe = SLAB_DECKS[name]
    seed = 3 if v == "true" else 13
    d, srce, d_obs, im0 = _case(nxe, nze, NB, SLAB_NT, True, seed=seed)
    if v == "decoy":
        srce = (srce * np.float32(0.5) + np.float32(1.0)).astype(np.float32)
    p0, pp0 = random_fields(d, seed + 2, amp=0.01)
    s0, s1 = random_fields(d, seed + 3, amp=0.1)
    img0 = np.zeros((nxe, nze), np.float32)
    img0[NB:nxe - NB, NB:nze - NB] = im0
    return SC._freeze(dict(d=d, v2=d["v2"], srce=srce, d_obs=d_obs, im0=im0, img0=img0, p0=p0, pp0=pp0, s0=s0, s1=s1,
                           samples=np.ascontiguousarray(d_obs.T[::-1])))


@functools.lru_cache(maxsize=None)
def slab_want(name, v):
    """The single-domain oracle's answers: the forward chain's P (damped once), PP and trace rows [nt][nx]; fd_back's image onto im0."""
    from test_slabs_record import NB
    i = slab_inputs(name, v)
    d = i["d"]
    sx, sz, gz = _slab_place(name)
    orc = O.Oracle(*args_of(d), compat=True)
    c = line_restatement(orc, d, i["v2"], None, sz, gz=gz, p0=i["p0"], pp0=i["pp0"], point=(sx, i["srce"]))
    image = orc.back(i["v2"], i["s0"], i["s1"], i["d_obs"], gz, imloc=i["im0"], nsteps=SLAB_NT)
    assert np.count_nonzero(image != i["im0"]) > d["nxe"] - 2 * NB
    return SC._freeze(dict(P=c["P"], PP=c["PP"], rec=np.ascontiguousarray(c["data"].T), image=image))


@pytest.mark.parametrize("name", list(SLAB_DECKS))
def test_the_slab_decoys_matter(name):
    t, d = slab_want(name, "true"), slab_want(name, "decoy")
    i = slab_inputs(name, "true")
    for k in ("P", "PP", "rec"):
        _adequate({k: t[k]}, {k: d[k]}, name)
    changed = t["image"] != i["im0"]                         # the image moves where the receiver field has arrived: compare there
    assert (t["image"][changed] != d["image"][changed]).mean() > 0.5 and (i["im0"] != slab_inputs(name, "decoy")["im0"]).all()


def _slab_rank(name, kind, calls, r, comms, delay, torch, gate):
    """One rank: decoys in place, device synchronised, then producer stream P_r (delay, true inputs), an event the slab stream waits for,
    the call(s), an event on the slab stream that alone orders the consumer stream's copies of the outputs."""
    from test_slabs_record import _slabs
    world, ksteps, (nxe, nze), pipe = SLAB_DECKS[name]
    true, decoy = slab_inputs(name, "true"), slab_inputs(name, "decoy")
    d = true["d"]
    nx = nxe - 2 * d["nxb"]
    sx, sz, gz = _slab_place(name)
    s = _slabs(d, comms[r], ksteps)
    assert (s.nbuf == 4) == pipe
    if pipe:      # the last pass of the first cycle really splits into boundary strips (side stream) and interior (compute stream)
        assert s.own1 - s.own0 >= 2 * 4 * s.ksteps + 16 and SLAB_NT > s.ksteps
    lo, hi = s.x_off, s.x_off + s.nxl

    def up(a, rows=True):
        a = np.array(a[lo:hi] if rows else a, np.float32, order="C")
        if not rows:
            return torch.from_numpy(a).to("cuda:0")
        t = torch.zeros((s.nxl, s.pitch), device="cuda:0")
        t[:, :nze] = torch.from_numpy(a).to("cuda:0")
        return t

    back = kind == "back"
    nfb, nrb = s.back_buffers()
    names = (("f0", "s0"), ("f1", "s1"), ("img", "img0"), ("smp", "samples")) if back else (("b0", "p0"), ("b1", "pp0"), ("src", "srce"))
    flat = ("smp", "src")
    dev = {k: up(decoy[src], k not in flat) for k, src in names}
    stage = {k: up(true[src], k not in flat) for k, src in names}
    dev["v2"], stage["v2"] = up(decoy["v2"]), up(true["v2"])
    if back:
        for k in range(2, nfb):
            dev[f"f{k}"] = up(np.full((nxe, nze), 7.0, np.float32))
        for k in range(nrb):                                        # the receiver fields start at zero, as fd_back's do (no decoy to give them)
            dev[f"r{k}"] = torch.zeros((s.nxl, s.pitch), device="cuda:0") if k < 2 else up(np.full((nxe, nze), -7.0, np.float32))
    else:
        for k in range(2, s.nbuf):
            dev[f"b{k}"] = up(np.full((nxe, nze), 7.0 if k == 2 else -7.0, np.float32))
        dev["rec"] = torch.full((SLAB_NT, nx), 9.0, device="cuda:0")
    res = {k: torch.empty_like(t) for k, t in dev.items()}
    P, Cn, X = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.ExternalStream(s.stream)
    torch.cuda.synchronize()
    gate.wait(timeout=60)                                                     # no rank's delay is running while another rank still synchronises
    with torch.cuda.stream(P):
        delay(DELAY_MS * (r + 1))
        for k, t in stage.items():
            dev[k].copy_(t, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(P)
    X.wait_event(ev)
    if back:
        role = (0, 1, 0, 1)
        fp, rp = [dev[f"f{k}"].data_ptr() for k in range(nfb)], [dev[f"r{k}"].data_ptr() for k in range(nrb)]
        for it0, n in calls:
            role = s.dev_back(fp, rp, dev["v2"].data_ptr(), dev["smp"].data_ptr(), gz, dev["img"].data_ptr(), it0, n, role)
        where = role
    else:
        ip, ipp = 0, 1
        bp = [dev[f"b{k}"].data_ptr() for k in range(s.nbuf)]
        for k, (it0, n) in enumerate(calls):
            if kind == "record":
                ip, ipp = s.dev_record_forward(bp, dev["v2"].data_ptr(), dev["src"].data_ptr(), sx, sz, gz, dev["rec"].data_ptr(), it0, n, k > 0, ip, ipp)
            else:
                ip, ipp = s.dev_forward(bp, dev["v2"].data_ptr(), dev["src"].data_ptr(), sx, sz, it0, n, k > 0, ip, ipp)
        s.taper_finalize(dev[f"b{ip}"].data_ptr())                  # on the slab stream
        where = (ip, ipp)
    held = not P.query()
    done = torch.cuda.Event()
    done.record(X)
    Cn.wait_event(done)
    with torch.cuda.stream(Cn):
        for k, t in dev.items():
            res[k].copy_(t, non_blocking=True)
    Cn.synchronize()
    s.synchronize()
    out = {k: t.cpu().numpy() for k, t in res.items()}
    geo = (s.x_off, s.own0, s.own1)
    s.close()
    return out, where, geo, held


@gpu
@pytest.mark.parametrize("calls", [((0, 9),), ((0, 5), (5, 4))], ids=["one-call", "chained-5+4"])
@pytest.mark.parametrize("kind", ["forward", "record", "back"])
@pytest.mark.parametrize("name", list(SLAB_DECKS))
def test_slab_drivers_behind_late_producers(name, kind, calls, torch_delay, monkeypatch):
    """What a caller of the slab entry points must wait on is fdw_slabs_stream alone: the comm and side streams start behind it (so behind
    the caller's event), neighbours of different lateness are ordered by the communicator's events, and at the end of a call everything
    the side and comm streams wrote is visible to a consumer that waits on that stream only."""
    import parallel_finite_difference_computation_amd as F
    from test_slabs_record import NB, _run_ranks
    torch, delay = torch_delay
    world, ksteps, (nxe, nze), pipe = SLAB_DECKS[name]
    monkeypatch.setenv("FDW_SLAB_PIPE", "1" if pipe else "0")
    want = slab_want(name, "true")
    comms = F.Comm.local(world)
    gate = threading.Barrier(world)
    res, err = _run_ranks(lambda r: _slab_rank(name, kind, calls, r, comms, delay, torch, gate), world)
    for c in comms:
        c.close()
    for e in err:
        if e is not None:
            raise e
    nx, nz = nxe - 2 * NB, nze - 2 * NB
    what = f"{name} {kind} {calls}"
    assert all(held for _, _, _, held in res), f"{what}: a rank's producer had finished before its calls were issued"
    covered = 0
    for out, where, (x_off, o0, o1), _ in res:
        rows = slice(o0 - x_off, o1 - x_off)
        a, b = max(o0, NB) - NB, max(min(o1, NB + nx), NB) - NB
        if kind == "back":
            assert_bit_equal(out["img"][a + NB - x_off:b + NB - x_off, NB:NB + nz], want["image"][a:b], f"owned rows of the image, {what}")
        else:
            ip, ipp = where
            assert_bit_equal(out[f"b{ipp}"][rows, :nze], want["PP"][o0:o1], f"owned rows of d_pp, {what}")
            assert_bit_equal(out[f"b{ip}"][rows, :nze], want["P"][o0:o1], f"owned rows of d_p, {what}")
            if kind == "record":
                assert_bit_equal(out["rec"][:, a:b], want["rec"][:, a:b], f"trace rows of owned receivers [{a},{b}), {what}")
        covered += b - a
    assert covered == nx

"""One context through sequences of DIFFERENT host-API calls, every returned array against the CPU oracle bit for bit.

The host-array API keeps its device state in one fdw_ctx and reuses it from call to call ("What a context carries from call to
call"): eight to ten work fields of which each entry point clears only some, output buffers of the two-step and pipeline kernels whose
static rows and columns are filled by other code than the stepped cells, buffers that grow and never shrink or get cleared (wavelet,
gathers, trace rows, frame stores, batch buffers), the resident-model flags, the batch state, the tuning.  The other GPU modules build a
fresh context per case or repeat one call; here the previous call is a different one with different arguments.

  * every ordered pair (first, second) of call kinds of a dialect: a fresh context runs `first` with argument set A, then `second` with
    argument set B (tests/context_reuse_cases.py: the kinds, A and B, the oracle's answers);
  * three seeded walks of 40 calls per dialect that also change the kernel family, the prefetch distance and the chunk length between calls;
  * two contexts of different grid, order and dialect on one device, their calls alternating, one of them closed and rebuilt midway;
  * the sequences the buffers that only grow are there for: batches of 3, 2, 3 shots; wavelets of 14, 40, 14 samples; recording and
    residual migration alternating on the trace buffer they share; libfdwave_rtm_compat.so through a second fd_init with another grid.

The reference is never "the same call on a fresh context" -- that is the code under test -- but the oracle's answer, computed once per
(configuration, kind, argument set).  test_the_oracle_cases_can_tell_a_stale_answer runs without a GPU and checks what the matrix rests
on: no case is vacuous, and A's answer differs from B's in more than half of its cells.

Padding columns [nze, pitch): the context's own buffers have no accessor in the ABI (fdw_download_field takes a device pointer, and the
context hands none of its own out), so their staying zero is checked only through its consequences: every kernel family reads its z halo
across column nze on this grid (pitch 320 > nze 301), and a walk of 40 calls would carry a non-zero padding cell into a compared output."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np
import pytest

import context_reuse_cases as K
import parallel_finite_difference_computation_amd as F
from conftest import ROOT, assert_bit_equal
from context_reuse_cases import MOD, RTM, STORED, Cfg

FDW_EINVAL, FDW_ESTATE = -1, -5
Config = namedtuple("Config", "id cfg two_step env")            # env: variables the context is created under


def _families(prefix, dialect, geom, modes):
    return [Config(f"{prefix}-{name}-{'fast' if num else 'exact'}", Cfg(dialect, geom, 8, num), ts, {})
            for name, ts in modes for num in (0, 1)]


FAMILIES = (("one-step", -1), ("two-step", 1), ("pipeline", 4))
RTM_CONFIGS = (_families("ragged", RTM, K.RAGGED, FAMILIES)
               + [Config("ragged-one-step-order4", Cfg(RTM, K.RAGGED, 4, 0), -1, {}), Config("ragged-one-step-order12", Cfg(RTM, K.RAGGED, 12, 0), -1, {})]
               # every receiver row time-stepped: the batched launches (one-step) and the backward pipeline run here and only here
               + _families("stepped", RTM, K.STEPPED, (FAMILIES[0], FAMILIES[2])))
# the backward loop's other forms: the kinds that run it, as first and as second call
BACK_CONFIGS = [Config("ragged-one-step-two-launches", Cfg(RTM, K.RAGGED, 8, 0), -1, {"FDW_NO_FUSED_BACK": "1"}),
                Config("stepped-pipeline-no-back-pipe", Cfg(RTM, K.STEPPED, 8, 0), 4, {"FDW_NO_BACK_PIPE": "1"}),
                Config("stepped-pipeline-two-pass", Cfg(RTM, K.STEPPED, 8, 0), 4, {"FDW_NO_BACK_FUSED": "1"})]      # brings fld[8], fld[9] into play
MOD_CONFIGS = _families("mod", MOD, K.RAGGED, FAMILIES) + [Config("mod-one-step-order4", Cfg(MOD, K.RAGGED, 4, 0), -1, {})]
STORED_CONFIGS = _families("stored", STORED, K.STORED_GEOM, FAMILIES[:1]) + [Config("stored-one-step-order4", Cfg(STORED, K.STORED_GEOM, 4, 0), -1, {})]
ALL_CONFIGS = RTM_CONFIGS + BACK_CONFIGS + MOD_CONFIGS + STORED_CONFIGS
ALL_CFGS = sorted({c.cfg for c in ALL_CONFIGS} | {Cfg(MOD, K.ONE_STRIP, 4, 0)})
BACK_ENV = ("FDW_NO_FUSED_BACK", "FDW_NO_BACK_PIPE", "FDW_NO_BACK_FUSED")
WALK_SEEDS = (20261, 20262, 20263)


def _steps_per_pass(cfg, two_step):
    if cfg.order != 8 or two_step < 0 or cfg.dialect == STORED:
        return 1
    if two_step == 4:
        return 4
    return 2 if cfg.dialect == RTM else 1                    # the two-step kernel belongs to the RTM dialect


def tune(ctx, cfg, two_step, prefetch=0, xchunk=0):
    ctx.set_tuning(two_step=two_step, prefetch=prefetch, xchunk=xchunk)
    assert ctx.steps_per_pass() == _steps_per_pass(cfg, two_step), (cfg, two_step)
    assert ctx.two_step_active() == (cfg.dialect == RTM and cfg.order == 8 and two_step > 0), (cfg, two_step)


def new_ctx(config, monkeypatch):
    for name in BACK_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in config.env.items():
        monkeypatch.setenv(name, value)
    ctx = K.make_ctx(config.cfg)
    tune(ctx, config.cfg, config.two_step)
    if config.cfg.dialect == RTM:
        nxe, nze, nxb, nzb = config.cfg.geom
        assert ctx.extents() == (64, 296, 8) and ctx.pitch == 320 > nze
        stepped = config.cfg.geom == K.STEPPED
        assert bool(F.lib().fdw_back_pipe_active(ctx._h)) == (stepped and config.two_step == 4 and "FDW_NO_BACK_PIPE" not in config.env)
        assert (ctx.shot_batch_max() > 1) == (stepped and config.two_step < 0 and config.cfg.order <= 8), config.id
    return ctx


class Session:
    """A context, and whether it should hold a resident squared model; every call is checked against the oracle, and after every call
    that leaves no resident model shot_resident must be refused."""

    def __init__(self, ctx, cfg):
        self.ctx, self.cfg, self.resident, self.history = ctx, cfg, False, []

    def call(self, kind, v):
        self.history.append(f"{kind.name}({v})")
        what = f"{self.cfg}: " + " -> ".join(self.history[-4:]) + (f" (entry {len(self.history)} of this context's history)" if len(self.history) > 2 else "")
        want = kind.want(self.cfg, v)
        batched = self.cfg.dialect == RTM and self.ctx.shot_batch_max() > 1
        K.check(kind.run(self.ctx, self.cfg, v), want, what)
        if self.cfg.dialect != RTM:
            return
        self.resident = K.resident_after(kind, batched, self.resident)
        if not self.resident:
            i = K.rtm_inputs(self.cfg.geom, v)
            with pytest.raises(F.FdwError) as e:
                self.ctx.shot_resident(*K.place(self.cfg, v), i["srce"], i["d_obs"])
            assert e.value.code == FDW_ESTATE, "shot_resident after " + what


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: what the matrix rests on
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL_CFGS, ids=lambda c: f"dialect{c.dialect}-{'x'.join(map(str, c.geom))}-order{c.order}-numerics{c.numerics}")
def test_the_oracle_cases_can_tell_a_stale_answer(cfg):
    """Every cached oracle case of this configuration runs (each asserts that its own output holds a signal and no NaN), and the answers
    to A and to B differ in more than half of their non-zero cells, the gathers on every live trace; forward's outputs are non-zero on the
    static rows and in the columns >= zlim (asserted in its case)."""
    kinds = K.kinds_of(cfg.dialect)
    assert len(kinds) == {RTM: 19, MOD: 4, STORED: 4}[cfg.dialect]
    for k in kinds:
        K.assert_distinct(k, cfg)
    if cfg.dialect == RTM:                                       # the numerics and the order are part of the answer, the kernel family is not
        other = cfg._replace(numerics=1 - cfg.numerics) if cfg.order == 8 else cfg._replace(order=8)
        a, b = K.KINDS["shot_fields"].want(cfg, "A"), K.KINDS["shot_fields"].want(other, "A")
        assert (a["PP"] != b["PP"]).any() and (a["image"] != b["image"]).any()


def test_the_walks_are_reproducible():
    assert _walk_plan(WALK_SEEDS[0], RTM) == _walk_plan(WALK_SEEDS[0], RTM) != _walk_plan(WALK_SEEDS[1], RTM)
    for dialect in (RTM, MOD, STORED):
        for seed in WALK_SEEDS:
            plan = _walk_plan(seed, dialect)
            assert len(plan) == 40 and {p[1] for p in plan} == {"A", "B"}
            assert {p[2] for p in plan} == {-1, 1, 4} and {p[3] for p in plan} == {1, 2, 3} and {p[4] for p in plan} == {0, 13}


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: every ordered pair
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pairs(config, first, followers, monkeypatch):
    for second in followers:
        ctx = new_ctx(config, monkeypatch)
        s = Session(ctx, config.cfg)
        s.call(first, "A")
        s.call(second, "B")
        ctx.close()


def _ids(configs, kinds):
    return [pytest.param(c, k, id=f"{c.id}-{k.name}") for c in configs for k in kinds]


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", _ids(RTM_CONFIGS, K.kinds_of(RTM)))
def test_every_pair_of_rtm_calls(config, first, monkeypatch):
    _pairs(config, first, K.kinds_of(RTM), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", _ids(BACK_CONFIGS, K.kinds_of(RTM)))
def test_every_pair_with_a_backward_loop_in_its_other_forms(config, first, monkeypatch):
    _pairs(config, first, [k for k in K.kinds_of(RTM) if first.backward or k.backward], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", _ids(MOD_CONFIGS, K.kinds_of(MOD)))
def test_every_pair_of_modelling_calls(config, first, monkeypatch):
    _pairs(config, first, K.kinds_of(MOD), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", _ids(STORED_CONFIGS, K.kinds_of(STORED)))
def test_every_pair_of_stored_wavefield_calls(config, first, monkeypatch):
    _pairs(config, first, K.kinds_of(STORED), monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: seeded walks
# ---------------------------------------------------------------------------------------------------------------------------------------
def _walk_plan(seed, dialect):
    """40 x (kind, argument set, two_step, prefetch, xchunk)."""
    rng = np.random.default_rng(seed)
    kinds = K.kinds_of(dialect)
    return [(kinds[rng.integers(len(kinds))].name, "AB"[rng.integers(2)], (-1, 1, 4)[rng.integers(3)], int(rng.integers(1, 4)), (0, 13)[rng.integers(2)])
            for _ in range(40)]


WALKS = [Config("rtm-ragged", Cfg(RTM, K.RAGGED, 8, 0), -1, {}), Config("rtm-stepped-fast", Cfg(RTM, K.STEPPED, 8, 1), -1, {}),
         Config("rtm-stepped-two-pass", Cfg(RTM, K.STEPPED, 8, 0), -1, {"FDW_NO_BACK_FUSED": "1"}),
         Config("mod", Cfg(MOD, K.RAGGED, 8, 0), -1, {}), Config("stored-fast", Cfg(STORED, K.STORED_GEOM, 8, 1), -1, {})]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", WALK_SEEDS)
@pytest.mark.parametrize("config", WALKS, ids=lambda c: c.id)
def test_seeded_walk(config, seed, monkeypatch):
    """The printed sequence replays a failure as a pair: the failing call after the one before it (or after all of them)."""
    cfg = config.cfg
    for name in BACK_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in config.env.items():
        monkeypatch.setenv(name, value)
    ctx = K.make_ctx(cfg)
    s = Session(ctx, cfg)
    plan = _walk_plan(seed, cfg.dialect)
    print(f"walk {config.id} seed {seed}: " + "; ".join(f"{n}({v}) two_step={ts} prefetch={pf} xchunk={xc}" for n, v, ts, pf, xc in plan))
    for name, v, two_step, prefetch, xchunk in plan:
        tune(ctx, cfg, two_step, prefetch, xchunk)
        s.history.append(f"[two_step={two_step} prefetch={prefetch} xchunk={xchunk}]")
        s.call(K.KINDS[name], v)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: two contexts interleaved
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("two_step", [-1, 1, 4])
def test_two_contexts_interleaved(two_step, monkeypatch):
    """An order-8 RTM context on the ragged grid and an order-4 modelling context on a one-strip grid, one device, calls alternating;
    the second is closed and rebuilt after half of them (its memory goes back to the allocator the first keeps using)."""
    one = Config("first", Cfg(RTM, K.RAGGED, 8, 0), two_step, {})
    two = Config("second", Cfg(MOD, K.ONE_STRIP, 4, 0), -1, {})
    a, b = Session(new_ctx(one, monkeypatch), one.cfg), Session(new_ctx(two, monkeypatch), two.cfg)
    assert b.ctx.pitch == 256 == K.ONE_STRIP[1]
    first = [K.KINDS[n] for n in ("forward13", "shot_illum", "laplacian", "shot_residual", "back3", "shot_snaps_4_3", "record_shot", "shot_batch2",
                                  "shot_resident", "shot_fields")]
    second = K.kinds_of(MOD)
    for j, k in enumerate(first):
        a.call(k, "AB"[j % 2])
        b.call(second[j % len(second)], "BA"[j % 2])
        if j == len(first) // 2:
            b.ctx.close()
            b = Session(new_ctx(two, monkeypatch), two.cfg)
    a.ctx.close()
    b.ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU 4: the sequences the growing buffers are there for
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sequence(config, steps, monkeypatch):
    s = Session(new_ctx(config, monkeypatch), config.cfg)
    for name, v in steps:
        s.call(K.KINDS[name], v)
    s.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", [c for c in RTM_CONFIGS if c.cfg.order == 8 and c.two_step != 1], ids=lambda c: c.id)
def test_batches_of_three_two_and_three_shots(config, monkeypatch):
    """The batch buffers keep the larger earlier batch; the illumination and trace buffers of a batch are allocated apart from them."""
    _sequence(config, [("shot_batch3", "A"), ("shot_batch2", "B"), ("shot_batch3", "B"), ("shot_batch_illum3", "A"), ("shot_batch2", "A"),
                       ("shot_batch_residual3", "B"), ("record_shot_batch3", "A"), ("shot_batch_resident2", "B"), ("shot_batch3", "A")], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config", [c for c in RTM_CONFIGS if c.cfg.order == 8], ids=lambda c: c.id)
def test_recording_and_residual_migration_alternate_on_the_trace_buffer(config, monkeypatch):
    _sequence(config, [("record_shot", "A"), ("shot_residual", "B"), ("record_shot", "B"), ("shot_residual_illum", "A"), ("record_shot_batch3", "B"),
                       ("shot_residual", "A"), ("record_shot", "A")], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config", MOD_CONFIGS, ids=lambda c: c.id)
def test_wavelets_of_14_40_and_14_samples(config, monkeypatch):
    """The trace buffer shrinks logically inside the larger allocation; the batch has its own."""
    _sequence(config, [("model_shot14", "A"), ("model_shot40", "B"), ("model_shot14", "B"), ("model_shot_batch3x14", "A"), ("model_shot40", "A"),
                       ("model_shot_batch2x40", "B"), ("model_shot14", "A")], monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config", [c for c in RTM_CONFIGS if c.cfg.order == 8 and c.cfg.numerics == 0], ids=lambda c: c.id)
def test_the_resident_model_survives_calls_that_upload_none(config, monkeypatch):
    """laplacian touches no model, and a batch of host models that runs through the batched launches keeps them in the batch buffers: after
    either, shot_resident still runs on the model dev_extendvel_linear drew -- and gives the oracle's answer for it."""
    cfg = config.cfg
    ctx = new_ctx(config, monkeypatch)
    s = Session(ctx, cfg)
    s.call(K.KINDS["shot_resident"], "A")
    keepers = ["laplacian"] + (["shot_batch3", "record_shot_batch3"] if ctx.shot_batch_max() > 1 else [])
    for name in keepers:
        s.call(K.KINDS[name], "B")
        assert s.resident
        i = K.rtm_inputs(cfg.geom, "A")
        img, P, PP = ctx.shot_resident(*K.place(cfg, "A"), i["srce"], i["d_obs"], imloc=i["im0"], want_fields=True)
        K.check(dict(image=img, P=P, PP=PP), K.KINDS["shot_resident"].want(cfg, "A"), f"{config.id}: shot_resident again after {name}(B)")
    ctx.close()


@pytest.mark.gpu
def test_a_refused_call_that_was_given_a_model_invalidates_the_resident_one(monkeypatch):
    """The entry points that take a model drop the resident one before they look at their other arguments."""
    config = RTM_CONFIGS[0]
    cfg = config.cfg
    i = K.rtm_inputs(cfg.geom, "B")
    sx, sz, gz = K.place(cfg, "B")
    calls = {"record_shot": lambda c: c.record_shot(i["v2"], sx, sz, -1, i["srce"]),
             "shot_residual": lambda c: c.shot_residual(i["v2"], sx, sz, 296, i["srce"], i["d_obs"])}
    for name, refused in calls.items():
        ctx = new_ctx(config, monkeypatch)
        s = Session(ctx, cfg)
        s.call(K.KINDS["shot_resident"], "A")
        with pytest.raises(F.FdwError) as e:
            refused(ctx)
        assert e.value.code == FDW_EINVAL, name
        with pytest.raises(F.FdwError) as e:
            ctx.shot_resident(sx, sz, gz, i["srce"], i["d_obs"])
        assert e.value.code == FDW_ESTATE, name
        ctx.close()


@pytest.mark.gpu
def test_compat_library_through_a_second_fd_init():
    """libfdwave_rtm_compat.so keeps one global context; a second fd_init with another grid destroys it and builds a new one:
    fd_init(A) -> fd_forward -> fd_init(B) -> fd_forward -> fd_back, every array against the oracle."""
    L = C.CDLL(os.path.join(ROOT, "parallel_finite_difference_computation_amd", "libfdwave_rtm_compat.so"))
    fpp = C.POINTER(C.POINTER(C.c_float))
    L.fd_init.argtypes = [C.c_int] * 7 + [C.c_float] * 4
    L.fd_forward.argtypes = [C.c_int, fpp, fpp, fpp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]
    L.fd_back.argtypes = [C.c_int, fpp, fpp, fpp, fpp, fpp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(fpp), fpp, fpp]

    def rows(a):   # alloc2float layout: row pointers into one contiguous block
        return (C.POINTER(C.c_float) * a.shape[0])(*[C.cast(a[i].ctypes.data, C.POINTER(C.c_float)) for i in range(a.shape[0])])

    def forward(cfg, v):
        nxe, nze, nxb, nzb = cfg.geom
        i = K.rtm_inputs(cfg.geom, v)
        sx, sz, gz = K.place(cfg, v)
        P, PP = np.array(i["p0"]), np.array(i["pp0"])
        v2, srce = np.array(i["v2"]), np.array(i["srce"])
        L.fd_forward(cfg.order, rows(P), rows(PP), rows(v2), nze, nxe, K.NT, 0, sz, (C.c_int * 1)(sx), srce.ctypes.data_as(C.POINTER(C.c_float)), 0)
        oP, oPP = K.oracle_of(cfg).forward(i["v2"], sx, sz, i["srce"], i["p0"], i["pp0"])
        assert_bit_equal(P, oP, f"fd_forward P, {cfg}")
        assert_bit_equal(PP, oPP, f"fd_forward PP, {cfg}")
        assert (oPP != i["pp0"]).mean() > 0.9
        return P, PP, v2, gz

    a, b = Cfg(RTM, K.STEPPED, 8, 0), Cfg(RTM, K.RAGGED, 8, 0)
    L.fd_init(*K.ctx_args(a)[:6], 1, 0.75, 10.0, 12.5, K.DT)
    forward(a, "A")
    L.fd_init(*K.ctx_args(b)[:6], 1, 0.75, 10.0, 12.5, K.DT)
    P, PP, v2, gz = forward(b, "B")
    nxe, nze, nxb, nzb, nx, nz = K.dims(b)
    i = K.rtm_inputs(b.geom, "B")
    snaps = np.stack([P, PP])
    snap_rows = [rows(snaps[0]), rows(snaps[1])]
    snaps_pp = (fpp * 2)(C.cast(snap_rows[0], fpp), C.cast(snap_rows[1], fpp))
    imloc, d_obs = np.array(i["im0"]), np.array(i["d_obs"])
    dobs_rows = (C.POINTER(C.c_float) * 1)(C.cast(d_obs.ctypes.data, C.POINTER(C.c_float)))
    z = np.zeros((nxe, nze), np.float32)
    L.fd_back(8, rows(z), rows(z), rows(z), rows(z), rows(v2), nze, nxe, K.NT, 0, 0, gz, snaps_pp, rows(imloc), dobs_rows)
    want = K.oracle_of(b).back(i["v2"], P, PP, i["d_obs"], gz, imloc=i["im0"])
    lo, hi = K.live_traces(b)
    assert np.count_nonzero(want != i["im0"]) > (hi - lo) * (b.order + 1) // 2      # (the threshold of the back kinds)
    assert_bit_equal(imloc, want, "fd_back imloc after the second fd_init")
    L.fd_free()

"""tests/test_context_reuse.py's matrix extended to the families that came after it: line sources, excitation imaging, Born modelling, DTT
imaging, extended images, least-squares migration ("The families that came later").

Those families added more state to fdw_ctx than everything before them and reuse the old buffers under new clearing rules: d_born_m is the
reflectivity of the Born calls and the search direction of the LSM visits; d_rec serves recording, residual migration and Born modelling,
with d_born_rec0 beside it; d_wav serves every line-source call and the excitation shot's receiver loop; d_eimg is sized for the largest H
seen; born_shot_impl and lsm_visit_dev clear fld[0..3], which nobody cleared before, and the old families still leave in fld[2..3] and
fld[6..7] whatever they wrote.  Each family's own module builds a fresh context per case or repeats its own calls; here one context runs a
call of one family after a call of another, with other arguments, and every returned array is compared with the CPU restatement's cached
answer bit for bit (context_reuse_cases.check; no tolerance anywhere).  The families' modules already hold each entry point to its
restatement bit for bit on a fresh context, so a difference here is carried state.

  * pairs: every ordered pair of call kinds of which at least one is new (tests/context_reuse_family_cases.py: 23 kinds; with the 19 of
    tests/context_reuse_cases.py 23 x 42 + 19 x 23 = 1403 ordered pairs), a fresh context per pair, first(A) -> second(B), in nine
    configurations; one test is one first kind with its followers of one registry (the old 19 or the new 23), so that a test runs about as
    many pairs as a test of tests/test_context_reuse.py;
  * three seeded walks of 40 calls over all 42 kinds on three contexts, the kernel family, prefetch distance and chunk length redrawn
    before every call;
  * named sequences for the buffers with more than one user: d_born_m, d_rec / d_born_rec0, d_wav, d_eimg, the batch buffers, the
    resident model;
  * two RTM contexts of different grid and order, their calls alternating, the second closed and rebuilt midway.

Order 12 (ragged-one-step-order12): born_fused() and dtt_fused() (csrc/fdw_api.cpp) both ask for an order <= 8, so at order 12 the Born loop
runs its two step launches, fdw_born_diff and the scatter kernel through d_born_w, and the DTT backward loop its plain steps and
fdw_dev_dtt_image through d_dtt_w; the library exposes no query for either, the same arrangement is what FDW_NO_BORN_FUSED=1 and
FDW_NO_FUSED_BACK=1 force at order 8, and tests/test_born.py and tests/test_dtt.py pin it there by the kernels a child process launches."""
import numpy as np
import pytest

import context_reuse_cases as K
import context_reuse_family_cases as FK
import test_context_reuse as T
from context_reuse_cases import RTM, Cfg
from test_context_reuse import Config, Session

NKINDS = 23
FUSION_ENV = ("FDW_NO_BORN_FUSED",)                            # on top of test_context_reuse.BACK_ENV, which new_ctx clears itself
CONFIGS = [Config("ragged-one-step-exact", Cfg(RTM, K.RAGGED, 8, 0), -1, {}), Config("ragged-one-step-fast", Cfg(RTM, K.RAGGED, 8, 1), -1, {}),
           # every receiver row time-stepped: the batched launches (one-step) and the backward pipeline run here and only here
           Config("stepped-one-step-exact", Cfg(RTM, K.STEPPED, 8, 0), -1, {}), Config("stepped-one-step-fast", Cfg(RTM, K.STEPPED, 8, 1), -1, {}),
           Config("stepped-pipeline-exact", Cfg(RTM, K.STEPPED, 8, 0), 4, {}), Config("stepped-pipeline-fast", Cfg(RTM, K.STEPPED, 8, 1), 4, {}),
           # neither the Born nor the DTT loop is fused above order 8 (module docstring): d_born_w and d_dtt_w are in play
           Config("ragged-one-step-order12", Cfg(RTM, K.RAGGED, 12, 0), -1, {})]
NO_BORN_FUSED = Config("stepped-one-step-no-born-fused", Cfg(RTM, K.STEPPED, 8, 0), -1, {"FDW_NO_BORN_FUSED": "1"})
NO_FUSED_BACK = Config("stepped-one-step-no-fused-back", Cfg(RTM, K.STEPPED, 8, 0), -1, {"FDW_NO_FUSED_BACK": "1"})
ENV_CONFIGS = [NO_BORN_FUSED, NO_FUSED_BACK]
ENV_FAMILIES = ("born", "dtt", "lsm")                          # the families whose loops the two variables rearrange
ORDER8_STEPPED = [c for c in CONFIGS if c.cfg.geom == K.STEPPED]
SECOND = Cfg(RTM, K.ONE_STRIP, 4, 0)                           # the second context of the interleaved test
SECOND_KINDS = ("born_shot", "shot_dtt", "born_shot_line", "shot_line_dtt", "born_shot_field", "shot_dtt_residual_illum", "born_shot_batch3",
                "shot_batch_dtt2")
ALL_CFGS = sorted({c.cfg for c in CONFIGS + ENV_CONFIGS})
WALK_SEEDS = (31339, 31341, 31362)                             # every plan visits every family; together they draw all 42 kinds


def new_ctx(config, monkeypatch):
    """test_context_reuse.new_ctx with the fusion variables cleared first.  Under FDW_NO_FUSED_BACK=1 batch_ok() is false on every grid, so
    on STEPPED the batches fall back to one shot after the other: new_ctx's expectation of shot_batch_max() does not cover that case (its
    own FDW_NO_FUSED_BACK configuration is on RAGGED), and the context is built here with the expectation that does."""
    for name in FUSION_ENV:
        monkeypatch.delenv(name, raising=False)
    if config.env.get("FDW_NO_FUSED_BACK") and config.cfg.geom == K.STEPPED:
        for name in T.BACK_ENV:
            monkeypatch.delenv(name, raising=False)
        for name, value in config.env.items():
            monkeypatch.setenv(name, value)
        ctx = K.make_ctx(config.cfg)
        T.tune(ctx, config.cfg, config.two_step)
        assert ctx.extents() == (64, 296, 8) and ctx.pitch == 320 and ctx.shot_batch_max() == 1
        return ctx
    return T.new_ctx(config, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: what the matrix rests on
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_registries():
    """23 new kinds in a registry of their own; the old module's 19 and their order are what they were, so its walks keep their sequences."""
    assert len(FK.family_kinds()) == NKINDS == 23 and len(K.kinds_of(RTM)) == 19 and len(FK.all_kinds()) == 42
    assert not set(FK.FAMILY_KINDS) & set(K.KINDS)
    assert [k.name for k in FK.all_kinds()[:19]] == [k.name for k in K.kinds_of(RTM)]
    per_family = {f: sum(FK.family_of(k) == f for k in FK.family_kinds()) for f in ("line", "excitation", "born", "dtt", "ext", "lsm")}
    assert per_family == dict(line=5, excitation=3, born=5, dtt=4, ext=3, lsm=3)
    assert {k.model for k in FK.family_kinds()} == {"clear", "set", "batch_host"}
    assert sorted(FK.RESIDENT_FORMS) == ["born", "dtt", "excitation", "ext", "lsm"]
    assert all(n in FK.FAMILY_KINDS for n in SECOND_KINDS)


@pytest.mark.parametrize("cfg", ALL_CFGS, ids=lambda c: f"{'x'.join(map(str, c.geom))}-order{c.order}-numerics{c.numerics}")
def test_the_restatement_cases_can_tell_a_stale_answer(cfg):
    """Every cached case of this configuration runs (each asserts that its own output holds a signal and no NaN), and the answers to A and
    to B differ in more than half of their non-zero cells, the gathers on every live trace.  Every plane of the extended images holds a signal
    of its own (asserted in the case), and the H = 1 planes are not the head (nor the middle) of the H = 3 planes."""
    for k in FK.family_kinds():
        FK.assert_distinct(k, cfg)
    for v in "AB":
        e3, e1 = FK.FAMILY_KINDS["shot_ext3"].want(cfg, v)["eimg"], FK.FAMILY_KINDS["shot_ext1"].want(cfg, v)["eimg"]
        e0 = FK.FAMILY_KINDS["shot_ext0"].want(cfg, v)["eimg"]
        assert e3.shape[0] == 7 and e1.shape[0] == 3 and e0.shape[0] == 1
        for j in range(3):
            assert (e1[j] != e3[j]).any() and (e1[j] != e3[2 + j]).any(), (v, j)
        assert (e0[0] != e1[1]).any() and (e0[0] != e3[3]).any()
    # the scattering kind, the model and the numerics / order are part of the answer
    born, field = FK.FAMILY_KINDS["born_shot"], FK.FAMILY_KINDS["born_shot_field"]
    assert (born.want(cfg, "A")["scattered"] != field.want(cfg, "A")["scattered"]).any()
    assert (born.want(cfg, "A")["scattered"] != FK.FAMILY_KINDS["born_shot_resident"].want(cfg, "A")["scattered"]).any()
    other = cfg._replace(numerics=1 - cfg.numerics) if cfg.order == 8 else cfg._replace(order=8)
    for name, out in (("born_shot", "scattered"), ("shot_dtt", "image"), ("lsm_visit", "h")):
        assert (FK.FAMILY_KINDS[name].want(cfg, "A")[out] != FK.FAMILY_KINDS[name].want(other, "A")[out]).any(), name
    # the resident forms of the residency sequence: B's arguments on A's drawn model are neither B's nor A's own answer
    for family, (want, _) in FK.RESIDENT_FORMS.items():
        mixed = want(cfg, "B", "A")
        for name, a in mixed.items():
            assert np.isfinite(a).all() and (a != want(cfg, "B", "host")[name]).any() and (a != want(cfg, "B", "B")[name]).any(), (family, name)


def test_the_second_context_of_the_interleaved_test():
    for name in SECOND_KINDS:
        FK.assert_distinct(FK.FAMILY_KINDS[name], SECOND)


def test_the_walks_are_reproducible():
    assert _walk_plan(WALK_SEEDS[0]) == _walk_plan(WALK_SEEDS[0]) != _walk_plan(WALK_SEEDS[1])
    drawn = set()
    for seed in WALK_SEEDS:
        plan = _walk_plan(seed)
        assert len(plan) == 40 and {p[1] for p in plan} == {"A", "B"}
        assert {p[2] for p in plan} == {-1, 1, 4} and {p[3] for p in plan} == {1, 2, 3} and {p[4] for p in plan} == {0, 13}
        names = {p[0] for p in plan}
        assert names & set(K.KINDS) and {FK.family_of(FK.kind_of(n)) for n in names} >= {"line", "excitation", "born", "dtt", "ext", "lsm"}, seed
        drawn |= names
    assert drawn == {k.name for k in FK.all_kinds()}, sorted({k.name for k in FK.all_kinds()} - drawn)


def test_the_pair_matrix_covers_every_pair_with_a_new_kind_once():
    new, old = FK.family_kinds(), K.kinds_of(RTM)
    pairs = [(a.name, b.name) for a in new for b in old] + [(a.name, b.name) for a in new for b in new] + [(a.name, b.name) for a in old for b in new]
    assert len(pairs) == len(set(pairs)) == 23 * 42 + 19 * 23 == 1403
    env = [(a, b) for a, b in pairs if _rearranged(FK.kind_of(a)) or _rearranged(FK.kind_of(b))]
    assert len(env) == 12 * 42 + 30 * 12 == 864


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU 1: every ordered pair with a new kind
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rearranged(k):
    return FK.family_of(k) in ENV_FAMILIES


def _pairs(config, first, followers, monkeypatch):
    for second in followers:
        ctx = new_ctx(config, monkeypatch)
        s = Session(ctx, config.cfg)
        s.call(first, "A")
        s.call(second, "B")
        ctx.close()


def _env_followers(first, followers):
    """Under the two environment configurations: the pairs in which at least one side is a Born, DTT or LSM kind."""
    return [k for k in followers if _rearranged(first) or _rearranged(k)]


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", T._ids(CONFIGS, FK.family_kinds()))
def test_a_new_call_then_every_old_call(config, first, monkeypatch):
    _pairs(config, first, K.kinds_of(RTM), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", T._ids(CONFIGS, FK.family_kinds()))
def test_a_new_call_then_every_new_call(config, first, monkeypatch):
    _pairs(config, first, FK.family_kinds(), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", T._ids(CONFIGS, K.kinds_of(RTM)))
def test_an_old_call_then_every_new_call(config, first, monkeypatch):
    _pairs(config, first, FK.family_kinds(), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", T._ids(ENV_CONFIGS, [k for k in FK.family_kinds() if _rearranged(k)]))
def test_unfused_loops_a_new_call_then_every_old_call(config, first, monkeypatch):
    """FDW_NO_BORN_FUSED=1 / FDW_NO_FUSED_BACK=1 at order 8: d_born_w / d_dtt_w, and the one-launch-per-shot fall-back of the batches."""
    _pairs(config, first, _env_followers(first, K.kinds_of(RTM)), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", T._ids(ENV_CONFIGS, FK.family_kinds()))
def test_unfused_loops_a_new_call_then_every_new_call(config, first, monkeypatch):
    _pairs(config, first, _env_followers(first, FK.family_kinds()), monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("config,first", T._ids(ENV_CONFIGS, K.kinds_of(RTM)))
def test_unfused_loops_an_old_call_then_every_new_call(config, first, monkeypatch):
    _pairs(config, first, _env_followers(first, FK.family_kinds()), monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU 2: seeded walks over the 42 kinds
# ---------------------------------------------------------------------------------------------------------------------------------------
def _walk_plan(seed):
    """40 x (kind, argument set, two_step, prefetch, xchunk)."""
    rng = np.random.default_rng(seed)
    kinds = FK.all_kinds()
    return [(kinds[rng.integers(len(kinds))].name, "AB"[rng.integers(2)], (-1, 1, 4)[rng.integers(3)], int(rng.integers(1, 4)), (0, 13)[rng.integers(2)])
            for _ in range(40)]


WALKS = [Config("ragged-exact", Cfg(RTM, K.RAGGED, 8, 0), -1, {}), Config("stepped-fast", Cfg(RTM, K.STEPPED, 8, 1), -1, {}),
         Config("stepped-exact-no-born-fused", Cfg(RTM, K.STEPPED, 8, 0), -1, {"FDW_NO_BORN_FUSED": "1"})]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", WALK_SEEDS)
@pytest.mark.parametrize("config", WALKS, ids=lambda c: c.id)
def test_seeded_walk(config, seed, monkeypatch):
    """The printed sequence replays a failure as a pair: the failing call after the one before it (or after all of them)."""
    cfg = config.cfg
    ctx = new_ctx(config, monkeypatch)
    s = Session(ctx, cfg)
    plan = _walk_plan(seed)
    print(f"walk {config.id} seed {seed}: " + "; ".join(f"{n}({v}) two_step={ts} prefetch={pf} xchunk={xc}" for n, v, ts, pf, xc in plan))
    for name, v, two_step, prefetch, xchunk in plan:
        T.tune(ctx, cfg, two_step, prefetch, xchunk)
        s.history.append(f"[two_step={two_step} prefetch={prefetch} xchunk={xchunk}]")
        s.call(FK.kind_of(name), v)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU 3: named sequences for the buffers with more than one user
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sequence(config, steps, monkeypatch):
    s = Session(new_ctx(config, monkeypatch), config.cfg)
    for name, v in steps:
        s.call(FK.kind_of(name), v)
    s.ctx.close()


stepped = pytest.mark.parametrize("config", ORDER8_STEPPED, ids=lambda c: c.id)


@pytest.mark.gpu
@stepped
def test_reflectivity_and_search_direction_share_d_born_m(config, monkeypatch):
    _sequence(config, [("born_shot", "A"), ("lsm_visit", "B"), ("born_shot", "B"), ("lsm_visit_batch3", "A"), ("born_shot_batch3", "B"),
                       ("lsm_solve", "A"), ("born_shot", "A")], monkeypatch)


@pytest.mark.gpu
@stepped
def test_recording_residual_migration_and_born_modelling_share_d_rec(config, monkeypatch):
    """born_shot and born_shot_line are the kinds with the background gather: d_born_rec0 beside d_rec."""
    _sequence(config, [("record_shot", "A"), ("born_shot", "B"), ("shot_residual", "A"), ("born_shot_line", "B"), ("record_shot_batch3", "A"),
                       ("born_shot", "B")], monkeypatch)


@pytest.mark.gpu
@stepped
def test_the_line_source_calls_share_d_wav(config, monkeypatch):
    _sequence(config, [("shot_line", "A"), ("born_shot_line", "B"), ("shot_line_dtt", "A"), ("record_shot_line", "B"), ("shot_line_batch3", "A"),
                       ("shot_line_residual", "B")], monkeypatch)


@pytest.mark.gpu
@stepped
def test_extended_images_of_half_widths_3_1_3_0_then_a_plain_shot(config, monkeypatch):
    """d_eimg keeps the planes of the largest H seen and a smaller H uses their head; shot_fields runs shot_impl's loop without ext_H."""
    _sequence(config, [("shot_ext3", "A"), ("shot_ext1", "B"), ("shot_ext3", "B"), ("shot_ext0", "A"), ("shot_fields", "B"), ("shot_ext1", "A")],
              monkeypatch)


@pytest.mark.gpu
@stepped
def test_batches_of_every_family_on_the_batch_buffers(config, monkeypatch):
    """Both layouts of ensure_batch_buffers, batches of 3 and 2, every family's own use of bfld[] (the excitation maps in bfld[4..6], the
    scattered pairs in bfld[2..3])."""
    _sequence(config, [("shot_batch3", "A"), ("born_shot_batch3", "B"), ("shot_batch2", "A"), ("shot_excitation_batch3", "B"), ("shot_batch_dtt2", "A"),
                       ("lsm_visit_batch3", "B"), ("record_shot_batch3", "A"), ("born_shot_batch3", "A"), ("shot_batch3", "B")], monkeypatch)


@pytest.mark.gpu
@stepped
def test_the_resident_model_survives_the_calls_with_no_model_and_ends_with_one(config, monkeypatch):
    """After shot_resident(A) each family's single-shot form runs with v2=None on B's other arguments: it gives the restatement's answer
    for A's drawn model, and shot_resident is still accepted and still gives the oracle's answer for that model.  The same form with a
    model ends the residency: shot_resident is refused with FDW_ESTATE (Session checks that after every call that leaves no model)."""
    cfg = config.cfg
    ctx = new_ctx(config, monkeypatch)
    s = Session(ctx, cfg)
    i = K.rtm_inputs(cfg.geom, "A")
    with_model = dict(born="born_shot", excitation="shot_excitation", dtt="shot_dtt", ext="shot_ext1", lsm="lsm_visit")
    for family, (want, run) in sorted(FK.RESIDENT_FORMS.items()):
        s.call(K.KINDS["shot_resident"], "A")
        assert s.resident
        K.check(run(ctx, cfg, "B", None), want(cfg, "B", "A"), f"{config.id}: {family}(B, v2=None) after shot_resident(A)")
        img, P, PP = ctx.shot_resident(*K.place(cfg, "A"), i["srce"], i["d_obs"], imloc=i["im0"], want_fields=True)
        K.check(dict(image=img, P=P, PP=PP), K.KINDS["shot_resident"].want(cfg, "A"), f"{config.id}: shot_resident again after {family}(B, v2=None)")
        s.call(FK.FAMILY_KINDS[with_model[family]], "B")
        assert not s.resident
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU 4: two contexts interleaved
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("two_step", [-1, 4])
def test_two_contexts_interleaved(two_step, monkeypatch):
    """An order-8 RTM context on the ragged grid runs new kinds; an order-4 RTM context on the one-strip grid (pitch = nze) runs Born and
    DTT kinds, calls alternating; the second is closed and rebuilt after half of them."""
    one = Config("first", Cfg(RTM, K.RAGGED, 8, 0), two_step, {})

    def second():
        ctx = K.make_ctx(SECOND)
        T.tune(ctx, SECOND, -1)
        assert ctx.pitch == 256 == K.ONE_STRIP[1]
        return Session(ctx, SECOND)
    a, b = Session(new_ctx(one, monkeypatch), one.cfg), second()
    first = [FK.kind_of(n) for n in ("shot_line", "born_shot", "shot_excitation", "lsm_visit", "shot_ext3", "shot_dtt", "shot_excitation_batch3",
                                     "born_shot_resident", "shot_fields", "lsm_solve", "shot_ext1", "shot_line_dtt")]
    for j, k in enumerate(first):
        a.call(k, "AB"[j % 2])
        b.call(FK.FAMILY_KINDS[SECOND_KINDS[j % len(SECOND_KINDS)]], "BA"[j % 2])
        if j == len(first) // 2:
            b.ctx.close()
            b = second()
    a.ctx.close()
    b.ctx.close()

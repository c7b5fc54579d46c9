"""Guard-band tests of the device-array entry points: every fdw_dev_* call of tests/stream_cases.py -- the 100 cases
of the stream contract, the same builders on three edge decks, and calls on row ranges -- runs once with ALL its buffers carved from one
guarded arena (tests/footprint_arena.py).  Afterwards the answers must equal the CPU oracle's bit for bit (a value pulled in from a guard
is a NaN) and the footprint must be what fdwave.h says: guard words untouched, padding columns +0.0, `const` and untouched buffers as
uploaded, rows outside the rows asked for as uploaded.  The excitation entry points (stream_cases.EXC_CASES and, on
the edge decks, EXC_FOOTPRINT_CASES) run the same way; their maps and images carry a sentinel word in the padding columns, which must
come back, and d_texc travels as int32 words.

Unmarked tests: the checker sees a planted word in each place it guards (and passes a clean arena); the cases of the edge decks are not
vacuous; the decks have the properties they were chosen for; the catalogue of tests/test_stream_contract.py is unchanged.

Measured on one MI355X: see DESIGN.md sections 6o and 6s for the case counts, the wall times and what the module found."""
import numpy as np
import pytest

import footprint_arena as FA
import stream_cases as SC
from conftest import assert_bit_equal
from excitation_restatement import image_selection

gpu = pytest.mark.gpu
EXC_ALL = SC.EXC_CASES + SC.EXC_FOOTPRINT_CASES
ALL_CASES = SC.CASES + SC.FOOTPRINT_CASES + EXC_ALL
FP = {c.name: c for c in SC.FOOTPRINT_CASES + EXC_ALL}


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the catalogue is what it was
# ---------------------------------------------------------------------------------------------------------------------------------------
STREAM_CONTRACT_NAMES = """
steps2-ragged-one-step steps2-ragged-two-step steps2-stepped-pipeline record-ragged-one-step record-ragged-two-step record-stepped-pipeline
illum-ragged-one-step illum-ragged-two-step illum-stepped-pipeline record_illum-ragged-one-step record_illum-ragged-two-step
record_illum-stepped-pipeline line-ragged-one-step line-ragged-two-step line-stepped-pipeline line_rec-ragged-one-step line_rec-ragged-two-step
line_rec-stepped-pipeline line_ill-ragged-one-step line_ill-ragged-two-step line_ill-stepped-pipeline line_rec_ill-ragged-one-step
line_rec_ill-ragged-two-step line_rec_ill-stepped-pipeline record-ragged-pipeline steps2-ragged-one-step-fast steps2-ragged-two-step-fast
steps2-stepped-pipeline-fast record-ragged-one-step-fast record-ragged-two-step-fast record-stepped-pipeline-fast illum-ragged-one-step-fast
illum-ragged-two-step-fast illum-stepped-pipeline-fast record_illum-ragged-one-step-fast record_illum-ragged-two-step-fast
record_illum-stepped-pipeline-fast line-ragged-one-step-fast line-ragged-two-step-fast line-stepped-pipeline-fast line_rec-ragged-one-step-fast
line_rec-ragged-two-step-fast line_rec-stepped-pipeline-fast line_ill-ragged-one-step-fast line_ill-ragged-two-step-fast
line_ill-stepped-pipeline-fast line_rec_ill-ragged-one-step-fast line_rec_ill-ragged-two-step-fast line_rec_ill-stepped-pipeline-fast
record-ragged-pipeline-fast steps2-chained-ragged-one-step steps2-chained-ragged-two-step steps2-chained-stepped-pipeline
record-chained-ragged-one-step record-chained-ragged-two-step record-chained-stepped-pipeline line-chained-ragged-one-step
line-chained-ragged-two-step line-chained-stepped-pipeline steps2-tiles-pipeline record-tiles-pipeline illum-tiles-pipeline
record_illum-tiles-pipeline line-tiles-pipeline line_rec_ill-tiles-pipeline steps2-tiles-pipeline-fast steps-ragged steps_shrink-ragged
step_fwd-ragged step2-ragged step4-stepped step_plain-ragged step_recv-ragged back_iter0-ragged back_iter1-ragged back4-stepped
model_steps-ragged-one-step laplacian-ragged steps-ragged-fast steps_shrink-ragged-fast step_fwd-ragged-fast step2-ragged-fast
step4-stepped-fast step_plain-ragged-fast step_recv-ragged-fast back_iter0-ragged-fast back_iter1-ragged-fast back4-stepped-fast
model_steps-ragged-one-step-fast laplacian-ragged-fast step4-two-ranges-tiles step4-two-ranges-stepped back4-tiles back4-two-pass-stepped
model_steps-stepped-pipeline model_steps-tiles-pipeline taper_finalize-ragged gather_residual-ragged gather_residual-in-place-ragged
snapshot-ragged
""".split()


def _arena(case):
    return FA.build(case, SC.inputs(case.deck, "true"), damp=lambda a: SC.damped_once(case.deck, a))


def test_the_stream_contract_catalogue_is_unchanged():
    """tests/test_stream_contract.py runs SC.CASES: the same 100 names in the same order as before the edge decks existed."""
    assert len(SC.CASES) == 100 and len(STREAM_CONTRACT_NAMES) == 100
    assert [c.name for c in SC.CASES] == STREAM_CONTRACT_NAMES
    assert not {c.deck for c in SC.CASES} & set(SC.EDGE_DECKS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the edge decks are what the table says, and their cases are not vacuous
# ---------------------------------------------------------------------------------------------------------------------------------------
#            pitch, xlim, zlim, ztap, strips of the pipeline (224 columns each), of the two-step kernel (240), of a 256-column strip
DECK_FACTS = {"flush": (320, 64, 320, 8, 2, 2, 2), "onecol": (512, 69, 449, 10, 3, 3, 2), "narrow": (64, 40, 56, 8, 1, 1, 1)}


@pytest.mark.parametrize("deck", SC.EDGE_DECKS)
def test_the_edge_decks_have_their_properties(deck):
    nxe, nze, nxb, nzb = SC.DECKS[deck]["geom"]
    pitch, xlim, zlim, ztap, pipe, two, one = DECK_FACTS[deck]
    sx, sz, gz = SC.DECKS[deck]["place"]
    assert FA.pitch_of(nze) == pitch
    assert SC.extents_of(SC.inputs(deck, "true")["d"]) == (xlim, zlim, ztap)
    cells = pitch // 4
    assert (-(-cells // 56), -(-cells // 60), -(-pitch // 256)) == (pipe, two, one)
    assert 0 <= sz < zlim and 0 <= gz < zlim and nxb <= sx < min(xlim, nxe - nxb)      # every entry point accepts the placement as it is
    assert nxb + (nxe - 2 * nxb) <= xlim                                               # every receiver row is time-stepped: fdw_dev_back4 runs
    if deck == "flush":
        assert pitch == nze and 2 * 224 - pitch == 128 and 2 * 256 - pitch == 192 and xlim < nxe
    if deck == "onecol":
        assert nze - 2 * 224 == 1 and gz == 448 and 224 <= sz < 448 and pitch - nze == 63
    if deck == "narrow":
        assert nxe < 43 and nxe - 27 < 16 and pitch - nze == 3


@pytest.mark.parametrize("case", SC.FOOTPRINT_CASES + EXC_ALL, ids=repr)
def test_the_footprint_cases_are_not_vacuous(case):
    """No oracle answer holds a sentinel or a NaN, and each differs from what its buffer held before the call in more than half of its
    cells (a field that fdw_dev_taper_finalize alone touches, the `const` d_p of fdw_dev_step included: of the cells that pass damps at all
    -- rows below xlim of the damped strip; the rest it must hand back).  A loop's fields end in two of its four rotating buffers, and which
    two only the real call says (the stand-in context knows no rotation): their answers are held against what EVERY one of b0..b3 held.
    The excitation maps and images are counted over the cells fdwave.h lets the call write (Case.cells: the update extents, the interior);
    for those cases the oracle's answer to the decoys also differs from the true one in more than half of those cells."""
    i = SC.inputs(case.deck, "true")
    arena = _arena(case)
    labels = case.call(_NullCtx(), {name: 0 for name in arena.bufs}, None)
    want = case.want("true")
    before = FA.results(arena, arena.up, labels)
    assert sorted(want) == sorted(before)
    rotating = {name for name in case.scratch if name.startswith("b")}
    where = {label: name for label, name, _, _ in labels}
    for label, a in want.items():
        others = [arena.bufs[n].values(arena.up) for n in sorted(rotating)] if where[label] in rotating else []
        for b in [before[label]] + others:
            _differs(case, i, label, a, b)
    if case in EXC_ALL:
        decoy = case.want("decoy")
        for label, a in want.items():
            share = (a.view(np.uint32) != decoy[label].view(np.uint32))[case.cells.get(label, (slice(None),) * a.ndim)].mean()
            assert share > 0.5, f"{case.name}: {label} of the decoys equals the true answer in {1 - share:.0%} of the cells"


def _differs(case, i, label, a, b):
    assert a.shape == b.shape and a.size > 0, (case.name, label)
    assert np.isfinite(a).all(), (case.name, label)
    for s in SC.SENTINELS:
        assert not (a == s).any(), f"{case.name}: {label} holds the sentinel {s}"
    diff = a.view(np.uint32) != b.view(np.uint32)
    if label in case.cells:
        diff = diff[case.cells[label]]
    if case.name.startswith("taper_finalize") or (case.name.startswith("step_fwd-") and label == "P"):      # a damping pass is all the call owes it
        xlim, _, ztap = SC.extents_of(i["d"])
        diff = diff[:xlim, :ztap]
    assert diff.mean() > 0.5, f"{case.name}: {label} equals what the buffer held before in {1 - diff.mean():.0%} of the cells"


class _NullCtx:
    """Stands in for a context where only the labels of a case are wanted: every dev_* method does nothing; a loop gets back the buffer
    indices it passed in, NOT the ones the real loop ends on (the GPU test takes the labels from the real call) -- so a CPU test that
    needs to know where a loop's fields end must not rely on these labels (test_the_footprint_cases_are_not_vacuous does not)."""

    def __getattr__(self, name):
        assert name.startswith("dev_"), name
        return lambda *a, **k: (k.get("ip", 0), k.get("ipp", 1))


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the checker sees what it looks for
# ---------------------------------------------------------------------------------------------------------------------------------------
def _answered(arena, labels, want):
    """A download as a correct call would leave it: the oracle's answers written over the labelled buffers (those compared as they lie)."""
    down = np.array(arena.up)
    for name, a in arena.outside.items():
        arena.bufs[name].view(down)[:, :arena.nze] = a
    for label, name, post, rows in labels:
        if post is None:
            b = arena.bufs[name]
            v = b.view(down)[:, :b.nze] if b.kind in FA.FIELD_KINDS else b.view(down)
            v[slice(None) if rows is None else rows] = np.asarray(want[label], np.float32).reshape(v[slice(None) if rows is None else rows].shape).view(np.uint32)
    return down


def _control(name):
    case = FP[name]
    arena = _arena(case)
    labels = case.call(_NullCtx(), {n: 0 for n in arena.bufs}, None)
    return case, arena, labels, _answered(arena, labels, case.want("true"))


PLANTS = [
    # case, rule, where the word is planted (buffer, offset in words relative to the buffer's first word, or (row, column)), what the report says
    ("step4-two-ranges-flush", "a", ("O1", -1), "1 floats BEFORE O1"),
    ("step4-two-ranges-flush", "a", ("O1", "end"), "1 floats AFTER the end of O1"),
    ("step4-two-ranges-flush", "a", ("NEW", -40 * 320), "12800 floats BEFORE NEW (40 rows and 0 floats"),
    ("step4-two-ranges-onecol", "b", ("O1", (5, 449)), "O1[5][449] (a padding column)"),
    ("step4-two-ranges-flush", "c", ("v2", (3, 7)), "v2[3][7]"),
    ("step4-two-ranges-flush", "c", ("NEW", (68, 319)), "NEW[68][319]"),
    ("step4-two-ranges-flush", "d", ("O1", (30, 2)), "O1[30][2]"),
    ("step_recv-rows17-30-narrow", "d", ("IMG", (16, 60)), "IMG[16][60]"),
    ("steps_shrink-flush", "d", ("A", (3, 0)), "A[3][0]"),
    ("back4-flush", "c", ("L0", (33, 100)), "L0[33][100]"),
    # the excitation cases: a sentinel pad word, the `const int *d_texc` of a pick, the float before it
    ("excite-onecol-one-step", "b", ("amp", (5, 449)), "amp[5][449] (a padding column)"),
    ("pick-flush-pipeline", "c", ("texc", (63, 319)), "texc[63][319]"),
    ("pick-narrow-pipeline-fast", "a", ("texc", -1), "1 floats BEFORE texc"),
]


def test_control_a_clean_arena_passes():
    for name in sorted({p[0] for p in PLANTS}):
        case, arena, labels, down = _control(name)
        assert (down != arena.up).any()
        assert FA.check(arena, down, labels) == [], name
        if not case.finalized:      # (else the case's own damping pass is still owed to the rows outside)
            assert FA.check(arena, arena.up, labels) == [], name


@pytest.mark.parametrize("name,rule,where,says", PLANTS, ids=[f"plant{k}-rule-{p[1]}-{p[2][0]}-{p[0]}" for k, p in enumerate(PLANTS)])
def test_control_a_planted_word_is_reported_at_its_place(name, rule, where, says):
    case, arena, labels, down = _control(name)
    b = arena.bufs[where[0]]
    w = b.off + (b.size if where[1] == "end" else where[1] if isinstance(where[1], int) else where[1][0] * b.cols + where[1][1])
    down[w] ^= 0x00400000
    bad = FA.check(arena, down, labels)
    assert len(bad) == 1, bad
    assert f"rule ({rule})" in bad[0] and says in bad[0] and case.name in bad[0] and f"arena word {w}:" in bad[0], bad[0]


def test_control_a_changed_border_word_of_the_image_fails_the_answer():
    """A border word of d_img in an interior ROW: rule (d) speaks of rows and is silent; the whole-array answer is what catches it."""
    case, arena, labels, down = _control("exc_image-narrow")
    _assert_answers(case, arena, down, labels)
    nxb = SC.DECKS["narrow"]["geom"][2]
    b = arena.bufs["IMG"]
    down[b.off + (nxb + 1) * b.cols + 2] ^= 0x00400000
    assert FA.check(arena, down, labels) == []
    with pytest.raises(AssertionError, match="img, exc_image-narrow: 1 of"):
        _assert_answers(case, arena, down, labels)
    down[b.off + 1 * b.cols + 2] ^= 0x00400000      # and one in a border row: rule (d) names it
    bad = FA.check(arena, down, labels)
    assert len(bad) == 1 and "rule (d)" in bad[0] and "IMG[1][2]" in bad[0], bad


def test_the_pad_words_and_texc_reach_the_arena_as_words():
    """d_texc is int32: the arena holds exactly the int32 words of the map (no float conversion on the way), the answers carry them back as
    words, and the padding columns of the maps hold their sentinel words, everything else's +0.0."""
    for name in ("excite-onecol-one-step", "pick-narrow-pipeline-fast", "exc_chain-flush-pipeline", "exc_image-onecol"):
        case = FP[name]
        i = SC.inputs(case.deck, "true")
        arena = _arena(case)
        ins = case.ins(i)
        for bname, b in arena.bufs.items():
            pad = b.view(arena.up)[:, b.nze:]
            if b.kind in FA.FIELD_KINDS:
                assert (pad == case.pad_words.get(bname, 0)).all() and (bname in case.pad_words) == (bname in SC.PAD_WORDS), (name, bname)
            if b.kind == "ifield":
                src = ins[bname][1]
                assert src.dtype == np.int32 and (src > 0).all()
                assert np.array_equal(b.view(arena.up)[:, :b.nze].view(np.int32), src), (name, bname)
                assert np.array_equal(b.values(arena.up).view(np.int32), src), (name, bname)
        assert any(b.kind == "ifield" for b in arena.bufs.values()) or name.startswith("exc_image")
    want = FP["excite-onecol-one-step"].want("true")["texc"]
    assert want.dtype == np.float32 and 1 <= want.view(np.int32).min() and np.isfinite(want).all()


@pytest.mark.parametrize("deck", ["ragged"] + list(SC.EDGE_DECKS))
def test_the_image_peak_is_the_interiors(deck):
    """The image cases' peak map: border cells 50 times the noise.  With the peak taken over the whole array no cell would be selected at
    eps = 0.05; over the interior (fdwave.h) most are -- and the answer changes most of the interior."""
    i = SC.inputs(deck, "true")
    inner = SC._interior(deck)
    whole = image_selection(i["amp_img"], SC.EXC_EPS).reshape(i["amp_img"].shape)
    own = image_selection(i["amp_img"][inner], SC.EXC_EPS)
    print(f"{deck}: the whole-array peak selects {int(whole[inner].sum())} interior cells, the interior peak {own.mean():.1%} of them")
    assert whole[inner].sum() == 0 and own.mean() > 0.75
    # ... and a peak word left four times too high by the case's first call (a memset on the wrong stream) would change the selection
    a32 = np.abs(i["amp_img"][inner]).ravel()
    stale = a32 > np.float32(SC.EXC_EPS) * (np.float32(4.0) * a32.max())
    assert (stale != own).mean() > 0.25
    case = FP[f"exc_image-{deck}"]
    want = case.want("true")["img"]
    assert (want[inner].view(np.uint32) != i["img0"][inner].view(np.uint32)).mean() > 0.75
    outside = np.ones(want.shape, bool)
    outside[inner] = False
    assert np.array_equal(want[outside].view(np.uint32), i["img0"][outside].view(np.uint32))


def test_the_excitation_answers_keep_the_entry_words_outside_the_extents():
    """What the whole-array comparison of amp, texc and exc stands on: outside [:xlim, :zlim] the answers ARE the entry words (on the decks
    that have such cells), inside most cells changed; a pick never changes texc."""
    for name in ("excite-flush-one-step", "excite-narrow-pipeline", "pick-flush-two-step", "pick-narrow-one-step"):
        case = FP[name]
        i = SC.inputs(case.deck, "true")
        rows, cols = SC._update_extents(case.deck)
        outside = np.ones(i["amp0"].shape, bool)
        outside[rows, cols] = False
        assert outside.any()
        want = case.want("true")
        entry = dict(amp=i["amp0"], texc=i["texc_maps"].view(np.float32), exc=i["exc0"])
        for label in set(want) & set(entry):
            assert np.array_equal(want[label][outside].view(np.uint32), entry[label][outside].view(np.uint32)), (name, label)
            assert (want[label][rows, cols].view(np.uint32) != entry[label][rows, cols].view(np.uint32)).mean() > 0.5, (name, label)


def test_control_the_fused_back4_labels_leave_the_levels_out():
    """What makes rule (c) cover d_lvl0 / d_lvl1: the fused fdw_dev_back4 names neither, the two-pass form names both."""
    for name, named in (("back4-flush", False), ("back4-two-pass-flush", True)):
        case, arena, labels, _ = _control(name)
        assert ({"L0", "L1"} <= {n for _, n, _, _ in labels}) is named and not set(case.scratch) & {"L0", "L1"}


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def _run(case, torch, after=None):
    """One context, one arena, one call on a stream of the test's own; returns (arena, downloaded words, labels)."""
    ctx = case.make_ctx()
    try:
        arena = _arena(case)
        assert ctx.pitch == arena.pitch
        dev = torch.from_numpy(np.array(arena.up).view(np.int32)).to("cuda:0")
        S = torch.cuda.Stream()
        torch.cuda.synchronize()
        labels = case.call(ctx, arena.pointers(dev.data_ptr()), S.cuda_stream)
        if after is not None:
            with torch.cuda.stream(S):
                after(arena, dev)
        S.synchronize()
        down = dev.cpu().numpy().view(np.uint32)
    finally:
        ctx.close()
    return arena, down, labels


def _assert_answers(case, arena, down, labels):
    want, got = case.want("true"), FA.results(arena, down, labels)
    assert sorted(got) == sorted(want), case.name
    for label in sorted(want):
        assert_bit_equal(got[label], want[label], f"{label}, {case.name}")


@gpu
@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_footprint(case):
    import torch
    arena, down, labels = _run(case, torch)
    bad = FA.check(arena, down, labels)
    try:
        _assert_answers(case, arena, down, labels)
    except AssertionError as e:      # both findings in one report: where the call went, and what it did to the answer
        bad.append(str(e))
    assert not bad, "\n".join(bad)


@gpu
def test_control_a_torch_write_into_a_guard_is_caught():
    """Pure torch, no kernel misbehaves: after a passing call, one word written into a guard on the same stream fails the checker."""
    import torch
    case = FP["steps2-flush-pipeline"]
    arena, down, labels = _run(case, torch)
    assert FA.check(arena, down, labels) == []
    _assert_answers(case, arena, down, labels)
    w = arena.bufs["b2"].off - 3

    def poke(arena, dev):
        dev[w:w + 1] = 0x12345678
    arena, down, labels = _run(case, torch, after=poke)
    bad = FA.check(arena, down, labels)
    assert len(bad) == 1 and "rule (a)" in bad[0] and "3 floats BEFORE b2" in bad[0] and "-> 0x12345678" in bad[0], bad
    _assert_answers(case, arena, down, labels)


@gpu
def test_upload_and_download_stay_inside_an_arena_field():
    """fdw_upload_field into, and fdw_download_field out of, a field of the arena: the value columns arrive, the padding columns of a field
    that held zeros there stay +0.0, the guards and the other field are untouched, and the download returns what lies there."""
    import torch
    case = FP["taper_finalize-onecol"]
    i = SC.inputs("onecol", "true")
    ctx = case.make_ctx()
    try:
        arena = FA.Arena(case, i["d"]["nze"], [("DST", "field", np.full_like(i["p0"], 7.0)), ("SRC", "field", np.asarray(i["pp0"]))])
        dev = torch.from_numpy(np.array(arena.up).view(np.int32)).to("cuda:0")
        ptr = arena.pointers(dev.data_ptr())
        torch.cuda.synchronize()
        ctx.upload(ptr["DST"], i["p0"])
        got = ctx.download(ptr["SRC"])
        torch.cuda.synchronize()
        down = dev.cpu().numpy().view(np.uint32)
    finally:
        ctx.close()
    bad = FA.check(arena, down, [("uploaded", "DST", None, None)])
    assert not bad, "\n".join(bad)
    assert_bit_equal(arena.bufs["DST"].values(down), i["p0"], "the uploaded field")
    assert_bit_equal(got, i["pp0"], "the downloaded field")


@gpu
@pytest.mark.parametrize("deck", ["ragged", "flush", "narrow", "onecol"])
def test_check_field_changes_nothing(deck):
    """fdw_dev_check_field on a clean and on a violating field of the arena (the decks with static rows): the verdicts are right and not a
    word of the arena has changed -- the field is `const`, and the flag the check writes is the library's own."""
    import torch
    import parallel_finite_difference_computation_amd as F
    case = [c for c in ALL_CASES if c.name == f"taper_finalize-{deck}"][0]
    i = SC.inputs(deck, "true")
    ctx = case.make_ctx()
    try:
        arena = FA.Arena(case, i["d"]["nze"], [("CLEAN", "field", np.asarray(i["clean"])), ("PLANTED", "field", np.asarray(i["planted"]))])
        dev = torch.from_numpy(np.array(arena.up).view(np.int32)).to("cuda:0")
        ptr = arena.pointers(dev.data_ptr())
        S = torch.cuda.Stream()
        torch.cuda.synchronize()
        ctx.dev_check_field(ptr["CLEAN"], stream=S.cuda_stream)
        if (i["planted"] != i["clean"]).any():
            with pytest.raises(F.FdwError) as ei:
                ctx.dev_check_field(ptr["PLANTED"], stream=S.cuda_stream)
            assert ei.value.code == SC.EINVAL and "3 cells" in str(ei.value), str(ei.value)
        else:
            ctx.dev_check_field(ptr["PLANTED"], stream=S.cuda_stream)      # no static rows on this deck: nothing to check
        torch.cuda.synchronize()
        down = dev.cpu().numpy().view(np.uint32)
    finally:
        ctx.close()
    bad = FA.check(arena, down, [])
    assert not bad, "\n".join(bad)

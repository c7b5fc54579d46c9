"""TEST HELPER (not a conftest) of tests/test_stream_contract.py: the stream-taking entry points of fdwave.h as CASES -- for each one the
device buffers it works on with two valid argument sets (the TRUE inputs and the DECOYS: another model, other fields, another wavelet, another
gather, another entry image and illumination, other excitation maps), the call itself, and the CPU oracle's answer to either set -- and the late-producer machinery
that runs a case: a delay on the caller's stream, then the true inputs copied over the decoys, then the entry point, then the outputs copied
out, all on that one stream and with no synchronisation before the end.

The answers come from the restatements the other modules already pin: tests/test_line_source.py's line_restatement (the forward chain with
a point or a line source, its trace rows and its illumination; with a point source it is Oracle.forward bit for bit, pinned there on the
CPU), Oracle.slab_step / slab_back_iter (one forward / backward iteration on row ranges), O.mod_steps, tests/context_reuse_cases.py's
oracle_laplacian, numpy slicing / fp32 subtraction for the two copy-like kernels, and tests/excitation_restatement.py's maps_restatement,
pick_restatement and image_formula for the excitation entry points (EXC_CASES, EXC_FOOTPRINT_CASES)."""
import functools
import os
import time

import numpy as np

from conftest import make_deck, random_fields
from context_reuse_cases import oracle_laplacian
from excitation_restatement import image_formula, maps_restatement, pick_restatement
from oracle import oracle as O
from test_line_source import args_of, extents_of, line_restatement

NT = 9                                    # a four-step pass, a two-step pass and an odd tail; 5 + 4 when chained
SENTINELS = (7.0, -7.0, 9.0)              # what pure outputs hold before the call; no oracle answer holds any of them (checked on the CPU)
EINVAL = -1
MOD_FAC = 0.05
EXC_EPS = 0.05                            # fdw_dev_image_excitation's eps in the image cases (noise peaks: |amp| > 0.05 max |amp| holds for most cells)
# ... and in the chain cases, whose amp comes from the excite call: the source sample (the wavelet x 1000) puts the peak near 100 on the
# compat decks while the noise-born amplitudes have a median of 0.38 and a tenth percentile of 0.16 to 0.19 (CPU oracle, all decks), so
# eps = 0.002 puts the threshold near 0.2: most interior cells are selected, some are not
EXC_CHAIN_EPS = 0.002
# what the padding columns of the excitation maps and images hold (fdwave.h: they "keep their words"): 123.5, a quiet NaN, -321.25, a negative quiet NaN
PAD_WORDS = dict(amp=0x42F70000, texc=0x7FC12345, exc=0xC3A0A000, IMG=0xFFC54321, EXC=0xC3A0A000, AMP=0x42F70000, AMPB=0x42F70000, IMGB=0xFFC54321)

# name: geometry (nxe, nze, nxb, nzb), compat, spacings, (sx, sz, gz), tuning every context on it gets on top of its family
DECKS = {
    # the ragged compat grid of tests/context_reuse_cases.py: rows 64..68 never time-stepped, receiver rows 64, 65 among them (record_static,
    # static_receiver_rows and even_steps_tail all have work), zlim 296, ztap 8, pitch 320 > nze
    "ragged": dict(geom=(69, 301, 3, 10), compat=True, dx=10.0, dz=12.5, place=(26, 258, 255), tuning={}),
    # the same grid with every receiver row time-stepped: what fdw_dev_back4 needs
    "stepped": dict(geom=(69, 301, 8, 10), compat=True, dx=10.0, dz=12.5, place=(26, 258, 255), tuning={}),
    # the deck of tests/test_tile_classes.py: 14 chunk rows x 3 strips at 13-row chunks, lean and full tiles in one launch
    "tiles": dict(geom=(180, 500, 12, 14), compat=False, dx=10.0, dz=10.0, place=(84, 300, 310), tuning=dict(xchunk=13)),
    # ---- the edge decks of tests/test_dev_footprint.py (FOOTPRINT_CASES only) ----
    # pitch == nze == 320: no padding column absorbs a stray store; the second pipeline strip (columns 224..447) and the second 256-column
    # strip of the one-step kernels run 128 / 192 columns past the row end, into the next row.  Rows 64..68 static, every receiver row
    # (8..60) time-stepped, so fdw_dev_back4 runs.  xlim 64, zlim 320, ztap 8.  Every placement is accepted as the table gives it.
    "flush": dict(geom=(69, 320, 8, 10), compat=True, dx=10.0, dz=12.5, place=(26, 258, 255), tuning={}),
    # 449 = 2 x 224 + 1: the third pipeline strip owns ONE column (448), which is the receiver column; the source sits in the last owned
    # columns of strip 1 (sz = 446, so the 7 x 7 source of the modelling dialect is cut off by the grid edge at column 448); pitch 512,
    # 63 padding columns.  Whole-grid update: xlim 69, zlim 449.  Every placement is accepted as given.
    "onecol": dict(geom=(69, 449, 8, 10), compat=False, dx=10.0, dz=10.0, place=(26, 446, 448), tuning={}),
    # one partial strip (61 columns, pitch 64) and 41 rows: shorter than the shortest automatic chunk of the pipeline (43) and hardly longer
    # than its 27-step prologue, so every wave spends most of its march outside the grid.  xlim 40, zlim 56, ztap 8.  Placements as given.
    "narrow": dict(geom=(41, 61, 6, 9), compat=True, dx=10.0, dz=12.5, place=(20, 40, 38), tuning={}),
}
EDGE_DECKS = ("flush", "onecol", "narrow")
FAMILIES = {"one-step": -1, "two-step": 1, "pipeline": 4}


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(deck, v):
    """Argument set v ("true" or "decoy") on a deck: everything an entry point reads from device memory."""
    D = DECKS[deck]
    nxe, nze, nxb, nzb = D["geom"]
    nx = nxe - 2 * nxb
    seed = 3 if v == "true" else 11
    d = make_deck(nxe, nze, nxb, nzb, NT, seed=seed, compat=D["compat"], dx=D["dx"], dz=D["dz"])
    rng = np.random.default_rng(500 + seed)
    f = np.float32
    p0, pp0 = random_fields(d, seed + 1, amp=0.1)
    f1, f0 = random_fields(d, seed + 2, amp=0.1)
    pr, ppr = random_fields(d, seed + 3, amp=0.1)
    m0, m1 = random_fields(d, seed + 4, amp=1e-3)
    base = O.ricker_wavelet(NT, d["dt"], 30.0)
    srce = (base * 1000.0 + 0.5).astype(f) if v == "true" else (base * 700.0 + 3.0).astype(f)
    clean = np.array(p0)
    planted = np.array(clean)
    xlim, _, ztap = extents_of(d)
    if D["compat"] and xlim < nxe and ztap > 0:
        planted[xlim, 0], planted[nxe - 1, ztap - 1], planted[min(xlim + 1, nxe - 1), 3] = 1e-30, -4.0, 2.5
    # the excitation maps, from a generator of their own (the arrays above are what they were before these existed).  Every texc word is
    # positive: as float words the answers are subnormals, not NaNs
    erng = np.random.default_rng(900 + seed)
    nxb, nzb = d["nxb"], d["nzb"]
    amp0 = (0.01 * erng.standard_normal((nxe, nze))).astype(f)
    exc0 = erng.standard_normal((nxe, nze)).astype(f)
    texc_maps = erng.integers(100, 1100, (nxe, nze)).astype(np.int32)          # no iteration writes (excite) or meets (pick) any of them
    texc_pick = erng.integers(1, NT + 4, (nxe, nze)).astype(np.int32)           # uniform in [1, NT + 3]: with top = NT, 9 of 12 values meet an iteration
    amp_img = erng.standard_normal((nxe, nze)).astype(f)                        # a peak map whose border cells tower over the interior
    border = np.ones((nxe, nze), bool)
    border[nxb:nxe - nxb, nzb:nze - nzb] = False
    amp_img[border] *= f(50.0)
    exc_maps = dict(amp0=amp0, exc0=exc0, texc_maps=texc_maps, texc_pick=texc_pick, amp_img=amp_img)
    return _freeze(dict(exc_maps, d=d, v2=d["v2"], p0=p0, pp0=pp0, f1=f1, f0=f0, pr=pr, ppr=ppr, m0=m0, m1=m1, srce=srce,
                        msrce=(1e-2 * rng.standard_normal(NT)).astype(f), w=rng.standard_normal((NT, nx)).astype(f),
                        il0=(0.5 + rng.random((nxe, nze))).astype(f), img0=rng.standard_normal((nxe, nze)).astype(f),
                        samples=rng.standard_normal((4, nx)).astype(f), ga=rng.standard_normal((NT, nx)).astype(f),
                        gb=rng.standard_normal((NT, nx)).astype(f), lap_in=rng.standard_normal((nxe, nze)).astype(f), clean=clean, planted=planted))


@functools.lru_cache(maxsize=None)
def oracle(deck, numerics):
    D = DECKS[deck]
    return O.Oracle(*args_of(inputs(deck, "true")["d"]), compat=D["compat"], numerics=numerics)


def damped_once(deck, field):
    """The field after the one damping pass fdw_dev_taper_finalize applies to it (Oracle.slab_step with no row to step)."""
    f = np.array(field, np.float32, order="C")
    oracle(deck, 0).slab_step(0, f, np.zeros_like(f), np.ascontiguousarray(inputs(deck, "true")["v2"]), 0, 0, -1, 0, 0.0)
    return f


@functools.lru_cache(maxsize=None)
def chain(deck, numerics, v, line, nsteps=NT):
    """P (damped once, as fdw_dev_taper_finalize leaves it), PP, data[nx][nsteps] and illum after nsteps forward iterations from (p0, pp0, il0)."""
    i = inputs(deck, v)
    sx, sz, gz = DECKS[deck]["place"]
    return _freeze(line_restatement(oracle(deck, numerics), i["d"], i["v2"], i["w"][:nsteps] if line else None, sz, gz=gz, p0=i["p0"], pp0=i["pp0"],
                                    il0=i["il0"], point=None if line else (sx, i["srce"][:nsteps])))


@functools.lru_cache(maxsize=None)
def back_chain(deck, numerics, v, n, step_source):
    """n iterations of fd_back's loop body (Oracle.slab_back_iter on the whole grid) from (f1, f0, pr, ppr, img0) with the sample rows
    samples[0..n): F = the reconstructed source fields, r_new / r_old = the receiver pair after the last swap (r_old damped as the next
    iteration would read it: fdw_dev_taper_finalize), img."""
    i = inputs(deck, v)
    nxe = i["d"]["nxe"]
    gz = DECKS[deck]["place"][2]
    f1, f0, pr, ppr, img = (np.array(i[k], np.float32, order="C") for k in ("f1", "f0", "pr", "ppr", "img0"))
    F = []
    for j in range(n):
        oracle(deck, numerics).slab_back_iter(0, step_source, f1, f0, pr, ppr, i["v2"], 0, nxe, i["samples"][j], gz, img)
        if step_source:
            F.append(f0.copy())
            f1, f0 = f0, f1
        pr, ppr = ppr, pr
    out = dict(r_new=pr, r_old=ppr, img=img)
    out.update({f"F{j}": a for j, a in enumerate(F)})
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def shrink_chain(deck, numerics, v, nsteps):
    """nsteps cycle steps j = 1.. of a slab with neighbours on both sides: step j updates rows [4 j, nxe - 4 j) (fdw_dev_steps_shrink)."""
    i = inputs(deck, v)
    sx, sz, _ = DECKS[deck]["place"]
    nxe = i["d"]["nxe"]
    P, PP = np.array(i["p0"], np.float32, order="C"), np.array(i["pp0"], np.float32, order="C")
    for k in range(nsteps):
        P, PP = PP, P
        oracle(deck, numerics).slab_step(0, P, PP, i["v2"], 4 * (k + 1), nxe - 4 * (k + 1), sx, sz, float(i["srce"][k]))
    return _freeze(dict(P=P, PP=PP))


@functools.lru_cache(maxsize=None)
def mod_chain(deck, numerics, v):
    i = inputs(deck, v)
    nxe, nze, nxb, nzb = DECKS[deck]["geom"]
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    D = DECKS[deck]
    sx, sz, gz = D["place"]
    P, PP, data = O.mod_steps(8, nx, nz, nxb, nzb, D["dx"], D["dz"], 0.001, MOD_FAC, i["v2"], sx, sz, gz, i["msrce"],
                              O.mod_taper_apply(i["m0"], nx, nz, nxb, nzb, MOD_FAC, 1), O.mod_taper_apply(i["m1"], nx, nz, nxb, nzb, MOD_FAC, 2),
                              numerics=numerics)
    return _freeze(dict(P=P, PP=PP, rec=np.ascontiguousarray(data.T)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """name; deck; numerics; two_step (None: the context's default); dialect.
    ins(i) -> {buffer: (kind, array)} for an argument set i; kind "field" = [nxe][pitch] on the device, "flat" = dense, "ifield" = a field of
              int32 words (d_texc): an int32 array, uploaded, downloaded and compared as words (its answer: the words seen as float32).
    outs   -> {buffer: (kind, shape, sentinel)}: pure outputs.
    call(ctx, ptr, stream) -> [(label, buffer, post or None, rows or None)]: makes the call(s) and says where each answer lies.
    want(v) -> {label: array}.
    What tests/test_dev_footprint.py reads on top (fdwave.h's words about who writes what, not what the code does):
    scratch       buffers the call may overwrite although no label names them (the rotating buffers of a loop);
    written_rows  {buffer: rows} where the rows a call may write are not the rows of the buffer's label (an image compared on its
                  interior; fdw_dev_steps_shrink, whose rows between the valid ones hold intermediate values);
    finalized     buffers the case itself hands to fdw_dev_taper_finalize after the call: their rows outside the rows asked for come back
                  damped once (damped_once), not as uploaded;
    tuning        set_tuning arguments of this case alone, on top of the deck's;
    pad_words     {buffer: 32-bit word} what the padding columns of a field hold before the call instead of +0.0 (and must hold after it);
    cells         {label: (rows, columns)} the cells fdwave.h lets the call write in a label's array where that is not the whole array: the
                  non-vacuity tests count changed / differing cells there."""

    def __init__(self, name, deck, numerics, two_step, ins, outs, call, want, dialect=0, env=None, scratch=(), written_rows=None, tuning=None,
                 finalized=(), pad_words=None, cells=None):
        self.name, self.deck, self.numerics, self.two_step, self.dialect, self.env = name, deck, numerics, two_step, dialect, env or {}
        self.ins, self.outs, self.call, self.want = ins, outs, call, want
        self.scratch, self.written_rows, self.tuning, self.finalized = tuple(scratch), dict(written_rows or {}), dict(tuning or {}), tuple(finalized)
        self.pad_words, self.cells = dict(pad_words or {}), dict(cells or {})

    def make_ctx(self):
        """The context of the case; self.env holds switches the library reads when a context is created."""
        old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        try:
            return self._make_ctx()
        finally:
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v

    def _make_ctx(self):
        import parallel_finite_difference_computation_amd as F
        D = DECKS[self.deck]
        d = inputs(self.deck, "true")["d"]
        if self.dialect == 1:
            ctx = F.FDWave(8, d["nxe"], d["nze"], d["nxb"], d["nzb"], NT, MOD_FAC, D["dx"], D["dz"], 0.001, device=0, dialect=1, numerics=self.numerics)
        else:
            ctx = F.FDWave(*args_of(d), compat=D["compat"], device=0, numerics=self.numerics)
        if self.two_step is not None:      # (one set_tuning call: it sets every knob, the ones left out to their defaults)
            ctx.set_tuning(two_step=self.two_step, **dict(D["tuning"], **self.tuning))
            assert ctx.steps_per_pass() == {-1: 1, 1: 2 if self.dialect == 0 else 1, 4: 4}[self.two_step]
        elif self.tuning:
            ctx.set_tuning(**self.tuning)
        return ctx

    def __repr__(self):
        return self.name


CASES = []                # what tests/test_stream_contract.py runs: 100 cases, names and order pinned by tests/test_dev_footprint.py
FOOTPRINT_CASES = []      # the same builders on the edge decks, and the row-range cases: tests/test_dev_footprint.py only


def _add(name, deck, numerics, two_step, ins, outs, call, want, to=None, **kw):
    tag = f"{name}-{deck}" + ("" if two_step is None else "-" + {v: k for k, v in FAMILIES.items()}[two_step]) + ("-fast" if numerics else "")
    (CASES if to is None else to).append(Case(tag, deck, numerics, two_step, ins, outs, call, want, **kw))


def _dims(deck):
    nxe, nze, nxb, nzb = DECKS[deck]["geom"]
    return nxe, nze, nxb, nzb, nxe - 2 * nxb, nze - 2 * nzb


def _loop_case(kind, deck, numerics, two_step, split=((0, NT),), to=None):
    """The forward loops over four rotating buffers: kind = steps2 | record | illum | record_illum | line | line_rec | line_ill | line_rec_ill."""
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    sx, sz, gz = DECKS[deck]["place"]
    line = kind.startswith("line")
    rec = kind in ("record", "record_illum", "line_rec", "line_rec_ill")
    ill = kind in ("illum", "record_illum", "line_ill", "line_rec_ill")

    def ins(i):
        b = dict(b0=("field", i["p0"]), b1=("field", i["pp0"]), v2=("field", i["v2"]), src=("flat", i["w"] if line else i["srce"]))
        if ill:
            b["il"] = ("field", i["il0"])
        return b

    outs = dict(b2=("field", (nxe, nze), 7.0), b3=("field", (nxe, nze), -7.0))
    if rec:
        outs["rec"] = ("flat", (NT, nx), 9.0)

    def call(ctx, p, stream):
        bufs = [p["b0"], p["b1"], p["b2"], p["b3"]]
        ip, ipp = 0, 1
        for k, (it0, n) in enumerate(split):
            a = dict(first_pp_twice=k > 0, ip=ip, ipp=ipp, stream=stream)
            if kind == "steps2":
                ip, ipp = ctx.dev_steps2(bufs, p["v2"], p["src"], sx, sz, it0, n, **a)
            elif kind == "record":
                ip, ipp = ctx.dev_record_steps(bufs, p["v2"], p["src"], sx, sz, gz, p["rec"], it0, n, **a)
            elif kind == "illum":
                ip, ipp = ctx.dev_illum_steps(bufs, p["v2"], p["src"], sx, sz, p["il"], it0, n, **a)
            elif kind == "record_illum":
                ip, ipp = ctx.dev_record_illum_steps(bufs, p["v2"], p["src"], sx, sz, gz, p["rec"], p["il"], it0, n, **a)
            elif kind == "line_rec_ill":
                ip, ipp = ctx.dev_line_record_illum_steps(bufs, p["v2"], p["src"], sz, gz, p["rec"], p["il"], it0, n, **a)
            else:
                ip, ipp = ctx.dev_line_steps(bufs, p["v2"], p["src"], sz, it0, n, gz=gz, d_rec=p["rec"] if rec else None, d_illum=p["il"] if ill else None, **a)
        ctx.dev_taper_finalize(bufs[ip], stream=stream)
        out = [("PP", f"b{ipp}", None, None), ("P", f"b{ip}", None, None)]
        if rec:
            out.append(("rec", "rec", None, None))
        if ill:
            out.append(("illum", "il", None, None))
        return out

    def want(v):
        c = chain(deck, numerics, v, line)
        out = dict(PP=c["PP"], P=c["P"])
        if rec:
            out["rec"] = np.ascontiguousarray(c["data"].T)
        if ill:
            out["illum"] = c["illum"]
        return out

    _add(kind + ("" if len(split) == 1 else "-chained"), deck, numerics, two_step, ins, outs, call, want, to=to, scratch=("b0", "b1", "b2", "b3"))


LOOP_KINDS = ("steps2", "record", "illum", "record_illum", "line", "line_rec", "line_ill", "line_rec_ill")
for _num in (0, 1):
    for _kind in LOOP_KINDS:
        for _fam, _deck in ((-1, "ragged"), (1, "ragged"), (4, "stepped")):
            _loop_case(_kind, _deck, _num, _fam)
    _loop_case("record", "ragged", _num, 4)               # the pipeline's trace rows with static receiver rows beside them
for _kind in ("steps2", "record", "line"):                 # 5 + 4 steps, no host synchronisation in between
    for _fam, _deck in ((-1, "ragged"), (1, "ragged"), (4, "stepped")):
        _loop_case(_kind, _deck, 0, _fam, split=((0, 5), (5, 4)))
for _kind in ("steps2", "record", "illum", "record_illum", "line", "line_rec_ill"):      # lean and full tiles behind the late producer
    _loop_case(_kind, "tiles", 0, 4)
_loop_case("steps2", "tiles", 1, 4)


def _two_buffer_case(kind, deck, numerics, to=None):
    """fdw_dev_steps (9 steps) and fdw_dev_steps_shrink (3 cycle steps, both sides shrinking) on two buffers: always the one-step kernel."""
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    sx, sz, gz = DECKS[deck]["place"]
    n = NT if kind == "steps" else 3
    rows = None if kind == "steps" else slice(4 * n, nxe - 4 * n)

    def ins(i):
        return dict(A=("field", i["p0"]), B=("field", i["pp0"]), v2=("field", i["v2"]), src=("flat", i["srce"]))

    def call(ctx, p, stream):
        if kind == "steps":
            ctx.dev_steps(p["A"], p["B"], p["v2"], p["src"], sx, sz, 0, n, False, stream=stream)
        else:
            ctx.dev_steps_shrink(p["A"], p["B"], p["v2"], p["src"], sx, sz, 0, n, False, 1, 1, 1, stream=stream)
        ctx.dev_taper_finalize(p["B"], stream=stream)      # n is odd: the newest field lies in the buffer passed as d_p
        return [("PP", "A", None, rows), ("P", "B", None, rows)]

    def want(v):
        c = chain(deck, numerics, v, False) if kind == "steps" else shrink_chain(deck, numerics, v, n)
        return dict(PP=c["PP"] if rows is None else c["PP"][rows], P=c["P"] if rows is None else c["P"][rows])

    # fdw_dev_steps_shrink: the rows between the outermost four on either side and the valid ones hold intermediate values
    _add(kind, deck, numerics, None, ins, {}, call, want, to=to, scratch=("A", "B"),
         written_rows=None if rows is None else dict(A=slice(4, nxe - 4), B=slice(4, nxe - 4)), finalized=() if rows is None else ("B",))


def _pass_case(kind, deck, numerics, ranges=None, to=None, tag="-two-ranges"):
    """One pass of fdw_dev_step (FWD), fdw_dev_step2 or fdw_dev_step4 from (p0, pp0); step4 optionally on two row ranges."""
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    sx, sz, gz = DECKS[deck]["place"]
    n = dict(step_fwd=1, step2=2, step4=4)[kind]
    rows = None
    if ranges:
        rows = np.zeros(nxe, bool)
        rows[ranges["r0"]:ranges["r1"]] = True
        rows[ranges["r0b"]:ranges["r1b"]] = True

    def ins(i):      # forward()'s convention: the kernel's p (newest) is pp0
        return dict(NEW=("field", i["pp0"]), OLD=("field", i["p0"]), v2=("field", i["v2"]), src=("flat", i["srce"]))

    outs = {} if kind == "step_fwd" else dict(O1=("field", (nxe, nze), 7.0), O2=("field", (nxe, nze), -7.0))

    def call(ctx, p, stream):
        from parallel_finite_difference_computation_amd._lib import MODE_FWD
        if kind == "step_fwd":
            ctx.dev_step(MODE_FWD, p["NEW"], p["OLD"], p["v2"], 0, nxe, pp_twice=False, d_inj=p["src"], inj_x=sx, inj_z=sz, stream=stream)
            ctx.dev_taper_finalize(p["NEW"], stream=stream)
            return [("PP", "OLD", None, None), ("P", "NEW", None, None)]
        if kind == "step2":
            ctx.dev_step2(p["NEW"], p["OLD"], p["v2"], p["O1"], p["O2"], pp_twice=False, d_srce_it=p["src"], sx=sx, sz=sz, stream=stream)
        else:
            ctx.dev_step4(p["NEW"], p["OLD"], p["v2"], p["O1"], p["O2"], pp_twice=False, d_srce_it=p["src"], sx=sx, sz=sz,
                          xchunk=DECKS[deck]["tuning"].get("xchunk", 0), stream=stream, **(ranges or {}))
        ctx.dev_taper_finalize(p["O1"], stream=stream)
        return [("PP", "O2", None, rows), ("P", "O1", None, rows)]

    def want(v):
        c = chain(deck, numerics, v, False, n)
        return dict(PP=c["PP"] if rows is None else c["PP"][rows], P=c["P"] if rows is None else c["P"][rows])

    _add(kind + (tag if ranges else ""), deck, numerics, None, ins, outs, call, want, to=to, finalized=("O1",) if ranges else ())


def _back_case(kind, deck, numerics, two_pass=False, to=None):
    """fdw_dev_step PLAIN / RECV, fdw_dev_back_iter (step_source 0 / 1) and fdw_dev_back4 from noise-filled source and receiver fields.
    The image is compared on the interior cells: d_img lies on the extended grid, the kernels also accumulate in its border cells inside
    their launch extents, and only the interior is what fd_back's kernel_img defines (and what the host entry points return).
    two_pass (FDW_NO_BACK_FUSED): fdw_dev_back4 as a PLAIN_ALL and a RECV pass, which also leaves F_it, F_it+1 in d_lvl0, d_lvl1 -- the fused
    pass keeps those two levels on the chip and does not touch the two buffers."""
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    gz = DECKS[deck]["place"][2]

    def crop(a):
        return np.ascontiguousarray(a[nxb:nxb + nx, nzb:nzb + nz])

    def ins(i):
        return dict(F1=("field", i["f1"]), F0=("field", i["f0"]), PR=("field", i["pr"]), PPR=("field", i["ppr"]), v2=("field", i["v2"]),
                    IMG=("field", i["img0"]), SAMP=("flat", i["samples"]))

    outs = {}
    if kind == "back4":
        outs = {k: ("field", (nxe, nze), s) for k, s in (("FO1", 7.0), ("FO2", -7.0), ("L0", 7.0), ("L1", -7.0), ("RO1", 9.0), ("RO2", -7.0))}

    def call(ctx, p, stream):
        from parallel_finite_difference_computation_amd._lib import MODE_PLAIN, MODE_RECV
        if kind == "step_plain":
            ctx.dev_step(MODE_PLAIN, p["F1"], p["F0"], p["v2"], 0, nxe, pp_twice=False, stream=stream)
            return [("F0", "F0", None, None)]
        if kind == "step_recv":
            ctx.dev_step(MODE_RECV, p["PR"], p["PPR"], p["v2"], 0, nxe, pp_twice=False, d_inj=p["SAMP"], inj_x=0, inj_z=gz, d_psrc=p["F1"], d_img=p["IMG"],
                         stream=stream)
            return [("r_new", "PPR", None, None), ("img", "IMG", crop, None)]
        if kind in ("back_iter0", "back_iter1"):
            ss = int(kind[-1])
            ctx.dev_back_iter(ss, p["F1"], p["F0"], p["PR"], p["PPR"], p["v2"], 0, nxe, False, p["SAMP"], gz, p["IMG"], stream=stream)
            return [("r_new", "PPR", None, None), ("img", "IMG", crop, None)] + ([("F0", "F0", None, None)] if ss else [])
        ctx.dev_back4(p["F1"], p["F0"], p["FO1"], p["FO2"], p["L0"], p["L1"], p["PR"], p["PPR"], p["RO1"], p["RO2"], p["v2"], p["SAMP"], nx, gz, p["IMG"],
                      pp_twice=False, xchunk=DECKS[deck]["tuning"].get("xchunk", 0), stream=stream)
        ctx.dev_taper_finalize(p["RO1"], stream=stream)
        levels = [("F0", "L0", None, None), ("F1", "L1", None, None)] if two_pass else []
        return levels + [("F2", "FO1", None, None), ("F3", "FO2", None, None), ("r_new", "RO2", None, None), ("r_old", "RO1", None, None),
                         ("img", "IMG", crop, None)]

    def want(v):
        c = dict(back_chain(deck, numerics, v, 4 if kind == "back4" else 1, 0 if kind in ("step_recv", "back_iter0") else 1))
        c["img"] = crop(c["img"])
        if kind == "back4":
            return {k: a for k, a in c.items() if two_pass or k not in ("F0", "F1")}
        if kind == "step_plain":
            return dict(F0=c["F0"])
        return {k: c[k] for k in ("r_new", "img") + (("F0",) if kind == "back_iter1" else ())}

    _add(kind + ("-two-pass" if two_pass else ""), deck, numerics, None, ins, outs, call, want, to=to, env={"FDW_NO_BACK_FUSED": "1"} if two_pass else None)


def _model_case(deck, numerics, two_step, to=None):
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    sx, sz, gz = DECKS[deck]["place"]

    def ins(i):
        return dict(A=("field", i["m0"]), B=("field", i["m1"]), v2=("field", i["v2"]), src=("flat", i["msrce"]))

    def call(ctx, p, stream):
        ctx.dev_model_steps(p["A"], p["B"], p["v2"], p["src"], sx, sz, gz, p["rec"], 0, NT, stream=stream)
        # the device arrays hold the fields before the damping the loop still owes them (P one pass short, PP two); NT is odd: they swapped
        return [("rec", "rec", None, None), ("P", "B", lambda a: O.mod_taper_apply(a, nx, nz, nxb, nzb, MOD_FAC, 1), None),
                ("PP", "A", lambda a: O.mod_taper_apply(a, nx, nz, nxb, nzb, MOD_FAC, 2), None)]

    _add("model_steps", deck, numerics, two_step, ins, dict(rec=("flat", (NT, nx), 9.0)), call, lambda v: dict(mod_chain(deck, numerics, v)), to=to, dialect=1,
         scratch=("A", "B"))


def _small_case(kind, deck, numerics=0, to=None):
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    D = DECKS[deck]
    DEC = 3

    if kind == "taper_finalize":
        ins = lambda i: dict(FLD=("field", i["p0"]))                                                                           # noqa: E731
        outs = {}
        call = lambda ctx, p, s: (ctx.dev_taper_finalize(p["FLD"], stream=s), [("field", "FLD", None, None)])[1]             # noqa: E731

        def want(v):
            i = inputs(deck, v)
            f = np.array(i["p0"], np.float32, order="C")
            oracle(deck, numerics).slab_step(0, f, np.array(i["pp0"], np.float32, order="C"), i["v2"], 0, 0, -1, 0, 0.0)      # one damping pass, no row stepped
            return dict(field=f)
    elif kind == "laplacian":
        ins = lambda i: dict(IN=("field", i["lap_in"]))                                                                        # noqa: E731
        outs = dict(LAP=("field", (nxe, nze), 7.0))
        call = lambda ctx, p, s: (ctx.dev_laplacian(p["IN"], p["LAP"], stream=s), [("lap", "LAP", None, None)])[1]            # noqa: E731
        want = lambda v: dict(lap=oracle_laplacian(8, nxe, nze, D["dx"], D["dz"], inputs(deck, v)["lap_in"], numerics))       # noqa: E731
    elif kind in ("gather_residual", "gather_residual-in-place"):
        inplace = kind.endswith("in-place")
        ins = lambda i: dict(GA=("flat", i["ga"]), GB=("flat", i["gb"]))                                                       # noqa: E731
        outs = {} if inplace else dict(OUT=("flat", (NT, nx), 9.0))
        call = lambda ctx, p, s: (ctx.dev_gather_residual(p["GA"], p["GB"], p["GA" if inplace else "OUT"], NT * nx, stream=s),   # noqa: E731
                                  [("resid", "GA" if inplace else "OUT", None, None)])[1]
        want = lambda v: dict(resid=(inputs(deck, v)["ga"] - inputs(deck, v)["gb"]).astype(np.float32))                       # noqa: E731
    else:
        assert kind == "snapshot"
        ins = lambda i: dict(FLD=("field", i["p0"]))                                                                           # noqa: E731
        outs = dict(FRAME=("flat", (-(-nx // DEC), -(-nz // DEC)), 9.0))
        call = lambda ctx, p, s: (ctx.dev_snapshot(p["FLD"], DEC, p["FRAME"], stream=s), [("frame", "FRAME", None, None)])[1]  # noqa: E731
        want = lambda v: dict(frame=np.ascontiguousarray(inputs(deck, v)["p0"][nxb:nxb + nx:DEC, nzb:nzb + nz:DEC]))          # noqa: E731
    _add(kind, deck, numerics, None, ins, outs, call, want, to=to)


for _num in (0, 1):
    _two_buffer_case("steps", "ragged", _num)
    _two_buffer_case("steps_shrink", "ragged", _num)
    for _kind in ("step_fwd", "step2"):
        _pass_case(_kind, "ragged", _num)
    _pass_case("step4", "stepped", _num)
    for _kind in ("step_plain", "step_recv", "back_iter0", "back_iter1"):
        _back_case(_kind, "ragged", _num)
    _back_case("back4", "stepped", _num)
    _model_case("ragged", _num, -1)
    _small_case("laplacian", "ragged", _num)
_pass_case("step4", "tiles", 0, ranges=dict(r0=16, r1=50, r0b=120, r1b=164))
_pass_case("step4", "stepped", 0, ranges=dict(r0=0, r1=30, r0b=36, r1b=64))
_back_case("back4", "tiles", 0)
_back_case("back4", "stepped", 0, two_pass=True)
_model_case("stepped", 0, 4)
_model_case("tiles", 0, 4)
for _kind in ("taper_finalize", "gather_residual", "gather_residual-in-place", "snapshot"):
    _small_case(_kind, "ragged")

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------------------------------------------
# FOOTPRINT_CASES (tests/test_dev_footprint.py): calls on row ranges, and the catalogue on the edge decks
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rows_case(kind, deck, r0, r1, tuning=None, to=None):
    """fdw_dev_step FWD / PLAIN / RECV and fdw_dev_back_iter(step_source = 1) on local rows [r0, r1) only, from fresh fields (pp_twice = 0),
    against Oracle.slab_step / slab_back_iter on the same rows.  The field read as d_p is not finalized afterwards: it is `const` and must
    come back as it went in.  The image is compared on its interior; the rows the call may write in it are [r0, r1)."""
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    sx, sz, gz = DECKS[deck]["place"]
    rows = slice(r0, r1)
    irows = slice(max(r0, nxb) - nxb, max(min(r1, nxb + nx), nxb) - nxb)      # the interior rows among them, as rows of the cropped image

    def crop(a):
        return np.ascontiguousarray(a[nxb:nxb + nx, nzb:nzb + nz])

    if kind == "step_fwd":
        ins = lambda i: dict(NEW=("field", i["pp0"]), OLD=("field", i["p0"]), v2=("field", i["v2"]), src=("flat", i["srce"]))      # noqa: E731
    else:
        ins = lambda i: dict(F1=("field", i["f1"]), F0=("field", i["f0"]), PR=("field", i["pr"]), PPR=("field", i["ppr"]), v2=("field", i["v2"]),      # noqa: E731
                             IMG=("field", i["img0"]), SAMP=("flat", i["samples"]))

    def call(ctx, p, stream):
        from parallel_finite_difference_computation_amd._lib import MODE_FWD, MODE_PLAIN, MODE_RECV
        if kind == "step_fwd":
            ctx.dev_step(MODE_FWD, p["NEW"], p["OLD"], p["v2"], r0, r1, pp_twice=False, d_inj=p["src"], inj_x=sx, inj_z=sz, stream=stream)
            return [("PP", "OLD", None, rows)]
        if kind == "step_plain":
            ctx.dev_step(MODE_PLAIN, p["F1"], p["F0"], p["v2"], r0, r1, pp_twice=False, stream=stream)
            return [("F0", "F0", None, rows)]
        if kind == "step_recv":
            ctx.dev_step(MODE_RECV, p["PR"], p["PPR"], p["v2"], r0, r1, pp_twice=False, d_inj=p["SAMP"], inj_x=0, inj_z=gz, d_psrc=p["F1"], d_img=p["IMG"],
                         stream=stream)
            return [("r_new", "PPR", None, rows), ("img", "IMG", crop, irows)]
        ctx.dev_back_iter(1, p["F1"], p["F0"], p["PR"], p["PPR"], p["v2"], r0, r1, False, p["SAMP"], gz, p["IMG"], stream=stream)
        return [("r_new", "PPR", None, rows), ("img", "IMG", crop, irows), ("F0", "F0", None, rows)]

    @functools.lru_cache(maxsize=None)
    def answers(v):
        i = inputs(deck, v)
        orc = oracle(deck, 0)
        if kind == "step_fwd":
            P, PP = np.array(i["pp0"], np.float32, order="C"), np.array(i["p0"], np.float32, order="C")
            orc.slab_step(0, P, PP, i["v2"], r0, r1, sx, sz, float(i["srce"][0]))
            return _freeze(dict(PP=PP[rows]))
        f1, f0, pr, ppr, img = (np.array(i[k], np.float32, order="C") for k in ("f1", "f0", "pr", "ppr", "img0"))
        if kind == "step_plain":      # F_k = leap-frog(f1, f0) over f0: no taper, no source (R:317-318) -- the source half of slab_back_iter
            orc.slab_back_iter(0, 1, f1, f0, pr, ppr, i["v2"], r0, r1, i["samples"][0], gz, img)
            return _freeze(dict(F0=f0[rows]))
        ss = 0 if kind == "step_recv" else 1
        orc.slab_back_iter(0, ss, f1, f0, pr, ppr, i["v2"], r0, r1, i["samples"][0], gz, img)
        out = dict(r_new=ppr[rows], img=crop(img)[irows])
        if ss:
            out["F0"] = f0[rows]
        return _freeze(out)

    _add(f"{kind}-rows{r0}-{r1}", deck, 0, None, ins, {}, call, lambda v: dict(answers(v)), to=to, tuning=tuning,
         written_rows={} if kind in ("step_fwd", "step_plain") else dict(IMG=rows))


def _footprint_cases():
    to = FOOTPRINT_CASES
    def limits(deck):      # nxe, xlim as fdw_get_extents gives it (pinned per deck by tests/test_dev_footprint.py)
        nxe = DECKS[deck]["geom"][0]
        return nxe, 8 * (nxe // 8) if DECKS[deck]["compat"] else nxe

    for deck in ("ragged",) + EDGE_DECKS:
        nxe, xlim = limits(deck)
        for kind in ("step_fwd", "step_plain", "step_recv", "back_iter1"):
            _rows_case(kind, deck, 0, 9, to=to)
            # the shortest chunk: fill_geometry (csrc/fdw_api.cpp) takes the context's xchunk for the one-step kernels as it stands, so
            # every wave marches one row -- thirteen chunk borders inside the range; the answer does not depend on it, the footprint could
            _rows_case(kind, deck, 17, 30, tuning=dict(xchunk=1), to=to)
            _rows_case(kind, deck, xlim - 9, nxe, to=to)
    for deck in EDGE_DECKS:
        nxe, xlim = limits(deck)
        for kind in LOOP_KINDS:
            for fam in (-1, 1, 4):
                _loop_case(kind, deck, 0, fam, to=to)
        for fam in (-1, 1, 4):      # FAST kernels are separate instantiations: one loop per family
            _loop_case("steps2", deck, 1, fam, to=to)
        _two_buffer_case("steps", deck, 0, to=to)
        _two_buffer_case("steps_shrink", deck, 0, to=to)
        for kind in ("step_fwd", "step2", "step4"):
            _pass_case(kind, deck, 0, to=to)
        # two row ranges that touch row 0 and the last time-stepped row, six rows apart
        _pass_case("step4", deck, 0, ranges=dict(r0=0, r1=(xlim - 6) // 2, r0b=(xlim - 6) // 2 + 6, r1b=xlim), to=to)
        if xlim + 4 < nxe:      # static rows (flush: 64..68) among the rows asked for: copied from the inputs, they and no others
            # a range that ends inside them, a gap of two static rows, a second range that holds static rows only
            _pass_case("step4", deck, 0, ranges=dict(r0=0, r1=xlim + 1, r0b=xlim + 3, r1b=nxe), to=to, tag="-static-gap")
            # no time-stepped row asked for at all: nothing is launched, two static rows are copied
            _pass_case("step4", deck, 0, ranges=dict(r0=xlim, r1=xlim + 2, r0b=0, r1b=0), to=to, tag="-static-only")
        for kind in ("step_plain", "step_recv", "back_iter0", "back_iter1", "back4"):
            _back_case(kind, deck, 0, to=to)
        _back_case("back4", deck, 0, two_pass=True, to=to)
        _model_case(deck, 0, -1, to=to)
        _model_case(deck, 0, 4, to=to)
        for kind in ("laplacian", "taper_finalize", "snapshot", "gather_residual", "gather_residual-in-place"):
            _small_case(kind, deck, to=to)


_footprint_cases()
assert len({c.name for c in CASES + FOOTPRINT_CASES}) == len(CASES) + len(FOOTPRINT_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------------
# EXC_CASES (both modules) and EXC_FOOTPRINT_CASES (tests/test_dev_footprint.py): the excitation entry points
# ---------------------------------------------------------------------------------------------------------------------------------------
EXC_CASES = []                # fdw_dev_excite_steps, fdw_dev_line_pick_steps, fdw_dev_image_excitation on ragged / stepped / tiles
EXC_FOOTPRINT_CASES = []      # the same builders on the edge decks


def _interior(deck):
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    return slice(nxb, nxb + nx), slice(nzb, nzb + nz)


def _update_extents(deck):
    xlim, zlim, _ = extents_of(inputs(deck, "true")["d"])
    return slice(0, xlim), slice(0, zlim)


@functools.lru_cache(maxsize=None)
def excite_answers(deck, numerics, v):
    """amp, texc (as float words), P (damped once), PP after NT iterations of the forward loop with the maps, from (p0, pp0, amp0, texc_maps).
    The answer arrays carry the entry words outside the update extents."""
    i = inputs(deck, v)
    sx, sz, _ = DECKS[deck]["place"]
    xlim, zlim, _ = extents_of(i["d"])
    amp, texc, _, PP = maps_restatement(oracle(deck, numerics), i["v2"], sx, sz, i["srce"], xlim, zlim, i["p0"], i["pp0"], i["amp0"], i["texc_maps"])
    c = chain(deck, numerics, v, False)
    assert np.array_equal(PP.view(np.uint32), c["PP"].view(np.uint32)), "the chain of maps_restatement is the forward chain of the loop cases"
    assert texc.dtype == np.int32 and (texc > 0).all()
    return _freeze(dict(amp=amp, texc=texc.view(np.float32), itexc=texc, P=c["P"], PP=c["PP"]))


@functools.lru_cache(maxsize=None)
def pick_answers(deck, numerics, v, fields="p", texc_from=None):
    """exc, P (damped once, as fdw_dev_taper_finalize leaves it), PP after NT iterations of the line loop at depth gz with the pick (top = NT), from noise fields (fields "p":
    p0, pp0; "r": pr, ppr), exc0 and texc_pick -- or, texc_from = "excite", the map the excite case leaves."""
    i = inputs(deck, v)
    gz = DECKS[deck]["place"][2]
    texc = i["texc_pick"] if texc_from is None else excite_answers(deck, numerics, v)["itexc"]
    a, b = ("p0", "pp0") if fields == "p" else ("pr", "ppr")
    r = pick_restatement(oracle(deck, numerics), i["d"], i["v2"], i["w"], gz, texc, NT, i["exc0"], i[a], i[b])
    return _freeze(dict(exc=r["exc"], P=r["P"], PP=r["PP"], picked=r["picked"]))      # P as line_restatement gives it: damped once already


def image_answer(deck, exc, amp, img0, eps=EXC_EPS):
    """The entry image with image_formula applied to the interiors: every word outside the interior is the entry word."""
    inner = _interior(deck)
    out = np.array(img0, np.float32)
    out[inner] = image_formula(exc[inner], amp[inner], eps, out[inner])
    return out


@functools.lru_cache(maxsize=None)
def chain_answers(deck, numerics, v):
    e = excite_answers(deck, numerics, v)
    k = pick_answers(deck, numerics, v, fields="r", texc_from="excite")
    return _freeze(dict(amp=e["amp"], texc=e["texc"], exc=k["exc"], img=image_answer(deck, k["exc"], e["amp"], inputs(deck, v)["img0"], EXC_CHAIN_EPS)))


def _exc_case(kind, deck, numerics, two_step, split=((0, NT),), tuning=None, to=None):
    """kind = excite | pick: fdw_dev_excite_steps / fdw_dev_line_pick_steps over four rotating buffers, then fdw_dev_taper_finalize as
    _loop_case does; image: fdw_dev_image_excitation (twice, see there); chain: excite, pick on the excite call's texc (a second quartet of buffers), image of
    that exc and amp, on one stream with nothing in between.  Every map and image has a sentinel word in its padding columns."""
    nxe, nze, nxb, nzb, nx, nz = _dims(deck)
    sx, sz, gz = DECKS[deck]["place"]
    ext, inner = _update_extents(deck), _interior(deck)
    field_outs = lambda names: {n: ("field", (nxe, nze), s) for n, s in zip(names, (7.0, -7.0, 9.0, -7.0))}      # noqa: E731

    def loops(ctx, bufs, stream, fn):
        ip, ipp = 0, 1
        for k, (it0, n) in enumerate(split):
            ip, ipp = fn(bufs, it0, n, dict(first_pp_twice=k > 0, ip=ip, ipp=ipp, stream=stream))
        return ip, ipp

    if kind == "excite":
        ins = lambda i: dict(b0=("field", i["p0"]), b1=("field", i["pp0"]), v2=("field", i["v2"]), src=("flat", i["srce"]),      # noqa: E731
                             amp=("field", i["amp0"]), texc=("ifield", i["texc_maps"]))
        outs, scratch = field_outs(("b2", "b3")), ("b0", "b1", "b2", "b3")

        def call(ctx, p, stream):
            bufs = [p["b0"], p["b1"], p["b2"], p["b3"]]
            ip, ipp = loops(ctx, bufs, stream, lambda b, it0, n, a: ctx.dev_excite_steps(b, p["v2"], p["src"], sx, sz, p["amp"], p["texc"], it0, n, **a))
            ctx.dev_taper_finalize(bufs[ip], stream=stream)
            return [("PP", f"b{ipp}", None, None), ("P", f"b{ip}", None, None), ("amp", "amp", None, None), ("texc", "texc", None, None)]

        want = lambda v: {k: a for k, a in excite_answers(deck, numerics, v).items() if k != "itexc"}      # noqa: E731
        cells = dict(amp=ext, texc=ext)
    elif kind == "pick":      # texc is neither labelled nor scratch: rule (c) checks that the `const int *` comes back as uploaded
        ins = lambda i: dict(b0=("field", i["p0"]), b1=("field", i["pp0"]), v2=("field", i["v2"]), src=("flat", i["w"]),      # noqa: E731
                             texc=("ifield", i["texc_pick"]), exc=("field", i["exc0"]))
        outs, scratch = field_outs(("b2", "b3")), ("b0", "b1", "b2", "b3")

        def call(ctx, p, stream):
            bufs = [p["b0"], p["b1"], p["b2"], p["b3"]]
            ip, ipp = loops(ctx, bufs, stream, lambda b, it0, n, a: ctx.dev_line_pick_steps(b, p["v2"], p["src"], gz, p["texc"], NT, p["exc"], it0, n, **a))
            ctx.dev_taper_finalize(bufs[ip], stream=stream)
            return [("PP", f"b{ipp}", None, None), ("P", f"b{ip}", None, None), ("exc", "exc", None, None)]

        want = lambda v: {k: a for k, a in pick_answers(deck, numerics, v).items() if k != "picked"}      # noqa: E731
        cells = dict(exc=ext)
    elif kind == "image":      # EXC, AMP and AMPB are only read
        # Two calls in a row on the stream.  The first forms another image (IMGB) from a peak map four times as high (AMPB): the context
        # holds ONE peak word, cleared by a memset at the start of each call, and a memset issued on another stream runs EARLY (during the
        # delay) -- harmless for a single call, but before the first call's peak kernel here, so that the second call would meet a
        # stale peak four times too high and select fewer cells.
        big = lambda i: (np.float32(4.0) * i["amp_img"]).astype(np.float32)      # noqa: E731
        ins = lambda i: dict(EXC=("field", i["exc0"]), AMP=("field", i["amp_img"]), IMG=("field", i["img0"]), AMPB=("field", big(i)),      # noqa: E731
                             IMGB=("field", i["lap_in"]))
        outs, scratch = {}, ()

        def call(ctx, p, stream):
            ctx.dev_image_excitation(p["EXC"], p["AMPB"], EXC_EPS, p["IMGB"], stream=stream)
            ctx.dev_image_excitation(p["EXC"], p["AMP"], EXC_EPS, p["IMG"], stream=stream)
            return [("img", "IMG", None, None), ("img_first", "IMGB", None, None)]

        want = lambda v: dict(img=image_answer(deck, inputs(deck, v)["exc0"], inputs(deck, v)["amp_img"], inputs(deck, v)["img0"]),      # noqa: E731
                              img_first=image_answer(deck, inputs(deck, v)["exc0"], big(inputs(deck, v)), inputs(deck, v)["lap_in"]))
        cells = dict(img=inner, img_first=inner)
    else:
        assert kind == "chain"
        ins = lambda i: dict(a0=("field", i["p0"]), a1=("field", i["pp0"]), c0=("field", i["pr"]), c1=("field", i["ppr"]), v2=("field", i["v2"]),      # noqa: E731
                             src=("flat", i["srce"]), w=("flat", i["w"]), amp=("field", i["amp0"]), texc=("ifield", i["texc_maps"]),
                             exc=("field", i["exc0"]), IMG=("field", i["img0"]))
        outs, scratch = field_outs(("a2", "a3", "c2", "c3")), ("a0", "a1", "a2", "a3", "c0", "c1", "c2", "c3")

        def call(ctx, p, stream):
            ctx.dev_excite_steps([p[f"a{k}"] for k in range(4)], p["v2"], p["src"], sx, sz, p["amp"], p["texc"], 0, NT, stream=stream)
            ctx.dev_line_pick_steps([p[f"c{k}"] for k in range(4)], p["v2"], p["w"], gz, p["texc"], NT, p["exc"], 0, NT, stream=stream)
            ctx.dev_image_excitation(p["exc"], p["amp"], EXC_CHAIN_EPS, p["IMG"], stream=stream)
            return [("amp", "amp", None, None), ("texc", "texc", None, None), ("exc", "exc", None, None), ("img", "IMG", None, None)]

        want = lambda v: dict(chain_answers(deck, numerics, v))      # noqa: E731
        cells = dict(amp=ext, texc=ext, exc=ext, img=inner)
    name = dict(excite="excite", pick="pick", image="exc_image", chain="exc_chain")[kind]
    name += ("" if len(split) == 1 else "-chained") + ("-generic" if tuning else "")
    _add(name, deck, numerics, two_step, ins, outs, call, want, to=to, scratch=scratch, tuning=tuning, cells=cells,
         # the border ROWS of d_img must come back as uploaded
         written_rows=dict(IMG=inner[0], IMGB=inner[0]) if kind == "image" else dict(IMG=inner[0]) if kind == "chain" else None,
         pad_words=dict(PAD_WORDS))


def _exc_cases():
    fams = ((-1, "ragged"), (1, "ragged"), (4, "stepped"))
    for num in (0, 1):
        for kind in ("excite", "pick"):
            for fam, deck in fams:
                _exc_case(kind, deck, num, fam, to=EXC_CASES)
    for kind in ("excite", "pick"):
        for fam, deck in fams:      # 5 + 4 steps, the maps carried over, no host synchronisation in between
            _exc_case(kind, deck, 0, fam, split=((0, 5), (5, 4)), to=EXC_CASES)
    for kind in ("excite", "pick"):
        _exc_case(kind, "tiles", 0, 4, to=EXC_CASES)      # lean and full tiles
    for kind in ("excite", "pick"):      # the generic step followed by the compare-and-select / pick kernel
        _exc_case(kind, "ragged", 0, -1, tuning=dict(use_generic=True), to=EXC_CASES)
    _exc_case("image", "ragged", 0, None, to=EXC_CASES)
    _exc_case("chain", "ragged", 0, -1, to=EXC_CASES)
    _exc_case("chain", "stepped", 0, 4, to=EXC_CASES)
    for deck in EDGE_DECKS:
        for num in (0, 1):
            for kind in ("excite", "pick"):
                for fam in (-1, 1, 4):
                    _exc_case(kind, deck, num, fam, to=EXC_FOOTPRINT_CASES)
        for kind in ("excite", "pick"):
            _exc_case(kind, deck, 0, -1, tuning=dict(use_generic=True), to=EXC_FOOTPRINT_CASES)
        _exc_case("image", deck, 0, None, to=EXC_FOOTPRINT_CASES)
        _exc_case("chain", deck, 0, 4, to=EXC_FOOTPRINT_CASES)


_exc_cases()
_ALL = CASES + FOOTPRINT_CASES + EXC_CASES + EXC_FOOTPRINT_CASES
assert len({c.name for c in _ALL}) == len(_ALL)
EXC_BY_NAME = {c.name: c for c in EXC_CASES}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the late producer
# ---------------------------------------------------------------------------------------------------------------------------------------
class Delay:
    """A kernel that keeps a stream busy for a given time: torch.cuda._sleep(cycles), calibrated once with two events; where that does not
    hold a stream (it returned within a fifth of the time asked for), element-wise passes over a 256 MiB tensor calibrated the same way."""

    def __init__(self, torch):
        self.torch = torch
        self.scratch = None
        n = 20_000_000
        torch.cuda._sleep(1000)
        self.per_ms = n / self._time(lambda: torch.cuda._sleep(n))
        if not 0.2 * 25.0 < self._time(lambda: torch.cuda._sleep(int(25.0 * self.per_ms))) < 5 * 25.0:
            self.scratch = torch.zeros(64 << 20, device="cuda:0")
            self.scratch.add_(1.0)
            self.per_ms = 8 / self._time(lambda: [self.scratch.add_(1.0) for _ in range(8)])

    def _time(self, fn):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def __call__(self, ms):
        """Enqueue ms milliseconds of delay on the current stream."""
        k = max(1, int(ms * self.per_ms))
        if self.scratch is None:
            self.torch.cuda._sleep(k)
        else:
            for _ in range(k):
                self.scratch.add_(1.0)


WALLS = {}            # case name -> host milliseconds from the first enqueue on the stream to the return of the entry point


class Run:
    """One case behind a late producer.  Construction allocates and fills everything (decoys in the inputs, sentinels in the outputs, the true
    inputs in staging tensors), makes the call once on the context's own stream so that no code object is loaded and nothing is allocated
    inside the timed part, and puts the decoys and sentinels back; the caller then synchronises the device ONCE.  enqueue() issues delay,
    producer copies, entry point and output copies on one stream; finish() synchronises that stream and compares with the oracle."""

    def __init__(self, case, torch, ctx=None):
        self.case, self.torch = case, torch
        self.ctx = ctx or case.make_ctx()
        self.nze = DECKS[case.deck]["geom"][1]
        true, decoy = case.ins(inputs(case.deck, "true")), case.ins(inputs(case.deck, "decoy"))
        self.dev, self.stage = {}, {}
        for name, (kind, arr) in decoy.items():
            self.dev[name] = self._up(kind, arr, name)
            self.stage[name] = self._up(kind, true[name][1], name)
        self.kinds = {name: kind for name, (kind, _) in decoy.items()}
        for name, (kind, shape, val) in case.outs.items():
            self.dev[name] = self._up(kind, np.full(shape, val, np.float32))
            self.kinds[name] = kind
        self.first = {name: t.clone() for name, t in self.dev.items()}
        self.res = {name: torch.empty_like(t) for name, t in self.dev.items()}
        self.ptr = {name: t.data_ptr() for name, t in self.dev.items()}
        self.warm_labels = case.call(self.ctx, self.ptr, None)
        torch.cuda.synchronize()
        for name, t in self.dev.items():
            t.copy_(self.first[name])

    def _up(self, kind, arr, name=None):
        torch = self.torch
        if kind == "flat":
            return torch.from_numpy(np.array(arr, np.float32, order="C")).to("cuda:0")
        # a field: built on the host as words, so that an int32 map and a NaN pad word arrive bit for bit
        dt = np.int32 if kind == "ifield" else np.float32
        arr = np.ascontiguousarray(arr)
        assert kind == "field" or arr.dtype == np.int32, (name, arr.dtype)
        h = np.full((arr.shape[0], self.ctx.pitch), self.case.pad_words.get(name, 0), np.uint32)      # padding columns [nze, pitch): +0.0 or the case's word
        h[:, :arr.shape[1]] = np.asarray(arr, dt).view(np.uint32)
        return torch.from_numpy(h.view(dt)).to("cuda:0")

    def enqueue(self, S, delay, ms, entry=None, collect=True):
        """entry: the stream handed to the entry point (default S, the producer's own)."""
        torch = self.torch
        t0 = time.perf_counter()
        with torch.cuda.stream(S):
            delay(ms)
            for name, t in self.stage.items():
                self.dev[name].copy_(t, non_blocking=True)
            self.labels = self.case.call(self.ctx, self.ptr, (entry or S).cuda_stream)
            self.wall_ms = 1e3 * (time.perf_counter() - t0)
            self.busy = not S.query()
            if collect:
                self.collect(S)
        WALLS[self.case.name] = max(WALLS.get(self.case.name, 0.0), self.wall_ms)

    def collect(self, S):
        with self.torch.cuda.stream(S):
            for name, t in self.dev.items():
                self.res[name].copy_(t, non_blocking=True)

    def results(self):
        """{label: host array} of what the stream left, after the caller synchronised it."""
        out = {}
        for label, name, post, rows in self.labels:
            a = self.res[name].cpu().numpy()
            if self.kinds[name] in ("field", "ifield"):
                a = np.ascontiguousarray(a[:, :self.nze]).view(np.float32)
            if post is not None:
                a = post(a)
            out[label] = a if rows is None else a[rows]
        return out

    def close(self):
        self.ctx.close()

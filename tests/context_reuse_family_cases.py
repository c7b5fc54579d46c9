"""TEST HELPER (not a conftest) of tests/test_context_reuse_families.py: the call kinds of the families that came after
tests/context_reuse_cases.py was written -- line sources, excitation imaging, Born modelling, DTT imaging, extended images, least-squares
migration --, each with the two argument sets A and B of that module and the CPU restatement's answer to both.

The kinds live in a registry of their own (FAMILY_KINDS): context_reuse_cases.kinds_of(RTM) keeps its 19, and with them the seeded walks of
tests/test_context_reuse.py keep their sequences.  Everything A and B already differ in there (model, sx, (sz, gz), wavelet, gather, entry
image, entry illumination) is taken from rtm_inputs; family_inputs adds what the new entry points take on top: reflectivity, search
direction, mask, entry stack, start model, line gathers (one, and three of a batch), entry planes.

want(cfg, v) comes from the restatements the families' own modules pin their entry points to bit for bit (tests/test_line_source.py::
line_restatement, excitation_restatement, born_restatement, born_line_restatement, dtt_restatement, ext_restatement, lsm_restatement),
computed once (functools.lru_cache) and held finite and non-vacuous on the restatement's output alone.  The single-shot wants take the
model as an argument (`which`): "host", the argument set's own squared model, or "A" / "B", the border model drawn on that set's interior
model -- the second is what a call with v2=None runs on.

No family refuses the RAGGED geometry: check_born_args, check_line_args, check_exc_shot and check_lsm_shots ask for sz, gz < zlim and source
rows < xlim, check_ext_ctx for the dialect, a full grid and H; receiver rows 64 and 65, which are never stepped, are recorded as the static
rows they are (record_static) and the restatements say the same.  So every kind runs on RAGGED and on STEPPED.

Doubles (n2, the misfit history) travel through context_reuse_cases.check, which compares float32 arrays, as their four 16-bit words, each an
exact float32 (words()): the comparison stays one of every bit.  texc (int32) travels as the float32 words of the same bits."""
import functools

import numpy as np

import context_reuse_cases as K
import lsm_restatement as R
from born_line_restatement import born_line_restatement
from born_restatement import DTT, FIELD, born_restatement, embed_m
from context_reuse_cases import NT, RTM, Kind
from dtt_restatement import dtt_back_restatement
from excitation_restatement import image_formula, shot_restatement
from ext_restatement import ext_back_restatement
from test_line_source import line_restatement

f32 = np.float32
# fdw_shot_excitation's threshold.  Over 23 steps |amp| spans many decades around the source; at 1e-7 of its maximum the selection takes some
# hundreds of the cells that hold an amplitude and leaves thousands, and dozens of the selected cells hold a non-zero pick
EPS = 1e-7
NSOLVE, NITER = 2, 2                                          # lsm_solve: shots (two: the oracle side of three costs a third more), iterations


def deck(cfg):
    nxe, nze, nxb, nzb = cfg.geom
    return dict(nxe=nxe, nze=nze, nxb=nxb, nzb=nzb, compat=True)


def inner(cfg, a):
    nxe, nze, nxb, nzb = cfg.geom
    return np.ascontiguousarray(a[..., nxb:nxe - nxb, nzb:nze - nzb])


def embed(cfg, a):
    """Interior arrays [..][nx][nz] as fields [..][nxe][nze], zero outside."""
    a = np.asarray(a, f32)
    if a.ndim == 2:
        return embed_m(deck(cfg), a)
    return np.stack([embed_m(deck(cfg), p) for p in a])


def words(a):
    """float64 values as their four 16-bit words, each an exact float32."""
    return np.frombuffer(np.ascontiguousarray(a, np.float64).tobytes(), np.uint16).astype(f32)


def as_f32_bits(texc):
    return np.ascontiguousarray(texc, np.int32).view(f32)


@functools.lru_cache(maxsize=None)
def family_inputs(geom, v):
    nxe, nze, nxb, nzb = geom
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    a = v == "A"
    rng = np.random.default_rng(7000 + (3 if a else 11))
    rn = lambda *shape: rng.standard_normal(shape)      # noqa: E731
    out = dict(
        m=((0.3 if a else 0.2) * rn(nx, nz)).astype(f32), p=((0.3 if a else 0.4) * rn(nx, nz)).astype(f32),
        mask=rng.integers(0, 3, (nx, nz)).astype(f32) * f32(0.5), h0=rn(nx, nz).astype(f32), m0=(0.1 * rn(nx, nz)).astype(f32),
        wav=((100.0 if a else 70.0) * rn(nx, NT)).astype(f32), bwav=((100.0 if a else 70.0) * rn(3, nx, NT)).astype(f32),
        eimg3=rn(7, nx, nz).astype(f32), eimg1=rn(3, nx, nz).astype(f32))
    return K._freeze(out)


def _fi(cfg, v):
    return family_inputs(cfg.geom, v)


def model(cfg, v, which):
    """The squared model a single-shot call of argument set v runs on: its own ("host"), or the border model of set `which`'s draw."""
    return K._in(cfg, v)["v2"] if which == "host" else K.border_v2(cfg.geom, which, K.draw_index(which))


def draw(ctx, cfg, v):
    ctx.model_resident(K._in(cfg, v)["vp"])
    ctx.dev_extendvel_linear(K.draw_index(v) * ctx.border_draws())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the registry
# ---------------------------------------------------------------------------------------------------------------------------------------
FAMILY_KINDS = {}
RESIDENT_FORMS = {}      # family -> (want(cfg, v, which), run(ctx, cfg, v, v2)): the single-shot form the residency sequence runs with v2=None


def kind(name, family, run, **kw):
    def deco(want):
        k = FAMILY_KINDS[name] = Kind(name, RTM, want, run, **kw)
        k.family = family
        return want
    return deco


def single_shot(name, family, want, run, backward=False, resident=None):
    """The kind `name` on the argument set's own model and, with resident=<name>, the same call with v2=None after model_resident +
    dev_extendvel_linear, as shot_resident does it."""
    kind(name, family, lambda ctx, cfg, v: run(ctx, cfg, v, K._in(cfg, v)["v2"]), backward=backward)(lambda cfg, v: want(cfg, v, "host"))
    if resident:
        def run_resident(ctx, cfg, v):
            draw(ctx, cfg, v)
            return run(ctx, cfg, v, None)
        kind(resident, family, run_resident, backward=backward, model="set")(lambda cfg, v: want(cfg, v, v))


def family_kinds():
    return list(FAMILY_KINDS.values())


def all_kinds():
    """The 19 kinds of context_reuse_cases, then the new ones."""
    return K.kinds_of(RTM) + family_kinds()


def kind_of(name):
    return FAMILY_KINDS[name] if name in FAMILY_KINDS else K.KINDS[name]


def family_of(k):
    return getattr(k, "family", "rtm")


def _live(cfg):
    return K.live_traces(cfg)


# ---------------------------------------------------------------------------------------------------------------------------------------
# line sources
# ---------------------------------------------------------------------------------------------------------------------------------------
def _line_forward(cfg, v2, wav, sz, gz, il0=None):
    """line_restatement of one shot: P, PP, data[nx][nt], illum (a field)."""
    nxe, nze, nxb, nzb, nx, nz = K.dims(cfg)
    il = None if il0 is None else embed(cfg, il0)
    r = line_restatement(K.oracle_of(cfg), deck(cfg), v2, np.ascontiguousarray(wav.T), sz, gz=gz, il0=il)
    lo, hi = _live(cfg)
    assert np.count_nonzero(r["PP"]) > 1000 and all(r["data"][ix].any() for ix in range(lo, hi)) and not r["data"][hi:].any()
    return r


@functools.lru_cache(maxsize=None)
def _line_shot(cfg, v, which, residual, s=None):
    """shot_line / shot_line_residual of argument set v (s: shot s of its batch): image, illum, gather, resid, P, PP."""
    i, f = K._in(cfg, v), _fi(cfg, v)
    _, sz, gz = K.place(cfg, v)
    single = s is None
    v2 = model(cfg, v, which) if single else i["v2_all"][s]
    wav, d_obs, im0 = (f["wav"], i["d_obs"], i["im0"]) if single else (f["bwav"][s], i["bd_obs"][s], i["bim0"][s])
    r = _line_forward(cfg, v2, wav, sz, gz, il0=i["il0"] if single else None)
    out = dict(P=r["P"], PP=r["PP"], gather=r["data"], illum=inner(cfg, r["illum"]))
    data = d_obs
    if residual:
        data = out["resid"] = (d_obs - r["data"]).astype(f32)
    out["image"] = K.oracle_of(cfg).back(v2, r["P"], r["PP"], data, gz, imloc=im0)
    lo, hi = _live(cfg)
    assert np.count_nonzero(out["image"] != im0) > 2 * (hi - lo)
    if single:
        assert np.count_nonzero(out["illum"] > i["il0"]) > 2 * (hi - lo) and not (out["illum"] < i["il0"]).any()
    return K._freeze(out)


def _line_args(cfg, v):
    _, sz, gz = K.place(cfg, v)
    return sz, gz, _fi(cfg, v)["wav"], K._in(cfg, v)["d_obs"]


def _run_shot_line(ctx, cfg, v, v2):
    i = K._in(cfg, v)
    img, il = ctx.shot_line(v2, *_line_args(cfg, v), imloc=i["im0"], want_illum=True, illum=i["il0"])
    return dict(image=img, illum=il)


single_shot("shot_line", "line", lambda cfg, v, which: K._pick(_line_shot(cfg, v, which, False), "image", "illum"), _run_shot_line, backward=True)


def _run_record_line(ctx, cfg, v, v2):
    sz, gz, wav, _ = _line_args(cfg, v)
    data, P, PP = ctx.record_shot_line(v2, sz, gz, wav, want_fields=True)
    return dict(gather=data, P=P, PP=PP)


single_shot("record_shot_line", "line", lambda cfg, v, which: K._pick(_line_shot(cfg, v, which, False), "gather", "P", "PP"), _run_record_line)


def _run_line_residual(ctx, cfg, v, v2):
    return ctx.shot_line_residual(v2, *_line_args(cfg, v), imloc=K._in(cfg, v)["im0"], want_fields=True)


single_shot("shot_line_residual", "line", lambda cfg, v, which: K._pick(_line_shot(cfg, v, which, True), "image", "resid", "P", "PP"),
            _run_line_residual, backward=True)


def _line_batch_args(cfg, v, ns):
    _, sz, gz = K.place(cfg, v)
    return ns, sz, gz, _fi(cfg, v)["bwav"][:ns]


def _run_line_batch3(ctx, cfg, v):
    i = K._in(cfg, v)
    return dict(image=ctx.shot_line_batch(*_line_batch_args(cfg, v, 3), i["bd_obs"], v2_all=i["v2_all"], imloc=i["bim0"]))


@kind("shot_line_batch3", "line", _run_line_batch3, backward=True, model="batch_host")
def _(cfg, v):
    return K._stack([_line_shot(cfg, v, "host", False, s) for s in range(3)], "image")


def _run_record_line_batch2(ctx, cfg, v):
    return dict(gather=ctx.record_shot_line_batch(*_line_batch_args(cfg, v, 2), v2_all=K._in(cfg, v)["v2_all"][:2]))


@kind("record_shot_line_batch2", "line", _run_record_line_batch2, model="batch_host")
def _(cfg, v):
    return K._stack([_line_shot(cfg, v, "host", False, s) for s in range(2)], "gather")


# ---------------------------------------------------------------------------------------------------------------------------------------
# excitation-amplitude imaging
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exc_maps(cfg, v, which, s=None):
    """The interiors of exc, amp, texc and the fields P, PP of one excitation shot (s: shot s of argument set v's batch)."""
    i = K._in(cfg, v)
    sx, sz, gz = K.place(cfg, v)
    v2, d_obs = model(cfg, v, which), i["d_obs"]
    if s is not None:
        sx0, dsx = K.batch_rows(v)
        v2, sx, d_obs = i["v2_all"][s], sx0 + s * dsx, i["bd_obs"][s]
    exc, amp, texc, P, PP, iters = shot_restatement(K.oracle_of(cfg), deck(cfg), v2, sx, sz, gz, i["srce"], d_obs)
    out = dict(exc=inner(cfg, exc), amp=inner(cfg, amp), texc=as_f32_bits(inner(cfg, texc)), P=P, PP=PP)
    # the pick finds non-zero receiver values in many cells, in more than one iteration.  (Over 23 steps both wavelets are still rising, so the
    # excitation times are the last few steps and the picks, at iteration nt - texc, fall into the first few: tests/test_excitation.py's five
    # iterations belong to its 60 steps.)
    assert np.count_nonzero(out["exc"]) >= 100 and len(iters) >= 3, (np.count_nonzero(out["exc"]), sorted(iters))
    return K._freeze(out)


@functools.lru_cache(maxsize=None)
def _exc_shot(cfg, v, which):
    im0 = K._in(cfg, v)["im0"]
    out = dict(_exc_maps(cfg, v, which))
    out["image"] = image_formula(out["exc"], out["amp"], EPS, im0)
    assert (out["image"].view(np.uint32) != im0.view(np.uint32)).sum() >= 20
    return K._freeze(out)


def _run_excitation(ctx, cfg, v, v2):
    i = K._in(cfg, v)
    img, exc, amp, texc, P, PP = ctx.shot_excitation(v2, *K.place(cfg, v), i["srce"], i["d_obs"], EPS, i["im0"], want_fields=True)
    return dict(image=img, exc=exc, amp=amp, texc=as_f32_bits(texc), P=P, PP=PP)


single_shot("shot_excitation", "excitation", _exc_shot, _run_excitation, resident="shot_excitation_resident")
RESIDENT_FORMS["excitation"] = (_exc_shot, _run_excitation)


def _run_excitation_batch3(ctx, cfg, v):
    i, a = K._batch_call_args(cfg, v, 3)
    got = ctx.shot_excitation_batch(*a, i["bd_obs"], EPS, v2_all=i["v2_all"], imloc=i["im0"])
    got["texc"] = as_f32_bits(got["texc"])
    return got


# with host models it always ends the residency (fdw_shot_excitation_batch drops it before it knows whether its launches batch)
@kind("shot_excitation_batch3", "excitation", _run_excitation_batch3)
def _(cfg, v):
    shots = [_exc_maps(cfg, v, "host", s) for s in range(3)]
    out = K._stack(shots, "exc", "amp", "texc")
    img, stack = K._in(cfg, v)["im0"], []
    for s in shots:
        new = image_formula(s["exc"], s["amp"], EPS, img)
        assert (new.view(np.uint32) != np.asarray(img).view(np.uint32)).any(), "the shot does not move the running image"
        img = new
        stack.append(img)
    out.update(image=img, stack=np.stack(stack))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# Born modelling
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _born(cfg, v, which, scattering, line=False, s=None):
    """born_shot / born_shot_line with the background gather: scattered, gather (the background's), both [nx][nt]."""
    i, f = K._in(cfg, v), _fi(cfg, v)
    sx, sz, gz = K.place(cfg, v)
    v2 = model(cfg, v, which)
    if s is not None:
        sx0, dsx = K.batch_rows(v)
        v2, sx = i["v2_all"][s], sx0 + s * dsx
    m = embed(cfg, f["m"])
    if line:
        r = born_line_restatement(K.oracle_of(cfg), deck(cfg), v2, m, scattering, sz, gz, np.ascontiguousarray(f["wav"].T))
    else:
        r = born_restatement(K.oracle_of(cfg), deck(cfg), v2, m, scattering, sx, sz, gz, i["srce"])
    out = dict(scattered=np.ascontiguousarray(r["rec"].T), gather=np.ascontiguousarray(r["rec0"].T))
    lo, hi = _live(cfg)
    nx = K.dims(cfg)[4]
    for a in out.values():
        assert np.count_nonzero(a[lo:hi]) > nx and not a[hi:].any() and not a[:lo].any()
    return K._freeze(out)


def _run_born(scattering, line):
    def run(ctx, cfg, v, v2):
        i, f = K._in(cfg, v), _fi(cfg, v)
        sx, sz, gz = K.place(cfg, v)
        if line:
            data, data0 = ctx.born_shot_line(v2, f["m"], sz, gz, f["wav"], kind=scattering, want_background=True)
        else:
            data, data0 = ctx.born_shot(v2, f["m"], sx, sz, gz, i["srce"], kind=scattering, want_background=True)
        return dict(scattered=data, gather=data0)
    return run


# one per scattering kind of fdwave.h (enum { FDW_BORN_FIELD = 0, FDW_BORN_DTT = 1 })
single_shot("born_shot_field", "born", lambda cfg, v, which: _born(cfg, v, which, FIELD), _run_born(FIELD, False))
single_shot("born_shot", "born", lambda cfg, v, which: _born(cfg, v, which, DTT), _run_born(DTT, False), resident="born_shot_resident")
single_shot("born_shot_line", "born", lambda cfg, v, which: _born(cfg, v, which, DTT, line=True), _run_born(DTT, True))
RESIDENT_FORMS["born"] = (lambda cfg, v, which: _born(cfg, v, which, DTT), _run_born(DTT, False))


def _run_born_batch3(ctx, cfg, v):
    i, (ns, sx0, dsx, sz, gz, srce) = K._batch_call_args(cfg, v, 3)
    data, data0 = ctx.born_shot_batch(ns, _fi(cfg, v)["m"], sx0, dsx, sz, gz, srce, v2_all=i["v2_all"], want_background=True)
    return dict(scattered=data, gather=data0)


# with host models it always ends the residency (born_batch_impl)
@kind("born_shot_batch3", "born", _run_born_batch3)
def _(cfg, v):
    return K._stack([_born(cfg, v, "host", DTT, s=s) for s in range(3)], "scattered", "gather")


# ---------------------------------------------------------------------------------------------------------------------------------------
# DTT imaging
# ---------------------------------------------------------------------------------------------------------------------------------------
def _dtt_image(cfg, v2, P, PP, data, gz, im0):
    r = dtt_back_restatement(K.oracle_of(cfg), deck(cfg), v2, P, PP, np.ascontiguousarray(data.T[::-1]), gz, img0=embed(cfg, im0))
    img = inner(cfg, r["img"])
    lo, hi = _live(cfg)
    assert np.count_nonzero(img != im0) > 2 * (hi - lo), np.count_nonzero(img != im0)
    return img


@functools.lru_cache(maxsize=None)
def _dtt_shot(cfg, v, which, residual, s=None):
    i = K._in(cfg, v)
    sx, sz, gz = K.place(cfg, v)
    v2, d_obs, im0 = model(cfg, v, which), i["d_obs"], i["im0"]
    if s is not None:
        sx0, dsx = K.batch_rows(v)
        v2, sx, d_obs, im0 = i["v2_all"][s], sx0 + s * dsx, i["bd_obs"][s], i["bim0"][s]
    o = K._oracle_shot(cfg, v2, sx, sz, gz, i["srce"], d_obs, im0, il0=i["il0"] if residual else None, residual=residual)
    out = K._pick(o, "P", "PP", *(("resid", "illum") if residual else ()))
    out["image"] = _dtt_image(cfg, v2, o["P"], o["PP"], o["resid"] if residual else d_obs, gz, im0)
    assert (out["image"] != o["image"]).any()                    # (not the cross-correlation image of the same chain)
    return K._freeze(out)


def _run_shot_dtt(ctx, cfg, v, v2):
    i = K._in(cfg, v)
    return ctx.shot_dtt(v2, *K.place(cfg, v), i["srce"], i["d_obs"], imloc=i["im0"], want_fields=True)


def _want_shot_dtt(cfg, v, which):
    return K._pick(_dtt_shot(cfg, v, which, False), "image", "P", "PP")


single_shot("shot_dtt", "dtt", _want_shot_dtt, _run_shot_dtt, backward=True)
RESIDENT_FORMS["dtt"] = (_want_shot_dtt, _run_shot_dtt)


def _run_shot_dtt_residual(ctx, cfg, v, v2):
    i = K._in(cfg, v)
    return ctx.shot_dtt(v2, *K.place(cfg, v), i["srce"], i["d_obs"], imloc=i["im0"], residual=True, want_illum=True, illum=i["il0"])


single_shot("shot_dtt_residual_illum", "dtt", lambda cfg, v, which: K._pick(_dtt_shot(cfg, v, which, True), "image", "resid", "illum"),
            _run_shot_dtt_residual, backward=True)


@functools.lru_cache(maxsize=None)
def _line_dtt(cfg, v, which):
    i = K._in(cfg, v)
    sz, gz, wav, d_obs = _line_args(cfg, v)
    v2 = model(cfg, v, which)
    r = _line_forward(cfg, v2, wav, sz, gz)
    return K._freeze(dict(image=_dtt_image(cfg, v2, r["P"], r["PP"], d_obs, gz, i["im0"]), P=r["P"], PP=r["PP"]))


def _run_line_dtt(ctx, cfg, v, v2):
    return ctx.shot_line_dtt(v2, *_line_args(cfg, v), imloc=K._in(cfg, v)["im0"], want_fields=True)


single_shot("shot_line_dtt", "dtt", _line_dtt, _run_line_dtt, backward=True)


def _run_batch_dtt2(ctx, cfg, v):
    i, a = K._batch_call_args(cfg, v, 2)
    return ctx.shot_batch_dtt(*a, i["bd_obs"][:2], v2_all=i["v2_all"][:2], imloc=i["bim0"][:2])


@kind("shot_batch_dtt2", "dtt", _run_batch_dtt2, backward=True, model="batch_host")
def _(cfg, v):
    return K._stack([_dtt_shot(cfg, v, "host", False, s) for s in range(2)], "image")


# ---------------------------------------------------------------------------------------------------------------------------------------
# subsurface-offset extended images
# ---------------------------------------------------------------------------------------------------------------------------------------
def entry_planes(cfg, v, H):
    """Entry planes of noise for H = 3 and H = 1, drawn apart; H = 0 starts from zeros."""
    return _fi(cfg, v)[f"eimg{H}"] if H else None


@functools.lru_cache(maxsize=None)
def _ext_shot(cfg, v, which, H):
    i = K._in(cfg, v)
    sx, sz, gz = K.place(cfg, v)
    v2 = model(cfg, v, which)
    o = K._oracle_shot(cfg, v2, sx, sz, gz, i["srce"], i["d_obs"], i["im0"])
    entry = entry_planes(cfg, v, H)
    r = ext_back_restatement(K.oracle_of(cfg), deck(cfg), v2, o["P"], o["PP"], np.ascontiguousarray(i["d_obs"].T[::-1]), gz, H,
                             E0=None if entry is None else embed(cfg, entry))
    eimg = inner(cfg, r["E"])
    before = np.zeros_like(eimg) if entry is None else entry
    for j in range(2 * H + 1):                                   # every plane holds a signal of its own
        assert eimg[j].any() and np.count_nonzero(eimg[j] != before[j]) > 20, (H, j, np.count_nonzero(eimg[j] != before[j]))
    return K._freeze(dict(eimg=eimg, image=o["image"]))


def _ext_kind(H):
    def run(ctx, cfg, v, v2):
        i = K._in(cfg, v)
        return ctx.shot_ext(v2, *K.place(cfg, v), i["srce"], i["d_obs"], H, eimg=entry_planes(cfg, v, H), imloc=i["im0"])

    def want(cfg, v, which):
        return _ext_shot(cfg, v, which, H)
    single_shot(f"shot_ext{H}", "ext", want, run, backward=True)
    return want, run


_ext_kind(3)
RESIDENT_FORMS["ext"] = _ext_kind(1)
_ext_kind(0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# least-squares migration
# ---------------------------------------------------------------------------------------------------------------------------------------
def _gather_rows(a):
    """[..][nx][nt] -> the restatement's [..][nt][nx]."""
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


@functools.lru_cache(maxsize=None)
def _lsm_visit(cfg, v, which):
    i, f = K._in(cfg, v), _fi(cfg, v)
    r = R.visit(K.oracle_of(cfg), deck(cfg), model(cfg, v, which), embed(cfg, f["p"]), *K.place(cfg, v), i["srce"], _gather_rows(i["d_obs"]),
                embed(cfg, f["mask"]), embed(cfg, f["h0"]))
    h = inner(cfg, r["h"])
    assert np.count_nonzero(r["q"]) >= 20 and (h != f["h0"]).sum() >= 10 and r["n2"] > 0, "the visit reaches the stack"
    return K._freeze(dict(h=h, n2=words([r["n2"]]), data=_gather_rows(r["w"])))


def _run_lsm_visit(ctx, cfg, v, v2):
    i, f = K._in(cfg, v), _fi(cfg, v)
    got = ctx.lsm_visit(v2, f["p"], *K.place(cfg, v), i["srce"], d_obs=i["d_obs"], mask=f["mask"], h=f["h0"], want_data=True)
    got["n2"] = words([got["n2"]])
    return got


single_shot("lsm_visit", "lsm", _lsm_visit, _run_lsm_visit, backward=True)
RESIDENT_FORMS["lsm"] = (_lsm_visit, _run_lsm_visit)


def _run_lsm_visit_batch3(ctx, cfg, v):
    i, (ns, sx0, dsx, sz, gz, srce) = K._batch_call_args(cfg, v, 3)
    f = _fi(cfg, v)
    got = ctx.lsm_visit_batch(ns, f["p"], sx0, dsx, sz, gz, srce, d_obs=i["bd_obs"], mask=f["mask"], h=f["h0"], v2_all=i["v2_all"], want_data=True)
    got["n2"] = words(got["n2"])
    return got


# with host models both LSM batches always end the residency (lsm_plan)
@kind("lsm_visit_batch3", "lsm", _run_lsm_visit_batch3, backward=True)
def _(cfg, v):
    i, f = K._in(cfg, v), _fi(cfg, v)
    _, sz, gz = K.place(cfg, v)
    sx0, dsx = K.batch_rows(v)
    h, n2, w = embed(cfg, f["h0"]), [], []
    for s in range(3):
        r = R.visit(K.oracle_of(cfg), deck(cfg), i["v2_all"][s], embed(cfg, f["p"]), sx0 + s * dsx, sz, gz, i["srce"], _gather_rows(i["bd_obs"][s]),
                    embed(cfg, f["mask"]), h)
        assert (inner(cfg, r["h"]) != inner(cfg, h)).sum() >= 10 and r["n2"] > 0, s
        h = r["h"]
        n2.append(r["n2"])
        w.append(_gather_rows(r["w"]))
    return dict(h=inner(cfg, h), n2=words(n2), data=np.stack(w))


def _run_lsm_solve(ctx, cfg, v):
    i, (ns, sx0, dsx, sz, gz, srce) = K._batch_call_args(cfg, v, NSOLVE)
    f = _fi(cfg, v)
    got = ctx.lsm_solve(ns, sx0, dsx, sz, gz, srce, i["bd_obs"][:ns], NITER, m=f["m0"], mask=f["mask"], v2_all=i["v2_all"][:ns], verify=True, want_resid=True)
    got["misfit"] = words(got["misfit"])
    return got


@kind("lsm_solve", "lsm", _run_lsm_solve, backward=True)
def _(cfg, v):
    i, f = K._in(cfg, v), _fi(cfg, v)
    _, sz, gz = K.place(cfg, v)
    sx0, dsx = K.batch_rows(v)
    r = R.solve(K.oracle_of(cfg), deck(cfg), i["v2_all"][:NSOLVE], [sx0 + s * dsx for s in range(NSOLVE)], sz, gz, i["srce"],
                _gather_rows(i["bd_obs"][:NSOLVE]), NITER, m0=embed(cfg, f["m0"]), mask=embed(cfg, f["mask"]), verify=True)
    m = inner(cfg, r["m"])
    assert (m != f["m0"]).sum() >= 50 and r["misfit"][0] > 0 and all(a != 0 for a in r["alphas"] + r["betas"])
    assert r["misfit"].size == NITER + 2
    return dict(m=m, misfit=words(r["misfit"]), resid=_gather_rows(r["resid"]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the matrix rests on
# ---------------------------------------------------------------------------------------------------------------------------------------
TRACES = ("scattered", "resid", "data")                        # gathers [..][nx][nt] under other names than context_reuse_cases' "gather"


def assert_distinct(k, cfg):
    """context_reuse_cases.assert_distinct, and its rule for "gather" on the other gathers: A and B differ on every live trace that the
    signal of either reaches."""
    K.assert_distinct(k, cfg)
    a, b = k.want(cfg, "A"), k.want(cfg, "B")
    lo, hi = _live(cfg)
    for name in TRACES:
        if name not in a:
            continue
        xs, ys = a[name].reshape(-1, *a[name].shape[-2:]), b[name].reshape(-1, *b[name].shape[-2:])
        for s in range(xs.shape[0]):
            reached = [ix for ix in range(lo, hi) if xs[s, ix].any() or ys[s, ix].any()]
            assert len(reached) >= min(hi - lo, (cfg.order // 2) * xs.shape[-1]), (k.name, name, cfg, s, len(reached))
            same = [ix for ix in reached if np.array_equal(xs[s, ix], ys[s, ix])]
            assert not same, (k.name, name, cfg, f"shot {s}: traces {same} of A and B are equal")

"""Excitation-amplitude imaging (fdwave.h, "excitation-amplitude imaging"): fdw_dev_excite_steps, fdw_dev_line_pick_steps, fdw_shot_excitation,
fdw_image_excitation and rtm_code's exc=1 decks.

The restatements (tests/excitation_restatement.py) use existing oracle calls only.
  Maps: the chain of tests/test_illum.py::illum_restatement (Oracle.forward, one iteration per call, PP after the call is the level u) with
        `win = |u| > |amp|; amp[win] = u[win]; texc[win] = it + 1` inside the update extents.
  Pick: the chain of tests/test_line_source.py::line_restatement (swap, Oracle.slab_step, the line add) with
        `hit = texc == top - it; exc[hit] = PP[hit]` inside the update extents.
No arithmetic touches the maps, so every comparison is bit for bit (NaNs by position where the fields hold any)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from conftest import ROOT, assert_bit_equal, make_deck, random_fields
from excitation_restatement import image_formula, image_selection, maps_restatement, pick_restatement, shot_restatement  # noqa: F401  (the restatements; also imported from here)
from oracle import oracle as O
from test_line_source import args_of, extents_of, line_restatement
from test_record import interface_hits, two_layer_case
from test_stepn_isa_budget import isa  # noqa: F401  (a fixture)
from value_classes import FINITE, assert_same_nonfinite, deck_cuts, patched

BIN = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin")
EINVAL, ESTATE = -1, -5
LEAN, FULL = 0, 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatements' guards
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numerics", [0, 1])
def test_restatement_guards(numerics):
    nt = 11
    d = make_deck(87, 70, 12, 10, nt, seed=4)
    p0, pp0 = random_fields(d, 6, amp=0.1)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0 + np.float32(3.0)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    xlim, zlim, _ = extents_of(d)
    amp, texc, P, PP = maps_restatement(orc, d["v2"], d["sx"], d["sz"], srce, xlim, zlim, p0, pp0, maps=False)
    oP, oPP = orc.forward(d["v2"], d["sx"], d["sz"], srce, p0, pp0)
    assert_bit_equal(P, oP, "maps left out: P")
    assert_bit_equal(PP, oPP, "maps left out: PP")
    assert not amp.any() and not texc.any()
    # with the maps the fields are the same, and the maps say what they should
    amp, texc, P, PP = maps_restatement(orc, d["v2"], d["sx"], d["sz"], srce, xlim, zlim, p0, pp0)
    assert_bit_equal(PP, oPP, "maps: PP")
    assert texc[:xlim, :zlim].min() >= 1 and texc.max() == nt and not texc[xlim:].any() and not texc[:, zlim:].any()
    # a texc nothing matches: the pick chain is line_restatement
    rng = np.random.default_rng(1)
    w = rng.standard_normal((nt, 63)).astype(np.float32)
    exc0 = rng.standard_normal(orc.shape).astype(np.float32)
    got = pick_restatement(orc, d, d["v2"], w, d["sz"], np.full(orc.shape, -5, np.int32), nt, exc0, p0, pp0)
    want = line_restatement(orc, d, d["v2"], w, d["sz"], p0=p0, pp0=pp0)
    assert_bit_equal(got["PP"], want["PP"], "no match: PP")
    assert_bit_equal(got["P"], want["P"], "no match: P")
    assert_bit_equal(got["exc"], exc0, "no match: exc")


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: fdw_image_excitation against its formula, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
def _image_cases():
    rng = np.random.default_rng(12)
    n = 1000
    exc = rng.standard_normal(n).astype(np.float32)
    amp = (rng.standard_normal(n) * rng.random(n) ** 4).astype(np.float32)
    img = rng.standard_normal(n).astype(np.float32)
    img[::7] = -0.0
    yield "random", exc, amp, img, 1e-3
    yield "eps 0", exc, amp, img, 0.0
    yield "eps 0.5", exc, amp, img, 0.5
    yield "amp all zero", exc, np.zeros(n, np.float32), img, 1e-3
    yield "amp all zero, eps 0", exc, np.zeros(n, np.float32), img, 0.0
    a = amp.copy()
    a[3], a[10], a[11] = np.nan, np.inf, -np.inf
    e = exc.copy()
    e[5], e[6], e[10] = np.nan, np.inf, np.inf
    yield "nan and inf", e, a, img, 1e-3
    yield "nan and inf, eps 0", e, a, img, 0.0
    a = amp.copy()
    a[3] = np.nan
    e = exc.copy()
    e[5], e[6] = np.nan, -np.inf
    yield "nan in amp, finite max", e, a, img, 1e-2
    yield "subnormal amp", exc, (amp * np.float32(1e-40)).astype(np.float32), img, 1e-3


@pytest.mark.parametrize("case", list(_image_cases()), ids=lambda c: c[0])
def test_image_excitation_matches_formula(case):
    _, exc, amp, img, eps = case
    want = image_formula(exc, amp, eps, img)
    got = F.image_excitation(exc, amp, eps, img)
    assert_same_nonfinite(got, want, case[0])
    untouched = ~image_selection(amp, eps)
    assert_bit_equal(got[untouched], img[untouched], "cells that are not selected keep their word (-0.0 included)")
    if "all zero" in case[0]:
        assert_bit_equal(got, img, "amp all zero: img comes back word for word")


def test_image_excitation_refusals_and_empty():
    L = F.lib()
    x = np.ones(4, np.float32)
    img = np.full(4, -0.0, np.float32)
    for eps in (-1e-3, np.nan, np.inf, -np.inf):
        assert L.fdw_image_excitation(x.ctypes.data, x.ctypes.data, 4, eps, img.ctypes.data) == EINVAL
        with pytest.raises(F.FdwError):
            F.image_excitation(x, x, eps)
    assert_bit_equal(img, np.full(4, -0.0, np.float32), "a refused call writes nothing")
    assert L.fdw_image_excitation(None, x.ctypes.data, 4, 1e-3, img.ctypes.data) == EINVAL
    assert L.fdw_image_excitation(x.ctypes.data, None, 4, 1e-3, img.ctypes.data) == EINVAL
    assert L.fdw_image_excitation(x.ctypes.data, x.ctypes.data, 4, 1e-3, None) == EINVAL
    assert L.fdw_image_excitation(None, None, 0, 1e-3, None) == 0                  # nothing to do is not an error
    assert F.image_excitation(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).shape == (0, 3)
    got = F.image_excitation(np.full((2, 2), 3.0, np.float32), np.full((2, 2), 2.0, np.float32))
    assert_bit_equal(got, np.full((2, 2), 1.5, np.float32), "img=None starts from zeros")


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the built library
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_excitation_symbol_is_exported():
    L = F.lib()
    for name in ("fdw_dev_excite_steps", "fdw_dev_line_pick_steps", "fdw_shot_excitation", "fdw_image_excitation"):
        assert hasattr(L, name)
    for name in ("dev_excite_steps", "dev_line_pick_steps", "shot_excitation"):
        assert hasattr(F.FDWave, name)
    assert callable(F.image_excitation)


EXC_KERNELS = ("fdw_step_exc_kernel", "fdw_step_line_pick_kernel", "fdw_stepn_exc_kernel", "fdw_stepn_line_pick_kernel")


def test_excitation_kernels_exist_in_both_numerics_without_spills(isa):      # noqa: F811
    names = [k for k in isa if any(b in k for b in EXC_KERNELS + ("fdw_exc_select_kernel", "fdw_exc_pick_kernel"))]
    for base in EXC_KERNELS:
        for num in (0, 1):
            assert any(f"{base}I" in k and k.split("EEEv")[0].endswith(f"Li{num}") for k in names), (base, num, names)
    assert any("fdw_exc_select_kernelE" in k for k in names) and any("fdw_exc_pick_kernelE" in k for k in names), names
    for k in names:
        meta = isa[k][0]
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (k, meta)
    # one one-step variant per order the register-ring kernel serves (2, 4, 6, 8), EXACT and FAST; prefetch 1 and 3 for the exact order 8
    for base in ("fdw_step_exc_kernel", "fdw_step_line_pick_kernel"):
        for h in (1, 2, 3, 4):
            for num in (0, 1):
                assert any(f"{base}ILi{h}ELi2ELi{num}EEEv" in k for k in names), (base, h, num)
        for pf in (1, 3):
            assert any(f"{base}ILi4ELi{pf}ELi0EEEv" in k for k in names), (base, pf)
    # the pipeline kernels keep three workgroups per CU: 52 KiB of LDS each (3 x 52 = 156 of the CU's 160 KiB)
    lds = _lds_bytes()
    for k in names:
        if "fdw_stepn_" in k:
            assert lds[k] == 52 * 1024, (k, lds[k])


def _lds_bytes():
    """{kernel symbol: group_segment_fixed_size} from the metadata notes of the embedded code objects (the isa fixture keeps the register figures)."""
    import re
    import tempfile

    import test_stepn_isa_budget as B
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in B._code_objects(td):
            notes = subprocess.run([f"{B.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            for block in re.split(r"\n  - \.", notes)[1:]:
                name, size = re.search(r"\.name:\s+(\S+)", block), re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
                if name and size:
                    out[name.group(1)] = int(size.group(1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the physics on the oracle alone
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_oracle_excitation_images_the_two_layer_interface():
    """Three shots over the two-layer model, the reflections taken as record(two layers) - record(upper layer): the RAW stacked image has its
    strongest value within 2 cells of the interface in at least 0.9 of the central columns, and each shot picks more than 0.9 of the interior."""
    args, nx, nz, nb, iface, v2, h2, shots = two_layer_case()
    nt = args[5]
    sz = gz = nb + 2
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    orc = O.Oracle(*args, compat=True)
    d = dict(nxe=args[1], nze=args[2], nxb=nb, nzb=nb, compat=True)
    xlim, zlim, _ = extents_of(d)
    img = np.zeros((nx, nz), np.float32)
    for sx in shots:
        Pl = PPl = P = PP = None
        refl = np.zeros((nx, nt), np.float32)
        amp, texc = np.zeros(orc.shape, np.float32), np.zeros(orc.shape, np.int32)
        for it in range(nt):
            Pl, PPl = orc.forward(v2, sx, sz, srce[it:it + 1], Pl, PPl)          # the data: two layers
            P, PP = orc.forward(h2, sx, sz, srce[it:it + 1], P, PP)              # the migration model: the upper layer only
            refl[:, it] = PPl[nb:nb + nx, gz] - PP[nb:nb + nx, gz]
            u, a, t = PP[:xlim, :zlim], amp[:xlim, :zlim], texc[:xlim, :zlim]
            win = np.abs(u) > np.abs(a)
            a[win] = u[win]
            t[win] = it + 1
        r = pick_restatement(orc, d, h2, np.ascontiguousarray(refl[:, ::-1].T), gz, texc, nt, np.zeros(orc.shape, np.float32))
        share = r["picked"][nb:nb + nx, nb:nb + nz].mean()
        print(f"shot at {sx}: {share:.3f} of the interior cells picked")
        assert share > 0.9, (sx, share)
        img = image_formula(r["exc"][nb:nb + nx, nb:nb + nz], amp[nb:nb + nx, nb:nb + nz], 1e-3, img)
    hits = interface_hits(img, nz, nb, iface)
    print(f"oracle: raw excitation-amplitude image: interface hits {hits:.3f}")
    assert hits >= 0.9, hits


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: rtm_code's and the Python driver's refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def _write_min_deck(tmp_path, extra):
    np.full((20, 30), 2000.0, np.float32).tofile(tmp_path / "vp.bin")
    np.zeros(2 * 30 * 10, np.float32).tofile(tmp_path / "dobs.bin")
    (tmp_path / "out").mkdir(exist_ok=True)
    (tmp_path / "input.dat").write_text("tmpdir=./out\nvpfile=./vp.bin\ndatfile=./dobs.bin\nnz=20\nnx=30\nnt=10\ndz=10\ndx=10\ndt=0.001\nfpeak=25\n"
                                        "ns=2\nsz=1\nfsx=3\nds=5\ngz=2\nnxb=8\nnzb=8\nfac=0.75\norder=8\n" + extra)


def _run_rtm_code(tmp_path, env=None):
    base = {k: v for k, v in os.environ.items() if k not in ("FDW_SLABS", "FDW_GPUS")}
    base.update(env or {})
    return subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=base)


@pytest.mark.parametrize("extra,word", [("illum=1\n", "illum"), ("resid=1\n", "resid"), ("pw=1\n", "pw"), ("snap=5\n", "snap"), ("slabs=2\n", "slabs"),
                                        ("gpus=2\n", "gpus")])
def test_rtm_code_refuses_exc_key_combinations(tmp_path, extra, word):
    """Before any thread, communicator or device call: runs where no GPU is."""
    _write_min_deck(tmp_path, "exc=1\n" + extra)
    r = _run_rtm_code(tmp_path)
    assert r.returncode != 0 and "exc" in r.stderr and word in r.stderr, r.stderr
    assert os.listdir(tmp_path / "out") == []                     # refused before any output file was opened
    assert not os.path.exists(tmp_path / "image.num")


def test_rtm_code_refuses_exc_with_the_environments_slabs_and_gpus_and_a_bad_eps(tmp_path):
    _write_min_deck(tmp_path, "exc=1\n")
    for env, word in ((dict(FDW_SLABS="2"), "slabs"), (dict(FDW_GPUS="2"), "gpus")):
        r = _run_rtm_code(tmp_path, env)
        assert r.returncode != 0 and "exc" in r.stderr and word in r.stderr, r.stderr
    for bad in ("-0.5", "nan", "inf"):
        _write_min_deck(tmp_path, f"exc=1\nexc_eps={bad}\n")
        r = _run_rtm_code(tmp_path)
        assert r.returncode != 0 and "exc_eps" in r.stderr, r.stderr
    assert os.listdir(tmp_path / "out") == []


def test_python_driver_refuses_an_exc_deck(tmp_path):
    from parallel_finite_difference_computation_amd import rtm
    _write_min_deck(tmp_path, "exc=1\n")
    with pytest.raises(ValueError, match="exc"):
        rtm.read_deck(str(tmp_path / "input.dat"))
    (tmp_path / "input.dat").write_text((tmp_path / "input.dat").read_text().replace("exc=1", "exc=0"))
    assert rtm.read_deck(str(tmp_path / "input.dat"))["exc"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the device state of one run
# ---------------------------------------------------------------------------------------------------------------------------------------
class Device:
    """Entry state of one run on the device: four field buffers (p, pp, two spares holding sentinels), v2, the samples (wavelet or line gather
    [nt][nx]) and the three maps on [nxe][pitch], padding columns included, pre-filled with what the caller hands over."""

    def __init__(self, ctx, d, p0, pp0, samples, amp0=None, texc0=None, exc0=None):
        import torch
        self.torch, self.ctx, self.nze = torch, ctx, d["nze"]
        dev = torch.device("cuda:0")
        nxe, nze = d["nxe"], d["nze"]
        self.bufs = [torch.zeros((nxe, ctx.pitch), device=dev) for _ in range(4)]
        self.bufs[0][:, :nze] = torch.from_numpy(np.array(p0)).to(dev)
        self.bufs[1][:, :nze] = torch.from_numpy(np.array(pp0)).to(dev)
        self.bufs[2][:, :nze] = 7.0
        self.bufs[3][:, :nze] = -7.0
        self.v2 = torch.zeros((nxe, ctx.pitch), device=dev)
        self.v2[:, :nze] = torch.from_numpy(np.array(d["v2"])).to(dev)
        self.samples = torch.from_numpy(np.array(samples, np.float32, order="C")).to(dev)
        self.maps = {}
        for name, a, dt in (("amp", amp0, np.float32), ("texc", texc0, np.int32), ("exc", exc0, np.float32)):
            host = np.zeros((nxe, ctx.pitch), dt) if a is None else np.array(a, dt)
            assert host.shape == (nxe, ctx.pitch)
            self.maps[name] = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()

    def ptrs(self):
        return [b.data_ptr() for b in self.bufs]

    def excite(self, sx, sz, it0, nsteps, first=False, ip=0, ipp=1, stream=None):
        return self.ctx.dev_excite_steps(self.ptrs(), self.v2.data_ptr(), self.samples.data_ptr(), sx, sz, self.maps["amp"].data_ptr(),
                                         self.maps["texc"].data_ptr(), it0, nsteps, first_pp_twice=first, ip=ip, ipp=ipp, stream=stream)

    def pick(self, sz, top, it0, nsteps, first=False, ip=0, ipp=1, stream=None):
        return self.ctx.dev_line_pick_steps(self.ptrs(), self.v2.data_ptr(), self.samples.data_ptr(), sz, self.maps["texc"].data_ptr(), top,
                                            self.maps["exc"].data_ptr(), it0, nsteps, first_pp_twice=first, ip=ip, ipp=ipp, stream=stream)

    def field(self, i, finalize=False):
        if finalize:
            self.ctx.dev_taper_finalize(self.bufs[i].data_ptr())
        self.torch.cuda.synchronize()
        return self.bufs[i][:, :self.nze].cpu().numpy()

    def map(self, name):
        """The whole array [nxe][pitch], padding columns included."""
        self.torch.cuda.synchronize()
        return self.maps[name].cpu().numpy()


def entry_maps(shape_p, nze, seed, nt):
    """Entry amp (noise x 0.01), texc (non-zero, some inside [-1, nt + 2]) and exc (noise) on [nxe][pitch]; the padding columns hold sentinels."""
    rng = np.random.default_rng(seed)
    amp = (0.01 * rng.standard_normal(shape_p)).astype(np.float32)
    texc = rng.integers(-1, nt + 3, shape_p).astype(np.int32)
    texc[texc == 0] = -7
    exc = rng.standard_normal(shape_p).astype(np.float32)
    amp[:, nze:], texc[:, nze:], exc[:, nze:] = 123.5, 0x7FC12345, -321.25
    return amp, texc, exc


def embed(host_p, inner):
    """host_p [nxe][pitch] with its first nze columns replaced by `inner`."""
    out = np.array(host_p)
    out[:, :inner.shape[1]] = inner
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_dev_excite_steps against the chained oracle, every kernel family
# ---------------------------------------------------------------------------------------------------------------------------------------
NXE, NZE, NXB, NZB = 69, 301, 3, 10                      # compat: rows >= 64 never time-stepped; zlim = 296; ztap = 8
STEP_COUNTS = (1, 2, 3, 4, 5, 8, 9)                      # leftovers of the pair and of the pipeline
FAMILIES = [  # (order, tuning, source depths on either side of the family's strip border)
    (2, {}, (255, 256)), (4, {}, (255, 256)), (6, {}, (255, 256)), (10, {}, (255, 256)),
    (8, dict(two_step=-1), (255, 256)), (8, dict(use_generic=True, two_step=-1), (255, 256)),
    (8, dict(two_step=1), (239, 240)), (8, dict(two_step=4), (223, 224)),
    (8, dict(two_step=-1, prefetch=1), (255, 256)), (8, dict(two_step=-1, prefetch=3), (255, 256)),
]


def _deck(nt, order=8):
    return make_deck(NXE, NZE, NXB, NZB, nt, seed=3, order=order, dx=10.0, dz=12.5)


@functools.lru_cache(maxsize=None)
def excite_case(order, numerics, sz, nsteps):
    """The restatement's maps for one (order, numerics, depth, step count), shared by the tunings of one order; never modified."""
    nt = max(STEP_COUNTS)
    d = _deck(nt, order)
    p0, pp0 = random_fields(d, 5)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0 + np.float32(3.0)          # a sample that shows from the first iteration on
    xlim, zlim, _ = O.extents(NXE, NZE, NZB, True)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    pitch = -(-NZE // 64) * 64
    amp0, texc0, _ = entry_maps((NXE, 4 * pitch), NZE, 9, nt)                   # wide enough for any pitch; cropped by the caller
    amp, texc, _, oPP = maps_restatement(orc, d["v2"], 30, sz, srce[:nsteps], xlim, zlim, p0, pp0, amp0[:, :NZE], texc0[:, :NZE])
    for a in (amp, texc, oPP, amp0, texc0, p0, pp0, srce, d["v2"]):
        a.setflags(write=False)
    return d, p0, pp0, srce, amp0, texc0, amp, texc, oPP


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("order,tuning,depths", FAMILIES, ids=lambda v: str(v) if not isinstance(v, tuple) else None)
def test_dev_excite_steps_vs_chained_oracle(order, tuning, depths, numerics):
    """Noise-filled entry fields, a non-zero entry amp (noise x 0.01) and a non-zero entry texc: both maps equal the restatement inside the update
    extents and keep their entry words outside (sentinels in the padding columns); fields and indices are fdw_dev_steps2's."""
    import torch
    xlim, zlim = 64, 296
    ctx = F.FDWave(*args_of(_deck(max(STEP_COUNTS), order)), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    assert ctx.extents()[:2] == (xlim, zlim)
    if "two_step" in tuning:
        assert ctx.steps_per_pass() == {-1: 1, 1: 2, 4: 4}[tuning["two_step"]]
    for sz in depths:
        for nsteps in STEP_COUNTS:
            what = f"order {order} {tuning} numerics {numerics} sz {sz}, {nsteps} steps"
            d, p0, pp0, srce, amp0, texc0, amp, texc, oPP = excite_case(order, numerics, sz, nsteps)
            amp0p, texc0p = amp0[:, :ctx.pitch], np.array(texc0[:, :ctx.pitch])
            amp0p = np.array(amp0p)
            amp0p[:, NZE:], texc0p[:, NZE:] = 123.5, 0x7FC12345
            # what is compared is not empty: most cells inside the extents changed, at more than one level when there is more than one
            changed = texc[:xlim, :zlim] != texc0[:xlim, :zlim]
            assert changed.mean() > 0.9 and len(np.unique(texc[:xlim, :zlim][changed])) <= nsteps
            assert nsteps == 1 or len(np.unique(texc[:xlim, :zlim][changed])) > 1, what
            assert_bit_equal(amp[xlim:], amp0[xlim:, :NZE], "restatement outside the extents")
            assert_bit_equal(texc[:, zlim:].view(np.float32), texc0[:, zlim:NZE].view(np.float32), "restatement outside the extents")
            a = Device(ctx, d, p0, pp0, srce, amp0p, texc0p)
            ia = a.excite(30, sz, 0, nsteps)
            b = Device(ctx, d, p0, pp0, srce, amp0p, texc0p)
            ib = ctx.dev_steps2(b.ptrs(), b.v2.data_ptr(), b.samples.data_ptr(), 30, sz, 0, nsteps)
            torch.cuda.synchronize()
            assert_bit_equal(a.map("amp"), embed(amp0p, amp), "amp, " + what)
            assert_bit_equal(a.map("texc").view(np.float32), embed(texc0p, texc).view(np.float32), "texc, " + what)
            assert ia == ib, what
            for i in range(4):
                assert_bit_equal(a.field(i), b.field(i), f"buffer {i}, " + what)
            assert_bit_equal(a.field(ia[1]), oPP, "PP vs oracle, " + what)
            assert_bit_equal(b.map("amp"), amp0p, "dev_steps2 leaves the maps alone")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_dev_line_pick_steps against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
NT = 11
PICK_FAMILIES = [(o, t) for o, t, _ in FAMILIES]


@functools.lru_cache(maxsize=None)
def pick_case(order, numerics, grid=(87, 70, 12, 10)):
    """The small (and ragged) case of tests/test_line_source.py: deck, entry fields, line samples with 1e30 on rows >= nsrc, and the
    restatement's answers for a depth outside (13) and one inside (5) the damped strip; never modified."""
    d = make_deck(*grid, NT, seed=3, order=order, dx=10.0, dz=12.5)
    nx = d["nxe"] - 2 * d["nxb"]
    rng = np.random.default_rng(11)
    p0, pp0 = random_fields(d, 5, amp=0.1)
    w = rng.standard_normal((NT, nx)).astype(np.float32)
    xlim, zlim, _ = extents_of(d)
    w[:, max(0, xlim - d["nxb"]):] = 1e30                 # rows the loop never time-steps: their samples must have no effect
    _, texc0, exc0 = entry_maps((d["nxe"], 4 * 128), d["nze"], 17, NT)
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    want = {sz: pick_restatement(orc, d, d["v2"], w, sz, texc0[:, :d["nze"]], NT, exc0[:, :d["nze"]], p0, pp0) for sz in (13, 5)}
    for a in (p0, pp0, w, texc0, exc0, d["v2"]) + tuple(x for r in want.values() for x in r.values() if isinstance(x, np.ndarray)):
        a.setflags(write=False)
    return d, p0, pp0, w, texc0, exc0, want


def check_pick(ctx, case, sz, what, nsteps_split=None):
    d, p0, pp0, w, texc0, exc0, want = case
    xlim, zlim, _ = extents_of(d)
    nze = d["nze"]
    texc0p, exc0p = np.array(texc0[:, :ctx.pitch]), np.array(exc0[:, :ctx.pitch])
    texc0p[:, nze:], exc0p[:, nze:] = 0x7FC12345, -321.25
    r = want[sz]
    share = r["picked"][:xlim, :zlim].mean()
    assert share > 0.7, (what, share)                             # 11 of the 14 seeded values match some iteration
    assert not r["picked"][xlim:].any() and not r["picked"][:, zlim:].any()
    assert_bit_equal(r["exc"][~r["picked"]], exc0[:, :nze][~r["picked"]], "restatement: the unpicked words are the entry noise")
    dv = Device(ctx, d, p0, pp0, w, None, texc0p, exc0p)
    if nsteps_split is None:
        ip, ipp = dv.pick(sz, NT, 0, NT)
    else:
        ip, ipp = dv.pick(sz, NT, 0, nsteps_split)
        ip, ipp = dv.pick(sz, NT, nsteps_split, NT - nsteps_split, first=True, ip=ip, ipp=ipp)
    assert_bit_equal(dv.map("exc"), embed(exc0p, r["exc"]), "exc, " + what)
    assert_bit_equal(dv.map("texc").view(np.float32), texc0p.view(np.float32), "texc is only read, " + what)
    raw = [dv.field(i) for i in range(4)]                        # as the loop left them (P still owes one damping pass)
    assert_bit_equal(raw[ipp], r["PP"], "PP, " + what)
    assert_bit_equal(dv.field(ip, finalize=True), r["P"], "P, " + what)
    return raw, (ip, ipp)


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("order,tuning", PICK_FAMILIES, ids=str)
def test_dev_line_pick_steps_vs_restatement(order, tuning, numerics):
    """87 x 70, 11 iterations from noise fields, the line outside and inside the damped strip, texc seeded uniformly in [-1, nt + 2], top = nt,
    entry exc noise: exc, the fields and the indices against the restatement; the fields also against fdw_dev_line_steps."""
    case = pick_case(order, numerics)
    ctx = F.FDWave(*args_of(case[0]), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    for sz in (13, 5):
        what = f"order {order} {tuning} numerics {numerics} sz {sz}"
        raw, idx = check_pick(ctx, case, sz, what)
        ref = Device(ctx, case[0], case[1], case[2], case[3])
        assert idx == ctx.dev_line_steps(ref.ptrs(), ref.v2.data_ptr(), ref.samples.data_ptr(), sz, 0, NT), what
        for i in range(4):
            assert_bit_equal(raw[i], ref.field(i), f"buffer {i} vs fdw_dev_line_steps, " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("order,tuning", [(8, dict(two_step=-1)), (8, dict(two_step=1)), (8, dict(two_step=4)), (4, {}), (10, {}),
                                          (8, dict(use_generic=True, two_step=-1))], ids=str)
def test_ragged_grid_pick_ends_before_the_static_rows(order, tuning):
    """nxe = 87, nxb = 3: xlim = 80, nsrc = 77 of nx = 81.  The samples of rows >= nsrc (1e30) have no effect; rows >= xlim are never picked."""
    case = pick_case(order, 0, (87, 70, 3, 10))
    d, w = case[0], case[3]
    assert extents_of(d)[0] == 80 and (w[:, 77:] == 1e30).all() and w.shape[1] == 81
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(**tuning)
    check_pick(ctx, case, 13, f"ragged order {order} {tuning}")
    assert np.abs(case[6][13]["PP"]).max() < 1e3


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the pipeline deck of tests/test_tile_classes.py, lean and full tiles in one launch, both loops
# ---------------------------------------------------------------------------------------------------------------------------------------
XCHUNK = 13


@functools.lru_cache(maxsize=None)
def pipe_case(numerics):
    d = make_deck(180, 500, 12, 14, 8, seed=21, compat=False)
    nx = d["nxe"] - 2 * d["nxb"]
    rng = np.random.default_rng(7)
    p0, pp0 = random_fields(d, seed=5, amp=0.1)
    w = rng.standard_normal((8, nx)).astype(np.float32)
    srce = O.ricker_wavelet(8, 0.001, 30.0) * 1000.0 + np.float32(3.0)
    amp0, texc0, exc0 = entry_maps((180, 1024), 500, 23, 8)
    orc = O.Oracle(*args_of(d), compat=False, numerics=numerics)
    maps = {sz: maps_restatement(orc, d["v2"], 90, sz, srce, 180, 500, p0, pp0, amp0[:, :500], texc0[:, :500]) for sz in (16, 300)}
    picks = {sz: pick_restatement(orc, d, d["v2"], w, sz, texc0[:, :500], 8, exc0[:, :500], p0, pp0) for sz in (16, 300)}
    return d, p0, pp0, w, srce, amp0, texc0, exc0, maps, picks


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1], ids=["exact", "fast"])
def test_pipeline_deck_lean_and_full_tiles_both_loops(numerics):
    """180 x 500 at 13-row chunks: 14 chunk rows x 3 strips.  Source / line at depth 16 (strip 0): the lean tiles of strip 1 survive; at depth
    300 (strip 1): the tiles there run the full body.  8 steps (two pipeline passes) from noise fields."""
    d, p0, pp0, w, srce, amp0, texc0, exc0, maps, picks = pipe_case(numerics)
    ctx = F.FDWave(*args_of(d), compat=False, device=0, numerics=numerics)
    ctx.set_tuning(two_step=4, xchunk=XCHUNK)
    assert ctx.steps_per_pass() == 4
    amp0p, texc0p, exc0p = (np.array(a[:, :ctx.pitch]) for a in (amp0, texc0, exc0))
    amp0p[:, 500:], texc0p[:, 500:], exc0p[:, 500:] = 123.5, 0x7FC12345, -321.25
    for sz in (16, 300):
        nblk, nstrip, cls = ctx.debug_step4_plan_line(sz, xchunk=XCHUNK)
        cls = cls.reshape(-1, nstrip)
        assert cls.shape == (14, 3) and (cls[:, 0] == FULL).all() and (cls[:, 2] == FULL).all()
        if sz == 16:
            assert list(cls[:, 1]) == [FULL] * 4 + [LEAN] * 5 + [FULL] * 5, "the line in strip 0 leaves strip 1's lean tiles lean"
        else:
            assert (cls == FULL).all(), "the line crosses every tile of strip 1"
        what = f"pipeline deck numerics {numerics} sz {sz}"
        amp, texc, _, oPP = maps[sz]
        assert (texc != texc0[:, :500]).mean() > 0.9 and len(np.unique(texc[texc != texc0[:, :500]])) > 4
        a = Device(ctx, d, p0, pp0, srce, amp0p, texc0p)
        ia = a.excite(90, sz, 0, 8)
        b = Device(ctx, d, p0, pp0, srce)
        assert ia == ctx.dev_steps2(b.ptrs(), b.v2.data_ptr(), b.samples.data_ptr(), 90, sz, 0, 8)
        assert_bit_equal(a.map("amp"), embed(amp0p, amp), "amp, " + what)
        assert_bit_equal(a.map("texc").view(np.float32), embed(texc0p, texc).view(np.float32), "texc, " + what)
        for i in range(4):
            assert_bit_equal(a.field(i), b.field(i), f"buffer {i}, " + what)
        assert_bit_equal(a.field(ia[1]), oPP, "PP vs oracle, " + what)
        r = picks[sz]
        assert r["picked"].mean() > 0.6 and len(r["iters"]) == 8           # 8 of the 12 seeded values match some iteration
        dv = Device(ctx, d, p0, pp0, w, None, texc0p, exc0p)
        ip, ipp = dv.pick(sz, 8, 0, 8)
        assert_bit_equal(dv.map("exc"), embed(exc0p, r["exc"]), "exc, " + what)
        assert_bit_equal(dv.field(ipp), r["PP"], "PP of the pick loop, " + what)
        assert_bit_equal(dv.field(ip, finalize=True), r["P"], "P of the pick loop, " + what)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: continuing a loop; the refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("two_step", [-1, 1, 4])
def test_loops_continue_and_refuse(two_step):
    """it0 > 0 with first_pp_twice: 5 + 4 steps of the maps equal 9, 5 + 6 of the pick equal 11; every refusal of fdwave.h, none of which
    enqueues anything."""
    d, p0, pp0, srce, amp0, texc0, amp, texc, oPP = excite_case(8, 0, 223, 9)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(two_step=two_step)
    amp0p, texc0p = np.array(amp0[:, :ctx.pitch]), np.array(texc0[:, :ctx.pitch])
    two = Device(ctx, d, p0, pp0, srce, amp0p, texc0p)
    ip, ipp = two.excite(30, 223, 0, 5)
    ip, ipp = two.excite(30, 223, 5, 4, first=True, ip=ip, ipp=ipp)
    assert_bit_equal(two.map("amp"), embed(amp0p, amp), "amp after 5 + 4 steps")
    assert_bit_equal(two.map("texc").view(np.float32), embed(texc0p, texc).view(np.float32), "texc after 5 + 4 steps")
    assert_bit_equal(two.field(ipp), oPP, "PP after 5 + 4 steps")
    case = pick_case(8, 0)
    pctx = F.FDWave(*args_of(case[0]), compat=True, device=0)
    pctx.set_tuning(two_step=two_step)
    check_pick(pctx, case, 13, f"5 + 6 steps, two_step {two_step}", nsteps_split=5)
    if two_step != 4:
        return
    # ---- refusals (once, on the pipeline context: they happen before a family is chosen).  Not exercised: a context inside a batch
    # (FDW_ESTATE) -- nbatch is set only inside the batch calls themselves, no caller can reach a dev loop in that state ----
    dv = Device(ctx, d, p0, pp0, srce, amp0p, texc0p)
    ptrs, v2, s = dv.ptrs(), dv.v2.data_ptr(), dv.samples.data_ptr()
    am, tx = dv.maps["amp"].data_ptr(), dv.maps["texc"].data_ptr()
    zlim, xlim = 296, 64

    def code(fn, *a, **kw):
        with pytest.raises(F.FdwError) as e:
            fn(*a, **kw)
        return e.value.code
    L = F.lib()
    ex = ctx.dev_excite_steps
    assert code(ex, ptrs, v2, s, 30, 223, None, tx, 0, 4) == EINVAL
    assert code(ex, ptrs, v2, s, 30, 223, am, None, 0, 4) == EINVAL
    assert code(ex, ptrs, None, s, 30, 223, am, tx, 0, 4) == EINVAL
    assert code(ex, ptrs, v2, s, 30, 223, am, tx, -1, 4) == EINVAL
    assert code(ex, ptrs, v2, s, 30, zlim, am, tx, 0, 4) == EINVAL
    assert code(ex, ptrs, v2, s, 30, -1, am, tx, 0, 4) == EINVAL
    assert code(ex, ptrs, v2, s, xlim, 223, am, tx, 0, 4) == EINVAL                # a source row the loop never time-steps, as fdw_dev_steps2 refuses it
    assert code(ex, [ptrs[0], None, ptrs[2], ptrs[3]], v2, s, 30, 223, am, tx, 0, 4) == EINVAL          # a NULL buffer entry
    assert L.fdw_dev_excite_steps(ctx._h, None, v2, s, 30, 223, am, tx, 0, 4, 0, C.byref(C.c_int(0)), C.byref(C.c_int(1)), None) == EINVAL      # NULL d_buf
    pk = ctx.dev_line_pick_steps
    ex_p = dv.maps["exc"].data_ptr()
    assert code(pk, ptrs, v2, s, 13, None, 9, ex_p, 0, 4) == EINVAL
    assert code(pk, ptrs, v2, s, 13, tx, 9, None, 0, 4) == EINVAL
    assert code(pk, ptrs, v2, None, 13, tx, 9, ex_p, 0, 4) == EINVAL
    assert code(pk, ptrs, v2, s, 13, tx, 9, ex_p, -1, 4) == EINVAL
    assert code(pk, ptrs, v2, s, zlim, tx, 9, ex_p, 0, 4) == EINVAL
    assert code(pk, ptrs, v2, s, -1, tx, 9, ex_p, 0, 4) == EINVAL
    assert code(pk, [ptrs[0], ptrs[1], None, ptrs[3]], v2, s, 13, tx, 9, ex_p, 0, 4) == EINVAL
    assert L.fdw_dev_line_pick_steps(ctx._h, None, v2, s, 13, tx, 9, ex_p, 0, 4, 0, C.byref(C.c_int(0)), C.byref(C.c_int(1)), None) == EINVAL
    slab = F.FDWave(*args_of(d), compat=True, device=0, slab=(0, 40))
    mod = F.FDWave(*args_of(d), compat=True, device=0, dialect=1)
    stored = F.FDWave(*args_of(d), compat=True, device=0, dialect=2)
    for other in (slab, mod, stored):
        assert code(other.dev_excite_steps, ptrs, v2, s, 30, 223, am, tx, 0, 4) == ESTATE
        assert code(other.dev_line_pick_steps, ptrs, v2, s, 13, tx, 9, ex_p, 0, 4) == ESTATE
    nx, nz = NXE - 2 * NXB, NZE - 2 * NZB
    dobs = np.zeros((nx, d["nt"]), np.float32)
    sh = ctx.shot_excitation
    assert code(sh, d["v2"], 30, zlim, 20, srce, dobs) == EINVAL
    assert code(sh, d["v2"], -1, 223, 20, srce, dobs) == EINVAL                   # a shot from rest needs its source
    assert code(sh, d["v2"], xlim, 223, 20, srce, dobs) == EINVAL
    assert code(sh, d["v2"], 30, 223, zlim, srce, dobs) == EINVAL
    assert code(sh, d["v2"], 30, 223, 20, srce, dobs, eps=-1.0) == EINVAL
    assert code(sh, d["v2"], 30, 223, 20, srce, dobs, eps=float("nan")) == EINVAL
    assert code(sh, None, 30, 223, 20, srce, dobs) == ESTATE                      # no resident model
    assert L.fdw_shot_excitation(ctx._h, d["v2"].ctypes.data, 30, 223, 20, srce.ctypes.data, dobs.ctypes.data, 1e-3, None, None, None, None, None,
                                 None) == EINVAL                                    # all four outputs NULL
    for other in (slab, mod, stored):
        assert code(other.shot_excitation, d["v2"], 30, 223, 20, srce, dobs) == ESTATE
    dv.torch.cuda.synchronize()
    assert_bit_equal(dv.field(0), p0, "a refused call enqueues nothing")
    assert_bit_equal(dv.field(1), pp0, "a refused call enqueues nothing")
    assert_bit_equal(dv.map("amp"), amp0p, "a refused call enqueues nothing")
    assert_bit_equal(dv.map("texc").view(np.float32), texc0p.view(np.float32), "a refused call enqueues nothing")
    assert ctx.dev_excite_steps(ptrs, v2, s, 30, zlim - 1, am, tx, 0, 1) == (1, 0)      # the deepest column is accepted


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the value domain
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tuning", [dict(two_step=-1), dict(two_step=1), dict(two_step=4), dict(use_generic=True, two_step=-1)], ids=str)
def test_maps_and_pick_at_the_edges_of_the_value_domain(tuning):
    """Entry fields of subnormals, +-0, tiny and 2^60 patches with +-inf and NaN cells; entry amp with a NaN cell and an inf cell.  A NaN
    never wins, a NaN or inf in amp is never replaced, +-0 never wins, picked values keep their bits."""
    nt = 5
    d = _deck(nt)
    xc, zc = deck_cuts(d, np.random.default_rng(1), 3)
    p0 = patched((NXE, NZE), 31, FINITE, xc, zc)
    pp0 = patched((NXE, NZE), 32, FINITE, xc, zc)
    for f, cells in ((p0, ((20, 100, np.inf), (21, 230, np.nan), (40, 5, -np.inf))), (pp0, ((30, 150, np.nan), (31, 40, np.inf)))):
        for x, z, v in cells:
            f[x, z] = v
    p0[64:, :8] = 0
    pp0[64:, :8] = 0
    xlim, zlim = 64, 296
    srce = (O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0).astype(np.float32)
    orc = O.Oracle(*args_of(d), compat=True)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(**tuning)
    amp0p, texc0p, exc0p = entry_maps((NXE, ctx.pitch), NZE, 41, nt)
    amp0p[:, :NZE] = patched((NXE, NZE), 33, ("subnormal", "pzero", "nzero", "tiny"), xc, zc)      # entry peaks small enough to lose against normals
    amp0p[10, 10], amp0p[11, 11], amp0p[12, 200] = np.nan, np.inf, -np.inf
    amp, texc, _, oPP = maps_restatement(orc, d["v2"], 30, 223, srce, xlim, zlim, p0, pp0, amp0p[:, :NZE], texc0p[:, :NZE])
    # the restatement shows the rules at work
    assert np.isnan(oPP).any() and np.isinf(oPP).any()
    assert np.isnan(amp[10, 10]) and amp[11, 11] == np.inf and amp[12, 200] == -np.inf
    assert texc[10, 10] == texc0p[10, 10] and texc[11, 11] == texc0p[11, 11]
    assert np.isnan(amp[:xlim, :zlim]).sum() == 1, "a NaN never wins"
    kept = texc[:xlim, :zlim] == texc0p[:xlim, :zlim]
    assert kept.sum() > 3 and (np.isinf(amp[:xlim, :zlim]).sum() > 2)
    sub = (np.abs(amp[:xlim, :zlim]) < np.float32(2.0 ** -126)) & (amp[:xlim, :zlim] != 0) & ~kept
    assert sub.sum() > 20, "subnormal winners"
    a = Device(ctx, d, p0, pp0, srce, amp0p, texc0p)
    ia = a.excite(30, 223, 0, nt)
    assert_same_nonfinite(a.map("amp"), embed(amp0p, amp), f"amp {tuning}")
    assert_bit_equal(a.map("texc").view(np.float32), embed(texc0p, texc).view(np.float32), f"texc {tuning}")
    assert_same_nonfinite(a.field(ia[1]), oPP, f"PP {tuning}")
    # the pick on the same fields: values of every class keep their bits
    w = np.random.default_rng(3).standard_normal((nt, NXE - 2 * NXB)).astype(np.float32)
    w[:, 3], w[:, 10:20], w[2, 40] = -0.0, np.float32(1e-41), np.inf
    r = pick_restatement(orc, d, d["v2"], w, 20, texc0p[:, :NZE], nt, exc0p[:, :NZE], p0, pp0)
    got_cls = r["exc"][r["picked"]]
    assert np.isnan(got_cls).any() and np.isinf(got_cls).any() and ((np.abs(got_cls) < np.float32(2.0 ** -126)) & (got_cls != 0)).sum() > 20
    b = Device(ctx, d, p0, pp0, w, None, texc0p, exc0p)
    ip, ipp = b.pick(20, nt, 0, nt)
    assert_same_nonfinite(b.map("exc"), embed(exc0p, r["exc"]), f"exc {tuning}")
    assert_same_nonfinite(b.field(ipp), r["PP"], f"PP of the pick loop {tuning}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: whole shots
# ---------------------------------------------------------------------------------------------------------------------------------------
SHOT_GRIDS = {"69x301": (69, 301, 3, 10), "87x70": (87, 70, 12, 10)}


@functools.lru_cache(maxsize=None)
def shot_case(grid, order, numerics):
    nxe, nze, nxb, nzb = SHOT_GRIDS[grid]
    nt = 23
    # dx = dz = 10: on the dz = 12.5 deck of the loops above the order-4 shot at sx 40 on 69 x 301 picks 98 non-zero cells, short of the 100
    # the test asks of every case; here the restatement gives 107 .. 268 cells from 7 .. 12 iterations over all cases
    d = make_deck(nxe, nze, nxb, nzb, nt, seed=3, order=order)
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    srce = O.ricker_wavelet(nt, 0.001, 120.0) * 1000.0
    d_obs = np.random.default_rng(2).standard_normal((nx, nt)).astype(np.float32)
    sz, gz = nzb + 30, nzb + 26
    orc = O.Oracle(*args_of(d), compat=True, numerics=numerics)
    out = {}
    for sx in (30, 40):
        exc, amp, texc, P, PP, iters = shot_restatement(orc, d, d["v2"], sx, sz, gz, srce, d_obs)
        inner = (slice(nxb, nxb + nx), slice(nzb, nzb + nz))
        out[sx] = dict(exc=exc[inner], amp=amp[inner], texc=texc[inner], P=P, PP=PP, iters=iters)
    return d, nx, nz, srce, d_obs, sz, gz, out


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("order,tuning", [(8, dict(two_step=-1)), (8, dict(two_step=1)), (8, dict(two_step=4)), (4, {}), (10, {})], ids=str)
@pytest.mark.parametrize("grid", list(SHOT_GRIDS))
def test_shot_excitation_from_rest(grid, order, tuning, numerics):
    d, nx, nz, srce, d_obs, sz, gz, want = shot_case(grid, order, numerics)
    ctx = F.FDWave(*args_of(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    img = None
    stack = np.zeros((nx, nz), np.float32)
    for sx in (30, 40):
        w = want[sx]
        nonzero = (w["exc"] != 0).sum()
        print(f"{grid} order {order} numerics {numerics} sx {sx}: {nonzero} picked non-zero cells from {len(w['iters'])} iterations")
        assert nonzero >= 100 and len(w["iters"]) >= 5, (nonzero, w["iters"])
        img, exc, amp, texc, P, PP = ctx.shot_excitation(d["v2"], sx, sz, gz, srce, d_obs, 1e-3, img, want_fields=True)
        what = f"{grid} order {order} {tuning} numerics {numerics} sx {sx}"
        assert_bit_equal(amp, w["amp"], "amp, " + what)
        assert_bit_equal(texc.view(np.float32), w["texc"].view(np.float32), "texc, " + what)
        assert_bit_equal(exc, w["exc"], "exc, " + what)
        stack = image_formula(w["exc"], w["amp"], 1e-3, stack)
        assert_bit_equal(img, stack, "imloc (the second shot accumulates into the first), " + what)
        img0, P0, PP0 = ctx.shot(d["v2"], sx, sz, gz, srce, d_obs, want_fields=True)
        assert_bit_equal(P, P0, "P is fdw_shot's, " + what)
        assert_bit_equal(PP, PP0, "PP is fdw_shot's, " + what)
        assert_bit_equal(PP, w["PP"], "PP vs oracle, " + what)
    assert np.abs(stack).max() > 0


@pytest.mark.gpu
def test_shot_excitation_on_the_resident_model():
    nxe, nze, nxb, nzb, nt = 91, 77, 12, 10, 29
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    d = dict(nxe=nxe, nze=nze, nxb=nxb, nzb=nzb, compat=True)
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    rng = np.random.default_rng(3)
    vp = (1500 + 1000 * rng.random((nx, nz))).astype(np.float32)
    srce = O.ricker_wavelet(nt, 0.001, 120.0) * 100.0
    d_obs = rng.standard_normal((nx, nt)).astype(np.float32)
    sx, sz, gz = 45, nzb + 30, nzb + 26
    ctx.model_resident(vp)
    with pytest.raises(F.FdwError):
        ctx.shot_excitation(None, sx, sz, gz, srce, d_obs)            # no squared model drawn yet
    vel = ctx.dev_extendvel_linear(2 * ctx.border_draws(), want_vel=True)
    img, exc, amp, texc = ctx.shot_excitation(None, sx, sz, gz, srce, d_obs)
    orc = O.Oracle(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True)
    wexc, wamp, wtexc, _, _, iters = shot_restatement(orc, d, (vel * vel).astype(np.float32), sx, sz, gz, srce, d_obs)
    inner = (slice(nxb, nxb + nx), slice(nzb, nzb + nz))
    assert (wexc[inner] != 0).sum() >= 100 and len(iters) >= 5
    assert_bit_equal(amp, wamp[inner], "resident model: amp")
    assert_bit_equal(texc.view(np.float32), wtexc[inner].view(np.float32), "resident model: texc")
    assert_bit_equal(exc, wexc[inner], "resident model: exc")
    assert_bit_equal(img, image_formula(exc, amp, 1e-3, np.zeros((nx, nz), np.float32)), "resident model: image")
    assert ctx.shot_excitation(None, sx, sz, gz, srce, d_obs)[0].any()             # the model is still resident


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: state and streams
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("two_step", [-1, 4])
def test_one_context_through_shot_excitation_shot(two_step):
    d, nx, nz, srce, d_obs, sz, gz, want = shot_case("87x70", 8, 0)

    def fresh():
        c = F.FDWave(*args_of(d), compat=True, device=0)
        c.set_tuning(two_step=two_step)
        return c
    one = fresh()
    a1 = one.shot(d["v2"], 30, sz, gz, srce, d_obs)
    b = one.shot_excitation(d["v2"], 40, sz, gz, srce, d_obs)
    a2 = one.shot(d["v2"], 30, sz, gz, srce, d_obs)
    b2 = one.shot_excitation(d["v2"], 40, sz, gz, srce, d_obs)
    assert_bit_equal(a1, fresh().shot(d["v2"], 30, sz, gz, srce, d_obs), "shot before")
    assert_bit_equal(a2, a1, "shot after an excitation shot")
    for x, y, name in zip(b, fresh().shot_excitation(d["v2"], 40, sz, gz, srce, d_obs), ("img", "exc", "amp", "texc")):
        assert_bit_equal(x.view(np.float32), y.view(np.float32), name + " vs a fresh context")
    for x, y, name in zip(b2, b, ("img", "exc", "amp", "texc")):
        assert_bit_equal(x.view(np.float32), y.view(np.float32), name + " of the second excitation shot")
    assert_bit_equal(b[1], want[40]["exc"], "exc vs the restatement")


@pytest.mark.gpu
@pytest.mark.parametrize("two_step", [-1, 1, 4])
def test_both_loops_chained_on_one_callers_stream(two_step):
    """The maps' loop and then the pick loop (on the map the first has just written, a second set of fields) on one caller's stream without any
    host synchronisation in between equal the same two calls with a synchronisation after each."""
    import torch
    nt = 9
    d, p0, pp0, srce, amp0, texc0, _, _, _ = excite_case(8, 0, 223, nt)
    ctx = F.FDWave(*args_of(d), compat=True, device=0)
    ctx.set_tuning(two_step=two_step)
    w = np.random.default_rng(5).standard_normal((nt, NXE - 2 * NXB)).astype(np.float32)
    amp0p, texc0p = np.array(amp0[:, :ctx.pitch]), np.array(texc0[:, :ctx.pitch])

    def run(sync):
        a = Device(ctx, d, p0, pp0, srce, amp0p, texc0p)
        b = Device(ctx, d, pp0, p0, w)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        a.excite(30, 223, 0, nt, stream=st.cuda_stream)
        if sync:
            torch.cuda.synchronize()
        ip, ipp = ctx.dev_line_pick_steps(b.ptrs(), b.v2.data_ptr(), b.samples.data_ptr(), 20, a.maps["texc"].data_ptr(), nt, b.maps["exc"].data_ptr(),
                                          0, nt, stream=st.cuda_stream)
        st.synchronize()
        torch.cuda.synchronize()
        return a.map("amp"), a.map("texc"), b.map("exc"), b.field(ipp)
    x, y = run(False), run(True)
    for u, v, name in zip(x, y, ("amp", "texc", "exc", "PP of the pick loop")):
        assert_bit_equal(u.view(np.float32), v.view(np.float32), name + ": chained vs synchronised")
    assert np.count_nonzero(x[2]) > 1000


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the physics on the device
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_excitation_images_the_two_layer_interface():
    """Three shots over the two-layer model: the raw stacked image has interface_hits >= 0.9; amp, texc and exc of the middle shot equal the
    restatement (900 oracle steps of each loop) bit for bit."""
    args, nx, nz, nb, iface, v2, h2, shots = two_layer_case()
    nt = args[5]
    sz = gz = nb + 2
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    ctx = F.FDWave(*args, compat=True, device=0)
    img = None
    for sx in shots:
        refl = ctx.record_shot(v2, sx, sz, gz, srce) - ctx.record_shot(h2, sx, sz, gz, srce)
        img, exc, amp, texc = ctx.shot_excitation(h2, sx, sz, gz, srce, refl, 1e-3, img)
        picked = (texc >= 1).mean()
        print(f"shot at {sx}: {picked:.3f} of the interior cells have an excitation time")
        assert picked > 0.9
        if sx == shots[1]:
            keep = (exc, amp, texc, refl)
    hits = interface_hits(img, nz, nb, iface)
    print(f"MI355X: raw excitation-amplitude image: interface hits {hits:.3f}")
    assert hits >= 0.9, hits
    exc, amp, texc, refl = keep
    orc = O.Oracle(*args, compat=True)
    d = dict(nxe=args[1], nze=args[2], nxb=nb, nzb=nb, compat=True)
    wexc, wamp, wtexc, _, _, iters = shot_restatement(orc, d, h2, shots[1], sz, gz, srce, refl)
    inner = (slice(nb, nb + nx), slice(nb, nb + nz))
    assert len(iters) > 100
    assert_bit_equal(amp, wamp[inner], "two-layer shot: amp")
    assert_bit_equal(texc.view(np.float32), wtexc[inner].view(np.float32), "two-layer shot: texc")
    assert_bit_equal(exc, wexc[inner], "two-layer shot: exc")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: rtm_code's exc=1 deck
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rtm_code_exc_deck_equals_the_python_composition(tmp_path):
    """Three shots: dir.image is the stack, in shot order, of shot_excitation per shot on the border models the program draws."""
    nx, nz, nxb, nzb, nt, ns = 40, 50, 12, 10, 60, 3
    rng = np.random.default_rng(6)
    vp = (1800.0 + 600.0 * rng.random((nx, nz))).astype(np.float32)
    d_obs = rng.standard_normal((ns, nx, nt)).astype(np.float32)
    vp.tofile(tmp_path / "vp.bin")
    d_obs.tofile(tmp_path / "dobs.bin")
    (tmp_path / "out").mkdir()
    (tmp_path / "input.dat").write_text(f"tmpdir=./out\nvpfile=./vp.bin\ndatfile=./dobs.bin\nnz={nz}\nnx={nx}\nnt={nt}\ndz=10\ndx=10\ndt=0.001\nfpeak=25\n"
                                        f"ns={ns}\nsz=1\nfsx=5\nds=12\ngz=2\nnxb={nxb}\nnzb={nzb}\nfac=0.75\norder=8\nexc=1\nexc_eps=0.002\n")
    r = _run_rtm_code(tmp_path)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(tmp_path / "out" / "dir.image", np.float32).reshape(nx, nz)
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    ctx.model_resident(vp)
    srce = F.ricker_wavelet(nt, 0.001, 25.0)
    img = None
    for s in range(ns):
        ctx.dev_extendvel_linear(s * ctx.border_draws())
        img = ctx.shot_excitation(None, 5 + 12 * s + nxb, 1 + nzb, 2 + nzb, srce, d_obs[s], 0.002, img)[0]
    assert np.abs(img).max() > 0
    assert got.tobytes() == img.tobytes(), "dir.image vs the Python composition"

"""Source illumination of the RTM forward loop (fdw_dev_illum_steps, fdw_shot_illum, fdw_shot_resident_illum, rtm_code's illum=1) and the
compensated image (fdw_image_compensate).  Definition (fdwave.h): for every cell inside the update extents and every iteration in order,
I = I (+) u (*) u with u = what fd_forward's d_pp holds at the end of the iteration, product and sum rounded separately.  The CPU oracle
gives every u (its fd_forward chained one iteration per call, PP after the call, as tests/test_record.py::oracle_gather reads the gathers);
`il = il + u * u` in np.float32 is the whole restatement."""
import os
import subprocess

import numpy as np
import pytest

import parallel_finite_difference_computation_amd as F
from conftest import ROOT, assert_bit_equal, bits, make_deck, random_fields
from oracle import oracle as O
from test_record import interface_hits, two_layer_case
from test_stepn_isa_budget import isa  # noqa: F401  (a fixture)

BIN = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "bin")
MIN_SUBNORMAL_SHARE = 0.10          # the constant of tests/test_value_domain.py (importing that module would import the whole GPU parity suite)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------------------
def illum_restatement(orc, v2, sx, sz, srce, xlim, zlim, p0=None, pp0=None, il0=None):
    """(illumination, P, PP) after len(srce) iterations of the oracle's fd_forward chained one per call; the sum in np.float32, one rounded
    product and one rounded sum per cell and iteration, inside the update extents only."""
    P, PP = p0, pp0
    il = np.zeros(orc.shape, np.float32) if il0 is None else np.array(il0, np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for it in range(len(srce)):
            P, PP = orc.forward(v2, sx, sz, srce[it:it + 1], P, PP)
            u = PP[:xlim, :zlim]
            sq = (u * u).astype(np.float32)
            il[:xlim, :zlim] = (il[:xlim, :zlim] + sq).astype(np.float32)
    return il, P, PP


def compensate_formula(img, il, eps):
    """fdw_image_compensate spelled in np.float32 (fdwave.h)."""
    img, il = np.asarray(img, np.float32).ravel(), np.asarray(il, np.float32).ravel()
    m = np.float32(0.0)
    for v in il:
        if v > m:
            m = v
    with np.errstate(all="ignore"):
        s = np.float32(eps) * m
        d = (il + s).astype(np.float32)
        q = (img / np.where(d > 0, d, np.float32(1.0))).astype(np.float32)
    return np.where(d > 0, q, np.float32(0.0)).astype(np.float32)


def _compensate_raw(img, il, eps, out=None):
    """The C entry point on raw pointers (out=None: in place over img)."""
    out = img if out is None else out
    rc = F.lib().fdw_image_compensate(img.ctypes.data, il.ctypes.data, img.size, eps, out.ctypes.data)
    return rc, out


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: fdw_image_compensate against its formula, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
def _compensate_cases():
    rng = np.random.default_rng(17)
    n = 1500
    img = rng.standard_normal(n).astype(np.float32)
    pos = (rng.random(n) * 3.0 + 0.01).astype(np.float32)
    some_zero = pos.copy()
    some_zero[::7] = 0.0
    sub = (rng.integers(1, 1 << 23, n).astype(np.uint32)).view(np.float32).copy()           # subnormals only
    sub_mixed = sub.copy()
    sub_mixed[::3] = pos[::3] * np.float32(1e-37)
    negz = img.copy()
    negz[5] = -0.0
    negz[6] = 0.0
    nan_il = pos.copy()
    nan_il[11] = np.nan
    nan_il[0] = np.nan                                                                      # a NaN first: it must not become m either
    return {"random": (img, pos, 1e-3), "all-zero illumination": (img, np.zeros(n, np.float32), 1e-3),
            "eps 0, zero cells": (img, some_zero, 0.0), "eps 0, all zero": (img, np.zeros(n, np.float32), 0.0),
            "subnormal illumination": (img * np.float32(1e-30), sub, 1e-3), "subnormal and tiny normal": (img * np.float32(1e-30), sub_mixed, 0.25),
            "-0.0 image cell": (negz, pos, 1e-3), "NaN illumination cell": (img, nan_il, 1e-3), "large eps": (img, pos, 1e30)}


@pytest.mark.parametrize("case", list(_compensate_cases()))
def test_image_compensate_matches_formula(case):
    img, il, eps = _compensate_cases()[case]
    want = compensate_formula(img, il, eps)
    got = F.image_compensate(img, il, eps)
    assert_bit_equal(got, want, case)
    if case.startswith("all-zero") or case == "eps 0, all zero":
        assert not bits(got).any()                      # every output +0.0
    if case == "eps 0, zero cells":
        assert not bits(got[::7]).any() and np.isfinite(got).all()
    if case == "-0.0 image cell":
        assert bits(got)[5] == 0x80000000 and bits(got)[6] == 0
    if case == "NaN illumination cell":
        assert bits(got)[11] == 0 and bits(got)[0] == 0 and np.isfinite(got).all()      # NaN > 0 is false: the cell gives +0.0; m is finite
    if case.startswith("subnormal"):
        assert (got != 0).any()
    # in place over the image
    buf = img.copy()
    rc, out = _compensate_raw(buf, il.copy(), eps)
    assert rc == 0
    assert_bit_equal(out, want, case + ", in place")


def test_image_compensate_2d_and_refusals():
    rng = np.random.default_rng(3)
    img, il = rng.standard_normal((20, 30)).astype(np.float32), rng.random((20, 30)).astype(np.float32)
    got = F.image_compensate(img, il, 0.01)
    assert got.shape == (20, 30)
    assert_bit_equal(got.ravel(), compensate_formula(img, il, 0.01), "2-D")
    for eps in (-1e-3, float("nan"), float("inf"), -0.5):
        with pytest.raises(F.FdwError):
            F.image_compensate(img, il, eps)
    L, out = F.lib(), np.zeros_like(img)
    assert L.fdw_image_compensate(None, il.ctypes.data, il.size, 1e-3, out.ctypes.data) != 0
    assert L.fdw_image_compensate(img.ctypes.data, None, il.size, 1e-3, out.ctypes.data) != 0
    assert L.fdw_image_compensate(img.ctypes.data, il.ctypes.data, il.size, 1e-3, None) != 0
    assert L.fdw_image_compensate(img.ctypes.data, il.ctypes.data, 0, 1e-3, out.ctypes.data) == 0      # nothing to do is not an error
    assert not out.any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the physics: one shot over a two-layer model
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_compensated_image(img, il, nz, nb, iface, sx_int, sz_int, what):
    """img, il on the interior [nx][nz].  The illumination peaks on the source cell; compensation lowers the shallow energy relative to the
    reflector (a strict inequality, no fixed number); the strongest value below the first 15 cells sits on the interface."""
    comp = F.image_compensate(img, il, 1e-3)
    assert np.unravel_index(np.argmax(il), il.shape) == (sx_int, sz_int), (what, np.unravel_index(np.argmax(il), il.shape))
    ratio = {}
    for name, im in (("raw", img), ("compensated", comp)):
        shallow = float(np.abs(im[:, :15]).max())
        reflector = float(np.abs(im[40:120, iface - 2:iface + 3]).max())
        ratio[name] = shallow / reflector
        hits = interface_hits(im, nz, nb, iface)
        print(f"{what}: {name}: top 15 cells / reflector = {ratio[name]:.4f}, interface hits {hits:.3f}")
        assert hits >= 0.9, (what, name, hits)
    assert ratio["compensated"] < ratio["raw"], (what, ratio)


def test_oracle_illumination_compensates_the_two_layer_image():
    """CPU only (about 15 s on one core): the restatement's illumination and the library's host formula on the oracle's one-shot image."""
    args, nx, nz, nb, iface, v2, h2, shots = two_layer_case()
    nt, sx = args[5], shots[1]
    sz = gz = nb + 2
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    orc = O.Oracle(*args, compat=True)
    xlim, zlim, _ = O.extents(args[1], args[2], nb, True)
    il = np.zeros(orc.shape, np.float32)
    P = PP = Pl = PPl = None
    refl = np.zeros((nx, nt), np.float32)
    for it in range(nt):
        Pl, PPl = orc.forward(v2, sx, sz, srce[it:it + 1], Pl, PPl)          # the data: two layers
        P, PP = orc.forward(h2, sx, sz, srce[it:it + 1], P, PP)              # the migration model: the upper layer only
        refl[:, it] = PPl[nb:nb + nx, gz] - PP[nb:nb + nx, gz]
        u = PP[:xlim, :zlim]
        il[:xlim, :zlim] = il[:xlim, :zlim] + u * u
    img = orc.back(h2, P, PP, refl, gz)
    check_compensated_image(img, il[nb:nb + nx, nb:nb + nz], nz, nb, iface, sx - nb, sz - nb, "oracle")


@pytest.mark.gpu
def test_gpu_illumination_compensates_the_two_layer_image():
    args, nx, nz, nb, iface, v2, h2, shots = two_layer_case()
    nt, sx = args[5], shots[1]
    sz = gz = nb + 2
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    ctx = F.FDWave(*args, compat=True, device=0)
    refl = ctx.record_shot(v2, sx, sz, gz, srce) - ctx.record_shot(h2, sx, sz, gz, srce)
    img, il = ctx.shot(h2, sx, sz, gz, srce, refl, want_illum=True)
    assert_bit_equal(img, ctx.shot(h2, sx, sz, gz, srce, refl), "image with and without illumination")
    check_compensated_image(img, il, nz, nb, iface, sx - nb, sz - nb, "MI355X")


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the built library and the program's refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
ILLUM_KERNELS = ("fdw_step_illum_kernel", "fdw_step2_illum_kernel", "fdw_stepn_illum_kernel")


def test_illumination_kernels_exist_in_both_numerics_without_spills(isa):      # noqa: F811
    names = [k for k in isa if "_illum_" in k and "_kernel" in k]
    for base in ILLUM_KERNELS:
        for num in (0, 1):
            assert any(f"{base}I" in k and k.split("EEEv")[0].endswith(f"Li{num}") for k in names), (base, num, names)
    assert any("fdw_illum_add_kernelE" in k for k in names), names
    for k in names:
        meta = isa[k][0]
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (k, meta)
    # one one-step variant per order the register-ring kernel serves (2, 4, 6, 8), EXACT and FAST
    for h in (1, 2, 3, 4):
        for num in (0, 1):
            assert any(f"fdw_step_illum_kernelILi{h}ELi2ELi{num}EEEv" in k for k in names), (h, num)


def test_every_illumination_symbol_is_exported():
    L = F.lib()
    for name in ("fdw_dev_illum_steps", "fdw_shot_illum", "fdw_shot_resident_illum", "fdw_image_compensate"):
        assert hasattr(L, name)


def _write_min_deck(tmp_path, extra):
    np.full((20, 30), 2000.0, np.float32).tofile(tmp_path / "vp.bin")
    np.zeros(2 * 30 * 10, np.float32).tofile(tmp_path / "dobs.bin")
    (tmp_path / "out").mkdir()
    (tmp_path / "input.dat").write_text("tmpdir=./out\nvpfile=./vp.bin\ndatfile=./dobs.bin\nnz=20\nnx=30\nnt=10\ndz=10\ndx=10\ndt=0.001\nfpeak=25\n"
                                        "ns=2\nsz=1\nfsx=3\nds=5\ngz=2\nnxb=8\nnzb=8\nfac=0.75\norder=8\n" + extra)


def test_rtm_code_refuses_illum_with_slabs(tmp_path):
    """Before any thread, communicator or device call: runs where no GPU is."""
    _write_min_deck(tmp_path, "illum=1\nslabs=2\n")
    env = {k: v for k, v in os.environ.items() if k not in ("FDW_SLABS", "FDW_GPUS")}
    r = subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode != 0
    assert "illum" in r.stderr and "slabs" in r.stderr, r.stderr
    assert os.listdir(tmp_path / "out") == []                     # refused before any output file was opened
    assert not os.path.exists(tmp_path / "image.num")
    # the environment's FDW_SLABS counts like the key
    _write_min_deck_again = (tmp_path / "input.dat").read_text().replace("slabs=2\n", "")
    (tmp_path / "input.dat").write_text(_write_min_deck_again)
    r = subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=dict(env, FDW_SLABS="2"))
    assert r.returncode != 0 and "illum" in r.stderr and "slabs" in r.stderr, r.stderr
    # a bad illum_eps is refused as early
    (tmp_path / "input.dat").write_text(_write_min_deck_again + "illum_eps=-0.5\n")
    r = subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "illum_eps" in r.stderr, r.stderr


def test_python_driver_refuses_an_illum_deck(tmp_path):
    from parallel_finite_difference_computation_amd import rtm
    _write_min_deck(tmp_path, "illum=1\n")
    with pytest.raises(ValueError, match="illum"):
        rtm.read_deck(str(tmp_path / "input.dat"))
    (tmp_path / "input.dat").write_text((tmp_path / "input.dat").read_text().replace("illum=1", "illum=0"))
    assert rtm.read_deck(str(tmp_path / "input.dat"))["illum"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: fdw_dev_illum_steps against the chained oracle, every kernel family
# ---------------------------------------------------------------------------------------------------------------------------------------
# the geometry of tests/test_record.py: compat, nxe = 69 -> rows >= 64 never time-stepped; nze = 301 -> zlim = 296; nzb = 10 -> ztap = 8
NXE, NZE, NXB, NZB = 69, 301, 3, 10
STEP_COUNTS = (1, 2, 3, 4, 5, 8, 9)                    # leftovers of the pair and of the pipeline
FAMILIES = [  # (order, tuning, source depths on either side of the family's strip border)
    (2, {}, (255, 256)), (4, {}, (255, 256)), (6, {}, (255, 256)), (10, {}, (255, 256)),
    (8, dict(two_step=-1), (255, 256)), (8, dict(use_generic=True, two_step=-1), (255, 256)),
    (8, dict(two_step=1), (239, 240)), (8, dict(two_step=4), (223, 224)),
]


def _deck(nt, order=8):
    return make_deck(NXE, NZE, NXB, NZB, nt, seed=3, order=order, dx=10.0, dz=12.5)


def _args(d):
    return (d["order"], d["nxe"], d["nze"], d["nxb"], d["nzb"], d["nt"], d["fac"], d["dx"], d["dz"], d["dt"])


class _Device:
    """Entry state of one forward run on the device: four field buffers (p, pp, two spares holding junk), v2, wavelet, illumination."""

    def __init__(self, ctx, d, p0, pp0, il0, srce):
        import torch
        self.torch, self.ctx = torch, ctx
        dev = torch.device("cuda:0")
        nxe, nze = d["nxe"], d["nze"]
        self.nze = nze
        self.bufs = [torch.zeros((nxe, ctx.pitch), device=dev) for _ in range(4)]
        self.bufs[0][:, :nze] = torch.from_numpy(p0).to(dev)
        self.bufs[1][:, :nze] = torch.from_numpy(pp0).to(dev)
        self.bufs[2][:, :nze] = 7.0
        self.bufs[3][:, :nze] = -7.0
        self.v2 = torch.zeros((nxe, ctx.pitch), device=dev)
        self.v2[:, :nze] = torch.from_numpy(d["v2"]).to(dev)
        self.il = torch.zeros((nxe, ctx.pitch), device=dev)
        self.il[:, :nze] = torch.from_numpy(il0).to(dev)
        self.srce = torch.from_numpy(np.ascontiguousarray(srce, np.float32)).to(dev)
        torch.cuda.synchronize()

    def ptrs(self):
        return [b.data_ptr() for b in self.bufs]

    def field(self, i):
        return self.bufs[i][:, :self.nze].cpu().numpy()

    def illum(self):
        self.torch.cuda.synchronize()
        assert not self.il[:, self.nze:].any()              # padding columns stay zero
        return self.il[:, :self.nze].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("order,tuning,depths", FAMILIES)
def test_dev_illum_steps_vs_chained_oracle(order, tuning, depths, numerics):
    """Noise-filled entry fields (every cell contributes, the damped strip included) and a positive entry illumination: the whole extended
    grid equals the restatement inside the update extents and the entry values outside; fields and indices are fdw_dev_steps2's."""
    import torch
    nt = max(STEP_COUNTS)
    d = _deck(nt, order)
    p0, pp0 = random_fields(d, 5)
    il0 = (0.5 + np.random.default_rng(9).random((NXE, NZE))).astype(np.float32)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0 + np.float32(3.0)          # a sample that shows from the first iteration on
    xlim, zlim, _ = O.extents(NXE, NZE, NZB, True)
    assert (xlim, zlim) == (64, 296)
    orc = O.Oracle(*_args(d), compat=True, numerics=numerics)
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    assert ctx.extents()[:2] == (xlim, zlim)
    sx = 30
    for sz in depths:
        for nsteps in STEP_COUNTS:
            what = f"order {order} {tuning} numerics {numerics} sz {sz}, {nsteps} steps"
            want, _, oPP = illum_restatement(orc, d["v2"], sx, sz, srce[:nsteps], xlim, zlim, p0, pp0, il0)
            assert_bit_equal(want[xlim:], il0[xlim:], "restatement outside the extents")
            assert_bit_equal(want[:, zlim:], il0[:, zlim:], "restatement outside the extents")
            a = _Device(ctx, d, p0, pp0, il0, srce)
            ia = ctx.dev_illum_steps(a.ptrs(), a.v2.data_ptr(), a.srce.data_ptr(), sx, sz, a.il.data_ptr(), 0, nsteps)
            b = _Device(ctx, d, p0, pp0, il0, srce)
            ib = ctx.dev_steps2(b.ptrs(), b.v2.data_ptr(), b.srce.data_ptr(), sx, sz, 0, nsteps)
            torch.cuda.synchronize()
            assert_bit_equal(a.illum(), want, "illumination, " + what)
            assert ia == ib, what
            for i in range(4):
                assert_bit_equal(a.field(i), b.field(i), f"buffer {i}, " + what)
            assert_bit_equal(a.field(ia[1]), oPP, "PP vs oracle, " + what)
            assert_bit_equal(b.illum(), il0, "dev_steps2 leaves the illumination alone")


@pytest.mark.gpu
def test_dev_illum_steps_continues_a_loop_and_refuses():
    """it0 > 0 with first_pp_twice: two calls of 5 + 4 steps equal one of 9; NULL accumulator, slab context, the sibling's dialects: refused."""
    import torch
    nt = 9
    d = _deck(nt)
    p0, pp0 = random_fields(d, 5)
    il0 = np.zeros((NXE, NZE), np.float32)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0
    ctx = F.FDWave(*_args(d), compat=True, device=0)
    ctx.set_tuning(two_step=4)
    one = _Device(ctx, d, p0, pp0, il0, srce)
    ctx.dev_illum_steps(one.ptrs(), one.v2.data_ptr(), one.srce.data_ptr(), 30, 223, one.il.data_ptr(), 0, 9)
    two = _Device(ctx, d, p0, pp0, il0, srce)
    ip, ipp = ctx.dev_illum_steps(two.ptrs(), two.v2.data_ptr(), two.srce.data_ptr(), 30, 223, two.il.data_ptr(), 0, 5)
    ctx.dev_illum_steps(two.ptrs(), two.v2.data_ptr(), two.srce.data_ptr(), 30, 223, two.il.data_ptr(), 5, 4, True, ip, ipp)
    torch.cuda.synchronize()
    assert_bit_equal(two.illum(), one.illum(), "5 + 4 steps vs 9")
    assert one.illum().max() > 0
    with pytest.raises(F.FdwError) as e:
        ctx.dev_illum_steps(one.ptrs(), one.v2.data_ptr(), one.srce.data_ptr(), 30, 223, None, 0, 4)
    assert e.value.code == -1                                   # FDW_EINVAL
    slab = F.FDWave(*_args(d), compat=True, device=0, slab=(0, 40))
    mod = F.FDWave(*_args(d), compat=True, device=0, dialect=1)
    for other in (slab, mod):
        with pytest.raises(F.FdwError) as e:
            other.dev_illum_steps(one.ptrs(), one.v2.data_ptr(), one.srce.data_ptr(), 30, 223, one.il.data_ptr(), 0, 4)
        assert e.value.code == -5                               # FDW_ESTATE


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: whole shots
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("order,tuning", [(8, dict(two_step=-1)), (8, dict(two_step=1)), (8, dict(two_step=4)), (4, {}), (10, {})])
def test_shot_with_illumination_from_rest(order, tuning, numerics):
    nt = 23
    d = _deck(nt, order)
    nx, nz = NXE - 2 * NXB, NZE - 2 * NZB
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 1000.0
    d_obs = np.random.default_rng(2).standard_normal((nx, nt)).astype(np.float32)
    sx, sz, gz = 30, 223, 20
    xlim, zlim, _ = O.extents(NXE, NZE, NZB, True)
    orc = O.Oracle(*_args(d), compat=True, numerics=numerics)
    want, _, _ = illum_restatement(orc, d["v2"], sx, sz, srce, xlim, zlim)
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(**tuning)
    img, P, PP, il = ctx.shot(d["v2"], sx, sz, gz, srce, d_obs, want_fields=True, want_illum=True)
    assert_bit_equal(il, want[NXB:NXB + nx, NZB:NZB + nz], f"illumination order {order} {tuning}")
    assert il.max() > 0
    assert not il[xlim - NXB:].any()                              # rows never time-stepped
    img0, P0, PP0 = ctx.shot(d["v2"], sx, sz, gz, srce, d_obs, want_fields=True)
    for name, x, y in (("image", img, img0), ("P", P, P0), ("PP", PP, PP0)):
        assert_bit_equal(x, y, name + " with and without illumination")
    # accumulated into what the caller hands over
    img2, il2 = ctx.shot(d["v2"], sx, sz, gz, srce, d_obs, want_illum=True, illum=il)
    want2, _, _ = illum_restatement(orc, d["v2"], sx, sz, srce, xlim, zlim, il0=np.pad(il, ((NXB, NXB), (NZB, NZB))))
    assert_bit_equal(il2, want2[NXB:NXB + nx, NZB:NZB + nz], "second shot into the same illumination")
    assert_bit_equal(img2, img0, "image of the second shot")


@pytest.mark.gpu
def test_shot_resident_with_illumination():
    nxe, nze, nxb, nzb, nt = 91, 77, 12, 10, 29
    nx, nz = nxe - 2 * nxb, nze - 2 * nzb
    ctx = F.FDWave(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True, device=0)
    rng = np.random.default_rng(3)
    vp = (1500 + 1000 * rng.random((nx, nz))).astype(np.float32)
    srce = O.ricker_wavelet(nt, 0.001, 30.0) * 100.0
    d_obs = rng.standard_normal((nx, nt)).astype(np.float32)
    sx, sz, gz = 45, nzb + 2, nzb + 1
    ctx.model_resident(vp)
    with pytest.raises(F.FdwError):
        ctx.shot_resident(sx, sz, gz, srce, d_obs, want_illum=True)      # no squared model drawn yet
    vel = ctx.dev_extendvel_linear(2 * ctx.border_draws(), want_vel=True)
    img, P, PP, il = ctx.shot_resident(sx, sz, gz, srce, d_obs, want_fields=True, want_illum=True)
    img0, P0, PP0 = ctx.shot_resident(sx, sz, gz, srce, d_obs, want_fields=True)
    for name, x, y in (("image", img, img0), ("P", P, P0), ("PP", PP, PP0)):
        assert_bit_equal(x, y, name + " with and without illumination")
    xlim, zlim, _ = O.extents(nxe, nze, nzb, True)
    orc = O.Oracle(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True)
    want, _, _ = illum_restatement(orc, (vel * vel).astype(np.float32), sx, sz, srce, xlim, zlim)
    assert_bit_equal(il, want[nxb:nxb + nx, nzb:nzb + nz], "resident model")
    assert il.max() > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: full size
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("n", [4096, 8192])
def test_illumination_full_size_pipeline(n, numerics):
    """Noise-filled fields, 8 steps.  The automatic path (the wave pipeline: lean and full tiles) equals the same entry point called one step at
    a time (the one-step family) on the whole field; on a seeded sample of rows both equal the np.float32 sum over the levels fdw_dev_steps2
    delivers one step at a time, which involves no illumination kernel."""
    import torch
    dev = torch.device("cuda:0")
    nb, nsteps = 40, 8
    ctx = F.FDWave(8, n, n, nb, nb, nsteps, 0.75, 10.0, 10.0, 0.001, compat=True, device=0, numerics=numerics)
    assert ctx.steps_per_pass() == 4 and ctx.extents()[:2] == (n, n)
    g = torch.Generator(device=dev).manual_seed(n + numerics)
    pitch = ctx.pitch
    entry = [torch.zeros((n, pitch), device=dev) for _ in range(2)]
    for e in entry:
        e[:, :n] = torch.randn((n, n), device=dev, generator=g)
    v2 = torch.zeros((n, pitch), device=dev)
    v2[:, :n] = (1500.0 + 2000.0 * torch.rand((n, n), device=dev, generator=g)) ** 2
    il0 = torch.zeros((n, pitch), device=dev)
    il0[:, :n] = 0.5 + torch.rand((n, n), device=dev, generator=g)
    srce = (torch.from_numpy(O.ricker_wavelet(nsteps, 0.001, 30.0)) * 1000.0 + 5.0).to(dev)
    sx, sz = n // 2 + 3, 221

    def fresh():
        b = [entry[0].clone(), entry[1].clone(), torch.full((n, pitch), 7.0, device=dev), torch.full((n, pitch), -7.0, device=dev)]
        torch.cuda.synchronize()
        return b

    def ptrs(b):
        return [x.data_ptr() for x in b]

    # the automatic path
    a, ila = fresh(), il0.clone()
    torch.cuda.synchronize()          # the library runs on the context's own stream: torch's copies must have landed
    ia = ctx.dev_illum_steps(ptrs(a), v2.data_ptr(), srce.data_ptr(), sx, sz, ila.data_ptr(), 0, nsteps)
    torch.cuda.synchronize()
    c = fresh()
    ic = ctx.dev_steps2(ptrs(c), v2.data_ptr(), srce.data_ptr(), sx, sz, 0, nsteps)
    torch.cuda.synchronize()
    assert ia == ic
    for k in (ia[0], ia[1]):
        assert torch.equal(a[k].view(torch.int32), c[k].view(torch.int32)), "fields of dev_illum_steps and dev_steps2 differ"
    del c
    # one step at a time: the one-step illumination kernel, and the levels themselves through fdw_dev_steps2
    ctx.set_tuning(two_step=-1)
    assert ctx.steps_per_pass() == 1
    rows = np.sort(np.random.default_rng(n).choice(n, 48, replace=False))
    rows = np.unique(np.concatenate([rows, [0, 1, n - 1, sx, sx + 1, n // 2 - 100]]))
    rt = torch.from_numpy(rows).to(dev)
    b, ilb = fresh(), il0.clone()
    lv = fresh()
    torch.cuda.synchronize()
    ip, ipp, lp, lpp = 0, 1, 0, 1
    want = il0[rt][:, :n].cpu().numpy()
    for k in range(nsteps):
        ip, ipp = ctx.dev_illum_steps(ptrs(b), v2.data_ptr(), srce.data_ptr(), sx, sz, ilb.data_ptr(), k, 1, k > 0, ip, ipp)
        lp, lpp = ctx.dev_steps2(ptrs(lv), v2.data_ptr(), srce.data_ptr(), sx, sz, k, 1, k > 0, lp, lpp)
        torch.cuda.synchronize()
        u = lv[lpp][rt][:, :n].cpu().numpy()
        want = (want + (u * u).astype(np.float32)).astype(np.float32)
    assert torch.equal(ila.view(torch.int32), ilb.view(torch.int32)), f"{n}^2: the pipeline's illumination differs from the one-step kernel's"
    assert torch.equal(a[ia[1]].view(torch.int32), b[ipp].view(torch.int32))
    assert_bit_equal(ila[rt][:, :n].cpu().numpy(), want, f"{n}^2: sampled rows against the levels of dev_steps2")
    assert not ila[:, n:].any()
    assert bool((ila[:, :n] > il0[:, :n]).any())


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: squares at the edges of the fp32 range
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("numerics", [0, 1])
@pytest.mark.parametrize("two_step", [4, -1])
@pytest.mark.parametrize("k", [-66, 60])
def test_illumination_of_scaled_fields(k, two_step, numerics):
    """The 69 x 301 deck, noise-filled entry fields times 2^k, a silent source, 8 steps from a zero illumination.  2^-66: the squares land in
    the subnormal range (they must neither be flushed nor vanish); 2^60: part of them overflow to +inf (compared bitwise)."""
    import torch
    nsteps = 8
    d = _deck(nsteps)
    p0, pp0 = random_fields(d, 5)
    scale = np.float32(2.0) ** np.float32(k)
    p0, pp0 = (p0 * scale).astype(np.float32), (pp0 * scale).astype(np.float32)
    il0 = np.zeros((NXE, NZE), np.float32)
    srce = np.zeros(nsteps, np.float32)
    xlim, zlim, _ = O.extents(NXE, NZE, NZB, True)
    orc = O.Oracle(*_args(d), compat=True, numerics=numerics)
    want, _, _ = illum_restatement(orc, d["v2"], d["sx"], d["sz"], srce, xlim, zlim, p0, pp0, il0)
    inside = want[:xlim, :zlim]
    if k < 0:      # vacuity: the restatement's own output holds what the case is about
        sub = float(np.mean((np.abs(inside) < np.float32(2.0 ** -126)) & (inside != 0)))
        print(f"2^{k}: subnormal share {sub:.3f}, zeros {int((inside == 0).sum())}")
        assert sub >= MIN_SUBNORMAL_SHARE and not (inside == 0).any()
    else:
        inf = float(np.mean(np.isposinf(inside)))
        print(f"2^{k}: +inf share {inf:.3f}, NaNs {int(np.isnan(inside).sum())}")
        assert 0.01 <= inf <= 0.50 and not np.isnan(inside).any()
    ctx = F.FDWave(*_args(d), compat=True, device=0, numerics=numerics)
    ctx.set_tuning(two_step=two_step)
    a = _Device(ctx, d, p0, pp0, il0, srce)
    ctx.dev_illum_steps(a.ptrs(), a.v2.data_ptr(), a.srce.data_ptr(), d["sx"], d["sz"], a.il.data_ptr(), 0, nsteps)
    torch.cuda.synchronize()
    assert_bit_equal(a.illum(), want, f"2^{k}, two_step {two_step}, numerics {numerics}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the program
# ---------------------------------------------------------------------------------------------------------------------------------------
def _six_shot_deck(tmp_path, extra=""):
    nx, nz, nxb, nzb, nt, ns, ds = 50, 37, 10, 9, 47, 6, 7
    rng = np.random.default_rng(11)
    vp = (1500 + 2500 * np.linspace(0, 1, nz, dtype=np.float32)[None, :] + 100 * rng.standard_normal((nx, nz))).astype(np.float32)
    (tmp_path / "models").mkdir()
    (tmp_path / "output").mkdir()
    vp.tofile(tmp_path / "models" / "vp.bin")
    dobs = rng.standard_normal((ns, nx, nt)).astype(np.float32)
    dobs.tofile(tmp_path / "models" / "dobs.bin")
    (tmp_path / "input.dat").write_text("tmpdir=./output\nvpfile=./models/vp.bin\ndatfile=./models/dobs.bin\n"
                                        f"nz={nz}\nnx={nx}\nnt={nt}\ndz=10\ndx=10\ndt=0.001\nfpeak=25.\nns={ns}\nsz=1\nfsx=5\nds={ds}\ngz=2\n"
                                        f"nxb={nxb}\nnzb={nzb}\nrnd=1\nfac=0.75\norder=8\n" + extra)
    return nx, nz, nxb, nzb, nt, ns, ds, vp


def _run_rtm_code(tmp_path, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("FDW_SHOT_WORKERS", "FDW_SLABS", "FDW_GPUS")}
    env.update(env_extra or {})
    r = subprocess.run([os.path.join(BIN, "rtm_code"), "./input.dat"], cwd=tmp_path, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    out = tmp_path / "output"
    return {name: (out / name).read_bytes() for name in sorted(os.listdir(out))}, (tmp_path / "image.num").read_bytes()


@pytest.mark.gpu
def test_rtm_code_illum_key(tmp_path):
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    (tmp_path / "on1").mkdir()
    _six_shot_deck(tmp_path / "off", "illum=0\n")
    nx, nz, nxb, nzb, nt, ns, ds, vp = _six_shot_deck(tmp_path / "on", "illum=1\n")
    _six_shot_deck(tmp_path / "on1", "illum=1\nillum_eps=0.05\n")
    off, num_off = _run_rtm_code(tmp_path / "off")
    on, num_on = _run_rtm_code(tmp_path / "on")                                       # the default four workers
    on1, num_on1 = _run_rtm_code(tmp_path / "on1", {"FDW_SHOT_WORKERS": "1"})
    assert sorted(off) == ["dir.image", "dir.image_lap", "dir.snapr", "dir.snaps", "dir.snaps_rec"]
    assert sorted(on) == sorted(on1) == sorted(list(off) + ["dir.illum", "dir.image_illum"])
    for name in off:
        assert on[name] == off[name] and on1[name] == off[name], name         # untouched by the key, whatever the number of workers
    assert num_on == num_off and num_on1 == num_off
    assert on1["dir.illum"] == on["dir.illum"]                                    # one worker and four: the same bytes
    # the stack of the per-shot restatements, in shot order
    nxe, nze = nx + 2 * nxb, nz + 2 * nzb
    srce = O.ricker_wavelet(nt, 0.001, 25.0)
    orc = O.Oracle(8, nxe, nze, nxb, nzb, nt, 0.75, 10.0, 10.0, 0.001, compat=True)
    xlim, zlim, _ = O.extents(nxe, nze, nzb, True)
    vpe = np.zeros((nxe, nze), np.float32)
    vpe[nxb:nxb + nx, nzb:nzb + nz] = vp
    ill = np.zeros((nx, nz), np.float32)
    for s in range(ns):
        O.extendvel_linear(vpe, nx, nz, nxb, nzb, seed=1 if s == 0 else None)      # the reference never seeds rand()
        il, _, _ = illum_restatement(orc, (vpe * vpe).astype(np.float32), 5 + s * ds + nxb, 1 + nzb, srce, xlim, zlim)
        ill = ill + il[nxb:nxb + nx, nzb:nzb + nz]
    got = np.frombuffer(on["dir.illum"], np.float32).reshape(nx, nz)
    assert_bit_equal(got, ill, "dir.illum")
    assert got.max() > 0
    img = np.frombuffer(on["dir.image"], np.float32)
    assert_bit_equal(np.frombuffer(on["dir.image_illum"], np.float32), compensate_formula(img, got, 1e-3), "dir.image_illum, default illum_eps")
    assert_bit_equal(np.frombuffer(on1["dir.image_illum"], np.float32), compensate_formula(img, got, 0.05), "dir.image_illum, illum_eps=0.05")
    # the same three files, byte for byte, from one worker with the default eps
    (tmp_path / "on" / "output" / "dir.illum").unlink()
    (tmp_path / "on" / "output" / "dir.image_illum").unlink()
    again, _ = _run_rtm_code(tmp_path / "on", {"FDW_SHOT_WORKERS": "1"})
    for name in ("dir.image", "dir.illum", "dir.image_illum"):
        assert again[name] == on[name], name


@pytest.mark.gpu
def test_rtm_code_illum_in_groups_of_two_shots(tmp_path):
    """illum=1 under a batch budget that lets fdw_shot_batch_max be 2 (groups {0, 1}, {2, 3}, {4} through fdw_shot_batch_illum): dir.image,
    dir.illum and dir.image_illum against the oracle's shot loop stacked in shot order, every file against the run one shot at a time."""
    import batch_groups as G
    nx, nz, nxb, nzb, nt, ns, vp, d_obs, _ = G.five_shot_case(tmp_path / "grouped", extra="illum=1\n")
    G.five_shot_case(tmp_path / "single", extra="illum=1\n")
    grouped, r = G.run_program("rtm_code", tmp_path / "grouped", G.group_env(nx + 2 * nxb, nz + 2 * nzb, nxb, nzb, nt))
    G.assert_grouped(r.stderr, "fdw_shot_batch_illum")
    want = G.five_shot_oracle()
    img, ill = G.stack(want["image"]), G.stack(want["illum"])
    assert_bit_equal(np.frombuffer(grouped["dir.image"], np.float32).reshape(nx, nz), img, "dir.image")
    assert_bit_equal(np.frombuffer(grouped["dir.illum"], np.float32).reshape(nx, nz), ill, "dir.illum")
    assert_bit_equal(np.frombuffer(grouped["dir.image_illum"], np.float32), compensate_formula(img.ravel(), ill.ravel(), 1e-3), "dir.image_illum")
    assert ill.max() > 0 and all((want["illum"][s] != want["illum"][t]).any() for s in range(ns) for t in range(s))
    single, r1 = G.run_program("rtm_code", tmp_path / "single", {"FDW_NO_SHOT_BATCH": "1", "FDW_TIMING": "1"})
    G.assert_grouped(r1.stderr, "one by one", 1)
    assert sorted(grouped) == sorted(single)
    for name in single:
        assert grouped[name] == single[name], name
    assert (tmp_path / "grouped" / "image.num").read_bytes() == (tmp_path / "single" / "image.num").read_bytes()

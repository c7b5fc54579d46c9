"""fdw_dev_steps2 with the passes of the four-step kernel cut into row bands on side streams (fdwave.h: fdw_set_pass_bands).

A 230 x 300 extended grid with 23-row chunks (ten chunk rows, two strips) and 23 steps -- five passes plus three left-over steps -- from
noise-filled fields.  Bands / depth 3/1, 3/2, 5/3, 10/2 and 10/3 (the last two: bands of ONE chunk row) must give the CPU oracle's fields bit
for bit and the fields of the plain loop (1/1) bit for bit, in EXACT numerics and once in FAST; with the source on row 114 and on row 115,
either side of the band edge at row 115 = 5 x 23; on a compat deck whose rows 224..229 are never time-stepped (the last band copies them);
through one context in two calls (12 then 11 steps: first_pp_twice 0 then 1, it0 > 0, streams and events reused).  13-row chunks with ten
bands are too thin and must report one band.

Stream contract, in the manner of tests/test_stream_contract.py: behind a LATE PRODUCER on the caller's stream (decoys in every input until
a delay lets device copies put the true inputs in place) the call returns while the stream is busy and gives the oracle's answer to the
true inputs -- the side streams started behind the caller's stream; a CONSUMER copy queued on the caller's stream right after the call, no
device synchronisation in between, sees the final fields -- the side streams were joined."""
import ctypes as C
import functools

import numpy as np
import pytest

import stream_cases as SC
from conftest import assert_bit_equal, make_deck, random_fields
from oracle import oracle as O
from test_line_source import args_of
from test_stream_contract import DELAY_MS

gpu = pytest.mark.gpu
NXE, NZE, NXB, NZB, NT, XCHUNK = 230, 300, 12, 14, 23, 23
SETTINGS = [(1, 1), (3, 1), (3, 2), (5, 3), (10, 2), (10, 3)]
# name: compat, numerics, source row
DECKS = {"exact-114": (False, 0, 114), "exact-115": (False, 0, 115), "exact-static-rows-114": (True, 0, 114), "fast-115": (False, 1, 115)}
SZ = NZB + 40


@functools.lru_cache(maxsize=None)
def case(name, v="true"):
    """Inputs (v = "decoy": a second, different set on the same geometry) and the oracle's (P damped once, PP) after NT steps."""
    compat, numerics, sx = DECKS[name]
    seed = 5 if v == "true" else 17
    d = make_deck(NXE, NZE, NXB, NZB, NT, seed=seed, compat=compat, dz=12.5)
    base = O.ricker_wavelet(NT, d["dt"], 30.0)
    srce = (base * 1000.0 + 0.5).astype(np.float32) if v == "true" else (base * 700.0 + 3.0).astype(np.float32)
    p0, pp0 = random_fields(d, seed + 1, amp=0.1)
    orc = O.Oracle(*args_of(d), compat=compat, numerics=numerics)
    P, PP = orc.forward(d["v2"], sx, SZ, srce, p0, pp0, nsteps=NT)
    out = dict(d=d, v2=d["v2"], srce=srce, p0=p0, pp0=pp0, P=P, PP=PP, sx=sx)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


class RawStream:
    """A non-blocking HIP stream of the test's own, made by the runtime the library is linked to and handed to torch as an external stream.
    torch.cuda.Stream() would draw from torch's pool of 32 streams, and which of them share one of the process's four hardware queues is
    settled when each is first used: a module that draws from the pool shifts the streams every later module gets
    (tests/test_stream_contract.py's controls skip when their two streams share a queue).  This module leaves the pool as it found it."""

    def __init__(self, torch):
        import parallel_finite_difference_computation_amd as F
        self._hip, self._h = F.lib(), C.c_void_p()
        self._hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        self._hip.hipStreamDestroy.argtypes = [C.c_void_p]
        assert self._hip.hipStreamCreateWithFlags(C.byref(self._h), 1) == 0      # hipStreamNonBlocking
        self.stream = torch.cuda.ExternalStream(self._h.value)

    def close(self):
        assert self._hip.hipStreamDestroy(self._h) == 0


class Rig:
    """One context on a deck with its device buffers."""

    def __init__(self, name, torch, xchunk=XCHUNK):
        import parallel_finite_difference_computation_amd as F
        compat, numerics, _ = DECKS[name]
        self.name, self.torch, self.c = name, torch, case(name)
        self.ctx = F.FDWave(*args_of(self.c["d"]), compat=compat, device=0, numerics=numerics)
        self.ctx.set_tuning(xchunk=xchunk, two_step=4)
        assert self.ctx.steps_per_pass() == 4
        assert self.ctx.extents()[0] == (224 if compat else NXE)
        self.v2, self.srce = self.field(self.c["v2"]), torch.from_numpy(np.array(self.c["srce"])).to("cuda:0")
        self.bufs = [torch.zeros((NXE, self.ctx.pitch), device="cuda:0") for _ in range(4)]
        self._raw = RawStream(torch)
        self.stream = self._raw.stream

    def field(self, a):
        t = self.torch.zeros((NXE, self.ctx.pitch), device="cuda:0")
        t[:, :NZE] = self.torch.from_numpy(np.array(a)).to("cuda:0")
        return t

    def fill(self, c=None):
        c = c or self.c
        self.bufs[0].copy_(self.field(c["p0"]))
        self.bufs[1].copy_(self.field(c["pp0"]))
        for b, s in ((self.bufs[2], 7.0), (self.bufs[3], -7.0)):      # stale contents of the spare buffers must not matter
            b.fill_(s)
            b[:, NZE:] = 0

    def steps(self, it0, n, twice, ip, ipp, stream=None):
        s = stream or self.stream
        return self.ctx.dev_steps2([b.data_ptr() for b in self.bufs], self.v2.data_ptr(), self.srce.data_ptr(), self.c["sx"], SZ, it0, n,
                                   first_pp_twice=twice, ip=ip, ipp=ipp, stream=s.cuda_stream)

    def run(self, bands, depth, split=((0, NT),)):
        """(P damped once, PP) on the host after the calls of `split` on one stream, with no synchronisation between them."""
        torch = self.torch
        self.ctx.set_pass_bands(bands, depth)
        self.fill()
        torch.cuda.synchronize()
        ip, ipp = 0, 1
        for k, (it0, n) in enumerate(split):
            ip, ipp = self.steps(it0, n, k > 0, ip, ipp)
        self.ctx.dev_taper_finalize(self.bufs[ip].data_ptr(), stream=self.stream.cuda_stream)
        self.stream.synchronize()
        return self.bufs[ip][:, :NZE].cpu().numpy(), self.bufs[ipp][:, :NZE].cpu().numpy()

    def close(self):
        self.stream.synchronize()
        self.ctx.close()
        self._raw.close()


@gpu
@pytest.mark.parametrize("name", list(DECKS))
def test_banded_passes_equal_the_oracle_and_the_plain_loop(name):
    import torch
    rig = Rig(name, torch)
    plain = None
    for bands, depth in SETTINGS:
        P, PP = rig.run(bands, depth)
        assert rig.ctx.pass_bands() == (bands, depth), f"{name}: {bands}/{depth} was not used"
        what = f"{name}, bands/depth {bands}/{depth}"
        assert_bit_equal(PP, rig.c["PP"], "PP against the oracle, " + what)
        assert_bit_equal(P, rig.c["P"], "P against the oracle, " + what)
        if plain is None:
            plain = (P, PP)
        assert_bit_equal(PP, plain[1], "PP against the plain loop, " + what)
        assert_bit_equal(P, plain[0], "P against the plain loop, " + what)
    rig.close()


@gpu
@pytest.mark.parametrize("name", ["exact-115", "exact-static-rows-114"])
def test_one_context_through_two_calls(name):
    """12 steps (three passes), then 11 (two passes and three single steps) with it0 = 12 and first_pp_twice = 1, queued back to back."""
    import torch
    rig = Rig(name, torch)
    for bands, depth in ((3, 2), (10, 3), (5, 3), (1, 1)):
        P, PP = rig.run(bands, depth, split=((0, 12), (12, 11)))
        what = f"{name}, 12 + 11 steps, bands/depth {bands}/{depth}"
        assert rig.ctx.pass_bands() == (bands, depth)
        assert_bit_equal(PP, rig.c["PP"], "PP, " + what)
        assert_bit_equal(P, rig.c["P"], "P, " + what)
    rig.close()


@gpu
def test_thin_bands_run_as_one_band():
    """Ten bands of 13-row chunks are below the 16 rows a pass reads beyond its own: the plain loop, and it says so.  So does automatic."""
    import torch
    rig = Rig("exact-115", torch, xchunk=13)
    P, PP = rig.run(10, 2)
    assert rig.ctx.pass_bands() == (1, 1)
    assert_bit_equal(PP, rig.c["PP"], "PP, 13-row chunks")
    assert_bit_equal(P, rig.c["P"], "P, 13-row chunks")
    P, PP = rig.run(0, 0)
    assert rig.ctx.pass_bands() == (1, 1)
    assert_bit_equal(PP, rig.c["PP"], "PP, automatic")
    import parallel_finite_difference_computation_amd as F
    for bad in ((3, 0), (0, 2), (-1, 1), (3, 4)):
        with pytest.raises(F.FdwError):
            rig.ctx.set_pass_bands(*bad)
    rig.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the stream contract
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_delay():
    import torch
    return torch, SC.Delay(torch)


def test_the_decoys_matter():
    for name in ("exact-115", "exact-static-rows-114"):
        t, d = case(name), case(name, "decoy")
        for k in ("P", "PP"):
            assert (t[k].view(np.uint32) != d[k].view(np.uint32)).mean() > 0.5 and not np.isin(t[k], (7.0, -7.0)).any()


def _behind_a_late_producer(rig, bands, depth, delay, finalize):
    """Decoys in place and the device synchronised; then on ONE stream: delay, the true inputs, the call, copies of all four buffers.
    Returns (busy when the call returned, ip, ipp, the copies)."""
    torch = rig.torch
    decoy = case(rig.name, "decoy")
    rig.ctx.set_pass_bands(bands, depth)
    rig.fill()
    torch.cuda.synchronize()
    rig.steps(0, NT, False, 0, 1)                       # code objects, side streams and events exist before the timed part
    rig.stream.synchronize()
    assert rig.ctx.pass_bands() == (bands, depth)
    stage = [rig.field(rig.c["p0"]), rig.field(rig.c["pp0"]), rig.field(rig.c["v2"]), rig.srce.clone()]
    rig.fill(decoy)
    rig.v2.copy_(rig.field(decoy["v2"]))
    rig.srce.copy_(torch.from_numpy(np.array(decoy["srce"])).to("cuda:0"))
    res = [torch.empty_like(b) for b in rig.bufs]
    raw = RawStream(torch)
    S = raw.stream
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        delay(DELAY_MS)
        for dst, src in zip((rig.bufs[0], rig.bufs[1], rig.v2, rig.srce), stage):
            dst.copy_(src, non_blocking=True)
        ip, ipp = rig.steps(0, NT, False, 0, 1, stream=S)
        if finalize:
            rig.ctx.dev_taper_finalize(rig.bufs[ip].data_ptr(), stream=S.cuda_stream)
        busy = not S.query()
        for r, b in zip(res, rig.bufs):
            r.copy_(b, non_blocking=True)
    S.synchronize()
    raw.close()
    return busy, ip, ipp, [r[:, :NZE].cpu().numpy() for r in res]


@gpu
@pytest.mark.parametrize("bands,depth", [(3, 2), (10, 3)])
@pytest.mark.parametrize("name", ["exact-115", "exact-static-rows-114"])
def test_late_producer(name, bands, depth, torch_delay):
    torch, delay = torch_delay
    rig = Rig(name, torch)
    busy, ip, ipp, res = _behind_a_late_producer(rig, bands, depth, delay, finalize=True)
    assert busy, f"{name} {bands}/{depth}: the stream was idle when the call returned: it synchronised, or outlasted the delay"
    assert_bit_equal(res[ipp], rig.c["PP"], f"PP behind a late producer, {name} {bands}/{depth}")
    assert_bit_equal(res[ip], rig.c["P"], f"P behind a late producer, {name} {bands}/{depth}")
    rig.close()


@gpu
@pytest.mark.parametrize("bands,depth", [(3, 2), (10, 3)])
def test_consumer_on_the_callers_stream_sees_the_final_fields(bands, depth, torch_delay):
    """The copies follow the call directly on the caller's stream: they read rows the side streams wrote last (and, for P, rows the
    left-over steps wrote after the join).  P is compared undamped, against the plain loop's buffer."""
    torch, delay = torch_delay
    rig = Rig("exact-115", torch)
    rig.ctx.set_pass_bands(1, 1)
    rig.fill()
    torch.cuda.synchronize()
    pip, pipp = rig.steps(0, NT, False, 0, 1)
    rig.stream.synchronize()
    raw_p = rig.bufs[pip][:, :NZE].cpu().numpy()
    busy, ip, ipp, res = _behind_a_late_producer(rig, bands, depth, delay, finalize=False)
    assert busy and (ip, ipp) == (pip, pipp)
    assert_bit_equal(res[ipp], rig.c["PP"], f"PP as a consumer on the caller's stream sees it, {bands}/{depth}")
    assert_bit_equal(res[ip], raw_p, f"P (undamped) as a consumer on the caller's stream sees it, {bands}/{depth}")
    rig.close()

"""The ISA of the EXACT four-step kernels as built into libfdwave.so (csrc/fdw_device.h, laplacian_quad): the z half shares its products
between lanes through DPP adds, and the register budget the launch bounds set still holds.  Reads the embedded gfx950 code objects with the
ROCm LLVM tools (no GPU)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LIB = os.path.join(ROOT, "parallel_finite_difference_computation_amd", "libfdwave.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
HEADLINE = "_ZN3fdw16fdw_stepn_kernelILi4ELi4ELb1ELi1ELi2ELb0ELi0ELi0EEEvNS_9Step2ArgsE"      # fdw_stepn_kernel<4,4,true,1,2,false,0,0>
# the EXACT kernels whose Laplacian is lap_quad<0>: forward (FWD, PLAIN, PLAIN_ALL), receiver field, trace recording, fused backward
EXACT_QUAD = re.compile(r"^(_ZN3fdw16fdw_stepn_kernelILi4ELi4ELb[01]ELi[0-2]ELi2ELb0ELi[0-2]ELi0EEEvNS_9Step2ArgsE"
                        r"|_ZN3fdw20fdw_stepn_rec_kernelILi0EEEvNS_9Step2ArgsE|_ZN3fdw16fdw_back4_kernelILi4ELi4ELi2ELi0EEEvNS_9Step2ArgsE)$")
DPP_WAIT_STATES = 2      # a VALU write of a VGPR, then a DPP read of it (LLVM's GCNHazardRecognizer::checkDPPHazards)


def _code_objects(td):
    fat = os.path.join(td, "fatbin.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", LIB, fat], check=True)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    for i, a in enumerate(starts):
        piece = os.path.join(td, f"bundle{i}.bin")
        open(piece, "wb").write(blob[a:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        co = os.path.join(td, f"code{i}.co")
        r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={piece}", f"--output={co}"],
                           capture_output=True, text=True)
        if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) > 0:
            yield co


@pytest.fixture(scope="module")
def isa():
    """{kernel symbol: (metadata dict, [(mnemonic, operands)])} for every kernel of the library."""
    if not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/llvm-objdump")):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in _code_objects(td):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            meta = {}
            for block in re.split(r"\n  - \.", notes)[1:]:            # one block per entry of amdhsa.kernels
                name = re.search(r"\.name:\s+(\S+)", block)
                if name:
                    meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count):\s+(\d+)", block)}
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout
            func = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    func = m.group(1)
                    out.setdefault(func, (meta.get(func, {}), []))
                    continue
                m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//\s*[0-9A-Fa-f]+:", line)
                if m and func:
                    out[func][1].append((m.group(1), [o.strip() for o in m.group(2).split(",")] if m.group(2) else []))
    assert HEADLINE in out, "the headline kernel was not found in the disassembly"
    return out


def _vregs(tok):
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", tok)
    return {int(m.group(1))} if m else set()


def test_exact_four_step_kernels_fit_their_launch_bounds_without_scratch(isa):
    """The headline kernel stays at 96 VGPRs (5 workgroups of four waves per CU); no EXACT four-step kernel spills a VGPR or uses scratch."""
    quad = [k for k in isa if EXACT_QUAD.match(k)]
    assert len(quad) == 6, sorted(quad)
    for k in quad:
        meta = isa[k][0]
        assert meta.get("private_segment_fixed_size") == 0 and meta.get("vgpr_spill_count") == 0, (k, meta)
    assert isa[HEADLINE][0]["vgpr_count"] <= 96, isa[HEADLINE][0]


def test_exact_four_step_z_half_shares_products_through_dpp_adds(isa):
    """No lane moves (v_mov_b32_dpp) are left in the EXACT four-step kernels; a march step's Laplacian holds the shared z half's 14
    v_add_f32_dpp (four partial sums from the left lane, ten products from the right lane), so the code between two workgroup barriers in
    address order holds a multiple of 14 (two bodies can meet there)."""
    for k in (k for k in isa if EXACT_QUAD.match(k)):
        body = isa[k][1]
        assert not any(mn == "v_mov_b32_dpp" for mn, _ in body), k
        counts, n = [], 0
        for mn, _ in body:
            if mn == "s_barrier":
                counts.append(n)
                n = 0
            elif mn == "v_add_f32_dpp":
                n += 1
        assert counts and all(c % 14 == 0 for c in counts) and 14 in counts, (k, sorted(set(counts)))


def test_no_dpp_read_within_two_wait_states_of_a_valu_write(isa):
    """Every DPP instruction of the library reads VGPRs that no VALU instruction wrote in the two wait states before it (straight-line code,
    s_nop N = N + 1 wait states): the hazard hipcc pads for instructions it emitted itself, checked on what was built."""
    ndpp = 0
    for k, (_, body) in isa.items():
        for i, (mn, ops) in enumerate(body):
            if not mn.endswith("_dpp"):
                continue
            ndpp += 1
            reads = set().union(*(_vregs(o.split()[0]) for o in ops[1:])) if len(ops) > 1 else set()
            states, j = 0, i - 1
            while states < DPP_WAIT_STATES and j >= 0:
                pmn, pops = body[j]
                if pmn == "s_nop":
                    states += int(pops[0], 0) + 1 if pops else 1
                else:
                    if pmn.startswith("v_") and not pmn.startswith(("v_cmp", "v_readlane", "v_readfirstlane", "v_nop")) and pops:
                        assert not (_vregs(pops[0]) & reads), f"{k}: {pmn} {', '.join(pops)} then {mn} {', '.join(ops)} after {states} wait state(s)"
                    states += 1
                j -= 1
    assert ndpp > 100, "no DPP instructions found in the disassembly"

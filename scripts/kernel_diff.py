#!/usr/bin/env python3
"""kernel_diff.py LIB_A LIB_B -- do two builds of libfdwave.so hold the same device code?

Unbundles the gfx950 code objects of both libraries (as tests/test_stepn_isa_budget.py does) and compares, per kernel symbol,
  - the instruction text of `llvm-objdump -d`: mnemonics and operands in order, addresses and encodings stripped;
  - the figures of `llvm-readelf --notes`: VGPRs, AGPRs, SGPRs, both spill counts, scratch, LDS and kernel-argument bytes.
Lists the symbols only one library has and those a library holds in more than one code object.  Exit status 0 if and only if both libraries
hold the same kernels, each once, identical in text and in every figure: the check of a change that must leave the device code alone.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("FDW_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
           "group_segment_fixed_size", "kernarg_segment_size")


def code_objects(lib, td):
    fat = os.path.join(td, "fatbin.bin")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
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


def kernels(lib):
    """{kernel symbol: (figures dict, [instruction lines])} and the symbols found in more than one code object."""
    out, twice = {}, []
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(lib, td):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
            meta = {}
            for block in re.split(r"\n  - \.", notes)[1:]:            # one block per entry of amdhsa.kernels
                name = re.search(r"\.name:\s+(\S+)", block)
                if name:
                    meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIGURES), block)}
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout
            body = {}
            func = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    func = m.group(1)
                    body.setdefault(func, [])
                    continue
                m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//\s*[0-9A-Fa-f]+:", line)
                if m and func:
                    body[func].append((m.group(1) + " " + re.sub(r"\s*<[^>]*>", "", m.group(2))).strip())
            for name, fig in meta.items():
                if name in out:
                    twice.append(name)
                out[name] = (fig, body.get(name, []))
    return out, twice


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    (ka, twice_a), (kb, twice_b) = kernels(argv[1]), kernels(argv[2])
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    both = sorted(set(ka) & set(kb))
    fig_diff = [k for k in both if ka[k][0] != kb[k][0]]
    text_diff = [k for k in both if ka[k][1] != kb[k][1]]
    empty = [k for k in both if not ka[k][1] or not kb[k][1]]
    print(f"A: {argv[1]}: {len(ka)} kernels   B: {argv[2]}: {len(kb)} kernels   in both: {len(both)}")
    print(f"only in A: {len(only_a)}   only in B: {len(only_b)}   in more than one code object: A {len(twice_a)}, B {len(twice_b)}")
    print(f"identical figures ({', '.join(FIGURES)}): {len(both) - len(fig_diff)} of {len(both)}")
    print(f"identical instruction text: {len(both) - len(text_diff)} of {len(both)}   instructions compared: {sum(len(ka[k][1]) for k in both)}")
    for title, names in (("only in A", only_a), ("only in B", only_b), ("twice in A", twice_a), ("twice in B", twice_b), ("no disassembly found", empty)):
        for k in names:
            print(f"{title}: {k}")
    for k in fig_diff:
        print(f"figures differ: {k}: " + ", ".join(f"{f} {ka[k][0].get(f)} -> {kb[k][0].get(f)}" for f in FIGURES if ka[k][0].get(f) != kb[k][0].get(f)))
    for k in text_diff:
        ta, tb = ka[k][1], kb[k][1]
        first = next((i for i, (x, y) in enumerate(zip(ta, tb)) if x != y), min(len(ta), len(tb)))
        print(f"text differs: {k}: {len(ta)} -> {len(tb)} instructions, first at {first}: "
              f"{ta[first] if first < len(ta) else '(end)'} | {tb[first] if first < len(tb) else '(end)'}")
    same = not (only_a or only_b or twice_a or twice_b or empty or fig_diff or text_diff) and len(both) > 0
    print("SAME DEVICE CODE" if same else "DEVICE CODE DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))

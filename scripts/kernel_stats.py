#!/usr/bin/env python
"""Register, LDS and scratch figures and the instruction count of the kernels of a built library, read from its gfx950
code object (llvm-readelf notes, llvm-objdump): what tests/test_abi.py holds to budgets, as a table.

    python scripts/kernel_stats.py gym_anm_amd/_build/libanm_<topology>.so [substring ...]

Only kernels whose demangled name contains one of the substrings are listed (default: all)."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ANM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def kernel_stats(lib):
    with tempfile.TemporaryDirectory() as td:
        sec, co = os.path.join(td, "fat.bin"), os.path.join(td, "gfx950.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + sec, lib], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + sec, "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
    count, scratch, cur = {}, {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            count[cur], scratch[cur] = 0, 0
        elif cur and re.match(r"^\s+[a-z]", line):
            count[cur] += 1
            if re.search(r"\b(scratch_|buffer_(load|store))", line):
                scratch[cur] += 1
    out = {}
    for blk in notes.split("- .agpr_count")[1:]:
        mangled = re.search(r"\.name:\s+(\S+)", blk).group(1)
        name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
        g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))  # noqa: E731
        out[name] = dict(vgpr=g("vgpr_count"), sgpr=g("sgpr_count"), vgpr_spill=g("vgpr_spill_count"), sgpr_spill=g("sgpr_spill_count"),
                         lds=g("group_segment_fixed_size"), scratch=g("private_segment_fixed_size"),
                         scratch_insts=scratch.get(mangled, 0), insts=count.get(mangled, 0))
    return out


def main(argv):
    if len(argv) < 2:
        print(__doc__)
        return 2
    subs = argv[2:]
    print("%-100s %5s %5s %6s %6s %7s %7s %6s %7s" % ("kernel", "vgpr", "sgpr", "vspill", "sspill", "lds B", "scr B", "scr i", "insts"))
    for name, s in sorted(kernel_stats(argv[1]).items()):
        short = name.split("(anm::")[0].replace("(anonymous namespace)::", "")
        if subs and not any(x in short for x in subs):
            continue
        print("%-100s %5d %5d %6d %6d %7d %7d %6d %7d" % (short[:100], s["vgpr"], s["sgpr"], s["vgpr_spill"], s["sgpr_spill"], s["lds"],
                                                       s["scratch"], s["scratch_insts"], s["insts"]))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

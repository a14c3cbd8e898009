"""Compare the gfx950 code of two builds of a library, kernel by kernel, as text.

    python scripts/isa_diff.py [--mnemonics] LIB_A LIB_B [name filter]

Each library's gfx950 code object is extracted (as scripts/kernel_resources.py does) and disassembled with
llvm-objdump -d; addresses, encodings and the numbering of labels are dropped.  One line per kernel: `identical`, or the
instruction counts of both and the first differing instruction.  Exit status 1 when some kernel differs or is missing.
--mnemonics: compare the mnemonic streams alone (operands dropped) -- a kernel whose arguments moved inside the kernarg
segment, or whose registers were renumbered, is then still `identical`.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(lib, td, tag):
    co = os.path.join(td, tag + ".co")
    unbundle = [os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", TARGET, "--output=" + co]
    subprocess.run(unbundle + ["--input=" + lib], check=False, capture_output=True)
    if not os.path.exists(co) or os.path.getsize(co) == 0:
        sec = os.path.join(td, tag + ".fatbin")  # the fat binary sits in a section of the shared library
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + sec, lib], check=True)
        subprocess.run(unbundle + ["--input=" + sec], check=True)
    return co


def kernels(lib, td, tag):
    """{symbol: [instruction text, ...]} of every function of the library's gfx950 code object"""
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", code_object(lib, td, tag)],
                         capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:\s*$", line.strip())
        if m:
            if re.match(r"^L\d+$", m.group(1)) is None:  # a branch target inside a kernel is not a new kernel
                cur = out.setdefault(m.group(1), [])
            continue
        ins = line.split("//")[0].strip()  # (the comment holds the address and the encoding)
        if cur is None or not ins or ins.startswith("Disassembly of") or "file format" in ins:
            continue
        cur.append(re.sub(r"\bL\d+\b", "L", re.sub(r"\s+", " ", ins)))
    return out


def main():
    mnemonics = "--mnemonics" in sys.argv
    if mnemonics:
        sys.argv.remove("--mnemonics")
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    with tempfile.TemporaryDirectory() as td:
        a, b = kernels(sys.argv[1], td, "a"), kernels(sys.argv[2], td, "b")
    if mnemonics:
        a, b = ({k: [ins.split(" ")[0] for ins in v] for k, v in x.items()} for x in (a, b))
    differ = False
    for name in sorted(set(a) | set(b)):
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if flt and flt not in dem:
            continue
        if name not in a or name not in b:
            verdict = "only in " + ("A" if name in a else "B")
        elif a[name] == b[name]:
            verdict = "identical"
        else:
            k = next((i for i, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
            at = lambda v: v[k] if k < len(v) else "(end)"  # noqa: E731
            verdict = "%d / %d instructions, first difference at %d: %s | %s" % (len(a[name]), len(b[name]), k, at(a[name]), at(b[name]))
        differ = differ or verdict != "identical"
        print("%s: %s" % (dem, verdict))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()

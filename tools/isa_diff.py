#!/usr/bin/env python3
"""Per-kernel ISA comparison of two builds (manual tool for behaviour-preserving refactors).

usage: tools/isa_diff.py A B [name-substring]
A and B are built libqmfx.so or object files.  Every gfx950 code object in each is disassembled
as tests/test_isa.py does; per mangled kernel name the instruction text (encodings included,
addresses dropped) is compared and `same`, `differs`, `only in A` or `only in B` is printed."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def kernels(path):
    """{mangled name: instruction text} over every code object bundled in `path`."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run(["objcopy", "--dump-section", ".hip_fatbin=" + fat, path], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(MAGIC, blob)] + [len(blob)]
        for n, (b, e) in enumerate(zip(starts, starts[1:])):
            one, co = os.path.join(d, "b%d" % n), os.path.join(d, "c%d" % n)
            open(one, "wb").write(blob[b:e])
            subprocess.run([LLVM + "/clang-offload-bundler", "--type=o", "--unbundle",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + one,
                            "--output=" + co], check=True)
            if not os.path.getsize(co):
                continue
            text = subprocess.run([LLVM + "/llvm-objdump", "-d", co], check=True,
                                  capture_output=True, text=True).stdout
            name = None
            for line in text.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = m.group(1)
                    out[name] = []
                elif name and "//" in line:
                    # mnemonic and operands, then the encoding words (not the address)
                    ins, enc = line.split("//", 1)
                    out[name].append(ins.strip() + " ;" + enc.split(":", 1)[1])
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pick = sys.argv[3] if len(sys.argv) > 3 else ""
    counts = {}
    for name in sorted(set(a) | set(b)):
        if pick not in name:
            continue
        verdict = ("only in B" if name not in a else "only in A" if name not in b
                   else "same" if a[name] == b[name] else "differs")
        counts[verdict] = counts.get(verdict, 0) + 1
        print("%-9s %s" % (verdict, name))
    print(" ".join("%s: %d" % kv for kv in sorted(counts.items())), file=sys.stderr)
    return 1 if set(counts) - {"same"} else 0


if __name__ == "__main__":
    sys.exit(main())

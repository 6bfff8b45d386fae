#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --cuda-device-only -S) kernel by kernel.

usage: tools/asm_diff_kernels.py OLD.s NEW.s

Kernels are the symbols with an .amdhsa_kernel descriptor; a __device__ function that was not inlined has none
and is not compared.  Reports symbols present on one side only, and
kernels whose instruction text or .amdhsa_* descriptor differs; the order of the kernels in the file and
compiler-numbered local labels (.LBB<n>_, .Ltmp<n>, .Lfunc_end<n>) do not count.  Exit status 1 on any difference.
"""
import re
import sys

LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+")


def kernels(path):
    text = open(path).read().split("\n")
    desc, body = {}, {}
    i = 0
    while i < len(text):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", text[i])
        if m:
            j = i
            while ".end_amdhsa_kernel" not in text[j]:
                j += 1
            desc[m.group(1)] = [l.strip() for l in text[i + 1:j]]
            i = j
        i += 1
    label = {l.split(":")[0]: k for k, l in enumerate(text) if l[:1] not in ("", "\t", " ", ".", ";") and ":" in l}
    for name in desc:
        start = label[name]
        end = start
        while not text[end].startswith(".Lfunc_end"):
            end += 1
        lines = []
        for l in text[start + 1:end]:
            l = l.split(";")[0].strip()   # drop comments
            if l and not l.startswith((".loc", ".file", ".cfi")):
                lines.append(LOCAL.sub(lambda m: ".L" + m.group(1), l))
        body[name] = lines
    return desc, body


def main():
    (d0, b0), (d1, b1) = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for n in sorted(set(d0) - set(d1)):
        print("only in old:", n); bad += 1
    for n in sorted(set(d1) - set(d0)):
        print("only in new:", n); bad += 1
    for n in sorted(set(d0) & set(d1)):
        if b0[n] != b1[n]:
            print("instructions differ:", n); bad += 1
        if d0[n] != d1[n]:
            print("descriptor differs:", n); bad += 1
    print(f"{sys.argv[2]}: {len(d1)} kernels, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Per-kernel comparison of two sets of gfx950 assembly files (hipcc --cuda-device-only -S).

usage: kernel_asm_diff.py [-v] OLD NEW
OLD, NEW: a directory of *.s files, or a comma-separated list of them.

For every kernel symbol (one with an .amdhsa_kernel block), in whichever file of a side holds it:
the instruction stream and the .amdhsa_kernel ... .end_amdhsa_kernel descriptor are compared
separately, after stripping comments, .file / .loc / .ident lines and local label numbers. Reports
same / differs per kernel with the instruction counts of both sides, kernels present on one side
only and kernels defined twice on a side; -v prints a unified diff of what differs. Exits non-zero
on any difference.
"""
import difflib
import glob
import os
import re
import sys

LABEL = re.compile(r"\.?L(BB|func_end|func_begin|tmp|JTI)?[0-9_]+")


def clean(line):
    line = re.sub(r"\s*(;|//).*$", "", line).strip()
    if not line or re.match(r"\.(file|loc|ident)\b", line):
        return None
    return LABEL.sub(".L", line)


def kernels(spec):
    files = sorted(glob.glob(os.path.join(spec, "*.s"))) if os.path.isdir(spec) else spec.split(",")
    code, desc, dup = {}, {}, []
    for path in files:
        lines = open(path).read().split("\n")
        names = [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
        for name in names:
            if name in code:
                dup.append(name)
            start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
            d0 = next(i for i, ln in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"$", ln))
            d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
            code[name] = [c for c in map(clean, lines[start + 1 : d0]) if c]
            desc[name] = [c for c in map(clean, lines[d0 : d1 + 1]) if c]
    return code, desc, dup


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    (c0, d0, dup0), (c1, d1, dup1) = kernels(args[0]), kernels(args[1])
    bad = 0
    for name in sorted(set(c0) | set(c1)):
        if name not in c0 or name not in c1:
            print(f"{name}: only in {'OLD' if name in c0 else 'NEW'}")
            bad += 1
            continue
        insn = lambda c: sum(1 for x in c if not x.startswith(".") and not x.endswith(":"))
        cs, ds = c0[name] == c1[name], d0[name] == d1[name]
        print(f"{name}: code {'same' if cs else 'differs'} ({insn(c0[name])} / {insn(c1[name])} instructions), "
              f"descriptor {'same' if ds else 'differs'}")
        bad += (not cs) + (not ds)
        if verbose:
            for a, b in ((c0, c1), (d0, d1)):
                if a[name] != b[name]:
                    print("\n".join(difflib.unified_diff(a[name], b[name], "OLD", "NEW", lineterm="", n=2)))
    for side, dup in (("OLD", dup0), ("NEW", dup1)):
        for name in dup:
            print(f"{name}: defined more than once in {side}")
            bad += 1
    print(f"{len(set(c0) | set(c1))} kernels, {bad} differences")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

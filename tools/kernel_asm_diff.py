#!/usr/bin/env python3
"""Compare the device assembly of two builds, symbol by symbol.

usage: kernel_asm_diff.py DIR_A DIR_B

Each directory holds one .s file per .hip source, made with the Makefile's HIPFLAGS plus
`--cuda-device-only -S`.  A symbol is a kernel or device function: the lines from its label to
its `.Lfunc_end` label.  Prints per file how many symbols there are and which differ, and exits
with status 1 if any does.

Ignored, because they change without the code changing:
  - blank lines, comment lines (`;`, `//`) and trailing `;` comments;
  - `.file` and `.ident` lines, and quoted absolute paths (replaced by "PATH");
  - the `__hip_cuid_*` symbol, a hash of the translation unit's source;
  - everything between symbols (section directives, the metadata notes).
"""
import os
import re
import sys

LABEL = re.compile(r"^([A-Za-z_][\w.$]*):$")


def clean(line):
    """The line as it is compared, or None if it is dropped."""
    t = line.strip()
    if not t or t.startswith((";", "//", ".file", ".ident")):
        return None
    t = re.sub(r"\s*;.*$", "", t)
    return re.sub(r'"/[^"]*"', '"PATH"', t)


def symbols(path):
    """{symbol: its cleaned lines} of one assembly file."""
    out, name = {}, None
    with open(path) as f:
        for line in f:
            t = clean(line)
            if t is None:
                continue
            m = LABEL.match(t)
            if m and not t.startswith(".L"):
                name = None if m.group(1).startswith("__hip_cuid") else m.group(1)
                if name:
                    out.setdefault(name, [])
            if name:
                out[name].append(t)
            if t.startswith(".Lfunc_end"):
                name = None
    return out


def main(dir_a, dir_b):
    total = differ = 0
    for fn in sorted(set(os.listdir(dir_a)) | set(os.listdir(dir_b))):
        if not fn.endswith(".s"):
            continue
        a = symbols(os.path.join(dir_a, fn)) if os.path.exists(os.path.join(dir_a, fn)) else {}
        b = symbols(os.path.join(dir_b, fn)) if os.path.exists(os.path.join(dir_b, fn)) else {}
        names = sorted(set(a) | set(b))
        bad = [n for n in names if a.get(n) != b.get(n)]
        total += len(names)
        differ += len(bad)
        print(f"{fn}: {len(names)} symbols, {len(bad)} differ", *bad)
    print(f"total: {total} symbols, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

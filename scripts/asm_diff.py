#!/usr/bin/env python3
"""Compare two gfx950 assembly listings kernel by kernel (refactors that must not move an instruction).

Build the same .hip file from two trees with the Makefile's flags plus -save-temps=obj and pass the two
*-gfx950.s listings.  `;` comments and blank lines are dropped; a kernel's text is everything from its `.globl` line to
the next kernel's (code, .amdhsa_* directives, its constants) plus its entry of the metadata block.  Exit status 1 if
any kernel differs or exists on one side only.
"""
import re
import sys


def kernels(path):
    lines = []
    for ln in open(path):
        ln = ln.split(";", 1)[0].rstrip()
        if ln.strip():
            lines.append(ln)
    meta0 = next((i for i, ln in enumerate(lines) if ln.strip() == ".amdgpu_metadata"), len(lines))
    out, name = {}, None
    for ln in lines[:meta0]:
        m = re.match(r"\s*\.globl\s+(\S+)", ln)
        if "__hip_cuid" in ln:   # the id object of the build that follows the last kernel: not kernel text
            name = None
        elif m:
            name = m.group(1)
        if name:
            out.setdefault(name, []).append(ln)
    entry = []
    for ln in lines[meta0:] + ["  - .end"]:   # one YAML list item per kernel under amdhsa.kernels
        if ln.startswith("  - ") and entry:
            nm = [e.split(":", 1)[1].strip() for e in entry if e.startswith("    .name:")]   # (arguments sit deeper)
            if nm and nm[0] in out:
                out[nm[0]] += entry
            entry = []
        entry.append(ln)
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(set(a) | set(b))
    same = [n for n in names if a.get(n) == b.get(n)]
    for n in names:
        if n not in same:
            where = "differs" if n in a and n in b else "only in " + (sys.argv[1] if n in a else sys.argv[2])
            print(f"{where}: {n}")
    print(f"{len(names)} kernel symbols, {len(same)} identical")
    return 0 if len(same) == len(names) else 1


if __name__ == "__main__":
    sys.exit(main())

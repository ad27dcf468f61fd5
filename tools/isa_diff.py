#!/usr/bin/env python3
"""Compare the device assembly of two builds, symbol by symbol.

    hipcc --offload-arch=gfx950 <the Makefile's flags> --offload-device-only -S dn_x.hip -o <dir>/dn_x.s    (both trees)
    python tools/isa_diff.py <dir before> <dir after>

Per .s file: kernels before / after, symbols gone, symbols new, symbols whose code differs.  A symbol's code is the text from
`<symbol>:` to its `.Lfunc_end`, plus its `.amdhsa_kernel` block (registers, LDS, scratch).  Comments, trailing blanks, the
per-file function index in local labels and the `__hip_cuid_<hash>` symbol are normalised away; nothing else is: text only.
Exit status 1 if any symbol differs or is new.
"""
import os
import re
import sys

_SUBS = [(re.compile(r"\.LBB\d+_"), ".LBB#_"), (re.compile(r"\.LJTI\d+_"), ".LJTI#_"), (re.compile(r"\bBB\d+_"), "BB#_"),
         (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1#"), (re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_#")]


def _norm(line):
    line = line.split(";", 1)[0].rstrip()
    for rx, to in _SUBS:
        line = rx.sub(to, line)
    return line


def symbols(path):
    """{symbol: normalised code}, set of kernel symbols"""
    lines = open(path).read().split("\n")
    funcs = [m.group(1) for m in (re.match(r"\s*\.type\s+([^,\s]+),@function", ln) for ln in lines) if m]
    start = {m.group(1): i for i, m in enumerate(re.match(r"([^.\s][^:\s]*):", ln) for ln in lines) if m}
    code, kernels = {}, set()
    for f in funcs:
        i = start[f]
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        code[f] = [_norm(ln) for ln in lines[i:j + 1]]
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
            code[m.group(1)] += [_norm(x) for x in lines[i:j + 1]]
            kernels.add(m.group(1))
    return {f: "\n".join(x for x in c if x) for f, c in code.items()}, kernels


def main(before, after):
    bad = 0
    names = sorted(set(os.listdir(before)) | set(os.listdir(after)))
    for name in (n for n in names if n.endswith(".s")):
        pb, pa = os.path.join(before, name), os.path.join(after, name)
        (cb, kb), (ca, ka) = (symbols(p) if os.path.exists(p) else ({}, set()) for p in (pb, pa))
        gone, new = sorted(set(cb) - set(ca)), sorted(set(ca) - set(cb))
        differ = sorted(f for f in set(cb) & set(ca) if cb[f] != ca[f])
        print("%-28s kernels %3d -> %3d   symbols gone %d, new %d, differ %d" % (name, len(kb), len(ka), len(gone), len(new), len(differ)))
        for tag, group in (("gone", gone), ("new", new), ("differs", differ)):
            for f in group:
                print("    %-8s %s" % (tag, f))
        bad += len(new) + len(differ)
    print("TOTAL: %d symbols new or different" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

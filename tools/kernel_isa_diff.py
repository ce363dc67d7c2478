#!/usr/bin/env python3
"""Compare the kernels of two device assembly listings (hipcc --cuda-device-only -S) function by function: which kernels have the same
instruction stream in both, which differ, which exist on one side only -- and, from a listing's .amdhsa directives, the registers and the
scratch of the kernels named.

    tools/kernel_isa_diff.py before.s after.s [--resources SUBSTRING ...]

A function's stream is its lines between its label and .Lfunc_end, without comments, directives that carry no code (.loc, .file, .cfi_*,
.p2align), blank lines and debug labels; local labels are renumbered in order of appearance, so that code added elsewhere in the file does
not make an untouched kernel look different."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        s = line.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+|\w+):\s*$", s)
        if name is None:
            if m and not s.startswith(".L"):
                name, body = m.group(1), []
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = s.strip()
        if not t or t.startswith((".loc", ".file", ".cfi_", ".p2align", ".Ltmp", ".Lfunc_begin")):
            continue
        body.append(t)
    return out


def renumbered(body):
    names = {}

    def local(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))
    return [re.sub(r"\.LBB\d+_\d+", local, t) for t in body]


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size|accum_offset)\s+(\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
        m = re.match(r"\s*;\s*(ScratchSize|NumVgprs|NumSgprs|NumAgprs|Occupancy|codeLenInByte):\s*(\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    a, b = functions(argv[1]), functions(argv[2])
    same = [k for k in a if k in b and renumbered(a[k]) == renumbered(b[k])]
    differ = [k for k in a if k in b and k not in same]
    print("%d functions in both with the same instruction stream" % len(same))
    for k in differ:
        print("DIFFERS   %s (%d -> %d lines)" % (k, len(a[k]), len(b[k])))
    for k in a:
        if k not in b:
            print("REMOVED   %s" % k)
    for k in b:
        if k not in a:
            print("NEW       %s (%d lines)" % (k, len(b[k])))
    if "--resources" in argv:
        want = argv[argv.index("--resources") + 1:]
        for k, r in resources(argv[2]).items():
            if any(w in k for w in want):
                print("%s: %s" % (k, " ".join("%s=%d" % kv for kv in sorted(r.items()))))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

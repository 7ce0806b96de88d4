#!/usr/bin/env python3
"""Compare device assembly files (hipcc ... --cuda-device-only -S) function by function.

    python tools/isa_same.py OLD.s NEW.s [NEW2.s ...] [--meta REGEX]

NEW may be several files, the units a source file was split into: their union is compared with
OLD, and a symbol that more than one NEW file defines is a difference (a kernel instantiated in
two units).  A plain text comparison: a function is the lines from its label to its .size
directive (for a kernel that includes its descriptor block), with blank lines, assembler comment
lines and trailing ; comments dropped, and the function's ordinal in its unit taken out of the
local labels (.LBB<n>_<m> -> .LBB_<m>, .Lfunc_end<n> -> .Lfunc_end), so that neither the order
of the functions in a unit nor the unit they stand in shows; functions are matched by symbol.
Prints "same" or the first differing line plus the two line counts for every function, compares
the register, scratch and LDS figures of every kernel's metadata, and with --meta prints those
figures for the kernels whose symbol matches REGEX.  Exit status 1 on any difference.

The files come from the same command on the two trees, e.g. in csrc/ with the Makefile's
HIPFLAGS:  hipcc $HIPFLAGS --cuda-device-only -S -o new_mid.s cfp_tp_mid.hip
"""
import argparse
import re
import sys

META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
             ".private_segment_fixed_size", ".group_segment_fixed_size")


# a trailing comment: white space, then ; to the end of the line (function bodies only: the label
# line "symbol: ; @symbol" is parsed as it stands; no operand of this output holds " ;")
TRAILING = re.compile(r"\s+;.*$")
ORDINAL = re.compile(r"\.(LBB|Lfunc_end)\d+")


def functions(path):
    """{symbol: [lines]} of every @function symbol, in file order."""
    funcs, types, cur = {}, set(), None
    with open(path) as f:
        for raw in f:
            line = TRAILING.sub("", raw).strip() if cur is not None else raw.strip()
            if not line or line.startswith(";"):
                continue
            line = ORDINAL.sub(r".\1", line)
            m = re.match(r"\.type\s+([^,\s]+),@function", line)
            if m:
                types.add(m.group(1))
                continue
            if cur is None:
                label = line.split(";")[0].strip()  # "symbol: ; @symbol"
                if label.endswith(":") and label[:-1] in types and label[:-1] not in funcs:
                    cur = label[:-1]
                    funcs[cur] = []
                continue
            if re.match(r"\.size\s+%s," % re.escape(cur), line):
                cur = None
                continue
            funcs[cur].append(line)
    return funcs


def metadata(path):
    """{kernel symbol: {key: value}} from the amdhsa.kernels metadata."""
    meta, cur = {}, None
    with open(path) as f:
        for raw in f:
            # a kernel's keys sit at the list's own indent ("  - .key:" opens an entry, "    .key:"
            # continues it); its arguments' keys are indented further
            m = re.match(r"(  - |    )(\.[a-z_]+):\s*(\S+)$", raw.rstrip())
            if not m:
                continue
            if m.group(1) == "  - ":
                cur = {}
            key, val = m.group(2), m.group(3)
            if cur is None:
                continue
            if key in META_KEYS:
                cur[key] = val
            elif key == ".name":
                meta[val] = cur
    return meta


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new", nargs="+")
    ap.add_argument("--meta", metavar="REGEX", help="print the metadata figures of the kernels matching REGEX")
    args = ap.parse_args()
    fo, fn, mn = functions(args.old), {}, {}
    bad = 0
    for path in args.new:
        f, m = functions(path), metadata(path)
        for name in sorted((set(f) & set(fn)) | (set(m) & set(mn))):
            print("DUPLICATE  %s  also in %s" % (name, path))
            bad += 1
        fn.update(f)
        mn.update(m)
    new_names = " ".join(args.new)
    for name in list(fo) + [n for n in fn if n not in fo]:
        if name not in fn or name not in fo:
            print("only in %s  %s" % (args.old if name in fo else new_names, name))
            bad += 1
            continue
        a, b = fo[name], fn[name]
        k = next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), None)
        if k is None and len(a) == len(b):
            print("same  %5d lines  %s" % (len(a), name))
            continue
        bad += 1
        k = min(len(a), len(b)) if k is None else k
        print("DIFF  %d / %d lines  %s" % (len(a), len(b), name))
        print("  line %d: %s" % (k + 1, a[k] if k < len(a) else "<end>"))
        print("  line %d: %s" % (k + 1, b[k] if k < len(b) else "<end>"))
    mo = metadata(args.old)
    mbad = 0
    for name in list(mo) + [n for n in mn if n not in mo]:
        if mo.get(name) != mn.get(name):
            print("METADATA DIFF  %s\n  %s\n  %s" % (name, mo.get(name), mn.get(name)))
            mbad += 1
        if args.meta and re.search(args.meta, name):
            print("meta  %s  %s" % (name, " ".join("%s %s" % (k, v) for k, v in sorted(mn.get(name, {}).items()))))
    print("%d functions, %d differ; %d kernels' metadata, %d differ" % (len(set(fo) | set(fn)), bad, len(set(mo) | set(mn)), mbad))
    return 1 if bad or mbad else 0


if __name__ == "__main__":
    sys.exit(main())

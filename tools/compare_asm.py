#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    python tools/compare_asm.py OLD.s NEW.s [--map MAPFILE]

Prints one markdown table row per kernel of NEW: the kernel of OLD it is compared with, both instruction
counts, both next_free_vgpr, NEW's scratch bytes and a verdict: `identical` (the same instruction text
once comments, directives and label numbers are stripped), `same opcodes` (the same opcodes in the same
order, operands differ), `reordered` (the same opcodes, in another order) or `differs`.  A kernel of NEW
is compared with the kernel of OLD of the same demangled name unless MAPFILE renames it: lines
`new_name<*, tail> = old_name`, where `tail` is the last template arguments of the new kernel, which the
old one does not have (`nt_update_kernel<*, false, true> = some_kernel` compares nt_update_kernel<K, S,
false, true> with some_kernel<K, S>).  Exit status 1 if a kernel of NEW has no partner.
"""
import argparse
import collections
import re
import subprocess
import sys


def kernels(path):
    """{demangled name<args>: (instructions, next_free_vgpr, scratch bytes)}"""
    text, meta, cur = {}, {}, None
    for line in open(path):
        s = line.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel (\S+)", s)
        if m:
            cur = ("meta", m.group(1))
            meta[m.group(1)] = {}
        elif s == ".end_amdhsa_kernel":
            cur = None
        elif cur and cur[0] == "meta":
            k, _, v = s.partition(" ")
            meta[cur[1]][k] = v
        elif re.match(r"\.Lfunc_end\d+:", s):
            cur = None
        elif re.match(r"[A-Za-z_][\w$.]*:$", s) and not s.startswith(".L"):
            cur = ("text", s[:-1])
            text[cur[1]] = []
        elif cur and s and not s.startswith(".") and not s.endswith(":"):
            text[cur[1]].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    names = [n for n in text if n in meta]
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, d in zip(names, plain):
        d = re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "")
        d = d[: d.index(">(") + 1] if ">(" in d else d.split("(")[0]
        out[d] = (text[n], int(meta[n][".amdhsa_next_free_vgpr"]), int(meta[n][".amdhsa_private_segment_fixed_size"]))
    return out


def partner(name, renames):
    base, _, args = name.partition("<")
    args = [a.strip() for a in args.rstrip(">").split(",")] if args else []
    for new_base, tail, old_base in renames:
        if base == new_base and args[len(args) - len(tail):] == tail:
            return "%s<%s>" % (old_base, ", ".join(args[: len(args) - len(tail)]))
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map")
    a = ap.parse_args()
    renames = []
    for line in open(a.map) if a.map else []:
        m = re.match(r"\s*(\w+)<\*((?:,\s*\w+)*)>\s*=\s*(\w+)\s*$", line)
        if m:
            renames.append((m.group(1), [t.strip() for t in m.group(2).split(",")[1:]], m.group(3)))
    old, new = kernels(a.old), kernels(a.new)
    print("| parent kernel | kernel | instructions | next_free_vgpr | scratch | text |")
    print("|---|---|---|---|---|---|")
    missing = 0
    for name, (t1, v1, s1) in new.items():
        p = partner(name, renames)
        if p not in old:
            print("| - | `%s` | - / %d | - / %d | %d | no partner |" % (name, len(t1), v1, s1))
            missing += 1
            continue
        t0, v0, _ = old[p]
        op0, op1 = [x.split()[0] for x in t0], [x.split()[0] for x in t1]
        verdict = ("identical" if t0 == t1 else "same opcodes" if op0 == op1 else
                   "reordered" if collections.Counter(op0) == collections.Counter(op1) else "differs")
        print("| `%s` | `%s` | %d / %d (%+.2f %%) | %d / %d | %d | %s |"
              % (p, name, len(t0), len(t1), 100.0 * (len(t1) - len(t0)) / len(t0), v0, v1, s1, verdict))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())

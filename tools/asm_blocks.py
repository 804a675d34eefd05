#!/usr/bin/env python3
"""Per-basic-block instruction counts of env_rollout_kernel from its assembly (make asm):
python3 tools/asm_blocks.py /tmp/env_rollout.s [min_valu] [--kernel NAME]
(the first env_rollout_kernel instantiation of the file unless --kernel names another by a piece of its
mangled name: env_rollout_kernelILi1ELb0E is <kAddrMfma, narrow>, the benchmark's; ILi1ELb1E <kAddrMfma, wide>;
ILi0ELb0E / ILi0ELb1E the VALU-address pair)

One line per block: label, VALU, of which v_cndmask, LDS reads, scratch_* instructions,
v_readlane / v_writelane, s_waitcnt lgkmcnt, and the branch targets, so the inner loop's header, its two
pair variants, the masked reset blocks and the tail can be read off and summed.

python3 tools/asm_blocks.py /tmp/env_rollout.s path <label,label,...> sums a path of blocks by
instruction class (the per-pair tables of profiles/r13a and r14a).
"""
import re
import sys


def blocks(path, kernel="env_rollout_kernel"):
    out, cur, inside = [], None, False
    for line in open(path):
        t = line.strip()
        if not inside:
            if re.match(r"^_Z\w*%s\w*:" % kernel, t):
                inside = True
                cur = {"label": "entry", "ins": []}
                out.append(cur)
            continue
        if t.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            cur = {"label": m.group(1), "ins": []}
            out.append(cur)
            continue
        if not t or t.startswith((";", ".", "//")):
            continue
        cur["ins"].append(t.split(";")[0].strip())
        if t.startswith("s_cbranch"):  # the fall-through of a conditional branch is a block of its own
            base, _, k = cur["label"].partition("+")
            cur = {"label": "%s+%d" % (base, int(k or 0) + 1), "ins": []}
            out.append(cur)
    return out


def path_totals(path, labels, kernel="env_rollout_kernel"):
    """The per-pair table of profiles/r13a and r14a: totals by instruction class over the blocks `labels`
    (comma list, in execution order), e.g. the fast pair's no-ending path
    .LBB0_37,.LBB0_55,.LBB0_55+1,.LBB0_58,.LBB0_60,.LBB0_61,.LBB0_61+1"""
    bl = {b["label"]: b for b in blocks(path, kernel)}
    ins = [i for l in labels.split(",") for i in bl[l]["ins"]]
    op = [i.split()[0] for i in ins]
    lane = ("v_readlane", "v_writelane", "v_readfirstlane")
    n = lambda *p: sum(o.startswith(p) for o in op)
    nop, wait = sum(o == "s_nop" for o in op), sum(o == "s_waitcnt" for o in op)
    vcc = sum(o.startswith("v_cndmask") and i.rstrip().endswith("vcc") for o, i in zip(op, ins))
    print(f"all {len(ins)}  VALU {n('v_') - n(*lane)}  scalar {n('s_') - nop - wait}  s_nop {nop}  waits {wait}  "
          f"v_cndmask {n('v_cndmask')} ({vcc} VCC / {n('v_cndmask') - vcc} SGPR pair)  v_cmp {n('v_cmp')}  v_perm {n('v_perm_b32')}  "
          f"v_bitop3 {n('v_bitop3')}  LDS {n('ds_')}  stores {n('global_store')}  scratch {n('scratch_')}  lane {n(*lane)}")


def main():
    kernel = "env_rollout_kernel"
    if "--kernel" in sys.argv:
        k = sys.argv.index("--kernel")
        kernel = sys.argv[k + 1]
        del sys.argv[k:k + 2]
    if len(sys.argv) > 3 and sys.argv[2] == "path":
        return path_totals(sys.argv[1], sys.argv[3], kernel)
    path = sys.argv[1]
    min_valu = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    print(f"{'block':<12}{'ins':>6}{'valu':>6}{'cnd':>5}{'lds_rd':>7}{'scr':>5}{'lane':>5}{'lgkm':>5}  branches")
    for b in blocks(path, kernel):
        ins = b["ins"]
        op = [i.split()[0] for i in ins]
        valu = sum(o.startswith("v_") and not o.startswith(("v_readlane", "v_writelane", "v_readfirstlane")) for o in op)
        cnd = sum(o.startswith("v_cndmask") for o in op)
        lds = sum(o.startswith("ds_read") or o.startswith("ds_load") for o in op)
        scr = sum(o.startswith("scratch_") for o in op)
        lane = sum(o.startswith(("v_readlane", "v_writelane")) for o in op)
        lgkm = sum(o == "s_waitcnt" and "lgkmcnt" in i for o, i in zip(op, ins))
        br = [i.split()[0][2:] + "->" + i.split()[-1] for i in ins if i.startswith(("s_cbranch", "s_branch"))]
        if valu >= min_valu:
            print(f"{b['label']:<12}{len(ins):>6}{valu:>6}{cnd:>5}{lds:>7}{scr:>5}{lane:>5}{lgkm:>5}  {' '.join(br)}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Diagnostics (not product): per-loop instruction counts of one kernel in a gfx950 assembly listing
(tools/isa_stats.py --keep out.s writes one).

    python tools/isa_loops.py out.s rollout_async_kernel [--min 200]

A loop is the span from a label to the last backward branch to it; the outermost spans of at least --min
instructions are listed in order (for rollout_async_kernel: the search waves' for (;;) and the env waves'
while).  Blocks that the compiler placed behind a loop's back edge and that jump back into it (rare paths) are
counted with the loop: a span grows over every later block that branches into it.  Per span: instructions,
VALU, SALU, scalar loads, s_waitcnt with an lgkmcnt field (and how many of them wait for 0), lane spills
(v_readlane / v_writelane), 64-bit right shifts, and the select_bit copies: runs of four v_bfe_u32 of variable
width at offset 0, each followed by v_bcnt_u32_b32 (level 16's width is a constant and compiles to an AND), with
the VALU count from the low half's popcount to the final OR.
"""
import re
import sys


def kernel_body(path, name):
    out, on = [], False
    for ln in open(path):
        m = re.match(r"^(_Z\S+):", ln)
        if m:
            on = name in m.group(1)
            continue
        if ln.startswith(".Lfunc_end"):
            on = False
        if on:
            out.append(ln.rstrip("\n"))
    return out


def main():
    path, name = sys.argv[1], sys.argv[2]
    lo_min = int(sys.argv[sys.argv.index("--min") + 1]) if "--min" in sys.argv else 200
    ins, labels = [], {}  # instructions as (mnemonic, operands); label -> index of the next instruction
    for ln in kernel_body(path, name):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        s = ln.split(";")[0].strip()
        if s and re.match(r"^[a-z]", s) and not s.startswith("."):
            p = s.split(None, 1)
            ins.append((p[0], p[1] if len(p) > 1 else ""))
    spans = []
    for i, (op, args) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            t = labels.get(args.strip())
            if t is not None and t <= i:
                spans.append([t, i])
    spans.sort()
    top = []
    for a, b in spans:  # outermost: merge nested and overlapping spans
        if top and a <= top[-1][1]:
            top[-1][1] = max(top[-1][1], b)
        else:
            top.append([a, b])
    grown = True
    while grown:  # later blocks that branch back into a span belong to it
        grown = False
        for sp in top:
            for i in range(sp[1] + 1, len(ins)):
                op, args = ins[i]
                t = labels.get(args.strip()) if op.startswith("s_cbranch") or op == "s_branch" else None
                if t is not None and sp[0] <= t <= sp[1] and not any(o is not sp and o[0] <= i <= o[1] for o in top):
                    sp[1] = i
                    grown = True
    merged = []
    for a, b in sorted(top):
        if merged and a <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    print(f"{name}: {len(ins)} instructions")
    for a, b in merged:
        body = ins[a:b + 1]
        if len(body) < lo_min:
            continue
        ops = [o for o, _ in body]
        waits = [x for o, x in body if o == "s_waitcnt" and "lgkmcnt" in x]
        print(f"loop [{a}, {b}] insts {len(body)} valu {sum(o.startswith('v_') for o in ops)} "
              f"salu {sum(o.startswith('s_') for o in ops)} "
              f"s_load {sum(o.startswith('s_load_') or o.startswith('s_buffer_load_') for o in ops)} "
              f"lgkmcnt_waits {len(waits)} (to 0: {sum('lgkmcnt(0)' in x for x in waits)}) "
              f"readlane {ops.count('v_readlane_b32')} writelane {ops.count('v_writelane_b32')} "
              f"lshr64 {ops.count('v_lshrrev_b64')} bfe {ops.count('v_bfe_u32')} bcnt {ops.count('v_bcnt_u32_b32')}")
        # select_bit copies: the levels 8, 4, 2, 1 are extracts of a variable width at offset 0 (level 16's width
        # is a constant and compiles to an AND with 0xffff), each followed by its popcount
        var = [i for i in range(len(body) - 1)
               if ops[i] == "v_bfe_u32" and re.search(r", 0, v\d+$", body[i][1]) and "v_bcnt_u32_b32" in ops[i + 1:i + 4]]
        k, copies = 0, []
        while k + 3 < len(var):
            if var[k + 3] - var[k] > 60:
                k += 1
                continue
            start, seen = var[k], 0
            while start > 0 and seen < 2:  # back over level 16's popcount to the low half's
                start -= 1
                seen += ops[start] == "v_bcnt_u32_b32"
            end = var[k + 3]
            while end + 1 < len(body) and not ops[end].startswith("v_cndmask"):
                end += 1
            end += 1  # the OR with the half's 32
            copies.append(sum(o.startswith("v_") for o in ops[start:end + 1]))
            k += 4
        print(f"  select_bit copies {len(copies)}; VALU from the low half's popcount to the final OR, other "
              f"chains' instructions scheduled in between included: {copies}")


if __name__ == "__main__":
    main()

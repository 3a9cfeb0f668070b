#!/usr/bin/env python3
"""Diagnostics (not product): compile a csrc/*.hip file to gfx950 assembly with the
library's own flags (runtime/build.py HIPCC_FLAGS) and report, per kernel,
registers, LDS, scratch and the instruction mix
(tools/isa_stats.py [file.hip] [-D...] [--keep out.s] | --asm file.s)."""
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "block-blast-ai---reinforcement-learning-agent_amd")
CSRC = os.path.join(PKG, "csrc")
sys.path.insert(0, PKG)


def main():
    src = os.path.join(CSRC, "bb_env.hip")
    defs = []
    out = asm = None
    args = sys.argv[1:]
    while args:
        a = args.pop(0)
        if a.startswith("-D"):
            defs.append(a)
        elif a == "--keep":  # write the assembly here
            out = args.pop(0)
        elif a == "--asm":  # read this assembly instead of compiling
            asm = args.pop(0)
        else:
            src = a if os.path.isabs(a) else os.path.join(CSRC, a)
    if asm is None:
        from runtime.build import HIPCC_FLAGS

        asm = out or os.path.join(tempfile.mkdtemp(), "k.s")
        flags = [f for f in HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
        subprocess.run(["/opt/rocm/bin/hipcc", *flags, f"-I{os.path.join(REPO, 'include')}", "--cuda-device-only", "-S",
                        *defs, "-o", asm, src], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read().splitlines()
    kern = None
    body = collections.defaultdict(list)
    meta = {}
    for ln in text:
        m = re.match(r"^\s+\.amdhsa_kernel (_Z\S+)", ln)
        if m:
            kd = m.group(1)
        m = re.match(r"^\s+\.amdhsa_group_segment_fixed_size (\d+)", ln)
        if m:
            meta.setdefault(kd, {})["lds"] = int(m.group(1))
        m = re.match(r"^(_Z\S+):", ln)
        if m:
            kern = m.group(1)
            continue
        if ln.startswith("\t.size") or ln.startswith(".Lfunc_end"):
            kern = None
        if kern and re.match(r"^\s+[a-z]", ln) and not ln.strip().startswith("."):
            body[kern].append(ln.split()[0])
        m = re.match(r"^\s+\.set (_Z\S+)\.(num_vgpr|numbered_sgpr|private_seg_size), (\d+)", ln)
        if m:
            meta.setdefault(m.group(1), {})[m.group(2)] = int(m.group(3))
    for k, ins in body.items():
        name = re.sub(r"^_ZN2bb\d+", "", k)[:40]
        c = collections.Counter(ins)
        md = meta.get(k, {})
        print(f"{name:40s} vgpr {md.get('num_vgpr')} sgpr {md.get('numbered_sgpr')} lds {md.get('lds')} scratch {md.get('private_seg_size')} "
              f"insts {len(ins)} valu {sum(v for x, v in c.items() if x.startswith('v_'))} "
              f"salu {sum(v for x, v in c.items() if x.startswith('s_'))} "
              f"scratch_ops {sum(v for x, v in c.items() if x.startswith('scratch_'))} "
              f"readlane {c['v_readlane_b32']} writelane {c['v_writelane_b32']}")


if __name__ == "__main__":
    main()

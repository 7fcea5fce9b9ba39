"""Static instruction-class counts of the kernels in a gfx950 assembly listing.

  hipcc <the Makefile's flags for the TU> --cuda-device-only -S rtg_solve_fbp_soa.hip -o soa.s
  python tools/static_mix.py soa.s [kernel-name substring ...]

Per kernel (a global function symbol with an .amdhsa_kernel record): VALU instructions, of them packed f32
(v_pk_{mul,add,fma}_f32), register-to-register v_mov_b32, v_cndmask, f64 ops, and the s_nop count.  `issue_slots`
counts a packed op twice: a packed f32 op issues at the rate of the two plain ops it replaces, and SQ_INSTS_VALU
counts it once.  Static counts: every instruction once, whatever its trip count.

  python tools/static_mix.py --loops soa.s [kernel-name substring ...]

Per loop of a kernel instead: a loop is the stretch of the listing from a label to the last branch back to it (a back
edge); stretches that overlap without nesting are merged (one loop with several back edges), and an inner loop's
instructions count in its outer loops too.  For each: the header label, first and last
instruction index within the kernel, and VALU, v_mov_b32, v_cmp*, v_cndmask, transcendentals (v_rcp / v_rsq / v_sqrt /
v_exp / v_log / v_sin / v_cos) and s_*_saveexec in that stretch.  Loops of fewer than `--min-valu N` (default 40)
VALU are left out.
"""
from __future__ import annotations

import json
import re
import sys


def kernels(path):
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(\w+):", line)
        if m:
            cur = m.group(1) if m.group(1) in names else (cur if not line.startswith("_Z") else None)
            if cur is not None and cur not in out:
                out[cur] = []
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith("\t.section"):
            continue
        if cur is not None:
            op = line.strip().split(" ", 1)[0].split("\t", 1)[0]
            if re.match(r"^[vs]_|^(ds|global|buffer|flat|scratch)_", op):
                out[cur].append(line.strip())
    return out


def classify(insts):
    valu = [i for i in insts if i.startswith("v_")]
    op = lambda i: i.split()[0]
    pk = [i for i in valu if re.match(r"v_pk_(mul|add|fma)_f32", op(i))]
    mov = [i for i in valu if op(i).startswith("v_mov_b32")]
    mov_rr = [i for i in mov if re.match(r"v_mov_b32(_e32)?\s+v\d+,\s*v\d+\s*$", i)]
    return {"valu": len(valu), "packed_f32": len(pk), "v_mov_b32": len(mov), "v_mov_b32_reg_reg": len(mov_rr),
            "v_cndmask": sum(op(i).startswith("v_cndmask") for i in valu),
            "f64": sum("_f64" in op(i) for i in valu),
            # one v_div_fixup_f32 per inlined IEEE f32 division (11 VALU each), one v_sqrt_f32 per inlined cr_sqrt /
            # cr_sqrt_nt (14 / 9 VALU), v_rcp_f32: the divisions' plus one per shared-reciprocal group (fdiv_n)
            "ieee_div_f32": sum(op(i).startswith("v_div_fixup_f32") for i in valu),
            "v_rcp_f32": sum(op(i).startswith("v_rcp_f32") for i in valu),
            "v_sqrt_f32": sum(op(i).startswith("v_sqrt_f32") for i in valu), "s_nop": sum(op(i) == "s_nop" for i in insts),
            "ds": sum(op(i).startswith("ds_") for i in insts), "global": sum(op(i).startswith("global_") for i in insts),
            "plain": len(valu) - len(pk), "issue_slots": len(valu) + len(pk)}


TRANS = re.compile(r"v_(rcp|rsq|sqrt|exp|log|sin|cos)_")


def loops(path):
    """kernel -> [(header label, first index, last index, instructions)] for every back-edge stretch."""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur, insts, labels, edges = {}, None, [], {}, {}

    def close():
        if cur is None:
            return
        iv = sorted((a, b, lab) for lab, (a, b) in edges.items())
        merged = True
        while merged:   # stretches that overlap without nesting are one loop with several back edges: their union
            merged = False
            for i in range(len(iv)):
                for j in range(i + 1, len(iv)):
                    (a, b, la), (c, d, _) = iv[i], iv[j]
                    if a < c <= b < d or (a, b) == (c, d):
                        iv[i] = (a, max(b, d), la)
                        del iv[j]
                        merged = True
                        break
                if merged:
                    break
            iv.sort()
        out[cur] = [(lab, a, b, insts[a:b + 1]) for a, b, lab in iv]

    for line in text.splitlines():
        m = re.match(r"^([\w.$]+):", line)
        if m and not m.group(1).startswith(".L"):
            close()
            cur = m.group(1) if m.group(1) in names else None
            insts, labels, edges = [], {}, {}
            continue
        if cur is None:
            continue
        if m:
            labels[m.group(1)] = len(insts)
            continue
        t = line.strip()
        if re.match(r"^[vs]_|^(ds|global|buffer|flat|scratch)_", t):
            b = re.match(r"^s_c?branch\w*\s+(\.L\S+)", t)
            if b and b.group(1) in labels:   # a branch to a label already seen: a back edge
                a = labels[b.group(1)]
                edges[b.group(1)] = (a, max(len(insts), edges.get(b.group(1), (a, 0))[1]))
            insts.append(t)
    close()
    return out


def loop_report(path, want, min_valu):
    op = lambda i: i.split()[0]
    for name, ls in loops(path).items():
        if want and not any(w in name for w in want):
            continue
        for lab, a, b, insts in ls:
            valu = [i for i in insts if i.startswith("v_")]
            if len(valu) < min_valu:
                continue
            print(json.dumps({"kernel": name, "loop": lab, "first": a, "last": b, "valu": len(valu),
                              "v_mov_b32": sum(op(i).startswith("v_mov_b32") for i in valu),
                              "v_cmp": sum(op(i).startswith("v_cmp") for i in valu),
                              "v_cndmask": sum(op(i).startswith("v_cndmask") for i in valu),
                              "trans": sum(bool(TRANS.match(op(i))) for i in valu),
                              "saveexec": sum(bool(re.match(r"s_\w+_saveexec", op(i))) for i in insts)}))


def main():
    if "--loops" in sys.argv:
        args = [a for a in sys.argv[1:] if a != "--loops"]
        min_valu = 40
        if "--min-valu" in args:
            i = args.index("--min-valu")
            min_valu = int(args[i + 1])
            del args[i:i + 2]
        loop_report(args[0], args[1:], min_valu)
        return
    ks = kernels(sys.argv[1])
    want = sys.argv[2:]
    for name, insts in ks.items():
        if want and not any(w in name for w in want):
            continue
        print(json.dumps({"kernel": name, **classify(insts)}))


if __name__ == "__main__":
    main()

"""Static instruction-class counts of the kernels in a gfx950 assembly listing.

  hipcc <the Makefile's flags for the TU> --cuda-device-only -S rtg_solve_fbp_soa.hip -o soa.s
  python tools/static_mix.py soa.s [kernel-name substring ...]

Per kernel (a global function symbol with an .amdhsa_kernel record): VALU instructions, of them packed f32
(v_pk_{mul,add,fma}_f32), register-to-register v_mov_b32, v_cndmask, f64 ops, and the s_nop count.  `issue_slots`
counts a packed op twice: a packed f32 op issues at the rate of the two plain ops it replaces, and SQ_INSTS_VALU
counts it once.  Static counts: every instruction once, whatever its trip count.
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


def main():
    ks = kernels(sys.argv[1])
    want = sys.argv[2:]
    for name, insts in ks.items():
        if want and not any(w in name for w in want):
            continue
        print(json.dumps({"kernel": name, **classify(insts)}))


if __name__ == "__main__":
    main()

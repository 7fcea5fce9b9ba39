"""A/B of the lane-group kernels (rtg_fk.hip, rtg_fk_grad.hip, rtg_dof_fit.hip, rtg_retarget_to.hip) across library
builds, interleaved like tools/ab_small.py: each build runs in its own process (RTG_LIB).

Bits: every output of the lane-group entry points on fixed seeded inputs at small ragged shapes (B = F + 1 for both
tile shapes, F = 16 and 8) is hashed per case, and every hash must equal the first build's -- also where no oracle pins
the bits (the gradient and fit kernels are built with -ffp-contract=fast and their tests only bound the error).
Time: device events at B = 262144 on the shapes of tools/extra_bench.py's modes fk, retarget_to, fit and pose_fit.  A
base build from before an entry point existed is served: the cases and times it cannot give are left out.  A build passes
when each of its medians is at most the first build's median plus the first build's own max - min over its rounds.

  python tools/ab_groups.py base=.../variants/parent.so new=humanoid-real-time-retarget_amd/librtg_hip.so [--rounds 4]
"""
from __future__ import annotations

import hashlib
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plan(tag):
    """the retarget_to fixture plan `tag` and its source / target joint counts (tools/extra_bench.py retarget_to)"""
    import numpy as np
    from rtg import assets
    from rtg.bridge import retarget_plan
    G = os.path.join(REPO, "tests", "golden")
    with open(os.path.join(G, "retarget_to_names.json")) as f:
        e = json.load(f)[tag]
    gold = np.load(os.path.join(G, "retarget_to.npz"))
    s, t = assets.load(e["source"]), assets.load(e["target"])
    Js, Jt = len(e["source_names"]), len(e["target_names"])
    sj = [e["source_names"].index(a) for a in e["mapping"]]
    tj = [e["target_names"].index(b) for b in e["mapping"].values()]
    sp, tp = s["parent_indices"].astype(np.int32), t["parent_indices"].astype(np.int32)
    tps, tps_t = s["tensor"][:Js * 4].reshape(Js, 4), s["tensor"][Js * 4:Js * 4 + 3]
    tpt, tpt_t = t["tensor"][:Jt * 4].reshape(Jt, 4), t["tensor"][Jt * 4:Jt * 4 + 3]
    plan = retarget_plan((sp, s["local_translation"], s["quat"]), (tp, t["local_translation"], t["quat"]), sj, tj, tps,
                         tps_t, tpt, tpt_t, gold[f"{tag}_R"], float(gold[f"{tag}_scale"].reshape(-1)[0]))
    return plan, Js, Jt


def child():
    import importlib
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import extra_bench as xb
    import ctypes
    from rtg import _lib, ops
    from rtg.runtime import DofModel, Topology, ptr, stream_handle
    older = ctypes.CDLL(_lib.LIB_PATH)   # a base build from before a symbol existed: its cases are left out
    for name in [n for n in _lib.SIGNATURES if not hasattr(older, n)]:
        del _lib.SIGNATURES[name]
    lib, check, sh = _lib.lib(), _lib.check, stream_handle()
    gen = torch.Generator(device="cuda").manual_seed(14)
    rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)
    unit = lambda *s: torch.nn.functional.normalize(rnd(*s), dim=-1)
    empty = lambda *s: torch.full(s, 7.0, device="cuda")
    hashes = {}

    def put(name, *outs):
        torch.cuda.synchronize()
        h = hashlib.sha1()
        for o in outs:
            h.update(o.cpu().numpy().tobytes())
        hashes[name] = h.hexdigest()[:16]

    # ---- bits: B = F + 1 (one whole tile and a one-frame tile) on a 16-frame and an 8-frame model
    hu = importlib.import_module("retarget.robot_config.Hu")
    rng = np.random.default_rng(37)
    par37 = np.array([-1] + [(j - 1) // 2 for j in range(1, 37)], np.int32)
    topos = {16: xb.topo("hu_v5"), 8: xb.topo("vtrdyn_full")}
    models = {16: DofModel(xb.topo("hu"), hu.Hu_DOF_AXIS, hu.Hu_DOF_LOWER.numpy(), hu.Hu_DOF_UPPER.numpy()),
              8: DofModel(Topology(par37, rng.normal(0, 0.3, (37, 3)).astype(np.float32)),
                          rng.integers(0, 3, 36).astype(np.int32), (-0.5 - rng.uniform(0, 1, 36)).astype(np.float32),
                          (0.5 + rng.uniform(0, 1, 36)).astype(np.float32))}
    J_of = {16: 33, 8: 37}
    segs = []
    for F in (16, 8):
        B, T = F + 1, topos[F]
        J = T.num_joints
        lr, rt = unit(B, J, 4), rnd(B, 3)
        segs.append((T, lr, rt))
        for state in (False, True):
            g, p = ops.forward_kinematics(T, lr, rt, state=state)
            put(f"fk_F{F}_state{int(state)}", g, p)
            put(f"local_rotation_F{F}_state{int(state)}", ops.local_rotation(T, g, state=state))
        g = ops.forward_kinematics(T, lr, rt)[0].contiguous()
        cr, cp = rnd(B, J, 4), rnd(B, J, 3)
        for rot in (cr, None):
            gl, grt = empty(B, J, 4), empty(B, 3)
            check(lib.rtg_fk_backward_f32(T.handle, ptr(lr), ptr(g), ptr(rot), ptr(cp), B, ptr(gl), ptr(grt), sh))
            put(f"fk_backward_F{F}_rot{int(rot is not None)}", gl, grt)
        M, J = models[F], J_of[F]
        dof, rr, rt = rnd(B, J - 1) * 2, unit(B, 4) * 1.5, rnd(B, 3)
        cr, cp = rnd(B, J, 4), rnd(B, J, 3)
        for clip in (0, 1):
            g, p = empty(B, J, 4), empty(B, J, 3)
            check(lib.rtg_dof_fk_f32(M.handle, ptr(dof), ptr(rr), ptr(rt), B, clip, ptr(g), ptr(p), sh))
            put(f"dof_fk_F{F}_clip{clip}", g, p)
            for rot in (cr, None):
                gd, grr, grt = empty(B, J - 1), empty(B, 4), empty(B, 3)
                check(lib.rtg_dof_fk_backward_f32(M.handle, ptr(dof), ptr(g), ptr(rot), ptr(cp), B, clip, ptr(gd),
                                                  ptr(grr), ptr(grt), sh))
                put(f"dof_fk_backward_F{F}_clip{clip}_rot{int(rot is not None)}", gd, grr, grt)
        tgt, w = rnd(B, J, 3) * 0.5, torch.rand(J, device="cuda", generator=gen)
        for iters in (0, 3):
            for state in (False, True):
                m, v = (torch.zeros(B, J - 1, device="cuda"), torch.zeros(B, J - 1, device="cuda")) if state else (None, None)
                out, loss, grad = empty(B, J - 1), empty(B), empty(B, J - 1)
                check(lib.rtg_dof_fit_f32(M.handle, ptr(tgt), ptr(w), ptr(rr), ptr(rt), ptr(dof), B, 1, iters, 0.02,
                                          0.9, 0.999, 1e-8, 0, ptr(m), ptr(v), ptr(out), ptr(loss), ptr(grad), sh))
                put(f"dof_fit_F{F}_iters{iters}_state{int(state)}", out, loss, grad, *([m, v] if state else []))
                if "rtg_dof_fit_root_f32" not in _lib.SIGNATURES:
                    continue
                for mask in (0, 3):
                    m, v, rs = (torch.zeros(B, n, device="cuda") for n in (J - 1, J - 1, 14)) if state else (None,) * 3
                    outs = [empty(B, J - 1), empty(B, 4), empty(B, 3), empty(B), empty(B, J - 1), empty(B, 7)]
                    check(lib.rtg_dof_fit_root_f32(M.handle, ptr(tgt), ptr(w), ptr(rr), ptr(rt), ptr(dof), B, 1, mask,
                                                   iters, 0.02, 0.01, 0.03, 0.9, 0.999, 1e-8, 0, ptr(m), ptr(v), ptr(rs),
                                                   *(ptr(o) for o in outs), sh))
                    put(f"pose_fit_F{F}_mask{mask}_iters{iters}_state{int(state)}", *outs, *([m, v, rs] if state else []))
    fk_out, inv_out = ops.kinematics_multi(segs, [(T, ops.forward_kinematics(T, lr, rt)[0]) for T, lr, rt in segs])
    put("kinematics_multi", *[x for pair in fk_out for x in pair], *inv_out)
    for tag in ("vtrdyn_hu_v5_local", "vtrdyn_full_hu"):
        plan, Js, Jt = _plan(tag)
        for B in (17, 9):
            rot, root = unit(B, Js, 4), rnd(B, 3)
            for local in (True, False):
                put(f"retarget_to_{tag}_B{B}_local{int(local)}", *ops.retarget_to(plan, rot, root, is_local=local))

    # ---- time: B = 262144
    B = 262144
    t = {k: v["ms"] * 1e3 for k, v in xb.fk().items() if k != "mixed_4x65536"}
    plan, Js, Jt = _plan("vtrdyn_hu_v5_local")
    rot, root = unit(B, Js, 4), rnd(B, 3)
    out_rot, out_root = torch.empty((B, Jt, 4), device="cuda"), torch.empty((B, 3), device="cuda")
    args = (plan.handle, ptr(rot), ptr(root), 1, B, ptr(out_rot), ptr(out_root), sh)
    check(lib.rtg_retarget_to_f32(*args))
    t["retarget_to_262144"] = xb.time_events(lambda: lib.rtg_retarget_to_f32(*args)) * 1e3
    M, tgt, rr, rt, start = xb._fit_setup(B)
    out, loss = torch.empty((B, 32), device="cuda"), torch.empty((B,), device="cuda")
    t["fit_32_iters_262144"] = xb.time_events(xb._fit_call(M, tgt, rr, rt, start, B, 32, out, loss, None), reps=10, warm=2) * 1e3
    if "rtg_dof_fit_root_f32" in _lib.SIGNATURES:
        outs = (out, torch.empty((B, 4), device="cuda"), torch.empty((B, 3), device="cuda"), loss, None, None)
        t["pose_fit_32_iters_262144"] = xb.time_events(xb._pose_fit_call(M, tgt, rr, rt, start, B, 32, 3, outs), reps=10,
                                                       warm=2) * 1e3
    print(json.dumps({"kernel_us": t, "hashes": hashes}))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = 4
    if "--rounds" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1])
        args = [a for a in args if a != str(rounds)]
    builds = [a.split("=", 1) for a in args]
    res = {n: [] for n, _ in builds}
    for _ in range(rounds):
        for name, lib in builds:
            env = dict(os.environ, RTG_LIB=os.path.abspath(lib), RTG_ALLOW_MEASUREMENT_BUILD="1")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                               text=True, timeout=300)
            if r.returncode != 0:
                print(json.dumps({"build": name, "returncode": r.returncode, "error": r.stderr[-1500:]}), flush=True)
                sys.exit(1)
            res[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps({"build": name, **res[name][-1]}), flush=True)
    base = res[builds[0][0]]
    ref = base[0]["hashes"]
    summary, ok = {}, True
    for name, runs in res.items():
        bad = sorted({k for r in runs for k in ref if r["hashes"].get(k) != ref[k]})
        us = {k: sorted(round(r["kernel_us"][k], 2) for r in runs) for k in runs[0]["kernel_us"]}
        slow = {}
        for k, v in us.items():
            if k not in base[0]["kernel_us"]:   # the base build has no such kernel
                continue
            b = sorted(r["kernel_us"][k] for r in base)
            bound = statistics.median(b) + (b[-1] - b[0])
            if statistics.median(v) > bound:
                slow[k] = {"median": statistics.median(v), "bound": round(bound, 2)}
        summary[name] = {"kernel_us": us, "hash_cases": len(ref), "hash_mismatches": bad, "slower_than_bound": slow}
        ok = ok and not bad and not slow
    print(json.dumps({"summary": summary, "pass": ok}), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()

"""A/B of the small-batch FULL_BODY_POS kernels (k_fbp_frame1 at B = 1, k_fbp_quad at 16 / 256 / 4096, k_fbp_latency5
at 8192 / 32768; precise gripper, AoS rows as the drop-in passes them) across library builds, interleaved like
tools/ab_headline.py: each build runs in its own process (RTG_LIB), kernel time by device events over 400 launches,
and the DOFs of every build are hashed and must match the first.

  python tools/ab_small.py base=.../variants/parent.so new=humanoid-real-time-retarget_amd/librtg_hip.so [--rounds 3]
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 16, 256, 4096, 8192, 32768)

CHILD = r"""
import hashlib, json, os, sys, numpy as np, torch
sys.path.insert(0, os.path.join(sys.argv[1], "humanoid-real-time-retarget_amd"))
from rtg import _lib, assets
from rtg.runtime import Solver
zp = np.load(os.path.join(sys.argv[1], "tests", "golden", "zero_pose.npz"))
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "full_body_pos_precise.npz"))
S = Solver(_lib.SOLVER_FULL_BODY_POS, zp["vtrdyn_full_local_t"], zp["vtrdyn_full_global_t"], assets.parents("vtrdyn_full"), True)
out, h = {}, hashlib.sha1()
for B in json.loads(sys.argv[2]):
    idx = np.arange(B) % len(g["body"])
    ins = [torch.from_numpy(np.ascontiguousarray(g[k][idx])).cuda() for k in ("body", "lh", "rh")]
    dof = torch.empty((B, 30), device="cuda")
    for _ in range(20):
        S.retarget(ins, out_dof=dof)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(400):
        S.retarget(ins, out_dof=dof)
    e1.record(); e1.synchronize()
    out[str(B)] = e0.elapsed_time(e1) / 400 * 1e3
    h.update(dof.cpu().numpy().tobytes())
out["dof_sha"] = h.hexdigest()[:16]
print(json.dumps(out))
"""


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = 3
    if "--rounds" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1])
        args = [a for a in args if a != str(rounds)]
    builds = [a.split("=", 1) for a in args]
    res = {n: [] for n, _ in builds}
    for _ in range(rounds):
        for name, lib in builds:
            env = dict(os.environ, RTG_LIB=os.path.abspath(lib), RTG_ALLOW_MEASUREMENT_BUILD="1")
            r = subprocess.run([sys.executable, "-c", CHILD, REPO, json.dumps(SIZES)], env=env, capture_output=True,
                               text=True, timeout=300)
            if r.returncode != 0:
                print(json.dumps({"build": name, "error": r.stderr[-1500:]}), flush=True)
                sys.exit(1)
            res[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps({"build": name, **res[name][-1]}), flush=True)
    ref = res[builds[0][0]][0]["dof_sha"]
    summary = {name: {"kernel_us": {str(B): sorted(round(r[str(B)], 3) for r in runs) for B in SIZES},
                      "bits_match_first_build": all(r["dof_sha"] == ref for r in runs)}
               for name, runs in res.items()}
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()

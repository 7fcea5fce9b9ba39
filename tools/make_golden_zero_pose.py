"""Generate ``tests/golden/zero_pose_transform.npz``: the reference's zero-pose transforms of mocap rotations.

Build-container only (it runs the reference under ``tools/refharness.py``, with the working directory at the reference
root: retarget/utils/parse_mocap.py opens its t-pose pickles relative to it).  ``retarget.utils.parse_mocap`` is
imported if it imports under the harness (pandas present, the viewers stubbed); otherwise the reference's own
``RobotZeroPose``, ``quat_from_angle_axis``, ``quat_mul_norm`` and ``quat_inverse`` are called in the order of its
lines 65-134, over the extracted assets.  ``meta_source`` says which of the two ran.

Recorded (tests/rot_ingest_frames.py builds the inputs):
  t2zero_vtrdyn (21,4), t2zero_vtrdyn_full (59,4)      the two *_t2zero_pose_transform_quat arrays
  pre_vtrdyn, pre_vtrdyn_full, pre_broadcast (4)       the axis rotation of each function
  unit_21 / unit_59 (64,J,4)                           unit frames
  family_21 / family_59 (144,J,4), family_names        8 frames of each of the 18 quaternion families
  broadcast_23 (64,23,4)                               raw broadcast rows
  out_<input>_<function>                               vtrdyn_zero_pose_transform and vtrdyn_broadcast_zero_pose_transform
                                                       on the 21-joint inputs (and on broadcast_23 gathered to 21 rows),
                                                       vtrdyn_full_zero_pose_transform on the 59-joint inputs
  out_broadcast_23_full_scatter (64,21,4)              sim_full_body_teleop.py:97-102 per frame: gathered to 21 rows,
                                                       scattered into an identity 59-joint pose, transformed, gathered
Data only; fixed zip timestamps, so a rerun reproduces the file byte for byte.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import refharness as rh  # noqa: E402
from make_golden_grad import save_npz  # noqa: E402

rh.load_rtg_module("synth")   # tests/other_solver_frames.py imports rtg lazily; loaded by location, never via sys.path

OUT = os.path.join(REPO, "tests", "golden", "zero_pose_transform.npz")


def _frames_module():
    path = list(sys.path)
    sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")]
    try:
        import rot_ingest_frames as rf
    finally:
        sys.path[:] = path   # tests/conftest.py puts the drop-in packages in front of the reference's
    return rf


def _from_parse_mocap():
    import retarget.utils.parse_mocap as pm
    return dict(vtrdyn=pm.vtrdyn_zero_pose_transform, vtrdyn_full=pm.vtrdyn_full_zero_pose_transform,
                broadcast=pm.vtrdyn_broadcast_zero_pose_transform,
                t2zero_vtrdyn=pm.vtrdyn_t2zero_pose_transform_quat,
                t2zero_vtrdyn_full=pm.vtrdyn_full_t2zero_pose_transform_quat)


def _from_primitives(ref, rf):
    """parse_mocap.py:65-134 spelled out with the reference's own functions over the extracted assets."""
    import torch
    r3 = ref.rotation3d
    t2zero = {}
    for asset in ("vtrdyn_full", "vtrdyn"):
        pose = rh.ref_zero_pose(ref, asset)
        lr = pose.local_rotation.clone()
        for j, angle, axis in rf.T2ZERO_EDITS[asset]:
            e = [0.0, 0.0, 0.0]
            e[axis] = 1.0
            lr[j] = r3.quat_from_angle_axis(torch.tensor(angle), torch.tensor(e))
        t2zero[asset] = pose.rebuild_pose_by_local_rotation(lr)

    def make(axis, t2z):
        def fn(global_rotation):
            rotation = r3.quat_from_angle_axis(torch.tensor(torch.pi / 2), torch.tensor(axis))
            out = r3.quat_mul_norm(global_rotation.clone(), rotation)
            return r3.quat_mul_norm(out, r3.quat_inverse(t2z))
        return fn
    return dict(vtrdyn=make([0., 0., 1.], t2zero["vtrdyn"]), vtrdyn_full=make([0., 0., 1.], t2zero["vtrdyn_full"]),
                broadcast=make([1., 0., 0.], t2zero["vtrdyn"]), t2zero_vtrdyn=t2zero["vtrdyn"],
                t2zero_vtrdyn_full=t2zero["vtrdyn_full"])


def main() -> None:
    import torch
    torch.set_num_threads(1)
    rf = _frames_module()
    ref = rh.load_reference()
    os.chdir(rh.REF)
    try:
        fns, source = _from_parse_mocap(), "retarget.utils.parse_mocap"
    except Exception as e:   # the import needs pandas and unpickles the reference's t-poses
        print(f"retarget.utils.parse_mocap does not import under the harness ({type(e).__name__}: {e}); "
              "composing lines 65-134 from the reference's primitives")
        fns, source = _from_primitives(ref, rf), "primitives"
    r3 = ref.rotation3d

    def run(fn, q):
        return fn(torch.from_numpy(q)).numpy().astype(np.float32).copy()

    out = {"meta_source": np.asarray(source), "family_names": np.asarray(rf.FAMILY_NAMES),
           "t2zero_vtrdyn": fns["t2zero_vtrdyn"].numpy().copy(),
           "t2zero_vtrdyn_full": fns["t2zero_vtrdyn_full"].numpy().copy()}
    half_pi = torch.tensor(torch.pi / 2)
    out["pre_vtrdyn"] = r3.quat_from_angle_axis(half_pi, torch.tensor([0., 0., 1])).numpy().copy()
    out["pre_vtrdyn_full"] = r3.quat_from_angle_axis(half_pi, torch.tensor([0., 0., 1])).numpy().copy()
    out["pre_broadcast"] = r3.quat_from_angle_axis(half_pi, torch.tensor([1., 0., 0])).numpy().copy()
    ins = {"unit_21": rf.unit_frames(64, 21), "unit_59": rf.unit_frames(64, 59), "family_21": rf.family_frames(21),
           "family_59": rf.family_frames(59), "broadcast_23": rf.broadcast_frames(64)}
    out.update(ins)
    with np.errstate(all="ignore"):
        for tag in ("unit_21", "family_21"):
            out[f"out_{tag}_vtrdyn"] = run(fns["vtrdyn"], ins[tag])
            out[f"out_{tag}_broadcast"] = run(fns["broadcast"], ins[tag])
        for tag in ("unit_59", "family_59"):
            out[f"out_{tag}_vtrdyn_full"] = run(fns["vtrdyn_full"], ins[tag])
        b21 = np.ascontiguousarray(ins["broadcast_23"][:, rf.BODY23_TO_21])
        out["out_broadcast_23_vtrdyn"] = run(fns["vtrdyn"], b21)
        out["out_broadcast_23_broadcast"] = run(fns["broadcast"], b21)
        rows = []
        for f in range(len(b21)):   # sim_full_body_teleop.py:97-102, frame by frame as the loop does
            body_quat = torch.from_numpy(ins["broadcast_23"][f])[rf.BODY23_TO_21]
            full = r3.quat_identity([59, ])
            full[rf.BODY21_IN_FULL59] = body_quat
            full = fns["vtrdyn_full"](full)
            rows.append(full[rf.BODY21_IN_FULL59].numpy().reshape(21, 4).astype(np.float32).copy())
        out["out_broadcast_23_full_scatter"] = np.stack(rows)
    save_npz(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays; source: {source})")


if __name__ == "__main__":
    main()

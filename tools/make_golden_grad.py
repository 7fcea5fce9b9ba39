"""Generate ``tests/golden/fk_grad.npz``: the reference's kinematics under autograd.

Build-container only (it imports the reference through ``tools/refharness.py``).  The reference's own
``quat_from_angle_axis`` + ``cal_forward_kinematics`` (plain torch, differentiable) are run in float32 and in
float64 on the same float32 inputs, and a loss ``sum(cot_rot * g_rot) + sum(cot_pos * g_pos)`` with random
cotangents is back-propagated.  Three cases of 64 frames:

  hu_v5_noclip   HuForwardModel semantics on the 31-link Hu v5, no clipping        (tests/golden/dof_fk.npz's case)
  hu_clip        the same on the 33-link Hu with the straight-through clip         (tests/golden/dof_fk.npz's case)
  vtrdyn_full    plain cal_forward_kinematics on the 59-joint VTRDyn skeleton, local rotations not unit

Angles are uniform in +-3 pi (so quat_from_angle_axis's w < 0 flip occurs, and the clipped case sits well outside
its limits), root quaternions have norm 0.5-2 (the root is taken unnormalised).  Per case the file holds the inputs,
the topology, the two cotangents, the float32 forward outputs and every gradient in float32 and float64.  Data only;
written with fixed zip timestamps, so a rerun reproduces the file byte for byte.
"""
from __future__ import annotations

import importlib
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import refharness as rh  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "fk_grad.npz")
N = 64


def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            with z.open(zi, "w") as f:
                np.lib.format.write_array(f, np.ascontiguousarray(v), allow_pickle=False)


def scaled_quats(rng, shape):
    q = rng.normal(size=shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return (q * rng.uniform(0.5, 2.0, shape + (1,))).astype(np.float32)


def n32(t):
    return t.detach().numpy().astype(np.float32).copy()


def n64(t):
    return t.detach().numpy().astype(np.float64).copy()


def dof_case(ref, torch, out, tag, name, mod, clip, seed):
    cfg = importlib.import_module(mod)
    tree = rh.ref_skeleton_state(ref, name).skeleton_tree
    J = tree.num_joints
    rng = np.random.default_rng(seed)
    dof = rng.uniform(-3 * np.pi, 3 * np.pi, (N, J - 1)).astype(np.float32)
    root_rot = scaled_quats(rng, (N,))
    root_t = rng.normal(0, 0.3, (N, 3)).astype(np.float32)
    cot_rot = rng.normal(size=(N, J, 4)).astype(np.float32)
    cot_pos = rng.normal(size=(N, J, 3)).astype(np.float32)
    out[f"{tag}_parents"] = np.asarray(tree.parent_indices, np.int32)
    out[f"{tag}_local_t"] = n32(tree.local_translation)
    out[f"{tag}_axis"] = np.asarray(cfg.Hu_DOF_AXIS, np.int32)
    if clip:
        out[f"{tag}_lower"] = n32(cfg.Hu_DOF_LOWER)
        out[f"{tag}_upper"] = n32(cfg.Hu_DOF_UPPER)
    for k, v in (("dof", dof), ("root_rot", root_rot), ("root_t", root_t), ("cot_rot", cot_rot), ("cot_pos", cot_pos)):
        out[f"{tag}_{k}"] = v
    for dt, sfx in ((torch.float32, "f32"), (torch.float64, "f64")):
        a = torch.from_numpy(dof).to(dt).reshape(N, J - 1, 1).requires_grad_(True)
        rr = torch.from_numpy(root_rot).to(dt).reshape(N, 1, 4).requires_grad_(True)
        rt = torch.from_numpy(root_t).to(dt).requires_grad_(True)
        x = a
        if clip:   # HuForwardModel._clip_angles, hu_forward_model.py:27-33
            lo = cfg.Hu_DOF_LOWER.to(dt).reshape(1, -1, 1)
            hi = cfg.Hu_DOF_UPPER.to(dt).reshape(1, -1, 1)
            c = torch.clamp(x.clone(), min=lo, max=hi)
            x = (c - x).detach() + x
        axis = torch.eye(3, dtype=dt)[cfg.Hu_DOF_AXIS].repeat(N, 1, 1).clone()          # :16, :21
        lr = ref.rotation3d.quat_from_angle_axis(x.reshape(-1), axis.reshape(-1, 3))      # :22
        lr = torch.concatenate([rr, lr.reshape(N, J - 1, 4)], dim=1)                      # :23-24
        gr, gp = ref.rkm.cal_forward_kinematics(motion_local_rotation=lr, motion_root_translation=rt,
                                                parent_indices=tree.parent_indices,
                                                zero_pose_local_translation=tree.local_translation.to(dt))
        loss = (gr * torch.from_numpy(cot_rot).to(dt)).sum() + (gp * torch.from_numpy(cot_pos).to(dt)).sum()
        loss.backward()
        conv = n32 if dt == torch.float32 else n64
        out[f"{tag}_grad_dof_{sfx}"] = conv(a.grad)[..., 0]
        out[f"{tag}_grad_root_rot_{sfx}"] = conv(rr.grad)[:, 0]
        out[f"{tag}_grad_root_t_{sfx}"] = conv(rt.grad)
        if dt == torch.float32:
            out[f"{tag}_g_rot"] = n32(gr)
            out[f"{tag}_g_pos"] = n32(gp)


def fk_case(ref, torch, out, tag, name, seed):
    tree = rh.ref_skeleton_state(ref, name).skeleton_tree
    J = tree.num_joints
    rng = np.random.default_rng(seed)
    local_rot = scaled_quats(rng, (N, J))
    root_t = rng.normal(0, 0.3, (N, 3)).astype(np.float32)
    cot_rot = rng.normal(size=(N, J, 4)).astype(np.float32)
    cot_pos = rng.normal(size=(N, J, 3)).astype(np.float32)
    out[f"{tag}_parents"] = np.asarray(tree.parent_indices, np.int32)
    out[f"{tag}_local_t"] = n32(tree.local_translation)
    for k, v in (("local_rot", local_rot), ("root_t", root_t), ("cot_rot", cot_rot), ("cot_pos", cot_pos)):
        out[f"{tag}_{k}"] = v
    for dt, sfx in ((torch.float32, "f32"), (torch.float64, "f64")):
        lr = torch.from_numpy(local_rot).to(dt).requires_grad_(True)
        rt = torch.from_numpy(root_t).to(dt).requires_grad_(True)
        gr, gp = ref.rkm.cal_forward_kinematics(lr, rt, tree.parent_indices, tree.local_translation.to(dt))
        loss = (gr * torch.from_numpy(cot_rot).to(dt)).sum() + (gp * torch.from_numpy(cot_pos).to(dt)).sum()
        loss.backward()
        conv = n32 if dt == torch.float32 else n64
        out[f"{tag}_grad_local_rot_{sfx}"] = conv(lr.grad)
        out[f"{tag}_grad_root_t_{sfx}"] = conv(rt.grad)
        if dt == torch.float32:
            out[f"{tag}_g_rot"] = n32(gr)
            out[f"{tag}_g_pos"] = n32(gp)


def main() -> None:
    import torch
    torch.set_num_threads(1)
    ref = rh.load_reference()
    out = {}
    dof_case(ref, torch, out, "hu_v5_noclip", "hu_v5", "retarget.robot_config.Hu_v5", False, 900)
    dof_case(ref, torch, out, "hu_clip", "hu", "retarget.robot_config.Hu", True, 901)
    fk_case(ref, torch, out, "vtrdyn_full", "vtrdyn_full", 902)
    save_npz(OUT, out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()

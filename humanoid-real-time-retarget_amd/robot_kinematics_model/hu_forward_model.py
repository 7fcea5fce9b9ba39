"""Drop-in ``HuForwardModel`` (robot_kinematics_model/hu_forward_model.py:13-33).

Joint angles -> quat_from_angle_axis about each DOF's axis -> FK, as one HIP
launch (``rtg_dof_fk_f32``: the local rotations are built in-lane and never
stored).  The reference module imports ``motion_convert.*``, which it does not
ship; its tables are retarget/robot_config/Hu.py (33-link Hu, 32 DOFs, with
limits).  For the 31-link Hu v5 the axes are Hu_v5.Hu_DOF_AXIS; Hu_v5's limit
tables hold 32 entries for 30 DOFs, so clip_angles=True raises there (where the
reference's torch.clamp would fail to broadcast).
"""
from __future__ import annotations

import torch

from robot_kinematics_model.base_forward_model import BaseForwardModel
from rtg import ops
from rtg.bridge import home_device, topology
from rtg.runtime import DofModel


def _default_tables(num_dofs: int):
    if num_dofs == 32:
        from retarget.robot_config import Hu
        return Hu.Hu_DOF_AXIS, Hu.Hu_DOF_LOWER, Hu.Hu_DOF_UPPER
    if num_dofs == 30:
        from retarget.robot_config import Hu_v5
        return Hu_v5.Hu_DOF_AXIS, None, None
    raise ValueError(f"no Hu DOF table for {num_dofs} DOFs; pass dof_axis (and limits) explicitly")


class HuForwardModel(BaseForwardModel):
    def __init__(self, skeleton_tree, device="cuda:0", dof_axis=None, dof_lower=None, dof_upper=None):
        super().__init__(skeleton_tree, device)
        n = self.num_joints - 1
        if dof_axis is None:
            dof_axis, dof_lower, dof_upper = _default_tables(n)
        self.joint_rotation_axis = torch.eye(3)[list(dof_axis)]   # :16
        self.dof_lower = dof_lower
        self.dof_upper = dof_upper
        topo = topology(self.parent_indices, self.sk_local_translation)
        self._model = DofModel(topo, dof_axis, dof_lower, dof_upper)
        self.node_names = list(getattr(skeleton_tree, "node_names", None) or [])

    def _rotation_targets(self, target_rotations, rotation_links, rotation_weight):
        """fit_keypoints' / fit_pose's orientation arguments as ops': links as joint indices (names resolved through the
        tree's node names), (L, K, 4) target rotations, (K,) weights or None.  All None: no orientation targets."""
        if target_rotations is None and rotation_links is None and rotation_weight is None:
            return {}
        if target_rotations is None or rotation_links is None:
            raise ValueError("orientation targets need both target_rotations and rotation_links")
        names = getattr(self, "node_names", [])
        joints = []
        for link in rotation_links:
            if isinstance(link, str):
                if link not in names:
                    raise ValueError(f"rotation_links: the skeleton has no node named {link!r}")
                joints.append(names.index(link))
            else:
                joints.append(int(link))
        return dict(rot_joints=joints, target_rot=target_rotations, rot_weight=rotation_weight)

    def forward_kinematics(self, motion_joint_angles, motion_root_translation, motion_root_rotation, clip_angles):
        """(L, J-1, 1) angles, (L, 3) root translation, (L, 1, 4) root rotation -> ((L, J, 4), (L, J, 3))."""
        if clip_angles and not self._model.has_limits:
            raise ValueError("clip_angles needs DOF limits with one entry per DOF")
        dev = home_device(motion_joint_angles, motion_root_translation, motion_root_rotation)
        g_rot, g_pos = ops.dof_forward_kinematics(self._model, motion_joint_angles, motion_root_rotation,
                                                  motion_root_translation, clip=bool(clip_angles))
        return g_rot.to(dev), g_pos.to(dev)

    def fit_keypoints(self, target_positions, motion_root_translation, motion_root_rotation,
                      motion_joint_angles=None, weight=None, iters=32, lr=0.02, betas=(0.9, 0.999), eps=1e-8,
                      clip_angles=True, state=None, return_grad=False, target_rotations=None, rotation_links=None,
                      rotation_weight=None):
        """Not in the reference, which only ships the forward model of its optimisation-based converter: the loop that
        model is for -- a keypoint loss sum_j weight[j] |g_pos[:, j] - target_positions[:, j]|^2 minimised over the
        joint angles with torch.optim.Adam -- as one launch (ops.dof_fit).  (L, J, 3) targets, (L, 3) root translation,
        (L, 1, 4) root rotation, (L, J-1, 1) starting angles (default: zeros) -> ((L, J-1, 1) angles, (L,) loss,
        state[, (L, J-1, 1) gradient]); ``state`` from an earlier call continues its optimiser.  The angles are not
        projected onto the limits: apply _clip_angles (or a clamp) to the result for the final pose.
        ``target_rotations`` (L, K, 4), ``rotation_links`` (K node names or joint indices, K <= 8) and
        ``rotation_weight`` (K,) add fit_pose's orientation term for those links, the root given."""
        if clip_angles and not self._model.has_limits:
            raise ValueError("clip_angles needs DOF limits with one entry per DOF")
        dev = home_device(target_positions, motion_root_translation, motion_root_rotation)
        n = self.num_joints - 1
        res = ops.dof_fit(self._model, target_positions, motion_root_rotation, motion_root_translation,
                          dof0=motion_joint_angles, weight=weight, iters=iters, lr=lr, betas=betas, eps=eps,
                          clip=bool(clip_angles), state=state, return_grad=return_grad,
                          **self._rotation_targets(target_rotations, rotation_links, rotation_weight))
        dof, loss, new_state = res[:3]
        shaped = lambda a: a.reshape(tuple(loss.shape) + (n, 1)).to(dev)
        out = (shaped(dof), loss.to(dev), new_state)
        return out + (shaped(res[3]),) if return_grad else out

    def fit_pose(self, target_positions, motion_root_translation, motion_root_rotation, motion_joint_angles=None,
                 weight=None, iters=32, lr=0.02, lr_root_t=None, lr_root_rot=None, fit_root_t=True, fit_root_rot=True,
                 betas=(0.9, 0.999), eps=1e-8, clip_angles=True, state=None, return_grad=False, target_rotations=None,
                 rotation_links=None, rotation_weight=None):
        """fit_keypoints with the floating base among the parameters (ops.pose_fit): mocap keypoints come from a body
        of other proportions, and with the root pinned the legs cannot reach them.  (L, J, 3) targets, (L, 3) root
        translation and (L, 1, 4) root rotation to start from (or given, where fit_root_t / fit_root_rot is False),
        (L, J-1, 1) starting angles (default: zeros) -> ((L, J-1, 1) angles, (L, 3) root translation, (L, 1, 4) root
        rotation, (L,) loss, state[, (L, J-1, 1) gradient, (L, 7) root gradient {dL/dt, dL/dq}]); ``state`` from an
        earlier call continues its optimiser.  The fitted rotation comes back unit.
        ``target_rotations`` (L, K, 4) [x, y, z, w], ``rotation_links`` (K node names or joint indices, K <= 8) and
        ``rotation_weight`` (K,, default ones): global rotations those links are pulled towards in the same launch, by
        the loss term rotation_weight[k] (2 sin(theta_k / 2))^2 of the angle to the target -- "this hand points this
        way, this foot is flat".  Keypoints alone leave wrists, ankles, the head and every link's twist where the
        start had them."""
        if clip_angles and not self._model.has_limits:
            raise ValueError("clip_angles needs DOF limits with one entry per DOF")
        dev = home_device(target_positions, motion_root_translation, motion_root_rotation)
        n = self.num_joints - 1
        res = ops.pose_fit(self._model, target_positions, motion_root_rotation, motion_root_translation,
                           dof0=motion_joint_angles, weight=weight, iters=iters, lr=lr, lr_root_t=lr_root_t,
                           lr_root_rot=lr_root_rot, fit_root_t=fit_root_t, fit_root_rot=fit_root_rot, betas=betas,
                           eps=eps, clip=bool(clip_angles), state=state, return_grad=return_grad,
                           **self._rotation_targets(target_rotations, rotation_links, rotation_weight))
        lead = tuple(res.loss.shape)
        shaped = lambda a: a.reshape(lead + (n, 1)).to(dev)
        out = (shaped(res.dof), res.root_t.to(dev), res.root_rot.reshape(lead + (1, 4)).to(dev), res.loss.to(dev),
               res.state)
        return out + (shaped(res.grad), res.grad_root.to(dev)) if return_grad else out

    def _clip_angles(self, motion_joint_angles):
        """:27-33, forward value: (clamp(a, lo, hi) - a) + a, elementwise on the angles' device."""
        a = motion_joint_angles
        lo = torch.as_tensor(self.dof_lower, dtype=a.dtype, device=a.device).reshape(1, -1, 1)
        hi = torch.as_tensor(self.dof_upper, dtype=a.dtype, device=a.device).reshape(1, -1, 1)
        c = torch.clamp(a.clone(), min=lo, max=hi)
        return (c - a).detach() + a

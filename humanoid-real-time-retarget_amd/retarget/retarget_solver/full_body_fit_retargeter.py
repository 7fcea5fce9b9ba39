"""``VtrdynFullBodyFitRetargeter``: not in the reference, whose closed-form solvers write the arm DOFs only.  Mocap body
positions to ALL joint angles and the floating base of a Hu skeleton: the limb-wise rescale of the mapped keypoints to
the robot's proportions (``HuForwardModel.keypoint_targets``, one launch) and the fused pose fit on them
(``fit_pose`` / ``fit_motion``, one launch per round) -- ``HuForwardModel.fit_mocap`` with the previous call's result
carried as the next start, as its posture prior and with its optimiser state: frame t from frame t - 1.

No joint mapping is shipped: ``joint_mapping`` is the caller's {mocap joint name: robot link name} dict, as
``SkeletonState.retarget_to`` takes it, with the robot's root link among the targets.
"""
from __future__ import annotations

import torch

from robot_kinematics_model.hu_forward_model import HuForwardModel
from rtg.runtime import require_gpu_rtg


class VtrdynFullBodyFitRetargeter:
    def __init__(self, mocap_zero_pose, target_zero_pose, joint_mapping, dof_axis=None, dof_lower=None, dof_upper=None,
                 prior_weight=0.1, **defaults):
        """mocap_zero_pose / target_zero_pose: RobotZeroPose (or anything with ``skeleton_tree``); the DOF tables
        default to HuForwardModel's for the tree.  ``prior_weight``: the weight per rad^2 of the posture prior towards
        the previous call's angles (a number or (J-1,); 0 or None: no prior).  ``defaults``: fit_mocap's keywords for
        every call (iters, lr, dir, root_scale, smooth_weight, project_angles, apart, ...)."""
        self.source_zero_pose, self.target_zero_pose = mocap_zero_pose, target_zero_pose
        self.joint_mapping = dict(joint_mapping)
        self._tables = (dof_axis, dof_lower, dof_upper)
        self.prior_weight = prior_weight
        self.defaults = dict(defaults)
        self._model = None
        self.reset()

    def reset(self):
        """Forget the previous call: the next one starts from fit_mocap's defaults."""
        self._angles = self._root_rot = self._state = None

    @property
    def model(self) -> HuForwardModel:
        if self._model is None:   # built lazily so construction works before a GPU is touched
            require_gpu_rtg()
            self._model = HuForwardModel(self.target_zero_pose.skeleton_tree, dof_axis=self._tables[0],
                                         dof_lower=self._tables[1], dof_upper=self._tables[2])
        return self._model

    def retarget_batch(self, body_global_translation, **keywords):
        """B frames: body (B, J_s, 3) (the 21 VTRDyn body joints) -> (dof (B, J-1), root_t (B, 3), root_rot (B, 4),
        loss (B,)).  A call of the same B as the one before starts from its angles and root rotation, holds the
        angles to them by the posture prior and continues its optimiser; any other B starts afresh.  ``keywords``
        override the defaults for this call.  Raises RtgError without a GPU."""
        hu = self.model
        kw = dict(self.defaults, **keywords)
        body = torch.as_tensor(body_global_translation)
        B = int(body.shape[0])
        if self._angles is not None and int(self._angles.shape[0]) != B:
            self.reset()
        smooth = float(kw.get("smooth_weight", 0.0)) > 0.0
        if self._angles is not None:
            if self.prior_weight is not None and not smooth and "prior_angles" not in kw:   # fit_motion sets its own
                kw.update(prior_angles=self._angles, prior_weight=self.prior_weight)
            if not smooth:
                kw.setdefault("state", self._state)
        res = hu.fit_mocap(self.source_zero_pose.skeleton_tree, self.joint_mapping, body,
                           motion_root_rotation=self._root_rot, motion_joint_angles=self._angles, **kw)
        angles, root_t, root_rot, loss, state = res[:5]
        self._angles, self._root_rot, self._state = angles, root_rot, state
        return angles[..., 0], root_t, root_rot[..., 0, :], loss

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
from rtg.bridge import fit_targets_plan, home_device, topology
from rtg.runtime import DofModel, require_gpu_rtg


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

    def _posture_prior(self, prior_angles, prior_weight, project_angles):
        """fit_keypoints' / fit_pose's posture arguments as ops': (L, J-1, 1) or (L, J-1) prior angles, a number or
        (J-1,) weights, the projection (it needs the limits)."""
        if project_angles and not self._model.has_limits:
            raise ValueError("project_angles needs DOF limits with one entry per DOF")
        return dict(prior=prior_angles, prior_weight=prior_weight, project=bool(project_angles))

    @staticmethod
    def _robust(keypoint_confidence, robust_scale):
        """fit_pose's ``keypoint_confidence`` (L, J) and ``robust_scale`` as ops.pose_fit's keywords."""
        return dict(frame_weight=keypoint_confidence, robust_scale=robust_scale)

    def forward_kinematics(self, motion_joint_angles, motion_root_translation, motion_root_rotation, clip_angles):
        """(L, J-1, 1) angles, (L, 3) root translation, (L, 1, 4) root rotation -> ((L, J, 4), (L, J, 3))."""
        if clip_angles and not self._model.has_limits:
            raise ValueError("clip_angles needs DOF limits with one entry per DOF")
        dev = home_device(motion_joint_angles, motion_root_translation, motion_root_rotation)
        g_rot, g_pos = ops.dof_forward_kinematics(self._model, motion_joint_angles, motion_root_rotation,
                                                  motion_root_translation, clip=bool(clip_angles))
        return g_rot.to(dev), g_pos.to(dev)

    def link_velocities(self, angles, root_translation, root_rotation, joint_velocities, root_velocity=None,
                        root_angular_velocity=None, clip_angles=False):
        """Not in the reference's forward model; what its SkeletonMotion carries (skeleton3d.py:1026-1146) from joint
        velocities instead of finite differences: (L, J-1, 1) or (L, J-1) angles and joint velocities, (L, 3) root
        translation, (L, 1, 4) root rotation and the root's world-frame linear and angular velocity (L, 3) each (None:
        zero) -> (global_velocity (L, J, 3), global_angular_velocity (L, J, 3)), world frame, in one launch
        (ops.dof_link_velocity).  With ``clip_angles`` a joint whose angle lies outside its limits does not turn."""
        if clip_angles and not self._model.has_limits:
            raise ValueError("clip_angles needs DOF limits with one entry per DOF")
        dev = home_device(angles, root_translation, root_rotation)
        root_vel = None
        if root_velocity is not None or root_angular_velocity is not None:
            v, w = (None if x is None else torch.as_tensor(x, dtype=torch.float32)
                    for x in (root_velocity, root_angular_velocity))
            ref = v if v is not None else w
            if tuple(ref.shape[-1:]) != (3,) or (v is not None and w is not None and v.shape != w.shape):
                raise ValueError("root_velocity / root_angular_velocity must be (L, 3) each")
            root_vel = torch.cat([torch.zeros_like(ref) if v is None else v,
                                  torch.zeros_like(ref) if w is None else w.to(ref.device)], dim=-1)
        _, _, g_vel = ops.dof_link_velocity(self._model, angles, root_rotation, root_translation, joint_velocities,
                                            root_vel, clip=bool(clip_angles), want_pose=False)
        return g_vel[..., :3].to(dev), g_vel[..., 3:].to(dev)

    def motion_library(self, clips):
        """``rtg.motion.DofMotionLibrary(self, clips)``: fitted clips -- (angles, root translation, root rotation, fps)
        tuples, fit_pose's first three results in its order -- packed for sampling at arbitrary times."""
        from rtg.motion import DofMotionLibrary
        return DofMotionLibrary(self, clips)

    def fit_keypoints(self, target_positions, motion_root_translation, motion_root_rotation,
                      motion_joint_angles=None, weight=None, iters=32, lr=0.02, betas=(0.9, 0.999), eps=1e-8,
                      clip_angles=True, state=None, return_grad=False, target_rotations=None, rotation_links=None,
                      rotation_weight=None, prior_angles=None, prior_weight=None, project_angles=False, apart=None,
                      keypoint_confidence=None, robust_scale=None):
        """Not in the reference, which only ships the forward model of its optimisation-based converter: the loop that
        model is for -- a keypoint loss sum_j weight[j] |g_pos[:, j] - target_positions[:, j]|^2 minimised over the
        joint angles with torch.optim.Adam -- as one launch (ops.dof_fit).  (L, J, 3) targets, (L, 3) root translation,
        (L, 1, 4) root rotation, (L, J-1, 1) starting angles (default: zeros) -> ((L, J-1, 1) angles, (L,) loss,
        state[, (L, J-1, 1) gradient]); ``state`` from an earlier call continues its optimiser.  The angles are not
        projected onto the limits unless ``project_angles`` is set: without it apply _clip_angles (or a clamp) to the
        result for the final pose.
        ``target_rotations`` (L, K, 4), ``rotation_links`` (K node names or joint indices, K <= 8) and
        ``rotation_weight`` (K,) add fit_pose's orientation term for those links, the root given.  ``prior_angles``,
        ``prior_weight``, ``project_angles``: fit_pose's posture prior and projection.  ``apart``: its keep-apart spheres
        and floor.  ``keypoint_confidence`` (L, J), ``robust_scale``: its per-frame keypoint weights and robust keypoint
        loss."""
        if clip_angles and not self._model.has_limits:
            raise ValueError("clip_angles needs DOF limits with one entry per DOF")
        dev = home_device(target_positions, motion_root_translation, motion_root_rotation)
        n = self.num_joints - 1
        res = ops.dof_fit(self._model, target_positions, motion_root_rotation, motion_root_translation,
                          dof0=motion_joint_angles, weight=weight, iters=iters, lr=lr, betas=betas, eps=eps,
                          clip=bool(clip_angles), state=state, return_grad=return_grad,
                          **self._rotation_targets(target_rotations, rotation_links, rotation_weight),
                          **self._posture_prior(prior_angles, prior_weight, project_angles), apart=apart,
                          **self._robust(keypoint_confidence, robust_scale))
        dof, loss, new_state = res[:3]
        shaped = lambda a: a.reshape(tuple(loss.shape) + (n, 1)).to(dev)
        out = (shaped(dof), loss.to(dev), new_state)
        return out + (shaped(res[3]),) if return_grad else out

    def fit_pose(self, target_positions, motion_root_translation, motion_root_rotation, motion_joint_angles=None,
                 weight=None, iters=32, lr=0.02, lr_root_t=None, lr_root_rot=None, fit_root_t=True, fit_root_rot=True,
                 betas=(0.9, 0.999), eps=1e-8, clip_angles=True, state=None, return_grad=False, target_rotations=None,
                 rotation_links=None, rotation_weight=None, prior_angles=None, prior_weight=None, project_angles=False,
                 apart=None, keypoint_confidence=None, robust_scale=None):
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
        start had them.
        ``prior_angles`` (L, J-1, 1) or (L, J-1) and ``prior_weight`` (a number or (J-1,), default ones) add the posture
        term sum_d prior_weight[d] (angle_d - prior_d)^2 on the iterate: it holds DOFs no target observes, and a
        redundant arm's swivel, to a rest pose or to the last frame's solution.  ``project_angles`` clamps every angle
        to its limits after each step, so an unreachable target cannot push the iterate past a limit without bound.
        ``apart``: keep-apart spheres and a floor, built once with ``rtg.ops.apart(self, links, radii, ...)`` (links by
        node name or joint index): spheres riding on links, pairs of them pushed apart where they overlap, and spheres
        held above a ground plane -- what keeps a wrist out of the torso, one gripper out of the other and an ankle
        above the floor when the keypoints come from a body of other proportions.  No default radii are shipped: the
        repository holds Hu's skeleton only, no collision geometry; measure them or take them from the robot's URDF.
        ``keypoint_confidence`` (L, J): per-frame, per-keypoint weights multiplied into ``weight`` -- a vision
        tracker's confidences, a foot held hard in the frames where it is in contact.  A keypoint whose confidence is 0
        is skipped in that frame: its target row may hold anything, NaN included (an occluded marker, a dropped frame).
        ``robust_scale`` (metres, None: off) makes the keypoint term the pseudo-Huber loss of that scale: quadratic
        for residuals well below it, linear far out, so one glitched or swapped marker no longer drags its limb and,
        through the floating base, the body.  Both act inside the one launch (ops.pose_fit)."""
        if clip_angles and not self._model.has_limits:
            raise ValueError("clip_angles needs DOF limits with one entry per DOF")
        dev = home_device(target_positions, motion_root_translation, motion_root_rotation)
        n = self.num_joints - 1
        res = ops.pose_fit(self._model, target_positions, motion_root_rotation, motion_root_translation,
                           dof0=motion_joint_angles, weight=weight, iters=iters, lr=lr, lr_root_t=lr_root_t,
                           lr_root_rot=lr_root_rot, fit_root_t=fit_root_t, fit_root_rot=fit_root_rot, betas=betas,
                           eps=eps, clip=bool(clip_angles), state=state, return_grad=return_grad,
                           **self._rotation_targets(target_rotations, rotation_links, rotation_weight),
                           **self._posture_prior(prior_angles, prior_weight, project_angles), apart=apart,
                           **self._robust(keypoint_confidence, robust_scale))
        lead = tuple(res.loss.shape)
        shaped = lambda a: a.reshape(lead + (n, 1)).to(dev)
        out = (shaped(res.dof), res.root_t.to(dev), res.root_rot.reshape(lead + (1, 4)).to(dev), res.loss.to(dev),
               res.state)
        return out + (shaped(res.grad), res.grad_root.to(dev)) if return_grad else out

    def fit_motion(self, target_positions, motion_root_translation, motion_root_rotation, motion_joint_angles=None,
                   smooth_weight=0.1, rounds=8, iters=8, **fit_pose_keywords):
        """fit_pose for a clip whose rows are consecutive frames: frames fitted on their own jitter with the keypoint
        noise, so the fit runs ``rounds`` times ``iters`` steps, and before each round every frame's angles get a
        posture prior towards the mean of its two neighbours in the current iterate,
        prior[f] = (a[max(f-1, 0)] + a[min(f+1, L-1)]) / 2 (the ends repeat, like the reference's "nearest" Gaussian
        filters), with ``smooth_weight`` per rad^2.  Each round is one fit_pose launch from the current angles and
        root that carries the optimiser state.  ``smooth_weight == 0`` passes no prior: that is one fit_pose of
        rounds * iters steps, bit for bit.  Only the angles are smoothed: the root can be regularised through
        weight[0] and an orientation target on link 0.  The other keywords are fit_pose's (``prior_angles`` and
        ``state`` are this method's to set; ``prior_weight`` scales smooth_weight per DOF; ``apart``,
        ``keypoint_confidence`` and ``robust_scale`` go to every round).  A frame whose keypoints are all masked
        (``keypoint_confidence`` 0) has only the prior left: with ``smooth_weight > 0`` it is held by its neighbours'
        mean, round after round, so a gap of dropped frames is filled in from its ends.  Returns what fit_pose
        returns, after the last round."""
        for k in ("prior_angles", "state"):
            if k in fit_pose_keywords:
                raise ValueError(f"fit_motion sets {k} itself")
        rounds, smooth_weight = int(rounds), float(smooth_weight)
        if rounds < 1:
            raise ValueError(f"rounds must be at least 1, got {rounds}")
        if not smooth_weight >= 0.0:
            raise ValueError(f"smooth_weight must not be negative, got {smooth_weight}")
        pw = fit_pose_keywords.pop("prior_weight", None)
        want_grad = bool(fit_pose_keywords.pop("return_grad", False))
        a, t, q, state = motion_joint_angles, motion_root_translation, motion_root_rotation, None
        for r in range(rounds):
            prior = {}
            if smooth_weight > 0.0:
                if a is None:   # fit_pose's default start
                    a = torch.zeros(tuple(target_positions.shape[:-2]) + (self.num_joints - 1, 1),
                                    device=target_positions.device, dtype=torch.float32)
                a = torch.as_tensor(a)
                prior = dict(prior_angles=0.5 * (torch.cat([a[:1], a[:-1]]) + torch.cat([a[1:], a[-1:]])),
                             prior_weight=smooth_weight if pw is None else smooth_weight * torch.as_tensor(pw))
            res = self.fit_pose(target_positions, t, q, a, iters=iters, state=state,
                                return_grad=want_grad and r == rounds - 1, **prior, **fit_pose_keywords)
            a, t, q, state = res[0], res[1], res[2], res[4]
        return res

    def keypoint_targets(self, source_tree, joint_mapping, source_positions, dir=None, root_scale=None,
                         root_offset=None):
        """Where fit_pose's ``target_positions`` come from: mocap keypoints of a body of other proportions, every
        mapped limb rescaled to this robot's length (ops.fit_targets, one launch).  ``source_tree``: the mocap
        skeleton (node_names, parent_indices, local_translation); ``joint_mapping``: {source name: target name}, as
        ``retarget_to`` takes it, the robot's root among the targets; ``source_positions`` (L, J_s, 3) global
        positions.  ``dir`` (3,) flips the source axes (coord_transform), ``root_scale`` (3,) scales the root's travel
        (ops.limb_ratio of a foot gives the leg-length ratio), ``root_offset`` (3,) is added after it.  ->
        ((L, J, 3) targets, (J,) weight): the weight is 1 for the mapped links and 0 for the others, whose rows are
        finite placeholders.  Plans are cached per (tree, mapping, constants)."""
        require_gpu_rtg()
        src_names, names = list(source_tree.node_names), list(self.node_names)
        sj, tj = [], []
        for s, t in joint_mapping.items():
            if s not in src_names:
                raise ValueError(f"joint_mapping: the source skeleton has no node named {s!r}")
            if t not in names:
                raise ValueError(f"joint_mapping: the skeleton has no node named {t!r}")
            sj.append(src_names.index(s))
            tj.append(names.index(t))
        plan = fit_targets_plan((source_tree.parent_indices, source_tree.local_translation),
                                (self.parent_indices, self.sk_local_translation), sj, tj, dir, root_scale, root_offset)
        targets = ops.fit_targets(plan, source_positions)
        return targets, torch.from_numpy(plan.weight.copy()).to(targets.device)

    def fit_mocap(self, source_tree, joint_mapping, source_positions, motion_root_rotation=None,
                  motion_joint_angles=None, smooth_weight=0.0, dir=None, root_scale=None, root_offset=None, weight=None,
                  source_confidence=None, valid=None, **fit_keywords):
        """Mocap keypoints to a pose in two launches: keypoint_targets, then fit_pose -- or fit_motion when
        ``smooth_weight > 0`` -- on them.  The root translation starts at the root's target row, the root rotation at
        ``motion_root_rotation`` (L, 1, 4) or the identity, the angles at ``motion_joint_angles`` or fit_pose's
        default; the plan's weight masks the unmapped links (multiplied into ``weight`` (J,) when given).  The other
        keywords are fit_pose's (fit_motion's with smoothing).
        ``source_confidence`` (L, J_s) and ``valid`` (L,) bool -- what ``ingest_vtrdyn`` returns next to the positions
        -- become fit_pose's ``keypoint_confidence`` (multiplied into one passed among the keywords): a link takes the
        confidence of the source joint mapped to it, an unmapped link 0, and a frame that is not valid has its whole
        row zeroed, so nothing of a dropped frame reaches the fit (its rows may be zeros or NaN).  A dropped frame is
        then fitted to nothing: it keeps its start unless ``smooth_weight > 0``, where the neighbours' mean holds it
        and a gap is filled in from its ends.  Where the root's own row is masked and not finite, the root translation
        starts at zero.  Returns what they return, plus the targets."""
        targets, w = self.keypoint_targets(source_tree, joint_mapping, source_positions, dir, root_scale, root_offset)
        lead = tuple(targets.shape[:-2])
        t0 = targets[..., 0, :].clone()
        conf = self._mocap_confidence(source_tree, joint_mapping, lead, source_confidence, valid, targets.device)
        if conf is not None:
            given = fit_keywords.pop("keypoint_confidence", None)
            if given is not None:
                conf = conf * torch.as_tensor(given, dtype=torch.float32).to(conf.device)
            fit_keywords["keypoint_confidence"] = conf
            lost = (conf[..., 0] == 0) & ~torch.isfinite(t0).all(dim=-1)
            t0[lost] = 0.0
        q0 = motion_root_rotation
        if q0 is None:
            q0 = torch.zeros(lead + (1, 4), device=targets.device, dtype=torch.float32)
            q0[..., 3] = 1.0
        if weight is not None:
            w = w * torch.as_tensor(weight, dtype=torch.float32).to(w.device)
        if float(smooth_weight) > 0.0:
            res = self.fit_motion(targets, t0, q0, motion_joint_angles, smooth_weight=smooth_weight, weight=w,
                                  **fit_keywords)
        else:
            res = self.fit_pose(targets, t0, q0, motion_joint_angles, weight=w, **fit_keywords)
        return tuple(res) + (targets,)

    def _mocap_confidence(self, source_tree, joint_mapping, lead, source_confidence, valid, device):
        """fit_mocap's per-frame weights (L, J) from the source's: source_confidence (L, J_s) gathered through the
        joint mapping (unmapped links 0; None: ones on every link), a frame with ``valid`` False zeroed.  None when
        neither is given."""
        if source_confidence is None and valid is None:
            return None
        J = self.num_joints
        if source_confidence is None:
            conf = torch.ones(lead + (J,), device=device, dtype=torch.float32)
        else:
            src_names, names = list(source_tree.node_names), list(self.node_names)
            sc = torch.as_tensor(source_confidence)
            if tuple(sc.shape) != lead + (len(src_names),):
                raise ValueError(f"source_confidence {tuple(sc.shape)} must be {lead + (len(src_names),)}")
            sc = sc.to(device=device, dtype=torch.float32)
            conf = torch.zeros(lead + (J,), device=device, dtype=torch.float32)
            sj = [src_names.index(a) for a in joint_mapping]
            tj = [names.index(b) for b in joint_mapping.values()]
            conf[..., tj] = sc[..., sj]
        if valid is not None:
            ok = torch.as_tensor(valid)
            if tuple(ok.shape) != lead:
                raise ValueError(f"valid {tuple(ok.shape)} must be {lead}")
            conf = conf * (ok.to(device) != 0).to(torch.float32).unsqueeze(-1)
        return conf

    def _clip_angles(self, motion_joint_angles):
        """:27-33, forward value: (clamp(a, lo, hi) - a) + a, elementwise on the angles' device."""
        a = motion_joint_angles
        lo = torch.as_tensor(self.dof_lower, dtype=a.dtype, device=a.device).reshape(1, -1, 1)
        hi = torch.as_tensor(self.dof_upper, dtype=a.dtype, device=a.device).reshape(1, -1, 1)
        c = torch.clamp(a.clone(), min=lo, max=hi)
        return (c - a).detach() + a

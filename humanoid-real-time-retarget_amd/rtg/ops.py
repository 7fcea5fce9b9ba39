"""Functional device ops over the C ABI (batched forms of the reference's functions).

Each function takes tensors (host or device; moved to the current HIP device as
contiguous float32) and returns device tensors.  Reference semantics are cited
per op; all arithmetic happens in librtg_hip.so.
"""
from __future__ import annotations

import collections
import ctypes
import functools
from typing import Sequence

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import check, lib
from .runtime import (FitTargetsPlan, MotionLib, RetargetPlan, Topology, dev_f32, layout_code, ptr, require_gpu, require_gpu_rtg,
                      stream_handle)


def _flat(t: torch.Tensor, tail: int) -> torch.Tensor:
    return t.reshape(-1, tail) if tail else t.reshape(-1)


def _quat_op(op, a, b=None, c=None, a_tail=4, b_tail=4, c_tail=3, out_tail=4):
    a = dev_f32(a)
    lead = a.shape[:-1] if a_tail else a.shape
    n = int(torch.Size(lead).numel())
    af = _flat(a, a_tail)
    bf = None if b is None else _flat(dev_f32(b).expand(*lead, *( (b_tail,) if b_tail else ())).contiguous(), b_tail)
    cf = None if c is None else _flat(dev_f32(c).expand(*lead, *((c_tail,) if c_tail else ())).contiguous(), c_tail)
    out_shape = tuple(lead) + ((out_tail,) if isinstance(out_tail, int) and out_tail else tuple(out_tail or ()))
    out = torch.empty(out_shape, device=a.device, dtype=torch.float32)
    check(lib().rtg_quat_op_f32(op, ptr(af), ptr(bf), ptr(cf), n, ptr(out), stream_handle()))
    return out


def _bcast(a, b, ta, tb):
    a, b = dev_f32(a), dev_f32(b)
    lead = torch.broadcast_shapes(a.shape[:-1], b.shape[:-1])
    return a.expand(*lead, ta).contiguous(), b.expand(*lead, tb).contiguous()


def quat_mul(a, b):
    """rotation3d.py:14-27"""
    a, b = _bcast(a, b, 4, 4)
    return _quat_op(_lib.OP_QUAT_MUL, a, b)


def quat_mul_norm(a, b):
    """rotation3d.py:196-202"""
    a, b = _bcast(a, b, 4, 4)
    return _quat_op(_lib.OP_QUAT_MUL_NORM, a, b)


def quat_normalize(q):
    """rotation3d.py:92-98"""
    return _quat_op(_lib.OP_QUAT_NORMALIZE, q)


def quat_inverse(q):
    """rotation3d.py:214-219"""
    return _quat_op(_lib.OP_QUAT_INVERSE, q)


def quat_rotate(q, v):
    """rotation3d.py:205-211"""
    q, v = _bcast(q, v, 4, 3)
    return _quat_op(_lib.OP_QUAT_ROTATE, q, v, b_tail=3, out_tail=3)


def quat_from_angle_axis(angle, axis):
    """rotation3d.py:122-143 (angle (...), axis (...,3))"""
    angle = dev_f32(angle)
    axis = dev_f32(axis)
    lead = torch.broadcast_shapes(angle.shape, axis.shape[:-1])
    angle = angle.expand(lead).contiguous()
    axis = axis.expand(*lead, 3).contiguous()
    n = int(torch.Size(lead).numel())
    out = torch.empty(tuple(lead) + (4,), device=angle.device, dtype=torch.float32)
    check(lib().rtg_quat_op_f32(_lib.OP_QUAT_FROM_ANGLE_AXIS, ptr(angle), ptr(axis), None, n, ptr(out),
                                stream_handle()))
    return out


def quat_from_rotation_matrix(m):
    """rotation3d.py:146-193 (m (...,3,3))"""
    m = dev_f32(m, (3, 3), "m")
    lead = m.shape[:-2]
    n = int(torch.Size(lead).numel())
    out = torch.empty(tuple(lead) + (4,), device=m.device, dtype=torch.float32)
    check(lib().rtg_quat_op_f32(_lib.OP_QUAT_FROM_ROTMAT, ptr(m), None, None, n, ptr(out), stream_handle()))
    return out


def quat_to_exp_map(q):
    """rotation3d.py:620-627"""
    return _quat_op(_lib.OP_QUAT_TO_EXP_MAP, q, out_tail=3)


def quat_to_angle_axis(q):
    """rotation3d.py:587-608 -> (angle (...), axis (...,3))"""
    r = _quat_op(_lib.OP_QUAT_TO_ANGLE_AXIS, q, out_tail=4)
    return r[..., 0], r[..., 1:]


def quat_abs(q):
    """rotation3d.py:41-47"""
    return _quat_op(_lib.OP_QUAT_ABS, q, out_tail=0)


def quat_unit(q):
    """rotation3d.py:50-56"""
    return _quat_op(_lib.OP_QUAT_UNIT, q)


def quat_angle_axis(q):
    """rotation3d.py:230-240 -> (angle in [0, pi] (...), unit axis (...,3))"""
    r = _quat_op(_lib.OP_QUAT_ANGLE_AXIS, q, out_tail=4)
    return r[..., 0], r[..., 1:]


def normalize_angle(x):
    """rotation3d.py:582-584 (atan2 with glibc atan2f semantics: the reference's <32-element path)"""
    x = dev_f32(x)
    out = torch.empty_like(x)
    check(lib().rtg_quat_op_f32(_lib.OP_NORMALIZE_ANGLE, ptr(x), None, None, x.numel(), ptr(out), stream_handle()))
    return out


def radians_between_vecs(v1, v2, n):
    """transform3d.py:77-100, batched over leading dims"""
    v1, v2, n = dev_f32(v1), dev_f32(v2), dev_f32(n)
    lead = torch.broadcast_shapes(v1.shape[:-1], v2.shape[:-1], n.shape[:-1])
    v1, v2, n = (t.expand(*lead, 3).contiguous() for t in (v1, v2, n))
    cnt = int(torch.Size(lead).numel())
    out = torch.empty(tuple(lead), device=v1.device, dtype=torch.float32)
    check(lib().rtg_quat_op_f32(_lib.OP_RADIANS_BETWEEN, ptr(v1), ptr(v2), ptr(n), cnt, ptr(out), stream_handle()))
    return out


def proj_in_plane(v, n):
    """transform3d.py:61-75, batched"""
    nn = dev_f32(n)
    if bool((torch.linalg.norm(nn, dim=-1) <= 1e-6).any()):
        raise AssertionError("proj_in_plane: plane normal has (near) zero length")   # transform3d.py:70
    v, nn = _bcast(v, nn, 3, 3)
    return _quat_op(_lib.OP_PROJ_IN_PLANE, v, nn, a_tail=3, b_tail=3, out_tail=3)


def quat_to_dof_pos_hu(local_rot):
    """transform3d.py:176-183 with Hu_DOF_AXIS over local_rot[..., 1:, :] (local_rot (...,31,4))"""
    lr = dev_f32(local_rot, (31, 4), "local_rot")
    lead = lr.shape[:-2]
    n = int(torch.Size(lead).numel())
    out = torch.empty(tuple(lead) + (30,), device=lr.device, dtype=torch.float32)
    check(lib().rtg_quat_op_f32(_lib.OP_QUAT_TO_DOF_POS, ptr(lr), None, None, n, ptr(out), stream_handle()))
    return out


def cal_shoulder_pr(v1, v0, parent):
    """full_body_pos_retargeter.py:246-278, batched: returns (pitch (...,4), roll (...,4))"""
    v1, v0, parent = dev_f32(v1), dev_f32(v0), dev_f32(parent)
    lead = torch.broadcast_shapes(v1.shape[:-1], v0.shape[:-1], parent.shape[:-1])
    v1, v0, parent = v1.expand(*lead, 3).contiguous(), v0.expand(*lead, 3).contiguous(), parent.expand(*lead, 4).contiguous()
    n = int(torch.Size(lead).numel())
    out = torch.empty(tuple(lead) + (2, 4), device=v1.device, dtype=torch.float32)
    check(lib().rtg_quat_op_f32(_lib.OP_SHOULDER_PR, ptr(v1), ptr(v0), ptr(parent), n, ptr(out), stream_handle()))
    return out[..., 0, :], out[..., 1, :]


def cal_elbow_py(v1, v0, parent):
    """full_body_pos_retargeter.py:220-243, batched: returns (shoulder_yaw, elbow_pitch)"""
    v1, v0, parent = dev_f32(v1), dev_f32(v0), dev_f32(parent)
    lead = torch.broadcast_shapes(v1.shape[:-1], v0.shape[:-1], parent.shape[:-1])
    v1, v0, parent = v1.expand(*lead, 3).contiguous(), v0.expand(*lead, 3).contiguous(), parent.expand(*lead, 4).contiguous()
    n = int(torch.Size(lead).numel())
    out = torch.empty(tuple(lead) + (2, 4), device=v1.device, dtype=torch.float32)
    check(lib().rtg_quat_op_f32(_lib.OP_ELBOW_PY, ptr(v1), ptr(v0), ptr(parent), n, ptr(out), stream_handle()))
    return out[..., 0, :], out[..., 1, :]


def cal_joint_quat(zero_vectors, motion_vectors):
    """transform3d.py:31-50 (Kabsch).  (..., n, 3) x (..., n, 3) -> (..., 4)"""
    Z, M = dev_f32(zero_vectors), dev_f32(motion_vectors)
    lead = torch.broadcast_shapes(Z.shape[:-2], M.shape[:-2])
    npts = int(Z.shape[-2])
    if M.shape[-2] != npts:
        raise ValueError("cal_joint_quat: point counts differ")
    Z = Z.expand(*lead, npts, 3).contiguous()
    M = M.expand(*lead, npts, 3).contiguous()
    n = int(torch.Size(lead).numel())
    out = torch.empty(tuple(lead) + (4,), device=Z.device, dtype=torch.float32)
    check(lib().rtg_cal_joint_quat_f32(ptr(Z), ptr(M), npts, n, ptr(out), stream_handle()))
    return out


def quat_in_xyz_axis(q, seq: str = "xyz"):
    """transform3d.py:52-59: three single-axis quaternions (each (...,4))."""
    q = dev_f32(q, (4,), "q")
    lead = q.shape[:-1]
    n = int(torch.Size(lead).numel())
    out = torch.empty(tuple(lead) + (3, 4), device=q.device, dtype=torch.float32)
    check(lib().rtg_quat_in_xyz_axis_f32(ptr(q), seq.encode(), n, ptr(out), stream_handle()))
    return out[..., 0, :], out[..., 1, :], out[..., 2, :]


def _fk_launch(topo: Topology, lr, rt, state: bool):
    J = topo.num_joints
    lead = lr.shape[:-2]
    B = int(torch.Size(lead).numel())
    g_rot = torch.empty(tuple(lead) + (J, 4), device=lr.device, dtype=torch.float32)
    g_pos = torch.empty(tuple(lead) + (J, 3), device=lr.device, dtype=torch.float32)
    fn = lib().rtg_state_fk_f32 if state else lib().rtg_fk_f32
    check(fn(topo.handle, ptr(lr), ptr(rt), B, ptr(g_rot), ptr(g_pos), stream_handle()))
    return g_rot, g_pos


def _cotangent(g):
    """An upstream gradient as the kernels read it (None stays None: not read, not zero-filled)."""
    return None if g is None else g.to(torch.float32).contiguous()


class _FK(torch.autograd.Function):
    """forward_kinematics(state=False) with its HIP adjoint (rtg_fk_backward_f32); the forward is the same launch."""

    @staticmethod
    def forward(ctx, topo, lr, rt):
        ctx.set_materialize_grads(False)
        g_rot, g_pos = _fk_launch(topo, lr, rt, False)
        ctx.topo = topo
        ctx.save_for_backward(lr, g_rot)
        return g_rot, g_pos

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_g_rot, grad_g_pos):
        need_lr, need_rt = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if (grad_g_rot is None and grad_g_pos is None) or not (need_lr or need_rt):
            return None, None, None
        lr, g_rot = ctx.saved_tensors
        B = int(torch.Size(lr.shape[:-2]).numel())
        ggr, ggp = _cotangent(grad_g_rot), _cotangent(grad_g_pos)
        g_lr = torch.empty_like(lr) if need_lr else None
        g_rt = torch.empty(tuple(lr.shape[:-2]) + (3,), device=lr.device, dtype=torch.float32) if need_rt else None
        check(lib().rtg_fk_backward_f32(ctx.topo.handle, ptr(lr), ptr(g_rot), ptr(ggr), ptr(ggp), B, ptr(g_lr),
                                        ptr(g_rt), stream_handle()))
        return None, g_lr, g_rt


def forward_kinematics(topo: Topology, local_rot, root_t, state: bool = False):
    """kinematics.py:13-39 (state=False) / SkeletonState FK skeleton3d.py:402-425 (state=True).  state=False is
    differentiable with respect to local_rot and root_t (the reference's FK is plain torch); state=True is not."""
    J = topo.num_joints
    lr = dev_f32(local_rot, (J, 4), "local_rot")
    lead = lr.shape[:-2]
    rt = dev_f32(root_t, (3,), "root_t").expand(*lead, 3).contiguous()
    if not state and torch.is_grad_enabled() and (lr.requires_grad or rt.requires_grad):
        return _FK.apply(topo, lr, rt)
    return _fk_launch(topo, lr, rt, state)


def local_rotation(topo: Topology, g_rot, state: bool = False):
    """kinematics.py:41-63 (state=False) / SkeletonState.local_rotation skeleton3d.py:460-484."""
    J = topo.num_joints
    g = dev_f32(g_rot, (J, 4), "g_rot")
    B = int(torch.Size(g.shape[:-2]).numel())
    out = torch.empty_like(g)
    fn = lib().rtg_state_local_rotation_f32 if state else lib().rtg_local_rotation_f32
    check(fn(topo.handle, ptr(g), B, ptr(out), stream_handle()))
    return out


def retarget_to(plan: RetargetPlan, rot, root_t, is_local: bool = True):
    """SkeletonState.retarget_to (skeleton3d.py:742-889) in one launch: the source state's rotations (B, J_s, 4) as
    the state stores them (local or global per ``is_local``) and root translations (B, 3) -> the target state's local
    rotations (B, J_t, 4) and root translations (B, 3).  Raises RtgError without a GPU: there is no CPU fallback."""
    require_gpu_rtg()
    Js, Jt = plan.num_source_joints, plan.num_target_joints
    r = dev_f32(rot, (Js, 4), "rotation")
    if r.dim() != 3:
        raise ValueError(f"rotation must be (B, {Js}, 4), got {tuple(r.shape)}")
    B = int(r.shape[0])
    t = dev_f32(root_t, (3,), "root_translation")
    if t.dim() > 2 or (t.dim() == 2 and t.shape[0] not in (1, B)):
        raise ValueError(f"root_translation must broadcast to ({B}, 3), got {tuple(t.shape)}")
    t = t.expand(B, 3).contiguous()
    if r.device != plan.device:
        raise ValueError(f"rotation is on {r.device}; this plan lives on {plan.device}")
    out_rot = torch.empty((B, Jt, 4), device=r.device, dtype=torch.float32)
    out_root = torch.empty((B, 3), device=r.device, dtype=torch.float32)
    check(lib().rtg_retarget_to_f32(plan.handle, ptr(r), ptr(t), int(bool(is_local)), B, ptr(out_rot), ptr(out_root),
                                    stream_handle()))
    return out_rot, out_root


def motion_sample(topo: Topology, mlib: MotionLib, rot, root_t, clip_ids, times, vec=None, normalize: bool = False,
                  want_global: bool = False, state: bool = False):
    """Sample a motion library at (clip, time) pairs in one launch (rtg.h rtg_motion_sample_f32): per query the two
    frames around ``time * fps`` of its clip, ``quat_slerp`` (transform3d.py:152-174) of every joint's local rotation
    (``quat_normalize`` after it with ``normalize``), torch's ``(1 - b) * a + b * c`` on the root translation and the
    ``vec`` rows, and with ``want_global`` the forward kinematics of the blended pose (SkeletonState's with ``state``).

    rot (F_total, J, 4), root_t (F_total, 3) and vec (F_total, K, 3) | None are the library's packed arrays, clip_ids
    (N) int32 and times (N) float32 the queries.  Returns (local_rot (N, J, 4), root_t (N, 3), vec (N, K, 3) | None,
    g_rot (N, J, 4) | None, g_pos (N, J, 3) | None) on the device.  A query whose clip id is outside 0..C-1 gives NaN
    rows.  Raises RtgError without a GPU: there is no CPU fallback."""
    dev = require_gpu_rtg()
    J, Ft = topo.num_joints, mlib.total_frames
    r = dev_f32(rot, (J, 4), "rot")
    t = dev_f32(root_t, (3,), "root_t")
    if tuple(r.shape) != (Ft, J, 4) or tuple(t.shape) != (Ft, 3):
        raise ValueError(f"rot / root_t must be ({Ft}, {J}, 4) / ({Ft}, 3), got {tuple(r.shape)} / {tuple(t.shape)}")
    v, K = None, 0
    if vec is not None:
        v = dev_f32(vec, (3,), "vec")
        if v.dim() != 3 or v.shape[0] != Ft or v.shape[1] < 1:
            raise ValueError(f"vec must be ({Ft}, K, 3) with K >= 1, got {tuple(v.shape)}")
        K = int(v.shape[1])
    c = clip_ids if isinstance(clip_ids, torch.Tensor) else torch.as_tensor(clip_ids)
    if c.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"clip_ids must be integers, got {c.dtype}")
    c = c.to(device=dev, dtype=torch.int32).contiguous()
    tm = dev_f32(times)
    if c.dim() != 1 or tm.shape != c.shape:
        raise ValueError(f"clip_ids / times must be (N,) each, got {tuple(c.shape)} / {tuple(tm.shape)}")
    if mlib.device != dev:
        raise ValueError(f"the queries are on {dev}; this library lives on {mlib.device}")
    N = int(c.shape[0])
    out_rot = torch.empty((N, J, 4), device=dev, dtype=torch.float32)
    out_root = torch.empty((N, 3), device=dev, dtype=torch.float32)
    out_vec = torch.empty((N, K, 3), device=dev, dtype=torch.float32) if v is not None else None
    g_rot = torch.empty((N, J, 4), device=dev, dtype=torch.float32) if want_global else None
    g_pos = torch.empty((N, J, 3), device=dev, dtype=torch.float32) if want_global else None
    flags = (_lib.MOTION_NORMALIZE if normalize else 0) | (_lib.MOTION_GLOBAL if want_global else 0) | \
        (_lib.MOTION_STATE if state else 0)
    check(lib().rtg_motion_sample_f32(topo.handle, mlib.handle, ptr(r), ptr(t), ptr(v), K, ptr(c), ptr(tm), N, flags,
                                      ptr(out_rot), ptr(out_root), ptr(out_vec), ptr(g_rot), ptr(g_pos),
                                      stream_handle()))
    return out_rot, out_root, out_vec, g_rot, g_pos


# what dof_motion_sample returns, device tensors: dof (N, J-1), dof_vel (N, J-1), root_rot (N, 4), root_t (N, 3),
# root_vel (N, 6) {linear, angular}, g_rot (N, J, 4), g_pos (N, J, 3), key_pos (N, K, 3), g_vel (N, J, 6) and key_vel
# (N, K, 6) {linear, angular}; the parts not asked for are None
DofMotionSampleResult = collections.namedtuple("DofMotionSampleResult",
                                               "dof dof_vel root_rot root_t root_vel g_rot g_pos key_pos g_vel key_vel",
                                               defaults=(None, None))


def dof_motion_sample(model, mlib: MotionLib, dof, root_rot, root_t, clip_ids, times, normalize: bool = False,
                      clip: bool = False, want_velocity: bool = True, want_global: bool = True, key_links=None,
                      want_link_velocity: bool = False, want_key_velocity: bool = False):
    """Sample a library of joint-angle clips at (clip, time) pairs in one launch (rtg.h rtg_dof_motion_sample_f32): per
    query the two frames around ``time * fps`` of its clip, torch's ``(1 - b) * a + b * c`` on the joint angles and the
    root translation, ``quat_slerp`` of the root rotation (``quat_normalize`` after it with ``normalize``), with
    ``want_velocity`` the forward differences of the bracketing frames over the frame time (joint velocities, root
    linear velocity) and SkeletonMotion's unfiltered angular velocity of the root pair, with ``want_global`` the
    forward kinematics of the blended angles (clamped to the model's limits with ``clip``), and with ``key_links`` (up
    to 32 joint indices, repeats allowed) those links' positions alone.  ``want_link_velocity`` adds every link's
    world-frame twist {linear, angular} as ``g_vel`` (N, J, 6) -- rtg.h rtg_dof_fk_vel_f32's rule on the launch's own
    angles, joint velocities and root twist -- and ``want_key_velocity`` the key links' as ``key_vel`` (N, K, 6); both
    need ``want_velocity``, and neither needs ``want_global``.

    dof (F_total, J-1), root_rot (F_total, 4) and root_t (F_total, 3) are the library's packed arrays, clip_ids (N)
    int32 and times (N) float32 the queries.  Returns a DofMotionSampleResult on the device.  A query whose clip id is
    outside 0..C-1 gives NaN rows.  Raises RtgError without a GPU: there is no CPU fallback."""
    import numpy as np
    if (want_link_velocity or want_key_velocity) and not want_velocity:
        raise ValueError("want_link_velocity / want_key_velocity need want_velocity: the link velocities come from the "
                         "sampled joint and root velocities")
    if want_key_velocity and (key_links is None or len(key_links) == 0):
        raise ValueError("want_key_velocity needs key_links")
    dev = require_gpu_rtg()
    nd, Ft = model.num_dofs, mlib.total_frames
    J = nd + 1
    d = dev_f32(dof, (nd,), "dof")
    rr = dev_f32(root_rot, (4,), "root_rot")
    rt = dev_f32(root_t, (3,), "root_t")
    if tuple(d.shape) != (Ft, nd) or tuple(rr.shape) != (Ft, 4) or tuple(rt.shape) != (Ft, 3):
        raise ValueError(f"dof / root_rot / root_t must be ({Ft}, {nd}) / ({Ft}, 4) / ({Ft}, 3), got {tuple(d.shape)} / "
                         f"{tuple(rr.shape)} / {tuple(rt.shape)}")
    c = clip_ids if isinstance(clip_ids, torch.Tensor) else torch.as_tensor(clip_ids)
    if c.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"clip_ids must be integers, got {c.dtype}")
    c = c.to(device=dev, dtype=torch.int32).contiguous()
    tm = dev_f32(times)
    if c.dim() != 1 or tm.shape != c.shape:
        raise ValueError(f"clip_ids / times must be (N,) each, got {tuple(c.shape)} / {tuple(tm.shape)}")
    if mlib.device != dev:
        raise ValueError(f"the queries are on {dev}; this library lives on {mlib.device}")
    if clip and not model.has_limits:
        raise ValueError("clip needs a model with DOF limits")
    keys = np.zeros(0, np.int32) if key_links is None else np.ascontiguousarray(np.asarray(key_links, np.int64).reshape(-1))
    K = int(keys.shape[0])
    if K > _lib.DOF_MOTION_MAX_KEY_LINKS:
        raise ValueError(f"{K} key links, at most {_lib.DOF_MOTION_MAX_KEY_LINKS}")
    if K and (keys.min() < 0 or keys.max() >= J):
        raise ValueError(f"key_links must lie in 0..{J - 1}, got {keys.tolist()}")
    keys = keys.astype(np.int32)
    N = int(c.shape[0])

    def out(*shape):
        return torch.empty((N,) + shape, device=dev, dtype=torch.float32)

    o_dof, o_rr, o_rt = out(nd), out(4), out(3)
    o_dv, o_rv = (out(nd), out(6)) if want_velocity else (None, None)
    g_rot, g_pos = (out(J, 4), out(J, 3)) if want_global else (None, None)
    key_pos = out(K, 3) if K else None
    g_vel = out(J, 6) if want_link_velocity else None
    key_vel = out(K, 6) if want_key_velocity else None
    flags = (_lib.DOF_MOTION_NORMALIZE if normalize else 0) | (_lib.DOF_MOTION_CLIP if clip else 0)
    if g_vel is not None or key_vel is not None:
        check(lib().rtg_dof_motion_sample_vel_f32(
            model.handle, mlib.handle, ptr(d), ptr(rr), ptr(rt), ptr(c), ptr(tm), N, flags,
            keys.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if K else None, K, ptr(o_dof), ptr(o_dv), ptr(o_rr),
            ptr(o_rt), ptr(o_rv), ptr(g_rot), ptr(g_pos), ptr(key_pos), ptr(g_vel), ptr(key_vel), stream_handle()))
        return DofMotionSampleResult(o_dof, o_dv, o_rr, o_rt, o_rv, g_rot, g_pos, key_pos, g_vel, key_vel)
    check(lib().rtg_dof_motion_sample_f32(model.handle, mlib.handle, ptr(d), ptr(rr), ptr(rt), ptr(c), ptr(tm), N, flags,
                                          keys.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if K else None, K,
                                          ptr(o_dof), ptr(o_dv), ptr(o_rr), ptr(o_rt), ptr(o_rv), ptr(g_rot), ptr(g_pos),
                                          ptr(key_pos), stream_handle()))
    return DofMotionSampleResult(o_dof, o_dv, o_rr, o_rt, o_rv, g_rot, g_pos, key_pos)


def dof_forward_kinematics(model, dof, root_rot, root_t, clip: bool = False):
    """HuForwardModel.forward_kinematics (hu_forward_model.py:17-33): joint angles (..., J-1) [or (..., J-1, 1)],
    root rotation (..., 4) [or (..., 1, 4)], root translation (..., 3) -> g_rot (..., J, 4), g_pos (..., J, 3)."""
    def _t(x):
        return x if isinstance(x, torch.Tensor) else torch.as_tensor(x)

    n = model.num_dofs
    d = _t(dof)
    if d.dim() >= 2 and d.shape[-1] == 1 and d.shape[-2] == n:
        d = d[..., 0]
    d = dev_f32(d, (n,), "motion_joint_angles")
    lead = d.shape[:-1]
    rr = _t(root_rot)
    if rr.dim() >= 2 and rr.shape[-2] == 1 and rr.shape[-1] == 4:
        rr = rr[..., 0, :]
    rr = dev_f32(rr, (4,), "motion_root_rotation").expand(*lead, 4).contiguous()
    rt = dev_f32(root_t, (3,), "motion_root_translation").expand(*lead, 3).contiguous()
    if torch.is_grad_enabled() and (d.requires_grad or rr.requires_grad or rt.requires_grad):
        return _DofFK.apply(model, bool(clip), d, rr, rt)
    return _dof_fk_launch(model, bool(clip), d, rr, rt)


def dof_link_velocity(model, dof, root_rot, root_t, dof_vel, root_vel=None, clip: bool = False,
                      want_pose: bool = True):
    """Link velocities from joint velocities in one launch (rtg.h rtg_dof_fk_vel_f32): joint angles and joint
    velocities (..., J-1) [or (..., J-1, 1)], root rotation (..., 4) [or (..., 1, 4)], root translation (..., 3) and the
    root twist ``root_vel`` (..., 6) {linear, angular}, world frame (None: zero) -> (g_rot (..., J, 4), g_pos
    (..., J, 3), g_vel (..., J, 6)), g_vel[..., j, :3] the world-frame linear velocity of link j's origin and
    g_vel[..., j, 3:] its angular velocity.  g_rot / g_pos are dof_forward_kinematics' bits, or None with
    ``want_pose=False`` (the same g_vel).  With ``clip`` a joint whose angle lies outside its limits does not turn.
    Not differentiable."""
    def _t(x):
        return x if isinstance(x, torch.Tensor) else torch.as_tensor(x)

    def _angles(x, name):
        x = _t(x)
        if x.dim() >= 2 and x.shape[-1] == 1 and x.shape[-2] == n:
            x = x[..., 0]
        return dev_f32(x.detach(), (n,), name)

    n = model.num_dofs
    if clip and not model.has_limits:
        raise ValueError("clip needs a model with DOF limits")
    d = _angles(dof, "motion_joint_angles")
    lead = d.shape[:-1]
    dv = _angles(dof_vel, "joint_velocities")
    if dv.shape != d.shape:
        raise ValueError(f"dof_vel must have dof's shape {tuple(d.shape)}, got {tuple(dv.shape)}")
    rr = _t(root_rot)
    if rr.dim() >= 2 and rr.shape[-2] == 1 and rr.shape[-1] == 4:
        rr = rr[..., 0, :]
    rr = dev_f32(rr.detach(), (4,), "motion_root_rotation").expand(*lead, 4).contiguous()
    rt = dev_f32(_t(root_t).detach(), (3,), "motion_root_translation").expand(*lead, 3).contiguous()
    rv = None
    if root_vel is not None:
        rv = dev_f32(_t(root_vel).detach(), (6,), "root_vel").expand(*lead, 6).contiguous()
    B = int(torch.Size(lead).numel())
    J = n + 1

    def out(*shape):
        return torch.empty(tuple(lead) + shape, device=d.device, dtype=torch.float32)

    g_rot, g_pos = (out(J, 4), out(J, 3)) if want_pose else (None, None)
    g_vel = out(J, 6)
    check(lib().rtg_dof_fk_vel_f32(model.handle, ptr(d), ptr(rr), ptr(rt), ptr(dv), ptr(rv), B, int(bool(clip)),
                                   ptr(g_rot), ptr(g_pos), ptr(g_vel), stream_handle()))
    return g_rot, g_pos, g_vel


def _dof_fk_launch(model, clip: bool, d, rr, rt):
    lead = d.shape[:-1]
    B = int(torch.Size(lead).numel())
    J = model.num_dofs + 1
    g_rot = torch.empty(tuple(lead) + (J, 4), device=d.device, dtype=torch.float32)
    g_pos = torch.empty(tuple(lead) + (J, 3), device=d.device, dtype=torch.float32)
    check(lib().rtg_dof_fk_f32(model.handle, ptr(d), ptr(rr), ptr(rt), B, int(clip), ptr(g_rot), ptr(g_pos),
                               stream_handle()))
    return g_rot, g_pos


class _DofFK(torch.autograd.Function):
    """dof_forward_kinematics with its HIP adjoint (rtg_dof_fk_backward_f32); the forward is the same launch.  The
    clip is straight-through, as in the reference (hu_forward_model.py:27-33)."""

    @staticmethod
    def forward(ctx, model, clip, d, rr, rt):
        ctx.set_materialize_grads(False)
        g_rot, g_pos = _dof_fk_launch(model, clip, d, rr, rt)
        ctx.model, ctx.clip = model, clip
        ctx.save_for_backward(d, g_rot)
        return g_rot, g_pos

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_g_rot, grad_g_pos):
        need_d, need_rr, need_rt = ctx.needs_input_grad[2:5]
        if (grad_g_rot is None and grad_g_pos is None) or not (need_d or need_rr or need_rt):
            return None, None, None, None, None
        d, g_rot = ctx.saved_tensors
        lead = tuple(d.shape[:-1])
        B = int(torch.Size(lead).numel())
        ggr, ggp = _cotangent(grad_g_rot), _cotangent(grad_g_pos)
        g_d = torch.empty_like(d) if need_d else None
        g_rr = torch.empty(lead + (4,), device=d.device, dtype=torch.float32) if need_rr else None
        g_rt = torch.empty(lead + (3,), device=d.device, dtype=torch.float32) if need_rt else None
        if d.shape[-1] == 0 and g_rr is None and g_rt is None:   # a one-joint model has no angles: nothing to compute
            return None, None, g_d, None, None
        check(lib().rtg_dof_fk_backward_f32(ctx.model.handle, ptr(d), ptr(g_rot), ptr(ggr), ptr(ggp), B, int(ctx.clip),
                                            ptr(g_d), ptr(g_rr), ptr(g_rt), stream_handle()))
        return None, None, g_d, g_rr, g_rt


DOF_FIT_MAX_ITERS = 4096   # rtg.h RTG_DOF_FIT_MAX_ITERS


def _as_tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(x)


def _fit_inputs(model, target_pos, root_rot, root_t, dof, weight):
    """The fit's inputs as contiguous float32 device tensors: target_pos (..., J, 3) sets the batch shape; the angles
    (..., J-1) [or (..., J-1, 1)], root rotation (..., 4) [or (..., 1, 4)] and translation (..., 3) as in
    dof_forward_kinematics; weight (J,) or None."""
    require_gpu_rtg()
    n = model.num_dofs
    tp = dev_f32(target_pos, (n + 1, 3), "target_pos")
    lead = tuple(tp.shape[:-2])
    if dof is None:
        d = torch.zeros(lead + (n,), device=tp.device, dtype=torch.float32)
    else:
        d = _as_tensor(dof)
        if d.dim() >= 2 and d.shape[-1] == 1 and d.shape[-2] == n:
            d = d[..., 0]
        d = dev_f32(d, (n,), "motion_joint_angles")
        if tuple(d.shape[:-1]) != lead:
            raise ValueError(f"motion_joint_angles {tuple(d.shape)} do not match target_pos {tuple(tp.shape)}")
    rr = _as_tensor(root_rot)
    if rr.dim() >= 2 and rr.shape[-2] == 1 and rr.shape[-1] == 4:
        rr = rr[..., 0, :]
    rr = dev_f32(rr, (4,), "motion_root_rotation").expand(*lead, 4).contiguous()
    rt = dev_f32(root_t, (3,), "motion_root_translation").expand(*lead, 3).contiguous()
    w = None
    if weight is not None:
        w = dev_f32(weight, (n + 1,), "weight")
        if w.dim() != 1:
            raise ValueError(f"weight must be ({n + 1},), got {tuple(w.shape)}")
    return tp, d, rr, rt, w


FIT_MAX_ROT_LINKS = 8   # rtg.h RTG_FIT_MAX_ROT_LINKS

Orient = collections.namedtuple("Orient", "joints K target_rot rot_weight")   # joints: the host int32 array of the call


def _orient_inputs(model, lead, rot_joints, target_rot, rot_weight):
    """The orientation targets of a fit, checked before the C ABI sees a pointer: rot_joints K <= 8 distinct joint
    indices in 0..J-1 (host integers: they travel in the launch's arguments); target_rot (..., K, 4) [x, y, z, w] over
    the batch shape ``lead``, as a contiguous float32 device tensor with 16-byte aligned rows (copied where it is not);
    rot_weight (K,) or None.  None when none of the three is given."""
    if rot_joints is None and target_rot is None and rot_weight is None:
        return None
    if rot_joints is None or target_rot is None:
        raise ValueError("orientation targets need both rot_joints and target_rot")
    import numpy as np
    if isinstance(rot_joints, torch.Tensor):
        rot_joints = rot_joints.detach().cpu().numpy()
    jn = np.asarray(rot_joints)
    if jn.ndim != 1 or (jn.size and not np.issubdtype(jn.dtype, np.integer)):
        raise ValueError(f"rot_joints must be a 1-D sequence of joint indices, got {rot_joints!r}")
    joints = [int(j) for j in jn]
    K, J = len(joints), model.num_dofs + 1
    if K > FIT_MAX_ROT_LINKS:
        raise ValueError(f"at most {FIT_MAX_ROT_LINKS} oriented links, got {K}")
    if any(not 0 <= j < J for j in joints) or len(set(joints)) != K:
        raise ValueError(f"rot_joints must be distinct joint indices in 0..{J - 1}, got {joints}")
    tr = _as_tensor(target_rot)
    if tr.dtype not in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        raise ValueError(f"target_rot must be floating point, got {tr.dtype}")
    tr = dev_f32(tr.detach(), (K, 4), "target_rot")
    if tuple(tr.shape[:-2]) != tuple(lead):
        raise ValueError(f"target_rot {tuple(tr.shape)} does not match the batch shape {tuple(lead)} of target_pos")
    if tr.data_ptr() % 16:
        tr = tr.clone()
    rw = None
    if rot_weight is not None:
        rw = dev_f32(rot_weight, (K,), "rot_weight")
        if rw.dim() != 1:
            raise ValueError(f"rot_weight must be ({K},), got {tuple(rw.shape)}")
    return Orient((ctypes.c_int32 * max(K, 1))(*joints), K, tr, rw)


FIT_PROJECT = 1   # rtg.h RTG_FIT_PROJECT

Prior = collections.namedtuple("Prior", "rows weight flags")   # rows / weight: device tensors or None


def _prior_inputs(model, d, prior, prior_weight, project):
    """The posture prior and the projection of a fit, checked before the C ABI sees a pointer: prior (..., J-1) [or
    (..., J-1, 1)] over the angles' own shape ``d.shape``, as a contiguous float32 device tensor (never part of the
    graph); prior_weight a number or (J-1,), None for ones; project needs a model with limits.  None when none of the
    three is given."""
    if prior is None and prior_weight is None and not project:
        return None
    if prior is None and prior_weight is not None:
        raise ValueError("prior_weight needs a prior")
    if project and not model.has_limits:
        raise ValueError("project needs a model with DOF limits")
    n = model.num_dofs
    rows = pw = None
    if prior is not None:
        p = _as_tensor(prior)
        if p.dtype not in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
            raise ValueError(f"prior must be floating point, got {p.dtype}")
        if p.dim() >= 2 and p.shape[-1] == 1 and p.shape[-2] == n:
            p = p[..., 0]
        rows = dev_f32(p.detach(), (n,), "prior")
        if tuple(rows.shape) != tuple(d.shape):
            raise ValueError(f"prior {tuple(rows.shape)} does not match the angles {tuple(d.shape)}")
    if prior_weight is not None:
        w = _as_tensor(prior_weight)
        if w.dim() == 0:
            w = w.reshape(1).expand(n)
        pw = dev_f32(w.detach(), (n,), "prior_weight")
        if pw.dim() != 1:
            raise ValueError(f"prior_weight must be a number or ({n},), got {tuple(pw.shape)}")
    return Prior(rows, pw, FIT_PROJECT if project else 0)


FIT_MAX_SPHERES, FIT_MAX_PAIRS = 16, 32   # rtg.h RTG_FIT_MAX_SPHERES, RTG_FIT_MAX_PAIRS

# what ops.apart builds: ``spec`` is the rtg_fit_apart of the call (a host struct; the other fields are the host arrays
# it points into, which also say what it holds: links (S,) int32, spheres (S,4) {offset, radius}, pairs (Pn,2) int32,
# pair_weight (Pn,) or None, plane (4,) {unit-length or not normal, h0} or None)
Apart = collections.namedtuple("Apart", "spec links spheres pairs pair_weight margin plane floor_mask floor_weight")


def apart(model, links, radii, offsets=None, pairs=None, pair_weight=None, margin: float = 0.0, floor=None,
          floor_links=None, floor_weight: float = 1.0):
    """The keep-apart term of pose_fit and its relatives (rtg_dof_fit_apart_f32), built once and passed as ``apart=``:
    S <= 16 spheres riding on links, Pn <= 32 pairs of them that are pushed apart where they overlap, and a floor.

    ``model``: a DofModel, or anything with the tree's ``parents`` (or ``parent_indices``) and, for links given by
    name, ``node_names``.  ``links`` (S) names or joint indices, one per sphere (a link may carry several); ``radii``
    (S) or a number; ``offsets`` (S, 3) in the link's frame, default zeros (a sphere at the link's origin moves with
    the link's position alone and adds no rotation gradient).  ``pairs`` (Pn, 2) sphere indices; None: every pair of
    spheres whose links are neither the same nor parent and child (neighbours overlap by construction) -- it raises
    when that is more than 32.  ``pair_weight`` (Pn) or a number, None for ones.  Pair (a, b) adds
    pair_weight max(0, r_a + r_b + margin - |c_a - c_b|)^2 to a frame's loss.  ``floor``: (n_x, n_y, n_z, h0), the
    half-space n . x >= h0 (n of any non-zero length); the spheres on ``floor_links`` (None: every sphere) add
    floor_weight max(0, r + h0 - n . c)^2.  Nothing here is differentiable.

    No radii are shipped: the repository holds Hu's skeleton only, no collision geometry -- measure them on the robot
    or take them from its URDF."""
    import numpy as np
    parents = getattr(model, "parents", None)
    if parents is None and getattr(model, "topo", None) is not None:
        parents = model.topo.parents
    if parents is None:
        parents = getattr(model, "parent_indices", None)
    if parents is None:
        raise ValueError("apart needs the tree: a DofModel, or an object with parents")
    par = [int(x) for x in (parents.tolist() if hasattr(parents, "tolist") else parents)]
    J = len(par)
    names = list(getattr(model, "node_names", None) or [])

    def joint(link, what):
        if isinstance(link, str):
            if link not in names:
                raise ValueError(f"{what}: the skeleton has no node named {link!r}")
            return names.index(link)
        j = int(link)
        if not 0 <= j < J:
            raise ValueError(f"{what}: joint {j} is outside 0..{J - 1}")
        return j

    lk = np.asarray([joint(x, "links") for x in links], np.int32)
    S = len(lk)
    if S > FIT_MAX_SPHERES:
        raise ValueError(f"at most {FIT_MAX_SPHERES} spheres, got {S}")
    r = np.broadcast_to(np.asarray(radii, np.float32), (S,)) if np.ndim(radii) == 0 else np.asarray(radii, np.float32)
    off = np.zeros((S, 3), np.float32) if offsets is None else np.asarray(offsets, np.float32)
    if r.shape != (S,) or off.shape != (S, 3):
        raise ValueError(f"radii must be ({S},) and offsets ({S}, 3), got {r.shape} and {off.shape}")
    if not (np.isfinite(r).all() and (r >= 0).all() and np.isfinite(off).all()):
        raise ValueError("radii must be finite and not negative, offsets finite")
    spheres = np.ascontiguousarray(np.concatenate([off, r[:, None]], axis=1), np.float32)
    if pairs is None:
        related = lambda a, b: lk[a] == lk[b] or par[lk[a]] == lk[b] or par[lk[b]] == lk[a]
        pr = [(a, b) for a in range(S) for b in range(a + 1, S) if not related(a, b)]
        if len(pr) > FIT_MAX_PAIRS:
            raise ValueError(f"{S} spheres give {len(pr)} pairs of unrelated links, at most {FIT_MAX_PAIRS}: pass pairs")
    else:
        pr = [(int(a), int(b)) for a, b in pairs]
        if len(pr) > FIT_MAX_PAIRS:
            raise ValueError(f"at most {FIT_MAX_PAIRS} pairs, got {len(pr)}")
        if any(not (0 <= a < S and 0 <= b < S) or a == b for a, b in pr):
            raise ValueError(f"pairs must join two different spheres in 0..{S - 1}, got {pr}")
    pr = np.ascontiguousarray(np.asarray(pr, np.int32).reshape(-1, 2))
    Pn = len(pr)
    pw = None
    if pair_weight is not None:
        pw = np.ascontiguousarray(np.broadcast_to(np.asarray(pair_weight, np.float32), (Pn,)))
        if not (np.isfinite(pw).all() and (pw >= 0).all()):
            raise ValueError("pair_weight must be finite and not negative")
    margin = float(margin)
    if not np.isfinite(margin):
        raise ValueError(f"margin must be finite, got {margin}")
    plane, mask = None, 0
    if floor is not None:
        plane = np.ascontiguousarray(np.asarray(floor, np.float32).reshape(-1))
        if plane.shape != (4,) or not np.isfinite(plane).all() or not np.abs(plane[:3]).max() > 0:
            raise ValueError(f"floor must be four finite numbers (n_x, n_y, n_z, h0) with n not zero, got {floor!r}")
        if floor_links is None:
            mask = (1 << S) - 1
        else:
            on = {joint(x, "floor_links") for x in floor_links}
            mask = sum(1 << i for i in range(S) if int(lk[i]) in on)
    elif floor_links is not None:
        raise ValueError("floor_links needs a floor")
    floor_weight = float(floor_weight)
    if not (np.isfinite(floor_weight) and floor_weight >= 0):
        raise ValueError(f"floor_weight must be finite and not negative, got {floor_weight}")
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    at = lambda a, t: a.ctypes.data_as(t) if a is not None and a.size else None
    spec = _lib.FitApart(S, at(lk, ip), at(spheres, fp), Pn, at(pr, ip), at(pw, fp), margin, at(plane, fp), mask,
                         floor_weight)
    return Apart(spec, lk, spheres, pr, pw, margin, plane, mask, floor_weight)


def _apart_input(apart):
    """``apart=`` of the fits: None, or what ops.apart built."""
    if apart is not None and not isinstance(apart, Apart):
        raise ValueError("apart must be built with ops.apart")
    return apart


Robust = collections.namedtuple("Robust", "rows scale")   # rows: the (..., J) device tensor or None; scale: a float


def _robust_inputs(model, target_pos, frame_weight, robust_scale):
    """The per-frame keypoint weights and the robust scale of a fit, checked before anything asks for the device:
    frame_weight (..., J) over the batch shape of target_pos (..., J, 3), real (bool and integer masks are converted);
    robust_scale None or 0 for the quadratic loss, else a finite positive number of metres.  None when neither is given:
    the launch without them.  _robust_rows then puts the rows on the device."""
    import math
    import numbers
    lead = tuple(_as_tensor(target_pos).shape[:-2])
    scale = 0.0 if robust_scale is None else robust_scale
    if isinstance(scale, torch.Tensor) and scale.numel() == 1:
        scale = scale.item()
    if isinstance(scale, bool) or not isinstance(scale, numbers.Real):
        raise ValueError(f"robust_scale must be a number, got {robust_scale!r}")
    scale = float(scale)
    if not math.isfinite(scale) or scale < 0.0:
        raise ValueError(f"robust_scale must be 0 or a finite positive number, got {robust_scale!r}")
    rows = None
    if frame_weight is not None:
        fw = _as_tensor(frame_weight)
        if fw.is_complex():
            raise ValueError(f"frame_weight must be real, got {fw.dtype}")
        J = model.num_dofs + 1
        if fw.dim() < 1 or fw.shape[-1] != J or tuple(fw.shape[:-1]) != tuple(lead):
            raise ValueError(f"frame_weight {tuple(fw.shape)} does not match the batch shape {tuple(lead)} of target_pos "
                             f"with {J} keypoints")
        rows = fw.detach()
    if rows is None and scale == 0.0:
        return None
    return Robust(rows, scale)


def _robust_rows(robust):
    """_robust_inputs' result with the rows as a contiguous float32 device tensor (never part of the graph)."""
    if robust is None or robust.rows is None:
        return robust
    return Robust(dev_f32(robust.rows, (robust.rows.shape[-1],), "frame_weight"), robust.scale)


def _fit_state(model, d, dof0, iters, state):
    """What dof_fit and pose_fit share around their launches: ``iters`` range-checked; the angles' optimiser state
    ``(m, v, step)`` -- fresh (zeros, 0) for ``state`` None, else the caller's, copied (the launch updates it in
    place); and ``as_dof0``, which gives an angle-shaped result (or None) the trailing 1 of a ``dof0`` passed as
    (..., J-1, 1).  Returns (iters, m, v, step, as_dof0)."""
    iters = int(iters)
    if not 0 <= iters <= DOF_FIT_MAX_ITERS:
        raise ValueError(f"iters must be in 0..{DOF_FIT_MAX_ITERS}, got {iters}")
    if state is None:
        m, v, step = torch.zeros_like(d), torch.zeros_like(d), 0
    else:
        m, v, step = state
        m, v = (dev_f32(x, (model.num_dofs,), "state").reshape(d.shape).clone() for x in (m, v))
        step = int(step)
    tail = dof0 is not None and tuple(_as_tensor(dof0).shape) == tuple(d.shape) + (1,)
    return iters, m, v, step, (lambda t: t.unsqueeze(-1) if tail and t is not None else t)


def _fit_launch(model, clip, tp, w, rr, rt, d, iters=0, lr=0.0, betas=(0.9, 0.999), eps=1e-8, step0=0, m=None, v=None,
                want_dof=False, want_loss=True, want_grad=False):
    """rtg_dof_fit_f32 on prepared tensors; m, v are updated in place.  Returns (dof_out, loss, grad), None where not
    asked for."""
    lead = tuple(tp.shape[:-2])
    B = int(torch.Size(lead).numel())
    out = torch.empty_like(d) if want_dof else None
    loss = torch.empty(lead, device=d.device, dtype=torch.float32) if want_loss else None
    grad = torch.empty_like(d) if want_grad else None
    check(lib().rtg_dof_fit_f32(model.handle, ptr(tp), ptr(w), ptr(rr), ptr(rt), ptr(d), B, int(bool(clip)), int(iters),
                                float(lr), float(betas[0]), float(betas[1]), float(eps), int(step0), ptr(m), ptr(v),
                                ptr(out), ptr(loss), ptr(grad), stream_handle()))
    return out, loss, grad


def dof_fit(model, target_pos, root_rot, root_t, dof0=None, weight=None, iters: int = 32, lr: float = 0.02,
            betas=(0.9, 0.999), eps: float = 1e-8, clip: bool = False, state=None, return_grad: bool = False,
            rot_joints=None, target_rot=None, rot_weight=None, prior=None, prior_weight=None, project: bool = False,
            apart=None, frame_weight=None, robust_scale=None):
    """Fit the joint angles of a DofModel to target keypoints: ``iters`` steps of torch.optim.Adam (no weight decay, no
    amsgrad) on L_f = sum_j weight[j] |P_j(a_f) - target_pos[f, j]|^2, P the positions of dof_forward_kinematics --
    forward model, loss, gradient and optimiser in ONE launch (rtg_dof_fit_f32).

    target_pos (..., J, 3); root_rot / root_t as in dof_forward_kinematics (given, not fitted); dof0 (..., J-1) [or
    (..., J-1, 1)] the start, default zeros; weight (J,) or None for all ones.  ``state`` is the optimiser's
    ``(m, v, step)`` from an earlier call (None: a fresh optimiser); it is returned updated, so calls chain: two calls
    of n steps give the bits of one call of 2n.  The iterate is not projected onto the limits (``clip`` only clips
    inside the forward model, straight-through) unless ``project`` is set; without it the final pose is the clamp the
    caller applies.

    Returns ``(dof, loss, state)`` -- the angles after the last step (dof0's shape), the per-frame loss there (...),
    and the new state -- plus the gradient there (dof's shape) when ``return_grad``.  ``iters=0`` only evaluates.
    ``rot_joints``, ``target_rot``, ``rot_weight``: pose_fit's orientation targets, with the root given
    (rtg_dof_fit_orient_f32 with fit_root = 0; an oriented root then only adds to the loss).
    ``prior``, ``prior_weight``, ``project``: pose_fit's posture prior and projection (rtg_dof_fit_prior_f32 with
    fit_root = 0).  ``apart``: pose_fit's keep-apart spheres and floor (ops.apart; rtg_dof_fit_apart_f32 with
    fit_root = 0).  ``frame_weight``, ``robust_scale``: pose_fit's per-frame keypoint weights and robust keypoint
    loss (rtg_dof_fit_robust_f32 with fit_root = 0).
    Raises RtgError without a GPU: there is no CPU fallback."""
    rob = _robust_inputs(model, target_pos, frame_weight, robust_scale)
    tp, d, rr, rt, w = _fit_inputs(model, target_pos, root_rot, root_t, dof0, weight)
    iters, m, v, step, as_dof0 = _fit_state(model, d, dof0, iters, state)
    orient = _orient_inputs(model, tuple(tp.shape[:-2]), rot_joints, target_rot, rot_weight)
    pri = _prior_inputs(model, d, prior, prior_weight, project)
    apart = _apart_input(apart)
    rob = _robust_rows(rob)
    if orient is None and pri is None and apart is None and rob is None:
        out, loss, grad = _fit_launch(model, clip, tp, w, rr, rt, d.detach(), iters, lr, betas, eps, step, m, v,
                                      want_dof=True, want_grad=bool(return_grad))
    else:   # the root is given: its state is neither read nor written, the buffer only pairs with m and v
        rs = torch.zeros(tuple(tp.shape[:-2]) + (14,), device=d.device, dtype=torch.float32)
        out, _, _, loss, grad, _ = _pose_launch(model, clip, 0, tp, w, rr, rt, d.detach(), iters, lr, 0.0, 0.0, betas, eps,
                                                step, m if m.numel() else rs, v if v.numel() else rs, rs,
                                                want_iterate=True, want_grad=bool(return_grad), orient=orient, prior=pri,
                                                apart=apart, robust=rob)
    res = (as_dof0(out), loss, (m, v, step + iters))
    return res + (as_dof0(grad),) if return_grad else res


def keypoint_loss(model, dof, target_pos, root_rot, root_t, weight=None, clip: bool = False, rot_joints=None,
                  target_rot=None, rot_weight=None, prior=None, prior_weight=None, apart=None, frame_weight=None,
                  robust_scale=None):
    """The per-frame keypoint loss L_f = sum_j weight[j] |P_j(dof_f) - target_pos[f, j]|^2 of dof_fit, (...), as the
    evaluate-only launch of rtg_dof_fit_f32.  Differentiable in ``dof`` (only): the launch computes the gradient
    along with the loss, and backward scales its rows by the upstream cotangent -- for callers who keep their own
    optimiser.  Under no_grad, or when dof does not require grad, it is the plain launch without the gradient.
    ``rot_joints``, ``target_rot``, ``rot_weight``: dof_fit's orientation targets.  ``prior``, ``prior_weight``: its
    posture term sum_d prior_weight[d] (dof_d - prior_d)^2 (the loss is not differentiable in them).  ``apart``: its
    keep-apart spheres and floor (ops.apart; not differentiable in the spec either).  ``frame_weight``,
    ``robust_scale``: its per-frame keypoint weights and robust keypoint loss (the gradient is the robust loss's; the
    frame weights are not differentiable)."""
    rob = _robust_inputs(model, target_pos, frame_weight, robust_scale)
    tp, d, rr, rt, w = _fit_inputs(model, target_pos, root_rot, root_t, dof, weight)
    orient = _orient_inputs(model, tuple(tp.shape[:-2]), rot_joints, target_rot, rot_weight)
    pri = _prior_inputs(model, d, prior, prior_weight, False)
    rob = _robust_rows(rob)
    if rob is not None:
        apart = _apart_input(apart)
        if torch.is_grad_enabled() and d.requires_grad:
            return _RobustPoseLoss.apply(model, bool(clip), 0, d, rr.detach(), rt.detach(), tp, w, orient, pri, apart, rob)
        return _pose_launch(model, clip, 0, tp, w, rr, rt, d.detach(), orient=orient, prior=pri, apart=apart,
                            robust=rob)[3]
    if _apart_input(apart) is not None:
        if torch.is_grad_enabled() and d.requires_grad:
            return _ApartPoseLoss.apply(model, bool(clip), 0, d, rr.detach(), rt.detach(), tp, w, orient, pri, apart)
        return _pose_launch(model, clip, 0, tp, w, rr, rt, d.detach(), orient=orient, prior=pri, apart=apart)[3]
    if pri is not None:
        if torch.is_grad_enabled() and d.requires_grad:
            return _PriorPoseLoss.apply(model, bool(clip), 0, d, rr.detach(), rt.detach(), tp, w, orient, pri)
        return _pose_launch(model, clip, 0, tp, w, rr, rt, d.detach(), orient=orient, prior=pri)[3]
    if orient is not None:
        if torch.is_grad_enabled() and d.requires_grad:
            return _OrientPoseLoss.apply(model, bool(clip), 0, d, rr.detach(), rt.detach(), tp, w, orient)
        return _pose_launch(model, clip, 0, tp, w, rr, rt, d.detach(), orient=orient)[3]
    if torch.is_grad_enabled() and d.requires_grad:
        return _KeypointLoss.apply(model, bool(clip), d, tp, rr, rt, w)
    return _fit_launch(model, clip, tp, w, rr, rt, d.detach())[1]


class _KeypointLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, clip, d, tp, rr, rt, w):
        _, loss, grad = _fit_launch(model, clip, tp, w, rr, rt, d, want_grad=True)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return None, None, grad * grad_loss.unsqueeze(-1), None, None, None, None


FIT_ROOT_T, FIT_ROOT_ROT = 1, 2   # rtg.h RTG_FIT_ROOT_*

PoseFit = collections.namedtuple("PoseFit", "dof root_rot root_t loss state")
PoseFitGrad = collections.namedtuple("PoseFitGrad", "dof root_rot root_t loss state grad grad_root")


def _pose_launch(model, clip, fit_root, tp, w, rr, rt, d, iters=0, lr=0.0, lr_root_t=0.0, lr_root_rot=0.0,
                 betas=(0.9, 0.999), eps=1e-8, step0=0, m=None, v=None, root_state=None, want_iterate=False,
                 want_loss=True, want_grad=False, orient=None, prior=None, apart=None, robust=None):
    """rtg_dof_fit_root_f32 -- with ``orient`` (an Orient) rtg_dof_fit_orient_f32, with ``prior`` (a Prior)
    rtg_dof_fit_prior_f32, with ``apart`` (an Apart) rtg_dof_fit_apart_f32, with ``robust`` (a Robust)
    rtg_dof_fit_robust_f32 -- on prepared tensors; m, v, root_state are updated in place.  Returns (dof_out, root_rot_out, root_t_out, loss, grad, grad_root), None where
    not asked for."""
    lead = tuple(tp.shape[:-2])
    B = int(torch.Size(lead).numel())
    new = lambda like, *tail: torch.empty(lead + tail, device=like.device, dtype=torch.float32)
    out, rr_out, rt_out = (torch.empty_like(d), torch.empty_like(rr), torch.empty_like(rt)) if want_iterate else (None,) * 3
    loss = new(d) if want_loss else None
    grad, grad_root = (torch.empty_like(d), new(d, 7)) if want_grad else (None, None)
    tail = (ptr(rr), ptr(rt), ptr(d), B, int(bool(clip)), int(fit_root), int(iters), float(lr), float(lr_root_t),
            float(lr_root_rot), float(betas[0]), float(betas[1]), float(eps), int(step0), ptr(m), ptr(v), ptr(root_state),
            ptr(out), ptr(rr_out), ptr(rt_out), ptr(loss), ptr(grad), ptr(grad_root), stream_handle())
    if robust is not None:
        o = orient if orient is not None else Orient(None, 0, None, None)
        h = prior if prior is not None else Prior(None, None, 0)
        check(lib().rtg_dof_fit_robust_f32(model.handle, ptr(tp), ptr(w), o.joints, ptr(o.target_rot), ptr(o.rot_weight),
                                           o.K, ptr(h.rows), ptr(h.weight), h.flags, *tail[:-1],
                                           ctypes.byref(apart.spec) if apart is not None else None, ptr(robust.rows),
                                           robust.scale, tail[-1]))
    elif apart is not None:
        o = orient if orient is not None else Orient(None, 0, None, None)
        h = prior if prior is not None else Prior(None, None, 0)
        check(lib().rtg_dof_fit_apart_f32(model.handle, ptr(tp), ptr(w), o.joints, ptr(o.target_rot), ptr(o.rot_weight),
                                          o.K, ptr(h.rows), ptr(h.weight), h.flags, *tail[:-1], ctypes.byref(apart.spec),
                                          tail[-1]))
    elif prior is not None:
        o = orient if orient is not None else Orient(None, 0, None, None)
        check(lib().rtg_dof_fit_prior_f32(model.handle, ptr(tp), ptr(w), o.joints, ptr(o.target_rot), ptr(o.rot_weight),
                                          o.K, ptr(prior.rows), ptr(prior.weight), prior.flags, *tail))
    elif orient is None:
        check(lib().rtg_dof_fit_root_f32(model.handle, ptr(tp), ptr(w), *tail))
    else:
        check(lib().rtg_dof_fit_orient_f32(model.handle, ptr(tp), ptr(w), orient.joints, ptr(orient.target_rot),
                                           ptr(orient.rot_weight), orient.K, *tail))
    return out, rr_out, rt_out, loss, grad, grad_root


def pose_fit(model, target_pos, root_rot0, root_t0, dof0=None, weight=None, iters: int = 32, lr: float = 0.02,
             lr_root_t=None, lr_root_rot=None, fit_root_t: bool = True, fit_root_rot: bool = True, betas=(0.9, 0.999),
             eps: float = 1e-8, clip: bool = False, state=None, return_grad: bool = False, rot_joints=None,
             target_rot=None, rot_weight=None, prior=None, prior_weight=None, project: bool = False, apart=None,
             frame_weight=None, robust_scale=None):
    """dof_fit with the floating base among the parameters: the joint angles and -- where ``fit_root_t`` /
    ``fit_root_rot`` -- the root translation and rotation of every frame, fitted to target keypoints by ``iters`` steps
    of torch.optim.Adam with three parameter groups (``lr`` for the angles, ``lr_root_t``, ``lr_root_rot``; None: ``lr``)
    in ONE launch (rtg_dof_fit_root_f32).  A fitted rotation enters the forward model as q / |q| (no sign flip), its
    gradient goes through that normalisation and the iterate is renormalised after each step; a block that is not
    fitted is given, as in dof_fit (a given rotation is used unnormalised).

    target_pos (..., J, 3); root_rot0 (..., 4) [or (..., 1, 4)] / root_t0 (..., 3): the start; dof0 (..., J-1) [or
    (..., J-1, 1)], default zeros; weight (J,) or None.  ``state`` is ``(m, v, root_state, step)`` from an earlier call
    (None: a fresh optimiser), root_state (..., 14) = {m_t, m_q, v_t, v_q}; it is returned updated, and calls chain:
    two calls of n steps give the bits of one call of 2n.

    Orientation targets (rtg_dof_fit_orient_f32, still one launch): ``rot_joints`` K <= 8 distinct joint indices,
    ``target_rot`` (..., K, 4) [x, y, z, w] their global rotations (any norm, either sign), ``rot_weight`` (K,) or
    None for ones.  The loss gains sum_k rot_weight[k] 4 (1 - <G_k, target_k / |target_k|>^2) -- the squared chord
    (2 sin(theta/2))^2 of the angle between the link's rotation and its target, theta^2 for small angles -- which is what
    poses leaf joints (wrists, ankles, the head) and a link's twist; positions alone give those DOFs a gradient of
    exactly 0.  The term is stationary at theta = pi.  With none of the three given this is the position-only launch.

    Posture prior and projection (rtg_dof_fit_prior_f32, still one launch): ``prior`` (..., J-1) [or (..., J-1, 1)]
    adds sum_d prior_weight[d] (a_d - prior_d)^2 to the loss, a the iterate itself (not the clamped angle of ``clip``),
    ``prior_weight`` a number or (J-1,), None for ones: what holds an unobserved DOF or a redundant chain's swivel to a
    rest pose or to the last frame's solution (``prior=dof0`` is "stay near where you started").  ``project``: each
    angle is clamped to its limits after its Adam step (the loop ``opt.step(); a.clamp_(lower, upper)``; the moments are
    not touched), so the iterate cannot run away past a limit under ``clip``'s straight-through gradient; it needs a
    model with limits.  Without ``project`` the iterate is not projected.  The root is not regularised here:
    weight[0] with target_pos[..., 0, :] is a prior on its translation, an orientation target on joint 0 on its
    rotation.  With none of the three given this is the launch without them, bit for bit.

    Keep-apart spheres and a floor (rtg_dof_fit_apart_f32, still one launch): ``apart``, built once with ops.apart --
    spheres riding on links, pairs of them pushed apart where they overlap by pair_weight max(0, r_a + r_b + margin -
    |c_a - c_b|)^2, and spheres held above a plane by floor_weight max(0, r + h0 - n . c)^2.  It is what keeps a wrist
    out of the torso, one gripper out of the other and an ankle above the ground when the keypoints come from a body of
    other proportions.  The term acts on the iterate inside the launch; None is the launch without it, bit for bit.

    Per-frame keypoint weights and a robust keypoint loss (rtg_dof_fit_robust_f32, still one launch): ``frame_weight``
    (..., J) over target_pos's batch shape multiplies ``weight`` per frame and keypoint -- a tracker's confidences, a
    foot held hard while it is in contact -- and a keypoint whose frame weight is 0 is skipped altogether: it adds
    nothing and pulls nothing whatever its target row holds, NaN included (a dropped frame is a row of zeros).
    ``robust_scale`` = delta > 0 (metres) replaces |d|^2 in the keypoint term by the pseudo-Huber
    2 |d|^2 / (sqrt(1 + |d|^2 / delta^2) + 1): quadratic for |d| << delta, 2 delta |d| far out, so a glitched marker
    half a metre off no longer drags its limb.  The other terms are unchanged.  The frame weights are used as given
    (not checked, negative ones included).  With neither given this is the launch without them, bit for bit.

    Returns the named tuple ``(dof, root_rot, root_t, loss, state)`` -- the iterate after the last step (root_rot
    (..., 4), unit where fitted), the per-frame loss there -- plus ``grad`` (dof's shape) and ``grad_root`` (..., 7) =
    {dL/dt, dL/dq} there when ``return_grad``.  ``iters=0`` only evaluates.  Raises RtgError without a GPU: there is
    no CPU fallback."""
    rob = _robust_inputs(model, target_pos, frame_weight, robust_scale)
    tp, d, rr, rt, w = _fit_inputs(model, target_pos, root_rot0, root_t0, dof0, weight)
    iters, m, v, step, as_dof0 = _fit_state(model, d, dof0, iters, None if state is None else (*state[:2], state[3]))
    lead = tuple(tp.shape[:-2])
    if state is None:
        rs = torch.zeros(lead + (14,), device=d.device, dtype=torch.float32)
    else:
        rs = dev_f32(state[2], (14,), "root_state").reshape(lead + (14,)).clone()
    fit_root = (FIT_ROOT_T if fit_root_t else 0) | (FIT_ROOT_ROT if fit_root_rot else 0)
    orient = _orient_inputs(model, lead, rot_joints, target_rot, rot_weight)
    pri = _prior_inputs(model, d, prior, prior_weight, project)
    rob = _robust_rows(rob)
    # (a one-joint model has no angle moments: their arguments only say that a state is given)
    out, rr_out, rt_out, loss, grad, grad_root = _pose_launch(
        model, clip, fit_root, tp, w, rr.detach(), rt.detach(), d.detach(), iters, lr,
        lr if lr_root_t is None else lr_root_t, lr if lr_root_rot is None else lr_root_rot, betas, eps, step,
        m if m.numel() else rs, v if v.numel() else rs, rs, want_iterate=True, want_grad=bool(return_grad),
        orient=orient, prior=pri, apart=_apart_input(apart), robust=rob)
    new_state = (m, v, rs, step + iters)
    if return_grad:
        return PoseFitGrad(as_dof0(out), rr_out, rt_out, loss, new_state, as_dof0(grad), grad_root)
    return PoseFit(as_dof0(out), rr_out, rt_out, loss, new_state)


def pose_loss(model, dof, root_rot, root_t, target_pos, weight=None, clip: bool = False, normalize_root: bool = True,
              rot_joints=None, target_rot=None, rot_weight=None, prior=None, prior_weight=None, apart=None,
              frame_weight=None, robust_scale=None):
    """The per-frame keypoint loss of pose_fit, (...), as the evaluate-only launch of rtg_dof_fit_root_f32,
    differentiable in ``dof``, ``root_rot`` and ``root_t``: the launch computes the three gradients along with the
    loss and backward scales their rows by the upstream cotangent -- for callers who keep their own optimiser.
    ``normalize_root``: the root rotation enters as q / |q| and its gradient is tangent (pose_fit's model of a fitted
    rotation); False: as given, like keypoint_loss.  Under no_grad, or when no input requires grad, it is the plain
    launch without the gradients.  ``rot_joints``, ``target_rot``, ``rot_weight``: pose_fit's orientation targets;
    ``prior``, ``prior_weight``: its posture term; ``apart``: its keep-apart spheres and floor (ops.apart) (the loss is
    not differentiable in any of them); ``frame_weight``, ``robust_scale``: its per-frame keypoint weights and robust
    keypoint loss (the gradients are the robust loss's; the frame weights are not differentiable)."""
    rob = _robust_inputs(model, target_pos, frame_weight, robust_scale)
    tp, d, rr, rt, w = _fit_inputs(model, target_pos, root_rot, root_t, dof, weight)
    fit_root = FIT_ROOT_ROT if normalize_root else 0   # no step is taken: the mask only selects the model
    orient = _orient_inputs(model, tuple(tp.shape[:-2]), rot_joints, target_rot, rot_weight)
    pri = _prior_inputs(model, d, prior, prior_weight, False)
    rob = _robust_rows(rob)
    if rob is not None:
        apart = _apart_input(apart)
        if torch.is_grad_enabled() and (d.requires_grad or rr.requires_grad or rt.requires_grad):
            return _RobustPoseLoss.apply(model, bool(clip), fit_root, d, rr, rt, tp, w, orient, pri, apart, rob)
        return _pose_launch(model, clip, fit_root, tp, w, rr.detach(), rt.detach(), d.detach(), orient=orient, prior=pri,
                            apart=apart, robust=rob)[3]
    if _apart_input(apart) is not None:
        if torch.is_grad_enabled() and (d.requires_grad or rr.requires_grad or rt.requires_grad):
            return _ApartPoseLoss.apply(model, bool(clip), fit_root, d, rr, rt, tp, w, orient, pri, apart)
        return _pose_launch(model, clip, fit_root, tp, w, rr.detach(), rt.detach(), d.detach(), orient=orient, prior=pri,
                            apart=apart)[3]
    if pri is not None:
        if torch.is_grad_enabled() and (d.requires_grad or rr.requires_grad or rt.requires_grad):
            return _PriorPoseLoss.apply(model, bool(clip), fit_root, d, rr, rt, tp, w, orient, pri)
        return _pose_launch(model, clip, fit_root, tp, w, rr.detach(), rt.detach(), d.detach(), orient=orient, prior=pri)[3]
    if torch.is_grad_enabled() and (d.requires_grad or rr.requires_grad or rt.requires_grad):
        if orient is not None:
            return _OrientPoseLoss.apply(model, bool(clip), fit_root, d, rr, rt, tp, w, orient)
        return _PoseLoss.apply(model, bool(clip), fit_root, d, rr, rt, tp, w)
    return _pose_launch(model, clip, fit_root, tp, w, rr.detach(), rt.detach(), d.detach(), orient=orient)[3]


class _PoseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, clip, fit_root, d, rr, rt, tp, w):
        _, _, _, loss, grad, grad_root = _pose_launch(model, clip, fit_root, tp, w, rr, rt, d, want_grad=True)
        ctx.save_for_backward(grad, grad_root)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        grad, grad_root = ctx.saved_tensors
        c = grad_loss.unsqueeze(-1)
        return None, None, None, grad * c, grad_root[..., 3:] * c, grad_root[..., :3] * c, None, None


class _OrientPoseLoss(torch.autograd.Function):
    """_PoseLoss with orientation targets: the evaluate-only launch of rtg_dof_fit_orient_f32."""
    @staticmethod
    def forward(ctx, model, clip, fit_root, d, rr, rt, tp, w, orient):
        _, _, _, loss, grad, grad_root = _pose_launch(model, clip, fit_root, tp, w, rr, rt, d, want_grad=True,
                                                      orient=orient)
        ctx.save_for_backward(grad, grad_root)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        grad, grad_root = ctx.saved_tensors
        c = grad_loss.unsqueeze(-1)
        return None, None, None, grad * c, grad_root[..., 3:] * c, grad_root[..., :3] * c, None, None, None


class _PriorPoseLoss(torch.autograd.Function):
    """_OrientPoseLoss (orient may be None) with the posture term: the evaluate-only launch of rtg_dof_fit_prior_f32."""
    @staticmethod
    def forward(ctx, model, clip, fit_root, d, rr, rt, tp, w, orient, prior):
        _, _, _, loss, grad, grad_root = _pose_launch(model, clip, fit_root, tp, w, rr, rt, d, want_grad=True,
                                                      orient=orient, prior=prior)
        ctx.save_for_backward(grad, grad_root)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        grad, grad_root = ctx.saved_tensors
        c = grad_loss.unsqueeze(-1)
        return None, None, None, grad * c, grad_root[..., 3:] * c, grad_root[..., :3] * c, None, None, None, None


class _ApartPoseLoss(torch.autograd.Function):
    """_PriorPoseLoss (orient and prior may be None) with the keep-apart term: the evaluate-only launch of
    rtg_dof_fit_apart_f32."""
    @staticmethod
    def forward(ctx, model, clip, fit_root, d, rr, rt, tp, w, orient, prior, apart):
        _, _, _, loss, grad, grad_root = _pose_launch(model, clip, fit_root, tp, w, rr, rt, d, want_grad=True,
                                                      orient=orient, prior=prior, apart=apart)
        ctx.save_for_backward(grad, grad_root)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        grad, grad_root = ctx.saved_tensors
        c = grad_loss.unsqueeze(-1)
        return None, None, None, grad * c, grad_root[..., 3:] * c, grad_root[..., :3] * c, None, None, None, None, None


class _RobustPoseLoss(torch.autograd.Function):
    """_ApartPoseLoss (orient, prior and apart may be None) with the per-frame weights and the robust keypoint loss:
    the evaluate-only launch of rtg_dof_fit_robust_f32."""
    @staticmethod
    def forward(ctx, model, clip, fit_root, d, rr, rt, tp, w, orient, prior, apart, robust):
        _, _, _, loss, grad, grad_root = _pose_launch(model, clip, fit_root, tp, w, rr, rt, d, want_grad=True,
                                                      orient=orient, prior=prior, apart=apart, robust=robust)
        ctx.save_for_backward(grad, grad_root)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        grad, grad_root = ctx.saved_tensors
        c = grad_loss.unsqueeze(-1)
        return (None, None, None, grad * c, grad_root[..., 3:] * c, grad_root[..., :3] * c) + (None,) * 6


def rescale_motion(topo: Topology, motion, dir=None):
    """Retarget.rescale_motion_to_standard_size (retarget/main.py:37-47) after coord_transform(dir) (:170)."""
    J = topo.num_joints
    m = dev_f32(motion, (J, 3), "motion_global_translation")
    B = int(torch.Size(m.shape[:-2]).numel())
    out = torch.empty_like(m)
    d = None
    if dir is not None:
        import numpy as np
        dv = np.ascontiguousarray(np.asarray(dir.cpu() if isinstance(dir, torch.Tensor) else dir, np.float32).reshape(3))
        d = dv.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    check(lib().rtg_rescale_motion_f32(topo.handle, ptr(m), B, d, ptr(out), stream_handle()))
    return out


def fit_targets(plan: FitTargetsPlan, src_pos):
    """Keypoint targets for the pose fit from mocap positions of a body of other proportions, in one launch (rtg.h
    rtg_fit_targets_f32): source positions (..., J_s, 3) -> target positions (..., J_t, 3) on the input's device, every
    mapped limb rescaled to the target skeleton's length and hung from its nearest mapped ancestor, the unmapped links
    placeholders of weight 0 (``plan.weight``).  Raises RtgError without a GPU: there is no CPU fallback."""
    require_gpu_rtg()
    Js, Jt = plan.num_source_joints, plan.num_target_joints
    home = src_pos.device if isinstance(src_pos, torch.Tensor) else torch.device("cpu")
    x = dev_f32(src_pos, (Js, 3), "source_positions")
    if x.device != plan.device:
        raise ValueError(f"source_positions is on {x.device}; this plan lives on {plan.device}")
    lead = tuple(x.shape[:-2])
    B = int(torch.Size(lead).numel())
    out = torch.empty(lead + (Jt, 3), device=x.device, dtype=torch.float32)
    check(lib().rtg_fit_targets_f32(plan.handle, ptr(x), B, ptr(out), stream_handle()))
    return out if out.device == home else out.to(home)


def fit_targets_tables(num_source_joints, tgt_parents, tgt_local_translation, src_joint, tgt_joint) -> dict:
    """The host tables of a keypoint-target plan (rtg.h rtg_fit_targets_plan_tables; no GPU needed): anchor (K), seg
    (K, 3), weight (J_t), src_of (J_t)."""
    from .runtime import fit_targets_tables as tables
    return tables(num_source_joints, tgt_parents, tgt_local_translation, src_joint, tgt_joint)


def limb_ratio(src_tree, tgt_tree, mapping, link) -> float:
    """The root-travel scale of a keypoint-target plan (host only): over the mapped pairs on the path root -> ``link``
    of the target tree, the summed length of the target zero pose's segments over the same sum in the source zero
    pose -- for a foot, target leg length over source leg length.  src_tree / tgt_tree: (parent_indices,
    local_translation[, ...]); mapping: (src_joint, tgt_joint) index arrays; link: a target joint index."""
    import numpy as np
    sp, tp = (np.asarray(t[0], np.int64).reshape(-1) for t in (src_tree, tgt_tree))
    slt, tlt = (np.asarray(t[1].cpu() if isinstance(t[1], torch.Tensor) else t[1], np.float32).reshape(-1, 3)
                for t in (src_tree, tgt_tree))
    sj, tj = (np.asarray(a, np.int32).reshape(-1) for a in mapping)
    tab = fit_targets_tables(len(sp), tp, tlt, sj, tj)
    if not 0 <= int(link) < len(tp):
        raise ValueError(f"link {link} is outside 0..{len(tp) - 1}")
    Gs = np.zeros_like(slt)   # the source zero pose's global translations, as the plan takes the target's
    for j in range(1, len(sp)):
        Gs[j] = Gs[sp[j]] + slt[j]
    k = int(tab["src_of"][int(link)])
    num = den = 0.0
    while tab["anchor"][k] >= 0:
        a = int(tab["anchor"][k])
        num += float(np.linalg.norm(tab["seg"][k].astype(np.float64)))
        den += float(np.linalg.norm((Gs[sj[k]] - Gs[sj[a]]).astype(np.float64)))
        k = a
    if den == 0.0:
        raise ValueError(f"no mapped source segment of non-zero length between the root and link {link}")
    return num / den


def quat_between_two_vecs(v1, v2):
    """transform3d.py:8-21 (batch-level identity branch included): (..., 3) x (..., 3) -> (..., 4)."""
    a = dev_f32(v1, (3,), "vec1")
    b = dev_f32(v2, (3,), "vec2")
    if a.shape != b.shape:
        a, b = torch.broadcast_tensors(a, b)
        a, b = a.contiguous(), b.contiguous()
    n = int(torch.Size(a.shape[:-1]).numel())
    out = torch.empty(tuple(a.shape[:-1]) + (4,), device=a.device, dtype=torch.float32)
    ws = torch.empty(2, device=a.device, dtype=torch.float32)
    check(lib().rtg_quat_between_f32(ptr(a), ptr(b), n, ptr(out), ptr(ws), stream_handle()))
    return out


def rebuild_vtrdyn(topo: Topology, motion):
    """RetargetHuV5fromMocap._rebuild_with_vtrdyn_zero_pose (retarget/main.py:116-165) up to its SkeletonState:
    (B, 21, 3) rescaled positions -> (global rotations (B, 21, 4), root translation (B, 3))."""
    J = topo.num_joints
    m = dev_f32(motion, (J, 3), "motion_global_translation")
    B = int(m.shape[0])
    g_rot = torch.empty((B, J, 4), device=m.device, dtype=torch.float32)
    root = torch.empty((B, 3), device=m.device, dtype=torch.float32)
    ws = torch.empty(J, device=m.device, dtype=torch.float32)
    check(lib().rtg_rebuild_vtrdyn_f32(topo.handle, ptr(m), B, ptr(g_rot), ptr(root), ptr(ws), stream_handle()))
    return g_rot, root


def forward_kinematics_multi(segments: Sequence[tuple]):
    """One launch over several (topology, local_rot (B,J,4), root_t (B,3)) segments.

    Returns a list of (g_rot, g_pos) per segment.
    """
    require_gpu()
    if len(segments) > _lib.MAX_SEGMENTS:
        raise ValueError(f"at most {_lib.MAX_SEGMENTS} segments per launch")
    segs, keep, outs = _fk_segments(segments)
    check(lib().rtg_fk_multi_f32(segs, len(segments), stream_handle()))
    return outs


def _fk_segments(segments):
    """ctypes FK segment table with per-segment shape checks: local_rot (B, J, 4) and a root translation that
    broadcasts to (B, 3) -- a 2-D local_rot would otherwise make the kernel read B*J*4 floats of a J*4 buffer."""
    segs = (_lib.FkSegment * max(1, len(segments)))()
    keep, outs = [], []
    for i, (topo, lr, rt) in enumerate(segments):
        J = topo.num_joints
        lr = dev_f32(lr, (J, 4), "local_rot")
        if lr.dim() != 3:
            raise ValueError(f"segment {i}: local_rot must be (B, {J}, 4), got {tuple(lr.shape)}")
        B = int(lr.shape[0])
        rt = dev_f32(rt, (3,), "root_t")
        if rt.dim() > 2 or (rt.dim() == 2 and rt.shape[0] not in (1, B)):
            raise ValueError(f"segment {i}: root_t must broadcast to ({B}, 3), got {tuple(rt.shape)}")
        rt = rt.expand(B, 3).contiguous()   # a (3,) / (1,3) root translation is shared by every frame
        g_rot = torch.empty((B, J, 4), device=lr.device, dtype=torch.float32)
        g_pos = torch.empty((B, J, 3), device=lr.device, dtype=torch.float32)
        segs[i] = _lib.FkSegment(topo.handle.value, lr.data_ptr(), rt.data_ptr(), g_rot.data_ptr(), g_pos.data_ptr(), B)
        keep += [lr, rt]
        outs.append((g_rot, g_pos))
    return segs, keep, outs


def _inv_segments(segments):
    segs = (_lib.LocalRotationSegment * max(1, len(segments)))()
    keep, outs = [], []
    for i, (topo, g) in enumerate(segments):
        J = topo.num_joints
        g = dev_f32(g, (J, 4), "g_rot")
        if g.dim() != 3:
            raise ValueError(f"segment {i}: g_rot must be (B, {J}, 4), got {tuple(g.shape)}")
        out = torch.empty_like(g)
        segs[i] = _lib.LocalRotationSegment(topo.handle.value, g.data_ptr(), out.data_ptr(), int(g.shape[0]))
        keep.append(g)
        outs.append(out)
    return segs, keep, outs


def local_rotation_multi(segments: Sequence[tuple]):
    """One launch of cal_local_rotation (kinematics.py:41-63) over several (topology, g_rot (B,J,4)) segments."""
    require_gpu()
    if len(segments) > _lib.MAX_SEGMENTS:
        raise ValueError(f"at most {_lib.MAX_SEGMENTS} segments per launch")
    segs, keep, outs = _inv_segments(segments)
    check(lib().rtg_local_rotation_multi_f32(segs, len(segments), stream_handle()))
    return outs


def kinematics_multi(fk_segments: Sequence[tuple], inv_segments: Sequence[tuple]):
    """FK segments (topology, local_rot, root_t) and inverse-FK segments (topology, g_rot) in ONE launch
    (BASELINE config 5).  Returns ([(g_rot, g_pos)...], [local_rot...])."""
    require_gpu()
    if len(fk_segments) + len(inv_segments) > _lib.MAX_SEGMENTS:
        raise ValueError(f"at most {_lib.MAX_SEGMENTS} segments per launch")
    fsegs, keep, fouts = _fk_segments(fk_segments)
    isegs, ikeep, iouts = _inv_segments(inv_segments)
    check(lib().rtg_kinematics_multi_f32(fsegs, len(fk_segments), isegs, len(inv_segments), stream_handle()))
    return fouts, iouts


@functools.lru_cache(maxsize=8)
def gaussian_taps(sigma: float = 2.0, truncate: float = 4.0):
    """scipy.ndimage.gaussian_filter1d's taps (float64), as the reference applies them (sigma 2).  Cached (the
    velocity calls take them every time); the array is read-only."""
    import numpy as np
    radius = int(truncate * float(sigma) + 0.5)
    try:
        from scipy.ndimage._filters import _gaussian_kernel1d
        w = _gaussian_kernel1d(sigma, 0, radius)[::-1]
    except Exception:  # noqa: BLE001 -- same formula without scipy
        x = np.arange(-radius, radius + 1)
        w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        w = (w / w.sum())[::-1]
    w = np.ascontiguousarray(w, dtype=np.float64)
    w.flags.writeable = False
    return w, radius


def _time_axis_view(x, tail):
    x = dev_f32(x)
    if x.dim() < 1 + tail:
        raise ValueError("need a frame axis")
    L = int(x.shape[-1 - tail])
    nseq = int(torch.Size(x.shape[:-1 - tail]).numel())
    return x, nseq, L


def motion_velocity(p, dt: float, smooth: bool = True, sigma: float = 2.0):
    """SkeletonMotion._compute_velocity (skeleton3d.py:1126-1135): p (..., L, J, 3) -> (..., L, J, 3).  ``sigma``:
    the smoothing filter's (the reference's is 2; radius 4 sigma, at most 16)."""
    x, nseq, L = _time_axis_view(p, 2)
    S = int(x.shape[-2] * x.shape[-1])
    out = torch.empty_like(x)
    tmp = torch.empty_like(x) if smooth else None
    w, r = gaussian_taps(sigma) if smooth else (None, 0)
    check(lib().rtg_linear_velocity_f32(ptr(x), nseq, L, S, ctypes.c_float(dt),
                                        w.ctypes.data_as(ctypes.c_void_p) if smooth else None, r, ptr(tmp), ptr(out),
                                        stream_handle()))
    return out


def motion_angular_velocity(r, dt: float, smooth: bool = True, sigma: float = 2.0):
    """SkeletonMotion._compute_angular_velocity (skeleton3d.py:1137-1146): r (..., L, J, 4) -> (..., L, J, 3).
    ``sigma`` as in motion_velocity."""
    x, nseq, L = _time_axis_view(r, 2)
    J = int(x.shape[-2])
    out = torch.empty(tuple(x.shape[:-1]) + (3,), device=x.device, dtype=torch.float32)
    tmp = torch.empty_like(out) if smooth else None
    w, rad = gaussian_taps(sigma) if smooth else (None, 0)
    check(lib().rtg_angular_velocity_f32(ptr(x), nseq, L, J, ctypes.c_float(dt),
                                         w.ctypes.data_as(ctypes.c_void_p) if smooth else None, rad, ptr(tmp),
                                         ptr(out), stream_handle()))
    return out


def synth_full_body(topo_full: Topology, B: int, seed: int = 1234, frame_offset: int = 0, want_rot: bool = False,
                    out=None, layout="aos"):
    """Synthetic VTRDyn frames generated on the device (rtg_synth_full_body_f32), as (B,P,C) rows (``"aos"``)
    or (P,C,B) component planes (``"soa"``)."""
    dev = require_gpu()
    code = layout_code(layout)
    shp = (lambda P, C: (P, C, B)) if code == _lib.LAYOUT_SOA else (lambda P, C: (B, P, C))
    if out is None:
        body = torch.empty(shp(21, 3), device=dev, dtype=torch.float32)
        lh = torch.empty(shp(20, 3), device=dev, dtype=torch.float32)
        rh = torch.empty(shp(20, 3), device=dev, dtype=torch.float32)
    else:
        body, lh, rh = out
        for t, want in ((body, shp(21, 3)), (lh, shp(20, 3)), (rh, shp(20, 3))):
            if tuple(t.shape) != want or not t.is_contiguous() or t.dtype != torch.float32:
                raise ValueError(f"synth_full_body: output buffer {tuple(t.shape)} != {want}")
    rot = torch.empty(shp(21, 4), device=dev, dtype=torch.float32) if want_rot else None
    check(lib().rtg_synth_full_body_f32(topo_full.handle, ctypes.c_uint64(seed), frame_offset, B, code, ptr(body),
                                        ptr(lh), ptr(rh), ptr(rot), stream_handle()))
    return (body, lh, rh, rot) if want_rot else (body, lh, rh)


# ---- the rest of the rotation3d / transform3d surface (rtg_quat_op_f32 ops 18-31, rtg_quat_as_euler_f64)
def exp_map_to_angle_axis(e):
    """rotation3d.py:629-646 -> (angle (...), axis (...,3))"""
    r = _quat_op(_lib.OP_EXP_MAP_TO_ANGLE_AXIS, e, a_tail=3, out_tail=4)
    return r[..., 0], r[..., 1:]


def exp_map_to_quat(e):
    """rotation3d.py:648-652 / transform3d.py:146-150"""
    return _quat_op(_lib.OP_EXP_MAP_TO_QUAT, e, a_tail=3, out_tail=4)


def quat_slerp(q0, q1, t):
    """transform3d.py:152-174: q0, q1 (...,4), t broadcastable to (...,1) -> (...,4)"""
    q0, q1 = _bcast(q0, q1, 4, 4)
    t = dev_f32(t)
    if t.dim() >= 1 and t.shape[-1] == 1 and t.dim() == q0.dim():
        t = t[..., 0]
    t = t.expand(q0.shape[:-1]).contiguous()
    return _quat_op(_lib.OP_QUAT_SLERP, q0, q1, t, c_tail=0)


def quat_from_xyz(xyz):
    """rotation3d.py:101-108 per row: (...,3) -> (...,4) [xyz, 1 - |xyz|]"""
    return _quat_op(_lib.OP_QUAT_FROM_XYZ, xyz, a_tail=3, out_tail=4)


def rot_matrix_det(m):
    """rotation3d.py:338-350: (...,3,3) -> (...)"""
    m = dev_f32(m, (3, 3), "m")
    lead = m.shape[:-2]
    out = torch.empty(tuple(lead), device=m.device, dtype=torch.float32)
    check(lib().rtg_quat_op_f32(_lib.OP_ROT_MATRIX_DET, ptr(m), None, None, int(torch.Size(lead).numel()), ptr(out),
                                stream_handle()))
    return out


def rot_matrix_from_quaternion(q):
    """rotation3d.py:398-427: (...,4) -> (...,3,3)"""
    return _quat_op(_lib.OP_ROT_MATRIX_FROM_QUAT, q, out_tail=(3, 3))


def extract_rotation_along_axis(q, axis: int):
    """rotation3d.py:534-556: (n,4) -> (n)"""
    if axis not in (0, 1, 2):
        raise ValueError("Invalid axis. Axis must be 0 (x), 1 (y), or 2 (z).")
    return _quat_op(_lib.OP_ROTATION_ALONG_X + axis, q, out_tail=0)


def project_quat_to_axis(q, which: str):
    """project_quat_to_axis_{x,y,z,xy,xz} (rotation3d.py:479-530): (n,4) -> (n,4)"""
    return _quat_op(_lib.OP_PROJECT_QUAT[which], q)


def quat_as_euler(q, seq: str, degrees: bool = False):
    """scipy Rotation.from_quat(q).as_euler(seq, degrees) in float64 on the device: (...,4) -> (...,3) f64."""
    q = dev_f32(q, (4,), "q")
    lead = q.shape[:-1]
    out = torch.empty(tuple(lead) + (3,), device=q.device, dtype=torch.float64)
    check(lib().rtg_quat_as_euler_f64(ptr(q), seq.encode(), int(bool(degrees)), int(torch.Size(lead).numel()),
                                      ptr(out), stream_handle()))
    return out


def side_kernel_residency(kind: int, precise_gripper: bool = False, layout: str = "aos") -> int:
    """rtg_side_kernel_residency (rtg.h): workgroups of the solver kind's throughput kernel resident per compute unit."""
    require_gpu()
    n = ctypes.c_int32(0)
    check(lib().rtg_side_kernel_residency(int(kind), int(bool(precise_gripper)), layout_code(layout), ctypes.byref(n)))
    return int(n.value)


def box_probe() -> dict:
    """rtg_box_probe (rtg.h): the current GPU's shader clock under load, f32 FMA rate and HBM copy bandwidth,
    measured now -- recorded beside every bench line so throughput from different boxes can be compared."""
    require_gpu()
    out = (ctypes.c_double * _lib.PROBE_FIELDS)()
    check(lib().rtg_box_probe(out, _lib.PROBE_FIELDS, stream_handle()))
    return {"sclk_mhz_under_load": out[0], "valu_f32_fma_T_lane_ops_s": out[1], "hbm_copy_GBs": out[2],
            "valu_kernel_ms": out[3], "copy_kernel_ms": out[4], "compute_units": int(out[5])}

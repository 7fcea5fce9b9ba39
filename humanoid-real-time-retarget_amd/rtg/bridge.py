"""Glue between the reference-shaped Python API and the device ops.

The reference's functions take CPU float32 tensors.  The drop-in modules keep
that contract -- a CPU tensor in gives a CPU tensor out -- while all arithmetic
runs on the MI355X; device tensors stay on the device.  Topologies built from
(parent_indices, local_translation[, quat]) are uploaded once and cached.
"""
from __future__ import annotations

import hashlib
from typing import Optional, Tuple

import numpy as np
import torch

from .runtime import FitTargetsPlan, RetargetPlan, Topology, require_gpu, require_gpu_rtg


def as_tensor(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    return torch.as_tensor(np.asarray(x, dtype=np.float32))


def home_device(*xs) -> torch.device:
    """Device results are returned on: the first tensor argument's device (CPU default)."""
    for x in xs:
        if isinstance(x, torch.Tensor):
            return x.device
    return torch.device("cpu")


def back(t: torch.Tensor, dev: torch.device) -> torch.Tensor:
    return t if t.device == dev else t.to(dev)


_TOPO_CACHE: dict = {}


def _key(*arrays) -> str:
    h = hashlib.sha1()
    for a in arrays:
        if a is None:
            h.update(b"none")
            continue
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _np(x, dtype) -> Optional[np.ndarray]:
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=dtype))


def topology(parent_indices, local_translation, tree_quat=None) -> Topology:
    require_gpu()
    p = _np(parent_indices, np.int32)
    lt = _np(local_translation, np.float32).reshape(-1, 3)
    tq = _np(tree_quat, np.float32)
    k = _key(p, lt, tq)
    topo = _TOPO_CACHE.get(k)
    if topo is None:
        topo = Topology(p, lt, tq)
        _TOPO_CACHE[k] = topo
    return topo


_PLAN_CACHE: dict = {}
_FIT_PLAN_CACHE: dict = {}


def retarget_plan(src_tree, tgt_tree, src_joint, tgt_joint, src_tpose_local_rot, src_tpose_root_t,
                  tgt_tpose_local_rot, tgt_tpose_root_t, rotation_to_target, scale) -> RetargetPlan:
    """The device-resident plan of a ``retarget_to`` call, cached by content like ``topology``.  src_tree / tgt_tree:
    (parent_indices, local_translation, quat) of the two skeleton trees; the mapping as joint index pairs; the t-poses
    and the rotation as tensors or numpy, on the CPU or on the device."""
    require_gpu_rtg()
    sj, tj = _np(src_joint, np.int32), _np(tgt_joint, np.int32)
    consts = [_np(a, np.float32) for a in (src_tpose_local_rot, src_tpose_root_t, tgt_tpose_local_rot,
                                           tgt_tpose_root_t, rotation_to_target)]
    sc = np.float32(scale)
    trees = [(_np(t[0], np.int32), _np(t[1], np.float32), _np(t[2], np.float32)) for t in (src_tree, tgt_tree)]
    k = _key(*trees[0], *trees[1], sj, tj, *consts, np.asarray(sc))
    plan = _PLAN_CACHE.get(k)
    if plan is None:
        plan = RetargetPlan(topology(*trees[0]), topology(*trees[1]), sj, tj, *consts, float(sc))
        _PLAN_CACHE[k] = plan
    return plan


def fit_targets_plan(src_tree, tgt_tree, src_joint, tgt_joint, dir=None, root_scale=None,
                     root_offset=None) -> FitTargetsPlan:
    """The device-resident plan of a keypoint-target launch (``ops.fit_targets``), cached by content like
    ``retarget_plan``.  src_tree / tgt_tree: (parent_indices, local_translation[, quat]) of the two skeleton trees; the
    mapping as joint index pairs; dir / root_scale / root_offset: 3 values each or None."""
    require_gpu_rtg()
    sj, tj = _np(src_joint, np.int32), _np(tgt_joint, np.int32)
    consts = [_np(a, np.float32) for a in (dir, root_scale, root_offset)]
    trees = [(_np(t[0], np.int32), _np(t[1], np.float32), _np(t[2], np.float32) if len(t) > 2 else None)
             for t in (src_tree, tgt_tree)]
    k = _key(*trees[0], *trees[1], sj, tj, *consts)
    plan = _FIT_PLAN_CACHE.get(k)
    if plan is None:
        plan = FitTargetsPlan(topology(*trees[0]), topology(*trees[1]), sj, tj, *consts)
        _FIT_PLAN_CACHE[k] = plan
    return plan


def split_lead(t: torch.Tensor, tail: int) -> Tuple[torch.Size, torch.Tensor]:
    lead = t.shape[:-tail] if tail else t.shape
    return lead, t

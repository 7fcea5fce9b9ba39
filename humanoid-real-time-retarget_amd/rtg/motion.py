"""A motion library on the device: many clips of one skeleton, sampled at arbitrary (clip, time) pairs in one launch.

``MotionLibrary(motions)`` packs ``SkeletonMotion``s of one skeleton tree once into the arrays
``ops.motion_sample`` reads (local rotations, root translations, ``[global_velocity | global_angular_velocity]`` rows)
and ``.sample(clip_ids, times)`` returns the poses between the stored frames: ``quat_slerp`` of the local rotations,
linear blends of the rest, forward kinematics of the blended pose.  Nothing here touches the device
at import; there is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .runtime import MotionLib, require_gpu_rtg

__all__ = ["MotionLibrary", "MotionSample"]


@dataclass
class MotionSample:
    """What ``MotionLibrary.sample`` returns, device tensors: (N, J, 4) rotations, (N, 3) / (N, J, 3) vectors; the
    parts not asked for are None."""
    local_rotation: torch.Tensor
    root_translation: torch.Tensor
    global_rotation: Optional[torch.Tensor] = None
    global_translation: Optional[torch.Tensor] = None
    global_velocity: Optional[torch.Tensor] = None
    global_angular_velocity: Optional[torch.Tensor] = None


def _same_tree(a, b) -> bool:
    return (list(a.node_names) == list(b.node_names) and torch.equal(a.parent_indices.cpu(), b.parent_indices.cpu())
            and torch.equal(a.local_translation.cpu(), b.local_translation.cpu())
            and torch.equal(a.quat.cpu(), b.quat.cpu()))


class MotionLibrary:
    """One or many ``SkeletonMotion``s of ONE skeleton tree, packed frame-major on the current device.  A motion that
    stores global rotations goes through ``local_rotation`` first.  ``with_velocity=False`` leaves the velocity rows
    out (``sample(want_velocity=True)`` then raises)."""

    def __init__(self, motions, with_velocity: bool = True):
        motions = list(motions) if isinstance(motions, (list, tuple)) else [motions]
        if not motions:
            raise ValueError("MotionLibrary: no motions")
        tree = getattr(motions[0], "skeleton_tree", None)
        if tree is None:
            raise ValueError("MotionLibrary: expected SkeletonMotion objects")
        J = tree.num_joints
        if not 1 <= J <= 64:
            raise ValueError(f"MotionLibrary: serves skeletons of 1..64 joints, this tree has {J}")
        width = J * 4 + 3 + (J * 6 if with_velocity else 0)
        fps = []
        for i, m in enumerate(motions):
            if getattr(m, "skeleton_tree", None) is None or not hasattr(m, "fps"):
                raise ValueError(f"MotionLibrary: motion {i} is not a SkeletonMotion")
            if not _same_tree(tree, m.skeleton_tree):
                raise ValueError(f"MotionLibrary: motion {i} is on another skeleton tree than motion 0")
            t = m.tensor
            if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < width:
                raise ValueError(f"MotionLibrary: motion {i} must be (frames >= 1, >= {width}) for {J} joints, got "
                                 f"{tuple(t.shape)}")
            f = float(np.float32(m.fps))
            if not (np.isfinite(f) and f > 0):
                raise ValueError(f"MotionLibrary: motion {i} has fps {m.fps!r}")
            fps.append(f)
        dev = require_gpu_rtg()
        self.skeleton_tree = tree
        self.topology = tree.topology()
        lengths = np.array([m.tensor.shape[0] for m in motions], np.int32)
        start = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]).astype(np.int64)

        def pack(parts):
            return torch.cat([p.to(device=dev, dtype=torch.float32) for p in parts], dim=0).contiguous()

        self.rot = pack([m.local_rotation.reshape(-1, J, 4) for m in motions])
        self.root_t = pack([m.root_translation.reshape(-1, 3) for m in motions])
        self.vec = pack([torch.cat([m.global_velocity, m.global_angular_velocity], dim=-2) for m in motions]) \
            if with_velocity else None
        self._lib = MotionLib(start, lengths, np.asarray(fps, np.float32), int(lengths.sum()))
        self._lengths, self._fps = lengths, np.asarray(fps, np.float32)

    @property
    def num_clips(self) -> int:
        return int(self._lengths.shape[0])

    @property
    def lengths(self) -> np.ndarray:
        """Frames per clip (int32)."""
        return self._lengths

    @property
    def fps(self) -> np.ndarray:
        """Frame rate per clip (float32)."""
        return self._fps

    @property
    def durations(self) -> np.ndarray:
        """Seconds from each clip's first frame to its last (float64): (length - 1) / fps."""
        return (self._lengths.astype(np.float64) - 1.0) / self._fps.astype(np.float64)

    def sample(self, clip_ids, times, want_global: bool = True, want_velocity: bool = True, state: bool = True,
               normalize: bool = True) -> MotionSample:
        """The library's poses at ``times`` (seconds from the first frame of clip ``clip_ids[n]``; clamped to the
        clip, no wrap-around) in one launch.  ``state``: the global outputs as SkeletonState computes them (with the
        tree quaternions), else as plain forward kinematics.  ``normalize``: ``quat_normalize`` after the slerp.  A
        clip id outside 0..num_clips-1 gives NaN rows."""
        if want_velocity and self.vec is None:
            raise ValueError("this library was packed without velocities (with_velocity=False)")
        J = self.skeleton_tree.num_joints
        lr, rt, v, g_rot, g_pos = ops.motion_sample(self.topology, self._lib, self.rot, self.root_t, clip_ids, times,
                                                    vec=self.vec if want_velocity else None, normalize=normalize,
                                                    want_global=want_global, state=state)
        return MotionSample(lr, rt, g_rot, g_pos, None if v is None else v[:, :J], None if v is None else v[:, J:])

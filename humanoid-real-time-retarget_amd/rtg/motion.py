"""A motion library on the device: many clips of one skeleton, sampled at arbitrary (clip, time) pairs in one launch.

``MotionLibrary(motions)`` packs ``SkeletonMotion``s of one skeleton tree once into the arrays
``ops.motion_sample`` reads (local rotations, root translations, ``[global_velocity | global_angular_velocity]`` rows)
and ``.sample(clip_ids, times)`` returns the poses between the stored frames: ``quat_slerp`` of the local rotations,
linear blends of the rest, forward kinematics of the blended pose.

``DofMotionLibrary(model, clips)`` is the same for clips in the robot's own coordinates -- joint angles, root
translation, root rotation per frame, what ``HuForwardModel.fit_pose`` / ``fit_motion`` / ``fit_mocap`` return -- and
``.sample`` returns the reference states a tracking controller or a simulator reads: DOF positions and velocities, the
root's pose and velocities, link poses or a few key links' positions.

Nothing here touches the device at import; there is no CPU fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .runtime import MotionLib, require_gpu_rtg

__all__ = ["MotionLibrary", "MotionSample", "DofMotionLibrary", "DofMotionSample"]


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


@dataclass
class DofMotionSample:
    """What ``DofMotionLibrary.sample`` returns, device tensors: dof_pos / dof_vel (N, J-1), root_translation /
    root_velocity / root_angular_velocity (N, 3), root_rotation (N, 4), global_rotation (N, J, 4), global_translation
    (N, J, 3), key_translation (N, K, 3); the parts not asked for are None.  With ``link_velocities`` the sample also
    carries global_velocity / global_angular_velocity (N, J, 3) and key_velocity / key_angular_velocity (N, K, 3), world
    frame: plain attributes that default to None, set after construction, so that the dataclass's fields -- and every
    positional construction -- stay what they were."""
    dof_pos: torch.Tensor
    root_translation: torch.Tensor
    root_rotation: torch.Tensor
    dof_vel: Optional[torch.Tensor] = None
    root_velocity: Optional[torch.Tensor] = None
    root_angular_velocity: Optional[torch.Tensor] = None
    global_rotation: Optional[torch.Tensor] = None
    global_translation: Optional[torch.Tensor] = None
    key_translation: Optional[torch.Tensor] = None
    global_velocity = None            # (not annotated: not dataclass fields, see above)
    global_angular_velocity = None
    key_velocity = None
    key_angular_velocity = None


def _rows(x, width: int, squeeze_axis: int):
    """A clip's (L, width) rows from (L, width), or with the singleton axis of fit_pose's (L, J-1, 1) / (L, 1, 4)."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() == 3 and t.shape[squeeze_axis] == 1:
        t = t.squeeze(squeeze_axis)
    return t if t.dim() == 2 and t.shape[1] == width else None


class DofMotionLibrary:
    """One or many joint-angle clips of ONE model, packed frame-major on the current device.  ``model``: a
    ``HuForwardModel`` (or an ``rtg.runtime.DofModel``); ``clips``: ``(angles, root_translation, root_rotation, fps)``
    tuples -- the first three items of ``fit_pose``'s return in that order -- with angles (L, J-1, 1) or (L, J-1), root
    translation (L, 3), root rotation (L, 1, 4) or (L, 4)."""

    def __init__(self, model, clips):
        if isinstance(clips, tuple) and len(clips) == 4 and not isinstance(clips[3], (tuple, list)):
            clips = [clips]   # one clip, not a list of them
        clips = list(clips)
        if not clips:
            raise ValueError("DofMotionLibrary: no clips")
        dof_model = getattr(model, "_model", model)
        nd = getattr(dof_model, "num_dofs", None)
        if nd is None:
            raise ValueError("DofMotionLibrary: expected a HuForwardModel or a DofModel")
        J = int(nd) + 1
        if not 1 <= J <= 64:
            raise ValueError(f"DofMotionLibrary: serves models of 1..64 joints, this one has {J}")
        parts, fps = [], []
        for i, clip in enumerate(clips):
            if not isinstance(clip, (tuple, list)) or len(clip) != 4:
                raise ValueError(f"DofMotionLibrary: clip {i} is not (angles, root_translation, root_rotation, fps)")
            a, t, r = _rows(clip[0], nd, 2), _rows(clip[1], 3, 1), _rows(clip[2], 4, 1)
            if a is None or t is None or r is None:
                raise ValueError(f"DofMotionLibrary: clip {i} must be (L, {nd}[, 1]) angles, (L, 3) root translation and "
                                 f"(L[, 1], 4) root rotation, got "
                                 f"{' / '.join(str(tuple(np.shape(x))) for x in clip[:3])}")
            if not (a.shape[0] == t.shape[0] == r.shape[0]) or a.shape[0] < 1:
                raise ValueError(f"DofMotionLibrary: clip {i} must have one length >= 1, got {a.shape[0]} / {t.shape[0]} / "
                                 f"{r.shape[0]} frames")
            try:
                f = float(np.float32(clip[3]))
            except (TypeError, ValueError):
                f = float("nan")
            if not (np.isfinite(f) and f > 0):
                raise ValueError(f"DofMotionLibrary: clip {i} has fps {clip[3]!r}")
            parts.append((a, t, r))
            fps.append(f)
        dev = require_gpu_rtg()
        self.model = dof_model
        self.node_names = list(getattr(model, "node_names", None) or [])
        lengths = np.array([p[0].shape[0] for p in parts], np.int32)
        start = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.int64)]).astype(np.int64)

        def pack(k):
            return torch.cat([p[k].detach().to(device=dev, dtype=torch.float32) for p in parts], dim=0).contiguous()

        self.dof, self.root_t, self.root_rot = pack(0), pack(1), pack(2)
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

    def _link_indices(self, key_links):
        if key_links is None:
            return None
        out = []
        for link in key_links:
            if isinstance(link, str):
                if link not in self.node_names:
                    raise ValueError(f"key_links: the skeleton has no node named {link!r}")
                out.append(self.node_names.index(link))
            else:
                out.append(int(link))
        return out

    def sample(self, clip_ids, times, key_links=None, want_velocity: bool = True, want_global: bool = True,
               normalize: bool = True, clip_angles: bool = False, link_velocities: bool = False) -> DofMotionSample:
        """The library's states at ``times`` (seconds from the first frame of clip ``clip_ids[n]``; clamped to the
        clip, no wrap-around) in one launch.  ``key_links``: up to 32 node names or joint indices whose positions come
        back as ``key_translation`` (also with ``want_global=False``, which skips the full link poses).
        ``want_velocity``: the forward differences of the bracketing frames (DOF and root linear velocity) and the
        pair's angular velocity.  ``normalize``: ``quat_normalize`` after the root rotation's slerp.  ``clip_angles``:
        the link poses from the angles clamped to the model's limits.  ``link_velocities`` (needs ``want_velocity``):
        the world-frame linear and angular velocity of every link (``global_velocity``, ``global_angular_velocity``,
        with ``want_global``) and of the key links (``key_velocity``, ``key_angular_velocity``), from the sampled joint
        and root velocities in the same launch; with ``clip_angles`` a joint held at a limit does not turn.  A clip id
        outside 0..num_clips-1 gives NaN rows."""
        if clip_angles and not self.model.has_limits:
            raise ValueError("clip_angles needs DOF limits with one entry per DOF")
        if link_velocities and not want_velocity:
            raise ValueError("link_velocities needs want_velocity: the link velocities come from the sampled joint and "
                             "root velocities")
        keys = self._link_indices(key_links)
        r = ops.dof_motion_sample(self.model, self._lib, self.dof, self.root_rot, self.root_t, clip_ids, times,
                                  normalize=normalize, clip=clip_angles, want_velocity=want_velocity,
                                  want_global=want_global, key_links=keys,
                                  want_link_velocity=bool(link_velocities and want_global),
                                  want_key_velocity=bool(link_velocities and keys))
        rv = r.root_vel
        out = DofMotionSample(r.dof, r.root_t, r.root_rot, r.dof_vel, None if rv is None else rv[:, :3],
                              None if rv is None else rv[:, 3:], r.g_rot, r.g_pos, r.key_pos)
        if r.g_vel is not None:
            out.global_velocity, out.global_angular_velocity = r.g_vel[..., :3], r.g_vel[..., 3:]
        if r.key_vel is not None:
            out.key_velocity, out.key_angular_velocity = r.key_vel[..., :3], r.key_vel[..., 3:]
        return out

"""Drop-in ``poselib.poselib.skeleton.skeleton3d`` (reference poselib/poselib/skeleton/skeleton3d.py).

``SkeletonTree`` / ``SkeletonState`` / ``SkeletonMotion`` keep the reference's
attribute layout (``_node_names``, ``_parent_indices``, ``_local_translation``,
``_quat``, ``_node_indices``; ``tensor``, ``_skeleton_tree``, ``_is_local``,
``_fps``), so the reference's pickled assets unpickle into these classes
unchanged.  Forward / inverse kinematics (``global_transformation``,
``local_rotation``), the quaternion algebra and ``retarget_to`` (one fused
launch per call) run in librtg_hip.so.  ``drop_nodes_by_names`` /
``keep_nodes_by_names`` are host code on the tree and existing device ops plus
a torch reduction on a state; neither mutates the tree it is called on (the
reference's does).

Offline tools of the reference (``from_mjcf``, ``from_fbx``, ``crop``,
``compute_forward_vector``) are outside the hot path and not provided
(SURVEY.md §2 row 3).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List

import numpy as np
import torch

from rtg import ops
from rtg.bridge import as_tensor, back, retarget_plan, topology
from rtg.safe_pickle import load_skeleton_state_arrays

from ..core.backend import Serializable
from ..core.rotation3d import quat_identity, quat_normalize

__all__ = ["SkeletonTree", "SkeletonState", "SkeletonMotion", "MotionDICT", "load_skeleton_state"]


class SkeletonTree(Serializable):
    """Parent-indexed rigid skeleton (skeleton3d.py:22-263)."""

    def __init__(self, node_names, parent_indices, local_translation, quat=None):
        ln, lp, ll = len(node_names), len(parent_indices), len(local_translation)
        assert len(set((ln, lp, ll))) == 1          # skeleton3d.py:87-88
        self._node_names = node_names
        self._parent_indices = torch.as_tensor(parent_indices).long()
        self._local_translation = as_tensor(local_translation)
        self._quat = quat_identity([len(node_names)]) if quat is None else as_tensor(quat)
        self._node_indices = {self.node_names[i]: i for i in range(len(self))}

    def __len__(self):
        return len(self.node_names)

    def __iter__(self):
        yield from self.node_names

    def __getitem__(self, item):
        return self.node_names[item]

    def __repr__(self):
        return (f"SkeletonTree(\n    node_names={self.node_names!r},\n    parent_indices={self.parent_indices!r},"
                f"\n    local_translation={self.local_translation!r}\n)")

    @property
    def node_names(self):
        return self._node_names

    @property
    def parent_indices(self):
        return self._parent_indices

    @property
    def local_translation(self):
        return self._local_translation

    @property
    def quat(self):
        return getattr(self, "_quat", None) if getattr(self, "_quat", None) is not None else quat_identity([len(self)])

    @property
    def num_joints(self):
        return len(self)

    def parent_of(self, node_name):
        return self[int(self.parent_indices[self.index(node_name)].item())]

    def index(self, node_name):
        return self._node_indices[node_name]

    def topology(self):
        """Device-resident topology of this tree (cached by content)."""
        return topology(self.parent_indices, self.local_translation, self.quat)

    def drop_nodes_by_names(self, node_names: List[str], pairwise_translation=None) -> "SkeletonTree":
        """skeleton3d.py:226-259: the tree without ``node_names``; a kept node hangs from its nearest kept ancestor,
        its translation the sum over the dropped links (or ``pairwise_translation[new parent, node]``).  This tree is
        left as it is: the reference adds the dropped links into its own translations (:241), INTEGRATION.md."""
        drop = set(node_names)
        parents = [int(p) for p in self.parent_indices]
        names, new_parents, rows, new_index = [], [], [], {}
        for j, name in enumerate(self.node_names):
            if name in drop:
                continue
            t = self.local_translation[j].clone()
            p = parents[j]
            if p != -1:
                while p != -1 and self[p] in drop:
                    t = t + self.local_translation[p]
                    p = parents[p]
                assert p != -1, "the root node cannot be dropped"
                if pairwise_translation is not None:
                    t = as_tensor(pairwise_translation)[p, j, :].to(t.device, t.dtype)
            new_index[j] = len(names)
            names.append(name)
            new_parents.append(-1 if p == -1 else new_index[p])
            rows.append(t)
        lt = torch.stack(rows) if rows else torch.zeros(0, 3, dtype=self.local_translation.dtype)
        return SkeletonTree(names, torch.as_tensor(new_parents, dtype=self.parent_indices.dtype), lt)

    def keep_nodes_by_names(self, node_names: List[str], pairwise_translation=None) -> "SkeletonTree":
        """skeleton3d.py:261-263"""
        keep = set(node_names)
        return self.drop_nodes_by_names([n for n in self if n not in keep], pairwise_translation)

    @classmethod
    def from_dict(cls, dict_repr, *args, **kwargs):
        def arr(d):
            return torch.from_numpy(np.asarray(d["arr"]).astype(d["context"]["dtype"]))
        return cls(list(map(str, dict_repr["node_names"])), arr(dict_repr["parent_indices"]),
                   arr(dict_repr["local_translation"]), arr(dict_repr["quat"]) if "quat" in dict_repr else None)

    def to_dict(self):
        def d(x):
            x = x.detach().cpu().numpy()
            return {"arr": x, "context": {"dtype": x.dtype.name}}
        return OrderedDict([("node_names", self.node_names), ("parent_indices", d(self.parent_indices)),
                            ("local_translation", d(self.local_translation))])


class SkeletonState(Serializable):
    """A static pose: rotations (local or global) + root translation (skeleton3d.py:266-934)."""

    def __init__(self, tensor_backend, skeleton_tree, is_local):
        self._skeleton_tree = skeleton_tree
        self._is_local = is_local
        self.tensor = as_tensor(tensor_backend).clone()

    def __len__(self):
        return self.tensor.shape[0]

    # -- raw views of the state vector [J*4 rotations, 3 root translation]
    @property
    def rotation(self):
        J = self.num_joints
        return self.tensor[..., :J * 4].reshape(*(self.tensor.shape[:-1] + (J, 4)))

    @property
    def root_translation(self):
        J = self.num_joints
        return self.tensor[..., J * 4:J * 4 + 3]

    @property
    def is_local(self):
        return self._is_local

    @property
    def invariant_property(self):
        return {"skeleton_tree": self.skeleton_tree, "is_local": self.is_local}

    @property
    def num_joints(self):
        return self.skeleton_tree.num_joints

    @property
    def skeleton_tree(self):
        return self._skeleton_tree

    # -- kinematics
    @property
    def local_rotation(self):
        """Local rotations; for a global state, inverse FK incl. the tree-quat fix-up (skeleton3d.py:460-484)."""
        if self._is_local:
            return self.rotation
        cached = self.__dict__.get("_comp_local_rotation")
        if cached is None:
            g = self.rotation
            lead = g.shape[:-2]
            loc = ops.local_rotation(self.skeleton_tree.topology(), g.reshape(-1, self.num_joints, 4), state=True)
            cached = back(loc.reshape(*lead, self.num_joints, 4), g.device)
            self._comp_local_rotation = cached
        return cached

    @property
    def local_translation(self):
        """Tree translations with the root replaced by the root translation (skeleton3d.py:494-505)."""
        cached = self.__dict__.get("_local_translation")
        if cached is None:
            shape = tuple(self.tensor.shape[:-1]) + (self.num_joints, 3)
            cached = self.skeleton_tree.local_translation.to(self.tensor.device).broadcast_to(*shape).clone()
            cached[..., 0, :] = self.root_translation
            self._local_translation = cached
        return cached

    @property
    def local_transformation(self):
        return torch.cat([self.local_rotation, self.local_translation], dim=-1)

    @property
    def global_transformation(self):
        """FK through transform_mul with the tree pre-rotation (skeleton3d.py:402-425), on the MI355X."""
        cached = self.__dict__.get("_global_transformation")
        if cached is None:
            lr = self.local_rotation
            lead = lr.shape[:-2]
            J = self.num_joints
            rt = self.root_translation.reshape(-1, 3)
            g_rot, g_pos = ops.forward_kinematics(self.skeleton_tree.topology(), lr.reshape(-1, J, 4), rt, state=True)
            cached = back(torch.cat([g_rot, g_pos], dim=-1).reshape(*lead, J, 7), lr.device)
            self._global_transformation = cached
        return cached

    @property
    def global_rotation(self):
        if not self._is_local:
            return self.rotation
        return self.global_transformation[..., :4]

    @property
    def global_translation(self):
        return self.global_transformation[..., 4:]

    @property
    def global_root_rotation(self):
        return self.global_rotation[..., 0, :]

    @staticmethod
    def _to_state_vector(rot, rt):
        state_shape = rot.shape[:-2]
        vr = rot.reshape(*(state_shape + (-1,)))
        vt = rt.to(rot.device).broadcast_to(*state_shape + rt.shape[-1:]).reshape(*(state_shape + (-1,)))
        return torch.cat([vr, vt], dim=-1)

    @classmethod
    def from_rotation_and_root_translation(cls, skeleton_tree, r, t, is_local=True):
        """skeleton3d.py:594-617 -- rotations are normalised (on the device) first."""
        r = as_tensor(r)
        assert r.dim() > 0, "the rotation needs to have at least 1 dimension"
        r = quat_normalize(r)
        return cls(SkeletonState._to_state_vector(r, as_tensor(t)), skeleton_tree=skeleton_tree, is_local=is_local)

    @classmethod
    def zero_pose(cls, skeleton_tree):
        return cls.from_rotation_and_root_translation(skeleton_tree, skeleton_tree.quat,
                                                      torch.zeros(3, dtype=skeleton_tree.local_translation.dtype),
                                                      is_local=True)

    def local_repr(self):
        if self.is_local:
            return self
        return SkeletonState.from_rotation_and_root_translation(self.skeleton_tree, self.local_rotation,
                                                                self.root_translation, is_local=True)

    def global_repr(self):
        if not self.is_local:
            return self
        return SkeletonState.from_rotation_and_root_translation(self.skeleton_tree, self.global_rotation,
                                                                self.root_translation, is_local=False)

    # -- reduced skeletons and the generic retarget (skeleton3d.py:668-934)
    def _transfer_to(self, new_skeleton_tree: SkeletonTree):
        """skeleton3d.py:676-683: this state's global rotations at the new tree's joints, as a global state."""
        old = [self.skeleton_tree.index(n) for n in new_skeleton_tree]
        return SkeletonState.from_rotation_and_root_translation(new_skeleton_tree, self.global_rotation[..., old, :],
                                                                self.root_translation, is_local=False)

    def drop_nodes_by_names(self, node_names: List[str],
                            estimate_local_translation_from_states: bool = True) -> "SkeletonState":
        """skeleton3d.py:685-702.  The averaged translation (:668-674) is computed only for the (new parent, node)
        pairs the reduced tree reads -- mean over frames of quat_rotate(conj(G_parent), P_node - P_parent) -- not
        as the reference's frames x J x J tensor."""
        tree = self.skeleton_tree
        new_tree = tree.drop_nodes_by_names(node_names)
        if estimate_local_translation_from_states:
            nodes = [tree.index(n) for n in new_tree]
            pairs = [(nodes[int(p)], j) for j, p in zip(nodes, new_tree.parent_indices) if int(p) != -1]
            J = tree.num_joints
            pairwise = torch.zeros(J, J, 3, dtype=torch.float32)
            if pairs:
                pi, ni = [p for p, _ in pairs], [j for _, j in pairs]
                G = self.global_rotation.reshape(-1, J, 4)
                P = self.global_translation.reshape(-1, J, 3)
                rel = ops.quat_rotate(ops.quat_inverse(G[:, pi]), P[:, ni] - P[:, pi])
                pairwise[pi, ni] = rel.double().mean(dim=0).float().cpu()
            new_tree = tree.drop_nodes_by_names(node_names, pairwise)
        return self._transfer_to(new_tree)

    def keep_nodes_by_names(self, node_names: List[str],
                            estimate_local_translation_from_states: bool = True) -> "SkeletonState":
        """skeleton3d.py:704-719 (it filters the tree's node names; the reference iterates the state and raises)."""
        keep = set(node_names)
        return self.drop_nodes_by_names([n for n in self.skeleton_tree if n not in keep],
                                        estimate_local_translation_from_states)

    def retarget_to(self, joint_mapping: Dict[str, str], source_tpose_local_rotation, source_tpose_root_translation,
                    target_skeleton_tree: SkeletonTree, target_tpose_local_rotation, target_tpose_root_translation,
                    rotation_to_target_skeleton, scale_to_target_skeleton: float, z_up: bool = True) -> "SkeletonState":
        """skeleton3d.py:742-889 on the MI355X, one launch: this state's rotations relative to the source t-pose,
        re-applied to the target t-pose over the mapped joints.  Returns a local state on ``target_skeleton_tree``.
        The state needs exactly one leading batch dimension (the reference indexes it, :863 / :880); ``z_up`` is
        accepted and unused, as there."""
        if self.tensor.dim() != 2:
            raise ValueError(f"retarget_to needs a state with exactly one batch dimension, got shape "
                             f"{tuple(self.tensor.shape[:-1])}")
        src, tgt = self.skeleton_tree, target_skeleton_tree
        inv = {t: s for s, t in joint_mapping.items()}
        # the reference's checks, in its order: the reduced source tree (:828), the reduced target tree, the counts (:729)
        assert src[0] in joint_mapping, "the root node cannot be dropped"
        assert tgt[0] in inv, "the root node cannot be dropped"
        kept_s = [n for n in src if n in joint_mapping]
        kept_t = [n for n in tgt if n in inv]
        assert len({len(joint_mapping), len(kept_s), len(kept_t)}) == 1, \
            "the joint mapping is not consistent with the skeleton trees"
        plan = retarget_plan((src.parent_indices, src.local_translation, src.quat),
                             (tgt.parent_indices, tgt.local_translation, tgt.quat),
                             [src.index(s) for s in joint_mapping], [tgt.index(t) for t in joint_mapping.values()],
                             source_tpose_local_rotation, source_tpose_root_translation, target_tpose_local_rotation,
                             target_tpose_root_translation, rotation_to_target_skeleton, scale_to_target_skeleton)
        rot, root = ops.retarget_to(plan, self.rotation, self.root_translation, self.is_local)
        dev = self.tensor.device
        return SkeletonState(SkeletonState._to_state_vector(back(rot, dev), back(root, dev)), tgt, True)

    def retarget_to_by_tpose(self, joint_mapping: Dict[str, str], source_tpose: "SkeletonState",
                             target_tpose: "SkeletonState", rotation_to_target_skeleton,
                             scale_to_target_skeleton: float) -> "SkeletonState":
        """skeleton3d.py:891-934 with the assertion it intends: both t-poses are single poses (the reference reads a
        ``.shape`` a SkeletonState does not have and raises AttributeError)."""
        assert source_tpose.tensor.dim() == 1 and target_tpose.tensor.dim() == 1, \
            "the retargeting script currently doesn't support vectorized operations"
        return self.retarget_to(joint_mapping, source_tpose.local_rotation, source_tpose.root_translation,
                                target_tpose.skeleton_tree, target_tpose.local_rotation,
                                target_tpose.root_translation, rotation_to_target_skeleton, scale_to_target_skeleton)

    def to_dict(self):
        def d(x):
            x = x.detach().cpu().numpy()
            return {"arr": x, "context": {"dtype": x.dtype.name}}
        return OrderedDict([("rotation", d(self.rotation)), ("root_translation", d(self.root_translation)),
                            ("skeleton_tree", self.skeleton_tree.to_dict()), ("is_local", self.is_local)])

    @classmethod
    def from_dict(cls, dict_repr, *args, **kwargs):
        def arr(d):
            return torch.from_numpy(np.asarray(d["arr"]).astype(d["context"]["dtype"]))
        return cls(SkeletonState._to_state_vector(arr(dict_repr["rotation"]), arr(dict_repr["root_translation"])),
                   SkeletonTree.from_dict(dict_repr["skeleton_tree"]), dict_repr["is_local"])


class SkeletonMotion(SkeletonState):
    """A state sequence with per-joint velocities appended (skeleton3d.py:935-1292)."""

    def __init__(self, tensor_backend, skeleton_tree, is_local, fps, *args, **kwargs):
        self._fps = fps
        super().__init__(tensor_backend, skeleton_tree, is_local)

    def clone(self):
        return SkeletonMotion(self.tensor.clone(), self.skeleton_tree, self._is_local, self._fps)

    @property
    def invariant_property(self):
        return {"skeleton_tree": self.skeleton_tree, "is_local": self.is_local, "fps": self.fps}

    @property
    def global_velocity(self):
        J = self.num_joints
        c = J * 4 + 3
        return self.tensor[..., c:c + J * 3].reshape(*(self.tensor.shape[:-1] + (J, 3)))

    @property
    def global_angular_velocity(self):
        J = self.num_joints
        c = J * 7 + 3
        return self.tensor[..., c:c + J * 3].reshape(*(self.tensor.shape[:-1] + (J, 3)))

    @property
    def fps(self):
        return self._fps

    @property
    def time_delta(self):
        return 1.0 / self.fps

    @property
    def global_root_velocity(self):
        return self.global_velocity[..., 0, :]

    @property
    def global_root_angular_velocity(self):
        return self.global_angular_velocity[..., 0, :]

    @classmethod
    def from_state_vector_and_velocity(cls, skeleton_tree, state_vector, global_velocity, global_angular_velocity,
                                       is_local, fps):
        state_vector = as_tensor(state_vector)
        shape = state_vector.shape[:-1]
        v = as_tensor(global_velocity).to(state_vector.device).reshape(*(shape + (-1,)))
        av = as_tensor(global_angular_velocity).to(state_vector.device).reshape(*(shape + (-1,)))
        return cls(torch.cat([state_vector, v, av], dim=-1), skeleton_tree=skeleton_tree, is_local=is_local, fps=fps)

    @classmethod
    def from_skeleton_state(cls, skeleton_state: SkeletonState, fps: int):
        """Velocities by np.gradient + gaussian_filter1d(sigma=2, nearest) over frames
        (skeleton3d.py:1026-1049, 1126-1146), computed on the MI355X."""
        assert type(skeleton_state) == SkeletonState, \
            f"expected type of {SkeletonState}, got {type(skeleton_state)}"
        dt = 1 / fps
        gv = ops.motion_velocity(skeleton_state.global_translation, dt)
        gav = ops.motion_angular_velocity(skeleton_state.global_rotation, dt)
        dev = skeleton_state.tensor.device
        return cls.from_state_vector_and_velocity(skeleton_state.skeleton_tree, skeleton_state.tensor,
                                                  back(gv, dev), back(gav, dev), skeleton_state.is_local, fps)

    def resample(self, fps) -> "SkeletonMotion":
        """This motion at another frame rate (not in the reference, whose ``crop`` only decimates by an integer
        factor): frames at ``float32(k / fps)`` seconds for k = 0 .. floor((L - 1) * fps / self.fps), each between the
        two stored frames around it -- ``quat_slerp`` of the local rotations, then ``quat_normalize``; the root
        translation blended linearly -- in one launch (rtg.motion).  The result is a local motion; its
        velocities are not interpolated but recomputed by ``from_skeleton_state`` at the new rate."""
        import math

        from rtg.motion import MotionLibrary
        if self.tensor.dim() != 2:
            raise ValueError(f"resample needs a motion with exactly one batch dimension, got shape "
                             f"{tuple(self.tensor.shape[:-1])}")
        if not (math.isfinite(float(fps)) and float(fps) > 0):
            raise ValueError(f"resample: fps must be finite and positive, got {fps!r}")
        lib = MotionLibrary(self, with_velocity=False)
        n = int(math.floor((len(self) - 1) * float(fps) / float(self.fps))) + 1
        times = (np.arange(n, dtype=np.float64) / float(fps)).astype(np.float32)
        s = lib.sample(np.zeros(n, np.int32), times, want_global=False, want_velocity=False, normalize=True)
        dev = self.tensor.device
        state = SkeletonState(SkeletonState._to_state_vector(back(s.local_rotation, dev), back(s.root_translation, dev)),
                              self.skeleton_tree, True)
        return SkeletonMotion.from_skeleton_state(state, fps)

    def retarget_to(self, joint_mapping: Dict[str, str], source_tpose_local_rotation, source_tpose_root_translation,
                    target_skeleton_tree: SkeletonTree, target_tpose_local_rotation, target_tpose_root_translation,
                    rotation_to_target_skeleton, scale_to_target_skeleton: float, z_up: bool = True) -> "SkeletonMotion":
        """skeleton3d.py:1185-1249: the retargeted states with their velocities at this motion's fps."""
        return SkeletonMotion.from_skeleton_state(
            super().retarget_to(joint_mapping, source_tpose_local_rotation, source_tpose_root_translation,
                                target_skeleton_tree, target_tpose_local_rotation, target_tpose_root_translation,
                                rotation_to_target_skeleton, scale_to_target_skeleton, z_up), self.fps)

    def retarget_to_by_tpose(self, joint_mapping: Dict[str, str], source_tpose: "SkeletonState",
                             target_tpose: "SkeletonState", rotation_to_target_skeleton,
                             scale_to_target_skeleton: float, z_up: bool = True) -> "SkeletonMotion":
        """skeleton3d.py:1251-1292"""
        assert source_tpose.tensor.dim() == 1 and target_tpose.tensor.dim() == 1, \
            "the retargeting script currently doesn't support vectorized operations"
        return self.retarget_to(joint_mapping, source_tpose.local_rotation, source_tpose.root_translation,
                                target_tpose.skeleton_tree, target_tpose.local_rotation,
                                target_tpose.root_translation, rotation_to_target_skeleton, scale_to_target_skeleton,
                                z_up)

    @staticmethod
    def _to_state_vector(rot, rt, vel, avel):
        """[J*4 rotations, 3 root, J*3 velocities, J*3 angular velocities] (skeleton3d.py:1051-1058)."""
        shape = rot.shape[:-2]
        parts = [rot, rt.to(rot.device).broadcast_to(*shape + rt.shape[-1:]), vel.to(rot.device), avel.to(rot.device)]
        return torch.cat([x.reshape(*(shape + (-1,))) for x in parts], dim=-1)

    def to_dict(self):
        def arr(x):
            x = x.detach().cpu().numpy()
            return {"arr": x, "context": {"dtype": x.dtype.name}}
        return OrderedDict([("rotation", arr(self.rotation)), ("root_translation", arr(self.root_translation)),
                            ("global_velocity", arr(self.global_velocity)),
                            ("global_angular_velocity", arr(self.global_angular_velocity)),
                            ("skeleton_tree", self.skeleton_tree.to_dict()), ("is_local", self.is_local),
                            ("fps", self.fps)])

    @classmethod
    def from_dict(cls, dict_repr, *args, **kwargs):
        """skeleton3d.py:1061-1071"""
        def arr(d):
            return torch.from_numpy(np.asarray(d["arr"]).astype(d["context"]["dtype"]))
        return cls(SkeletonMotion._to_state_vector(arr(dict_repr["rotation"]), arr(dict_repr["root_translation"]),
                                                   arr(dict_repr["global_velocity"]),
                                                   arr(dict_repr["global_angular_velocity"])),
                   skeleton_tree=SkeletonTree.from_dict(dict_repr["skeleton_tree"]), is_local=dict_repr["is_local"],
                   fps=dict_repr["fps"])


class MotionDICT:
    """Global translations + skeleton tree, indexable by frame (skeleton3d.py:1295-1315; the viewers' input)."""

    def __init__(self, gt, sk_tree, get_state=False) -> None:
        self.global_translation = as_tensor(gt).clone()
        self.skeleton_tree = sk_tree
        if not get_state and self.global_translation.dim() == 2:
            self.global_translation = self.global_translation[None, ...]

    def clone(self):
        return MotionDICT(self.global_translation.clone(), self.skeleton_tree)

    def __getitem__(self, t):
        return MotionDICT(self.global_translation[t].clone(), self.skeleton_tree, get_state=True)

    def __len__(self):
        return self.global_translation.shape[0]


def load_skeleton_state(path: str) -> SkeletonState:
    """Load a reference ``SkeletonState`` pickle WITHOUT unpickling (opcode walker, rtg.safe_pickle)."""
    d = load_skeleton_state_arrays(path)
    tree = SkeletonTree(d["node_names"], torch.from_numpy(d["parent_indices"]),
                        torch.from_numpy(d["local_translation"]), torch.from_numpy(d["quat"]))
    return SkeletonState(torch.from_numpy(d["tensor"]), tree, d["is_local"])

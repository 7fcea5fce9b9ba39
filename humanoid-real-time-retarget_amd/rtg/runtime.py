"""Device runtime: tensor plumbing, topology and solver handles.

PyTorch is used only for device memory and streams: tensors are handed to the
C ABI as raw device pointers plus the current HIP stream (``torch.cuda`` is HIP
on ROCm).  Every compute call goes to ``librtg_hip.so``; there is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import check, lib


def require_gpu_rtg() -> torch.device:
    """require_gpu for the entry points that report every failure as an RtgError (retarget_to)."""
    try:
        return require_gpu()
    except _lib.RtgError:
        raise
    except (RuntimeError, ImportError) as e:
        raise _lib.RtgError(2, str(e)) from e   # RTG_ERR_DEVICE


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("humanoid-real-time-retarget_amd: no HIP device visible; the retarget path runs only on "
                           "MI355X (gfx950) -- there is no CPU fallback")
    lib()
    return torch.device("cuda", torch.cuda.current_device())


def stream_handle(stream: Optional[torch.cuda.Stream] = None) -> ctypes.c_void_p:
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def dev_f32(x, shape_tail: Sequence[int] = (), name: str = "tensor") -> torch.Tensor:
    """Contiguous float32 device tensor (copies host data / other dtypes)."""
    dev = require_gpu()
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.device != dev or t.dtype != torch.float32:
        t = t.to(device=dev, dtype=torch.float32)
    t = t.contiguous()
    tail = tuple(shape_tail)
    if tail and tuple(t.shape[-len(tail):]) != tail:
        raise ValueError(f"{name}: expected trailing shape {tail}, got {tuple(t.shape)}")
    return t


def ptr(t: Optional[torch.Tensor]) -> Optional[ctypes.c_void_p]:
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _host_f32(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _host_i32(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


class Handle:
    """What the classes that own one handle of the C ABI share: ``_h``, the ``handle`` property, and its release
    through the library's ``_destroy`` symbol when the object goes (unless the library went first, at shutdown)."""
    _destroy = ""   # e.g. "rtg_topology_destroy"
    _h = None

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib._lib is not None:
            getattr(_lib._lib, self._destroy)(h)
            self._h = None


class Topology(Handle):
    """A parent-indexed skeleton resident on the device (``rtg_topology_t``)."""
    _destroy = "rtg_topology_destroy"

    def __init__(self, parent_indices, local_translation, tree_quat=None):
        require_gpu()
        p = _host_i32(parent_indices)
        lt = _host_f32(local_translation).reshape(-1, 3)
        tq = None if tree_quat is None else _host_f32(tree_quat).reshape(-1, 4)
        J = int(p.shape[0])
        if lt.shape[0] != J or (tq is not None and tq.shape[0] != J):
            raise ValueError("parent_indices / local_translation / quat lengths differ")   # skeleton3d.py:87-88
        h = ctypes.c_void_p()
        check(lib().rtg_topology_create(p.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        lt.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                        None if tq is None else tq.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                        J, ctypes.byref(h)))
        self._h = h
        self.num_joints = J
        self.parents = p
        self.local_translation = lt


class DofModel(Handle):
    """A joint-angle forward model (``rtg_dof_model_t``, HuForwardModel hu_forward_model.py:13-33):
    a topology, one rotation axis per DOF (0/1/2) and optional DOF limits."""
    _destroy = "rtg_dof_model_destroy"

    def __init__(self, topo: Topology, axis, lower=None, upper=None):
        require_gpu()
        ax = _host_i32(axis)
        n = topo.num_joints - 1
        if ax.shape[0] != n:
            raise ValueError(f"{ax.shape[0]} DOF axes for a {topo.num_joints}-joint topology (need {n})")
        lo = hi = None
        if (lower is None) != (upper is None):
            raise ValueError("give both DOF limit tables or neither")
        if lower is not None:
            lo, hi = _host_f32(lower).reshape(-1), _host_f32(upper).reshape(-1)
            if lo.shape[0] != n or hi.shape[0] != n:   # the reference's torch.clamp would fail to broadcast
                raise ValueError(f"DOF limits hold {lo.shape[0]}/{hi.shape[0]} entries for {n} DOFs")
        fp = ctypes.POINTER(ctypes.c_float)
        h = ctypes.c_void_p()
        check(lib().rtg_dof_model_create(topo.handle, ax.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                         None if lo is None else lo.ctypes.data_as(fp),
                                         None if hi is None else hi.ctypes.data_as(fp), ctypes.byref(h)))
        self._h = h
        self.topo = topo   # borrowed by the handle: keep it alive
        self.num_dofs = n
        self.has_limits = lo is not None


def retarget_tables(src_parents, tgt_parents, src_joint, tgt_joint) -> dict:
    """rtg_retarget_plan_tables (host only, no GPU needed): the tables of a retarget_to plan -- kept_src, kept_tgt,
    src_reduced_parents, tgt_reduced_parents, perm (K each) and src_of (J_t) -- as int32 arrays.  A bad mapping raises
    RtgError with the reference's assertion text."""
    sp, tp, sj, tj = (_host_i32(a).reshape(-1) for a in (src_parents, tgt_parents, src_joint, tgt_joint))
    if sj.shape != tj.shape:
        raise ValueError("src_joint / tgt_joint lengths differ")
    K, Jt = int(sj.shape[0]), int(tp.shape[0])
    out = {k: np.zeros(max(n, 1), np.int32) for k, n in (("kept_src", K), ("src_reduced_parents", K), ("kept_tgt", K),
                                                         ("tgt_reduced_parents", K), ("perm", K), ("src_of", Jt))}
    ip = ctypes.POINTER(ctypes.c_int32)
    check(lib().rtg_retarget_plan_tables(sp.ctypes.data_as(ip), int(sp.shape[0]), tp.ctypes.data_as(ip), Jt,
                                         sj.ctypes.data_as(ip), tj.ctypes.data_as(ip), K,
                                         *(out[k].ctypes.data_as(ip) for k in ("kept_src", "src_reduced_parents",
                                                                               "kept_tgt", "tgt_reduced_parents",
                                                                               "perm", "src_of"))))
    return {k: v[:(Jt if k == "src_of" else K)] for k, v in out.items()}


class RetargetPlan(Handle):
    """Everything of a ``SkeletonState.retarget_to`` call that does not depend on the frame (``rtg_retarget_plan_t``):
    the two trees, the joint mapping as index pairs, both t-poses, rotation_to_target_skeleton and the scale."""
    _destroy = "rtg_retarget_plan_destroy"

    def __init__(self, src: Topology, tgt: Topology, src_joint, tgt_joint, src_tpose_local_rot, src_tpose_root_t,
                 tgt_tpose_local_rot, tgt_tpose_root_t, rotation_to_target, scale: float):
        require_gpu_rtg()
        sj, tj = _host_i32(src_joint).reshape(-1), _host_i32(tgt_joint).reshape(-1)
        if sj.shape != tj.shape:
            raise ValueError("src_joint / tgt_joint lengths differ")
        arrs = []
        for a, n, name in ((src_tpose_local_rot, src.num_joints * 4, "source t-pose rotations"),
                           (src_tpose_root_t, 3, "source t-pose root translation"),
                           (tgt_tpose_local_rot, tgt.num_joints * 4, "target t-pose rotations"),
                           (tgt_tpose_root_t, 3, "target t-pose root translation"),
                           (rotation_to_target, 4, "rotation_to_target_skeleton")):
            a = _host_f32(a).reshape(-1)
            if a.shape[0] != n:
                raise ValueError(f"{name}: expected {n} values (a single pose), got {a.shape[0]}")
            arrs.append(a)
        ip, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        h = ctypes.c_void_p()
        check(lib().rtg_retarget_plan_create(src.handle, tgt.handle, sj.ctypes.data_as(ip), tj.ctypes.data_as(ip),
                                             int(sj.shape[0]), *(a.ctypes.data_as(fp) for a in arrs),
                                             ctypes.c_float(float(scale)), ctypes.byref(h)))
        self._h = h
        self.src, self.tgt = src, tgt
        self.num_source_joints, self.num_target_joints = src.num_joints, tgt.num_joints
        self.device = torch.device("cuda", torch.cuda.current_device())   # owns the constants (rtg.h)


def fit_targets_tables(num_source_joints: int, tgt_parents, tgt_local_translation, src_joint, tgt_joint) -> dict:
    """rtg_fit_targets_plan_tables (host only, no GPU needed): the tables of a keypoint-target plan -- anchor (K) the
    pair of the nearest mapped proper ancestor (-1: the root pair), seg (K, 3) the target zero pose's segment between
    the two, weight (J_t) 1 for a mapped link, src_of (J_t) the pair of a link's nearest mapped ancestor-or-self.  Pairs
    are numbered as given.  A bad mapping raises RtgError with the reason."""
    tp, sj, tj = (_host_i32(a).reshape(-1) for a in (tgt_parents, src_joint, tgt_joint))
    lt = _host_f32(tgt_local_translation).reshape(-1, 3)
    if sj.shape != tj.shape:
        raise ValueError("src_joint / tgt_joint lengths differ")
    if lt.shape[0] != tp.shape[0]:
        raise ValueError("parent_indices / local_translation lengths differ")
    K, Jt = int(sj.shape[0]), int(tp.shape[0])
    out = {"anchor": np.zeros(max(K, 1), np.int32), "seg": np.zeros((max(K, 1), 3), np.float32),
           "weight": np.zeros(max(Jt, 1), np.float32), "src_of": np.zeros(max(Jt, 1), np.int32)}
    ip, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    check(lib().rtg_fit_targets_plan_tables(int(num_source_joints), tp.ctypes.data_as(ip), lt.ctypes.data_as(fp), Jt,
                                            sj.ctypes.data_as(ip), tj.ctypes.data_as(ip), K,
                                            out["anchor"].ctypes.data_as(ip), out["seg"].ctypes.data_as(fp),
                                            out["weight"].ctypes.data_as(fp), out["src_of"].ctypes.data_as(ip)))
    return {k: v[:(K if k in ("anchor", "seg") else Jt)] for k, v in out.items()}


class FitTargetsPlan(Handle):
    """Everything of a keypoint-target launch that does not depend on the frame (``rtg_fit_targets_plan_t``): the two
    trees, the joint mapping as index pairs and the constants dir / root_scale / root_offset (3 floats each or None).
    ``weight`` (J_t,) is the pose fit's weight mask of the mapped links; ``tables`` the host tables."""
    _destroy = "rtg_fit_targets_plan_destroy"

    def __init__(self, src: Topology, tgt: Topology, src_joint, tgt_joint, dir=None, root_scale=None, root_offset=None):
        require_gpu_rtg()
        sj, tj = _host_i32(src_joint).reshape(-1), _host_i32(tgt_joint).reshape(-1)
        if sj.shape != tj.shape:
            raise ValueError("src_joint / tgt_joint lengths differ")
        consts = []
        for a, name in ((dir, "dir"), (root_scale, "root_scale"), (root_offset, "root_offset")):
            a = None if a is None else _host_f32(a).reshape(-1)
            if a is not None and a.shape[0] != 3:
                raise ValueError(f"{name}: expected 3 values, got {a.shape[0]}")
            consts.append(a)
        ip, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        h = ctypes.c_void_p()
        check(lib().rtg_fit_targets_plan_create(src.handle, tgt.handle, sj.ctypes.data_as(ip), tj.ctypes.data_as(ip),
                                                int(sj.shape[0]),
                                                *(None if a is None else a.ctypes.data_as(fp) for a in consts),
                                                ctypes.byref(h)))
        self._h = h
        self.src, self.tgt = src, tgt
        self.num_source_joints, self.num_target_joints = src.num_joints, tgt.num_joints
        self.src_joint, self.tgt_joint = sj, tj
        self.dir, self.root_scale, self.root_offset = consts
        self.tables = fit_targets_tables(src.num_joints, tgt.parents, tgt.local_translation, sj, tj)
        self.weight = self.tables["weight"]
        self.device = torch.device("cuda", torch.cuda.current_device())   # owns the tables (rtg.h)


class MotionLib(Handle):
    """The clip table of a motion library (``rtg_motion_lib_t``): per clip its first row in the packed arrays, its
    length in frames and its frame rate.  The arrays themselves stay with the caller (``ops.motion_sample``).  The
    table is validated on the host first: a bad one raises RtgError with the reason, GPU or not."""
    _destroy = "rtg_motion_lib_destroy"

    def __init__(self, start, length, fps, total_frames: int):
        s = np.ascontiguousarray(np.asarray(start, dtype=np.int64).reshape(-1))
        n = _host_i32(length).reshape(-1)
        f = _host_f32(fps).reshape(-1)
        if not (s.shape == n.shape == f.shape):
            raise ValueError("start / length / fps lengths differ")
        h = ctypes.c_void_p()
        check(lib().rtg_motion_lib_create(s.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                          n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          f.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(s.shape[0]),
                                          int(total_frames), ctypes.byref(h)))
        self._h = h
        self.num_clips = int(s.shape[0])
        self.total_frames = int(total_frames)
        self.start, self.length, self.fps = s, n, f
        self.device = torch.device("cuda", torch.cuda.current_device())   # owns the table (rtg.h)


# Frames the reference raises on (rtg.h rtg_frame_error): the batched solve marks them -- every dof of the row NaN,
# dof[f, 0] = RTG_FRAME_NAN | code -- and the per-frame calls raise what the reference raises.
FRAME_ERRORS = {
    # transform3d.py:40: eager torch.linalg.svd raises torch.linalg.LinAlgError naming the batch element; through the
    # reference's @torch.jit.script cal_joint_quat it surfaces as a plain RuntimeError.  LinAlgError subclasses
    # RuntimeError, so callers catching either form see it
    _lib.FRAME_SVD_NONFINITE: (torch.linalg.LinAlgError, "linalg.svd: (Batch element {i}): The algorithm failed to "
                                                         "converge because the input matrix contained non-finite values."),
    _lib.FRAME_ZERO_NORM_QUAT: (ValueError, "Found zero norm quaternions in `quat`."),           # transform3d.py:53
}


def frame_status(dof: torch.Tensor) -> torch.Tensor:
    """Per-frame rtg_frame_error code (int8, dof's device) of solver outputs dof (..., 30): 0 where the reference
    returns a result, 1 where its torch.linalg.svd raises, 2 where scipy's from_quat raises."""
    d0 = dof[..., 0].contiguous().view(torch.int32)
    marked = (d0 & ~0xF) == _lib.FRAME_NAN
    return torch.where(marked, d0 & 0xF, torch.zeros_like(d0)).to(torch.int8)


def raise_frame_error(code: int, index: int = 0) -> None:
    """Raise the exception the reference raises on a frame with this rtg_frame_error code (no-op for 0).  index is
    the batch element torch names in the SVD message: 0 for the reference's per-frame (1, 3, 3) call, the first
    marked element for a batched primitive call."""
    code = int(code)
    if code:
        exc, msg = FRAME_ERRORS.get(code, (RuntimeError, f"rtg frame error {code}"))
        raise exc(msg.format(i=int(index)))


# per-frame input rows of each solver kind (rtg.h rtg_solver_kind): (points, components)
IN_TAILS = {_lib.SOLVER_FULL_BODY_POS: [(21, 3), (20, 3), (20, 3)], _lib.SOLVER_UPPER_BODY: [(21, 3)],
            _lib.SOLVER_FULL_BODY_ROT: [(21, 4), (21, 3), (20, 3), (20, 3)], _lib.SOLVER_BODY_ROT: [(21, 4)]}
LAYOUTS = {"aos": _lib.LAYOUT_AOS, "soa": _lib.LAYOUT_SOA}


def layout_code(layout) -> int:
    if isinstance(layout, str):
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
        return LAYOUTS[layout]
    if int(layout) not in LAYOUTS.values():
        raise ValueError(f"bad layout {layout!r}")
    return int(layout)


class Solver(Handle):
    """A retarget solver (``rtg_solver_t``) of one of the four reference kinds."""
    _destroy = "rtg_solver_destroy"

    N_INPUTS = {k: len(v) for k, v in IN_TAILS.items()}

    def __init__(self, kind: int, src_local_t, src_global_t=None, src_parents=None, precise_gripper=False):
        require_gpu()
        lt = _host_f32(src_local_t).reshape(-1, 3)
        gt = None if src_global_t is None else _host_f32(src_global_t).reshape(-1, 3)
        par = None if src_parents is None else _host_i32(src_parents)
        h = ctypes.c_void_p()
        fp = ctypes.POINTER(ctypes.c_float)
        check(lib().rtg_solver_create(int(kind), lt.ctypes.data_as(fp), None if gt is None else gt.ctypes.data_as(fp),
                                      None if par is None else par.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      int(lt.shape[0]), int(bool(precise_gripper)), ctypes.byref(h)))
        self._h = h
        self.kind = int(kind)
        self.precise_gripper = bool(precise_gripper)
        self.device = torch.device("cuda", torch.cuda.current_device())   # owns the angle table (rtg.h)

    def retarget(self, inputs: Sequence[torch.Tensor], want_local_rot=False, want_body_rot=False,
                 out_dof: Optional[torch.Tensor] = None, stream=None, layout="aos"):
        """Batched solve.  ``inputs``: contiguous float32 tensors on the solver's device, in the order of rtg.h,
        shaped (B, P, C) per IN_TAILS (``layout="aos"``, the reference's rows) or (P, C, B) (``"soa"``).

        Returns (dof (B,30), local_rot (B,31,4) | None, body_rot (B,59,4) | None).
        """
        n = self.N_INPUTS[self.kind]
        if len(inputs) != n:
            raise ValueError(f"solver kind {self.kind} takes {n} inputs, got {len(inputs)}")
        code = layout_code(layout)
        tails = IN_TAILS[self.kind]
        soa = code == _lib.LAYOUT_SOA
        B = int(inputs[0].shape[-1] if soa else inputs[0].shape[0]) if inputs[0].dim() == 3 else -1
        for i, (t, tail) in enumerate(zip(inputs, tails)):
            want = tuple(tail) + (B,) if soa else (B,) + tuple(tail)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != want:
                raise ValueError(f"input {i}: expected shape {want} ({'SoA' if soa else 'AoS'}), got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"input {i}: must be a contiguous float32 device tensor")
            if t.device != self.device:
                raise ValueError(f"input {i} is on {t.device}; this solver lives on {self.device}")
        dev = self.device
        if out_dof is not None:
            if not (isinstance(out_dof, torch.Tensor) and tuple(out_dof.shape) == (B, 30) and
                    out_dof.dtype == torch.float32 and out_dof.is_contiguous() and out_dof.device == dev):
                raise ValueError(f"out_dof must be a contiguous float32 ({B}, 30) tensor on {dev}")
            dof = out_dof
        else:
            dof = torch.empty((B, 30), device=dev, dtype=torch.float32)
        lr = torch.empty((B, 31, 4), device=dev, dtype=torch.float32) if want_local_rot else None
        br = torch.empty((B, 59, 4), device=dev, dtype=torch.float32) if want_body_rot else None
        ins = [ptr(t) for t in inputs] + [None] * (4 - n)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        check(lib().rtg_retarget_f32(self._h, ins[0], ins[1], ins[2], ins[3], B, code, ptr(dof), ptr(lr), ptr(br),
                                     stream_handle(s)))
        return dof, lr, br

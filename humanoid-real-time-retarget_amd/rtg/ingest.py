"""VTRDyn ingest: the data formats in front of the retarget solver.

* Socket frames (mocap_communication/mocap_receiver.py:21-26, 49-59): a 4-byte
  big-endian length, then a pickled ``dict`` of float32 arrays ``body_pos``
  (23,3), ``body_quat`` (23,4), ``left_hand_pos`` / ``right_hand_pos`` (20,3).
  The reference ``pickle.loads`` the network bytes, which runs whatever the
  sender names.  :func:`decode_frame` walks the opcodes instead
  (:mod:`rtg.safe_pickle`) and rebuilds arrays only through numpy's own
  reconstructors, from raw bytes; any other callable is rejected.
* CSV recordings (retarget/utils/parse_mocap.py:26-62): one column per joint
  and axis, ``"{joint} position X(m)"`` / ``"{joint} quaternion X"``.
* Reindexing (sim_full_body_teleop.py:109-112): the 23-joint broadcast body to
  the 21-joint VTRDYN order, the 20-point hands to the solver's order.  Batches
  are gathered on the device (``rtg_ingest_vtrdyn_f32``), which also flags the
  frames the teleop loop skips (``np.allclose(body_pos, 0)``, :92).
* Rotations (retarget/utils/parse_mocap.py:65-134, zero_pose_transform.py:16-41, sim_full_body_teleop.py:97-106):
  the zero-pose transform every caller puts recorded quaternions through before a rotation solver,
  ``quat_mul_norm(quat_mul_norm(q, r), quat_inverse(t2zero))``, as one launch (:class:`ZeroPoseTransform`,
  ``rtg_rot_ingest_f32``) with the row gather of the broadcast folded in, and the reference's functions by name.
"""
from __future__ import annotations

import ctypes
import io
import math
import pickle
import struct
from typing import Any, Dict, Optional

import numpy as np
import torch

from ._lib import LAYOUT_SOA, check, lib
from .bridge import as_tensor, back
from .runtime import Handle, _host_f32, _host_i32, dev_f32, layout_code, ptr, stream_handle
from .safe_pickle import Call, Global, Obj, _run_vm

# sim_full_body_teleop.py:109 (23 -> 21) and :111-112 (hand point order)
BODY23_TO_21 = [0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22]
HAND_ORDER = [0, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 12, 13, 14, 15, 1, 2, 3]
FRAME_KEYS = {"body_pos": (23, 3), "body_quat": (23, 4), "left_hand_pos": (20, 3), "right_hand_pos": (20, 3)}

_RECONSTRUCT = {("numpy.core.multiarray", "_reconstruct"), ("numpy._core.multiarray", "_reconstruct")}
_FROMBUFFER = {("numpy.core.numeric", "_frombuffer"), ("numpy._core.numeric", "_frombuffer")}
_SCALAR = {("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar")}


def _is(g: Any, names) -> bool:
    return isinstance(g, Global) and (g.module, g.name) in names


def _dtype(node: Any) -> np.dtype:
    """numpy.dtype(code, align, copy) + its BUILD state (version, byte order, ...)."""
    if not (isinstance(node, Call) and _is(node.func, {("numpy", "dtype")})):
        raise ValueError("expected a numpy dtype record")
    dt = np.dtype(str(node.args[0]))
    st = node.state
    if isinstance(st, tuple) and len(st) > 1 and st[1] in ("<", ">"):
        dt = dt.newbyteorder(st[1])
    if dt.hasobject:
        raise ValueError("object arrays are not accepted")
    return dt


def _value(node: Any) -> Any:
    """Inert tree -> Python / numpy values; only numpy array / scalar reconstructors are honoured."""
    if isinstance(node, dict):
        return {_value(k): _value(v) for k, v in node.items()}
    if isinstance(node, list):
        return [_value(v) for v in node]
    if isinstance(node, tuple):
        return tuple(_value(v) for v in node)
    if isinstance(node, (str, int, float, bool, bytes, type(None))):
        return node
    if isinstance(node, bytearray):
        return bytes(node)
    if isinstance(node, Call):
        if _is(node.func, _RECONSTRUCT):   # protocol <= 4: _reconstruct(ndarray, (0,), b'b') + __setstate__
            _ver, shape, dt, fortran, raw = node.state
            raw = _value(raw)
            a = np.frombuffer(raw, dtype=_dtype(dt)).reshape(tuple(shape), order="F" if fortran else "C")
            return a.copy()
        if _is(node.func, _FROMBUFFER):    # protocol 5, in-band buffer
            buf, dt, shape, order = node.args
            return np.frombuffer(bytes(buf), dtype=_dtype(dt)).reshape(tuple(shape), order=order).copy()
        if _is(node.func, _SCALAR):
            dt, raw = node.args
            return np.frombuffer(_value(raw), dtype=_dtype(dt))[0]
        if _is(node.func, {("_codecs", "encode")}) and len(node.args) == 2 and node.args[1] == "latin1":
            return str(node.args[0]).encode("latin1")   # protocol 2 spelling of bytes
        raise ValueError(f"refusing to call {getattr(node.func, 'qualname', node.func)!r} from a mocap frame")
    if isinstance(node, Obj):
        raise ValueError("refusing to instantiate objects from a mocap frame")
    raise ValueError(f"unsupported value {type(node).__name__} in a mocap frame")


def decode_frame(payload: bytes) -> Dict[str, np.ndarray]:
    """One frame payload (the bytes after the length prefix) -> dict of float32 arrays, executing nothing."""
    d = _value(_run_vm(io.BytesIO(payload)))
    if not isinstance(d, dict):
        raise ValueError("mocap frame is not a dict")
    out = {}
    for k, shape in FRAME_KEYS.items():
        if k in d:
            a = np.asarray(d[k], dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"{k}: expected {shape}, got {a.shape}")
            out[k] = a
    return out


def encode_frame(frame: Dict[str, np.ndarray]) -> bytes:
    """The sender side: 4-byte big-endian length + pickled dict (mocap_receiver.py:49-59)."""
    body = pickle.dumps({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in frame.items()})
    return struct.pack(">I", len(body)) + body


def read_frame(sock) -> Optional[Dict[str, np.ndarray]]:
    """Read one length-prefixed frame from a connected stream socket; None when the peer closed."""
    def recv_n(n):
        data = b""
        while len(data) < n:
            pkt = sock.recv(n - len(data))
            if not pkt:
                return None
            data += pkt
        return data

    hdr = recv_n(4)
    if hdr is None:
        return None
    body = recv_n(int.from_bytes(hdr, "big"))
    return None if body is None else decode_frame(body)


# ---------------------------------------------------------------- CSV recordings (parse_mocap.py:26-62)
def _columns(df, names, fields) -> np.ndarray:
    out = np.zeros((len(df), len(names), len(fields)))        # float64, as the reference
    for j, name in enumerate(names):
        for c, field in enumerate(fields):
            out[:, j, c] = df[f"{name} {field}"]
    return out


_POS = ("position X(m)", "position Y(m)", "position Z(m)")
_QUAT = ("quaternion X", "quaternion Y", "quaternion Z", "quaternion W")


def get_vtrdyn_translation(df) -> np.ndarray:
    from retarget.robot_config import VTRDYN
    return _columns(df, VTRDYN.VTRDYN_JOINT_NAMES, _POS)


def get_vtrdyn_rotation(df) -> np.ndarray:
    from retarget.robot_config import VTRDYN
    return _columns(df, VTRDYN.VTRDYN_JOINT_NAMES, _QUAT)


def get_vtrdyn_full_translation(df) -> np.ndarray:
    from retarget.robot_config import VTRDYN_FULL
    return _columns(df, VTRDYN_FULL.VTRDYN_JOINT_NAMES, _POS)


def get_vtrdyn_full_rotation(df) -> np.ndarray:
    from retarget.robot_config import VTRDYN_FULL
    return _columns(df, VTRDYN_FULL.VTRDYN_JOINT_NAMES, _QUAT)


# ---------------------------------------------------------------- batched device reindex
def reindex_frames(body23, left20, right20, layout="aos"):
    """(B,23,3), (B,20,3), (B,20,3) raw broadcast frames -> solver inputs (B,21,3), (B,20,3), (B,20,3) and a
    (B,) bool "frame carries data" flag (not np.allclose(body_pos, 0)), gathered on the device.  ``layout="soa"``
    emits the solver inputs as component planes (21,3,B), (20,3,B), (20,3,B) directly (rtg.h rtg_layout)."""
    b = dev_f32(body23, (23, 3), "body_pos")
    lh = dev_f32(left20, (20, 3), "left_hand_pos")
    rh = dev_f32(right20, (20, 3), "right_hand_pos")
    B = int(b.shape[0])
    if lh.shape[0] != B or rh.shape[0] != B:
        raise ValueError("frame batches differ in length")
    code = layout_code(layout)
    soa = code == LAYOUT_SOA
    ob = torch.empty((21, 3, B) if soa else (B, 21, 3), device=b.device, dtype=torch.float32)
    ol = torch.empty((20, 3, B) if soa else (B, 20, 3), device=b.device, dtype=torch.float32)
    orr = torch.empty((20, 3, B) if soa else (B, 20, 3), device=b.device, dtype=torch.float32)
    valid = torch.empty((B,), device=b.device, dtype=torch.uint8)
    check(lib().rtg_ingest_vtrdyn_f32(ptr(b), ptr(lh), ptr(rh), B, code, ptr(ob), ptr(ol), ptr(orr), ptr(valid),
                                      stream_handle()))
    return ob, ol, orr, valid.bool()

# ---------------------------------------------------------------- rotations: the zero-pose transform
# frames per block of k_rot_ingest, AoS / SoA out (csrc/rtg_knobs.h RTG_ROT_INGEST_TILE_AOS / _SOA; rtg_build_info
# reports the library's): the batch sizes at which the kernel's last tile changes shape
ROT_TILE_AOS = 16
ROT_TILE_SOA = 16
# sim_full_body_teleop.py:100, 102: where the 21 body joints sit in the 59-joint VTRDYN_FULL order
BODY21_IN_FULL59 = [0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 34, 35, 36, 37, 38, 39, 11, 12, 13, 14]
_HALF_PI = math.pi / 2
_X, _Z = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
# the four arm joints turned a quarter turn in the zero-pose tree (parse_mocap.py:73-76, :98-101): joint, angle, axis
_T2ZERO_EDITS = {
    "vtrdyn": ((18, -_HALF_PI, _X), (19, -_HALF_PI, _Z), (14, _HALF_PI, _X), (15, _HALF_PI, _Z)),
    "vtrdyn_full": ((12, -_HALF_PI, _X), (13, -_HALF_PI, _Z), (37, _HALF_PI, _X), (38, _HALF_PI, _Z)),
}
_T2ZERO: dict = {}


def _axis_quat(angle: float, axis) -> np.ndarray:
    """quat_from_angle_axis(torch.tensor(angle), torch.tensor(axis)) as the reference calls it, (4,) float32."""
    from poselib.poselib.core.rotation3d import quat_from_angle_axis
    return _host_f32(quat_from_angle_axis(torch.tensor(angle), torch.tensor(axis, dtype=torch.float32))).reshape(4)


def t2zero_pose_transform_quat(asset: str) -> np.ndarray:
    """``vtrdyn_t2zero_pose_transform_quat`` ("vtrdyn", (21,4)) / ``vtrdyn_full_t2zero_pose_transform_quat``
    ("vtrdyn_full", (59,4)) of parse_mocap.py:65-104: the global rotations of the tree under identity local rotations
    with four arm joints turned a quarter turn.  The reference builds them from its t-pose pickles, which have the
    zero-pose assets' parents, node order and rotations and differ only in local_translation; a global rotation does
    not depend on translations, so the package's zero-pose assets give the same rows.  rebuild_pose_by_local_rotation
    overwrites its pose's translations: the pose built here is private.  Computed once, on the device."""
    if asset not in _T2ZERO:
        from robot_kinematics_model import RobotZeroPose
        pose = RobotZeroPose.from_asset(asset)
        lr = pose.local_rotation
        for j, angle, axis in _T2ZERO_EDITS[asset]:
            lr[j] = torch.from_numpy(_axis_quat(angle, axis))
        _T2ZERO[asset] = _host_f32(pose.rebuild_pose_by_local_rotation(lr))
    return _T2ZERO[asset].copy()


def _conj(q: np.ndarray) -> np.ndarray:
    return (q * np.array([-1.0, -1.0, -1.0, 1.0], np.float32)).astype(np.float32)   # quat_inverse, rotation3d.py:214-219


class _RotIngestHandle(Handle):
    """One ``rtg_rot_ingest_t``: a transform's constants on the current device."""
    _destroy = "rtg_rot_ingest_destroy"

    def __init__(self, J_in: int, src, pre, post):
        ip, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
        h = ctypes.c_void_p()
        check(lib().rtg_rot_ingest_create(J_in, int(post.shape[0]), None if src is None else src.ctypes.data_as(ip),
                                          pre.ctypes.data_as(fp), post.ctypes.data_as(fp), ctypes.byref(h)))
        self._h = h


class ZeroPoseTransform:
    """``out[f, j] = quat_mul_norm(quat_mul_norm(q[f, src[j]], pre), post[j])`` as one fused launch
    (``rtg_rot_ingest_t``): ``pre`` (4) one axis rotation, ``post`` (J_out, 4) the conjugated zero-pose rows, ``src``
    (J_out) the input row of every output joint (None: the identity).  The named constructors build their constants
    on first use; the device handle is created on first call, per device."""

    def __init__(self, J_in: int, src=None, pre=None, post=None, _build=None):
        self.J_in = int(J_in)
        self._build = _build
        self._handles: dict = {}
        if _build is None:
            self._set(src, pre, post)

    def _set(self, src, pre, post):
        self._pre = _host_f32(pre).reshape(-1)
        self._post = _host_f32(post)
        if self._pre.shape != (4,) or self._post.ndim != 2 or self._post.shape[1] != 4:
            raise ValueError("pre must hold 4 values and post (J_out, 4)")
        self._src = None if src is None else _host_i32(src).reshape(-1)
        if self._src is not None and self._src.shape[0] != self._post.shape[0]:
            raise ValueError("src and post differ in length")

    def _consts(self):
        if self._build is not None:
            build, self._build = self._build, None
            self._set(*build())
        return self._src, self._pre, self._post

    @property
    def src(self):
        s = self._consts()[0]
        return np.arange(self.J_in, dtype=np.int32) if s is None else s.copy()

    @property
    def pre(self) -> np.ndarray:
        return self._consts()[1].copy()

    @property
    def post(self) -> np.ndarray:
        return self._consts()[2].copy()

    @property
    def J_out(self) -> int:
        return int(self._consts()[2].shape[0])

    # ---- the reference's transforms
    @classmethod
    def vtrdyn(cls):
        """vtrdyn_zero_pose_transform (parse_mocap.py:106-114; zero_pose_transform_quat): 21 -> 21."""
        return cls(21, _build=lambda: (None, _axis_quat(_HALF_PI, _Z), _conj(t2zero_pose_transform_quat("vtrdyn"))))

    @classmethod
    def vtrdyn_full(cls):
        """vtrdyn_full_zero_pose_transform (parse_mocap.py:81-89): 59 -> 59."""
        return cls(59, _build=lambda: (None, _axis_quat(_HALF_PI, _Z),
                                       _conj(t2zero_pose_transform_quat("vtrdyn_full"))))

    @classmethod
    def vtrdyn_broadcast(cls, reindex: bool = True):
        """vtrdyn_broadcast_zero_pose_transform (parse_mocap.py:126-134) on the broadcast's raw 23 rows, the 23 -> 21
        gather of sim_full_body_teleop.py:105 folded in; reindex=False: the reference's function itself, 21 -> 21."""
        return cls(23 if reindex else 21, _build=lambda: (
            BODY23_TO_21 if reindex else None, _axis_quat(_HALF_PI, _X), _conj(t2zero_pose_transform_quat("vtrdyn"))))

    @classmethod
    def vtrdyn_full_from_broadcast(cls):
        """sim_full_body_teleop.py:97-102: the raw 23 rows gathered to 21, scattered into an identity 59-joint pose,
        through vtrdyn_full_zero_pose_transform, and the 21 body rows gathered back -- the 59-joint constants at the
        body joints' indices; the other 38 rows never reach the result."""
        return cls(23, _build=lambda: (BODY23_TO_21, _axis_quat(_HALF_PI, _Z),
                                       _conj(t2zero_pose_transform_quat("vtrdyn_full"))[BODY21_IN_FULL59]))

    # ---- device
    def _handle(self, dev: torch.device):
        key = dev.index
        if key not in self._handles:
            with torch.cuda.device(dev):
                self._handles[key] = _RotIngestHandle(self.J_in, *self._consts())
        return self._handles[key].handle

    def __call__(self, q, layout="aos") -> torch.Tensor:
        """q (..., J_in, 4), on the CPU or the device -> the transformed rotations on the device: (..., J_out, 4), or
        with layout="soa" the component planes (J_out, 4, B) a rotation solver reads (rtg.h rtg_layout)."""
        code = layout_code(layout)
        t = dev_f32(q, (self.J_in, 4), "q")
        lead = t.shape[:-2]
        B = int(torch.Size(lead).numel())
        Jo = self.J_out
        out = torch.empty((Jo, 4, B) if code == LAYOUT_SOA else tuple(lead) + (Jo, 4), device=t.device,
                          dtype=torch.float32)
        check(lib().rtg_rot_ingest_f32(self._handle(t.device), ptr(t), B, code, ptr(out), stream_handle()))
        return out


_NAMED: dict = {}


def _named(name: str, **kw) -> ZeroPoseTransform:
    key = (name, tuple(sorted(kw.items())))
    if key not in _NAMED:
        _NAMED[key] = getattr(ZeroPoseTransform, name)(**kw)
    return _NAMED[key]


def _drop_in(transform: ZeroPoseTransform, global_rotation):
    g = as_tensor(global_rotation)
    return back(transform(g), g.device)


def vtrdyn_zero_pose_transform(global_rotation):
    """parse_mocap.py:106-114: (..., 21, 4) -> (..., 21, 4), on the input's device."""
    return _drop_in(_named("vtrdyn"), global_rotation)


def vtrdyn_full_zero_pose_transform(global_rotation):
    """parse_mocap.py:81-89: (..., 59, 4) -> (..., 59, 4), on the input's device."""
    return _drop_in(_named("vtrdyn_full"), global_rotation)


def vtrdyn_broadcast_zero_pose_transform(global_rotation):
    """parse_mocap.py:126-134: (..., 21, 4), the broadcast's rows already gathered -> (..., 21, 4)."""
    return _drop_in(_named("vtrdyn_broadcast", reindex=False), global_rotation)


def zero_pose_transform_quat(global_rotation):
    """retarget_solver/zero_pose_transform.py:33-41: vtrdyn_zero_pose_transform under its other name."""
    return _drop_in(_named("vtrdyn"), global_rotation)


def ingest_rotations(body_quat23, transform: Optional[ZeroPoseTransform] = None, layout="aos"):
    """(B, 23, 4) raw broadcast ``body_quat`` -> the rotation solvers' (B, 21, 4) input (or (21, 4, B) planes), gathered
    and transformed in one launch.  transform: ZeroPoseTransform.vtrdyn_broadcast() (the default) or
    .vtrdyn_full_from_broadcast(), the two paths of sim_full_body_teleop.py:97-106."""
    tr = _named("vtrdyn_broadcast") if transform is None else transform
    if tr.J_in != 23:
        raise ValueError(f"ingest_rotations needs a transform of the 23-row broadcast, got J_in = {tr.J_in}")
    return tr(body_quat23, layout)


def hold_last_valid(dof: torch.Tensor, valid: torch.Tensor, last: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The teleop loop's fallback (sim_full_body_teleop.py:92, 121-123): a frame without data repeats the
    previous frame's DOFs (``last`` before the first one; zeros by default, :86)."""
    B = dof.shape[0]
    idx = torch.where(valid, torch.arange(B, device=dof.device), torch.full((B,), -1, device=dof.device))
    src = torch.cummax(idx, dim=0).values
    prev = torch.zeros_like(dof[0]) if last is None else last.to(dof.device, dof.dtype)
    return torch.where((src >= 0).unsqueeze(-1), dof[src.clamp(min=0)], prev.expand_as(dof))


def stack_frames(frames) -> Dict[str, np.ndarray]:
    """List of decoded frames -> contiguous (B, ...) host arrays (pin them for asynchronous H2D copies)."""
    return {k: np.stack([f[k] for f in frames]).astype(np.float32) for k in ("body_pos", "left_hand_pos",
                                                                             "right_hand_pos")}


__all__ = ["BODY23_TO_21", "HAND_ORDER", "decode_frame", "encode_frame", "read_frame", "get_vtrdyn_translation",
           "get_vtrdyn_rotation", "get_vtrdyn_full_translation", "get_vtrdyn_full_rotation", "reindex_frames",
           "hold_last_valid", "stack_frames", "ROT_TILE_AOS", "ROT_TILE_SOA", "BODY21_IN_FULL59", "ZeroPoseTransform",
           "t2zero_pose_transform_quat", "vtrdyn_zero_pose_transform", "vtrdyn_full_zero_pose_transform",
           "vtrdyn_broadcast_zero_pose_transform", "zero_pose_transform_quat", "ingest_rotations"]

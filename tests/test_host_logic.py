"""CPU-only: the C ABI loads and exports every symbol rtg.h declares; host-side
validation mirrors the reference's assertions; the drop-in modules import
without a GPU and fail loudly (no CPU fallback) when asked to compute."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _declared_symbols():
    src = open(os.path.join(REPO, "include", "rtg.h")).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char \*)\s*(rtg_\w+)\s*\(", src, flags=re.M)))


def test_library_exports_every_declared_symbol():
    from rtg import _lib
    lib = _lib.lib()
    syms = _declared_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
    assert lib.rtg_abi_version() == _lib.ABI_VERSION


def test_topology_validation_before_device_work():
    from rtg import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    fp = ctypes.POINTER(ctypes.c_float)
    ip = ctypes.POINTER(ctypes.c_int32)
    lt = np.zeros((3, 3), np.float32)
    bad = np.array([-1, 2, 0], np.int32)          # parent after child
    rc = lib.rtg_topology_create(bad.ctypes.data_as(ip), lt.ctypes.data_as(fp), None, 3, ctypes.byref(h))
    assert rc == 1 and b"parents[1]" in lib.rtg_last_error()
    noroot = np.array([0, 0, 1], np.int32)
    assert lib.rtg_topology_create(noroot.ctypes.data_as(ip), lt.ctypes.data_as(fp), None, 3, ctypes.byref(h)) == 1


def test_solver_and_op_validation():
    from rtg import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    fp = ctypes.POINTER(ctypes.c_float)
    zl = np.zeros((21, 3), np.float32)
    assert lib.rtg_solver_create(0, zl.ctypes.data_as(fp), zl.ctypes.data_as(fp), None, 21, 0, ctypes.byref(h)) == 1
    assert b"59-joint" in lib.rtg_last_error()
    assert lib.rtg_solver_create(9, zl.ctypes.data_as(fp), None, None, 21, 0, ctypes.byref(h)) == 1
    assert lib.rtg_quat_in_xyz_axis_f32(None, b"XyZ", 1, None, None) == 1          # mixed case
    assert lib.rtg_quat_in_xyz_axis_f32(None, b"XXZ", 1, None, None) == 1          # repeated axis
    assert lib.rtg_quat_op_f32(99, None, None, None, 1, None, None) == 1
    assert lib.rtg_cal_joint_quat_f32(None, None, 9, 1, None, None) == 4
    assert lib.rtg_retarget_f32(None, None, None, None, None, 1, 0, None, None, None, None) == 1
    assert lib.rtg_frame_server_launch(None, None, None, None, None, None, 200, None) == 1
    assert b"NULL solver" in lib.rtg_last_error()


def test_dof_model_validation():
    from rtg import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    ax = np.zeros(4, np.int32)
    ip = ctypes.POINTER(ctypes.c_int32)
    assert lib.rtg_dof_model_create(None, ax.ctypes.data_as(ip), None, None, ctypes.byref(h)) == 1
    assert b"NULL topology" in lib.rtg_last_error()
    assert lib.rtg_dof_fk_f32(None, None, None, None, 1, 0, None, None, None) == 1


def test_empty_batches_are_noops():
    from rtg import _lib
    lib = _lib.lib()
    assert lib.rtg_quat_op_f32(0, None, None, None, 0, None, None) == 0
    assert lib.rtg_cal_joint_quat_f32(None, None, 3, 0, None, None) == 0


def test_dropin_modules_import_without_gpu():
    import poselib.poselib.core.rotation3d  # noqa: F401
    import poselib.poselib.skeleton.skeleton3d  # noqa: F401
    import retarget.retarget_solver  # noqa: F401
    import retarget.spatial_transform.transform3d  # noqa: F401
    import robot_kinematics_model  # noqa: F401
    from retarget.retarget_solver import VtrdynFullBodyPosRetargeter  # noqa: F401
    from robot_kinematics_model.hu_forward_model import HuForwardModel  # noqa: F401
    from retarget.main import Retarget, RetargetHuV5fromMocap  # noqa: F401


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="checks the no-GPU behaviour")
def test_compute_without_gpu_fails_loudly():
    import torch
    from poselib.poselib.core.rotation3d import quat_mul
    with pytest.raises(RuntimeError, match="no HIP device"):
        quat_mul(torch.zeros(1, 4), torch.zeros(1, 4))


def test_safe_pickle_reader_roundtrip(tmp_path):
    """rtg.safe_pickle decodes a SkeletonState pickle (our own file) without unpickling."""
    import pickle
    import torch
    from poselib.poselib.skeleton.skeleton3d import SkeletonState, SkeletonTree
    from rtg.safe_pickle import load_skeleton_state_arrays
    from rtg import assets
    tree = SkeletonTree([str(s) for s in assets.load("vtrdyn")["node_names"]], torch.from_numpy(assets.parents("vtrdyn")),
                        torch.from_numpy(assets.local_translation("vtrdyn")))
    st = SkeletonState(torch.from_numpy(assets.load("vtrdyn")["tensor"]), tree, True)
    st.__class__.__module__ = "poselib.poselib.skeleton.skeleton3d"
    p = tmp_path / "state.pkl"
    with open(p, "wb") as f:
        pickle.dump(st, f, protocol=4)
    d = load_skeleton_state_arrays(str(p))
    np.testing.assert_array_equal(d["local_translation"], assets.local_translation("vtrdyn"))
    np.testing.assert_array_equal(d["parent_indices"], assets.parents("vtrdyn"))
    assert d["node_names"] == [str(s) for s in assets.load("vtrdyn")["node_names"]]


def test_synthetic_generator_deterministic():
    from rtg import synth
    a = synth.synth_full_body_inputs(8, 5)
    b = synth.synth_full_body_inputs(8, 5)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert a[0].shape == (8, 21, 3) and a[1].shape == (8, 20, 3) and a[0].dtype == np.float32


def _fake_solver(kind):
    """A Solver shell (no device handle) to exercise the host-side argument checks without a GPU."""
    import torch
    from rtg.runtime import Solver
    s = Solver.__new__(Solver)
    s._h, s.kind, s.precise_gripper, s.device = None, kind, True, torch.device("cuda", 0)
    return s


def test_solver_rejects_bad_input_shapes():
    """trailing shapes are checked against the kind's rows before anything reaches the C ABI (which
    cannot see shapes): a raw (B,23,3) broadcast body, short hands, mismatched batches, a bad layout."""
    import torch
    from rtg import _lib
    s = _fake_solver(_lib.SOLVER_FULL_BODY_POS)
    B = 4
    good = [torch.zeros(B, 21, 3), torch.zeros(B, 20, 3), torch.zeros(B, 20, 3)]
    cases = [
        [torch.zeros(B, 23, 3), good[1], good[2]],           # raw 23-joint broadcast body
        [good[0], torch.zeros(B, 19, 3), good[2]],            # short hand
        [good[0], good[1], torch.zeros(B + 1, 20, 3)],        # batch mismatch
        [good[0], good[1]],                                   # missing input
    ]
    for ins in cases:
        with pytest.raises(ValueError):
            s.retarget(ins)
    with pytest.raises(ValueError):
        s.retarget(good, layout="planar")
    with pytest.raises(ValueError):   # AoS tensors handed over as SoA
        s.retarget(good, layout="soa")
    with pytest.raises(ValueError):   # CPU tensors of the right shape: not device tensors
        s.retarget(good)
    r = _fake_solver(_lib.SOLVER_FULL_BODY_ROT)
    with pytest.raises(ValueError):   # rotations need 4 components
        r.retarget([torch.zeros(B, 21, 3), torch.zeros(B, 21, 3), torch.zeros(B, 20, 3), torch.zeros(B, 20, 3)])


def test_build_info_reports_every_knob_and_no_wrong_answer_build():
    """rtg_build_info(): every RTG_* knob the sources define is reported, and the product library carries none of
    the measurement-only knobs that change results (rtg._lib.lib() refuses such a build)."""
    import json
    import glob
    from rtg import _lib
    info = _lib.build_info()
    assert info["wrong_answer_knobs"] == 0 and info["abi"] == _lib.ABI_VERSION
    src = "".join(open(p).read() for ext in ("*.hip", "*.cuh", "*.h", "*.cpp")
                  for p in glob.glob(os.path.join(REPO, "humanoid-real-time-retarget_amd", "csrc", ext)))
    defined = set(re.findall(r"#ifndef (RTG_[A-Z0-9_]+)", src)) - {"RTG_H"}
    assert defined <= set(info["knobs"]), defined - set(info["knobs"])
    for k in _lib.WRONG_ANSWER_KNOBS:
        assert info["knobs"][k] == 0
    json.dumps(info)


def _overlay():
    import json
    return json.load(open(os.path.join(REPO, "tests", "golden", "overlay_names.json")))


def _star(modname):
    import importlib
    m = importlib.import_module(modname)
    names = getattr(m, "__all__", None)
    return set(names) if names is not None else {n for n in vars(m) if not n.startswith("_")}


def test_overlay_exports_every_name_the_reference_uses():
    """tools/overlay_names.py scanned every reference module the drop-in does NOT replace (retarget/utils, the
    sim_*_teleop entry points, the viewers, the asset generators) for the names they take from replaced modules
    -- explicit imports, star imports (then every free name used) and Cls.attr on imported classes.  The drop-ins
    export every one, and each star-imported drop-in module star-exports at least the reference module's set."""
    import importlib
    d = _overlay()
    assert len(d["names"]) >= 40 and "retarget.spatial_transform.transform3d" in d["star_exports"]
    for e in d["names"]:
        m = importlib.import_module(e["module"])
        assert hasattr(m, e["name"]), (e["module"], e["name"], e["used_by"])
    for mod, names in d["star_exports"].items():
        missing = set(names) - _star(mod)
        assert not missing, (mod, sorted(missing))
    for e in d["class_attributes"]:
        if "out_of_scope" in e:
            continue
        cls_name, attr = e["attr"].split(".", 1)
        cls = getattr(importlib.import_module(e["module"]), cls_name)
        assert hasattr(cls, attr), (e["module"], e["attr"], e["used_by"])
    # the verdict's list, by name (transform3d.py:9,147,153; rotation3d.py:101,243,629-661)
    t3 = importlib.import_module("retarget.spatial_transform.transform3d")
    r3 = importlib.import_module("poselib.poselib.core.rotation3d")
    for n in ("quat_between_two_vecs", "exp_map_to_quat", "quat_slerp"):
        assert callable(getattr(t3, n))
    for n in ("exp_map_to_angle_axis", "exp_map_to_quat", "quat_from_xyz", "quat_yaw_rotation", "quat_to_eular"):
        assert callable(getattr(r3, n))


def test_from_urdf_delegates_to_the_reference_parser(tmp_path):
    """RobotZeroPose.from_urdf (base_robot.py:71-81) calls retarget.utils.parse_urdf.parse_urdf from the reference
    checkout the drop-in overlays -- found through the drop-in packages' extended __path__ when that checkout comes
    later on sys.path -- and raises ImportError naming the parser only when it cannot be imported."""
    import subprocess
    import sys
    ref = tmp_path / "checkout"
    (ref / "retarget" / "utils").mkdir(parents=True)
    (ref / "retarget" / "utils" / "__init__.py").write_text("")
    (ref / "retarget" / "utils" / "parse_urdf.py").write_text(
        "import torch\n"
        "from types import SimpleNamespace as NS\n"
        "CALLS = []\n"
        "def parse_urdf(urdf_path):\n"
        "    CALLS.append(urdf_path)\n"
        "    tree = NS(parent_indices=torch.tensor([-1, 0]), num_joints=2, node_names=['base', 'link'])\n"
        "    zp = NS(local_translation=torch.tensor([[0., 0, 0], [0, 0, 1]]),\n"
        "            global_translation=torch.tensor([[0., 0, 0], [0, 0, 1]]), skeleton_tree=tree)\n"
        "    return zp, ['base.stl', 'link.stl']\n")
    code = ("import sys\n"
            "from robot_kinematics_model.base_robot import RobotZeroPose\n"
            "z = RobotZeroPose.from_urdf('asset/hu/hu_v5.urdf')\n"
            "import retarget.utils.parse_urdf as P\n"
            "mod = sys.modules['retarget.utils.parse_urdf']\n"
            "assert mod.CALLS == ['asset/hu/hu_v5.urdf'], mod.CALLS\n"
            "assert z.num_joints == 2 and z.node_names == ['base', 'link'] and z.num_dofs == 1\n"
            "assert z.global_translation[1, 2].item() == 1.0\n"
            "print('ok')\n")
    pkg = os.path.join(REPO, "humanoid-real-time-retarget_amd")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([pkg, str(ref)]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]
    # without a checkout: ImportError that names the parser
    env = dict(os.environ, PYTHONPATH=pkg)
    r = subprocess.run([sys.executable, "-c", "from robot_kinematics_model.base_robot import RobotZeroPose\n"
                        "RobotZeroPose.from_urdf('x.urdf')"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ImportError" in r.stderr and "parse_urdf" in r.stderr


def test_serializable_json_and_npy_roundtrip(tmp_path):
    """Serializable.to_file / from_file (poselib core/backend/abstract.py:94-128) for SkeletonTree / SkeletonState /
    SkeletonMotion; the .npy path is read by the non-executing pickle walker, not np.load(allow_pickle=True)."""
    import torch
    from poselib.poselib.skeleton.skeleton3d import SkeletonMotion, SkeletonState, SkeletonTree
    tree = SkeletonTree(["a", "b", "c"], torch.tensor([-1, 0, 1]), torch.arange(9, dtype=torch.float32).reshape(3, 3))
    rot = torch.rand(4, 3, 4)
    st = SkeletonState(SkeletonState._to_state_vector(rot, torch.rand(4, 3)), tree, True)
    mo = SkeletonMotion(SkeletonMotion._to_state_vector(rot, torch.rand(4, 3), torch.rand(4, 3, 3), torch.rand(4, 3, 3)),
                        tree, True, 30)
    for obj in (tree, st, mo):
        for ext in ("json", "npy"):
            p = str(tmp_path / f"{type(obj).__name__}.{ext}")
            obj.to_file(p)
            back = type(obj).from_file(p)
            if isinstance(obj, SkeletonTree):
                assert back.node_names == tree.node_names and torch.equal(back.parent_indices, tree.parent_indices)
                assert torch.equal(back.local_translation, tree.local_translation)
            else:
                assert torch.equal(back.tensor, obj.tensor) and back.is_local == obj.is_local
            if isinstance(obj, SkeletonMotion):
                assert back.fps == 30 and torch.equal(back.global_angular_velocity, obj.global_angular_velocity)
    with pytest.raises(AssertionError):
        SkeletonState.from_file(str(tmp_path / "SkeletonTree.json"))


def test_frame_server_post_protocol_on_the_host():
    """rtg_frame_server_post (the teleop per-frame round trip in one C call) against a host thread standing in for
    k_frame_server: the frame's rows land in the inbox `in` before its sequence word (in[RTG_SERVER_SEQ_WORD]) = seq,
    the outputs are copied out only after ctl[1] = seq, a server that ended before taking the frame reports
    RTG_SERVER_ENDED, a silent one times out; rtg_frame_server_signal stores the word alone."""
    import threading
    import time
    from rtg import _lib
    lib = _lib.lib()
    vp = ctypes.c_void_p
    ctl = np.zeros(4, np.uint32)
    inb = np.zeros(_lib.SERVER_INBOX_FLOATS, np.float32)
    word = inb[_lib.SERVER_SEQ_WORD:_lib.SERVER_SEQ_WORD + 1].view(np.uint32)
    out = np.zeros(390, np.float32)   # local_rot 124 | dof 30 | body_rot 236, as FrameServer lays out its pinned buffer
    rng = np.random.default_rng(5)
    body, lh, rh = (rng.normal(size=s).astype(np.float32) for s in ((21, 3), (20, 3), (20, 3)))
    seen = {}

    def device(seq):
        while word[0] != seq:
            time.sleep(0)
        seen["in"] = inb[:183].copy()
        out[:] = np.arange(390, dtype=np.float32) + seq
        ctl[1] = seq

    def post(seq, timeout_us=2_000_000):
        dof, lr, br = np.empty(30, np.float32), np.empty((31, 4), np.float32), np.empty((59, 4), np.float32)
        a = lambda x: vp(x.ctypes.data)
        rc = lib.rtg_frame_server_post(a(ctl), seq, a(inb), a(body), a(lh), a(rh), vp(out.ctypes.data + 4 * 124),
                                       a(out), vp(out.ctypes.data + 4 * 154), a(dof), a(lr), a(br), timeout_us)
        return rc, dof, lr, br

    th = threading.Thread(target=device, args=(7,))
    th.start()
    rc, dof, lr, br = post(7)
    th.join()
    assert rc == 0
    np.testing.assert_array_equal(seen["in"], np.concatenate([body.ravel(), lh.ravel(), rh.ravel()]))
    np.testing.assert_array_equal(lr.ravel(), np.arange(124, dtype=np.float32) + 7)
    np.testing.assert_array_equal(dof, np.arange(124, 154, dtype=np.float32) + 7)
    np.testing.assert_array_equal(br.ravel(), np.arange(154, 390, dtype=np.float32) + 7)
    ctl[2] = 1                                       # the server has ended (idle) and never takes frame 8
    assert post(8)[0] == _lib.SERVER_ENDED
    ctl[2] = 0
    t0 = time.perf_counter()
    assert post(9, timeout_us=20_000)[0] == _lib.ERR_TIMEOUT
    assert time.perf_counter() - t0 < 5.0
    assert b"not served" in lib.rtg_last_error()
    assert lib.rtg_frame_server_signal(vp(inb.ctypes.data), _lib.SERVER_QUIT) == 0 and word[0] == _lib.SERVER_QUIT
    assert lib.rtg_frame_server_signal(None, 1) == 1
    assert lib.rtg_frame_server_post(None, 1, *([None] * 10), 10) == 1
    assert lib.rtg_frame_server_post(vp(ctl.ctypes.data), _lib.SERVER_QUIT, *([vp(inb.ctypes.data)] * 5),
                                     *([None] * 5), 10) == 1


def test_frame_post_extension_refuses_what_it_cannot_post():
    """rtg/_frame_post (the server's per-frame round trip with tensor arguments) checks its inputs before it posts:
    a non-float32, non-contiguous or wrongly sized frame returns NOT_HOST_F32 without calling the C function (the
    null function address here would crash if it were called), so FrameServer converts and takes the ctypes path."""
    import torch
    fp = pytest.importorskip("rtg._frame_post")
    good = (torch.zeros(21, 3), torch.zeros(20, 3), torch.zeros(20, 3))
    bad = [(good[0].double(), good[1], good[2]), (good[0], torch.zeros(3, 20).t(), good[2]),
           (good[0], good[1], torch.zeros(21, 3))]
    for b, l, r in bad:
        rc, code, *_ = fp.post(0, 0, 1, 0, b, l, r, 0, 0, 0, 1000)
        assert rc == fp.NOT_HOST_F32 and code == 0
    assert fp.SERVER_ENDED == 6


def test_group_scheduler_invariants(tmp_path):
    """The lane-group list scheduler (csrc/rtg_group_sched.h, plain C++) through its stand-alone check
    (tests/group_sched_check.cpp): every included joint exactly once, parents strictly earlier, complete ascending
    child links, on chains, stars, random trees and masks -- and the 31-joint Hu tree on 4 lanes takes the 10 steps
    DESIGN.md quotes."""
    import subprocess
    from rtg import assets
    exe = str(tmp_path / "group_sched_check")
    src = os.path.join(REPO, "tests", "group_sched_check.cpp")
    inc = os.path.join(REPO, "humanoid-real-time-retarget_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", inc, src, "-o", exe], check=True, timeout=120)
    hu = [str(int(p)) for p in assets.parents("hu_v5")]
    assert len(hu) == 31
    r = subprocess.run([exe, "10"] + hu, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-2000:]

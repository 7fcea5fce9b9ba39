"""The joint-angle motion sampler's host side (no GPU): properties of its composition oracle
(tests/dof_motion_ref.py), the argument checks of rtg_dof_motion_sample_f32 that need no device -- their expectations
are written here, not in tests/golden/api_messages.json -- and rtg.motion.DofMotionLibrary's clip validation.  The
rejections that need a live model (clip flag without limits, a key link at or past the model's J, more than 64
joints, overlaps) are in tests/test_gpu_dof_motion.py."""
import ctypes
import types

import numpy as np
import pytest

import dof_motion_ref as ref
from dof_motion_ref import bits


def hu_model():
    from rtg import assets
    return ref.make_model(assets.parents("hu_v5"), assets.local_translation("hu_v5"))


# ------------------------------------------------------------------------------------------- reference properties
def test_reference_at_stored_frames_and_past_the_end():
    """At the exact stored frames of a finite library with no -0 rows dof equals the stored row and dof_vel equals
    (next - this) / dt; at and past the last frame both velocities are +0."""
    m = hu_model()
    lib = ref.make_library(30, "smooth")
    assert np.isfinite(lib["dof"]).all() and not np.signbit(lib["dof"][lib["dof"] == 0]).any()
    covered = 0
    for c, (L, fps) in enumerate(zip(lib["len"], lib["fps"])):
        L, s = int(L), int(lib["start"][c])
        k = np.arange(L)
        t = (k / float(fps)).astype(np.float32)
        k = k[t.astype(np.float64) * float(fps) == k]    # the frames whose instant is a float32 (all of them at 32 and 1 fps)
        assert k[0] == 0 and (len(k) == L or fps not in (32.0, 1.0))
        covered += len(k)
        t = t[k]
        out = ref.sample(lib, np.full(len(k), c, np.int32), t, normalize=True, model=m, key_links=[0, 5])
        assert (out["row0"] == s + k).all() and (out["b"] == 0).all()
        np.testing.assert_array_equal(bits(out["dof"]), bits(lib["dof"][s + k]))
        np.testing.assert_array_equal(bits(out["root_t"]), bits(lib["root_t"][s + k]))
        dt = ref.frame_time(fps)
        nxt = np.minimum(k + 1, L - 1)
        want = ref.diff_over_dt(lib["dof"][s + nxt], lib["dof"][s + k], np.full(len(k), dt, np.float32))
        np.testing.assert_array_equal(bits(out["dof_vel"]), bits(want))
        assert (out["dof_vel"][k < L - 1] != 0).any() or L == 1
        np.testing.assert_array_equal(bits(out["key_pos"]), bits(out["g_pos"][:, [0, 5]]))
        # at and past the last frame: i0 == i1, both velocities +0 (the sign included)
        late = np.array([(L - 1) / float(fps), L / float(fps), (L + 100.5) / float(fps), 3e38, np.inf], np.float32)
        out = ref.sample(lib, np.full(len(late), c, np.int32), late, model=m, want_global=False)
        assert (out["row0"] == out["row1"]).all() and (out["row0"] == s + L - 1).all()
        assert (bits(out["dof_vel"]) == 0).all() and (bits(out["root_vel"]) == 0).all()
    assert covered >= 3 + 17 + 3


def test_reference_invalid_clip_ids_are_nan_and_read_nothing():
    m = hu_model()
    lib = ref.make_library(30, "smooth")
    clip = np.array([-1, 5, 0, 4, -2**31, 2**31 - 1, 6, 2], np.int32)
    time = np.array([0.0, 0.1, 0.01, 1.0, 0.5, 0.5, np.nan, 0.03], np.float32)
    out = ref.sample(lib, clip, time, normalize=True, model=m, key_links=[3])
    bad = ~((clip >= 0) & (clip < 5))
    assert (out["valid"] == ~bad).all() and bad.sum() == 5
    assert (out["row0"][bad] == 0).all() and (out["row1"][bad] == 0).all()
    for k in ref.KEYS:
        assert (bits(out[k][bad]) == ref.bits(np.float32(np.nan))).all(), k
        assert not np.isnan(out[k][~bad]).any(), k
    # the rows do not matter to an invalid query: a library of NaN rows gives the same invalid rows and never raises
    poisoned = dict(lib, dof=np.full_like(lib["dof"], np.nan))
    out2 = ref.sample(poisoned, clip[bad], time[bad], model=m, key_links=[3])
    for k in ref.KEYS:
        np.testing.assert_array_equal(bits(out2[k]), bits(out[k][bad]))


# ------------------------------------------------------------------------------------------- the entry's checks
def _lib():
    from rtg import _lib as L
    return L, L.lib()


def test_dof_motion_sample_rejections_need_no_device():
    L, lib = _lib()
    assert lib.rtg_abi_version() == 7
    assert hasattr(lib, "rtg_dof_motion_sample_f32") and "rtg_dof_motion_sample_f32" in L.SIGNATURES
    assert (L.DOF_MOTION_NORMALIZE, L.DOF_MOTION_CLIP, L.DOF_MOTION_MAX_KEY_LINKS) == (1, 2, 32)
    P, Q16 = 0x10000, 0x10008   # fake device addresses: every check below comes before any use
    fn = lib.rtg_dof_motion_sample_f32

    def call(dof=P, rr=P + 0x1000, rt=P + 0x2000, clip=P + 0x3000, time=P + 0x4000, N=4, flags=0, keys=None,
             K=None, do=P + 0x5000, dv=None, rro=P + 0x6000, rto=P + 0x7000, rv=None, gr=None, gp=None, kp=None):
        p = lambda x: None if x is None else ctypes.c_void_p(x)   # noqa: E731
        ka = None if keys is None else np.asarray(keys, np.int32)
        kptr = None if ka is None else ka.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        rc = fn(None, None, p(dof), p(rr), p(rt), p(clip), p(time), N, flags, kptr,
                (0 if ka is None else len(ka)) if K is None else K, p(do), p(dv), p(rro), p(rto), p(rv), p(gr), p(gp),
                p(kp), None)
        return rc, lib.rtg_last_error().decode()

    KP = P + 0xA000
    for kw, word in ((dict(N=-1), "N=-1"),
                     (dict(K=-1), "K=-1"), (dict(K=33, keys=[0] * 33, kp=KP), "K=33"),
                     (dict(flags=4), "unknown flags 0x4"), (dict(flags=64), "unknown flags"),
                     (dict(flags=L.MOTION_GLOBAL | L.MOTION_STATE), "unknown flags"),
                     (dict(keys=[0, -1], kp=KP), "key_links[1]=-1"), (dict(keys=[64], kp=KP), "key_links[0]=64"),
                     (dict(keys=[3, 2**31 - 1], kp=KP), "key_links[1]"),
                     (dict(K=2, kp=KP), "key_links NULL"),
                     (dict(keys=[1, 2]), "key_pos"), (dict(kp=KP), "key_pos"),
                     (dict(dv=P + 0x8000), "dof_vel_out"),
                     (dict(gr=P + 0x8000), "g_rot"), (dict(gp=P + 0x8000), "g_rot"),
                     (dict(rr=None), "NULL buffer"), (dict(rt=None), "NULL buffer"), (dict(clip=None), "NULL buffer"),
                     (dict(time=None), "NULL buffer"), (dict(rro=None), "NULL buffer"), (dict(rto=None), "NULL buffer"),
                     (dict(rr=Q16), "aligned"), (dict(rro=Q16), "aligned"),
                     (dict(gr=Q16, gp=P + 0x9000), "aligned"),
                     (dict(), "NULL model"),
                     (dict(N=0), "NULL model"),
                     (dict(dv=P + 0x8000, rv=P + 0x9000, gr=P + 0xB000, gp=P + 0xC000, keys=[0, 0, 63], kp=KP,
                           flags=3), "NULL model")):
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("rtg_dof_motion_sample_f32: ") and word in msg, (kw, rc, msg)
    # the existing entry's flag set did not move: the new enum is its own
    rc = lib.rtg_motion_sample_f32(None, None, *([ctypes.c_void_p(P)] * 3), 0, ctypes.c_void_p(P), ctypes.c_void_p(P), 4, 8,
                                   *([ctypes.c_void_p(P)] * 5), None)
    assert rc == 1 and "rtg_motion_sample_f32: unknown flags 0x8" in lib.rtg_last_error().decode()


# ------------------------------------------------------------------------------------------- the Python class
def test_dof_motion_library_imports_and_validates_without_a_gpu():
    import torch
    import rtg.motion as M
    from rtg import ops
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    assert hasattr(ops, "dof_motion_sample") and hasattr(HuForwardModel, "motion_library")
    assert {"dof_pos", "dof_vel", "root_translation", "root_rotation", "root_velocity", "root_angular_velocity",
            "global_rotation", "global_translation", "key_translation"} == set(M.DofMotionSample.__dataclass_fields__)
    model = types.SimpleNamespace(num_dofs=3, has_limits=False)

    def clip(L=4, nd=3, fps=30.0, Lt=None, Lr=None, fit_shaped=True):
        a, r = torch.zeros(L, nd), torch.zeros(Lr or L, 4)
        return (a[..., None] if fit_shaped else a, torch.zeros(Lt or L, 3), r[:, None] if fit_shaped else r, fps)

    with pytest.raises(ValueError, match="no clips"):
        M.DofMotionLibrary(model, [])
    with pytest.raises(ValueError, match=r"must be \(L, 3"):
        M.DofMotionLibrary(model, [clip(), clip(nd=2)])                       # wrong angle width
    with pytest.raises(ValueError, match="clip 0 must be"):
        M.DofMotionLibrary(model, [(torch.zeros(4, 3), torch.zeros(4, 2), torch.zeros(4, 4), 30.0)])
    with pytest.raises(ValueError, match="clip 0 must be"):
        M.DofMotionLibrary(model, [(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), 30.0)])
    with pytest.raises(ValueError, match="clip 1 must have one length"):
        M.DofMotionLibrary(model, [clip(), clip(Lt=5)])
    with pytest.raises(ValueError, match="clip 0 must have one length"):
        M.DofMotionLibrary(model, [clip(Lr=3, fit_shaped=False)])
    for bad in (0.0, -30.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="fps"):
            M.DofMotionLibrary(model, [clip(fps=bad)])
    with pytest.raises(ValueError, match="not \\(angles"):
        M.DofMotionLibrary(model, [clip()[:3]])
    with pytest.raises(ValueError, match="1..64"):
        M.DofMotionLibrary(types.SimpleNamespace(num_dofs=64), [clip(nd=64)])
    with pytest.raises(ValueError, match="HuForwardModel"):
        M.DofMotionLibrary(object(), [clip()])
    # valid clips in both accepted forms pass every host check: what is left is the device
    from rtg._lib import RtgError
    import torch.cuda
    if not torch.cuda.is_available():
        with pytest.raises(RtgError):
            M.DofMotionLibrary(model, [clip(), clip(L=1, fit_shaped=False)])
        with pytest.raises(RtgError):
            M.DofMotionLibrary(model, clip())                                  # one clip, not a list

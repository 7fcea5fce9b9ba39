"""CPU-only checks of the fused keypoint fit (rtg_dof_fit_f32): the symbol is there, every argument check that needs
no handle answers RTG_ERR_INVALID_ARGUMENT with its own message before any device work (the handle is NULL and every
address a dummy in all of these calls), and the Python entry points raise RtgError without a GPU -- there is no CPU
fallback."""
import ctypes

import numpy as np
import pytest
import torch

INVALID = 1   # RTG_ERR_INVALID_ARGUMENT


def _call(lib, **kw):
    """rtg_dof_fit_f32 with a NULL model and never-dereferenced dummy addresses, fields overridden by name."""
    x = ctypes.c_void_p(64)
    a = dict(model=None, target_pos=x, weight=x, root_rot=x, root_t=x, dof_in=x, B=1, clip=0, iters=1, lr=0.02,
             beta1=0.9, beta2=0.999, eps=1e-8, step0=0, m=x, v=x, dof_out=x, loss=x, grad=x, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return lib.rtg_dof_fit_f32(*a.values())


def test_symbol_and_abi_version():
    from rtg import _lib
    lib = _lib.lib()
    assert hasattr(lib, "rtg_dof_fit_f32")
    assert lib.rtg_abi_version() == 7   # a new symbol only: nothing that existed changed


@pytest.mark.parametrize("kw, msg", [
    (dict(), b"NULL model"),
    (dict(B=0), b"NULL model"),
    (dict(B=-1), b"< 0"),
    (dict(target_pos=None), b"NULL buffer"),
    (dict(root_rot=None), b"NULL buffer"),
    (dict(root_t=None), b"NULL buffer"),
    (dict(m=None), b"both Adam moment buffers"),
    (dict(v=None), b"both Adam moment buffers"),
    (dict(iters=-1), b"iters=-1"),
    (dict(iters=4097), b"iters=4097"),
    (dict(step0=-1), b"step0=-1"),
    (dict(lr=float("nan")), b"must be finite"),
    (dict(lr=float("inf")), b"must be finite"),
    (dict(eps=float("nan")), b"must be finite"),
    (dict(eps=float("-inf")), b"must be finite"),
    (dict(beta1=float("nan")), b"must lie in [0, 1)"),
    (dict(beta1=1.0), b"must lie in [0, 1)"),
    (dict(beta1=-0.1), b"must lie in [0, 1)"),
    (dict(beta2=float("inf")), b"must lie in [0, 1)"),
    (dict(beta2=1.0), b"must lie in [0, 1)"),
    (dict(beta2=-1e-3), b"must lie in [0, 1)"),
    (dict(dof_out=None, loss=None, grad=None), b"every output is NULL"),
])
def test_validation_before_device_work(kw, msg):
    from rtg import _lib
    lib = _lib.lib()
    assert _call(lib, **kw) == INVALID
    assert msg in lib.rtg_last_error(), lib.rtg_last_error()
    assert b"rtg_dof_fit_f32" in lib.rtg_last_error()


def test_valid_hyperparameters_reach_the_handle_check():
    """The edges of the allowed ranges pass the checks before the handle's: the call then stops at the NULL model."""
    from rtg import _lib
    lib = _lib.lib()
    for kw in (dict(iters=0), dict(iters=4096), dict(beta1=0.0, beta2=0.0), dict(m=None, v=None), dict(weight=None),
               dict(dof_out=None, grad=None), dict(step0=2 ** 31 - 1), dict(lr=0.0, eps=0.0)):
        assert _call(lib, **kw) == INVALID and b"NULL model" in lib.rtg_last_error(), kw


class _NoDeviceModel:
    """What ops looks at before it asks for the device."""
    num_dofs = 32
    has_limits = True
    handle = None


def test_python_entry_points_raise_rtg_error_without_a_gpu(monkeypatch):
    from rtg import _lib, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the same test on a machine that has one
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    tp = np.zeros((2, 33, 3), np.float32)
    rr = np.tile(np.array([0, 0, 0, 1], np.float32), (2, 1))
    rt = np.zeros((2, 3), np.float32)
    with pytest.raises(_lib.RtgError):
        ops.dof_fit(_NoDeviceModel(), tp, rr, rt, iters=1)
    with pytest.raises(_lib.RtgError):
        ops.keypoint_loss(_NoDeviceModel(), np.zeros((2, 32), np.float32), tp, rr, rt)
    hu = HuForwardModel.__new__(HuForwardModel)   # its constructor already needs the device
    hu._model, hu.num_joints = _NoDeviceModel(), 33
    with pytest.raises(_lib.RtgError):
        hu.fit_keypoints(torch.from_numpy(tp), torch.from_numpy(rt), torch.from_numpy(rr[:, None]))

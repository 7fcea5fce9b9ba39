"""CPU-only checks of the pose fit with orientation targets (rtg_dof_fit_orient_f32): the symbol is there under ABI 7
with its prototype, every argument check that needs no handle answers with its own message before any device work (the
handle is NULL and every device address a dummy in all of these calls; rot_joint is a host array, as the header says),
the Python entry points raise RtgError without a GPU, and the reference the GPU tests use -- the torch restatement of
tests/test_pose_fit_host.py with the rotation term

    sum_k rot_weight[k] 4 (1 - <G_j(k), R_k / max(|R_k|, 1e-9)>^2)

added to the keypoint loss -- is anchored: its float64 autograd gradient agrees with central differences and with the
closed form -8 rot_weight c R^ the kernel uses, and it gives an oriented wrist's DOF the gradient that positions alone
leave at exactly 0."""
import ctypes

import numpy as np
import pytest
import torch

from test_fk_grad_host import dof_fk
from test_pose_fit_host import B1, B2, EPS, FIT_ROT, FIT_T, LR, _Hu, _t, root_unit

INVALID, UNSUPPORTED = 1, 4   # RTG_ERR_INVALID_ARGUMENT, RTG_ERR_UNSUPPORTED
MAX_LINKS = 8                 # RTG_FIT_MAX_ROT_LINKS
HU_HANDS_FEET_HEAD = (20, 29, 6, 12, 32)   # left / right wrist yaw link, left / right toe link, neck link


# ------------------------------------------------------------------ the reference: restatement + loss + Adam
def ref_orient_terms(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw):
    """-> (position part (B), rotation part (B), c (B,K), g_rot (B,J,4)) of the restatement's loss."""
    q = _t(q, dtype)
    lo, hi = (_t(s.lo, dtype), _t(s.hi, dtype)) if clip else (None, None)
    g_rot, gp = dof_fk(_t(dof, dtype), root_unit(q) if fit_root & FIT_ROT else q, _t(t, dtype), [int(p) for p in s.par],
                       _t(s.lt, dtype), s.axis, lo, hi)
    pos = (_t(w, dtype).reshape(1, -1, 1) * (gp - _t(tgt, dtype)) ** 2).sum(dim=(-1, -2))
    K = len(joints)
    R = _t(R, dtype).reshape(gp.shape[0], K, 4)
    Rh = R / R.norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
    c = (g_rot[:, [int(j) for j in joints]] * Rh).sum(dim=-1)
    rwt = torch.ones(K, dtype=dtype) if rw is None else _t(rw, dtype)
    return pos, (rwt.reshape(1, K) * (4.0 * (1.0 - c * c))).sum(dim=-1), c, g_rot


def ref_orient_loss(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw):
    pos, rot, _, _ = ref_orient_terms(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw)
    return pos + rot


def ref_orient_loss_grad(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw):
    """-> loss (B), grad (B,J-1), grad_root (B,7) = {dL/dt, dL/dq}, numpy."""
    a, qq, tt = (_t(x, dtype).clone().requires_grad_(True) for x in (dof, q, t))
    loss = ref_orient_loss(s, a, qq, tt, tgt, w, clip, dtype, fit_root, joints, R, rw)
    loss.sum().backward()
    g = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    return loss.detach().numpy(), g(a).numpy(), torch.cat([g(tt), g(qq)], dim=-1).numpy()


def ref_orient_fit(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw, iters, lr=LR, lr_t=LR, lr_q=LR):
    """ref_pose_fit's loop on the loss with the rotation term -> (loss, dof, q, t) after ``iters`` steps, numpy."""
    a, qq, tt = (_t(x, dtype).clone().requires_grad_(True) for x in (dof, q, t))
    groups = [dict(params=[a], lr=lr)]
    if fit_root & FIT_T:
        groups.append(dict(params=[tt], lr=lr_t))
    if fit_root & FIT_ROT:
        groups.append(dict(params=[qq], lr=lr_q))
    opt = torch.optim.Adam(groups, betas=(B1, B2), eps=EPS)
    for _ in range(iters):
        opt.zero_grad()
        ref_orient_loss(s, a, qq, tt, tgt, w, clip, dtype, fit_root, joints, R, rw).sum().backward()
        opt.step()
        if fit_root & FIT_ROT:
            with torch.no_grad():
                qq.copy_(root_unit(qq))
    with torch.no_grad():
        loss = ref_orient_loss(s, a, qq, tt, tgt, w, clip, dtype, fit_root, joints, R, rw)
    return tuple(x.detach().numpy().copy() for x in (loss, a, qq, tt))


def orient_error(s, dof, q, t, clip, joints, R):
    """The angle (rad) between each listed link's rotation and its target, (B,K), float64."""
    with torch.no_grad():
        c = ref_orient_terms(s, dof, q, t, np.zeros((len(dof), s.J, 3)), np.zeros(s.J), clip, torch.float64, 0, joints, R,
                             None)[2]
    return 2.0 * np.arccos(np.clip(np.abs(c.numpy()), 0.0, 1.0))


# ------------------------------------------------------------------ the symbol and its argument checks
def _call(lib, **kw):
    """rtg_dof_fit_orient_f32 with a NULL model and never-dereferenced dummy device addresses, fields overridden by
    name; rot_joint: a host array (the call reads it)."""
    x = ctypes.c_void_p(64)
    a = dict(model=None, target_pos=x, weight=x, rot_joint=[0, 5, 2], target_rot=x, rot_weight=x, K=3, root_rot=x, root_t=x,
             dof_in=x, B=1, clip=0, fit_root=3, iters=1, lr=0.02, lr_root_t=0.02, lr_root_rot=0.02, beta1=0.9,
             beta2=0.999, eps=1e-8, step0=0, m=x, v=x, root_state=x, dof_out=x, root_rot_out=x, root_t_out=x, loss=x,
             grad=x, grad_root=x, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    if a["rot_joint"] is not None:
        a["rot_joint"] = (ctypes.c_int32 * max(len(a["rot_joint"]), 1))(*a["rot_joint"])
    return lib.rtg_dof_fit_orient_f32(*a.values())


def test_symbol_prototype_and_abi_version():
    from rtg import _lib
    lib = _lib.lib()
    fn = lib.rtg_dof_fit_orient_f32
    assert lib.rtg_abi_version() == 7   # a new symbol only: nothing that existed changed
    root = lib.rtg_dof_fit_root_f32.argtypes
    assert fn.restype is ctypes.c_int
    # rtg_dof_fit_root_f32's arguments with (rot_joint, target_rot, rot_weight, K) after weight
    assert list(fn.argtypes) == list(root[:3]) + [ctypes.c_void_p] * 3 + [ctypes.c_int32] + list(root[3:])


_NO_OUT = dict(dof_out=None, root_rot_out=None, root_t_out=None, loss=None, grad=None, grad_root=None)


@pytest.mark.parametrize("kw, code, msg", [
    # rtg_dof_fit_root_f32's
    (dict(), INVALID, b"NULL model"),
    (dict(B=0), INVALID, b"NULL model"),
    (dict(B=-1), INVALID, b"< 0"),
    (dict(target_pos=None), INVALID, b"NULL buffer"),
    (dict(root_rot=None), INVALID, b"NULL buffer"),
    (dict(root_t=None), INVALID, b"NULL buffer"),
    (dict(m=None), INVALID, b"both Adam moment buffers"),
    (dict(v=None), INVALID, b"both Adam moment buffers"),
    (dict(root_state=None), INVALID, b"root_state"),
    (dict(m=None, v=None), INVALID, b"root_state"),
    (dict(fit_root=4), INVALID, b"fit_root=4"),
    (dict(fit_root=-1), INVALID, b"fit_root=-1"),
    (dict(iters=-1), INVALID, b"iters=-1"),
    (dict(iters=4097), INVALID, b"iters=4097"),
    (dict(step0=-1), INVALID, b"step0=-1"),
    (dict(lr=float("nan")), INVALID, b"must be finite"),
    (dict(eps=float("-inf")), INVALID, b"must be finite"),
    (dict(lr_root_t=-1e-3), INVALID, b"finite and not negative"),
    (dict(lr_root_rot=float("nan")), INVALID, b"finite and not negative"),
    (dict(beta1=1.0), INVALID, b"must lie in [0, 1)"),
    (dict(beta2=-1e-3), INVALID, b"must lie in [0, 1)"),
    (_NO_OUT, INVALID, b"every output is NULL"),
    # the orientation block's
    (dict(K=-1), INVALID, b"K=-1"),
    (dict(K=MAX_LINKS + 1, rot_joint=list(range(MAX_LINKS + 1))), UNSUPPORTED, b"at most 8"),
    (dict(K=2 ** 31 - 1), UNSUPPORTED, b"at most 8"),
    (dict(rot_joint=None), INVALID, b"rot_joint or target_rot NULL"),
    (dict(target_rot=None), INVALID, b"rot_joint or target_rot NULL"),
    (dict(target_rot=ctypes.c_void_p(68)), INVALID, b"16-byte aligned"),
    (dict(rot_joint=[0, -1, 2]), INVALID, b"rot_joint[1]=-1"),
    (dict(rot_joint=[4, 5, 4]), INVALID, b"listed twice"),
    (dict(K=2, rot_joint=[0, 0]), INVALID, b"listed twice"),
])
def test_validation_before_device_work(kw, code, msg):
    from rtg import _lib
    lib = _lib.lib()
    assert _call(lib, **kw) == code
    assert msg in lib.rtg_last_error(), lib.rtg_last_error()
    assert b"rtg_dof_fit_orient_f32" in lib.rtg_last_error()


def test_valid_arguments_reach_the_handle_check():
    """The edges of the allowed ranges pass the checks before the handle's: the call then stops at the NULL model.
    With K == 0 the three pointers are not looked at."""
    from rtg import _lib
    lib = _lib.lib()
    for kw in (dict(K=0, rot_joint=None, target_rot=None, rot_weight=None), dict(K=0, target_rot=ctypes.c_void_p(68)),
               dict(K=1), dict(K=MAX_LINKS, rot_joint=list(range(MAX_LINKS))), dict(rot_weight=None),
               dict(rot_joint=[63, 0, 1]), dict(fit_root=0), dict(iters=0), dict(m=None, v=None, root_state=None),
               dict(B=0, target_rot=None), dict(dict(_NO_OUT, loss=ctypes.c_void_p(64)))):
        assert _call(lib, **kw) == INVALID and b"NULL model" in lib.rtg_last_error(), (kw, lib.rtg_last_error())


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
    dof = np.zeros((2, 32), np.float32)
    o = dict(rot_joints=[20, 32], target_rot=np.tile(rr[:, None], (1, 2, 1)), rot_weight=[1.0, 0.5])
    with pytest.raises(_lib.RtgError):
        ops.pose_fit(_NoDeviceModel(), tp, rr, rt, iters=1, **o)
    with pytest.raises(_lib.RtgError):
        ops.pose_loss(_NoDeviceModel(), dof, rr, rt, tp, **o)
    with pytest.raises(_lib.RtgError):
        ops.dof_fit(_NoDeviceModel(), tp, rr, rt, iters=1, **o)
    with pytest.raises(_lib.RtgError):
        ops.keypoint_loss(_NoDeviceModel(), dof, tp, rr, rt, **o)
    hu = HuForwardModel.__new__(HuForwardModel)   # its constructor already needs the device
    hu._model, hu.num_joints, hu.node_names = _NoDeviceModel(), 33, [f"n{j}" for j in range(33)]
    h = dict(target_rotations=torch.from_numpy(o["target_rot"]), rotation_links=["n20", 32])
    with pytest.raises(_lib.RtgError):
        hu.fit_pose(torch.from_numpy(tp), torch.from_numpy(rt), torch.from_numpy(rr[:, None]), **h)
    with pytest.raises(_lib.RtgError):
        hu.fit_keypoints(torch.from_numpy(tp), torch.from_numpy(rt), torch.from_numpy(rr[:, None]), **h)
    with pytest.raises(ValueError, match="no node named"):   # names are resolved before anything else
        hu.fit_pose(torch.from_numpy(tp), torch.from_numpy(rt), torch.from_numpy(rr[:, None]),
                    target_rotations=h["target_rotations"], rotation_links=["n20", "left_hand"])


# ------------------------------------------------------------------ the reference itself
def _case(B=3, seed=11):
    s = _Hu()
    rng = np.random.default_rng(seed)
    quat = lambda *n: (lambda q: q / np.linalg.norm(q, axis=-1, keepdims=True))(rng.normal(size=n + (4,)))
    joints = [0, 6, 19, 20, 32]   # the root, a toe, a wrist pitch link and its child the wrist yaw link, the neck
    x = dict(dof=rng.uniform(s.lo, s.hi, (B, s.J - 1)), q=quat(B) * rng.uniform(0.5, 2.0, (B, 1)),
             t=rng.normal(0, 0.3, (B, 3)), tgt=rng.normal(0, 0.5, (B, s.J, 3)),
             R=quat(B, len(joints)) * rng.uniform(0.5, 2.0, (B, len(joints), 1)), rw=rng.uniform(0.2, 2.0, len(joints)))
    x["R"][:, ::2] *= -1.0
    return s, joints, x


@pytest.mark.parametrize("fit_root", [0, FIT_ROT])
def test_the_rotation_term_gradient_agrees_with_central_differences(fit_root):
    """float64, the rotation term alone (every position weight 0), h = 1e-5: the truncation error h^2 |f'''| / 6 is
    below 1e-8 for a term of a few units and third derivatives of at most some hundreds, the rounding error
    2^-52 |L| / h about 1e-10: the bound 1e-7 max|grad| leaves room for both and none for a wrong factor."""
    s, joints, x = _case()
    w0 = np.zeros(s.J)
    f = lambda dof, q, t: ref_orient_loss(s, dof, q, t, x["tgt"], w0, True, torch.float64, fit_root, joints, x["R"], x["rw"])
    _, g, gr = ref_orient_loss_grad(s, x["dof"], x["q"], x["t"], x["tgt"], w0, True, torch.float64, fit_root, joints,
                                    x["R"], x["rw"])
    assert np.abs(g).max() > 0.1 and np.abs(gr[:, 3:]).max() > 0.1 and not gr[:, :3].any()
    h = 1e-5
    for name, ad in (("dof", g), ("q", gr[:, 3:])):
        fd = np.zeros_like(ad)
        for i in range(ad.shape[1]):
            args = {k: x[k].copy() for k in ("dof", "q", "t")}
            with torch.no_grad():
                args[name][:, i] += h
                up = f(**args).numpy()
                args[name][:, i] -= 2 * h
                dn = f(**args).numpy()
            fd[:, i] = (up - dn) / (2 * h)
        err = np.abs(fd - ad).max() / np.abs(ad).max()
        print(f"fit_root={fit_root} {name}: max |central difference - autograd| / max |autograd| = {err:.2e}")
        assert err <= 1e-7


def test_the_upstream_adjoint_is_minus_8_w_c_r():
    """dL/dG_j of the rotation term, by autograd on the restatement's own global rotations, is -8 rot_weight[k] c_k R^_k
    -- what the kernel hands child_pull -- it does not see the sign of a target, and 4 (1 - c^2) is the squared chord
    (2 sin(theta / 2))^2 of the angle between unit rotations."""
    s, joints, x = _case()
    dt = torch.float64
    pos, rot, c, g_rot = ref_orient_terms(s, _t(x["dof"], dt).requires_grad_(True), x["q"], x["t"], x["tgt"], np.zeros(s.J),
                                          True, dt, FIT_ROT, joints, x["R"], x["rw"])
    (gb,) = torch.autograd.grad(rot.sum(), g_rot)
    Rh = _t(x["R"], dt) / _t(x["R"], dt).norm(dim=-1, keepdim=True)
    want = torch.zeros_like(gb)
    want[:, joints] = -8.0 * _t(x["rw"], dt).reshape(1, -1, 1) * c.detach().unsqueeze(-1) * Rh
    assert torch.allclose(gb, want, rtol=1e-13, atol=1e-13) and gb.abs().max() > 1
    flipped = ref_orient_terms(s, x["dof"], x["q"], x["t"], x["tgt"], np.zeros(s.J), True, dt, FIT_ROT, joints, -x["R"],
                               x["rw"])[1]
    assert torch.equal(flipped, rot.detach())
    theta = 2.0 * torch.acos(c.detach().abs().clamp(max=1.0))
    assert torch.allclose(4.0 * (1.0 - c.detach() ** 2), (2.0 * torch.sin(theta / 2)) ** 2, atol=1e-12)
    assert not pos.any()


def test_an_oriented_wrist_gets_the_gradient_positions_leave_at_zero():
    """Positions alone: with no weight on the grippers the wrist yaw DOF moves no weighted keypoint and its gradient is
    exactly 0, like the toes' and the neck's.  Orienting those links gives each of these DOFs a gradient."""
    s, _, x = _case(B=4, seed=12)
    w = np.ones(s.J)
    w[[21, 22, 30, 31]] = 0.0   # the grippers: the wrist yaw links become leaves of the weighted tree
    dofs = [j - 1 for j in HU_HANDS_FEET_HEAD]
    joints = list(HU_HANDS_FEET_HEAD)
    R = x["R"]
    args = (s, x["dof"], x["q"], x["t"], x["tgt"], w, True, torch.float64, FIT_ROT)
    _, g0, _ = ref_orient_loss_grad(*args, [], np.zeros((4, 0, 4)), None)
    _, g1, _ = ref_orient_loss_grad(*args, joints, R, None)
    assert (g0[:, dofs] == 0).all()
    assert (g1[:, dofs] != 0).all() and (np.abs(g1[:, dofs]).max(axis=0) > 0.1).all()
    print(f"|dL/da| over the five links' own DOFs with orientation targets: {np.abs(g1[:, dofs]).min():.2e} to "
          f"{np.abs(g1[:, dofs]).max():.2f}")

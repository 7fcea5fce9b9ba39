"""CPU-only checks of the kinematics' gradients: the two backward entry points validate their arguments before any
device work, and a short torch restatement of angle-axis -> FK (the op structure of the drop-in's documented semantics:
rotation3d.py:14-56, :92-98, :122-143, :196-211, kinematics.py:13-39, hu_forward_model.py:17-33) reproduces the
reference's autograd results recorded in tests/golden/fk_grad.npz.  That ties the restatement to the reference, so
tests/test_gpu_fk_grad.py can use it as the reference on a machine without one."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden


# ------------------------------------------------------------------ the restatement (any float dtype, differentiable)
def quat_mul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2
    x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2
    y = w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2
    z = w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2
    return torch.stack([x, y, z, w], dim=-1)


def quat_normalize(q):
    q = (1 - 2 * (q[..., 3:] < 0).to(q.dtype)) * q                        # quat_pos
    return q / q.norm(p=2, dim=-1).unsqueeze(-1).clamp(min=1e-9)          # quat_unit


def quat_rotate(q, v):
    vq = torch.cat([v, torch.zeros_like(v[..., :1])], dim=-1)
    conj = torch.cat([-q[..., :3], q[..., 3:]], dim=-1)
    return quat_mul(quat_mul(q, vq), conj)[..., :3]


def quat_from_angle_axis(angle, axis):
    theta = (angle / 2).unsqueeze(-1)
    axis = axis / axis.norm(p=2, dim=-1, keepdim=True).clamp(min=1e-9)
    return quat_normalize(torch.cat([axis * theta.sin(), theta.cos()], dim=-1))


def fk(local_rot, root_t, parents, local_t):
    """cal_forward_kinematics: (B,J,4), (B,3) -> (B,J,4), (B,J,3); the root is taken unnormalised."""
    g_rot, g_pos = [], []
    for j, p in enumerate(parents):
        if p == -1:
            g_rot.append(local_rot[..., j, :])
            g_pos.append(root_t)
        else:
            g_rot.append(quat_normalize(quat_mul(g_rot[p], local_rot[..., j, :])))
            g_pos.append(quat_rotate(g_rot[p], local_t[j].expand_as(root_t)) + g_pos[p])
    return torch.stack(g_rot, dim=-2), torch.stack(g_pos, dim=-2)


def dof_fk(dof, root_rot, root_t, parents, local_t, axis, lower=None, upper=None):
    """HuForwardModel.forward_kinematics: dof (B,J-1), root_rot (B,4), root_t (B,3); limits given = clip_angles."""
    B, n = dof.shape
    a = dof
    if lower is not None:   # the straight-through clamp
        c = torch.clamp(a.clone(), min=lower.reshape(1, -1), max=upper.reshape(1, -1))
        a = (c - a).detach() + a
    ax = torch.eye(3, dtype=dof.dtype)[torch.as_tensor(axis, dtype=torch.long)].repeat(B, 1, 1)
    lr = quat_from_angle_axis(a.reshape(-1), ax.reshape(-1, 3)).reshape(B, n, 4)
    return fk(torch.cat([root_rot.unsqueeze(1), lr], dim=1), root_t, parents, local_t)


def restated_grads(kind, inputs, consts, cot_rot, cot_pos, dtype=torch.float64):
    """Gradients of sum(cot_rot g_rot) + sum(cot_pos g_pos) through the restatement, on the CPU.  kind "dof": inputs
    (dof, root_rot, root_t), consts (parents, local_t, axis, lower, upper); kind "fk": inputs (local_rot, root_t),
    consts (parents, local_t).  A cotangent may be None.  Returns (forward outputs, gradients), numpy."""
    leaves = [torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_(True) for x in inputs]
    parents = [int(p) for p in consts[0]]
    zl = torch.as_tensor(np.asarray(consts[1])).to(dtype)
    if kind == "dof":
        lo, hi = (None if c is None else torch.as_tensor(np.asarray(c)).to(dtype) for c in consts[3:5])
        g_rot, g_pos = dof_fk(*leaves, parents, zl, consts[2], lo, hi)
    else:
        g_rot, g_pos = fk(*leaves, parents, zl)
    loss = 0
    if cot_rot is not None:
        loss = loss + (g_rot * torch.as_tensor(np.asarray(cot_rot)).to(dtype)).sum()
    if cot_pos is not None:
        loss = loss + (g_pos * torch.as_tensor(np.asarray(cot_pos)).to(dtype)).sum()
    loss.backward()
    return ((g_rot.detach().numpy(), g_pos.detach().numpy()),
            [torch.zeros_like(x).numpy() if x.grad is None else x.grad.numpy() for x in leaves])


DOF_CASES = ("hu_v5_noclip", "hu_clip")
DOF_GRADS = ("dof", "root_rot", "root_t")
FK_GRADS = ("local_rot", "root_t")


def fixture_case(d, tag):
    """(kind, inputs, consts, cot_rot, cot_pos, gradient names) of one fk_grad.npz case."""
    if tag in DOF_CASES:
        lo, hi = (d[f"{tag}_lower"], d[f"{tag}_upper"]) if f"{tag}_lower" in d.files else (None, None)
        return ("dof", [d[f"{tag}_dof"], d[f"{tag}_root_rot"], d[f"{tag}_root_t"]],
                (d[f"{tag}_parents"], d[f"{tag}_local_t"], d[f"{tag}_axis"], lo, hi),
                d[f"{tag}_cot_rot"], d[f"{tag}_cot_pos"], DOF_GRADS)
    return ("fk", [d[f"{tag}_local_rot"], d[f"{tag}_root_t"]], (d[f"{tag}_parents"], d[f"{tag}_local_t"]),
            d[f"{tag}_cot_rot"], d[f"{tag}_cot_pos"], FK_GRADS)


def rel_err(x, g64):
    """E(x) = max|x - g64| / max|g64| of one gradient tensor."""
    g64 = np.asarray(g64, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - g64).max() / np.abs(g64).max())


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("tag", DOF_CASES + ("vtrdyn_full",))
def test_restatement_reproduces_the_reference_gradients(tag):
    """f64 gradients to 1e-12 relative, f32 forward values within the VML residual pinned in test_oracle_golden.py."""
    d = golden("fk_grad")
    kind, inputs, consts, cr, cp, names = fixture_case(d, tag)
    _, grads = restated_grads(kind, inputs, consts, cr, cp, torch.float64)
    for name, g in zip(names, grads):
        want = d[f"{tag}_grad_{name}_f64"]
        assert g.shape == want.shape
        e = rel_err(g, want)
        assert e <= 1e-12, (tag, name, e)
    (g_rot, g_pos), grads32 = restated_grads(kind, inputs, consts, cr, cp, torch.float32)
    assert np.abs(g_rot - d[f"{tag}_g_rot"]).max() <= 2e-6
    assert np.abs(g_pos - d[f"{tag}_g_pos"]).max() <= 2e-6
    for name, g in zip(names, grads32):   # and its f32 gradients err like the reference's own f32 gradients
        want = d[f"{tag}_grad_{name}_f64"]
        assert rel_err(g, want) <= 8 * rel_err(d[f"{tag}_grad_{name}_f32"], want), (tag, name)


def test_fixture_covers_what_it_is_for():
    d = golden("fk_grad")
    for tag in DOF_CASES:
        a = d[f"{tag}_dof"]
        assert a.shape[0] == 64 and (np.abs(a) > np.pi).mean() > 0.5      # the w < 0 flips occur
        n = np.linalg.norm(d[f"{tag}_root_rot"], axis=-1)
        assert n.min() >= 0.5 - 1e-6 and n.max() <= 2 + 1e-6 and n.std() > 0.2
    a, lo, hi = d["hu_clip_dof"], d["hu_clip_lower"], d["hu_clip_upper"]
    assert ((a < lo) | (a > hi)).mean() > 0.8                              # well outside the limits
    assert np.abs(d["hu_clip_grad_dof_f64"][(a < lo) | (a > hi)]).min() > 0   # straight-through: not zeroed
    n = np.linalg.norm(d["vtrdyn_full_local_rot"], axis=-1)
    assert n.min() >= 0.5 - 1e-6 and n.max() <= 2 + 1e-6 and n.std() > 0.2


def test_backward_entry_points_validate_before_device_work():
    from rtg import _lib
    lib = _lib.lib()
    INVALID = 1   # RTG_ERR_INVALID_ARGUMENT
    x = ctypes.c_void_p(64)   # a non-NULL address that is never dereferenced: every call below fails validation
    dof_bw, fk_bw = lib.rtg_dof_fk_backward_f32, lib.rtg_fk_backward_f32
    # NULL handle
    assert dof_bw(None, x, x, x, x, 1, 0, x, x, x, None) == INVALID and b"NULL model" in lib.rtg_last_error()
    assert fk_bw(None, x, x, x, x, 1, x, x, None) == INVALID and b"NULL topology" in lib.rtg_last_error()
    assert dof_bw(None, None, None, None, None, 0, 0, None, None, None, None) == INVALID
    assert fk_bw(None, None, None, None, None, 0, None, None, None) == INVALID
    # B < 0
    assert dof_bw(None, x, x, x, x, -1, 0, x, x, x, None) == INVALID and b"< 0" in lib.rtg_last_error()
    assert fk_bw(None, x, x, x, x, -1, x, x, None) == INVALID and b"< 0" in lib.rtg_last_error()
    # both upstream gradients NULL
    assert dof_bw(None, x, x, None, None, 1, 0, x, x, x, None) == INVALID
    assert b"both upstream gradients" in lib.rtg_last_error()
    assert fk_bw(None, x, x, None, None, 1, x, x, None) == INVALID
    assert b"both upstream gradients" in lib.rtg_last_error()
    # every output NULL
    assert dof_bw(None, x, x, x, None, 1, 0, None, None, None, None) == INVALID
    assert b"every output" in lib.rtg_last_error()
    assert fk_bw(None, x, x, None, x, 1, None, None, None) == INVALID
    assert b"every output" in lib.rtg_last_error()

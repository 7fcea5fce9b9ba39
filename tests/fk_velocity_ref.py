"""Test-side restatement of the link-velocity rule (rtg.h rtg_dof_fk_vel_f32): the tangent sweep written from
``oracle.dof_fk``, ``oracle.quat_rotate`` and numpy float32 products, sums and differences, one rounding each (numpy
does not fuse).  Not a test module.

Per frame, with G, P the poses of ``oracle.dof_fk`` (or poses handed in: a launch's own g_rot isolates the sweep from
the pose bits), l_j joint j's local translation, e_j the unit axis of DOF j - 1 and p the parent of j:
    row 0 = the root twist {v0, w0} (zeros when None);
    r = quat_rotate(G_p, l_j);  c = w_p x r as (product) - (product) per component;  v_j = v_p + c;
    u = quat_rotate(G_j, e_j);  w_j = w_p + (u * s);  s = ad[j-1], or with clip +0 where a[j-1] lies outside its limits.
``sweep`` is the rule itself in the dtype of its inputs with the rotation passed in, so the host tests run the same
lines in float64 (``quat_rotate64``, ``dof_fk64``) against a tangent of the model.  Model: tests/dof_motion_ref.py's
dict (parents, local_t, axis, lower, upper)."""
import numpy as np

import oracle as orc
from motion_sample_ref import bits


def rates(dof, dof_vel, lower=None, upper=None, clip=False):
    """The joints' rates as the sweep takes them: dof_vel, and with clip +0 where the angle is outside [lower, upper] (a
    NaN angle and an angle exactly at a limit keep the rate)."""
    s = np.array(dof_vel, copy=True)
    if clip:
        a = np.asarray(dof)
        with np.errstate(invalid="ignore"):
            out = (a < np.asarray(lower, a.dtype)[None, :]) | (a > np.asarray(upper, a.dtype)[None, :])
        s[out] = 0.0
    return s


def sweep(parents, local_t, axis, g_rot, rate, root_vel, rotate):
    """g_rot (B, J, 4), rate (B, J-1), root_vel (B, 6) -> g_vel (B, J, 6) in g_rot's dtype.  rotate(q (B, 4), v (B, 3))
    is quat_rotate in that dtype."""
    dt = g_rot.dtype
    B, J = g_rot.shape[:2]
    tw = np.zeros((B, J, 6), dt)
    tw[:, 0] = root_vel
    eye = np.eye(3, dtype=dt)
    with np.errstate(all="ignore"):
        for j in range(1, J):
            p = int(parents[j])
            assert 0 <= p < j
            r = rotate(np.ascontiguousarray(g_rot[:, p]), np.ascontiguousarray(np.broadcast_to(local_t[j].astype(dt), (B, 3))))
            v, w = tw[:, p, :3], tw[:, p, 3:]
            c = np.stack([(w[:, 1] * r[:, 2]) - (w[:, 2] * r[:, 1]),
                          (w[:, 2] * r[:, 0]) - (w[:, 0] * r[:, 2]),
                          (w[:, 0] * r[:, 1]) - (w[:, 1] * r[:, 0])], axis=1)
            u = rotate(np.ascontiguousarray(g_rot[:, j]), np.ascontiguousarray(np.broadcast_to(eye[int(axis[j - 1])], (B, 3))))
            tw[:, j, :3] = v + c
            tw[:, j, 3:] = w + (u * rate[:, j - 1:j])
    return tw


def link_twists(model, dof, dof_vel, root_rot, root_t, root_vel=None, clip=False, poses=None):
    """The float32 rule -> (g_rot, g_pos, g_vel).  poses = (g_rot, g_pos) handed in replaces oracle.dof_fk's."""
    dof, dof_vel = np.ascontiguousarray(dof, np.float32), np.ascontiguousarray(dof_vel, np.float32)
    B, J = len(root_rot), len(model["parents"])
    if poses is None:
        lo, hi = (model["lower"], model["upper"]) if clip else (None, None)
        with np.errstate(all="ignore"):
            g_rot, g_pos = orc.dof_fk(model["parents"], model["local_t"], model["axis"], dof.reshape(B, J - 1),
                                      np.ascontiguousarray(root_rot, np.float32), np.ascontiguousarray(root_t, np.float32),
                                      lo, hi)
    else:
        g_rot, g_pos = (np.ascontiguousarray(x, np.float32) for x in poses)
    s = rates(dof.reshape(B, J - 1), dof_vel.reshape(B, J - 1), model["lower"], model["upper"], clip)
    rv = np.zeros((B, 6), np.float32) if root_vel is None else np.ascontiguousarray(root_vel, np.float32)
    return g_rot, g_pos, sweep(model["parents"], np.asarray(model["local_t"], np.float32), model["axis"], g_rot, s, rv,
                               orc.quat_rotate)


# ------------------------------------------------------------------------------------------------ float64 restatements
def qmul64(a, b):
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def quat_rotate64(q, v):
    """q (v, 0) conj(q): quat_rotate (a non-unit q scales by |q|^2)."""
    qv = np.concatenate([v, np.zeros(v.shape[:-1] + (1,), v.dtype)], axis=-1)
    return qmul64(qmul64(q, qv), q * np.array([-1.0, -1.0, -1.0, 1.0]))[..., :3]


def dof_fk64(model, dof, root_rot, root_t, clip=False):
    """The model in float64: local[j] = quat_from_angle_axis(a'[j-1], e), G_j = normalize(G_p local[j]) (the root as
    given), P_j = quat_rotate(G_p, l_j) + P_p; with clip a' = clamp(a, lower, upper)."""
    a = np.asarray(dof, np.float64)
    if clip:
        a = np.clip(a, np.asarray(model["lower"], np.float64), np.asarray(model["upper"], np.float64))
    B, J = len(a), len(model["parents"])
    G, P = np.zeros((B, J, 4)), np.zeros((B, J, 3))
    G[:, 0], P[:, 0] = root_rot, root_t
    lt = np.asarray(model["local_t"], np.float64)
    for j in range(1, J):
        p = int(model["parents"][j])
        lq = np.zeros((B, 4))
        lq[:, int(model["axis"][j - 1])] = np.sin(a[:, j - 1] / 2)
        lq[:, 3] = np.cos(a[:, j - 1] / 2)
        g = qmul64(G[:, p], lq)
        G[:, j] = g / np.linalg.norm(g, axis=-1, keepdims=True)
        P[:, j] = quat_rotate64(G[:, p], np.broadcast_to(lt[j], (B, 3))) + P[:, p]
    return G, P


def link_twists64(model, dof, dof_vel, root_rot, root_t, root_vel=None, clip=False):
    """The rule's own lines in float64 on the float64 model's poses -> (G, P, g_vel)."""
    dof, dof_vel = np.asarray(dof, np.float64), np.asarray(dof_vel, np.float64)
    G, P = dof_fk64(model, dof, root_rot, root_t, clip)
    s = rates(dof, dof_vel, model["lower"], model["upper"], clip)
    rv = np.zeros((len(G), 6)) if root_vel is None else np.asarray(root_vel, np.float64)
    return G, P, sweep(model["parents"], np.asarray(model["local_t"], np.float64), model["axis"], G, s, rv, quat_rotate64)


def advance64(model, dof, dof_vel, root_rot, root_t, root_vel, h):
    """The inputs moved along their velocities for a time h (float64): angles a + h ad, root translation t + h v0, root
    rotation exp(h w0 / 2) q0 -- the world-frame angular velocity w0 applied on the left."""
    rv = np.zeros((len(root_rot), 6)) if root_vel is None else np.asarray(root_vel, np.float64)
    w = rv[:, 3:]
    ang = np.linalg.norm(w, axis=-1, keepdims=True) * h
    half = ang / 2
    k = np.where(ang > 0, np.sin(half) / np.where(ang > 0, ang, 1.0), 0.5)   # sin(|w| h / 2) / (|w| h)
    dq = np.concatenate([w * h * k, np.cos(half)], axis=-1)
    return (np.asarray(dof, np.float64) + h * np.asarray(dof_vel, np.float64), qmul64(dq, np.asarray(root_rot, np.float64)),
            np.asarray(root_t, np.float64) + h * rv[:, :3])


def central_twists64(model, dof, dof_vel, root_rot, root_t, root_vel=None, clip=False, h=1e-6):
    """Central differences of the float64 model along the velocities: v from the positions, w as the world-frame
    angular velocity of G(+h) conj(G(-h)) -> g_vel (B, J, 6)."""
    Gp, Pp = dof_fk64(model, *advance64(model, dof, dof_vel, root_rot, root_t, root_vel, +h), clip)
    Gm, Pm = dof_fk64(model, *advance64(model, dof, dof_vel, root_rot, root_t, root_vel, -h), clip)
    d = qmul64(Gp, Gm * np.array([-1.0, -1.0, -1.0, 1.0]))
    d = d * np.where(d[..., 3:] < 0, -1.0, 1.0)
    n = np.linalg.norm(d[..., :3], axis=-1, keepdims=True)
    ang = 2 * np.arctan2(n, d[..., 3:])
    w = d[..., :3] / np.where(n > 0, n, 1.0) * ang / (2 * h)
    return np.concatenate([(Pp - Pm) / (2 * h), w], axis=-1)


def frame_error(got, want):
    """Per frame: the largest absolute error over the frame's largest magnitude -> (B,)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    B = len(got)
    return np.abs(got - want).reshape(B, -1).max(1) / np.abs(want).reshape(B, -1).max(1)


__all__ = ["rates", "sweep", "link_twists", "link_twists64", "dof_fk64", "quat_rotate64", "qmul64", "advance64",
           "central_twists64", "frame_error", "bits"]

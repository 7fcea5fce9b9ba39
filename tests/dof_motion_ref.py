"""Test-side reference of the joint-angle motion sampler (rtg.h rtg_dof_motion_sample_f32) composed from oracle
primitives and tests/motion_sample_ref.py only, and the builders of its input.  Not a test module.

sample(lib, clip, time, ...): ``motion_sample_ref.index_rule`` and ``blend`` (the angles, the root translation),
``oracle.quat_slerp`` (then ``oracle.quat_normalize``) on the root rotation, dt = float32(1 / float64(fps)), the
velocities as a float32 subtraction and a float32 division (each computed in float64 and rounded once: 53 >= 2 * 24 + 2
bits, so the double rounding is the correctly rounded float32 operation, subnormal quotients included),
``oracle.angular_velocity`` on the two-row sequence [r0, r1] (row 0) and ``oracle.dof_fk`` on the sampled rows for the
global outputs.  An invalid query (clip id outside 0..C-1) is the quiet NaN 0x7FC00000 everywhere.

Library: a dict with dof (F_total, J-1), root_rot (F_total, 4), root_t (F_total, 3), start (C) int64, len (C) int32,
fps (C) float32.  Model: a dict with parents (J) int32, local_t (J, 3), axis (J-1) int32, lower / upper (J-1)."""
import numpy as np

import oracle as orc
from kinematics_frames import rot_sequence
from motion_sample_ref import LIB_FPS, LIB_LENGTHS, bits, blend, f32, index_rule

KEYS = ("dof", "dof_vel", "root_rot", "root_t", "root_vel", "g_rot", "g_pos", "key_pos")


def frame_time(fps):
    """dt = (float)(1.0 / (double)fps)."""
    return f32(1.0 / np.asarray(fps, np.float32).astype(np.float64))


def diff_over_dt(a1, a0, dt):
    """(a1 - a0) / dt in float32: one subtraction, one division.  dt broadcasts over the trailing axes."""
    a1, a0 = np.asarray(a1, np.float32).astype(np.float64), np.asarray(a0, np.float32).astype(np.float64)
    d64 = np.asarray(dt, np.float32).astype(np.float64).reshape((-1,) + (1,) * (a1.ndim - 1))
    with np.errstate(all="ignore"):
        return f32(f32(a1 - a0).astype(np.float64) / d64)


def pair_angular_velocity(r0, r1, dt):
    """SkeletonMotion's raw angular velocity of each pair (r0[n], r1[n]) over dt[n]: oracle.angular_velocity on the
    two-row sequence, row 0; one call per distinct dt (the oracle takes one dt per call)."""
    out = np.zeros((len(r0), 3), np.float32)
    dt = np.asarray(dt, np.float32)
    for d in np.unique(dt.view(np.uint32)).view(np.float32):
        m = dt.view(np.uint32) == np.float32(d).view(np.uint32)
        seq = np.ascontiguousarray(np.stack([r0[m], r1[m]], axis=1)[:, :, None, :], np.float32)   # (n, 2, 1, 4)
        out[m] = orc.angular_velocity(seq, float(d))[:, 0, 0, :]
    return out


def sample(lib, clip, time, normalize=False, velocity=True, model=None, clip_angles=False, want_global=True,
           key_links=None):
    """-> dict of KEYS (None where not asked for) plus valid, row0, row1, b, dt.  ``model`` is needed for the global
    outputs and the key links."""
    clip, time = np.asarray(clip, np.int32), np.asarray(time, np.float32)
    dof, rr, rt = lib["dof"], lib["root_rot"], lib["root_t"]
    N, nd = len(clip), dof.shape[1]
    valid, i0, i1, b = index_rule(clip, time, lib["len"], lib["fps"])
    c = np.where(valid, clip.astype(np.int64), 0)
    st = np.asarray(lib["start"], np.int64)[c]
    r0, r1 = np.where(valid, st + i0, 0), np.where(valid, st + i1, 0)
    assert N == 0 or (r0.min() >= 0 and r1.max() < len(rr))
    dt = frame_time(np.asarray(lib["fps"], np.float32)[c])
    nan = np.float32(np.nan)
    out = {k: None for k in KEYS}
    out.update(valid=valid, row0=r0, row1=r1, b=b, dt=dt)
    d = blend(dof[r0], dof[r1], b) if nd else np.zeros((N, 0), np.float32)
    q = orc.quat_slerp(rr[r0], rr[r1], b) if N else np.zeros((0, 4), np.float32)
    if normalize and N:
        q = orc.quat_normalize(q)
    t = blend(rt[r0], rt[r1], b)
    for x in (d, q, t):
        x[~valid] = nan
    out["dof"], out["root_rot"], out["root_t"] = d, q, t
    if velocity:
        dv = diff_over_dt(dof[r1], dof[r0], dt) if nd else np.zeros((N, 0), np.float32)
        rv = np.concatenate([diff_over_dt(rt[r1], rt[r0], dt), pair_angular_velocity(rr[r0], rr[r1], dt)], axis=1) \
            if N else np.zeros((0, 6), np.float32)
        dv[~valid] = nan
        rv[~valid] = nan
        out["dof_vel"], out["root_vel"] = dv, rv
    keys = None if key_links is None or len(key_links) == 0 else np.asarray(key_links, np.int64)
    if want_global or keys is not None:
        J = nd + 1
        if N:
            lo, hi = (model["lower"], model["upper"]) if clip_angles else (None, None)
            with np.errstate(all="ignore"):
                gr, gp = orc.dof_fk(model["parents"], model["local_t"], model["axis"], d, q, t, lo, hi)
        else:
            gr, gp = np.zeros((0, J, 4), np.float32), np.zeros((0, J, 3), np.float32)
        gr[~valid] = nan
        gp[~valid] = nan
        if want_global:
            out["g_rot"], out["g_pos"] = gr, gp
        if keys is not None:
            out["key_pos"] = np.ascontiguousarray(gp[:, keys])
    return out


# ------------------------------------------------------------------------------------------------ input builders
def make_model(parents, local_t, seed=0):
    """Random axes and limits per DOF for a tree: the model dict."""
    J = len(parents)
    rng = np.random.default_rng(300 + 11 * J + seed)
    lo = rng.uniform(-2.5, -0.2, J - 1).astype(np.float32)
    hi = rng.uniform(0.2, 2.5, J - 1).astype(np.float32)
    return {"parents": np.asarray(parents, np.int32), "local_t": np.asarray(local_t, np.float32),
            "axis": rng.integers(0, 3, J - 1).astype(np.int32), "lower": lo, "upper": hi}


def make_library(nd, family="smooth", lengths=LIB_LENGTHS, fps=LIB_FPS, seed=0):
    """Clips of `lengths` frames at `fps`: angles within +-1.5 rad (a random walk per DOF, so some pass the limits of
    make_model), root rotations of kinematics_frames.rot_sequence(family), random root translations."""
    rng = np.random.default_rng(7000 + 13 * nd + seed)
    Ft = int(sum(lengths))
    dof = np.concatenate([np.clip(rng.normal(0, 0.6, (1, nd)) + rng.normal(0, 0.08, (L, nd)).cumsum(0), -1.5, 1.5)
                          for L in lengths]).astype(np.float32)
    rr = np.concatenate([rot_sequence(family, L, 1, seed + c)[:, 0] for c, L in enumerate(lengths)])
    return {"dof": np.ascontiguousarray(dof), "root_rot": np.ascontiguousarray(rr, np.float32),
            "root_t": rng.normal(0, 0.5, (Ft, 3)).astype(np.float32),
            "start": np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64),
            "len": np.asarray(lengths, np.int32), "fps": np.asarray(fps, np.float32)}


__all__ = ["KEYS", "sample", "frame_time", "diff_over_dt", "pair_angular_velocity", "make_model", "make_library", "bits"]

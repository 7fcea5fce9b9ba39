"""CPU-only checks of the pose fit with the posture prior and the projection (rtg_dof_fit_prior_f32): the symbol is
there under ABI 7 with its prototype, every argument check that needs no handle answers with its own message before any
device work (the handle is NULL and every device address a dummy in all of these calls), the Python entry points raise
RtgError without a GPU, and the reference the GPU tests use -- the restatement of tests/test_orient_fit_host.py with

    sum_d prior_weight[d] (a_d - prior_d)^2     on the iterate a (not on the clamped angle)

added to the loss and ``a.clamp_(lower, upper)`` after ``opt.step()`` -- is anchored: the term's float64 autograd
gradient agrees with central differences and with the closed form 2 prior_weight (a - prior), and on the two pinned
recipes the float64 loop shows what the two options are for: projecting the iterate lets a fit recover after its
targets were out of reach, and a prior towards the neighbours' mean smooths a clip fitted to noisy keypoints."""
import ctypes

import numpy as np
import pytest
import torch

from test_fk_grad_host import dof_fk
from test_orient_fit_host import INVALID, MAX_LINKS, UNSUPPORTED, ref_orient_loss
from test_pose_fit_host import B1, B2, EPS, FIT_ROT, FIT_T, LR, _Hu, _t, ref_pose_loss, root_unit

PROJECT = 1   # RTG_FIT_PROJECT


# ------------------------------------------------------------------ the reference: restatement + term + clamp + Adam
def ref_prior_loss(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw, prior, pw):
    """ref_pose_loss (no links) / ref_orient_loss plus the posture term on the iterate; prior None: no term."""
    if len(joints):
        loss = ref_orient_loss(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw)
    else:
        loss = ref_pose_loss(s, dof, q, t, tgt, w, clip, dtype, fit_root)
    if prior is None:
        return loss
    a = _t(dof, dtype)
    pwt = torch.ones(a.shape[-1], dtype=dtype) if pw is None else _t(pw, dtype)
    return loss + (pwt * (a - _t(prior, dtype)) ** 2).sum(dim=-1)


def ref_prior_loss_grad(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw, prior, pw):
    """-> loss (B), grad (B,J-1), grad_root (B,7) = {dL/dt, dL/dq}, numpy."""
    a, qq, tt = (_t(x, dtype).clone().requires_grad_(True) for x in (dof, q, t))
    loss = ref_prior_loss(s, a, qq, tt, tgt, w, clip, dtype, fit_root, joints, R, rw, prior, pw)
    loss.sum().backward()
    g = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    return loss.detach().numpy(), g(a).numpy(), torch.cat([g(tt), g(qq)], dim=-1).numpy()


class RefFit:
    """The torch loop: torch.optim.Adam with one parameter group per block, the fitted rotation renormalised and --
    with ``project`` -- the angles clamped to the limits after each step.  The optimiser lives as long as the object,
    so targets and prior may change between runs while the state is carried."""
    def __init__(self, s, dof, q, t, w, clip, dtype, fit_root, project=False, joints=(), rw=None, lr=LR, lr_t=LR, lr_q=LR):
        self.s, self.w, self.clip, self.dtype, self.fit_root, self.project = s, w, clip, dtype, fit_root, project
        self.joints, self.rw = list(joints), rw
        self.a, self.q, self.t = (_t(x, dtype).clone().requires_grad_(True) for x in (dof, q, t))
        groups = [dict(params=[self.a], lr=lr)]
        if fit_root & FIT_T:
            groups.append(dict(params=[self.t], lr=lr_t))
        if fit_root & FIT_ROT:
            groups.append(dict(params=[self.q], lr=lr_q))
        self.opt = torch.optim.Adam(groups, betas=(B1, B2), eps=EPS)
        self.lo, self.hi = _t(s.lo, dtype), _t(s.hi, dtype)

    def loss(self, tgt, prior=None, pw=None, R=None):
        return ref_prior_loss(self.s, self.a, self.q, self.t, tgt, self.w, self.clip, self.dtype, self.fit_root,
                              self.joints, R, self.rw, prior, pw)

    def run(self, tgt, iters, prior=None, pw=None, R=None):
        for _ in range(iters):
            self.opt.zero_grad()
            self.loss(tgt, prior, pw, R).sum().backward()
            self.opt.step()
            with torch.no_grad():
                if self.fit_root & FIT_ROT:
                    self.q.copy_(root_unit(self.q))
                if self.project:
                    self.a.copy_(torch.clamp(self.a, self.lo, self.hi))
        return self

    def result(self, tgt, prior=None, pw=None, R=None):
        """-> (loss, dof, q, t) at the iterate, numpy."""
        with torch.no_grad():
            loss = self.loss(tgt, prior, pw, R)
        return tuple(x.detach().numpy().copy() for x in (loss, self.a, self.q, self.t))


def neighbour_mean(a):
    """fit_motion's prior: (a[max(f-1, 0)] + a[min(f+1, L-1)]) / 2 along the first axis."""
    return 0.5 * (np.concatenate([a[:1], a[:-1]]) + np.concatenate([a[1:], a[-1:]]))


def roughness(a):
    """Mean squared second difference of the angles along the frames."""
    return float((np.diff(np.asarray(a, np.float64), 2, axis=0) ** 2).mean())


def _fk64(s, a, clip):
    B = len(a)
    f64 = lambda x: _t(x, torch.float64)
    q = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1))
    with torch.no_grad():
        return dof_fk(f64(a), f64(q), f64(np.zeros((B, 3))), [int(p) for p in s.par], f64(s.lt), s.axis,
                      f64(s.lo) if clip else None, f64(s.hi) if clip else None)[1].numpy()


def _given_root(B):
    return np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1)), np.zeros((B, 3), np.float32)


def projection_recipe():
    """The pinned projection recipe: 33-link Hu, B = 64, the root given as identity, clip on, weights 1, the start at
    mid-range.  Phase 1: 128 steps on targets nobody can reach -- the unclipped FK of angles 0.25-0.5 of the range
    beyond a limit, on a random side per DOF.  Phase 2: 32 steps on the FK of angles at 0.2-0.8 of the range, the
    optimiser state carried.  (Seed 1: the first one tried; none was rejected.)"""
    s = _Hu()
    rng = np.random.default_rng(1)
    B, n = 64, s.J - 1
    span = s.hi - s.lo
    beyond = rng.uniform(0.25, 0.5, (B, n)) * span
    far = np.where(rng.random((B, n)) < 0.5, s.lo - beyond, s.hi + beyond)
    near = s.lo + rng.uniform(0.2, 0.8, (B, n)) * span
    q, t = _given_root(B)
    return s, dict(tgt1=_fk64(s, far, False).astype(np.float32), tgt2=_fk64(s, near, True).astype(np.float32), q=q, t=t,
                   start=np.tile((0.5 * (s.lo + s.hi)).astype(np.float32), (B, 1)), w=np.ones(s.J, np.float32))


def smoothing_recipe():
    """The pinned smoothing recipe: 64 consecutive frames of the 33-link Hu, angles mid + 0.3 range sin(2 pi k f / 64 +
    phi_d) with k in {1, 2} per DOF, the targets their FK plus N(0, 1 cm) noise; the root given as identity, clip on,
    weights 1, the start at mid-range; 8 rounds of 8 steps with projection, smooth_weight 0.1.  (Seed 1: the first one
    tried; none was rejected.)"""
    s = _Hu()
    rng = np.random.default_rng(1)
    L, n = 64, s.J - 1
    mid, span = 0.5 * (s.lo + s.hi), s.hi - s.lo
    k, phi = rng.integers(1, 3, n), rng.uniform(0, 2 * np.pi, n)
    f = np.arange(L)[:, None]
    clean = mid + 0.3 * span * np.sin(2 * np.pi * k * f / L + phi)
    tgt = _fk64(s, clean, True) + rng.normal(0, 0.01, (L, s.J, 3))
    q, t = _given_root(L)
    return s, dict(clean=clean, tgt=tgt.astype(np.float32), q=q, t=t, start=np.tile(mid.astype(np.float32), (L, 1)),
                   w=np.ones(s.J, np.float32), smooth_weight=0.1, rounds=8, iters=8)


def ref_projection_outcome(dtype=torch.float64):
    """-> {project: per-frame loss on the phase-2 targets after both phases}, and how far past a limit the unprojected
    iterate was after phase 1 (rad)."""
    s, x = projection_recipe()
    out, past = {}, None
    for project in (False, True):
        fit = RefFit(s, x["start"], x["q"], x["t"], x["w"], True, dtype, 0, project=project).run(x["tgt1"], 128)
        if not project:
            a = fit.a.detach().numpy()
            past = float(np.maximum(s.lo - a, a - s.hi).max())
        out[project] = fit.run(x["tgt2"], 32).result(x["tgt2"])[0]
    return out, past


def ref_smoothing_outcome(dtype=torch.float64):
    """-> {smoothed: (angles, per-frame keypoint loss on the noisy targets)} and the clean motion's roughness."""
    s, x = smoothing_recipe()
    out = {}
    for smoothed in (False, True):
        fit = RefFit(s, x["start"], x["q"], x["t"], x["w"], True, dtype, 0, project=True)
        for _ in range(x["rounds"]):
            prior = neighbour_mean(fit.a.detach().numpy()) if smoothed else None
            pw = np.full(s.J - 1, x["smooth_weight"]) if smoothed else None
            fit.run(x["tgt"], x["iters"], prior, pw)
        loss, a, _, _ = fit.result(x["tgt"])
        out[smoothed] = (a, loss)
    return out, roughness(x["clean"])


# ------------------------------------------------------------------ the symbol and its argument checks
def _call(lib, **kw):
    """rtg_dof_fit_prior_f32 with a NULL model and never-dereferenced dummy device addresses, fields overridden by
    name; rot_joint: a host array (the call reads it)."""
    x = ctypes.c_void_p(64)
    a = dict(model=None, target_pos=x, weight=x, rot_joint=[0, 5, 2], target_rot=x, rot_weight=x, K=3, prior=x,
             prior_weight=x, flags=PROJECT, root_rot=x, root_t=x, dof_in=x, B=1, clip=0, fit_root=3, iters=1, lr=0.02,
             lr_root_t=0.02, lr_root_rot=0.02, beta1=0.9, beta2=0.999, eps=1e-8, step0=0, m=x, v=x, root_state=x,
             dof_out=x, root_rot_out=x, root_t_out=x, loss=x, grad=x, grad_root=x, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    if a["rot_joint"] is not None:
        a["rot_joint"] = (ctypes.c_int32 * max(len(a["rot_joint"]), 1))(*a["rot_joint"])
    return lib.rtg_dof_fit_prior_f32(*a.values())


def test_symbol_prototype_and_abi_version():
    from rtg import _lib
    lib = _lib.lib()
    fn = lib.rtg_dof_fit_prior_f32
    assert lib.rtg_abi_version() == 7   # a new symbol only: nothing that existed changed
    ori = list(lib.rtg_dof_fit_orient_f32.argtypes)
    assert fn.restype is ctypes.c_int
    # rtg_dof_fit_orient_f32's arguments with (prior, prior_weight, flags) after K
    assert ori[6] is ctypes.c_int32
    assert list(fn.argtypes) == ori[:7] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] + ori[7:]


_NO_OUT = dict(dof_out=None, root_rot_out=None, root_t_out=None, loss=None, grad=None, grad_root=None)


@pytest.mark.parametrize("kw, code, msg", [
    # rtg_dof_fit_orient_f32's
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
    (dict(iters=-1), INVALID, b"iters=-1"),
    (dict(iters=4097), INVALID, b"iters=4097"),
    (dict(step0=-1), INVALID, b"step0=-1"),
    (dict(lr=float("nan")), INVALID, b"must be finite"),
    (dict(lr_root_t=-1e-3), INVALID, b"finite and not negative"),
    (dict(beta1=1.0), INVALID, b"must lie in [0, 1)"),
    (_NO_OUT, INVALID, b"every output is NULL"),
    (dict(K=-1), INVALID, b"K=-1"),
    (dict(K=MAX_LINKS + 1, rot_joint=list(range(MAX_LINKS + 1))), UNSUPPORTED, b"at most 8"),
    (dict(rot_joint=None), INVALID, b"rot_joint or target_rot NULL"),
    (dict(target_rot=ctypes.c_void_p(68)), INVALID, b"16-byte aligned"),
    (dict(rot_joint=[4, 5, 4]), INVALID, b"listed twice"),
    # the new arguments'
    (dict(flags=2), INVALID, b"flags=2 has unknown bits"),
    (dict(flags=3), INVALID, b"flags=3 has unknown bits"),
    (dict(flags=-1), INVALID, b"flags=-1 has unknown bits"),
    (dict(flags=-2 ** 31), INVALID, b"has unknown bits"),
    (dict(prior=None), INVALID, b"prior_weight given without prior"),
    (dict(prior=None, flags=0), INVALID, b"prior_weight given without prior"),
    (dict(prior=None, K=0), INVALID, b"prior_weight given without prior"),
])
def test_validation_before_device_work(kw, code, msg):
    from rtg import _lib
    lib = _lib.lib()
    assert _call(lib, **kw) == code
    assert msg in lib.rtg_last_error(), lib.rtg_last_error()
    assert b"rtg_dof_fit_prior_f32" in lib.rtg_last_error()


def test_valid_arguments_reach_the_handle_check():
    """Every allowed combination of the new arguments passes the checks before the handle's: the call then stops at
    the NULL model (RTG_FIT_PROJECT on a model without limits needs a model: tests/test_gpu_prior_fit.py)."""
    from rtg import _lib
    lib = _lib.lib()
    for kw in (dict(flags=0), dict(flags=PROJECT), dict(prior_weight=None), dict(prior=None, prior_weight=None),
               dict(prior=None, prior_weight=None, flags=0), dict(K=0, rot_joint=None, target_rot=None, rot_weight=None),
               dict(prior=ctypes.c_void_p(68)), dict(fit_root=0), dict(iters=0), dict(m=None, v=None, root_state=None),
               dict(B=0, prior=None, prior_weight=None), dict(dict(_NO_OUT, loss=ctypes.c_void_p(64)))):
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
    o = dict(prior=dof + 0.1, prior_weight=np.full(32, 0.5, np.float32))
    with pytest.raises(_lib.RtgError):
        ops.pose_fit(_NoDeviceModel(), tp, rr, rt, iters=1, project=True, **o)
    with pytest.raises(_lib.RtgError):
        ops.pose_loss(_NoDeviceModel(), dof, rr, rt, tp, **o)
    with pytest.raises(_lib.RtgError):
        ops.dof_fit(_NoDeviceModel(), tp, rr, rt, iters=1, project=True, **o)
    with pytest.raises(_lib.RtgError):
        ops.keypoint_loss(_NoDeviceModel(), dof, tp, rr, rt, **o)
    hu = HuForwardModel.__new__(HuForwardModel)   # its constructor already needs the device
    hu._model, hu.num_joints, hu.node_names = _NoDeviceModel(), 33, [f"n{j}" for j in range(33)]
    h = dict(prior_angles=torch.from_numpy(o["prior"])[..., None], prior_weight=0.5, project_angles=True)
    args = (torch.from_numpy(tp), torch.from_numpy(rt), torch.from_numpy(rr[:, None]))
    with pytest.raises(_lib.RtgError):
        hu.fit_pose(*args, **h)
    with pytest.raises(_lib.RtgError):
        hu.fit_keypoints(*args, **h)
    with pytest.raises(_lib.RtgError):
        hu.fit_motion(*args, project_angles=True)
    with pytest.raises(_lib.RtgError):
        hu.fit_motion(*args, smooth_weight=0.0)
    with pytest.raises(ValueError, match="fit_motion sets prior_angles itself"):   # before anything else
        hu.fit_motion(*args, prior_angles=h["prior_angles"])
    hu._model = type("NoLimits", (_NoDeviceModel,), dict(has_limits=False))()
    with pytest.raises(ValueError, match="project_angles needs DOF limits"):
        hu.fit_pose(*args, clip_angles=False, project_angles=True)


# ------------------------------------------------------------------ the reference itself
def _case(B=3, seed=21):
    s = _Hu()
    rng = np.random.default_rng(seed)
    n = s.J - 1
    quat = lambda *k: (lambda q: q / np.linalg.norm(q, axis=-1, keepdims=True))(rng.normal(size=k + (4,)))
    dof = rng.uniform(s.lo - 0.3, s.hi + 0.3, (B, n))   # some iterates outside the limits
    x = dict(dof=dof, q=quat(B), t=rng.normal(0, 0.3, (B, 3)), tgt=rng.normal(0, 0.5, (B, s.J, 3)),
             prior=dof + rng.uniform(0.5, 2.0, (B, n)) * rng.choice([-1.0, 1.0], (B, n)), pw=rng.uniform(0.2, 2.0, n))
    x["pw"][::3] = 0.0
    return s, x


def test_the_prior_term_gradient_agrees_with_central_differences_and_the_closed_form():
    """float64, the term alone (every position weight 0, clip on: the clamp must not reach the term).  The term is
    quadratic, so the central difference has no truncation error; its rounding error 2^-52 |L| / h with |L| of some
    hundreds and h = 1e-4 is about 1e-9: the bound 1e-7 max|grad| leaves room for it and none for a wrong factor.
    Against the closed form 2 prior_weight (a - prior) autograd owes only the rounding of a handful of operations."""
    s, x = _case()
    w0 = np.zeros(s.J)
    args = (x["q"], x["t"], x["tgt"], w0, True, torch.float64, 0, [], None, None, x["prior"], x["pw"])
    loss, g, gr = ref_prior_loss_grad(s, x["dof"], *args)
    closed = 2.0 * x["pw"] * (x["dof"] - x["prior"])
    assert np.abs(g).max() > 1 and not gr.any()
    assert np.allclose(g, closed, rtol=1e-14, atol=0)
    assert (g[:, ::3] == 0).all()
    assert np.allclose(loss, (x["pw"] * (x["dof"] - x["prior"]) ** 2).sum(-1), rtol=1e-14)
    out = (x["dof"] < s.lo) | (x["dof"] > s.hi)
    assert out.any() and (np.abs(g[out & (x["pw"] > 0)]) > 0).all()   # a run-away iterate is pulled back
    h = 1e-4
    fd = np.zeros_like(g)
    for i in range(g.shape[1]):
        with torch.no_grad():
            up, dn = x["dof"].copy(), x["dof"].copy()
            up[:, i] += h
            dn[:, i] -= h
            fd[:, i] = (ref_prior_loss(s, up, *args).numpy() - ref_prior_loss(s, dn, *args).numpy()) / (2 * h)
    err = np.abs(fd - g).max() / np.abs(g).max()
    print(f"max |central difference - autograd| / max |autograd| = {err:.2e}")
    assert err <= 1e-7
    # with the keypoints' weights on, the term adds to the fit's gradient and a missing prior adds nothing
    full = (x["q"], x["t"], x["tgt"], np.ones(s.J), True, torch.float64, FIT_ROT, [], None, None)
    _, g0, gr0 = ref_prior_loss_grad(s, x["dof"], *full, None, None)
    _, g1, gr1 = ref_prior_loss_grad(s, x["dof"], *full, x["prior"], x["pw"])
    assert np.allclose(g1 - g0, closed, rtol=0, atol=1e-12 * np.abs(g0).max()) and np.array_equal(gr0, gr1)


def test_projection_lets_the_fit_recover_from_unreachable_targets():
    """The float64 loop on the projection recipe: without the projection the straight-through clip lets the iterate
    run past the limits while the targets are out of reach, and 32 steps on reachable targets do not bring it back."""
    loss, past = ref_projection_outcome()
    ratio = loss[False].mean() / loss[True].mean()
    frames = loss[False] / loss[True]
    print(f"unprojected iterate after phase 1: {past:.2f} rad past a limit; mean final loss unprojected "
          f"{loss[False].mean():.3f}, projected {loss[True].mean():.3f}, ratio {ratio:.2f}; per-frame ratio "
          f"min {frames.min():.2f}, median {np.median(frames):.2f}")
    assert past > 1.0
    assert ratio >= 1.5
    assert (loss[True] < loss[False]).all()


def test_a_prior_towards_the_neighbours_smooths_a_noisy_clip():
    """The float64 loop on the smoothing recipe: 8 rounds of 8 projected steps, the prior towards the lagged mean of
    the two neighbours refreshed before each round."""
    out, clean = ref_smoothing_outcome()
    r_ind, r_smo = roughness(out[False][0]), roughness(out[True][0])
    l_ind, l_smo = out[False][1].mean(), out[True][1].mean()
    print(f"roughness: clean {clean:.2e}, independent {r_ind:.2e}, smoothed {r_smo:.2e}, ratio {r_ind / r_smo:.1f}; "
          f"mean noisy-target loss independent {l_ind:.5f}, smoothed {l_smo:.5f} ({100 * (l_smo / l_ind - 1):+.2f} %)")
    assert r_ind / r_smo >= 10
    assert l_smo <= 1.02 * l_ind

"""CPU-only checks of the pose fit with per-frame keypoint weights and a robust keypoint loss (rtg_dof_fit_robust_f32):
the symbol is there under ABI 7 with its prototype, every new argument check answers with its own message before any
device work (the handle is NULL and every device address a dummy in all of these calls), the Python entry points raise
RtgError without a GPU and ValueError on a keyword of the wrong shape or type, and the reference the GPU tests use -- the
restatement of tests/test_apart_fit_host.py with the keypoint term replaced by

    sum over the j with frame_weight[f,j] != 0 of  weight[j] frame_weight[f,j] rho(|P_j - T_fj|^2),
    rho(s) = s  or, with robust_scale = delta > 0,  2 s / (sqrt(1 + s / delta^2) + 1)

-- is anchored: masked target rows are replaced by zeros before the residual is formed (so a masked NaN cannot leak
through autograd), the float64 autograd gradient agrees with central differences and with the closed form
2 e d / sqrt(1 + s / delta^2), and rho's cancellation-free form equals 2 delta^2 (sqrt(1 + s / delta^2) - 1).  On two
pinned recipes the float64 loop shows what the two options are for: a keypoint half a metre off no longer drags the
other links, and dropped frames are filled in from their neighbours."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_apart_fit_host import _apart, ref_apart_loss
from test_fk_grad_host import dof_fk
from test_orient_fit_host import INVALID
from test_pose_fit_host import FIT_ROT, FIT_T, _Hu, _t, root_unit
from test_prior_fit_host import PROJECT, RefFit, _fk64, _NoDeviceModel, neighbour_mean, smoothing_recipe


# ------------------------------------------------------------------ the reference: restatement with the new keypoint term
def inv_d2(delta, dtype):
    """1 / delta^2 as the launch receives it: formed in double; float32: rounded once.  delta may be a (B,) array, one
    scale per frame with 0 for the quadratic loss (rho with 1 / delta^2 = 0 is s exactly): -> (B,1) tensor."""
    d = np.asarray(delta, np.float64)
    with np.errstate(divide="ignore"):
        v = np.where(d > 0, 1.0 / (d * d), 0.0)
    if dtype == torch.float32:
        v = v.astype(np.float32)
    return float(v) if v.ndim == 0 else torch.as_tensor(v).to(dtype).reshape(-1, 1)


class _Rho(torch.autograd.Function):
    """rho(s) = 2 s / (sqrt(1 + s inv) + 1) with the header's adjoint d rho / d s = 1 / sqrt(1 + s inv): what the float32
    restatement of the launch computes (autograd of the quotient can lose where the closed form is finite)."""
    @staticmethod
    def forward(ctx, s, inv):
        q = torch.sqrt(1 + s * inv)
        ctx.save_for_backward(q)
        return (2 * s) / (q + 1)

    @staticmethod
    def backward(ctx, g):
        (q,) = ctx.saved_tensors
        return g / q, None


def rho(s, delta, dtype, closed=False):
    if np.ndim(delta) == 0 and not delta:
        return s
    inv = inv_d2(delta, dtype)
    return _Rho.apply(s, inv) if closed else (2 * s) / (torch.sqrt(1 + s * inv) + 1)


def ref_keypoint_term(s, dof, q, t, tgt, w, clip, dtype, fit_root, fw, delta, closed=False):
    """The keypoint term per frame (B,).  fw (B,J) or None for ones.  A masked keypoint's target row is replaced by
    zeros BEFORE d is formed and its weight by 0: torch.where on the product alone would still send NaN back."""
    q = _t(q, dtype)
    lo, hi = (_t(s.lo, dtype), _t(s.hi, dtype)) if clip else (None, None)
    gp = dof_fk(_t(dof, dtype), root_unit(q) if fit_root & FIT_ROT else q, _t(t, dtype), [int(p) for p in s.par],
                _t(s.lt, dtype), s.axis, lo, hi)[1]
    tg = _t(tgt, dtype)
    wt = torch.ones(s.J, dtype=dtype) if w is None else _t(w, dtype)
    if fw is None:
        e = wt.reshape(1, -1).expand(gp.shape[0], -1)
    else:
        f = _t(fw, dtype)
        on = f != 0
        tg = torch.where(on[..., None], tg, torch.zeros_like(tg))
        e = torch.where(on, wt.reshape(1, -1) * f, torch.zeros_like(f))
    ss = ((gp - tg) ** 2).sum(dim=-1)
    terms = e * rho(ss, delta, dtype, closed)
    if fw is not None:
        terms = torch.where(on, terms, torch.zeros_like(terms))
    return terms.sum(dim=-1)


def ref_robust_loss(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw, prior, pw, ap, fw, delta, closed=False):
    """ref_apart_loss with the keypoint term above in place of its own (taken out by zero weights on zero targets)."""
    B = _t(dof, dtype).shape[0]
    term = ref_keypoint_term(s, dof, q, t, tgt, w, clip, dtype, fit_root, fw, delta, closed)
    if not len(joints) and ap is None:   # nothing else needs the forward model: the posture term as ref_prior_loss has it
        if prior is None:
            return term
        a = _t(dof, dtype)
        pwt = torch.ones(a.shape[-1], dtype=dtype) if pw is None else _t(pw, dtype)
        return term + (pwt * (a - _t(prior, dtype)) ** 2).sum(dim=-1)
    rest = ref_apart_loss(s, dof, q, t, np.zeros((B, s.J, 3)), np.zeros(s.J), clip, dtype, fit_root, joints, R, rw, prior, pw, ap)
    return rest + term


def ref_robust_loss_grad(s, dof, q, t, *rest, **kw):
    """-> loss (B), grad (B,J-1), grad_root (B,7) = {dL/dt, dL/dq}, numpy."""
    a, qq, tt = (_t(x, rest[3]).clone().requires_grad_(True) for x in (dof, q, t))
    loss = ref_robust_loss(s, a, qq, tt, *rest, **kw)
    loss.sum().backward()
    g = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    return loss.detach().numpy(), g(a).numpy(), torch.cat([g(tt), g(qq)], dim=-1).numpy()


def frame_weights(B, J, seed):
    """Random frame weights in 0.2-2, a third of them 0 (the GPU tests' generator)."""
    rng = np.random.default_rng(seed)
    fw = rng.uniform(0.2, 2.0, (B, J))
    fw[rng.random((B, J)) < 1 / 3] = 0.0
    return fw.astype(np.float32)


class RefRobustFit(RefFit):
    """test_prior_fit_host.RefFit's loop on the loss with frame weights ``fw`` and the robust scale ``delta`` (a number,
    or one per frame: frames are independent and Adam is elementwise, so runs that differ only in fw and delta can be
    stacked along the batch and give what they give alone)."""
    def __init__(self, *args, fw=None, delta=0.0, **kw):
        super().__init__(*args, **kw)
        self.fw, self.delta = fw, delta

    def loss(self, tgt, prior=None, pw=None, R=None):
        return ref_robust_loss(self.s, self.a, self.q, self.t, tgt, self.w, self.clip, self.dtype, self.fit_root, self.joints,
                               R, self.rw, prior, pw, None, self.fw, self.delta)


# ------------------------------------------------------------------ the two pinned recipes
OUTLIER_JOINT, OUTLIER_SHIFT, OUTLIER_DELTA = 20, 0.5, 0.05
DROPPED = np.r_[20:24, 40:48]


def outlier_recipe():
    """The pinned outlier recipe: the smoothing recipe's clean clip (64 frames of the 33-link Hu, the root given as
    identity, clip and projection on, weights 1, the start at mid-range), the targets its FK, and joint 20 -- an arm
    keypoint -- moved 0.5 m along a random unit vector in frames 0, 4, 8, ...; 512 projected steps.  (Seed 1 for the
    directions: the first one tried; none was rejected.)"""
    s, x = smoothing_recipe()
    rng = np.random.default_rng(1)
    L = len(x["clean"])
    clean_pos = _fk64(s, x["clean"], True)
    bad = np.arange(0, L, 4)
    u = rng.normal(size=(len(bad), 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    tgt = clean_pos.copy()
    tgt[bad, OUTLIER_JOINT] += OUTLIER_SHIFT * u
    fw = np.ones((L, s.J), np.float32)
    fw[bad, OUTLIER_JOINT] = 0.0
    return s, dict(x, tgt=tgt.astype(np.float32), clean_pos=clean_pos, bad=bad, fw=fw, iters=512, delta=OUTLIER_DELTA)


def dropout_recipe(fill=0.0):
    """The pinned dropout recipe: the smoothing recipe itself (its targets carry N(0, 1 cm) noise; seed 1) with frames
    20-23 and 40-47 arriving as rows of ``fill`` (zeros: what the ingest hands out for a dropped packet); 16 rounds of
    8 projected steps.  Nothing random is added: no further seed."""
    s, x = smoothing_recipe()
    tgt = x["tgt"].copy()
    tgt[DROPPED] = fill
    fw = np.ones((len(tgt), s.J), np.float32)
    fw[DROPPED] = 0.0
    return s, dict(x, tgt=tgt, clean_pos=_fk64(s, x["clean"], True), fw=fw, rounds=16, iters=8)


def link_error(s, a, clean_pos, frames, skip=()):
    """Mean distance (m) of the fitted links to the clean motion's over ``frames``, the links in ``skip`` left out."""
    keep = np.array([j for j in range(s.J) if j not in skip])
    d = np.linalg.norm(_fk64(s, a, True) - clean_pos, axis=-1)
    return float(d[np.ix_(np.asarray(frames), keep)].mean())


@functools.lru_cache(maxsize=None)
def ref_outlier_outcome():
    """-> {run: (error of the other links in the corrupted frames, in the clean frames)} for quadratic, robust, masked."""
    s, x = outlier_recipe()
    L = len(x["tgt"])
    good = np.setdiff1d(np.arange(L), x["bad"])
    runs = ("quadratic", "robust", "masked")   # stacked along the batch
    x3 = lambda a: np.concatenate([a] * 3)
    fit = RefRobustFit(s, x3(x["start"]), x3(x["q"]), x3(x["t"]), x["w"], True, torch.float64, 0, project=True,
                       fw=np.concatenate([np.ones_like(x["fw"]), np.ones_like(x["fw"]), x["fw"]]),
                       delta=np.repeat([0.0, x["delta"], 0.0], L))
    a = fit.run(x3(x["tgt"]), x["iters"]).result(x3(x["tgt"]))[1]
    return {run: (link_error(s, a[i * L:(i + 1) * L], x["clean_pos"], x["bad"], (OUTLIER_JOINT,)),
                  link_error(s, a[i * L:(i + 1) * L], x["clean_pos"], good, (OUTLIER_JOINT,))) for i, run in enumerate(runs)}


@functools.lru_cache(maxsize=None)
def ref_dropout_outcome():
    """-> {(masked, smoothed): (error in the dropped frames, in the kept frames)}."""
    s, x = dropout_recipe()
    L = len(x["tgt"])
    kept = np.setdiff1d(np.arange(L), DROPPED)
    x2 = lambda a: np.concatenate([a] * 2)
    out = {}
    for smoothed in (False, True):   # unmasked and masked stacked along the batch, each clip with its own neighbours
        fit = RefRobustFit(s, x2(x["start"]), x2(x["q"]), x2(x["t"]), x["w"], True, torch.float64, 0, project=True,
                           fw=np.concatenate([np.ones_like(x["fw"]), x["fw"]]))
        for _ in range(x["rounds"]):
            a = fit.a.detach().numpy()
            prior = np.concatenate([neighbour_mean(a[:L]), neighbour_mean(a[L:])]) if smoothed else None
            pw = np.full(s.J - 1, x["smooth_weight"]) if smoothed else None
            fit.run(x2(x["tgt"]), x["iters"], prior, pw)
        a = fit.result(x2(x["tgt"]))[1]
        for masked in (False, True):
            am = a[L:] if masked else a[:L]
            out[masked, smoothed] = (link_error(s, am, x["clean_pos"], DROPPED), link_error(s, am, x["clean_pos"], kept))
    return out


# ------------------------------------------------------------------ the symbol and its argument checks
def _call(lib, apart=None, **kw):
    """rtg_dof_fit_robust_f32 with a NULL model and never-dereferenced dummy device addresses, fields overridden by
    name; apart: _apart's overrides, or None for a NULL struct."""
    x = ctypes.c_void_p(64)
    a = dict(model=None, target_pos=x, weight=x, rot_joint=[0, 5, 2], target_rot=x, rot_weight=x, K=3, prior=x,
             prior_weight=x, flags=PROJECT, root_rot=x, root_t=x, dof_in=x, B=1, clip=0, fit_root=3, iters=1, lr=0.02,
             lr_root_t=0.02, lr_root_rot=0.02, beta1=0.9, beta2=0.999, eps=1e-8, step0=0, m=x, v=x, root_state=x,
             dof_out=x, root_rot_out=x, root_t_out=x, loss=x, grad=x, grad_root=x)
    tail = dict(frame_weight=x, robust_scale=0.05)
    assert set(kw) <= set(a) | set(tail)
    a.update({k: v for k, v in kw.items() if k in a})
    tail.update({k: v for k, v in kw.items() if k in tail})
    if a["rot_joint"] is not None:
        a["rot_joint"] = (ctypes.c_int32 * max(len(a["rot_joint"]), 1))(*a["rot_joint"])
    st, keep = (None, None) if apart is None else _apart(**dict(apart))
    return lib.rtg_dof_fit_robust_f32(*a.values(), None if st is None else ctypes.byref(st), tail["frame_weight"],
                                      tail["robust_scale"], None)


def test_symbol_prototype_and_abi_version():
    from rtg import _lib
    lib = _lib.lib()
    fn = lib.rtg_dof_fit_robust_f32
    assert lib.rtg_abi_version() == 7   # a new symbol only: nothing that existed changed
    ap = list(lib.rtg_dof_fit_apart_f32.argtypes)
    assert fn.restype is ctypes.c_int
    # rtg_dof_fit_apart_f32's arguments with (frame_weight, robust_scale) before the stream
    assert list(fn.argtypes) == ap[:-1] + [ctypes.c_void_p, ctypes.c_float, ap[-1]]


@pytest.mark.parametrize("kw, apart, msg", [
    (dict(robust_scale=-0.05), None, b"robust_scale=-0.05 must be finite and not negative"),
    (dict(robust_scale=-1e-30), None, b"must be finite and not negative"),
    (dict(robust_scale=float("inf")), None, b"robust_scale=inf must be finite and not negative"),
    (dict(robust_scale=float("-inf")), None, b"robust_scale=-inf must be finite and not negative"),
    (dict(robust_scale=float("nan")), None, b"robust_scale=nan must be finite and not negative"),
    (dict(robust_scale=-1.0, frame_weight=None), None, b"robust_scale=-1 must be finite and not negative"),
    (dict(robust_scale=-1.0, B=0), None, b"robust_scale=-1 must be finite and not negative"),
    # rtg_dof_fit_apart_f32's come through the new symbol under its name
    (dict(B=-1), None, b"< 0"),
    (dict(flags=2), None, b"flags=2 has unknown bits"),
    (dict(target_pos=None), None, b"NULL buffer"),
    (dict(), dict(S=-1), b"S=-1 < 0"),
    (dict(), dict(margin=float("nan")), b"margin=nan must be finite"),
])
def test_validation_before_device_work(kw, apart, msg):
    from rtg import _lib
    lib = _lib.lib()
    assert _call(lib, apart, **kw) == INVALID
    assert msg in lib.rtg_last_error(), lib.rtg_last_error()
    assert b"rtg_dof_fit_robust_f32" in lib.rtg_last_error()


def test_valid_arguments_reach_the_handle_check():
    """Every allowed combination of the new arguments passes the checks before the handle's: the call then stops at
    the NULL model."""
    from rtg import _lib
    lib = _lib.lib()
    for kw in (dict(), dict(frame_weight=None), dict(robust_scale=0.0), dict(frame_weight=None, robust_scale=0.0),
               dict(robust_scale=-0.0), dict(robust_scale=1e-30), dict(robust_scale=1e30), dict(B=0),
               dict(frame_weight=ctypes.c_void_p(68)), dict(B=0, frame_weight=None)):
        for apart in (None, {}):
            assert _call(lib, apart, **kw) == INVALID and b"NULL model" in lib.rtg_last_error(), (kw, lib.rtg_last_error())


def test_python_entry_points_raise_rtg_error_without_a_gpu(monkeypatch):
    from rtg import _lib, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the same test on a machine that has one
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    tp = np.zeros((2, 33, 3), np.float32)
    rr = np.tile(np.array([0, 0, 0, 1], np.float32), (2, 1))
    rt = np.zeros((2, 3), np.float32)
    dof = np.zeros((2, 32), np.float32)
    fw = np.ones((2, 33), np.float32)
    for o in (dict(frame_weight=fw), dict(robust_scale=0.05), dict(frame_weight=fw > 0, robust_scale=0.05)):
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
    h = dict(keypoint_confidence=torch.from_numpy(fw), robust_scale=0.05)
    args = (torch.from_numpy(tp), torch.from_numpy(rt), torch.from_numpy(rr[:, None]))
    with pytest.raises(_lib.RtgError):
        hu.fit_pose(*args, **h)
    with pytest.raises(_lib.RtgError):
        hu.fit_keypoints(*args, **h)
    with pytest.raises(_lib.RtgError):
        hu.fit_motion(*args, **h)
    tree = type("Tree", (), dict(node_names=["a", "b"], parent_indices=[-1, 0], local_translation=np.zeros((2, 3))))
    with pytest.raises(_lib.RtgError):
        hu.fit_mocap(tree, {"a": "n0"}, np.zeros((2, 2, 3), np.float32), source_confidence=np.ones((2, 2)), valid=[True, False])


@pytest.mark.parametrize("o, msg", [
    (dict(frame_weight=np.ones((2, 32), np.float32)), "frame_weight"),
    (dict(frame_weight=np.ones((3, 33), np.float32)), "frame_weight"),
    (dict(frame_weight=np.ones(33, np.float32)), "frame_weight"),
    (dict(frame_weight=np.ones((2, 33, 1), np.float32)), "frame_weight"),
    (dict(frame_weight=np.ones((2, 33), np.complex64)), "frame_weight must be real"),
    (dict(robust_scale=-0.05), "robust_scale"),
    (dict(robust_scale=float("nan")), "robust_scale"),
    (dict(robust_scale=float("inf")), "robust_scale"),
    (dict(robust_scale="0.05"), "robust_scale must be a number"),
    (dict(robust_scale=[0.05]), "robust_scale must be a number"),
])
def test_shape_and_dtype_errors_of_the_new_keywords(o, msg):
    """Checked before anything asks for the device: a ValueError with or without a GPU."""
    from rtg import ops
    tp = np.zeros((2, 33, 3), np.float32)
    rr = np.tile(np.array([0, 0, 0, 1], np.float32), (2, 1))
    rt = np.zeros((2, 3), np.float32)
    dof = np.zeros((2, 32), np.float32)
    with pytest.raises(ValueError, match=msg):
        ops.pose_fit(_NoDeviceModel(), tp, rr, rt, iters=1, **o)
    with pytest.raises(ValueError, match=msg):
        ops.dof_fit(_NoDeviceModel(), tp, rr, rt, iters=1, **o)
    with pytest.raises(ValueError, match=msg):
        ops.pose_loss(_NoDeviceModel(), dof, rr, rt, tp, **o)
    with pytest.raises(ValueError, match=msg):
        ops.keypoint_loss(_NoDeviceModel(), dof, tp, rr, rt, **o)


# ------------------------------------------------------------------ the reference itself
def _case(B=3, seed=41):
    s = _Hu()
    rng = np.random.default_rng(seed)
    n = s.J - 1
    quat = lambda *k: (lambda q: q / np.linalg.norm(q, axis=-1, keepdims=True))(rng.normal(size=k + (4,)))
    x = dict(dof=rng.uniform(s.lo, s.hi, (B, n)), q=quat(B), t=rng.normal(0, 0.3, (B, 3)), w=rng.uniform(0.2, 2.0, s.J),
             fw=frame_weights(B, s.J, seed + 1).astype(np.float64))
    x["tgt"] = _fk64(s, x["dof"], True) * 0 + rng.normal(0, 0.5, (B, s.J, 3))   # residuals from well below delta to far above
    x["tgt"][:, ::2] = 0.02 * rng.normal(size=x["tgt"][:, ::2].shape)
    return s, x


def test_rho_has_no_cancellation_and_the_right_limits():
    """float64: the form used equals 2 delta^2 (sqrt(1 + s / delta^2) - 1) to rounding where that form has digits left,
    is s to first order and 2 delta |d| far out."""
    for delta in (1e-3, 0.05, 2.0):
        s = torch.logspace(-12, 6, 400, dtype=torch.float64) * delta * delta
        r = rho(s, delta, torch.float64)
        naive = 2 * delta * delta * (torch.sqrt(1 + s / (delta * delta)) - 1)
        big = s >= 1e-3 * delta * delta    # the naive form has lost at most 3 of its 16 digits there
        assert torch.allclose(r[big], naive[big], rtol=1e-12, atol=0)
        small = s <= 1e-10 * delta * delta
        assert torch.allclose(r[small], s[small], rtol=1e-9, atol=0)       # s (1 - s / (4 delta^2) + ...)
        far = s >= 1e10 * delta * delta
        assert torch.allclose(r[far], 2 * delta * torch.sqrt(s[far]), rtol=1e-4, atol=0)
        assert (r <= s).all() and (r[1:] > r[:-1]).all()
    # float32, small s: the naive form cancels to nothing, the form used keeps s
    s32 = torch.tensor([1e-10], dtype=torch.float32)
    assert float(rho(s32, 0.05, torch.float32)) == pytest.approx(1e-10, rel=1e-6)
    assert float(2 * 0.05 ** 2 * (torch.sqrt(1 + s32 / 0.05 ** 2) - 1)) == 0.0


@pytest.mark.parametrize("delta", [0.0, 0.05])
def test_the_gradient_agrees_with_central_differences_and_the_closed_form(delta):
    """float64.  Central differences with h = 1e-6 on a loss of order 10 with third derivatives of order 10 / delta^2:
    truncation about h^2 / 6 * 4e3 = 1e-9 and rounding 2^-52 * 10 / h = 2e-9 against gradients of order 1: the bound
    1e-6 max|grad| leaves room for both and none for a wrong factor.  The closed form 2 e d / sqrt(1 + s / delta^2) is
    what the launch uses as the keypoints' adjoint: autograd of the restatement with it agrees with plain autograd to
    rounding."""
    s, x = _case()
    args = (x["q"], x["t"], x["tgt"], x["w"], True, torch.float64, FIT_T | FIT_ROT, [], None, None, None, None, None, x["fw"], delta)
    loss, g, gr = ref_robust_loss_grad(s, x["dof"], *args)
    _, gc, grc = ref_robust_loss_grad(s, x["dof"], *args, closed=True)
    assert np.allclose(g, gc, rtol=0, atol=1e-13 * np.abs(g).max()) and np.allclose(gr, grc, rtol=0, atol=1e-13 * np.abs(gr).max())
    # dL/dt is the sum of the keypoints' adjoints: the closed form itself
    gp = _fk64(s, x["dof"], True)
    with torch.no_grad():
        qn = root_unit(_t(x["q"], torch.float64))
        gp = dof_fk(_t(x["dof"], torch.float64), qn, _t(x["t"], torch.float64), [int(p) for p in s.par],
                    _t(s.lt, torch.float64), s.axis, _t(s.lo, torch.float64), _t(s.hi, torch.float64))[1].numpy()
    d = gp - x["tgt"]
    ss = (d ** 2).sum(-1)
    e = x["w"] * x["fw"]
    adj = 2 * e[..., None] * d / np.sqrt(1 + ss / delta ** 2)[..., None] if delta else 2 * e[..., None] * d
    assert np.allclose(gr[:, :3], adj.sum(1), rtol=1e-12, atol=1e-12)
    assert (x["fw"] == 0).any() and (x["fw"] != 0).any()
    h = 1e-6
    fd = np.zeros_like(g)
    for i in range(g.shape[1]):
        with torch.no_grad():
            up, dn = x["dof"].copy(), x["dof"].copy()
            up[:, i] += h
            dn[:, i] -= h
            fd[:, i] = (ref_robust_loss(s, up, *args).numpy() - ref_robust_loss(s, dn, *args).numpy()) / (2 * h)
    err = np.abs(fd - g).max() / np.abs(g).max()
    print(f"delta={delta}: max |central difference - autograd| / max |autograd| = {err:.2e}")
    assert err <= 1e-6
    # frame weights of ones are no frame weights, and without either this is the restatement it started from
    ones = args[:-2] + (np.ones_like(x["fw"]), delta)
    none = args[:-2] + (None, delta)
    assert np.array_equal(ref_robust_loss_grad(s, x["dof"], *ones)[0], ref_robust_loss_grad(s, x["dof"], *none)[0])
    if not delta:
        old = ref_apart_loss(s, x["dof"], x["q"], x["t"], x["tgt"], x["w"], True, torch.float64, FIT_T | FIT_ROT, [], None, None,
                             None, None, None).numpy()
        assert np.allclose(ref_robust_loss_grad(s, x["dof"], *none)[0], old, rtol=1e-14)


@pytest.mark.parametrize("delta", [0.0, 0.05])
def test_a_masked_target_row_cannot_leak(delta):
    """Masked rows of NaN, inf and 1e300: the loss and every gradient are those of the run with the rows zeroed, bit for
    bit, in float64 and float32; the same rows unmasked do poison their frames (and only theirs)."""
    s, x = _case()
    for dtype in (torch.float64, torch.float32):
        args = lambda tgt, fw: (x["q"], x["t"], tgt, x["w"], True, dtype, FIT_T | FIT_ROT, [], None, None, None, None, None, fw, delta)
        bad, zero = x["tgt"].copy(), x["tgt"].copy()
        off = x["fw"] == 0
        fill = np.resize([np.nan, np.inf, -np.inf, 1e300], int(off.sum()))
        bad[off] = fill[:, None]
        zero[off] = 0.0
        got, want = ref_robust_loss_grad(s, x["dof"], *args(bad, x["fw"])), ref_robust_loss_grad(s, x["dof"], *args(zero, x["fw"]))
        for a, b in zip(got, want):
            assert np.isfinite(a).all() and np.array_equal(a, b)
        fw = x["fw"].copy()
        fw[1] = 1.0
        loss, g, gr = ref_robust_loss_grad(s, x["dof"], *args(bad, fw))
        assert not np.isfinite(loss[1]) and np.isfinite(loss[[0, 2]]).all() and np.isfinite(g[[0, 2]]).all()
    # a frame with every keypoint masked: a keypoint loss of exactly 0 and no gradient
    fw = x["fw"].copy()
    fw[0] = 0.0
    loss, g, gr = ref_robust_loss_grad(s, x["dof"], x["q"], x["t"], x["tgt"], x["w"], True, torch.float64, 3, [], None, None, None,
                                       None, None, fw, delta)
    assert loss[0] == 0 and not g[0].any() and not gr[0].any() and loss[1] > 0


# ------------------------------------------------------------------ the two pinned outcomes on the float64 loop
def test_a_robust_loss_or_a_mask_keeps_an_outlier_from_dragging_the_other_links():
    """The float64 loop on the outlier recipe.  Measured: the other links' mean error in the corrupted frames is
    15.46 mm under the quadratic loss, 2.15 mm with the robust kernel (delta = 0.05 m) and 2.13 mm with that keypoint
    masked in those frames (7.2 times less either way); in the clean frames 2.36, 0.53 and 2.36 mm.  The pins leave
    room for another torch's rounding, not for a lost effect."""
    out = ref_outlier_outcome()
    (q_bad, q_good), (r_bad, r_good), (m_bad, m_good) = out["quadratic"], out["robust"], out["masked"]
    print(f"other links' mean error in the corrupted frames: quadratic {1e3 * q_bad:.2f} mm, robust (delta = "
          f"{OUTLIER_DELTA}) {1e3 * r_bad:.2f} mm, masked {1e3 * m_bad:.2f} mm; in the clean frames: quadratic "
          f"{1e3 * q_good:.2f} mm, robust {1e3 * r_good:.2f} mm, masked {1e3 * m_good:.2f} mm")
    assert q_bad >= PIN["outlier_quadratic_min"]
    assert r_bad <= PIN["outlier_robust_max"] and m_bad <= PIN["outlier_masked_max"]
    assert q_bad / r_bad >= PIN["outlier_ratio_min"] and q_bad / m_bad >= PIN["outlier_ratio_min"]
    assert r_good <= 1.05 * q_good + 1e-4   # the clean frames are no worse with the robust kernel


def test_masked_frames_are_filled_in_from_their_neighbours():
    """The float64 loop on the dropout recipe: unmasked, the zero rows pull the dropped frames to a heap at the origin,
    smoothed or not; masked and fitted alone they stay at the start; masked with the neighbour-mean prior they are
    filled in from the ends of their gap.  The kept frames are not touched by the mask.  Measured, mean error in the
    dropped frames: unmasked 0.4015 m (smoothed 0.3943 m), masked 0.1961 m, masked and smoothed 0.0753 m; in the kept
    frames 18.26 / 19.52 / 18.26 / 18.72 mm."""
    out = ref_dropout_outcome()
    txt = ", ".join(f"{'masked' if m else 'unmasked'}{' + smoothing' if sm else ''} {d:.4f} m (kept frames {1e3 * k:.2f} mm)"
                    for (m, sm), (d, k) in out.items())
    print(f"mean error in the dropped frames: {txt}")
    assert min(out[False, False][0], out[False, True][0]) >= PIN["dropout_unmasked_min"]
    assert out[True, False][0] <= PIN["dropout_masked_max"]
    assert out[True, True][0] <= PIN["dropout_filled_max"]
    assert out[True, True][0] <= 0.5 * out[True, False][0] <= 0.5 * out[False, True][0]
    assert out[True, False][1] <= 1.02 * out[False, False][1]   # the kept frames, fitted alone: unchanged by the mask
    assert out[True, True][1] <= 1.02 * out[False, True][1] + 1e-4


# the measured outcomes (float64 loop, this file's recipes) and the pins taken from them
PIN = dict(outlier_quadratic_min=0.012, outlier_robust_max=0.003, outlier_masked_max=0.003, outlier_ratio_min=5.0,
           dropout_unmasked_min=0.3, dropout_masked_max=0.25, dropout_filled_max=0.1)

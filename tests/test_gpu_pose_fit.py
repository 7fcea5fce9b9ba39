"""GPU: the keypoint fit with the floating base (rtg_dof_fit_root_f32: the joint angles and, by the fit_root mask, the
root translation and rotation, fitted in one launch) against the torch restatement of tests/test_pose_fit_host.py --
a normalised root where the rotation is fitted, torch.optim.Adam with three parameter groups, the renormalisation
after each step -- on the CPU in float64 and float32.

The criterion is the project's own, per tensor: E(x) = max|x - x64| / max|x64|, and E(gpu) <= 8 max(E(restatement
f32), 2^-24).  The root's Adam step is checked on its own against the update formula in float64 on the GPU's own
gradient, and everything that has to hold bit for bit (fit_root = 0 against rtg_dof_fit_f32, given blocks, chained
launches, batch and tile independence, repeatability, aliasing, autograd, a bad frame staying in its rows) is checked
bit for bit."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_dof_fit import SKELS, Skel, bits, check_criterion, fit, inputs, skel
from test_pose_fit_host import (B1, B2, EPS, FIT_ROT, FIT_T, LR, recipe, ref_pose_fit, ref_pose_loss,
                                ref_pose_loss_grad)

pytestmark = pytest.mark.gpu

FACTOR = 8.0
FLOOR = 2.0 ** -24
U = 2.0 ** -24   # the relative half-ulp of float32
MASKS = (0, FIT_T, FIT_ROT, FIT_T | FIT_ROT)
OUTS = ("dof", "rr", "rt", "loss", "grad", "groot")


# ------------------------------------------------------------------ the launch, straight through the C ABI
def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def pfit(s, tgt, w, rr, rt, dof, clip, mask, iters=0, lr=LR, lr_t=LR, lr_q=LR, betas=(B1, B2), eps=EPS, step0=0, m=None,
         v=None, rs=None, alias=False, want=OUTS, status=False):
    """rtg_dof_fit_root_f32 on host arrays -> dict of host arrays (dof, rr, rt, loss, grad, groot, m, v, rs)."""
    from rtg import _lib
    from rtg.runtime import ptr
    B, n = tgt.shape[0], s.J - 1
    d_in, rr_in, rt_in = _dev(dof), _dev(rr), _dev(rt)
    bufs = dict(tp=_dev(tgt), w=_dev(w), m=_dev(m), v=_dev(v), rs=_dev(rs))
    new = lambda *shape: torch.full(shape, 7.0, device="cuda")
    out = {"dof": None if "dof" not in want else d_in if alias else new(B, n),
           "rr": None if "rr" not in want else rr_in if alias else new(B, 4),
           "rt": None if "rt" not in want else rt_in if alias else new(B, 3),
           "loss": new(B) if "loss" in want else None, "grad": new(B, n) if "grad" in want else None,
           "groot": new(B, 7) if "groot" in want else None}
    rc = _lib.lib().rtg_dof_fit_root_f32(
        s.model.handle, ptr(bufs["tp"]), ptr(bufs["w"]), ptr(rr_in), ptr(rt_in), ptr(d_in), B, int(clip), mask, iters,
        lr, lr_t, lr_q, betas[0], betas[1], eps, step0, ptr(bufs["m"]), ptr(bufs["v"]), ptr(bufs["rs"]),
        *(ptr(out[k]) for k in OUTS), None)
    if status:
        return rc, _lib.lib().rtg_last_error()
    assert rc == 0, _lib.lib().rtg_last_error()
    torch.cuda.synchronize()
    res = {k: _np(x) for k, x in out.items()}
    res.update(m=_np(bufs["m"]), v=_np(bufs["v"]), rs=_np(bufs["rs"]))
    return res


def assert_same_bits(a, b, what="", keys=None):
    for k in keys or a:
        if a[k] is not None:
            np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=f"{what} {k}")


def random_state(x, seed, scale=1.0):
    """Moments as after some steps: v0 >= m0^2."""
    rng = np.random.default_rng(seed)
    B = x["dof"].shape[0]
    m0 = rng.normal(0, scale, x["dof"].shape).astype(np.float32)
    rm = rng.normal(0, scale, (B, 7))
    mom = lambda m, k: (m.astype(np.float64) ** 2 * rng.uniform(1.0, 3.0, m.shape) + k).astype(np.float32)
    rs = np.concatenate([rm, mom(rm, 1e-3 * scale * scale)], axis=-1).astype(np.float32)
    return dict(m=m0, v=mom(m0, 1e-3 * scale * scale), rs=rs)


# ------------------------------------------------------------------ 1. evaluate
@functools.lru_cache(maxsize=None)
def _evaluate_reference(name, clip, normalised):
    s = skel(name)
    x = inputs(s, max(s.batches()), clip, 9 * s.J + clip)
    mask = FIT_ROT if normalised else 0
    args = (s, x["dof"], x["rr"], x["rt"], x["tgt"], x["w"], clip)
    return x, ref_pose_loss_grad(*args, torch.float64, mask), ref_pose_loss_grad(*args, torch.float32, mask)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", SKELS)
def test_evaluate_against_autograd(gpu, name, clip):
    """iters = 0: loss, grad and grad_root of all four masks against float64 autograd of the restatement (the root
    rotation normalised where it is fitted, as given where not; root norms 0.5-2, a third of the weights 0)."""
    s = skel(name)
    for mask in MASKS:
        x, (l64, g64, r64), (l32, g32, r32) = _evaluate_reference(name, clip, bool(mask & FIT_ROT))
        n = np.linalg.norm(x["rr"], axis=-1)
        assert n.min() < 0.8 and n.max() > 1.3
        zero_dof = s.strict_subtree_weight(x["w"]) == 0
        full = None
        for B in sorted(s.batches(), reverse=True):
            r = pfit(s, x["tgt"][:B], x["w"], x["rr"][:B], x["rt"][:B], x["dof"][:B], clip, mask)
            assert r["loss"].shape == (B,) and r["grad"].shape == (B, s.J - 1) and r["groot"].shape == (B, 7)
            what = f"{name} clip={clip} mask={mask} B={B}"
            check_criterion(f"{what} loss", r["loss"], l32[:B], l64[:B])
            check_criterion(f"{what} grad", r["grad"], g32[:B], g64[:B])
            check_criterion(f"{what} grad_t", r["groot"][:, :3], r32[:B, :3], r64[:B, :3])
            check_criterion(f"{what} grad_q", r["groot"][:, 3:], r32[:B, 3:], r64[:B, 3:])
            for k, a in (("dof", x["dof"]), ("rr", x["rr"]), ("rt", x["rt"])):   # iters = 0: the inputs' bits
                np.testing.assert_array_equal(bits(r[k]), bits(a[:B]), err_msg=f"{what} {k}")
            assert (r["grad"][:, zero_dof] == 0).all()                           # exactly +-0, not noise
            if full is None:
                full = r
            assert_same_bits(r, {k: a[:B] for k, a in full.items() if a is not None}, what,   # the leading frames
                             ("loss", "grad", "groot"))
            if s.J == 1:   # dL/dt = 2 w_0 (t - T_0): a subtraction and a product, two roundings; dL/dq: nothing moves
                want = 2.0 * x["w"][0].astype(np.float64) * (x["rt"][:B].astype(np.float64) - x["tgt"][:B, 0])
                assert (np.abs(r["groot"][:, :3] - want) <= 2 * U * np.abs(want)).all() and np.abs(want).max() > 0.1
                assert (r["groot"][:, 3:] == 0).all()


@pytest.mark.parametrize("name", ["hu33", "chain64", "two"])
def test_the_fitted_rotation_gradient_is_tangent(gpu, name):
    """|grad_q . q^| / |grad_q| per frame: at most 8 times the float32 restatement's own largest value."""
    s = skel(name)
    for mask in (FIT_ROT, FIT_T | FIT_ROT):
        x, _, (_, _, r32) = _evaluate_reference(name, True, True)
        r = pfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask)
        qh = x["rr"].astype(np.float64) / np.linalg.norm(x["rr"].astype(np.float64), axis=-1, keepdims=True)
        off = lambda g: np.abs((g.astype(np.float64)[:, 3:] * qh).sum(-1)) / np.linalg.norm(g.astype(np.float64)[:, 3:], axis=-1)
        got, ref = off(r["groot"]).max(), off(r32).max()
        print(f"{name} mask={mask}: max |grad_q . q^| / |grad_q| GPU {got:.3e}, restatement f32 {ref:.3e}")
        assert np.linalg.norm(r["groot"][:, 3:], axis=-1).min() > 0
        assert got <= FACTOR * max(ref, FLOOR)


def test_unsupported_and_rejected(gpu):
    rng = np.random.default_rng(65)
    big = Skel("chain65", list(range(-1, 64)), rng.normal(0, 0.3, (65, 3)).astype(np.float32),
               rng.integers(0, 3, 64).astype(np.int32), np.full(64, -1.0, np.float32), np.full(64, 1.0, np.float32))
    x = inputs(big, 3, False, 1)
    rc, msg = pfit(big, x["tgt"], None, x["rr"], x["rt"], x["dof"], False, 3, status=True)
    assert rc == 4 and b"1..64 joints" in msg                                    # RTG_ERR_UNSUPPORTED
    s = skel("two")
    x = inputs(s, 3, False, 2)
    rc, _ = pfit(s, x["tgt"][:0], None, x["rr"][:0], x["rt"][:0], x["dof"][:0], False, 3, status=True)
    assert rc == 0                                                               # B == 0: a no-op


# ------------------------------------------------------------------ 2. outcome
@pytest.fixture(scope="module")
def outcome():
    """The pinned recipe of tests/test_pose_fit_host.py; the reference loop in float64 and float32 after 8 and 64
    steps: (loss, dof, q, t) each."""
    s, x = recipe()
    hu = skel("hu33")
    assert np.array_equal(hu.par, s.par)
    args = (s, x["start"], x["q0"], x["t0"], x["tgt"], x["w"], True)
    ref = {dt: ref_pose_fit(*args, dt, FIT_T | FIT_ROT, 64, record=(8, 64)) for dt in (torch.float64, torch.float32)}
    return hu, x, ref


@pytest.mark.parametrize("iters", [8, 64])
def test_outcome_against_the_torch_loop(gpu, outcome, iters):
    s, x, ref = outcome
    (l64, _, q64, t64), (l32, _, q32, t32) = ref[torch.float64][iters], ref[torch.float32][iters]
    args = (x["tgt"], None, x["q0"], x["t0"], x["start"], True)
    r = pfit(s, *args, FIT_T | FIT_ROT, iters=iters)
    pinned = pfit(s, *args, 0, iters=iters)
    print(f"{iters} steps: mean loss GPU {r['loss'].mean():.4f}, reference {l64.mean():.4f}, GPU angles only "
          f"{pinned['loss'].mean():.4f}; min over frames of angles-only / root-fit {(pinned['loss'] / r['loss']).min():.2f}")
    check_criterion(f"outcome {iters} steps loss", r["loss"], l32, l64)
    check_criterion(f"outcome {iters} steps root_rot", r["rr"], q32, q64)
    check_criterion(f"outcome {iters} steps root_t", r["rt"], t32, t64)
    assert (r["loss"] < pinned["loss"]).all()
    assert np.abs(np.linalg.norm(r["rr"].astype(np.float64), axis=-1) - 1).max() <= 4 * U   # root_rot_out is unit
    np.testing.assert_array_equal(bits(pinned["rr"]), bits(x["q0"]))
    np.testing.assert_array_equal(bits(pinned["rt"]), bits(x["t0"]))


# ------------------------------------------------------------------ 3. the root's Adam step alone
@pytest.mark.parametrize("name", ["hu33", "chain64", "one"])
def test_one_root_adam_step_against_the_formula(gpu, name):
    """iters = 1 from a random state (v0 >= m0^2, five steps taken) with three different step sizes, against the
    update formula in float64 on the GPU's own iters = 0 gradient, the hyper-parameters as the launch receives them
    (float32), the rotation renormalised.  The bound is that of the angles' step in tests/test_gpu_dof_fit.py:
    |delta| <= 8 2^-24 (|old| + |update|) per element; the start rotations are unit, as root_rot_out is."""
    s = skel(name)
    B, step0 = 4 * s.F + 3, 5
    x = inputs(s, B, True, 71)
    q0 = x["rr"].astype(np.float64)
    x["rr"] = (q0 / np.linalg.norm(q0, axis=-1, keepdims=True)).astype(np.float32)
    st = random_state(x, 72)
    if s.J == 1:   # no angle moments: their buffers only say that a state is given
        st["m"] = st["v"] = np.zeros((B, 1), np.float32)
    lrs = dict(lr=LR, lr_t=0.03, lr_q=0.01)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, FIT_T | FIT_ROT)
    g = pfit(s, *args)["groot"].astype(np.float64)
    r = pfit(s, *args, iters=1, step0=step0, **lrs, **st)
    b1, b2, eps = (float(np.float32(h)) for h in (B1, B2, EPS))
    lr7 = np.array([float(np.float32(lrs["lr_t"]))] * 3 + [float(np.float32(lrs["lr_q"]))] * 4)
    t = step0 + 1
    m0, v0 = st["rs"][:, :7].astype(np.float64), st["rs"][:, 7:].astype(np.float64)
    m = b1 * m0 + (1 - b1) * g
    v = b2 * v0 + (1 - b2) * g * g
    upd = lr7 / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    old = np.concatenate([x["rt"], x["rr"]], axis=-1).astype(np.float64)
    new = old - upd
    new[:, 3:] /= np.linalg.norm(new[:, 3:], axis=-1, keepdims=True)
    got = np.concatenate([r["rt"], r["rr"]], axis=-1)
    excess = np.abs(got - new) / (U * (np.abs(old) + np.abs(upd)))
    print(f"{name}: root Adam step, max |delta| / (2^-24 (|old| + |update|)): t {excess[:, :3].max():.2f}, "
          f"q {excess[:, 3:].max():.2f} (bound 8)")
    assert excess.max() <= 8
    assert (np.abs(r["rs"][:, :7] - m) <= 2 * U * (np.abs(b1 * m0) + np.abs((1 - b1) * g))).all()
    assert (np.abs(r["rs"][:, 7:] - v) <= 2 * U * v).all()
    assert np.abs(upd[:, :3]).max() > 1e-3                                       # the step is not a no-op
    if s.J > 1:
        assert np.abs(upd[:, 3:]).max() > 1e-3


def test_zero_weights_leave_the_bits(gpu):
    s = skel("hu33")
    B = 4 * s.F + 3
    x = inputs(s, B, True, 31)
    x["rt"][0] = [-0.0, 0.0, 1e-42]
    w0 = np.zeros(s.J, np.float32)
    for kw in (random_state(x, 32, 0.0), dict()):                                # explicit zero state, and none
        r = pfit(s, x["tgt"], w0, x["rr"], x["rt"], x["dof"], True, 3, iters=3, **kw)
        np.testing.assert_array_equal(bits(r["rt"]), bits(x["rt"]))              # a fitted t keeps its bits
        np.testing.assert_array_equal(bits(r["dof"]), bits(x["dof"]))
        assert (r["loss"] == 0).all() and (r["grad"] == 0).all() and (r["groot"] == 0).all()
    # with weights: the DOFs that carry none stay, the root moves
    r = pfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, iters=3)
    still = s.strict_subtree_weight(x["w"]) == 0
    assert still.any() and not still.all()
    np.testing.assert_array_equal(bits(r["dof"][:, still]), bits(x["dof"][:, still]))
    assert (bits(r["rt"]) != bits(x["rt"])).all() and (bits(r["rr"]) != bits(x["rr"])).any(axis=-1).all()


# ------------------------------------------------------------------ 4. bit for bit
@pytest.mark.parametrize("name", ["hu33", "vtrdyn59", "tree37"])
def test_fit_root_0_is_rtg_dof_fit(gpu, name):
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 41)
    st = random_state(x, 42, 0.1)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    for iters in (0, 8):
        old = fit(s, *args, iters=iters, step0=3, m=st["m"], v=st["v"])
        r = pfit(s, *args, 0, iters=iters, step0=3, lr_t=0.5, lr_q=0.5, **st)
        assert_same_bits(old, r, f"{name} iters={iters}")                        # dof, loss, grad, m, v
        np.testing.assert_array_equal(bits(r["rs"]), bits(st["rs"]))             # root_state: untouched
        np.testing.assert_array_equal(bits(r["rr"]), bits(x["rr"]))
        np.testing.assert_array_equal(bits(r["rt"]), bits(x["rt"]))
    old, r = fit(s, *args, iters=4), pfit(s, *args, 0, iters=4)                  # and without a state
    assert_same_bits({k: old[k] for k in ("dof", "loss", "grad")}, r, f"{name} no state")


@pytest.mark.parametrize("name", ["hu33", "vtrdyn59"])
def test_self_consistency(gpu, name):
    s = skel(name)
    F = s.F
    B = 4 * F + 3
    x = inputs(s, B, True, 43)
    st = random_state(x, 44, 0.1)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    kw = dict(iters=8, step0=3, lr_t=0.01, lr_q=0.03)
    for mask in (FIT_T, FIT_ROT, FIT_T | FIT_ROT):
        one = pfit(s, *args, mask, **kw, **st)
        assert all(np.isfinite(a).all() for a in one.values())
        # a given block's rows come back as they went in, its moments too
        if not mask & FIT_ROT:
            np.testing.assert_array_equal(bits(one["rr"]), bits(x["rr"]))
            np.testing.assert_array_equal(bits(one["rs"][:, [3, 4, 5, 6, 10, 11, 12, 13]]),
                                          bits(st["rs"][:, [3, 4, 5, 6, 10, 11, 12, 13]]))
        if not mask & FIT_T:
            np.testing.assert_array_equal(bits(one["rt"]), bits(x["rt"]))
            np.testing.assert_array_equal(bits(one["rs"][:, [0, 1, 2, 7, 8, 9]]), bits(st["rs"][:, [0, 1, 2, 7, 8, 9]]))
        # two identical launches
        assert_same_bits(one, pfit(s, *args, mask, **kw, **st), f"repeat mask={mask}")
        # eight launches of one step, carrying (dof, root, m, v, root_state, step)
        c = dict(dof=x["dof"], rr=x["rr"], rt=x["rt"], **st)
        for k in range(8):
            c = pfit(s, x["tgt"], x["w"], c["rr"], c["rt"], c["dof"], True, mask, **dict(kw, iters=1, step0=3 + k),
                     m=c["m"], v=c["v"], rs=c["rs"])
        assert_same_bits(one, c, f"chained mask={mask}")
        # dof_out, root_rot_out, root_t_out aliasing the inputs
        assert_same_bits(one, pfit(s, *args, mask, **kw, **st, alias=True), f"alias mask={mask}")
    # a frame of the large launch is that frame run alone (mask 3, from the loop's last round)
    for f in (0, F - 1, 2 * F + 1, B - 1):
        sl = slice(f, f + 1)
        alone = pfit(s, x["tgt"][sl], x["w"], x["rr"][sl], x["rt"][sl], x["dof"][sl], True, 3, **kw,
                     **{k: a[sl] for k, a in st.items()})
        assert_same_bits(alone, {k: a[sl] for k, a in one.items()}, f"frame {f}")
    # no state given: starts at zero, as an explicit zero state does; outputs are optional one by one
    a, b = pfit(s, *args, 3, iters=4), pfit(s, *args, 3, iters=4, **random_state(x, 45, 0.0))
    assert a["m"] is None and a["v"] is None and a["rs"] is None
    assert_same_bits({k: a[k] for k in OUTS}, b, "no state")
    for k in OUTS:
        assert_same_bits(pfit(s, *args, 3, iters=4, want=(k,)), {k: a[k]}, f"only {k}", (k,))


def test_python_entry_points(gpu):
    from rtg import ops
    from robot_kinematics_model import RobotZeroPose
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    s = skel("hu33")
    B = 19
    x = inputs(s, B, True, 51)
    # ops.pose_loss: the evaluate-only launch under autograd, in all three inputs
    for normalise, mask in ((True, FIT_ROT), (False, 0)):
        r = pfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask)
        a, q, t = (_dev(x[k]).requires_grad_(True) for k in ("dof", "rr", "rt"))
        loss = ops.pose_loss(s.model, a, q, t, x["tgt"], weight=x["w"], clip=True, normalize_root=normalise)
        assert loss.shape == (B,) and loss.grad_fn is not None
        np.testing.assert_array_equal(bits(_np(loss)), bits(r["loss"]))
        loss.sum().backward()
        np.testing.assert_array_equal(bits(_np(a.grad)), bits(r["grad"]))
        np.testing.assert_array_equal(bits(_np(t.grad)), bits(r["groot"][:, :3]))
        np.testing.assert_array_equal(bits(_np(q.grad)), bits(r["groot"][:, 3:]))
        with torch.no_grad():
            plain = ops.pose_loss(s.model, a, q, t, x["tgt"], weight=x["w"], clip=True, normalize_root=normalise)
        assert plain.grad_fn is None and torch.equal(plain, loss.detach())
    q1 = _dev(x["rr"][:, None]).requires_grad_(True)                             # the reference's (L, 1, 4) rotation
    c = torch.linspace(-2.0, 3.0, B, device="cuda")
    (ops.pose_loss(s.model, x["dof"], q1, x["rt"], x["tgt"], weight=x["w"], clip=True, normalize_root=False) * c).sum().backward()
    assert q1.grad.shape == (B, 1, 4) and torch.equal(q1.grad[:, 0], _dev(r["groot"][:, 3:]) * c[:, None])
    # ops.pose_fit: the launch, its named tuple, and the chain 4 + 4 = 8
    kw = dict(weight=x["w"], lr=LR, lr_root_t=0.01, clip=True)
    r8 = pfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, iters=8, lr_t=0.01)
    p8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, return_grad=True, **kw)
    for k, a in (("dof", p8.dof), ("rr", p8.root_rot), ("rt", p8.root_t), ("loss", p8.loss), ("grad", p8.grad),
                 ("groot", p8.grad_root)):
        np.testing.assert_array_equal(bits(_np(a)), bits(r8[k]), err_msg=k)
    p4 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, **kw)
    q8 = ops.pose_fit(s.model, x["tgt"], p4.root_rot, p4.root_t, p4.dof, iters=4, state=p4.state, **kw)
    assert p4.state[3] == 4 and q8.state[3] == p8.state[3] == 8 and p4.state[2].shape == (B, 14)
    assert all(torch.equal(a, b) for a, b in zip(q8[:4] + q8.state[:3], p8[:4] + p8.state[:3]))
    only_t = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, fit_root_rot=False, **kw)
    np.testing.assert_array_equal(bits(_np(only_t.root_rot)), bits(x["rr"]))
    # the drop-in: the reference's shapes, results on the inputs' device
    hu = HuForwardModel(RobotZeroPose.from_asset("hu").skeleton_tree)
    tgt, rt, rr = torch.from_numpy(x["tgt"]), torch.from_numpy(x["rt"]), torch.from_numpy(x["rr"][:, None])
    ang, t, q, loss, state, grad, groot = hu.fit_pose(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), iters=8, lr=LR,
                                                      return_grad=True)
    assert ang.shape == (B, 32, 1) and t.shape == (B, 3) and q.shape == (B, 1, 4) and loss.shape == (B,)
    assert grad.shape == (B, 32, 1) and groot.shape == (B, 7) and state[3] == 8
    assert all(a.device.type == "cpu" for a in (ang, t, q, loss, grad, groot))
    want = ops.pose_fit(hu._model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, lr=LR, clip=True)
    assert torch.equal(ang[..., 0], want.dof.cpu()) and torch.equal(q[:, 0], want.root_rot.cpu())
    assert torch.equal(t, want.root_t.cpu()) and torch.equal(loss, want.loss.cpu())
    ang0 = hu.fit_pose(tgt, rt, rr, iters=0)[0]                                  # default start: zeros
    assert ang0.shape == (B, 32, 1) and not ang0.any()


# ------------------------------------------------------------------ 5. a bad frame stays its own
def test_a_bad_frame_stays_its_own(gpu):
    s = skel("hu33")
    B = 3 * s.F
    f = B // 2
    x = inputs(s, B, True, 61)
    args = lambda y: (y["tgt"], y["w"], y["rr"], y["rt"], y["dof"], True, FIT_T | FIT_ROT)
    clean = pfit(s, *args(x), iters=3)
    clean0 = pfit(s, *args(x))
    assert all(np.isfinite(a).all() for a in clean.values() if a is not None)
    ok = np.arange(B) != f

    def spoil(which):
        y = {k: a.copy() for k, a in x.items()}
        if "target" in which:
            y["tgt"][f, np.flatnonzero(x["w"])[3], 1] = np.nan
        if "angle" in which:
            y["dof"][f, 2] = np.inf
        if "rotation" in which:
            y["rr"][f] = 0.0
        if "translation" in which:
            y["rt"][f, 1] = np.nan
        return y
    for which in (("target",), ("angle",), ("rotation",), ("translation",), ("target", "angle", "rotation", "translation")):
        y = spoil(which)
        bad = pfit(s, *args(y), iters=3)
        for k in OUTS:
            np.testing.assert_array_equal(bits(bad[k][ok]), bits(clean[k][ok]), err_msg=f"{which} {k}")
        bad0 = pfit(s, *args(y))
        for k in ("loss", "grad", "groot"):
            np.testing.assert_array_equal(bits(bad0[k][ok]), bits(clean0[k][ok]), err_msg=f"{which} {k}")
        sl = slice(f, f + 1)
        with np.errstate(all="ignore"), torch.no_grad():
            want = ref_pose_loss(s, y["dof"][sl], y["rr"][sl], y["rt"][sl], y["tgt"][sl], y["w"], True, torch.float32,
                                 FIT_ROT).numpy()
        assert np.isnan(bad0["loss"][f]) == np.isnan(want[0]), which
        if not np.isnan(want[0]):   # a zero root rotation: every joint at the root translation, a finite loss -- a
            # sum of 99 non-negative float32 terms, each a few roundings, in both: well within 1e-5 relative
            assert abs(bad0["loss"][f] - want[0]) <= 1e-5 * abs(want[0])

"""GPU: the pose fit with per-frame keypoint weights and a robust keypoint loss (rtg_dof_fit_robust_f32: the keep-apart
launch with the keypoint term sum_j [fw_fj != 0] weight[j] fw_fj rho(|P_j - T_fj|^2), rho the pseudo-Huber kernel of
scale robust_scale or the square) against the torch restatement of tests/test_robust_fit_host.py on the CPU in float64
and float32.

The criterion is the project's own, per tensor (tests/test_gpu_dof_fit.py check_criterion): E(x) = max|x - x64| /
max|x64|, and E(gpu) <= 8 max(E(restatement f32), 2^-24).  One Adam step is checked on its own against the update
formula, and everything the header promises bit for bit -- nothing given is the older launches, ones are no weights, a
masked keypoint's target row may hold anything, a fully masked frame, chained launches, batch and tile independence,
repeatability, a bad weight row staying in its frame, aliasing -- is checked bit for bit.  Hostile scales and distances
must land in the float32 restatement's class element by element.  The two outcome recipes of the host file are
replayed through HuForwardModel for their direction only (float32 trajectories diverge: DESIGN 5i)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_apart_fit_host import apart_case, to_ops
from test_gpu_apart_fit import apfit, struct_of
from test_gpu_dof_fit import bits, check_criterion, fit, inputs, skel
from test_gpu_orient_fit import targets, zero_dofs
from test_gpu_pose_fit import MASKS, OUTS, U, _dev, _np, assert_same_bits, pfit, random_state
from test_gpu_prior_fit import _hu_on, link_set, prfit, priors
from test_orient_fit_host import INVALID
from test_pose_fit_host import B1, B2, EPS, FIT_ROT, FIT_T, LR
from test_prior_fit_host import PROJECT
from test_robust_fit_host import (DROPPED, OUTLIER_JOINT, dropout_recipe, frame_weights, link_error, outlier_recipe,
                                  ref_robust_loss_grad)

pytestmark = pytest.mark.gpu

SKELS = ("hu33", "chain64", "tree37", "star61", "two", "one")
STATE = OUTS + ("m", "v", "rs")
DELTA = 0.05


# ------------------------------------------------------------------ the launch, straight through the C ABI
def rbfit(s, tgt, w, rr, rt, dof, clip, mask, ap=None, fw=None, delta=0.0, joints=(), R=None, rw=None, prior=None, pw=None,
          flags=0, iters=0, lr=LR, lr_t=LR, lr_q=LR, betas=(B1, B2), eps=EPS, step0=0, m=None, v=None, rs=None, want=OUTS,
          status=False, alias=False, prior_alias=None):
    """rtg_dof_fit_robust_f32 on host arrays -> dict of host arrays (dof, rr, rt, loss, grad, groot, m, v, rs, fw).
    ap: a spec of the apart host file, None for a NULL struct, or a ready (struct, arrays) pair; fw (B,J) or None.
    alias: dof_out, root_rot_out, root_t_out ARE the inputs; prior_alias "in" / "out": the prior is dof_in's buffer /
    lives in dof_out's."""
    from rtg import _lib
    from rtg.runtime import ptr
    B, n, K = tgt.shape[0], s.J - 1, len(joints)
    d_in, rr_in, rt_in = _dev(dof), _dev(rr), _dev(rt)
    bufs = dict(tp=_dev(tgt), w=_dev(w), m=_dev(m), v=_dev(v), rs=_dev(rs), rw=_dev(rw), pw=_dev(pw), fw=_dev(fw))
    R_dev = None if R is None else _dev(np.asarray(R, np.float32).reshape(B, K, 4))
    new = lambda *shape: torch.full(shape, 7.0, device="cuda")
    out = {"dof": None if "dof" not in want else d_in if alias else new(B, n),
           "rr": None if "rr" not in want else rr_in if alias else new(B, 4),
           "rt": None if "rt" not in want else rt_in if alias else new(B, 3),
           "loss": new(B) if "loss" in want else None, "grad": new(B, n) if "grad" in want else None,
           "groot": new(B, 7) if "groot" in want else None}
    if prior_alias == "in":
        p_dev = d_in
    elif prior_alias == "out":
        assert not alias and out["dof"] is not None
        p_dev = out["dof"]
        p_dev.copy_(_dev(prior))
    else:
        p_dev = _dev(prior)
    st, keep = (None, None) if ap is None else ap if isinstance(ap, tuple) else struct_of(ap)
    jarr = (ctypes.c_int32 * max(K, 1))(*[int(j) for j in joints])
    rc = _lib.lib().rtg_dof_fit_robust_f32(
        s.model.handle, ptr(bufs["tp"]), ptr(bufs["w"]), jarr if K else None, ptr(R_dev), ptr(bufs["rw"]), K, ptr(p_dev),
        ptr(bufs["pw"]), flags, ptr(rr_in), ptr(rt_in), ptr(d_in), B, int(clip), mask, iters, lr, lr_t, lr_q, betas[0],
        betas[1], eps, step0, ptr(bufs["m"]), ptr(bufs["v"]), ptr(bufs["rs"]), *(ptr(out[k]) for k in OUTS),
        None if st is None else ctypes.byref(st), ptr(bufs["fw"]), float(delta), None)
    if status:
        return rc, _lib.lib().rtg_last_error()
    assert rc == 0, _lib.lib().rtg_last_error()
    torch.cuda.synchronize()
    res = {k: _np(x) for k, x in out.items()}
    res.update(m=_np(bufs["m"]), v=_np(bufs["v"]), rs=_np(bufs["rs"]))
    if fw is not None:
        np.testing.assert_array_equal(bits(_np(bufs["fw"])), bits(fw))   # an input: its bits stay
    return res


@functools.lru_cache(maxsize=None)
def case(name, clip):
    """(skeleton, inputs of its largest batch with frame weights x["fw"], a keep-apart term)."""
    s = skel(name)
    x = inputs(s, max(s.batches()), clip, 43 * s.J + clip)
    x["fw"] = frame_weights(len(x["dof"]), s.J, 47 * s.J + clip)
    return s, x, apart_case(s, x, clip, 53 * s.J + clip, True, True)


# ------------------------------------------------------------------ 1. evaluate
# (delta, K, keep-apart, prior): every option on and off, with each other option in both states
CONFIGS = ((0.0, 0, True, False), (DELTA, 8, True, True), (DELTA, 0, False, False), (0.0, 8, False, True))


@functools.lru_cache(maxsize=None)
def _evaluate_reference(name, clip, cfg, normalised):
    delta, K, apart, prior = cfg
    s, x, ap = case(name, clip)
    joints = link_set(s, x["w"], K)
    R, rw = targets(len(x["dof"]), len(joints), 29 * s.J + K)
    p, pw = priors(s, x["dof"], 23 * s.J + clip) if prior and s.J > 1 else (None, None)
    rest = (x["tgt"], x["w"], clip)
    tail = (FIT_ROT if normalised else 0, joints, R, rw, p, pw, ap if apart else None, x["fw"], delta)
    return (joints, R, rw, p, pw, ref_robust_loss_grad(s, x["dof"], x["rr"], x["rt"], *rest, torch.float64, *tail),
            ref_robust_loss_grad(s, x["dof"], x["rr"], x["rt"], *rest, torch.float32, *tail, closed=True))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", SKELS)
def test_evaluate_against_autograd(gpu, name, clip):
    """iters = 0: loss, grad and grad_root against float64 autograd of the restatement -- random frame weights in 0.2-2
    with a third of them 0, the robust scale off and 0.05, K = 0 and 8 links, with and without a keep-apart term and a
    prior, all four masks; the inputs' bits come back, and each of the five batch sizes gives the bits of the
    largest's leading frames.  The criterion is taken per tensor of the case, the largest batch: a smaller batch holds
    the same numbers, and a tensor of one frame is one draw of the restatement's error, not its size (measured: chain64
    with clip, (0, 8, False, True), mask 2, frame 0 alone, grad_q: E(gpu) 2.28e-6 against E(restatement f32) 2.01e-7,
    that frame's being the smallest of the 35 frames' 2.0e-7 .. 1.1e-5 (median 1.2e-6; the launch: median 1.7e-6, max
    1.4e-5) -- and rtg_dof_fit_prior_f32 with that frame's weights folded into ``weight`` returns the same bits)."""
    s, x, ap = case(name, clip)
    st = struct_of(ap)
    for cfg in CONFIGS:
        delta, K, apart, prior = cfg
        for mask in MASKS:
            joints, R, rw, p, pw, (l64, g64, r64), (l32, g32, r32) = _evaluate_reference(name, clip, cfg, bool(mask & FIT_ROT))
            full = None
            for B in sorted(s.batches(), reverse=True):
                r = rbfit(s, x["tgt"][:B], x["w"], x["rr"][:B], x["rt"][:B], x["dof"][:B], clip, mask, st if apart else None,
                          x["fw"][:B], delta, joints, R[:B], rw, None if p is None else p[:B], pw, PROJECT if B % 2 else 0)
                what = f"{name} clip={clip} cfg={cfg} mask={mask} B={B}"
                if full is None:
                    check_criterion(f"{what} loss", r["loss"], l32, l64)
                    check_criterion(f"{what} grad", r["grad"], g32, g64)
                    check_criterion(f"{what} grad_t", r["groot"][:, :3], r32[:, :3], r64[:, :3])
                    check_criterion(f"{what} grad_q", r["groot"][:, 3:], r32[:, 3:], r64[:, 3:])
                for k, a in (("dof", x["dof"]), ("rr", x["rr"]), ("rt", x["rt"])):   # iters = 0: the inputs' bits
                    np.testing.assert_array_equal(bits(r[k]), bits(a[:B]), err_msg=f"{what} {k}")
                if full is None:
                    full = r
                assert_same_bits(r, {k: a[:B] for k, a in full.items() if a is not None}, what, ("loss", "grad", "groot"))


# ------------------------------------------------------------------ 2. one Adam step against the formula
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_one_adam_step_against_the_formula(gpu, name):
    """iters = 1 from a random state (v0 >= m0^2, five steps taken) against the update formula in float64 on the GPU's
    own iters = 0 gradient (frame weights, the robust kernel and the keep-apart term in it), the hyper-parameters as the
    launch receives them (float32): |delta| <= 8 2^-24 (|old| + |update|) per element."""
    s, x, ap = case(name, True)
    step0 = 5
    st = random_state(x, 83)
    args = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, FIT_T | FIT_ROT, ap, x["fw"], DELTA)
    e = rbfit(*args)
    r = rbfit(*args, iters=1, step0=step0, **st)
    b1, b2, eps, lr = (float(np.float32(h)) for h in (B1, B2, EPS, LR))
    t = step0 + 1
    g, m0, v0, old = (a.astype(np.float64) for a in (e["grad"], st["m"], st["v"], x["dof"]))
    m = b1 * m0 + (1 - b1) * g
    v = b2 * v0 + (1 - b2) * g * g
    upd = lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    assert (np.abs(r["m"] - m) <= 2 * U * (np.abs(b1 * m0) + np.abs((1 - b1) * g))).all()
    assert (np.abs(r["v"] - v) <= 2 * U * v).all()
    assert np.abs(upd).max() > 1e-3
    excess = np.abs(r["dof"] - (old - upd)) / (U * (np.abs(old) + np.abs(upd)))
    print(f"{name}: Adam step, max |delta| / (2^-24 (|old| + |update|)) {excess.max():.2f} (bound 8)")
    assert excess.max() <= 8
    # the root's blocks: the same formula on grad_root
    gr, rs0 = e["groot"].astype(np.float64), st["rs"].astype(np.float64)
    mt = b1 * rs0[:, :3] + (1 - b1) * gr[:, :3]
    vt = b2 * rs0[:, 7:10] + (1 - b2) * gr[:, :3] ** 2
    updt = lr / (1 - b1 ** t) * mt / (np.sqrt(vt) / np.sqrt(1 - b2 ** t) + eps)
    oldt = x["rt"].astype(np.float64)
    assert (np.abs(r["rt"] - (oldt - updt)) <= 8 * U * (np.abs(oldt) + np.abs(updt))).all()


# ------------------------------------------------------------------ 3. (a), (b): nothing given, and ones
@pytest.mark.parametrize("name", ["hu33", "chain64", "one"])
def test_nothing_given_is_the_older_launches_and_ones_are_no_weights(gpu, name):
    """(a) frame_weight NULL with robust_scale 0: rtg_dof_fit_apart_f32's bits with a term, rtg_dof_fit_prior_f32's
    without one, rtg_dof_fit_root_f32's with nothing else, rtg_dof_fit_f32's with the root given -- every output and
    state row, iters 0 and 4.  (b) all ones: with the scale 0 the same outputs as numbers, with it on the bits of NULL."""
    s, x, ap = case(name, True)
    B = len(x["dof"])
    st = random_state(x, 92, 0.1)
    if s.J == 1:
        st["m"] = st["v"] = np.zeros((B, 1), np.float32)
    p, pw = priors(s, x["dof"], 93)
    ones = np.ones((B, s.J), np.float32)
    a = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    for K in (0, 8):
        joints = link_set(s, x["w"], K)
        R, rw = targets(B, len(joints), 95)
        for mask in (0, 3):
            for iters in (0, 4):
                kw = dict(joints=joints, R=R, rw=rw, prior=p, pw=pw, flags=PROJECT, iters=iters, step0=3, lr_t=0.01, **st)
                what = f"{name} K={K} mask={mask} iters={iters}"
                for term in (ap, None):
                    want = apfit(*a, mask, term, **kw)
                    assert_same_bits(want, rbfit(*a, mask, term, **kw), f"{what} NULL, 0")
                    got = rbfit(*a, mask, term, ones, **kw)
                    for k in STATE:
                        assert np.array_equal(want[k], got[k]), f"{what} ones, 0: {k}"
                    assert_same_bits(rbfit(*a, mask, term, None, DELTA, **kw), rbfit(*a, mask, term, ones, DELTA, **kw),
                                     f"{what} ones against NULL, delta")
                assert_same_bits(prfit(*a, mask, **kw), rbfit(*a, mask, None, **kw), f"{what} prior launch")
    for mask in (0, 3):
        kw = dict(iters=4, step0=3, lr_t=0.01, **st)
        assert_same_bits(pfit(*a, mask, **kw), rbfit(*a, mask, **kw), f"{name} mask={mask} root launch")
    if s.J > 1:
        old = fit(*a, iters=4, step0=3, m=st["m"], v=st["v"])
        new = rbfit(*a, 0, iters=4, step0=3, **st)
        assert_same_bits(old, new, f"{name} rtg_dof_fit_f32", ("dof", "loss", "grad", "m", "v"))


# ------------------------------------------------------------------ 4. (c): masked keypoints
@pytest.mark.parametrize("delta", [0.0, DELTA])
@pytest.mark.parametrize("name", ["hu33", "chain64", "one"])
def test_a_masked_keypoint_contributes_nothing_whatever_its_row_holds(gpu, name, delta):
    """Masked target rows of NaN, +-inf, 1e30 and subnormals: every output is finite and has the bits of the run with
    those rows replaced by zeros, at iters 0 and after 8 steps, with and without the keep-apart term."""
    s, x, ap = case(name, True)
    off = x["fw"] == 0
    assert off.any() and (~off).any()
    fill = np.resize(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-42, -1e-45], np.float32), int(off.sum()))
    bad, zero = x["tgt"].copy(), x["tgt"].copy()
    bad[off] = fill[:, None]
    zero[off] = 0.0
    st = random_state(x, 101, 0.1)
    if s.J == 1:
        st["m"] = st["v"] = np.zeros((len(x["dof"]), 1), np.float32)
    for term in (ap, None):
        for iters in (0, 8):
            a = lambda tgt: rbfit(s, tgt, x["w"], x["rr"], x["rt"], x["dof"], True, 3, term, x["fw"], delta, iters=iters, **st)
            got, want = a(bad), a(zero)
            assert all(np.isfinite(v).all() for v in got.values() if v is not None), (name, iters)
            assert_same_bits(got, want, f"{name} delta={delta} iters={iters}")


@pytest.mark.parametrize("delta", [0.0, DELTA])
def test_masked_frames_and_subtrees_keep_their_bits(gpu, delta):
    """Hu, no other term.  A frame with every keypoint masked: a loss of exactly 0, gradients of +-0, and after 8 steps
    from a zero state the bits of its angles and of its fitted root, whatever its target rows hold.  A frame with the
    keypoints of one arm masked: the DOFs whose strict subtree then carries no weight get +-0 in that frame only and
    keep their bits there.  A masked root row leaves a fitted translation's bits when nothing else pulls: every other
    keypoint given weight 0 by ``weight``."""
    s = skel("hu33")
    B = 2 * s.F + 3
    x = inputs(s, B, True, 111)
    x["w"][:] = np.random.default_rng(112).uniform(0.2, 2.0, s.J).astype(np.float32)   # every keypoint weighted
    fw = np.ones((B, s.J), np.float32)
    dead = [s.F - 1, s.F]          # fully masked, on both sides of a tile boundary
    fw[dead] = 0.0
    arm = [j for j in range(s.J) if j >= 14 and j <= 22]
    part = [3, s.F + 2]
    for f in part:
        fw[f, arm] = 0.0
    tgt = x["tgt"].copy()
    tgt[dead] = np.nan
    tgt[part[0], arm] = np.inf
    a = (s, tgt, x["w"], x["rr"], x["rt"], x["dof"], True, 3, None, fw, delta)
    e = rbfit(*a)
    assert (e["loss"][dead] == 0).all() and (e["grad"][dead] == 0).all() and (e["groot"][dead] == 0).all()
    live = np.setdiff1d(np.arange(B), dead)
    assert np.isfinite(e["loss"]).all() and (e["loss"][live] > 0).all()
    r = rbfit(*a, iters=8)
    assert all(np.isfinite(v).all() for v in r.values() if v is not None)
    for k in ("dof", "rt"):   # (the fitted rotation is renormalised after its step: it keeps its direction, not its bits)
        np.testing.assert_array_equal(bits(r[k][dead]), bits(x[k][dead]), err_msg=k)
    for f in part:
        wf = x["w"] * fw[f]
        still = zero_dofs(s, wf, [])
        assert still.sum() >= 3 and not zero_dofs(s, x["w"], []).all()
        assert (e["grad"][f, still] == 0).all() and (np.abs(e["grad"][f, ~still]) > 0).any()
        np.testing.assert_array_equal(bits(r["dof"][f, still]), bits(x["dof"][f, still]))
        other = [g for g in live if g not in part]
        assert (np.abs(e["grad"][other][:, still]) > 0).any()      # in the other frames those DOFs are pulled
    # a masked root row, nothing else pulling on the root: t keeps its bits, with the root's target row NaN
    w0 = np.zeros(s.J, np.float32)
    w0[0] = 1.5
    fw0 = np.ones((B, s.J), np.float32)
    fw0[::2, 0] = 0.0
    tg0 = x["tgt"].copy()
    tg0[::2, 0] = np.nan
    r0 = rbfit(s, tg0, w0, x["rr"], x["rt"], x["dof"], True, FIT_T, None, fw0, delta, iters=8)
    np.testing.assert_array_equal(bits(r0["rt"][::2]), bits(x["rt"][::2]))
    assert (r0["rt"][1::2] != x["rt"][1::2]).any() and np.isfinite(r0["rt"]).all() and (r0["loss"][::2] == 0).all()


# ------------------------------------------------------------------ 5. (d): self-consistency
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_self_consistency(gpu, name):
    """Two launches give the same bits; eight launches of one step that carry the state equal one launch of eight; a
    frame of the large launch is that frame run alone; outputs aliasing the inputs and the prior aliasing dof_in or
    dof_out change nothing."""
    s, x, ap = case(name, True)
    B, F = len(x["dof"]), s.F
    st = random_state(x, 122, 0.1)
    p, pw = priors(s, x["dof"], 123)
    stc = struct_of(ap)
    kw = dict(iters=8, step0=3, lr_t=0.01, lr_q=0.03)
    for K, flags, term, delta in ((0, PROJECT, None, DELTA), (8, 0, stc, DELTA), (0, 0, stc, 0.0)):
        joints = link_set(s, x["w"], K)
        R, rw = targets(B, len(joints), 124)
        ori = (joints, R, rw)
        for mask in (0, 3):
            a = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask, term, x["fw"], delta, *ori, p, pw, flags)
            one = rbfit(*a, **kw, **st)
            what = f"{name} K={K} mask={mask} delta={delta}"
            assert all(np.isfinite(v).all() for v in one.values())
            assert_same_bits(one, rbfit(*a, **kw, **st), f"repeat {what}")
            c = dict(dof=x["dof"], rr=x["rr"], rt=x["rt"], **st)
            for k in range(8):
                c = rbfit(s, x["tgt"], x["w"], c["rr"], c["rt"], c["dof"], True, mask, term, x["fw"], delta, *ori, p, pw, flags,
                          **dict(kw, iters=1, step0=3 + k), m=c["m"], v=c["v"], rs=c["rs"])
            assert_same_bits(one, c, f"chained {what}")
            assert_same_bits(one, rbfit(*a, **kw, **st, alias=True), f"alias {what}")
            assert_same_bits(one, rbfit(*a, **kw, **st, prior_alias="out"), f"prior in dof_out {what}")
        for f in (0, F - 1, 2 * F + 1, B - 1):   # mask 3, from the loop's last round
            sl = slice(f, f + 1)
            alone = rbfit(s, x["tgt"][sl], x["w"], x["rr"][sl], x["rt"][sl], x["dof"][sl], True, 3, term, x["fw"][sl], delta,
                          joints, R[sl], rw, p[sl], pw, flags, **kw, **{k: v[sl] for k, v in st.items()})
            assert_same_bits(alone, {k: v[sl] for k, v in one.items()}, f"frame {f} K={K}")
    a = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, stc, x["fw"], DELTA)
    same = rbfit(*a, prior=x["dof"], pw=pw, iters=4, **st)
    assert_same_bits(same, rbfit(*a, pw=pw, iters=4, **st, prior_alias="in"), "prior = dof_in")
    assert_same_bits(same, rbfit(*a, pw=pw, iters=4, **st, prior_alias="in", alias=True), "prior = dof_in = dof_out")
    # the weights and the kernel are in the steps, not only in the loss
    plain = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, stc, iters=4)["dof"]
    assert not np.array_equal(rbfit(*a[:-2], x["fw"], 0.0, iters=4)["dof"], plain)
    assert not np.array_equal(rbfit(*a[:-2], None, DELTA, iters=4)["dof"], plain)


# ------------------------------------------------------------------ 6. (e): a bad weight row stays its frame's
def test_a_bad_frame_weight_row_stays_its_own(gpu):
    """A NaN or inf frame weight in the last frame of a tile or the first of the next: that frame's loss and gradient
    are non-finite where the float32 restatement's are, every other frame keeps its bits, at iters 0 and after 3 steps.
    Negative frame weights are used as given: the loss is the restatement's."""
    s, x, ap = case("hu33", True)
    B = len(x["dof"])
    stc = struct_of(ap)
    j = int(np.flatnonzero((x["w"] > 0))[-1])
    cls = lambda a: ~np.isfinite(a)   # sums of infinities of both signs are NaN in one order and inf in another
    for delta in (0.0, DELTA):
        args = lambda fw: (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, FIT_T | FIT_ROT, stc, fw, delta)
        clean, clean0 = rbfit(*args(x["fw"]), iters=3), rbfit(*args(x["fw"]))
        assert all(np.isfinite(a).all() for a in clean.values() if a is not None)
        for f in (s.F - 1, s.F):
            ok = np.arange(B) != f
            for val in (np.nan, np.inf, -np.inf):
                fw = x["fw"].copy()
                fw[f, j] = val
                bad, bad0 = rbfit(*args(fw), iters=3), rbfit(*args(fw))
                for k in OUTS:
                    np.testing.assert_array_equal(bits(bad[k][ok]), bits(clean[k][ok]), err_msg=f"{val} {f} {k}")
                for k in ("loss", "grad", "groot"):
                    np.testing.assert_array_equal(bits(bad0[k][ok]), bits(clean0[k][ok]), err_msg=f"{val} {f} {k}")
                sl = slice(f, f + 1)
                l32, g32, r32 = ref_robust_loss_grad(s, x["dof"][sl], x["rr"][sl], x["rt"][sl], x["tgt"][sl], x["w"], True,
                                                     torch.float32, FIT_ROT, [], None, None, None, None, ap, fw[sl], delta,
                                                     closed=True)
                assert not np.isfinite(l32).all()
                np.testing.assert_array_equal(cls(bad0["loss"][sl]), cls(l32), err_msg=f"{val} {f} loss")
                np.testing.assert_array_equal(cls(bad0["grad"][sl]), cls(g32), err_msg=f"{val} {f} grad")
                np.testing.assert_array_equal(cls(bad0["groot"][sl]), cls(r32), err_msg=f"{val} {f} groot")
        neg = x["fw"] * np.where(np.arange(s.J) % 2, -1.0, 1.0).astype(np.float32)
        tail = (FIT_ROT, [], None, None, None, None, ap, neg, delta)
        l64, g64, r64 = ref_robust_loss_grad(s, x["dof"], x["rr"], x["rt"], x["tgt"], x["w"], True, torch.float64, *tail)
        l32, g32, r32 = ref_robust_loss_grad(s, x["dof"], x["rr"], x["rt"], x["tgt"], x["w"], True, torch.float32, *tail, closed=True)
        r = rbfit(*args(neg))
        check_criterion(f"negative weights delta={delta} grad", r["grad"], g32, g64)
        check_criterion(f"negative weights delta={delta} grad_t", r["groot"][:, :3], r32[:, :3], r64[:, :3])
        scale = np.abs(ref_robust_loss_grad(s, x["dof"], x["rr"], x["rt"], x["tgt"], x["w"], True, torch.float64,
                                            *tail[:-2], np.abs(neg), delta)[0])
        # the signed loss cancels: its error is relative to the sum of the terms' magnitudes
        assert (np.abs(r["loss"] - l64) <= 8 * np.maximum(np.abs(l32 - l64), 33 * U * scale)).all()


# ------------------------------------------------------------------ 7. hostile scales and distances
def test_hostile_scales_and_distances(gpu):
    """One-joint model, the translation fitted: the loss is e rho(r^2) and dL/dt = 2 e d / sqrt(1 + r^2 / delta^2) of one
    keypoint, element by element.  delta from 1e-6 to 1e6, residuals from 1e-20 to 1e18 along a fixed direction: each
    element is finite, inf or NaN where the float32 restatement's is, and the finite ones meet the criterion."""
    s = skel("one")
    rs_ = np.array([10.0 ** k for k in range(-20, 19, 2)] + [0.0, 3e-3, 0.05, 0.7], np.float32)
    B = len(rs_)
    u = np.array([0.6, -0.48, 0.64], np.float32)
    rr = np.tile(np.array([0, 0, 0, 1], np.float32), (B, 1))
    rt = np.zeros((B, 3), np.float32)
    tgt = (-rs_[:, None] * u)[:, None, :].astype(np.float32)
    w = np.array([1.5], np.float32)
    fw = np.full((B, 1), 0.75, np.float32)
    dof = np.zeros((B, 0), np.float32)
    cls = lambda a: np.where(np.isnan(a), 2, np.where(np.isinf(a), 1, 0))
    for delta in (1e-6, 1e-3, 0.05, 1.0, 1e3, 1e6):
        r = rbfit(s, tgt, w, rr, rt, dof, False, FIT_T, None, fw, delta)
        tail = (FIT_T, [], None, None, None, None, None, fw, delta)
        with np.errstate(all="ignore"):
            l32, _, r32 = ref_robust_loss_grad(s, dof, rr, rt, tgt, w, False, torch.float32, *tail, closed=True)
            l64, _, r64 = ref_robust_loss_grad(s, dof, rr, rt, tgt, w, False, torch.float64, *tail, closed=True)
        np.testing.assert_array_equal(cls(r["loss"]), cls(l32), err_msg=f"delta={delta} loss")
        np.testing.assert_array_equal(cls(r["groot"][:, :3]), cls(r32[:, :3]), err_msg=f"delta={delta} grad_t")
        assert (cls(l32) == 0).sum() >= B // 2
        # element by element: each is its own sum, so the criterion holds per element, relative to that element
        for got, a32, a64, what in ((r["loss"], l32, l64, "loss"), (r["groot"][:, :3], r32[:, :3], r64[:, :3], "grad_t")):
            fin = (cls(a32) == 0) & np.isfinite(a64)
            e_gpu, e_32 = np.abs(got - a64)[fin], np.abs(a32 - a64)[fin]
            tiny = np.abs(a64[fin]) < 1e-30     # below the normal range the float32 answers are a few subnormal steps
            bound = 8 * np.maximum(e_32, U * np.abs(a64[fin])) + np.where(tiny, 8 * 1.5e-45, 0.0)
            worst = (e_gpu / np.maximum(bound, 1e-300)).max()
            print(f"delta={delta:g} {what}: {fin.sum()} finite elements, worst error / bound {worst:.2f}")
            assert (e_gpu <= bound).all(), (delta, what)


# ------------------------------------------------------------------ 8. what is rejected, and the Python surface
def test_rejected_and_small_models(gpu):
    s = skel("two")
    x = inputs(s, 3, False, 2)
    a = (s, x["tgt"], None, x["rr"], x["rt"], x["dof"], False, 3, None, np.ones((3, 2), np.float32))
    assert np.isfinite(rbfit(*a, 0.05, iters=2)["loss"]).all()
    for bad in (-0.05, float("nan"), float("inf")):
        rc, err = rbfit(*a, bad, status=True)
        assert rc == INVALID and b"robust_scale" in err and b"rtg_dof_fit_robust_f32" in err, err
    rc, err = rbfit(*a, 0.05, flags=2, status=True)
    assert rc == INVALID and b"flags=2 has unknown bits" in err and b"rtg_dof_fit_robust_f32" in err
    rc, _ = rbfit(s, x["tgt"][:0], None, x["rr"][:0], x["rt"][:0], x["dof"][:0], False, 3, None, np.ones((0, 2), np.float32),
                  0.05, status=True)
    assert rc == 0                                                               # B == 0: a no-op
    # a one-joint model: frame_weight applies to the root's row
    one = skel("one")
    y = inputs(one, 5, False, 3)
    fw = np.array([[1.0], [0.0], [2.0], [0.0], [0.5]], np.float32)
    tg = y["tgt"].copy()
    tg[fw[:, 0] == 0] = np.nan
    r = rbfit(one, tg, y["w"] * 0 + 1, y["rr"], y["rt"], y["dof"], False, FIT_T, None, fw, 0.0)
    d = y["rt"].astype(np.float64) - y["tgt"][:, 0]
    want = fw[:, 0] * (d ** 2).sum(-1)
    assert (r["loss"][[1, 3]] == 0).all() and (r["groot"][[1, 3]] == 0).all()
    assert np.allclose(r["loss"], want, rtol=1e-5) and np.allclose(r["groot"][:, :3], 2 * fw * d, rtol=1e-5, atol=1e-6)


def test_python_entry_points(gpu):
    from rtg import ops
    s, x, ap = case("hu33", True)
    B = 19
    x = {k: (v[:B] if k != "w" else v) for k, v in x.items()}
    p, pw = priors(s, x["dof"], 162)
    joints = [20, 32]
    R, rw = targets(B, 2, 163)
    spec_ = to_ops(s, ap)
    ap = dict(ap, mask=spec_.floor_mask)
    o = dict(prior=p, prior_weight=pw, apart=spec_, frame_weight=x["fw"], robust_scale=DELTA)
    # ops.pose_loss / keypoint_loss: the evaluate-only launch under autograd; a cotangent scales row by row
    for ori, okw in (((), {}), ((joints, R, rw), dict(rot_joints=joints, target_rot=R, rot_weight=rw))):
        for normalise, mask in ((True, FIT_ROT), (False, 0)):
            r = rbfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask, ap, x["fw"], DELTA,
                      *(ori or ((), None, None)), p, pw)
            a, q, t = (_dev(x[k]).requires_grad_(True) for k in ("dof", "rr", "rt"))
            c = torch.linspace(-2.0, 3.0, B, device="cuda")
            loss = ops.pose_loss(s.model, a, q, t, x["tgt"], weight=x["w"], clip=True, normalize_root=normalise, **o, **okw)
            assert loss.shape == (B,) and loss.grad_fn is not None
            np.testing.assert_array_equal(bits(_np(loss)), bits(r["loss"]))
            loss.sum().backward()
            np.testing.assert_array_equal(bits(_np(a.grad)), bits(r["grad"]))
            np.testing.assert_array_equal(bits(_np(t.grad)), bits(r["groot"][:, :3]))
            np.testing.assert_array_equal(bits(_np(q.grad)), bits(r["groot"][:, 3:]))
            with torch.no_grad():
                plain = ops.pose_loss(s.model, a, q, t, x["tgt"], weight=x["w"], clip=True, normalize_root=normalise, **o, **okw)
            assert plain.grad_fn is None and torch.equal(plain, loss.detach())
            a2 = _dev(x["dof"]).requires_grad_(True)
            (ops.pose_loss(s.model, a2, x["rr"], x["rt"], x["tgt"], weight=x["w"], clip=True, normalize_root=normalise, **o,
                           **okw) * c).sum().backward()
            assert torch.equal(a2.grad, _dev(r["grad"]) * c[:, None])
        g0 = rbfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, ap, x["fw"], DELTA, *(ori or ((), None, None)), p, pw)
        a = _dev(x["dof"]).requires_grad_(True)
        kl = ops.keypoint_loss(s.model, a, x["tgt"], x["rr"], x["rt"], weight=x["w"], clip=True, **o, **okw)
        kl.sum().backward()
        np.testing.assert_array_equal(bits(_np(kl)), bits(g0["loss"]))
        np.testing.assert_array_equal(bits(_np(a.grad)), bits(g0["grad"]))
    # each keyword alone (no prior, no links, no spheres); a bool mask is a weight of 0 / 1
    for kw, fw, delta in ((dict(frame_weight=x["fw"]), x["fw"], 0.0), (dict(robust_scale=DELTA), None, DELTA),
                          (dict(frame_weight=x["fw"] > 0), (x["fw"] > 0).astype(np.float32), 0.0)):
        r = rbfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, FIT_ROT, None, fw, delta)
        a = _dev(x["dof"]).requires_grad_(True)
        loss = ops.pose_loss(s.model, a, x["rr"], x["rt"], x["tgt"], weight=x["w"], clip=True, **kw)
        loss.sum().backward()
        np.testing.assert_array_equal(bits(_np(loss)), bits(r["loss"]))
        np.testing.assert_array_equal(bits(_np(a.grad)), bits(r["grad"]))
    # ops.pose_fit / dof_fit: the launch, the chain 4 + 4 = 8
    kw = dict(weight=x["w"], lr=LR, lr_root_t=0.01, clip=True)
    r8 = rbfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, ap, x["fw"], DELTA, (), None, None, p, pw, PROJECT,
               iters=8, lr_t=0.01)
    p8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, return_grad=True, project=True, **kw, **o)
    for k, v in (("dof", p8.dof), ("rr", p8.root_rot), ("rt", p8.root_t), ("loss", p8.loss), ("grad", p8.grad),
                 ("groot", p8.grad_root)):
        np.testing.assert_array_equal(bits(_np(v)), bits(r8[k]), err_msg=k)
    p4 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, project=True, **kw, **o)
    q8 = ops.pose_fit(s.model, x["tgt"], p4.root_rot, p4.root_t, p4.dof, iters=4, state=p4.state, project=True, **kw, **o)
    assert all(torch.equal(u, v) for u, v in zip(q8[:4] + q8.state[:3], p8[:4] + p8.state[:3]))
    g8 = rbfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, ap, x["fw"], DELTA, (), None, None, p, pw, PROJECT, iters=8)
    d8 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=8, lr=LR, clip=True, return_grad=True,
                     project=True, **o)
    for i, k in ((0, "dof"), (1, "loss"), (3, "grad")):
        np.testing.assert_array_equal(bits(_np(d8[i])), bits(g8[k]), err_msg=k)
    d4 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=8, lr=LR, clip=True, frame_weight=x["fw"])
    np.testing.assert_array_equal(bits(_np(d4[0])), bits(rbfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, None,
                                                               x["fw"], 0.0, iters=8)["dof"]))
    # neither keyword: the old functions' bits
    old = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, ap, prior=p, pw=pw, iters=8, lr_t=0.01)
    n8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, prior=p, prior_weight=pw, apart=spec_,
                      frame_weight=None, robust_scale=None, **kw)
    for k, v in (("dof", n8.dof), ("rr", n8.root_rot), ("rt", n8.root_t), ("loss", n8.loss)):
        np.testing.assert_array_equal(bits(_np(v)), bits(old[k]), err_msg=k)
    z8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, prior=p, prior_weight=pw, apart=spec_,
                      robust_scale=0.0, **kw)
    assert torch.equal(z8.dof, n8.dof)
    # what ops refuses before the C ABI sees a pointer
    with pytest.raises(ValueError, match="frame_weight"):
        ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=1, frame_weight=x["fw"][:, :-1])
    with pytest.raises(ValueError, match="robust_scale"):
        ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=1, robust_scale=-1.0)
    # the drop-in: results on the inputs' device
    hu = _hu_on(s)
    tgt, rt, rr = torch.from_numpy(x["tgt"]), torch.from_numpy(x["rt"]), torch.from_numpy(x["rr"][:, None])
    want = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, lr=LR, clip=True, project=True, **o)
    h = dict(prior_angles=torch.from_numpy(p), prior_weight=torch.from_numpy(pw), project_angles=True, apart=spec_,
             keypoint_confidence=torch.from_numpy(x["fw"]), robust_scale=DELTA)
    ang, t, q, loss, state = hu.fit_pose(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), iters=8, lr=LR, **h)
    assert ang.shape == (B, 32, 1) and all(v.device.type == "cpu" for v in (ang, t, q, loss))
    assert torch.equal(ang[..., 0], want.dof.cpu()) and torch.equal(loss, want.loss.cpu())
    ang, loss, state = hu.fit_keypoints(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), weight=x["w"], iters=8, lr=LR, **h)
    assert torch.equal(ang[..., 0], d8[0].cpu()) and torch.equal(loss, d8[1].cpu())
    m1 = hu.fit_motion(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), smooth_weight=0.0, rounds=2, iters=4, lr=LR,
                       **{k: v for k, v in h.items() if k not in ("prior_angles", "prior_weight")})
    f1 = hu.fit_pose(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), iters=8, lr=LR,
                     **{k: v for k, v in h.items() if k not in ("prior_angles", "prior_weight")})
    assert torch.equal(m1[0], f1[0]) and torch.equal(m1[3], f1[3])


def test_fit_mocap_takes_what_the_ingest_returns(gpu):
    """fit_mocap(source_confidence=..., valid=...) is fit_pose on keypoint_targets' rows with the hand-built (L, J)
    weights: the mapped links take their source joint's confidence, the others 0, an invalid frame a row of zeros --
    whose source rows may then be NaN."""
    import fit_targets_ref as ref
    from robot_kinematics_model import RobotZeroPose
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    from test_gpu_fit_targets import _tree
    y = ref.outcome_recipe()
    hu = HuForwardModel(RobotZeroPose.from_asset("hu").skeleton_tree)
    tree = _tree(y["names"], y["s"].par, y["human_lt"])
    mapping = {y["names"][j]: y["names"][j] for j in y["links"]}
    src = torch.from_numpy(y["human"][:19])
    L, Js, J = src.shape[0], src.shape[1], hu.num_joints
    rng = np.random.default_rng(7)
    conf = rng.uniform(0.1, 1.0, (L, Js)).astype(np.float32)
    conf[rng.random((L, Js)) < 0.2] = 0.0
    valid = np.ones(L, bool)
    valid[[2, L - 1]] = False
    bad = src.clone()
    bad[~torch.from_numpy(valid)] = float("nan")
    names, snames = list(hu.node_names), list(tree.node_names)
    want_fw = np.zeros((L, J), np.float32)
    for a, b in mapping.items():
        want_fw[:, names.index(b)] = conf[:, snames.index(a)]
    want_fw[~valid] = 0.0
    kw = dict(iters=8, lr=LR, robust_scale=DELTA)
    res = hu.fit_mocap(tree, mapping, bad, source_confidence=conf, valid=valid, **kw)
    targets_, w = hu.keypoint_targets(tree, mapping, src)
    np.testing.assert_array_equal(_np(res[-1])[valid], _np(targets_)[valid])
    t0 = targets_[..., 0, :].clone()
    t0[~torch.from_numpy(valid).to(t0.device)] = 0.0
    q0 = torch.zeros((L, 1, 4), device=t0.device)
    q0[..., 3] = 1.0
    ref = hu.fit_pose(targets_, t0, q0, weight=w, keypoint_confidence=torch.from_numpy(want_fw), **kw)
    for u, v in zip(res[:4], ref[:4]):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    only = hu.fit_mocap(tree, mapping, bad, valid=valid, iters=8, lr=LR)
    ref = hu.fit_pose(targets_, t0, q0, weight=w, keypoint_confidence=torch.from_numpy(np.repeat(valid[:, None], J, 1)),
                      iters=8, lr=LR)
    assert all(torch.equal(u, v) for u, v in zip(only[:4], ref[:4]))
    with pytest.raises(ValueError, match="source_confidence"):
        hu.fit_mocap(tree, mapping, src, source_confidence=conf[:, :-1])
    with pytest.raises(ValueError, match="valid"):
        hu.fit_mocap(tree, mapping, src, valid=valid[:-1])


# ------------------------------------------------------------------ 9. the two recipes, for their direction
def test_outlier_recipe_through_the_model(gpu):
    """The host file's outlier recipe through HuForwardModel.fit_pose (float32, one launch of 512 steps each): the other
    links' error in the corrupted frames is lower with the robust kernel and with the keypoint masked than under the
    quadratic loss.  (float64 loop: 15.46 mm against 2.15 and 2.13 mm.)"""
    s, x = outlier_recipe()
    hu = _hu_on(skel("hu33"))
    tgt, t, q = torch.from_numpy(x["tgt"]), torch.from_numpy(x["t"]), torch.from_numpy(x["q"][:, None])
    start = torch.from_numpy(x["start"][..., None])
    kw = dict(lr=LR, iters=x["iters"], fit_root_t=False, fit_root_rot=False, clip_angles=True, project_angles=True)
    err = {}
    for run, o in (("quadratic", {}), ("robust", dict(robust_scale=x["delta"])),
                   ("masked", dict(keypoint_confidence=torch.from_numpy(x["fw"])))):
        a = hu.fit_pose(tgt, t, q, start, **kw, **o)[0]
        assert torch.isfinite(a).all()
        err[run] = link_error(s, a[..., 0].numpy().astype(np.float64), x["clean_pos"], x["bad"], (OUTLIER_JOINT,))
    print(f"outlier recipe on the GPU: other links' mean error in the corrupted frames quadratic {1e3 * err['quadratic']:.2f} mm, "
          f"robust {1e3 * err['robust']:.2f} mm (ratio {err['quadratic'] / err['robust']:.2f}), masked {1e3 * err['masked']:.2f} mm "
          f"(ratio {err['quadratic'] / err['masked']:.2f})")
    assert err["robust"] < err["quadratic"] and err["masked"] < err["quadratic"]


def test_dropout_recipe_through_the_model(gpu):
    """The host file's dropout recipe through HuForwardModel.fit_motion (16 rounds of 8 steps, smooth_weight 0.1): the
    masked and smoothed error in the dropped frames is below the unmasked one's, and with the dropped rows NaN every
    output is finite and has the bits of the run with zero rows.  (float64 loop: 0.075 m against 0.39 m.)"""
    s, x = dropout_recipe()
    hu = _hu_on(skel("hu33"))
    t, q = torch.from_numpy(x["t"]), torch.from_numpy(x["q"][:, None])
    start = torch.from_numpy(x["start"][..., None])
    kw = dict(lr=LR, smooth_weight=x["smooth_weight"], rounds=x["rounds"], iters=x["iters"], fit_root_t=False,
              fit_root_rot=False, clip_angles=True, project_angles=True)
    conf = torch.from_numpy(x["fw"])
    err = {}
    for masked in (False, True):
        res = hu.fit_motion(torch.from_numpy(x["tgt"]), t, q, start, **kw, **(dict(keypoint_confidence=conf) if masked else {}))
        err[masked] = link_error(s, res[0][..., 0].numpy().astype(np.float64), x["clean_pos"], DROPPED)
    nan = hu.fit_motion(torch.from_numpy(dropout_recipe(np.nan)[1]["tgt"]), t, q, start, keypoint_confidence=conf, **kw)
    assert all(torch.isfinite(v).all() for v in nan[:4])
    assert all(torch.equal(u, v) for u, v in zip(nan[:4], res[:4]))
    print(f"dropout recipe on the GPU: mean error in the dropped frames unmasked {err[False]:.4f} m, masked and smoothed "
          f"{err[True]:.4f} m (ratio {err[False] / err[True]:.2f})")
    assert err[True] < err[False]

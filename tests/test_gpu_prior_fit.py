"""GPU: the pose fit with the posture prior and the projection (rtg_dof_fit_prior_f32: the pose fit's loss plus
sum_d prior_weight[d] (a_d - prior_d)^2 on the iterate, and on request a clamp of each angle to its limits after its
Adam step) against the torch restatement of tests/test_prior_fit_host.py on the CPU in float64 and float32.

The criterion is the project's own, per tensor: E(x) = max|x - x64| / max|x64|, and E(gpu) <= 8 max(E(restatement
f32), 2^-24).  One Adam step is checked on its own against the update formula in float64 on the GPU's own gradient,
with and without the clamp, and everything the header promises bit for bit (no prior and no flag against
rtg_dof_fit_orient_f32 and rtg_dof_fit_f32, zero weights, the DOFs nothing else reaches, chained launches, batch and
tile independence, repeatability, the prior aliasing dof_in or dof_out, autograd, a bad frame staying in its rows) is
checked bit for bit.  The two outcome recipes of the host file are replayed on the GPU for the effect, not for parity:
float32 trajectories of 160 clamped steps diverge from the float64 loop's (1.66, 28.6 and +0.6 % there).

Measured on the MI355X: see DESIGN 5i and profiles/r23/prior_fit/test_ratios.txt."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_dof_fit import bits, check_criterion, fit, inputs, skel
from test_gpu_orient_fit import link_sets, ofit, targets, zero_dofs
from test_gpu_pose_fit import MASKS, OUTS, U, _dev, _np, assert_same_bits, pfit, random_state
from test_orient_fit_host import INVALID
from test_pose_fit_host import B1, B2, EPS, FIT_ROT, FIT_T, LR
from test_prior_fit_host import (PROJECT, RefFit, projection_recipe, ref_prior_loss, ref_prior_loss_grad, roughness,
                                 smoothing_recipe)

pytestmark = pytest.mark.gpu

NAMES = ("hu33", "chain64", "tree37", "star61", "two", "one")
STATE = OUTS + ("m", "v", "rs")


# ------------------------------------------------------------------ the launch, straight through the C ABI
def prfit(s, tgt, w, rr, rt, dof, clip, mask, joints=(), R=None, rw=None, prior=None, pw=None, flags=0, iters=0, lr=LR,
          lr_t=LR, lr_q=LR, betas=(B1, B2), eps=EPS, step0=0, m=None, v=None, rs=None, alias=False, want=OUTS, status=False,
          prior_alias=None):
    """rtg_dof_fit_prior_f32 on host arrays -> dict of host arrays (dof, rr, rt, loss, grad, groot, m, v, rs).
    prior_alias: "in" -- the prior IS dof_in's buffer (``prior`` is ignored); "out" -- the prior lives in dof_out's."""
    from rtg import _lib
    from rtg.runtime import ptr
    B, n, K = tgt.shape[0], s.J - 1, len(joints)
    d_in, rr_in, rt_in = _dev(dof), _dev(rr), _dev(rt)
    bufs = dict(tp=_dev(tgt), w=_dev(w), m=_dev(m), v=_dev(v), rs=_dev(rs), rw=_dev(rw), pw=_dev(pw))
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
    jarr = (ctypes.c_int32 * max(K, 1))(*[int(j) for j in joints])
    rc = _lib.lib().rtg_dof_fit_prior_f32(
        s.model.handle, ptr(bufs["tp"]), ptr(bufs["w"]), jarr if K else None, ptr(R_dev), ptr(bufs["rw"]), K, ptr(p_dev),
        ptr(bufs["pw"]), flags, ptr(rr_in), ptr(rt_in), ptr(d_in), B, int(clip), mask, iters, lr, lr_t, lr_q, betas[0],
        betas[1], eps, step0, ptr(bufs["m"]), ptr(bufs["v"]), ptr(bufs["rs"]), *(ptr(out[k]) for k in OUTS), None)
    if status:
        return rc, _lib.lib().rtg_last_error()
    assert rc == 0, _lib.lib().rtg_last_error()
    torch.cuda.synchronize()
    res = {k: _np(x) for k, x in out.items()}
    res.update(m=_np(bufs["m"]), v=_np(bufs["v"]), rs=_np(bufs["rs"]))
    return res


def priors(s, dof, seed):
    """Priors 0.5-2 rad from the angles on a random side (so some lie outside the limits); prior_weight 0.2-2, a third
    of them 0."""
    rng = np.random.default_rng(seed)
    B, n = dof.shape
    p = (dof + rng.uniform(0.5, 2.0, (B, n)) * rng.choice([-1.0, 1.0], (B, n))).astype(np.float32)
    pw = rng.uniform(0.2, 2.0, n).astype(np.float32)
    pw[rng.permutation(n)[: n // 3]] = 0.0
    return p, pw


def link_set(s, w, K):
    if K == 0:
        return []
    sets = link_sets(s, w)
    return sets.get("k8", sets["root"])


# ------------------------------------------------------------------ 1. evaluate
@functools.lru_cache(maxsize=None)
def _case(name, clip):
    s = skel(name)
    x = inputs(s, max(s.batches()), clip, 19 * s.J + clip)
    x["prior"], x["pw"] = priors(s, x["dof"], 23 * s.J + clip)
    return s, x


@functools.lru_cache(maxsize=None)
def _evaluate_reference(name, clip, K, normalised):
    s, x = _case(name, clip)
    joints = link_set(s, x["w"], K)
    R, rw = targets(len(x["dof"]), len(joints), 29 * s.J + K)
    tail = (x["tgt"], x["w"], clip)
    rest = (FIT_ROT if normalised else 0, joints, R, rw, x["prior"], x["pw"])
    return (joints, R, rw, ref_prior_loss_grad(s, x["dof"], x["rr"], x["rt"], *tail, torch.float64, *rest),
            ref_prior_loss_grad(s, x["dof"], x["rr"], x["rt"], *tail, torch.float32, *rest))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_evaluate_against_autograd(gpu, name, clip):
    """iters = 0: loss, grad and grad_root with K = 0 and K = 8 links, all four masks and all five batch sizes against
    float64 autograd of the restatement; the inputs' bits come back, with and without RTG_FIT_PROJECT."""
    s, x = _case(name, clip)
    for K in (0, 8):
        for mask in MASKS:
            joints, R, rw, (l64, g64, r64), (l32, g32, r32) = _evaluate_reference(name, clip, K, bool(mask & FIT_ROT))
            full = None
            for B in sorted(s.batches(), reverse=True):
                r = prfit(s, x["tgt"][:B], x["w"], x["rr"][:B], x["rt"][:B], x["dof"][:B], clip, mask, joints, R[:B], rw,
                          x["prior"][:B], x["pw"], PROJECT if B % 2 else 0)
                what = f"{name} clip={clip} K={len(joints)} mask={mask} B={B}"
                check_criterion(f"{what} loss", r["loss"], l32[:B], l64[:B])
                check_criterion(f"{what} grad", r["grad"], g32[:B], g64[:B])
                check_criterion(f"{what} grad_t", r["groot"][:, :3], r32[:B, :3], r64[:B, :3])
                check_criterion(f"{what} grad_q", r["groot"][:, 3:], r32[:B, 3:], r64[:B, 3:])
                for k, a in (("dof", x["dof"]), ("rr", x["rr"]), ("rt", x["rt"])):   # iters = 0: the inputs' bits
                    np.testing.assert_array_equal(bits(r[k]), bits(a[:B]), err_msg=f"{what} {k}")
                if full is None:
                    full = r
                assert_same_bits(r, {k: a[:B] for k, a in full.items() if a is not None}, what, ("loss", "grad", "groot"))
    # prior_weight NULL is all ones
    B = max(s.batches())
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], clip, 3)
    a = prfit(s, *args, prior=x["prior"], pw=None)
    assert_same_bits(a, prfit(s, *args, prior=x["prior"], pw=np.ones(s.J - 1, np.float32)), f"{name} prior_weight NULL", OUTS)


def test_rejected(gpu):
    from rtg.runtime import DofModel, Topology
    s = skel("two")
    x = inputs(s, 3, False, 2)
    p, pw = priors(s, x["dof"], 3)
    a = (s, x["tgt"], None, x["rr"], x["rt"], x["dof"], False, 3)
    rc, msg = prfit(*a, prior=p, pw=pw, flags=2, status=True)
    assert rc == INVALID and b"flags=2 has unknown bits" in msg
    rc, msg = prfit(*a, prior=None, pw=pw, status=True)
    assert rc == INVALID and b"prior_weight given without prior" in msg

    class NoLimits:
        J, F = s.J, s.F
        model = DofModel(Topology(s.par, s.lt), s.axis)
    for flags, prior in ((PROJECT, p), (PROJECT, None)):
        rc, msg = prfit(NoLimits, *a[1:], prior=prior, flags=flags, iters=1, status=True)
        assert rc == INVALID and b"RTG_FIT_PROJECT requested but the model has no DOF limits" in msg
        assert b"rtg_dof_fit_prior_f32" in msg
    r = prfit(NoLimits, *a[1:], prior=p, pw=pw, iters=2)                          # the prior alone needs no limits
    assert_same_bits(r, prfit(*a, prior=p, pw=pw, iters=2), "no limits", OUTS)
    rc, _ = prfit(s, x["tgt"][:0], None, x["rr"][:0], x["rt"][:0], x["dof"][:0], False, 3, prior=p[:0], status=True)
    assert rc == 0                                                               # B == 0: a no-op
    # a one-joint model: neither pointer is dereferenced (dummy addresses), the projection has nothing to do
    one = skel("one")
    y = inputs(one, 5, True, 4)
    want = pfit(one, y["tgt"], y["w"], y["rr"], y["rt"], y["dof"], True, 3, iters=2)
    from rtg import _lib
    from rtg.runtime import ptr
    t = {k: _dev(y[k]) for k in ("tgt", "w", "rr", "rt")}
    out = dict(rr=torch.empty(5, 4, device="cuda"), rt=torch.empty(5, 3, device="cuda"), loss=torch.empty(5, device="cuda"))
    bad = ctypes.c_void_p(64)
    rc = _lib.lib().rtg_dof_fit_prior_f32(one.model.handle, ptr(t["tgt"]), ptr(t["w"]), None, None, None, 0, bad, bad, PROJECT,
                                          ptr(t["rr"]), ptr(t["rt"]), None, 5, 1, 3, 2, LR, LR, LR, B1, B2, EPS, 0, None, None,
                                          None, None, ptr(out["rr"]), ptr(out["rt"]), ptr(out["loss"]), None, None, None)
    assert rc == 0, _lib.lib().rtg_last_error()
    torch.cuda.synchronize()
    assert_same_bits({k: _np(a) for k, a in out.items()}, want, "one joint")


# ------------------------------------------------------------------ 2. one Adam step against the formula
@pytest.mark.parametrize("project", [False, True])
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_one_adam_step_against_the_formula(gpu, name, project):
    """iters = 1 from a random state (v0 >= m0^2, five steps taken) against the update formula in float64 on the GPU's
    own iters = 0 gradient (the prior's term in it), the hyper-parameters as the launch receives them (float32):
    |delta| <= 8 2^-24 (|old| + |update|) per element.  Projected: an angle the formula leaves outside its limits by
    more than that bound lands on the limit's bits, one it leaves inside by more than the bound is the formula's; the
    moments are the unprojected step's."""
    s = skel(name)
    B, step0 = 4 * s.F + 3, 5
    x = inputs(s, B, True, 81)
    x["dof"][:, ::2] = np.random.default_rng(82).uniform(s.lo, s.hi, x["dof"].shape).astype(np.float32)[:, ::2]
    q0 = x["rr"].astype(np.float64)
    x["rr"] = (q0 / np.linalg.norm(q0, axis=-1, keepdims=True)).astype(np.float32)
    st = random_state(x, 83)
    p, pw = priors(s, x["dof"], 84)
    joints = link_set(s, x["w"], 8)
    R, rw = targets(B, len(joints), 85)
    flags = PROJECT if project else 0
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, FIT_T | FIT_ROT, joints, R, rw, p, pw, flags)
    e = prfit(s, *args)
    r = prfit(s, *args, iters=1, step0=step0, **st)
    b1, b2, eps, lr = (float(np.float32(h)) for h in (B1, B2, EPS, LR))
    t = step0 + 1
    g, m0, v0, old = (a.astype(np.float64) for a in (e["grad"], st["m"], st["v"], x["dof"]))
    m = b1 * m0 + (1 - b1) * g
    v = b2 * v0 + (1 - b2) * g * g
    upd = lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    new = old - upd
    tol = 8 * U * (np.abs(old) + np.abs(upd))
    assert (np.abs(r["m"] - m) <= 2 * U * (np.abs(b1 * m0) + np.abs((1 - b1) * g))).all()
    assert (np.abs(r["v"] - v) <= 2 * U * v).all()
    assert np.abs(upd).max() > 1e-3
    if not project:
        excess = np.abs(r["dof"] - new) / (tol / 8)
        print(f"{name}: Adam step with the prior, max |delta| / (2^-24 (|old| + |update|)) {excess.max():.2f} (bound 8)")
        assert excess.max() <= 8
        return
    lo, hi = s.lo.astype(np.float64), s.hi.astype(np.float64)
    below, above, inside = new < lo - tol, new > hi + tol, (new > lo + tol) & (new < hi - tol)
    assert below.sum() > B and above.sum() > B and inside.sum() > B
    np.testing.assert_array_equal(bits(r["dof"][below]), bits(np.broadcast_to(s.lo, new.shape)[below]))
    np.testing.assert_array_equal(bits(r["dof"][above]), bits(np.broadcast_to(s.hi, new.shape)[above]))
    assert (np.abs(r["dof"] - new)[inside] <= tol[inside]).all()
    assert ((r["dof"] >= s.lo) & (r["dof"] <= s.hi)).all()


# ------------------------------------------------------------------ 3. bit for bit
@pytest.mark.parametrize("name", ["hu33", "chain64", "tree37", "one"])
def test_no_prior_and_no_flag_is_the_oriented_fit(gpu, name):
    """Guarantee (a): prior NULL and flags 0 through the new symbol, for K = 0 and K > 0, iters 0, 4, 8; at mask 0 and
    K = 0 that is rtg_dof_fit_f32."""
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 91)
    st = random_state(x, 92, 0.1)
    if s.J == 1:
        st["m"] = st["v"] = np.zeros((B, 1), np.float32)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    for K in (0, 8):
        joints = link_set(s, x["w"], K)
        R, rw = targets(B, len(joints), 93)
        for mask in MASKS:
            for iters in (0, 4, 8):
                kw = dict(iters=iters, step0=3, lr_t=0.01, lr_q=0.03, **st)
                assert_same_bits(ofit(s, *args, mask, joints, R, rw, **kw), prfit(s, *args, mask, joints, R, rw, **kw),
                                 f"{name} K={len(joints)} mask={mask} iters={iters}")
    if s.J > 1:
        for iters in (0, 4, 8):
            old = fit(s, *args, iters=iters, step0=3, m=st["m"], v=st["v"])
            assert_same_bits(old, prfit(s, *args, 0, iters=iters, step0=3, **st), f"{name} rtg_dof_fit_f32 iters={iters}")


@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_zero_prior_weights_change_no_number(gpu, name):
    """Guarantee (b): prior_weight all zero, finite inputs: every output and state row equals the launch without a
    prior as a number (a zero may change sign)."""
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 101)
    st = random_state(x, 102, 0.1)
    p, _ = priors(s, x["dof"], 103)
    pw0 = np.zeros(s.J - 1, np.float32)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    for K in (0, 8):
        joints = link_set(s, x["w"], K)
        R, rw = targets(B, len(joints), 104)
        for iters in (0, 4, 8):
            for mask in (0, 3):
                kw = dict(iters=iters, step0=3, **st)
                a = ofit(s, *args, mask, joints, R, rw, **kw)
                b = prfit(s, *args, mask, joints, R, rw, p, pw0, **kw)
                for k in STATE:
                    assert np.array_equal(a[k], b[k]), f"{name} K={K} iters={iters} mask={mask} {k}"


@pytest.mark.parametrize("name", ["hu33", "tree37"])
def test_unreached_dofs_get_the_prior_alone(gpu, name):
    """Guarantee (c) on the DOF set computed from the tree (no position weight strictly below, no oriented link at or
    below): with prior_weight > 0 the gradient is fl(2 pw) fl(a - p) to the bit, with prior_weight == 0 it is +-0 and
    from a zero state the angle keeps its bits."""
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 111)
    leaves = [j for j in range(s.J) if j not in set(int(q) for q in s.par)]
    joints = [leaves[0], 0]
    R, rw = targets(B, len(joints), 112)
    p, pw = priors(s, x["dof"], 113)
    still = np.flatnonzero(zero_dofs(s, x["w"], joints))
    assert len(still) >= 4
    pw[still[::2]] = 0.0
    pw[still[1::2]] = np.abs(pw[still[1::2]]) + 0.3
    held, free = still[1::2], still[::2]
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, joints, R, rw, p, pw)
    for flags in (0, PROJECT):
        e = prfit(s, *args, flags)
        want = (np.float32(2.0) * pw[held]) * (x["dof"][:, held] - p[:, held])
        np.testing.assert_array_equal(bits(e["grad"][:, held]), bits(want))
        assert (e["grad"][:, free] == 0).all()
    for kw in (random_state(x, 114, 0.0), dict()):                               # explicit zero state, and none
        r = prfit(s, *args, 0, iters=3, **kw)
        np.testing.assert_array_equal(bits(r["dof"][:, free]), bits(x["dof"][:, free]))
        assert (bits(r["dof"][:, held]) != bits(x["dof"][:, held])).all()
        assert (np.abs(r["dof"][:, held] - p[:, held]) < np.abs(x["dof"][:, held] - p[:, held])).all()


@pytest.mark.parametrize("project", [False, True])
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_self_consistency(gpu, name, project):
    s = skel(name)
    F = s.F
    B = 4 * F + 3
    x = inputs(s, B, True, 121)
    st = random_state(x, 122, 0.1)
    p, pw = priors(s, x["dof"], 123)
    flags = PROJECT if project else 0
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    kw = dict(iters=8, step0=3, lr_t=0.01, lr_q=0.03)
    for K in (0, 8):
        joints = link_set(s, x["w"], K)
        R, rw = targets(B, len(joints), 124)
        ori = (joints, R, rw)
        for mask in (0, 3):
            one = prfit(s, *args, mask, *ori, p, pw, flags, **kw, **st)
            assert all(np.isfinite(a).all() for a in one.values())
            # two identical launches
            assert_same_bits(one, prfit(s, *args, mask, *ori, p, pw, flags, **kw, **st), f"repeat K={K} mask={mask}")
            # eight launches of one step, carrying (dof, root, m, v, root_state, step)
            c = dict(dof=x["dof"], rr=x["rr"], rt=x["rt"], **st)
            for k in range(8):
                c = prfit(s, x["tgt"], x["w"], c["rr"], c["rt"], c["dof"], True, mask, *ori, p, pw, flags,
                          **dict(kw, iters=1, step0=3 + k), m=c["m"], v=c["v"], rs=c["rs"])
            assert_same_bits(one, c, f"chained K={K} mask={mask}")
            # dof_out, root_rot_out, root_t_out aliasing the inputs
            assert_same_bits(one, prfit(s, *args, mask, *ori, p, pw, flags, **kw, **st, alias=True), f"alias K={K} mask={mask}")
            # the prior in dof_out's buffer
            assert_same_bits(one, prfit(s, *args, mask, *ori, p, pw, flags, **kw, **st, prior_alias="out"),
                             f"prior in dof_out K={K} mask={mask}")
        # a frame of the large launch is that frame run alone (mask 3, from the loop's last round)
        for f in (0, F - 1, 2 * F + 1, B - 1):
            sl = slice(f, f + 1)
            alone = prfit(s, x["tgt"][sl], x["w"], x["rr"][sl], x["rt"][sl], x["dof"][sl], True, 3, joints, R[sl], rw, p[sl], pw,
                          flags, **kw, **{k: a[sl] for k, a in st.items()})
            assert_same_bits(alone, {k: a[sl] for k, a in one.items()}, f"frame {f} K={K}")
    # the prior IS dof_in ("stay near where you started"), also with dof_out on top of both
    for iters in (0, 4, 8):
        a = prfit(s, *args, 3, prior=x["dof"].copy(), pw=pw, flags=flags, iters=iters, **st)
        assert_same_bits(a, prfit(s, *args, 3, pw=pw, flags=flags, iters=iters, **st, prior_alias="in"), f"prior = dof_in {iters}")
        assert_same_bits(a, prfit(s, *args, 3, pw=pw, flags=flags, iters=iters, **st, prior_alias="in", alias=True),
                         f"prior = dof_in = dof_out {iters}")
    # outputs are optional one by one
    a = prfit(s, *args, 3, prior=p, pw=pw, flags=flags, iters=4)
    for k in OUTS:
        assert_same_bits(prfit(s, *args, 3, prior=p, pw=pw, flags=flags, iters=4, want=(k,)), {k: a[k]}, f"only {k}", (k,))


def test_a_bad_frame_stays_its_own(gpu):
    """A NaN prior, an inf angle and a NaN angle under projection in the middle frame of three tiles: every other frame
    keeps its bits, the bad frame's loss is NaN where the float32 restatement's is, and the clamp lets a NaN angle
    through as torch.clamp does."""
    s = skel("hu33")
    B = 3 * s.F
    f = B // 2
    x = inputs(s, B, True, 131)
    x["prior"], pw = priors(s, x["dof"], 132)
    pw[:] = np.abs(pw) + 0.3
    args = lambda y: (y["tgt"], y["w"], y["rr"], y["rt"], y["dof"], True, FIT_T | FIT_ROT, (), None, None, y["prior"], pw,
                      PROJECT)
    clean = prfit(s, *args(x), iters=3)
    clean0 = prfit(s, *args(x))
    assert all(np.isfinite(a).all() for a in clean.values() if a is not None)
    ok = np.arange(B) != f
    for which in ("prior", "inf", "nan"):
        y = {k: a.copy() for k, a in x.items()}
        if which == "prior":
            y["prior"][f, 5] = np.nan
        else:
            y["dof"][f, 2] = np.inf if which == "inf" else np.nan
        bad = prfit(s, *args(y), iters=3)
        for k in OUTS:
            np.testing.assert_array_equal(bits(bad[k][ok]), bits(clean[k][ok]), err_msg=f"{which} {k}")
        bad0 = prfit(s, *args(y))
        for k in ("loss", "grad", "groot"):
            np.testing.assert_array_equal(bits(bad0[k][ok]), bits(clean0[k][ok]), err_msg=f"{which} {k}")
        sl = slice(f, f + 1)
        with np.errstate(all="ignore"), torch.no_grad():
            want = ref_prior_loss(s, y["dof"][sl], y["rr"][sl], y["rt"][sl], y["tgt"][sl], y["w"], True, torch.float32,
                                  FIT_ROT, [], None, None, y["prior"][sl], pw).numpy()
        assert np.isnan(want[0]) and np.isnan(bad0["loss"][f]), which
        if which == "prior":   # the term's own gradient: NaN on that DOF at least, and after a step the angle
            assert np.isnan(bad0["grad"][f, 5]) and np.isnan(bad["dof"][f, 5])
        if which == "nan":     # torch.clamp passes NaN
            assert np.isnan(bad["dof"][f, 2])


# ------------------------------------------------------------------ 4. the projected iterate lies inside the limits
@pytest.mark.parametrize("name", ["hu33", "chain64", "two"])
def test_the_projected_iterate_is_inside_the_limits(gpu, name):
    """Guarantee (e), exactly: starts 0.2-4 rad outside the limits, priors outside them too, clip on and off, after 1
    and after 16 steps; iters = 0 passes the input's bits through."""
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 141)
    p, pw = priors(s, x["dof"], 142)
    assert ((x["dof"] < s.lo) | (x["dof"] > s.hi)).mean() > 0.5
    for clip in (True, False):
        for prior in (p, None):
            args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], clip, 3, (), None, None, prior, None if prior is None else pw)
            r0 = prfit(s, *args, PROJECT)
            np.testing.assert_array_equal(bits(r0["dof"]), bits(x["dof"]))
            for iters in (1, 16):
                r = prfit(s, *args, PROJECT, iters=iters)
                assert ((r["dof"] >= s.lo) & (r["dof"] <= s.hi)).all(), (name, clip, iters)
                u = prfit(s, *args, 0, iters=iters)
                assert not ((u["dof"] >= s.lo) & (u["dof"] <= s.hi)).all()


# ------------------------------------------------------------------ 5. the prior alone
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_the_prior_alone(gpu, name):
    """Every position weight 0, K = 0, prior_weight 1 (NULL), 32 steps: against the float64 loop by the criterion, and
    every DOF ends nearer its prior than it started."""
    s = skel(name)
    B = s.F + 1
    x = inputs(s, B, True, 151)
    p, _ = priors(s, x["dof"], 152)
    w0 = np.zeros(s.J, np.float32)
    ref = {dt: RefFit(s, x["dof"], x["rr"], x["rt"], w0, True, dt, 0).run(x["tgt"], 32, p).result(x["tgt"], p)
           for dt in (torch.float64, torch.float32)}
    r = prfit(s, x["tgt"], w0, x["rr"], x["rt"], x["dof"], True, 0, prior=p, iters=32)
    check_criterion(f"{name} prior alone, 32 steps: dof", r["dof"], ref[torch.float32][1], ref[torch.float64][1])
    check_criterion(f"{name} prior alone, 32 steps: loss", r["loss"], ref[torch.float32][0], ref[torch.float64][0])
    assert (np.abs(r["dof"] - p) < np.abs(x["dof"] - p)).all()


# ------------------------------------------------------------------ 6. outcomes on the two pinned recipes
def test_projection_outcome(gpu):
    """The projection recipe on the GPU: 128 steps on unreachable targets, then 32 on reachable ones with the state
    carried.  Mean final loss unprojected over projected >= 1.3 (1.66 on the float64 loop)."""
    _, x = projection_recipe()
    s = skel("hu33")
    loss = {}
    for project in (False, True):
        flags = PROJECT if project else 0
        st = dict(m=np.zeros_like(x["start"]), v=np.zeros_like(x["start"]), rs=np.zeros((len(x["start"]), 14), np.float32))
        a = prfit(s, x["tgt1"], x["w"], x["q"], x["t"], x["start"], True, 0, flags=flags, iters=128, **st)
        if project:
            assert ((a["dof"] >= s.lo) & (a["dof"] <= s.hi)).all()
        b = prfit(s, x["tgt2"], x["w"], x["q"], x["t"], a["dof"], True, 0, flags=flags, iters=32, step0=128, m=a["m"], v=a["v"],
                  rs=a["rs"])
        loss[project] = b["loss"]
    ratio = loss[False].mean() / loss[True].mean()
    print(f"projection recipe on the GPU: mean final loss unprojected {loss[False].mean():.3f}, projected "
          f"{loss[True].mean():.3f}, ratio {ratio:.2f} (bound 1.3; float64 loop 1.66)")
    assert ratio >= 1.3


def _hu_on(s):
    """HuForwardModel's fitting methods on a test skeleton's model."""
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    hu = HuForwardModel.__new__(HuForwardModel)
    hu._model, hu.num_joints, hu.node_names = s.model, s.J, [f"n{j}" for j in range(s.J)]
    return hu


def test_smoothing_outcome_and_fit_motion(gpu):
    """The smoothing recipe through HuForwardModel.fit_motion: roughness independent over smoothed >= 5 (28.6 on the
    float64 loop), mean noisy-target loss within 5 % of the independent fit's (+0.6 % there).  smooth_weight = 0 is
    one fit_pose of rounds * iters steps, bit for bit."""
    _, x = smoothing_recipe()
    s = skel("hu33")
    hu = _hu_on(s)
    tgt, t, q = torch.from_numpy(x["tgt"]), torch.from_numpy(x["t"]), torch.from_numpy(x["q"][:, None])
    start = torch.from_numpy(x["start"][..., None])
    kw = dict(lr=LR, fit_root_t=False, fit_root_rot=False, clip_angles=True, project_angles=True)
    out = {}
    for smoothed in (False, True):
        res = hu.fit_motion(tgt, t, q, start, smooth_weight=x["smooth_weight"] if smoothed else 0.0, rounds=x["rounds"],
                            iters=x["iters"], **kw)
        a = res[0][..., 0].numpy()
        assert res[0].shape == (64, 32, 1) and res[4][3] == 64
        keypoints = pfit(s, x["tgt"], x["w"], x["q"], x["t"], a, True, 0)["loss"]   # without the prior's term
        out[smoothed] = (a, keypoints, res)
    one = hu.fit_pose(tgt, t, q, start, iters=64, **kw)
    for a, b in zip(out[False][2][:4] + out[False][2][4][:3], one[:4] + one[4][:3]):
        assert torch.equal(a, b)
    r_ind, r_smo = roughness(out[False][0]), roughness(out[True][0])
    l_ind, l_smo = out[False][1].mean(), out[True][1].mean()
    print(f"smoothing recipe on the GPU: roughness independent {r_ind:.2e}, smoothed {r_smo:.2e}, ratio {r_ind / r_smo:.1f} "
          f"(bound 5; float64 loop 28.6); mean noisy-target loss independent {l_ind:.5f}, smoothed {l_smo:.5f} "
          f"({100 * (l_smo / l_ind - 1):+.2f} %, bound 5 %)")
    assert r_ind / r_smo >= 5
    assert abs(l_smo / l_ind - 1) <= 0.05


# ------------------------------------------------------------------ 7. the Python surface
def test_python_entry_points(gpu):
    from rtg import ops
    s = skel("hu33")
    B = 19
    x = inputs(s, B, True, 161)
    p, pw = priors(s, x["dof"], 162)
    joints = [20, 32]
    R, rw = targets(B, 2, 163)
    o = dict(prior=p, prior_weight=pw)
    # ops.pose_loss / keypoint_loss: the evaluate-only launch under autograd; a cotangent scales row by row
    for ori, okw in (((), {}), ((joints, R, rw), dict(rot_joints=joints, target_rot=R, rot_weight=rw))):
        for normalise, mask in ((True, FIT_ROT), (False, 0)):
            r = prfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask, *(ori or ((), None, None)), p, pw)
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
        g0 = prfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, *(ori or ((), None, None)), p, pw)
        a = _dev(x["dof"]).requires_grad_(True)
        kl = ops.keypoint_loss(s.model, a, x["tgt"], x["rr"], x["rt"], weight=x["w"], clip=True, **o, **okw)
        kl.sum().backward()
        np.testing.assert_array_equal(bits(_np(kl)), bits(g0["loss"]))
        np.testing.assert_array_equal(bits(_np(a.grad)), bits(g0["grad"]))
    # ops.pose_fit / dof_fit: the launch, the chain 4 + 4 = 8, a scalar weight, the (..., J-1, 1) form
    kw = dict(weight=x["w"], lr=LR, lr_root_t=0.01, clip=True)
    r8 = prfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, (), None, None, p, pw, PROJECT, iters=8, lr_t=0.01)
    p8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, return_grad=True, project=True, **kw, **o)
    for k, a in (("dof", p8.dof), ("rr", p8.root_rot), ("rt", p8.root_t), ("loss", p8.loss), ("grad", p8.grad),
                 ("groot", p8.grad_root)):
        np.testing.assert_array_equal(bits(_np(a)), bits(r8[k]), err_msg=k)
    p4 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, project=True, **kw, **o)
    q8 = ops.pose_fit(s.model, x["tgt"], p4.root_rot, p4.root_t, p4.dof, iters=4, state=p4.state, project=True, **kw, **o)
    assert all(torch.equal(a, b) for a, b in zip(q8[:4] + q8.state[:3], p8[:4] + p8.state[:3]))
    half = prfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, (), None, None, p, np.full(32, 0.5, np.float32),
                 iters=4, lr_t=0.01)
    h4 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"][..., None], iters=4, prior=p[..., None], prior_weight=0.5, **kw)
    assert h4.dof.shape == (B, 32, 1)
    np.testing.assert_array_equal(bits(_np(h4.dof[..., 0])), bits(half["dof"]))
    only = prfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, flags=PROJECT, iters=4, lr_t=0.01)
    np.testing.assert_array_equal(bits(_np(ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, project=True,
                                                        **kw).dof)), bits(only["dof"]))
    g8 = prfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, (), None, None, p, pw, PROJECT, iters=8)
    d8 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=8, lr=LR, clip=True, return_grad=True,
                     project=True, **o)
    for i, k in ((0, "dof"), (1, "loss"), (3, "grad")):
        np.testing.assert_array_equal(bits(_np(d8[i])), bits(g8[k]), err_msg=k)
    # none of the keywords: the old functions' bits
    old = pfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, iters=8, lr_t=0.01)
    n8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, **kw)
    for k, a in (("dof", n8.dof), ("rr", n8.root_rot), ("rt", n8.root_t), ("loss", n8.loss)):
        np.testing.assert_array_equal(bits(_np(a)), bits(old[k]), err_msg=k)
    # what ops refuses before the C ABI sees a pointer
    from rtg.runtime import DofModel, Topology
    for bad in (dict(prior=p[:, :31]), dict(prior=p[:5]), dict(prior_weight=pw), dict(prior=p, prior_weight=pw[:3]),
                dict(prior=p.astype(np.int32)), dict(prior=p, prior_weight=np.ones((2, 32), np.float32))):
        with pytest.raises(ValueError):
            ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=1, **kw, **bad)
    with pytest.raises(ValueError, match="limits"):
        ops.pose_fit(DofModel(Topology(s.par, s.lt), s.axis), x["tgt"], x["rr"], x["rt"], x["dof"], iters=1, project=True)
    # the drop-in: (L, J-1, 1) priors, results on the inputs' device
    hu = _hu_on(s)
    tgt, rt, rr = torch.from_numpy(x["tgt"]), torch.from_numpy(x["rt"]), torch.from_numpy(x["rr"][:, None])
    want = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, lr=LR, clip=True, project=True, **o)
    for pa in (torch.from_numpy(p[..., None]), torch.from_numpy(p)):
        ang, t, q, loss, state = hu.fit_pose(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), iters=8, lr=LR,
                                             prior_angles=pa, prior_weight=torch.from_numpy(pw), project_angles=True)
        assert ang.shape == (B, 32, 1) and all(a.device.type == "cpu" for a in (ang, t, q, loss))
        assert torch.equal(ang[..., 0], want.dof.cpu()) and torch.equal(loss, want.loss.cpu())
    ang, loss, state = hu.fit_keypoints(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), weight=x["w"], iters=8, lr=LR,
                                        prior_angles=torch.from_numpy(p), prior_weight=torch.from_numpy(pw), project_angles=True)
    assert torch.equal(ang[..., 0], d8[0].cpu()) and torch.equal(loss, d8[1].cpu())

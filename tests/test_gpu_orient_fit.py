"""GPU: the pose fit with orientation targets (rtg_dof_fit_orient_f32: the keypoint loss plus
sum_k rot_weight[k] 4 (1 - <G_j(k), R^_k>^2) for K <= 8 chosen links, fitted in the one launch of the pose fit) against
the torch restatement of tests/test_orient_fit_host.py on the CPU in float64 and float32.

The criterion is the project's own, per tensor: E(x) = max|x - x64| / max|x64|, and E(gpu) <= 8 max(E(restatement
f32), 2^-24).  One Adam step is checked on its own against the update formula in float64 on the GPU's own gradient,
and everything that has to hold bit for bit (K = 0 against rtg_dof_fit_root_f32 and rtg_dof_fit_f32, the +-0 rule, R
against -R, chained launches, batch and tile independence, repeatability, aliasing, autograd, a bad frame staying in
its rows) is checked bit for bit.

Measured on the MI355X (ratios E(gpu) / max(E(restatement f32), 2^-24), bound 8; the full list is
profiles/r19/orient_fit/test_ratios.txt): see DESIGN 5h."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_gpu_dof_fit import SKELS, bits, check_criterion, fit, inputs, skel
from test_gpu_pose_fit import MASKS, OUTS, U, _dev, _np, assert_same_bits, pfit, random_state
from test_orient_fit_host import (HU_HANDS_FEET_HEAD, INVALID, UNSUPPORTED, orient_error, ref_orient_fit, ref_orient_loss,
                                  ref_orient_loss_grad)
from test_pose_fit_host import B1, B2, EPS, FIT_ROT, FIT_T, LR, _t, recipe
from test_fk_grad_host import dof_fk

pytestmark = pytest.mark.gpu

NAMES = ("hu33", "chain64", "tree37", "star61", "two", "one")
assert set(NAMES) <= set(SKELS)


# ------------------------------------------------------------------ the launch, straight through the C ABI
def ofit(s, tgt, w, rr, rt, dof, clip, mask, joints=(), R=None, rw=None, iters=0, lr=LR, lr_t=LR, lr_q=LR, betas=(B1, B2),
         eps=EPS, step0=0, m=None, v=None, rs=None, alias=False, want=OUTS, status=False, misalign=False):
    """rtg_dof_fit_orient_f32 on host arrays -> dict of host arrays (dof, rr, rt, loss, grad, groot, m, v, rs)."""
    from rtg import _lib
    from rtg.runtime import ptr
    B, n, K = tgt.shape[0], s.J - 1, len(joints)
    d_in, rr_in, rt_in = _dev(dof), _dev(rr), _dev(rt)
    bufs = dict(tp=_dev(tgt), w=_dev(w), m=_dev(m), v=_dev(v), rs=_dev(rs), rw=_dev(rw))
    R_dev = None
    if R is not None:
        flat = torch.zeros(B * K * 4 + 1, device="cuda")
        R_dev = flat[1:] if misalign else flat[:-1]
        R_dev.copy_(_dev(np.asarray(R, np.float32).reshape(-1)))
    new = lambda *shape: torch.full(shape, 7.0, device="cuda")
    out = {"dof": None if "dof" not in want else d_in if alias else new(B, n),
           "rr": None if "rr" not in want else rr_in if alias else new(B, 4),
           "rt": None if "rt" not in want else rt_in if alias else new(B, 3),
           "loss": new(B) if "loss" in want else None, "grad": new(B, n) if "grad" in want else None,
           "groot": new(B, 7) if "groot" in want else None}
    jarr = (ctypes.c_int32 * max(K, 1))(*[int(j) for j in joints])
    rc = _lib.lib().rtg_dof_fit_orient_f32(
        s.model.handle, ptr(bufs["tp"]), ptr(bufs["w"]), jarr if K else None, ptr(R_dev), ptr(bufs["rw"]), K, ptr(rr_in),
        ptr(rt_in), ptr(d_in), B, int(clip), mask, iters, lr, lr_t, lr_q, betas[0], betas[1], eps, step0, ptr(bufs["m"]),
        ptr(bufs["v"]), ptr(bufs["rs"]), *(ptr(out[k]) for k in OUTS), None)
    if status:
        return rc, _lib.lib().rtg_last_error()
    assert rc == 0, _lib.lib().rtg_last_error()
    torch.cuda.synchronize()
    res = {k: _np(x) for k, x in out.items()}
    res.update(m=_np(bufs["m"]), v=_np(bufs["v"]), rs=_np(bufs["rs"]))
    return res


# ------------------------------------------------------------------ link sets and targets
def leaves(s):
    return [j for j in range(s.J) if j not in set(int(p) for p in s.par)]


def link_sets(s, w):
    """K = 1 on a leaf, K = 1 on the root, K = 8 (or every joint of a smaller tree), a parent and its child, and a
    link whose position weight is 0 (with one that has weight)."""
    J = s.J
    if J == 1:
        return {"root": [0]}
    sets = {"leaf": [leaves(s)[-1]], "root": [0]}
    rng = np.random.default_rng(1000 + J)
    sets["k8"] = [int(j) for j in rng.permutation(J)[:8]]
    if 0 not in sets["k8"]:
        sets["k8"][3 % len(sets["k8"])] = 0   # the root among them
    inner = np.flatnonzero(s.par > 0)   # joints whose parent is not the root (none in a star: the root and a child)
    c = int(inner[J // 3]) if len(inner) > J // 3 else J - 1
    sets["parent_child"] = [int(s.par[c]), c]
    z = int(np.flatnonzero(w == 0)[-1]) if (w == 0).any() else J - 1
    sets["zero_weight"] = sorted({z, int(np.flatnonzero(w != 0)[0])}, reverse=True)
    return sets


def targets(B, K, seed):
    """Target rotations of norm 0.5-2, every other row of a frame negated; rot_weight 0.2-2, a third of them 0."""
    rng = np.random.default_rng(seed)
    R = rng.normal(size=(B, K, 4))
    R *= rng.uniform(0.5, 2.0, (B, K, 1)) / np.linalg.norm(R, axis=-1, keepdims=True)
    R[:, ::2] *= -1.0
    rw = rng.uniform(0.2, 2.0, K)
    rw[rng.permutation(K)[: K // 3]] = 0.0
    return R.astype(np.float32), rw.astype(np.float32)


def zero_dofs(s, w, joints):
    """Per DOF (joint j >= 1): no position weight in joint j's strict subtree and no oriented link in its subtree,
    itself included -- the DOFs the launch owes an exact +-0 gradient."""
    pos = s.strict_subtree_weight(w) == 0
    ori = np.zeros(s.J, bool)
    ori[list(joints)] = True
    for j in range(s.J - 1, 0, -1):
        ori[s.par[j]] |= ori[j]
    return pos & ~ori[1:]


# ------------------------------------------------------------------ 1. evaluate
@functools.lru_cache(maxsize=None)
def _case(name, clip):
    s = skel(name)
    x = inputs(s, max(s.batches()), clip, 13 * s.J + clip)
    return s, x, link_sets(s, x["w"])


@functools.lru_cache(maxsize=None)
def _evaluate_reference(name, clip, which, normalised):
    s, x, sets = _case(name, clip)
    joints = sets[which]
    R, rw = targets(len(x["dof"]), len(joints), 17 * s.J + len(joints))
    args = (s, x["dof"], x["rr"], x["rt"], x["tgt"], x["w"], clip)
    tail = (FIT_ROT if normalised else 0, joints, R, rw)
    return R, rw, ref_orient_loss_grad(*args, torch.float64, *tail), ref_orient_loss_grad(*args, torch.float32, *tail)


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_evaluate_against_autograd(gpu, name, clip):
    """iters = 0: loss, grad and grad_root of every link set, all four masks and all five batch sizes against float64
    autograd of the restatement (target norms 0.5-2, every other target negated, a third of the rot_weights 0)."""
    s, x, sets = _case(name, clip)
    for which, joints in sets.items():
        for mask in MASKS:
            R, rw, (l64, g64, r64), (l32, g32, r32) = _evaluate_reference(name, clip, which, bool(mask & FIT_ROT))
            zero = zero_dofs(s, x["w"], joints)
            full = None
            for B in sorted(s.batches(), reverse=True):
                r = ofit(s, x["tgt"][:B], x["w"], x["rr"][:B], x["rt"][:B], x["dof"][:B], clip, mask, joints, R[:B], rw)
                what = f"{name} clip={clip} links={which}{joints} mask={mask} B={B}"
                check_criterion(f"{what} loss", r["loss"], l32[:B], l64[:B])
                check_criterion(f"{what} grad", r["grad"], g32[:B], g64[:B])
                check_criterion(f"{what} grad_t", r["groot"][:, :3], r32[:B, :3], r64[:B, :3])
                check_criterion(f"{what} grad_q", r["groot"][:, 3:], r32[:B, 3:], r64[:B, 3:])
                for k, a in (("dof", x["dof"]), ("rr", x["rr"]), ("rt", x["rt"])):   # iters = 0: the inputs' bits
                    np.testing.assert_array_equal(bits(r[k]), bits(a[:B]), err_msg=f"{what} {k}")
                assert (r["grad"][:, zero] == 0).all()                               # exactly +-0, not noise
                if full is None:
                    full = r
                assert_same_bits(r, {k: a[:B] for k, a in full.items() if a is not None}, what,   # the leading frames
                                 ("loss", "grad", "groot"))
    if s.J > 2:   # the rotation term reaches DOFs the positions leave at exactly 0
        joints = sets["leaf"]
        R, rw, _, _ = _evaluate_reference(name, clip, "leaf", True)
        r = ofit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], clip, 3, joints, R, rw)
        p = pfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], clip, 3)
        assert (p["grad"][:, joints[0] - 1] == 0).all() and (r["grad"][:, joints[0] - 1] != 0).all()


def test_unsupported_and_rejected(gpu):
    s = skel("two")
    x = inputs(s, 3, False, 2)
    R, rw = targets(3, 2, 3)
    a = (s, x["tgt"], None, x["rr"], x["rt"], x["dof"], False, 3)
    rc, msg = ofit(*a, [0, 2], R, rw, status=True)
    assert rc == INVALID and b"rot_joint[1]=2 is outside 0..1" in msg
    rc, msg = ofit(*a, [1, 1], R, rw, status=True)
    assert rc == INVALID and b"listed twice" in msg
    rc, msg = ofit(*a, [0, 1], R, rw, status=True, misalign=True)
    assert rc == INVALID and b"16-byte aligned" in msg
    R9, rw9 = targets(3, 9, 4)
    rc, msg = ofit(skel("hu33"), *(inputs(skel("hu33"), 3, False, 2)[k] for k in ("tgt", "w", "rr", "rt", "dof")), False, 3,
                   list(range(9)), R9, rw9, status=True)
    assert rc == UNSUPPORTED and b"at most 8" in msg
    rc, _ = ofit(s, x["tgt"][:0], None, x["rr"][:0], x["rt"][:0], x["dof"][:0], False, 3, [0, 1], R[:0], rw, status=True)
    assert rc == 0                                                               # B == 0: a no-op


# ------------------------------------------------------------------ 2. bit for bit
@pytest.mark.parametrize("name", ["hu33", "chain64", "tree37", "one"])
def test_k_0_is_the_pose_fit(gpu, name):
    """K = 0 through the new symbol: rtg_dof_fit_root_f32's outputs on all masks, rtg_dof_fit_f32's at mask 0."""
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 41)
    st = random_state(x, 42, 0.1)
    if s.J == 1:
        st["m"] = st["v"] = np.zeros((B, 1), np.float32)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    for mask in MASKS:
        for iters in (0, 8):
            kw = dict(iters=iters, step0=3, lr_t=0.01, lr_q=0.03, **st)
            assert_same_bits(pfit(s, *args, mask, **kw), ofit(s, *args, mask, **kw), f"{name} mask={mask} iters={iters}")
        assert_same_bits(pfit(s, *args, mask, iters=4), ofit(s, *args, mask, iters=4), f"{name} mask={mask} no state", OUTS)
    if s.J > 1:
        old = fit(s, *args, iters=8, step0=3, m=st["m"], v=st["v"])
        assert_same_bits(old, ofit(s, *args, 0, iters=8, step0=3, **st), f"{name} rtg_dof_fit_f32")


@pytest.mark.parametrize("name", ["hu33", "tree37"])
def test_unreached_dofs_keep_their_bits(gpu, name):
    """The +-0 rule on a DOF set computed from the tree: no position weight strictly below and no oriented link at or
    below -> a gradient of exactly +-0 and, from a zero state, the angle's bits after 3 steps.  A link with rot_weight
    0 still counts as oriented.  The two oriented leaves' own DOFs, which positions alone would leave still, move."""
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 31)
    joints = [leaves(s)[0], leaves(s)[-1], int(s.par[leaves(s)[-1]]), 0]
    R, rw = targets(B, len(joints), 32)
    rw[:] = [1.0, 0.5, 0.0, 0.7]
    still = zero_dofs(s, x["w"], joints)
    moves = [joints[0] - 1, joints[1] - 1]
    assert still.any() and (s.strict_subtree_weight(x["w"])[moves] == 0).all() and not still[moves].any()
    for kw in (random_state(x, 32, 0.0), dict()):                                # explicit zero state, and none
        r = ofit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, joints, R, rw, iters=3, **kw)
        np.testing.assert_array_equal(bits(r["dof"][:, still]), bits(x["dof"][:, still]))
        assert (r["grad"][:, still] == 0).all()
        assert (bits(r["dof"][:, moves]) != bits(x["dof"][:, moves])).all()
    # every weight zero and no link: the angles and a fitted t keep their bits (a fitted rotation is renormalised)
    w0 = np.zeros(s.J, np.float32)
    r = ofit(s, x["tgt"], w0, x["rr"], x["rt"], x["dof"], True, 3, iters=3)
    for k in ("dof", "rt"):
        np.testing.assert_array_equal(bits(r[k]), bits(x[k]))
    assert (r["loss"] == 0).all() and (r["grad"] == 0).all() and (r["groot"] == 0).all()


@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_self_consistency(gpu, name):
    s = skel(name)
    F = s.F
    B = 4 * F + 3
    x = inputs(s, B, True, 43)
    st = random_state(x, 44, 0.1)
    joints = link_sets(s, x["w"])["k8"]
    R, rw = targets(B, len(joints), 45)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    ori = (joints, R, rw)
    kw = dict(iters=8, step0=3, lr_t=0.01, lr_q=0.03)
    for mask in MASKS:
        one = ofit(s, *args, mask, *ori, **kw, **st)
        assert all(np.isfinite(a).all() for a in one.values())
        if not mask & FIT_ROT:   # a given block's rows come back as they went in
            np.testing.assert_array_equal(bits(one["rr"]), bits(x["rr"]))
        if not mask & FIT_T:
            np.testing.assert_array_equal(bits(one["rt"]), bits(x["rt"]))
        if mask == 0:
            np.testing.assert_array_equal(bits(one["rs"]), bits(st["rs"]))
        # R against -R, and against a mix of signs
        assert_same_bits(one, ofit(s, *args, mask, joints, -R, rw, **kw, **st), f"-R mask={mask}")
        mixed = R * np.where(np.arange(R.size // 4).reshape(R.shape[:2] + (1,)) % 3 == 0, -1.0, 1.0).astype(np.float32)
        assert_same_bits(one, ofit(s, *args, mask, joints, mixed, rw, **kw, **st), f"mixed signs mask={mask}")
        # two identical launches
        assert_same_bits(one, ofit(s, *args, mask, *ori, **kw, **st), f"repeat mask={mask}")
        # eight launches of one step, carrying (dof, root, m, v, root_state, step)
        c = dict(dof=x["dof"], rr=x["rr"], rt=x["rt"], **st)
        for k in range(8):
            c = ofit(s, x["tgt"], x["w"], c["rr"], c["rt"], c["dof"], True, mask, *ori, **dict(kw, iters=1, step0=3 + k),
                     m=c["m"], v=c["v"], rs=c["rs"])
        assert_same_bits(one, c, f"chained mask={mask}")
        # dof_out, root_rot_out, root_t_out aliasing the inputs
        assert_same_bits(one, ofit(s, *args, mask, *ori, **kw, **st, alias=True), f"alias mask={mask}")
    # a frame of the large launch is that frame run alone (mask 3, from the loop's last round)
    for f in (0, F - 1, 2 * F + 1, B - 1):
        sl = slice(f, f + 1)
        alone = ofit(s, x["tgt"][sl], x["w"], x["rr"][sl], x["rt"][sl], x["dof"][sl], True, 3, joints, R[sl], rw, **kw,
                     **{k: a[sl] for k, a in st.items()})
        assert_same_bits(alone, {k: a[sl] for k, a in one.items()}, f"frame {f}")
    # rot_weight NULL is all ones; outputs are optional one by one
    a = ofit(s, *args, 3, joints, R, None, iters=4)
    assert_same_bits(a, ofit(s, *args, 3, joints, R, np.ones(len(joints), np.float32), iters=4), "rot_weight NULL", OUTS)
    for k in OUTS:
        assert_same_bits(ofit(s, *args, 3, joints, R, None, iters=4, want=(k,)), {k: a[k]}, f"only {k}", (k,))


def test_a_bad_frame_stays_its_own(gpu):
    """A NaN target rotation, a zero target rotation and an inf angle in the middle frame of three tiles: every other
    frame keeps its bits, the bad frame's loss is NaN or finite where the float32 restatement's is."""
    s = skel("hu33")
    B = 3 * s.F
    f = B // 2
    x = inputs(s, B, True, 61)
    joints = list(HU_HANDS_FEET_HEAD) + [0]
    x["R"], rw = targets(B, len(joints), 62)
    rw[:] = np.abs(rw) + 0.3
    args = lambda y: (y["tgt"], y["w"], y["rr"], y["rt"], y["dof"], True, FIT_T | FIT_ROT, joints, y["R"], rw)
    clean = ofit(s, *args(x), iters=3)
    clean0 = ofit(s, *args(x))
    assert all(np.isfinite(a).all() for a in clean.values() if a is not None)
    ok = np.arange(B) != f

    def spoil(which):
        y = {k: a.copy() for k, a in x.items()}
        if "nan" in which:
            y["R"][f, 2, 1] = np.nan
        if "zero" in which:
            y["R"][f, 4] = 0.0
        if "angle" in which:
            y["dof"][f, 2] = np.inf
        return y
    for which in (("nan",), ("zero",), ("angle",), ("nan", "zero", "angle")):
        y = spoil(which)
        bad = ofit(s, *args(y), iters=3)
        for k in OUTS:
            np.testing.assert_array_equal(bits(bad[k][ok]), bits(clean[k][ok]), err_msg=f"{which} {k}")
        bad0 = ofit(s, *args(y))
        for k in ("loss", "grad", "groot"):
            np.testing.assert_array_equal(bits(bad0[k][ok]), bits(clean0[k][ok]), err_msg=f"{which} {k}")
        sl = slice(f, f + 1)
        with np.errstate(all="ignore"), torch.no_grad():
            want = ref_orient_loss(s, y["dof"][sl], y["rr"][sl], y["rt"][sl], y["tgt"][sl], y["w"], True, torch.float32,
                                   FIT_ROT, joints, y["R"][sl], rw).numpy()
        assert np.isnan(bad0["loss"][f]) == np.isnan(want[0]), which
        if not np.isnan(want[0]):   # a zero target: the constant 4 rot_weight; a sum of some hundred non-negative
            # float32 terms, each a few roundings, in both: well within 1e-5 relative
            assert which == ("zero",) and abs(bad0["loss"][f] - want[0]) <= 1e-5 * abs(want[0])
            assert np.isfinite(bad0["grad"][f]).all() and np.isfinite(bad["dof"][f]).all()


# ------------------------------------------------------------------ 3. one Adam step against the formula
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_one_adam_step_against_the_formula(gpu, name):
    """iters = 1 from a random state (v0 >= m0^2, five steps taken) with three different step sizes, against the update
    formula in float64 on the GPU's own iters = 0 gradient of the oriented loss, the hyper-parameters as the launch
    receives them (float32), the rotation renormalised: |delta| <= 8 2^-24 (|old| + |update|) per element, for the
    angles and for the fitted root's 3 + 4 parameters."""
    s = skel(name)
    B, step0 = 4 * s.F + 3, 5
    x = inputs(s, B, True, 71)
    q0 = x["rr"].astype(np.float64)
    x["rr"] = (q0 / np.linalg.norm(q0, axis=-1, keepdims=True)).astype(np.float32)
    st = random_state(x, 72)
    joints = link_sets(s, x["w"])["k8"]
    R, rw = targets(B, len(joints), 73)
    lrs = dict(lr=LR, lr_t=0.03, lr_q=0.01)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, FIT_T | FIT_ROT, joints, R, rw)
    e = ofit(s, *args)
    r = ofit(s, *args, iters=1, step0=step0, **lrs, **st)
    b1, b2, eps = (float(np.float32(h)) for h in (B1, B2, EPS))
    t = step0 + 1

    def step(g, m0, v0, old, lr):
        g, m0, v0, old = (a.astype(np.float64) for a in (g, m0, v0, old))
        m = b1 * m0 + (1 - b1) * g
        v = b2 * v0 + (1 - b2) * g * g
        upd = lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
        return old - upd, upd, m, v
    new, upd, m, v = step(e["grad"], st["m"], st["v"], x["dof"], float(np.float32(lrs["lr"])))
    excess_a = np.abs(r["dof"] - new) / (U * (np.abs(x["dof"].astype(np.float64)) + np.abs(upd)))
    assert (np.abs(r["m"] - m) <= 2 * U * (np.abs(b1 * st["m"].astype(np.float64)) + np.abs((1 - b1) * e["grad"]))).all()
    assert (np.abs(r["v"] - v) <= 2 * U * v).all()
    lr7 = np.array([float(np.float32(lrs["lr_t"]))] * 3 + [float(np.float32(lrs["lr_q"]))] * 4)
    old7 = np.concatenate([x["rt"], x["rr"]], axis=-1)
    new7, upd7, m7, v7 = step(e["groot"], st["rs"][:, :7], st["rs"][:, 7:], old7, lr7)
    new7[:, 3:] /= np.linalg.norm(new7[:, 3:], axis=-1, keepdims=True)
    got7 = np.concatenate([r["rt"], r["rr"]], axis=-1)
    excess_r = np.abs(got7 - new7) / (U * (np.abs(old7.astype(np.float64)) + np.abs(upd7)))
    print(f"{name}: oriented Adam step, max |delta| / (2^-24 (|old| + |update|)): angles {excess_a.max():.2f}, "
          f"t {excess_r[:, :3].max():.2f}, q {excess_r[:, 3:].max():.2f} (bound 8)")
    assert excess_a.max() <= 8 and excess_r.max() <= 8
    assert (np.abs(r["rs"][:, :7] - m7) <= 2 * U * (np.abs(b1 * st["rs"][:, :7].astype(np.float64)) + np.abs((1 - b1) * e["groot"]))).all()
    assert (np.abs(r["rs"][:, 7:] - v7) <= 2 * U * v7).all()
    assert np.abs(upd).max() > 1e-3 and np.abs(upd7[:, :3]).max() > 1e-3 and np.abs(upd7[:, 3:]).max() > 1e-3


# ------------------------------------------------------------------ 4. outcome
@pytest.fixture(scope="module")
def outcome():
    """The pinned recipe of tests/test_pose_fit_host.py with the rotations of both hands, both feet and the head as
    the same FK gives them (reachable): the recipe's own draws replayed for the pose behind its targets.  The
    reference loop after 32 steps in float64 and float32."""
    s, x = recipe()
    rng = np.random.default_rng(5)
    B = 64
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    q_true, t_true = unit(rng.normal(size=(B, 4))), rng.normal(0, 0.3, (B, 3))
    truth = rng.uniform(s.lo, s.hi, (B, s.J - 1)).astype(np.float32)
    f64 = lambda a: _t(a, torch.float64)
    with torch.no_grad():
        g_rot, g_pos = dof_fk(f64(truth), f64(q_true), f64(t_true), [int(p) for p in s.par], f64(s.lt), s.axis, f64(s.lo),
                              f64(s.hi))
    assert np.array_equal(g_pos.numpy().astype(np.float32), x["tgt"])            # the recipe's pose
    joints = list(HU_HANDS_FEET_HEAD)
    R = g_rot.numpy()[:, joints].astype(np.float32)
    args = (s, x["start"], x["q0"], x["t0"], x["tgt"], x["w"], True)
    ref = {dt: ref_orient_fit(*args, dt, FIT_T | FIT_ROT, joints, R, None, 32) for dt in (torch.float64, torch.float32)}
    return skel("hu33"), s, x, joints, R, ref


def test_outcome_against_the_torch_loop(gpu, outcome):
    hu, s, x, joints, R, ref = outcome
    (l64, _, q64, t64), (l32, _, q32, t32) = ref[torch.float64], ref[torch.float32]
    args = (x["tgt"], None, x["q0"], x["t0"], x["start"], True, FIT_T | FIT_ROT)
    r = ofit(hu, *args, joints, R, None, iters=32)
    p = pfit(hu, *args, iters=32)
    err = lambda o: orient_error(s, o["dof"], o["rr"], o["rt"], True, joints, R)
    e0 = orient_error(s, x["start"], x["q0"], x["t0"], True, joints, R).mean()
    er, ep = err(r).mean(), err(p).mean()
    print(f"32 steps: mean loss GPU {r['loss'].mean():.4f}, reference {l64.mean():.4f}; mean orientation error of the "
          f"five links: start {e0:.4f} rad, oriented fit {er:.4f} rad, position-only fit {ep:.4f} rad")
    check_criterion("outcome 32 steps loss", r["loss"], l32, l64)
    check_criterion("outcome 32 steps root_rot", r["rr"], q32, q64)
    check_criterion("outcome 32 steps root_t", r["rt"], t32, t64)
    assert er < ep
    leaf_dofs = [j - 1 for j in joints if j in leaves(hu)]                       # the toes' and the neck's own DOFs
    assert len(leaf_dofs) == 3
    np.testing.assert_array_equal(bits(p["dof"][:, leaf_dofs]), bits(x["start"][:, leaf_dofs]))   # positions cannot
    assert (bits(r["dof"][:, leaf_dofs]) != bits(x["start"][:, leaf_dofs])).all()                 # orientations do


# ------------------------------------------------------------------ 5. the Python surface
def test_python_entry_points(gpu):
    from rtg import ops
    from robot_kinematics_model import RobotZeroPose
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    s = skel("hu33")
    B = 19
    x = inputs(s, B, True, 51)
    joints = list(HU_HANDS_FEET_HEAD)
    R, rw = targets(B, len(joints), 52)
    o = dict(rot_joints=joints, target_rot=R, rot_weight=rw)
    # ops.pose_loss: the evaluate-only launch under autograd, in all three inputs; a cotangent scales row by row
    for normalise, mask in ((True, FIT_ROT), (False, 0)):
        r = ofit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask, joints, R, rw)
        a, q, t = (_dev(x[k]).requires_grad_(True) for k in ("dof", "rr", "rt"))
        loss = ops.pose_loss(s.model, a, q, t, x["tgt"], weight=x["w"], clip=True, normalize_root=normalise, **o)
        assert loss.shape == (B,) and loss.grad_fn is not None
        np.testing.assert_array_equal(bits(_np(loss)), bits(r["loss"]))
        loss.sum().backward()
        np.testing.assert_array_equal(bits(_np(a.grad)), bits(r["grad"]))
        np.testing.assert_array_equal(bits(_np(t.grad)), bits(r["groot"][:, :3]))
        np.testing.assert_array_equal(bits(_np(q.grad)), bits(r["groot"][:, 3:]))
        with torch.no_grad():
            plain = ops.pose_loss(s.model, a, q, t, x["tgt"], weight=x["w"], clip=True, normalize_root=normalise, **o)
        assert plain.grad_fn is None and torch.equal(plain, loss.detach())
        a2, q2, t2 = (_dev(x[k]).requires_grad_(True) for k in ("dof", "rr", "rt"))
        c = torch.linspace(-2.0, 3.0, B, device="cuda")
        (ops.pose_loss(s.model, a2, q2, t2, x["tgt"], weight=x["w"], clip=True, normalize_root=normalise, **o) * c).sum().backward()
        assert torch.equal(a2.grad, _dev(r["grad"]) * c[:, None]) and torch.equal(q2.grad, _dev(r["groot"][:, 3:]) * c[:, None])
        assert torch.equal(t2.grad, _dev(r["groot"][:, :3]) * c[:, None])
    # shapes (..., K, 4): a (2, B/2, ...) batch is the flat one
    flat = ops.pose_loss(s.model, x["dof"], x["rr"], x["rt"], x["tgt"], weight=x["w"], clip=True, **o)
    two = ops.pose_loss(s.model, x["dof"][:18].reshape(2, 9, -1), x["rr"][:18].reshape(2, 9, 4), x["rt"][:18].reshape(2, 9, 3),
                        x["tgt"][:18].reshape(2, 9, -1, 3), weight=x["w"], clip=True, rot_joints=joints,
                        target_rot=R[:18].reshape(2, 9, -1, 4), rot_weight=rw)
    assert two.shape == (2, 9) and torch.equal(two.reshape(-1), flat[:18])
    # ops.pose_fit: the launch, its named tuple, and the chain 4 + 4 = 8
    kw = dict(weight=x["w"], lr=LR, lr_root_t=0.01, clip=True)
    r8 = ofit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, joints, R, rw, iters=8, lr_t=0.01)
    p8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, return_grad=True, **kw, **o)
    for k, a in (("dof", p8.dof), ("rr", p8.root_rot), ("rt", p8.root_t), ("loss", p8.loss), ("grad", p8.grad),
                 ("groot", p8.grad_root)):
        np.testing.assert_array_equal(bits(_np(a)), bits(r8[k]), err_msg=k)
    p4 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, **kw, **o)
    q8 = ops.pose_fit(s.model, x["tgt"], p4.root_rot, p4.root_t, p4.dof, iters=4, state=p4.state, **kw, **o)
    assert all(torch.equal(a, b) for a, b in zip(q8[:4] + q8.state[:3], p8[:4] + p8.state[:3]))
    # none of the keywords: the old functions' bits
    old = pfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, iters=8, lr_t=0.01)
    n8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, **kw)
    for k, a in (("dof", n8.dof), ("rr", n8.root_rot), ("rt", n8.root_t), ("loss", n8.loss)):
        np.testing.assert_array_equal(bits(_np(a)), bits(old[k]), err_msg=k)
    oldf = fit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, iters=8)
    nf = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=8, lr=LR, clip=True)
    np.testing.assert_array_equal(bits(_np(nf[0])), bits(oldf["dof"]))
    np.testing.assert_array_equal(bits(_np(nf[1])), bits(oldf["loss"]))
    # ops.dof_fit / keypoint_loss with the keywords: the new symbol with the root given
    g8 = ofit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, joints, R, rw, iters=8)
    d8 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=8, lr=LR, clip=True,
                     return_grad=True, **o)
    np.testing.assert_array_equal(bits(_np(d8[0])), bits(g8["dof"]))
    np.testing.assert_array_equal(bits(_np(d8[1])), bits(g8["loss"]))
    np.testing.assert_array_equal(bits(_np(d8[3])), bits(g8["grad"]))
    d4 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=4, lr=LR, clip=True, **o)
    c8 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], d4[0], weight=x["w"], iters=4, lr=LR, clip=True, state=d4[2], **o)
    assert torch.equal(c8[0], d8[0]) and c8[2][2] == 8
    g0 = ofit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, joints, R, rw)
    a = _dev(x["dof"]).requires_grad_(True)
    kl = ops.keypoint_loss(s.model, a, x["tgt"], x["rr"], x["rt"], weight=x["w"], clip=True, **o)
    kl.sum().backward()
    np.testing.assert_array_equal(bits(_np(kl)), bits(g0["loss"]))
    np.testing.assert_array_equal(bits(_np(a.grad)), bits(g0["grad"]))
    # what ops refuses before the C ABI sees a pointer
    for bad in (dict(o, rot_joints=[20, 20, 6, 12, 32]), dict(o, rot_joints=[20, 29, 6, 12, 33]), dict(o, target_rot=R[:, :4]),
                dict(o, target_rot=R[:5]), dict(o, rot_weight=rw[:3]), dict(rot_joints=joints), dict(target_rot=R),
                dict(rot_joints=list(range(9)), target_rot=np.zeros((B, 9, 4), np.float32)),
                dict(o, rot_joints=[0.5, 1, 2, 3, 4]), dict(o, target_rot=R.astype(np.int32))):
        with pytest.raises(ValueError):
            ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=1, **kw, **bad)
    # the drop-in: (L, K, 4) targets, links by name or index, results on the inputs' device
    hu = HuForwardModel(RobotZeroPose.from_asset("hu").skeleton_tree)
    names = ["left_wrist_yaw_link", "right_wrist_yaw_link", "left_toe_link", "right_toe_link", "neck_link"]
    assert [hu.node_names.index(n) for n in names] == joints
    tgt, rt, rr = torch.from_numpy(x["tgt"]), torch.from_numpy(x["rt"]), torch.from_numpy(x["rr"][:, None])
    want = ops.pose_fit(hu._model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, lr=LR, clip=True, **o)
    for links in (names, joints, names[:2] + joints[2:]):
        ang, t, q, loss, state = hu.fit_pose(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), iters=8, lr=LR,
                                             target_rotations=torch.from_numpy(R), rotation_links=links,
                                             rotation_weight=torch.from_numpy(rw))
        assert ang.shape == (B, 32, 1) and q.shape == (B, 1, 4) and all(a.device.type == "cpu" for a in (ang, t, q, loss))
        assert torch.equal(ang[..., 0], want.dof.cpu()) and torch.equal(q[:, 0], want.root_rot.cpu())
        assert torch.equal(t, want.root_t.cpu()) and torch.equal(loss, want.loss.cpu())
    ang, loss, state = hu.fit_keypoints(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), weight=x["w"], iters=8, lr=LR,
                                        target_rotations=torch.from_numpy(R), rotation_links=names,
                                        rotation_weight=torch.from_numpy(rw))
    hd8 = ops.dof_fit(hu._model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=8, lr=LR, clip=True, **o)
    assert torch.equal(ang[..., 0], hd8[0].cpu()) and torch.equal(loss, hd8[1].cpu())

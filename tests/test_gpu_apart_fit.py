"""GPU: the pose fit with keep-apart spheres and a floor (rtg_dof_fit_apart_f32: the prior launch's loss plus
sum_p pair_weight[p] max(0, r_a + r_b + margin - |c_a - c_b|)^2 over pairs of spheres riding on links and
floor_weight max(0, r_s + h0 - n . c_s)^2 over the spheres held above a plane) against the torch restatement of
tests/test_apart_fit_host.py on the CPU in float64 and float32.

The criterion is the project's own, per tensor (tests/test_gpu_dof_fit.py check_criterion): E(x) = max|x - x64| /
max|x64|, and E(gpu) <= 8 max(E(restatement f32), 2^-24).  The inputs come from the host file's generator, which keeps
every term at least 1e-3 m from its hinge on the float64 reference (asserted there), so the three evaluations agree on
which terms are active.  One Adam step is checked on its own against the update formula, and everything the header
promises bit for bit (nothing given is the prior launch, chained launches, batch and tile independence, repeatability,
a bad frame staying in its rows, the DOFs a zero-offset sphere must not reach) is checked bit for bit.  The two outcome
recipes of the host file are replayed on the GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_apart_fit_host import (GPU_SKELS, RefApartFit, _apart, apart_case, floor_recipe, gpu_case, hands_recipe, penetration,
                                 ref_apart_loss_grad, ref_outcome, spec, to_ops)
from test_gpu_dof_fit import bits, check_criterion, inputs, skel
from test_gpu_orient_fit import targets, zero_dofs
from test_gpu_pose_fit import MASKS, OUTS, U, _dev, _np, assert_same_bits, random_state
from test_gpu_prior_fit import _hu_on, link_set, prfit, priors
from test_orient_fit_host import INVALID
from test_pose_fit_host import B1, B2, EPS, FIT_ROT, FIT_T, LR
from test_prior_fit_host import PROJECT

pytestmark = pytest.mark.gpu

STATE = OUTS + ("m", "v", "rs")


# ------------------------------------------------------------------ the launch, straight through the C ABI
def struct_of(ap):
    """The host file's spec as an rtg_fit_apart -> (struct, the arrays it points into)."""
    return _apart(S=len(ap["links"]), sphere_link=ap["links"], sphere=ap["spheres"], Pn=len(ap["pairs"]),
                  pair=ap["pairs"] if len(ap["pairs"]) else None, pair_weight=ap["pw"] if len(ap["pairs"]) else None,
                  margin=ap["margin"], plane=ap["plane"], floor_mask=ap["mask"], floor_weight=ap["wf"])


def apfit(s, tgt, w, rr, rt, dof, clip, mask, ap, joints=(), R=None, rw=None, prior=None, pw=None, flags=0, iters=0, lr=LR,
          lr_t=LR, lr_q=LR, betas=(B1, B2), eps=EPS, step0=0, m=None, v=None, rs=None, want=OUTS, status=False):
    """rtg_dof_fit_apart_f32 on host arrays -> dict of host arrays (dof, rr, rt, loss, grad, groot, m, v, rs).
    ap: a spec of the host file, None for a NULL struct, or a ready (struct, arrays) pair."""
    from rtg import _lib
    from rtg.runtime import ptr
    B, n, K = tgt.shape[0], s.J - 1, len(joints)
    d_in, rr_in, rt_in = _dev(dof), _dev(rr), _dev(rt)
    bufs = dict(tp=_dev(tgt), w=_dev(w), m=_dev(m), v=_dev(v), rs=_dev(rs), rw=_dev(rw), pw=_dev(pw), p=_dev(prior))
    R_dev = None if R is None else _dev(np.asarray(R, np.float32).reshape(B, K, 4))
    new = lambda *shape: torch.full(shape, 7.0, device="cuda")
    out = {"dof": new(B, n) if "dof" in want else None, "rr": new(B, 4) if "rr" in want else None,
           "rt": new(B, 3) if "rt" in want else None, "loss": new(B) if "loss" in want else None,
           "grad": new(B, n) if "grad" in want else None, "groot": new(B, 7) if "groot" in want else None}
    st, keep = (None, None) if ap is None else ap if isinstance(ap, tuple) else struct_of(ap)
    jarr = (ctypes.c_int32 * max(K, 1))(*[int(j) for j in joints])
    rc = _lib.lib().rtg_dof_fit_apart_f32(
        s.model.handle, ptr(bufs["tp"]), ptr(bufs["w"]), jarr if K else None, ptr(R_dev), ptr(bufs["rw"]), K, ptr(bufs["p"]),
        ptr(bufs["pw"]), flags, ptr(rr_in), ptr(rt_in), ptr(d_in), B, int(clip), mask, iters, lr, lr_t, lr_q, betas[0],
        betas[1], eps, step0, ptr(bufs["m"]), ptr(bufs["v"]), ptr(bufs["rs"]), *(ptr(out[k]) for k in OUTS),
        None if st is None else ctypes.byref(st), None)
    if status:
        return rc, _lib.lib().rtg_last_error()
    assert rc == 0, _lib.lib().rtg_last_error()
    torch.cuda.synchronize()
    res = {k: _np(x) for k, x in out.items()}
    res.update(m=_np(bufs["m"]), v=_np(bufs["v"]), rs=_np(bufs["rs"]))
    return res


# ------------------------------------------------------------------ 1. evaluate
# (K, prior, offsets, plane): every option on and off, with each other option in both states
CONFIGS = ((0, False, False, True), (8, True, True, True), (0, True, True, False), (8, False, False, False))


def _config(name, cfg):
    K, prior, offsets, plane = cfg
    if name == "one":
        plane = True   # spheres on one rigid link keep their distances: without a floor the term has no gradient in the
                       # root rotation, float64 autograd leaves rounding noise there, and a relative error means nothing
                       # (and with zero offsets they share one centre: only a floor has something to hold)
    return K, prior, offsets, plane


@functools.lru_cache(maxsize=None)
def _evaluate_reference(name, clip, cfg, normalised):
    K, prior, offsets, plane = _config(name, cfg)
    s, x, ap = gpu_case(name, clip, offsets, plane)
    joints = link_set(s, x["w"], K)
    R, rw = targets(len(x["dof"]), len(joints), 29 * s.J + K)
    p, pw = priors(s, x["dof"], 23 * s.J + clip) if prior else (None, None)
    rest = (x["tgt"], x["w"], clip)
    tail = (FIT_ROT if normalised else 0, joints, R, rw, p, pw, ap)
    return (joints, R, rw, p, pw, ap, ref_apart_loss_grad(s, x["dof"], x["rr"], x["rt"], *rest, torch.float64, *tail),
            ref_apart_loss_grad(s, x["dof"], x["rr"], x["rt"], *rest, torch.float32, *tail))


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", GPU_SKELS)
def test_evaluate_against_autograd(gpu, name, clip):
    """iters = 0: loss, grad and grad_root against float64 autograd of the restatement -- K = 0 and 8 links, the prior
    on and off, zero and non-zero offsets, the plane on and off, all four masks and all five batch sizes; the inputs'
    bits come back, and a smaller batch gives the bits of the largest's leading frames."""
    for cfg in CONFIGS:
        for mask in MASKS:
            joints, R, rw, p, pw, ap, (l64, g64, r64), (l32, g32, r32) = _evaluate_reference(name, clip, cfg, bool(mask & FIT_ROT))
            s, x, _ = gpu_case(name, clip, *_config(name, cfg)[2:])
            st = struct_of(ap)
            full = None
            for B in sorted(s.batches(), reverse=True):
                r = apfit(s, x["tgt"][:B], x["w"], x["rr"][:B], x["rt"][:B], x["dof"][:B], clip, mask, st, joints, R[:B], rw,
                          None if p is None else p[:B], pw, PROJECT if B % 2 else 0)
                what = f"{name} clip={clip} cfg={cfg} mask={mask} B={B}"
                check_criterion(f"{what} loss", r["loss"], l32[:B], l64[:B])
                check_criterion(f"{what} grad", r["grad"], g32[:B], g64[:B])
                check_criterion(f"{what} grad_t", r["groot"][:, :3], r32[:B, :3], r64[:B, :3])
                check_criterion(f"{what} grad_q", r["groot"][:, 3:], r32[:B, 3:], r64[:B, 3:])
                for k, a in (("dof", x["dof"]), ("rr", x["rr"]), ("rt", x["rt"])):   # iters = 0: the inputs' bits
                    np.testing.assert_array_equal(bits(r[k]), bits(a[:B]), err_msg=f"{what} {k}")
                if full is None:
                    full = r
                assert_same_bits(r, {k: a[:B] for k, a in full.items() if a is not None}, what, ("loss", "grad", "groot"))
    # pair_weight NULL is all ones
    s, x, ap = gpu_case(name, clip, True, True)
    if len(ap["pairs"]):
        args = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], clip, 3)
        ones = dict(ap, pw=np.ones(len(ap["pairs"]), np.float32))
        assert_same_bits(apfit(*args, dict(ap, pw=None)), apfit(*args, ones), f"{name} pair_weight NULL", OUTS)


# ------------------------------------------------------------------ 2. one Adam step against the formula
@pytest.mark.parametrize("project", [False, True])
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_one_adam_step_against_the_formula(gpu, name, project):
    """iters = 1 from a random state (v0 >= m0^2, five steps taken) against the update formula in float64 on the GPU's
    own iters = 0 gradient (the term in it), the hyper-parameters as the launch receives them (float32): |delta| <=
    8 2^-24 (|old| + |update|) per element; projected: inside the limits, on a limit's bits where the formula leaves the
    angle outside by more than that bound."""
    s, x, ap = gpu_case(name, True, True, True)
    x = dict(x)
    B, step0 = len(x["dof"]), 5
    st = random_state(x, 83)
    p, pw = priors(s, x["dof"], 84)
    args = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, FIT_T | FIT_ROT, ap, (), None, None, p, pw,
            PROJECT if project else 0)
    e = apfit(*args)
    r = apfit(*args, iters=1, step0=step0, **st)
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
        print(f"{name}: Adam step with the term, max |delta| / (2^-24 (|old| + |update|)) {excess.max():.2f} (bound 8)")
        assert excess.max() <= 8
        return
    lo, hi = s.lo.astype(np.float64), s.hi.astype(np.float64)
    below, above, inside = new < lo - tol, new > hi + tol, (new > lo + tol) & (new < hi - tol)
    assert below.sum() > B and above.sum() > B
    np.testing.assert_array_equal(bits(r["dof"][below]), bits(np.broadcast_to(s.lo, new.shape)[below]))
    np.testing.assert_array_equal(bits(r["dof"][above]), bits(np.broadcast_to(s.hi, new.shape)[above]))
    assert (np.abs(r["dof"] - new)[inside] <= tol[inside]).all()
    assert ((r["dof"] >= s.lo) & (r["dof"] <= s.hi)).all()


# ------------------------------------------------------------------ 3. nothing given is the prior launch
@pytest.mark.parametrize("name", ["hu33", "chain64", "one"])
def test_nothing_given_is_the_prior_launch(gpu, name):
    """apart NULL, S = 0, spheres without a pair or a floor, a plane without mask bits: rtg_dof_fit_prior_f32's bits on
    every output and state row, K = 0 and 8, iters 0 and 4.  Every pair apart and no plane: its outputs as numbers."""
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 91)
    st = random_state(x, 92, 0.1)
    if s.J == 1:
        st["m"] = st["v"] = np.zeros((B, 1), np.float32)
    p, pw = priors(s, x["dof"], 93)
    ap = apart_case(s, x, True, 94, True, s.J == 1)
    none = [None, spec([], np.zeros((0, 4))), dict(ap, pairs=np.zeros((0, 2), np.int32), pw=None, plane=None, mask=0),
            dict(ap, pairs=np.zeros((0, 2), np.int32), pw=None, plane=np.array([0, 0, 1, 9.0], np.float32), mask=0)]
    far = dict(ap, spheres=np.concatenate([ap["spheres"][:, :3], np.zeros((len(ap["links"]), 1), np.float32)], axis=1),
               margin=-1e3, plane=None, mask=0)
    for K in (0, 8):
        joints = link_set(s, x["w"], K)
        R, rw = targets(B, len(joints), 95)
        for flags, prior in ((0, None), (PROJECT, p)):
            for mask in (0, 3):
                for iters in (0, 4):
                    a = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask)
                    kw = dict(joints=joints, R=R, rw=rw, prior=prior, pw=None if prior is None else pw, flags=flags, iters=iters,
                              step0=3, lr_t=0.01, **st)
                    want = prfit(*a, **kw)
                    for i, q in enumerate(none):
                        assert_same_bits(want, apfit(*a, q, **kw), f"{name} K={K} flags={flags} mask={mask} iters={iters} none[{i}]")
                    if len(far["pairs"]):
                        got = apfit(*a, far, **kw)
                        for k in STATE:
                            assert np.array_equal(want[k], got[k]), f"{name} K={K} flags={flags} mask={mask} iters={iters} {k}"


# ------------------------------------------------------------------ 4. self-consistency
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_self_consistency(gpu, name):
    """Two launches give the same bits; eight launches of one step that carry the state equal one launch of eight; a
    frame of the large launch is that frame run alone; outputs are optional one by one."""
    s, x, ap = gpu_case(name, True, True, True)
    B, F = len(x["dof"]), s.F
    st = random_state(x, 122, 0.1)
    p, pw = priors(s, x["dof"], 123)
    stc = struct_of(ap)
    kw = dict(iters=8, step0=3, lr_t=0.01, lr_q=0.03)
    for K, flags in ((0, PROJECT), (8, 0)):
        joints = link_set(s, x["w"], K)
        R, rw = targets(B, len(joints), 124)
        ori = (joints, R, rw)
        for mask in (0, 3):
            a = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask, stc, *ori, p, pw, flags)
            one = apfit(*a, **kw, **st)
            assert all(np.isfinite(v).all() for v in one.values())
            assert_same_bits(one, apfit(*a, **kw, **st), f"repeat K={K} mask={mask}")
            c = dict(dof=x["dof"], rr=x["rr"], rt=x["rt"], **st)
            for k in range(8):
                c = apfit(s, x["tgt"], x["w"], c["rr"], c["rt"], c["dof"], True, mask, stc, *ori, p, pw, flags,
                          **dict(kw, iters=1, step0=3 + k), m=c["m"], v=c["v"], rs=c["rs"])
            assert_same_bits(one, c, f"chained K={K} mask={mask}")
        for f in (0, F - 1, 2 * F + 1, B - 1):   # mask 3, from the loop's last round
            sl = slice(f, f + 1)
            alone = apfit(s, x["tgt"][sl], x["w"], x["rr"][sl], x["rt"][sl], x["dof"][sl], True, 3, stc, joints, R[sl], rw, p[sl],
                          pw, flags, **kw, **{k: v[sl] for k, v in st.items()})
            assert_same_bits(alone, {k: v[sl] for k, v in one.items()}, f"frame {f} K={K}")
    a = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, stc, iters=4)
    for k in OUTS:
        assert_same_bits(apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, stc, iters=4, want=(k,)), {k: a[k]},
                         f"only {k}", (k,))
    # without the term's gradient the fit goes elsewhere: the term is in the steps, not only in the loss
    assert not np.array_equal(a["dof"], prfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, iters=4)["dof"])


# ------------------------------------------------------------------ 5. a bad frame stays its own
def test_a_bad_frame_stays_its_own(gpu):
    """A NaN target row or a NaN angle in the last frame of a tile or the first of the next: that frame's loss and
    gradient are NaN, every other frame keeps its bits, at iters 0 and after 3 steps."""
    s, x, ap = gpu_case("hu33", True, True, True)
    B = len(x["dof"])
    stc = struct_of(ap)
    args = lambda y: (s, y["tgt"], y["w"], y["rr"], y["rt"], y["dof"], True, FIT_T | FIT_ROT, stc)
    clean, clean0 = apfit(*args(x), iters=3), apfit(*args(x))
    assert all(np.isfinite(a).all() for a in clean.values() if a is not None)
    j = int(np.flatnonzero(x["w"] > 0)[-1])
    for f in (s.F - 1, s.F):
        ok = np.arange(B) != f
        for which in ("target", "angle"):
            y = {k: a.copy() for k, a in x.items()}
            if which == "target":
                y["tgt"][f, j] = np.nan
            else:
                y["dof"][f, 2] = np.nan
            bad, bad0 = apfit(*args(y), iters=3), apfit(*args(y))
            for k in OUTS:
                np.testing.assert_array_equal(bits(bad[k][ok]), bits(clean[k][ok]), err_msg=f"{which} {f} {k}")
            for k in ("loss", "grad", "groot"):
                np.testing.assert_array_equal(bits(bad0[k][ok]), bits(clean0[k][ok]), err_msg=f"{which} {f} {k}")
            assert np.isnan(bad0["loss"][f]) and np.isnan(bad0["grad"][f]).any() and np.isnan(bad["dof"][f]).any(), (which, f)


def test_coincident_centres_add_a_constant_and_no_gradient(gpu):
    """Hu's link 21 has a zero offset from link 20: two zero-offset spheres there share their centre in every frame.
    The pair adds the finite pair_weight (r_a + r_b + margin)^2 to the loss and no gradient: grad and grad_root equal
    the launch's without the pair as numbers.  The loss: the constant joins one lane's part, and the at most 5 additions
    from there to the frame's loss each round to half an ulp of at most the loss, in either launch: 2 * 5 * 2^-24 * loss,
    taken as 16 * 2^-24 * loss -- some 1e-5 against a constant of 0.016."""
    s = skel("hu33")
    assert int(s.par[21]) == 20 and not s.lt[21].any()
    B = s.F + 3
    x = inputs(s, B, True, 171)
    ap = spec([20, 21], [[0, 0, 0, 0.03], [0, 0, 0, 0.04]], [(1, 0)], [2.5], margin=0.01)
    a = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3)
    got, want = apfit(*a, ap), prfit(*a)
    const = 2.5 * (0.03 + 0.04 + 0.01) ** 2
    assert np.isfinite(got["loss"]).all() and np.isfinite(got["grad"]).all() and np.isfinite(got["groot"]).all()
    assert (np.abs(got["loss"].astype(np.float64) - (want["loss"].astype(np.float64) + const)) <= 16 * U * want["loss"]).all()
    assert np.array_equal(got["grad"], want["grad"]) and np.array_equal(got["groot"], want["groot"])


# ------------------------------------------------------------------ 6. what a zero-offset sphere must not reach
def test_zero_offset_spheres_leave_unobserved_leaf_dofs_alone(gpu):
    """Spheres with zero offsets on Hu's wrists and grippers, every one of them pushed by a floor far above: a DOF with
    no position weight and no sphere strictly below it keeps a gradient of exactly +-0 -- the leaf links' own DOFs among
    them, whose links carry spheres -- and from a zero state its bits.  An offset on the left gripper's sphere gives that
    link's own DOF a gradient."""
    s = skel("hu33")
    B = s.F + 3
    x = inputs(s, B, True, 181)
    links = [19, 21, 22, 28, 30, 31]
    x["w"][[20, 21, 22, 29, 30, 31]] = 0.0
    still = zero_dofs(s, x["w"], [])
    below = np.zeros(s.J, bool)   # a sphere in joint j's strict subtree
    for j in links:
        q = int(s.par[j])
        while q >= 0:
            below[q] = True
            q = int(s.par[q])
    still &= ~below[1:]
    own = [j - 1 for j in (21, 22, 30, 31)]   # the leaves' own DOFs
    assert still[own].all() and still.sum() >= 6
    zero = spec(links, [[0, 0, 0, 0.05]] * 6, [(0, 3), (1, 4)], plane=[0, 0, 1, 9.0], mask=0x3F, wf=0.7)
    a = (s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3)
    e = apfit(*a, zero)
    assert (e["grad"][:, still] == 0).all()
    assert not np.array_equal(e["grad"], prfit(*a)["grad"])     # the spheres do push: the arms' DOFs feel it
    r = apfit(*a, zero, iters=3)
    np.testing.assert_array_equal(bits(r["dof"][:, still]), bits(x["dof"][:, still]))
    off = dict(zero, spheres=zero["spheres"].copy())
    off["spheres"][1, :3] = (0.08, 0.02, 0.0)
    g = apfit(*a, off)
    assert (np.abs(g["grad"][:, 20]) > 0).all()                # joint 21's own angle
    rest = still.copy()
    rest[20] = False
    assert (g["grad"][:, rest] == 0).all()


# ------------------------------------------------------------------ 7. outcomes on the two pinned recipes
@pytest.mark.parametrize("which", ["hands", "floor"])
def test_outcome(gpu, which):
    """The host file's recipes on the GPU: the deepest penetration with the term is at most half of that without (the
    float64 loop's quarter leaves the margin for the float32 path), and the final losses meet the criterion against the
    float64 and float32 loops."""
    _, x = hands_recipe() if which == "hands" else floor_recipe()
    s = skel("hu33")
    ref64 = ref_outcome(which)
    pen = {}
    for on in (False, True):
        ap = x["ap"] if on else None
        r = apfit(s, x["tgt"], x["w"], x["q"], x["t"], x["start"], True, x["fit_root"], ap, flags=PROJECT, iters=x["iters"],
                  lr=x["lr"])
        pen[on] = penetration(s, r["dof"], x["q"], x["t"], True, x["fit_root"], x["ap"]).max()
        l32 = RefApartFit(s, x["start"], x["q"], x["t"], x["w"], True, torch.float32, x["fit_root"], ap, project=True,
                          lr=x["lr"]).run(x["tgt"], x["iters"]).result(x["tgt"])[0]
        check_criterion(f"{which} recipe, term {'on' if on else 'off'}: final loss", r["loss"], l32, ref64[on][1])
        assert ((r["dof"] >= s.lo) & (r["dof"] <= s.hi)).all()
    print(f"{which} recipe on the GPU: deepest penetration without the term {pen[False]:.4f} m, with it {pen[True]:.4f} m "
          f"({pen[False] / pen[True]:.1f} times; bound 2; float64 loop {ref64[False][0].max() / ref64[True][0].max():.1f})")
    assert pen[True] <= 0.5 * pen[False]


def test_fit_motion_with_the_term_is_its_fit_pose_rounds(gpu):
    """fit_motion(..., apart=...) on the hands recipe, 3 rounds of 16 steps (the recipe's 48, by which the hands have met):
    the bits of the three fit_pose launches it stands for, the neighbour-mean prior refreshed in between; with
    smooth_weight = 0 those of one fit_pose of 48 steps, which differ from the fit without the term."""
    _, x = hands_recipe()
    s = skel("hu33")
    hu = _hu_on(s)
    ap = to_ops(s, x["ap"])
    tgt, t, q = (torch.from_numpy(x[k]) for k in ("tgt", "t", "q"))
    q, start = q[:, None], torch.from_numpy(x["start"][..., None])
    kw = dict(weight=x["w"], lr=x["lr"], fit_root_t=False, fit_root_rot=False, clip_angles=True, project_angles=True, apart=ap)
    res = hu.fit_motion(tgt, t, q, start, smooth_weight=0.1, rounds=3, iters=16, **kw)
    a, tt, qq, state = start, t, q, None
    for _ in range(3):
        prior = 0.5 * (torch.cat([a[:1], a[:-1]]) + torch.cat([a[1:], a[-1:]]))
        a, tt, qq, loss, state = hu.fit_pose(tgt, tt, qq, a, iters=16, state=state, prior_angles=prior, prior_weight=0.1, **kw)
    for u, v in zip(res[:4] + res[4][:3], (a, tt, qq, loss) + state[:3]):
        assert torch.equal(u, v)
    assert res[4][3] == 48
    one = hu.fit_pose(tgt, t, q, start, iters=48, **kw)
    flat = hu.fit_motion(tgt, t, q, start, smooth_weight=0.0, rounds=3, iters=16, **kw)
    for u, v in zip(flat[:4] + flat[4][:3], one[:4] + one[4][:3]):
        assert torch.equal(u, v)
    bare = hu.fit_pose(tgt, t, q, start, iters=48, **dict(kw, apart=None))
    assert not torch.equal(bare[0], one[0])


# ------------------------------------------------------------------ 8. what is rejected, and the Python surface
def test_rejected(gpu):
    s = skel("two")
    x = inputs(s, 3, False, 2)
    ok = spec([0, 1, 1], [[0, 0, 0, 0.1], [0.1, 0, 0, 0.05], [0, 0, 0, 0.02]], [(0, 1), (2, 0)], plane=[0, 0, 1, 0.0], mask=5)
    a = (s, x["tgt"], None, x["rr"], x["rt"], x["dof"], False, 3)
    assert np.isfinite(apfit(*a, ok, iters=2)["loss"]).all()
    for bad, msg in ((dict(links=[0, 1, 2]), b"sphere_link[2]=2 is outside 0..1"),
                     (dict(links=[7, 1, 1]), b"sphere_link[0]=7 is outside 0..1"),
                     (dict(links=[0, -1, 1]), b"sphere_link[1]=-1 < 0"),
                     (dict(pairs=[(0, 3), (2, 0)]), b"pair[0]=(0, 3) is outside 0..2"),
                     (dict(pairs=[(1, 1), (2, 0)]), b"pair[0] joins sphere 1 with itself"),
                     (dict(mask=8), b"floor_mask=0x8 has bits at or above S=3"),
                     (dict(plane=[0, 0, 0, 1.0]), b"plane normal has zero length"),
                     (dict(margin=float("inf")), b"margin=inf must be finite"),
                     (dict(wf=-1.0), b"floor_weight=-1 must be finite and not negative")):
        rc, err = apfit(*a, dict(ok, **{k: np.asarray(v) if isinstance(v, list) else v for k, v in bad.items()}), status=True)
        assert rc == INVALID and msg in err and b"rtg_dof_fit_apart_f32" in err, err
    # a link that only the floor would use, or that no pair and no floor uses, is still checked
    rc, err = apfit(*a, dict(ok, links=np.array([0, 1, 5]), pairs=np.zeros((0, 2), np.int32), pw=None), status=True)
    assert rc == INVALID and b"sphere_link[2]=5 is outside 0..1" in err
    # the prior launch's own errors come through the new symbol under its name
    rc, err = apfit(*a, ok, flags=2, status=True)
    assert rc == INVALID and b"flags=2 has unknown bits" in err and b"rtg_dof_fit_apart_f32" in err
    rc, _ = apfit(s, x["tgt"][:0], None, x["rr"][:0], x["rt"][:0], x["dof"][:0], False, 3, ok, status=True)
    assert rc == 0                                                               # B == 0: a no-op
    # the plane's normal may have any length: the host normalises it
    long = dict(ok, plane=np.array([0, 0, 7.5, 0.0], np.float32))
    assert_same_bits(apfit(*a, ok), apfit(*a, long), "normal of length 7.5", OUTS)


def test_python_entry_points(gpu):
    from rtg import ops
    s, x, ap = gpu_case("hu33", True, True, True)
    B = 19
    x = {k: (v[:B] if k != "w" else v) for k, v in x.items()}
    p, pw = priors(s, x["dof"], 162)
    joints = [20, 32]
    R, rw = targets(B, 2, 163)
    spec_ = to_ops(s, ap)
    assert spec_.spec.S == len(ap["links"]) and spec_.pairs.tolist() == ap["pairs"].tolist()
    # ops.apart chooses the floor's spheres by link, the generator by sphere: every sphere of a masked sphere's link
    on = {int(ap["links"][i]) for i in range(len(ap["links"])) if ap["mask"] >> i & 1}
    assert spec_.floor_mask == sum(1 << i for i, j in enumerate(ap["links"]) if int(j) in on)
    ap = dict(ap, mask=spec_.floor_mask)
    o = dict(prior=p, prior_weight=pw, apart=spec_)
    # ops.pose_loss / keypoint_loss: the evaluate-only launch under autograd; a cotangent scales row by row
    for ori, okw in (((), {}), ((joints, R, rw), dict(rot_joints=joints, target_rot=R, rot_weight=rw))):
        for normalise, mask in ((True, FIT_ROT), (False, 0)):
            r = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, mask, ap, *(ori or ((), None, None)), p, pw)
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
        g0 = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, ap, *(ori or ((), None, None)), p, pw)
        a = _dev(x["dof"]).requires_grad_(True)
        kl = ops.keypoint_loss(s.model, a, x["tgt"], x["rr"], x["rt"], weight=x["w"], clip=True, **o, **okw)
        kl.sum().backward()
        np.testing.assert_array_equal(bits(_np(kl)), bits(g0["loss"]))
        np.testing.assert_array_equal(bits(_np(a.grad)), bits(g0["grad"]))
    # the term alone (no prior, no links) under autograd
    r = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, FIT_ROT, ap)
    a = _dev(x["dof"]).requires_grad_(True)
    loss = ops.pose_loss(s.model, a, x["rr"], x["rt"], x["tgt"], weight=x["w"], clip=True, apart=spec_)
    loss.sum().backward()
    np.testing.assert_array_equal(bits(_np(loss)), bits(r["loss"]))
    np.testing.assert_array_equal(bits(_np(a.grad)), bits(r["grad"]))
    # ops.pose_fit / dof_fit: the launch, the chain 4 + 4 = 8
    kw = dict(weight=x["w"], lr=LR, lr_root_t=0.01, clip=True)
    r8 = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, ap, (), None, None, p, pw, PROJECT, iters=8, lr_t=0.01)
    p8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, return_grad=True, project=True, **kw, **o)
    for k, v in (("dof", p8.dof), ("rr", p8.root_rot), ("rt", p8.root_t), ("loss", p8.loss), ("grad", p8.grad),
                 ("groot", p8.grad_root)):
        np.testing.assert_array_equal(bits(_np(v)), bits(r8[k]), err_msg=k)
    p4 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, project=True, **kw, **o)
    q8 = ops.pose_fit(s.model, x["tgt"], p4.root_rot, p4.root_t, p4.dof, iters=4, state=p4.state, project=True, **kw, **o)
    assert all(torch.equal(u, v) for u, v in zip(q8[:4] + q8.state[:3], p8[:4] + p8.state[:3]))
    only = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, ap, iters=4, lr_t=0.01)
    np.testing.assert_array_equal(bits(_np(ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, apart=spec_,
                                                        **kw).dof)), bits(only["dof"]))
    g8 = apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, ap, (), None, None, p, pw, PROJECT, iters=8)
    d8 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=8, lr=LR, clip=True, return_grad=True,
                     project=True, **o)
    for i, k in ((0, "dof"), (1, "loss"), (3, "grad")):
        np.testing.assert_array_equal(bits(_np(d8[i])), bits(g8[k]), err_msg=k)
    d4 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], weight=x["w"], iters=8, lr=LR, clip=True, apart=spec_)
    np.testing.assert_array_equal(bits(_np(d4[0])), bits(apfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 0, ap,
                                                               iters=8)["dof"]))
    # apart=None: the old functions' bits
    old = prfit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, 3, prior=p, pw=pw, iters=8, lr_t=0.01)
    n8 = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, prior=p, prior_weight=pw, apart=None, **kw)
    for k, v in (("dof", n8.dof), ("rr", n8.root_rot), ("rt", n8.root_t), ("loss", n8.loss)):
        np.testing.assert_array_equal(bits(_np(v)), bits(old[k]), err_msg=k)
    # what ops refuses before the C ABI sees a pointer, and what the C ABI refuses once it knows the model
    with pytest.raises(ValueError, match="built with ops.apart"):
        ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=1, apart=dict(S=3))
    from rtg import _lib
    wide = ops.apart(type("Tree", (), dict(parents=list(range(-1, 63)))), [40, 2], 0.1)
    with pytest.raises(_lib.RtgError, match="sphere_link\\[0\\]=40 is outside 0..32"):
        ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=1, apart=wide)
    # the builder on a DofModel: the tree is the model's
    mine = ops.apart(s.model, ap["links"], ap["spheres"][:, 3], ap["spheres"][:, :3], pairs=ap["pairs"], pair_weight=ap["pw"],
                     margin=ap["margin"], floor=ap["plane"], floor_weight=ap["wf"],
                     floor_links=sorted({int(ap["links"][i]) for i in range(len(ap["links"])) if ap["mask"] >> i & 1}))
    assert mine.floor_mask == spec_.floor_mask
    # the drop-in: results on the inputs' device
    hu = _hu_on(s)
    tgt, rt, rr = torch.from_numpy(x["tgt"]), torch.from_numpy(x["rt"]), torch.from_numpy(x["rr"][:, None])
    want = ops.pose_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, lr=LR, clip=True, project=True, **o)
    ang, t, q, loss, state = hu.fit_pose(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), iters=8, lr=LR,
                                         prior_angles=torch.from_numpy(p), prior_weight=torch.from_numpy(pw),
                                         project_angles=True, apart=mine)
    assert ang.shape == (B, 32, 1) and all(v.device.type == "cpu" for v in (ang, t, q, loss))
    assert torch.equal(ang[..., 0], want.dof.cpu()) and torch.equal(loss, want.loss.cpu())
    ang, loss, state = hu.fit_keypoints(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), weight=x["w"], iters=8, lr=LR,
                                        prior_angles=torch.from_numpy(p), prior_weight=torch.from_numpy(pw), project_angles=True,
                                        apart=mine)
    assert torch.equal(ang[..., 0], d8[0].cpu()) and torch.equal(loss, d8[1].cpu())

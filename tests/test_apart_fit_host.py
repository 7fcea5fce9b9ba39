"""CPU-only checks of the pose fit with keep-apart spheres and a floor (rtg_dof_fit_apart_f32): the symbol is there
under ABI 7 with its prototype, every argument check that needs no handle answers with its own message before any
device work (the handle is NULL and every device address a dummy in all of these calls), the Python entry points raise
RtgError without a GPU, ops.apart's default pair rule holds on Hu, and the reference the GPU tests use -- the
restatement of tests/test_prior_fit_host.py with, for spheres c_s = P_j + rot(G_j, o_s),

    sum_p pair_weight[p] max(0, r_a + r_b + margin - |c_a - c_b|)^2 + sum_{s in mask} floor_weight max(0, r_s + h0 - n . c_s)^2

added to the loss (torch.where / torch.clamp only) -- is anchored: its float64 autograd gradient agrees with central
differences and, in the centres, with the closed form of rtg.h.  The input generator of the GPU tests is asserted here,
on the float64 reference and for every skeleton they use: no term within 1e-3 m of its hinge (so a float32 and a
float64 evaluation agree on the active set), no active pair nearer than 1e-3 m, at least a quarter of the terms active
and a quarter inactive.  It moves radii, never frames.  On two pinned recipes the float64 loop shows what the term is
for: wrists brought to one point in front of the torso stay out of it and of each other, and ankles whose targets lie
under the floor stay above it.

The spheres of the two recipes are made up for these tests (the repository holds Hu's skeleton, no collision geometry):
torso 0.16 m at (0, 0, 0.25) of link 13, wrists 0.05 m on links 19 and 28, grippers 0.04 m at (0.08, 0, 0) of links 21
and 30, ankles 0.05 m on links 6 and 12."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_fk_grad_host import dof_fk, quat_rotate
from test_gpu_dof_fit import inputs, skel
from test_orient_fit_host import INVALID, UNSUPPORTED
from test_pose_fit_host import B1, B2, EPS, FIT_ROT, FIT_T, LR, _Hu, _t, root_unit
from test_prior_fit_host import PROJECT, ref_prior_loss

MAX_SPHERES, MAX_PAIRS = 16, 32   # RTG_FIT_MAX_SPHERES, RTG_FIT_MAX_PAIRS
HINGE = 1e-3                      # no term of a generated case lies nearer its hinge, no active pair nearer than this


# ------------------------------------------------------------------ the reference: restatement + the two terms
def spec(links, spheres, pairs=(), pw=None, margin=0.0, plane=None, mask=0, wf=1.0):
    """The term as plain host data: links (S,), spheres (S,4) {offset, radius}, pairs (Pn,2), pair_weight (Pn,) or
    None, margin, plane (4,) {normal of any length, h0} or None, floor mask and weight."""
    return dict(links=np.asarray(links, np.int32).reshape(-1), spheres=np.asarray(spheres, np.float32).reshape(-1, 4),
                pairs=np.asarray(pairs, np.int32).reshape(-1, 2), pw=None if pw is None else np.asarray(pw, np.float32),
                margin=float(margin), plane=None if plane is None else np.asarray(plane, np.float32), mask=int(mask),
                wf=float(wf))


def ref_centres(s, dof, q, t, clip, dtype, fit_root, ap):
    """c_s = P_j + rot(G_j, o_s) (B,S,3), G and P as the forward model holds them (the root normalised with FIT_ROT)."""
    q = _t(q, dtype)
    lo, hi = (_t(s.lo, dtype), _t(s.hi, dtype)) if clip else (None, None)
    G, P = dof_fk(_t(dof, dtype), root_unit(q) if fit_root & FIT_ROT else q, _t(t, dtype), [int(p) for p in s.par],
                  _t(s.lt, dtype), s.axis, lo, hi)
    lk = torch.as_tensor(ap["links"], dtype=torch.long)
    off = _t(ap["spheres"][:, :3], dtype).expand(G.shape[0], -1, -1)
    return P[:, lk] + quat_rotate(G[:, lk], off)


def pair_hinges(c, ap, dtype):
    """-> (d, x): the pairs' centre distances and r_a + r_b + margin - d, (B,Pn); d = 0 exactly where the centres
    coincide (and no gradient from there); NaN passes."""
    a, b = (torch.as_tensor(ap["pairs"][:, k], dtype=torch.long) for k in (0, 1))
    r = _t(ap["spheres"][:, 3], dtype)
    ss = ((c[:, a] - c[:, b]) ** 2).sum(dim=-1)
    apart = ~(ss == 0)
    d = torch.where(apart, torch.where(apart, ss, torch.ones_like(ss)).sqrt(), torch.zeros_like(ss))
    return d, (r[a] + r[b] + ap["margin"]) - d


def floor_hinges(c, ap, dtype):
    """-> r_s + h0 - n . c_s of the masked spheres, (B,Sf), the normal normalised."""
    on = torch.as_tensor([i for i in range(len(ap["links"])) if ap["mask"] >> i & 1], dtype=torch.long)
    pl = _t(ap["plane"], dtype)
    n = pl[:3] / pl[:3].norm()
    return (_t(ap["spheres"][:, 3], dtype)[on] + pl[3]) - (c[:, on] * n).sum(dim=-1)


def ref_apart_terms(c, ap, dtype):
    """The two terms of the loss from the centres (B,S,3) -> (B,)."""
    loss = torch.zeros(c.shape[0], dtype=dtype)
    if len(ap["pairs"]):
        pw = torch.ones(len(ap["pairs"]), dtype=dtype) if ap["pw"] is None else _t(ap["pw"], dtype)
        loss = loss + (pw * torch.clamp(pair_hinges(c, ap, dtype)[1], min=0) ** 2).sum(dim=-1)
    if ap["plane"] is not None and ap["mask"]:
        loss = loss + ap["wf"] * (torch.clamp(floor_hinges(c, ap, dtype), min=0) ** 2).sum(dim=-1)
    return loss


def ref_apart_loss(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw, prior, pw, ap):
    """ref_prior_loss plus the keep-apart terms; ap None: none."""
    loss = ref_prior_loss(s, dof, q, t, tgt, w, clip, dtype, fit_root, joints, R, rw, prior, pw)
    if ap is None or not len(ap["links"]):
        return loss
    return loss + ref_apart_terms(ref_centres(s, dof, q, t, clip, dtype, fit_root, ap), ap, dtype)


def ref_apart_loss_grad(s, dof, q, t, *rest):
    """-> loss (B), grad (B,J-1), grad_root (B,7) = {dL/dt, dL/dq}, numpy."""
    a, qq, tt = (_t(x, rest[3]).clone().requires_grad_(True) for x in (dof, q, t))
    loss = ref_apart_loss(s, a, qq, tt, *rest)
    loss.sum().backward()
    g = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    return loss.detach().numpy(), g(a).numpy(), torch.cat([g(tt), g(qq)], dim=-1).numpy()


def penetration(s, dof, q, t, clip, fit_root, ap):
    """The deepest overlap of a pose in metres, per frame (float64): max over the pairs' and the floor's hinges, 0
    where nothing overlaps."""
    with torch.no_grad():
        c = ref_centres(s, dof, q, t, clip, torch.float64, fit_root, ap)
        h = [torch.zeros(c.shape[0], 1, dtype=torch.float64)]
        if len(ap["pairs"]):
            h.append(pair_hinges(c, ap, torch.float64)[1])
        if ap["plane"] is not None and ap["mask"]:
            h.append(floor_hinges(c, ap, torch.float64))
        return torch.cat(h, dim=-1).clamp(min=0).max(dim=-1).values.numpy()


class RefApartFit:
    """test_prior_fit_host.RefFit's loop (torch.optim.Adam, one group per block, the fitted rotation renormalised, the
    angles clamped with ``project``) on the loss with the keep-apart terms; no links, no prior."""
    def __init__(self, s, dof, q, t, w, clip, dtype, fit_root, ap, project=False, lr=LR):
        self.s, self.w, self.clip, self.dtype, self.fit_root, self.ap, self.project = s, w, clip, dtype, fit_root, ap, project
        self.a, self.q, self.t = (_t(x, dtype).clone().requires_grad_(True) for x in (dof, q, t))
        groups = [dict(params=[self.a], lr=lr)]
        if fit_root & FIT_T:
            groups.append(dict(params=[self.t], lr=lr))
        if fit_root & FIT_ROT:
            groups.append(dict(params=[self.q], lr=lr))
        self.opt = torch.optim.Adam(groups, betas=(B1, B2), eps=EPS)
        self.lo, self.hi = _t(s.lo, dtype), _t(s.hi, dtype)

    def loss(self, tgt):
        return ref_apart_loss(self.s, self.a, self.q, self.t, tgt, self.w, self.clip, self.dtype, self.fit_root, [], None,
                              None, None, None, self.ap)

    def run(self, tgt, iters):
        for _ in range(iters):
            self.opt.zero_grad()
            self.loss(tgt).sum().backward()
            self.opt.step()
            with torch.no_grad():
                if self.fit_root & FIT_ROT:
                    self.q.copy_(root_unit(self.q))
                if self.project:
                    self.a.copy_(torch.clamp(self.a, self.lo, self.hi))
        return self

    def result(self, tgt):
        """-> (loss, dof, q, t) at the iterate, numpy."""
        with torch.no_grad():
            loss = self.loss(tgt)
        return tuple(x.detach().numpy().copy() for x in (loss, self.a, self.q, self.t))


# ------------------------------------------------------------------ the GPU tests' input generator
GPU_SKELS = ("hu33", "chain64", "two", "one")
_GRID = 0.0025 * np.arange(400)   # the radii a sphere may be moved through: 1 m in steps of 2.5 mm


def _hinges64(s, x, clip, ap):
    """Every hinge value of the case in float64, for the root as given and normalised: (pairs (2,B,Pn), distances
    (2,B,Pn), floor (2,B,Sf))."""
    out = [[], [], []]
    with torch.no_grad():
        for fit_root in (0, FIT_ROT):
            c = ref_centres(s, x["dof"], x["rr"], x["rt"], clip, torch.float64, fit_root, ap)
            d, h = pair_hinges(c, ap, torch.float64) if len(ap["pairs"]) else (torch.zeros(len(c), 0),) * 2
            f = floor_hinges(c, ap, torch.float64) if ap["plane"] is not None and ap["mask"] else torch.zeros(len(c), 0)
            for o, v in zip(out, (h, d, f)):
                o.append(v.numpy())
    return tuple(np.stack(o) for o in out)


def apart_case(s, x, clip, seed, offsets=True, plane=True):
    """The keep-apart term of a GPU test on the inputs x of skeleton s (test_gpu_dof_fit.inputs): up to 16 spheres on
    random links (several on some), up to 32 random pairs of spheres with different centres, random pair weights (a
    quarter of them 0), a margin, and -- with ``plane`` -- a tilted floor through the cloud of centres under half of
    the spheres.  ``offsets``: three spheres in four sit off their link's origin (up to some 0.3 m).  The radii start
    at half the median centre distance of a sphere's pairs (so about half of the terms are active) and are then moved,
    sphere by sphere, to the nearest value of a 2.5 mm grid at which no term the sphere takes part in lies within 1e-3 m
    of its hinge, for the root as given and normalised; the frames are never touched."""
    rng = np.random.default_rng(seed)
    J = s.J
    S = {1: 3, 2: 6}.get(J, MAX_SPHERES)
    links = rng.integers(0, J, S)
    off = rng.normal(0, 0.15, (S, 3)).astype(np.float32)
    if offsets:
        off[::4] = 0.0
        if J == 1:
            off[0] = 0.0   # and the others differ: the root's spheres have centres of their own
    else:
        off[:] = 0.0
    far = lambda a, b: links[a] != links[b] or off[a].any() or off[b].any()
    cand = [(a, b) if rng.random() < 0.5 else (b, a) for a in range(S) for b in range(a + 1, S) if far(a, b)]
    pairs = [cand[i] for i in rng.permutation(len(cand))[:MAX_PAIRS]]
    pw = rng.uniform(0.5, 3.0, len(pairs)).astype(np.float32)
    pw[rng.permutation(len(pairs))[: len(pairs) // 4]] = 0.0
    ap = spec(links, np.concatenate([off, np.zeros((S, 1), np.float32)], axis=1), pairs, pw, margin=0.01)
    if plane:
        n = np.array([0.2, -0.1, 1.0]) * 1.7
        with torch.no_grad():
            c = ref_centres(s, x["dof"], x["rr"], x["rt"], clip, torch.float64, FIT_ROT, ap).numpy()
        h0 = float(np.median(c @ (n / np.linalg.norm(n))))
        ap.update(plane=np.array([*n, h0], np.float32), mask=int(sum(1 << i for i in range(0, S, 2))), wf=1.5)
    elif not pairs:
        raise ValueError("nothing to test: no pair has two centres and no plane is asked for")
    # the start: half the median distance of the sphere's pairs, 0.1 m for a sphere only the floor sees
    ap["spheres"][:, 3] = 0.0
    _, d, _ = _hinges64(s, x, clip, dict(ap, margin=0.0))
    for i in range(S):
        mine = [p for p, (a, b) in enumerate(pairs) if i in (a, b)]
        ap["spheres"][i, 3] = 0.5 * np.median(d[:, :, mine]) if mine else 0.1
    # the nudge: sphere by sphere, against the spheres already settled
    for i in range(S):
        mine = [p for p, (a, b) in enumerate(pairs) if i in (a, b) and max(a, b) == i]
        fl = [k for k, j in enumerate(j for j in range(S) if ap["mask"] >> j & 1) if j == i] if ap["plane"] is not None else []
        h, _, f = _hinges64(s, x, clip, ap)
        mine_h = np.concatenate([h[:, :, mine].reshape(-1), f[:, :, fl].reshape(-1)])   # at the start radius r0
        r0 = float(ap["spheres"][i, 3])
        for r in sorted(_GRID[_GRID > 0.02], key=lambda v: abs(v - r0)):
            rf = float(np.float32(r))
            if not len(mine_h) or np.abs(mine_h + (rf - r0)).min() > 1.5 * HINGE:
                ap["spheres"][i, 3] = rf
                break
        else:
            raise AssertionError(f"no radius for sphere {i}")
    return ap


def to_ops(s, ap):
    """The case as ops.apart builds it, on the test skeleton's tree."""
    from rtg import ops
    tree = type("Tree", (), dict(parents=[int(p) for p in s.par]))
    fl = None if ap["plane"] is None else sorted({int(ap["links"][i]) for i in range(len(ap["links"])) if ap["mask"] >> i & 1})
    return ops.apart(tree, ap["links"], ap["spheres"][:, 3], ap["spheres"][:, :3], pairs=ap["pairs"], pair_weight=ap["pw"],
                     margin=ap["margin"], floor=ap["plane"], floor_links=fl, floor_weight=ap["wf"])


@functools.lru_cache(maxsize=None)
def gpu_case(name, clip, offsets, plane):
    """(skeleton, inputs of its largest batch, the term): what tests/test_gpu_apart_fit.py evaluates."""
    s = skel(name)
    x = inputs(s, max(s.batches()), clip, 31 * s.J + clip)
    return s, x, apart_case(s, x, clip, 37 * s.J + 2 * offsets + plane, offsets, plane)


# (zero offsets on the one-joint model put every centre on the root: there only the floor has something to hold)
GPU_CASES = [(n, c, o, p) for n in GPU_SKELS for c in (False, True) for o in (False, True) for p in (False, True)
             if not (n == "one" and not o and not p)]


@pytest.mark.parametrize("name, clip, offsets, plane", GPU_CASES)
def test_the_generator_keeps_every_term_off_its_hinge(name, clip, offsets, plane):
    s, x, ap = gpu_case(name, clip, offsets, plane)
    h, d, f = _hinges64(s, x, clip, ap)
    terms = np.concatenate([h.reshape(-1), f.reshape(-1)])
    active = terms > 0
    print(f"{name} clip={clip} offsets={offsets} plane={plane}: S={len(ap['links'])} Pn={len(ap['pairs'])} "
          f"{terms.size} terms, {active.mean():.2f} active, nearest its hinge {np.abs(terms).min():.2e} m, "
          f"nearest active pair {d[h > 0].min() if (h > 0).any() else np.inf:.3f} m")
    assert np.abs(terms).min() > HINGE
    assert not (d[h > 0] < HINGE).any()
    assert active.mean() >= 0.25 and (~active).mean() >= 0.25
    assert (ap["spheres"][:, 3] > 0).all() and len(x["dof"]) == max(s.batches())   # every frame stays
    if name != "one" or offsets:
        assert len(ap["pairs"]) >= 3
    if offsets:
        assert (ap["spheres"][:, :3] != 0).any() and not ap["spheres"][0, :3].any()


# ------------------------------------------------------------------ the symbol and its argument checks
def _apart(**kw):
    """A valid rtg_fit_apart (3 spheres, 2 pairs, a plane), fields overridden by name; -> (struct, what it points to)."""
    from rtg import _lib
    a = dict(S=3, sphere_link=[0, 4, 4], sphere=[[0, 0, 0, 0.1], [0.1, 0, 0, 0.05], [0, 0, 0, 0.0]], Pn=2,
             pair=[[0, 1], [2, 0]], pair_weight=[1.0, 0.0], margin=0.01, plane=[0, 0, 2, 0.0], floor_mask=5,
             floor_weight=1.0)
    assert set(kw) <= set(a)
    a.update(kw)
    arr = lambda v, t: None if v is None else np.ascontiguousarray(np.asarray(v, t).reshape(-1))
    keep = dict(sphere_link=arr(a["sphere_link"], np.int32), sphere=arr(a["sphere"], np.float32), pair=arr(a["pair"], np.int32),
                pair_weight=arr(a["pair_weight"], np.float32), plane=arr(a["plane"], np.float32))
    p = lambda k, t: None if keep[k] is None else keep[k].ctypes.data_as(ctypes.POINTER(t))
    st = _lib.FitApart(a["S"], p("sphere_link", ctypes.c_int32), p("sphere", ctypes.c_float), a["Pn"], p("pair", ctypes.c_int32),
                       p("pair_weight", ctypes.c_float), a["margin"], p("plane", ctypes.c_float), a["floor_mask"],
                       a["floor_weight"])
    return st, keep


def _call(lib, apart=(), **kw):
    """rtg_dof_fit_apart_f32 with a NULL model and never-dereferenced dummy device addresses, fields overridden by
    name; apart: _apart's overrides, or None for a NULL struct."""
    x = ctypes.c_void_p(64)
    a = dict(model=None, target_pos=x, weight=x, rot_joint=[0, 5, 2], target_rot=x, rot_weight=x, K=3, prior=x,
             prior_weight=x, flags=PROJECT, root_rot=x, root_t=x, dof_in=x, B=1, clip=0, fit_root=3, iters=1, lr=0.02,
             lr_root_t=0.02, lr_root_rot=0.02, beta1=0.9, beta2=0.999, eps=1e-8, step0=0, m=x, v=x, root_state=x,
             dof_out=x, root_rot_out=x, root_t_out=x, loss=x, grad=x, grad_root=x)
    assert set(kw) <= set(a)
    a.update(kw)
    if a["rot_joint"] is not None:
        a["rot_joint"] = (ctypes.c_int32 * max(len(a["rot_joint"]), 1))(*a["rot_joint"])
    st, keep = (None, None) if apart is None else _apart(**dict(apart))
    return lib.rtg_dof_fit_apart_f32(*a.values(), None if st is None else ctypes.byref(st), None)


def test_symbol_prototype_and_abi_version():
    from rtg import _lib
    lib = _lib.lib()
    fn = lib.rtg_dof_fit_apart_f32
    assert lib.rtg_abi_version() == 7   # a new symbol only: nothing that existed changed
    pri = list(lib.rtg_dof_fit_prior_f32.argtypes)
    assert fn.restype is ctypes.c_int
    # rtg_dof_fit_prior_f32's arguments with the host struct before the stream
    assert list(fn.argtypes) == pri[:-1] + [ctypes.POINTER(_lib.FitApart), pri[-1]]
    names = [f[0] for f in _lib.FitApart._fields_]
    assert names == ["S", "sphere_link", "sphere", "Pn", "pair", "pair_weight", "margin", "plane", "floor_mask", "floor_weight"]
    from rtg import ops
    assert (ops.FIT_MAX_SPHERES, ops.FIT_MAX_PAIRS) == (MAX_SPHERES, MAX_PAIRS)


_NAN, _INF = float("nan"), float("inf")
_SPH = [[0, 0, 0, 0.1], [0.1, 0, 0, 0.05], [0, 0, 0, 0.0]]


def _sph(i, c, v):
    rows = [list(r) for r in _SPH]
    rows[i][c] = v
    return rows


@pytest.mark.parametrize("kw, apart, code, msg", [
    # rtg_dof_fit_prior_f32's, with the struct and without
    (dict(), {}, INVALID, b"NULL model"),
    (dict(), None, INVALID, b"NULL model"),
    (dict(B=-1), {}, INVALID, b"< 0"),
    (dict(target_pos=None), {}, INVALID, b"NULL buffer"),
    (dict(m=None), {}, INVALID, b"both Adam moment buffers"),
    (dict(fit_root=4), {}, INVALID, b"fit_root=4"),
    (dict(iters=4097), {}, INVALID, b"iters=4097"),
    (dict(K=9, rot_joint=list(range(9))), {}, UNSUPPORTED, b"at most 8"),
    (dict(rot_joint=[4, 5, 4]), {}, INVALID, b"listed twice"),
    (dict(flags=2), {}, INVALID, b"flags=2 has unknown bits"),
    (dict(prior=None), {}, INVALID, b"prior_weight given without prior"),
    # the struct's
    (dict(), dict(S=-1), INVALID, b"S=-1 < 0"),
    (dict(), dict(Pn=-1), INVALID, b"Pn=-1 < 0"),
    (dict(), dict(S=MAX_SPHERES + 1), UNSUPPORTED, b"S=17 spheres, at most 16"),
    (dict(), dict(Pn=MAX_PAIRS + 1), UNSUPPORTED, b"Pn=33 pairs, at most 32"),
    (dict(), dict(sphere_link=None), INVALID, b"S=3 with sphere_link or sphere NULL"),
    (dict(), dict(sphere=None), INVALID, b"S=3 with sphere_link or sphere NULL"),
    (dict(), dict(pair=None), INVALID, b"Pn=2 with pair NULL"),
    (dict(), dict(margin=_NAN), INVALID, b"margin=nan must be finite"),
    (dict(), dict(margin=_INF), INVALID, b"margin=inf must be finite"),
    (dict(), dict(sphere=_sph(1, 3, -0.01)), INVALID, b"sphere[1] has the negative radius -0.01"),
    (dict(), dict(sphere=_sph(2, 3, _NAN)), INVALID, b"sphere[2] is not finite"),
    (dict(), dict(sphere=_sph(0, 3, _INF)), INVALID, b"sphere[0] is not finite"),
    (dict(), dict(sphere=_sph(1, 0, _INF)), INVALID, b"sphere[1] is not finite"),
    (dict(), dict(sphere=_sph(2, 2, _NAN)), INVALID, b"sphere[2] is not finite"),
    (dict(), dict(sphere_link=[0, -1, 4]), INVALID, b"sphere_link[1]=-1 < 0"),
    (dict(), dict(pair=[[0, 1], [3, 0]]), INVALID, b"pair[1]=(3, 0) is outside 0..2"),
    (dict(), dict(pair=[[0, -1], [2, 0]]), INVALID, b"pair[0]=(0, -1) is outside 0..2"),
    (dict(), dict(pair=[[0, 1], [2, 2]]), INVALID, b"pair[1] joins sphere 2 with itself"),
    (dict(), dict(S=0, floor_mask=0), INVALID, b"is outside 0..-1"),
    (dict(), dict(pair_weight=[1.0, -0.5]), INVALID, b"pair_weight[1]=-0.5 must be finite and not negative"),
    (dict(), dict(pair_weight=[_NAN, 1.0]), INVALID, b"pair_weight[0]=nan must be finite and not negative"),
    (dict(), dict(plane=[0, 0, 1, _NAN]), INVALID, b"plane is not finite"),
    (dict(), dict(plane=[_INF, 0, 1, 0]), INVALID, b"plane is not finite"),
    (dict(), dict(plane=[0, 0, 0, 0.5]), INVALID, b"plane normal has zero length"),
    (dict(), dict(floor_weight=-1.0), INVALID, b"floor_weight=-1 must be finite and not negative"),
    (dict(), dict(floor_weight=_NAN), INVALID, b"floor_weight=nan must be finite and not negative"),
    (dict(), dict(floor_mask=8), INVALID, b"floor_mask=0x8 has bits at or above S=3"),
    (dict(), dict(floor_mask=0x80000001), INVALID, b"floor_mask=0x80000001 has bits at or above S=3"),
])
def test_validation_before_device_work(kw, apart, code, msg):
    from rtg import _lib
    lib = _lib.lib()
    assert _call(lib, apart, **kw) == code
    assert msg in lib.rtg_last_error(), lib.rtg_last_error()
    assert b"rtg_dof_fit_apart_f32" in lib.rtg_last_error()


def test_valid_arguments_reach_the_handle_check():
    """Every allowed combination of the new arguments passes the checks before the handle's: the call then stops at
    the NULL model (a link outside 0..J-1 needs a model: tests/test_gpu_apart_fit.py)."""
    from rtg import _lib
    lib = _lib.lib()
    full = [[i, (i + 1) % MAX_SPHERES] for i in range(MAX_SPHERES)] * 2
    for ap in (None, {}, dict(S=0, Pn=0, floor_mask=0), dict(S=0, Pn=0, sphere_link=None, sphere=None, pair=None, plane=None),
               dict(Pn=0, pair=None, pair_weight=None), dict(pair_weight=None), dict(plane=None), dict(margin=-0.02),
               dict(plane=None, floor_mask=0xFFFFFFFF, floor_weight=_NAN), dict(floor_mask=0), dict(floor_weight=0.0),
               dict(sphere_link=[0, 4, 10 ** 6]), dict(plane=[3, -4, 12, -1.0]),
               dict(S=MAX_SPHERES, sphere_link=list(range(MAX_SPHERES)), sphere=[[0, 0, 0, 0.1]] * MAX_SPHERES, Pn=MAX_PAIRS,
                    pair=full, pair_weight=None, floor_mask=0xFFFF)):
        assert _call(lib, ap) == INVALID and b"NULL model" in lib.rtg_last_error(), (ap, lib.rtg_last_error())
    assert _call(lib, {}, B=0) == INVALID and b"NULL model" in lib.rtg_last_error()


class _NoDeviceModel:
    """What ops looks at before it asks for the device."""
    num_dofs = 32
    has_limits = True
    handle = None
    parents = _Hu().par


def test_python_entry_points_raise_rtg_error_without_a_gpu(monkeypatch):
    from rtg import _lib, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # the same test on a machine that has one
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    tp = np.zeros((2, 33, 3), np.float32)
    rr = np.tile(np.array([0, 0, 0, 1], np.float32), (2, 1))
    rt = np.zeros((2, 3), np.float32)
    dof = np.zeros((2, 32), np.float32)
    ap = ops.apart(_NoDeviceModel(), [13, 19, 28], [0.16, 0.05, 0.05], floor=(0, 0, 1, 0.0), floor_links=[19])
    with pytest.raises(_lib.RtgError):
        ops.pose_fit(_NoDeviceModel(), tp, rr, rt, iters=1, apart=ap)
    with pytest.raises(_lib.RtgError):
        ops.pose_loss(_NoDeviceModel(), dof, rr, rt, tp, apart=ap)
    with pytest.raises(_lib.RtgError):
        ops.dof_fit(_NoDeviceModel(), tp, rr, rt, iters=1, apart=ap)
    with pytest.raises(_lib.RtgError):
        ops.keypoint_loss(_NoDeviceModel(), dof, tp, rr, rt, apart=ap)
    hu = HuForwardModel.__new__(HuForwardModel)   # its constructor already needs the device
    hu._model, hu.num_joints, hu.node_names = _NoDeviceModel(), 33, [f"n{j}" for j in range(33)]
    hu.parent_indices = torch.as_tensor(_Hu().par)
    named = ops.apart(hu, ["n13", "n19", 28], [0.16, 0.05, 0.05], floor=(0, 0, 1, 0.0), floor_links=["n19"])
    assert named.links.tolist() == ap.links.tolist() and named.floor_mask == ap.floor_mask == 2
    args = (torch.from_numpy(tp), torch.from_numpy(rt), torch.from_numpy(rr[:, None]))
    with pytest.raises(_lib.RtgError):
        hu.fit_pose(*args, apart=named)
    with pytest.raises(_lib.RtgError):
        hu.fit_keypoints(*args, apart=named)
    with pytest.raises(_lib.RtgError):
        hu.fit_motion(*args, apart=named)


def test_the_builder_and_its_default_pairs_on_hu():
    """pairs=None: every pair of spheres whose links are neither the same nor parent and child, in (a, b) order with
    a < b; more than 32 of them raise; what the builder refuses."""
    from rtg import ops
    s = _Hu()
    par = [int(p) for p in s.par]
    tree = type("Tree", (), dict(parents=par, node_names=[f"n{j}" for j in range(s.J)]))
    links = [13, 13, 0, 14, 19, 20, 21, 28, 32]   # torso twice, its parent the root, its children 14 and 32, an arm's chain
    ap = ops.apart(tree, links, 0.05)
    related = lambda a, b: links[a] == links[b] or par[links[a]] == links[b] or par[links[b]] == links[a]
    want = [[a, b] for a in range(len(links)) for b in range(a + 1, len(links)) if not related(a, b)]
    assert ap.pairs.tolist() == want and len(want) <= MAX_PAIRS
    gone = {(a, b) for a in range(len(links)) for b in range(a + 1, len(links))} - {tuple(p) for p in want}
    assert gone == {(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (0, 8), (1, 8), (4, 5), (5, 6)}
    assert ap.spec.S == 9 and ap.spec.Pn == len(want) and not ap.spec.pair_weight and not ap.spec.plane
    assert ap.spheres.shape == (9, 4) and (ap.spheres[:, 3] == np.float32(0.05)).all() and not ap.spheres[:, :3].any()
    assert ap.floor_mask == 0
    leaves = [6, 12, 19, 21, 22, 28, 30, 31, 32, 3, 9]   # 11 links, no two of them related: 55 pairs
    with pytest.raises(ValueError, match="55 pairs of unrelated links, at most 32"):
        ops.apart(tree, leaves, 0.05)
    assert ops.apart(tree, leaves, 0.05, pairs=[(0, 1)]).spec.Pn == 1
    assert ops.apart(tree, leaves[:8], 0.05).spec.Pn == 28
    fl = ops.apart(tree, ["n6", "n12", 13], [0.05, 0.05, 0.2], floor=(0, 0, 1, 0), floor_links=["n6", 12], floor_weight=2.0)
    assert fl.floor_mask == 3 and fl.spec.floor_weight == 2.0 and fl.pairs.tolist() == [[0, 1], [0, 2], [1, 2]]
    assert ops.apart(tree, [6, 12], 0.05, floor=(0, 0, 1, 0)).floor_mask == 3
    for bad in (dict(links=["nope"]), dict(links=[33]), dict(links=[-1]), dict(links=list(range(17))),
                dict(radii=[0.1, 0.1]), dict(radii=-0.1), dict(radii=np.nan), dict(offsets=np.zeros((2, 3))),
                dict(offsets=np.full((3, 3), np.inf)), dict(pairs=[(0, 0)]), dict(pairs=[(0, 3)]),
                dict(pairs=[(0, 1)] * 33), dict(pair_weight=-1.0), dict(margin=np.inf), dict(floor=(0, 0, 0, 1)),
                dict(floor=(0, 0, 1)), dict(floor_links=[6]), dict(floor=(0, 0, 1, 0), floor_links=["nope"]),
                dict(floor_weight=-1.0)):
        with pytest.raises(ValueError):
            ops.apart(tree, **dict(dict(links=[6, 12, 13], radii=0.05), **bad))


# ------------------------------------------------------------------ the reference itself
def _case(B=3, seed=41):
    s = _Hu()
    rng = np.random.default_rng(seed)
    quat = lambda *k: (lambda q: q / np.linalg.norm(q, axis=-1, keepdims=True))(rng.normal(size=k + (4,)))
    x = dict(dof=rng.uniform(s.lo, s.hi, (B, s.J - 1)), rr=quat(B) * rng.uniform(0.7, 1.5, (B, 1)),
             rt=rng.normal(0, 0.3, (B, 3)), tgt=rng.normal(0, 0.5, (B, s.J, 3)), w=np.ones(s.J))
    return s, x


def test_the_terms_gradient_agrees_with_central_differences():
    """float64, the terms alone (every position weight 0), clip on, the root as given and normalised, with offsets:
    every active term is (at least 1e-3 from its hinge, so) smooth over h = 1e-6 and the central difference's truncation
    error is h^2 times a third derivative, 1e-12 of some units; its rounding error 2^-52 |L| / h is 1e-10 for losses
    up to 1.  The bound 1e-6 max|grad| leaves room for both and none for a wrong factor or a missing term."""
    s, x = _case()
    ap = apart_case(s, x, True, 43)
    h, _, f = _hinges64(s, x, True, ap)
    assert (h > 0).any() and (h < 0).any() and (f > 0).any() and (f < 0).any()
    for fit_root in (0, FIT_ROT):
        rest = (x["tgt"], np.zeros(s.J), True, torch.float64, fit_root, [], None, None, None, None, ap)
        loss, g, gr = ref_apart_loss_grad(s, x["dof"], x["rr"], x["rt"], *rest)
        assert loss.min() > 0 and np.abs(g).max() > 0.1 and np.abs(gr).max() > 0.1
        e = 1e-6
        packed = np.concatenate([x["dof"], x["rt"], x["rr"]], axis=1)
        grad = np.concatenate([g, gr], axis=1)
        fd = np.zeros_like(grad)
        n = s.J - 1
        for i in range(packed.shape[1]):
            with torch.no_grad():
                v = []
                for sgn in (1.0, -1.0):
                    y = packed.copy()
                    y[:, i] += sgn * e
                    v.append(ref_apart_loss(s, y[:, :n], y[:, n + 3:], y[:, n:n + 3], *rest).numpy())
                fd[:, i] = (v[0] - v[1]) / (2 * e)
        err = np.abs(fd - grad).max() / np.abs(grad).max()
        print(f"fit_root={fit_root}: max |central difference - autograd| / max |autograd| = {err:.2e}")
        assert err <= 1e-6
        without = ref_apart_loss_grad(s, x["dof"], x["rr"], x["rt"], *rest[:-1], None)
        assert not without[0].any() and not without[1].any() and not without[2].any()   # nothing else is in it


def test_the_centre_gradients_agree_with_the_closed_form():
    """With zero offsets the centres are the links' positions, and autograd's gradient in them is rtg.h's closed form:
    -2 w h (c_a - c_b) / |c_a - c_b| to a's sphere and its negative to b's, -2 w_f h n from the floor, summed per
    sphere; coincident centres add w (r_a + r_b + margin)^2 and no gradient; a NaN centre passes."""
    s, x = _case(B=5)
    ap = apart_case(s, x, True, 47, offsets=False)
    with torch.no_grad():
        c0 = ref_centres(s, x["dof"], x["rr"], x["rt"], True, torch.float64, FIT_ROT, ap)
        P = dof_fk(_t(x["dof"], torch.float64), root_unit(_t(x["rr"], torch.float64)), _t(x["rt"], torch.float64),
                   [int(p) for p in s.par], _t(s.lt, torch.float64), s.axis, _t(s.lo, torch.float64), _t(s.hi, torch.float64))[1]
    assert torch.equal(c0, P[:, torch.as_tensor(ap["links"], dtype=torch.long)])
    c = c0.clone().requires_grad_(True)
    loss = ref_apart_terms(c, ap, torch.float64)
    loss.sum().backward()
    cn, r, S = c0.numpy(), ap["spheres"][:, 3].astype(np.float64), len(ap["links"])
    g, want = np.zeros_like(cn), np.zeros(len(cn))
    for p, (a, b) in enumerate(ap["pairs"]):
        diff = cn[:, a] - cn[:, b]
        d = np.linalg.norm(diff, axis=-1)
        hh = np.maximum(0.0, r[a] + r[b] + ap["margin"] - d)
        t = (-2.0 * float(ap["pw"][p]) * hh / np.maximum(d, 1e-9))[:, None] * diff
        g[:, a] += t
        g[:, b] -= t
        want += float(ap["pw"][p]) * hh ** 2
    n = ap["plane"][:3].astype(np.float64) / np.linalg.norm(ap["plane"][:3].astype(np.float64))
    for i in range(S):
        if ap["mask"] >> i & 1:
            hh = np.maximum(0.0, r[i] + float(ap["plane"][3]) - cn[:, i] @ n)
            g[:, i] += (-2.0 * ap["wf"] * hh)[:, None] * n
            want += ap["wf"] * hh ** 2
    assert np.abs(g).max() > 0.1
    assert np.allclose(c.grad.numpy(), g, rtol=0, atol=1e-13 * np.abs(g).max())
    assert np.allclose(loss.detach().numpy(), want, rtol=1e-13)
    # coincident centres, and a NaN
    two = spec([1, 2], [[0, 0, 0, 0.1], [0, 0, 0, 0.2]], [(0, 1)], [2.0], margin=0.05)
    c = torch.zeros(3, 2, 3, dtype=torch.float64)
    c[1, 1, 0] = 0.3
    c[2, 0, 1] = float("nan")
    c.requires_grad_(True)
    loss = ref_apart_terms(c, two, torch.float64)
    loss[:2].sum().backward()
    assert loss[0].item() == pytest.approx(2.0 * 0.35 ** 2, rel=1e-6) and not c.grad[0].any()
    assert loss[1].item() == pytest.approx(2.0 * 0.05 ** 2, rel=1e-6) and c.grad[1, 0, 0].item() > 0
    assert torch.isnan(loss[2])


# ------------------------------------------------------------------ what the term is for: two pinned recipes
TORSO, WRISTS, GRIPPERS, ANKLES = 13, (19, 28), (21, 30), (6, 12)


def _rest(s, B):
    a = np.zeros((B, s.J - 1))
    q, t = np.tile([0.0, 0.0, 0.0, 1.0], (B, 1)), np.zeros((B, 3))
    with torch.no_grad():
        f64 = lambda v: _t(v, torch.float64)
        P = dof_fk(f64(a), f64(q), f64(t), [int(p) for p in s.par], f64(s.lt), s.axis, f64(s.lo), f64(s.hi))[1].numpy()
    return a.astype(np.float32), q.astype(np.float32), t.astype(np.float32), P


def hands_recipe():
    """The pinned hands recipe: 33-link Hu, B = 64, the root given as identity, clip on, the start at zero angles.
    Targets: the rest pose for every link at weight 0.05, but both wrists (links 19 and 28) at weight 1 on ONE point per
    frame, drawn uniformly from a 0.16 x 0.2 x 0.24 m box centred 0.22 m in front of the torso sphere's centre -- so the
    hands would meet there, and in many frames inside the torso's 0.16 m sphere.  Spheres: the torso, the two wrists,
    the two grippers (the file's header has the made-up radii); pairs: every one of the default rule, weight 30;
    margin 0.  48 steps at lr 0.05, the iterate projected.  (Seed 1: the first one tried; none was rejected.)"""
    s = _Hu()
    rng = np.random.default_rng(1)
    B = 64
    a0, q, t, P = _rest(s, B)
    w = np.full(s.J, 0.05, np.float32)
    w[list(WRISTS)] = 1.0
    centre = P[0, TORSO] + np.array([0.0, 0.0, 0.25])
    point = centre + np.array([0.22, 0.0, 0.0]) + rng.uniform(-1, 1, (B, 3)) * np.array([0.08, 0.10, 0.12])
    tgt = P.copy()
    tgt[:, list(WRISTS)] = point[:, None]
    links = [TORSO, *WRISTS, *GRIPPERS]
    spheres = [[0, 0, 0.25, 0.16], [0, 0, 0, 0.05], [0, 0, 0, 0.05], [0.08, 0, 0, 0.04], [0.08, 0, 0, 0.04]]
    par = [int(p) for p in s.par]
    pairs = [(a, b) for a in range(5) for b in range(a + 1, 5)
             if not (links[a] == links[b] or par[links[a]] == links[b] or par[links[b]] == links[a])]
    ap = spec(links, spheres, pairs, np.full(len(pairs), 30.0, np.float32))
    return s, dict(tgt=tgt.astype(np.float32), q=q, t=t, start=a0, w=w, ap=ap, iters=48, lr=0.05, fit_root=0)


def floor_recipe():
    """The pinned floor recipe: 33-link Hu, B = 64, the root given as identity, clip on, the start at zero angles.
    Targets: the rest pose at weight 1, the floor z = h0 drawn per recipe 0.12 m above the rest pose's ankles -- so both
    ankle targets lie under it and the knees have to bend.  Spheres: 0.05 m on both ankles (links 6 and 12), no pairs;
    floor_weight 30; 48 steps at lr 0.05, the iterate projected."""
    s = _Hu()
    B = 64
    rng = np.random.default_rng(1)
    a0, q, t, P = _rest(s, B)
    tgt = P + rng.normal(0, 0.01, P.shape)
    h0 = float(P[0, ANKLES[0], 2] + 0.12)
    ap = spec(list(ANKLES), [[0, 0, 0, 0.05]] * 2, plane=[0, 0, 1, h0], mask=3, wf=30.0)
    return s, dict(tgt=tgt.astype(np.float32), q=q, t=t, start=a0, w=np.ones(s.J, np.float32), ap=ap, iters=48, lr=0.05, fit_root=0)


@functools.lru_cache(maxsize=None)
def ref_outcome(which, dtype=torch.float64):
    """-> {with the term: (per-frame deepest penetration, per-frame loss with the term's part, angles)}."""
    s, x = hands_recipe() if which == "hands" else floor_recipe()
    out = {}
    for on in (False, True):
        fit = RefApartFit(s, x["start"], x["q"], x["t"], x["w"], True, dtype, x["fit_root"], x["ap"] if on else None,
                          project=True, lr=x["lr"]).run(x["tgt"], x["iters"])
        loss, a, q, t = fit.result(x["tgt"])
        out[on] = (penetration(s, a, q, t, True, x["fit_root"], x["ap"]), loss, a)
    return out


@pytest.mark.parametrize("which", ["hands", "floor"])
def test_the_term_keeps_the_robot_out_of_itself_and_of_the_floor(which):
    """The float64 loop on the two recipes: the deepest penetration over the 64 frames with the term is at most a
    quarter of that without.  Measured: hands 0.0952 m without, 0.0072 m with (13.2 times); floor 0.1717 m without,
    0.0213 m with (8.1 times)."""
    out = ref_outcome(which)
    without, with_ = out[False][0].max(), out[True][0].max()
    print(f"{which} recipe, float64 loop: deepest penetration without the term {without:.4f} m, with it {with_:.4f} m "
          f"({without / with_:.1f} times); frames that overlap without {np.mean(out[False][0] > 0):.2f}, with "
          f"{np.mean(out[True][0] > 1e-3):.2f}")
    assert without > 0.05
    assert with_ <= 0.25 * without

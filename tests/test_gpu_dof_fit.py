"""GPU: the fused keypoint fit (rtg_dof_fit_f32: forward model, weighted keypoint loss, gradient and Adam in one
launch) against the torch restatement of tests/test_fk_grad_host.py wrapped in that loss and in torch.optim.Adam, on
the CPU in float64 and float32.

The criterion is the project's own, per tensor: E(x) = max|x - x64| / max|x64|, and E(gpu) <= 8 max(E(restatement
f32), 2^-24) -- the GPU may err like float32 torch does, not more.  The Adam step is checked on its own against the
update formula in float64 on the GPU's own gradient, and everything that has to hold bit for bit (chained launches,
batch and tile independence, repeatability, aliasing, a bad frame staying in its rows) is checked bit for bit."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_fk_grad_host import dof_fk, fixture_case, rel_err

pytestmark = pytest.mark.gpu

FACTOR = 8.0
FLOOR = 2.0 ** -24
U = 2.0 ** -24   # the relative half-ulp of float32
LR, B1, B2, EPS = 0.02, 0.9, 0.999, 1e-8


# ------------------------------------------------------------------ skeletons
class Skel:
    def __init__(self, name, par, lt, axis, lo, hi):
        self.name, self.par, self.lt, self.axis, self.lo, self.hi = name, np.asarray(par, np.int32), lt, axis, lo, hi
        self.J = len(self.par)
        self.F = 16 if self.J <= 36 else 8
        self._model = None

    @property
    def model(self):
        if self._model is None:
            from rtg.runtime import DofModel, Topology
            self._model = DofModel(Topology(self.par, self.lt), self.axis, self.lo, self.hi)
        return self._model

    def batches(self):
        F = self.F
        return (1, F - 1, F, F + 1, 4 * F + 3)

    def strict_subtree_weight(self, w):
        """Per DOF (joint j >= 1): the largest weight among joint j's strict descendants (a_j moves only those)."""
        s = np.zeros(self.J)
        for j in range(self.J - 1, 0, -1):
            p = self.par[j]
            s[p] = max(s[p], s[j], abs(w[j]))
        return s[1:]


def _random_skel(name, par, seed):
    rng = np.random.default_rng(seed)
    J = len(par)
    return Skel(name, par, rng.normal(0, 0.3, (J, 3)).astype(np.float32), rng.integers(0, 3, J - 1).astype(np.int32),
                (-0.5 - rng.uniform(0, 1, J - 1)).astype(np.float32), (0.5 + rng.uniform(0, 1, J - 1)).astype(np.float32))


def _make(name):
    if name == "hu33":
        _, _, (par, lt, axis, lo, hi), _, _, _ = fixture_case(golden("fk_grad"), "hu_clip")
        return Skel(name, par, lt, axis, lo, hi)
    if name == "vtrdyn59":
        from rtg import assets
        s = _random_skel(name, assets.parents("vtrdyn_full"), 59)
        s.lt = np.ascontiguousarray(assets.local_translation("vtrdyn_full"), np.float32).reshape(-1, 3)
        return s
    par = {"one": [-1], "two": [-1, 0], "star61": [-1] + [0] * 60, "chain64": list(range(-1, 63)),
           "tree37": [-1] + [(j - 1) // 2 for j in range(1, 37)]}[name]
    return _random_skel(name, par, 100 + len(par))


SKELS = ("hu33", "vtrdyn59", "one", "two", "star61", "chain64", "tree37")
_CACHE = {}


def skel(name):
    if name not in _CACHE:
        _CACHE[name] = _make(name)
    return _CACHE[name]


# ------------------------------------------------------------------ the reference: restatement + loss (+ Adam)
def _t(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def ref_positions(s, dof, rr, rt, clip, dtype):
    lo, hi = (_t(s.lo, dtype), _t(s.hi, dtype)) if clip else (None, None)
    return dof_fk(dof, _t(rr, dtype), _t(rt, dtype), [int(p) for p in s.par], _t(s.lt, dtype), s.axis, lo, hi)[1]


def ref_loss(s, dof, rr, rt, tgt, w, clip, dtype):
    gp = ref_positions(s, dof, rr, rt, clip, dtype)
    return (_t(w, dtype).reshape(1, -1, 1) * (gp - _t(tgt, dtype)) ** 2).sum(dim=(-1, -2))


def ref_loss_grad(s, dof, rr, rt, tgt, w, clip, dtype):
    a = _t(dof, dtype).requires_grad_(True)
    loss = ref_loss(s, a, rr, rt, tgt, w, clip, dtype)
    if a.numel():
        loss.sum().backward()
    return loss.detach().numpy(), (torch.zeros_like(a) if a.grad is None else a.grad).numpy()


# ------------------------------------------------------------------ the launch, straight through the C ABI
def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def fit(s, tgt, w, rr, rt, dof, clip, iters=0, lr=LR, betas=(B1, B2), eps=EPS, step0=0, m=None, v=None, alias=False,
        want=("dof", "loss", "grad"), status=False):
    """rtg_dof_fit_f32 on host arrays -> dict of host arrays (dof, loss, grad, m, v)."""
    from rtg import _lib
    from rtg.runtime import ptr
    B, n = tgt.shape[0], s.J - 1
    d_in = _dev(dof)
    bufs = dict(tp=_dev(tgt), w=_dev(w), rr=_dev(rr), rt=_dev(rt), m=_dev(m), v=_dev(v))
    out = {"dof": d_in if alias else torch.full((B, n), 7.0, device="cuda") if "dof" in want else None,
           "loss": torch.full((B,), 7.0, device="cuda") if "loss" in want else None,
           "grad": torch.full((B, n), 7.0, device="cuda") if "grad" in want else None}
    rc = _lib.lib().rtg_dof_fit_f32(s.model.handle, ptr(bufs["tp"]), ptr(bufs["w"]), ptr(bufs["rr"]), ptr(bufs["rt"]),
                                    ptr(d_in), B, int(clip), iters, lr, betas[0], betas[1], eps, step0, ptr(bufs["m"]),
                                    ptr(bufs["v"]), ptr(out["dof"]), ptr(out["loss"]), ptr(out["grad"]), None)
    if status:
        return rc, _lib.lib().rtg_last_error()
    assert rc == 0, _lib.lib().rtg_last_error()
    torch.cuda.synchronize()
    res = {k: _np(x) for k, x in out.items()}
    res["m"], res["v"] = _np(bufs["m"]), _np(bufs["v"])
    return res


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(a, b, what=""):
    for k in a:
        if a[k] is not None:
            np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=f"{what} {k}")


def _scaled_quats(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return (q * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)


def inputs(s, B, clip, seed):
    """clip off: angles in +-3 pi (the w < 0 flips occur); clip on: most angles outside the limits; root norms 0.5-2;
    random weights, a third of them 0."""
    rng = np.random.default_rng(seed)
    n = s.J - 1
    if clip:
        dof = np.where(rng.random((B, n)) < 0.8,
                       np.where(rng.random((B, n)) < 0.5, s.lo - rng.uniform(0.2, 4, (B, n)), s.hi + rng.uniform(0.2, 4, (B, n))),
                       rng.uniform(s.lo, s.hi, (B, n))).astype(np.float32)
    else:
        dof = rng.uniform(-3 * np.pi, 3 * np.pi, (B, n)).astype(np.float32)
    w = rng.uniform(0.2, 2.0, s.J).astype(np.float32)
    w[rng.permutation(s.J)[: s.J // 3]] = 0.0
    return dict(dof=dof, rr=_scaled_quats(rng, B), rt=rng.normal(0, 0.3, (B, 3)).astype(np.float32),
                tgt=rng.normal(0, 0.5, (B, s.J, 3)).astype(np.float32), w=w)


def check_criterion(what, got, ref32, ref64):
    if np.asarray(ref64).size == 0:
        assert np.asarray(got).size == 0
        return
    if not np.asarray(ref64).any():   # nothing to be relative to (every DOF a leaf's): the zeros are owed exactly
        assert not np.asarray(got).any(), what
        return
    e, er = rel_err(got, ref64), rel_err(ref32, ref64)
    print(f"{what}: E(gpu) {e:.3e}  E(restatement f32) {er:.3e}  ratio {e / max(er, FLOOR):.2f}")
    assert e <= FACTOR * max(er, FLOOR), (what, e, er)


# ------------------------------------------------------------------ 1. evaluate
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", SKELS)
def test_evaluate_against_the_restatement(gpu, name, clip):
    s = skel(name)
    Bm = max(s.batches())
    x = inputs(s, Bm, clip, 7 * s.J + clip)
    l64, g64 = ref_loss_grad(s, x["dof"], x["rr"], x["rt"], x["tgt"], x["w"], clip, torch.float64)
    l32, g32 = ref_loss_grad(s, x["dof"], x["rr"], x["rt"], x["tgt"], x["w"], clip, torch.float32)
    if clip and s.J > 2:
        assert ((x["dof"] < s.lo) | (x["dof"] > s.hi)).mean() > 0.6
    zero_dof = s.strict_subtree_weight(x["w"]) == 0
    if s.J > 2:
        assert zero_dof.any()
    full = None
    for B in sorted(s.batches(), reverse=True):
        r = fit(s, x["tgt"][:B], x["w"], x["rr"][:B], x["rt"][:B], x["dof"][:B], clip)
        assert r["loss"].shape == (B,) and r["grad"].shape == (B, s.J - 1)
        check_criterion(f"{name} clip={clip} B={B} loss", r["loss"], l32[:B], l64[:B])
        check_criterion(f"{name} clip={clip} B={B} grad", r["grad"], g32[:B], g64[:B])
        np.testing.assert_array_equal(bits(r["dof"]), bits(x["dof"][:B]))       # iters = 0: dof_out is dof_in
        assert (r["grad"][:, zero_dof] == 0).all()                              # exactly +-0, not noise
        if full is None:
            full = r
        for k in ("loss", "grad"):                                              # a smaller batch is its leading frames
            np.testing.assert_array_equal(bits(r[k]), bits(full[k][:B]))


@pytest.mark.parametrize("name", ["hu33", "vtrdyn59"])
def test_evaluate_properties(gpu, name):
    from rtg import ops
    s = skel(name)
    B = 4 * s.F + 3
    x = inputs(s, B, True, 11)
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    # all weights 0: loss 0, gradient 0
    r = fit(s, x["tgt"], np.zeros(s.J, np.float32), x["rr"], x["rt"], x["dof"], True)
    assert (r["loss"] == 0).all() and (r["grad"] == 0).all()
    # weight = NULL is weight = 1
    assert_same_bits(fit(s, x["tgt"], None, *args[2:]), fit(s, x["tgt"], np.ones(s.J, np.float32), *args[2:]))
    # outputs are optional one by one
    r = fit(s, *args)
    assert_same_bits(fit(s, *args, want=("loss",)), {"loss": r["loss"]})
    assert_same_bits(fit(s, *args, want=("grad",)), {"grad": r["grad"]})
    # ops.keypoint_loss: the same launch under autograd
    a = _dev(x["dof"]).requires_grad_(True)
    loss = ops.keypoint_loss(s.model, a, x["tgt"], x["rr"], x["rt"], weight=x["w"], clip=True)
    assert loss.shape == (B,) and loss.grad_fn is not None
    np.testing.assert_array_equal(bits(_np(loss)), bits(r["loss"]))
    loss.sum().backward()
    np.testing.assert_array_equal(bits(_np(a.grad)), bits(r["grad"]))
    c = torch.linspace(-2.0, 3.0, B, device="cuda")
    a.grad = None
    (ops.keypoint_loss(s.model, a, x["tgt"], x["rr"], x["rt"], weight=x["w"], clip=True) * c).sum().backward()
    assert torch.equal(a.grad, _dev(r["grad"]) * c[:, None])                     # scaled row by row
    with torch.no_grad():
        plain = ops.keypoint_loss(s.model, a, x["tgt"], x["rr"], x["rt"], weight=x["w"], clip=True)
    assert plain.grad_fn is None and torch.equal(plain, loss.detach())
    a1 = _dev(x["dof"][..., None]).requires_grad_(True)                          # the reference's (L, J-1, 1) angles
    ops.keypoint_loss(s.model, a1, x["tgt"], x["rr"][:, None], x["rt"], weight=x["w"], clip=True).sum().backward()
    assert a1.grad.shape == (B, s.J - 1, 1)
    np.testing.assert_array_equal(bits(_np(a1.grad)[..., 0]), bits(r["grad"]))


def test_unsupported_and_rejected(gpu):
    from rtg import _lib
    big = _random_skel("chain65", list(range(-1, 64)), 65)
    x = inputs(big, 3, False, 1)
    rc, msg = fit(big, x["tgt"], None, x["rr"], x["rt"], x["dof"], False, status=True)
    assert rc == 4 and b"1..64 joints" in msg                                    # RTG_ERR_UNSUPPORTED
    s = skel("two")
    nolim = Skel("two_nolimits", s.par, s.lt, s.axis, None, None)
    x = inputs(s, 3, False, 2)
    rc, msg = fit(nolim, x["tgt"], None, x["rr"], x["rt"], x["dof"], True, status=True)
    assert rc == 1 and b"no DOF limits" in msg
    rc, _ = fit(nolim, x["tgt"][:0], None, x["rr"][:0], x["rt"][:0], x["dof"][:0], False, status=True)
    assert rc == 0                                                               # B == 0: a no-op


# ------------------------------------------------------------------ 2. the Adam step alone
@pytest.mark.parametrize("name", ["hu33", "chain64"])
def test_one_adam_step_against_the_formula(gpu, name):
    """iters = 1 from a random state (v0 >= m0^2, five steps taken) against the update formula in float64 on the GPU's
    own iters = 0 gradient, with the hyper-parameters as the launch receives them (float32).  The chain from g to the
    new angle has at most eight float32 roundings: |delta| <= 8 2^-24 (|a_old| + |update|) per element.  The moments
    see at most two roundings per term."""
    s = skel(name)
    B, step0 = 4 * s.F + 3, 5
    x = inputs(s, B, True, 21)
    rng = np.random.default_rng(22)
    m0 = rng.normal(0, 1.0, x["dof"].shape).astype(np.float32)
    v0 = (m0.astype(np.float64) ** 2 * rng.uniform(1.0, 3.0, m0.shape) + 1e-3).astype(np.float32)
    assert (v0 >= m0 * m0).all()
    args = (x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True)
    g = fit(s, *args)["grad"].astype(np.float64)
    r = fit(s, *args, iters=1, step0=step0, m=m0, v=v0)
    lr, b1, b2, eps = (float(np.float32(h)) for h in (LR, B1, B2, EPS))
    t = step0 + 1
    m = b1 * m0 + (1 - b1) * g
    v = b2 * v0 + (1 - b2) * g * g
    upd = lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    a_old = x["dof"].astype(np.float64)
    excess = np.abs(r["dof"] - (a_old - upd)) / (U * (np.abs(a_old) + np.abs(upd)))
    print(f"{name}: Adam step, max |delta| / (2^-24 (|a_old| + |update|)) = {excess.max():.2f} (bound 8)")
    assert excess.max() <= 8
    assert (np.abs(r["m"] - m) <= 2 * U * (np.abs(b1 * m0) + np.abs((1 - b1) * g))).all()
    assert (np.abs(r["v"] - v) <= 2 * U * v).all()
    assert np.abs(upd).max() > 1e-3                                              # the step is not a no-op


def test_zero_gradient_and_zero_state_leave_the_bits(gpu):
    s = skel("hu33")
    B = 4 * s.F + 3
    x = inputs(s, B, True, 31)
    dof = x["dof"].copy()
    dof[0, :4] = [-0.0, 0.0, 1e-42, -1e30]
    w0 = np.zeros(s.J, np.float32)
    z = np.zeros_like(dof)
    for kw in (dict(m=z, v=z), dict()):                                          # explicit zero state, and none
        r = fit(s, x["tgt"], w0, x["rr"], x["rt"], dof, True, iters=3, **kw)
        np.testing.assert_array_equal(bits(r["dof"]), bits(dof))
    # and with weights: only the DOFs that carry none (the leaf DOFs among them) stay
    r = fit(s, x["tgt"], x["w"], x["rr"], x["rt"], dof, True, iters=3)
    still = s.strict_subtree_weight(x["w"]) == 0
    assert still.any() and not still.all()
    np.testing.assert_array_equal(bits(r["dof"][:, still]), bits(dof[:, still]))
    # (a DOF can carry weight and still have no gradient -- Hu has co-located joints -- so "moves" is asked of the
    # elements whose float64 gradient at the start is not small; Adam's first step there is lr whatever its size)
    _, g64 = ref_loss_grad(s, dof[1:], x["rr"][1:], x["rt"][1:], x["tgt"][1:], x["w"], True, torch.float64)
    moves = np.abs(g64) > 1e-3 * np.abs(g64).max()
    assert moves.mean() > 0.5 and not moves[:, still].any()
    assert (bits(r["dof"][1:]) != bits(dof[1:]))[moves].all()


# ------------------------------------------------------------------ 3. self-consistency, bit for bit
@pytest.mark.parametrize("name", ["hu33", "vtrdyn59", "tree37"])
def test_self_consistency(gpu, name):
    s = skel(name)
    F = s.F
    B = 4 * F + 3
    x = inputs(s, B, True, 41)
    rng = np.random.default_rng(42)
    m0 = rng.normal(0, 0.1, x["dof"].shape).astype(np.float32)
    v0 = (m0 * m0 + 1e-4).astype(np.float32)
    args = (x["tgt"], x["w"], x["rr"], x["rt"])
    one = fit(s, *args, x["dof"], True, iters=8, step0=3, m=m0, v=v0)
    # two identical launches
    assert_same_bits(one, fit(s, *args, x["dof"], True, iters=8, step0=3, m=m0, v=v0), "repeat")
    # eight launches of one step, carrying (m, v, step)
    st = dict(dof=x["dof"], m=m0, v=v0)
    for k in range(8):
        st = fit(s, *args, st["dof"], True, iters=1, step0=3 + k, m=st["m"], v=st["v"])
    assert_same_bits(one, st, "chained")
    # dof_out aliasing dof_in
    assert_same_bits(one, fit(s, *args, x["dof"], True, iters=8, step0=3, m=m0, v=v0, alias=True), "alias")
    # a frame of the large launch is that frame run alone
    for f in (0, F - 1, 2 * F + 1, B - 1):
        alone = fit(s, x["tgt"][f:f + 1], x["w"], x["rr"][f:f + 1], x["rt"][f:f + 1], x["dof"][f:f + 1], True, iters=8,
                    step0=3, m=m0[f:f + 1], v=v0[f:f + 1])
        assert_same_bits(alone, {k: a[f:f + 1] for k, a in one.items()}, f"frame {f}")
    # no state given: starts at zero, as an explicit zero state does
    z = np.zeros_like(m0)
    a, b = fit(s, *args, x["dof"], True, iters=4), fit(s, *args, x["dof"], True, iters=4, m=z, v=z)
    assert a["m"] is None and a["v"] is None
    assert_same_bits({k: a[k] for k in ("dof", "loss", "grad")}, b, "no state")


def test_python_entry_points_chain(gpu):
    from rtg import ops
    from robot_kinematics_model import RobotZeroPose
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    s = skel("hu33")
    x = inputs(s, 19, True, 51)
    kw = dict(weight=x["w"], lr=LR, clip=True)
    dof8, loss8, st8, grad8 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, return_grad=True, **kw)
    d4, _, st4 = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=4, **kw)
    d8, l8, st = ops.dof_fit(s.model, x["tgt"], x["rr"], x["rt"], d4, iters=4, state=st4, **kw)
    assert st[2] == st8[2] == 8 and st4[2] == 4
    assert torch.equal(d8, dof8) and torch.equal(l8, loss8) and torch.equal(st[0], st8[0]) and torch.equal(st[1], st8[1])
    r = fit(s, x["tgt"], x["w"], x["rr"], x["rt"], x["dof"], True, iters=8)
    np.testing.assert_array_equal(bits(_np(dof8)), bits(r["dof"]))
    np.testing.assert_array_equal(bits(_np(grad8)), bits(r["grad"]))
    # the drop-in: the reference's shapes, results on the inputs' device
    hu = HuForwardModel(RobotZeroPose.from_asset("hu").skeleton_tree)
    tgt, rt, rr = torch.from_numpy(x["tgt"]), torch.from_numpy(x["rt"]), torch.from_numpy(x["rr"][:, None])
    ang, loss, state = hu.fit_keypoints(tgt, rt, rr, torch.from_numpy(x["dof"][..., None]), iters=8, lr=LR)
    assert ang.shape == (19, 32, 1) and loss.shape == (19,) and ang.device.type == "cpu" and state[2] == 8
    want, wl, _ = ops.dof_fit(hu._model, x["tgt"], x["rr"], x["rt"], x["dof"], iters=8, lr=LR, clip=True)
    assert torch.equal(ang[..., 0], want.cpu()) and torch.equal(loss, wl.cpu())
    ang0, _, _ = hu.fit_keypoints(tgt, rt, rr, iters=0)                          # default start: zeros
    assert ang0.shape == (19, 32, 1) and not ang0.any()


# ------------------------------------------------------------------ 4. outcome
@pytest.fixture(scope="module")
def outcome():
    """33-link Hu, B = 128, clip on, weights 1; targets: the FK of angles uniform inside the limits; start: mid-range;
    the torch.optim.Adam loop on the restatement, float64 and float32, its per-frame losses after 8 and 32 steps."""
    s = skel("hu33")
    rng = np.random.default_rng(1)
    B = 128
    q = rng.normal(size=(B, 4))
    rr = (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)
    rt = rng.normal(0, 0.3, (B, 3)).astype(np.float32)
    truth = rng.uniform(s.lo, s.hi, (B, s.J - 1)).astype(np.float32)
    tgt = ref_positions(s, _t(truth, torch.float64), rr, rt, True, torch.float64).numpy().astype(np.float32)
    start = np.tile((0.5 * (s.lo + s.hi)).astype(np.float32), (B, 1))
    w = np.ones(s.J, np.float32)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        a = _t(start, dtype).clone().requires_grad_(True)   # (a float32 tensor would share the array's memory)
        opt = torch.optim.Adam([a], lr=LR, betas=(B1, B2), eps=EPS)
        for k in range(1, 33):
            opt.zero_grad()
            ref_loss(s, a, rr, rt, tgt, w, True, dtype).sum().backward()
            opt.step()
            if k in (8, 32):
                with torch.no_grad():
                    ref[dtype, k] = ref_loss(s, a, rr, rt, tgt, w, True, dtype).numpy()
        if dtype == torch.float64:
            with torch.no_grad():
                ref["start"] = ref_loss(s, _t(start, dtype), rr, rt, tgt, w, True, dtype).numpy()
    return s, dict(tgt=tgt, rr=rr, rt=rt, start=start), ref


@pytest.mark.parametrize("iters", [8, 32])
def test_outcome_against_the_torch_loop(gpu, outcome, iters):
    s, x, ref = outcome
    l64, l32 = ref[torch.float64, iters], ref[torch.float32, iters]
    e32 = rel_err(l32, l64)
    print(f"{iters} steps: reference mean loss {ref['start'].mean():.3f} -> {l64.mean():.3f}; E(loss, f32 loop) {e32:.3e}")
    assert e32 <= 1e-3                                                           # the reference itself is tame
    assert l64.mean() < ref["start"].mean()
    r = fit(s, x["tgt"], None, x["rr"], x["rt"], x["start"], True, iters=iters)
    check_criterion(f"outcome {iters} steps loss", r["loss"], l32, l64)
    print(f"{iters} steps: GPU mean loss {r['loss'].mean():.4f}, reference {l64.mean():.4f}")
    assert r["loss"].astype(np.float64).mean() <= 1.01 * l64.mean()


# ------------------------------------------------------------------ 5. a bad frame stays its own
def test_a_bad_frame_stays_its_own(gpu):
    s = skel("hu33")
    B = 3 * s.F
    f = B // 2
    x = inputs(s, B, True, 61)
    args = lambda y: (y["tgt"], y["w"], y["rr"], y["rt"], y["dof"], True)
    clean = fit(s, *args(x), iters=3)
    clean0 = fit(s, *args(x))
    assert all(np.isfinite(a).all() for a in clean.values() if a is not None)
    ok = np.arange(B) != f

    def spoil(which):
        y = {k: a.copy() for k, a in x.items()}
        if "target" in which:
            y["tgt"][f, np.flatnonzero(x["w"])[3], 1] = np.nan
        if "angle" in which:
            y["dof"][f, 2] = np.inf
        if "root" in which:
            y["rr"][f] = 0.0
        return y
    for which in (("target",), ("angle",), ("root",), ("target", "angle", "root")):
        y = spoil(which)
        bad = fit(s, *args(y), iters=3)
        for k in ("dof", "loss", "grad"):
            np.testing.assert_array_equal(bits(bad[k][ok]), bits(clean[k][ok]), err_msg=f"{which} {k}")
        bad0 = fit(s, *args(y))
        np.testing.assert_array_equal(bits(bad0["loss"][ok]), bits(clean0["loss"][ok]))
        with np.errstate(all="ignore"), torch.no_grad():
            want = ref_loss(s, _t(y["dof"][f:f + 1], torch.float64), y["rr"][f:f + 1], y["rt"][f:f + 1], y["tgt"][f:f + 1],
                            y["w"], True, torch.float64).numpy()
        assert np.isnan(bad0["loss"][f]) == np.isnan(want[0]), which
        if not np.isnan(want[0]):   # a zero root rotation: every joint at the root translation, a finite loss -- a
            # sum of 99 non-negative float32 terms, each a few roundings: well within 1e-5 relative
            assert abs(bad0["loss"][f] - want[0]) <= 1e-5 * abs(want[0])


@pytest.mark.parametrize("name", ["hu33", "tree37"])
@pytest.mark.parametrize("iters", [0, 3])
def test_targets_at_any_alignment(gpu, name, iters):
    """target_pos 4 bytes into its buffer: the target rows then come in dword by dword instead of as dwordx4 pieces,
    and loss and gradient (iters = 0), angles and moments (iters = 3) keep the bits of the aligned call.  One whole
    tile plus a one-frame tile of both lane-group shapes."""
    from rtg import _lib
    from rtg.runtime import ptr
    s = skel(name)
    B, n = s.F + 1, s.J - 1
    x = inputs(s, B, True, 7000 + s.J + iters)
    aligned = _dev(x["tgt"])
    buf = torch.empty(x["tgt"].size + 1, dtype=torch.float32, device="cuda")
    shifted = buf[1:].view(x["tgt"].shape)
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4

    def run(tp):
        w, rr, rt, dof = _dev(x["w"]), _dev(x["rr"]), _dev(x["rt"]), _dev(x["dof"])
        m, v = torch.zeros((B, n), device="cuda"), torch.zeros((B, n), device="cuda")
        out = {k: torch.full(sh, 7.0, device="cuda") for k, sh in (("dof", (B, n)), ("loss", (B,)), ("grad", (B, n)))}
        rc = _lib.lib().rtg_dof_fit_f32(s.model.handle, ptr(tp), ptr(w), ptr(rr), ptr(rt), ptr(dof), B, 1, iters, LR, B1,
                                        B2, EPS, 0, ptr(m), ptr(v), ptr(out["dof"]), ptr(out["loss"]), ptr(out["grad"]),
                                        None)
        assert rc == 0, _lib.lib().rtg_last_error()
        torch.cuda.synchronize()
        return dict({k: _np(t) for k, t in out.items()}, m=_np(m), v=_np(v))

    assert_same_bits(run(aligned), run(shifted), f"{name} iters={iters}")

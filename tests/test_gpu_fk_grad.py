"""GPU: the kinematics' gradients (rtg_dof_fk_backward_f32 / rtg_fk_backward_f32 through torch.autograd) against the
reference's float64 autograd results -- from tests/golden/fk_grad.npz, or from the torch restatement that
tests/test_fk_grad_host.py ties to that fixture.

The criterion, per gradient tensor: E(x) = max|x - g64| / max|g64|, and E(gpu) <= FACTOR x E(reference f32), both
computed here.  On tensors of a handful of elements E(reference f32) can come out below what float32 can represent at
all (even exactly 0), so it is floored at 2^-24, the relative half-ulp of the tensor's largest element; on tensors of a
few thousand elements (the fixture, the large batches) the floor never acts.  A wrong sign, a missing |q|^2 term or
a dropped sibling shows at 1e-1."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_fk_grad_host import DOF_CASES, fixture_case, rel_err, restated_grads

pytestmark = pytest.mark.gpu

FACTOR = 8.0
FIXTURE_FACTOR = 4.0   # the fixture's measured ratios are all below 2 (0.62 - 1.63): tightened from 8
FLOOR = 2.0 ** -24


def _np(t):
    return t.detach().cpu().numpy()


def _check(got, ref32, g64, what, factor=FACTOR):
    for name, x, r in zip(what[1], got, ref32):
        if g64[name].size == 0:
            assert x.size == 0
            continue
        e, er = rel_err(x, g64[name]), rel_err(r, g64[name])
        print(f"{what[0]} {name}: E(gpu) {e:.3e}  E(ref f32) {er:.3e}  ratio {e / max(er, FLOOR):.2f}")
        assert e <= factor * max(er, FLOOR), (what[0], name, e, er)


def _leaf(x, dev="cuda"):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(dev).requires_grad_(True)


def _backward(outs, cots):
    pairs = [(o, torch.as_tensor(np.asarray(c), dtype=torch.float32).cuda()) for o, c in zip(outs, cots) if c is not None]
    torch.autograd.backward([o for o, _ in pairs], [c for _, c in pairs])


def gpu_dof_grads(model, inputs, clip, cot_rot, cot_pos):
    from rtg import ops
    dof = np.asarray(inputs[0])
    leaves = [_leaf(dof[..., None]), _leaf(inputs[1]), _leaf(inputs[2])]   # the reference's (L, J-1, 1) angles
    _backward(ops.dof_forward_kinematics(model, *leaves, clip=clip), (cot_rot, cot_pos))
    return [_np(leaves[0].grad)[..., 0], _np(leaves[1].grad), _np(leaves[2].grad)]


def gpu_fk_grads(topo, inputs, cot_rot, cot_pos):
    from rtg import ops
    leaves = [_leaf(x) for x in inputs]
    _backward(ops.forward_kinematics(topo, *leaves), (cot_rot, cot_pos))
    return [_np(x.grad) for x in leaves]


def _model(consts):
    from rtg.runtime import DofModel, Topology
    par, lt, axis, lo, hi = consts
    return DofModel(Topology(par, lt), axis, lo, hi)


@pytest.mark.parametrize("tag", DOF_CASES + ("vtrdyn_full",))
def test_fixture_cases(gpu, tag):
    from rtg.runtime import Topology
    d = golden("fk_grad")
    kind, inputs, consts, cr, cp, names = fixture_case(d, tag)
    if kind == "dof":
        got = gpu_dof_grads(_model(consts), inputs, consts[3] is not None, cr, cp)
    else:
        got = gpu_fk_grads(Topology(consts[0], consts[1]), inputs, cr, cp)
    _check(got, [d[f"{tag}_grad_{n}_f32"] for n in names], {n: d[f"{tag}_grad_{n}_f64"] for n in names}, (tag, names),
           factor=FIXTURE_FACTOR)


def _tree(kind, J):
    if kind == "chain":
        return np.arange(-1, J - 1, dtype=np.int32)
    if kind == "star":   # every joint a child of the root: J - 1 siblings
        return np.array([-1] + [0] * (J - 1), np.int32)
    return np.array([-1] + [(j - 1) // 2 for j in range(1, J)], np.int32)   # bushy: a binary tree


def _scaled_quats(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return (q * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)


BATCHES = (1, 15, 16, 17, 4097)   # partial tiles of both lane-group shapes (16 and 8 frames), and many tiles


@pytest.mark.parametrize("kind", ["chain", "bushy", "star"])
@pytest.mark.parametrize("J", [1, 2, 31, 36, 37, 64, 65, 97])
def test_random_trees_through_the_restatement(gpu, J, kind):
    """Both lane-group shapes and their limits (J <= 36: 16 frames per wave, J <= 64: 8), the lane walk (J = 65, 97),
    one joint (no DOFs), clip off and on, every batch size; plain FK on the same tree.  The float64 and float32
    references are computed once for the largest batch; frames are independent, so a smaller batch is its leading
    frames (and the device rows of a smaller batch must be the bits of those frames in the largest)."""
    from rtg.runtime import DofModel, Topology
    rng = np.random.default_rng(1000 + 10 * J + len(kind))
    par = _tree(kind, J)
    lt = rng.normal(0, 0.3, (J, 3)).astype(np.float32)
    axis = rng.integers(0, 3, J - 1).astype(np.int32)
    lo = (-0.5 - rng.uniform(0, 1, J - 1)).astype(np.float32)
    hi = (0.5 + rng.uniform(0, 1, J - 1)).astype(np.float32)
    Bm = max(BATCHES)
    dof = rng.uniform(-3 * np.pi, 3 * np.pi, (Bm, J - 1)).astype(np.float32)
    rr = _scaled_quats(rng, Bm)
    rt = rng.normal(0, 0.3, (Bm, 3)).astype(np.float32)
    cr = rng.normal(size=(Bm, J, 4)).astype(np.float32)
    cp = rng.normal(size=(Bm, J, 3)).astype(np.float32)
    topo = Topology(par, lt)
    model = DofModel(topo, axis, lo, hi)
    names = ("dof", "root_rot", "root_t")
    for clip in (False, True):
        consts = (par, lt, axis, lo if clip else None, hi if clip else None)
        _, g64 = restated_grads("dof", [dof, rr, rt], consts, cr, cp, torch.float64)
        _, g32 = restated_grads("dof", [dof, rr, rt], consts, cr, cp, torch.float32)
        full = None
        for B in sorted(BATCHES, reverse=True):
            got = gpu_dof_grads(model, [dof[:B], rr[:B], rt[:B]], clip, cr[:B], cp[:B])
            assert got[0].shape == (B, J - 1) and got[1].shape == (B, 4) and got[2].shape == (B, 3)
            _check(got, [g[:B] for g in g32], {n: g[:B] for n, g in zip(names, g64)},
                   (f"{kind} J={J} B={B} clip={clip}", names))
            if full is None:
                full = got
            for a, b in zip(got, full):
                np.testing.assert_array_equal(a, b[:B])
    lr = np.ascontiguousarray(_scaled_quats(rng, Bm * J).reshape(Bm, J, 4))
    _, g64 = restated_grads("fk", [lr, rt], (par, lt), cr, cp, torch.float64)
    _, g32 = restated_grads("fk", [lr, rt], (par, lt), cr, cp, torch.float32)
    for B in (Bm, 17):
        got = gpu_fk_grads(topo, [lr[:B], rt[:B]], cr[:B], cp[:B])
        _check(got, [g[:B] for g in g32], {n: g[:B] for n, g in zip(("local_rot", "root_t"), g64)},
               (f"fk {kind} J={J} B={B}", ("local_rot", "root_t")))


@pytest.fixture(scope="module")
def hu_clip():
    d = golden("fk_grad")
    kind, inputs, consts, cr, cp, names = fixture_case(d, "hu_clip")
    return inputs, consts, cr, cp


def test_absent_cotangent_equals_explicit_zeros(gpu, hu_clip):
    """A loss on positions only (or rotations only) takes the NULL path -- the missing gradient is neither read nor
    zero-filled -- and gives the bits of the run with an explicit zero tensor."""
    from rtg.runtime import Topology
    inputs, consts, cr, cp = hu_clip
    model = _model(consts)
    for a, b in (((None, cp), (np.zeros_like(cr), cp)), ((cr, None), (cr, np.zeros_like(cp)))):
        assert np.abs(gpu_dof_grads(model, inputs, True, *a)[0]).max() > 0
        for x, y in zip(gpu_dof_grads(model, inputs, True, *a), gpu_dof_grads(model, inputs, True, *b)):
            np.testing.assert_array_equal(x, y)
    d = golden("fk_grad")
    _, inputs, consts, cr, cp, _ = fixture_case(d, "vtrdyn_full")
    topo = Topology(consts[0], consts[1])
    for a, b in (((None, cp), (np.zeros_like(cr), cp)), ((cr, None), (cr, np.zeros_like(cp)))):
        for x, y in zip(gpu_fk_grads(topo, inputs, *a), gpu_fk_grads(topo, inputs, *b)):
            np.testing.assert_array_equal(x, y)


def test_straight_through_clip(gpu, hu_clip):
    """Every angle clamped: grad_dof is the gradient at the clamped angle passed through unchanged, not zero."""
    inputs, consts, cr, cp = hu_clip
    par, lt, axis, lo, hi = consts
    rng = np.random.default_rng(5)
    dof = np.where(rng.random(inputs[0].shape) < 0.5, lo - rng.uniform(0.5, 6, inputs[0].shape),
                   hi + rng.uniform(0.5, 6, inputs[0].shape)).astype(np.float32)
    ins = [dof, inputs[1], inputs[2]]
    _, g64 = restated_grads("dof", ins, consts, cr, cp, torch.float64)
    _, g32 = restated_grads("dof", ins, consts, cr, cp, torch.float32)
    got = gpu_dof_grads(_model(consts), ins, True, cr, cp)
    assert (got[0] != 0).mean() > 0.99
    names = ("dof", "root_rot", "root_t")
    _check(got, g32, dict(zip(names, g64)), ("all clamped", names))


@pytest.mark.parametrize("norm", [0.5, 2.0])
def test_non_unit_root_rotation(gpu, hu_clip, norm):
    inputs, consts, cr, cp = hu_clip
    rr = inputs[1] / np.linalg.norm(inputs[1], axis=-1, keepdims=True) * np.float32(norm)
    ins = [inputs[0], rr.astype(np.float32), inputs[2]]
    _, g64 = restated_grads("dof", ins, consts, cr, cp, torch.float64)
    _, g32 = restated_grads("dof", ins, consts, cr, cp, torch.float32)
    names = ("dof", "root_rot", "root_t")
    _check(gpu_dof_grads(_model(consts), ins, True, cr, cp), g32, dict(zip(names, g64)), (f"|root| = {norm}", names))


def _star_case(B, J=61):
    from rtg.runtime import DofModel, Topology
    rng = np.random.default_rng(77)
    par = _tree("star", J)
    lt = rng.normal(0, 0.3, (J, 3)).astype(np.float32)
    model = DofModel(Topology(par, lt), rng.integers(0, 3, J - 1).astype(np.int32))
    ins = [rng.uniform(-3 * np.pi, 3 * np.pi, (B, J - 1)).astype(np.float32), _scaled_quats(rng, B),
           rng.normal(0, 0.3, (B, 3)).astype(np.float32)]
    return model, ins, rng.normal(size=(B, J, 4)).astype(np.float32), rng.normal(size=(B, J, 3)).astype(np.float32)


def test_two_runs_are_bit_identical(gpu):
    """60 siblings per step under one parent: the parent pulls them in index order, so no sum depends on timing."""
    model, ins, cr, cp = _star_case(4097)
    a = gpu_dof_grads(model, ins, False, cr, cp)
    b = gpu_dof_grads(model, ins, False, cr, cp)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_a_bad_frame_stays_in_its_rows(gpu):
    """One frame with a NaN angle, one with an inf cotangent (the same tile, and a tile of their own): only those
    frames' gradient rows are non-finite, every other row has the bits of the clean run."""
    model, ins, cr, cp = _star_case(100, J=31)
    clean = gpu_dof_grads(model, ins, False, cr, cp)
    bad = [x.copy() for x in ins]
    bcr, bcp = cr.copy(), cp.copy()
    bad[0][5, 7] = np.nan
    bcp[9, 3, 1] = np.inf
    bad[0][40, 0] = np.nan
    bcr[70, 30, 2] = np.inf
    hit = [5, 9, 40, 70]
    ok = np.setdiff1d(np.arange(100), hit)
    got = gpu_dof_grads(model, bad, False, bcr, bcp)
    for g, c in zip(got, clean):
        np.testing.assert_array_equal(g[ok], c[ok])
        assert np.isfinite(c).all()
    for f in hit:   # (the root translation's gradient is a plain sum of cotangents: a NaN angle leaves it finite)
        assert not all(np.isfinite(g[f]).all() for g in got), f


def test_forward_is_the_same_launch(gpu, hu_clip):
    """Outputs under autograd have the bits of the plain call; without a requires_grad input nothing is recorded."""
    from rtg import ops
    from rtg.runtime import Topology
    inputs, consts, cr, cp = hu_clip
    model = _model(consts)
    plain = ops.dof_forward_kinematics(model, *inputs, clip=True)
    assert all(o.grad_fn is None and not o.requires_grad for o in plain)
    rec = ops.dof_forward_kinematics(model, *[_leaf(x) for x in inputs], clip=True)
    assert all(o.grad_fn is not None for o in rec)
    for a, b in zip(plain, rec):
        assert torch.equal(a, b.detach())
    with torch.no_grad():
        off = ops.dof_forward_kinematics(model, *[_leaf(x) for x in inputs], clip=True)
    assert all(o.grad_fn is None for o in off)
    d = golden("fk_grad")
    _, inputs, consts, _, _, _ = fixture_case(d, "vtrdyn_full")
    topo = Topology(consts[0], consts[1])
    plain = ops.forward_kinematics(topo, *inputs)
    assert all(o.grad_fn is None for o in plain)
    rec = ops.forward_kinematics(topo, *[_leaf(x) for x in inputs])
    assert all(o.grad_fn is not None for o in rec)
    for a, b in zip(plain, rec):
        assert torch.equal(a, b.detach())
    st = ops.forward_kinematics(topo, *[_leaf(x) for x in inputs], state=True)   # out of scope: not differentiable
    assert all(o.grad_fn is None for o in st)


def test_dropin_models_backpropagate(gpu, hu_clip):
    """HuForwardModel.forward_kinematics with a CPU leaf of the reference's (L, J-1, 1) shape and clip_angles=True, and
    cal_forward_kinematics with a device leaf: loss.backward() fills .grad as the reference's does."""
    from robot_kinematics_model import RobotZeroPose, cal_forward_kinematics
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    inputs, consts, _, _ = hu_clip
    L, n = inputs[0].shape
    m = HuForwardModel(RobotZeroPose.from_asset("hu").skeleton_tree)
    ang = torch.from_numpy(inputs[0].copy()).reshape(L, n, 1).requires_grad_(True)
    rr = torch.from_numpy(inputs[1].copy()).reshape(L, 1, 4).requires_grad_(True)
    rt = torch.from_numpy(inputs[2].copy()).requires_grad_(True)
    g_rot, g_pos = m.forward_kinematics(ang, rt, rr, clip_angles=True)
    assert g_pos.device.type == "cpu"
    g_pos.square().sum().backward()
    assert ang.grad.shape == (L, n, 1) and rr.grad.shape == (L, 1, 4) and ang.grad.device.type == "cpu"

    def ref(dtype):
        leaves = [torch.from_numpy(x).to(dtype).requires_grad_(True) for x in inputs]
        from test_fk_grad_host import dof_fk
        _, gp = dof_fk(*leaves, [int(p) for p in consts[0]], torch.from_numpy(consts[1]).to(dtype), consts[2],
                       torch.from_numpy(consts[3]).to(dtype), torch.from_numpy(consts[4]).to(dtype))
        gp.square().sum().backward()
        return [x.grad.numpy() for x in leaves]
    names = ("dof", "root_rot", "root_t")
    _check([_np(ang.grad)[..., 0], _np(rr.grad)[:, 0], _np(rt.grad)], ref(torch.float32), dict(zip(names, ref(torch.float64))),
           ("HuForwardModel", names))

    d = golden("fk_grad")
    _, inputs, consts, _, _, _ = fixture_case(d, "vtrdyn_full")
    lr = torch.from_numpy(inputs[0].copy()).cuda().requires_grad_(True)
    rt = torch.from_numpy(inputs[1].copy()).cuda().requires_grad_(True)
    g_rot, g_pos = cal_forward_kinematics(lr, rt, [int(p) for p in consts[0]], torch.from_numpy(consts[1]))
    g_pos.square().sum().backward()

    def ref_fk(dtype):
        leaves = [torch.from_numpy(x).to(dtype).requires_grad_(True) for x in inputs]
        from test_fk_grad_host import fk
        _, gp = fk(*leaves, [int(p) for p in consts[0]], torch.from_numpy(consts[1]).to(dtype))
        gp.square().sum().backward()
        return [x.grad.numpy() for x in leaves]
    names = ("local_rot", "root_t")
    _check([_np(lr.grad), _np(rt.grad)], ref_fk(torch.float32), dict(zip(names, ref_fk(torch.float64))),
           ("cal_forward_kinematics", names))


def test_clip_without_limits_is_rejected(gpu):
    from rtg import _lib
    from rtg.runtime import ptr
    model, ins, cr, cp = _star_case(4, J=5)
    x = torch.zeros(64, device="cuda")
    rc = _lib.lib().rtg_dof_fk_backward_f32(model.handle, ptr(x), ptr(x), ptr(x), ptr(x), 1, 1, ptr(x), None, None, None)
    assert rc == 1 and b"no DOF limits" in _lib.lib().rtg_last_error()
    assert _lib.lib().rtg_dof_fk_backward_f32(model.handle, None, None, None, None, 0, 0, None, None, None, None) == 0


@pytest.mark.parametrize("J", [65, 97])
def test_dof_fk_lane_walk_forward_vs_oracle(gpu, J):
    """The joint-angle forward on trees beyond the lane groups (k_dof_fk_walk), which the backward tests above lean
    on for their saved rotations: bit for bit the oracle's, clip off and on."""
    import oracle as orc
    from rtg import ops
    from rtg.runtime import DofModel, Topology
    rng = np.random.default_rng(3 * J)
    par = np.array([-1] + [int(rng.integers(0, j)) for j in range(1, J)], np.int32)
    lt = rng.normal(0, 0.2, (J, 3)).astype(np.float32)
    axis = rng.integers(0, 3, J - 1).astype(np.int32)
    lo = (-0.5 - rng.uniform(0, 1, J - 1)).astype(np.float32)
    hi = (0.5 + rng.uniform(0, 1, J - 1)).astype(np.float32)
    model = DofModel(Topology(par, lt), axis, lo, hi)
    B = 1001
    dof = rng.uniform(-4, 4, (B, J - 1)).astype(np.float32)
    rr = rng.normal(size=(B, 4)).astype(np.float32)
    rt = rng.normal(0, 0.3, (B, 3)).astype(np.float32)
    for clip in (False, True):
        gr, gp = ops.dof_forward_kinematics(model, dof, rr, rt, clip=clip)
        ogr, ogp = orc.dof_fk(par, lt, axis, dof, rr, rt, lo if clip else None, hi if clip else None)
        np.testing.assert_array_equal(_np(gr), ogr)
        np.testing.assert_array_equal(_np(gp), ogp)


def _offset4(x):
    """A device copy of x that starts 4 bytes into its buffer: its rows are not 16-byte aligned."""
    buf = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    view = buf[1:].view(x.shape)
    view.copy_(torch.as_tensor(x))
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("kind,J,Bs", [("hu", 33, (17,)), ("bushy", 37, (9,)), ("chain", 1, (1, 17))])
def test_position_cotangent_at_any_alignment(gpu, hu_clip, kind, J, Bs):
    """grad_g_pos 4 bytes into its buffer: the position rows then come in dword by dword instead of as dwordx4 pieces,
    and every output of both adjoints, with and without the rotation cotangent, keeps the bits of the aligned call.
    The 33-link Hu model (16 frames per wave) and the 37-joint binary tree (8) at one whole tile plus a one-frame tile;
    the one-joint chain, whose lone frame is a 12-byte row with no whole 16-byte piece to load."""
    from rtg import _lib, ops
    from rtg.runtime import DofModel, Topology, ptr
    rng = np.random.default_rng(4000 + J)
    if kind == "hu":
        par, lt, axis, lo, hi = hu_clip[1]
    else:
        par, lt = _tree(kind, J), rng.normal(0, 0.3, (J, 3)).astype(np.float32)
        axis = rng.integers(0, 3, J - 1).astype(np.int32)
        lo, hi = (-0.5 - rng.uniform(0, 1, J - 1)).astype(np.float32), (0.5 + rng.uniform(0, 1, J - 1)).astype(np.float32)
    topo = Topology(par, lt)
    model = DofModel(topo, axis, lo, hi)
    lib = _lib.lib()
    for B in Bs:
        dev = lambda a: torch.as_tensor(a).cuda()
        dof = dev(rng.uniform(-3, 3, (B, J - 1)).astype(np.float32))
        rr, rt = dev(_scaled_quats(rng, B)), dev(rng.normal(0, 0.3, (B, 3)).astype(np.float32))
        lr = dev(np.ascontiguousarray(_scaled_quats(rng, B * J).reshape(B, J, 4)))
        cr = dev(rng.normal(size=(B, J, 4)).astype(np.float32))
        cp = rng.normal(size=(B, J, 3)).astype(np.float32)
        g_dof = ops.dof_forward_kinematics(model, dof, rr, rt, clip=True)[0].contiguous()
        g_fk = ops.forward_kinematics(topo, lr, rt)[0].contiguous()

        def run(form, cot_rot, cot_pos):
            outs = [torch.full(s, 7.0, device="cuda") for s in
                    (((B, J - 1), (B, 4), (B, 3)) if form == "dof" else ((B, J, 4), (B, 3)))]
            if form == "dof":
                rc = lib.rtg_dof_fk_backward_f32(model.handle, ptr(dof) if J > 1 else None, ptr(g_dof), ptr(cot_rot),
                                                 ptr(cot_pos), B, 1, ptr(outs[0]) if J > 1 else None, ptr(outs[1]),
                                                 ptr(outs[2]), None)
            else:
                rc = lib.rtg_fk_backward_f32(topo.handle, ptr(lr), ptr(g_fk), ptr(cot_rot), ptr(cot_pos), B,
                                             ptr(outs[0]), ptr(outs[1]), None)
            assert rc == 0, lib.rtg_last_error()
            torch.cuda.synchronize()
            return [_np(o).view(np.uint32) for o in outs]

        for form in ("dof", "fk"):
            for cot_rot in (cr, None):
                for a, b in zip(run(form, cot_rot, dev(cp)), run(form, cot_rot, _offset4(cp))):
                    np.testing.assert_array_equal(a, b, err_msg=f"{kind} J={J} B={B} {form} rot={cot_rot is not None}")

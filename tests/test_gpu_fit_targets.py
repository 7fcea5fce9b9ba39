"""Keypoint targets for the pose fit on the MI355X (rtg_fit_targets_f32): the launch equals the float32 restatement
(tests/fit_targets_ref.py, tied to the reference's recorded rescale by tests/test_fit_targets_host.py) bit for bit,
NaN-aware -- on the golden mappings and on synthetic trees up to the 64-joint limit, at ragged batch sizes on both tile
shapes, with and without each constant; it equals the existing one-tree launch and the composition of existing
launches; hostile frames stay in their rows; and HuForwardModel.fit_mocap / VtrdynFullBodyFitRetargeter carry its
output into the pose fit."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import fit_targets_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN_CASES = ("vtrdyn_full_hu", "vtrdyn_hu_v5_global", "noitom_hu_v5")
SYNTHETIC = ("chain64", "chain64_half", "star60", "j2", "k1")
DIR, SCALE, OFFSET = [-1.0, -1.0, 1.0], [0.7407407, 0.7407407, 0.9], [0.125, -3.0, 1e-3]


def _asset(name):
    from rtg import assets
    return assets.parents(name).astype(np.int32), assets.local_translation(name)


def case_trees(case):
    """(src parents, src local_t, tgt parents, tgt local_t, src_joint, tgt_joint)"""
    if case in SYNTHETIC:
        return ref.synthetic(case)
    s, t, sj, tj, _ = ref.golden_mapping(case)
    return _asset(s) + _asset(t) + (sj, tj)


def tile_frames(Js, Jt):
    return 16 if max(Js, Jt) <= 36 else 8   # group_frames (csrc/rtg_kernels.cuh)


def frames(B, J, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.4, (B, J, 3)) + rng.normal(0, 1.0, (B, 1, 3))).astype(np.float32)


def plan_of(trees, **consts):
    from rtg.bridge import fit_targets_plan
    sp, slt, tp, tlt, sj, tj = trees
    return fit_targets_plan((sp, slt), (tp, tlt), sj, tj, **consts)


def launch(plan, x):
    from rtg import ops
    out = ops.fit_targets(plan, torch.from_numpy(np.ascontiguousarray(x)).cuda())
    return out.cpu().numpy()


def restate(trees, x, **consts):
    _, _, tp, tlt, sj, tj = trees
    return ref.fit_targets(tp, tlt, sj, tj, x, **consts)


# ------------------------------------------------------------------ bit for bit against the restatement
@pytest.mark.parametrize("case", GOLDEN_CASES + SYNTHETIC)
def test_launch_is_the_restatement(gpu, case):
    trees = case_trees(case)
    Js, Jt = len(trees[0]), len(trees[2])
    F = tile_frames(Js, Jt)
    x = frames(4 * F + 3, Js, seed=len(case))
    for on in itertools.product((False, True), repeat=3):
        consts = {k: v for k, v, o in zip(("dir", "root_scale", "root_offset"), (DIR, SCALE, OFFSET), on) if o}
        want = restate(trees, x, **consts)   # frames are independent: a shorter batch is a prefix
        plan = plan_of(trees, **consts)
        assert plan.weight.dtype == np.float32 and plan.weight.shape == (Jt,) and plan.weight.sum() == len(trees[4])
        for B in (1, F - 1, F, F + 1, 4 * F + 3):
            got = launch(plan, x[:B])
            assert got.shape == (B, Jt, 3)
            assert ref.same_bits(got, want[:B]), (case, consts, B)
    root = launch(plan_of(trees), x)[:, 0]   # no constant: the root row keeps the source row's bits
    assert np.array_equal(root.view(np.uint32), x[:, trees[4][list(trees[5]).index(0)]].view(np.uint32))


def test_tile_shapes_are_both_covered():
    shapes = {tile_frames(len(case_trees(c)[0]), len(case_trees(c)[2])) for c in GOLDEN_CASES + SYNTHETIC}
    assert shapes == {8, 16}


def test_any_leading_shape_and_the_inputs_device(gpu):
    from rtg import ops
    trees = case_trees("vtrdyn_hu_v5_global")
    plan = plan_of(trees, dir=DIR)
    x = frames(12, 21, seed=3)
    want = restate(trees, x, dir=DIR)
    out = ops.fit_targets(plan, torch.from_numpy(x.reshape(3, 2, 2, 21, 3)))   # a CPU tensor comes back on the CPU
    assert out.device.type == "cpu" and tuple(out.shape) == (3, 2, 2, 31, 3)
    assert ref.same_bits(out.numpy().reshape(12, 31, 3), want)
    out = ops.fit_targets(plan, torch.from_numpy(x).cuda()[:0])
    assert out.is_cuda and tuple(out.shape) == (0, 31, 3)
    assert plan_of(trees, dir=DIR) is plan and plan_of(trees) is not plan   # cached per (trees, mapping, constants)
    with pytest.raises(ValueError):
        ops.fit_targets(plan, torch.from_numpy(x[:, :20]))


# ------------------------------------------------------------------ against the existing launches
@pytest.mark.parametrize("name", ["vtrdyn", "vtrdyn_full"])   # F = 16 and F = 8
def test_one_tree_and_the_identity_mapping_is_rescale_motion(gpu, name):
    """On these trees every G[j] - G[parent] has local_t[j]'s bits (asserted), so the plan's segments are the one-tree
    kernel's and the two launches agree bit for bit."""
    from rtg import ops
    from rtg.bridge import topology
    par, lt = _asset(name)
    J = len(par)
    G = ref.zero_pose_global(par, lt)
    assert all(np.array_equal((G[j] - G[par[j]]).view(np.uint32), lt[j].view(np.uint32)) for j in range(1, J))
    ident = np.arange(J, dtype=np.int32)
    trees = (par, lt, par, lt, ident, ident)
    x = torch.from_numpy(frames(4 * tile_frames(J, J) + 3, J, seed=J)).cuda()
    for d in (None, DIR):
        a = ops.fit_targets(plan_of(trees, **({} if d is None else {"dir": d})), x)
        b = ops.rescale_motion(topology(par, lt), x, dir=d)
        assert ref.same_bits(a.cpu().numpy(), b.cpu().numpy()), d


@pytest.mark.parametrize("case", ["vtrdyn_full_hu", "noitom_hu_v5"])
def test_cross_tree_launch_is_the_composition_of_existing_launches(gpu, case):
    """index_select of the mapped source rows, ops.rescale_motion on the reduced tree whose local translations are the
    plan's segments, scatter through src_of."""
    from rtg import ops
    from rtg.runtime import Topology
    trees = case_trees(case)
    sp, _, tp, tlt, sj, tj = trees
    tab = ref.tables(tp, tlt, sj, tj)
    order = np.argsort(tj)   # the reduced tree's joints: the pairs by ascending target index
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    red_par = np.array([-1 if tab["anchor"][k] < 0 else rank[tab["anchor"][k]] for k in order], np.int32)
    red = Topology(red_par, tab["seg"][order])
    x = torch.from_numpy(frames(4 * tile_frames(len(sp), len(tp)) + 3, len(sp), seed=11)).cuda()
    for d in (None, DIR):
        rows = x.index_select(1, torch.from_numpy(sj[order].astype(np.int64)).cuda())
        comp = ops.rescale_motion(red, rows, dir=d).index_select(1, torch.from_numpy(rank[tab["src_of"]]).cuda())
        got = ops.fit_targets(plan_of(trees, **({} if d is None else {"dir": d})), x)
        assert ref.same_bits(got.cpu().numpy(), comp.cpu().numpy()), d


# ------------------------------------------------------------------ hostile frames
def _descendants(tab, k):
    """Pair k and the pairs below it in the reduced target tree."""
    out = {k}
    grew = True
    while grew:
        grew = False
        for i, a in enumerate(tab["anchor"]):
            if int(a) in out and i not in out:
                out.add(i)
                grew = True
    return out


@pytest.mark.parametrize("case", ["vtrdyn_hu_v5_global", "vtrdyn_full_hu"])   # F = 16 and F = 8
def test_hostile_frames_stay_in_their_rows(gpu, case):
    trees = case_trees(case)
    sp, _, tp, tlt, sj, tj, = trees
    _, _, _, _, c = ref.golden_mapping(case)
    Js, Jt = len(sp), len(tp)
    F = tile_frames(Js, Jt)
    tab = ref.tables(tp, tlt, sj, tj)
    clean = frames(3 * F, Js, seed=5)
    plan = plan_of(trees, dir=DIR, root_scale=SCALE)
    base = launch(plan, clean)
    assert np.isfinite(base).all() and ref.same_bits(base, restate(trees, clean, dir=DIR, root_scale=SCALE))
    spots = (F - 1, F, F + F // 2)   # both sides of a tile boundary, the middle frame of the middle tile
    knee = list(tj).index(c["target_names"].index("left_knee_link"))
    below, mapped = _descendants(tab, knee), set(int(t) for t in tj)

    def zero_segment(x):   # the knee's source joint on its anchor's: 0 / 0
        x[:, sj[knee]] = x[:, sj[tab["anchor"][knee]]]

    def specials(x):
        x[:, sj[knee], 0], x[:, sj[0], 1], x[:, sj[1], 2], x[:, sj[2]] = np.nan, np.inf, -0.0, 1e-41

    def huge(x):
        x *= np.float32(1e18)

    def overflow(x):
        x *= np.float32(1e25)

    def tiny(x):
        x *= np.float32(1e-30)

    for hostile in (zero_segment, specials, huge, overflow, tiny):
        x = clean.copy()
        rows = x[list(spots)]
        hostile(rows)
        x[list(spots)] = rows
        got, want = launch(plan, x), restate(trees, x, dir=DIR, root_scale=SCALE)
        assert ref.same_bits(got, want), hostile.__name__
        rest = np.setdiff1d(np.arange(3 * F), spots)
        assert np.array_equal(got[rest].view(np.uint32), base[rest].view(np.uint32)), hostile.__name__   # the neighbours
        assert ref.same_bits(launch(plan, x[F:F + 1]), want[F:F + 1])
        for f in spots:
            nan = np.isnan(got[f]).any(-1)
            if hostile is zero_segment:   # NaN in the link and below it in the reduced tree, nowhere else
                for j in range(Jt):
                    assert nan[j] == (int(tab["src_of"][j]) in below), (f, j)
                assert nan.any() and not nan.all()
            if hostile is overflow:   # the norm overflows, scale = inf: every mapped link sits on its anchor, the root
                assert np.isinf(ref.lnorm3(x[f, sj[knee]] - x[f, sj[tab["anchor"][knee]]]))
                assert np.array_equal(got[f], np.broadcast_to(got[f, 0], (Jt, 3))) and np.isfinite(got[f]).all()
            if hostile is huge:
                assert np.isfinite(got[f]).all()
    assert mapped


def test_a_zero_length_target_segment_puts_the_child_on_its_anchor(gpu):
    sp, slt, tp, tlt, sj, tj = case_trees("vtrdyn_hu_v5_global")
    _, _, _, _, c = ref.golden_mapping("vtrdyn_hu_v5_global")
    knee, hip = (c["target_names"].index(n) for n in ("left_knee_link", "left_hip_pitch_link"))
    assert tp[knee] == hip
    tlt = tlt.copy()
    tlt[knee] = 0
    trees = (sp, slt, tp, tlt, sj, tj)
    assert not ref.tables(tp, tlt, sj, tj)["seg"][list(tj).index(knee)].any()
    x = frames(35, len(sp), seed=9)
    got = launch(plan_of(trees), x)
    assert ref.same_bits(got, restate(trees, x)) and np.isfinite(got).all()
    assert np.array_equal(got[:, knee], got[:, hip])


# ------------------------------------------------------------------ determinism, streams, the C ABI's checks
def test_runs_repeat_and_streams_and_argument_checks(gpu):
    from rtg import _lib
    from rtg.runtime import ptr, stream_handle
    lib = _lib.lib()
    trees = case_trees("vtrdyn_full_hu")
    plan = plan_of(trees, dir=DIR, root_scale=SCALE, root_offset=OFFSET)
    B = 4 * 8 + 3
    x = torch.from_numpy(frames(B, 59, seed=2)).cuda()
    a, b = launch(plan, x.cpu().numpy()), launch(plan, x.cpu().numpy())
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for f in (0, 7, 8, 20, B - 1):   # a frame of the batch equals that frame launched alone
        assert np.array_equal(launch(plan, x[f:f + 1].cpu().numpy()).view(np.uint32), a[f:f + 1].view(np.uint32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = torch.empty((B, 33, 3), device="cuda")
    with torch.cuda.stream(side):
        _lib.check(lib.rtg_fit_targets_f32(plan.handle, ptr(x), B, ptr(out), stream_handle(side)))
    side.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), a.view(np.uint32))
    # an output that does not start on 16 bytes, a source likewise: dword by dword, the same bits
    xo = torch.empty(B * 59 * 3 + 1, device="cuda")[1:].view(B, 59, 3).copy_(x)
    oo = torch.empty(B * 33 * 3 + 1, device="cuda")[1:].view(B, 33, 3)
    _lib.check(lib.rtg_fit_targets_f32(plan.handle, ptr(xo), B, ptr(oo), stream_handle()))
    assert np.array_equal(oo.cpu().numpy().view(np.uint32), a.view(np.uint32))
    # the checks that need a plan
    before = out.clone()
    call = lambda *args: lib.rtg_fit_targets_f32(plan.handle, *args, stream_handle())
    assert call(ptr(x), 0, ptr(out)) == 0 and call(None, 0, None) == 0   # B == 0 is a no-op
    for args, msg in (((None, B, ptr(out)), b"NULL buffer"), ((ptr(x), B, None), b"NULL buffer"),
                      ((ptr(x), -1, ptr(out)), b"B=-1 < 0"), ((ptr(x), B, ptr(x)), b"src_pos and target_pos overlap"),
                      ((ptr(x), B, ctypes.c_void_p(x.data_ptr() + 4 * (B * 59 * 3 - 1))), b"overlap")):
        assert call(*args) == 1 and msg in lib.rtg_last_error(), lib.rtg_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, before)


# ------------------------------------------------------------------ end to end: into the pose fit
def _tree(names, par, lt):
    from poselib.poselib.skeleton.skeleton3d import SkeletonTree
    return SkeletonTree(list(names), torch.as_tensor(np.asarray(par)), torch.from_numpy(np.asarray(lt, np.float32)))


@pytest.fixture(scope="module")
def outcome():
    """The outcome recipe's float32 inputs, the robot model and the human's tree."""
    from robot_kinematics_model import RobotZeroPose
    from robot_kinematics_model.hu_forward_model import HuForwardModel
    x = ref.outcome_recipe()
    s = x["s"]
    hu = HuForwardModel(RobotZeroPose.from_asset("hu").skeleton_tree)
    assert hu.node_names == x["names"] and np.array_equal(np.asarray(hu.dof_lower, np.float32), np.asarray(s.lo, np.float32))
    human = _tree(x["names"], s.par, x["human_lt"])
    mapping = {x["names"][j]: x["names"][j] for j in x["links"]}
    return x, hu, human, mapping


def test_fit_mocap_lands_closer_than_raw_keypoints(gpu, outcome):
    """fit_mocap on the recipe's float32 inputs against fit_pose on the raw keypoints, 128 steps at lr 0.02 each: the
    error ratio raw / rescaled reaches at least half the float64 loop's (6.70 there).  Measured on the MI355X: raw loss
    0.2155, error 0.0608 m; rescaled loss 0.00197, error 0.0091 m; error ratio 6.70."""
    x, hu, human, mapping = outcome
    t = torch.from_numpy
    start = t(x["start"])[..., None]
    kw = dict(iters=128, lr=0.02)
    raw = hu.fit_pose(t(x["human"]), t(x["human"][:, 0].copy()), t(x["q0"])[:, None], start, weight=t(x["w"]), **kw)
    r = np.float32(x["ratio"])
    res = hu.fit_mocap(human, mapping, t(x["human"]), motion_joint_angles=start, root_scale=[r, r, r], **kw)
    assert len(res) == 6 and tuple(res[5].shape) == (64, 33, 3)
    want = ref.fit_targets(x["s"].par, x["s"].lt, x["links"], x["links"], x["human"], root_scale=[r, r, r])
    assert ref.same_bits(res[5].numpy(), want)
    err = {k: ref.outcome_error(x, v[0][..., 0].numpy(), v[2][:, 0].numpy()) for k, v in (("raw", raw), ("rescaled", res))}
    loss = {k: float(v[3].mean()) for k, v in (("raw", raw), ("rescaled", res))}
    f64 = ref.outcome_float64()
    ratio64 = f64["raw"][1] / f64["rescaled"][1]
    print(f"GPU float32: raw loss {loss['raw']:.4f} error {err['raw']:.4f} m; rescaled loss {loss['rescaled']:.5f} error "
          f"{err['rescaled']:.4f} m; error ratio {err['raw'] / err['rescaled']:.2f} (float64 loop {ratio64:.2f})")
    assert err["raw"] / err["rescaled"] >= 0.5 * ratio64


def test_fit_mocap_is_keypoint_targets_then_fit_pose(gpu, outcome):
    x, hu, human, mapping = outcome
    t = torch.from_numpy
    src = t(x["human"][:19]).cuda()
    kw = dict(iters=6, lr=0.02, project_angles=True)
    res = hu.fit_mocap(human, mapping, src, dir=DIR, root_offset=OFFSET, smooth_weight=0, **kw)
    targets, w = hu.keypoint_targets(human, mapping, src, dir=DIR, root_offset=OFFSET)
    assert targets.is_cuda and np.array_equal(w.cpu().numpy(), x["w"])
    q0 = torch.zeros(19, 1, 4, device="cuda")
    q0[..., 3] = 1
    two = hu.fit_pose(targets, targets[:, 0].clone(), q0, weight=w, **kw)
    assert all(torch.equal(a, b) for a, b in zip(res[:4], two[:4])) and torch.equal(res[5], targets)
    assert all(torch.equal(a, b) for a, b in zip(res[4][:3], two[4][:3]))
    # a caller's weight multiplies the plan's; smoothing goes through fit_motion
    half = hu.fit_mocap(human, mapping, src, dir=DIR, root_offset=OFFSET, weight=np.full(33, 0.5, np.float32), **kw)
    two = hu.fit_pose(targets, targets[:, 0].clone(), q0, weight=0.5 * w, **kw)
    assert all(torch.equal(a, b) for a, b in zip(half[:4], two[:4]))
    smooth = hu.fit_mocap(human, mapping, src, dir=DIR, root_offset=OFFSET, smooth_weight=0.1, rounds=2, iters=3, lr=0.02)
    two = hu.fit_motion(targets, targets[:, 0].clone(), q0, smooth_weight=0.1, rounds=2, iters=3, lr=0.02, weight=w)
    assert all(torch.equal(a, b) for a, b in zip(smooth[:4], two[:4]))
    with pytest.raises(ValueError):
        hu.keypoint_targets(human, {"no_such_joint": "pelvis_link"}, src)


def test_retargeter_continues_from_its_previous_call(gpu, outcome):
    from retarget.retarget_solver import VtrdynFullBodyFitRetargeter
    x, hu, human, mapping = outcome

    class Zero:
        def __init__(self, tree):
            self.skeleton_tree = tree
    from robot_kinematics_model import RobotZeroPose
    target = RobotZeroPose.from_asset("hu")
    r = np.float32(x["ratio"])
    kw = dict(iters=8, lr=0.02, root_scale=[r, r, r], project_angles=True)
    rt = VtrdynFullBodyFitRetargeter(Zero(human), target, mapping, prior_weight=0.1, **kw)
    body = torch.from_numpy(x["human"][:21])
    dof1, t1, q1, loss1 = rt.retarget_batch(body)
    assert tuple(dof1.shape) == (21, 32) and tuple(t1.shape) == (21, 3) and tuple(q1.shape) == (21, 4) and tuple(loss1.shape) == (21,)
    first = hu.fit_mocap(human, mapping, body, **kw)
    assert torch.equal(dof1, first[0][..., 0]) and torch.equal(q1, first[2][:, 0]) and torch.equal(loss1, first[3])
    dof2, t2, q2, loss2 = rt.retarget_batch(body)   # the same frames again: from call 1's angles, root and optimiser
    second = hu.fit_mocap(human, mapping, body, motion_root_rotation=first[2], motion_joint_angles=first[0],
                          prior_angles=first[0], prior_weight=0.1, state=first[4], **kw)
    assert torch.equal(dof2, second[0][..., 0]) and torch.equal(t2, second[1]) and torch.equal(q2, second[2][:, 0])
    assert torch.equal(loss2, second[3]) and not torch.equal(dof2, dof1)
    assert second[4][3] == 16   # the optimiser's step count went on
    rt.reset()
    again = rt.retarget_batch(body)
    assert torch.equal(again[0], dof1) and torch.equal(again[3], loss1)
    rt.retarget_batch(body[:5])   # another batch size starts afresh
    assert tuple(rt.retarget_batch(body[:5])[0].shape) == (5, 32)

"""``retarget_to`` on the MI355X: the fused kernel's output equals the composition of oracle primitives
(tests/retarget_to_ref.py, tied to the reference's recorded outputs by tests/test_retarget_to_host.py) bit for bit,
NaN-aware -- through the drop-in classes, through the ops layer at ragged batch sizes on both tile shapes, and on random
trees and mappings up to the 64-joint limit."""
import ctypes

import numpy as np
import pytest
import torch

import retarget_to_ref as ref
from retarget_to_ref import FIXTURE_CASES, bits, fixture, fixture_plan

pytestmark = pytest.mark.gpu


def poselib_tree(names, parents, local_t, quat=None):
    from poselib.poselib.skeleton.skeleton3d import SkeletonTree
    return SkeletonTree(list(names), torch.as_tensor(np.asarray(parents)), torch.from_numpy(np.asarray(local_t, np.float32)),
                        None if quat is None else torch.from_numpy(np.asarray(quat, np.float32)))


def asset_tree(name):
    a = ref.asset(name)
    return poselib_tree([str(s) for s in a["node_names"]], a["parent_indices"], a["local_translation"], a["quat"])


def state_of(tree, rot, root_t, is_local, device="cpu"):
    from poselib.poselib.skeleton.skeleton3d import SkeletonState
    v = np.concatenate([np.asarray(rot, np.float32).reshape(len(rot), -1), np.asarray(root_t, np.float32)], axis=-1)
    return SkeletonState(torch.from_numpy(v).to(device), tree, is_local)


def fixture_call(tag, device="cpu"):
    """The fixture case for the drop-in classes -> (source state, retarget_to's arguments)."""
    d, names = fixture()
    e = names[tag]
    src, tgt = asset_tree(e["source"]), asset_tree(e["target"])
    st = state_of(src, d[f"{tag}_rot"], d[f"{tag}_root_t"], bool(d[f"{tag}_is_local"]), device)
    args = (e["mapping"], torch.from_numpy(d[f"{tag}_src_tpose_rot"]), d[f"{tag}_src_tpose_root_t"], tgt,
            d[f"{tag}_tgt_tpose_rot"], torch.from_numpy(d[f"{tag}_tgt_tpose_root_t"]).to(device), d[f"{tag}_R"],
            float(d[f"{tag}_scale"].reshape(-1)[0]))
    return st, args


@pytest.mark.parametrize("tag", FIXTURE_CASES)
def test_fixture_cases_through_the_drop_in(gpu, tag):
    d, _ = fixture()
    st, args = fixture_call(tag, "cuda" if tag == "noitom_hu_v5" else "cpu")   # a device state stays on the device
    res = st.retarget_to(*args)
    assert res.is_local and res.skeleton_tree is args[3] and res.tensor.device == st.tensor.device
    assert type(res).__name__ == "SkeletonState" and tuple(res.tensor.shape) == (64, args[3].num_joints * 4 + 3)
    plan, _ = fixture_plan(tag)
    want_rot, want_root = plan(d[f"{tag}_rot"], d[f"{tag}_root_t"], bool(d[f"{tag}_is_local"]))
    rot, root = res.rotation.cpu().numpy(), res.root_translation.cpu().numpy()
    np.testing.assert_array_equal(bits(rot), bits(want_rot))
    np.testing.assert_array_equal(bits(root), bits(want_root))
    np.testing.assert_array_equal(bits(rot), bits(d[f"{tag}_out_rot"]))      # and the reference's own output
    np.testing.assert_array_equal(bits(root), bits(d[f"{tag}_out_root_t"]))
    # by t-pose states: the same call
    from poselib.poselib.skeleton.skeleton3d import SkeletonState
    tp_s = SkeletonState.from_rotation_and_root_translation(st.skeleton_tree, args[1], args[2], is_local=True)
    tp_t = SkeletonState.from_rotation_and_root_translation(args[3], args[4], args[5].cpu(), is_local=True)
    res2 = st.retarget_to_by_tpose(args[0], tp_s, tp_t, args[6], args[7])
    np.testing.assert_array_equal(bits(res2.tensor.cpu().numpy()), bits(res.tensor.cpu().numpy()))


def gpu_plan(plan: ref.Plan, src_lt, tgt_lt, src_tp, src_tp_t, tgt_tp, tgt_tp_t):
    from rtg.bridge import retarget_plan
    sj = [plan.kept_s[plan.perm[k]] for k in range(plan.K)]
    return retarget_plan((plan.sp, src_lt, plan.stq), (plan.tp, tgt_lt, plan.ttq), sj, plan.kept_t, src_tp, src_tp_t,
                         tgt_tp, tgt_tp_t, plan.R, float(plan.scale))


def fixture_gpu_plan(tag):
    d, names = fixture()
    plan, e = fixture_plan(tag)
    s, t = ref.asset(e["source"]), ref.asset(e["target"])
    return plan, gpu_plan(plan, s["local_translation"], t["local_translation"], d[f"{tag}_src_tpose_rot"],
                          d[f"{tag}_src_tpose_root_t"], d[f"{tag}_tgt_tpose_rot"], d[f"{tag}_tgt_tpose_root_t"])


def random_frames(rng, B, J):
    """Rows of norm 0.5-2 (the kernel's first normalisation is off the near-unit table), some with w < 0."""
    q = rng.normal(size=(B, J, 4))
    q = q / np.linalg.norm(q, axis=-1, keepdims=True) * rng.uniform(0.5, 2.0, (B, J, 1))
    return q.astype(np.float32), rng.normal(0, 0.5, (B, 3)).astype(np.float32)


# 16 frames per wave (J <= 36) and 8 (J <= 64); ragged, single-tile and many-tile launches of each
@pytest.mark.parametrize("tag,F", [("vtrdyn_hu_v5_local", 16), ("vtrdyn_full_hu", 8)])
def test_batch_sizes_through_the_ops_layer(gpu, tag, F):
    from rtg import ops
    plan, gp = fixture_gpu_plan(tag)
    rng = np.random.default_rng(77)
    q, t = random_frames(rng, 4097, len(plan.sp))
    for local in (True, False):
        want_rot, want_root = plan(q, t, local)
        qd, td = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
        for B in (1, F - 1, F, F + 1, 3 * F + 5, 4097):
            rot, root = ops.retarget_to(gp, qd[:B], td[:B], local)
            assert rot.shape == (B, len(plan.tp), 4) and root.shape == (B, 3)
            np.testing.assert_array_equal(bits(rot.cpu().numpy()), bits(want_rot[:B]), err_msg=f"B={B} local={local}")
            np.testing.assert_array_equal(bits(root.cpu().numpy()), bits(want_root[:B]), err_msg=f"B={B} local={local}")
    rot, root = ops.retarget_to(gp, qd[:0], td[:0], True)   # B = 0: a no-op
    assert rot.shape == (0, len(plan.tp), 4) and root.shape == (0, 3)


def random_tree(rng, J, shape):
    if shape == "chain":
        par = [-1] + list(range(J - 1))
    elif shape == "binary":
        par = [-1] + [(j - 1) // 2 for j in range(1, J)]
    else:
        par = [-1] + [0] * (J - 1)
    tq = rng.normal(size=(J, 4))
    tq = (tq / np.linalg.norm(tq, axis=-1, keepdims=True)).astype(np.float32)   # non-identity tree quaternions
    return np.asarray(par, np.int32), tq, rng.normal(0, 0.3, (J, 3)).astype(np.float32)


SIZES = (1, 2, 7, 36, 37, 64)   # 36 | 37: sixteen or eight frames per wave; 64: the limit
SHAPES = ("chain", "binary", "star")


@pytest.mark.parametrize("Js", SIZES)
@pytest.mark.parametrize("Jt", SIZES)
def test_random_trees_and_mappings(gpu, Js, Jt):
    from rtg import ops
    rng = np.random.default_rng(1000 * Js + Jt)
    m = min(Js, Jt)
    ks = [m, int(rng.integers(1, m + 1)), 1]
    for i, shape in enumerate(SHAPES):
        K = ks[(i + Js + Jt) % 3]
        sp, stq, slt = random_tree(rng, Js, shape)
        tp, ttq, tlt = random_tree(rng, Jt, SHAPES[(i + Jt) % 3])
        sj = [0] + sorted(rng.choice(np.arange(1, Js), K - 1, replace=False).tolist()) if K > 1 else [0]
        tj = [0] + sorted(rng.choice(np.arange(1, Jt), K - 1, replace=False).tolist()) if K > 1 else [0]
        tj = [tj[k] for k in rng.permutation(K)]   # the roots are mapped, not always to each other
        tps, tps_t = random_frames(rng, 1, Js)
        tpt, tpt_t = random_frames(rng, 1, Jt)
        R = rng.normal(size=4)
        R = (R / np.linalg.norm(R)).astype(np.float32)
        plan = ref.Plan((sp, stq), (tp, ttq), sj, tj, tps[0], tps_t[0], tpt[0], tpt_t[0], R, rng.uniform(0.2, 3.0))
        from rtg.bridge import retarget_plan
        gp = retarget_plan((sp, slt, stq), (tp, tlt, ttq), sj, tj, tps[0], tps_t[0], tpt[0], tpt_t[0], R,
                           float(plan.scale))
        B = 37   # more than one tile at either frame count, the last one ragged
        q, t = random_frames(rng, B, Js)
        q[3, Js // 2] = 0.0
        q[5, 0, 3] = -abs(q[5, 0, 3])
        for local in (True, False):
            want_rot, want_root = plan(q, t, local)
            rot, root = ops.retarget_to(gp, q, t, local)
            msg = f"{shape} Js={Js} Jt={Jt} K={K} local={local}"
            np.testing.assert_array_equal(bits(rot.cpu().numpy()), bits(want_rot), err_msg=msg)
            np.testing.assert_array_equal(bits(root.cpu().numpy()), bits(want_root), err_msg=msg)


@pytest.mark.parametrize("tag,F", [("vtrdyn_hu_v5_local", 16), ("vtrdyn_full_hu", 8)])
def test_frames_are_isolated_and_runs_repeat(gpu, tag, F):
    from rtg import ops
    plan, gp = fixture_gpu_plan(tag)
    rng = np.random.default_rng(5)
    B = 3 * F
    q, t = random_frames(rng, B, len(plan.sp))
    for local in (True, False):
        rot0, root0 = ops.retarget_to(gp, q, t, local)
        rot1, root1 = ops.retarget_to(gp, q, t, local)
        assert torch.equal(rot0.view(torch.int32), rot1.view(torch.int32))          # the same bits run to run
        assert torch.equal(root0.view(torch.int32), root1.view(torch.int32))
        bad = F + 1                                                                  # a frame inside the middle tile
        qp, tpo = q.copy(), t.copy()
        qp[bad], tpo[bad] = np.nan, np.nan
        rot2, root2 = ops.retarget_to(gp, qp, tpo, local)
        others = [f for f in range(B) if f != bad]                                   # its tile's and both neighbours'
        assert torch.equal(rot2[others].view(torch.int32), rot0[others].view(torch.int32))
        assert torch.equal(root2[others].view(torch.int32), root0[others].view(torch.int32))
        assert torch.isnan(rot2[bad]).all() and torch.isnan(root2[bad]).all()


def test_unaligned_root_translation_buffers(gpu):
    """tgt_root_t (and src_root_t) four bytes off a 16-byte boundary, straight through the C ABI."""
    from rtg import _lib
    from rtg.runtime import ptr, stream_handle
    plan, gp = fixture_gpu_plan("vtrdyn_hu_v5_local")
    rng = np.random.default_rng(6)
    B = 53
    q, t = random_frames(rng, B, len(plan.sp))
    want_rot, want_root = plan(q, t, True)
    qd = torch.from_numpy(q).cuda()
    tin = torch.zeros(3 * B + 1, device="cuda")
    tin[1:] = torch.from_numpy(t).cuda().reshape(-1)
    out_rot = torch.empty((B, len(plan.tp), 4), device="cuda")
    guard = torch.full((3 * B + 2,), 7.0, device="cuda")
    assert guard.data_ptr() % 16 == 0
    _lib.check(_lib.lib().rtg_retarget_to_f32(gp.handle, ptr(qd), ctypes.c_void_p(tin.data_ptr() + 4), 1, B,
                                              ptr(out_rot), ctypes.c_void_p(guard.data_ptr() + 4), stream_handle()))
    torch.cuda.synchronize()
    g = guard.cpu().numpy()
    assert g[0] == 7.0 and g[-1] == 7.0                       # nothing outside the 3 B floats was written
    np.testing.assert_array_equal(bits(g[1:-1].reshape(B, 3)), bits(want_root))
    np.testing.assert_array_equal(bits(out_rot.cpu().numpy()), bits(want_rot))


def test_large_trees_are_rejected_at_plan_creation(gpu):
    from rtg import _lib
    from rtg.bridge import retarget_plan
    J = 65
    par = np.asarray([-1] + list(range(J - 1)), np.int32)
    big = (par, np.zeros((J, 3), np.float32), None)
    small = (np.asarray([-1, 0], np.int32), np.zeros((2, 3), np.float32), None)
    idq = lambda n: np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1))
    for src, tgt in ((big, small), (small, big)):
        with pytest.raises(_lib.RtgError, match="1\\.\\.64 joints") as ei:
            retarget_plan(src, tgt, [0], [0], idq(len(src[0])), np.zeros(3), idq(len(tgt[0])), np.zeros(3), idq(1)[0], 1.0)
        assert ei.value.status == 4   # RTG_ERR_UNSUPPORTED


def test_motion_retarget_is_the_state_retarget_with_velocities(gpu):
    from poselib.poselib.skeleton.skeleton3d import SkeletonMotion
    st, args = fixture_call("vtrdyn_hu_v5_local")
    keep = slice(6, 64)                                       # the ordinary frames: velocities run over time
    st = state_of(st.skeleton_tree, st.rotation[keep].numpy(), st.root_translation[keep].numpy(), True)
    fps = 50
    motion = SkeletonMotion.from_skeleton_state(st, fps)
    res = motion.retarget_to(*args)
    want = SkeletonMotion.from_skeleton_state(st.retarget_to(*args), fps)
    assert isinstance(res, SkeletonMotion) and res.fps == fps and res.is_local
    assert res.tensor.shape == want.tensor.shape == (58, args[3].num_joints * 10 + 3)
    np.testing.assert_array_equal(bits(res.tensor.numpy()), bits(want.tensor.numpy()))
    from poselib.poselib.skeleton.skeleton3d import SkeletonState
    tp_s = SkeletonState.from_rotation_and_root_translation(st.skeleton_tree, args[1], args[2], is_local=True)
    tp_t = SkeletonState.from_rotation_and_root_translation(args[3], args[4], args[5], is_local=True)
    res2 = motion.retarget_to_by_tpose(args[0], tp_s, tp_t, args[6], args[7])
    np.testing.assert_array_equal(bits(res2.tensor.numpy()), bits(want.tensor.numpy()))


def rel_err(x, x64):
    """E(x) = max|x - x64| / max|x64|."""
    x64 = np.asarray(x64, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / np.abs(x64).max())


def test_state_drop_nodes_by_names(gpu):
    """Names, parents and rotations as the reference's; the averaged translations within 4x the reference's own
    float32 error against its float64 run (E(reference f32) = 1.3e-7 on these 64 frames)."""
    d, names = fixture()
    e = names[names["drop"]["case"]]
    tree = asset_tree(e["source"])
    before = tree.local_translation.clone()
    from poselib.poselib.skeleton.skeleton3d import SkeletonState
    st = SkeletonState.from_rotation_and_root_translation(tree, torch.from_numpy(d["drop_rot_in"]),   # as the fixture's
                                                          torch.from_numpy(d["drop_root_t_in"]), is_local=True)
    red = st.drop_nodes_by_names(names["drop"]["dropped"])
    assert torch.equal(tree.local_translation, before)
    assert list(red.skeleton_tree.node_names) == names["drop"]["names"]
    assert [int(p) for p in red.skeleton_tree.parent_indices] == [int(p) for p in d["drop_parents"]]
    assert red.is_local == bool(d["drop_is_local"])
    np.testing.assert_array_equal(bits(red.rotation.numpy()), bits(d["drop_rot"]))
    ours = rel_err(red.skeleton_tree.local_translation.numpy(), d["drop_local_t_f64"])
    theirs = rel_err(d["drop_local_t_f32"], d["drop_local_t_f64"])
    print(f"drop_nodes_by_names translations: E(ours) = {ours:.3g}, E(reference f32) = {theirs:.3g}, "
          f"ratio {ours / theirs:.3g}")
    assert ours <= 4 * theirs
    kept = st.keep_nodes_by_names(names["drop"]["names"])
    assert list(kept.skeleton_tree.node_names) == names["drop"]["names"]
    np.testing.assert_array_equal(bits(kept.tensor.numpy()), bits(red.tensor.numpy()))
    assert torch.equal(kept.skeleton_tree.local_translation, red.skeleton_tree.local_translation)
    plain = st.drop_nodes_by_names(names["drop"]["dropped"], estimate_local_translation_from_states=False)
    assert torch.equal(plain.skeleton_tree.local_translation,
                       tree.drop_nodes_by_names(names["drop"]["dropped"]).local_translation)

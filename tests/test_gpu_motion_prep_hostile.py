"""The motion-level prep of retarget/main.py (rtg_rescale_motion_f32, rtg_quat_between_f32, rtg_rebuild_vtrdyn_f32) and the
teleop ingest (rtg_ingest_vtrdyn_f32) on hostile input, bit for bit against the C oracle (the ingest: against numpy's
gather and np.allclose): the batches of tests/motion_prep_frames.py at 1, 63, 64, 65, 255, 256, 257 and 513 frames (one
wave, one 256-thread block, ragged on both sides).  tests/test_motion_prep_hostile_host.py anchors the oracle on these
batches to the reference's own outputs.

quat_between_two_vecs decides one branch for the whole batch (the largest norm of either side <= 1e-6f: the identity
everywhere).  The kernels find the maximum with a wave reduction and an atomic maximum on the float bits, a NaN pinned
to the largest pattern, in a workspace the launch clears; a second launch reads it.  So the deciding row is put on the
first and last lane of a wave, in another wave, another block and the ragged tail, at the threshold and one ulp above,
and the workspace comes in dirty.

Every comparison is on the raw bits, every NaN reading alike (retarget_to_ref.bits)."""
import numpy as np
import pytest

from conftest import golden

import motion_prep_frames as mp
from retarget_to_ref import bits

pytestmark = pytest.mark.gpu

IDENT = np.float32([0, 0, 0, 1])
DIR = [-1.0, -1.0, 1.0]
_CACHE = {}


def _np(t):
    return t.detach().cpu().numpy()


def tree():
    """(Topology, parents, local_t) of the 21-joint VTRDYN zero pose, built once."""
    if "t" not in _CACHE:
        from rtg import assets
        from rtg.runtime import Topology
        par, zl = assets.parents("vtrdyn"), golden("zero_pose")["vtrdyn_local_t"]
        _CACHE["t"] = (Topology(par, zl), par, zl)
    return _CACHE["t"]


def _same(got, want, tag):
    bad = (bits(got) != bits(want)).reshape(len(want), -1).any(axis=1)
    assert not bad.any(), f"{tag}: {int(bad.sum())} of {len(bad)} rows differ from the oracle, first {np.flatnonzero(bad)[:8].tolist()}"


def _ident(q):
    return bool((bits(q) == bits(IDENT)).all())


def _oracle_rebuild(m):
    import oracle as orc
    _, par, zl = tree()
    with np.errstate(all="ignore"):
        return orc.rebuild_vtrdyn(par, zl, m)


def _gpu_rebuild(m):
    from rtg import ops
    g, r = ops.rebuild_vtrdyn(tree()[0], m)
    return _np(g), _np(r)


@pytest.mark.parametrize("B", mp.B_GPU)
def test_pair_batches_vs_oracle(gpu, B):
    """Every batch of pair_batches(B) through quat_between_two_vecs: the oracle's bits, and the branch the name says."""
    import oracle as orc
    from rtg import ops
    for name, (v1, v2) in mp.pair_batches(B).items():
        with np.errstate(all="ignore"):
            want = orc.quat_between(v1, v2)
        got = _np(ops.quat_between_two_vecs(v1, v2))
        _same(got, want, f"quat_between {name} B={B}")
        assert _ident(got) == mp.pair_identity(name, B), (name, B)


@pytest.mark.parametrize("B", mp.B_GPU)
def test_motion_families_vs_oracle(gpu, B):
    """Every family of motions(family, B): rescale_motion with dir = [-1, -1, 1] and without, rebuild_vtrdyn of the
    rescaled motion, and rebuild_vtrdyn of the raw motion (the rescale removes every short bone, so only the raw motion
    takes the rebuild's batch-level identity branch)."""
    import oracle as orc
    from rtg import ops
    T, par, zl = tree()
    for fam in mp.MOTION_FAMILIES:
        m = mp.motions(fam, B)
        with np.errstate(all="ignore"):
            r, rn = orc.rescale_motion(par, zl, m, dir=DIR), orc.rescale_motion(par, zl, m)
        _same(_np(ops.rescale_motion(T, m, dir=DIR)), r, f"rescale {fam} B={B}")
        _same(_np(ops.rescale_motion(T, m)), rn, f"rescale without dir {fam} B={B}")
        for tag, x in (("rescaled", r), ("raw", m)):
            (gr, rt), (ogr, ort) = _gpu_rebuild(x), _oracle_rebuild(x)
            _same(gr, ogr, f"rebuild of the {tag} motion, {fam} B={B}")
            _same(rt, ort, f"rebuild root of the {tag} motion, {fam} B={B}")


@pytest.mark.parametrize("name", ["vtrdyn", "vtrdyn_full", "one", "chain5"])
def test_rescale_on_other_trees_vs_oracle(gpu, name):
    """The rescale on the 21- and 59-joint zero poses, a one-joint tree and the 5-chain whose local_t rows are zero,
    1e-30, 1e25 and NaN long."""
    import oracle as orc
    from rtg import assets, ops
    from rtg.runtime import Topology
    zp = golden("zero_pose")
    for B in mp.B_GPU:
        par, lt, m = mp.topologies({n: assets.parents(n) for n in ("vtrdyn", "vtrdyn_full")},
                                   {n: zp[f"{n}_local_t"] for n in ("vtrdyn", "vtrdyn_full")}, B=B)[name]
        T = Topology(par, lt)
        for d in (None, DIR):
            with np.errstate(all="ignore"):
                want = orc.rescale_motion(par, lt, m, dir=d)
            _same(_np(ops.rescale_motion(T, m, dir=d)), want, f"rescale {name} B={B} dir={d}")


@pytest.mark.parametrize("length", [mp.EPS, mp.EPS_ABOVE, np.float32(np.nan)], ids=["eps", "eps_above", "nan"])
def test_the_deciding_row_anywhere_in_the_batch(gpu, length):
    """B = 513, every row but one 1e-7 long: the one row (1e-6f: the identity everywhere; 1e-6f + ulp and NaN: nowhere) on
    lane 0 and lane 63 of the first wave, in the second wave, on the last lane of the first block, in the second block and
    in the one-frame third block; quat_between with the small side v1 and v2, rebuild_vtrdyn with the bone 14 -> 15 and the
    bone 9 -> 10 (whose child joint is a Kabsch centre)."""
    import oracle as orc
    from rtg import ops
    B = 513
    ident = bool(length == mp.EPS)
    for row in mp.DECIDING_ROWS:
        for side in (1, 2):
            v1, v2 = mp.decision_pair(B, side, length, row, 1e-7)
            with np.errstate(all="ignore"):
                want = orc.quat_between(v1, v2)
            got = _np(ops.quat_between_two_vecs(v1, v2))
            _same(got, want, f"quat_between side {side} row {row}")
            assert _ident(got) == ident and (bits(got) == bits(IDENT)).all(axis=1).any() == ident, (side, row)
        for joint, parent in ((mp.TINY_BONE, 14), (10, 9)):
            m = mp.rebuild_decision(B, joint, length, row, 1e-7)
            (gr, _), (ogr, _) = _gpu_rebuild(m), _oracle_rebuild(m)
            _same(gr, ogr, f"rebuild bone {joint} row {row}")
            assert _ident(gr[:, parent]) == ident, (joint, row)


def test_a_degenerate_bone_turns_its_parents_row_alone(gpu):
    """B = 257, bone j 1e-7 long in every frame but frame 130: with 1e-6f there the batch is degenerate for j, with
    1e-6f + ulp it is not.  Between the two runs only row parent(j) changes (the identity in the first), in every frame
    but 130 (where joint j itself moved by an ulp): every other row, rows 0 and 10 included, keeps its bits.  For the
    children of joints 0 and 10, which the rebuild skips, no row changes at all."""
    _, par, _ = tree()
    B, row = 257, 130
    others = np.arange(B) != row
    for j in range(1, 21):
        p = int(par[j])
        deg, _ = _gpu_rebuild(mp.rebuild_decision(B, j, mp.EPS, row, 1e-7))
        non, _ = _gpu_rebuild(mp.rebuild_decision(B, j, mp.EPS_ABOVE, row, 1e-7))
        _same(deg, _oracle_rebuild(mp.rebuild_decision(B, j, mp.EPS, row, 1e-7))[0], f"degenerate bone {j}")
        keep = [r for r in range(21) if r != p or p in (0, 10)]
        assert (bits(deg[others][:, keep]) == bits(non[others][:, keep])).all(), f"bone {j}: another row moved"
        if p not in (0, 10):
            # (frame 130 aside: its bone lies along an axis, as some zero-pose bones do)
            assert _ident(deg[:, p]) and (bits(non[others][:, p]) != bits(IDENT)).any(axis=1).all(), j
        else:
            assert not _ident(deg[:, p]), j


def test_frames_are_isolated_and_runs_repeat(gpu):
    """B = 513.  rescale_motion: the frames are independent, so a *_single family moves the bits of its touched frames
    only against the tame batch it was made from.  rebuild_vtrdyn and quat_between couple the frames through the batch
    maximum alone: in a tame batch every bone's decision is "not degenerate", and a zero, 1e-30 or 1e25 bone in one
    frame leaves the maximum where it was, a NaN makes it NaN and an inf makes it inf -- none is <= 1e-6f, so all five
    *_single families, and the hostile rows of the mixed pair batch, leave every other frame's bits alone.  Two runs of
    each give the same bits."""
    import oracle as orc
    from rtg import ops
    T, par, zl = tree()
    B = 513
    clean = mp.motions("tame", B)
    r0 = _np(ops.rescale_motion(T, clean, dir=DIR))
    g0, _ = _gpu_rebuild(clean)
    touched = mp.single_frames(B)
    others = np.ones(B, bool)
    others[touched] = False
    for fam in mp.SINGLES:
        m = mp.motions(fam, B)
        assert (bits(m)[others] == bits(clean)[others]).all() and (bits(m)[touched] != bits(clean)[touched]).any()
        r1, r2 = (_np(ops.rescale_motion(T, m, dir=DIR)) for _ in range(2))
        with np.errstate(all="ignore"):
            want = orc.rescale_motion(par, zl, m, dir=DIR)
        assert (bits(r1) == bits(r2)).all(), f"{fam}: two rescale runs differ"
        assert (bits(r1)[others] == bits(r0)[others]).all(), f"{fam}: rescale moved a clean frame"
        _same(r1, want, f"rescale {fam}")
        (g1, _), (g2, _) = _gpu_rebuild(m), _gpu_rebuild(m)
        assert (bits(g1) == bits(g2)).all(), f"{fam}: two rebuild runs differ"
        assert (bits(g1)[others] == bits(g0)[others]).all(), f"{fam}: rebuild moved a clean frame"
        _same(g1, _oracle_rebuild(m)[0], f"rebuild {fam}")
    v1, v2, at = mp.mixed_rows(B)
    c1, c2, _ = mp.mixed_rows(B, kinds=())
    others = np.ones(B, bool)
    others[list(at.values())] = False
    assert len(at) == len(mp.MIXED_ROWS) and (bits(v1)[others] == bits(c1)[others]).all()
    q0 = _np(ops.quat_between_two_vecs(c1, c2))
    q1, q2 = (_np(ops.quat_between_two_vecs(v1, v2)) for _ in range(2))
    assert (bits(q1) == bits(q2)).all() and (bits(q1)[others] == bits(q0)[others]).all()
    with np.errstate(all="ignore"):
        _same(q1, orc.quat_between(v1, v2), "mixed pairs")


def _filled(n, pattern):
    """n device words holding the bit pattern."""
    import torch
    ws = torch.empty(n, device="cuda", dtype=torch.float32)
    ws.view(torch.int32).fill_(pattern - (1 << 32) if pattern >= 1 << 31 else pattern)
    return ws


def test_a_dirty_workspace_decides_nothing(gpu):
    """rtg_quat_between_f32 and rtg_rebuild_vtrdyn_f32 called with a workspace that holds FLT_MAX, the NaN pin and all
    ones: an all-degenerate batch still comes back as the identity.  Then two calls back to back on one stream that
    share one workspace, a non-degenerate batch and a degenerate one: each is its own oracle result."""
    import oracle as orc
    import torch
    from rtg._lib import check, lib
    from rtg.runtime import dev_f32, ptr, stream_handle
    T, par, zl = tree()
    B = 257

    def between(v1, v2, ws):
        a, b = dev_f32(v1), dev_f32(v2)
        out = torch.full((len(v1), 4), 7.0, device="cuda")
        check(lib().rtg_quat_between_f32(ptr(a), ptr(b), len(v1), ptr(out), ptr(ws), stream_handle()))
        return out

    def rebuild(m, ws):
        x = dev_f32(m)
        g, r = torch.full((len(m), 21, 4), 7.0, device="cuda"), torch.full((len(m), 3), 7.0, device="cuda")
        check(lib().rtg_rebuild_vtrdyn_f32(T.handle, ptr(x), len(m), ptr(g), ptr(r), ptr(ws), stream_handle()))
        return g

    small = mp.decision_pair(B, 2, mp.EPS, 200, 1e-7)
    big = mp.decision_pair(B, 2, np.float32(1e-5), 3, 1e-7)
    flat, tame = mp.motions("collapsed", B), mp.motions("tame", B)
    with np.errstate(all="ignore"):
        want_big = orc.quat_between(*big)
    want_flat, want_tame = _oracle_rebuild(flat)[0], _oracle_rebuild(tame)[0]
    assert _ident(want_flat) and not _ident(want_big)
    for pattern in (0x7f7fffff, 0x7fffffff, 0xffffffff):
        assert _ident(_np(between(*small, _filled(2, pattern)))), hex(pattern)
        _same(_np(rebuild(flat, _filled(21, pattern))), want_flat, f"rebuild, workspace {pattern:#x}")
    ws2, ws21 = _filled(2, 0), _filled(21, 0)
    a, b = between(*big, ws2), between(*small, ws2)
    c, d = rebuild(tame, ws21), rebuild(flat, ws21)
    _same(_np(a), want_big, "quat_between, first of two calls")
    assert _ident(_np(b))
    _same(_np(c), want_tame, "rebuild, first of two calls")
    _same(_np(d), want_flat, "rebuild, second of two calls")


@pytest.mark.parametrize("j", [2, 15])
def test_main_retarget_on_a_zero_bone_clip(gpu, j):
    """retarget/main.py RetargetHuV5fromMocap.retarget_from_global_translation on 24 frames whose bone j is zero in every
    frame (the rescale makes joint j and everything below it NaN; the rebuild's maximum for bone j is NaN): the mocap
    side equals the oracle composition of tests/test_gpu_dropin.py::test_main_retarget_from_global_translation."""
    import oracle as orc
    import retarget.main as M
    import torch
    from robot_kinematics_model import RobotZeroPose
    from rtg import assets
    x = mp.motions(f"zero_bone_every_frame_{j}", 24)
    got = []
    hook = M.plot_skeleton_H
    M.plot_skeleton_H = lambda motions, *a, **k: got.extend(motions)
    try:
        M.RetargetHuV5fromMocap(RobotZeroPose.from_asset("vtrdyn"), RobotZeroPose.from_asset("hu_v5")) \
            .retarget_from_global_translation(torch.from_numpy(x))
    finally:
        M.plot_skeleton_H = hook
    mocap = got[0]
    _, par, zl = tree()
    tq = assets.tree_quat("vtrdyn")
    with np.errstate(all="ignore"):
        r = orc.rescale_motion(par, zl, x, dir=DIR)
        gr, rt = orc.rebuild_vtrdyn(par, zl, r)
        _, gp = orc.state_fk(par, tq, zl, orc.state_local_rotation(par, tq, gr), rt)
    assert np.isnan(r[:, j]).all() and np.isfinite(r[:, :j]).all()
    _same(mocap.global_rotation.numpy(), gr, "mocap global rotation")
    _same(mocap.global_translation.numpy(), gp, "mocap global translation")


# ------------------------------------------------------------------------------------------------------- ingest
def _hands(rng, B):
    return rng.normal(size=(B, 20, 3)).astype(np.float32), rng.normal(size=(B, 20, 3)).astype(np.float32)


def _ingest_both(bp, lh, rh):
    """reindex_frames in both layouts against numpy's gather and np.allclose, and against each other; -> valid."""
    from rtg.ingest import BODY23_TO_21, HAND_ORDER, reindex_frames
    want = (bp[:, BODY23_TO_21], lh[:, HAND_ORDER], rh[:, HAND_ORDER])
    flag = ~np.array([np.allclose(x, 0) for x in bp])
    for layout in ("aos", "soa"):
        *outs, valid = reindex_frames(bp, lh, rh, layout=layout)
        for o, w, what in zip(outs, want, ("body", "left hand", "right hand")):
            o = _np(o)
            o = o.transpose(2, 0, 1) if layout == "soa" else o
            assert (bits(o) == bits(w)).all(), f"{layout} {what}: differs from the gather"
        np.testing.assert_array_equal(_np(valid), flag, err_msg=layout)
    return flag


@pytest.mark.parametrize("i", range(len(mp.ingest_values())), ids=[repr(float(v)) for v in mp.ingest_values()])
def test_ingest_flag_at_every_position(gpu, i):
    """69 frames of zeros, frame k with the value at position k of its 69 body floats (joints 4 and 8, which the 23 -> 21
    map drops, included), random hands; again in reversed order, where each frame sits in another slot of its tile."""
    v = mp.ingest_values()[i]
    rng = np.random.default_rng(i)
    bp = np.zeros((69, 69), np.float32)
    bp[np.arange(69), np.arange(69)] = v
    bp = bp.reshape(69, 23, 3)
    lh, rh = _hands(rng, 69)
    carries = mp.carries_data([v])
    for body in (bp, np.ascontiguousarray(bp[::-1])):
        flag = _ingest_both(body, lh, rh)
        assert flag.all() if carries else not flag.any(), v


@pytest.mark.parametrize("B", [1, 15, 16, 17, 31, 32, 33, 65])
def test_ingest_short_and_ragged_batches(gpu, B):
    """Random frames, all-zero frames on both sides of the tile edges (16 frames AoS, 32 SoA), a batch below one tile."""
    rng = np.random.default_rng(B)
    bp = rng.normal(size=(B, 23, 3)).astype(np.float32)
    lh, rh = _hands(rng, B)
    zero = [t for t in (15, 16, 31, 32) if t < B] or [B - 1]
    bp[zero] = 0.0
    flag = _ingest_both(bp, lh, rh)
    assert np.flatnonzero(~flag).tolist() == zero


def test_ingest_hostile_hands(gpu):
    """The flag reads the body alone: NaN and inf hands on a zero body are skipped frames, and are moved as they are."""
    rng = np.random.default_rng(3)
    B = 37
    bp = np.zeros((B, 23, 3), np.float32)
    lh, rh = _hands(rng, B)
    lh[::2, :, 1], rh[1::2, 3] = np.nan, (np.inf, -np.inf, -0.0)
    lh[5], rh[6] = np.float32(1e-45), np.float32(3e38)
    bp[20, 4, 0] = 1.0                     # one frame carries data, in a joint the map drops
    flag = _ingest_both(bp, lh, rh)
    assert np.flatnonzero(flag).tolist() == [20]

"""The motion sampler on the MI355X (rtg.h rtg_motion_sample_f32, ops.motion_sample, rtg.motion.MotionLibrary,
SkeletonMotion.resample): every output equals the composition of oracle primitives (tests/motion_sample_ref.py, tied
to the reference by tests/test_motion_sample_host.py) bit for bit, NaN as NaN, the sign of zero included -- on four
skeletons (both tile shapes), ragged launches, every flag combination, hostile rotations and times, the slerp
thresholds, single rare records, invalid queries, and through the drop-in classes.  No query is skipped or masked."""
import ctypes

import numpy as np
import pytest
import torch

import motion_sample_ref as ref
from motion_sample_ref import bits

pytestmark = pytest.mark.gpu

SKELETONS = ("one", "hu_v5", "vtrdyn_full", "rand64")
_TREES, _TOPOS = {}, {}


def tree(name):
    """(parents, local_t, tree_quat) of the one-joint chain, Hu v5 (31), VTRDyn-59 and a random 64-joint tree."""
    if name not in _TREES:
        from rtg import assets
        if name == "one":
            _TREES[name] = (np.array([-1], np.int32), np.zeros((1, 3), np.float32), np.array([[0, 0, 0, 1]], np.float32))
        elif name == "rand64":
            _TREES[name] = ref.random_tree(64)
        else:
            _TREES[name] = (assets.parents(name).astype(np.int32), assets.local_translation(name).astype(np.float32),
                            assets.tree_quat(name).astype(np.float32))
    return _TREES[name]


def topo(name):
    if name not in _TOPOS:
        from rtg.runtime import Topology
        _TOPOS[name] = Topology(*tree(name))
    return _TOPOS[name]


def frames_per_wave(J):
    return 16 if J <= 36 else 8


class DevLib:
    """A helper-format library on the device."""

    def __init__(self, lib):
        from rtg.runtime import MotionLib
        self.host = lib
        self.rot, self.root_t = torch.from_numpy(lib["rot"]).cuda(), torch.from_numpy(lib["root_t"]).cuda()
        self.vec = None if lib["vec"] is None else torch.from_numpy(lib["vec"]).cuda()
        self.handle = MotionLib(lib["start"], lib["len"], lib["fps"], len(lib["rot"]))


def run(name, dl, clip, time, normalize=False, mode=None, vec=True):
    """mode: None | 'fk' | 'state'.  -> dict of numpy outputs, as motion_sample_ref.sample names them."""
    from rtg import ops
    lr, rt, v, gr, gp = ops.motion_sample(topo(name), dl.handle, dl.rot, dl.root_t, torch.from_numpy(np.asarray(clip, np.int32)),
                                          torch.from_numpy(np.asarray(time, np.float32)),
                                          vec=dl.vec if vec else None, normalize=normalize, want_global=mode is not None,
                                          state=mode == "state")
    torch.cuda.synchronize()
    return {k: None if x is None else x.cpu().numpy()
            for k, x in (("local_rot", lr), ("root_t", rt), ("vec", v), ("g_rot", gr), ("g_pos", gp))}


def want(name, lib, clip, time, normalize=False, mode=None, vec=True):
    lib = lib if vec else dict(lib, vec=None)
    return ref.sample(lib, np.asarray(clip, np.int32), np.asarray(time, np.float32), normalize,
                      tree(name) if mode else None, mode == "state")


KEYS = ("local_rot", "root_t", "vec", "g_rot", "g_pos")


def same(got, exp, msg=""):
    for k in KEYS:
        assert (got[k] is None) == (exp[k] is None), (k, msg)
        if got[k] is not None:
            assert got[k].shape == exp[k].shape, (k, msg)
            np.testing.assert_array_equal(bits(got[k]), bits(exp[k]), err_msg=f"{k} {msg}")


def queries(lib, n, seed=0):
    """Every time family on every clip, then random (clip, time) pairs up to n queries."""
    c, t = ref.library_queries(lib)
    rng = np.random.default_rng(seed)
    m = max(0, n - len(c))
    rc = rng.integers(0, len(lib["len"]), m).astype(np.int32)
    dur = (lib["len"][rc] - 1) / lib["fps"][rc]
    rt = (rng.uniform(-0.05, 1.1, m) * dur).astype(np.float32)
    return np.concatenate([c, rc])[:n], np.concatenate([t, rt])[:n]


_BASE = {}


def base(name, n=4097):
    """Per skeleton, computed once and left unchanged: the smooth library with K = 2 J, its device copy, n queries and
    the reference of the fullest flag combination."""
    if name not in _BASE:
        J = len(tree(name)[0])
        lib = ref.make_library(J, "smooth", K=2 * J)
        c, t = queries(lib, n)
        _BASE[name] = (lib, DevLib(lib), c, t, want(name, lib, c, t, True, "state", True))
    return _BASE[name]


def head(w, n):
    return {k: None if w[k] is None else w[k][:n] for k in KEYS}


@pytest.mark.parametrize("name", SKELETONS)
def test_tile_edges_every_time_family_and_two_launches(gpu, name):
    lib, dl, c, t, w = base(name)
    F = frames_per_wave(len(tree(name)[0]))
    assert len(c) == 4097 and np.isnan(t).any() and (w["b"] == 1).any() and (w["row0"] == w["row1"]).any()
    for N in (1, F - 1, F, F + 1, 3 * F + 5, 4097):
        got = run(name, dl, c[:N], t[:N], True, "state", True)
        same(got, head(w, N), f"N={N}")
    again = run(name, dl, c, t, True, "state", True)
    same(again, got, "second launch")
    empty = run(name, dl, c[:0], t[:0], True, "state", True)   # N = 0: a no-op
    assert empty["local_rot"].shape == (0, len(tree(name)[0]), 4) and empty["g_pos"].shape == (0, len(tree(name)[0]), 3)


@pytest.mark.parametrize("name", SKELETONS)
def test_a_query_does_not_depend_on_its_place(gpu, name):
    lib, dl, c, t, w = base(name)
    N = 1000
    perm = np.random.default_rng(5).permutation(N)
    got = run(name, dl, c[:N][perm], t[:N][perm], True, "state", True)
    same(got, {k: w[k][:N][perm] for k in KEYS}, "permuted")


@pytest.mark.parametrize("name", SKELETONS)
@pytest.mark.parametrize("normalize", (False, True))
@pytest.mark.parametrize("mode", (None, "fk", "state"))
def test_every_flag_combination(gpu, name, normalize, mode):
    lib, dl, c, t, _ = base(name)
    J = len(tree(name)[0])
    N = 3 * frames_per_wave(J) + 5
    c, t = np.concatenate([c[:N], c[-N:]]), np.concatenate([t[:N], t[-N:]])
    same(run(name, dl, c, t, normalize, mode, True), want(name, lib, c, t, normalize, mode, True), "K=2J")
    same(run(name, dl, c, t, normalize, mode, False), want(name, lib, c, t, normalize, mode, False), "no vec")
    lib1 = dict(lib, vec=np.ascontiguousarray(lib["vec"][:, :1]))
    same(run(name, DevLib(lib1), c, t, normalize, mode, True), want(name, lib1, c, t, normalize, mode, True), "K=1")


@pytest.mark.parametrize("name", SKELETONS)
@pytest.mark.parametrize("state", (False, True))
def test_global_outputs_equal_forward_kinematics_of_the_local_outputs(gpu, name, state):
    """Device against device: g_rot / g_pos are rtg_fk_f32 / rtg_state_fk_f32 on this launch's own outputs."""
    from rtg import ops
    lib, dl, c, t, _ = base(name)
    N = 777
    lr, rt, _, gr, gp = ops.motion_sample(topo(name), dl.handle, dl.rot, dl.root_t, torch.from_numpy(c[:N]),
                                          torch.from_numpy(t[:N]), normalize=True, want_global=True, state=state)
    fr, fp = ops.forward_kinematics(topo(name), lr, rt, state=state)
    np.testing.assert_array_equal(bits(gr.cpu().numpy()), bits(fr.cpu().numpy()))
    np.testing.assert_array_equal(bits(gp.cpu().numpy()), bits(fp.cpu().numpy()))


@pytest.mark.parametrize("family", ref.ROT_FAMILIES)
@pytest.mark.parametrize("name,only", [("hu_v5", None), ("rand64", 37)])
def test_hostile_rotations(gpu, family, name, only):
    """Every family on all joints of the clips (Hu v5) and on one joint only (the 64-joint tree), with queries at and
    between every consecutive frame pair."""
    J = len(tree(name)[0])
    lib = ref.make_library(J, family, K=1, seed=11, only_joint=only)
    c, t = ref.library_queries(lib)
    dl = DevLib(lib)
    for normalize, mode in ((True, "state"), (False, "fk")):
        same(run(name, dl, c, t, normalize, mode, True), want(name, lib, c, t, normalize, mode, True), family)


@pytest.mark.parametrize("name", SKELETONS)
def test_slerp_threshold_pairs(gpu, name):
    J = len(tree(name)[0])
    lib, names = ref.threshold_library(J)
    bs = np.array([0.0, 0.25, 0.5, 0.75, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    c = np.repeat(np.arange(len(names), dtype=np.int32), len(bs))
    t = np.tile(bs, len(names))            # fps 1: the time is the blend factor
    dl = DevLib(lib)
    got = run(name, dl, c, t, False, "fk", False)
    same(got, want(name, lib, c, t, False, "fk", False))
    same(run(name, dl, c, t, True, None, False), want(name, lib, c, t, True, None, False))
    # the quirk inherited from the reference: below sin = 0.001 the midpoint comes back whatever b is
    k = names.index("sin_below")
    rows = got["local_rot"][c == k]
    assert (bits(rows) == bits(rows[:1])).all() and not (bits(rows[0]) == bits(lib["rot"][2 * k])).all()


def test_clip_boundaries_are_adjacent_rows_and_never_crossed(gpu):
    """The last frame of clip c and the first of clip c + 1 are adjacent rows: a query at or past the end of clip c
    returns clip c's last frame exactly, whatever follows it."""
    name = "hu_v5"
    lib, dl, _, _, _ = base(name)
    C = len(lib["len"])
    c = np.repeat(np.arange(C, dtype=np.int32), 3)
    end = (lib["len"] - 1) / lib["fps"].astype(np.float64)
    t = np.stack([end, end * 1.5 + 0.01, np.full(C, np.inf)], 1).reshape(-1).astype(np.float32)
    got = run(name, dl, c, t, False, None, True)
    same(got, want(name, lib, c, t, False, None, True))
    last = lib["start"][c] + lib["len"][c] - 1
    for n in range(len(c)):
        if (ref.index_rule(c[n:n + 1], t[n:n + 1], lib["len"], lib["fps"])[1] == lib["len"][c[n]] - 1).all():
            np.testing.assert_array_equal(bits(got["root_t"][n]), bits(ref.blend(lib["root_t"][last[n]][None],
                                                                                 lib["root_t"][last[n]][None], [0])[0]))


@pytest.mark.parametrize("name", ("hu_v5", "vtrdyn_full"))
@pytest.mark.parametrize("kind", ("antipodal", "midpoint", "nan"))
def test_one_rare_record_among_ordinary_ones(gpu, name, kind):
    """One antipodal / midpoint / NaN record at a moving joint and a moving query -- both sides of every tile boundary,
    the first and the last lane of a wave instruction -- among smooth rows: query n blends frames n and n + 1."""
    J = len(tree(name)[0])
    F = frames_per_wave(J)
    N = 3 * F
    lib0 = ref.make_library(J, "smooth", lengths=(N + 1,), fps=(30.0,), K=1, seed=21)
    c = np.zeros(N, np.int32)
    t = ((np.arange(N) + 0.5) / 30.0).astype(np.float32)
    assert (ref.index_rule(c, t, lib0["len"], lib0["fps"])[1] == np.arange(N)).all()
    spots = {(n, j) for n in (0, F - 1, F, 2 * F - 1, 2 * F, 3 * F - 1) for j in (0, J // 2, J - 1)}
    lane63 = [(r // J, r % J) for r in range(63, N * J, 64)]
    spots |= {lane63[0], lane63[-1], (F, 0)}
    for n, j in sorted(spots):
        lib = dict(lib0, rot=lib0["rot"].copy())
        if kind == "antipodal":
            lib["rot"][n + 1, j] = -lib["rot"][n, j]
        elif kind == "midpoint":           # a pair 1e-4 rad apart: sin(half angle) below 0.001
            lib["rot"][n + 1, j] = lib["rot"][n, j] + np.float32(3e-5)
        else:
            lib["rot"][n + 1, j, (n + j) % 4] = np.nan
        same(run(name, DevLib(lib), c, t, True, "state", True), want(name, lib, c, t, True, "state", True), f"{n},{j}")


@pytest.mark.parametrize("name", SKELETONS)
def test_invalid_queries_are_quiet_nan_and_leave_the_rest_alone(gpu, name):
    lib, dl, c, t, _ = base(name)
    J = len(tree(name)[0])
    F = frames_per_wave(J)
    N = 3 * F + 5
    c, t = c[100:100 + N].copy(), t[100:100 + N].copy()
    clean = run(name, dl, c, t, True, "state", True)
    bad = {0: -1, F - 1: len(lib["len"]), F + F // 2: -1, 2 * F: len(lib["len"]), N - 1: 2**31 - 1, F: -2**31}
    cb = c.copy()
    for n, v in bad.items():
        cb[n] = v
    got = run(name, dl, cb, t, True, "state", True)
    same(got, want(name, lib, cb, t, True, "state", True))
    rows = sorted(bad)
    keep = np.setdiff1d(np.arange(N), rows)
    for k in KEYS:
        raw = got[k][rows].view(np.uint32)
        assert (raw == 0x7FC00000).all(), k          # the raw bits: the quiet NaN itself, not merely a NaN
        np.testing.assert_array_equal(bits(got[k][keep]), bits(clean[k][keep]), err_msg=k)


# ------------------------------------------------------------------------------------------------ the drop-in level
def hu_tree():
    from poselib.poselib.skeleton.skeleton3d import SkeletonTree
    p, lt, tq = tree("hu_v5")
    return SkeletonTree([f"j{i}" for i in range(len(p))], torch.from_numpy(p.astype(np.int64)), torch.from_numpy(lt),
                        torch.from_numpy(tq))


def hu_motion(tr, L, fps, seed, is_local=True):
    from poselib.poselib.skeleton.skeleton3d import SkeletonMotion, SkeletonState
    from kinematics_frames import rot_sequence
    rot = torch.from_numpy(rot_sequence("smooth", L, 31, seed))
    root = torch.from_numpy(np.random.default_rng(seed).normal(0, 0.3, (L, 3)).astype(np.float32))
    st = SkeletonState.from_rotation_and_root_translation(tr, rot, root, is_local=True)
    if not is_local:
        st = st.global_repr()
    return SkeletonMotion.from_skeleton_state(st, fps)


def test_motion_library_over_a_local_and_a_global_motion(gpu):
    from rtg import ops
    from rtg.motion import MotionLibrary
    tr = hu_tree()
    a, b = hu_motion(tr, 40, 30, 1), hu_motion(tr, 17, 120, 2, is_local=False)
    ml = MotionLibrary([a, b])
    assert ml.num_clips == 2 and list(ml.lengths) == [40, 17] and list(ml.fps) == [30.0, 120.0]
    np.testing.assert_allclose(ml.durations, [39 / 30, 16 / 120])
    # the packing: the local motion's rows as stored, the global one's through local_rotation
    np.testing.assert_array_equal(bits(ml.rot[:40].cpu().numpy()), bits(a.rotation.numpy()))
    np.testing.assert_array_equal(bits(ml.rot[40:].cpu().numpy()),
                                  bits(ops.local_rotation(tr.topology(), b.rotation, state=True).cpu().numpy()))
    lib = {"rot": ml.rot.cpu().numpy(), "root_t": ml.root_t.cpu().numpy(), "vec": ml.vec.cpu().numpy(),
           "start": np.array([0, 40], np.int64), "len": ml.lengths, "fps": ml.fps}
    np.testing.assert_array_equal(bits(lib["vec"][:40, 31:]), bits(a.global_angular_velocity.numpy()))
    c, t = queries(lib, 300, seed=3)
    c[7] = 2                                                   # an invalid query among them
    for kw, mode in ((dict(), "state"), (dict(state=False), "fk"), (dict(want_global=False, want_velocity=False), None)):
        s = ml.sample(c, t, **kw)
        w = ref.sample(lib if kw.get("want_velocity", True) else dict(lib, vec=None), c, t, True,
                       tree("hu_v5") if mode else None, mode == "state")
        for got, exp in ((s.local_rotation, w["local_rot"]), (s.root_translation, w["root_t"]),
                         (s.global_rotation, w["g_rot"]), (s.global_translation, w["g_pos"]),
                         (s.global_velocity, None if w["vec"] is None else w["vec"][:, :31]),
                         (s.global_angular_velocity, None if w["vec"] is None else w["vec"][:, 31:])):
            assert (got is None) == (exp is None)
            if got is not None:
                np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(exp))


@pytest.mark.parametrize("old,new", [(120, 30), (120, 50), (30, 120)])
def test_skeleton_motion_resample(gpu, old, new):
    from poselib.poselib.skeleton.skeleton3d import SkeletonMotion, SkeletonState
    tr = hu_tree()
    m = hu_motion(tr, 130, old, 4)
    r = m.resample(new)
    n = int(np.floor(129 * new / old)) + 1
    assert type(r) is SkeletonMotion and r.fps == new and r.is_local and tuple(r.tensor.shape) == (n, 31 * 10 + 3)
    assert r.tensor.device == m.tensor.device
    lib = {"rot": m.rotation.numpy().copy(), "root_t": m.root_translation.numpy().copy(), "vec": None,
           "start": np.array([0], np.int64), "len": np.array([130], np.int32), "fps": np.array([old], np.float32)}
    t = (np.arange(n, dtype=np.float64) / new).astype(np.float32)
    w = ref.sample(lib, np.zeros(n, np.int32), t, normalize=True)
    np.testing.assert_array_equal(bits(r.rotation.numpy()), bits(w["local_rot"]))
    np.testing.assert_array_equal(bits(r.root_translation.numpy()), bits(w["root_t"]))
    again = SkeletonMotion.from_skeleton_state(SkeletonState(r.tensor[:, :31 * 4 + 3], tr, True), new)
    np.testing.assert_array_equal(bits(r.tensor.numpy()), bits(again.tensor.numpy()))
    if (old, new) == (30, 120):        # every fourth frame is a stored frame: the slerp at b = 0 of a unit row
        assert n == 517


# ------------------------------------------------------------------------------------------------ error paths
def test_error_paths_on_the_device(gpu):
    from rtg import _lib, ops
    from rtg.runtime import MotionLib, Topology
    lib, dl, c, t, _ = base("hu_v5")
    p65 = np.arange(-1, 64, dtype=np.int32)
    t65 = Topology(p65, np.zeros((65, 3), np.float32))
    with pytest.raises(_lib.RtgError) as e:
        ops.motion_sample(t65, dl.handle, torch.zeros(len(lib["rot"]), 65, 4), torch.from_numpy(lib["root_t"]), c[:4], t[:4])
    assert e.value.status == 4 and "rtg_motion_sample_f32" in str(e.value)          # RTG_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.motion_sample(topo("hu_v5"), dl.handle, dl.rot[:-1], dl.root_t, c[:4], t[:4])
    with pytest.raises(ValueError):
        ops.motion_sample(topo("hu_v5"), dl.handle, dl.rot, dl.root_t, c[:4], t[:5])
    with pytest.raises(_lib.RtgError):
        MotionLib([0], [200], [30.0], 153)
    # overlapping and misaligned buffers, through the C ABI
    L = _lib.lib()
    N, J = 8, 31
    cd, td = torch.from_numpy(c[:N]).cuda(), torch.from_numpy(t[:N]).cuda()
    out = torch.empty(N * J * 4 + 8, device="cuda")
    root_out = torch.empty(N, 3, device="cuda")

    def call(rot, lo, ro):
        rc = L.rtg_motion_sample_f32(topo("hu_v5").handle, dl.handle.handle, rot, dl.root_t.data_ptr(), None, 0,
                                     cd.data_ptr(), td.data_ptr(), N, 0, lo, ro, None, None, None, None)
        return rc, L.rtg_last_error().decode()

    rc, msg = call(dl.rot.data_ptr(), dl.rot.data_ptr() + 16 * J, root_out.data_ptr())
    assert rc == 1 and "overlap" in msg, msg
    rc, msg = call(dl.rot.data_ptr(), out.data_ptr(), dl.root_t.data_ptr() + 12)
    assert rc == 1 and "overlap" in msg, msg
    rc, msg = call(dl.rot.data_ptr(), out.data_ptr() + 4, root_out.data_ptr())
    assert rc == 1 and "aligned" in msg, msg
    rc, msg = call(dl.rot.data_ptr() + 8, out.data_ptr(), root_out.data_ptr())
    assert rc == 1 and "aligned" in msg, msg
    rc, msg = call(dl.rot.data_ptr(), out.data_ptr(), root_out.data_ptr())
    assert rc == 0, msg
    torch.cuda.synchronize()
